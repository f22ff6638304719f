/* Prints the byte layout of the four SVM instance structs and the naive Bayes instance struct as JSON.  Compiled
 * against the reference headers (-> tests/golden/abi_layout_ml.json) and against include/ (tests/test_ml.py); the two
 * must agree for the drop-in promise. */
#include <stddef.h>
#include <stdio.h>
#include "arm_math.h"

#define FIELD(T, f) printf(", \"" #f "\": %zu", offsetof(T, f))
#define OPEN(T) printf("  \"" #T "\": {\"size\": %zu", sizeof(T))
#define SVM_COMMON(T)                                                                                      \
  OPEN(T); FIELD(T, nbOfSupportVectors); FIELD(T, vectorDimension); FIELD(T, intercept);                   \
  FIELD(T, dualCoefficients); FIELD(T, supportVectors); FIELD(T, classes)

int main(void) {
  printf("{\n");
  SVM_COMMON(arm_svm_linear_instance_f32); printf("},\n");
  SVM_COMMON(arm_svm_polynomial_instance_f32); FIELD(arm_svm_polynomial_instance_f32, degree);
  FIELD(arm_svm_polynomial_instance_f32, coef0); FIELD(arm_svm_polynomial_instance_f32, gamma); printf("},\n");
  SVM_COMMON(arm_svm_rbf_instance_f32); FIELD(arm_svm_rbf_instance_f32, gamma); printf("},\n");
  SVM_COMMON(arm_svm_sigmoid_instance_f32); FIELD(arm_svm_sigmoid_instance_f32, coef0);
  FIELD(arm_svm_sigmoid_instance_f32, gamma); printf("},\n");
  OPEN(arm_gaussian_naive_bayes_instance_f32); FIELD(arm_gaussian_naive_bayes_instance_f32, vectorDimension);
  FIELD(arm_gaussian_naive_bayes_instance_f32, numberOfClasses); FIELD(arm_gaussian_naive_bayes_instance_f32, theta);
  FIELD(arm_gaussian_naive_bayes_instance_f32, sigma); FIELD(arm_gaussian_naive_bayes_instance_f32, classPriors);
  FIELD(arm_gaussian_naive_bayes_instance_f32, epsilon); printf("}\n");
  printf("}\n");
  return 0;
}
