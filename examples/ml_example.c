/* Classifiers and log-domain statistics through the drop-in ABI on host buffers: arm_vexp_f32 and arm_vlog_f32 undo
 * each other within rounding, the entropy of a uniform distribution is log(n), logsumexp of log-probabilities that
 * sum to one is zero, an rbf SVM with one support vector per cluster separates two clusters, and a Gaussian naive
 * Bayes model names the class whose mean a point sits on.  Prints SUCCESS. */
#include <math.h>
#include <stdio.h>

#include "arm_math.h"
#include "arm_math_mi355x.h"

#define N 32
#define DIM 4

int main(void) {
  float32_t x[N], e[N], back[N], p[N], lp[N];
  double worst = 0.0;
  for (int i = 0; i < N; ++i) {
    x[i] = -3.0f + 0.2f * (float32_t)i;
    p[i] = 1.0f / N;
    lp[i] = logf(p[i]);
  }
  arm_vexp_f32(x, e, N);
  arm_vlog_f32(e, back, N);
  for (int i = 0; i < N; ++i) worst = fmax(worst, fabs((double)back[i] - x[i]));
  const float32_t ent = arm_entropy_f32(p, N), lse = arm_logsumexp_f32(lp, N), kl = arm_kullback_leibler_f32(p, p, N);

  /* two clusters around (1, 1, 1, 1) and (-1, -1, -1, -1): one support vector each, dual coefficients +1 and -1 */
  const float32_t sv[2 * DIM] = {1, 1, 1, 1, -1, -1, -1, -1}, dual[2] = {1.0f, -1.0f};
  const int32_t classes[2] = {10, 20};
  arm_svm_rbf_instance_f32 S;
  arm_svm_rbf_init_f32(&S, 2, DIM, 0.0f, dual, sv, classes, 0.5f);
  const float32_t near_a[DIM] = {0.9f, 1.2f, 0.8f, 1.1f}, near_b[DIM] = {-1.1f, -0.7f, -1.0f, -0.9f};
  int32_t ca = 0, cb = 0;
  arm_svm_rbf_predict_f32(&S, near_a, &ca);
  arm_svm_rbf_predict_f32(&S, near_b, &cb);

  /* three classes with means 0, 2 and 4 in every dimension */
  float32_t theta[3 * DIM], sigma[3 * DIM], prob[3];
  const float32_t prior[3] = {0.3f, 0.3f, 0.4f}, at[DIM] = {2.1f, 1.9f, 2.0f, 2.2f};
  for (int c = 0; c < 3; ++c)
    for (int d = 0; d < DIM; ++d) {
      theta[c * DIM + d] = 2.0f * (float32_t)c;
      sigma[c * DIM + d] = 0.25f;
    }
  const arm_gaussian_naive_bayes_instance_f32 B = {DIM, 3, theta, sigma, prior, 1e-6f};
  const uint32_t cls = arm_gaussian_naive_bayes_predict_f32(&B, at, prob, NULL);

  if (arm_mi355x_last_error() != 0) {
    printf("FAILURE: %s\n", arm_mi355x_last_error_string());
    return 1;
  }
  printf("vlog(vexp(x)) - x   at most %.2e\n", worst);
  printf("entropy             %.6f (log %d = %.6f)\n", ent, N, log((double)N));
  printf("logsumexp           %.2e, kullback_leibler(p, p) %.2e\n", lse, kl);
  printf("rbf SVM             %d and %d\n", (int)ca, (int)cb);
  printf("naive Bayes         class %u, words %.3f %.3f %.3f\n", (unsigned)cls, prob[0], prob[1], prob[2]);
  int ok = worst < 2e-6 && fabs(ent - log((double)N)) < 1e-5 && fabsf(lse) < 1e-5f && kl == 0.0f;
  ok = ok && ca == 20 && cb == 10 && cls == 1 && prob[1] > prob[0] && prob[1] > prob[2];
  printf(ok ? "SUCCESS\n" : "FAILURE\n");
  return !ok;
}
