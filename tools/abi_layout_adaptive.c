/* Prints the byte layout of the IIR lattice and LMS / normalised LMS instance structs as JSON.  Compiled
 * against the reference headers (tools/make_golden_adaptive.py -> tests/golden/abi_layout_adaptive.json)
 * and against include/ (tests/test_adaptive.py); the two must agree for the drop-in promise. */
#include <stddef.h>
#include <stdio.h>
#include "arm_math.h"

#define FIELD(T, f) printf(", \"" #f "\": %zu", offsetof(T, f))
#define OPEN(T) printf("  \"" #T "\": {\"size\": %zu", sizeof(T))
#define IIR(T) OPEN(T); FIELD(T, numStages); FIELD(T, pState); FIELD(T, pkCoeffs); FIELD(T, pvCoeffs)
#define LMS(T) OPEN(T); FIELD(T, numTaps); FIELD(T, pState); FIELD(T, pCoeffs); FIELD(T, mu)

int main(void) {
  printf("{\n");
  IIR(arm_iir_lattice_instance_f32); printf("},\n");
  IIR(arm_iir_lattice_instance_q31); printf("},\n");
  IIR(arm_iir_lattice_instance_q15); printf("},\n");
  LMS(arm_lms_instance_f32); printf("},\n");
  LMS(arm_lms_instance_q31); FIELD(arm_lms_instance_q31, postShift); printf("},\n");
  LMS(arm_lms_instance_q15); FIELD(arm_lms_instance_q15, postShift); printf("},\n");
  LMS(arm_lms_norm_instance_f32); FIELD(arm_lms_norm_instance_f32, energy); FIELD(arm_lms_norm_instance_f32, x0);
  printf("},\n");
  LMS(arm_lms_norm_instance_q15); FIELD(arm_lms_norm_instance_q15, postShift);
  FIELD(arm_lms_norm_instance_q15, recipTable); FIELD(arm_lms_norm_instance_q15, energy);
  FIELD(arm_lms_norm_instance_q15, x0); printf("}\n");
  printf("}\n");
  return 0;
}
