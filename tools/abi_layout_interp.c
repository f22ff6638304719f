/* Prints the byte layout of the interpolation instance structs and the values of arm_spline_type as JSON.  Compiled
 * against the reference headers (-> tests/golden/abi_layout_interp.json) and against include/ (tests/test_interp.py);
 * the two must agree for the drop-in promise. */
#include <stddef.h>
#include <stdio.h>
#include "arm_math.h"

#define FIELD(T, f) printf(", \"" #f "\": %zu", offsetof(T, f))
#define OPEN(T) printf("  \"" #T "\": {\"size\": %zu", sizeof(T))
#define BILINEAR(T) OPEN(T); FIELD(T, numRows); FIELD(T, numCols); FIELD(T, pData); printf("},\n")

int main(void) {
  printf("{\n");
  OPEN(arm_linear_interp_instance_f32); FIELD(arm_linear_interp_instance_f32, nValues);
  FIELD(arm_linear_interp_instance_f32, x1); FIELD(arm_linear_interp_instance_f32, xSpacing);
  FIELD(arm_linear_interp_instance_f32, pYData); printf("},\n");
  BILINEAR(arm_bilinear_interp_instance_f32);
  BILINEAR(arm_bilinear_interp_instance_q31);
  BILINEAR(arm_bilinear_interp_instance_q15);
  BILINEAR(arm_bilinear_interp_instance_q7);
  OPEN(arm_spline_instance_f32); FIELD(arm_spline_instance_f32, type); FIELD(arm_spline_instance_f32, x);
  FIELD(arm_spline_instance_f32, y); FIELD(arm_spline_instance_f32, n_x); FIELD(arm_spline_instance_f32, coeffs);
  printf("},\n");
  printf("  \"arm_spline_type\": {\"size\": %zu, \"ARM_SPLINE_NATURAL\": %d, \"ARM_SPLINE_PARABOLIC_RUNOUT\": %d}\n",
         sizeof(arm_spline_type), (int)ARM_SPLINE_NATURAL, (int)ARM_SPLINE_PARABOLIC_RUNOUT);
  printf("}\n");
  return 0;
}
