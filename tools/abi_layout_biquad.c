/* Prints the byte layout of the biquad cascade instance structs as JSON.  Compiled against the
 * reference headers (tools/make_golden_biquad.py -> tests/golden/abi_layout_biquad.json) and against
 * include/ (tests/test_biquad.py); the two must agree for the drop-in promise. */
#include <stddef.h>
#include <stdio.h>
#include "arm_math.h"

#define FIELD(T, f) printf(", \"" #f "\": %zu", offsetof(T, f))
#define OPEN(T) printf("  \"" #T "\": {\"size\": %zu", sizeof(T))
#define BASE(T) OPEN(T); FIELD(T, numStages); FIELD(T, pState); FIELD(T, pCoeffs)

int main(void) {
  printf("{\n");
  BASE(arm_biquad_casd_df1_inst_q15); FIELD(arm_biquad_casd_df1_inst_q15, postShift); printf("},\n");
  BASE(arm_biquad_casd_df1_inst_q31); FIELD(arm_biquad_casd_df1_inst_q31, postShift); printf("},\n");
  BASE(arm_biquad_casd_df1_inst_f32); printf("},\n");
  BASE(arm_biquad_cas_df1_32x64_ins_q31); FIELD(arm_biquad_cas_df1_32x64_ins_q31, postShift); printf("},\n");
  BASE(arm_biquad_cascade_df2T_instance_f32); printf("},\n");
  BASE(arm_biquad_cascade_stereo_df2T_instance_f32); printf("}\n");
  printf("}\n");
  return 0;
}
