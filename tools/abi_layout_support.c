/* Prints the byte layout of the two sort instance structs and the sizes of the sort enums as JSON.  Compiled against
 * the reference headers (-> tests/golden/abi_layout_support.json) and against include/ (tests/test_support.py); the
 * two must agree for the drop-in promise. */
#include <stddef.h>
#include <stdio.h>
#include "arm_math.h"

#define FIELD(T, f) printf(", \"" #f "\": %zu", offsetof(T, f))
#define OPEN(T) printf("  \"" #T "\": {\"size\": %zu", sizeof(T))

int main(void) {
  printf("{\n");
  OPEN(arm_sort_instance_f32); FIELD(arm_sort_instance_f32, alg); FIELD(arm_sort_instance_f32, dir); printf("},\n");
  OPEN(arm_merge_sort_instance_f32); FIELD(arm_merge_sort_instance_f32, dir);
  FIELD(arm_merge_sort_instance_f32, buffer); printf("},\n");
  printf("  \"arm_sort_alg\": {\"size\": %zu, \"ARM_SORT_BITONIC\": %d, \"ARM_SORT_SELECTION\": %d},\n",
         sizeof(arm_sort_alg), (int)ARM_SORT_BITONIC, (int)ARM_SORT_SELECTION);
  printf("  \"arm_sort_dir\": {\"size\": %zu, \"ARM_SORT_DESCENDING\": %d, \"ARM_SORT_ASCENDING\": %d}\n",
         sizeof(arm_sort_dir), (int)ARM_SORT_DESCENDING, (int)ARM_SORT_ASCENDING);
  printf("}\n");
  return 0;
}
