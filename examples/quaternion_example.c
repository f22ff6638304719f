/* Quaternions through the drop-in ABI on host buffers: a quarter turn about z and a quarter turn about x are
 * normalised, multiplied, turned into a rotation matrix and back; the product's inverse undoes it; the norm of a unit
 * quaternion is 1.  Prints SUCCESS. */
#include <math.h>
#include <stdio.h>

#include "arm_math.h"
#include "arm_math_mi355x.h"

#define N 2

int main(void) {
  /* (w, x, y, z): twice the quarter turns, so that normalize has work to do */
  const float32_t raw[4 * N] = {2.0f, 0.0f, 0.0f, 2.0f, 3.0f, 3.0f, 0.0f, 0.0f};
  float32_t unit[4 * N], norms[N], both[4], inv[4], one[4], rot[9], back[4], conj[4];
  arm_quaternion_normalize_f32(raw, unit, N);
  arm_quaternion_norm_f32(unit, norms, N);
  arm_quaternion_product_single_f32(unit, unit + 4, both);          /* first about x, then about z */
  arm_quaternion_inverse_f32(both, inv, 1);
  arm_quaternion_conjugate_f32(both, conj, 1);
  arm_quaternion_product_f32(both, inv, one, 1);
  arm_quaternion2rotation_f32(both, rot, 1);
  arm_rotation2quaternion_f32(rot, back, 1);

  if (arm_mi355x_last_error() != 0) {
    printf("FAILURE: %s\n", arm_mi355x_last_error_string());
    return 1;
  }
  printf("norms               %.6f %.6f\n", norms[0], norms[1]);
  printf("z-turn * x-turn     %.4f %.4f %.4f %.4f\n", both[0], both[1], both[2], both[3]);
  printf("q * inverse(q)      %.4f %.4f %.4f %.4f\n", one[0], one[1], one[2], one[3]);
  printf("rotation            %.3f %.3f %.3f / %.3f %.3f %.3f / %.3f %.3f %.3f\n", rot[0], rot[1], rot[2], rot[3],
         rot[4], rot[5], rot[6], rot[7], rot[8]);
  printf("back                %.4f %.4f %.4f %.4f\n", back[0], back[1], back[2], back[3]);
  /* x -> y, y -> z, z -> x: the columns of the matrix */
  const float32_t want[9] = {0, 0, 1, 1, 0, 0, 0, 1, 0};
  int ok = fabsf(norms[0] - 1.0f) < 1e-6f && fabsf(norms[1] - 1.0f) < 1e-6f;
  for (int i = 0; i < 9; ++i) ok = ok && fabsf(rot[i] - want[i]) < 1e-6f;
  for (int i = 0; i < 4; ++i) {
    ok = ok && fabsf(both[i] - 0.5f) < 1e-6f && fabsf(back[i] - both[i]) < 1e-6f;
    ok = ok && fabsf(one[i] - (i == 0 ? 1.0f : 0.0f)) < 1e-6f && fabsf(conj[i] - inv[i]) < 1e-6f;
  }
  printf(ok ? "SUCCESS\n" : "FAILURE\n");
  return !ok;
}
