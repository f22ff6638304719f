/* Conversions, a sort and a barycenter through the drop-in ABI on host buffers: a float32 signal goes to q15 and
 * back (the round trip stays within one q15 step, 2^-15), is sorted in descending order (the first word is the
 * maximum, every word is at most its predecessor), and the barycenter of three points of the plane under the weights
 * 1, 2, 1 is compared with the value formed in double precision.  Prints SUCCESS. */
#include <math.h>
#include <stdio.h>

#include "arm_math.h"
#include "arm_math_mi355x.h"

#define N 100

static float32_t x[N], back[N], sorted[N];
static q15_t q[N];

int main(void) {
  float32_t maxv = -2.0f;
  for (int i = 0; i < N; ++i) {
    x[i] = (float32_t)(0.9 * sin(0.31 * i) * cos(0.07 * i));
    if (x[i] > maxv) maxv = x[i];
  }
  arm_float_to_q15(x, q, N);
  arm_q15_to_float(q, back, N);

  arm_sort_instance_f32 S;
  arm_sort_init_f32(&S, ARM_SORT_QUICK, ARM_SORT_DESCENDING);
  arm_sort_f32(&S, x, sorted, N);

  const float32_t points[6] = {0.0f, 0.0f, 4.0f, 0.0f, 0.0f, 8.0f}, weights[3] = {1.0f, 2.0f, 1.0f};
  float32_t centre[2] = {-1.0f, -1.0f};
  arm_barycenter_f32(points, weights, centre, 3, 2);
  if (arm_mi355x_last_error() != 0) {
    printf("FAILURE: %s\n", arm_mi355x_last_error_string());
    return 1;
  }

  int ok = sorted[0] == maxv;
  double worst = 0.0;
  for (int i = 0; i < N; ++i) {
    const double e = fabs((double)back[i] - x[i]);
    if (e > worst) worst = e;
    if (i && sorted[i] > sorted[i - 1]) ok = 0;
  }
  printf("q15 round trip      worst error %.3g (one step is %.3g)\n", worst, ldexp(1.0, -15));
  printf("sorted descending   %.6f .. %.6f\n", sorted[0], sorted[N - 1]);
  printf("barycenter          (%.6f, %.6f)\n", centre[0], centre[1]);
  ok = ok && worst < ldexp(1.0, -15) && centre[0] == 2.0f && centre[1] == 2.0f;
  printf(ok ? "SUCCESS\n" : "FAILURE\n");
  return !ok;
}
