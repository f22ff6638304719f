/* Distances through the drop-in ABI on host buffers: the euclidean and cosine distances of two short vectors are
 * compared with values formed in double precision, the hamming distance of two packed bit vectors with the count of
 * differing bits, and a query that is a template played at half speed is aligned to it by dynamic time warping under a
 * Sakoe-Chiba window: the distance is zero and the path runs from (0, 0) to the last cell.  Prints SUCCESS. */
#include <math.h>
#include <stdio.h>

#include "arm_math.h"
#include "arm_math_mi355x.h"

#define N 40
#define T 12
#define Q (2 * T)

static float32_t a[N], b[N];
static float32_t dist[Q * T], cost[Q * T];
static q7_t win[Q * T];
static int16_t path[2 * (Q + T)];

int main(void) {
  double ss = 0.0, dot = 0.0, pa = 0.0, pb = 0.0;
  for (int i = 0; i < N; ++i) {
    a[i] = (float32_t)sin(0.3 * i);
    b[i] = (float32_t)cos(0.2 * i);
    ss += ((double)a[i] - b[i]) * ((double)a[i] - b[i]);
    dot += (double)a[i] * b[i];
    pa += (double)a[i] * a[i];
    pb += (double)b[i] * b[i];
  }
  const float32_t eu = arm_euclidean_distance_f32(a, b, N), co = arm_cosine_distance_f32(a, b, N);

  const uint32_t bits = 70;                                 /* three words; of the last one the top six bits count */
  const uint32_t x[3] = {0xF0F0F0F0u, 0x00000000u, 0xFC000001u}, y[3] = {0xFFFF0000u, 0x00000001u, 0x04000002u};
  const float32_t ham = arm_hamming_distance(x, y, bits);   /* 16 + 1 + 5 differing booleans */

  float32_t templ[T], query[Q];
  for (int t = 0; t < T; ++t) templ[t] = (float32_t)sin(0.5 * t);
  for (int q = 0; q < Q; ++q) query[q] = templ[q / 2];
  for (int q = 0; q < Q; ++q)
    for (int t = 0; t < T; ++t) dist[q * T + t] = fabsf(query[q] - templ[t]);
  arm_matrix_instance_f32 D = {Q, T, dist}, C = {Q, T, cost};
  arm_matrix_instance_q7 W = {Q, T, win};
  float32_t dtw = -1.0f;
  uint32_t len = 0;
  arm_status st = arm_dtw_init_window_q7(ARM_DTW_SAKOE_CHIBA_WINDOW, T + 1, &W);
  if (st == ARM_MATH_SUCCESS) st = arm_dtw_distance_f32(&D, &W, &C, &dtw);
  if (st == ARM_MATH_SUCCESS) arm_dtw_path_f32(&C, path, &len);
  if (st != ARM_MATH_SUCCESS || arm_mi355x_last_error() != 0) {
    printf("FAILURE: status %d, %s\n", (int)st, arm_mi355x_last_error_string());
    return 1;
  }

  printf("euclidean   %.6f (double: %.6f)\n", eu, sqrt(ss));
  printf("cosine      %.6f (double: %.6f)\n", co, 1.0 - dot / sqrt(pa * pb));
  printf("hamming     %.6f (22 of 70)\n", ham);
  printf("dtw         %.6f over a path of %u points ending at (%d, %d)\n", dtw, (unsigned)len, path[2 * len - 2],
         path[2 * len - 1]);
  int ok = fabs(eu - sqrt(ss)) < 1e-5 && fabs(co - (1.0 - dot / sqrt(pa * pb))) < 1e-5 && ham == 22.0f / 70.0f;
  ok = ok && dtw == 0.0f && len >= Q && path[0] == 0 && path[1] == 0 && path[2 * len - 2] == Q - 1 &&
       path[2 * len - 1] == T - 1;
  printf(ok ? "SUCCESS\n" : "FAILURE\n");
  return !ok;
}
