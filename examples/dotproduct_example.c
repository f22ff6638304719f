/* A dot product two ways through the drop-in ABI on host buffers: arm_mult_f32 of two vectors followed by a running
 * arm_add_f32 over the products (the accumulator is both a source and the destination), and arm_dot_prod_f32 of the
 * same vectors.  Both round every product and then every add in element order, so the two results are the same
 * float32 word; a sum formed in double precision is printed beside them.  Prints SUCCESS. */
#include <math.h>
#include <stdio.h>
#include <string.h>

#include "arm_math.h"
#include "arm_math_mi355x.h"

#define N 48

static float32_t a[N], b[N], prod[N];

int main(void) {
  double want = 0.0;
  for (int i = 0; i < N; ++i) {
    a[i] = (float32_t)(0.75 * cos(0.37 * i) - 0.01 * i);      /* a chirp-like signal ... */
    b[i] = (float32_t)(0.5 - 0.5 * cos(2.0 * 3.14159265358979323846 * i / (N - 1)));   /* ... under a Hann window */
    want += (double)a[i] * b[i];
  }

  float32_t running = 0.0f, dot = -1.0f;
  arm_mult_f32(a, b, prod, N);
  for (int i = 0; i < N; ++i) arm_add_f32(&running, &prod[i], &running, 1);
  arm_dot_prod_f32(a, b, N, &dot);
  if (arm_mi355x_last_error() != 0) {
    printf("FAILURE: %s\n", arm_mi355x_last_error_string());
    return 1;
  }

  printf("mult + running add  %.9g\n", running);
  printf("arm_dot_prod_f32    %.9g\n", dot);
  printf("double precision    %.12g\n", want);
  /* N products and N adds of terms below 1, each rounded to 2^-24 relative: 2 N 2^-24 bounds the distance */
  const int same = memcmp(&running, &dot, sizeof dot) == 0;
  const int close = fabs(dot - want) < 2.0 * N * ldexp(1.0, -24);
  printf(same && close ? "SUCCESS\n" : "FAILURE\n");
  return !(same && close);
}
