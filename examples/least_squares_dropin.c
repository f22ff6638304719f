/*
 * Drop-in check: the least-squares fit X = inv(A^T A) A^T B written the way a CMSIS-DSP program writes it, with
 * arm_mat_trans_f32, arm_mat_mult_f32 and arm_mat_inverse_f32 on host buffers, linked against
 * libcmsisdsp_mi355x.so only.
 * Input file:  uint32 m, n, p, then A (m x n) and B (m x p), row-major float32.
 * Output file: At (n x m), AtA (n x n), the inverse (n x n), the pseudo-inverse inv(AtA) At (n x m) and
 *              X (n x p), row-major float32, in that order.
 * Build:  gcc -Iinclude examples/least_squares_dropin.c -Lcmsis-dsp_amd/lib -lcmsisdsp_mi355x -lm
 * Run:    LD_LIBRARY_PATH=cmsis-dsp_amd/lib ./a.out operands.bin results.bin    -> prints "OK m n p"
 */
#include <stdio.h>
#include <stdlib.h>

#include "arm_math.h"

static float32_t *matrix(arm_matrix_instance_f32 *S, uint32_t rows, uint32_t cols) {
  float32_t *p = (float32_t *)calloc((size_t)rows * cols, sizeof(float32_t));
  arm_mat_init_f32(S, (uint16_t)rows, (uint16_t)cols, p);
  return p;
}

static int put(FILE *f, const arm_matrix_instance_f32 *S) {
  const size_t n = (size_t)S->numRows * S->numCols;
  return fwrite(S->pData, sizeof(float32_t), n, f) == n;
}

int main(int argc, char **argv) {
  if (argc < 3) {
    fprintf(stderr, "usage: %s operands.bin results.bin\n", argv[0]);
    return 2;
  }
  uint32_t dim[3];
  FILE *f = fopen(argv[1], "rb");
  if (!f || fread(dim, sizeof(uint32_t), 3, f) != 3 || !dim[0] || !dim[1] || !dim[2] || dim[0] > 65535 ||
      dim[1] > 65535 || dim[2] > 65535) {
    fprintf(stderr, "cannot read the dimensions\n");
    return 2;
  }
  const uint32_t m = dim[0], n = dim[1], p = dim[2];
  arm_matrix_instance_f32 A, B, At, AtA, AtAinv, Pinv, X;
  if (!matrix(&A, m, n) || !matrix(&B, m, p) || !matrix(&At, n, m) || !matrix(&AtA, n, n) || !matrix(&AtAinv, n, n) ||
      !matrix(&Pinv, n, m) || !matrix(&X, n, p)) {
    fprintf(stderr, "out of memory\n");
    return 2;
  }
  if (fread(A.pData, sizeof(float32_t), (size_t)m * n, f) != (size_t)m * n ||
      fread(B.pData, sizeof(float32_t), (size_t)m * p, f) != (size_t)m * p) {
    fprintf(stderr, "cannot read the operands\n");
    return 2;
  }
  fclose(f);

  arm_status st = arm_mat_trans_f32(&A, &At);
  if (st == ARM_MATH_SUCCESS) st = arm_mat_mult_f32(&At, &A, &AtA);
  f = fopen(argv[2], "wb");
  int ok = f && st == ARM_MATH_SUCCESS && put(f, &At) && put(f, &AtA);
  /* arm_mat_inverse_f32 destroys its source, so AtA is written out first */
  if (ok) st = arm_mat_inverse_f32(&AtA, &AtAinv);
  if (ok && st == ARM_MATH_SUCCESS) st = arm_mat_mult_f32(&AtAinv, &At, &Pinv);
  if (ok && st == ARM_MATH_SUCCESS) st = arm_mat_mult_f32(&Pinv, &B, &X);
  ok = ok && st == ARM_MATH_SUCCESS && put(f, &AtAinv) && put(f, &Pinv) && put(f, &X);
  if (f) fclose(f);
  if (!ok) {
    fprintf(stderr, "failed: status %d\n", (int)st);
    return 1;
  }
  printf("OK %u %u %u\n", m, n, p);
  return 0;
}
