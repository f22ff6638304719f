/*
 * Drop-in check: the FFT-bin example's whole call sequence against libcmsisdsp_mi355x.so, with no host
 * arithmetic: arm_cfft_f32(&arm_cfft_sR_f32_len1024, buf, 0, 1), arm_cmplx_mag_f32, arm_max_f32, as a CMSIS-DSP
 * program writes them (examples/fft_bin_dropin.c does the last two steps with a host loop).  Input: the
 * example's 10 kHz test signal, read from a raw float32 file (tests/golden fixture).
 * Build:  gcc -Iinclude examples/fft_bin_example_full.c -Lcmsis-dsp_amd/lib -lcmsisdsp_mi355x -lm
 * Run:    LD_LIBRARY_PATH=cmsis-dsp_amd/lib ./a.out input.f32    -> prints "SUCCESS 213"
 */
#include <stdio.h>

#include "arm_math.h"
#include "arm_const_structs.h"

#define TEST_LENGTH_SAMPLES 2048

static float32_t testInput[TEST_LENGTH_SAMPLES];
static float32_t testOutput[TEST_LENGTH_SAMPLES / 2];

int main(int argc, char **argv) {
  const uint32_t fftSize = 1024, ifftFlag = 0, doBitReverse = 1, refIndex = 213;
  uint32_t testIndex = 0;
  float32_t maxValue = 0.0f;
  FILE *f = fopen(argc > 1 ? argv[1] : "input.f32", "rb");
  if (!f || fread(testInput, sizeof(float32_t), TEST_LENGTH_SAMPLES, f) != TEST_LENGTH_SAMPLES) {
    fprintf(stderr, "cannot read input\n");
    return 2;
  }
  fclose(f);
  /* the complex FFT, the magnitude at each bin, the bin of the largest magnitude */
  arm_cfft_f32(&arm_cfft_sR_f32_len1024, testInput, ifftFlag, doBitReverse);
  arm_cmplx_mag_f32(testInput, testOutput, fftSize);
  arm_max_f32(testOutput, fftSize, &maxValue, &testIndex);
  printf("%s %u\n", testIndex == refIndex ? "SUCCESS" : "FAILURE", testIndex);
  return testIndex == refIndex ? 0 : 1;
}
