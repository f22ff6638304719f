/* Mean, variance, standard deviation and rms of one signal through the drop-in ABI (arm_mean_f32, arm_var_f32,
 * arm_std_f32, arm_rms_f32 on host buffers), compared with the same four figures formed in double precision.
 * The signal is a 440 Hz tone at 16 kHz with an offset and a slow ramp, 1000 samples.  Prints SUCCESS. */
#include <math.h>
#include <stdio.h>

#include "arm_math.h"
#include "arm_math_mi355x.h"

#define N 1000

static float32_t signal[N];

int main(void) {
  double sum = 0.0, sumsq = 0.0, dev = 0.0;
  for (int i = 0; i < N; ++i) {
    signal[i] = (float32_t)(0.25 + 0.5 * sin(2.0 * 3.14159265358979323846 * 440.0 * i / 16000.0) + 1e-4 * i);
    sum += signal[i];
    sumsq += (double)signal[i] * signal[i];
  }
  const double mean = sum / N;
  for (int i = 0; i < N; ++i) dev += (signal[i] - mean) * (signal[i] - mean);
  const double want[4] = {mean, dev / (N - 1), sqrt(dev / (N - 1)), sqrt(sumsq / N)};

  float32_t got[4] = {-1.0f, -1.0f, -1.0f, -1.0f};
  arm_mean_f32(signal, N, &got[0]);
  arm_var_f32(signal, N, &got[1]);
  arm_std_f32(signal, N, &got[2]);
  arm_rms_f32(signal, N, &got[3]);
  if (arm_mi355x_last_error() != 0) {
    printf("FAILURE: %s\n", arm_mi355x_last_error_string());
    return 1;
  }
  /* N rounded adds of terms below 1 each: a relative error of N * 2^-24 = 6e-5 bounds every figure */
  static const char *name[4] = {"mean", "variance", "standard deviation", "rms"};
  int bad = 0;
  for (int k = 0; k < 4; ++k) {
    const double rel = fabs(got[k] - want[k]) / fabs(want[k]);
    printf("%-18s %.7f  (double: %.9f, relative error %.1e)\n", name[k], got[k], want[k], rel);
    if (!(rel < N * ldexp(1.0, -24))) bad = 1;
  }
  printf(bad ? "FAILURE\n" : "SUCCESS\n");
  return bad;
}
