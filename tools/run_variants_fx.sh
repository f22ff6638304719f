set -e
# Sweep cfft_q31/q15 N=4096 variants (tools/build_variant.sh <name> ...).
mkdir -p bench_out/var
for lib in base $VARIANTS; do
  if [ $lib = base ]; then L=cmsis-dsp_amd/lib/libcmsisdsp_mi355x.so; else L=cmsis-dsp_amd/lib/variants/lib_$lib.so; fi
  for wl in cfft_q31_4096 cfft_q15_4096; do
    CMSISDSP_MI355X_LIB=$L timeout -k 10 200 python bench.py --full --workload $wl --no-cpu-baseline > bench_out/var/${lib}_$wl.json 2> bench_out/var/${lib}_$wl.err
  done
done
