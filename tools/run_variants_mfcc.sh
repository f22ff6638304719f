set -e
mkdir -p bench_out/var
for lib in base u1 skip; do
  if [ $lib = base ]; then L=cmsis-dsp_amd/lib/libcmsisdsp_mi355x.so; else L=cmsis-dsp_amd/lib/variants/lib_$lib.so; fi
  CMSISDSP_MI355X_LIB=$L timeout -k 10 200 python bench.py --full --workload mfcc_f32 --no-cpu-baseline > bench_out/var/mfcc_$lib.json 2> bench_out/var/mfcc_$lib.err
done
