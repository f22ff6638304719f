set -e
mkdir -p bench_out/big
for n in 512 2048 4096; do
  timeout -k 10 120 python bench.py --full --workload cfft_f32_1024 --fftlen $n --steps 10 --warmup 3 --no-cpu-baseline --no-companion > bench_out/big/cfft_$n.json 2> bench_out/big/cfft_$n.err
done
for n in 1024 4096; do
  timeout -k 10 120 python bench.py --full --workload rfft_f32 --fftlen $n --steps 10 --warmup 3 --no-cpu-baseline > bench_out/big/rfft_$n.json 2> bench_out/big/rfft_$n.err
done
timeout -k 10 120 python bench.py --full --workload mfcc_f32 --steps 10 --warmup 3 --no-cpu-baseline > bench_out/big/mfcc.json 2> bench_out/big/mfcc.err
