# usage (on an MI355X, from anywhere): bash tools/refresh_profiles.sh <tag> <output folder>; then python3 tools/pmc_wrap.py <tag> <output folder>
# bench line, rocprofv3 kernel statistics of the same command, and four separate PMC passes (the guide's HBM / rocprofv3 recipe:
# FETCH_SIZE and WRITE_SIZE each in a pass of their own, never combined with tracing domains) -> <output folder>/<tag>_*
# Every bench.py run here is a --full one: the profiles cover the PCIe-inclusive and contiguous-track legs and the instrumented passes.
set -e
TAG=${1:-r03}
OUT=$(mkdir -p "${2:?usage: refresh_profiles.sh <tag> <output folder>}" && cd "$2" && pwd)
cd "$(dirname "$0")/.."
timeout -k 10 900 python bench.py --full > $OUT/${TAG}_bench.log 2>&1
grep "^{\"metric\"" $OUT/${TAG}_bench.log | tail -1 > $OUT/${TAG}_bench.json
timeout -k 10 300 rocprofv3 --kernel-trace --stats -d $OUT/ks -o ks --output-format csv -- python3 bench.py --full --no-cpu --no-extras > $OUT/ks.log 2>&1
cp $(find $OUT/ks -name "*kernel_stats.csv" | head -1) $OUT/${TAG}_bench_kernel_stats.csv
python3 tools/kstats.py $OUT/ks > $OUT/${TAG}_bench_kernel_stats.txt
rm -rf $OUT/ks
timeout -k 10 300 rocprofv3 --kernel-trace --pmc SQ_INSTS_VALU_MFMA_MOPS_F64 SQ_VALU_MFMA_BUSY_CYCLES SQ_BUSY_CYCLES SQ_WAVE_CYCLES -d $OUT/p1 -o p --output-format csv -- python3 bench.py --full --no-cpu --no-extras --steps 4 --warmup 1 > $OUT/p1.log 2>&1
timeout -k 10 300 rocprofv3 --kernel-trace --pmc FETCH_SIZE -d $OUT/p2 -o p --output-format csv -- python3 bench.py --full --no-cpu --no-extras --steps 4 --warmup 1 > $OUT/p2.log 2>&1
timeout -k 10 300 rocprofv3 --kernel-trace --pmc WRITE_SIZE -d $OUT/p3 -o p --output-format csv -- python3 bench.py --full --no-cpu --no-extras --steps 4 --warmup 1 > $OUT/p3.log 2>&1
timeout -k 10 300 rocprofv3 --kernel-trace --pmc SQ_INSTS_VALU SQ_INSTS_SALU SQ_INSTS_LDS SQ_INSTS_VMEM_RD SQ_LDS_BANK_CONFLICT SQ_WAVES -d $OUT/p4 -o p --output-format csv -- python3 bench.py --full --no-cpu --no-extras --steps 4 --warmup 1 > $OUT/p4.log 2>&1
python3 tools/pmc_summary.py $OUT/p1 $OUT/p2 $OUT/p3 $OUT/p4 > $OUT/${TAG}_pmc_kernels.json
rm -rf $OUT/p1 $OUT/p2 $OUT/p3 $OUT/p4
echo REFRESH-OK
