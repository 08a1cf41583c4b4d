#!/bin/bash
# Round-6 evidence at the final head: PMC traffic record (bound to the GEMM sources), rocprofv3 kernel stats of the bench command, the GEMM loss
# table, the c3 / c4 / c5 bench lines, the default bench line (bench.py --full: every leg).   bash tools/r06_evidence.sh OUT   (on the GPU box;
# results under the directory OUT, relative to the repository root)
R=${GRAFT_REPO_ROOT:-$PWD}
O=${1:?usage: bash tools/r06_evidence.sh OUT}
mkdir -p $R/$O
export PYTHONPATH=$R
bash tools/pmc_traffic_r06.sh $O/pmc_traffic_r06 $R/$O/r06_pmc_traffic.json > $O/r06_pmc_traffic.log 2>&1
cp $R/$O/r06_pmc_traffic.json $R/profiles/r06_pmc_traffic.json    # the bench lines below quote this record (bound to the GEMM sources by sources_sha)
cd /tmp && export TMPDIR=/tmp
timeout 900 rocprofv3 --kernel-trace --stats -d $R/$O/r06_prof -o bench --output-format csv -- python3 $R/bench.py --full --no-parity --no-cpu-baseline --steps 4 --warmup 1 > $R/$O/r06_bench_under_rocprof.json 2> $R/$O/r06_bench_under_rocprof.err
cd $R
find $O/r06_prof -name "*kernel_stats.csv" | head -1 | xargs -I{} cp {} $O/r06_bench_kernel_stats.csv
rm -rf $O/r06_prof $O/pmc_traffic_r06
timeout 400 python tools/gemm_loss_table.py 12 > $O/r06_gemm_loss_table.txt 2> $O/r06_gemm_loss_table.err
timeout 600 python bench.py --full --guidance clustered_threshold --no-cpu-baseline --no-parity > $O/r06_bench_c3.json 2> $O/r06_bench_c3.err
timeout 600 python bench.py --full --img2img --size 768 --batch 4 --no-cpu-baseline --no-parity > $O/r06_bench_c4.json 2> $O/r06_bench_c4.err
timeout 900 python bench.py --full --preset sd21 --size 768 --no-cpu-baseline --no-parity > $O/r06_bench_c5.json 2> $O/r06_bench_c5.err
timeout 900 python bench.py --full > $O/r06_bench.json 2> $O/r06_bench.err
cat $O/r06_pmc_traffic.log | tail -14; head -8 $O/r06_bench_kernel_stats.csv; head -6 $O/r06_gemm_loss_table.txt
python tools/bench_summary.py $O/r06_bench_c3.json $O/r06_bench_c4.json $O/r06_bench_c5.json $O/r06_bench.json $O/r06_bench_under_rocprof.json
