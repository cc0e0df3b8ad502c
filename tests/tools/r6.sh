#!/bin/bash
# round-6 profile at HEAD (run on the GPU box): kernel trace + PMC passes of the default bench, the un-profiled default bench (CPU
# baseline incl. one full-size evaluation, parity gates incl. the cold goldens at headline size, exact-fp32 / bf16x3 records, config-4
# Hessian), the other workloads, the A/B of the one-launch MLP sweeps, the per-sweep table, the size sweep, the kernel sequence
cd $GRAFT_REPO_ROOT
D=${PROF_OUT:-$PWD/prof_out}/r6
mkdir -p $D
bash tests/tools/pmc_bench.sh r6 > $D/stdout.txt 2>&1
python bench.py --full > $D/bench.json 2> $D/bench.err
rm -f $D/bench_other_workloads.jsonl
for w in batch256 md1024 taxol; do python bench.py --full --workload $w --no-hessian 2>/dev/null | tail -1 >> $D/bench_other_workloads.jsonl; done
bash tests/tools/ab_env.sh AIMNET_GEMM_CHAIN=0 --no-exact-f32 --no-hessian --no-repeat > $D/chain_ab.txt 2>&1
python tests/tools/chain_sweep.py 2>&1 | grep -v amdgpu > $D/chain_sweeps.txt
M=2304 python tests/tools/chain_sweep.py 2>&1 | grep -v amdgpu >> $D/chain_sweeps.txt
python tests/tools/size_sweep.py 2>/dev/null > $D/size_sweep.jsonl
AIMNET_GEMM_CHAIN=0 python tests/tools/size_sweep.py 2>/dev/null > $D/size_sweep_per_layer.jsonl
bash tests/tools/kseq.sh 2> /dev/null > $D/kernel_sequence.txt
tail -3 $D/stdout.txt; tail -c 1200 $D/bench.json; tail -5 $D/chain_ab.txt
