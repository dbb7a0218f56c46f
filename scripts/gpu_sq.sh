#!/bin/bash
# SQ counter passes (issue vs wait breakdown) of the C2 bench kernels. usage: scripts/gpu_sq.sh <outdir-name>
set -o pipefail
cd $GRAFT_REPO_ROOT
export TMPDIR=/tmp
O=gpurun_out/$1
mkdir -p $O
P1="SQ_WAVES SQ_WAVE_CYCLES SQ_BUSY_CYCLES SQ_INSTS_VALU SQ_ACTIVE_INST_VALU SQ_ACTIVE_INST_ANY SQ_WAIT_ANY SQ_WAIT_INST_ANY GRBM_GUI_ACTIVE"
P2="SQ_INSTS_SALU SQ_INSTS_SMEM SQ_INSTS_LDS SQ_INSTS_VMEM_RD SQ_INSTS_VMEM_WR SQ_ACTIVE_INST_LDS SQ_WAIT_INST_LDS SQ_INSTS_VALU_FMA_F64"
scripts/gpu_session.sh \
 "timeout -s KILL 120 rocprofv3 --pmc $P1 -d $O/c2_p1 -o p --output-format csv -- python bench.py --full --steps 10 --warmup 10 --no-cpu-baseline > $O/c2_p1.log 2>&1" \
 "timeout -s KILL 120 rocprofv3 --pmc $P2 -d $O/c2_p2 -o p --output-format csv -- python bench.py --full --steps 10 --warmup 10 --no-cpu-baseline > $O/c2_p2.log 2>&1"
