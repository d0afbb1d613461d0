#!/bin/bash
# Counters of the blend kernels for the backward's pair reduction: the kernel trace, then the VALU and
# LDS counters, each PMC pass in a run of its own (no trace domains), on the metric scene and the train-like scene.
#   TAG=branch bash tools/prof_reduction.sh                     # the current build
#   TAG=parent LIBDIR=<dir with another libgs4d.so> bash tools/prof_reduction.sh
# Output goes under $OUT_ROOT (default prof_out/, git-ignored): $OUT_ROOT/prof_<TAG>/<run>_<scene>/.
# Summary per run: python tools/pmc_kernels.py <that directory> render_
export TMPDIR=/tmp
OUT=${OUT_ROOT:-prof_out}/prof_${TAG:-reduction}
mkdir -p $OUT
[ -n "$LIBDIR" ] && export LD_LIBRARY_PATH=$LIBDIR${LD_LIBRARY_PATH:+:$LD_LIBRARY_PATH}
ARGS="--full --steps 10 --warmup 3 --no-cpu-baseline --no-train-step --no-extras"
run() {
    local name=$1 scene=$2; shift 2
    timeout -k 10 240 rocprofv3 "$@" -d $OUT/${name}_$scene -o run --output-format csv -- python3 bench.py $ARGS --scene $scene > $OUT/bench_${name}_$scene.log 2>&1 \
        || { echo "$name $scene rc=$?"; tail -20 $OUT/bench_${name}_$scene.log; exit 1; }
}
for scene in synthetic train_like; do
    run trace $scene --kernel-trace --stats
    run derived $scene --pmc VALUBusy
    run valu $scene --pmc SQ_INSTS_VALU SQ_ACTIVE_INST_VALU SQ_WAVE_CYCLES SQ_BUSY_CYCLES SQ_WAIT_INST_LDS
    run lds $scene --pmc SQ_INSTS_LDS SQ_ACTIVE_INST_LDS SQ_LDS_BANK_CONFLICT SQ_LDS_IDX_ACTIVE SQ_LDS_ADDR_CONFLICT
done
echo done
