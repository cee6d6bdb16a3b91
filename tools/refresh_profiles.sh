# (no set -e: a failing diagnostics step must not cost the rest of the evidence)
# One GPU-box run that regenerates the round's evidence under $OUT (copy what is to be judged into profiles/).
# Usage, from the repo root: bash tools/refresh_profiles.sh [round-label [outdir]]   (outdir relative to the repo root)
R=${1:-r3}
OUT=${2:-profile_runs/$R}
mkdir -p $OUT
python bench.py --full > $OUT/bench.json 2> $OUT/bench.err
python bench.py --full --streams 1 --no-cpu-baseline --no-other-configs > $OUT/bench_streams1.json 2>> $OUT/bench.err
python bench.py --full --schedule layered --no-cpu-baseline --no-other-configs > $OUT/bench_layered.json 2>> $OUT/bench.err
python tools/stamp_profile.py --mode f32t > $OUT/stamps.txt 2>&1
python tools/stamp_profile.py --mode f32x3 > $OUT/stamps_f32x3.txt 2>&1
ROOT=$PWD
cd /tmp && export TMPDIR=/tmp
rocprofv3 --kernel-trace --stats --output-format csv -d $ROOT/$OUT/prof -- python3 $ROOT/bench.py --full --steps 20 --warmup 5 --no-cpu-baseline --no-other-configs > $ROOT/$OUT/prof.log 2>&1
rocprofv3 --kernel-trace --stats --output-format csv -d $ROOT/$OUT/prof_s1 -- python3 $ROOT/bench.py --full --steps 20 --warmup 5 --streams 1 --no-cpu-baseline --no-other-configs > $ROOT/$OUT/prof_s1.log 2>&1
rocprofv3 --kernel-trace --stats --output-format csv -d $ROOT/$OUT/prof_layered -- python3 $ROOT/bench.py --full --steps 20 --warmup 5 --no-cpu-baseline --no-other-configs --schedule layered > $ROOT/$OUT/prof_layered.log 2>&1
rocprofv3 --kernel-trace --stats --output-format csv -d $ROOT/$OUT/prof_wide -- python3 $ROOT/tools/wide_probe.py > $ROOT/$OUT/prof_wide.log 2>&1
rocprofv3 --kernel-trace --stats --output-format csv -d $ROOT/$OUT/prof_wide_x3 -- python3 $ROOT/tools/wide_probe.py --mode f32x3 > $ROOT/$OUT/prof_wide_x3.log 2>&1
cd $ROOT
python tools/wide_probe.py > $OUT/wide_probe.json 2>> $OUT/bench.err
python tools/wide_probe.py --mode f32x3 >> $OUT/wide_probe.json 2>> $OUT/bench.err
python tools/wide_mode_bench.py --iters 20 > $OUT/wide_modes.json 2>> $OUT/bench.err
if [ -f ionic_mpnn_amd/csrc/ab/lib_STAMPS.so ]; then  # (a -DIMPNN_DIAG_WIDE_STAMPS build of the CURRENT sources)
  IMPNN_LIB=$ROOT/ionic_mpnn_amd/csrc/ab/lib_STAMPS.so python tools/wide_stamps.py > $OUT/wide_stamps.txt 2>&1 || true
  IMPNN_LIB=$ROOT/ionic_mpnn_amd/csrc/ab/lib_STAMPS.so python tools/wide_stamps.py --mode f32x3 > $OUT/wide_stamps_f32x3.txt 2>&1 || true
fi
bash tools/pmc_profile.sh $OUT/pmc > /dev/null 2>&1
bash tools/train_profiles.sh $OUT/train > /dev/null 2>&1   # training-step timings + config-5 kernel summaries
python tools/gu_pair_bench.py > $OUT/gu_pair_bench.jsonl 2>> $OUT/bench.err
cat $OUT/bench.json
