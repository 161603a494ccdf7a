#!/bin/bash
# Collects the artefacts profiles/ holds for a round, on a machine with the GPU (about 40 minutes):
#   bash tools/collect_profiles.sh
# then, where the tree is committed from:  python tools/install_profiles.py r04
# Every GPU leg runs under its own time limit, and the first leg that faults, aborts, times out or fails ends the collection
# (nothing more is started on the card).  PMC passes run alone (never with a trace domain).
set -u
cd "$(dirname "$0")/.."
export TMPDIR=/tmp
O=gpurun_out/collect
rm -rf "$O"; mkdir -p "$O"
leg() {  # leg SECONDS STDOUT STDERR COMMAND...
  local t=$1 out=$2 err=$3; shift 3
  timeout -k 10 "$t" "$@" > "$out" 2> "$err"
  local rc=$?
  if [ $rc -ne 0 ]; then echo "collect_profiles.sh: \`$*\` exited $rc; no further GPU leg is started" >&2; exit $rc; fi
}
# 1. the bench line itself (default flags: what the driver runs)
leg 700 "$O/bench.json" "$O/bench.err" python3 bench.py
# 2. the same command under the kernel trace (kernel averages must agree with the line's HIP-event figures)
leg 900 "$O/bench_under_rocprof.json" "$O/kt_bench.err" rocprofv3 --kernel-trace --stats --output-format csv -d "$O/kt_bench" -- python3 bench.py --no-cpu-baseline
# 3. THE HEADLINE ALONE (bench.py --headline-only: 200 pre-warm, 10 warm-up and 1000 timed steps of the four-deep loop in one round, nothing
#    else: 1210 MSMs): every k_acc_tasks<Fq> launch of the trace is a full 2^20-pair launch of the pipelined loop, so the stats file's average
#    for that kernel is close to roofline.kernel_ms of the line printed under the profiler, and the last 1000 launches (the timed ones) are it
#    (the pre-warm's cold-clock launches are a sixth of the launches)
leg 300 "$O/msm_under_rocprof.json" "$O/kt_msm.err" rocprofv3 --kernel-trace --stats --output-format csv -d "$O/kt_msm" -- python3 bench.py --headline-only --steps 1000 --warmup 10
python3 tools/kernel_table.py "$O/kt_msm" --per 1210 --last-of k_acc_tasks 1000 --title "bench.py --headline-only --steps 1000 --warmup 10 under rocprofv3 --kernel-trace (1210 MSMs of 2^20 pairs, the last 1000 timed); us per unit = per MSM" > "$O/msm_kernel_table.txt" 2>&1
# 3b. the prover alone (bench.py --groth16-only: setup, 17 warm + 3 x 16 blocking proofs, 2 + 3 x 32 proofs two in flight): the phase table behind DESIGN.md section 10
leg 400 "$O/g16_under_rocprof.json" "$O/kt_g16.err" rocprofv3 --kernel-trace --stats --output-format csv -d "$O/kt_g16" -- python3 bench.py --groth16-only --steps 16
python3 tools/kernel_table.py "$O/kt_g16" --per 163 --split-grid k_acc_tasks --title "bench.py --groth16-only --steps 16 under rocprofv3 --kernel-trace: 2 setups + 163 proofs of 2^18 constraints (1 + 16 warm, 3 x 16 blocking, 2 + 3 x 32 two in flight: medians of three rounds); us per unit = per proof (setup kernels included in the list, not in a proof)" > "$O/g16_phase_table.txt" 2>&1
# 3c. the G2 MSM alone (2^18 pairs: 24 + 3 x 20 four in flight, 1 + 5 alone, 2 + 20 blocking in two window groups)
leg 300 "$O/g2_under_rocprof.json" "$O/kt_g2.err" rocprofv3 --kernel-trace --stats --output-format csv -d "$O/kt_g2" -- python3 bench.py --msm-g2-only --steps 20 --rounds 3 --no-cpu-baseline
python3 tools/kernel_table.py "$O/kt_g2" --split-grid k_acc_tasks --title "bench.py --msm-g2-only --steps 20 --rounds 3 under rocprofv3 --kernel-trace" > "$O/g2_kernel_table.txt" 2>&1
# 4. HBM traffic: one counter per pass
for c in FETCH_SIZE WRITE_SIZE; do
  leg 300 "$O/pmc_$c.json" "$O/pmc_$c.err" rocprofv3 --pmc $c --output-format csv -d "$O/pmc_$c" -- python3 bench.py --headline-only --steps 3 --warmup 1 --rounds 1 --prewarm 4
done
# 5. the transform alone (2^22 forward NTT: the two k_ntt_tile kernels without the prover's 2^18 launches in the averages)
leg 300 "$O/ntt_under_rocprof.json" "$O/kt_ntt.err" rocprofv3 --kernel-trace --stats --output-format csv -d "$O/kt_ntt" -- python3 bench.py --ntt-only --ntt-variant dft --steps 300
# 5b. the other three transforms of fft.rs:100-127, one run each
for v in idft coset_dft coset_idft; do
  leg 300 "$O/ntt_${v}_under_rocprof.json" "$O/kt_ntt_$v.err" rocprofv3 --kernel-trace --stats --output-format csv -d "$O/kt_ntt_$v" -- python3 bench.py --ntt-only --ntt-variant $v --steps 300
done
for c in FETCH_SIZE WRITE_SIZE; do
  leg 300 "$O/pmcntt_$c.json" "$O/pmcntt_$c.err" rocprofv3 --pmc $c --output-format csv -d "$O/pmcntt_$c" -- python3 bench.py --ntt-only --ntt-variant dft --steps 10
done
# 6. SQ issue / wait counters of the same leg
leg 300 "$O/pmcntt_SQ.json" "$O/pmcntt_SQ.err" rocprofv3 --pmc SQ_WAVE_CYCLES SQ_WAIT_ANY SQ_WAIT_INST_ANY SQ_ACTIVE_INST_ANY SQ_ACTIVE_INST_VALU SQ_INSTS_VALU SQ_WAVES GRBM_GUI_ACTIVE --output-format csv -d "$O/pmcntt_SQ" -- python3 bench.py --ntt-only --ntt-variant dft --steps 10
leg 300 "$O/pmc_SQ.json" "$O/pmc_SQ.err" rocprofv3 --pmc SQ_WAVE_CYCLES SQ_WAIT_ANY SQ_WAIT_INST_ANY SQ_ACTIVE_INST_ANY SQ_ACTIVE_INST_VALU SQ_INSTS_VALU SQ_WAVES GRBM_GUI_ACTIVE --output-format csv -d "$O/pmc_SQ" -- python3 bench.py --headline-only --steps 3 --warmup 1 --rounds 1 --prewarm 4
# 7. the multiplier and the transform's register pass alone (tools/ubench; built in-tree before the call)
U=tools/ubench
if [ -x $U/mul_rate ]; then
  leg 120 "$O/mul_rate_raw.txt" "$O/mul_rate.err" $U/mul_rate
  { echo "== fp29.h as shipped (one multiply-accumulate chain per column)"; grep -E "SIMD=(1|2|4|8) " "$O/mul_rate_raw.txt"; } > "$O/mul_rate.txt"
  if [ -x $U/mul_rate_c ]; then
    leg 120 "$O/mul_rate_c_raw.txt" "$O/mul_rate_c.err" $U/mul_rate_c
    { echo "== -DKG_NO_ASM_MAC (the columns left to the compiler)"; grep -E "SIMD=(1|2|4|8) " "$O/mul_rate_c_raw.txt"; } >> "$O/mul_rate.txt"
  fi
fi
if [ -x $U/mfma_const_mul ]; then leg 120 "$O/mfma_const_mul.txt" "$O/mfma_const_mul.err" $U/mfma_const_mul; fi
if [ -x $U/group_scatter ]; then
  leg 120 "$O/group_scatter.txt" "$O/group_scatter.err" $U/group_scatter 24 20
  leg 120 "$O/group_scatter_20.txt" "$O/group_scatter_20.err" $U/group_scatter 20 16
  cat "$O/group_scatter_20.txt" >> "$O/group_scatter.txt"; rm -f "$O/group_scatter_20.txt"
fi
if [ -x $U/ntt_pass_rate ]; then leg 120 "$O/ntt_pass_rate.txt" "$O/ntt_pass_rate.err" $U/ntt_pass_rate; fi
ls -R "$O" | head -80
tail -c 600 "$O/bench.json"
