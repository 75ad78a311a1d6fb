#!/bin/bash
# AMG-PCG (--precond amg) against Jacobi / FSAI through the driver, on one MI355X:
#   1. tail pass: amg_tail_rows 0 / 256 / 1024 / 4096 / 16384 on tests/xn3b_A_18.txt and config 3
#   2. solves/s and iterations: config 3 (tol 1e-8), general_values (config 3's pattern with
#      per-row coefficients), xn3b_A_18 (config 2): jacobi, fsai, amg
#   3. config 4 (64 M-row 7-point operator): AMG set-up time and solve
#   4. rocprofv3 --kernel-trace --stats of AMG-PCG on config 3 and xn3b_A_18
#   5. (on request) the V-cycle's smoother: l1-Jacobi nu = 1, 2 against Chebyshev nu = 1, 2, 3 (ratio 10) and
#      nu = 2 (ratio 4) on xn3b_A_18 and config 3, two fresh processes each, the variants alternating
#   6. (on request) the V-cycle's precision: fp64 against fp32 (--amg-precision) at nu = 1, 2 on xn3b_A_18 and
#      config 3, two fresh processes each, the variants alternating; then tools/gpu_amg_cycle_bw.py: the time of one
#      application and amg_cycle_bytes over it
#   7. (on request) multicolour Gauss-Seidel (--amg-smoother mcgs) at nu = 1, 2 beside l1-Jacobi nu = 1, 2 and
#      Chebyshev nu = 2, fp64 and fp32 cycle, on xn3b_A_18 and config 3, two fresh processes each, the variants
#      alternating; then tools/gpu_amg_cycle_bw.py with every smoother
# Every GPU step has its own time limit; the script stops at the first step that fails.
# Usage: tools/gpu_amg_profile.sh OUT_DIR [steps]   (steps: a subset of "1234567", default "1234")
OUT=${1:?usage: tools/gpu_amg_profile.sh OUT_DIR [steps]}
STEPS=${2:-1234}
mkdir -p "$OUT"
D=lsbench_amd/csrc/driver
C3=synth:lap2d:nx=3162,ny=3162
CG=synth:lap2d:nx=3162,ny=3162,coef=1
C4=synth:lap3d:nx=400,ny=400,nz=400
XN="$OUT/xn3b_A_18.txt"
gunzip -c tests/golden/matrices/xn3b_A_18.txt.gz > "$XN" || exit 1

# run NAME LIMIT_S ARGS...: one driver invocation, its record line into $OUT/summary.txt
run() {
  local name=$1 lim=$2
  shift 2
  local t0=$(date +%s.%N)
  timeout -k 10 "$lim" "$D" --solver hip --verbose 1 "$@" > "$OUT/$name.out" 2> "$OUT/$name.err"
  local rc=$?
  local rec=$(grep -A1 '^===hip_cdna4' "$OUT/$name.out" | tail -n 1)
  local setup=$(grep -o 'set-up [0-9.]* s' "$OUT/$name.err" | head -n 1)
  printf '%-28s rc=%d wall=%.1fs  iters,relres,status,tol,solves_per_sec,nshards=%s  %s\n' "$name" $rc \
    "$(awk "BEGIN{print $(date +%s.%N) - $t0}")" "$rec" "$setup" | tee -a "$OUT/summary.txt"
  return $rc
}

if [[ $STEPS == *1* ]]; then
  for t in 0 256 1024 4096 16384; do
    run "xn3b_amg_tail$t" 120 --matrix "$XN" --precond amg --amg-tail-rows $t --trials=200 || exit $?
  done
  for t in 0 256 1024 4096 16384; do
    run "c3_amg_tail$t" 300 --matrix $C3 --operator raw --tol 1e-8 --precond amg --amg-tail-rows $t --trials=10 || exit $?
  done
fi
if [[ $STEPS == *2* ]]; then
  run c3_jacobi 300 --matrix $C3 --operator raw --tol 1e-8 --trials=3 || exit $?
  run c3_amg 300 --matrix $C3 --operator raw --tol 1e-8 --precond amg --trials=10 || exit $?
  run c3_amg_nu2 300 --matrix $C3 --operator raw --tol 1e-8 --precond amg --amg-sweeps 2 --trials=10 || exit $?
  run gv_jacobi 300 --matrix $CG --operator raw --tol 1e-8 --trials=3 || exit $?
  run gv_amg 300 --matrix $CG --operator raw --tol 1e-8 --precond amg --trials=10 || exit $?
  run xn3b_jacobi 120 --matrix "$XN" --trials=200 || exit $?
  run xn3b_fsai 120 --matrix "$XN" --precond fsai --trials=200 || exit $?
  run xn3b_amg 120 --matrix "$XN" --precond amg --trials=200 || exit $?
fi
if [[ $STEPS == *3* ]]; then
  run c4_amg 900 --matrix $C4 --operator raw --tol 1e-8 --precond amg --trials=2 || exit $?
fi
if [[ $STEPS == *4* ]]; then
  for m in c3 xn3b; do
    if [ $m = c3 ]; then args="--matrix $C3 --operator raw --tol 1e-8 --trials=5"; else args="--matrix $XN --trials=100"; fi
    timeout -k 10 600 rocprofv3 --kernel-trace --stats --output-format csv -d "$OUT/prof_$m" -o prof -- \
      "$D" --solver hip $args --precond amg > "$OUT/prof_$m.log" 2>&1 || exit $?
    f=$(find "$OUT/prof_$m" -name '*kernel_stats.csv' | head -n 1)
    echo "== $m: rocprofv3 kernel stats ($f)" | tee -a "$OUT/summary.txt"
    [ -n "$f" ] && cut -d, -f1-8 "$f" | head -n 16 | tee -a "$OUT/summary.txt"
  done
fi
if [[ $STEPS == *5* ]]; then
  smoothers() { # PREFIX LIMIT_S ARGS...
    local p=$1 lim=$2
    shift 2
    for rep in a b; do
      run ${p}_l1_nu1_$rep $lim "$@" --precond amg || exit $?
      run ${p}_cheb_nu1_$rep $lim "$@" --precond amg --amg-smoother cheb || exit $?
      run ${p}_l1_nu2_$rep $lim "$@" --precond amg --amg-sweeps 2 || exit $?
      run ${p}_cheb_nu2_$rep $lim "$@" --precond amg --amg-smoother cheb --amg-sweeps 2 || exit $?
      run ${p}_cheb_nu3_$rep $lim "$@" --precond amg --amg-smoother cheb --amg-sweeps 3 || exit $?
      run ${p}_cheb_nu2_r4_$rep $lim "$@" --precond amg --amg-smoother cheb --amg-sweeps 2 --amg-cheb-ratio 4 || exit $?
    done
  }
  smoothers xn3b 120 --matrix "$XN" --trials=200
  smoothers c3 300 --matrix $C3 --operator raw --tol 1e-8 --trials=10
fi
if [[ $STEPS == *6* ]]; then
  precisions() { # PREFIX LIMIT_S ARGS...
    local p=$1 lim=$2
    shift 2
    for rep in a b; do
      for nu in 1 2; do
        run ${p}_fp64_nu${nu}_$rep $lim "$@" --precond amg --amg-sweeps $nu || exit $?
        run ${p}_fp32_nu${nu}_$rep $lim "$@" --precond amg --amg-sweeps $nu --amg-precision fp32 || exit $?
      done
    done
  }
  precisions xn3b 120 --matrix "$XN" --trials=200
  precisions c3 300 --matrix $C3 --operator raw --tol 1e-8 --trials=10
  for m in "$XN" $C3; do
    timeout -k 10 300 python tools/gpu_amg_cycle_bw.py "$m" 2>&1 | tee -a "$OUT/summary.txt"
    [ ${PIPESTATUS[0]} -eq 0 ] || exit 1
  done
fi
if [[ $STEPS == *7* ]]; then
  mcgs_rows() { # PREFIX LIMIT_S ARGS...
    local p=$1 lim=$2
    shift 2
    for rep in a b; do
      for prec in fp64 fp32; do
        run ${p}_l1_nu1_${prec}_$rep $lim "$@" --precond amg --amg-precision $prec || exit $?
        run ${p}_mcgs_nu1_${prec}_$rep $lim "$@" --precond amg --amg-precision $prec --amg-smoother mcgs || exit $?
        run ${p}_l1_nu2_${prec}_$rep $lim "$@" --precond amg --amg-precision $prec --amg-sweeps 2 || exit $?
        run ${p}_cheb_nu2_${prec}_$rep $lim "$@" --precond amg --amg-precision $prec --amg-smoother cheb --amg-sweeps 2 || exit $?
        run ${p}_mcgs_nu2_${prec}_$rep $lim "$@" --precond amg --amg-precision $prec --amg-smoother mcgs --amg-sweeps 2 || exit $?
      done
    done
  }
  mcgs_rows xn3b 120 --matrix "$XN" --trials=200
  mcgs_rows c3 300 --matrix $C3 --operator raw --tol 1e-8 --trials=10
  for m in "$XN" $C3; do
    timeout -k 10 300 python tools/gpu_amg_cycle_bw.py "$m" all 2>&1 | tee -a "$OUT/summary.txt"
    [ ${PIPESTATUS[0]} -eq 0 ] || exit 1
  done
fi
exit 0
