#!/bin/bash
# A/B of library builds in ONE GPU session (boxes differ by several per cent, so only alternating runs on one box compare):
#   tools/ab_bench.sh out_dir libA.so libB.so [...]      -> bench.py headline-only runs, A B A B, key numbers per run
# AB_REPS alternations (default 2) of AB_STEPS timed proofs after AB_WARMUP (default 8 after 2).  A run that fails or times out ends the script: nothing more is started on a card that has just
# failed a run.
# Variant libraries are built with `python -m ark_plonk_amd.build` on a modified tree and copied to tools/bin/ (not tracked).
set -u
out=$1; shift
mkdir -p "$out"
for rep in $(seq 1 "${AB_REPS:-2}"); do
  for lib in "$@"; do
    name=$(basename "$lib" .so)
    ARK_PLONK_AMD_LIB="$lib" timeout -k 10 240 python bench.py --steps "${AB_STEPS:-8}" --warmup "${AB_WARMUP:-2}" --full --extra-legs off --streams-leg 0 --no-cpu-baseline \
      > "$out/${name}_$rep.json" 2> "$out/${name}_$rep.err" || { echo "$name run $rep failed (status $?)"; tail -n 5 "$out/${name}_$rep.err"; exit 1; }
    python - "$out/${name}_$rep.json" "$name" <<'PY'
import json, sys
d = json.load(open(sys.argv[1]))
b = d["msm_breakdown_ms_per_proof"]
print("%-28s %7.3f proofs/s  step %7.3f ms  acc %6.4f ms/launch  msm %6.2f (sort %5.2f reduce %5.2f accumulate %6.2f)  ntt %5.2f  %s" % (
      sys.argv[2], d["value"], d["ms_per_step"], d["roofline"]["avg_launch_ms"], d["msm_ms_per_proof"], b["sort"], b["reduce"], b["accumulate"],
      d["ntt_ms_per_proof"], d.get("commitments_sha256", "")[:12]))
PY
  done
done
