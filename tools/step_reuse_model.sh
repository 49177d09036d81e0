#!/bin/bash
# Step reuse inside the running model: the reference model with its chemistry on the GPU (oracle/_ref/mistra_gpu,
# oracle/build_gpu_model.sh), run twice per case for the minutes of the case's tests/golden/endstate_<case>.npz — once plain and once with
# MISTRA_CHEM_HSTART_REUSE=1 in its environment, which needs no relinking.  Per run: the model's "chemistry stem" line (wall time of the time loop and of the
# chemistry in it) and the distance of its chemical end state from the UNPATCHED model's (the golden end state), in the measure of tests/test_gpu_model.py;
# and the distance between the two runs.  Nothing is asserted about the reuse run: how far the reference algorithm moves when it starts at other step sizes
# over a chained run is what this states.  Run on the GPU box, from anywhere:
#   tools/step_reuse_model.sh > profiles/r08_step_reuse_model.txt
# Every model run has its own time limit; a run that fails ends the study (nothing more is started).
set -o pipefail
cd "$(dirname "${BASH_SOURCE[0]}")/.." || exit 1
TMP="$(mktemp -d "${TMPDIR:-/tmp}/step_reuse_model.XXXXXX")" || exit 1
BIN="$PWD/oracle/_ref/mistra_gpu"
[ -x "$BIN" ] || { echo "oracle/_ref/mistra_gpu is not built (oracle/build_gpu_model.sh)"; exit 1; }
LIMIT="${MISTRA_STUDY_LIMIT:-300}"      # seconds per model run

compare() {      # <case> <plain dump> <reuse dump>
python3 - "$1" "$2" "$3" <<'PY'
import sys
import numpy as np
case, plain, reuse = sys.argv[1:4]
g = np.load("tests/golden/endstate_%s.npz" % case)
KEYS = ("s1", "s3", "sl1", "sion1")


def load(path):      # as tests/test_gpu_model.py: _load_dump
    raw = open(path, "rb").read()
    j1, j5, nsl, nsi, n = (int(x) for x in np.frombuffer(raw, np.int32, 5))
    d, o, out = np.frombuffer(raw, np.float64, offset=20), 0, {}
    for key, width in zip(KEYS, (j1, j5, nsl, nsi)):
        out[key] = d[o:o + width * n].reshape(n, width)
        o += width * n
    return out


def distance(have, want):
    """tests/test_gpu_model.py's measure: entries above 1e-3 of their species' column maximum, relative; the others as a fraction of that maximum"""
    major_worst, minor_worst = 0.0, 0.0
    for key in KEYS:
        w, h = want[key], have[key]
        scale = np.abs(w).max(axis=0, keepdims=True)
        major = np.abs(w) > 1e-3 * scale
        if major.any():
            major_worst = max(major_worst, float((np.abs(h - w)[major] / np.abs(w[major])).max()))
        rest = ~major & (np.broadcast_to(scale, w.shape) > 0)
        if rest.any():
            minor_worst = max(minor_worst, float((np.abs(h - w)[rest] / np.broadcast_to(scale, w.shape)[rest]).max()))
    return major_worst, minor_worst


want = {k: g[k] for k in KEYS}
a, b = load(plain), load(reuse)
print("   end state, plain, from the unpatched model's:       %.2e (entries above 1e-3 of their species' column maximum), %.2e of that maximum (the others)" % distance(a, want))
print("   end state, step reuse, from the unpatched model's:  %.2e, %.2e" % distance(b, want))
print("   end state, step reuse, from the plain run's:        %.2e, %.2e" % distance(b, a))
PY
}

study() {      # <case>
  local case="$1" minutes line
  minutes=$(python3 -c "import numpy as np; print(int(np.load('tests/golden/endstate_$case.npz')['minutes']))") || return 1
  line=$(timeout -k 10 "$LIMIT" oracle/model_run.sh "$BIN" "$case" "$minutes" "$TMP/${case}_plain" MISTRA_COLUMN_DUMP="$TMP/${case}_plain.bin" MISTRA_CHEM_HSTART_REUSE=0) ||
    { echo "$case, plain: $line"; return 1; }
  echo "$case, $minutes model minutes, plain:      $line"
  line=$(timeout -k 10 "$LIMIT" oracle/model_run.sh "$BIN" "$case" "$minutes" "$TMP/${case}_reuse" MISTRA_COLUMN_DUMP="$TMP/${case}_reuse.bin" MISTRA_CHEM_HSTART_REUSE=1) ||
    { echo "$case, step reuse: $line"; return 1; }
  echo "$case, $minutes model minutes, step reuse: $line"
  compare "$case" "$TMP/${case}_plain.bin" "$TMP/${case}_reuse.bin"
}

study Joyce2014_basecase && study BTZ96
rc=$?
rm -rf "$TMP"
[ $rc -eq 0 ] || echo "the study stopped: a model run failed or ran into its time limit (status $rc)"
exit $rc
