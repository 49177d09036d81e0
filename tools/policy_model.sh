#!/bin/bash
# The integrator policy inside the running model: the reference model with its chemistry on the GPU (oracle/_ref/mistra_gpu,
# oracle/build_gpu_model.sh), run for the minutes of the case's tests/golden/endstate_<case>.npz — plain, and, for the case with cloudy `tot` layers (BTZ96),
# with MISTRA_CHEM_ATOL_REL_T=1e-13 and with MISTRA_CHEM_METHOD_T=rodas3 in its environment, which needs no relinking.  Per run: the model's "chemistry stem"
# line (wall time of the time loop and of the chemistry in it) and the distance of its chemical end state from the UNPATCHED model's (the golden end state)
# and from the plain run's, in the measure of tests/test_gpu_model.py.  Nothing is asserted about the policy runs: how far the reference algorithm moves at
# other settings over a chained run is what this states, and no speed-up is promised.  Run on the GPU box, from anywhere:
#   tools/policy_model.sh > profiles/r12_policy_model.txt
# Every model run has its own time limit; a run that fails ends the study (nothing more is started).
set -o pipefail
cd "$(dirname "${BASH_SOURCE[0]}")/.." || exit 1
TMP="$(mktemp -d "${TMPDIR:-/tmp}/policy_model.XXXXXX")" || exit 1
BIN="$PWD/oracle/_ref/mistra_gpu"
[ -x "$BIN" ] || { echo "oracle/_ref/mistra_gpu is not built (oracle/build_gpu_model.sh)"; exit 1; }
LIMIT="${MISTRA_STUDY_LIMIT:-300}"      # seconds per model run

compare() {      # <case> <label> <plain dump> <dump>
python3 - "$1" "$2" "$3" "$4" <<'PY'
import sys
import numpy as np
case, label, plain, other = sys.argv[1:5]
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
b = load(other)
print("   end state, %s, from the unpatched model's: %.2e (entries above 1e-3 of their species' column maximum), %.2e of that maximum (the others)" % ((label,) + distance(b, want)))
if plain != other:
    print("   end state, %s, from the plain run's:       %.2e, %.2e" % ((label,) + distance(b, load(plain))))
PY
}

run() {      # <case> <minutes> <label> <tag> [ENV=VALUE ...]: one model run, its line and its distances
  local case="$1" minutes="$2" label="$3" tag="$4" line
  shift 4
  line=$(env -u MISTRA_CHEM_METHOD -u MISTRA_CHEM_METHOD_G -u MISTRA_CHEM_METHOD_A -u MISTRA_CHEM_METHOD_T -u MISTRA_CHEM_ATOL_REL -u MISTRA_CHEM_ATOL_REL_G \
         -u MISTRA_CHEM_ATOL_REL_A -u MISTRA_CHEM_ATOL_REL_T \
         timeout -k 10 "$LIMIT" oracle/model_run.sh "$BIN" "$case" "$minutes" "$TMP/${case}_$tag" MISTRA_COLUMN_DUMP="$TMP/${case}_$tag.bin" MISTRA_CHEM_HSTART_REUSE=0 "$@") ||
    { echo "$case, $label: $line"; return 1; }
  echo "$case, $minutes model minutes, $label: $line"
  compare "$case" "$label" "$TMP/${case}_plain.bin" "$TMP/${case}_$tag.bin"
}

study() {      # <case> <with the tot policies: 0 | 1>
  local case="$1" minutes
  minutes=$(python3 -c "import numpy as np; print(int(np.load('tests/golden/endstate_$case.npz')['minutes']))") || return 1
  run "$case" "$minutes" "plain" plain || return 1
  [ "$2" = 1 ] || return 0
  run "$case" "$minutes" "MISTRA_CHEM_ATOL_REL_T=1e-13" atol MISTRA_CHEM_ATOL_REL_T=1e-13 || return 1
  run "$case" "$minutes" "MISTRA_CHEM_METHOD_T=rodas3" rodas3 MISTRA_CHEM_METHOD_T=rodas3 || return 1
}

study Joyce2014_basecase 0 && study BTZ96 1
rc=$?
rm -rf "$TMP"
[ $rc -eq 0 ] || echo "the study stopped: a model run failed or ran into its time limit (status $rc)"
exit $rc
