"""bench.py's plain run on the GPU (-m gpu): a fresh process times exactly --steps passes, leaves the --full objects null, and
--dump-outputs writes what its last timed step returned — bit for bit what one chem.integrate call gives for the same cells."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import REPO

pytestmark = pytest.mark.gpu


def test_plain_bench_run_dumps_what_the_timed_path_computed(tmp_path):
    import torch
    from mistra_amd import chem
    from mistra_amd.workload import make_batch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    cells = 64
    out = tmp_path / "dump"
    cmd = [sys.executable, os.path.join(REPO, "bench.py"), "--gpus", "1", "--mech", "tot", "--cells-per-gpu", str(cells), "--steps", "2",
           "--warmup", "1", "--dump-outputs", str(out)]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    line = json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][-1])
    assert line["steps"] == 2 and line["warmup"] == 1 and line["ms_per_step"] > 0 and line["config"]["failed_cells"] == 0
    assert line["parity"] is None and line["extra"] is None and "cpu_baseline" not in line
    got = {n: np.load(out / (n + ".npy")) for n in ("var_out", "ierr", "stats", "cells")}
    assert all(a.dtype == np.float64 for a in got.values())
    assert np.array_equal(got["cells"], np.arange(cells))
    chem.init(0)
    var, fix, rconst = make_batch("tot", 0, cells, torch.device("cuda", 0))
    res = chem.integrate("tot", var, fix, rconst)
    torch.cuda.synchronize()
    assert np.array_equal(got["var_out"], res.var.cpu().numpy())
    assert np.array_equal(got["ierr"], res.ierr.cpu().numpy()) and np.array_equal(got["stats"], res.stats.cpu().numpy())
