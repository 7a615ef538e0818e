"""``bench.py`` as the driver runs it: a plain run times the step and prints
the result line without the ``--full`` extras, and ``--dump-outputs DIR``
writes the last timed step's outputs as float32 ``.npy`` files."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_plain_run_dumps_last_step_outputs(tmp_path):
    sys.path.insert(0, REPO)
    import bench
    from modules import engine as E
    env = {k: v for k, v in os.environ.items()
           if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
    p = subprocess.run([sys.executable, os.path.join(REPO, "bench.py"), "--gpus", "1", "--steps", "2", "--warmup", "1",
                        "--dump-outputs", str(tmp_path / "out")], env=env, cwd=REPO, capture_output=True, text=True,
                       timeout=240)
    assert p.returncode == 0, p.stderr[-2000:]
    lines = [json.loads(x) for x in p.stdout.splitlines() if x.startswith("{")]
    assert len(lines) == 1, p.stdout
    r = lines[0]
    assert r["steps"] == 2 and r["ms_per_step"] > 0 and r["unit"] == "segments/s" and r["higher_is_better"]
    assert r["value"] == pytest.approx(512 / (r["ms_per_step"] * 1e-3), rel=1e-3)
    # what takes runs of its own stays behind --full
    assert not {"roofline", "cpu_baseline", "parity", "recon_loss_rel_delta"} & set(r)
    cfg = bench.CONFIGS["c2"]
    got = {f[:-4]: np.load(tmp_path / "out" / f) for f in sorted(os.listdir(tmp_path / "out"))}
    assert sorted(got) == ["feats", "grads", "last_hidden", "params", "scalars"]
    assert sum(a.nbytes for a in got.values()) <= bench.DUMP_BUDGET_BYTES
    for name, a in got.items():
        assert a.dtype == np.float32 and np.isfinite(a).all(), name
    assert got["scalars"].shape == (E.N_SCALARS,) and got["scalars"][E.STATUS] == 0
    assert round(float(got["scalars"][E.LOSS]), 4) == r["config"]["final_loss"]
    assert got["params"].shape == got["grads"].shape and got["params"].ndim == 1
    assert got["last_hidden"].shape == (cfg["B"], 4 * cfg["H"]) and got["feats"].shape == (cfg["B"], cfg["D"])
    assert np.abs(got["grads"]).max() > 0
