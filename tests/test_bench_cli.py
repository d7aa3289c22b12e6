"""The benchmark's command line: ``--steps`` is the number of timed steps, a plain run leaves out
what only ``--full`` measures, and ``--dump-outputs`` writes the last step's arrays."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def test_schedule_split_sums_to_steps():
    import bench
    for k in range(1, 400):
        n = bench.schedule_split(k)
        assert sum(n) == k and min(n) >= 0, (k, n)
        if k >= 3:
            assert min(n) >= 1, (k, n)
    assert bench.schedule_split(1344) == (256, 64, 1024)


@pytest.mark.gpu
def test_plain_run_times_the_steps_asked_for_and_dumps_outputs(tmp_path):
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    out = tmp_path / "dump"
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "4", "--warmup", "3",
                        "--dump-outputs", str(out)], cwd=ROOT, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    line = json.loads(r.stdout.strip().splitlines()[-1])
    assert line["steps"] == 4 and line["config"]["schedule_mix"] == [1, 1, 2]
    assert line["ms_per_step"] > 0 and line["value"] == pytest.approx(1e3 / line["ms_per_step"], rel=1e-3)
    assert line["ensemble9"] is None and line["finite"]              # the ensemble is measured by --full only
    arrs = {f[:-4]: np.load(out / f) for f in sorted(os.listdir(out))}
    assert set(arrs) == {"params", "history_train", "history_eval"}
    assert all(a.dtype == np.float32 and np.isfinite(a).all() for a in arrs.values())
    assert arrs["params"].shape == (1, 12233)
    assert arrs["history_train"].shape[:2] == (1, 4) and arrs["history_eval"].shape[:2] == (1, 3)
    assert arrs["history_train"][0, :, 0].tolist() == [1, 2, 3, 3]   # the phase of each timed step
    assert sum(a.nbytes for a in arrs.values()) < 64 << 20
