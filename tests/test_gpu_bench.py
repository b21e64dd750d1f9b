"""bench.py end to end on a small NFLX-shaped synthetic: a plain run carries the contract fields and
leaves the legs of --full out, --steps sets the timed epochs, and --dump-outputs writes the factors
the last timed epoch left -- bit for bit those of an in-process fit of warmup + steps epochs (the
systolic sweep has fixed cells and no atomics, so a fit repeats exactly)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import mfhip
from mfhip import _lib as L
from mfhip import synth

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SCALE, STEPS, WARMUP = 0.02, 2, 1


def test_plain_run_line_and_dumped_factors(tmp_path):
    out = tmp_path / "dump"
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", str(STEPS),
                        "--warmup", str(WARMUP), "--scale", str(SCALE), "--dump-outputs", str(out)],
                       capture_output=True, text=True, timeout=120, cwd=str(tmp_path))
    assert r.returncode == 0, r.stderr[-3000:]
    lines = r.stdout.strip().splitlines()
    assert len(lines) == 1, r.stdout[-2000:]
    d = json.loads(lines[0])
    assert d["unit"] == "updates/s" and d["higher_is_better"] is True and d["dtype"] == "f32"
    assert (d["steps"], d["warmup"], d["n_gpus"], d["full"]) == (STEPS, WARMUP, 1, False)
    assert d["ms_per_step"] > 0
    # value is the timed epochs' updates over their wall time: every epoch updates the training split
    # once (ms_per_step is rounded to 1 us, under 0.5% of an epoch of 8 launches)
    assert d["value"] == pytest.approx(d["config"]["train_ratings"] / (d["ms_per_step"] / 1e3), rel=5e-3)
    for leg in ("rmse", "roofline", "cpu_baseline", "online", "deterministic", "ml20m"):
        assert d[leg] is None, leg

    nu, ni, nr, k, nb = synth.CONFIGS["NFLX"]
    (tu, ti, tr), _ = synth.generate(int(nu * SCALE), int(ni * SCALE), int(nr * SCALE)).split()
    p = L.default_params()
    p.num_factors, p.num_blocks, p.seed, p.has_seed = k, nb, 0, 1
    p.iterations = WARMUP + STEPS
    p.mode = L.MODE_FAST_F32
    assert sorted(os.listdir(out)) == ["item_factors.npy", "item_ids.npy", "user_factors.npy", "user_ids.npy"]
    with mfhip.Context(p) as ctx:
        ctx.prepare(tu, ti, tr)
        ctx.run((WARMUP + STEPS) * nb)
        for side, name, col in ((0, "user", tu), (1, "item", ti)):
            ids = np.load(out / f"{name}_ids.npy")
            vecs = np.load(out / f"{name}_factors.npy")
            assert ids.dtype == np.float64 and vecs.dtype == np.float32
            assert ids.tolist() == np.unique(col).tolist()
            assert vecs.shape == (len(ids), k) and np.isfinite(vecs).all()
            want, found = ctx.lookup(side, ids.astype(np.int32))
            assert found.all()
            assert np.array_equal(vecs, want.astype(np.float32)), name
