"""bench.py's command line and the row sample of --dump-outputs (no GPU needed)."""
import sys

import numpy as np

import bench


def test_full_and_dump_outputs_are_off_by_default(monkeypatch):
    monkeypatch.setattr(sys, "argv", ["bench.py", "--gpus", "1", "--steps", "3", "--warmup", "2"])
    a = bench.parse()
    assert (a.steps, a.warmup, a.full, a.dump_outputs) == (3, 2, False, None)
    monkeypatch.setattr(sys, "argv", ["bench.py", "--full", "--dump-outputs", "out"])
    a = bench.parse()
    assert a.full and a.dump_outputs == "out"


def test_dump_sample_is_fixed_sorted_and_capped():
    col = np.array([7, 3, 3, 9, 0, 7, 12, 5], np.int32)
    whole = bench.dump_ids(col, 6, np.random.default_rng(bench.DUMP_SEED))
    assert whole.tolist() == [0, 3, 5, 7, 9, 12] and whole.dtype == np.int32
    one = bench.dump_ids(col, 4, np.random.default_rng(bench.DUMP_SEED))
    two = bench.dump_ids(col, 4, np.random.default_rng(bench.DUMP_SEED))
    assert one.tolist() == two.tolist() and len(one) == 4
    assert sorted(set(one.tolist())) == one.tolist() and set(one.tolist()) <= set(whole.tolist())


def test_both_dumped_sides_fit_the_64_mb_limit():
    for k, itemsize in ((64, 4), (128, 4), (256, 4), (128, 8), (256, 8)):
        rows = bench.DUMP_SIDE_BYTES // (k * itemsize)
        assert 2 * rows * (k * itemsize + 8) <= 64e6  # factor rows plus their float64 ids, both sides
