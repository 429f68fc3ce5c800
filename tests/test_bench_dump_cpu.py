"""bench.py --dump-outputs: the writer of the last timed step's outputs (host side, no GPU)."""
import os

import numpy as np

import bench


def _files(d):
    return {f: np.load(os.path.join(d, f)) for f in sorted(os.listdir(d))}


def test_small_outputs_are_written_whole(tmp_path):
    ie = np.arange(2 * 4 * 8, dtype=np.float32).reshape(2, 4, 8) / 7
    ids = np.arange(30, dtype=np.int64).reshape(3, 10) * 4001            # token ids: exact in float32
    f64 = np.linspace(0, 1, 5)
    bench.dump_outputs(str(tmp_path / "o"), {"ie": ie, "decode_answers": ids, "x": f64})
    got = _files(str(tmp_path / "o"))
    assert sorted(got) == ["decode_answers.npy", "ie.npy", "x.npy"]
    assert got["ie.npy"].dtype == np.float32 and np.array_equal(got["ie.npy"], ie)
    assert got["decode_answers.npy"].dtype == np.float32 and np.array_equal(got["decode_answers.npy"], ids)
    assert got["x.npy"].dtype == np.float64 and np.array_equal(got["x.npy"], f64)


def test_large_outputs_are_cut_to_a_fixed_sample_within_the_limit(tmp_path):
    rng = np.random.default_rng(3)
    a, b = rng.standard_normal((300, 50)).astype(np.float32), rng.standard_normal(9000)
    limit = 40000                                                       # bytes; a + b hold 132,000
    for d in ("o1", "o2"):
        bench.dump_outputs(str(tmp_path / d), {"a": a, "b": b}, limit=limit)
    g1, g2 = _files(str(tmp_path / "o1")), _files(str(tmp_path / "o2"))
    assert sum(os.path.getsize(tmp_path / "o1" / f) for f in g1) <= limit
    for f, src in (("a.npy", a), ("b.npy", b)):
        assert g1[f].dtype == src.dtype and np.array_equal(g1[f], g2[f])           # the same sample every run
        assert g1[f].size >= 0.25 * src.size and np.isin(g1[f], src.reshape(-1)).all()
    # the sample is of positions, not of values: another array of the same shape is cut at the same elements
    bench.dump_outputs(str(tmp_path / "o3"), {"a": a * 2, "b": b}, limit=limit)
    assert np.array_equal(_files(str(tmp_path / "o3"))["a.npy"], g1["a.npy"] * 2)


def test_the_limit_is_64_mb():
    assert bench.DUMP_LIMIT <= 64 * 2**20
