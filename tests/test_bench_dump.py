"""CPU: bench.py's --dump-outputs writer -- float32 stays float32, everything else becomes float64, and above 64 MB in all the
same fixed, seeded sample of states is taken from every array (its indices beside them)."""
import os

import numpy as np

import bench


def _load(d):
    return {f[:-4]: np.load(os.path.join(d, f)) for f in os.listdir(d)}


def test_small_outputs_are_written_whole(tmp_path):
    rng = np.random.default_rng(0)
    arrays = {"tau": rng.normal(size=(12, 100)), "f32": rng.normal(size=(3, 100)).astype(np.float32),
              "status": np.arange(100, dtype=np.int32)}
    bench.dump_outputs(str(tmp_path / "d"), arrays)
    got = _load(tmp_path / "d")
    assert set(got) == set(arrays)
    assert got["tau"].dtype == np.float64 and np.array_equal(got["tau"], arrays["tau"])
    assert got["f32"].dtype == np.float32 and np.array_equal(got["f32"], arrays["f32"])
    assert got["status"].dtype == np.float64 and np.array_equal(got["status"], np.arange(100))


def test_large_outputs_are_a_seeded_sample_of_states(tmp_path):
    n = 40000
    arrays = {"M": np.arange(171 * n, dtype=np.float64).reshape(171, n), "Jc": np.ones((216, n)), "iters": np.arange(n, dtype=np.int32)}
    assert sum(a.nbytes for a in arrays.values()) > bench.DUMP_MAX_BYTES
    for tag in ("a", "b"):
        bench.dump_outputs(str(tmp_path / tag), arrays)
    a, b = _load(tmp_path / "a"), _load(tmp_path / "b")
    assert set(a) == set(arrays) | {"state_index"}
    assert sum(x.nbytes for x in a.values()) <= bench.DUMP_MAX_BYTES
    idx = a["state_index"].astype(np.int64)
    assert len(idx) > 1000 and np.all(np.diff(idx) > 0) and idx[-1] < n
    assert np.array_equal(a["iters"], idx) and np.array_equal(a["M"], arrays["M"][:, idx])
    for k in a:
        assert np.array_equal(a[k], b[k]), k
