"""CPU: bench.py --dump-outputs writes float32 / float64 .npy files within its byte budget, the same rows every run."""
import importlib.util
import os

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bench():
    spec = importlib.util.spec_from_file_location("bench_under_test", os.path.join(ROOT, "bench.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)                     # defines functions only; main() is not run
    return mod


def test_dump_outputs_dtypes_and_budget(tmp_path):
    b = _bench()
    g = torch.Generator().manual_seed(0)
    outs = {"nodes": torch.randn(1000, 16, generator=g), "actors": torch.randn(100, 16, generator=g).half(),
            "exact": torch.randn(50, 4, generator=g, dtype=torch.float64)}
    assert b.dump_outputs(outs, str(tmp_path / "all")) == ["actors", "exact", "nodes"]
    got = {k: np.load(tmp_path / "all" / ("%s.npy" % k)) for k in outs}
    assert got["nodes"].dtype == np.float32 and np.array_equal(got["nodes"], outs["nodes"].numpy())
    assert got["actors"].dtype == np.float32 and np.array_equal(got["actors"], outs["actors"].float().numpy())
    assert got["exact"].dtype == np.float64 and np.array_equal(got["exact"], outs["exact"].numpy())
    # over budget: a fixed sample of rows of each array, in row order, the same on every call
    budget = 20000
    for run in ("a", "b"):
        b.dump_outputs(outs, str(tmp_path / run), budget=budget)
    total = 0
    for k, v in outs.items():
        a, a2 = np.load(tmp_path / "a" / ("%s.npy" % k)), np.load(tmp_path / "b" / ("%s.npy" % k))
        assert np.array_equal(a, a2) and a.shape[1:] == tuple(v.shape[1:]) and 1 <= len(a) < v.shape[0]
        full = v.double().numpy()
        rows = [int(np.flatnonzero((full == r).all(1))[0]) for r in a.astype(np.float64)]
        assert rows == sorted(rows)
        total += a.nbytes
    assert total <= budget
