"""GPU: the shared device-wide exclusive scan (csrc/lgcn_blockscan.hpp) at its seams, through lgcn_bool_square_bound:
cand_ptr must be numpy's exclusive cumsum of the per-row candidate counts, exactly, at one row, around a wave, around one
tile, across a few tiles, across several hundred (the add-back walks the totals in front of a block) and beyond 4096 tiles
(the totals get their own launch)."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

T = 2048          # the scan's tile: 256 threads x 8 items
SIZES = (1, 63, 64, 65, T - 1, T, T + 1, 2 * T + 1, 257 * T + 5, 4096 * T + 3)       # n + 1, the length of the scan


def random_csr(n, seed):
    """Row degrees 0..3; about one entry in eight points outside [0, n) (below, at n, or far above)."""
    rng = np.random.default_rng(seed)
    deg = rng.integers(0, 4, n)
    rowptr = np.concatenate([[0], np.cumsum(deg)]).astype(np.int32)
    nnz = int(rowptr[-1])
    col = rng.integers(0, max(n, 1), nnz)
    bad = rng.integers(0, 8, nnz) == 0
    col[bad] = rng.choice(np.array([-1, -7, n, n + 1, 2 ** 31 - 1]), int(bad.sum()))
    return rowptr, col.astype(np.int32)


def expected(rowptr, col, n):
    deg = np.diff(rowptr).astype(np.int64)
    ok = (col >= 0) & (col < n)
    per_entry = np.where(ok, deg[np.clip(col, 0, max(n - 1, 0))] if n else 0, 0)
    run = np.concatenate([[0], np.cumsum(per_entry)])
    counts = run[rowptr[1:]] - run[rowptr[:-1]]                     # candidates of every row
    return np.concatenate([[0], np.cumsum(counts)])                 # [n + 1]: exclusive, the total last


def test_tile_is_what_the_library_uses():
    import lanegcn_amd  # noqa: F401
    from lanegcn_amd import _lib as L
    lib = L.load()
    assert lib.lgcn_scan_ws_elems(T) == 2 and lib.lgcn_scan_ws_elems(T + 1) == 3


@pytest.mark.parametrize("n1", SIZES)
def test_cand_ptr_is_the_exclusive_cumsum(n1):
    import lanegcn_amd  # noqa: F401
    from lanegcn_amd import _lib as L
    from lanegcn_amd import ops
    lib = L.load()
    n = n1 - 1
    rowptr, col = random_csr(n, n1)
    want = expected(rowptr, col, n)
    assert want[-1] < 2 ** 31
    i32 = dict(dtype=torch.int32, device="cuda")
    d_rowptr = torch.from_numpy(rowptr).cuda()
    d_col = torch.from_numpy(col).cuda() if col.size else torch.zeros(1, **i32)
    cand_ptr = torch.full((n1,), -1, **i32)
    ws = torch.empty(lib.lgcn_scan_ws_elems(n1), **i32)
    L.check(lib.lgcn_bool_square_bound(ops._ptr(d_rowptr), ops._ptr(d_col), n, ops._ptr(cand_ptr), ops._ptr(ws), ops._stream()),
            "lgcn_bool_square_bound")
    got = cand_ptr.cpu().numpy()
    assert got.dtype == np.int32 and got.shape == (n1,)
    assert np.array_equal(got, want)
