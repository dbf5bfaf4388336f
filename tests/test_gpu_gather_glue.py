"""GPU: lgcn_gather_sum, lgcn_pair_add, lgcn_gather_rows (csrc/lgcn_bwd.hip) and lgcn_widen_i32 (csrc/lgcn_index.hip)
against the plain numpy models of tests/glue_cases.py (pinned by test_glue_cases_host.py), BIT FOR BIT: each kernel adds in
one documented order and the library is built with -ffp-contract=off, so the fp32 model reproduces the bits.  The C entries
are called directly with a prefilled `out`: rows from the device count to the capacity, and guard rows behind it, must keep
their sentinel.

Seams: 8 rows per workgroup and at most 4096 workgroups (row 32768 opens a second trip, row 65536 a third); the 4-way
unrolled walk of lgcn_gather_sum with tails of 0..3, with and without col; device counts of 0, 1, cap - 1, cap and the three
that the kernels read as cap (cap + 1, -1, -cap); 1024 workgroups of 256 threads for lgcn_widen_i32.

lgcn_gather_sum is also held to float64: |got - sum64| <= gamma_(k-1) sum|x| per element, gamma_n = n u / (1 - n u),
u = 2^-24, k the row's length -- the bound of k - 1 fp32 additions in ANY order.  Exact equality failing with the bound
holding would mean that the kernel's order is not the documented one.  Measured on an MI355X: equal bit for bit in every
case; the row of 1000 is within 5.0e-7 sum|x| of float64 (bound 5.95e-5), a row of 9 within 2.7e-7 (bound 4.8e-7), and rows
of two reach 1.000 of their bound (one addition rounded at a half ulp: gamma_1 is attained, not loose)."""
import numpy as np
import pytest
import torch

import glue_cases as G

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    import lanegcn_amd  # noqa: F401
    from lanegcn_amd import _lib as L
    from lanegcn_amd import ops
    return L.load(), L, ops


def cuda(x):
    return torch.from_numpy(np.ascontiguousarray(x)).cuda()


def bits(t):
    return t.cpu().numpy().view(np.uint32)


def same_bits(got, want):
    return np.array_equal(got.view(np.uint32), want.view(np.uint32))


def count(n):
    return torch.tensor([n], dtype=torch.int32, device="cuda")


# ------------------------------------------------------------------ lgcn_gather_sum
def run_gather_sum(dev, case, n_rows):
    lib, L, ops = dev
    src, rowptr = cuda(case["src"]), cuda(case["rowptr"])
    col = None if case["col"] is None else cuda(case["col"])
    out = cuda(G.sentinel_rows(n_rows + G.GUARD_ROWS))
    L.check(lib.lgcn_gather_sum(src.data_ptr(), rowptr.data_ptr(), None if col is None else col.data_ptr(), n_rows, out.data_ptr(),
                                ops._stream()), "lgcn_gather_sum")
    got = out.cpu().numpy()
    assert (got[n_rows:].view(np.uint32) == G.SENTINEL).all()                      # the guard rows
    assert same_bits(src.cpu().numpy(), case["src"])
    return got[:n_rows], (src, rowptr, col)


def check_gather_sum(dev, case, n_rows, what):
    got, on_dev = run_gather_sum(dev, case, n_rows)
    want = G.gather_sum_seq(case["src"], case["rowptr"], case["col"])
    s64, a64 = G.gather_sum_f64(case["src"], case["rowptr"], case["col"])
    k = np.diff(case["rowptr"]).reshape(-1, 1)
    bound = G.gamma(np.maximum(k - 1, 0)) * a64
    err = np.abs(got.astype(np.float64) - s64)
    ratio = float((err[bound > 0] / bound[bound > 0]).max()) if (bound > 0).any() else 0.0
    at = int(np.argmax((err / np.maximum(a64, 1e-300)).max(1)))
    print("%s: worst |got - sum64| / (gamma_(k-1) sum|x|) = %.3f; worst |got - sum64| / sum|x| = %.2e in a row of %d (bound %.2e); "
          "%d of %d rows differ from the sequential fp32 sum"
          % (what, ratio, float((err[at] / np.maximum(a64[at], 1e-300)).max()), int(k[at, 0]), G.gamma(max(int(k[at, 0]) - 1, 0)),
             int((got.view(np.uint32) != want.view(np.uint32)).any(1).sum()), n_rows))
    assert (err <= bound).all(), what                                              # float64: any order of the additions
    assert same_bits(got, want), what                                              # fp32: THE order, left to right
    ops = dev[2]                                                                   # the wrapper every user calls
    assert torch.equal(ops.gather_sum(on_dev[0], on_dev[1], on_dev[2], n_rows).view(torch.int32), cuda(want).view(torch.int32))


@pytest.mark.parametrize("with_col", [False, True], ids=["segments", "col"])
@pytest.mark.parametrize("n_rows", G.SUM_ROWS)
def test_gather_sum(dev, n_rows, with_col):
    check_gather_sum(dev, G.gather_sum_case(n_rows, with_col), n_rows, "gather_sum %d rows %s" % (n_rows, "col" if with_col else "segments"))


@pytest.mark.parametrize("with_col", [False, True], ids=["segments", "col"])
def test_gather_sum_every_tail_length(dev, with_col):
    n = len(G.SMALL_LENS)
    check_gather_sum(dev, G.gather_sum_case(n, with_col, G.SMALL_LENS), n, "gather_sum lengths 0..9 and %d" % G.LONG_ROW)


@pytest.mark.parametrize("n_rows", [9, G.ROW_SPAN + 1])
def test_gather_sum_of_empty_rows_is_zero(dev, n_rows):
    for with_col in (False, True):
        case = G.gather_sum_case(n_rows, with_col, np.zeros(n_rows, np.int64))
        assert case["rowptr"].max() == 0
        got, _ = run_gather_sum(dev, case, n_rows)
        assert (got.view(np.uint32) == 0).all()                                    # +0.0, every element


def test_gather_sum_of_no_rows_launches_nothing(dev):
    lib, L, ops = dev
    out = cuda(G.sentinel_rows(G.GUARD_ROWS))
    assert lib.lgcn_gather_sum(None, None, None, 0, out.data_ptr(), ops._stream()) == 0
    assert (bits(out) == G.SENTINEL).all()
    assert tuple(ops.gather_sum(torch.zeros(1, G.C, device="cuda"), torch.zeros(1, dtype=torch.int32, device="cuda"), None, 0).shape) == (0, G.C)


# ------------------------------------------------------------------ lgcn_pair_add, lgcn_gather_rows
@pytest.mark.parametrize("cap", G.PAIR_CAPS)
def test_pair_add(dev, cap):
    lib, L, ops = dev
    p = G.pair_case(cap)
    d = {k: cuda(v) for k, v in p.items()}
    base = G.sentinel_rows(cap + G.GUARD_ROWS)
    for n in G.device_counts(cap):
        out, n_dev = cuda(base), count(n)
        L.check(lib.lgcn_pair_add(d["c"].data_ptr(), d["U"].data_ptr(), d["hi"].data_ptr(), d["V"].data_ptr(), d["wi"].data_ptr(),
                                  n_dev.data_ptr(), cap, out.data_ptr(), ops._stream()), "lgcn_pair_add")
        want = G.pair_add(p["c"], p["U"], p["hi"], p["V"], p["wi"], n, cap, base)
        assert (want[G.dev_count(n, cap):].view(np.uint32) == G.SENTINEL).all()
        assert same_bits(out.cpu().numpy(), want), (cap, n)
    got = ops.pair_add(d["c"], d["U"], d["hi"], d["V"], d["wi"], count(cap), cap)
    assert same_bits(got.cpu().numpy(), G.pair_add(p["c"], p["U"], p["hi"], p["V"], p["wi"], cap, cap, base)[:cap])
    assert all(same_bits(d[k].cpu().numpy(), p[k]) for k in ("c", "U", "V"))


@pytest.mark.parametrize("cap", [9, G.ROW_SPAN + 1])
def test_pair_add_with_a_zero_row_for_v(dev, cap):
    """LanePooling's use: V is one row of zeros addressed by an all-zero index, so out = (c + U[hi]) + 0."""
    lib, L, ops = dev
    p = G.pair_case(cap)
    zero_row, zero_idx = np.zeros((1, G.C), np.float32), np.zeros(cap, np.int32)
    base = G.sentinel_rows(cap + G.GUARD_ROWS)
    c, U, hi, V, wi = (cuda(x) for x in (p["c"], p["U"], p["hi"], zero_row, zero_idx))
    for n in (cap, cap - 2):
        out, n_dev = cuda(base), count(n)
        L.check(lib.lgcn_pair_add(c.data_ptr(), U.data_ptr(), hi.data_ptr(), V.data_ptr(), wi.data_ptr(), n_dev.data_ptr(), cap,
                                  out.data_ptr(), ops._stream()), "lgcn_pair_add")
        want = G.pair_add(p["c"], p["U"], p["hi"], zero_row, zero_idx, n, cap, base)
        assert same_bits(want[:n], p["c"][:n] + p["U"][p["hi"][:n]])
        assert same_bits(out.cpu().numpy(), want), (cap, n)


@pytest.mark.parametrize("cap", G.PAIR_CAPS)
def test_gather_rows(dev, cap):
    lib, L, ops = dev
    rng = np.random.default_rng(cap)
    src, idx = G.features(rng, 41), G.index_case(cap, 41, cap + 2)
    src[5].view(np.uint32)[:] = np.arange(G.C, dtype=np.uint32) + 0x7f800001       # NaN payloads and denormals are copied as they are
    src[6].view(np.uint32)[:] = np.arange(G.C, dtype=np.uint32) + 1
    idx[cap // 3] = 5 + (cap & 1)
    d_src, d_idx = cuda(src), cuda(idx)
    base = G.sentinel_rows(cap + G.GUARD_ROWS)
    for n in G.device_counts(cap):
        out, n_dev = cuda(base), count(n)
        L.check(lib.lgcn_gather_rows(d_src.data_ptr(), d_idx.data_ptr(), n_dev.data_ptr(), cap, out.data_ptr(), ops._stream()),
                "lgcn_gather_rows")
        assert same_bits(out.cpu().numpy(), G.gather_rows(src, idx, n, cap, base)), (cap, n)
    assert same_bits(ops.gather_rows(d_src, d_idx, count(cap), cap).cpu().numpy(), src[idx])


# ------------------------------------------------------------------ lgcn_widen_i32
@pytest.mark.parametrize("cap", G.WIDEN_CAPS)
def test_widen_i32(dev, cap):
    lib, L, ops = dev
    x = G.widen_case(cap)
    d_x = cuda(x)
    base = np.full(cap + G.GUARD_ROWS, G.SENTINEL64, np.int64)
    for n in G.device_counts(cap):
        out, n_dev = cuda(base), count(n)
        L.check(lib.lgcn_widen_i32(d_x.data_ptr(), n_dev.data_ptr(), cap, out.data_ptr(), ops._stream()), "lgcn_widen_i32")
        got, want = out.cpu().numpy(), G.widen(x, n, cap, base)
        assert got.dtype == np.int64 and np.array_equal(got, want), (cap, n)
        m = G.dev_count(n, cap)
        assert (want[:m] < 0).any() or m < 2                                        # sign extension is seen
    assert np.array_equal(d_x.cpu().numpy(), x)
