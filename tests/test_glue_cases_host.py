"""CPU: the cases and models of tests/glue_cases.py are what they claim.  The launch constants are pinned to the source
text (a changed grid cap or rows-per-workgroup fails here instead of silently moving a seam), the numpy models agree with
plain loops, every position list lands where it says (float4 body, leftover, trip boundary, first and last thread), the
clean backgrounds are clean under the model, and the planted row lengths cover 0..9 and the long row."""
import os
import re

import numpy as np
import pytest

import glue_cases as G
from conftest import ROOT

CSRC = os.path.join(ROOT, "lanegcn-1_amd", "csrc")


def count(pattern, text):
    return len(re.findall(pattern, text))


# ------------------------------------------------------------------ the constants
def test_launch_constants_are_what_the_source_says():
    bwd = open(os.path.join(CSRC, "lgcn_bwd.hip")).read()
    # the detector: both entries size the grid alike, 256 threads, stride = the whole grid
    assert count(r"int64_t blocks = \(\(na \+ nb\) / 4 \+ %d\) / %d;" % (G.CF_F4_PER_BLOCK - 1, G.CF_F4_PER_BLOCK), bwd) == 2
    assert count(r"if \(blocks > %d\) blocks = %d;" % (G.CF_MAX_BLOCKS, G.CF_MAX_BLOCKS), bwd) == 2
    assert count(r"k_check_finite<(?:true|false)>, dim3\(\(unsigned\)blocks\), dim3\(%d\)" % G.CF_THREADS, bwd) == 2
    assert "stride = (int64_t)gridDim.x * blockDim.x, i0 = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;" in bwd
    assert "for (int64_t i = i0; i < na4 + nb4; i += stride)" in bwd and "if (i0 < ra + rb)" in bwd
    # the row kernels: 8 rows per workgroup of 256, at most 4096 workgroups
    assert count(r"int64_t blocks = \((?:n_rows|cap) \+ %d\) / %d;" % (G.ROWS_PER_BLOCK - 1, G.ROWS_PER_BLOCK), bwd) == 3
    assert count(r"if \(blocks > %d\) blocks = %d;" % (G.ROW_MAX_BLOCKS, G.ROW_MAX_BLOCKS), bwd) == 3
    assert count(r"blockIdx\.x \* %d \+ \(threadIdx\.x >> 5\); \w+ < \w+; \w+ \+= \(int64_t\)gridDim\.x \* %d\)"
                 % (G.ROWS_PER_BLOCK, G.ROWS_PER_BLOCK), bwd) == 3
    assert count(r"k_(?:gather_sum|pair_add|gather_rows), dim3\(\(unsigned\)blocks\), dim3\(256\)", bwd) == 3
    assert count(r"if \(n < 0 \|\| n > cap\) n = cap;", bwd) == 2
    assert G.C == 32 * 4 and count(r"\* 32 \+ l\]", bwd) >= 8
    index = open(os.path.join(CSRC, "lgcn_index.hip")).read()
    assert "k_widen, dim3(grid_for(cap, %d, %d)), dim3(%d)" % (G.WIDEN_THREADS, G.WIDEN_MAX_BLOCKS, G.WIDEN_THREADS) in index
    assert count(r"if \(n < 0 \|\| n > cap\) n = cap;", index[index.index("void k_widen"):index.index("grid_for(int64_t")]) == 1
    loss = open(os.path.join(CSRC, "lgcn_loss.hip")).read()
    for n in ("n_act", "n_agt"):
        assert "(%s < %d ? %s : %d)" % (n, G.LOSS_MAX_BLOCKS, n, G.LOSS_MAX_BLOCKS) in loss
    assert count(r"a = blockIdx\.x; a < p\.n_a[cg]t; a \+= gridDim\.x", loss) == 2
    # the exact comparisons of test_gpu_gather_glue.py rest on this
    assert "-ffp-contract=off" in open(os.path.join(CSRC, "Makefile")).read()


def test_grid_arithmetic():
    assert [G.cf_blocks(n) for n in (0, 1, 4095, 4096, 4099, 4100, 8388608, 8388612, 10485767)] == [1, 1, 1, 1, 1, 2, 2048, 2048, 2048]
    # 8388608 floats are 2048 * 1024 float4: the largest total whose grid the cap does not cut
    assert (8388608 // 4 + 1023) // 1024 == 2048 and (8388612 // 4 + 1023) // 1024 == 2049 and G.cf_blocks(8388608 - 4096) == 2047
    assert G.cf_stride(8388608) == 524288 and G.ROW_SPAN == 32768 and G.WIDEN_SPAN == 262144
    assert [G.row_blocks(n) for n in (1, 8, 9, 32767, 32768, 32769, 65537)] == [1, 1, 2, 4096, 4096, 4096, 4096]
    assert [G.row_trips(n) for n in G.SUM_ROWS] == [1, 1, 1, 1, 1, 1, 2, 3]
    assert [G.row_trips(n) for n in G.PAIR_CAPS] == [1, 1, 1, 1, 1, 1, 2]
    assert [G.widen_trips(n) for n in G.WIDEN_CAPS] == [1, 1, 1, 1, 1, 1, 2]
    assert G.LOSS_MAX_BLOCKS < 4097


# ------------------------------------------------------------------ the detector's model and cases
def finite_flag_loop(a, b, rows_a, row_a, rows_b, row_b):
    for x, r, w in ((a, rows_a, row_a), (b, rows_b, row_b)):
        if x is None:
            continue
        x = list(np.asarray(x, np.float32).reshape(-1))
        n_rows = len(x) // w
        if r is None or r >= n_rows:
            r = n_rows
        for row in range(max(r, 0)):
            for v in x[row * w:(row + 1) * w]:
                if v != v or v in (float("inf"), float("-inf")):
                    return True
    return False


def test_finite_flag_is_the_plain_loop():
    rng = np.random.default_rng(0)
    for name, bits in list(G.BAD.items()) + list(G.GOOD.items()):
        v = G.as_f32(bits)
        assert G.finite_flag(np.array([v])) == (name in G.BAD) == (not np.isfinite(v)), name
        assert v.view(np.uint32) == bits
    assert G.as_f32(G.GOOD["denormal"]) == np.float32(2.0 ** -149) and np.signbit(G.as_f32(G.GOOD["-0.0"]))
    assert not G.finite_flag(np.zeros(0, np.float32)) and not G.finite_flag(np.zeros(0, np.float32), None)
    seen = set()
    for _ in range(400):
        ra, wa, rb, wb = (int(v) for v in rng.integers(1, 6, 4))
        a, b = G.background(ra * wa, 3).reshape(ra, wa), G.background(rb * wb, 4).reshape(rb, wb)
        for x in (a, b):
            if rng.integers(0, 2):
                x.reshape(-1)[rng.integers(0, x.size)] = G.as_f32(list(G.BAD.values())[rng.integers(0, 5)])
        rows_a, rows_b = (None if rng.integers(0, 4) == 0 else int(rng.integers(-2, r + 3)) for r in (ra, rb))
        bb = None if rng.integers(0, 5) == 0 else b
        got = G.finite_flag(a, bb, rows_a, wa, rows_b, wb)
        assert got == finite_flag_loop(a, bb, rows_a, wa, rows_b, wb)
        seen.add((got, rows_a is None, bb is None))
    assert len(seen) == 8
    assert [G.clamp_rows(r, 11) for r in G.row_counts(11)] == [0, 0, 1, 10, 11, 11, 11]


def test_backgrounds_are_clean_and_hold_the_extremes():
    for n in list(G.TINY) + [4096, 4104, G.CAP_NA, G.CAP_TOTALS[1] - G.CAP_NA]:
        for seed in (1, 2):
            x = G.background(n, seed)
            assert x.dtype == np.float32 and x.shape == (n,) and not G.finite_flag(x) and not G.finite_flag(None, x)
            bits = x.view(np.uint32)
            if n >= 4:
                q = np.flatnonzero(bits == G.GOOD["+FLT_MAX"])
                assert any((bits[4 * (i // 4):4 * (i // 4) + 4] == G.GOOD["+FLT_MAX"]).all() for i in q)       # one whole float4
            if n >= 64:
                assert all((bits == v).sum() >= n // 40 for v in G.GOOD.values())
                assert np.abs(x[np.isfinite(x)]).min() == 0 and float(np.abs(x).max()) == float(np.finfo(np.float32).max)


@pytest.mark.parametrize("na", G.TINY)
def test_tiny_positions(na):
    for nb in G.TINY:
        pos = G.cf_positions(na, nb, every=True)
        # every float of both tensors, once
        assert sorted((w, i) for w, i, _ in pos) == [("a", i) for i in range(na)] + [("b", i) for i in range(nb)]
        assert G.cf_blocks(na + nb) == 1 and G.cf_trips(na, nb) == (1 if na // 4 + nb // 4 else 0)
        for w, i, tag in pos:
            n = na if w == "a" else nb
            assert (tag == "leftover") == (i >= 4 * (n // 4)) == (G.f4_thread(w, i, na, nb) is None)
    # nb = 6 r for odd r leaves 2 floats: the production shape of cls
    assert [t for w, _, t in G.cf_positions(0, 6, every=True) if w == "b"].count("leftover") == 2


@pytest.mark.parametrize("total", G.SEAM_TOTALS)
@pytest.mark.parametrize("how", ["a", "b", "ab"])
def test_seam_positions(total, how):
    na, nb = G.cf_split(total, how)
    assert na + nb == total and G.cf_blocks(total) == (1 if total < 4100 else 2)
    pos = G.cf_positions(na, nb)
    tags = [t for _, _, t in pos]
    left = (na % 4) + (nb % 4)
    assert tags.count("leftover") == left and tags.count("body_last") == (na >= 4) + (nb >= 4)
    assert (left > 0) == (total % 4 != 0 or how == "ab")
    threads = {G.f4_thread(w, i, na, nb) for w, i, t in pos if t != "leftover"}
    f4, stride = na // 4 + nb // 4, G.cf_stride(total)
    # one workgroup: four float4 per thread; two: the third trip holds at most two float4
    assert f4 in (1023, 1024, 1025, 1026) and G.cf_trips(na, nb) == (4 if stride == 256 else (2 if f4 <= 1024 else 3))
    assert (0, 0) in threads and ((f4 - 1) % stride, (f4 - 1) // stride) in threads            # the first and the last float4
    assert {trip for _, trip in threads} == set(range(G.cf_trips(na, nb)))
    if how == "ab":
        # b's first float4 follows a's 256 whole ones: thread 0's second trip of one workgroup, thread 0 of workgroup 1 of two
        assert na % 4 == 3 and na // 4 == 256 and ("a", 4 * 256 - 1, "body_last") in pos
        assert G.f4_thread("b", 0, na, nb) == ((0, 1) if stride == 256 else (256, 0))


@pytest.mark.parametrize("total", G.CAP_TOTALS)
def test_cap_positions(total):
    na, nb = G.CAP_NA, total - G.CAP_NA
    stride = G.cf_stride(total)
    assert G.cf_blocks(total) == G.CF_MAX_BLOCKS and stride == 524288
    # 8388608: four trips; 10485767: five whole trips and a sixth of one float4, a leftover of 3 (all of it a's)
    assert G.cf_trips(na, nb) == {8388608: 4, 10485767: 6}[total] and (na % 4, nb % 4) == {8388608: (3, 1), 10485767: (3, 0)}[total]
    assert 4 * total <= 42 * 10 ** 6
    pos = G.cf_positions(na, nb)
    assert len(pos) == len({(w, i) for w, i, _ in pos}) <= 48
    for w, n in (("a", na), ("b", nb)):
        mine = [(i, t) for ww, i, t in pos if ww == w]
        assert all(0 <= i < n for i, _ in mine)
        assert {0, 1, 3, 4, 4 * (n // 4) - 1} | set(range(4 * (n // 4), n)) <= {i for i, _ in mine}
        assert [t for _, t in mine].count("leftover") == n % 4
    seams = {}
    for w, i, t in pos:
        if t.startswith("trip"):
            thread, trip = G.f4_thread(w, i, na, nb)
            assert thread == {"trip_last": stride - 1, "trip_first": 0}[t]         # the last and the first thread of the grid
            seams.setdefault(t, set()).add(trip)
    trips = G.cf_trips(na, nb)
    f4 = na // 4 + nb // 4
    assert f4 % stride in (stride - 1, 1) and trips == (f4 - 1) // stride + 1
    assert seams["trip_first"] == set(range(1, trips)) and seams["trip_last"] == set(range(f4 // stride))
    # both tensors hold trip boundaries, and the join at na / 4 is not on one
    assert {w for w, _, t in pos if t.startswith("trip")} == {"a", "b"} and (na // 4) % stride not in (0, stride - 1)
    lanes = {i % 4 for _, i, t in pos if t.startswith("trip")}
    assert lanes == {0, 1, 2, 3}


def test_row_shapes():
    assert ((11, 360), (11, 6)) in G.ROW_SHAPES and ((37, 128), (11, 6)) in G.ROW_SHAPES
    assert {s[0][1] for s in G.ROW_SHAPES} >= {1, 2, 3, 5}
    assert any((sb[0] * sb[1]) % 4 == 2 for _, sb in G.ROW_SHAPES)                    # 11 rows of cls: 66 floats, 2 left over
    for sa, sb in G.ROW_SHAPES:
        for cap in (sa[0], sb[0]):
            assert len(set(G.row_counts(cap))) == 7 and {G.clamp_rows(r, cap) for r in G.row_counts(cap)} == {0, 1, cap - 1, cap}


# ------------------------------------------------------------------ the row kernels' models and cases
def gather_sum_loop(src, rowptr, col, dtype, backwards=False):
    out = np.zeros((len(rowptr) - 1, src.shape[1]), dtype)
    for n in range(len(rowptr) - 1):
        s = np.zeros(src.shape[1], dtype)
        for j in list(range(rowptr[n], rowptr[n + 1]))[::-1 if backwards else 1]:
            s = s + src[j if col is None else col[j]].astype(dtype)
        out[n] = s
    return out


@pytest.mark.parametrize("with_col", [False, True])
def test_gather_sum_models_are_the_plain_loops(with_col):
    for n_rows in (1, 9, 40):
        c = G.gather_sum_case(n_rows, with_col)
        for dtype in (np.float32, np.float64):
            got = G.gather_sum_seq(c["src"], c["rowptr"], c["col"], dtype)
            assert got.dtype == dtype and np.array_equal(got, gather_sum_loop(c["src"], c["rowptr"], c["col"], dtype))
        s64, a64 = G.gather_sum_f64(c["src"], c["rowptr"], c["col"])
        s32 = G.gather_sum_seq(c["src"], c["rowptr"], c["col"])
        k = np.diff(c["rowptr"]).reshape(-1, 1)
        assert (np.abs(s32 - s64) <= G.gamma(np.maximum(k - 1, 0)) * a64).all() and (a64 >= np.abs(s64)).all()
        if n_rows == 40:
            # the order matters at these magnitudes: walking the rows backwards gives other bits, within the same bound
            back = gather_sum_loop(c["src"], c["rowptr"], c["col"], np.float32, backwards=True)
            assert (back != s32).any() and (np.abs(back - s64) <= G.gamma(np.maximum(k - 1, 0)) * a64).all()
    assert G.gather_sum_seq(np.ones((1, G.C), np.float32), np.zeros(6, np.int32)).tolist() == np.zeros((5, G.C)).tolist()
    assert abs(G.gamma(999) - 999 * 2.0 ** -24) < 1e-8


@pytest.mark.parametrize("n_rows", G.SUM_ROWS)
def test_gather_sum_cases(n_rows):
    for with_col in (False, True):
        c = G.gather_sum_case(n_rows, with_col)
        lens = np.diff(c["rowptr"])
        assert len(lens) == n_rows and c["rowptr"].dtype == np.int32 and c["rowptr"][0] == 0 and lens.min() >= 0
        assert lens[-1] > 0                                                        # the last row of the last workgroup has work
        if n_rows >= 7:
            assert (lens == G.LONG_ROW).sum() == 1
        if n_rows >= 640:
            assert set(range(10)) <= set(lens.tolist()) and {k % 4 for k in lens.tolist()} == {0, 1, 2, 3}
        if n_rows > G.ROW_SPAN:
            assert lens[G.ROW_SPAN - 1] == 7 and lens[G.ROW_SPAN] == 6              # tail of 3 before, of 2 behind the trip boundary
        if c["col"] is None:
            assert len(c["src"]) == max(int(c["rowptr"][-1]), 1) and c["src"].nbytes <= 24 << 20
        else:
            assert len(c["src"]) == G.SRC_ROWS and len(c["col"]) == c["rowptr"][-1] and 0 <= c["col"].min() and c["col"].max() < G.SRC_ROWS
            if n_rows >= 7:
                assert {0, G.SRC_ROWS - 1} <= set(c["col"].tolist()) and len(np.unique(c["col"])) < len(c["col"])


def test_small_lengths_case():
    assert sorted(G.SMALL_LENS) == list(range(10)) + [G.LONG_ROW]
    for with_col in (False, True):
        c = G.gather_sum_case(len(G.SMALL_LENS), with_col, G.SMALL_LENS)
        assert np.diff(c["rowptr"]).tolist() == list(G.SMALL_LENS) and G.row_blocks(len(G.SMALL_LENS)) == 2


def test_pair_gather_widen_models_are_the_plain_loops():
    for cap in (1, 7, 9):
        p = G.pair_case(cap)
        x = G.widen_case(cap)
        src = G.features(np.random.default_rng(cap), 41)
        idx = G.index_case(cap, 41, 5)
        for n in G.device_counts(cap) + [cap + 100, -(2 ** 31)]:
            m = G.dev_count(n, cap)
            assert m == (n if 0 <= n <= cap else cap)
            base = G.sentinel_rows(cap + G.GUARD_ROWS)
            want = base.copy()
            for i in range(m):
                for ch in range(G.C):
                    want[i, ch] = np.float32(np.float32(p["c"][i, ch] + p["U"][p["hi"][i], ch]) + p["V"][p["wi"][i], ch])
            got = G.pair_add(p["c"], p["U"], p["hi"], p["V"], p["wi"], n, cap, base)
            assert np.array_equal(got.view(np.uint32), want.view(np.uint32)) and (base.view(np.uint32) == G.SENTINEL).all()
            want = base.copy()
            for i in range(m):
                want[i] = src[idx[i]]
            assert np.array_equal(G.gather_rows(src, idx, n, cap, base).view(np.uint32), want.view(np.uint32))
            base64 = np.full(cap + G.GUARD_ROWS, G.SENTINEL64, np.int64)
            want64 = np.array([int(v) for v in x[:m]] + [G.SENTINEL64] * (cap + G.GUARD_ROWS - m), np.int64)
            assert np.array_equal(G.widen(x, n, cap, base64), want64)
    assert np.isnan(G.sentinel_rows(2)).all()


@pytest.mark.parametrize("cap", G.PAIR_CAPS)
def test_pair_and_index_cases(cap):
    p = G.pair_case(cap)
    assert p["c"].shape == (cap, G.C) and p["hi"].dtype == p["wi"].dtype == np.int32
    for idx, n_src in ((p["hi"], len(p["U"])), (p["wi"], len(p["V"]))):
        assert len(idx) == cap and 0 <= idx.min() and idx.max() < n_src and idx[-1] == n_src - 1
        if cap >= 7:
            assert idx[0] == 0
        if cap >= n_src:
            assert len(np.unique(idx)) < cap                                       # repeats
        if cap > n_src:
            assert len(np.unique(idx)) == n_src
    assert len(G.device_counts(cap)) == (4 if cap == 1 else 7) and {-1, 0, cap, cap + 1} <= set(G.device_counts(cap))


@pytest.mark.parametrize("cap", G.WIDEN_CAPS)
def test_widen_cases(cap):
    x = G.widen_case(cap)
    assert x.dtype == np.int32 and len(x) == cap and x[-1] == -2 ** 31 and (x < 0).any()
    if cap > 2:
        assert x[0] == -1 and x.max() == 2 ** 31 - 1 and 0.3 < (x < 0).mean() < 0.7
    assert (G.widen(x, cap, cap, np.zeros(cap, np.int64)) == x.astype(np.int64)).all()
