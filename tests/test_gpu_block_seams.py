"""GPU: the users of csrc/lgcn_blockscan.hpp at their workgroup seams (tests/seam_cases.py; proven on the host by
tests/test_seam_cases_host.py): the pair search's 4096-row chunks and 1024-scene trips, the CSR plan's 4096-key scan tiles
up to the 1024th, and the batched dilation and left / right compactions past block 256, where block_base<256> takes its
second trip.  Every output is an integer array: each is compared element for element, dtype included, with a host model
that never calls the library, and no row is left out of a comparison.

What each case would show if a prefix were dropped:
  pairs, chunk 1        rowptr[4096 ..] loses the pairs of rows 0 .. 4095 (T4096: rowptr[T] = P alone would read 0)
  pairs, scene 1024     hi / wi of every scene from 1024 on lose the rows / context rows numbered before them
  CSR plan, tile 1      rowptr[4096 ..] loses tile 0's edges and col is filled over tile 0's rows
  block 256             out_rowptr / the compaction offset of item 65 536 on loses blocks 0 .. 255: pre_off / left_off
                        of the scenes behind it and every u / v written through them differ"""
import numpy as np
import pytest
import torch

import lanegcn_amd  # noqa: F401
import seam_cases as S

pytestmark = pytest.mark.gpu


def cuda(x):
    return torch.from_numpy(np.ascontiguousarray(x)).cuda()


def same(got, want, what):
    got = got.cpu().numpy() if torch.is_tensor(got) else np.asarray(got)
    assert got.dtype == want.dtype and got.shape == want.shape, (what, got.dtype, want.dtype, got.shape, want.shape)
    bad = np.flatnonzero(got != want)
    assert len(bad) == 0, (what, "first difference at", int(bad[0]), int(got[bad[0]]), int(want[bad[0]]), "of", len(bad))


# ------------------------------------------------------------------ 1. pair search
def search_of(case):
    agt, a_off, ctx, c_off, cap = S.pair_flat(case)
    return (cuda(agt), cuda(a_off), cuda(ctx), cuda(c_off), S.PAIR_TH, cap)


def check_pairs(ps, want, what):
    hi_w, wi_w, rp_w = want
    assert ps.count() == len(hi_w), what
    hi, wi = ps.hi_wi_long()
    same(hi, hi_w, what + " hi")
    same(wi, wi_w, what + " wi")
    same(ps.hi[:len(hi_w)], hi_w.astype(np.int32), what + " hi32")
    same(ps.n_pairs, np.asarray([len(hi_w)], np.int32), what + " n_pairs")
    same(ps.rowptr, rp_w, what + " rowptr")


PAIR_CASES = [("T", T) for T in sorted(S.PAIR_ROWS)] + [("B", B) for B in S.PAIR_SCENE_COUNTS]


def pair_case(kind, n):
    return S.pair_case_rows(n) if kind == "T" else S.pair_case_scenes(n)


@pytest.mark.parametrize("kind,n", PAIR_CASES)
def test_pairs_build_at_the_chunk_and_scene_seams(kind, n):
    from lanegcn_amd import ops
    case = pair_case(kind, n)
    search = search_of(case)
    for legacy in (True, False):
        check_pairs(ops.pairs_build(*search, legacy), S.pair_expected(case, legacy), "%s%d legacy=%s" % (kind, n, legacy))


def test_pairs_build_multi_three_jobs():
    from lanegcn_amd import ops
    cases = [S.pair_case_rows(4096), S.pair_case_scenes(1025), S.pair_case_rows(8193)]
    for legacy in (True, False):
        got = ops.pairs_build_multi([search_of(c) for c in cases], legacy)
        for c, ps in zip(cases, got):
            check_pairs(ps, S.pair_expected(c, legacy), "multi %s legacy=%s" % (c["name"], legacy))


def index_inputs(us, vs):
    """idx_local, seg_off, seg_base and rel_slices of ops.index_build: one segment per run, local = global."""
    runs = [t for pair in zip(us, vs) for t in pair]
    offs = S.csum([len(t) for t in runs])
    rel = [((int(offs[2 * r]), int(offs[2 * r + 1])), (int(offs[2 * r + 1]), int(offs[2 * r + 2]))) for r in range(len(us))]
    return cuda(np.concatenate(runs)), cuda(offs[:-1].copy()), torch.zeros(len(runs), dtype=torch.int64, device="cuda"), rel


def test_pairs_ride_behind_the_edge_workgroups():
    """index_build with three pair jobs, the middle one without a row: job_blocks = [0, a, a, b]."""
    from lanegcn_amd import ops
    n_nodes, n_rel = 4096, 3
    us, vs = S.csr_case(n_nodes, n_rel)
    rowptr, col = S.csr_expected(us, vs, n_nodes, n_rel)
    cases = [S.pair_case_scenes(1024), S.pair_case_rows(4097)]
    empty = (torch.zeros((0, 2), device="cuda"), torch.zeros(4, dtype=torch.int32, device="cuda"),
             cuda(np.ones((5, 2), np.float32)), cuda(np.asarray([0, 2, 2, 5], np.int32)), S.PAIR_TH, 8)
    searches = [search_of(cases[0]), empty, search_of(cases[1])]
    idx, seg_off, seg_base, rel = index_inputs(us, vs)
    for legacy in (True, False):
        plan, pairs = ops.index_build(idx, seg_off, seg_base, rel, n_nodes, searches, legacy)
        same(plan.rowptr, rowptr, "rowptr")
        same(plan.col[:len(col)], col, "col")
        check_pairs(pairs[0], S.pair_expected(cases[0], legacy), "job 0 legacy=%s" % legacy)
        check_pairs(pairs[2], S.pair_expected(cases[1], legacy), "job 2 legacy=%s" % legacy)
        assert pairs[1].count() == 0
        same(pairs[1].rowptr, np.zeros(1, np.int32), "job 1 rowptr")


# ------------------------------------------------------------------ 2. CSR plan
def check_plan(us, vs, n_nodes, n_rel):
    from lanegcn_amd import ops
    rowptr, col = S.csr_expected(us, vs, n_nodes, n_rel)
    n_edges = sum(len(u) for u in us)
    assert ops.index_fused_ok(n_nodes, n_rel, n_edges)
    idx, seg_off, seg_base, rel = index_inputs(us, vs)
    cnt = ops.index_counters(n_nodes, n_rel, idx.device)
    for rep in range(2):                                   # the counters come back to zero: the second run starts clean
        plan, _ = ops.index_build(idx, seg_off, seg_base, rel, n_nodes, cnt=cnt)
        same(plan.rowptr, rowptr, "index_build rowptr, run %d" % rep)
        same(plan.col[:len(col)], col, "index_build col, run %d" % rep)
        assert int(torch.count_nonzero(cnt)) == 0, rep
    plan = ops.csr_build([cuda(u) for u in us], [cuda(v) for v in vs], n_nodes)
    same(plan.rowptr, rowptr, "csr_build rowptr")
    same(plan.col[:len(col)], col, "csr_build col")


@pytest.mark.parametrize("n_nodes,n_rel", S.CSR_SMALL)
def test_csr_plan_at_the_tile_seams(n_nodes, n_rel):
    check_plan(*S.csr_case(n_nodes, n_rel), n_nodes, n_rel)


def test_csr_plan_at_the_largest_size():
    """1024 tiles: n_rel = 1, n_nodes = 4 194 288.  (One key more is refused on the host: test_seam_cases_host.py.)"""
    check_plan(*S.csr_case(S.CSR_MAX_NODES, 1, 100000, S.CSR_MAX_PLANT_TILES), S.CSR_MAX_NODES, 1)


# ------------------------------------------------------------------ 3. batched dilation
@pytest.mark.parametrize("N", S.GRAPH_NODES)
def test_dilate_batch_at_the_block_seams(N):
    from lanegcn_amd import ops
    pre = S.dilate_batch(N)
    suc = [S.transposed(c) for c in pre]
    flat = [cuda(np.concatenate([c[k] for c in rel])) for rel in (pre, suc) for k in "uv"]
    e_off = S.csum([len(c["u"]) for c in pre])
    got = ops.dilate_batch(*flat, S.csum([c["n"] for c in pre]), e_off, e_off, S.DILATE_SCALES)
    assert len(got) == S.DILATE_SCALES - 1
    want = {"pre": S.dilate_expected(pre), "suc": S.dilate_expected(suc)}
    for j, sc in enumerate(got):
        for k in ("pre", "suc"):
            w = want[k][j]
            same(sc[k + "_off"], w["off"], (N, k, j + 1, "off"))
            same(sc[k + "_u"], w["u"], (N, k, j + 1, "u"))
            same(sc[k + "_v"], w["v"], (N, k, j + 1, "v"))


# ------------------------------------------------------------------ 4. batched left / right
@pytest.mark.parametrize("N", S.GRAPH_NODES)
def test_cross_edges_batch_at_the_block_seams(N):
    from lanegcn_amd import ops
    scenes = S.cross_batch(N)
    arr, off = S.cross_flat(scenes)
    edges, offs = ops.cross_edges_batch(*(cuda(arr[k]) for k in ("ctrs", "feats", "lane_idcs") + S.CROSS_LISTS), off["node"],
                                        off["lane"], *(off[k] for k in S.CROSS_LISTS), 6.0)
    want = S.cross_expected(scenes, 6.0)
    for side in ("left", "right"):
        same(offs[side + "_off"], want[side + "_off"], (N, side, "off"))
        for c in "uv":
            same(edges["%s_%s" % (side, c)], want["%s_%s" % (side, c)], (N, side, c))
