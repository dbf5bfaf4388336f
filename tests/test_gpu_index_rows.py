"""GPU: the index stage's row bodies, row-scan tiles and LDS segment search (csrc/lgcn_index.hip) against host models only:
oracle.lanegcn_oracle.pair_search through tests/seam_cases.py and numpy.  Every output is an integer array and is compared
word for word.

  short row body     several target rows per wave (a group of lanes, at the narrowest one lane, per row): row groups that
                     straddle scene boundaries (scenes of 1, 63, 64, 65, 0 and 130 rows), context lists of 0, 1, 2, 63, 64,
                     65 and 130 around every trip length up to a wave's, distances exactly on the bound
  selection rule     jobs far on either side of it (mean list 8 and 400) and a sweep of uniform lists 48 .. 80 that crosses
                     it wherever it lies; the same scenes as four mixed jobs of one launch (job_blocks)
  capacity           a short-list job whose cap is below its count: n_pairs negative, rowptr describes [0, cap), nothing
                     is written behind hi[cap] / wi[cap]
  row-scan tiles     4095 / 4096 / 4097 / 8193 rows, a job without rows, a tile of rows without pairs between two with
                     pairs, scene boundaries exactly on the tile edges in legacy mode
  segment table      index_build on 1, 2 and 37 scenes with empty pieces, and on 600 scenes: 2400 pieces, more than the
                     2048 words the count pass stages in LDS, so the global search runs
  captured forward   replayed twice on S0: the pair sets and the bits of nodes / actors of the eager forward"""
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
    assert np.array_equal(got, want), (what, "first difference at", int(np.flatnonzero(got != want)[0]))


def make_case(name, rows, ctx, seed, far=()):
    """Scenes of rows[i] target rows and ctx[i] context rows on the integer grid; scenes listed in `far` hold no pair."""
    rng = np.random.default_rng(seed)
    return {"name": name, "agt": [S._grid(rng, n) for n in rows],
            "ctx": [S._grid(rng, n) + np.float32(500.0 if i in far else 0.0) for i, n in enumerate(ctx)]}


_EXPECTED = {}


def expected(case, legacy):
    key = (case["name"], legacy)
    if key not in _EXPECTED:
        hi, wi, rp = S.pair_expected(case, legacy)
        for a in (hi, wi, rp):
            a.setflags(write=False)
        _EXPECTED[key] = (hi, wi, rp)
    return _EXPECTED[key]


def search_of(case, cap=None):
    agt, a_off, ctx, c_off, bound = S.pair_flat(case)
    return (cuda(agt), cuda(a_off), cuda(ctx), cuda(c_off), S.PAIR_TH, bound if cap is None else cap)


def check_pairs(ps, case, legacy, what):
    hi_w, wi_w, rp_w = expected(case, legacy)
    what = "%s %s legacy=%s" % (what, case["name"], legacy)
    same(ps.n_pairs, np.asarray([len(hi_w)], np.int32), what + " n_pairs")
    same(ps.hi[:len(hi_w)], hi_w.astype(np.int32), what + " hi")
    same(ps.wi[:len(wi_w)], wi_w.astype(np.int32), what + " wi")
    same(ps.rowptr, rp_w, what + " rowptr_q")


def small_plan():
    """A CSR problem for the pair jobs to ride behind: (idx, seg_off, seg_base, rel, n_nodes, rowptr, col)."""
    n_nodes, n_rel = 64, 2
    us, vs = S.csr_case(n_nodes, n_rel, 200)
    runs = [t for pair in zip(us, vs) for t in pair]
    offs = S.csum([len(t) for t in runs])
    rel = [((int(offs[2 * r]), int(offs[2 * r + 1])), (int(offs[2 * r + 1]), int(offs[2 * r + 2]))) for r in range(n_rel)]
    rowptr, col = S.csr_expected(us, vs, n_nodes, n_rel)
    return cuda(np.concatenate(runs)), cuda(offs[:-1].copy()), torch.zeros(len(runs), dtype=torch.int64, device="cuda"), rel, n_nodes, rowptr, col


def all_routes(cases, what):
    """The jobs alone through pairs_build, together through pairs_build_multi and behind the edge workgroups of index_build."""
    from lanegcn_amd import ops
    assert 1 <= len(cases) <= 4
    idx, seg_off, seg_base, rel, n_nodes, rowptr, col = small_plan()
    for legacy in (True, False):
        for c in cases:
            check_pairs(ops.pairs_build(*search_of(c), legacy), c, legacy, what + " pairs_build")
        for c, ps in zip(cases, ops.pairs_build_multi([search_of(c) for c in cases], legacy)):
            check_pairs(ps, c, legacy, what + " multi")
        cnt = ops.index_counters(n_nodes, len(rel), idx.device)
        plan, pairs = ops.index_build(idx, seg_off, seg_base, rel, n_nodes, [search_of(c) for c in cases], legacy, cnt=cnt)
        same(plan.rowptr, rowptr, what + " plan rowptr")
        same(plan.col[:len(col)], col, what + " plan col")
        assert int(torch.count_nonzero(cnt)) == 0
        for c, ps in zip(cases, pairs):
            check_pairs(ps, c, legacy, what + " index_build")


# ------------------------------------------------------------------ short row body
ROWS6, CTX7 = (1, 63, 64, 65, 0, 130), (0, 1, 2, 63, 64, 65, 130)
STRADDLE = make_case("straddle", [ROWS6[i % 6] for i in range(42)], [CTX7[i % 7] for i in range(42)], 11)      # every combination


def test_case_sizes():
    agt, a_off, ctx, c_off, _ = S.pair_flat(STRADDLE)
    assert len(agt) == 7 * 323 and len(ctx) == 6 * 325
    cuts = set(a_off.tolist())
    assert any(c % 64 for c in cuts) and {1, 64, 128, 193} <= cuts          # boundaries inside and on the 64-row groups
    assert S.pair_counts(STRADDLE).sum() > 1000
    on = 0
    for a, c in zip(STRADDLE["agt"], STRADDLE["ctx"]):
        d = a.reshape(-1, 1, 2) - c.reshape(1, -1, 2)
        on += int(((d * d).sum(2) == np.float32(S.PAIR_TH) ** 2).sum())
    assert on > 50                                                           # distances exactly on the bound


def test_row_groups_straddle_scene_boundaries():
    all_routes([STRADDLE], "straddle")


# ------------------------------------------------------------------ selection rule
ROWS5 = (3, 70, 0, 65, 10)
MEAN8 = make_case("mean8", ROWS5, (8, 0, 16, 7, 9), 12)
MEAN400 = make_case("mean400", ROWS5, (400, 0, 800, 399, 401), 13)
SWEEP = {L: make_case("uniform%d" % L, (5, 66, 3), (L, L, L), 100 + L) for L in range(48, 81, 4)}


@pytest.mark.parametrize("case", [MEAN8, MEAN400], ids=lambda c: c["name"])
def test_both_sides_of_the_rule(case):
    all_routes([case], "rule")


def test_uniform_lists_across_the_rule():
    from lanegcn_amd import ops
    for L, case in SWEEP.items():
        for legacy in (True, False):
            check_pairs(ops.pairs_build(*search_of(case), legacy), case, legacy, "sweep")


@pytest.mark.parametrize("names", [("mean8", "mean400", 64, 68), (48, 80, "mean400", "straddle"), (60, "mean8", 72, 76)],
                         ids=lambda n: "-".join(str(x) for x in n))
def test_mixed_jobs_in_one_launch(names):
    by = {"mean8": MEAN8, "mean400": MEAN400, "straddle": STRADDLE}
    all_routes([by[n] if n in by else SWEEP[n] for n in names], "mixed")


# ------------------------------------------------------------------ capacity
@pytest.mark.parametrize("case", [MEAN8, STRADDLE], ids=lambda c: c["name"])
@pytest.mark.parametrize("short", [3, 0])
def test_capacity_in_a_short_list_job(case, short):
    from lanegcn_amd import ops
    GUARD, MARK = 16, -7
    for legacy in (True, False):
        hi_w, wi_w, rp_w = expected(case, legacy)
        P = len(hi_w)
        cap = P - short
        s = search_of(case, cap)
        T, B = s[0].shape[0], s[1].numel() - 1
        i32 = dict(dtype=torch.int32, device="cuda")
        bufs = (torch.full((cap + GUARD,), MARK, **i32), torch.full((cap + GUARD,), MARK, **i32), torch.full((1,), MARK, **i32),
                torch.full((T + 1,), MARK, **i32), torch.full((ops.pairs_alloc(T, B, 1, "cuda")[4].numel(),), MARK, **i32))
        ps = ops.pairs_build(*s[:5], cap, legacy, bufs=bufs)
        what = "%s cap=P-%d legacy=%s" % (case["name"], short, legacy)
        same(ps.n_pairs, np.asarray([-P if short else P], np.int32), what + " n_pairs")
        same(ps.hi[:cap], hi_w[:cap].astype(np.int32), what + " hi")
        same(ps.wi[:cap], wi_w[:cap].astype(np.int32), what + " wi")
        same(ps.hi[cap:], np.full(GUARD, MARK, np.int32), what + " words behind hi[cap]")
        same(ps.wi[cap:], np.full(GUARD, MARK, np.int32), what + " words behind wi[cap]")
        same(ps.rowptr, np.minimum(rp_w, cap).astype(np.int32), what + " rowptr_q describes [0, cap)")


# ------------------------------------------------------------------ row-scan tiles
@pytest.mark.parametrize("T", sorted(S.PAIR_ROWS))
def test_row_scan_tiles(T):
    from lanegcn_amd import ops
    case = S.pair_case_rows(T)
    for legacy in (True, False):
        check_pairs(ops.pairs_build(*search_of(case), legacy), case, legacy, "tiles")


ZERO_TILE = make_case("zero_tile", (4096, 4096, 100), (20, 20, 20), 14, far=(1,))


def test_a_tile_without_pairs_between_two_with_pairs():
    """Scene boundaries on rows 4096 and 8192, the tile edges; in legacy mode the middle scene does not advance."""
    assert S.pair_counts(ZERO_TILE)[1] == 0 and S.pair_counts(ZERO_TILE)[0] > 0 and S.pair_counts(ZERO_TILE)[2] > 0
    hi_l, hi_f = expected(ZERO_TILE, True)[0], expected(ZERO_TILE, False)[0]
    assert hi_l.max() < 4096 + 100 and hi_f.max() >= 8192
    all_routes([ZERO_TILE], "zero tile")


def test_a_job_without_rows():
    from lanegcn_amd import ops
    empty = (torch.zeros((0, 2), device="cuda"), torch.zeros(4, dtype=torch.int32, device="cuda"),
             cuda(np.ones((5, 2), np.float32)), cuda(np.asarray([0, 2, 2, 5], np.int32)), S.PAIR_TH, 8)
    idx, seg_off, seg_base, rel, n_nodes, rowptr, col = small_plan()
    for legacy in (True, False):
        got = ops.pairs_build_multi([search_of(MEAN8), empty, search_of(MEAN400)], legacy)
        _, both = ops.index_build(idx, seg_off, seg_base, rel, n_nodes, [empty, search_of(MEAN8)], legacy)
        alone = ops.pairs_build(*empty, legacy)
        check_pairs(got[0], MEAN8, legacy, "around an empty job")
        check_pairs(got[2], MEAN400, legacy, "around an empty job")
        check_pairs(both[1], MEAN8, legacy, "behind an empty job")
        for ps in (got[1], both[0], alone):
            same(ps.n_pairs, np.zeros(1, np.int32), "empty job n_pairs")
            same(ps.rowptr, np.zeros(1, np.int32), "empty job rowptr_q")


# ------------------------------------------------------------------ segment table
def scene_batch(B, seed):
    """B scenes of 3 .. 9 nodes and two relations, as the flat batch lays them out: per relation a run of local u and a run
    of local v, one piece per scene in each run.  Relation 1 has no edge in every third scene (equal neighbours in seg_off);
    a few local indices point outside their scene.  Returns (idx_local, seg_off, seg_base, rel, n_nodes, us, vs global)."""
    rng = np.random.default_rng(seed)
    n = rng.integers(3, 10, B)
    base = S.csum(n)
    runs, seg_len, seg_base, us, vs = [], [], [], [], []
    for r in range(2):
        m = [0 if (r == 1 and b % 3 == 0) else int(rng.integers(1, 12)) for b in range(B)]
        loc = [[rng.integers(0, n[b], m[b]) for b in range(B)] for _ in range(2)]
        if B > 1:
            loc[0][1] = np.concatenate([loc[0][1], [-1, n[1]]])
            loc[1][1] = np.concatenate([loc[1][1], [0, 1]])
        if B == 1:
            loc[0][0] = np.concatenate([loc[0][0], [-1, 0]])
            loc[1][0] = np.concatenate([loc[1][0], [0, n[0]]])
        for side in loc:
            runs.append(np.concatenate(side).astype(np.int64))
            seg_len += [len(x) for x in side]
            seg_base += [int(base[b]) for b in range(B)]
        us.append(np.concatenate([loc[0][b] + base[b] for b in range(B)]).astype(np.int64))
        vs.append(np.concatenate([loc[1][b] + base[b] for b in range(B)]).astype(np.int64))
    offs = S.csum([len(t) for t in runs])
    rel = [((int(offs[2 * r]), int(offs[2 * r + 1])), (int(offs[2 * r + 1]), int(offs[2 * r + 2]))) for r in range(2)]
    seg_off = S.csum(seg_len)[:-1].copy()
    assert len(seg_off) == 4 * B and (B < 3 or (np.diff(seg_off) == 0).any())
    return np.concatenate(runs), seg_off, np.asarray(seg_base, np.int64), rel, int(base[-1]), us, vs


@pytest.mark.parametrize("B", [1, 2, 37, 600])
def test_segment_search(B):
    """600 scenes are 2400 pieces: past the 2048 that fit the count pass's LDS table (kIdxSegLds), in well under a second."""
    from lanegcn_amd import ops
    idx, seg_off, seg_base, rel, n_nodes, us, vs = scene_batch(B, B)
    rowptr, col = S.csr_expected(us, vs, n_nodes, 2)
    assert len(col) < sum(len(u) for u in us) or B > 2                     # some edges leave [0, n_nodes) and are dropped
    cnt = ops.index_counters(n_nodes, 2, "cuda")
    for rep in range(2):
        plan, pairs = ops.index_build(cuda(idx), cuda(seg_off), cuda(seg_base), rel, n_nodes, [search_of(MEAN8)], cnt=cnt)
        same(plan.rowptr, rowptr, "B=%d rowptr, run %d" % (B, rep))
        same(plan.col[:len(col)], col, "B=%d col, run %d" % (B, rep))
        assert int(torch.count_nonzero(cnt)) == 0, (B, rep)
        check_pairs(pairs[0], MEAN8, True, "beside B=%d" % B)


# ------------------------------------------------------------------ a captured forward
def test_captured_forward_replayed_twice(monkeypatch):
    from lanegcn_amd import data as gen
    from lanegcn_amd import lanegcn as M
    from lanegcn_amd import ops
    from lanegcn_amd.engine import HotPathEngine, collate_flat
    prev = ops.get_mma()
    ops.set_mma("f16x2")
    try:
        fb = collate_flat(gen.synth_batch("S0", seed=3))
        actors = torch.from_numpy(np.random.default_rng(5).normal(0, 1, (fb.n_actors, 128)).astype(np.float32)).relu().cuda()
        torch.manual_seed(21)
        eng = HotPathEngine(*[cls(M.config).cuda().eval() for cls in (M.MapNet, M.A2M, M.M2M, M.M2A, M.A2A)])
        sets, real = [], ops.index_build
        monkeypatch.setattr(ops, "index_build", lambda *a, **k: (lambda r: (sets.append(r[1]), r)[1])(real(*a, **k)))

        def snapshot(out, pairs):
            torch.cuda.synchronize()
            res = {k: out[k].contiguous().view(torch.int32).cpu().numpy().copy() for k in ("nodes", "actors")}
            for i, ps in enumerate(pairs):
                P = int(ps.n_pairs.item())
                assert P > 0
                res["pairs%d" % i] = np.concatenate([[P], ps.hi[:P].cpu().numpy(), ps.wi[:P].cpu().numpy(), ps.rowptr.cpu().numpy()])
            return res

        want = snapshot(eng.forward(fb, actors), sets[-1])
        assert len(sets[-1]) == 3
        graph, out = eng.capture(fb, actors)
        captured = sets[-1]
        for rep in range(2):
            for ps in captured:                                            # a replay must rebuild every word it reads
                ps.hi.fill_(-3); ps.wi.fill_(-3); ps.rowptr.fill_(-3); ps.n_pairs.fill_(-3)
            graph.replay()
            got = snapshot(out, captured)
            for k in want:
                assert np.array_equal(got[k], want[k]), (k, rep)
    finally:
        ops.set_mma(prev)
