"""GPU: the node-side Att tail (ops.node_tail / lgcn_node_tail) against the row block it replaces (ops.agg_mlp), bit for
bit, the shapes it refuses, Att.pairs_tail's choice between the two, and the engine's forward with and without it."""
import ctypes as C

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ROWS = (1, 47, 48, 49, 97, 337)                # below / at / past one 48-row tile, ragged last tiles, several workgroups
PAD = 64                                       # poisoned rows in front of and behind every output
POISON = 0x7fc0dead                            # a NaN pattern no kernel writes
COUNTS = (0, 1, 2, 3, 5, 0, 1, 9)              # pairs per target, repeated; one target gets 40


@pytest.fixture(scope="module")
def hip():
    import lanegcn_amd  # noqa: F401
    from lanegcn_amd import lanegcn as M
    from lanegcn_amd import ops
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return M, ops


@pytest.fixture
def mode(request, hip):
    _, ops = hip
    prev = ops.get_mma()
    ops.set_mma(request.param)
    yield request.param
    ops.set_mma(prev)


def bits(t):
    return t.contiguous().view(torch.int32)


def poisoned(n_rows):
    """(buffer, view of its rows [PAD, PAD + n_rows))"""
    buf = torch.full((n_rows + 2 * PAD, 128), POISON, dtype=torch.int32, device="cuda").view(torch.float32)
    return buf, buf[PAD:PAD + n_rows]


def clean_outside(buf, n):
    b = bits(buf)
    return bool((b[:PAD] == POISON).all()) and bool((b[PAD + n:] == POISON).all())


def att_pair(M, seed=11):
    """Two Att layers with GroupNorm weights away from (1, 0): the tail of the first, the chained U of the second."""
    torch.manual_seed(seed)
    atts = [M.Att(128, 128).cuda().eval() for _ in range(2)]
    with torch.no_grad():
        for a in atts:
            for gn in (a.norm, a.linear.norm, a.query.norm):
                gn.weight.uniform_(0.5, 1.5)
                gn.bias.uniform_(-0.5, 0.5)
    return atts


def problem(T, counts=COUNTS, big=True, seed=0):
    """(agts [T,128], m [P,128], rowptr [T+1] int32): targets with 0, 1, ... pairs and, with `big`, one with 40."""
    g = torch.Generator().manual_seed(1000 + T + seed)
    cnt = torch.tensor([counts[i % len(counts)] for i in range(T)], dtype=torch.int64)
    if big and counts != (0,):
        cnt[T // 2] = 40
    rowptr = torch.zeros(T + 1, dtype=torch.int32)
    rowptr[1:] = torch.cumsum(cnt, 0).to(torch.int32)
    P = int(rowptr[-1])
    agts = torch.randn(T, 128, generator=g).relu()
    m = torch.randn(max(P, 1), 128, generator=g).relu()
    return agts.cuda(), m.cuda(), rowptr.cuda()


def tail_kw(M, ops, atts, agts, m, rowptr, chain, mode_rel=None):
    from lanegcn_amd import _lib as L
    att, nxt = atts
    rels = [ops.RelSpec(agts, ops.packed(att.agt.weight)),
            ops.RelSpec(m, ops.packed(att.ctx[1].weight), L.REL_RANGE if mode_rel is None else mode_rel)]
    kw = dict(rowptr=rowptr, gn1=M._gn(att.norm), wp2=ops.packed(att.linear.linear.weight), gn2=M._gn(att.linear.norm),
              res=agts, eps=att.norm.eps, chain_u=nxt.chain_u() if chain else None)
    return rels, kw


def launch(ops, entry, T, rels, kw):
    """One launch of `entry` (lgcn_agg_mlp / lgcn_node_tail) with out and the chained U in poisoned buffers.
    Returns (out buffer, out, U buffer or None, U or None)."""
    from lanegcn_amd import _lib as L
    obuf, out = poisoned(T)
    p, keep, _ = ops._agg_params(T, rels, L.F_GN1 | L.F_RELU1 | L.F_GEMM2 | L.F_GN2 | L.F_RES | L.F_RELU2, out=out, **kw)
    ubuf = u = None
    if kw.get("chain_u") is not None:
        ubuf, u = poisoned(T)
        p.ch_u_out = u.data_ptr()
    L.check(getattr(L.load(), entry)(C.byref(p), ops._stream()), entry)
    torch.cuda.synchronize()
    return obuf, out, ubuf, u


def check_equal(M, ops, atts, agts, m, rowptr, chain, tag):
    T = agts.shape[0]
    rels, kw = tail_kw(M, ops, atts, agts, m, rowptr, chain)
    _, want, _, want_u = launch(ops, "lgcn_agg_mlp", T, rels, kw)
    obuf, got, ubuf, got_u = launch(ops, "lgcn_node_tail", T, rels, kw)
    assert torch.equal(bits(got), bits(want)), (tag, T, chain, "out")
    assert clean_outside(obuf, T), (tag, T, chain, "wrote outside out's rows")
    if chain:
        assert torch.equal(bits(got_u), bits(want_u)), (tag, T, chain, "U")
        assert clean_outside(ubuf, T), (tag, T, chain, "wrote outside U's rows")
    return want, want_u


@pytest.mark.parametrize("mode", ["f16x2", "bf16"], indirect=True)
@pytest.mark.parametrize("chain", [False, True])
@pytest.mark.parametrize("n_rows", ROWS)
def test_equals_the_row_block_bit_for_bit(hip, mode, chain, n_rows):
    """Targets with 0, 1, 2, 3, 5, 9 pairs and one with 40; guard rows around out and U stay untouched."""
    M, ops = hip
    atts = att_pair(M)
    agts, m, rowptr = problem(n_rows)
    want, _ = check_equal(M, ops, atts, agts, m, rowptr, chain, mode)
    assert bool(torch.isfinite(want).all()) and float(want.abs().max()) > 0
    # through the wrapper, which allocates the outputs: same values
    rels, kw = tail_kw(M, ops, atts, agts, m, rowptr, chain)
    from lanegcn_amd import _lib as L
    full = L.F_GN1 | L.F_RELU1 | L.F_GEMM2 | L.F_GN2 | L.F_RES | L.F_RELU2
    a, b = ops.node_tail(n_rows, rels, full, **kw), ops.agg_mlp(n_rows, rels, full, **kw)
    for x, y in zip(a if chain else (a,), b if chain else (b,)):
        assert x.shape == (n_rows, 128) and torch.equal(bits(x), bits(y))


@pytest.mark.parametrize("mode", ["f16x2", "bf16"], indirect=True)
@pytest.mark.parametrize("chain", [False, True])
def test_a_set_without_pairs(hip, mode, chain):
    M, ops = hip
    atts = att_pair(M)
    agts, m, rowptr = problem(97, counts=(0,))
    assert int(rowptr[-1]) == 0
    check_equal(M, ops, atts, agts, m, rowptr, chain, mode)


@pytest.mark.parametrize("mode", ["f16x2", "bf16"], indirect=True)
def test_inf_and_nan_rows_stay_in_their_rows(hip, mode):
    """An inf in one target's own row and a NaN in a pair row of another: those two output rows are non-finite, as the row
    block gives them, and every other row has the bits of the run without them."""
    M, ops = hip
    atts = att_pair(M)
    agts, m, rowptr = problem(100)
    clean, clean_u = check_equal(M, ops, atts, agts, m, rowptr, True, mode)
    agts2, m2 = agts.clone(), m.clone()
    agts2[7, 5] = float("inf")
    tgt = 60
    assert int(rowptr[tgt + 1]) > int(rowptr[tgt])
    m2[int(rowptr[tgt]), 100] = float("nan")
    want, want_u = check_equal(M, ops, atts, agts2, m2, rowptr, True, mode)
    others = [i for i in range(100) if i not in (7, tgt)]
    for w, c in ((want, clean), (want_u, clean_u)):
        assert not torch.isfinite(w[7]).all() and not torch.isfinite(w[tgt]).all()
        assert torch.equal(bits(w[others]), bits(c[others]))


@pytest.mark.parametrize("mode", ["bf16x3", "f32"], indirect=True)
def test_other_modes_are_refused(hip, mode):
    M, ops = hip
    from lanegcn_amd import _lib as L
    atts = att_pair(M)
    agts, m, rowptr = problem(49)
    rels, kw = tail_kw(M, ops, atts, agts, m, rowptr, False)
    assert not ops.node_tail_ok()
    with pytest.raises(L.LgcnError, match=r"code -2"):      # LGCN_ESHAPE
        ops.node_tail(49, rels, M._FULL, **kw)


def test_other_shapes_are_refused(hip):
    M, ops = hip
    from lanegcn_amd import _lib as L
    prev = ops.get_mma()
    ops.set_mma("f16x2")
    try:
        atts = att_pair(M)
        agts, m, rowptr = problem(49)
        assert ops.node_tail_ok()
        rels, kw = tail_kw(M, ops, atts, agts, m, rowptr, False, mode_rel=L.REL_RANGE16)
        with pytest.raises(L.LgcnError, match=r"code -2"):
            ops.node_tail(49, rels, M._FULL, **kw)
        rels, kw = tail_kw(M, ops, atts, agts, m, rowptr, True)
        with pytest.raises(L.LgcnError, match=r"code -2"):
            ops.node_tail(49, rels, M._FULL, **dict(kw, chain_v=atts[1].chain_v()))
        with pytest.raises(L.LgcnError, match=r"code -2"):
            ops.node_tail(49, rels, M._FULL & ~L.F_RELU2, **kw)
        with pytest.raises(L.LgcnError, match=r"code -2"):
            ops.node_tail(49, rels[:1], M._FULL, **kw)
        assert ops.node_tail(0, rels, M._FULL, **dict(kw, chain_u=None)).shape == (0, 128)
    finally:
        ops.set_mma(prev)


def test_pairs_tail_picks_the_launch(hip):
    """Att.pairs_tail takes the new launch for many targets over few context rows without a chained V in f16x2, and the
    row block when a V is chained, when the context rows outnumber the targets (16-row pieces), in bf16x3 and in f32."""
    M, ops = hip
    prev = ops.get_mma()
    real_nt, real_agg = ops.node_tail, ops.agg_mlp
    calls = []
    try:
        ops.node_tail = lambda *a, **k: (calls.append("node_tail"), real_nt(*a, **k))[1]
        ops.agg_mlp = lambda *a, **k: (calls.append("agg_mlp"), real_agg(*a, **k))[1]

        def run(T, S, chain_v):
            atts = att_pair(M)
            g = torch.Generator().manual_seed(5)
            tc, sc = (torch.rand(T, 2, generator=g) * 12).cuda(), (torch.rand(S, 2, generator=g) * 12).cuda()
            off = lambda n: torch.tensor([0, n], dtype=torch.int32, device="cuda")
            ps = ops.pairs_build(tc, off(T), sc, off(S), 4.0, T * S)
            assert 0 < ps.count() < T * S
            agts = torch.randn(T, 128, generator=g).relu().cuda()
            ctx = torch.randn(S, 128, generator=g).relu().cuda()
            U, V = ops.agg_mlp_pair(atts[0].u_kw(agts), atts[0].v_kw(ctx))
            del calls[:]
            res = atts[0].pairs_tail(agts, S, ps, U, V, chain_u=atts[1].chain_u(), chain_v=atts[1].chain_v() if chain_v else None)
            torch.cuda.synchronize()
            return list(calls), res

        ops.set_mma("f16x2")
        took, got = run(97, 20, False)
        assert took == ["node_tail"]
        ops.node_tail_ok, ok = (lambda: False), ops.node_tail_ok
        try:
            took, want = run(97, 20, False)
        finally:
            ops.node_tail_ok = ok
        assert took == ["agg_mlp"]
        for x, y in zip(got, want):
            assert torch.equal(bits(x), bits(y))
        assert run(97, 20, True)[0] == ["agg_mlp"]           # a chained V
        assert run(20, 97, False)[0] == ["agg_mlp"]          # context rows outnumber the targets
        for other in ("bf16x3", "f32"):
            ops.set_mma(other)
            assert run(97, 20, False)[0] == ["agg_mlp"], other
    finally:
        ops.node_tail, ops.agg_mlp = real_nt, real_agg
        ops.set_mma(prev)


# ------------------------------------------------------------------ through the engine
@pytest.fixture(scope="module")
def s0(hip):
    from lanegcn_amd import data as gen
    from lanegcn_amd.engine import collate_flat
    scenes = gen.synth_batch("S0", seed=3)
    fb = collate_flat(scenes)
    actors = torch.from_numpy(np.random.default_rng(5).normal(0, 1, (fb.n_actors, 128)).astype(np.float32)).relu().cuda()
    return fb, actors


@pytest.mark.parametrize("mode", ["f16x2", "bf16"], indirect=True)
def test_forward_with_and_without_the_launch(hip, s0, mode):
    """HotPathEngine.forward on S0: A2M's two tails take the new launch; with ops.node_tail_ok patched to False they take
    the row block, and nodes and actors (and every stage) have the same bits."""
    M, ops = hip
    from lanegcn_amd.engine import HotPathEngine
    fb, actors = s0
    torch.manual_seed(21)
    eng = HotPathEngine(*[cls(M.config).cuda().eval() for cls in (M.MapNet, M.A2M, M.M2M, M.M2A, M.A2A)])
    launches = []
    real, ok = ops.node_tail, ops.node_tail_ok
    try:
        ops.node_tail = lambda *a, **k: (launches.append(1), real(*a, **k))[1]
        got = eng.forward(fb, actors, stages=True)
        n_new = len(launches)
        ops.node_tail_ok = lambda: False
        want = eng.forward(fb, actors, stages=True)
        torch.cuda.synchronize()
        assert n_new == 2 and len(launches) == 2
        for k in ("nodes", "actors", "a2m", "m2m", "m2a", "a2a"):
            assert torch.equal(bits(got[k]), bits(want[k])), k
        assert bool(torch.isfinite(want["actors"]).all()) and float(want["actors"].abs().max()) > 0
    finally:
        ops.node_tail, ops.node_tail_ok = real, ok
