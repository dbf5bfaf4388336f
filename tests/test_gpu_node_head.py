"""GPU: the node-side Att head (ops.node_head / lgcn_node_head) against the row-block launches it replaces (lgcn_agg_mlp,
ops.agg_mlp_multi), bit for bit, the problems it refuses, att_block's choice between the two, and the engine's forward with
and without it."""
import ctypes as C

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ROWS = (1, 47, 48, 49, 97, 337)                # below / at / past one 48-row tile, ragged last tiles, several workgroups
ROWS_SMALL = (1, 33, 48, 129)
PAD = 64                                       # poisoned rows in front of and behind every output
POISON = 0x7fc0dead                            # a NaN pattern no kernel writes
ESHAPE = -2


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


def untouched(buf):
    return bool((bits(buf) == POISON).all())


def a2m_block(M, seed=11):
    """A2M (meta + two Att layers) with GroupNorm weights away from (1, 0)."""
    torch.manual_seed(seed)
    a2m = M.A2M(M.config).cuda().eval()
    with torch.no_grad():
        for gn in [a2m.meta.norm] + [g for a in a2m.att for g in (a.norm, a.linear.norm, a.query.norm)]:
            gn.weight.uniform_(0.5, 1.5)
            gn.bias.uniform_(-0.5, 0.5)
    return a2m


def rows_of(n, seed=0):
    """(feat [n,128], turn [n,2], control [n], intersect [n]) on the GPU."""
    g = torch.Generator().manual_seed(2000 + n + seed)
    feat = torch.randn(n, 128, generator=g).relu()
    flag = lambda *s: (torch.rand(*s, generator=g) < 0.3).float()
    return feat.cuda(), flag(n, 2).cuda(), flag(n).cuda(), flag(n).cuda()


def head_kw(a2m, rows, chain=True, w4=True):
    kw = a2m.meta_kw(*rows)
    if not w4:
        kw = {k: v for k, v in kw.items() if k not in ("w4", "x4")}
    return dict(kw, chain_u=a2m.att[0].chain_u()) if chain else kw


def build(ops, kw):
    """(lgcn_agg_mlp_t, what it points at, [(buffer, rows)] of out and the chained U) with the outputs in poisoned buffers."""
    n = kw["n_rows"]
    held = [poisoned(n)]
    p, keep, _ = ops._agg_params(out=held[0][1], **kw)
    if kw.get("chain_u") is not None:
        held.append(poisoned(n))
        p.ch_u_out = held[1][1].data_ptr()
    return p, keep, held


def row_blocks(ops, kws):
    """Every problem as a launch of its own (lgcn_agg_mlp) -> [[(buffer, rows)]]"""
    from lanegcn_amd import _lib as L
    res = []
    for kw in kws:
        p, keep, held = build(ops, kw)
        L.check(L.load().lgcn_agg_mlp(C.byref(p), ops._stream()), "lgcn_agg_mlp")
        res.append(held)
    torch.cuda.synchronize()
    return res


def node_head(ops, kws, expect=0):
    """The problems in one lgcn_node_head launch -> [[(buffer, rows)]]"""
    from lanegcn_amd import _lib as L
    built = [build(ops, kw) for kw in kws]
    arr = (C.POINTER(L.AggMlp) * len(built))(*[C.pointer(b[0]) for b in built])
    rc = L.load().lgcn_node_head(arr, len(built), ops._stream())
    torch.cuda.synchronize()
    assert rc == expect, (rc, expect)
    return [b[2] for b in built]


def check_equal(ops, kws, tag):
    want, got = row_blocks(ops, kws), node_head(ops, kws)
    for i, (kw, w, g) in enumerate(zip(kws, want, got)):
        assert len(w) == len(g)
        for j, ((_, wr), (gb, gr)) in enumerate(zip(w, g)):
            assert torch.equal(bits(gr), bits(wr)), (tag, "problem", i, "output", j, kw["n_rows"])
            assert clean_outside(gb, kw["n_rows"]), (tag, "problem", i, "output", j, "wrote outside its rows")
    return want


@pytest.mark.parametrize("mode", ["f16x2", "bf16"], indirect=True)
@pytest.mark.parametrize("w4", [False, True])
@pytest.mark.parametrize("chain", [False, True])
@pytest.mark.parametrize("n_rows", ROWS)
def test_head_equals_the_row_block_bit_for_bit(hip, mode, chain, w4, n_rows):
    """A2M.meta with and without its rank-4 update and the chained U; guard rows around out and U stay untouched."""
    M, ops = hip
    a2m = a2m_block(M)
    kw = head_kw(a2m, rows_of(n_rows), chain, w4)
    want = check_equal(ops, [kw], mode)[0]
    for _, w in want:
        assert bool(torch.isfinite(w).all()) and float(w.abs().max()) > 0
    # through the wrapper, which allocates the outputs: same values
    a, b = ops.node_head([kw])[0], ops.agg_mlp(**kw)
    for x, y in zip(a if chain else (a,), b if chain else (b,)):
        assert x.shape == (n_rows, 128) and torch.equal(bits(x), bits(y))


def test_the_rank4_update_is_seen(hip):
    """The rank-4 rows change the head's output (a launch that dropped them would still agree with itself)."""
    M, ops = hip
    a2m = a2m_block(M)
    rows = rows_of(97)
    assert float(rows[1].abs().sum()) > 0
    a, b = ops.node_head([head_kw(a2m, rows, False, True)])[0], ops.node_head([head_kw(a2m, rows, False, False)])[0]
    assert not torch.equal(bits(a), bits(b))


@pytest.mark.parametrize("mode", ["f16x2", "bf16"], indirect=True)
@pytest.mark.parametrize("form", ["u-chain", "plain"])
@pytest.mark.parametrize("n_rows", ROWS_SMALL)
def test_u_chain_and_plain_alone(hip, mode, form, n_rows):
    M, ops = hip
    a2m = a2m_block(M)
    x = rows_of(n_rows)[0]
    kw = a2m.att[0].u_kw(x) if form == "u-chain" else a2m.att[0].v_kw(x)
    assert ops.node_head_form(kw) == form
    want = check_equal(ops, [kw], (mode, form))[0]
    assert bool(torch.isfinite(want[0][1]).all()) and float(want[0][1].abs().max()) > 0


@pytest.mark.parametrize("mode", ["f16x2", "bf16"], indirect=True)
@pytest.mark.parametrize("case", ["same rows", "other rows", "fewer rows"])
def test_two_plain_problems(hip, mode, case):
    """Two plain problems over the same rows (one tile range, rows read once), over different tensors and over a prefix of
    the same tensor: each equals a launch of its own."""
    M, ops = hip
    a2m = a2m_block(M)
    x = rows_of(129)[0]
    y = {"same rows": x, "other rows": rows_of(129, seed=1)[0], "fewer rows": x[:50]}[case]
    check_equal(ops, [a2m.att[0].v_kw(x), a2m.att[1].v_kw(y)], (mode, case))
    check_equal(ops, [a2m.att[1].v_kw(y), a2m.att[0].v_kw(x)], (mode, case, "swapped"))


@pytest.mark.parametrize("mode", ["f16x2", "bf16"], indirect=True)
@pytest.mark.parametrize("order", ["uv", "vu", "vvu", "uvv", "vuv", "vvv", "uu", "vuvu"])
def test_problems_over_the_same_rows(hip, mode, order):
    """A u-chain and up to two plain problems over the same rows run in one tile range, in whatever order they are listed;
    a third plain problem or a second u-chain opens another: each problem equals a launch of its own."""
    M, ops = hip
    atts = list(a2m_block(M).att) + list(a2m_block(M, seed=12).att)
    x = rows_of(129)[0]
    us, vs = [a.u_kw(x) for a in atts], [a.v_kw(x) for a in atts]
    probs = [(us if c == "u" else vs)[i] for i, c in enumerate(order)]
    check_equal(ops, probs, (mode, order))


def forward_list(a2m, m2a_att, n_nodes, n_actors):
    """What A2M's first launch carries in the folded forward: meta + chained U0 over the nodes, V0 and V1 over the actors,
    and M2A's U of layer 0 over the actors."""
    rows = rows_of(n_nodes)
    actors = rows_of(n_actors, seed=7)[0]
    return [head_kw(a2m, rows), a2m.att[0].v_kw(actors), a2m.att[1].v_kw(actors), m2a_att.u_kw(actors)]


@pytest.mark.parametrize("mode", ["f16x2", "bf16"], indirect=True)
@pytest.mark.parametrize("n_actors", [1, 50])
@pytest.mark.parametrize("n_nodes", [49, 337])
def test_the_forwards_combination(hip, mode, n_nodes, n_actors):
    M, ops = hip
    a2m = a2m_block(M)
    m2a_att = a2m_block(M, seed=12).att[1]
    probs = forward_list(a2m, m2a_att, n_nodes, n_actors)
    assert [ops.node_head_form(kw) for kw in probs] == ["head", "plain", "plain", "u-chain"]
    for n in (4, 1, 2, 3):
        part = probs[:n]
        want = ops.agg_mlp_multi(part)
        got = node_head(ops, part)
        torch.cuda.synchronize()
        for i, (kw, w, g) in enumerate(zip(part, want, got)):
            for j, (wr, (gb, gr)) in enumerate(zip(w if isinstance(w, tuple) else (w,), g)):
                assert torch.equal(bits(gr), bits(wr)), (mode, n, "problem", i, "output", j)
                assert clean_outside(gb, kw["n_rows"]), (mode, n, "problem", i, "output", j, "wrote outside its rows")
        # and each problem against a launch of its own
        check_equal(ops, part, (mode, n))


@pytest.mark.parametrize("mode", ["f16x2", "bf16"], indirect=True)
def test_inf_and_nan_rows_have_the_row_blocks_bits(hip, mode):
    """An inf and a NaN in two rows and an inf in a third row's rank-4 input: every output has the row block's bit patterns,
    those three rows are non-finite and every other row has the bits of the run without them."""
    M, ops = hip
    a2m = a2m_block(M)
    feat, turn, control, intersect = rows_of(100)
    lists = lambda rows: [head_kw(a2m, rows), a2m.att[0].u_kw(rows[0]), a2m.att[0].v_kw(rows[0]), a2m.att[1].v_kw(rows[0])]
    clean = check_equal(ops, lists((feat, turn, control, intersect)), mode)
    feat2, control2 = feat.clone(), control.clone()
    feat2[7, 5] = float("inf")
    feat2[60, 100] = float("nan")
    control2[31] = float("inf")
    want = check_equal(ops, lists((feat2, turn, control2, intersect)), mode)
    others = [i for i in range(100) if i not in (7, 31, 60)]
    for i, (w, c) in enumerate(zip(want, clean)):
        for (_, wr), (_, cr) in zip(w, c):
            bad = (7, 31, 60) if i == 0 else (7, 60)
            for r in bad:
                assert not torch.isfinite(wr[r]).all(), (i, r)
            keep = others + ([31] if i > 0 else [])
            assert torch.equal(bits(wr[keep]), bits(cr[keep])), i


def test_other_problems_are_refused(hip):
    """LGCN_ESHAPE before any launch: the output buffers keep their poison."""
    M, ops = hip
    from lanegcn_amd import _lib as L
    prev = ops.get_mma()
    ops.set_mma("f16x2")
    try:
        a2m = a2m_block(M)
        rows = rows_of(49)
        x = rows[0]
        att = a2m.att[0]
        good = att.v_kw(x)
        rowptr = torch.arange(50, dtype=torch.int32, device="cuda")
        two_rel = dict(good, rels=good["rels"] * 2)
        rng = dict(good, rels=[ops.RelSpec(x, good["rels"][0].wp, L.REL_RANGE)], rowptr=rowptr)
        u = att.u_kw(x)
        bad = {"two relations": two_rel, "a RANGE relation": rng,
               "GN2": dict(u, flags=u["flags"] | L.F_GN2, gn2=u["gn1"]),
               "RES": dict(u, flags=u["flags"] | L.F_RES, res=x),
               "RES on a head": dict(head_kw(a2m, rows, False), flags=L.F_GN1 | L.F_RELU1 | L.F_RES, res=x),
               "ch_wv": dict(head_kw(a2m, rows), chain_v=att.chain_v()),
               "tile_rb": dict(good, tile_rb=2)}
        for name, kw in bad.items():
            assert ops.node_head_form(kw) is None, name
            for kws in ([kw], [good, kw]):
                for held in node_head(ops, kws, expect=ESHAPE):
                    for buf, _ in held:
                        assert untouched(buf), name
            with pytest.raises(L.LgcnError, match=r"code -2"):
                ops.node_head([kw])
        for other in ("bf16x3", "f32"):
            ops.set_mma(other)
            assert not ops.node_head_ok()
            for kw in (att.v_kw(x), att.u_kw(x), head_kw(a2m, rows)):
                for held in node_head(ops, [kw], expect=ESHAPE):
                    for buf, _ in held:
                        assert untouched(buf), other
        ops.set_mma("f16x2")
        assert ops.node_head([dict(att.v_kw(x[:0]))])[0].shape == (0, 128)
    finally:
        ops.set_mma(prev)


def test_att_block_picks_the_launch(hip):
    """att_block takes the new launch once when a `head` produces its targets (A2M), the row block with ops.node_head_ok
    patched to False, in bf16x3 and in f32, and never the new launch without a head (M2A, A2A)."""
    M, ops = hip
    prev = ops.get_mma()
    real_nh, real_multi = ops.node_head, ops.agg_mlp_multi
    calls = []
    try:
        ops.node_head = lambda *a, **k: (calls.append("node_head"), real_nh(*a, **k))[1]
        ops.agg_mlp_multi = lambda *a, **k: (calls.append("agg_mlp_multi"), real_multi(*a, **k))[1]
        g = torch.Generator().manual_seed(5)
        T, S = 97, 20
        tc, sc = (torch.rand(T, 2, generator=g) * 12).cuda(), (torch.rand(S, 2, generator=g) * 12).cuda()
        off = lambda n: torch.tensor([0, n], dtype=torch.int32, device="cuda")
        rows = rows_of(T)
        actors = rows_of(S, seed=7)[0]

        def a2m_run(extra):
            a2m = a2m_block(M)
            ps = ops.pairs_build(tc, off(T), sc, off(S), 4.0, T * S)
            assert 0 < ps.count() < T * S
            del calls[:]
            res = a2m.run(*rows, actors, ps, extra=a2m_block(M, seed=12).att[0].u_kw(actors) if extra else None)
            torch.cuda.synchronize()
            return [c for c in calls], res

        ops.set_mma("f16x2")
        for extra in (False, True):
            took, got = a2m_run(extra)
            assert took == ["node_head"], extra
            ops.node_head_ok, ok = (lambda: False), ops.node_head_ok
            try:
                took, want = a2m_run(extra)
            finally:
                ops.node_head_ok = ok
            assert took == ["agg_mlp_multi"], extra
            for x, y in zip(got if extra else (got,), want if extra else (want,)):
                assert torch.equal(bits(x), bits(y))
        for other in ("bf16x3", "f32"):
            ops.set_mma(other)
            assert a2m_run(True)[0] == ["agg_mlp_multi"], other
        # without a head: M2A (few targets, the nodes as context) and A2A
        ops.set_mma("f16x2")
        atts = a2m_block(M).att
        ps = ops.pairs_build(sc, off(S), tc, off(T), 4.0, T * S)
        del calls[:]
        M.att_block(atts, actors, rows[0], ps)
        ps = ops.pairs_build(sc, off(S), sc, off(S), 6.0, S * S)
        M.att_block(atts, actors, actors, ps, ctx_is_agts=True)
        torch.cuda.synchronize()
        assert "node_head" not in calls and "agg_mlp_multi" in calls
    finally:
        ops.node_head, ops.agg_mlp_multi = real_nh, real_multi
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
    """HotPathEngine.forward on S0: A2M's first launch is the new one (once; the node tail twice, the context heads once);
    with ops.node_head_ok patched to False it is the row block, and nodes, actors and every stage have the same bits."""
    M, ops = hip
    from lanegcn_amd.engine import HotPathEngine
    fb, actors = s0
    torch.manual_seed(21)
    eng = HotPathEngine(*[cls(M.config).cuda().eval() for cls in (M.MapNet, M.A2M, M.M2M, M.M2A, M.A2A)])
    names = ("node_head", "node_tail", "ctx_heads")
    real, ok = {k: getattr(ops, k) for k in names}, ops.node_head_ok
    count = {k: 0 for k in names}

    def counted(k):
        def f(*a, **kw):
            count[k] += 1
            return real[k](*a, **kw)
        return f

    try:
        for k in names:
            setattr(ops, k, counted(k))
        got = eng.forward(fb, actors, stages=True)
        with_it = dict(count)
        ops.node_head_ok = lambda: False
        want = eng.forward(fb, actors, stages=True)
        torch.cuda.synchronize()
        assert with_it == {"node_head": 1, "node_tail": 2, "ctx_heads": 1}
        assert count == {"node_head": 1, "node_tail": 4, "ctx_heads": 2}
        for k in ("nodes", "actors", "a2m", "m2m", "m2a", "a2a"):
            assert torch.equal(bits(got[k]), bits(want[k])), k
        assert bool(torch.isfinite(want["actors"]).all()) and float(want["actors"].abs().max()) > 0
    finally:
        for k in names:
            setattr(ops, k, real[k])
        ops.node_head_ok = ok
