"""GPU: the context-heads launch (ops.ctx_heads / lgcn_ctx_heads) against the row block it replaces, bit for bit, and the
engine's forward that uses it (M2A starts with it, M2A's U of layer 0 rides in A2M's first launch) against the per-layer
route, eagerly and replayed from a captured graph."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ROWS = (1, 16, 47, 48, 49, 96, 100, 337)      # below / at / past one 48-row tile, ragged last tiles, several workgroups
PAD = 64                                       # poisoned rows in front of and behind every output
POISON = 0x7fc0dead                            # a NaN pattern no kernel writes


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


def check_against_row_block(M, ops, x, n_w, tag):
    """ops.ctx_heads(x, n_w weights of n_w different Att layers) == ops.agg_mlp(**att.v_kw(x)) as int32, and nothing is
    written outside the outputs' rows."""
    torch.manual_seed(11)
    atts = [M.Att(128, 128).cuda().eval() for _ in range(n_w)]
    n = x.shape[0]
    want = [ops.agg_mlp(**a.v_kw(x)) for a in atts]
    if n_w == 2:
        assert not torch.equal(want[0], want[1]), "the two weights must differ"
    held = [poisoned(n) for _ in range(n_w)]
    got = ops.ctx_heads(x, [a.chain_v() for a in atts], outs=[v for _, v in held])
    torch.cuda.synchronize()
    for j in range(n_w):
        assert got[j].data_ptr() == held[j][1].data_ptr()
        assert torch.equal(bits(got[j]), bits(want[j])), (tag, n, n_w, j)
        buf = bits(held[j][0])
        assert bool((buf[:PAD] == POISON).all()) and bool((buf[PAD + n:] == POISON).all()), (tag, n, n_w, j, "wrote outside its rows")
    return want


@pytest.mark.parametrize("mode", ["f16x2", "bf16"], indirect=True)
@pytest.mark.parametrize("n_w", [1, 2])
@pytest.mark.parametrize("n_rows", ROWS)
def test_equals_the_row_block_bit_for_bit(hip, mode, n_w, n_rows):
    M, ops = hip
    g = torch.Generator().manual_seed(100 + n_rows)
    x = torch.randn(n_rows, 128, generator=g).cuda()
    check_against_row_block(M, ops, x, n_w, mode)
    # allocated by the wrapper: same values
    torch.manual_seed(11)
    atts = [M.Att(128, 128).cuda().eval() for _ in range(n_w)]
    got = ops.ctx_heads(x, [a.chain_v() for a in atts])
    for a, o in zip(atts, got):
        assert o.shape == (n_rows, 128) and torch.equal(bits(o), bits(ops.agg_mlp(**a.v_kw(x))))


@pytest.mark.parametrize("mode", ["f16x2", "bf16"], indirect=True)
def test_inf_and_nan_rows_come_out_as_the_row_block_gives_them(hip, mode):
    M, ops = hip
    g = torch.Generator().manual_seed(3)
    x = torch.randn(100, 128, generator=g)
    x[7, 5] = float("inf")
    x[60, 100] = float("nan")
    want = check_against_row_block(M, ops, x.cuda(), 2, mode)
    for w in want:
        assert not torch.isfinite(w[7]).all() and torch.isnan(w[60]).all()       # the rows are really special
        assert torch.isfinite(w[8:60]).all()


@pytest.mark.parametrize("mode", ["bf16x3", "f32"], indirect=True)
def test_other_modes_are_refused(hip, mode):
    M, ops = hip
    from lanegcn_amd import _lib as L
    att = M.Att(128, 128).cuda().eval()
    x = torch.randn(49, 128).cuda()
    assert not ops.ctx_heads_ok()
    with pytest.raises(L.LgcnError, match=r"code -2"):      # LGCN_ESHAPE
        ops.ctx_heads(x, [att.chain_v()])


def test_empty_problem_is_a_no_op(hip):
    M, ops = hip
    att = M.Att(128, 128).cuda().eval()
    out = ops.ctx_heads(torch.empty(0, 128, device="cuda"), [att.chain_v()])
    assert out[0].shape == (0, 128)


# ------------------------------------------------------------------ through the engine
@pytest.fixture(scope="module")
def s0(hip):
    from lanegcn_amd import data as gen
    from lanegcn_amd.engine import collate_flat
    scenes = gen.synth_batch("S0", seed=3)
    fb = collate_flat(scenes)
    actors = torch.from_numpy(np.random.default_rng(5).normal(0, 1, (fb.n_actors, 128)).astype(np.float32)).relu().cuda()
    return fb, actors


def engine(M, seed=21):
    from lanegcn_amd.engine import HotPathEngine
    torch.manual_seed(seed)
    mods = [cls(M.config).cuda().eval() for cls in (M.MapNet, M.A2M, M.M2M, M.M2A, M.A2A)]
    return HotPathEngine(*mods)


@pytest.mark.parametrize("mode", ["f16x2", "bf16"], indirect=True)
def test_forward_equals_the_per_layer_route_eager_and_captured(hip, s0, mode):
    """HotPathEngine.forward on S0 (ctx-heads launch in M2A, M2A's U0 in A2M's first launch) against Att.fold = False, bit for
    bit on nodes and actors; the same forward captured in a graph and replayed twice gives the same bits."""
    M, ops = hip
    fb, actors = s0
    eng = engine(M)
    launches = []
    real = ops.ctx_heads
    prev = M.Att.fold
    try:
        ops.ctx_heads = lambda *a, **k: (launches.append(1), real(*a, **k))[1]
        M.Att.fold = True
        got = eng.forward(fb, actors, stages=True)
        n_folded = len(launches)
        M.Att.fold = False
        want = eng.forward(fb, actors, stages=True)
        assert n_folded == 1 and len(launches) == 1      # once per folded forward, never on the per-layer route
        M.Att.fold = True
        torch.cuda.synchronize()
        for k in ("nodes", "actors", "a2m", "m2m", "m2a", "a2a"):
            assert torch.equal(bits(got[k]), bits(want[k])), k
        assert bool(torch.isfinite(want["actors"]).all()) and float(want["actors"].abs().max()) > 0
        graph, out = eng.capture(fb, actors)
        for r in range(2):
            out["nodes"].zero_()
            out["actors"].zero_()
            graph.replay()
            torch.cuda.synchronize()
            for k in ("nodes", "actors"):
                assert torch.equal(bits(out[k]), bits(want[k])), ("replay", r, k)
    finally:
        ops.ctx_heads = real
        M.Att.fold = prev


def test_stage_functions_mirror_the_forward(hip, s0):
    """The per-stage cut used for measurement: the a2m stage emits M2A's U0, the m2a stage starts with the ctx-heads launch,
    and the stages give the forward's bits."""
    M, ops = hip
    fb, actors = s0
    prev = ops.get_mma()
    ops.set_mma("f16x2")
    try:
        eng = engine(M)
        want = eng.forward(fb, actors, stages=True)
        st, fns = eng.stage_functions(fb, actors)
        for _, fn in fns:
            fn()
        torch.cuda.synchronize()
        assert st["u_m2a"] is not None and st["u_m2a"].shape == (fb.n_actors, 128)
        assert torch.equal(bits(st["u_m2a"]), bits(ops.agg_mlp(**eng.m2a.att[0].u_kw(actors))))
        for k, s in (("a2m", "nodes_a2m"), ("m2m", "nodes_m2m"), ("m2a", "actors_m2a"), ("a2a", "actors_a2a")):
            assert torch.equal(bits(st[s]), bits(want[k])), k
    finally:
        ops.set_mma(prev)
