"""GPU: the forward kernels over OPERAND SCALE, every matrix mode against float64, each held to a model of its own format.

Every other GPU test draws weights from oracle.seeded_state (std 0.13 at K = 128) and O(1) activations, so none of them
moves the one quantity the split-precision formats are sensitive to.  f16x2 rounds both operands to two fp16 planes: below
fp16's normal range (6.1e-5) the second plane, then the first, runs out of bits, and the error against fp32 grows from
1e-7 to 6e-3 at max |W| = 8e-6.  That is the format, not a bug, so a flat 1e-4 cannot be the bar here.  Instead
(tests/split_model.py) the same formulas are evaluated in float64 with the operands rounded exactly where the kernel rounds
them, and every kernel, tensor and mode must satisfy

    rel_err(kernel, fp64) <= max(2 rel_err(model, fp64), 1e-6)          rel_err = max |got - ref| / max |ref|

(split_model.bar; the project's 1e-4 clamp holds where the model itself stays under 5e-5).  A flushed subnormal plane, a
pack kernel that rounds differently from split_store, or a dropped product shows as a kernel far above its model.

Scales are exact powers of two applied to one fixed seeded draw: s_x to the rows a GEMM reads (for the stages that form
their rows from [n, 2] inputs -- att_pairs, mapnet_input -- to those inputs and the first layer's bias, which scales the
rows exactly), s_w to every 128-wide weight (and, for att_pairs, to U and V).
  f16x2:        s_w in 2^{4, 0, -4, -8, -12, -16} at s_x = 1;  s_x in 2^{12, -8, -14} at s_w = 1
  bf16x3, f32:  (s_x, s_w) = (2^-100, 2^80), (2^60, 2^40), (2^-8, 2^-8)
  bf16:         the same three -- one bf16 plane, one product (Fmt<2>): fp32's exponent range at 8 significand bits, so
                its model stands at 1e-3 .. 5e-3 whatever the scale, and the bar is twice that
Rows: n = 1, 33, 130 (a single row, a ragged second tile, several tiles).  Each case prints, per tensor, the model's and the
kernel's error before anything is asserted.

At (2^60, 2^40) and (2^-100, 2^80) the values that reach a GroupNorm are ~2^100 / ~2^80 and their squares leave fp32: these
cases are what row_gn's wide path (csrc/lgcn_tile.hpp: row_rstd_wide) exists for -- without it the rows come out as beta
(error 0.3 .. 1 against float64), in every mode whose operands have fp32's exponent range: f32, bf16x3 and bf16.
Measured figures: DESIGN.md section 5c.
"""
import functools
import types

import numpy as np
import pytest
import torch

import split_model as S

pytestmark = pytest.mark.gpu

C = 128
EPS = 1e-5
ROWS = (1, 33, 130)
F16_GRID = [(0, 4), (0, 0), (0, -4), (0, -8), (0, -12), (0, -16), (12, 0), (-8, 0), (-14, 0)]
WIDE_GRID = [(-100, 80), (60, 40), (-8, -8)]
CASES = [("f16x2", ex, ew) for ex, ew in F16_GRID] + [(m, ex, ew) for m in ("bf16x3", "f32") for ex, ew in WIDE_GRID]
CASES += [("bf16", ex, ew) for ex, ew in WIDE_GRID]
IDS = ["%s-x2^%d-w2^%d" % c for c in CASES]
T_AGT, S_CTX, P_PAIRS = 9, 11, 33


@pytest.fixture(scope="module")
def mods():
    import lanegcn_amd  # noqa: F401
    from lanegcn_amd import _lib as L
    from lanegcn_amd import lanegcn as M
    from lanegcn_amd import ops
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return M, ops, L


def p2(t, e):
    """t * 2^e in fp32, exactly (no underflow, no overflow)."""
    out = torch.ldexp(t, torch.tensor(e))
    assert out.dtype == torch.float32 and torch.equal(out.double(), torch.ldexp(t.double(), torch.tensor(e)))
    return out


@functools.lru_cache(maxsize=None)
def draw():
    """The one seeded draw every case scales (CPU fp32).  Matrices as oracle.seeded_state makes them: N(0, 1 / fan_in) * 1.5."""
    g = torch.Generator().manual_seed(20260)
    n = max(ROWS)
    rn = lambda *s: torch.randn(*s, generator=g)
    mat = lambda o, i: rn(o, i) * (1.5 / i ** 0.5)
    gnp = lambda: (1 + 0.1 * rn(C), 0.1 * rn(C))
    d = dict(x=rn(n, C).relu(), w=[mat(C, C) for _ in range(4)], w384=mat(C, 3 * C), w2=mat(C, C), gn1=gnp(), gn2=gnp(),
             xy=[rn(n, 2), rn(n, 2)], w1=[mat(C, 2), mat(C, 2)], b1=[0.1 * rn(C), 0.1 * rn(C)],
             agt=rn(T_AGT, 2), ctx=rn(S_CTX, 2), U=rn(T_AGT, C), V=rn(S_CTX, C))
    return d


@functools.lru_cache(maxsize=None)
def multigraph(n, n_rel):
    """n_rel relations of 2 n random edges on n nodes: duplicates, rows without an edge, in-degree up to ~7."""
    rng = np.random.default_rng(100 + n)
    return [(torch.from_numpy(rng.integers(0, n, 2 * n)), torch.from_numpy(rng.integers(0, n, 2 * n))) for _ in range(n_rel)]


class Report:
    """Prints every figure, asserts at the end: one failing tensor does not hide the others' figures."""

    def __init__(self, entry, mode, ex, ew):
        self.head = "OPSCALE %s %s x2^%d w2^%d" % (entry, mode, ex, ew)
        self.bad = []

    def check(self, what, got, model, ref):
        got = got.detach().cpu().numpy().astype(np.float64)
        assert np.isfinite(ref).all() and np.isfinite(model).all(), "the case itself left the format's range: " + what
        e_m, e_k = S.rel_err(model, ref), S.rel_err(got, ref)
        b = S.bar(e_m)
        print("\n%s %s: model %.3e kernel %.3e bar %.3e" % (self.head, what, e_m, e_k, b), end="")
        if not e_k <= b:                      # a NaN fails
            self.bad.append((what, e_m, e_k, b))

    def done(self):
        assert not self.bad, "%s (tensor, model, kernel, bar): %s" % (self.head, self.bad)


def dev(t):
    return t.cuda()


# ------------------------------------------------------------------ the row block
@pytest.mark.parametrize("mode,ex,ew", CASES, ids=IDS)
@pytest.mark.parametrize("shape", ["ident", "block", "csr"])
def test_agg_mlp_plain(mods, shape, mode, ex, ew):
    """flags 0: one IDENT relation; a 128-column block of a [128, 384] weight; IDENT + two CSR relations (the gathered
    fp32 sum is what gets split)."""
    M, ops, L = mods
    d = draw()
    rep = Report("agg_mlp." + shape, mode, ex, ew)
    w384 = p2(d["w384"], ew)
    ws = [p2(w, ew) for w in d["w"][:3]]
    w384_d, ws_d = dev(w384), [dev(w) for w in ws]
    for n in ROWS:
        x = p2(d["x"][:n], ex).contiguous()
        x_d = dev(x)
        with ops.mma_scope(mode):
            if shape == "ident":
                rels = [(x, ws[0], None)]
                got = ops.agg_mlp(n, [ops.RelSpec(x_d, ops.packed(ws_d[0]), L.REL_IDENT)], 0)
            elif shape == "block":
                rels = [(x, w384[:, C:2 * C], None)]
                got = ops.agg_mlp(n, [ops.RelSpec(x_d, ops.packed(w384_d, C, C), L.REL_IDENT)], 0)
            else:
                edges = multigraph(n, 2)
                rels = [(x, ws[0], None), (x, ws[1], edges[0]), (x, ws[2], edges[1])]
                plan = ops.csr_build([dev(u) for u, _ in edges], [dev(v) for _, v in edges], n)
                got = ops.agg_mlp(n, [ops.RelSpec(x_d, ops.packed(ws_d[0]), L.REL_IDENT),
                                      ops.RelSpec(x_d, ops.packed(ws_d[1]), L.REL_CSR, 0),
                                      ops.RelSpec(x_d, ops.packed(ws_d[2]), L.REL_CSR, 1)], 0,
                                  rowptr=plan.rowptr, col=plan.col, n_rel_csr=2)
        rep.check("n=%d out" % n, got, S.row_block(n, rels, mode)["out"], S.row_block(n, rels, mode, model=False)["out"])
    rep.done()


@pytest.mark.parametrize("mode,ex,ew", CASES, ids=IDS)
def test_agg_mlp_two_stage(mods, mode, ex, ew):
    """F_GN1 | F_RELU1 | F_GEMM2: the stage-1 sums, the stage-2 operand and the output."""
    M, ops, L = mods
    d = draw()
    rep = Report("agg_mlp.gn_gemm2", mode, ex, ew)
    w1, w2, gn1 = p2(d["w"][0], ew), p2(d["w2"], ew), d["gn1"]
    w1_d, w2_d, gn1_d = dev(w1), dev(w2), tuple(dev(t) for t in gn1)
    for n in ROWS:
        x = p2(d["x"][:n], ex).contiguous()
        pre, mid = (torch.empty(n, C, device="cuda") for _ in range(2))
        with ops.mma_scope(mode):
            out = ops.agg_mlp(n, [ops.RelSpec(dev(x), ops.packed(w1_d), L.REL_IDENT)], L.F_GN1 | L.F_RELU1 | L.F_GEMM2,
                              gn1=gn1_d, wp2=ops.packed(w2_d), out_pre=pre, out_mid=mid)
        kw = dict(gn1=gn1, relu1=True, w2=w2)
        model, ref = S.row_block(n, [(x, w1, None)], mode, **kw), S.row_block(n, [(x, w1, None)], mode, model=False, **kw)
        for name, got in (("pre", pre), ("mid", mid), ("out", out)):
            rep.check("n=%d out_%s" % (n, name) if name != "out" else "n=%d out" % n, got, model[name], ref[name])
    rep.done()


# ------------------------------------------------------------------ LaneConv
@pytest.mark.parametrize("mode,ex,ew", CASES, ids=IDS)
@pytest.mark.parametrize("impl", ["tiled", "fused"])
def test_laneconv_layer(mods, impl, mode, ex, ew):
    """One LaneConv layer through the package's dispatcher (lanegcn.lane_conv) under both set_laneconv_impl values:
    lgcn_laneconv_fwd where the mode has it (f16x2, "tiled"), the one-launch lgcn_agg_mlp layer otherwise.  Relations
    pre0, suc0, left with edges, right without."""
    M, ops, L = mods
    d = draw()
    rep = Report("laneconv." + impl, mode, ex, ew)
    ws = [p2(w, ew) for w in d["w"]]
    w2 = p2(d["w2"], ew)
    ns = types.SimpleNamespace
    mod = lambda w: [ns(weight=dev(w))]
    fuse = {"ctr": mod(ws[0]), "pre0": mod(ws[1]), "suc0": mod(ws[2]), "left": mod(ws[3]), "right": mod(ws[3]),
            "norm": [ns(weight=dev(d["gn1"][0]), bias=dev(d["gn1"][1]), eps=EPS)],
            "ctr2": [ns(linear=ns(weight=dev(w2)), norm=ns(weight=dev(d["gn2"][0]), bias=dev(d["gn2"][1])))]}
    empty = torch.zeros(0, dtype=torch.int64)
    prev = ops.laneconv_impl()
    ops.set_laneconv_impl(impl)
    try:
        for n in ROWS:
            x = p2(d["x"][:n], ex).contiguous()
            edges = multigraph(n, 3)
            us, vs = [u for u, _ in edges] + [empty], [v for _, v in edges] + [empty]
            with ops.mma_scope(mode), torch.no_grad():
                plan = ops.csr_build([dev(u) for u in us], [dev(v) for v in vs], n)
                got = M.lane_conv(fuse, dev(x), plan, 1)
            units = [(ws[0], None)] + [(ws[1 + r], edges[r]) for r in range(3)]
            rep.check("n=%d out" % n, got, S.lane_conv(x, units, d["gn1"], w2, d["gn2"], mode),
                      S.lane_conv(x, units, d["gn1"], w2, d["gn2"], mode, model=False))
    finally:
        ops.set_laneconv_impl(prev)
    rep.done()


# ------------------------------------------------------------------ Att's pair stage
def pair_set(ops, agt, ctx):
    """33 pairs by hand: hi sorted over 7 of the 9 targets (a segment straddles pair 16 and pair 32), wi arbitrary over 9 of
    the 11 context rows; 7 spare rows of capacity."""
    g = torch.Generator().manual_seed(33)
    targets, contexts = (0, 1, 2, 4, 5, 6, 8), (0, 1, 3, 4, 5, 6, 7, 8, 10)
    hi = torch.tensor([targets[p * len(targets) // P_PAIRS] for p in range(P_PAIRS)])
    wi = torch.tensor(contexts)[torch.randint(len(contexts), (P_PAIRS,), generator=g)]
    cap = P_PAIRS + 7
    pad = torch.zeros(cap - P_PAIRS, dtype=torch.int64)
    rowptr = torch.zeros(T_AGT + 1, dtype=torch.int64)
    rowptr[1:] = torch.cumsum(torch.bincount(hi, minlength=T_AGT), 0)
    i32 = lambda t: t.to(torch.int32).cuda()
    ps = ops.PairSet(i32(torch.cat([hi, pad])), i32(torch.cat([wi, pad])), i32(torch.tensor([P_PAIRS])), i32(rowptr), cap, T_AGT,
                     dev(agt), dev(ctx))
    return ps, hi, wi


ATT_IMPLS = {"f32": ["stream"], "bf16x3": ["ws"], "f16x2": ["wi", "ws"], "bf16": ["wi", "ws"]}


@pytest.mark.parametrize("mode,ex,ew", CASES, ids=IDS)
def test_att_pairs(mods, mode, ex, ew):
    """lgcn_att_pairs (f32, "stream"), lgcn_att_pairs_ws (bf16x3; f16x2 and bf16 "ws") and lgcn_att_pairs_wi (f16x2 and
    bf16 "wi": the K-permuted images of packed_kperm), P = 33."""
    M, ops, L = mods
    d = draw()
    agt, ctx, bd0 = p2(d["agt"], ex), p2(d["ctx"], ex), p2(d["b1"][0], ex)
    w_d2, w_c0, U, V = p2(d["w"][0], ew), p2(d["w384"], ew), p2(d["U"], ew), p2(d["V"], ew)
    wd0, gn_d, gn_c = d["w1"][0], d["gn1"], d["gn2"]
    ps, hi, wi = pair_set(ops, agt, ctx)
    args = (agt, ctx, hi, wi, wd0, bd0, w_d2, gn_d, w_c0[:, :C], U, V, gn_c)
    model, ref = S.att_pairs(*args, mode), S.att_pairs(*args, mode, model=False)
    w_d2_d, w_c0_d = dev(w_d2), dev(w_c0)
    gd, gc = tuple(dev(t) for t in gn_d), tuple(dev(t) for t in gn_c)
    prev = ops._att_pairs_impl
    bad = []
    try:
        for impl in ATT_IMPLS[mode]:
            rep = Report("att_pairs." + impl, mode, ex, ew)
            if impl != "stream":
                ops.set_att_pairs_impl(impl)
            with ops.mma_scope(mode):
                assert ops.att_pairs_impl() == impl
                m = ops.att_pairs(ps, dev(wd0), dev(bd0), (w_d2_d, 0), gd, (w_c0_d, 0), dev(U), dev(V), gc)
            rep.check("P=%d m" % P_PAIRS, m[:P_PAIRS], model, ref)
            bad += [(rep.head,) + b for b in rep.bad]
    finally:
        ops.set_att_pairs_impl(prev)
    assert not bad, "(case, tensor, model, kernel, bar): %s" % bad


# ------------------------------------------------------------------ MapNet's input stage
@pytest.mark.parametrize("mode,ex,ew", CASES, ids=IDS)
def test_mapnet_input(mods, mode, ex, ew):
    M, ops, L = mods
    d = draw()
    rep = Report("mapnet_input", mode, ex, ew)
    wa2, ws2 = p2(d["w"][0], ew), p2(d["w"][1], ew)
    ba1, bs1 = p2(d["b1"][0], ex), p2(d["b1"][1], ex)
    wa1, ws1 = d["w1"]
    wa2_d, ws2_d = dev(wa2), dev(ws2)
    for n in ROWS:
        ctrs, feats = p2(d["xy"][0][:n], ex).contiguous(), p2(d["xy"][1][:n], ex).contiguous()
        with ops.mma_scope(mode):
            got = ops.mapnet_input(dev(ctrs), dev(feats), dev(wa1), dev(ba1), ops.packed(wa2_d), tuple(dev(t) for t in d["gn1"]),
                                   dev(ws1), dev(bs1), ops.packed(ws2_d), tuple(dev(t) for t in d["gn2"]))
        args = (ctrs, feats, wa1, ba1, wa2, d["gn1"], ws1, bs1, ws2, d["gn2"])
        rep.check("n=%d out" % n, got, S.mapnet_input(*args, mode), S.mapnet_input(*args, mode, model=False))
    rep.done()


# ------------------------------------------------------------------ ActorNet's conv units
CONV_SHAPES = [(3, 32, 3, 1), (32, 64, 3, 2), (128, 128, 1, 1)]          # cin, cout, k, stride; A = 5, L = 20


@functools.lru_cache(maxsize=None)
def conv_draw(shape):
    cin, cout, ks, _ = shape
    g = torch.Generator().manual_seed(7 * cin + cout)
    return (torch.randn(5, 20, cin, generator=g), torch.randn(cout, cin, ks, generator=g) * (1.5 / (cin * ks) ** 0.5),
            1 + 0.1 * torch.randn(cout, generator=g), 0.1 * torch.randn(cout, generator=g))


@pytest.mark.parametrize("ex,ew", F16_GRID, ids=["x2^%d-w2^%d" % c for c in F16_GRID])
@pytest.mark.parametrize("shape", CONV_SHAPES, ids=["%d-%d-k%d-s%d" % s for s in CONV_SHAPES])
def test_conv1d_unit(mods, shape, ex, ew):
    """lgcn_conv1d_gn_train: the two-plane units (exact=False) against the f16x2 model, the exact units (exact=True) at the
    floor at every scale; y (the convolution) and out (behind the GroupNorm over the actor's lout x cout values).
    The conv units take no matrix mode: ops.conv1d_gn / conv1d_gn_train run lgcn_conv1d_gn (two fp16 planes) or, with
    exact=True, lgcn_conv1d_gn_f32 whatever ops.set_mma() says, and no bf16 product is ever formed here -- so "bf16" adds
    no case to this test."""
    M, ops, L = mods
    x0, w0, gamma, beta = conv_draw(shape)
    x, w, stride = p2(x0, ex), p2(w0, ew), shape[3]
    ref_out, ref_y = S.conv1d_unit(x, w, stride, gamma, beta, "f32", model=False)
    bad = []
    for exact, mode in ((False, "f16x2"), (True, "f32")):
        rep = Report("conv1d.%s.%s" % ("exact" if exact else "planes", "%d-%d-k%d-s%d" % shape), mode, ex, ew)
        out, y = ops.conv1d_gn_train(dev(x), dev(w), stride, dev(gamma), dev(beta), EPS, exact=exact)
        m_out, m_y = S.conv1d_unit(x, w, stride, gamma, beta, mode)
        rep.check("y", y, m_y, ref_y)
        rep.check("out", out, m_out, ref_out)
        if exact:
            assert S.bar(S.rel_err(m_out, ref_out)) == 1e-6 and S.bar(S.rel_err(m_y, ref_y)) == 1e-6      # the floor
        bad += [(rep.head,) + b for b in rep.bad]
    assert not bad, "(case, tensor, model, kernel, bar): %s" % bad


# ------------------------------------------------------------------ the upper edge of f16x2
@pytest.mark.parametrize("where", ["x", "w"])
def test_f16x2_upper_edge(mods, where):
    """65504 (fp16's largest number) and 65519 (the largest fp32 value that still rounds to it; the second plane takes the
    15) are ordinary operands; 65520 rounds to fp16's infinity, the residual to -infinity, and everything that element
    touches is NaN -- which lgcn_check_finite reports."""
    M, ops, L = mods
    d = draw()
    n, row, k, ch = 33, 7, 3, 5
    for v in (65504.0, 65519.0, 65520.0):
        x, w = d["x"][:n].clone(), d["w"][0].clone()
        if where == "x":
            x[row, k] = v
        else:
            w[ch, k] = v
        w_d = dev(w)
        with ops.mma_scope("f16x2"):
            got = ops.agg_mlp(n, [ops.RelSpec(dev(x), ops.packed(w_d), L.REL_IDENT)], 0)
        flag = torch.zeros(1, dtype=torch.int32, device="cuda")
        ops.check_finite(flag, got)
        got = got.cpu()
        print("\nOPSCALE edge %s = %.0f: flag %d, non-finite %d of %d" % (where, v, int(flag.item()), int((~torch.isfinite(got)).sum()),
                                                                       got.numel()))
        if v < 65520.0:
            rep = Report("edge.%s=%.0f" % (where, v), "f16x2", 0, 0)
            rep.check("n=%d out" % n, got, S.row_block(n, [(x, w, None)], "f16x2")["out"],
                      S.row_block(n, [(x, w, None)], "f16x2", model=False)["out"])
            rep.done()
            assert int(flag.item()) == 0
        else:
            hit = torch.zeros(n, C, dtype=torch.bool)
            if where == "x":
                hit[row, :] = True
            else:
                hit[:, ch] = True
            assert torch.isnan(got[hit]).all() and torch.isfinite(got[~hit]).all()
            assert np.isnan(S.row_block(n, [(x, w, None)], "f16x2")["out"][hit.numpy()]).all()      # the model agrees
            assert int(flag.item()) == 1
