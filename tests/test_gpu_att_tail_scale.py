"""GPU: the Att tail roles over OPERAND SCALE, every matrix mode against float64, each held to the model of its own format.

tests/test_gpu_operand_scale.py holds the row block to float64 with flags 0 and with GN1 | RELU1 | GEMM2, over IDENT and
CSR gathers.  The roles an Att layer ends in were compared bit for bit with each other only (test_gpu_node_tail,
test_gpu_ctx_heads), on N(0, 1) rows and nn.Linear-default weights -- which says nothing where the row block itself is
wrong.  Here, on the problem of tests/att_tail_cases.py (T = 1, 49, 130 targets; 0, 1, 2, 3, 6, 9 and 40 pairs per target;
s_x on the target and pair rows, s_w on every weight, the residual rows a separate O(1) draw):

  1. the tail on the row block: ops.agg_mlp over [IDENT(a, W_agt), RANGE(m, W_c1)] with every flag -- plain, with the
     chained U, with the chained V, with both -- and the same through LGCN_REL_RANGE16 (only the first row of every
     16-aligned piece of a segment holds data; the other rows are NaN here and must not be read);
  2. ops.node_tail (f16x2 / bf16), plain and with the chained U;
  3. ops.ctx_heads (f16x2 / bf16), one and two weights over the same rows;
  4. the head pair ops.agg_mlp_pair(u_kw, v_kw).

Modes and scales: f16x2 on F16_GRID; bf16x3, f32 and the single-product bf16 on WIDE_GRID.  Every tensor of every role must
satisfy split_model.bar -- rel_err(kernel, fp64) <= max(2 rel_err(model, fp64), 1e-6) -- and prints model / kernel / bar
before anything is asserted.  At (2^60, 2^40) the stage-1 sums are ~2^100 and their squares leave fp32: a GroupNorm without
row_rstd_wide returns beta there (0.3 .. 0.8 against float64; the residual is O(1) so that this shows).

The bar cannot tell a truncating operand split from a rounding one (1.14 x in bf16).  test_flags0_elementwise can: where a
kernel's output is nothing but an fp32 accumulation of exact products of 16-bit planes (flags 0: agg_mlp ident / block /
csr / range, ctx_heads; 8 + 8 or 11 + 11 significand bits fit fp32), the model is the same sum in float64 and

    |kernel - model| <= 2 K NPROD 2^-24 sum_products |A_p| |B_q|^T       K = 128, elementwise

(the textbook accumulation bound, times 2 for an accumulator that truncates; a gathered fan-in is absorbed by the fp32
pre-sum, which the model forms in the kernels' order).  The bound is ~2e-3 (bf16) / ~6e-3 (f16x2) of a mean term
|a| |b|; the kernels measure 3e-3 .. 2e-2 of it.  A split that truncated where split_store rounds would move bf16 outputs by
~sqrt(128) 2^-9 of a term, ten times the bound; a swapped or missing main plane far more.  (What it cannot see: a dropped
cross product of f16x2, 2^-11 of a term, lands at about half the bound -- the 2 x bar sees that one, as 2^-11 against a
model at 2^-22.)  Cases with |ex|, |ew| <= 16 only: beyond, plane products approach fp32's subnormals.
Measured figures: DESIGN.md section 5c."""
import numpy as np
import pytest
import torch

import att_tail_cases as A
import split_model as S
from test_gpu_operand_scale import F16_GRID, WIDE_GRID, Report, draw, multigraph, p2  # noqa: F401  (the grids: A.CASES)

pytestmark = pytest.mark.gpu

C = 128
EPS = 1e-5
FAST = ("f16x2", "bf16")                                   # the modes lgcn_node_tail / lgcn_ctx_heads implement
FAST_CASES = [c for c in A.CASES if c[0] in FAST]
SPLIT_SMALL = [c for c in A.CASES if c[0] != "f32" and abs(c[1]) <= 16 and abs(c[2]) <= 16]
ids = lambda cases: ["%s-x2^%d-w2^%d" % c for c in cases]
CHAINS = {"plain": (False, False), "u": (True, False), "v": (False, True), "uv": (True, True)}


@pytest.fixture(scope="module")
def mods():
    import lanegcn_amd  # noqa: F401
    from lanegcn_amd import _lib as L
    from lanegcn_amd import ops
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return ops, L


def full(L):
    return L.F_GN1 | L.F_RELU1 | L.F_GEMM2 | L.F_GN2 | L.F_RES | L.F_RELU2


class Dev:
    """A problem's tensors on the device; weights packed for the matrix mode in force (call inside ops.mma_scope)."""

    def __init__(self, ops, c):
        self.ops, self.c = ops, c
        self.t = {k: c[k].cuda() for k in ("a", "m", "m16", "res", "rowptr") + A.WEIGHTS}
        self.gn = {k: tuple(t.cuda() for t in c[k]) for k in ("gn1", "gn2", "gq")}

    def wp(self, name):
        return self.ops.packed(self.t[name])

    def tail(self, L, entry, rel, chain_u, chain_v):
        ops, t = self.ops, self.t
        rels = [ops.RelSpec(t["a"], self.wp("w_agt"), L.REL_IDENT), ops.RelSpec(t["m16" if rel == L.REL_RANGE16 else "m"], self.wp("w_c1"), rel)]
        kw = dict(rowptr=t["rowptr"], gn1=self.gn["gn1"], wp2=self.wp("w2"), gn2=self.gn["gn2"], res=t["res"], eps=EPS,
                  chain_u=(self.wp("wq"), self.gn["gq"], self.wp("wu")) if chain_u else None)
        if chain_v:
            kw["chain_v"] = self.wp("wv")
        got = entry(self.c["T"], rels, full(L), **kw)
        names = ["out"] + ["U"] * chain_u + ["V"] * chain_v
        return dict(zip(names, got if isinstance(got, tuple) else (got,)))


# ------------------------------------------------------------------ 1. the tail on the row block
@pytest.mark.parametrize("mode,ex,ew", A.CASES, ids=A.IDS)
@pytest.mark.parametrize("rel", ["range", "range16"])
def test_tail_on_the_row_block(mods, rel, mode, ex, ew):
    ops, L = mods
    rep = Report("att_tail.agg_mlp." + rel, mode, ex, ew)
    rel16 = rel == "range16"
    for T in A.ROWS:
        c = A.problem(mode, ex, ew, T)
        model, ref = A.tail(mode, ex, ew, T, True, rel16), A.tail(mode, ex, ew, T, False)
        with ops.mma_scope(mode):
            d = Dev(ops, c)
            if rel16 and mode == "f32":                   # piece sums exist in the 16-bit-plane modes only (lgcn.h)
                with pytest.raises(L.LgcnError, match=r"code -2"):
                    d.tail(L, ops.agg_mlp, L.REL_RANGE16, False, False)
                continue
            for name, (cu, cv) in CHAINS.items():
                got = d.tail(L, ops.agg_mlp, L.REL_RANGE16 if rel16 else L.REL_RANGE, cu, cv)
                for k, v in got.items():
                    rep.check("T=%d %s %s" % (T, name, k), v, model[k], ref[k])
    rep.done()


# ------------------------------------------------------------------ 2. the weight-stationary tail
@pytest.mark.parametrize("mode,ex,ew", FAST_CASES, ids=ids(FAST_CASES))
def test_node_tail(mods, mode, ex, ew):
    ops, L = mods
    rep = Report("att_tail.node_tail", mode, ex, ew)
    for T in A.ROWS:
        c = A.problem(mode, ex, ew, T)
        model, ref = A.tail(mode, ex, ew, T), A.tail(mode, ex, ew, T, False)
        with ops.mma_scope(mode):
            assert ops.node_tail_ok()
            d = Dev(ops, c)
            for name in ("plain", "u"):
                for k, v in d.tail(L, ops.node_tail, L.REL_RANGE, name == "u", False).items():
                    rep.check("T=%d %s %s" % (T, name, k), v, model[k], ref[k])
    rep.done()


# ------------------------------------------------------------------ 3. the context heads
def check_elementwise(bad, head, got, model, bound):
    """|kernel - model| <= bound, elementwise; prints the largest ratio first."""
    got = got.detach().cpu().numpy().astype(np.float64)
    assert np.isfinite(model).all() and np.isfinite(bound).all() and got.shape == model.shape == bound.shape
    diff = np.abs(got - model)
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = np.where(bound > 0, diff / bound, np.where(diff > 0, np.inf, 0.0))
    worst = float(ratio.max()) if np.isfinite(got).all() else float("nan")
    print("\n%s: max |kernel - model| / bound %.3e  (max |model| %.3e, elements over %d of %d)"
          % (head, worst, np.abs(model).max(), int((ratio > 1).sum()), ratio.size), end="")
    if not worst <= 1.0:
        bad.append((head, worst))


@pytest.mark.parametrize("mode,ex,ew", FAST_CASES, ids=ids(FAST_CASES))
def test_ctx_heads(mods, mode, ex, ew):
    """One and two weights over the same rows, against the model and float64."""
    ops, L = mods
    rep = Report("att_tail.ctx_heads", mode, ex, ew)
    for T in A.ROWS:
        c = A.problem(mode, ex, ew, T)
        with ops.mma_scope(mode):
            assert ops.ctx_heads_ok()
            d = Dev(ops, c)
            for names in (("wv",), ("wv", "wu")):
                got = ops.ctx_heads(d.t["a"], [d.wp(k) for k in names])
                for k, v in zip(names, got):
                    rep.check("T=%d %d weights %s" % (T, len(names), k), v, S._mm(c["a"], c[k], mode, True), S._mm(c["a"], c[k], mode, False))
    rep.done()


# ------------------------------------------------------------------ 4. the head pair
@pytest.mark.parametrize("mode,ex,ew", A.CASES, ids=A.IDS)
def test_head_pair(mods, mode, ex, ew):
    """ops.agg_mlp_pair(Att.u_kw, Att.v_kw): U = ReLU(GN_q(a W_q^T)) W_u^T per target row and V = ctx W_v^T per context
    row, in one launch; the context rows are pair rows, as many as another entry of ROWS."""
    ops, L = mods
    rep = Report("att_tail.head_pair", mode, ex, ew)
    for T in A.ROWS:
        c = A.problem(mode, ex, ew, T)
        ctx = p2(A.head_rows(c), ex).contiguous()
        with ops.mma_scope(mode):
            d = Dev(ops, c)
            u_kw = dict(n_rows=T, rels=[ops.RelSpec(d.t["a"], d.wp("wq"))], flags=L.F_GN1 | L.F_RELU1 | L.F_GEMM2, gn1=d.gn["gq"],
                        wp2=d.wp("wu"), eps=EPS)
            v_kw = dict(n_rows=ctx.shape[0], rels=[ops.RelSpec(ctx.cuda(), d.wp("wv"))], flags=0)
            U, V = ops.agg_mlp_pair(u_kw, v_kw)
        kw = dict(gn1=c["gq"], relu1=True, w2=c["wu"])
        rep.check("T=%d U" % T, U, S.row_block(T, [(c["a"], c["wq"], None)], mode, **kw)["out"],
                  S.row_block(T, [(c["a"], c["wq"], None)], mode, model=False, **kw)["out"])
        rep.check("S=%d V" % ctx.shape[0], V, S._mm(ctx, c["wv"], mode, True), S._mm(ctx, c["wv"], mode, False))
    rep.done()


# ------------------------------------------------------------------ flags 0: the kernel against its own model, elementwise
@pytest.mark.parametrize("mode,ex,ew", SPLIT_SMALL, ids=ids(SPLIT_SMALL))
@pytest.mark.parametrize("shape", ["ident", "block", "csr", "range", "ctx_heads"])
def test_flags0_elementwise(mods, shape, mode, ex, ew):
    """ident / block / csr: the problems of test_gpu_operand_scale.test_agg_mlp_plain (n = 1, 33, 130); range: the tail's
    first stage alone, [IDENT(a, W_agt), RANGE(m, W_c1)] with flags 0, the segment sum formed in fp32 in pair order as
    the kernel forms it; ctx_heads: two weights (f16x2 / bf16; the other modes are refused)."""
    ops, L = mods
    bad = []
    head = "OPSCALE elementwise %s %s x2^%d w2^%d" % (shape, mode, ex, ew)
    if shape in ("ident", "block", "csr"):
        dd = draw()
        w384 = p2(dd["w384"], ew)
        ws = [p2(w, ew) for w in dd["w"][:3]]
        w384_d, ws_d = w384.cuda(), [w.cuda() for w in ws]
        for n in (1, 33, 130):
            x = p2(dd["x"][:n], ex).contiguous()
            x_d = x.cuda()
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
                    plan = ops.csr_build([u.cuda() for u, _ in edges], [v.cuda() for _, v in edges], n)
                    got = ops.agg_mlp(n, [ops.RelSpec(x_d, ops.packed(ws_d[0]), L.REL_IDENT),
                                          ops.RelSpec(x_d, ops.packed(ws_d[1]), L.REL_CSR, 0),
                                          ops.RelSpec(x_d, ops.packed(ws_d[2]), L.REL_CSR, 1)], 0,
                                      rowptr=plan.rowptr, col=plan.col, n_rel_csr=2)
            operands = [(S.gather_sum(xr, e, n), w) for xr, w, e in rels]
            check_elementwise(bad, "%s n=%d" % (head, n), got, S.row_block(n, rels, mode)["out"], A.accumulation_bound(operands, mode))
    else:
        for T in A.ROWS:
            c = A.problem(mode, ex, ew, T)
            with ops.mma_scope(mode):
                d = Dev(ops, c)
                if shape == "range":
                    pair_order = (c["hi"], np.arange(c["P"]))
                    operands = [(S.f32(c["a"]), c["w_agt"]), (S.gather_sum(c["m"][:c["P"]], pair_order, T), c["w_c1"])]
                    got = [ops.agg_mlp(T, [ops.RelSpec(d.t["a"], d.wp("w_agt"), L.REL_IDENT), ops.RelSpec(d.t["m"], d.wp("w_c1"), L.REL_RANGE)],
                                       0, rowptr=d.t["rowptr"])]
                    want = [sum(S.mm(a, w, mode) for a, w in operands)]
                    bounds = [A.accumulation_bound(operands, mode)]
                elif mode not in FAST:
                    assert not ops.ctx_heads_ok()
                    with pytest.raises(L.LgcnError, match=r"code -2"):
                        ops.ctx_heads(d.t["a"], [d.wp("wv")])
                    continue
                else:
                    got = ops.ctx_heads(d.t["a"], [d.wp("wv"), d.wp("wu")])
                    want = [S.mm(c["a"], c[k], mode) for k in ("wv", "wu")]
                    bounds = [A.accumulation_bound([(c["a"], c[k])], mode) for k in ("wv", "wu")]
            for j, (g, w, b) in enumerate(zip(got, want, bounds)):
                check_elementwise(bad, "%s T=%d out%d" % (head, T, j), g, w, b)
    assert not bad, "(case, max |kernel - model| / bound): %s" % bad
