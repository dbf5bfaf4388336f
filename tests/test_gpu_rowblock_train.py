"""GPU: the fused row-block backward (lgcn_rowblock_bwd; ops.rowblock_bwd; autograd.RowBlockFn.train_hip) -- the entry
against the header's formulas in float64 at a bar taken from today's composed calls, RowBlockFn against fp64 stock autograd in
every matrix mode, repeatable and independent of the matrix mode, rows past n_rows untouched, absent gradients skipped,
ineligible blocks on the composed route, one Att layer and whole training steps of Net with the switch on, off by default, and
fresh weight images after an optimizer step.

Row counts: 1, 31, 32, 33 (one tile, a full one, one row into the second) and 130 (5 tiles, the last ragged) with 1, 2 and 3
workgroups (5 / 3+2 / 2+2+1 tiles each): the smallest shapes at which tiling, the masking of rows past n_rows and the record
reduction can go wrong.  Weights are scaled 0.08, the GroupNorm weights lie in [0.5, 1.5].  Block shapes (SHAPES):
  a  GN + ReLU, one relation, [128,128]                 (layers.Linear, Att.query)
  b  GN + ReLU + residual, one relation                 (Att.linear)
  c  plain Linear on columns 128:256 of a [128,384]     (Att's U)
  d  GN + ReLU, two relations with two weights          (att_post)
  e  plain, two relations on columns 0:128 / 128:256 of one [128,256] weight      (AttDest)
  f  ReLU only                                          (Att without context rows)
  g  GN without ReLU, columns 0:128 of a [128,132]      (A2M.meta)

Every float64 reference takes its ReLU decisions from the output of the HIP forward under test (out > 0), never from its own
forward: a pre-activation within rounding of zero otherwise lands on the other side and the reference itself misses the bar.
Errors are rel_err = max |got - ref| / max |ref|; the bar is bar(e_cmp) = min(max(2 e_cmp, 1e-6), 1e-4) with e_cmp the error of
the composed path against a float64 reference of the same kind on the same inputs in mode f32.  Both are printed per tensor
before anything is asserted."""
import functools
import os
import types

import numpy as np
import pytest
import torch

import test_gpu_training as TG
from golden_io import load_scenes
from test_gpu_laneconv_train import check_rows, err, gn_bwd64, hat64, randomize, same_bits

pytestmark = pytest.mark.gpu

C = 128
EPS = 1e-5
CASES = [(1, None), (31, None), (32, None), (33, None), (130, 1), (130, 2), (130, 3)]
F = torch.nn.functional

# gn, relu, res; K: columns of each weight; rels: (source, weight, first column)
SHAPES = {
    "a": dict(gn=True, relu=True, res=False, K=[128], rels=[(0, 0, 0)]),
    "b": dict(gn=True, relu=True, res=True, K=[128], rels=[(0, 0, 0)]),
    "c": dict(gn=False, relu=False, res=False, K=[384], rels=[(0, 0, 128)]),
    "d": dict(gn=True, relu=True, res=False, K=[128, 128], rels=[(0, 0, 0), (1, 1, 0)]),
    "e": dict(gn=False, relu=False, res=False, K=[256], rels=[(0, 0, 0), (1, 0, 128)]),
    "f": dict(gn=False, relu=True, res=False, K=[128], rels=[(0, 0, 0)]),
    "g": dict(gn=True, relu=False, res=False, K=[132], rels=[(0, 0, 0)]),
}


@pytest.fixture(scope="module")
def mods():
    import lanegcn_amd  # noqa: F401
    from lanegcn_amd import _lib as L
    from lanegcn_amd import autograd as A
    from lanegcn_amd import lanegcn as M
    from lanegcn_amd import ops
    return M, A, ops, L


@pytest.fixture(scope="module")
def train_golden():
    with np.load(os.path.join(TG.GOLDEN_DIR, "train_b4.npz")) as z:
        return {k: z[k] for k in z.files}


@pytest.fixture
def mma_scope(mods):
    ops = mods[2]
    prev = ops.get_mma()
    yield ops.set_mma
    ops.set_mma(prev)


@pytest.fixture
def count_fused(mods, monkeypatch):
    """A list that grows by one with every ops.rowblock_bwd: its tag's relation count."""
    ops = mods[2]
    calls, real = [], ops.rowblock_bwd

    def counted(*a, **kw):
        calls.append(len(a[4]))
        return real(*a, **kw)

    monkeypatch.setattr(ops, "rowblock_bwd", counted)
    return calls


@pytest.fixture
def count_eligible(mods, monkeypatch):
    """A list that grows by one with every RowBlockFn.backward whose block the issue's rules make eligible: CUDA fp32 rows, one
    or two IDENT relations on distinct sources and distinct 128-column blocks."""
    A, L = mods[1], mods[3]
    seen, real = [], A.RowBlockFn.backward

    def spy(ctx, d_out):
        rels = ctx.spec.rels
        if (d_out.is_cuda and d_out.dtype == torch.float32 and ctx.spec.n_rows > 0 and 1 <= len(rels) <= 2
                and all(r.mode == L.REL_IDENT for r in rels) and len({r.src for r in rels}) == len(rels)
                and len({(r.w, r.col0) for r in rels}) == len(rels)):
            seen.append(len(rels))
        return real(ctx, d_out)

    monkeypatch.setattr(A.RowBlockFn, "backward", staticmethod(spy))
    return seen


@pytest.fixture
def rb_on(mods):
    A = mods[1]
    prev = A.RowBlockFn.train_hip
    A.RowBlockFn.train_hip = True
    yield
    A.RowBlockFn.train_hip = prev


@pytest.fixture
def all_on(mods, rb_on):
    """Every train_hip switch of the package."""
    from lanegcn_amd import layers
    M = mods[0]
    owners = [M.ActorNet, M.PredNet, M.Att, M.MapNet, M.M2M, layers.LinearRes]
    prev = [o.train_hip for o in owners]
    for o in owners:
        o.train_hip = True
    yield
    for o, p in zip(owners, prev):
        o.train_hip = p


@functools.lru_cache(maxsize=None)
def block_inputs(n, shape):
    """CPU fp32 inputs of one block of SHAPES on n rows."""
    s = SHAPES[shape]
    g = torch.Generator().manual_seed(2000 + 10 * n + ord(shape))
    rnd = lambda *sz: torch.randn(*sz, generator=g)
    return dict(srcs=[rnd(n, C) for _ in range(2)], ws=[rnd(C, k) * 0.08 for k in s["K"]], gamma=torch.rand(C, generator=g) + 0.5,
                beta=rnd(C) * 0.1, res=rnd(n, C), d_out=rnd(n, C))


def n_src(shape):
    return 1 + max(r[0] for r in SHAPES[shape]["rels"])


def names_of(shape):
    """Leaves of a block, by name."""
    s = SHAPES[shape]
    return (["src%d" % i for i in range(n_src(shape))] + ["w%d" % k for k in range(len(s["K"]))]
            + (["gamma", "beta"] if s["gn"] else []) + (["res"] if s["res"] else []))


def leaves_of(inp, shape, to, no_grad=()):
    d = {"src%d" % i: t for i, t in enumerate(inp["srcs"])}
    d.update({"w%d" % k: t for k, t in enumerate(inp["ws"])})
    d.update(gamma=inp["gamma"], beta=inp["beta"], res=inp["res"])
    return {k: to(d[k]).requires_grad_(k not in no_grad) for k in names_of(shape)}


def fn_step(mods, inp, shape, fused, mode="f32", no_grad=()):
    """RowBlockFn forward + backward in matrix mode `mode` on fresh device leaves: {"out", "d <leaf>": gradient or None}."""
    M, A, ops, L = mods
    s = SHAPES[shape]
    p = leaves_of(inp, shape, lambda t: t.cuda(), no_grad)
    gn = types.SimpleNamespace(weight=p["gamma"], bias=p["beta"], eps=EPS) if s["gn"] else None
    with ops.mma_scope(mode):
        out = A.row_block([p["src%d" % i] for i in range(n_src(shape))], [p["w%d" % k] for k in range(len(s["K"]))],
                          [A.Rel(si, wi, L.REL_IDENT, 0, c0) for si, wi, c0 in s["rels"]], inp["d_out"].shape[0], gn=gn,
                          relu=s["relu"], res=p.get("res"), fused_bwd=fused)
        out.backward(inp["d_out"].cuda())
    res = {"out": out.detach()}
    res.update({"d " + k: v.grad for k, v in p.items()})
    return res


class _Ctx:
    def save_for_backward(self, *t):
        self.saved = t


def hip_forward(mods, inp, shape, mode="f32"):
    """The forward of RowBlockFn itself in matrix mode `mode`: (pre or None, out) on the device."""
    M, A, ops, L = mods
    s = SHAPES[shape]
    srcs = [t.cuda() for t in inp["srcs"][:n_src(shape)]]
    ws = [t.cuda() for t in inp["ws"]]
    spec = A.BlockSpec(n_rows=inp["d_out"].shape[0], rels=[A.Rel(si, wi, L.REL_IDENT, 0, c0) for si, wi, c0 in s["rels"]],
                       gn=s["gn"], relu=s["relu"], has_res=s["res"], eps=EPS)
    gw, gb = (inp["gamma"].cuda(), inp["beta"].cuda()) if s["gn"] else (None, None)
    ctx = _Ctx()
    with torch.no_grad(), ops.mma_scope(mode):
        out = A.RowBlockFn.forward(ctx, spec, len(srcs), len(ws), *srcs, *ws, gw, gb, inp["res"].cuda() if s["res"] else None)
    pre = ctx.saved[-2] if (s["gn"] or s["relu"]) else None
    assert ctx.saved[-1] is out
    return pre, out


def forward64(p, shape, mask):
    s = SHAPES[shape]
    t = sum(p["src%d" % si] @ p["w%d" % wi][:, c0:c0 + C].t() for si, wi, c0 in s["rels"])
    if s["gn"]:
        t = F.group_norm(t, 1, p["gamma"], p["beta"], EPS)
    if s["res"]:
        t = t + p["res"]
    return t * mask if s["relu"] else t


def stock64(inp, shape, out):
    """The block in float64 stock autograd on the CPU, its ReLU a multiplication by out > 0 of the HIP forward `out`:
    {"out", "d <leaf>"}."""
    p = leaves_of(inp, shape, lambda t: t.double().clone())
    y = forward64(p, shape, (out > 0).cpu().double())
    y.backward(inp["d_out"].double())
    res = {"out": y.detach()}
    res.update({"d " + k: v.grad for k, v in p.items()})
    return res


def reference64(inp, shape, out):
    """The formulas of include/lgcn.h (lgcn_rowblock_bwd) in float64 on the CPU, the ReLU a multiplication by out > 0."""
    s = SHAPES[shape]
    srcs, ws = [t.double() for t in inp["srcs"]], [t.double() for t in inp["ws"]]
    d_out = inp["d_out"].double()
    g = d_out * (out > 0).cpu().double() if s["relu"] else d_out
    r = {}
    if s["res"]:
        r["d res"] = g
    if s["gn"]:
        pre = sum(srcs[si] @ ws[wi][:, c0:c0 + C].t() for si, wi, c0 in s["rels"])
        xh, rstd = hat64(pre)
        r["d gamma"], r["d beta"] = (g * xh).sum(0), g.sum(0)
        dT = gn_bwd64(g, xh, rstd, inp["gamma"].double())
    else:
        dT = g
    for k, w in enumerate(ws):
        r["d w%d" % k] = torch.zeros_like(w)
    for si, wi, c0 in s["rels"]:
        r["d src%d" % si] = dT @ ws[wi][:, c0:c0 + C]
        r["d w%d" % wi][:, c0:c0 + C] += dT.t() @ srcs[si]
    return r


def checked_reference64(inp, shape, out):
    """reference64, after checking that it is stock fp64 autograd with the same masks to 1e-12."""
    ref, stock = reference64(inp, shape, out), stock64(inp, shape, out)
    assert set(ref) == set(stock) - {"out"}
    for k, v in ref.items():
        e = float((v - stock[k]).abs().max() / (stock[k].abs().max() + 1e-300))
        assert e <= 1e-12, (shape, k, e)
    return ref


def entry(mods, inp, shape, pre, out, **kw):
    """ops.rowblock_bwd on the saved tensors of hip_forward, as {"d <leaf>": tensor}; want_res defaults to what the block has."""
    ops = mods[2]
    s = SHAPES[shape]
    srcs, ws = [t.cuda() for t in inp["srcs"]], [t.cuda() for t in inp["ws"]]
    kw.setdefault("want_res", s["res"] and s["relu"])
    g = ops.rowblock_bwd(inp["d_out"].cuda(), out if s["relu"] else None, pre if s["gn"] else None,
                         inp["gamma"].cuda() if s["gn"] else None, [(srcs[si], ws[wi], c0) for si, wi, c0 in s["rels"]], eps=EPS, **kw)
    assert g["w_index"] == [wi for _, wi, _ in s["rels"]]
    r = {"d src%d" % si: g["d_src"][i] for i, (si, _, _) in enumerate(s["rels"])}
    r.update({"d w%d" % k: v for k, v in enumerate(g["d_w"])})
    if s["gn"]:
        r["d gamma"], r["d beta"] = g["d_gamma"], g["d_beta"]
    if s["res"]:
        r["d res"] = g["d_res"]
    return r


# ------------------------------------------------------------------ 1. the entry against fp64
@pytest.mark.parametrize("shape", sorted(SHAPES))
@pytest.mark.parametrize("n,n_chunks", CASES)
def test_entry_against_fp64(mods, mma_scope, n, n_chunks, shape):
    """Every d_src, d_w, d_gamma, d_beta and d_res of ops.rowblock_bwd on the saved tensors of one HIP forward; outside the
    relations' column blocks a sliced weight's gradient is exactly zero."""
    mma_scope("f32")
    s = SHAPES[shape]
    inp = block_inputs(n, shape)
    pre, out = hip_forward(mods, inp, shape)
    ref = checked_reference64(inp, shape, out)
    got = entry(mods, inp, shape, pre, out, n_chunks=n_chunks)
    cmp_ = fn_step(mods, inp, shape, False)
    assert torch.equal(cmp_["out"], out)                                 # the composed path ran on the same forward
    assert set(got) == set(ref) and all(v is not None for v in got.values())
    for k, width in enumerate(s["K"]):
        covered = torch.zeros(width, dtype=torch.bool)
        for _, wi, c0 in s["rels"]:
            if wi == k:
                covered[c0:c0 + C] = True
        assert got["d w%d" % k].shape == (C, width)
        assert bool((got["d w%d" % k][:, ~covered.cuda()] == 0).all()), (shape, k)
        assert bool(covered.all()) == (shape in "abdef")
    rows = [(k, err(got[k], ref[k]), err(cmp_[k], ref[k])) for k in ref]
    check_rows(rows, "shape=%s n=%d chunks=%s" % (shape, n, n_chunks))


# ------------------------------------------------------------------ 2. RowBlockFn against stock autograd
@pytest.mark.parametrize("mode", ["f32", "bf16x3", "f16x2"])
@pytest.mark.parametrize("shape", sorted(SHAPES))
def test_function_against_stock_autograd(mods, mma_scope, count_fused, mode, shape):
    """RowBlockFn with fused_bwd, forward in every matrix mode, against fp64 stock autograd with that forward's masks; e_cmp:
    the composed backward in f32 mode against fp64 stock autograd with its forward's masks."""
    mma_scope(mode)
    inp = block_inputs(130, shape)
    got = fn_step(mods, inp, shape, True, mode)
    assert count_fused == [len(SHAPES[shape]["rels"])]
    ref = stock64(inp, shape, got["out"])
    cmp_ = fn_step(mods, inp, shape, False, "f32")
    assert len(count_fused) == 1
    ref_cmp = stock64(inp, shape, cmp_["out"])
    assert err(got["out"], ref["out"]) <= 1e-4
    assert set(got) == set(ref) and all(v is not None for v in got.values())
    rows = [(k, err(got[k], ref[k]), err(cmp_[k], ref_cmp[k])) for k in ref if k != "out"]
    check_rows(rows, "%s shape=%s" % (mode, shape))


# ------------------------------------------------------------------ 3. repeatable, mode-independent
@pytest.mark.parametrize("shape", ["b", "d", "e"])
def test_repeatable_and_independent_of_the_matrix_mode(mods, mma_scope, shape):
    inp = block_inputs(130, shape)
    pre, out = hip_forward(mods, inp, shape)
    runs = []
    for mode in ("f32", "f32", "f16x2"):
        mma_scope(mode)
        runs.append(entry(mods, inp, shape, pre, out, n_chunks=3))
    for r in runs[1:]:
        assert set(r) == set(runs[0])
        assert all(same_bits(runs[0][k], r[k]) and r[k] is not None for k in r), [k for k in r if not same_bits(runs[0][k], r[k])]


# ------------------------------------------------------------------ 4. ragged edge
@pytest.mark.parametrize("shape", ["b", "d"])
def test_rows_past_n_rows_are_untouched(mods, shape):
    s = SHAPES[shape]
    inp = block_inputs(33, shape)
    pre, out = hip_forward(mods, inp, shape)
    bufs = [torch.full((33 + 64, C), -7.5, device="cuda") for _ in range(len(s["rels"]) + 1)]
    got = entry(mods, inp, shape, pre, out, d_src=[b[:33] for b in bufs[:-1]], d_res=bufs[-1][:33] if s["res"] else None)
    torch.cuda.synchronize()
    plain = entry(mods, inp, shape, pre, out)
    used = bufs if s["res"] else bufs[:-1]
    names = ["d src%d" % si for si, _, _ in s["rels"]] + (["d res"] if s["res"] else [])
    for b, k in zip(used, names):
        assert got[k].data_ptr() == b.data_ptr(), k
        assert bool((b[33:] == -7.5).all()), k
        assert same_bits(b[:33], plain[k]), k
    assert all(bool(torch.isfinite(v).all()) for v in got.values())


# ------------------------------------------------------------------ 5. absent gradients
@pytest.mark.parametrize("shape", ["b", "d"])
def test_absent_gradients(mods, shape):
    """Each output left out in turn: the others keep their bits."""
    s = SHAPES[shape]
    inp = block_inputs(130, shape)
    pre, out = hip_forward(mods, inp, shape)
    full = entry(mods, inp, shape, pre, out, n_chunks=3)
    n_rel = len(s["rels"])
    variants = []
    for r, (si, wi, _) in enumerate(s["rels"]):
        variants.append((dict(want_src=[i != r for i in range(n_rel)]), {"d src%d" % si}))
        variants.append((dict(want_w=[i != r for i in range(n_rel)]), {"d w%d" % wi}))
    variants.append((dict(want_gn=False), {"d gamma", "d beta"}))
    if s["res"]:
        variants.append((dict(want_res=False), {"d res"}))
    variants.append((dict(want_w=[False] * n_rel, want_gn=False), {"d gamma", "d beta"} | {"d w%d" % wi for _, wi, _ in s["rels"]}))
    for kw, gone in variants:
        part = entry(mods, inp, shape, pre, out, n_chunks=3, **kw)
        assert set(part) == set(full)
        for k in full:
            assert (part[k] is None) == (k in gone), (kw, k)
            assert k in gone or same_bits(full[k], part[k]), (kw, k)
    # a column block of a wider weight gradient (row stride 256) next to an absent one: shape "e" with one relation's dW
    # left out writes the other's 128 columns with the bits of the full run and leaves the rest of the [128,256] tensor zero
    inp = block_inputs(33, "e")
    pre, out = hip_forward(mods, inp, "e")
    whole = entry(mods, inp, "e", pre, out, n_chunks=2)["d w0"]
    assert whole.shape == (C, 2 * C) and bool(whole[:, :C].abs().max() > 0) and bool(whole[:, C:].abs().max() > 0)
    for r in range(2):
        half = entry(mods, inp, "e", pre, out, n_chunks=2, want_w=[i == r for i in range(2)])["d w0"]
        assert same_bits(half[:, r * C:(r + 1) * C].contiguous(), whole[:, r * C:(r + 1) * C].contiguous()), r
        assert bool((half[:, (1 - r) * C:(2 - r) * C] == 0).all()), r


def test_no_parameter_gradient_needs_no_workspace(mods):
    """The C entry with row outputs only and ws = NULL."""
    M, A, ops, L = mods
    import ctypes
    inp = block_inputs(130, "b")
    pre, out = hip_forward(mods, inp, "b")
    full = entry(mods, inp, "b", pre, out)
    d_out, src, w, gamma = inp["d_out"].cuda(), inp["srcs"][0].cuda(), inp["ws"][0].cuda(), inp["gamma"].cuda()
    with ops.exact_mma():
        wpt = ops.packed_t(w)
    d_src, d_res = torch.empty(130, C, device="cuda"), torch.empty(130, C, device="cuda")
    q = L.RowBlockBwd()
    q.d_out, q.out, q.pre, q.gamma = d_out.data_ptr(), out.data_ptr(), pre.data_ptr(), gamma.data_ptr()
    q.src[0], q.wpt[0], q.d_src[0], q.d_res = src.data_ptr(), wpt.data_ptr(), d_src.data_ptr(), d_res.data_ptr()
    q.n_rows, q.eps, q.n_rel, q.n_chunks = 130, EPS, 1, 3
    assert L.load().lgcn_rowblock_bwd(ctypes.byref(q), ops._stream()) == 0
    torch.cuda.synchronize()
    assert same_bits(d_src, full["d src0"]) and same_bits(d_res, full["d res"])


@pytest.mark.parametrize("shape", ["b", "d"])
def test_input_without_grad_gets_none(mods, mma_scope, count_fused, shape):
    mma_scope("f32")
    inp = block_inputs(130, shape)
    full = fn_step(mods, inp, shape, True)
    for off in (("src0",), ("w0",), ("gamma", "beta"), ("src0", "w0", "gamma", "beta")):
        part = fn_step(mods, inp, shape, True, no_grad=off)
        for k in full:
            gone = k[2:] in off
            assert (part[k] is None) == gone, (off, k)
            assert gone or same_bits(full[k], part[k]), (off, k)
    assert len(count_fused) == 5


# ------------------------------------------------------------------ 6. ineligible blocks
def range_block_step(mods, seed=4):
    """A block with a RANGE relation, built as Att.run_train builds att_post: 33 targets, per-target segments of 0..4 rows."""
    M, A, ops, L = mods
    g = torch.Generator().manual_seed(seed)
    T = 33
    lens = torch.randint(0, 5, (T,), generator=g)
    P = int(lens.sum())
    assert P > 0 and bool((lens == 0).any())
    rowptr = torch.zeros(T + 1, dtype=torch.int32)
    rowptr[1:] = torch.cumsum(lens, 0).to(torch.int32)
    hi = torch.repeat_interleave(torch.arange(T), lens).to(torch.int32)
    p = dict(agts=torch.randn(T, C, generator=g), m=torch.randn(P, C, generator=g), w0=torch.randn(C, C, generator=g) * 0.08,
             w1=torch.randn(C, C, generator=g) * 0.08, gamma=torch.rand(C, generator=g) + 0.5, beta=torch.randn(C, generator=g) * 0.1)
    p = {k: v.cuda().requires_grad_(True) for k, v in p.items()}
    gn = types.SimpleNamespace(weight=p["gamma"], bias=p["beta"], eps=EPS)
    y = A.row_block([p["agts"], p["m"]], [p["w0"], p["w1"]], [A.Rel(0, 0, L.REL_IDENT), A.Rel(1, 1, L.REL_RANGE)], T, gn=gn,
                    relu=True, rowptr=rowptr.cuda(), seg_ids=hi.cuda(), n_seg_rows=torch.tensor([P], dtype=torch.int32).cuda(),
                    tag="att_post")
    y.backward(torch.randn(T, C, generator=g).cuda())
    return [y.detach()] + [v.grad for v in p.values()]


def same_source_step(mods, seed=5):
    """Two relations on one source (two weights): d src is a sum of two products, which the fused entry does not form."""
    M, A, ops, L = mods
    g = torch.Generator().manual_seed(seed)
    p = dict(x=torch.randn(33, C, generator=g), w0=torch.randn(C, C, generator=g) * 0.08, w1=torch.randn(C, C, generator=g) * 0.08)
    p = {k: v.cuda().requires_grad_(True) for k, v in p.items()}
    y = A.row_block([p["x"]], [p["w0"], p["w1"]], [A.Rel(0, 0, L.REL_IDENT), A.Rel(0, 1, L.REL_IDENT)], 33, relu=True)
    y.backward(torch.randn(33, C, generator=g).cuda())
    return [y.detach()] + [v.grad for v in p.values()]


@pytest.mark.parametrize("step", [range_block_step, same_source_step])
def test_ineligible_blocks_keep_the_composed_route(mods, mma_scope, count_fused, step):
    M, A, ops, L = mods
    mma_scope("f32")
    assert A.RowBlockFn.train_hip is False
    off = step(mods)
    A.RowBlockFn.train_hip = True
    try:
        on = step(mods)
    finally:
        A.RowBlockFn.train_hip = False
    assert not count_fused
    assert all(v is not None for v in on) and all(same_bits(a, b) for a, b in zip(on, off))


def test_cpu_tensors_keep_the_composed_route(mods, count_fused):
    """The package has no CPU path at all (a CPU tensor is an LgcnError in the first launch wrapper that meets it), so a block on
    CPU tensors has no gradients to compare: with the switch on, its backward makes the same refusal as with the switch off --
    that of the composed route's first wrapper -- and ops.rowblock_bwd is never called."""
    M, A, ops, L = mods
    g = torch.Generator().manual_seed(8)
    x, w, d_out = torch.randn(33, C, generator=g), torch.randn(C, C, generator=g) * 0.08, torch.randn(33, C, generator=g)
    said = []
    for flag in (False, True):
        spec = A.BlockSpec(n_rows=33, rels=[A.Rel(0, 0, L.REL_IDENT)], gn=False, relu=True, fused_bwd=flag)
        ctx = types.SimpleNamespace(spec=spec, n_src=1, n_w=1, saved_tensors=(x, w, x.clone(), x.clone()), has=(False, True),
                                    needs_input_grad=(False, False, False, True, True, False, False, False))
        with pytest.raises(L.LgcnError) as e:
            A.RowBlockFn.backward(ctx, d_out)
        said.append(str(e.value))
    assert said[0] == said[1] and "CUDA" in said[0]
    assert not count_fused


# ------------------------------------------------------------------ 7. one Att layer
def att_case(M):
    """One scene, 33 targets and 70 context rows; the threshold is the median over the targets of the distance to the nearest
    context row, so that about half of the targets have no pair at all."""
    g = torch.Generator().manual_seed(12)
    agt_ctrs, ctx_ctrs = torch.randn(33, 2, generator=g) * 6, torch.randn(70, 2, generator=g) * 6
    dist_th = float(torch.cdist(agt_ctrs, ctx_ctrs).min(1).values.median())
    agts, ctx, w_out = torch.randn(33, C, generator=g), torch.randn(70, C, generator=g), torch.randn(33, C, generator=g)
    return dict(agts=agts.cuda(), ctx=ctx.cuda(), w_out=w_out.cuda(), agt_ctrs=[agt_ctrs.cuda()], ctx_ctrs=[ctx_ctrs.cuda()],
                agt_idcs=[torch.arange(33).cuda()], ctx_idcs=[torch.arange(70).cuda()], dist_th=dist_th)


def att_step(M, att, case, ps):
    a, c = case["agts"].clone().requires_grad_(True), case["ctx"].clone().requires_grad_(True)
    att.zero_grad(set_to_none=True)
    out = att(a, case["agt_idcs"], case["agt_ctrs"], c, case["ctx_idcs"], case["ctx_ctrs"], case["dist_th"], pairs=ps)
    (out * case["w_out"]).sum().backward()
    res = {"out": out.detach(), "d agts": a.grad, "d ctx": c.grad}
    res.update({n: p.grad.clone() for n, p in att.named_parameters()})
    return res


def att_masks(mods, att, case, ps):
    """The ReLU masks of Att.run_train_hip's forward (its own calls, without autograd), as CPU float64, and its output."""
    M, A, ops, L = mods
    T = case["agts"].shape[0]
    c0, d, lin = att.ctx[0], att.dist, att.linear
    with torch.no_grad():
        q = A.linear_gn(case["agts"], att.query.linear.weight, gn=att.query.norm, relu=True)
        U = A.linear_gn(q, c0.linear.weight, col0=128)
        V = A.linear_gn(case["ctx"], c0.linear.weight, col0=256)
        m, masks = ops.att_pairs_train(ps, d[0].weight, d[0].bias, d[2].linear.weight, (d[2].norm.weight, d[2].norm.bias),
                                       c0.linear.weight, U, V, (c0.norm.weight, c0.norm.bias), eps=c0.norm.eps)
        S = ops.gather_sum(m, ps.rowptr, None, T)
        y = A.row_block([case["agts"], S], [att.agt.weight, att.ctx[1].weight], [A.Rel(0, 0, L.REL_IDENT), A.Rel(1, 1, L.REL_IDENT)],
                        T, gn=att.norm, relu=True)
        out = A.linear_gn(y, lin.linear.weight, gn=lin.norm, relu=True, res=case["agts"])
        pm = ops.att_pair_masks(masks, ps.count())
    f = lambda t: t.cpu().double()
    return dict(q=f(q > 0), pair=f(pm), y=f(y > 0), out=f(out > 0)), out


def att_reference64(att, case, ps, mk):
    """The Att layer (reference lanegcn.py:662-710, hoisted as run_train_hip hoists it) in float64 stock autograd on the CPU,
    every ReLU a multiplication by the HIP forward's mask (mk None: by its own, which makes it the oracle's layer)."""
    p = {n: v.detach().cpu().double().requires_grad_(True) for n, v in att.named_parameters()}
    a, c = case["agts"].cpu().double().requires_grad_(True), case["ctx"].cpu().double().requires_grad_(True)
    hi, wi = (t.cpu() for t in ps.hi_wi_long())
    gn = lambda x, name: F.group_norm(x, 1, p[name + ".weight"], p[name + ".bias"], EPS)
    pick = lambda key: mk[key] if isinstance(key, str) else mk["pair"][:, key]
    act = lambda x, key: x * (pick(key) if mk is not None else (x > 0).double())
    wc0 = p["ctx.0.linear.weight"]
    q = act(gn(a @ p["query.linear.weight"].t(), "query.norm"), "q")
    U, V = q @ wc0[:, C:2 * C].t(), c @ wc0[:, 2 * C:].t()
    delta = case["agt_ctrs"][0].cpu().double()[hi] - case["ctx_ctrs"][0].cpu().double()[wi]
    h1 = act(delta @ p["dist.0.weight"].t() + p["dist.0.bias"], 0)
    e = act(gn(h1 @ p["dist.2.linear.weight"].t(), "dist.2.norm"), 1)
    m = act(gn(e @ wc0[:, :C].t() + U[hi] + V[wi], "ctx.0.norm"), 2)
    S = torch.zeros_like(a).index_add(0, hi, m)
    y = act(gn(a @ p["agt.weight"].t() + S @ p["ctx.1.weight"].t(), "norm"), "y")
    out = act(gn(y @ p["linear.linear.weight"].t(), "linear.norm") + a, "out")
    (out * case["w_out"].cpu().double()).sum().backward()
    res = {"out": out.detach(), "d agts": a.grad, "d ctx": c.grad}
    res.update({n: v.grad for n, v in p.items()})
    return res


def test_att_layer_on_against_off(mods, mma_scope, count_fused):
    """One Att(128, 128) with Att.train_hip on both sides: RowBlockFn.train_hip moves its five node-side blocks (query, U, V,
    att_post, linear) to the fused entry; same forward, gradients at the bar."""
    M, A, ops, L = mods
    mma_scope("f32")
    case = att_case(M)
    att = randomize(M.Att(C, C), 41).cuda().train()
    ps = M.build_pairs(case["agt_idcs"], case["agt_ctrs"], case["ctx_idcs"], case["ctx_ctrs"], case["dist_th"])
    per_target = (ps.rowptr[1:] - ps.rowptr[:-1]).cpu()
    assert ps.count() > 0 and bool((per_target == 0).any()) and bool((per_target > 0).any())
    M.Att.train_hip = True
    try:
        off = att_step(M, att, case, ps)
        assert not count_fused
        A.RowBlockFn.train_hip = True
        try:
            on = att_step(M, att, case, ps)
        finally:
            A.RowBlockFn.train_hip = False
    finally:
        M.Att.train_hip = False
    assert sorted(count_fused) == [1, 1, 1, 1, 2], count_fused         # five fused calls, att_post with two relations
    assert torch.equal(on["out"], off["out"])
    mk, fwd = att_masks(mods, att, case, ps)
    assert torch.equal(fwd, on["out"])                                   # the masks are those of the forward under test
    ref = att_reference64(att, case, ps, mk)
    assert set(ref) == set(on) and all(v is not None for v in on.values())
    check_rows([(k, err(on[k], ref[k]), err(off[k], ref[k])) for k in ref], "Att P=%d" % ps.count())


# ------------------------------------------------------------------ 8. whole steps
@pytest.mark.parametrize("mode", ["f32", "f16x2"])
def test_whole_net_training_step(mods, all_on, mma_scope, count_fused, count_eligible, golden, train_golden, ref_state_names, mode):
    """Every train_hip switch on: the reference's own loss, gradients and Adam update (tests/golden/train_b4.npz), the body and
    the bars of test_training_step_matches_reference; every eligible row block of the step took the fused route."""
    mma_scope(mode)
    TG.test_training_step_matches_reference(golden, train_golden, ref_state_names, mode)
    print("row blocks of one Net step: %d eligible, %d fused (%d with two relations)"
          % (len(count_eligible), len(count_fused), sum(1 for c in count_fused if c == 2)))
    assert len(count_fused) > 0 and sorted(count_fused) == sorted(count_eligible)


def test_switch_off_means_untouched(mods, mma_scope, count_fused, count_eligible, golden, ref_state_names):
    """Off by default: a Net step on the batch-4 golden scenes calls ops.rowblock_bwd never, whatever it has of eligible blocks."""
    M, A, ops, L = mods
    from lanegcn_amd import data as gen
    from oracle import lanegcn_oracle as O
    mma_scope("f16x2")
    assert A.RowBlockFn.train_hip is False
    net = M.Net(M.config)
    net.load_state_dict(O.seeded_state(ref_state_names, 1), strict=True)
    net = net.cuda().train()
    batch = gen.collate_fn(load_scenes(golden))
    loss_fn = M.Loss(M.config).cuda()
    loss_fn(net(batch), batch)["loss"].backward()
    assert not count_fused and len(count_eligible) > 0


# ------------------------------------------------------------------ 10. optimizer step
def linear_step(mods, mod, x0, d_out, flag, mode):
    A, ops = mods[1], mods[2]
    prev = A.RowBlockFn.train_hip
    A.RowBlockFn.train_hip = flag
    try:
        x = x0.clone().requires_grad_(True)
        mod.zero_grad(set_to_none=True)
        with ops.mma_scope(mode):
            out = mod(x)
            out.backward(d_out)
    finally:
        A.RowBlockFn.train_hip = prev
    res = {"out": out.detach(), "d x": x.grad}
    res.update({n: p.grad.clone() for n, p in mod.named_parameters()})
    return res


def linear_reference64(mod, x0, d_out, out):
    p = {n: v.detach().cpu().double().requires_grad_(True) for n, v in mod.named_parameters()}
    x = x0.cpu().double().requires_grad_(True)
    y = F.group_norm(x @ p["linear.weight"].t(), 1, p["norm.weight"], p["norm.bias"], EPS) * (out > 0).cpu().double()
    y.backward(d_out.cpu().double())
    res = {"out": y.detach(), "d x": x.grad}
    res.update({n: v.grad for n, v in p.items()})
    return res


def test_fresh_images_after_optimizer_step(mods, count_fused):
    """After Optimizer.step the cached transposed F32 image of a layers.Linear's weight is rebuilt: the fused gradients of the
    second step (forward in f16x2, so that only the fused backward reads F32 images) meet the bar against float64 on the
    updated weights."""
    M, A, ops, L = mods
    from lanegcn_amd import layers
    g = torch.Generator().manual_seed(6)
    mod = randomize(layers.Linear(C, C, norm="GN", ng=1), 23).cuda().train()
    x0, d_out = torch.randn(130, C, generator=g).cuda(), torch.randn(130, C, generator=g).cuda()
    linear_step(mods, mod, x0, d_out, True, "f16x2")
    opt = M.Optimizer(mod.parameters(), M.config)
    before = {k: v.clone() for k, v in mod.state_dict().items()}
    opt.step(0.0)
    assert all(not torch.equal(before[k], v) for k, v in mod.state_dict().items())
    on = linear_step(mods, mod, x0, d_out, True, "f16x2")
    assert count_fused == [1, 1]
    off = linear_step(mods, mod, x0, d_out, False, "f32")
    assert len(count_fused) == 2
    ref, ref_off = linear_reference64(mod, x0, d_out, on["out"]), linear_reference64(mod, x0, d_out, off["out"])
    assert err(on["out"], ref["out"]) <= 1e-4
    check_rows([(k, err(on[k], ref[k]), err(off[k], ref_off[k])) for k in ref if k != "out"], "after step")
