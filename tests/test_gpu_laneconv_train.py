"""GPU: the fused LaneConv / LinearRes backward (lgcn_laneconv_bwd; autograd.BlockSpec.fused_bwd; MapNet.train_hip,
M2M.train_hip, LinearRes.train_hip) -- the entry against the header's formulas in float64 at a bar taken from today's composed
calls, LaneConvFn against fp64 stock autograd in every matrix mode, repeatable and independent of the matrix mode, rows past
n_rows untouched, absent gradients skipped, at module level against the composed path, inside whole training steps of Net
against the reference's own gradients, and with fresh weight images after an optimizer step.

Row counts: 1, 31, 32, 33 (one tile, a full one, one row into the second) and 130 (5 tiles, the last ragged) with 1, 2 and 3
workgroups (5 / 3+2 / 2+2+1 tiles each).  The CSR case is a random multigraph on 70 nodes: four relations, one empty,
duplicate edges, nodes without in-edges.  Weights are scaled 0.08, the GroupNorm weights lie in [0.5, 1.5].

test_entry_against_fp64 and the two module tests print, per tensor, the error of the fused and of the composed path against
float64 (rel_err = max |got - ref| / max |ref|) before they assert."""
import functools
import os

import numpy as np
import pytest
import torch

import test_gpu_training as TG
from backward_cases import bar, gn_bwd64, hat64
from conftest import to_torch_scene
from golden_io import load_scenes
from test_gpu_training import rel_err

pytestmark = pytest.mark.gpu
GOLDEN_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")

C = 128
EPS = 1e-5
CASES = [(1, None), (31, None), (32, None), (33, None), (130, 1), (130, 2), (130, 3)]
N_CSR = 70
VEC = ("d_w2", "d_g2", "d_b2", "d_g1", "d_b1")


@pytest.fixture(scope="module")
def mods():
    import lanegcn_amd  # noqa: F401
    from lanegcn_amd import _lib as L
    from lanegcn_amd import autograd as A
    from lanegcn_amd import lanegcn as M
    from lanegcn_amd import layers, ops
    return M, A, ops, L, layers


@pytest.fixture(scope="module")
def train_golden():
    with np.load(os.path.join(GOLDEN_DIR, "train_b4.npz")) as z:
        return {k: z[k] for k in z.files}


@pytest.fixture
def mma_scope(mods):
    ops = mods[2]
    prev = ops.get_mma()
    yield ops.set_mma
    ops.set_mma(prev)


@pytest.fixture
def count_fused(mods, monkeypatch):
    """A list that grows by one with every ops.laneconv_bwd: "ident1" or "rel"."""
    ops = mods[2]
    calls, real = [], ops.laneconv_bwd

    def counted(*a, **kw):
        calls.append("ident1" if kw.get("x") is not None else "rel")
        return real(*a, **kw)

    monkeypatch.setattr(ops, "laneconv_bwd", counted)
    return calls


@pytest.fixture
def hip_on(mods):
    M, layers = mods[0], mods[4]
    prev = M.MapNet.train_hip, M.M2M.train_hip, layers.LinearRes.train_hip
    M.MapNet.train_hip = M.M2M.train_hip = layers.LinearRes.train_hip = True
    yield
    M.MapNet.train_hip, M.M2M.train_hip, layers.LinearRes.train_hip = prev


def err(got, want):
    return rel_err(got.detach().double().cpu().numpy(), want.detach().double().cpu().numpy())


def check_rows(rows, label):
    for name, e_new, e_cmp in rows:
        print("%s %-28s fused %.3e composed %.3e" % (label, name, e_new, e_cmp))
    bad = [(n, a, b) for n, a, b in rows if not a <= bar(b)]
    assert not bad, bad


def same_bits(a, b):
    return (a is None and b is None) or (a is not None and b is not None and torch.equal(a.view(torch.int32), b.view(torch.int32)))


@functools.lru_cache(maxsize=None)
def block_inputs(n, csr=False):
    """CPU fp32 inputs of one block on n rows: x, the IDENT weight w1, four relation weights, w2, both norms, d_out, and for
    csr the multigraph (us, vs)."""
    g = torch.Generator().manual_seed(1000 + n + (7 if csr else 0))
    rnd = lambda *s: torch.randn(*s, generator=g)
    d = dict(x=rnd(n, C), w1=rnd(C, C) * 0.08, w_rel=[rnd(C, C) * 0.08 for _ in range(4)], w2=rnd(C, C) * 0.08,
             g1=torch.rand(C, generator=g) + 0.5, b1=rnd(C) * 0.1, g2=torch.rand(C, generator=g) + 0.5, b2=rnd(C) * 0.1,
             d_out=rnd(n, C), us=[], vs=[])
    if csr:
        d["us"] = [torch.randint(0, n - 5, (m,), generator=g) for m in (3 * n, n, 0, n // 2)]       # the last 5: no in-edge
        d["vs"] = [torch.randint(0, n, (len(u),), generator=g) for u in d["us"]]
        hit = torch.zeros(n, dtype=torch.bool)
        for u in d["us"]:
            hit[u] = True
        assert not bool(hit.all())                                       # some node has no in-edge
        assert len(torch.unique(torch.stack([d["us"][0], d["vs"][0]]), dim=1)[0]) < 3 * n      # duplicate edges
    return d


def hip_forward(mods, x, w1, rel_ws, plan, g1, b1, w2, g2, b2, mode="f32"):
    """One HIP forward in matrix mode `mode` (the launch of LaneConvFn.forward) on device tensors; rel_ws: (weight, relation
    index) of the CSR relations of `plan`.  Returns (T, Y, Z, out)."""
    M, A, ops, L, _ = mods
    n = x.shape[0]
    T, Y, Z = (torch.empty((n, C), device="cuda") for _ in range(3))
    with ops.mma_scope(mode):
        rels = [ops.RelSpec(x, ops.packed(w1))] + [ops.RelSpec(x, ops.packed(w), L.REL_CSR, r) for w, r in rel_ws]
        kw = dict(rowptr=plan.rowptr, col=plan.col, n_rel_csr=plan.n_rel) if rel_ws else {}
        flags = L.F_GN1 | L.F_RELU1 | L.F_GEMM2 | L.F_GN2 | L.F_RES | L.F_RELU2
        out = ops.agg_mlp(n, rels, flags, gn1=(g1, b1), wp2=ops.packed(w2), gn2=(g2, b2), res=x, out_pre=T, out_mid=Y,
                          out_pre2=Z, eps=EPS, **kw)
    return T, Y, Z, out


def forward_saved(mods, inp, csr=False):
    """hip_forward on block_inputs: (T, Y, Z, out) on the device."""
    ops = mods[2]
    d = {k: inp[k].cuda() for k in ("x", "w1", "g1", "b1", "w2", "g2", "b2")}
    plan, rel_ws = None, []
    if csr:
        plan = ops.csr_build([u.cuda() for u in inp["us"]], [v.cuda() for v in inp["vs"]], d["x"].shape[0])
        rel_ws = [(inp["w_rel"][r].cuda(), r) for r in range(4) if plan.n_edges[r] > 0]
    return hip_forward(mods, d["x"], d["w1"], rel_ws, plan, d["g1"], d["b1"], d["w2"], d["g2"], d["b2"])


def reference64(inp, saved, ident1):
    """The formulas of include/lgcn.h (lgcn_laneconv_bwd) in float64 on the saved tensors; the ReLUs are multiplications by
    Y > 0 and out > 0."""
    T, Y, Z, out = (t.double().cpu() for t in saved)
    d_out, w2, g1, g2w = (inp[k].double() for k in ("d_out", "w2", "g1", "g2"))
    r = {}
    g2 = d_out * (out > 0)
    zh, rstd2 = hat64(Z)
    r["d_g2"], r["d_b2"] = (g2 * zh).sum(0), g2.sum(0)
    dZ = gn_bwd64(g2, zh, rstd2, g2w)
    r["d_w2"] = dZ.t() @ Y
    g1_ = (dZ @ w2) * (Y > 0)
    th, rstd1 = hat64(T)
    r["d_g1"], r["d_b1"] = (g1_ * th).sum(0), g1_.sum(0)
    dT = gn_bwd64(g1_, th, rstd1, g1)
    if ident1:
        r["dX"] = dT @ inp["w1"].double() + g2
        r["d_w1"] = dT.t() @ inp["x"].double()
    else:
        r["dT"], r["g2"] = dT, g2
    return r


def composed(mods, inp, saved, ident1):
    """Today's composed calls (LaneConvFn.backward's lines) on the same tensors, f32 mode."""
    M, A, ops, L, _ = mods
    T, Y, Z, out = saved
    n = T.shape[0]
    d_out, w2, w1, x = inp["d_out"].cuda(), inp["w2"].cuda(), inp["w1"].cuda(), inp["x"].cuda()
    r = {}
    with ops.mma_scope("f32"):
        dZ, g2, r["d_g2"], r["d_b2"] = ops.gn_bwd(d_out, Z, out, inp["g2"].cuda(), eps=EPS, want_g=True)
        with ops.backward_mma():
            dY = ops.agg_mlp(n, [ops.RelSpec(dZ, ops.packed_t(w2))], 0)
        r["d_w2"] = ops.wgrad(n, [ops.RelSpec(Y, None)], dZ)[0]
        dT, _, r["d_g1"], r["d_b1"] = ops.gn_bwd(dY, T, Y, inp["g1"].cuda(), eps=EPS)
        if ident1:
            with ops.backward_mma():
                r["dX"] = ops.agg_mlp(n, [ops.RelSpec(dT, ops.packed_t(w1))], L.F_RES, res=g2)
            r["d_w1"] = ops.wgrad(n, [ops.RelSpec(x, None)], dT)[0]
        else:
            r["dT"], r["g2"] = dT, g2
    return r


def entry(mods, inp, saved, ident1, **kw):
    ops = mods[2]
    T, Y, Z, out = saved
    if ident1:
        kw.update(x=inp["x"].cuda(), w1=inp["w1"].cuda())
    return ops.laneconv_bwd(inp["d_out"].cuda(), out, Z, Y, T, inp["g1"].cuda(), inp["w2"].cuda(), inp["g2"].cuda(), eps=EPS, **kw)


# ------------------------------------------------------------------ 1. the entry against fp64
@pytest.mark.parametrize("n,n_chunks,ident1", [(n, c, i) for i in (False, True) for n, c in CASES] + [(N_CSR, "csr", False)])
def test_entry_against_fp64(mods, mma_scope, n, n_chunks, ident1):
    """dT, g2 (ident1: dX, d_w1), d_w2 and the four GroupNorm vectors on saved tensors of one HIP forward; "csr": T comes from
    the multigraph's forward."""
    csr = n_chunks == "csr"
    mma_scope("f32")
    inp = block_inputs(n, csr)
    saved = forward_saved(mods, inp, csr)
    ref = reference64(inp, saved, ident1)
    got = entry(mods, inp, saved, ident1, n_chunks=None if csr else n_chunks)
    cmp_ = composed(mods, inp, saved, ident1)
    assert set(got) == set(ref) and all(v is not None for v in got.values())
    rows = [(k, err(got[k], ref[k]), err(cmp_[k], ref[k])) for k in ref]
    check_rows(rows, "n=%d chunks=%s ident1=%d" % (n, n_chunks, ident1))


# ------------------------------------------------------------------ 2. LaneConvFn against stock autograd
def torch_lane_conv(x, us, vs, W_ctr, W_rel, g1, b1, W2, g2, b2, masks=None):
    """Stock-autograd statement of one LaneConv layer (reference lanegcn.py:331-362); no relations: a LinearRes.
    masks = (Y > 0, out > 0) of a HIP forward: the ReLUs as multiplications by them, so that a pre-activation within
    rounding of zero cannot put the reference on the other side of a ReLU than the code under test."""
    F = torch.nn.functional
    t = F.linear(x, W_ctr)
    for u, v, w in zip(us, vs, W_rel):
        t = t.index_add(0, u, F.linear(x[v], w))
    y = F.group_norm(t, 1, g1, b1, EPS)
    y = torch.relu(y) if masks is None else y * masks[0]
    z = F.group_norm(F.linear(y, W2), 1, g2, b2, EPS) + x
    return torch.relu(z) if masks is None else z * masks[1]


LEAVES = ("x", "w1", "w_rel0", "w_rel1", "w_rel2", "w_rel3", "w2", "g1", "b1", "g2", "b2")


def leaves_of(inp, to):
    d = {k: inp[k] for k in ("x", "w1", "w2", "g1", "b1", "g2", "b2")}
    d.update({"w_rel%d" % r: inp["w_rel"][r] for r in range(4)})
    return {k: to(d[k]).requires_grad_(True) for k in LEAVES}


@functools.lru_cache(maxsize=None)
def stock64(n, csr):
    inp = block_inputs(n, csr)
    p = leaves_of(inp, lambda t: t.double().clone())
    out = torch_lane_conv(p["x"], inp["us"], inp["vs"], p["w1"], [p["w_rel%d" % r] for r in range(4)] if csr else [], p["g1"],
                          p["b1"], p["w2"], p["g2"], p["b2"])
    out.backward(inp["d_out"].double())
    return out.detach(), {k: v.grad for k, v in p.items()}


def lane_conv_fn(mods, inp, csr, fused_bwd, x_grad=True):
    """LaneConvFn forward + backward on fresh device leaves: (out, leaves)."""
    M, A, ops, L, _ = mods
    n = inp["x"].shape[0]
    p = leaves_of(inp, lambda t: t.cuda())
    p["x"].requires_grad_(x_grad)
    rels, weights, kw = [A.Rel(0, 0, L.REL_IDENT)], [p["w1"]], {}
    if csr:
        ud, vd = [u.cuda() for u in inp["us"]], [v.cuda() for v in inp["vs"]]
        plan, plan_t = ops.csr_build(ud, vd, n), ops.csr_build(vd, ud, n)
        for r in range(4):
            if plan.n_edges[r] > 0:
                rels.append(A.Rel(0, len(weights), L.REL_CSR, r))
                weights.append(p["w_rel%d" % r])
        kw = dict(plan=plan, plan_t=plan_t)
    spec = A.BlockSpec(n_rows=n, rels=rels, gn=True, relu=True, has_res=True, fused_bwd=fused_bwd, **kw)
    out = A.LaneConvFn.apply(spec, p["x"], p["g1"], p["b1"], p["w2"], p["g2"], p["b2"], *weights)
    out.backward(inp["d_out"].cuda())
    return out.detach(), p


@pytest.mark.parametrize("mode", ["f32", "bf16x3", "f16x2"])
@pytest.mark.parametrize("csr", [True, False])
def test_function_against_stock_autograd(mods, mma_scope, count_fused, mode, csr):
    """Output, dX and every parameter gradient within 1e-4 of the tensor's scale (the bar of
    test_lane_conv_fn_gradients_vs_stock_autograd); the empty relation's gradient is None or zero."""
    mma_scope(mode)
    n = N_CSR if csr else 130
    inp = block_inputs(n, csr)
    out64, g64 = stock64(n, csr)
    out, p = lane_conv_fn(mods, inp, csr, True)
    assert count_fused == ["rel" if csr else "ident1"]
    assert err(out, out64) <= 1e-4
    for k in LEAVES:
        if k.startswith("w_rel") and (not csr or k == "w_rel2"):
            assert p[k].grad is None or float(p[k].grad.abs().max()) == 0.0, k
            continue
        e = err(p[k].grad, g64[k])
        print("%s csr=%d %-7s %.3e" % (mode, csr, k, e))
        assert e <= 1e-4, (mode, k, e)


# ------------------------------------------------------------------ 3. repeatable, mode-independent
@pytest.mark.parametrize("ident1", [False, True])
def test_repeatable_and_independent_of_the_matrix_mode(mods, mma_scope, ident1):
    inp = block_inputs(130)
    saved = forward_saved(mods, inp)
    runs = []
    for mode in ("f32", "f32", "f16x2"):
        mma_scope(mode)
        runs.append(entry(mods, inp, saved, ident1, n_chunks=3))
    names = (("dX", "d_w1") if ident1 else ("dT", "g2")) + VEC
    for r in runs[1:]:
        assert all(same_bits(runs[0][k], r[k]) and r[k] is not None for k in names), [k for k in names if not same_bits(runs[0][k], r[k])]


# ------------------------------------------------------------------ 4. ragged edge
def test_rows_past_n_rows_are_untouched(mods):
    inp = block_inputs(33)
    saved = forward_saved(mods, inp)
    dT, g2 = (torch.full((64, C), -7.5, device="cuda") for _ in range(2))
    got = entry(mods, inp, saved, False, dT=dT[:33], g2=g2[:33])
    torch.cuda.synchronize()
    assert got["dT"].data_ptr() == dT.data_ptr() and got["g2"].data_ptr() == g2.data_ptr()
    assert bool((dT[33:] == -7.5).all()) and bool((g2[33:] == -7.5).all())
    plain = entry(mods, inp, saved, False)
    assert same_bits(dT[:33], plain["dT"]) and same_bits(g2[:33], plain["g2"])
    assert all(bool(torch.isfinite(v).all()) for v in got.values())


# ------------------------------------------------------------------ 5. absent gradients
@pytest.mark.parametrize("ident1", [False, True])
def test_absent_gradients(mods, ident1):
    inp = block_inputs(130)
    saved = forward_saved(mods, inp)
    full = entry(mods, inp, saved, ident1, n_chunks=3)
    rows_out = ("dX",) if ident1 else ("dT", "g2")
    no_dx = entry(mods, inp, saved, ident1, n_chunks=3, want_dx=False)
    assert no_dx["dX" if ident1 else "g2"] is None
    assert all(same_bits(full[k], no_dx[k]) for k in full if k not in ("dX", "g2"))
    only_w2 = entry(mods, inp, saved, ident1, n_chunks=3, want=("d_w2",))
    assert set(only_w2) == set(rows_out) | {"d_w2"}
    assert all(same_bits(full[k], only_w2[k]) for k in only_w2)
    none = entry(mods, inp, saved, ident1, n_chunks=3, want=())
    assert set(none) == set(rows_out) and all(same_bits(full[k], none[k]) for k in none)
    if ident1:
        only_w1 = entry(mods, inp, saved, True, n_chunks=3, want=("d_w1", "d_b1"), want_dx=False)
        assert same_bits(full["d_w1"], only_w1["d_w1"]) and same_bits(full["d_b1"], only_w1["d_b1"])


def test_linear_res_input_without_grad(mods, mma_scope, count_fused):
    mma_scope("f32")
    inp = block_inputs(130)
    _, full = lane_conv_fn(mods, inp, False, True)
    _, part = lane_conv_fn(mods, inp, False, True, x_grad=False)
    assert count_fused == ["ident1", "ident1"]
    assert part["x"].grad is None and full["x"].grad is not None
    for k in ("w1", "w2", "g1", "b1", "g2", "b2"):
        assert same_bits(full[k].grad, part[k].grad), k


# ------------------------------------------------------------------ 6. module level
def randomize(module, seed):
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for name, p in module.named_parameters():
            if p.dim() == 2:
                p.copy_(torch.randn(p.shape, generator=g) * 0.08)
            elif name.endswith("weight"):
                p.copy_(torch.rand(p.shape, generator=g) + 0.5)
            else:
                p.copy_(torch.randn(p.shape, generator=g) * 0.1)
    return module


def linear_res_step(layers, mod, x0, w_out, flag):
    prev = layers.LinearRes.train_hip
    layers.LinearRes.train_hip = flag
    try:
        x = x0.clone().requires_grad_(True)
        mod.zero_grad(set_to_none=True)
        out = mod(x)
        (out * w_out).sum().backward()
    finally:
        layers.LinearRes.train_hip = prev
    res = {"out": out.detach(), "d x": x.grad}
    res.update({n: p.grad.clone() for n, p in mod.named_parameters()})
    return res


def linear_res_reference64(mods, mod, x0, w_out, fwd_out, mode):
    """The block in float64 stock autograd on the CPU, the ReLUs taken as multiplications by the masks of the HIP forward in
    `mode`, which is checked to be the forward under test (fwd_out)."""
    with torch.no_grad():
        _, Y, _, out = hip_forward(mods, x0, mod.linear1.weight, [], None, mod.norm1.weight, mod.norm1.bias, mod.linear2.weight,
                                   mod.norm2.weight, mod.norm2.bias, mode=mode)
    assert torch.equal(out, fwd_out)
    masks = ((Y > 0).cpu().double(), (out > 0).cpu().double())
    p = {n: v.detach().cpu().double().requires_grad_(True) for n, v in mod.named_parameters()}
    x = x0.cpu().double().requires_grad_(True)
    out = torch_lane_conv(x, [], [], p["linear1.weight"], [], p["norm1.weight"], p["norm1.bias"], p["linear2.weight"],
                          p["norm2.weight"], p["norm2.bias"], masks=masks)
    (out * w_out.cpu().double()).sum().backward()
    res = {"out": out.detach(), "d x": x.grad}
    res.update({n: v.grad for n, v in p.items()})
    return res


def test_linear_res_on_against_off(mods, mma_scope, count_fused):
    M, A, ops, L, layers = mods
    mma_scope("f32")
    g = torch.Generator().manual_seed(5)
    mod = randomize(layers.LinearRes(C, C, norm="GN", ng=1), 21).cuda().train()
    x0, w_out = torch.randn(130, C, generator=g).cuda(), torch.randn(130, C, generator=g).cuda()
    off = linear_res_step(layers, mod, x0, w_out, False)
    assert not count_fused
    on = linear_res_step(layers, mod, x0, w_out, True)
    assert count_fused == ["ident1"]
    assert torch.equal(on["out"], off["out"])
    ref = linear_res_reference64(mods, mod, x0, w_out, on["out"], "f32")
    assert set(ref) == set(on) and all(v is not None for v in on.values())
    check_rows([(k, err(on[k], ref[k]), err(off[k], ref[k])) for k in ref], "LinearRes")


def lane_conv_step(M, fuse, graph, x0, w_out, flag):
    x = x0.clone().requires_grad_(True)
    fuse.zero_grad(set_to_none=True)
    out = M.lane_conv_train(fuse, x, M.lane_plan(graph), M.lane_plan_t(graph), len(graph["pre"]), fused_bwd=flag)
    (out * w_out).sum().backward()
    res = {"out": out.detach(), "d x": x.grad}
    res.update({n: p.grad.clone() for n, p in fuse.named_parameters() if p.grad is not None})
    return res


def lane_conv_masks(mods, fuse, graph, x0):
    """(Y > 0, out > 0) of every layer of the HIP forward in f32 mode, on the CPU as float64, and the last layer's output."""
    M = mods[0]
    plan, keys = M.lane_plan(graph), M.rel_keys(len(graph["pre"]))
    masks, feat = [], x0
    with torch.no_grad():
        for i in range(4):
            rel_ws = [(fuse[k][i].weight, r) for r, k in enumerate(keys) if plan.n_edges[r] > 0]
            c2 = fuse["ctr2"][i]
            _, Y, _, feat = hip_forward(mods, feat, fuse["ctr"][i].weight, rel_ws, plan, fuse["norm"][i].weight,
                                        fuse["norm"][i].bias, c2.linear.weight, c2.norm.weight, c2.norm.bias)
            masks.append(((Y > 0).cpu().double(), (feat > 0).cpu().double()))
    return masks, feat


def lane_conv_reference64(M, fuse, graph, x0, w_out, masks):
    """The four LaneConv layers in float64 stock autograd on the CPU (reference lanegcn.py:331-362), the ReLUs taken as
    multiplications by the HIP forward's masks."""
    p = {n: v.detach().cpu().double().requires_grad_(True) for n, v in fuse.named_parameters()}
    keys = M.rel_keys(len(graph["pre"]))
    edges = []
    for i in range(len(graph["pre"])):
        edges += [graph["pre"][i], graph["suc"][i]]
    edges += [graph["left"], graph["right"]]
    us, vs = [e["u"].cpu() for e in edges], [e["v"].cpu() for e in edges]
    x = x0.cpu().double().requires_grad_(True)
    feat = x
    for i in range(4):
        feat = torch_lane_conv(feat, us, vs, p["ctr.%d.weight" % i], [p["%s.%d.weight" % (k, i)] for k in keys],
                               p["norm.%d.weight" % i], p["norm.%d.bias" % i], p["ctr2.%d.linear.weight" % i],
                               p["ctr2.%d.norm.weight" % i], p["ctr2.%d.norm.bias" % i], masks=masks[i])
    (feat * w_out.cpu().double()).sum().backward()
    res = {"out": feat.detach(), "d x": x.grad}
    res.update({n: v.grad for n, v in p.items() if v.grad is not None})
    return res


def test_lane_conv_on_against_off(mods, mma_scope, count_fused, golden):
    """lane_conv_train (four layers) on the batch-4 golden graph, fused backward on and off, f32 mode."""
    M, A, ops, L, layers = mods
    mma_scope("f32")
    scenes = [to_torch_scene(s) for s in load_scenes(golden)]
    graph = M.graph_gather([s["graph"] for s in scenes])
    n = graph["feats"].shape[0]
    ns = len(graph["pre"])
    g = torch.Generator().manual_seed(9)
    fuse = randomize(M._fuse_modules(C, ns), 31).cuda().train()
    x0, w_out = torch.randn(n, C, generator=g).cuda(), torch.randn(n, C, generator=g).cuda()
    off = lane_conv_step(M, fuse, graph, x0, w_out, False)
    assert not count_fused
    on = lane_conv_step(M, fuse, graph, x0, w_out, True)
    assert count_fused == ["rel"] * 4
    assert torch.equal(on["out"], off["out"])
    masks, feat = lane_conv_masks(mods, fuse, graph, x0)
    assert torch.equal(feat, on["out"])                                  # the masks are those of the forward under test
    ref = lane_conv_reference64(M, fuse, graph, x0, w_out, masks)
    live = [k for k in ref if k in on]
    assert set(on) == set(off) and {"out", "d x", "ctr.0.weight", "ctr2.3.norm.bias", "norm.0.weight", "pre0.0.weight"} <= set(live)
    check_rows([(k, err(on[k], ref[k]), err(off[k], ref[k])) for k in live if float(ref[k].abs().max()) > 0], "lane_conv n=%d" % n)


# ------------------------------------------------------------------ 7. whole steps
@pytest.mark.parametrize("mode", ["f32", "f16x2"])
def test_whole_net_training_step(mods, hip_on, mma_scope, count_fused, golden, train_golden, ref_state_names, mode):
    """All three switches on: the reference's own loss, gradients and Adam update (tests/golden/train_b4.npz), the body and
    the bars of test_training_step_matches_reference; all 8 LaneConv layers and all 7 LinearRes blocks took the fused route."""
    mma_scope(mode)
    TG.test_training_step_matches_reference(golden, train_golden, ref_state_names, mode)
    assert sorted(count_fused) == ["ident1"] * 7 + ["rel"] * 8, count_fused


@pytest.mark.parametrize("mode", ["f32", "f16x2"])
def test_batch32_training_step(mods, hip_on, count_fused, ref_state_names, mode):
    """The training step at batch 32 (S2) with the switches on against the reference's own loss and gradients
    (tests/golden/train_b32.npz): the body and the bars of test_training_step_batch32_matches_reference."""
    TG.test_training_step_batch32_matches_reference(ref_state_names, mode)
    assert sorted(count_fused) == ["ident1"] * 7 + ["rel"] * 8, count_fused


def test_switches_off_mean_untouched(mods, mma_scope, count_fused, golden, ref_state_names):
    """Off by default: a Net step calls the fused entry never; on: 8 LaneConv layers + 7 LinearRes blocks."""
    M, A, ops, L, layers = mods
    from lanegcn_amd import data as gen
    from oracle import lanegcn_oracle as O
    mma_scope("f16x2")
    assert not (M.MapNet.train_hip or M.M2M.train_hip or layers.LinearRes.train_hip)
    net = M.Net(M.config)
    net.load_state_dict(O.seeded_state(ref_state_names, 1), strict=True)
    net = net.cuda().train()
    batch = gen.collate_fn(load_scenes(golden))
    loss_fn = M.Loss(M.config).cuda()
    loss_fn(net(batch), batch)["loss"].backward()
    assert not count_fused
    M.MapNet.train_hip = M.M2M.train_hip = layers.LinearRes.train_hip = True
    try:
        loss_fn(net(batch), batch)["loss"].backward()
    finally:
        M.MapNet.train_hip = M.M2M.train_hip = layers.LinearRes.train_hip = False
    assert sorted(count_fused) == ["ident1"] * 7 + ["rel"] * 8, count_fused


# ------------------------------------------------------------------ 8. optimizer step
def test_fresh_images_after_optimizer_step(mods, mma_scope, count_fused):
    """After Optimizer.step the cached transposed F32 images of W1 and W2 are rebuilt: the fused gradients of the second step
    meet the bar of test_entry_against_fp64 against float64 on the updated weights."""
    M, A, ops, L, layers = mods
    mma_scope("f16x2")
    g = torch.Generator().manual_seed(6)
    mod = randomize(layers.LinearRes(C, C, norm="GN", ng=1), 22).cuda().train()
    x0, w_out = torch.randn(130, C, generator=g).cuda(), torch.randn(130, C, generator=g).cuda()
    linear_res_step(layers, mod, x0, w_out, True)
    opt = M.Optimizer(mod.parameters(), M.config)
    before = {k: v.clone() for k, v in mod.state_dict().items()}
    opt.step(0.0)
    assert all(not torch.equal(before[k], v) for k, v in mod.state_dict().items())
    on = linear_res_step(layers, mod, x0, w_out, True)
    assert count_fused == ["ident1", "ident1"]
    off = linear_res_step(layers, mod, x0, w_out, False)
    assert torch.equal(on["out"], off["out"])
    ref = linear_res_reference64(mods, mod, x0, w_out, on["out"], "f16x2")
    check_rows([(k, err(on[k], ref[k]), err(off[k], ref[k])) for k in ref], "after step")
