"""GPU: every backward over gradient scale and GroupNorm statistics (builders and float64 references: backward_cases.py).

Part A -- gradient scale.  A backward is linear in its incoming gradient and a power of two commutes with every fp32 rounding
and with the three-way bf16 split, so for every autograd Function grad(2^k d_out) == 2^k grad(d_out) BIT FOR BIT on the same
saved forward, k in (-40, -20, +20), in the matrix modes f32, bf16x3 and f16x2 (the mode is set for the forward and stays set:
the default-mode case is an f16x2 forward with its backward behind it).  An fp16 plane or an absolute threshold anywhere on a
gradient path breaks it: at k = -40 gradients sit near 1e-12, far below fp16's normal range, which is what ops.backward_mma is
for.  test_disabled_backward_mma_is_seen is the committed negative control.  At k = 0 every Function is compared once, in f32
mode, with float64 stock autograd that takes its ReLU decisions from the HIP forward, at the bar of Part B (the other modes at
k = 0 are held by the test_function_against_stock_autograd tests of the Functions' own files).

Part B -- statistics.  The backward entries on saved tensors that are set directly: 130 rows (5 actors / 5 or 37 items for the
conv norms) interleave the row classes ordinary / flat / offset / constant / dead of backward_cases.py, gamma is log-uniform in
[2^-8, 2^2] with random signs and exact zeros, the 128-wide weights are at 2^0, 2^-12 and 2^4 of the usual 0.08.  Error:
rel_err = max |got - ref| / max |ref| per row class for row tensors, per tensor for parameter gradients, no absolute floor.
Bar: bar(e_cmp) = min(max(2 e_cmp, 1e-6), 1e-4), e_cmp the error of stock fp32 autograd on ATen's CPU kernels (same inputs, same masks)
against the same float64: deterministic, and the figures test_backward_cases_host.py prints.  Dead rows are exactly zero.  Everything is printed before it is asserted.

Part C -- rows of magnitude 2^70 (f32 mode): the forward's GroupNorm takes row_rstd_wide there, and so do k_gn_bwd and
row_gn_hat; stock fp32 overflows on them, so e_cmp is useless and the bar is its 1e-4 ceiling."""
import types

import pytest
import torch

import backward_cases as B
import roi_loss_model as RM
import test_gpu_att_train as TA
import test_gpu_goal_decode_train as GD
import test_gpu_laneconv_train as LC
import test_gpu_prednet_train as PN
import test_gpu_roi_loss as RL
import test_gpu_rowblock_train as RB

pytestmark = pytest.mark.gpu

C, EPS, F = B.C, B.EPS, torch.nn.functional
MODES = ["f32", "bf16x3", "f16x2"]
ROW_TENSORS = {"dx", "g", "dT", "g2", "dX", "d res", "d src0", "d src1", "dres"}


@pytest.fixture(scope="module")
def mods():
    import lanegcn_amd  # noqa: F401
    from lanegcn_amd import _lib as L
    from lanegcn_amd import autograd as A
    from lanegcn_amd import lanegcn as M
    from lanegcn_amd import ops
    return M, A, ops, L


@pytest.fixture
def mma_scope(mods):
    ops = mods[2]
    prev = ops.get_mma()
    yield ops.set_mma
    ops.set_mma(prev)


def cuda_leaves(d):
    return {k: v.detach().cuda().requires_grad_(True) for k, v in d.items()}


def assert_homogeneous(outs, leaves, d_outs, label):
    """Part A's statement for one retained forward; returns the gradients at k = 0."""
    bad, base = B.homogeneous(outs, leaves, d_outs)
    assert not bad, (label, bad)
    assert any(v is not None and float(v.abs().max()) > 0 for v in base.values()), label
    return base


def assert_anchored(label, got, ref, cmp_):
    """k = 0 against float64 at bar(e_cmp), per tensor (ref / cmp_: {leaf: gradient} in float64 / stock fp32)."""
    rows = [(k, B.rel_err(got[k], ref[k]), B.rel_err(cmp_[k], ref[k])) for k in ref if ref[k] is not None]
    for k, e, ec in rows:
        print("%s %-10s hip %.3e stock fp32 %.3e" % (label, k, e, ec))
    bad = [r for r in rows if not r[1] <= B.bar(r[2])]
    assert not bad, (label, bad)


# ================================================================== Part A
# ------------------------------------------------------------------ RowBlockFn, IDENT relations
def rb_forward(mods, inp, shape, fused):
    M, A, ops, L = mods
    s = RB.SHAPES[shape]
    p = RB.leaves_of(inp, shape, lambda t: t.cuda())
    gn = types.SimpleNamespace(weight=p["gamma"], bias=p["beta"], eps=EPS) if s["gn"] else None
    out = A.row_block([p["src%d" % i] for i in range(RB.n_src(shape))], [p["w%d" % k] for k in range(len(s["K"]))],
                      [A.Rel(si, wi, L.REL_IDENT, 0, c0) for si, wi, c0 in s["rels"]], inp["d_out"].shape[0], gn=gn, relu=s["relu"],
                      res=p.get("res"), fused_bwd=fused)
    return out, p


def rb_stock(inp, shape, out, dtype, device):
    p = RB.leaves_of(inp, shape, lambda t: t.to(device=device, dtype=dtype).clone())
    RB.forward64(p, shape, (out > 0).to(device=device, dtype=dtype)).backward(inp["d_out"].to(device=device, dtype=dtype))
    return {k: v.grad for k, v in p.items()}


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("shape", sorted(RB.SHAPES))
def test_row_block_composed(mods, mma_scope, mode, shape):
    """IDENT blocks a-g of test_gpu_rowblock_train (with and without GN, ReLU, residual; column blocks of [128,384] / [128,256]
    / [128,132] weights) at n = 1, 33, 130: the composed backward (gn_bwd, agg_mlp under backward_mma, wgrad)."""
    mma_scope(mode)
    for n in (1, 33, 130):
        inp = RB.block_inputs(n, shape)
        out, p = rb_forward(mods, inp, shape, False)
        base = assert_homogeneous([out], p, [inp["d_out"].cuda()], "%s %s n=%d" % (mode, shape, n))
        if mode == "f32" and n == 130:
            assert_anchored("row_block %s" % shape, base, rb_stock(inp, shape, out.detach().cpu(), torch.float64, "cpu"),
                            rb_stock(inp, shape, out.detach(), torch.float32, "cpu"))


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("n_chunks", [1, 2, 3])
def test_row_block_fused(mods, mma_scope, monkeypatch, mode, n_chunks):
    """The same blocks on lgcn_rowblock_bwd (RowBlockFn.train_hip's route) with 1, 2 and 3 workgroups at n = 130."""
    ops = mods[2]
    mma_scope(mode)
    real, calls = ops.rowblock_bwd, []

    def chunked(*a, **kw):
        calls.append(1)
        return real(*a, **dict(kw, n_chunks=n_chunks))

    monkeypatch.setattr(ops, "rowblock_bwd", chunked)
    for shape in sorted(RB.SHAPES):
        inp = RB.block_inputs(130, shape)
        out, p = rb_forward(mods, inp, shape, True)
        base = assert_homogeneous([out], p, [inp["d_out"].cuda()], "%s fused %s chunks=%d" % (mode, shape, n_chunks))
        if mode == "f32" and n_chunks == 3:
            assert_anchored("row_block fused %s" % shape, base, rb_stock(inp, shape, out.detach().cpu(), torch.float64, "cpu"),
                            rb_stock(inp, shape, out.detach(), torch.float32, "cpu"))
    assert len(calls) == 4 * len(RB.SHAPES)


# ------------------------------------------------------------------ RowBlockFn, CSR and RANGE relations
def csr_block(mods):
    """GN + ReLU over an IDENT and the CSR relations of the 70-node multigraph of LC.block_inputs (one empty relation, duplicate
    edges, nodes without in-edges)."""
    M, A, ops, L = mods
    inp = LC.block_inputs(LC.N_CSR, True)
    n = LC.N_CSR
    p = cuda_leaves(dict(x=inp["x"], w1=inp["w1"], gamma=inp["g1"], beta=inp["b1"], **{"w_rel%d" % r: inp["w_rel"][r] for r in range(4)}))
    ud, vd = [u.cuda() for u in inp["us"]], [v.cuda() for v in inp["vs"]]
    plan, plan_t = ops.csr_build(ud, vd, n), ops.csr_build(vd, ud, n)
    rels, weights = [A.Rel(0, 0, L.REL_IDENT)], [p["w1"]]
    for r in range(4):
        if plan.n_edges[r] > 0:
            rels.append(A.Rel(0, len(weights), L.REL_CSR, r))
            weights.append(p["w_rel%d" % r])
    gn = types.SimpleNamespace(weight=p["gamma"], bias=p["beta"], eps=EPS)
    out = A.row_block([p["x"]], weights, rels, n, gn=gn, relu=True, plan=plan, plan_t=plan_t)
    leaves = {k: v for k, v in p.items() if k != "w_rel2"}              # the empty relation takes no part
    assert plan.n_edges[2] == 0

    def stock(mask, dtype, device):
        q = {k: v.detach().to(device=device, dtype=dtype).requires_grad_(True) for k, v in leaves.items()}
        t = F.linear(q["x"], q["w1"])
        for r in (0, 1, 3):
            t = t.index_add(0, inp["us"][r].to(device), F.linear(q["x"][inp["vs"][r].to(device)], q["w_rel%d" % r]))
        (F.group_norm(t, 1, q["gamma"], q["beta"], EPS) * mask.to(device=device, dtype=dtype)).backward(
            inp["d_out"].to(device=device, dtype=dtype))
        return {k: v.grad for k, v in q.items()}

    return out, leaves, inp["d_out"].cuda(), stock


def range_block(mods):
    """GN + ReLU over an IDENT and a RANGE relation, as Att builds att_post: 33 targets with segments of 0..4 rows."""
    M, A, ops, L = mods
    g = torch.Generator().manual_seed(4)
    T = 33
    lens = torch.randint(0, 5, (T,), generator=g)
    P = int(lens.sum())
    assert P > 0 and bool((lens == 0).any())
    rowptr = torch.zeros(T + 1, dtype=torch.int32)
    rowptr[1:] = torch.cumsum(lens, 0).to(torch.int32)
    hi = torch.repeat_interleave(torch.arange(T), lens)
    cpu = dict(agts=torch.randn(T, C, generator=g), m=torch.randn(P, C, generator=g), w0=torch.randn(C, C, generator=g) * 0.08,
               w1=torch.randn(C, C, generator=g) * 0.08, gamma=torch.rand(C, generator=g) + 0.5, beta=torch.randn(C, generator=g) * 0.1)
    d_out = torch.randn(T, C, generator=g)
    p = cuda_leaves(cpu)
    gn = types.SimpleNamespace(weight=p["gamma"], bias=p["beta"], eps=EPS)
    out = A.row_block([p["agts"], p["m"]], [p["w0"], p["w1"]], [A.Rel(0, 0, L.REL_IDENT), A.Rel(1, 1, L.REL_RANGE)], T, gn=gn,
                      relu=True, rowptr=rowptr.cuda(), seg_ids=hi.to(torch.int32).cuda(),
                      n_seg_rows=torch.tensor([P], dtype=torch.int32).cuda(), tag="att_post")

    def stock(mask, dtype, device):
        q = {k: v.to(device=device, dtype=dtype).requires_grad_(True) for k, v in cpu.items()}
        S = torch.zeros(T, C, dtype=dtype, device=device).index_add(0, hi.to(device), q["m"])
        t = F.linear(q["agts"], q["w0"]) + F.linear(S, q["w1"])
        (F.group_norm(t, 1, q["gamma"], q["beta"], EPS) * mask.to(device=device, dtype=dtype)).backward(
            d_out.to(device=device, dtype=dtype))
        return {k: v.grad for k, v in q.items()}

    return out, p, d_out.cuda(), stock


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("block", [csr_block, range_block])
def test_row_block_csr_and_range(mods, mma_scope, mode, block):
    mma_scope(mode)
    out, leaves, d_out, stock = block(mods)
    base = assert_homogeneous([out], leaves, [d_out], "%s %s" % (mode, block.__name__))
    if mode == "f32":
        mask = out.detach() > 0
        assert_anchored(block.__name__, base, stock(mask.cpu(), torch.float64, "cpu"), stock(mask, torch.float32, "cpu"))


# ------------------------------------------------------------------ LaneConvFn
def lane_conv_forward(mods, inp, csr, fused):
    """LaneConvFn on fresh device leaves, as LC.lane_conv_fn builds it: (out, leaves that take part)."""
    M, A, ops, L = mods
    n = inp["x"].shape[0]
    p = LC.leaves_of(inp, lambda t: t.cuda())
    rels, weights, kw = [A.Rel(0, 0, L.REL_IDENT)], [p["w1"]], {}
    live = ["x", "w1", "w2", "g1", "b1", "g2", "b2"]
    if csr:
        ud, vd = [u.cuda() for u in inp["us"]], [v.cuda() for v in inp["vs"]]
        plan, plan_t = ops.csr_build(ud, vd, n), ops.csr_build(vd, ud, n)
        for r in range(4):
            if plan.n_edges[r] > 0:
                rels.append(A.Rel(0, len(weights), L.REL_CSR, r))
                weights.append(p["w_rel%d" % r])
                live.append("w_rel%d" % r)
        kw = dict(plan=plan, plan_t=plan_t)
    spec = A.BlockSpec(n_rows=n, rels=rels, gn=True, relu=True, has_res=True, fused_bwd=fused, **kw)
    out = A.LaneConvFn.apply(spec, p["x"], p["g1"], p["b1"], p["w2"], p["g2"], p["b2"], *weights)
    return out, {k: p[k] for k in live}


def lane_conv_stock(mods, inp, csr, out, names, dtype, device):
    """torch_lane_conv with the masks of the HIP forward in f32 mode, which is checked to be the forward under test."""
    ops = mods[2]
    d = {k: inp[k].cuda() for k in ("x", "w1", "g1", "b1", "w2", "g2", "b2")}
    plan, rel_ws = None, []
    if csr:
        plan = ops.csr_build([u.cuda() for u in inp["us"]], [v.cuda() for v in inp["vs"]], d["x"].shape[0])
        rel_ws = [(inp["w_rel"][r].cuda(), r) for r in range(4) if plan.n_edges[r] > 0]
    with torch.no_grad():
        _, Y, _, o = LC.hip_forward((*mods, None), d["x"], d["w1"], rel_ws, plan, d["g1"], d["b1"], d["w2"], d["g2"], d["b2"], mode="f32")
    assert torch.equal(o, out)
    to = lambda t: t.to(device=device, dtype=dtype)
    p = LC.leaves_of(inp, lambda t: to(t).clone())
    us, vs = [u.to(device) for u in inp["us"]], [v.to(device) for v in inp["vs"]]
    res = LC.torch_lane_conv(p["x"], us, vs, p["w1"], [p["w_rel%d" % r] for r in range(4)] if csr else [], p["g1"], p["b1"], p["w2"],
                             p["g2"], p["b2"], masks=(to(Y > 0), to(o > 0)))
    res.backward(to(inp["d_out"]))
    return {k: p[k].grad for k in names}


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("fused", [False, True])
@pytest.mark.parametrize("n,csr", [(33, False), (130, False), (LC.N_CSR, True)])
def test_lane_conv(mods, mma_scope, mode, fused, n, csr):
    """LaneConvFn, composed and on lgcn_laneconv_bwd: the ident1 / LinearRes form at n = 33, 130 and the 70-node CSR multigraph."""
    mma_scope(mode)
    inp = LC.block_inputs(n, csr)
    out, leaves = lane_conv_forward(mods, inp, csr, fused)
    base = assert_homogeneous([out], leaves, [inp["d_out"].cuda()], "%s fused=%d n=%d csr=%d" % (mode, fused, n, csr))
    if mode == "f32" and n != 33:
        assert_anchored("lane_conv fused=%d csr=%d" % (fused, csr), base,
                        lane_conv_stock(mods, inp, csr, out.detach(), list(leaves), torch.float64, "cpu"),
                        lane_conv_stock(mods, inp, csr, out.detach(), list(leaves), torch.float32, "cpu"))


# ------------------------------------------------------------------ Att's pair stage: AttPairsFn, and composed (GNActFn, PairAddFn,
# GatherSumFn around two row blocks)
def att_stock(inp, hi, wi, masks, dtype, device, want_dc=False):
    """TA.reference64's graph in `dtype` on `device`: gradients by name (w_c0: columns 0:128)."""
    to = lambda t: t.to(device=device, dtype=dtype)
    x = {k: to(inp[k]).requires_grad_(True) for k in TA.NAMES if k != "w_c0"}
    wc = to(inp["w_c0"][:, :C]).requires_grad_(True)
    mk, hi, wi = to(masks), hi.to(device), wi.to(device)
    gn = lambda v, ga, be: F.group_norm(v, 1, ga, be, EPS)
    d = to(inp["agt_ctrs"])[hi] - to(inp["ctx_ctrs"])[wi]
    z0 = d @ x["wd0"].t() + x["bd0"]
    y1 = gn((z0 * mk[:, 0]) @ x["w_d2"].t(), x["gd"], x["btd"])
    c = (y1 * mk[:, 1]) @ wc.t() + x["U"][hi] + x["V"][wi]
    c.retain_grad()
    y2 = gn(c, x["gc"], x["btc"])
    Sx = torch.zeros(TA.T, C, dtype=dtype, device=device).index_add(0, hi, y2 * mk[:, 2])
    Sx.backward(to(inp["dS"]))
    grads = {k: v.grad for k, v in x.items()}
    grads["w_c0"] = wc.grad
    if want_dc:
        grads["dc"] = c.grad
        grads["c"] = c.detach()
    return grads


def att_composed_forward(mods, ps, x, P):
    """The pair stage as Att.run_train composes it (TA.composed's lines): (S, the masks [P, 3, 128] of its three ReLUs)."""
    M, A, ops, L = mods
    hi, wi = ps.hi[:P].long(), ps.wi[:P].long()
    gn = lambda w, b: types.SimpleNamespace(weight=w, bias=b, eps=EPS)
    delta = ps.agt_ctrs[hi] - ps.ctx_ctrs[wi]
    h1 = torch.relu(F.linear(delta, x["wd0"], x["bd0"]))
    e = A.linear_gn(h1, x["w_d2"], gn=gn(x["gd"], x["btd"]), relu=True)
    c = A.PairAddFn.apply(A.linear_gn(e, x["w_c0"], col0=0), x["U"], x["V"], ps)
    m = A.gn_act(c, gn=gn(x["gc"], x["btc"]), relu=True)
    i32 = dict(dtype=torch.int32, device="cuda")
    plan = types.SimpleNamespace(rowptr=ps.rowptr, col=None)
    plan_t = types.SimpleNamespace(rowptr=torch.arange(P + 1, **i32), col=ps.hi[:P].contiguous())
    S = A.GatherSumFn.apply(m, plan, plan_t, TA.T)
    return S, torch.stack([h1.detach() > 0, e.detach() > 0, m.detach() > 0], 1)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("fused", [False, True])
@pytest.mark.parametrize("P", [33, 70])
def test_att_pair_stage(mods, mma_scope, mode, fused, P):
    """AttPairsFn (Att.train_hip on) and the composed pair stage (off: two row blocks, PairAddFn, GNActFn, GatherSumFn) on the
    pair sets of test_gpu_att_train: 9 targets (two without a pair), a segment across the first tile boundary."""
    M, A, ops, L = mods
    mma_scope(mode)
    ps, inp, hi, wi = TA.make_case(ops, P)
    x = TA.leaves(inp)
    if fused:
        S = TA.fused(A, ps, x)
        d = {k: v.detach() for k, v in x.items()}
        _, raw = ops.att_pairs_train(ps, d["wd0"], d["bd0"], d["w_d2"], (d["gd"], d["btd"]), d["w_c0"], d["U"], d["V"], (d["gc"], d["btc"]))
        masks = ops.att_pair_masks(raw, P)
    else:
        S, masks = att_composed_forward(mods, ps, x, P)
    base = assert_homogeneous([S], x, [inp["dS"].cuda()], "%s att fused=%d P=%d" % (mode, fused, P))
    if mode == "f32":
        assert bool((base["w_c0"][:, C:] == 0).all())
        base = dict(base, w_c0=base["w_c0"][:, :C])
        assert_anchored("att pairs fused=%d P=%d" % (fused, P), base, att_stock(inp, hi, wi, masks.cpu(), torch.float64, "cpu"),
                        att_stock(inp, hi, wi, masks, torch.float32, "cpu"))


# ------------------------------------------------------------------ ActorNet's units: Conv1dGNFn, GNCLFn
def conv_fn_inputs(unit):
    cin, cout, ks, stride, res_mode = B.CONV_UNITS[unit]
    g = torch.Generator().manual_seed(300 + cin + cout)
    lout = (B.CONV_L + 2 * ((ks - 1) // 2) - ks) // stride + 1
    rnd = lambda *s: torch.randn(*s, generator=g)
    d = dict(x=rnd(B.CONV_A, B.CONV_L, cin) * 2 + 0.3, w=rnd(cout, cin, ks) * (1.0 / (cin * ks) ** 0.5),
             gamma=torch.rand(cout, generator=g) + 0.5, beta=torch.rand(cout, generator=g) - 0.5)
    if res_mode:
        d["res"] = rnd(B.CONV_A, lout // 2 if res_mode == 2 else lout, cout)
    return d, rnd(B.CONV_A, lout, cout)


def conv_fn_stock(unit, cpu, d_out, mask, dtype, device):
    cin, cout, ks, stride, res_mode = B.CONV_UNITS[unit]
    to = lambda t: t.to(device=device, dtype=dtype)
    q = {k: (to(v).transpose(1, 2).contiguous() if k in ("x", "res") else to(v)).requires_grad_(True) for k, v in cpu.items()}
    o = F.group_norm(F.conv1d(q["x"], q["w"], stride=stride, padding=(ks - 1) // 2), 1, q["gamma"], q["beta"], EPS)
    if res_mode:
        o = o + (B.up2(q["res"]) if res_mode == 2 else q["res"])
    (o * to(mask).transpose(1, 2)).backward(to(d_out).transpose(1, 2))
    return {k: (v.grad.transpose(1, 2) if k in ("x", "res") else v.grad) for k, v in q.items()}


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("unit", sorted(B.CONV_UNITS))
def test_conv1d_gn_fn(mods, mma_scope, mode, unit):
    """Conv1dGNFn on 5 actors of length 20: ActorNet's first unit, a strided one with a residual, the lateral 1x1 with the
    x2-upsampled residual."""
    M, A, ops, L = mods
    mma_scope(mode)
    cin, cout, ks, stride, res_mode = B.CONV_UNITS[unit]
    cpu, d_out = conv_fn_inputs(unit)
    p = cuda_leaves(cpu)
    out = A.Conv1dGNFn.apply(p["x"], p["w"], p["gamma"], p["beta"], p.get("res"), stride, res_mode, True, EPS, mode == "f32")
    base = assert_homogeneous([out], p, [d_out.cuda()], "%s conv %s" % (mode, unit))
    if mode == "f32":
        mask = out.detach() > 0
        assert_anchored("conv %s" % unit, base, conv_fn_stock(unit, cpu, d_out, mask.cpu(), torch.float64, "cpu"),
                        conv_fn_stock(unit, cpu, d_out, mask, torch.float32, "cpu"))


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("shape", [(5, 128, 5), (37, 64, 10)])
def test_gn_cl_fn(mods, mma_scope, mode, shape):
    M, A, ops, L = mods
    mma_scope(mode)
    g = torch.Generator().manual_seed(shape[0])
    n, c, l = shape
    cpu = dict(x=torch.randn(n, c, l, generator=g) * 2 + 0.3, gamma=torch.rand(c, generator=g) + 0.5, beta=torch.rand(c, generator=g) - 0.5,
               res=torch.randn(n, c, l, generator=g))
    d_out = torch.randn(n, c, l, generator=g)
    p = cuda_leaves(cpu)
    out = A.GNCLFn.apply(p["x"], p["gamma"], p["beta"], p["res"], True, EPS)
    base = assert_homogeneous([out], p, [d_out.cuda()], "%s gn_cl %s" % (mode, shape))
    if mode == "f32":
        def stock(dtype, device):
            q = {k: v.to(device=device, dtype=dtype).requires_grad_(True) for k, v in cpu.items()}
            o = (F.group_norm(q["x"], 1, q["gamma"], q["beta"], EPS) + q["res"]) * (out.detach() > 0).to(device=device, dtype=dtype)
            o.backward(d_out.to(device=device, dtype=dtype))
            return {k: v.grad for k, v in q.items()}
        assert_anchored("gn_cl %s" % (shape,), base, stock(torch.float64, "cpu"), stock(torch.float32, "cpu"))


# ------------------------------------------------------------------ PredNet's tail, the losses, the goal decoder
def pred_reg_stock(inputs, hd_mask, dtype):
    h0, w0, b0, ctrs, wd0, bd0, w_reg, w_hd = inputs
    a, m, t = h0[0].shape[0], len(h0), w0[0].shape[0] // 2
    q = {"h%d" % i: v for i, v in enumerate(h0)}
    q.update({"w%d" % i: v for i, v in enumerate(w0)})
    q.update({"b%d" % i: v for i, v in enumerate(b0)})
    q.update(wd=wd0, bd=bd0)
    q = {k: v.to(dtype).clone().requires_grad_(True) for k, v in q.items()}
    c = ctrs.to(dtype)
    reg = torch.stack([q["h%d" % i] @ q["w%d" % i].t() + q["b%d" % i] for i in range(m)], 1).view(a, m, t, 2) + c.view(a, 1, 1, 2)
    d = (c.view(a, 1, 2) - reg[:, :, -1].detach()).reshape(-1, 2)
    hd = (d @ q["wd"].t() + q["bd"]) * hd_mask.to(dtype)
    ((reg * w_reg.to(dtype)).sum() + (hd * w_hd.to(dtype)).sum()).backward()
    return {k: v.grad for k, v in q.items()}


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("a,m,t", [(1, 6, 30), (33, 3, 7)])
def test_pred_reg_fn(mods, mma_scope, mode, a, m, t):
    M, A, ops, L = mods
    mma_scope(mode)
    inputs = PN.reg_inputs(a, m, t)
    h0, w0, b0, ctrs, wd0, bd0, w_reg, w_hd = inputs
    p = {"h%d" % i: v for i, v in enumerate(h0)}
    p.update({"w%d" % i: v for i, v in enumerate(w0)})
    p.update({"b%d" % i: v for i, v in enumerate(b0)})
    p = cuda_leaves(dict(p, wd=wd0, bd=bd0))
    reg, hd = A.PredRegFn.apply(*(p["h%d" % i] for i in range(m)), *(p["w%d" % i] for i in range(m)), *(p["b%d" % i] for i in range(m)),
                                ctrs.cuda(), p["wd"], p["bd"])
    base = assert_homogeneous([reg, hd], p, [w_reg.cuda(), w_hd.cuda()], "%s pred_reg %s" % (mode, (a, m, t)))
    if mode == "f32":
        mask = hd.detach().cpu() > 0
        assert_anchored("pred_reg %s" % ((a, m, t),), base, pred_reg_stock(inputs, mask, torch.float64),
                        pred_reg_stock(inputs, mask, torch.float32))


def pred_final_stock(inputs, order, dtype):
    f0, wc0, bc0, reg0, w_cls, w_out = inputs
    a, m = reg0.shape[:2]
    q = {k: v.to(dtype).clone().requires_grad_(True) for k, v in dict(f=f0, wc=wc0, bc=bc0, reg=reg0).items()}
    sc = (q["f"] @ q["wc"].t() + q["bc"]).view(a, m)
    rows = torch.arange(a).view(-1, 1).expand_as(order)
    ((sc[rows, order] * w_cls.to(dtype)).sum() + (q["reg"][rows, order] * w_out.to(dtype)).sum()).backward()
    return {k: v.grad for k, v in q.items()}


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("a,m,t", [(1, 6, 30), (33, 3, 7)])
def test_pred_final_fn(mods, mma_scope, mode, a, m, t):
    M, A, ops, L = mods
    mma_scope(mode)
    inputs = PN.final_inputs(a, m, t)
    f0, wc0, bc0, reg0, w_cls, w_out = inputs
    p = cuda_leaves(dict(f=f0, wc=wc0, bc=bc0, reg=reg0))
    cls, out = A.PredFinalFn.apply(p["f"], p["wc"], p["bc"], p["reg"])
    base = assert_homogeneous([cls, out], p, [w_cls.cuda(), w_out.cuda()], "%s pred_final %s" % (mode, (a, m, t)))
    if mode == "f32":
        order = PN.order_of(out, p["reg"]).cpu().long()
        assert_anchored("pred_final %s" % ((a, m, t),), base, pred_final_stock(inputs, order, torch.float64),
                        pred_final_stock(inputs, order, torch.float32))


def pred_loss_inputs(n):
    """The inputs of test_pred_loss_hip_equals_stock_composition: never-observed actors, one observed at t = 0 only, a tie."""
    g = torch.Generator().manual_seed(3)
    gt = torch.cumsum(torch.randn(n, 30, 2, generator=g), 1)
    reg = gt.unsqueeze(1) + 0.6 * torch.randn(n, 6, 30, 2, generator=g) * torch.rand(n, 6, 1, 1, generator=g) * 3
    reg[:, 2] = reg[:, 1]
    cls = torch.randn(n, 6, generator=g) * 0.3
    has = torch.rand(n, 30, generator=g) > 0.3
    has[::5] = False
    if n > 3:
        has[3] = False
        has[3, 0] = True
    return cls, reg, gt, has


UP = (0.37, 0.011, 0.0045)          # upstream gradients of the loss sums: 1 / count-sized


@pytest.mark.parametrize("mode", MODES)
def test_pred_loss_fn(mods, mma_scope, mode):
    M, A, ops, L = mods
    mma_scope(mode)
    cls0, reg0, gt, has = pred_loss_inputs(7)
    p = cuda_leaves(dict(cls=cls0, reg=reg0))
    c_loss, r_loss, _ = A.PredLossFn.apply(p["cls"], p["reg"], gt.cuda(), has.cuda(), M.config)
    d_outs = [torch.tensor(v, device="cuda") for v in UP[:2]]
    base = assert_homogeneous([c_loss, r_loss], p, d_outs, "%s pred_loss" % mode)
    if mode == "f32":
        def stock(dtype):
            q = {k: v.to(dtype).clone().requires_grad_(True) for k, v in dict(cls=cls0, reg=reg0).items()}
            lo = M.PredLoss(M.config)({"cls": [q["cls"]], "reg": [q["reg"]]}, [gt.to(dtype)], [has])
            (UP[0] * lo["cls_loss"] + UP[1] * lo["reg_loss"]).backward()
            return {k: v.grad for k, v in q.items()}
        assert_anchored("pred_loss", base, stock(torch.float64), stock(torch.float32))


@pytest.mark.parametrize("n", [1025, 4097])
def test_pred_loss_past_the_grid(mods, mma_scope, n):
    """1025 actors: more than one per thread of the forward's 1024-thread block.  4097: one more than the 4096 workgroups of
    k_pred_loss_bwd, so workgroup 0 strides on to a second actor.  Gradients and both sums against the stock composition in
    float64 at bar(error of the stock composition in fp32); the counts equal; zero exactly where float64 is zero."""
    M, A, ops, L = mods
    mma_scope("f32")
    cls0, reg0, gt, has = pred_loss_inputs(n)
    p = cuda_leaves(dict(cls=cls0, reg=reg0))
    c_loss, r_loss, counts = A.PredLossFn.apply(p["cls"], p["reg"], gt.cuda(), has.cuda(), M.config)
    d_outs = [torch.tensor(v, device="cuda") for v in UP[:2]]
    got = dict(zip(p, torch.autograd.grad([c_loss, r_loss], list(p.values()), d_outs)))

    def stock(dtype):
        q = {k: v.to(dtype).clone().requires_grad_(True) for k, v in dict(cls=cls0, reg=reg0).items()}
        lo = M.PredLoss(M.config)({"cls": [q["cls"]], "reg": [q["reg"]]}, [gt.to(dtype)], [has])
        (UP[0] * lo["cls_loss"] + UP[1] * lo["reg_loss"]).backward()
        return {k: v.grad for k, v in q.items()}, lo

    ref, lo64 = stock(torch.float64)
    cmp_, lo32 = stock(torch.float32)
    assert_anchored("pred_loss A=%d" % n, got, ref, cmp_)
    rel = lambda x, y: abs(x.item() - y.item()) / abs(y.item())
    sums = [(k, rel(v, lo64[k]), rel(lo32[k], lo64[k])) for k, v in (("cls_loss", c_loss), ("reg_loss", r_loss))]
    for k, e, ec in sums:
        print("pred_loss A=%d %-10s hip %.3e stock fp32 %.3e" % (n, k, e, ec))
    assert all(e <= B.bar(ec) for _, e, ec in sums), sums
    assert counts.tolist() == [lo64["num_cls"], lo64["num_reg"]] == [lo32["num_cls"], lo32["num_reg"]] and min(counts.tolist()) > 0
    for k in ref:                                          # dropped actors, unselected modes, unobserved steps
        zero = ref[k] == 0
        assert bool(zero[::5].all()), k                     # pred_loss_inputs: every fifth actor is never observed, so it is dropped
        assert bool((got[k].cpu()[zero] == 0).all()), k
        assert bool((got[k].cpu()[~zero] != 0).all()), k


@pytest.mark.parametrize("mode", MODES)
def test_roi_loss_fn(mods, mma_scope, mode):
    M, A, ops, L = mods
    mma_scope(mode)
    logits, goals, trajs, gt, has = RL.device_inputs(RM.tiled())
    p = {k: v.requires_grad_(True) for k, v in dict(d_logits=logits, d_goals=goals, d_trajs=trajs).items()}
    ref = RM.reference()
    sums = A.RoiLossFn.apply(logits, goals, trajs, gt, has, float(RM.fixture()["reg_coef"]))[:3]
    base = assert_homogeneous(list(sums), p, [g.reshape(()) for g in RL.upstream(ref)], "%s roi_loss" % mode)
    if mode == "f32":
        cmp_ = RM.reference(None, torch.float32)
        assert_anchored("roi_loss", base, {k: torch.from_numpy(ref[k]) for k in p}, {k: torch.from_numpy(cmp_[k]) for k in p})


@pytest.mark.parametrize("mode", MODES)
def test_goal_decode_and_refine_fn(mods, mma_scope, mode):
    """GoalDecodeFn and GoalRefineFn on the decelerating agent of test_gpu_goal_decode_train (9 nodes, the clamped v_j)."""
    import numpy as np
    M, A, ops, L = mods
    mma_scope(mode)
    case = GD.synthetic_case()
    K = GD.K
    spans = case["spans"]
    pred_spans = [0] + [int(v) for v in np.cumsum([hi - lo for lo, hi in spans])]
    first = [lo for lo, _ in spans]
    n_agt = len(spans)
    cu = lambda x: torch.from_numpy(np.ascontiguousarray(x)).cuda()
    rng = np.random.default_rng(29)
    w = {k: torch.from_numpy(rng.normal(0, 1, sh).astype(np.float32))
         for k, sh in (("goals", (n_agt, K, 2)), ("logits", (n_agt, K)), ("coef", (n_agt, K, 6)), ("s_samples", (n_agt, K, 30)),
                       ("trajs", (n_agt, K, 30, 2)))}
    pred = cu(case["pred"]).requires_grad_(True)
    top, goals, logits, coef, ss = A.GoalDecodeFn.apply(pred, pred_spans, cu(case["anc_ctrs"]), cu(case["anc_dirs"]), first,
                                                        cu(case["agt_ctrs"]), cu(case["dir_last"]), cu(case["agt_vel"]), K, 2.0)
    base = assert_homogeneous([goals, logits, coef, ss], dict(pred=pred), [w[k].cuda() for k in ("goals", "logits", "coef", "s_samples")],
                              "%s goal_decode" % mode)
    lv = dict(s_samples=ss.detach().clone().requires_grad_(True), coef=coef.detach().clone().requires_grad_(True),
              traj_delta=cu(case["delta"]).requires_grad_(True))
    trajs = A.GoalRefineFn.apply(lv["s_samples"], lv["coef"], lv["traj_delta"])
    base.update(assert_homogeneous([trajs], lv, [w["trajs"].cuda()], "%s goal_refine" % mode))
    if mode == "f32":
        def model(dtype):
            t = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(dtype)
            q = t(case["pred"]).requires_grad_(True)
            dec = GD.DM.decode(q, pred_spans, t(case["anc_ctrs"]), t(case["anc_dirs"]), first, t(case["agt_ctrs"]), t(case["dir_last"]),
                               t(case["agt_vel"]), K, top_idx=top.cpu().numpy())
            sum((dec[k] * w[k].to(dtype)).sum() for k in ("goals", "logits", "coef", "s_samples")).backward()
            l = {k: v.detach().cpu().to(dtype).requires_grad_(True) for k, v in lv.items()}
            (GD.DM.refine(l["s_samples"], l["coef"], l["traj_delta"]) * w["trajs"].to(dtype)).sum().backward()
            return dict({k: v.grad for k, v in l.items()}, pred=q.grad)
        assert_anchored("goal", base, model(torch.float64), model(torch.float32))


# ------------------------------------------------------------------ the negative control
def test_disabled_backward_mma_is_seen(mods, mma_scope, monkeypatch):
    """ops.backward_mma switched off (its __enter__ leaves the mode alone), mode f16x2, k = -40: dT sits near 1e-12, both fp16
    planes of the backward GEMM's operand flush, and the composed RowBlockFn and LaneConvFn backward (a) are no longer 2^k times
    their own result at k = 0 and (b) miss float64 by more than the bar.  No fault is provoked: the launches are the ordinary
    f16x2 ones on small operands; this only shows that Part A's check sees what it is there to see."""
    M, A, ops, L = mods
    mma_scope("f16x2")

    def leave(self):
        self.prev = ops._mma
        return self

    monkeypatch.setattr(ops.backward_mma, "__enter__", leave)
    k = -40
    # RowBlockFn, shape a
    inp = RB.block_inputs(130, "a")
    out, p = rb_forward(mods, inp, "a", False)
    bad, base = B.homogeneous([out], p, [inp["d_out"].cuda()], ks=(k,))
    assert (k, "src0") in bad, bad
    g = B.grads_at([out], p, [inp["d_out"].cuda()], k)
    ref = rb_stock(inp, "a", out.detach().cpu(), torch.float64, "cpu")
    cmp_ = rb_stock(inp, "a", out.detach(), torch.float32, "cpu")
    e, e_cmp = B.rel_err(g["src0"] * 2.0 ** -k, ref["src0"]), B.rel_err(cmp_["src0"], ref["src0"])
    print("row_block a: d src0 at k=-40 without backward_mma %.3e, stock fp32 %.3e" % (e, e_cmp))
    assert e > B.bar(e_cmp)
    # LaneConvFn, the LinearRes form
    inp = LC.block_inputs(130, False)
    out, leaves = lane_conv_forward(mods, inp, False, False)
    bad, base = B.homogeneous([out], leaves, [inp["d_out"].cuda()], ks=(k,))
    assert (k, "x") in bad, bad
    g = B.grads_at([out], leaves, [inp["d_out"].cuda()], k)
    p64 = LC.leaves_of(inp, lambda t: t.double().clone())
    with torch.no_grad():
        d = {n_: inp[n_].cuda() for n_ in ("x", "w1", "g1", "b1", "w2", "g2", "b2")}
        _, Y, _, o = LC.hip_forward((*mods, None), d["x"], d["w1"], [], None, d["g1"], d["b1"], d["w2"], d["g2"], d["b2"], mode="f16x2")
    assert torch.equal(o, out.detach())
    LC.torch_lane_conv(p64["x"], [], [], p64["w1"], [], p64["g1"], p64["b1"], p64["w2"], p64["g2"], p64["b2"],
                       masks=((Y > 0).cpu().double(), (o > 0).cpu().double())).backward(inp["d_out"].double())
    e = B.rel_err(g["x"] * 2.0 ** -k, p64["x"].grad)
    print("lane_conv: d x at k=-40 without backward_mma %.3e" % e)
    assert e > 1e-4                                                      # above the bar's ceiling, whatever e_cmp is


# ================================================================== Part B / C
def check_entry(label, got, ref, cmp_, cls, dead_rows=True):
    """Per row class for row tensors, per tensor for parameter gradients: print, then assert the bar; dead rows exactly zero."""
    rows = []
    dead = cls == B.CLASSES.index("dead")
    for k, r in ref.items():
        if r is None:
            continue
        assert got[k] is not None, k
        if k in ROW_TENSORS:
            e, ec = B.class_errors(got[k], r, cls), B.class_errors(cmp_[k], r, cls)
            rows += [("%s[%s]" % (k, name), e[name], ec[name]) for name in e]
            assert not dead_rows or bool((got[k].detach().cpu()[dead] == 0).all()), (label, k, "dead rows")
        else:
            rows.append((k, B.rel_err(got[k], r), B.rel_err(cmp_[k], r)))
    for name, e, ec in rows:
        print("%s %-18s hip %.3e stock fp32 %.3e" % (label, name, e, ec))
    bad = [r for r in rows if not r[1] <= B.bar(r[2])]
    assert not bad, (label, bad)


def gn_entry(ops, case):
    d = {k: case[k].cuda() for k in ("dy", "x", "post", "gamma")}
    dx, g, dgamma, dbeta = ops.gn_bwd(d["dy"], d["x"], d["post"], d["gamma"], eps=EPS, want_g=True)
    return dict(dx=dx, g=g, dgamma=dgamma, dbeta=dbeta)


def rowblock_entry(ops, case, n_chunks=3):
    s = B.RB_SHAPES[case["shape"]]
    srcs, ws = [t.cuda() for t in case["srcs"]], [t.cuda() for t in case["ws"]]
    g = ops.rowblock_bwd(case["d_out"].cuda(), case["out"].cuda() if s["relu"] else None, case["pre"].cuda(), case["gamma"].cuda(),
                         [(srcs[si], ws[wi], c0) for si, wi, c0 in s["rels"]], eps=EPS, want_res=s["res"] and s["relu"],
                         n_chunks=n_chunks)
    r = {"d src%d" % si: g["d_src"][i] for i, (si, _, _) in enumerate(s["rels"])}
    r.update({"d w%d" % k: v for k, v in enumerate(g["d_w"])})
    r["d gamma"], r["d beta"] = g["d_gamma"], g["d_beta"]
    if s["res"]:
        r["d res"] = g["d_res"]
    return r


def laneconv_entry(ops, case, n_chunks=3):
    d = {k: case[k].cuda() for k in ("d_out", "out", "Z", "Y", "T", "g1", "w2", "g2", "x", "w1")}
    kw = dict(x=d["x"], w1=d["w1"]) if case["ident1"] else {}
    return ops.laneconv_bwd(d["d_out"], d["out"], d["Z"], d["Y"], d["T"], d["g1"], d["w2"], d["g2"], n_chunks=n_chunks, eps=EPS, **kw)


def test_gn_bwd_statistics(mods, mma_scope):
    ops = mods[2]
    mma_scope("f32")
    case = B.gn_case()
    check_entry("gn_bwd", gn_entry(ops, case), B.gn_reference64(case), B.gn_stock(case, torch.float32, "cpu"), case["cls"])


@pytest.mark.parametrize("wscale", [1.0, 2.0 ** -12, 2.0 ** 4])
@pytest.mark.parametrize("shape", sorted(B.RB_SHAPES))
def test_rowblock_bwd_statistics(mods, mma_scope, shape, wscale):
    ops = mods[2]
    mma_scope("f32")
    case = B.rowblock_case(shape, wscale)
    check_entry("rowblock_bwd %s w=%g" % (shape, wscale), rowblock_entry(ops, case), B.rowblock_reference64(case),
                B.rowblock_stock(case, torch.float32, "cpu"), case["cls"], dead_rows=B.RB_SHAPES[shape]["relu"])


@pytest.mark.parametrize("wscale", [1.0, 2.0 ** -12, 2.0 ** 4])
@pytest.mark.parametrize("ident1", [False, True])
def test_laneconv_bwd_statistics(mods, mma_scope, ident1, wscale):
    ops = mods[2]
    mma_scope("f32")
    case = B.laneconv_case(ident1, wscale)
    check_entry("laneconv_bwd ident1=%d w=%g" % (ident1, wscale), laneconv_entry(ops, case), B.laneconv_reference64(case),
                B.laneconv_stock(case, torch.float32, "cpu"), case["cls"])


@pytest.mark.parametrize("shape", [(5, 128, 5), (37, 64, 10)])
def test_gn_cl_bwd_statistics(mods, shape):
    ops = mods[2]
    case = B.gn_cl_case(*shape)
    dx, g, dgamma, dbeta = ops.gn_cl_bwd(case["dy"].cuda(), case["x"].cuda(), case["post"].cuda(), case["gamma"].cuda(), eps=EPS,
                                         want_g=True)
    check_entry("gn_cl_bwd %s" % (shape,), dict(dx=dx, g=g, dgamma=dgamma, dbeta=dbeta), B.gn_cl_reference64(case),
                B.gn_cl_stock(case, torch.float32, "cpu"), case["cls"])


@pytest.mark.parametrize("unit", sorted(B.CONV_UNITS))
def test_conv1d_gn_bwd_statistics(mods, unit):
    ops = mods[2]
    cin, cout, ks, stride, res_mode = B.CONV_UNITS[unit]
    case = B.conv_case(unit)
    dx, dw, dgamma, dbeta, dres = ops.conv1d_gn_bwd(case["d_out"].cuda(), case["x"].cuda(), case["y"].cuda(), case["out"].cuda(),
                                                    case["w"].cuda(), stride, case["gamma"].cuda(), EPS, res_mode=res_mode, relu=True)
    check_entry("conv1d_gn_bwd %s" % unit, dict(dx=dx, dw=dw, dgamma=dgamma, dbeta=dbeta, dres=dres), B.conv_reference64(case),
                B.conv_stock(case, torch.float32, "cpu"), case["cls"])


@pytest.mark.parametrize("entry", ["gn_bwd", "rowblock_bwd", "laneconv_bwd"])
def test_rows_beyond_fp32_squares(mods, mma_scope, entry):
    """Part C: pre-norm rows of magnitude 2^70, whose fp32 sum of squares is inf.  The forward's row_gn takes row_rstd_wide
    there; so do k_gn_bwd and row_gn_hat, and the gradients (dx ~ 2^-70 d_out, inside fp32) come out right instead of zero."""
    ops = mods[2]
    mma_scope("f32")
    if entry == "gn_bwd":
        case = B.gn_case(huge=True)
        got, ref, cmp_ = gn_entry(ops, case), B.gn_reference64(case), B.gn_stock(case, torch.float32, "cpu")
    elif entry == "rowblock_bwd":
        case = B.rowblock_case("b", huge=True)
        got, ref, cmp_ = rowblock_entry(ops, case), B.rowblock_reference64(case), B.rowblock_stock(case, torch.float32, "cpu")
    else:
        case = B.laneconv_case(False, huge=True)
        got, ref, cmp_ = laneconv_entry(ops, case), B.laneconv_reference64(case), B.laneconv_stock(case, torch.float32, "cpu")
    check_entry("2^70 " + entry, got, ref, cmp_, case["cls"])


@pytest.mark.parametrize("stat", ["ordinary", "flat", "offset"])
def test_att_pairs_bwd_statistics(mods, mma_scope, stat):
    """lgcn_att_pairs_bwd recomputes its forward, so the statistics of c = e Wc^T + U[hi] + V[wi] are steered through the inputs:
    flat -- U, V and the ctx.0 block scaled by 2^-12 (variance of c far below eps); offset -- U shifted by 2^10.  The pairs share
    U and V rows, so the classes are three runs instead of interleaved rows; 130 pairs, 3 workgroups, both norms with the gamma
    of backward_cases."""
    M, A, ops, L = mods
    mma_scope("f32")
    P = 130
    ps, inp, hi, wi = TA.make_case(ops, P)
    inp = dict(inp)
    inp["gd"], inp["btd"] = B.gamma_beta(12100)
    inp["gc"], inp["btc"] = B.gamma_beta(12200)
    if stat == "flat":
        inp["U"], inp["V"] = inp["U"] * 2.0 ** -12, inp["V"] * 2.0 ** -12
        inp["w_c0"] = torch.cat([inp["w_c0"][:, :C] * 2.0 ** -12, inp["w_c0"][:, C:]], 1)
    elif stat == "offset":
        inp["U"] = inp["U"] + 2.0 ** 10
    d = {k: inp[k].cuda() for k in TA.NAMES}
    _, raw = ops.att_pairs_train(ps, d["wd0"], d["bd0"], d["w_d2"], (d["gd"], d["btd"]), d["w_c0"], d["U"], d["V"], (d["gc"], d["btc"]))
    masks = ops.att_pair_masks(raw, P).cpu()
    out = ops.att_pairs_bwd(ps, inp["dS"].cuda(), raw, d["wd0"], d["bd0"], d["w_d2"], (d["gd"], d["btd"]), d["w_c0"], d["U"], d["V"],
                            (d["gc"], d["btc"]), n_chunks=3)
    rp, col = ps.csr_by_wi(TA.S)
    got = dict(wd0=out["d_wd0"], bd0=out["d_bd0"], w_d2=out["d_wd2"], gd=out["d_gd"], btd=out["d_btd"], w_c0=out["d_wc0e"],
               gc=out["d_gc"], btc=out["d_btc"], dc=out["dc"][:P], U=ops.gather_sum(out["dc"], ps.rowptr, None, TA.T),
               V=ops.gather_sum(out["dc"], rp, col, TA.S))
    ref = att_stock(inp, hi, wi, masks, torch.float64, "cpu", want_dc=True)
    cmp_ = att_stock(inp, hi, wi, masks, torch.float32, "cpu", want_dc=True)
    c = ref.pop("c")
    cmp_.pop("c")
    var, mean = c.var(1, unbiased=False), c.mean(1)
    if stat == "flat":
        assert float(var.max()) < EPS / 10
    elif stat == "offset":
        assert float((mean.abs() / var.sqrt()).min()) > 100
    else:
        assert float(var.min()) > 100 * EPS
    rows = [(k, B.rel_err(got[k], ref[k]), B.rel_err(cmp_[k], ref[k])) for k in ref]
    for k, e, ec in rows:
        print("att_pairs_bwd %-8s %-5s hip %.3e stock fp32 %.3e" % (stat, k, e, ec))
    bad = [r for r in rows if not r[1] <= B.bar(r[2])]
    assert not bad, (stat, bad)
