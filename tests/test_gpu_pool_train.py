"""GPU: the pair stage of the fork's LanePooling trained on HIP (LanePooling.train_hip): autograd.PoolPairsFn on
lgcn_pool_pairs_train / lgcn_pool_pairs_bwd -- against the float64 autograd model of tests/pool_train_model.py at a bar taken
from today's composed path, against the inference kernel (bitwise), repeatable and independent of the matrix mode, rows past
the pair count untouched, absent gradients skipped, what autograd saves, at module level against the composed path and
inside one whole training step of Net + Loss against float64 autograd.

Pair sets are made by hand: ti sorted, ci arbitrary, both with cap = P + 40 entries and far-out-of-range garbage past P;
T = 9 targets (3 and 7 without a pair; a segment straddles pair 32 whenever P > 32), S = 11 context rows (2 and 9 unused).
P = 1, 31, 32, 33 (one tile, a full one, one pair into the second) and 130 (5 tiles, the last ragged) with 1, 2 and 3
workgroups (5 / 3+2 / 2+2+1 tiles each).  Poses are multiples of 1/64 in [0, 4) (+ the shift), so every pose difference is
exact in fp32; the tests assert it.

The bar per tensor (the project's for exact-fp32 kernels, test_gpu_att_train.py): rel_err <= min(max(2 x the error of today's
composed path in f32 mode against the same float64 reference, 1e-6), 1e-4) with rel_err = max |got - ref| / max |ref|; both
errors are printed before the assertion.

PoolPairsFn hands the launches cap = P (LanePooling's inference path does the same: m is then [P,128], not [capacity,128]),
so the masks it saves are [P,8] int32; at the ops level the tests pass cap = P + 40."""
import types

import numpy as np
import pytest
import torch

import lanercnn_net_fixture as NF
import pool_pairs_model as PM
import pool_train_model as TM
import test_gpu_lanercnn_net as TN
from test_gpu_lanercnn_heads import GTOL, f32  # noqa: F401  (f32: fixture)

pytestmark = pytest.mark.gpu

T, S, C = 9, 11, 128
TARGETS = (0, 1, 2, 4, 5, 6, 8)
CONTEXTS = (0, 1, 3, 4, 5, 6, 7, 8, 10)
PAD, GARBAGE = 40, 1 << 30
CASES = [(1, None), (31, None), (32, None), (33, None), (130, 1), (130, 2), (130, 3)]
NAMES = ("wp", "bp", "w0", "U", "g", "bt")          # leaves of the pair stage; w0 = ctx.0's [128,256] weight
TENSORS = ("S", "U", "wp", "bp", "w0", "g", "bt", "dz")
EPS = 1e-5


@pytest.fixture(scope="module")
def mods():
    import lanegcn_amd  # noqa: F401
    from lanegcn_amd import autograd as A
    from lanegcn_amd import lanercnn as R
    from lanegcn_amd import ops
    return R, A, ops


@pytest.fixture
def mma_scope(mods):
    ops = mods[2]
    prev = ops.get_mma()
    yield ops.set_mma
    ops.set_mma(prev)


@pytest.fixture
def count_fused(mods, monkeypatch):
    """A list that grows by one with every PoolPairsFn.apply."""
    A = mods[1]
    calls, real = [], A.PoolPairsFn.apply
    monkeypatch.setattr(A.PoolPairsFn, "apply", staticmethod(lambda *a: calls.append(1) or real(*a)))
    return calls


def make_case(ops, P, scale=1.0, shift=0.0, count=None, valid_pad=False, seed=0):
    """(PairSet on the device, inputs on the CPU in fp32, ti, ci as CPU LongTensors over the rows the launch processes).
    The poses and weights come from the generator of test_gpu_pool_pairs.make_case."""
    g = torch.Generator().manual_seed(100 * P + seed)
    ti = torch.tensor([TARGETS[p * len(TARGETS) // P] for p in range(P)])
    ci = torch.tensor(CONTEXTS)[torch.randint(len(CONTEXTS), (P,), generator=g)]
    assert bool((ti[1:] >= ti[:-1]).all()) and (P <= 32 or ti[31] == ti[32])      # sorted; a segment straddles the first tile boundary
    if valid_pad:
        pad_t, pad_c = torch.randint(T, (PAD,), generator=g), torch.randint(S, (PAD,), generator=g)
    else:
        pad_t, pad_c = torch.full((PAD,), GARBAGE), -torch.full((PAD,), GARBAGE)
    cap = P + PAD
    rowptr = torch.zeros(T + 1, dtype=torch.int64)
    rowptr[1:] = torch.cumsum(torch.bincount(ti, minlength=T), 0)
    grid = lambda n: torch.randint(256, (n, 4), generator=g).float() / 64 + shift
    tgt_pose, ctx_pose = grid(T), grid(S)
    i32 = lambda t: t.to(torch.int32).cuda()
    ps = ops.PairSet(i32(torch.cat([ti, pad_t])), i32(torch.cat([ci, pad_c])), i32(torch.tensor([P if count is None else count])),
                     i32(rowptr), cap, T, tgt_pose[:, :2].contiguous().cuda(), ctx_pose[:, :2].contiguous().cuda())
    ps._p_host = P                       # the hand-made count may be negative or past cap: the host side knows P
    rn = lambda *shape, fan: torch.randn(*shape, generator=g) * (scale * 1.5 / fan ** 0.5)
    w0 = rn(C, 2 * C, fan=2 * C)
    cfeat = torch.randn(S, C, generator=g)
    inp = dict(wp=rn(C, 4, fan=4), bp=rn(C, fan=4), w0=w0, U=(cfeat.double() @ w0[:, :C].double().t()).float(),
               g=1 + 0.1 * (2 * torch.rand(C, generator=g) - 1), bt=0.1 * torch.randn(C, generator=g),
               ctx_pose=ctx_pose, tgt_pose=tgt_pose, dS=torch.randn(T, C, generator=g))
    d = ctx_pose[ci] - tgt_pose[ti]
    assert torch.equal(d.double(), ctx_pose.double()[ci] - tgt_pose.double()[ti])      # the subtraction is exact in fp32
    if valid_pad:
        ti, ci = torch.cat([ti, pad_t]), torch.cat([ci, pad_c])
    return ps, inp, ti, ci


def leaves(inp, only=None):
    return {k: inp[k].cuda().requires_grad_(only is None or k in only) for k in NAMES}


def fused(A, ps, inp, x):
    return A.PoolPairsFn.apply(ps, inp["ctx_pose"].cuda(), inp["tgt_pose"].cuda(), x["wp"], x["bp"], x["w0"], x["U"], x["g"],
                               x["bt"], EPS)


def op_args(inp, x):
    d = {k: v.detach() for k, v in x.items()}
    return (inp["ctx_pose"].cuda(), inp["tgt_pose"].cuda(), d["wp"], d["bp"], d["w0"], d["U"], (d["g"], d["bt"]))


def reference64(inp, ti, ci, masks):
    """tests/pool_train_model.py on this case: (S, gradients by TENSORS, the two pre-activations)."""
    x = dict(wp=inp["wp"], bp=inp["bp"], w0h=inp["w0"][:, C:], U=inp["U"], g=inp["g"], bt=inp["bt"])
    Sx, grads, pre = TM.train_step(inp["ctx_pose"], inp["tgt_pose"], ti, ci, x, masks, inp["dS"], EPS)
    grads["w0"] = grads.pop("w0h")
    return Sx, grads, pre


def composed(A, ops, ps, inp, P):
    """The pair stage as today's LanePooling._run composes it under autograd (the lines from `h` to `m`) on the same leaves,
    and its segment sum: (S, gradients by TENSORS)."""
    x = leaves(inp)
    t_idx, c_idx = ps.hi[:P].long(), ps.wi[:P].long()
    gn = types.SimpleNamespace(weight=x["g"], bias=x["bt"], eps=EPS)
    h = torch.relu(torch.nn.functional.linear(inp["ctx_pose"].cuda()[c_idx] - inp["tgt_pose"].cuda()[t_idx], x["wp"], x["bp"]))
    per_pair = A.linear_gn(h.contiguous(), x["w0"], col0=128)
    no_query = torch.zeros((T, C), dtype=torch.float32, device="cuda")
    pre = A.PairAddFn.apply(per_pair, no_query, x["U"], ps)
    m = A.gn_act(pre, gn=gn, relu=True)
    got = {}
    m.grad_fn.register_hook(lambda grad_in, grad_out: got.__setitem__("dz", grad_in[0].detach().clone()))
    i32 = dict(dtype=torch.int32, device="cuda")
    plan = types.SimpleNamespace(rowptr=ps.rowptr, col=None)
    plan_t = types.SimpleNamespace(rowptr=torch.arange(P + 1, **i32), col=ps.hi[:P].contiguous())
    Sx = A.GatherSumFn.apply(m, plan, plan_t, T)
    (Sx * inp["dS"].cuda()).sum().backward()
    got.update({k: v.grad for k, v in x.items()})
    got["w0"] = got["w0"][:, C:]
    return Sx.detach(), got


def err(got, want):
    return float((got.detach().double().cpu() - want).abs().max() / (want.abs().max() + 1e-12))


def outside_bar(rows):
    return [(n, a, b) for n, a, b in rows if not a <= min(max(2 * b, 1e-6), 1e-4)]


def check_against_fp64(mods, P, n_chunks, scale=1.0, shift=0.0):
    R, A, ops = mods
    tag = "P=%d chunks=%s scale=%g shift=%g" % (P, n_chunks, scale, shift)
    ps, inp, ti, ci = make_case(ops, P, scale=scale, shift=shift)
    x = leaves(inp)
    m, masks_raw = ops.pool_pairs_train(ps, *op_args(inp, x), eps=EPS)
    assert m.shape == (ps.cap, C) and masks_raw.shape == (ps.cap, 8) and masks_raw.dtype == torch.int32
    masks = ops.pool_pair_masks(masks_raw, P).cpu()
    assert masks.shape == (P, 2, C) and masks.dtype == torch.bool
    S_ref, g_ref, pre = reference64(inp, ti, ci, masks)
    # the stored masks are the signs of the pre-activations wherever those are not on the knife edge
    for k, z in enumerate(pre):
        clear = z.abs() > 1e-4 * z.abs().amax(1, keepdim=True)
        print("%s mask %d: %.5f of the entries clear" % (tag, k, float(clear.float().mean())))
        assert clear.float().mean() > 0.99
        assert bool(((z > 0) == masks[:, k])[clear].all()), k

    out = ops.pool_pairs_bwd(ps, inp["dS"].cuda(), masks_raw, *op_args(inp, x), eps=EPS, n_chunks=n_chunks)
    if n_chunks is None:
        Sx = fused(A, ps, inp, x)
        (Sx * inp["dS"].cuda()).sum().backward()
        got = {k: v.grad for k, v in x.items()}
        assert bool((got["w0"][:, :C] == 0).all())                 # the U row block owns those columns
        got["w0"] = got["w0"][:, C:]
    else:
        Sx = ops.gather_sum(m, ps.rowptr, None, T)
        rp, col = ps.csr_by_wi(S)
        got = dict(wp=out["d_wp"], bp=out["d_bp"], w0=out["d_w0h"], g=out["d_g"], bt=out["d_bt"],
                   U=ops.gather_sum(out["dz"], rp, col, S))
    got["dz"] = out["dz"][:P]
    S_cmp, g_cmp = composed(A, ops, ps, inp, P)

    rows = [("S", err(Sx, S_ref), err(S_cmp, S_ref))]
    rows += [(k, err(got[k], g_ref[k]), err(g_cmp[k], g_ref[k])) for k in TENSORS[1:]]
    for name, e_new, e_cmp in rows:
        print("%s %-3s fused %.3e composed %.3e" % (tag, name, e_new, e_cmp))
    bad = outside_bar(rows)
    assert not bad, bad


@pytest.mark.parametrize("P,n_chunks", CASES)
def test_against_fp64(mods, mma_scope, P, n_chunks):
    """S, dU, d_wp, d_bp, d_w0h, d_g, d_bt and dz against the float64 model, f32 mode."""
    mma_scope("f32")
    check_against_fp64(mods, P, n_chunks)


@pytest.mark.parametrize("scale,shift", [(0.1, 0.0), (8.0, 0.0), (1.0, 1e3)])
def test_against_fp64_over_weight_scale_and_pose_offset(mods, mma_scope, scale, shift):
    mma_scope("f32")
    check_against_fp64(mods, 130, None, scale=scale, shift=shift)


@pytest.mark.parametrize("P", [1, 33, 130])
def test_forward_is_inference_forward_bitwise(mods, mma_scope, P):
    R, A, ops = mods
    mma_scope("f32")
    ps, inp, _, _ = make_case(ops, P)
    x = {k: inp[k].cuda() for k in NAMES}
    m, _ = ops.pool_pairs_train(ps, *op_args(inp, x), eps=EPS)
    m_inf = ops.pool_pairs(ps, *op_args(inp, x), eps=EPS)
    assert torch.equal(m[:P].view(torch.int32), m_inf[:P].view(torch.int32))
    Sx = fused(A, ps, inp, x)
    assert torch.equal(Sx.view(torch.int32), ops.gather_sum(m, ps.rowptr, None, T).view(torch.int32))


def fwd_bwd(A, ps, inp, only=None, zero=False):
    x = leaves(inp, only)
    Sx = fused(A, ps, inp, x)
    (Sx * (0 if zero else inp["dS"].cuda())).sum().backward()
    return [Sx.detach()] + [x[k].grad for k in NAMES]


def same_bits(a, b):
    return (a is None and b is None) or torch.equal(a.view(torch.int32), b.view(torch.int32))


def test_repeatable_and_independent_of_the_matrix_mode(mods, mma_scope):
    R, A, ops = mods
    ps, inp, _, _ = make_case(ops, 130)
    runs = []
    for mode in ("f32", "f32", "bf16x3", "f16x2"):
        mma_scope(mode)
        runs.append(fwd_bwd(A, ps, inp))
    for r in runs[1:]:
        assert all(g is not None for g in r)
        assert all(same_bits(a, b) for a, b in zip(runs[0], r))


@pytest.mark.parametrize("P", [1, 33, 130])
def test_rows_past_the_count_are_untouched(mods, P):
    """cap = P + 40: m, masks and dz rows >= P keep their sentinel; ti / ci beyond P hold +-2^30 and are never used."""
    R, A, ops = mods
    ps, inp, _, _ = make_case(ops, P)
    x = {k: inp[k].cuda() for k in NAMES}
    m = torch.full((ps.cap, C), -7.5, device="cuda")
    masks = torch.full((ps.cap, 8), 0x5A5A5A5A, dtype=torch.int32, device="cuda")
    dz = torch.full((ps.cap, C), -7.5, device="cuda")
    got_m, got_masks = ops.pool_pairs_train(ps, *op_args(inp, x), m=m, masks=masks, eps=EPS)
    out = ops.pool_pairs_bwd(ps, inp["dS"].cuda(), masks, *op_args(inp, x), dz=dz, eps=EPS)
    torch.cuda.synchronize()
    assert got_m is m and got_masks is masks and out["dz"] is dz
    assert bool((m[P:] == -7.5).all()) and bool((dz[P:] == -7.5).all()) and bool((masks[P:] == 0x5A5A5A5A).all())
    assert bool(torch.isfinite(m[:P]).all()) and bool(torch.isfinite(dz[:P]).all()) and bool((m[:P] >= 0).all())
    assert all(bool(torch.isfinite(v).all()) for v in out.values())


@pytest.mark.parametrize("count", [-50, 1000])
def test_negative_or_oversized_count_processes_cap_rows(mods, mma_scope, count):
    """The pair search reports an overflow as a negative count: the launches then process all cap rows (valid padding); a
    count past cap is clamped as well.  Forward and gradients then are those of a pair set of cap pairs."""
    R, A, ops = mods
    mma_scope("f32")
    ps, inp, ti, ci = make_case(ops, 33, count=count, valid_pad=True)
    n = ps.cap
    assert len(ti) == n == 73
    x = {k: inp[k].cuda() for k in NAMES}
    m = torch.full((n, C), -7.5, device="cuda")
    masks_raw = torch.full((n, 8), 0x5A5A5A5A, dtype=torch.int32, device="cuda")
    dz = torch.full((n, C), -7.5, device="cuda")
    ops.pool_pairs_train(ps, *op_args(inp, x), m=m, masks=masks_raw, eps=EPS)
    out = ops.pool_pairs_bwd(ps, inp["dS"].cuda(), masks_raw, *op_args(inp, x), dz=dz, eps=EPS)
    masks = ops.pool_pair_masks(masks_raw, n).cpu()
    x64 = dict(wp=inp["wp"], bp=inp["bp"], w0h=inp["w0"][:, C:], U=inp["U"], g=inp["g"], bt=inp["bt"])
    m_ref, _ = TM.forward(inp["ctx_pose"], inp["tgt_pose"], ti, ci, x64, masks, T, EPS)
    _, g_ref, _ = TM.train_step(inp["ctx_pose"], inp["tgt_pose"], ti, ci, x64, masks, inp["dS"], EPS)
    rows = [("m", err(m, m_ref)), ("dz", err(dz, g_ref["dz"])), ("wp", err(out["d_wp"], g_ref["wp"])),
            ("bp", err(out["d_bp"], g_ref["bp"])), ("w0", err(out["d_w0h"], g_ref["w0h"])), ("g", err(out["d_g"], g_ref["g"])),
            ("bt", err(out["d_bt"], g_ref["bt"]))]
    print("count=%d" % count, ["%s %.3e" % r for r in rows])
    assert all(e <= 1e-4 for _, e in rows), rows


def test_absent_gradients(mods):
    R, A, ops = mods
    ps, inp, _, _ = make_case(ops, 130)
    full = fwd_bwd(A, ps, inp)
    assert all(g is not None and bool(g.abs().max() > 0) for g in full)
    assert bool((full[1 + NAMES.index("w0")][:, :C] == 0).all())
    zero = fwd_bwd(A, ps, inp, zero=True)
    assert all(g is not None and bool((g == 0).all()) for g in zero[1:])
    only_u = fwd_bwd(A, ps, inp, only=("U",))
    iu = 1 + NAMES.index("U")
    assert all(g is None for i, g in enumerate(only_u) if i not in (0, iu))
    assert same_bits(full[iu], only_u[iu]) and same_bits(full[0], only_u[0])
    # the kernel's shorter walks: nothing upstream of h wanted (no dh GEMM), relpose.0's parameters without dW_0h
    for only in (("w0", "g"), ("bt",), ("wp", "bp")):
        part = fwd_bwd(A, ps, inp, only=only)
        for i, k in enumerate(NAMES):
            assert (part[1 + i] is None) == (k not in only), (only, k)
            assert k not in only or same_bits(full[1 + i], part[1 + i]), (only, k)
    # the interleaved output alone: d_wp [128,4] takes the record's last four rows, and every output next to them is absent
    ps, inp, _, _ = make_case(ops, 33)
    x = {k: inp[k].cuda() for k in NAMES}
    _, masks = ops.pool_pairs_train(ps, *op_args(inp, x), eps=EPS)
    bwd = lambda **kw: ops.pool_pairs_bwd(ps, inp["dS"].cuda(), masks, *op_args(inp, x), eps=EPS, n_chunks=2, **kw)
    whole, alone = bwd(), bwd(want=("d_wp",), want_dz=False)
    assert set(alone) == {"dz", "d_wp"} and alone["dz"] is None and bool(whole["d_wp"].abs().max() > 0)
    assert same_bits(whole["d_wp"], alone["d_wp"])


def test_no_upstream_gradient_returns_none(mods):
    A = mods[1]
    assert A.PoolPairsFn.backward(types.SimpleNamespace(), None) == (None,) * 10


def test_saved_memory(mods):
    """PoolPairsFn at P = 130 saves nothing per pair but the masks: besides its own inputs (which exist anyway; ctx.0's
    [128,256] weight alone has more than P * 128 elements) the only tensor it saves is the masks, [rows,8] int32 for the
    rows it hands the launch, and no saved tensor, input or not, has a row per pair and 128 columns."""
    R, A, ops = mods
    P = 130
    ps, inp, _, _ = make_case(ops, P)
    x = leaves(inp)
    poses = (inp["ctx_pose"].cuda(), inp["tgt_pose"].cuda())
    saved = []
    with torch.autograd.graph.saved_tensors_hooks(lambda t: saved.append(t) or t, lambda t: t):
        Sx = A.PoolPairsFn.apply(ps, *poses, x["wp"], x["bp"], x["w0"], x["U"], x["g"], x["bt"], EPS)
    shapes = [tuple(t.shape) for t in saved]
    inputs = {t.data_ptr() for t in (*poses, *x.values())}
    own = [t for t in saved if t.data_ptr() not in inputs]
    assert len(saved) == 9 and len(own) == 1, shapes
    assert own[0].dtype == torch.int32 and own[0].numel() == P * 8 <= ps.cap * 8 and own[0].numel() < P * C
    assert not any(t.dim() == 2 and t.shape[0] >= P and t.shape[1] >= C for t in saved), shapes
    (Sx * inp["dS"].cuda()).sum().backward()
    assert all(x[k].grad is not None for k in NAMES)


# ------------------------------------------------------------------ module level
DIST_TH = 14.3            # no pair of grid points sits at this distance
POOL_KEYS = ("input.weight", "relpose.0.weight", "relpose.0.bias", "ctx.0.linear.weight", "ctx.0.norm.weight", "ctx.0.norm.bias",
             "ctx.1.weight", "mlp.0.linear.weight", "mlp.0.norm.weight", "mlp.0.norm.bias", "mlp.1.linear.weight",
             "mlp.1.norm.weight", "mlp.1.norm.bias", "norm.weight", "norm.bias")


def pool_inputs(seed=3):
    """Two scenes of 20 target and 15 context nodes on a 1/64 grid, a threshold that keeps a few hundred of the 2 x 20 x 15
    candidates; pose = (centre, a direction)."""
    g = torch.Generator().manual_seed(seed)
    pts = lambda n: (torch.randint(-1024, 1024, (n, 2), generator=g).float() / 64)
    graphs = []
    for n in (20, 15):
        ctrs = [pts(n) for _ in range(2)]
        pose = [torch.cat([c, torch.randint(-64, 65, (n, 2), generator=g).float() / 64], 1) for c in ctrs]
        graphs.append({"ctrs": ctrs, "pose": pose})
    tgt, ctx = graphs
    return dict(tgt=tgt, ctx=ctx, tfeat=torch.randn(40, C, generator=g), cfeat=torch.randn(30, C, generator=g),
                w_out=torch.randn(40, C, generator=g))


def pool_module(R, seed=11):
    torch.manual_seed(seed)
    pool = R.LanePooling(C, C)
    assert tuple(sorted(k for k, _ in pool.named_parameters())) == tuple(sorted(POOL_KEYS))
    with torch.no_grad():
        for n, p in pool.named_parameters():
            if "norm" in n and n.endswith("weight"):
                p.copy_(1 + 0.1 * (2 * torch.rand_like(p) - 1))
            elif "norm" in n:
                p.copy_(0.1 * torch.randn_like(p))
            elif p.dim() == 2:
                p.copy_(torch.randn_like(p) * (1.5 / p.shape[1] ** 0.5))
    return pool


def pool_step(pool, inputs, dist_th=DIST_TH, pose_grad=False):
    dev = lambda gr: {k: [t.cuda() for t in v] for k, v in gr.items()}
    tgt, ctx = dev(inputs["tgt"]), dev(inputs["ctx"])
    if pose_grad:
        tgt["pose"] = [t.requires_grad_(True) for t in tgt["pose"]]
    tf, cf = inputs["tfeat"].cuda().requires_grad_(True), inputs["cfeat"].cuda().requires_grad_(True)
    pool.zero_grad(set_to_none=True)
    out = pool(cf, ctx, tf, tgt, dist_th)
    (out * inputs["w_out"].cuda()).sum().backward()
    res = {"out": out.detach(), "d target_feat": tf.grad, "d context_feat": cf.grad}
    res.update({n: p.grad for n, p in pool.named_parameters()})
    return res


def pool_reference64(pool, inputs, dist_th=DIST_TH):
    """pool_pairs_model.lane_pooling in float64 on the CPU under autograd, for the loss of pool_step."""
    sd = {"pool." + n: p.detach().cpu().double().requires_grad_(True) for n, p in pool.named_parameters()}
    tf, cf = inputs["tfeat"].double().requires_grad_(True), inputs["cfeat"].double().requires_grad_(True)
    out, ci, _ = PM.lane_pooling(cf, inputs["ctx"], tf, inputs["tgt"], sd, "pool", dist_th)
    (out * inputs["w_out"].double()).sum().backward()
    res = {"out": out.detach(), "d target_feat": tf.grad, "d context_feat": cf.grad}
    res.update({n[5:]: v.grad for n, v in sd.items()})
    return res, len(ci)


def test_module_on_against_off(mods, mma_scope, count_fused):
    """LanePooling, switch off and on in f32 mode, each against the float64 module: output, d target_feat, d context_feat and
    every parameter gradient at the bar of test_against_fp64.  PoolPairsFn runs once per forward with the switch on, never
    with it off, and never when a pose requires a gradient."""
    R, A, ops = mods
    mma_scope("f32")
    inputs = pool_inputs()
    pool = pool_module(R).cuda().train()
    ref, P = pool_reference64(pool, inputs)
    assert 200 <= P <= 600, P
    assert R.LanePooling.train_hip is False
    res = {False: pool_step(pool, inputs)}
    assert not count_fused
    R.LanePooling.train_hip = True
    try:
        res[True] = pool_step(pool, inputs)
        assert len(count_fused) == 1
        with_pose = pool_step(pool, inputs, pose_grad=True)
        assert len(count_fused) == 1
    finally:
        R.LanePooling.train_hip = False
    assert same_bits(with_pose["out"], res[False]["out"])                       # the composed path's forward
    assert set(ref) == set(res[True]) and all(v is not None for v in res[True].values())
    rows = [(k, err(res[True][k], ref[k]), err(res[False][k], ref[k])) for k in ref]
    for name, e_new, e_cmp in rows:
        print("P=%d %-24s fused %.3e composed %.3e" % (P, name, e_new, e_cmp))
    bad = outside_bar(rows)
    assert not bad, bad


# ------------------------------------------------------------------ one whole training step
@pytest.mark.parametrize("others", [False, True], ids=["pool_only", "all_switches"])
def test_whole_training_step(mods, f32, count_fused, others):  # noqa: F811
    """One training step of Net + Loss on lanercnn_net_b3 with LanePooling.train_hip on, alone and together with
    RowBlockFn.train_hip and Decode.train_hip: every parameter gradient within GTOL of float64 autograd (the reference step
    of test_gpu_lanercnn_net.py); the three poolings take PoolPairsFn."""
    R, A, ops = mods
    from lanegcn_amd import data as gen
    g, names = NF.fixture()
    loss64, grads64, _ = TN.reference_step(g, names)
    net, loss_fn = TN.make_net(R, train=True), R.Loss(R.config).cuda()
    data = gen.collate_fn(NF.scenes())
    prev = (A.RowBlockFn.train_hip, R.Decode.train_hip, R.LanePooling.train_hip)
    A.RowBlockFn.train_hip = R.Decode.train_hip = others
    R.LanePooling.train_hip = True
    try:
        cap = TN.run_captured(R, net, data)
        loss_out = loss_fn(cap["out"], data)
        loss_out["loss"].backward()
    finally:
        A.RowBlockFn.train_hip, R.Decode.train_hip, R.LanePooling.train_hip = prev
    assert len(count_fused) == 3, len(count_fused)
    assert np.array_equal(cap["dec"]["top_idx"].cpu().numpy(), g["dec/top_k"])      # the indices the float64 run used
    loss = float(loss_out["loss"].detach())
    print("others=%s loss %.6f float64 %.6f" % (others, loss, loss64))
    assert np.isfinite(loss)
    worst = {}
    for k, prm in net.named_parameters():
        assert prm.grad is not None and bool(torch.isfinite(prm.grad).all()), k
        worst[k] = TN.rel(prm.grad, grads64[k])
    print("largest relative gradient errors:", sorted(worst.items(), key=lambda kv: -kv[1])[:4])
    assert all(v <= GTOL for v in worst.values()), {k: v for k, v in worst.items() if v > GTOL}
