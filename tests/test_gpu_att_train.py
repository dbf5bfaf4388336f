"""GPU: Att's pair stage trained on HIP (Att.train_hip): autograd.AttPairsFn on lgcn_att_pairs_train / lgcn_att_pairs_bwd --
against an fp64 CPU autograd restatement at a bar taken from today's composed path, against the inference kernel (bitwise),
repeatable and independent of the matrix mode, rows past the pair count untouched, absent gradients skipped, at module level
against the composed path, inside whole training steps of Net against the reference's own gradients, and with fresh weight
images after an optimizer step.

Pair sets are made by hand: hi sorted, wi arbitrary, both with cap = P + 40 entries and far-out-of-range garbage past P;
T = 9 targets (3 and 7 without a pair; a segment straddles pair 32 whenever P > 32), S = 11 context rows (2 and 9 unused).
P = 1, 31, 32, 33 (one tile, a full one, one pair into the second) and 130 (5 tiles, the last ragged) with 1, 2 and 3
workgroups (5 / 3+2 / 2+2+1 tiles each).

test_against_fp64 and test_module_on_against_off print, per tensor, the error of the fused and of the composed path against
float64 (rel_err = max |got - ref| / max |ref|) before they assert; no figures are recorded here or in DESIGN.md yet."""
import os
import types

import numpy as np
import pytest
import torch

import test_gpu_training as TG
from oracle import lanegcn_oracle as O
from test_gpu_training import rel_err

pytestmark = pytest.mark.gpu
GOLDEN_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")

T, S, C = 9, 11, 128
TARGETS = (0, 1, 2, 4, 5, 6, 8)
CONTEXTS = (0, 1, 3, 4, 5, 6, 7, 8, 10)
GARBAGE = 1 << 30
CASES = [(1, None), (31, None), (32, None), (33, None), (130, 1), (130, 2), (130, 3)]
NAMES = ("wd0", "bd0", "w_d2", "gd", "btd", "w_c0", "U", "V", "gc", "btc")
EPS = 1e-5


@pytest.fixture(scope="module")
def mods():
    import lanegcn_amd  # noqa: F401
    from lanegcn_amd import autograd as A
    from lanegcn_amd import lanegcn as M
    from lanegcn_amd import ops
    return M, A, ops


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
    """A list that grows by one with every AttPairsFn.apply."""
    A = mods[1]
    calls, real = [], A.AttPairsFn.apply
    monkeypatch.setattr(A.AttPairsFn, "apply", staticmethod(lambda *a: calls.append(1) or real(*a)))
    return calls


@pytest.fixture
def hip_on(mods):
    M = mods[0]
    prev = M.Att.train_hip
    M.Att.train_hip = True
    yield
    M.Att.train_hip = prev


def make_case(ops, P, seed=0):
    """(PairSet on the device, inputs on the CPU in fp32, hi, wi as CPU LongTensors [P])."""
    g = torch.Generator().manual_seed(100 * P + seed)
    hi = torch.tensor([TARGETS[p * len(TARGETS) // P] for p in range(P)])
    wi = torch.tensor(CONTEXTS)[torch.randint(len(CONTEXTS), (P,), generator=g)]
    if P > 32:
        assert hi[31] == hi[32]                                   # a segment straddles the first tile boundary
    cap = P + 40
    pad = torch.full((40,), GARBAGE)
    rowptr = torch.zeros(T + 1, dtype=torch.int64)
    rowptr[1:] = torch.cumsum(torch.bincount(hi, minlength=T), 0)
    agt_ctrs, ctx_ctrs = torch.randn(T, 2, generator=g) * 10, torch.randn(S, 2, generator=g) * 10
    i32 = lambda t: t.to(torch.int32).cuda()
    ps = ops.PairSet(i32(torch.cat([hi, pad])), i32(torch.cat([wi, -pad])), i32(torch.tensor([P])), i32(rowptr), cap, T,
                     agt_ctrs.cuda(), ctx_ctrs.cuda())
    rn = lambda *shape, fan: torch.randn(*shape, generator=g) * (1.5 / fan ** 0.5)
    inp = dict(wd0=rn(C, 2, fan=2), bd0=rn(C, fan=2), w_d2=rn(C, C, fan=C), w_c0=rn(C, 3 * C, fan=3 * C),
               gd=1 + 0.1 * (2 * torch.rand(C, generator=g) - 1), btd=0.1 * torch.randn(C, generator=g),
               gc=1 + 0.1 * (2 * torch.rand(C, generator=g) - 1), btc=0.1 * torch.randn(C, generator=g),
               U=torch.randn(T, C, generator=g), V=torch.randn(S, C, generator=g),
               dS=torch.randn(T, C, generator=g), agt_ctrs=agt_ctrs, ctx_ctrs=ctx_ctrs)
    return ps, inp, hi, wi


def leaves(inp, only=None):
    return {k: inp[k].cuda().requires_grad_(only is None or k in only) for k in NAMES}


def fused(A, ps, x):
    return A.AttPairsFn.apply(ps, x["wd0"], x["bd0"], x["w_d2"], x["gd"], x["btd"], x["w_c0"], x["U"], x["V"], x["gc"], x["btc"])


def gn64(x, g, b):
    mu = x.mean(1, keepdim=True)
    var = ((x - mu) ** 2).mean(1, keepdim=True)
    return (x - mu) / torch.sqrt(var + EPS) * g + b


def reference64(inp, hi, wi, masks):
    """The formulas of include/lgcn.h (lgcn_att_pairs_train / _bwd) in float64 on the CPU, per pair, index_add_ into S; the
    three ReLUs are multiplications with the masks the kernel stored.  Returns (S, gradients by name + "dc", the three
    pre-activations)."""
    x = {k: inp[k].double().requires_grad_(True) for k in NAMES if k != "w_c0"}
    wc = inp["w_c0"][:, :C].double().requires_grad_(True)
    mk = masks.double()
    d = inp["agt_ctrs"].double()[hi] - inp["ctx_ctrs"].double()[wi]
    z0 = d @ x["wd0"].t() + x["bd0"]
    y1 = gn64((z0 * mk[:, 0]) @ x["w_d2"].t(), x["gd"], x["btd"])
    c = (y1 * mk[:, 1]) @ wc.t() + x["U"][hi] + x["V"][wi]
    c.retain_grad()
    y2 = gn64(c, x["gc"], x["btc"])
    Sx = torch.zeros(T, C, dtype=torch.float64).index_add(0, hi, y2 * mk[:, 2])
    (Sx * inp["dS"].double()).sum().backward()
    grads = {k: v.grad for k, v in x.items()}
    grads["w_c0"], grads["dc"] = wc.grad, c.grad
    return Sx.detach(), grads, (z0.detach(), y1.detach(), y2.detach())


def composed(M, A, ops, ps, inp, P):
    """The pair stage as today's Att.run_train composes it (lanegcn.py, the lines from `delta` to `m`), on the same leaves,
    and its segment sum: (S, gradients by name + "dc")."""
    x = leaves(inp)
    hi, wi = ps.hi[:P].long(), ps.wi[:P].long()
    gn = lambda w, b: types.SimpleNamespace(weight=w, bias=b, eps=EPS)
    delta = ps.agt_ctrs[hi] - ps.ctx_ctrs[wi]
    h1 = torch.relu(torch.nn.functional.linear(delta, x["wd0"], x["bd0"]))
    e = A.linear_gn(h1, x["w_d2"], gn=gn(x["gd"], x["btd"]), relu=True)
    c = A.PairAddFn.apply(A.linear_gn(e, x["w_c0"], col0=0), x["U"], x["V"], ps)
    m = A.gn_act(c, gn=gn(x["gc"], x["btc"]), relu=True)
    got = {}
    m.grad_fn.register_hook(lambda grad_in, grad_out: got.__setitem__("dc", grad_in[0].detach().clone()))
    i32 = dict(dtype=torch.int32, device="cuda")
    plan = types.SimpleNamespace(rowptr=ps.rowptr, col=None)
    plan_t = types.SimpleNamespace(rowptr=torch.arange(P + 1, **i32), col=ps.hi[:P].contiguous())
    Sx = A.GatherSumFn.apply(m, plan, plan_t, T)
    (Sx * inp["dS"].cuda()).sum().backward()
    got.update({k: v.grad for k, v in x.items()})
    got["w_c0"] = got["w_c0"][:, :C]
    return Sx.detach(), got


def err(got, want):
    return rel_err(got.detach().double().cpu().numpy(), want.numpy())


@pytest.mark.parametrize("P,n_chunks", CASES)
def test_against_fp64(mods, mma_scope, P, n_chunks):
    """S, dU, dV, the eight parameter gradients and dc against the fp64 restatement.  Bar per tensor: twice the error of
    today's composed path (f32 mode) against the same reference, floored at 1e-6 -- both are fp32 chains of the same length,
    only the summation order differs -- under a hard ceiling of 1e-4, the project's parity bar."""
    M, A, ops = mods
    mma_scope("f32")
    ps, inp, hi, wi = make_case(ops, P)
    x = leaves(inp)
    m, masks_raw = ops.att_pairs_train(ps, x["wd0"].detach(), x["bd0"].detach(), x["w_d2"].detach(),
                                       (x["gd"].detach(), x["btd"].detach()), x["w_c0"].detach(), x["U"].detach(),
                                       x["V"].detach(), (x["gc"].detach(), x["btc"].detach()))
    masks = ops.att_pair_masks(masks_raw, P).cpu()
    assert masks.shape == (P, 3, C) and masks.dtype == torch.bool
    S_ref, g_ref, pre = reference64(inp, hi, wi, masks)
    # the stored masks are the signs of the pre-activations wherever those are not on the knife edge
    for k, z in enumerate(pre):
        clear = z.abs() > 1e-4 * z.abs().amax(1, keepdim=True)
        assert clear.float().mean() > 0.99
        assert bool(((z > 0) == masks[:, k])[clear].all()), k

    if n_chunks is None:
        Sx = fused(A, ps, x)
        (Sx * inp["dS"].cuda()).sum().backward()
        got = {k: v.grad for k, v in x.items()}
        assert bool((got["w_c0"][:, C:] == 0).all())               # the U / V row blocks own those columns
        got["w_c0"] = got["w_c0"][:, :C]
        got["dc"] = None
    else:
        Sx = ops.gather_sum(m, ps.rowptr, None, T)
        got = {"dc": None}
    d = {k: v.detach() for k, v in x.items()}
    out = ops.att_pairs_bwd(ps, inp["dS"].cuda(), masks_raw, d["wd0"], d["bd0"], d["w_d2"], (d["gd"], d["btd"]), d["w_c0"],
                            d["U"], d["V"], (d["gc"], d["btc"]), n_chunks=n_chunks)
    got["dc"] = out["dc"][:P]
    if n_chunks is not None:
        rp, col = ps.csr_by_wi(S)
        got.update(wd0=out["d_wd0"], bd0=out["d_bd0"], w_d2=out["d_wd2"], gd=out["d_gd"], btd=out["d_btd"], w_c0=out["d_wc0e"],
                   gc=out["d_gc"], btc=out["d_btc"], U=ops.gather_sum(out["dc"], ps.rowptr, None, T),
                   V=ops.gather_sum(out["dc"], rp, col, S))
    S_cmp, g_cmp = composed(M, A, ops, ps, inp, P)

    rows = [("S", err(Sx, S_ref), err(S_cmp, S_ref))]
    rows += [(k, err(got[k], g_ref[k]), err(g_cmp[k], g_ref[k])) for k in NAMES + ("dc",)]
    for name, e_new, e_cmp in rows:
        print("P=%d chunks=%s %-5s fused %.3e composed %.3e" % (P, n_chunks, name, e_new, e_cmp))
    bad = [(n, a, b) for n, a, b in rows if not a <= min(max(2 * b, 1e-6), 1e-4)]
    assert not bad, bad


@pytest.mark.parametrize("P", [1, 33, 130])
def test_forward_is_inference_forward_bitwise(mods, mma_scope, P):
    M, A, ops = mods
    mma_scope("f32")
    ps, inp, _, _ = make_case(ops, P)
    x = {k: inp[k].cuda() for k in NAMES}
    m, _ = ops.att_pairs_train(ps, x["wd0"], x["bd0"], x["w_d2"], (x["gd"], x["btd"]), x["w_c0"], x["U"], x["V"],
                               (x["gc"], x["btc"]))
    m_inf = ops.att_pairs(ps, x["wd0"], x["bd0"], ops.packed(x["w_d2"]), (x["gd"], x["btd"]), ops.packed(x["w_c0"], 0, C),
                          x["U"], x["V"], (x["gc"], x["btc"]))
    assert torch.equal(m[:P].view(torch.int32), m_inf[:P].view(torch.int32))
    Sx = fused(A, ps, x)
    assert torch.equal(Sx.view(torch.int32), ops.gather_sum(m, ps.rowptr, None, T).view(torch.int32))


def fwd_bwd(A, ps, inp, only=None):
    x = leaves(inp, only)
    Sx = fused(A, ps, x)
    (Sx * inp["dS"].cuda()).sum().backward()
    return [Sx.detach()] + [x[k].grad for k in NAMES]


def same_bits(a, b):
    return (a is None and b is None) or torch.equal(a.view(torch.int32), b.view(torch.int32))


def test_repeatable_and_independent_of_the_matrix_mode(mods, mma_scope):
    M, A, ops = mods
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
    """cap = P + 40: m, masks and dc rows >= P keep their sentinel; hi / wi beyond P hold +-2^30 and are never used."""
    M, A, ops = mods
    ps, inp, _, _ = make_case(ops, P)
    x = {k: inp[k].cuda() for k in NAMES}
    m = torch.full((ps.cap, C), -7.5, device="cuda")
    masks = torch.full((ps.cap, 12), 0x5A5A5A5A, dtype=torch.int32, device="cuda")
    dc = torch.full((ps.cap, C), -7.5, device="cuda")
    args = (x["wd0"], x["bd0"], x["w_d2"], (x["gd"], x["btd"]), x["w_c0"], x["U"], x["V"], (x["gc"], x["btc"]))
    ops.att_pairs_train(ps, *args, m=m, masks=masks)
    out = ops.att_pairs_bwd(ps, inp["dS"].cuda(), masks, *args, dc=dc)
    torch.cuda.synchronize()
    assert out["dc"] is dc
    assert bool((m[P:] == -7.5).all()) and bool((dc[P:] == -7.5).all()) and bool((masks[P:] == 0x5A5A5A5A).all())
    assert bool(torch.isfinite(m[:P]).all()) and bool(torch.isfinite(dc[:P]).all()) and bool((m[:P] >= 0).all())
    assert all(bool(torch.isfinite(v).all()) for v in out.values())


def test_absent_gradients(mods):
    M, A, ops = mods
    ps, inp, _, _ = make_case(ops, 130)
    x = leaves(inp)
    fused(A, ps, x).sum().backward()
    assert all(x[k].grad is not None and bool(x[k].grad.abs().max() > 0) for k in NAMES)
    z = leaves(inp)
    (fused(A, ps, z) * 0).sum().backward()
    assert all(z[k].grad is not None and bool((z[k].grad == 0).all()) for k in NAMES)
    full, only_u = fwd_bwd(A, ps, inp), fwd_bwd(A, ps, inp, only=("U",))
    iu = 1 + NAMES.index("U")
    assert all(g is None for i, g in enumerate(only_u) if i not in (0, iu))
    assert same_bits(full[iu], only_u[iu]) and same_bits(full[0], only_u[0])
    # the kernel's shorter walks: nothing upstream of e wanted (it stops after dW_c0e and the GN_c sums), and the dist
    # parameters without dW_c0e
    for only in (("w_c0", "gc"), ("btc",), ("w_d2",), ("wd0", "gd", "V")):
        part = fwd_bwd(A, ps, inp, only=only)
        for i, k in enumerate(NAMES):
            assert (part[1 + i] is None) == (k not in only), (only, k)
            assert k not in only or same_bits(full[1 + i], part[1 + i]), (only, k)


# ------------------------------------------------------------------ module level
def att_inputs(M, seed=3):
    """Two scenes, 40 targets and 30 context rows, a threshold that keeps a few hundred of the 2 x 20 x 15 candidates."""
    g = torch.Generator().manual_seed(seed)
    agt_ctrs = [(torch.randn(20, 2, generator=g) * 6).cuda() for _ in range(2)]
    ctx_ctrs = [(torch.randn(15, 2, generator=g) * 6).cuda() for _ in range(2)]
    agt_idcs = [torch.arange(20).cuda(), torch.arange(20, 40).cuda()]
    ctx_idcs = [torch.arange(15).cuda(), torch.arange(15, 30).cuda()]
    agts, ctx = torch.randn(40, C, generator=g).cuda(), torch.randn(30, C, generator=g).cuda()
    w_out = torch.randn(40, C, generator=g).cuda()
    return agts, agt_idcs, agt_ctrs, ctx, ctx_idcs, ctx_ctrs, w_out


def att_module(M, seed=11):
    torch.manual_seed(seed)
    att = M.Att(C, C)
    with torch.no_grad():
        for n, p in att.named_parameters():
            if "norm" in n and n.endswith("weight"):
                p.copy_(1 + 0.1 * (2 * torch.rand_like(p) - 1))
            elif "norm" in n:
                p.copy_(0.1 * torch.randn_like(p))
            elif p.dim() == 2:
                p.copy_(torch.randn_like(p) * (1.5 / p.shape[1] ** 0.5))
    return att


def att_step(M, att, inputs, dist_th=10.0):
    agts, agt_idcs, agt_ctrs, ctx, ctx_idcs, ctx_ctrs, w_out = inputs
    a, c = agts.clone().requires_grad_(True), ctx.clone().requires_grad_(True)
    att.zero_grad(set_to_none=True)
    ps = M.build_pairs(agt_idcs, agt_ctrs, ctx_idcs, ctx_ctrs, dist_th)
    out = att(a, agt_idcs, agt_ctrs, c, ctx_idcs, ctx_ctrs, dist_th, pairs=ps)
    (out * w_out).sum().backward()
    res = {"out": out.detach(), "d agts": a.grad, "d ctx": c.grad}
    res.update({n: p.grad for n, p in att.named_parameters()})
    return res, ps.count()


def att_reference64(att, inputs, dist_th=10.0):
    """The whole Att layer in float64 on the CPU: the oracle's statement of lanegcn.py:662-710 on double tensors, under
    autograd, for the same loss as att_step."""
    agts, agt_idcs, agt_ctrs, ctx, ctx_idcs, ctx_ctrs, w_out = inputs
    sd = {"att." + n: p.detach().cpu().double().requires_grad_(True) for n, p in att.named_parameters()}
    a, c = agts.cpu().double().requires_grad_(True), ctx.cpu().double().requires_grad_(True)
    out = O.att(a, [t.cpu().double() for t in agt_ctrs], c, [t.cpu().double() for t in ctx_ctrs], dist_th, sd, "att")
    (out * w_out.cpu().double()).sum().backward()
    res = {"out": out.detach(), "d agts": a.grad, "d ctx": c.grad}
    res.update({n[4:]: v.grad for n, v in sd.items()})
    return res


def test_module_on_against_off(mods, mma_scope):
    """Att(128,128), switch on and off in f32 mode, each against the float64 layer: output, d agts, d ctx and every parameter
    gradient at the bar of test_against_fp64 -- twice the composed path's error, floored at 1e-6, never above 1e-4."""
    M, A, ops = mods
    mma_scope("f32")
    inputs = att_inputs(M)
    att = att_module(M).cuda().train()
    res = {}
    for flag in (False, True):
        M.Att.train_hip = flag
        try:
            res[flag], P = att_step(M, att, inputs)
        finally:
            M.Att.train_hip = False
    assert 200 <= P <= 600, P
    ref = att_reference64(att, inputs)
    assert set(ref) == set(res[True]) and all(v is not None for v in res[True].values())
    rows = [(k, err(res[True][k], ref[k]), err(res[False][k], ref[k])) for k in ref]
    for name, e_new, e_cmp in rows:
        print("P=%d %-24s fused %.3e composed %.3e" % (P, name, e_new, e_cmp))
    bad = [(n, x, y) for n, x, y in rows if not x <= min(max(2 * y, 1e-6), 1e-4)]
    assert not bad, bad


@pytest.mark.parametrize("mode", ["f32", "f16x2"])
def test_whole_net_training_step(mods, hip_on, mma_scope, count_fused, golden, train_golden, ref_state_names, mode):
    """A2M / M2A / A2A with the switch on: the reference's own loss, gradients and Adam update (tests/golden/train_b4.npz),
    the body and the bars of test_training_step_matches_reference; every one of the six Att layers took the fused path."""
    mma_scope(mode)
    TG.test_training_step_matches_reference(golden, train_golden, ref_state_names, mode)
    assert len(count_fused) == 6, len(count_fused)


@pytest.mark.parametrize("mode", ["f32", "f16x2"])
def test_batch32_training_step(mods, hip_on, count_fused, ref_state_names, mode):
    """The training step at batch 32 (S2) with the switch on against the reference's own loss and gradients
    (tests/golden/train_b32.npz): the body and the bars of test_training_step_batch32_matches_reference."""
    TG.test_training_step_batch32_matches_reference(ref_state_names, mode)
    assert len(count_fused) == 6, len(count_fused)


def test_fresh_images_after_optimizer_step(mods, hip_on, mma_scope):
    """After Optimizer.step the next forward + backward is bit for bit that of a freshly constructed copy holding the updated
    weights: no stale F32 or transposed image."""
    M, A, ops = mods
    mma_scope("f16x2")
    inputs = att_inputs(M)
    att = att_module(M).cuda().train()
    att_step(M, att, inputs)
    opt = M.Optimizer(att.parameters(), M.config)
    before = {k: v.clone() for k, v in att.state_dict().items()}
    opt.step(0.0)
    assert any(not torch.equal(before[k], v) for k, v in att.state_dict().items())
    got, _ = att_step(M, att, inputs)
    fresh = M.Att(C, C)
    fresh.load_state_dict({k: v.detach().cpu().clone() for k, v in att.state_dict().items()})
    want, _ = att_step(M, fresh.cuda().train(), inputs)
    assert all(same_bits(got[k], want[k]) for k in want), [k for k in want if not same_bits(got[k], want[k])]


def test_switch_off_means_untouched(mods, monkeypatch, count_fused):
    M, A, ops = mods
    calls = count_fused
    assert M.Att.train_hip is False
    inputs = att_inputs(M)
    att = att_module(M).cuda().train()
    att_step(M, att, inputs)
    assert not calls
    monkeypatch.setattr(M.Att, "train_hip", True)
    att_step(M, att, inputs)
    assert len(calls) == 1
