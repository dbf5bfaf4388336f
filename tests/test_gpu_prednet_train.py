"""GPU: PredNet's tail trained on HIP (PredNet.train_hip): PredRegFn / PredFinalFn on lgcn_pred_reg, lgcn_pred_final_train,
lgcn_pred_reg_bwd and lgcn_pred_final_bwd -- against fp64 CPU autograd, against the inference forward (bitwise), against the
stock training path on the device, and inside one whole training step of Net."""
import json
import os

import numpy as np
import pytest
import torch

from golden_io import load_scenes
from oracle import lanegcn_oracle as O
from test_gpu_training import meta_relu_flips, rel_err, train_golden  # noqa: F401  (train_golden: a fixture)

pytestmark = pytest.mark.gpu
GOLDEN_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")

# (A, M, T): one actor (partial block, partial wave group); the M and np2 limits; np2 = 14 (no multiple of 8) one actor past a
# 32-actor block; the workload's M and T; more than one partial-sum chunk
SHAPES = [(1, 6, 30), (5, 8, 32), (33, 3, 7), (70, 6, 30), (333, 6, 30), (1600, 6, 30)]


@pytest.fixture(scope="module")
def mods():
    import lanegcn_amd  # noqa: F401
    from lanegcn_amd import autograd as A
    from lanegcn_amd import lanegcn as M
    from lanegcn_amd import ops
    return M, A, ops


@pytest.fixture
def train_hip(mods):
    M = mods[0]
    prev = M.PredNet.train_hip
    M.PredNet.train_hip = True
    yield
    M.PredNet.train_hip = prev


@pytest.fixture
def mma_scope(mods):
    ops = mods[2]
    prev = ops.get_mma()
    yield ops.set_mma
    ops.set_mma(prev)


def close(got, want):
    """The bar tests/test_gpu_actornet_train.py holds HIP backward kernels to: err <= 2e-5 max|ref| + 1e-6."""
    want = want.detach()
    scale = float(want.abs().max())
    err = float((got.detach().cpu().double().reshape(want.shape) - want).abs().max())
    print("err %.3e scale %.3e" % (err, scale))
    assert err <= 2e-5 * scale + 1e-6, (err, scale)


def order_of(out, reg):
    """order[a, j] = the mode whose (unsorted) reg row the forward put in slot j of out; rows of reg must be distinct."""
    eq = (out.detach()[:, :, None] == reg.detach()[:, None]).flatten(3).all(-1)          # [A, slot, mode]
    assert bool((eq.sum(-1) == 1).all())
    return eq.int().argmax(-1)


def reg_inputs(a, m, t, seed=0):
    g = torch.Generator().manual_seed(1000 * seed + 7 * a + 3 * m + t)
    h = [torch.randn(a, 128, generator=g).relu() for _ in range(m)]
    w = [torch.randn(2 * t, 128, generator=g) * 0.2 for _ in range(m)]
    b = [torch.randn(2 * t, generator=g) * 0.5 for _ in range(m)]
    ctrs = torch.randn(a, 2, generator=g) * 30
    wd = (torch.rand(128, 2, generator=g) * 2 - 1) * 0.7
    bd = (torch.rand(128, generator=g) * 2 - 1) * 0.7
    w_reg, w_hd = torch.randn(a, m, t, 2, generator=g), torch.randn(a * m, 128, generator=g)
    return h, w, b, ctrs, wd, bd, w_reg, w_hd


def final_inputs(a, m, t, seed=0):
    g = torch.Generator().manual_seed(2000 * seed + 7 * a + 3 * m + t)
    f = torch.randn(a * m, 128, generator=g)
    wc = (torch.rand(1, 128, generator=g) * 2 - 1) * 0.1
    bc = torch.rand(1, generator=g)
    reg = torch.randn(a, m, t, 2, generator=g) * 30
    w_cls, w_out = torch.randn(a, m, generator=g), torch.randn(a, m, t, 2, generator=g)
    return f, wc, bc, reg, w_cls, w_out


def leaves(ts, dtype=None, dev=None):
    out = []
    for t in ts:
        t = t.detach().clone()
        t = t.to(dtype) if dtype is not None else t
        t = t.to(dev) if dev is not None else t
        out.append(t.requires_grad_(True))
    return out


@pytest.mark.parametrize("a,m,t", SHAPES)
def test_pred_reg_fn_vs_fp64(mods, a, m, t):
    """PredRegFn alone: reg, hd and every gradient against fp64 CPU autograd that uses the HIP forward's own hd > 0 mask.
    lgcn_pred_reg_bwd sums over chunks of 64 actors: (70, 6, 30) is the first shape with two records, (333, 6, 30) and
    (1600, 6, 30) have 6 and 25."""
    M, A, ops = mods
    h0, w0, b0, ctrs, wd0, bd0, w_reg, w_hd = reg_inputs(a, m, t)
    h, w, b = leaves(h0, dev="cuda"), leaves(w0, dev="cuda"), leaves(b0, dev="cuda")
    wd, bd = leaves([wd0, bd0], dev="cuda")
    reg, hd = A.PredRegFn.apply(*h, *w, *b, ctrs.cuda(), wd, bd)
    assert reg.shape == (a, m, t, 2) and hd.shape == (a * m, 128)
    ((reg * w_reg.cuda()).sum() + (hd * w_hd.cuda()).sum()).backward()
    # fp64 reference
    hr, wr, br = leaves(h0, torch.float64), leaves(w0, torch.float64), leaves(b0, torch.float64)
    wdr, bdr = leaves([wd0, bd0], torch.float64)
    c = ctrs.double()
    regr = torch.stack([hr[i] @ wr[i].t() + br[i] for i in range(m)], 1).view(a, m, t, 2) + c.view(a, 1, 1, 2)
    d = (c.view(a, 1, 2) - regr[:, :, -1].detach()).reshape(-1, 2)
    hdr = (d @ wdr.t() + bdr) * (hd.detach().cpu() > 0)
    ((regr * w_reg.double()).sum() + (hdr * w_hd.double()).sum()).backward()
    close(reg, regr)
    close(hd, hdr)
    for i in range(m):
        close(h[i].grad, hr[i].grad)
        close(w[i].grad, wr[i].grad)
        close(b[i].grad, br[i].grad)
    close(wd.grad, wdr.grad)
    close(bd.grad, bdr.grad)


@pytest.mark.parametrize("a,m,t", SHAPES)
def test_pred_final_fn_vs_fp64(mods, a, m, t):
    """PredFinalFn alone: cls, out and every gradient against fp64 CPU autograd that gathers in the HIP forward's own order
    (read back from out).  lgcn_pred_final_bwd writes one record per 16 actors: (33, 3, 7) is the first shape with more
    than one, (1600, 6, 30) has 100."""
    M, A, ops = mods
    f0, wc0, bc0, reg0, w_cls, w_out = final_inputs(a, m, t)
    f, wc, bc, reg = leaves([f0, wc0, bc0, reg0], dev="cuda")
    cls, out = A.PredFinalFn.apply(f, wc, bc, reg)
    assert cls.shape == (a, m) and out.shape == (a, m, t, 2)
    ((cls * w_cls.cuda()).sum() + (out * w_out.cuda()).sum()).backward()
    order = order_of(out, reg).cpu().long()
    assert bool((cls.detach()[:, :-1] >= cls.detach()[:, 1:]).all())
    fr, wcr, bcr, regr = leaves([f0, wc0, bc0, reg0], torch.float64)
    s = (fr @ wcr.t() + bcr).view(a, m)
    rows = torch.arange(a).view(-1, 1).expand_as(order)
    clsr, outr = s[rows, order], regr[rows, order]
    ((clsr * w_cls.double()).sum() + (outr * w_out.double()).sum()).backward()
    close(cls, clsr)
    close(out, outr)
    close(f.grad, fr.grad)
    close(wc.grad, wcr.grad)
    close(bc.grad, bcr.grad)
    close(reg.grad, regr.grad)


def test_ties(mods):
    """Two and three modes of an actor with exactly equal scores: the training forward equals lgcn_pred_final bit for bit
    (equal scores keep mode order), and the gradient of each tied slot lands on the mode the forward put there."""
    M, A, ops = mods
    a, m, t = 5, 6, 30
    f0, wc0, bc0, reg0, w_cls, w_out = final_inputs(a, m, t, seed=1)
    f0 = f0.view(a, m, 128)
    f0[0, 4] = f0[0, 1]                       # actor 0: modes 1 and 4 tie
    f0[1, 2] = f0[1, 0]                       # actor 1: modes 0, 2 and 5 tie
    f0[1, 5] = f0[1, 0]
    f0 = f0.reshape(a * m, 128)
    f, wc, bc, reg = leaves([f0, wc0, bc0, reg0], dev="cuda")
    cls, out = A.PredFinalFn.apply(f, wc, bc, reg)
    with torch.no_grad():
        cls_i, out_i = ops.pred_final(f, wc, bc, reg)
    assert torch.equal(cls.detach().view(torch.int32), cls_i.view(torch.int32))
    assert torch.equal(out.detach().view(torch.int32), out_i.view(torch.int32))
    order = order_of(out, reg)
    c = cls.detach()
    pos = {(ai, int(order[ai, j])): j for ai in range(a) for j in range(m)}
    assert float(c[0, pos[0, 1]]) == float(c[0, pos[0, 4]]) and pos[0, 4] == pos[0, 1] + 1
    assert float(c[1, pos[1, 0]]) == float(c[1, pos[1, 2]]) == float(c[1, pos[1, 5]])
    assert pos[1, 2] == pos[1, 0] + 1 and pos[1, 5] == pos[1, 0] + 2
    g_cls, g_out = w_cls.cuda(), w_out.cuda()
    ((cls * g_cls).sum() + (out * g_out).sum()).backward()
    rows = torch.arange(a, device="cuda").view(-1, 1).expand_as(order)
    g_s = torch.zeros(a, m, device="cuda")
    g_s[rows, order.long()] = g_cls                                         # a permutation: no accumulation
    assert torch.equal(f.grad, (g_s.reshape(-1, 1) * wc.detach().view(1, 128)))    # one fp32 product per element
    want = torch.zeros_like(g_out)
    want[rows, order.long()] = g_out
    assert torch.equal(reg.grad, want)


def test_absent_gradients(mods):
    """A loss that uses one output only (the other's gradient is absent, not zeros) gives bit for bit what zeros give; an h
    that needs no gradient gets none and leaves the weight gradients unchanged bit for bit."""
    M, A, ops = mods
    a, m, t = 70, 6, 30
    f0, wc0, bc0, reg0, w_cls, w_out = final_inputs(a, m, t, seed=2)

    def final(loss):
        ts = leaves([f0, wc0, bc0, reg0], dev="cuda")
        cls, out = A.PredFinalFn.apply(*ts)
        loss(cls, out).backward()
        return [x.grad for x in ts]

    for only, zeros in ((lambda c, o: (c * w_cls.cuda()).sum(), lambda c, o: (c * w_cls.cuda()).sum() + (o * 0).sum()),
                        (lambda c, o: (o * w_out.cuda()).sum(), lambda c, o: (o * w_out.cuda()).sum() + (c * 0).sum())):
        got, want = final(only), final(zeros)
        for x, y in zip(got, want):
            assert x is not None and torch.equal(x, y)

    h0, w0, b0, ctrs, wd0, bd0, w_reg, w_hd = reg_inputs(a, m, t, seed=2)

    def regfn(loss, h_grad=True):
        h = leaves(h0, dev="cuda") if h_grad else [x.cuda() for x in h0]
        rest = leaves(w0 + b0, dev="cuda")
        wd, bd = leaves([wd0, bd0], dev="cuda")
        reg, hd = A.PredRegFn.apply(*h, *rest, ctrs.cuda(), wd, bd)
        loss(reg, hd).backward()
        return [x.grad for x in h], [x.grad for x in rest + [wd, bd]]

    full = lambda r, d: (r * w_reg.cuda()).sum() + (d * w_hd.cuda()).sum()
    only_reg, zeros_hd = (lambda r, d: (r * w_reg.cuda()).sum()), (lambda r, d: (r * w_reg.cuda()).sum() + (d * 0).sum())
    (gh, gw), (zh, zw) = regfn(only_reg), regfn(zeros_hd)
    for x, y in zip(gh + gw, zh + zw):
        assert x is not None and torch.equal(x, y)
    (fh, fw), (nh, nw) = regfn(full), regfn(full, h_grad=False)
    assert all(x is None for x in nh) and all(x is not None for x in fh)
    for x, y in zip(fw, nw):
        assert torch.equal(x, y)
    # the op itself: no d_h tensor is made
    reg, hd = ops.pred_reg([x.cuda() for x in h0], [x.cuda() for x in w0], [x.cuda() for x in b0], ctrs.cuda(), wd0.cuda(), bd0.cuda())
    d_h, d_w, d_b, d_wd, d_bd = ops.pred_reg_bwd(w_reg.cuda(), None, [x.cuda() for x in h0], [x.cuda() for x in w0], hd, reg,
                                                 ctrs.cuda(), want_h=[False] * m)
    assert d_h == [None] * m and float(d_wd.abs().max()) == 0.0 and float(d_bd.abs().max()) == 0.0
    for x, y in zip(d_w + d_b, gw[:2 * m]):
        assert torch.equal(x, y)


def pred_net(M, seed=21):
    torch.manual_seed(seed)
    return M.PredNet(M.config)


def net_inputs(sizes, seed):
    n = sum(sizes)
    g = torch.Generator().manual_seed(seed)
    actors = torch.randn(n, 128, generator=g).relu().cuda()
    ctrs = (torch.randn(n, 2, generator=g) * 30).cuda()
    idcs, lo = [], 0
    for s in sizes:
        idcs.append(torch.arange(lo, lo + s, device="cuda"))
        lo += s
    return actors, idcs, [ctrs[i] for i in idcs]


@pytest.mark.parametrize("mode", ["f32", "f16x2"])
@pytest.mark.parametrize("sizes", [(100, 33, 200), (1,)])
def test_train_forward_is_inference_forward_bitwise(mods, train_hip, mma_scope, mode, sizes):
    M, A, ops = mods
    mma_scope(mode)
    net = pred_net(M).cuda().train()
    actors, idcs, ctrs = net_inputs(sizes, 5)
    out = net(actors, idcs, ctrs)
    assert out["cls"][0].requires_grad and out["reg"][0].requires_grad
    with torch.no_grad():
        cls_i, reg_i = net.forward_flat(actors, torch.cat(ctrs, 0))
    cls_t, reg_t = torch.cat(out["cls"], 0).detach(), torch.cat(out["reg"], 0).detach()
    assert torch.equal(cls_t.view(torch.int32), cls_i.view(torch.int32))
    assert torch.equal(reg_t.view(torch.int32), reg_i.view(torch.int32))


def step(net, actors, idcs, ctrs, seed=3):
    out = net(actors, idcs, ctrs)
    cls, reg = torch.cat(out["cls"], 0), torch.cat(out["reg"], 0)
    g = torch.Generator().manual_seed(seed)
    w_cls, w_reg = torch.randn(cls.shape, generator=g).cuda(), torch.randn(reg.shape, generator=g).cuda()
    ((cls * w_cls).sum() + (reg * w_reg).sum()).backward()
    return cls.detach(), reg.detach()


def test_no_stock_op_in_the_tail(mods, train_hip, monkeypatch):
    """With the flag set no nn.Linear and no sort runs in PredNet's forward + backward; with it off the stock path does."""
    M, A, ops = mods
    net = pred_net(M).cuda().train()
    actors, idcs, ctrs = net_inputs((20, 17), 6)
    calls = []
    real_linear = torch.nn.functional.linear

    def refuse(*a, **k):
        raise AssertionError("stock op in PredNet's HIP training tail")

    with monkeypatch.context() as mp:
        mp.setattr(torch.nn.functional, "linear", refuse)
        mp.setattr(torch, "sort", refuse)
        mp.setattr(torch.Tensor, "sort", refuse)
        step(net, actors.clone().requires_grad_(True), idcs, ctrs)
    for n, p in net.named_parameters():
        assert p.grad is not None and bool(torch.isfinite(p.grad).all()), n

    def counted(*a, **k):
        calls.append(1)
        return real_linear(*a, **k)

    M.PredNet.train_hip = False
    with monkeypatch.context() as mp:
        mp.setattr(torch.nn.functional, "linear", counted)
        step(net, actors.clone().requires_grad_(True), idcs, ctrs)
    assert len(calls) >= len(net.pred) + 2                  # the heads, AttDest.dist[0], the score Linear


@pytest.mark.parametrize("n", [37, 1])
def test_module_vs_stock_training_path(mods, train_hip, mma_scope, n):
    """Flag on against flag off in strict f32 mode, same weights: the LinearRes / AttDest row-block Functions are shared, only
    the tail differs.  These inputs' smallest gap between adjacent sorted scores (2.4e-3 / 2.3e-2) and smallest AttDest
    pre-activation (6.9e-5 / 1.1e-3) are far above the 1e-4 by which the two forwards may differ."""
    M, A, ops = mods
    mma_scope("f32")
    net = pred_net(M, 21).cuda().train()
    g = torch.Generator().manual_seed(100 + n)
    actors0 = torch.randn(n, 128, generator=g).relu()
    ctrs = (torch.randn(n, 2, generator=g) * 30).cuda()
    idcs = [torch.arange(n, device="cuda")]
    res = {}
    for flag in (True, False):
        M.PredNet.train_hip = flag
        net.zero_grad(set_to_none=True)
        actors = actors0.cuda().requires_grad_(True)
        cls, reg = step(net, actors, idcs, [ctrs])
        res[flag] = (cls, reg, actors.grad.clone(), {k: p.grad.clone() for k, p in net.named_parameters()})
    (cls_h, reg_h, da_h, gp_h), (cls_s, reg_s, da_s, gp_s) = res[True], res[False]
    # the two paths sorted the modes alike: every slot of one is nearest to the same slot of the other
    dist = (reg_h[:, :, None] - reg_s[:, None]).flatten(3).abs().amax(-1)              # [A, slot, slot]
    assert bool((dist.argmin(-1) == torch.arange(reg_h.shape[1], device="cuda")).all())
    print("max |d cls| %.3e" % float((cls_h - cls_s).abs().max()))
    errs = {k: rel_err(gp_h[k].cpu().numpy(), gp_s[k].cpu().numpy()) for k in gp_s}
    errs["d actors"] = rel_err(da_h.cpu().numpy(), da_s.cpu().numpy())
    print(sorted(errs.items(), key=lambda kv: -kv[1])[:5])
    assert max(errs.values()) <= 1e-4, sorted(errs.items(), key=lambda kv: -kv[1])[:5]


def test_backward_is_repeatable(mods, train_hip):
    M, A, ops = mods
    net = pred_net(M).cuda().train()
    actors, idcs, ctrs = net_inputs((1600,), 8)
    grads = []
    for _ in range(2):
        net.zero_grad(set_to_none=True)
        x = actors.clone().requires_grad_(True)
        step(net, x, idcs, ctrs)
        grads.append([p.grad.clone() for p in net.parameters()] + [x.grad.clone()])
    for x, y in zip(*grads):
        assert torch.equal(x.view(torch.int32), y.view(torch.int32))


def test_whole_net_training_step(mods, train_hip, mma_scope, golden, train_golden, ref_state_names):  # noqa: F811
    """One step of Net on the train_b4 fixture in f16x2 with PredNet's tail on HIP, at the bars of
    test_training_step_matches_reference (f16x2: no A2M.meta flips, stored gradients at 1e-4)."""
    M, A, ops = mods
    from lanegcn_amd import data as gen
    mma_scope("f16x2")
    scenes = load_scenes(golden)
    net = M.Net(M.config)
    net.load_state_dict(O.seeded_state(ref_state_names, int(train_golden["seed"])), strict=True)
    net = net.cuda().train()
    loss_fn = M.Loss(M.config).cuda()
    batch = gen.collate_fn(scenes)
    loss_out = loss_fn(net(batch), batch)
    loss_out["loss"].backward()
    torch.cuda.synchronize()
    assert loss_out["num_cls"] == int(train_golden["loss/num_cls"])
    assert loss_out["num_reg"] == int(train_golden["loss/num_reg"])
    for k in ("cls_loss", "reg_loss", "loss"):
        assert float(loss_out[k].detach()) == pytest.approx(float(train_golden["loss/" + k]), rel=2e-5), k
    names = json.load(open(os.path.join(GOLDEN_DIR, "param_names.json")))
    params = dict(net.named_parameters())
    assert list(params) == names
    norms = np.array([float(params[n].grad.norm()) if params[n].grad is not None else -1.0 for n in names])
    assert (norms >= 0).all()
    bad = [(n, a, b) for n, a, b in zip(names, norms, train_golden["grad_norms"]) if abs(a - b) > 2e-3 * b + 1e-6]
    assert not bad, bad[:5]
    assert len(meta_relu_flips(net, scenes, ref_state_names, int(train_golden["seed"]))) == 0
    worst = {k[5:]: rel_err(params[k[5:]].grad.cpu().numpy(), ref) for k, ref in train_golden.items() if k.startswith("grad/")}
    print(sorted(worst.items(), key=lambda kv: -kv[1])[:5])
    assert max(worst.values()) <= 1e-4, sorted(worst.items(), key=lambda kv: -kv[1])[:5]


def test_fresh_weights_after_optimizer_step(mods, train_hip):
    """After SGD.step() the next train-mode forward uses the updated weights: bit for bit the no_grad forward of a fresh
    module loaded from the updated state_dict."""
    M, A, ops = mods
    net = pred_net(M).cuda().train()
    actors, idcs, ctrs = net_inputs((40, 9), 9)
    opt = torch.optim.SGD(net.parameters(), lr=0.05)
    step(net, actors, idcs, ctrs)
    before = {k: v.clone() for k, v in net.state_dict().items()}
    opt.step()
    assert any(not torch.equal(before[k], v) for k, v in net.state_dict().items())
    out = net(actors, idcs, ctrs)
    assert out["cls"][0].requires_grad
    fresh = M.PredNet(M.config)
    fresh.load_state_dict({k: v.detach().cpu().clone() for k, v in net.state_dict().items()})
    fresh = fresh.cuda().eval()
    with torch.no_grad():
        cls_i, reg_i = fresh.forward_flat(actors, torch.cat(ctrs, 0))
    assert torch.equal(torch.cat(out["cls"], 0).detach().view(torch.int32), cls_i.view(torch.int32))
    assert torch.equal(torch.cat(out["reg"], 0).detach().view(torch.int32), reg_i.view(torch.int32))
