"""GPU: ActorNet's exact-fp32 HIP units (lgcn_conv1d_gn_f32, ActorNet.exact) -- per-unit forward and gradients against
fp64, train forward = inference forward, every matrix mode, no stock convolution, the whole module against an fp64 copy,
repeatability, fresh weight images, the whole-Net graph cache, the range guard's re-run, and the batch-32 reference
training check with an ActorNet trained on HIP.

Inputs as in test_gpu_actornet_train.py: x = randn * 2 + 0.3, PyTorch's default Conv1d init, gamma ~ U(0.5, 1.5),
beta ~ U(-0.5, 0.5), fixed seeds."""
import copy

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import test_gpu_actornet_train as T
from golden_io import load_scenes
from oracle import lanegcn_oracle as O

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def mods():
    import lanegcn_amd  # noqa: F401
    from lanegcn_amd import autograd as A
    from lanegcn_amd import lanegcn as M
    from lanegcn_amd import ops
    return M, A, ops


@pytest.fixture
def exact(mods):
    """ActorNet.exact and train_hip set, matrix mode f32 (the mode the f16x2 units do not serve)."""
    M, _, ops = mods
    prev = (ops.get_mma(), M.ActorNet.impl, M.ActorNet.train_hip, M.ActorNet.exact, ops.get_guard())
    ops.set_mma("f32")
    M.ActorNet.impl, M.ActorNet.train_hip, M.ActorNet.exact = "hip", True, True
    yield
    ops.set_mma(prev[0])
    M.ActorNet.impl, M.ActorNet.train_hip, M.ActorNet.exact = prev[1:4]
    ops.set_guard(prev[4])


def bits(t):
    return t.detach().contiguous().view(torch.int32)


def _lout(shape):
    cin, cout, ks, stride, lin = shape
    return (lin + 2 * ((ks - 1) // 2) - ks) // stride + 1


def _unit_inputs(shape, n, res_mode):
    cin, cout, ks, stride, lin = shape
    torch.manual_seed(n + cin + 7 * cout + res_mode)
    conv = torch.nn.Conv1d(cin, cout, ks, stride=stride, padding=(ks - 1) // 2, bias=False)
    gn = torch.nn.GroupNorm(1, cout)
    with torch.no_grad():
        gn.weight.uniform_(0.5, 1.5)
        gn.bias.uniform_(-0.5, 0.5)
    lout = _lout(shape)
    x0 = torch.randn(n, lin, cin) * 2 + 0.3
    r0 = torch.randn(n, lout // 2 if res_mode == 2 else lout, cout) if res_mode else None
    return conv, gn, x0, r0


def _forward_cases():
    import lanegcn_amd  # noqa: F401
    from lanegcn_amd import lanegcn as M
    cases = []
    for shp in sorted(set(T.unit_shapes(M))):
        modes = (0, 1, 2) if _lout(shp) % 2 == 0 else (0, 1)
        cases += [(shp, n, m, relu) for n in (1600, 333, 3) for m in modes for relu in (False, True)]
    return cases


def _chain_conv(x, w, stride):
    """The convolution in fp32 on the CPU as ONE sequential accumulation chain per output: taps outer, channels inner,
    acc = acc + x * w (two roundings per step).  x [n, lin, cin], w [cout, cin, ks] -> [n, lout, cout]."""
    n, lin, cin = x.shape
    cout, _, ks = w.shape
    pad = (ks - 1) // 2
    lout = (lin + 2 * pad - ks) // stride + 1
    xp = F.pad(x, (0, 0, pad, pad))                                   # zero rows: adding 0 * w = 0 changes nothing
    acc = torch.zeros(n, lout, cout, dtype=torch.float32)
    for t in range(ks):
        xt = xp[:, t:t + (lout - 1) * stride + 1:stride, :]           # [n, lout, cin]
        for c in range(cin):
            acc = acc + xt[:, :, c:c + 1] * w[:, c, t].view(1, 1, cout)
    return acc


def _gn_two_pass(y, gamma, beta, eps):
    """GroupNorm(1 group) of y [n, lout, cout] in its dtype: mean, then the variance about it (biased)."""
    mean = y.mean(dim=(1, 2), keepdim=True)
    var = ((y - mean) ** 2).mean(dim=(1, 2), keepdim=True)
    return (y - mean) * (1.0 / torch.sqrt(var + eps)) * gamma.view(1, 1, -1) + beta.view(1, 1, -1)


def _epilogue(z, r, res_mode, relu, M):
    if res_mode:
        z = z + (M.upsample2_linear(r.transpose(1, 2)).transpose(1, 2) if res_mode == 2 else r)
    return z.relu() if relu else z


_REFS = {}                     # (shape, n, res_mode) -> (y64, y_chain) of the last case: the ReLU twin reuses them


@pytest.mark.parametrize("shape,n,res_mode,relu", _forward_cases())
def test_unit_forward_vs_fp64(mods, exact, shape, n, res_mode, relu):
    """out and the saved pre-norm y of one exact unit against fp64: the project's fp32-kernel bar (2e-5 scale + 1e-6) and
    the measured bar 1.5 e_chain + 2 ulp(scale), e_chain = the error of a one-chain fp32 emulation on the CPU."""
    M, A, ops = mods
    cin, cout, ks, stride, lin = shape
    conv, gn, x0, r0 = _unit_inputs(shape, n, res_mode)
    w0, g0, b0 = conv.weight.detach(), gn.weight.detach(), gn.bias.detach()
    # fp64
    key = (shape, n, res_mode)
    if key not in _REFS:
        _REFS.clear()
        _REFS[key] = (F.conv1d(x0.double().transpose(1, 2), w0.double(), stride=stride, padding=(ks - 1) // 2).transpose(1, 2),
                      _chain_conv(x0, w0, stride))
    y64, y_chain = _REFS[key]
    want = _epilogue(_gn_two_pass(y64, g0.double(), b0.double(), gn.eps), None if r0 is None else r0.double(), res_mode, relu, M)
    # the chain emulation in fp32 (the convolution does not depend on the residual mode or the ReLU: the seed does)
    out_chain = _epilogue(_gn_two_pass(y_chain, g0, b0, gn.eps), r0, res_mode, relu, M)
    # stock fp32 on the GPU
    xg, wg, gg, bg = x0.cuda(), w0.cuda(), g0.cuda(), b0.cuda()
    rg = None if r0 is None else r0.cuda()
    y_stock = F.conv1d(xg.transpose(1, 2), wg, stride=stride, padding=(ks - 1) // 2)
    out_stock = _epilogue(F.group_norm(y_stock, 1, gg, bg, gn.eps).transpose(1, 2), rg, res_mode, relu, M)
    # the unit
    out, y = ops.conv1d_gn_train(xg, wg, stride, gg, bg, gn.eps, res=rg, res_up2=res_mode == 2, relu=relu, exact=True)
    inf = ops.conv1d_gn(xg, wg, stride, gg, bg, gn.eps, res=rg, res_up2=res_mode == 2, relu=relu, exact=True)
    assert torch.equal(bits(out), bits(inf))

    def err(a, ref):
        return float((a.detach().cpu().double() - ref).abs().max())

    for what, hip, chain, stock, ref in (("y", y, y_chain, y_stock.transpose(1, 2), y64), ("out", out, out_chain, out_stock, want)):
        scale = float(ref.abs().max())
        e_hip, e_chain, e_stock = err(hip, ref), err(chain, ref), err(stock, ref)
        print("\n[exact unit %s n=%d res=%d relu=%d] %s: scale %.3g e_hip %.3e e_chain %.3e e_stock %.3e" %
              (shape, n, res_mode, relu, what, scale, e_hip, e_chain, e_stock))
        assert e_hip <= 2e-5 * scale + 1e-6, (what, e_hip, scale)
        assert e_hip <= 1.5 * e_chain + 2 * 2.0 ** -24 * scale, (what, e_hip, e_chain, scale)


@pytest.mark.parametrize("shape,n,res_mode,relu", T._cases())
def test_unit_gradients_vs_fp64(mods, exact, shape, n, res_mode, relu):
    """Conv1dGNFn with exact=True: dx, dW, dgamma, dbeta, dres against fp64 CPU autograd with the HIP forward's ReLU mask
    (the cases and the bar of test_gpu_actornet_train.test_unit_gradients_vs_fp64)."""
    M, A, ops = mods
    cin, cout, ks, stride, lin = shape
    conv, gn, x0, r0 = _unit_inputs(shape, n, res_mode)
    lout = _lout(shape)
    w0 = torch.randn(n, lout, cout)
    convg, gng = copy.deepcopy(conv).cuda(), copy.deepcopy(gn).cuda()
    xg = x0.cuda().requires_grad_(True)
    rg = r0.cuda().requires_grad_(True) if res_mode else None
    out = A.conv1d_gn(xg, convg, gng, res=rg, res_up2=res_mode == 2, relu=relu, exact=True)
    (out * w0.cuda()).sum().backward()
    xd = x0.double().transpose(1, 2).requires_grad_(True)
    wd = conv.weight.detach().double().requires_grad_(True)
    gd, bd = gn.weight.detach().double().requires_grad_(True), gn.bias.detach().double().requires_grad_(True)
    ref = F.group_norm(F.conv1d(xd, wd, stride=stride, padding=(ks - 1) // 2), 1, gd, bd, gn.eps)
    rd = None
    if res_mode:
        rd = r0.double().transpose(1, 2).requires_grad_(True)
        ref = ref + (M.upsample2_linear(rd) if res_mode == 2 else rd)
    if relu:
        ref = ref * (out.detach().cpu().double().transpose(1, 2) > 0)
    (ref * w0.double().transpose(1, 2)).sum().backward()

    def close(got, want):
        scale = float(want.abs().max()) + 1e-9
        err = float((got.detach().cpu().double() - want).abs().max())
        assert err <= 2e-5 * scale + 1e-6, (err, scale)

    close(out, ref.detach().transpose(1, 2))
    close(xg.grad, xd.grad.transpose(1, 2))
    close(convg.weight.grad, wd.grad)
    close(gng.weight.grad, gd.grad)
    close(gng.bias.grad, bd.grad)
    if res_mode:
        close(rg.grad, rd.grad.transpose(1, 2))


def test_train_forward_equals_inference_forward_bitwise(mods, exact):
    M, A, ops = mods
    net = T.make_net(M).cuda()
    for n in (1600, 333, 3):
        x = torch.randn(n, 3, 20).cuda() * 3.0
        assert net._hip_ok(x)
        got = net(x)
        assert got.requires_grad
        with torch.no_grad():
            want = net(x)
        assert torch.equal(bits(got), bits(want)), n


def test_every_matrix_mode(mods, exact):
    """The exact units take no matrix mode: bit-identical outputs under all four, HIP in all four; without the switch the
    HIP units serve f16x2 only, as before."""
    M, A, ops = mods
    net = T.make_net(M, seed=13).cuda()
    x = torch.randn(333, 3, 20).cuda() * 2 + 0.3
    outs = {}
    with torch.no_grad():
        for mode in ("f32", "bf16x3", "f16x2", "bf16"):
            ops.set_mma(mode)
            assert net._hip_ok(x), mode
            outs[mode] = net(x)
        for mode, o in outs.items():
            assert torch.equal(bits(o), bits(outs["f32"])), mode
        M.ActorNet.exact = False
        for mode in ("f32", "bf16x3", "f16x2", "bf16"):
            ops.set_mma(mode)
            assert net._hip_ok(x) == (mode == "f16x2"), mode


def test_no_stock_convolution(mods, exact, monkeypatch):
    """f32 mode with exact and train_hip: forward + backward without nn.Conv1d's stock convolution, inference without
    F.conv2d (the channels-last MIOpen path)."""
    M, A, ops = mods
    net = T.make_net(M, seed=5).cuda()
    x = torch.randn(333, 3, 20).cuda()

    def refuse(*a, **k):
        raise AssertionError("stock convolution called")
    monkeypatch.setattr(torch.nn.Conv1d, "_conv_forward", refuse)
    monkeypatch.setattr(F, "conv2d", refuse)
    assert ops.get_mma() == "f32"
    net(x).sum().backward()
    assert all(p.grad is not None for p in net.parameters())
    with torch.no_grad():
        assert torch.isfinite(net(x)).all()


def _fp64_with_masks(M, net64, x, masks, flips):
    masks = iter(masks)

    def unit(h, conv, gn, res=None, up2=False, relu=False):
        z = F.group_norm(F.conv1d(h, conv.weight, stride=conv.stride[0], padding=conv.padding[0]), 1, gn.weight, gn.bias, gn.eps)
        if res is not None:
            z = z + (M.upsample2_linear(res) if up2 else res)
        if relu:
            m = next(masks)
            flips.append(int(((z.detach() > 0).double() != m).sum()))
            z = z * m
        return z

    def res1d(b, h):
        o = unit(h, b.conv1, b.bn1, relu=True)
        skip = h if b.downsample is None else unit(h, b.downsample[0], b.downsample[1])
        return unit(o, b.conv2, b.bn2, res=skip, relu=b.act)

    out, pyramid = x.double(), []
    for g in net64.groups:
        for b in g:
            out = res1d(b, out)
        pyramid.append(out)
    out = unit(pyramid[-1], net64.lateral[-1].conv, net64.lateral[-1].norm, relu=net64.lateral[-1].act)
    for i in range(len(pyramid) - 2, -1, -1):
        out = unit(pyramid[i], net64.lateral[i].conv, net64.lateral[i].norm, res=out, up2=True)
    return res1d(net64.output, out)[:, :, -1]


def test_whole_actornet_vs_fp64(mods, exact):
    """1,600 actors: the exact HIP forward, the stock fp32 path and (for the record) the f16x2 units against an fp64 copy
    of the module; all parameter gradients of the exact path against fp64 with the HIP forward's ReLU masks."""
    M, A, ops = mods
    net = T.make_net(M, seed=11)
    net64 = copy.deepcopy(net).double()
    netg = net.cuda()
    x = torch.randn(1600, 3, 20) * 3.0
    w = torch.randn(1600, 128)
    with torch.no_grad():
        want = net64(x.double())
        hip = netg(x.cuda())
        M.ActorNet.impl = "miopen"
        stock = netg(x.cuda())
        M.ActorNet.impl, M.ActorNet.exact = "hip", False
        ops.set_mma("f16x2")
        f16 = netg(x.cuda())
        ops.set_mma("f32")
        M.ActorNet.exact = True
    e_hip, e_stock, e_f16 = (float((t.cpu().double() - want).abs().max()) for t in (hip, stock, f16))
    print("\n[ActorNet 1600 actors, max |out - fp64|, scale %.3g] exact HIP %.3e  stock fp32 %.3e  f16x2 HIP %.3e" %
          (float(want.abs().max()), e_hip, e_stock, e_f16))
    assert e_hip <= 1e-4
    assert e_hip <= 6 * e_stock, (e_hip, e_stock)

    rec, orig = [], A.conv1d_gn

    def wrapped(x_, conv, gn, **kw):
        out = orig(x_, conv, gn, **kw)
        assert kw.get("exact") is True
        rec.append((kw.get("relu", False), out.detach()))
        return out
    A.conv1d_gn = wrapped
    try:
        got = netg(x.cuda())
        (got * w.cuda()).sum().backward()
    finally:
        A.conv1d_gn = orig
    assert len(rec) == 20
    assert torch.equal(bits(got), bits(hip))
    flips = []
    out = _fp64_with_masks(M, net64, x, [(o.cpu() > 0).double().transpose(1, 2) for relu, o in rec if relu], flips)
    (out * w.double()).sum().backward()
    assert len(flips) == 14
    worst = {}
    p64 = dict(net64.named_parameters())
    for name, p in netg.named_parameters():
        ref = p64[name].grad
        worst[name] = float((p.grad.cpu().double() - ref).abs().max()) / (float(ref.abs().max()) + 1e-12)
    print("[ActorNet 1600 actors, exact] ReLU flips against fp64: %d; worst relative gradient error %.2e (%s)" %
          (sum(flips), max(worst.values()), max(worst, key=worst.get)))
    assert max(worst.values()) <= 1e-4, sorted(worst.items(), key=lambda kv: -kv[1])[:5]


def test_repeatable_and_fresh_images(mods, exact):
    M, A, ops = mods
    net = T.make_net(M, seed=3).cuda()
    x = torch.randn(1600, 3, 20).cuda()
    w = torch.randn(1600, 128).cuda()
    runs = []
    for _ in range(2):
        net.zero_grad(set_to_none=True)
        out = net(x)
        (out * w).sum().backward()
        runs.append([out.detach().clone()] + [p.grad.clone() for p in net.parameters()])
    for a, b in zip(*runs):
        assert torch.equal(bits(a), bits(b))
    # after an optimizer step: no stale fp32 fragment image
    opt = torch.optim.SGD(net.parameters(), lr=0.5)
    opt.step()
    net.zero_grad(set_to_none=True)
    got = net(x)
    (got * w).sum().backward()
    fresh = M.ActorNet(M.config).cuda()
    fresh.load_state_dict(net.state_dict())
    with torch.no_grad():
        want = fresh(x)
    assert not torch.equal(bits(got), bits(runs[0][0]))
    assert torch.equal(bits(got), bits(want))
    (fresh(x) * w).sum().backward()
    for a, b in zip(net.parameters(), fresh.parameters()):
        assert torch.equal(bits(a.grad), bits(b.grad))


def _golden_net(M, golden, ref_state_names):
    net = M.Net(M.config)
    net.load_state_dict(O.seeded_state(ref_state_names, int(golden["seed"])), strict=True)
    return net.cuda().eval()


def _cat(out):
    return torch.cat([t.reshape(-1) for t in out["cls"]] + [t.reshape(-1) for t in out["reg"]])


def test_graph_cache_sees_the_switch(mods, exact, golden, ref_state_names):
    """The whole-Net graph captured with the f16x2 units is not replayed once ActorNet.exact is flipped."""
    M, A, ops = mods
    from lanegcn_amd import data as gen
    ops.set_mma("f16x2")
    M.ActorNet.exact = False
    net = _golden_net(M, golden, ref_state_names)
    batch = gen.collate_fn(load_scenes(golden))
    with torch.no_grad():
        cached = [net(batch) for _ in range(3)][-1]
        assert net.__dict__["_graph_state"]["graph"] is not None
        M.ActorNet.exact = True
        got = net(batch)
        M.Net.graph_cache = False
        try:
            want = _golden_net(M, golden, ref_state_names)(batch)
        finally:
            M.Net.graph_cache = True
    assert torch.equal(bits(_cat(got)), bits(_cat(want)))
    assert not torch.equal(bits(_cat(got)), bits(_cat(cached)))


def test_guard_rerun_stays_on_hip(mods, exact, golden, ref_state_names, monkeypatch):
    """f16x2 mode, guard policy "reroute", a batch that trips the range guard: the bf16x3 re-run keeps ActorNet on the exact
    HIP units (no stock convolution anywhere) and equals a plain bf16x3-mode forward bit for bit.  The actor tracks are
    scaled up by 1e6: the f16x2 units would overflow on them, the exact units have no operand range and hand normalised
    features on -- so with them scaled tracks alone cannot trip the guard any more, and the hot-path operand that passes
    65504 here is MapNet's segment embedding (the lane segments scaled by 1e6; the pair sets depend on centres only)."""
    M, A, ops = mods
    from lanegcn_amd import data as gen
    from lanegcn_amd._lib import LgcnError
    scenes = copy.deepcopy(load_scenes(golden))
    for sc in scenes:
        sc["feats"] = (np.asarray(sc["feats"], np.float32) * 1e6).astype(np.float32)
        sc["graph"]["feats"] = (np.asarray(sc["graph"]["feats"], np.float32) * 1e6).astype(np.float32)
    batch = gen.collate_fn(scenes)
    net = _golden_net(M, golden, ref_state_names)

    def refuse(*a, **k):
        raise AssertionError("stock convolution called")
    monkeypatch.setattr(torch.nn.Conv1d, "_conv_forward", refuse)
    monkeypatch.setattr(F, "conv2d", refuse)
    M.Net.graph_cache = False
    try:
        with torch.no_grad():
            ops.set_mma("f16x2")
            ops.set_guard("raise")
            with pytest.raises(LgcnError):                  # the guard is tripped
                net(batch)
            ops.set_guard("reroute")
            got = net(batch)
            assert ops.get_mma() == "f16x2"
            ops.set_mma("bf16x3")
            want = net(batch)
    finally:
        M.Net.graph_cache = True
    assert torch.isfinite(_cat(got)).all()
    assert torch.equal(bits(_cat(got)), bits(_cat(want)))


def test_training_step_batch32_matches_reference_with_hip_actornet(mods, exact, ref_state_names):
    """test_gpu_training.test_training_step_batch32_matches_reference[f16x2] -- its body, assertions and bars as they are --
    with ActorNet trained on the exact HIP units (train_hip = exact = True) instead of the stock convolutions.  Measured on
    MI355X: no ReLU flip at any stage output, hot-path gradients max 7.8e-5 of their scale (median 9.2e-6; bar 1e-4), where
    the f16x2 units gave 3.1e-4.
    The same body in f32 hot-path mode does NOT meet its bars with the HIP-trained ActorNet and is therefore not a test:
    no flip is counted at the six stage outputs, so the 1e-4 bar applies, and the hot-path gradients reach 1.12e-3 of
    their scale (median 2.45e-4 over 35 tensors, a2a.att.1.ctx.1.weight worst; loss, gradient norms and the stage
    forwards agree).  DESIGN.md section 5b has both sets of figures."""
    import test_gpu_training as TT
    M, A, ops = mods
    assert M.ActorNet.train_hip and M.ActorNet.exact and M.ActorNet.impl == "hip"
    TT.test_training_step_batch32_matches_reference(ref_state_names, "f16x2")
