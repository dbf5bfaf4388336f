"""GPU: ActorNet under autograd on HIP (Conv1dGNFn: lgcn_conv1d_gn_train forward, lgcn_conv1d_gn_bwd backward) -- per-unit
gradients against fp64 CPU autograd, the train-mode forward bit for bit against the inference forward, the whole module's
gradients against an fp64 CPU copy, repeatability, no stock convolution in the f16x2 training step, fresh weight images
after an optimizer step."""
import copy

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def mods():
    import lanegcn_amd  # noqa: F401
    from lanegcn_amd import autograd as A
    from lanegcn_amd import lanegcn as M
    from lanegcn_amd import ops
    return M, A, ops


@pytest.fixture
def f16x2(mods):
    M, _, ops = mods
    prev, prev_impl, prev_train = ops.get_mma(), M.ActorNet.impl, M.ActorNet.train_hip
    ops.set_mma("f16x2")
    M.ActorNet.impl, M.ActorNet.train_hip = "hip", True
    yield
    ops.set_mma(prev)
    M.ActorNet.impl, M.ActorNet.train_hip = prev_impl, prev_train


def make_net(M, seed=7):
    torch.manual_seed(seed)
    net = M.ActorNet(M.config)
    with torch.no_grad():
        for p in net.parameters():
            if p.dim() == 1:
                p.uniform_(0.5, 1.5) if p.mean() > 0.5 else p.uniform_(-0.3, 0.3)
    return net


def unit_shapes(M):
    """(cin, cout, ks, stride, lin) of ActorNet's 20 conv units, in forward order."""
    net, lin, out = M.ActorNet(M.config), 20, []
    for g in net.groups:
        for b in g:
            lo = (lin + 2 - 3) // b.conv1.stride[0] + 1
            out.append((b.conv1.in_channels, b.conv1.out_channels, 3, b.conv1.stride[0], lin))
            if b.downsample is not None:
                out.append((b.downsample[0].in_channels, b.downsample[0].out_channels, 1, b.downsample[0].stride[0], lin))
            out.append((b.conv2.in_channels, b.conv2.out_channels, 3, 1, lo))
            lin = lo
    for i, lens in zip(range(2, -1, -1), (5, 10, 20)):
        out.append((net.lateral[i].conv.in_channels, net.lateral[i].conv.out_channels, 3, 1, lens))
    out += [(128, 128, 3, 1, 20), (128, 128, 3, 1, 20)]
    assert len(out) == 20
    return out


def _cases():
    import lanegcn_amd  # noqa: F401
    from lanegcn_amd import lanegcn as M
    cases = []
    for shp in sorted(set(unit_shapes(M))):
        cin, cout, ks, stride, lin = shp
        lout = (lin + 2 * ((ks - 1) // 2) - ks) // stride + 1
        cases += [(shp, 1600, 1, True), (shp, 333, 2 if lout % 2 == 0 else 0, False), (shp, 3, 0, True),
                  (shp, 333, 1, False), (shp, 3, 2 if lout % 2 == 0 else 1, True)]
    return cases


@pytest.mark.parametrize("shape,n,res_mode,relu", _cases())
def test_unit_gradients_vs_fp64(mods, f16x2, shape, n, res_mode, relu):
    """One unit (conv + GN [+ res | + up2(res)] [+ ReLU]) forward on HIP, backward on lgcn_conv1d_gn_bwd: dx, dW, dgamma,
    dbeta, dres against fp64 CPU autograd with the HIP forward's ReLU mask."""
    M, A, ops = mods
    cin, cout, ks, stride, lin = shape
    torch.manual_seed(n + cin + 7 * cout + res_mode)
    conv = torch.nn.Conv1d(cin, cout, ks, stride=stride, padding=(ks - 1) // 2, bias=False)
    gn = torch.nn.GroupNorm(1, cout)
    with torch.no_grad():
        gn.weight.uniform_(0.5, 1.5)
        gn.bias.uniform_(-0.5, 0.5)
    lout = (lin + 2 * ((ks - 1) // 2) - ks) // stride + 1
    x0 = torch.randn(n, lin, cin) * 2 + 0.3
    r0 = torch.randn(n, lout // 2 if res_mode == 2 else lout, cout) if res_mode else None
    w0 = torch.randn(n, lout, cout)
    convg, gng = copy.deepcopy(conv).cuda(), copy.deepcopy(gn).cuda()
    xg = x0.cuda().requires_grad_(True)
    rg = r0.cuda().requires_grad_(True) if res_mode else None
    out = A.conv1d_gn(xg, convg, gng, res=rg, res_up2=res_mode == 2, relu=relu)
    (out * w0.cuda()).sum().backward()
    # fp64 reference in NCL
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
    assert float((out.detach().cpu().double() - ref.detach().transpose(1, 2)).abs().max()) <= 2e-4

    def close(got, want):
        scale = float(want.abs().max()) + 1e-9
        err = float((got.detach().cpu().double() - want).abs().max())
        assert err <= 2e-5 * scale + 1e-6, (err, scale)

    close(xg.grad, xd.grad.transpose(1, 2))
    close(convg.weight.grad, wd.grad)
    close(gng.weight.grad, gd.grad)
    close(gng.bias.grad, bd.grad)
    if res_mode:
        close(rg.grad, rd.grad.transpose(1, 2))


def test_unit_skips_dx_when_input_needs_no_grad(mods, f16x2):
    M, A, ops = mods
    conv, gn = torch.nn.Conv1d(3, 32, 3, padding=1, bias=False).cuda(), torch.nn.GroupNorm(1, 32).cuda()
    x = torch.randn(50, 20, 3).cuda()
    out = A.conv1d_gn(x, conv, gn, relu=True)
    out.sum().backward()
    assert conv.weight.grad is not None and gn.weight.grad is not None and x.grad is None
    dx, dw, dg, db, dres = ops.conv1d_gn_bwd(torch.ones_like(out), x, out, out, conv.weight, 1, gn.weight, gn.eps,
                                             relu=True, want_dx=False)
    assert dx is None and dres is None and torch.equal(dw, ops.conv1d_gn_bwd(torch.ones_like(out), x, out, out, conv.weight,
                                                                               1, gn.weight, gn.eps, relu=True)[1])


def test_train_forward_equals_inference_forward_bitwise(mods, f16x2):
    """Train-mode ActorNet (Conv1dGNFn units) against the no-grad forward with fuse_blocks = False: bit for bit."""
    M, A, ops = mods
    net = make_net(M).cuda()
    for n in (1600, 333, 3):
        x = torch.randn(n, 3, 20).cuda() * 3.0
        assert net._hip_ok(x)
        got = net(x)
        assert got.requires_grad
        prev = M.ActorNet.fuse_blocks
        try:
            M.ActorNet.fuse_blocks = False
            with torch.no_grad():
                want = net(x)
        finally:
            M.ActorNet.fuse_blocks = prev
        assert torch.equal(got.detach().view(torch.int32), want.view(torch.int32)), n


def _record_units(A):
    rec, orig = [], A.conv1d_gn

    def wrapped(x, conv, gn, res=None, res_up2=False, relu=False):
        out = orig(x, conv, gn, res=res, res_up2=res_up2, relu=relu)
        rec.append((relu, out.detach()))
        return out
    return rec, orig, wrapped


def test_whole_actornet_gradients_vs_fp64(mods, f16x2):
    """All parameter gradients of ActorNet at 1,600 actors against an fp64 CPU copy of the module.  The fp64 side applies
    the HIP forward's ReLU masks at the 14 ReLUs (as the per-unit test does), so the bar does not depend on how many
    pre-activations sit within rounding of zero; those flips are counted and reported, and the module's own fp64 forward
    (its stock path) must agree with the HIP output."""
    M, A, ops = mods
    net = make_net(M, seed=11)
    net64 = copy.deepcopy(net).double()
    netg = net.cuda()
    x = torch.randn(1600, 3, 20) * 3.0
    w = torch.randn(1600, 128)
    rec, orig, wrapped = _record_units(A)
    A.conv1d_gn = wrapped
    try:
        got = netg(x.cuda())
        (got * w.cuda()).sum().backward()
    finally:
        A.conv1d_gn = orig
    assert len(rec) == 20
    with torch.no_grad():
        stock = net64(x.double())
    assert float((got.detach().cpu().double() - stock).abs().max()) <= 1e-4
    masks = iter([(o.cpu() > 0).double().transpose(1, 2) for relu, o in rec if relu])
    flips = []

    def unit(h, conv, gn, res=None, up2=False, relu=False):
        z = F.group_norm(F.conv1d(h, conv.weight, stride=conv.stride[0], padding=conv.padding[0]), 1, gn.weight, gn.bias,
                         gn.eps)
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
    out = res1d(net64.output, out)[:, :, -1]
    (out * w.double()).sum().backward()
    assert len(flips) == 14
    worst = {}
    p64 = dict(net64.named_parameters())
    for name, p in netg.named_parameters():
        ref = p64[name].grad
        worst[name] = float((p.grad.cpu().double() - ref).abs().max()) / (float(ref.abs().max()) + 1e-12)
    print("\n[ActorNet 1600 actors] ReLU flips against fp64: %d; worst relative gradient error %.2e (%s)" %
          (sum(flips), max(worst.values()), max(worst, key=worst.get)))
    assert max(worst.values()) <= 1e-4, sorted(worst.items(), key=lambda kv: -kv[1])[:5]


def test_backward_is_repeatable(mods, f16x2):
    M, A, ops = mods
    net = make_net(M, seed=3).cuda()
    x = torch.randn(1600, 3, 20).cuda()
    w = torch.randn(1600, 128).cuda()
    grads = []
    for _ in range(2):
        net.zero_grad(set_to_none=True)
        (net(x) * w).sum().backward()
        grads.append([p.grad.clone() for p in net.parameters()])
    for a, b in zip(*grads):
        assert torch.equal(a.view(torch.int32), b.view(torch.int32))


def test_train_hip_is_opt_in(mods):
    M, A, ops = mods
    assert M.ActorNet.train_hip is False
    net = make_net(M).cuda()
    x = torch.randn(20, 3, 20).cuda()
    prev = ops.get_mma()
    try:
        ops.set_mma("f16x2")
        assert not net._hip_ok(x)                      # parameters require grad: the stock training path
        with torch.no_grad():
            assert net._hip_ok(x) == (M.ActorNet.impl == "hip")
    finally:
        ops.set_mma(prev)


def test_no_stock_convolution_in_f16x2_training(mods, f16x2, monkeypatch):
    """f16x2 train mode: forward and backward without nn.Conv1d's stock convolution; f32 mode still calls it (the
    existing training path is kept outside the gate)."""
    M, A, ops = mods
    net = make_net(M, seed=5).cuda()
    x = torch.randn(333, 3, 20).cuda()
    calls = []
    stock = torch.nn.Conv1d._conv_forward

    def refuse(self, *a, **k):
        raise AssertionError("stock Conv1d called")
    monkeypatch.setattr(torch.nn.Conv1d, "_conv_forward", refuse)
    net(x).sum().backward()
    assert all(p.grad is not None for p in net.parameters())

    def count(self, *a, **k):
        calls.append(1)
        return stock(self, *a, **k)
    monkeypatch.setattr(torch.nn.Conv1d, "_conv_forward", count)
    ops.set_mma("f32")
    net(x).sum().backward()
    assert len(calls) == 20


def test_fresh_weight_images_after_optimizer_step(mods, f16x2):
    """After opt.step() the next train-mode forward equals the no-grad forward of a fresh copy of the updated weights,
    bit for bit, and so do the gradients (no stale packed forward or backward images)."""
    M, A, ops = mods
    net = make_net(M, seed=9).cuda()
    x = torch.randn(333, 3, 20).cuda()
    w = torch.randn(333, 128).cuda()
    opt = torch.optim.SGD(net.parameters(), lr=0.5)
    (net(x) * w).sum().backward()
    opt.step()
    net.zero_grad(set_to_none=True)
    got = net(x)
    (got * w).sum().backward()
    fresh = M.ActorNet(M.config).cuda()
    fresh.load_state_dict(net.state_dict())
    prev = M.ActorNet.fuse_blocks
    try:
        M.ActorNet.fuse_blocks = False
        with torch.no_grad():
            want = fresh(x)
    finally:
        M.ActorNet.fuse_blocks = prev
    assert torch.equal(got.detach().view(torch.int32), want.view(torch.int32))
    (fresh(x) * w).sum().backward()
    for a, b in zip(net.parameters(), fresh.parameters()):
        assert torch.equal(a.grad.view(torch.int32), b.grad.view(torch.int32))
