"""GPU: ActorNet's HIP convolution path against float64 over operand scale and statistics, every launch held to a model of
its operand format (tests/split_model.py: conv1d_unit / res1d_block / actor_net; cases: tests/actornet_cases.py).

The default f16x2 path runs ActorNet on lgcn_conv1d_gn / lgcn_res1d_gn / lgcn_res1d_pair_gn: 20 conv + GroupNorm units that
round both operands to two fp16 planes -- the input rows, the packed weight images and, inside the fused launches, the
intermediate rows that go back into LDS.  Every other test of that path draws O(1) weights and compares at an absolute
1e-4 (three single units apart, which test_gpu_operand_scale.py scales).  That bar does see a dropped plane or swapped
upsampling taps at O(1) ("ActorNet": the mutations tried), but nothing that depends on scale: with the fp16
subnormals of the staged rows flushed it passes, and the fused launches and the whole module were never scaled.  Here:

    one launch of one unit            rel_err(kernel) <= split_model.bar(e_model) = max(2 e_model, 1e-6)
    blocks, groups, the whole module  rel_err(kernel) <= hot_path_cases.bar(e_model, e_ref32) = max(2 e_model, 4 e_ref32, 1e-6)
    (both capped at 1e-4 wherever e_model <= 5e-5);   rel_err = max |x - fp64| / max |fp64|

e_model: the float64 model of the same launches with the operands rounded where the kernels round them; e_ref32: the stock
module's fp32 CPU run against its double run.  Both come from the CPU at test time (actornet_cases, cached); nothing comes
from the kernels.  The fused launches are also bit for bit their composition of single units, and the whole module with
fuse_blocks / fuse_groups on is bit for bit the module with them off, at every state, not only at O(1).

States: conv weights x 2^{0, -4, -8, -12, -16}; input x 2^{12, -8, -14}; the wide state (per-tensor scales 2^U[-8, 2], GroupNorm
scales in [0.05, 8] with 10 % negative, shifts x 5).  Inputs: randn and track-like (zero rows in front, a stationary actor).
Actor counts 1 and 17: one past a full workgroup at every level; one whole-module case at 333.
Rows past the end: the three entry points through the C ABI with the output inside poisoned pads.
The exact units (lgcn_conv1d_gn_f32) and lgcn_gn_cl / lgcn_gn_cl_bwd, which serve the f32 / bf16x3 modes, run at the
scales where the squares of the centred values leave fp32 (values ~2^100): without the wide path of conv_gn_stats /
k_gn_cl* their outputs are beta (error 0.3 .. 1 against float64).
Fresh modules and weight tensors per case (no packed image is reused), ops.set_guard("raise") throughout.  Each case prints
model / fp32 reference / kernel before it asserts.  Measured figures: DESIGN.md section 5c, "ActorNet"."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import actornet_cases as AC
import split_model as S
from test_gpu_actornet_train import unit_shapes

pytestmark = pytest.mark.gpu

EPS = S.EPS
PAD = 64                                       # poisoned words in front of and behind every output (test_gpu_node_tail.py)
POISON = 0x7fc0dead                            # a NaN pattern no kernel writes
SCALE_STATES = AC.UNIFORM + AC.INPUT
WIDE_GRID = [(-100, 80), (60, 40), (-8, -8)]  # (s_x, s_w) exponents, as test_gpu_operand_scale.py's exact modes


def _shapes():
    return sorted(set(unit_shapes(AC.modules())))


def _lout(shape):
    cin, cout, ks, stride, lin = shape
    return (lin + 2 * ((ks - 1) // 2) - ks) // stride + 1


def _res_modes(shape):
    return (0, 1, 2) if _lout(shape) % 2 == 0 else (0, 1)


SHAPE_IDS = ["%d-%d-k%d-s%d-l%d" % s for s in _shapes()]
STATE_IDS = [AC.case_id(s) for s in AC.STATES]


@pytest.fixture(scope="module")
def hip():
    import lanegcn_amd  # noqa: F401
    from lanegcn_amd import _lib as L
    from lanegcn_amd import lanegcn as M
    from lanegcn_amd import ops
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return M, ops, L


@pytest.fixture(autouse=True)
def guard_raises(hip):
    _, ops, _ = hip
    prev = ops.get_guard()
    ops.set_guard("raise")
    yield
    ops.set_guard(prev)


class Report:
    """Prints every figure, asserts at the end: one failing tensor does not hide the others' figures."""

    def __init__(self, head):
        self.head, self.bad = "ACTORNET " + head, []

    def check(self, what, got, e_model, truth, e_ref32=None, model=None):
        """e_ref32 None: one launch (split_model.bar); else hot_path_cases.bar."""
        got = got.detach().cpu().numpy().astype(np.float64)
        if model is not None:
            assert np.isfinite(truth).all() and np.isfinite(model).all(), "the case itself left the format's range: " + what
            e_model = S.rel_err(model, truth)
        assert got.shape == truth.shape and np.isfinite(truth).all(), what
        e_k = S.rel_err(got, truth)
        b = S.bar(e_model) if e_ref32 is None else AC.bar(e_model, e_ref32)
        print("\n%s %s: model %.3e fp32 ref %s kernel %.3e bar %.3e" % (self.head, what, e_model,
                                                                        "-" if e_ref32 is None else "%.3e" % e_ref32, e_k, b), end="")
        if not e_k <= b:                      # a NaN fails
            self.bad.append((what, e_model, e_ref32, e_k, b))

    def done(self):
        assert not self.bad, "%s (tensor, model, fp32 ref, kernel, bar): %s" % (self.head, self.bad)


def dev(t):
    return None if t is None else t.cuda()


def bits(t):
    return t.contiguous().view(torch.int32)


# ------------------------------------------------------------------ single units
@pytest.mark.parametrize("state", SCALE_STATES, ids=[AC.case_id(s) for s in SCALE_STATES])
@pytest.mark.parametrize("shape", _shapes(), ids=SHAPE_IDS)
def test_units_over_scale(hip, shape, state):
    """lgcn_conv1d_gn_train (out and the saved y) for every unit shape of ActorNet, residual modes 0 / 1 / 2 (the
    x2-upsampled one where lout is even), ReLU off and on, A = 1 and 17; lgcn_conv1d_gn is bit for bit its `out`."""
    M, ops, L = hip
    rep = Report("unit %d-%d-k%d-s%d-l%d %s" % (shape + (AC.case_id(state),)))
    for n_act in AC.COUNTS:
        for res_mode in _res_modes(shape):
            x, w, stride, gamma, beta, res = AC.unit_case(shape, n_act, state, res_mode)
            for relu in (False, True):
                kw = dict(res=res, res_up2=res_mode == 2, relu=relu)
                ref_out, ref_y = S.conv1d_unit(x, w, stride, gamma, beta, "f32", model=False, **kw)
                m_out, m_y = S.conv1d_unit(x, w, stride, gamma, beta, "f16x2", **kw)
                w_d = dev(w.clone())                                                   # a fresh tensor: a fresh packed image
                kw_d = dict(res=dev(res), res_up2=res_mode == 2, relu=relu)
                out, y = ops.conv1d_gn_train(dev(x), w_d, stride, dev(gamma), dev(beta), EPS, **kw_d)
                plain = ops.conv1d_gn(dev(x), w_d, stride, dev(gamma), dev(beta), EPS, **kw_d)
                tag = "A=%d res%d relu%d " % (n_act, res_mode, relu)
                rep.check(tag + "y", y, None, ref_y, model=m_y)
                rep.check(tag + "out", out, None, ref_out, model=m_out)
                assert torch.equal(bits(plain), bits(out)), tag + "lgcn_conv1d_gn differs from lgcn_conv1d_gn_train"
    rep.done()


# ------------------------------------------------------------------ fused launches
def _unit(ops, conv, norm, x, **kw):
    return ops.conv1d_gn(x, conv.weight, conv.stride[0], norm.weight, norm.bias, norm.eps, **kw)


def _composed(ops, blk, x):
    """A Res1d block as two or three single launches."""
    mid = _unit(ops, blk.conv1, blk.bn1, x, relu=True)
    skip = x if blk.downsample is None else _unit(ops, blk.downsample[0], blk.downsample[1], x)
    return _unit(ops, blk.conv2, blk.bn2, mid, res=skip, relu=blk.act)


@pytest.mark.parametrize("state", AC.STATES, ids=STATE_IDS)
@pytest.mark.parametrize("path,lin", AC.BLOCKS + AC.GROUPS, ids=[p for p, _ in AC.BLOCKS + AC.GROUPS])
def test_fused_launches_over_scale(hip, path, lin, state):
    """ops.res1d_gn(x, b) (lgcn_res1d_gn: identity and k = 1 downsample shortcuts) and ops.res1d_gn(x, b0, second=b1)
    (lgcn_res1d_pair_gn) for the blocks and groups ActorNet has: against the model, and bit for bit the single units."""
    M, ops, L = hip
    rep = Report("%s %s" % (path, AC.case_id(state)))
    sd = AC.state_dict(state)
    for n_act in AC.COUNTS:
        c = AC.block_cpu(path, lin, n_act, state)
        x = dev(AC.block_input(path, lin, n_act, state))
        with torch.no_grad():
            fused_mod = AC.submodule(AC.make_net(sd).cuda(), path)                    # fresh modules: fresh packed images
            unit_mod = AC.submodule(AC.make_net(sd).cuda(), path)
            if path.startswith("groups.") and path.count(".") == 1:
                got = ops.res1d_gn(x, fused_mod[0], second=fused_mod[1])
                units = _composed(ops, unit_mod[1], _composed(ops, unit_mod[0], x))
            else:
                got = ops.res1d_gn(x, fused_mod)
                units = _composed(ops, unit_mod, x)
        rep.check("A=%d out" % n_act, got, c["e_model"], c["truth"], e_ref32=c["e_ref32"])
        same = torch.equal(bits(got), bits(units))
        print(" units-bitwise %s" % same, end="")
        assert same, "%s A=%d: the fused launch differs from its single units by %.3e" % (rep.head, n_act,
                                                                                        float((got - units).abs().max()))
    rep.done()


# ------------------------------------------------------------------ the whole module
def _run_net(M, ops, sd, x, fuse):
    net = AC.make_net(sd).cuda()                                                      # fresh: no packed image is reused
    prev = (M.ActorNet.impl, M.ActorNet.exact, M.ActorNet.fuse_blocks, M.ActorNet.fuse_groups)
    try:
        M.ActorNet.impl, M.ActorNet.exact, M.ActorNet.fuse_blocks, M.ActorNet.fuse_groups = "hip", False, fuse, fuse
        with ops.mma_scope("f16x2"), torch.no_grad():
            assert ops.get_mma() == "f16x2" and ops.get_guard() == "raise" and net._hip_ok(x)
            return net(x)
    finally:
        M.ActorNet.impl, M.ActorNet.exact, M.ActorNet.fuse_blocks, M.ActorNet.fuse_groups = prev


def _whole(hip, draw, state, counts):
    M, ops, L = hip
    rep = Report("net %s %s" % (draw, AC.case_id(state)))
    sd = AC.state_dict(state)
    for n_act in counts:
        c = AC.net_cpu(draw, n_act, state)
        x = dev(AC.scaled_input(draw, n_act, state))
        got, unfused = _run_net(M, ops, sd, x, True), _run_net(M, ops, sd, x, False)
        rep.check("A=%d out" % n_act, got, c["e_model"], c["truth"], e_ref32=c["e_ref32"])
        rep.check("A=%d unfused" % n_act, unfused, c["e_model"], c["truth"], e_ref32=c["e_ref32"])
        assert torch.equal(bits(got), bits(unfused)), "%s A=%d: fuse_blocks / fuse_groups on differs from off by %.3e" % (
            rep.head, n_act, float((got - unfused).abs().max()))
    rep.done()


@pytest.mark.parametrize("draw", AC.DRAWS)
@pytest.mark.parametrize("state", AC.STATES, ids=STATE_IDS)
def test_actor_net_over_scale(hip, state, draw):
    """ActorNet on the f16x2 path against float64, fused launches on and off (bitwise equal), A = 1 and 17."""
    _whole(hip, draw, state, AC.COUNTS)


def test_actor_net_many_actors(hip):
    """The wide state at 333 actors: ragged last workgroups at every level, many workgroups."""
    _whole(hip, "randn", AC.WIDE, (333,))


# ------------------------------------------------------------------ rows past the end
def poisoned(n_words):
    """(buffer, view of its words [PAD, PAD + n_words))"""
    buf = torch.full((n_words + 2 * PAD,), POISON, dtype=torch.int32, device="cuda").view(torch.float32)
    return buf, buf[PAD:PAD + n_words]


def clean_outside(buf, n_words):
    b = bits(buf)
    return bool((b[:PAD] == POISON).all()) and bool((b[PAD + n_words:] == POISON).all())


@pytest.mark.parametrize("n_act", AC.COUNTS)
def test_nothing_is_written_past_the_last_actor(hip, n_act):
    """lgcn_conv1d_gn, lgcn_res1d_gn and lgcn_res1d_pair_gn through the C ABI with `out` inside poisoned pads: every word
    outside [A, lout, c] is untouched (the last workgroup holds 80 / lout - A % (80 / lout) absent actors), and the rows
    inside are the wrapper's."""
    M, ops, L = hip
    lib, ptr, st0 = L.load(), ops._ptr, ("uniform", 0)
    f32 = lambda t: t.detach().float().contiguous()
    for shape in _shapes():
        cin, cout, ks, stride, lin = shape
        for res_mode in _res_modes(shape):
            x, w, stride, gamma, beta, res = AC.unit_case(shape, n_act, st0, res_mode)
            x, w, gamma, beta, res = (dev(t) for t in (x, w, gamma, beta, res))
            n = n_act * _lout(shape) * cout
            buf, out = poisoned(n)
            L.check(lib.lgcn_conv1d_gn(ptr(x), n_act, lin, cin, ptr(ops.conv_packed(w)), cout, ks, stride, ptr(gamma), ptr(beta),
                                       EPS, ptr(res), res_mode, 1, ptr(out), ops._stream()), "lgcn_conv1d_gn")
            torch.cuda.synchronize()
            want = ops.conv1d_gn(x, w, stride, gamma, beta, EPS, res=res, res_up2=res_mode == 2, relu=True)
            assert clean_outside(buf, n), ("lgcn_conv1d_gn wrote outside out", shape, res_mode)
            assert torch.equal(bits(out), bits(want.reshape(-1))), (shape, res_mode)
    net = AC.make_net(AC.state_dict(st0)).cuda()
    for path, lin in AC.BLOCKS + AC.GROUPS:
        mod = AC.submodule(net, path)
        pair = isinstance(mod, torch.nn.Sequential)
        b0 = mod[0] if pair else mod
        x = dev(AC.block_input(path, lin, n_act, st0))
        cin, c, stride = b0.conv1.in_channels, b0.conv1.out_channels, b0.conv1.stride[0]
        lout = (lin + 2 - 3) // stride + 1
        buf, out = poisoned(n_act * lout * c)
        keep = [f32(t) for t in (b0.bn1.weight, b0.bn1.bias, b0.bn2.weight, b0.bn2.bias)]
        ds = b0.downsample
        keep_d = [f32(ds[1].weight), f32(ds[1].bias)] if ds is not None else [None, None]
        first = (ptr(x), n_act, lin, cin, c, stride, ptr(ops.conv_packed(b0.conv1.weight)), ptr(keep[0]), ptr(keep[1]),
                 ptr(ops.conv_packed(b0.conv2.weight)), ptr(keep[2]), ptr(keep[3]),
                 ptr(ops.conv_packed(ds[0].weight)) if ds is not None else None, ptr(keep_d[0]), ptr(keep_d[1]))
        if pair:
            b1 = mod[1]
            keep_q = [f32(t) for t in (b1.bn1.weight, b1.bn1.bias, b1.bn2.weight, b1.bn2.bias)]
            L.check(lib.lgcn_res1d_pair_gn(*first, ptr(ops.conv_packed(b1.conv1.weight)), ptr(keep_q[0]), ptr(keep_q[1]),
                                           ptr(ops.conv_packed(b1.conv2.weight)), ptr(keep_q[2]), ptr(keep_q[3]), EPS, ptr(out),
                                           ops._stream()), "lgcn_res1d_pair_gn")
            want = ops.res1d_gn(x, b0, second=b1)
        else:
            L.check(lib.lgcn_res1d_gn(*first, EPS, ptr(out), ops._stream()), "lgcn_res1d_gn")
            want = ops.res1d_gn(x, b0)
        torch.cuda.synchronize()
        assert clean_outside(buf, n_act * lout * c), ("a fused launch wrote outside out", path)
        assert torch.equal(bits(out), bits(want.reshape(-1))), path


# ------------------------------------------------------------------ the exact units and gn_cl where the squares leave fp32
@pytest.mark.parametrize("ex,ew", WIDE_GRID, ids=["x2^%d-w2^%d" % c for c in WIDE_GRID])
@pytest.mark.parametrize("shape", _shapes(), ids=SHAPE_IDS)
def test_exact_units_over_the_wide_grid(hip, shape, ex, ew):
    """lgcn_conv1d_gn_f32 (ops.conv1d_gn / conv1d_gn_train with exact=True), residual modes 0 / 1 / 2, at the scales that
    broke row_gn: at (2^60, 2^40) the convolution is ~2^100 and the squares of its centred values leave fp32.  Against
    float64 at the floor of split_model.bar (fp32 operands: the model error is 0)."""
    M, ops, L = hip
    rep = Report("exact %d-%d-k%d-s%d-l%d x2^%d w2^%d" % (shape + (ex, ew)))
    for n_act in AC.COUNTS:
        for res_mode in _res_modes(shape):
            x, w, stride, gamma, beta, res = AC.unit_case(shape, n_act, ("uniform", 0), res_mode)
            x, w, relu = AC.p2(x, ex), AC.p2(w, ew), res_mode != 1
            kw = dict(res=res, res_up2=res_mode == 2, relu=relu)
            ref_out, ref_y = S.conv1d_unit(x, w, stride, gamma, beta, "f32", model=False, **kw)
            m_out, m_y = S.conv1d_unit(x, w, stride, gamma, beta, "f32", **kw)
            kw_d = dict(res=dev(res), res_up2=res_mode == 2, relu=relu, exact=True)
            w_d = dev(w)
            out, y = ops.conv1d_gn_train(dev(x), w_d, stride, dev(gamma), dev(beta), EPS, **kw_d)
            plain = ops.conv1d_gn(dev(x), w_d, stride, dev(gamma), dev(beta), EPS, **kw_d)
            tag = "A=%d res%d relu%d " % (n_act, res_mode, relu)
            rep.check(tag + "y", y, None, ref_y, model=m_y)
            rep.check(tag + "out", out, None, ref_out, model=m_out)
            assert S.bar(S.rel_err(m_out, ref_out)) == 1e-6 and S.bar(S.rel_err(m_y, ref_y)) == 1e-6          # the floor
            assert torch.equal(bits(plain), bits(out)), tag
    rep.done()


def _gn_ref(x, gamma, beta, res=None, up2=False, relu=False):
    """float64 GroupNorm(1 group) of x [n, C, L] (+ res | + up2(res)) (+ ReLU) on the fp32 inputs."""
    out = F.group_norm(x.double(), 1, gamma.double(), beta.double(), EPS)
    if res is not None:
        out = out + (F.interpolate(res.double(), scale_factor=2, mode="linear", align_corners=False) if up2 else res.double())
    return out.relu() if relu else out


@pytest.mark.parametrize("e", [70, 100])
def test_gn_cl_where_the_squares_leave_fp32(hip, e):
    """ops.gn_cl (k_gn_cl_vec<10>, <16> and the generic k_gn_cl; NCL and channels-last; with and without the upsampled
    residual) and ops.gn_cl_bwd on inputs x 2^70 and x 2^100, A = 1 and 17: against float64 at the floor of split_model.bar."""
    M, ops, L = hip
    rep = Report("gn_cl x2^%d" % e)
    g = torch.Generator().manual_seed(700 + e)
    rn = lambda *s: torch.randn(*s, generator=g)
    cl = torch.channels_last
    for n in AC.COUNTS:
        for C_, L_, layout, res_mode, relu in ((128, 20, "ncl", 0, True), (128, 20, "ncl", 1, False), (128, 20, "ncl", 2, False),
                                               (128, 20, "cl", 2, False), (128, 20, "cl", 0, True), (128, 28, "ncl", 0, False),
                                               (64, 5, "ncl", 1, True), (32, 10, "cl", 2, True)):
            x = AC.p2(rn(n, C_, L_) + 0.3, e)
            gamma, beta = 1 + 0.1 * rn(C_), 0.1 * rn(C_)
            res = None if res_mode == 0 else rn(n, C_, L_ // 2 if res_mode == 2 else L_)
            want = _gn_ref(x, gamma, beta, res, res_mode == 2, relu).numpy()
            if layout == "cl":
                x_d = dev(x).unsqueeze(2).contiguous(memory_format=cl)
                res_d = None if res is None else dev(res).unsqueeze(2).contiguous(memory_format=cl)
                got = ops.gn_cl(x_d, dev(gamma), dev(beta), EPS, res=res_d, relu=relu, res_up2=res_mode == 2)[:, :, 0, :]
            else:
                got = ops.gn_cl(dev(x), dev(gamma), dev(beta), EPS, res=dev(res), relu=relu, res_up2=res_mode == 2)
            rep.check("A=%d %dx%d %s res%d relu%d out" % (n, C_, L_, layout, res_mode, relu), got, 0.0, want)
        # backward, with and without the ReLU mask of the forward's output
        for relu in (False, True):
            x = AC.p2(rn(n, 128, 20) + 0.3, e)
            gamma, beta, dy = 1 + 0.1 * rn(128), 0.1 * rn(128), rn(n, 128, 20)
            post = ops.gn_cl(dev(x), dev(gamma), dev(beta), EPS, relu=True) if relu else None
            dx, _, dgamma, dbeta = ops.gn_cl_bwd(dev(dy), dev(x), post, dev(gamma), EPS)
            xd, gd, bd = (t.double().requires_grad_(True) for t in (x, gamma, beta))
            ref = F.group_norm(xd, 1, gd, bd, EPS)
            if relu:
                ref = ref * (post.cpu() > 0).double()
            (ref * dy.double()).sum().backward()
            for name, got, want in (("dx", dx, xd.grad), ("dgamma", dgamma, gd.grad), ("dbeta", dbeta, bd.grad)):
                rep.check("A=%d bwd relu%d %s" % (n, relu, name), got, 0.0, want.numpy())
    rep.done()
