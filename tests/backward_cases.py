"""GPU-free half of the backward tests over gradient scale and GroupNorm statistics (test_gpu_backward_scale.py): input
builders, stock-autograd restatements that run in float32 and float64 on any device, and the float64 references that restate
the formulas of include/lgcn.h.  test_backward_cases_host.py checks all of it on the CPU.

Row classes.  One input of n rows interleaves five classes, row i has class i % 5, so that every 32-row tile holds all of them:
  ordinary  randn
  flat      a per-row constant (randn) plus 2^-12 randn: variance about 6e-8, far below eps = 1e-5
  offset    mean 2^10, spread 1
  constant  exactly constant rows, every second one all-zero: xhat = 0 exactly
  dead      randn rows whose output is <= 0 in every channel: dx and the residual gradient are exactly zero
gamma is log-uniform in [2^-8, 2^2] with random signs and a few exact zeros, beta 0.5 randn, so the ReLU masks are mixed.

Saved tensors are set directly (statistics are then what the class says); the parameters keep their gradient through
sub(value, expr) = value + (expr - expr.detach()): the value of the saved tensor, the derivative of the expression.  In any
floating type expr - expr is exactly zero, so the restatement computes on exactly the tensors the kernel reads.

Gradient scale.  A backward is linear in d_out and a power of two commutes with every fp32 rounding while nothing reaches
fp32's subnormals (2^-126) or infinity.  The builders keep inputs O(1) and weights at 0.08, so with k in KS = (-40, -20, +20)
the smallest non-zero gradient entry stays near 1e-18 and the largest near 1e8: homogeneous() is an exact statement there."""
import functools
import math

import torch

C = 128
EPS = 1e-5
F = torch.nn.functional
KS = (-40, -20, 20)
CLASSES = ("ordinary", "flat", "offset", "constant", "dead")
N_ROWS = 130


# ------------------------------------------------------------------ measures
def rel_err(got, ref):
    """max |got - ref| / max |ref| in float64 (ref all zero: max |got|)."""
    got, ref = got.detach().double().cpu(), ref.detach().double().cpu()
    scale = float(ref.abs().max()) if ref.numel() else 0.0
    e = float((got - ref).abs().max()) if ref.numel() else 0.0
    return e / scale if scale > 0 else e


def bar(e_cmp):
    """Twice the comparison path's error against the same reference (both are fp32 chains of the same length that differ in
    summation order), floored at 1e-6, never above 1e-4, the project's parity bar.  A comparison path that did not survive the
    inputs (inf / NaN) says nothing: the ceiling holds."""
    return min(max(2 * e_cmp, 1e-6), 1e-4) if math.isfinite(e_cmp) else 1e-4


def class_errors(got, ref, cls):
    """rel_err per row class: {class name: error} for a row tensor whose first dimension is indexed by cls."""
    out = {}
    for c, name in enumerate(CLASSES):
        sel = cls == c
        if bool(sel.any()):
            out[name] = rel_err(got.detach().cpu()[sel], ref.detach().cpu()[sel])
    return out


def scaled_bits_equal(g_k, g_0, k):
    """g_k == 2^k g_0 bit for bit (None only with None)."""
    if g_k is None or g_0 is None:
        return g_k is None and g_0 is None
    want = g_0 * (2.0 ** k)
    return g_k.shape == want.shape and torch.equal(g_k.contiguous().view(torch.int32), want.contiguous().view(torch.int32))


def grads_at(outs, leaves, d_outs, k):
    """Gradients of `outs` (tensors of one retained forward) with respect to the dict `leaves` for 2^k d_outs."""
    gs = torch.autograd.grad(list(outs), list(leaves.values()), [d * (2.0 ** k) for d in d_outs], retain_graph=True,
                             allow_unused=True)
    return dict(zip(leaves, gs))


def homogeneous(outs, leaves, d_outs, ks=KS):
    """[(k, leaf name)] of every gradient that is not 2^k times the gradient at k = 0 bit for bit, and the gradients at 0."""
    base = grads_at(outs, leaves, d_outs, 0)
    bad = []
    for k in ks:
        g = grads_at(outs, leaves, d_outs, k)
        bad += [(k, name) for name in leaves if not scaled_bits_equal(g[name], base[name], k)]
    return bad, base


# ------------------------------------------------------------------ the formulas of include/lgcn.h in float64
def hat64(v, eps=EPS):
    mu = v.mean(1, keepdim=True)
    rstd = 1.0 / torch.sqrt(((v - mu) ** 2).mean(1, keepdim=True) + eps)
    return (v - mu) * rstd, rstd


def gn_bwd64(g, xh, rstd, gamma):
    d = g * gamma
    return rstd * (d - d.mean(1, keepdim=True) - xh * (d * xh).mean(1, keepdim=True))


def sub(value, expr):
    """`value` with the derivative of `expr` (expr - expr.detach() is exactly zero)."""
    return value + (expr - expr.detach())


# ------------------------------------------------------------------ inputs
def row_class(n):
    return torch.arange(n) % len(CLASSES)


def class_rows(n, seed, width=C):
    """[n, width] fp32 rows, row i of class i % 5 (the dead rows are ordinary here: their output makes them dead)."""
    g = torch.Generator().manual_seed(seed)
    rnd = lambda *s: torch.randn(*s, generator=g)
    cls = row_class(n)
    x = rnd(n, width)
    flat = rnd(n, 1) + 2.0 ** -12 * rnd(n, width)
    offset = 2.0 ** 10 + rnd(n, width)
    const = (rnd(n, 1) * ((torch.arange(n) // len(CLASSES)) % 2 == 0).float().unsqueeze(1)).expand(n, width)
    for c, t in ((1, flat), (2, offset), (3, const)):
        x = torch.where((cls == c).unsqueeze(1), t, x)
    return x.contiguous()


def gamma_beta(seed, width=C):
    """gamma log-uniform in [2^-8, 2^2] with random signs and exact zeros at channels 5 and width - 3; beta = 0.5 randn."""
    g = torch.Generator().manual_seed(seed)
    gamma = 2.0 ** (torch.rand(width, generator=g) * 10 - 8) * (torch.randint(0, 2, (width,), generator=g) * 2 - 1).float()
    gamma[5] = 0.0
    gamma[width - 3] = 0.0
    return gamma, 0.5 * torch.randn(width, generator=g)


def gn32(x, gamma, beta, eps=EPS):
    """GroupNorm(1 group) of the rows of x ([n, ...]: statistics over everything but the first dimension; gamma / beta on the
    last one) in x's type, two-pass: the forward that builds the saved outputs of a case."""
    flat = x.reshape(x.shape[0], -1)
    mu = flat.mean(1, keepdim=True)
    var = ((flat - mu) ** 2).mean(1, keepdim=True)
    return (((flat - mu) / torch.sqrt(var + eps)).reshape(x.shape)) * gamma + beta


def gn_saved(x, gamma, beta):
    """The GroupNorm that builds a case's saved outputs: gn32 in float64, rounded to fp32 (rows of magnitude 2^70 included)."""
    return gn32(x.double(), gamma.double(), beta.double()).float()


def kill_dead(out, cls):
    """The output with the rows of class dead set to zero (post <= 0 in every channel)."""
    out = out.clone()
    out[cls == CLASSES.index("dead")] = 0.0
    return out


@functools.lru_cache(maxsize=None)
def gn_case(n=N_ROWS, seed=0, huge=False):
    """lgcn_gn_bwd: x (pre-norm rows), gamma, res, post = ReLU(GN(x) + res) with dead rows, dy.  huge: x of magnitude 2^70."""
    g = torch.Generator().manual_seed(7000 + seed)
    x = class_rows(n, 7100 + seed)
    if huge:
        x = (torch.randn(n, C, generator=g) * 2.0 ** 70).contiguous()
    gamma, beta = gamma_beta(7200 + seed)
    res = torch.randn(n, C, generator=g)
    cls = row_class(n)
    post = kill_dead(torch.relu(gn_saved(x, gamma, beta) + res), cls)
    return dict(x=x, gamma=gamma, beta=beta, res=res, post=post, dy=torch.randn(n, C, generator=g), cls=cls)


def gn_stock(case, dtype, device="cpu"):
    """Stock autograd of post = (GN(x) + res) * (post > 0): {"dx", "g", "dgamma", "dbeta"}."""
    to = lambda t: t.to(device=device, dtype=dtype)
    x, gamma, beta, res = (to(case[k]).requires_grad_(True) for k in ("x", "gamma", "beta", "res"))
    y = (F.group_norm(x, 1, gamma, beta, EPS) + res) * to(case["post"] > 0)
    y.backward(to(case["dy"]))
    return dict(dx=x.grad, g=res.grad, dgamma=gamma.grad, dbeta=beta.grad)


def gn_reference64(case):
    x, gamma, dy = (case[k].double() for k in ("x", "gamma", "dy"))
    g = dy * (case["post"] > 0).double()
    xh, rstd = hat64(x)
    return dict(dx=gn_bwd64(g, xh, rstd, gamma), g=g, dgamma=(g * xh).sum(0), dbeta=g.sum(0))


# gn, relu, res; K: columns of each weight; rels: (source, weight, first column) -- the blocks of test_gpu_rowblock_train.SHAPES
# that have a GroupNorm
RB_SHAPES = {
    "a": dict(gn=True, relu=True, res=False, K=[128], rels=[(0, 0, 0)]),
    "b": dict(gn=True, relu=True, res=True, K=[128], rels=[(0, 0, 0)]),
    "d": dict(gn=True, relu=True, res=False, K=[128, 128], rels=[(0, 0, 0), (1, 1, 0)]),
    "g": dict(gn=True, relu=False, res=False, K=[132], rels=[(0, 0, 0)]),
}


@functools.lru_cache(maxsize=None)
def rowblock_case(shape, wscale=1.0, n=N_ROWS, huge=False):
    """lgcn_rowblock_bwd on a block of RB_SHAPES: sources, weights at wscale * 0.08, the saved pre (row classes; huge: 2^70
    randn), gamma, beta, res, out (None without a ReLU) and d_out."""
    s = RB_SHAPES[shape]
    g = torch.Generator().manual_seed(8000 + ord(shape))
    rnd = lambda *sz: torch.randn(*sz, generator=g)
    cls = row_class(n)
    d = dict(srcs=[rnd(n, C) for _ in range(2)], ws=[rnd(C, k) * (0.08 * wscale) for k in s["K"]], res=rnd(n, C), d_out=rnd(n, C),
             cls=cls, shape=shape)
    d["gamma"], d["beta"] = gamma_beta(8100 + ord(shape))
    d["pre"] = (rnd(n, C) * 2.0 ** 70).contiguous() if huge else class_rows(n, 8200 + ord(shape))
    y = gn_saved(d["pre"], d["gamma"], d["beta"])
    if s["res"]:
        y = y + d["res"]
    d["out"] = kill_dead(torch.relu(y), cls) if s["relu"] else None
    return d


def rowblock_stock(case, dtype, device="cpu"):
    """Stock autograd of the block with the saved pre substituted for its value: {"d src<i>", "d w<k>", "d gamma", "d beta",
    "d res"} as test_gpu_rowblock_train names them."""
    s = RB_SHAPES[case["shape"]]
    to = lambda t: t.to(device=device, dtype=dtype)
    n_src = 1 + max(r[0] for r in s["rels"])
    srcs = [to(t).requires_grad_(True) for t in case["srcs"][:n_src]]
    ws = [to(t).requires_grad_(True) for t in case["ws"]]
    gamma, beta, res = (to(case[k]).requires_grad_(True) for k in ("gamma", "beta", "res"))
    lin = sum(srcs[si] @ ws[wi][:, c0:c0 + C].t() for si, wi, c0 in s["rels"])
    y = F.group_norm(sub(to(case["pre"]), lin), 1, gamma, beta, EPS)
    if s["res"]:
        y = y + res
    if s["relu"]:
        y = y * to(case["out"] > 0)
    y.backward(to(case["d_out"]))
    r = {"d src%d" % i: t.grad for i, t in enumerate(srcs)}
    r.update({"d w%d" % k: t.grad for k, t in enumerate(ws)})
    r["d gamma"], r["d beta"] = gamma.grad, beta.grad
    if s["res"]:
        r["d res"] = res.grad
    return r


def rowblock_reference64(case):
    """The formulas of include/lgcn.h (lgcn_rowblock_bwd) in float64 on the saved tensors."""
    s = RB_SHAPES[case["shape"]]
    srcs, ws = [t.double() for t in case["srcs"]], [t.double() for t in case["ws"]]
    g = case["d_out"].double()
    if s["relu"]:
        g = g * (case["out"] > 0).double()
    r = {}
    if s["res"]:
        r["d res"] = g
    xh, rstd = hat64(case["pre"].double())
    r["d gamma"], r["d beta"] = (g * xh).sum(0), g.sum(0)
    dT = gn_bwd64(g, xh, rstd, case["gamma"].double())
    for k, w in enumerate(ws):
        r["d w%d" % k] = torch.zeros_like(w)
    for si, wi, c0 in s["rels"]:
        r["d src%d" % si] = dT @ ws[wi][:, c0:c0 + C]
        r["d w%d" % wi][:, c0:c0 + C] += dT.t() @ srcs[si]
    return r


@functools.lru_cache(maxsize=None)
def laneconv_case(ident1, wscale=1.0, n=N_ROWS, huge=False):
    """lgcn_laneconv_bwd: x, w1, w2 at wscale * 0.08, both norms, the saved T and Z (row classes, two draws), Y = ReLU(GN1(T)),
    out = ReLU(GN2(Z) + x) with dead rows, d_out.  huge: T of the even rows and Z of the odd rows are 2^70 randn -- never both in
    one row, whose dT ~ rstd1 rstd2 = 2^-140 would leave fp32 on its own."""
    g = torch.Generator().manual_seed(9000 + int(ident1))
    rnd = lambda *sz: torch.randn(*sz, generator=g)
    cls = row_class(n)
    d = dict(x=rnd(n, C), w1=rnd(C, C) * (0.08 * wscale), w2=rnd(C, C) * (0.08 * wscale), d_out=rnd(n, C), cls=cls, ident1=ident1)
    d["g1"], d["b1"] = gamma_beta(9100)
    d["g2"], d["b2"] = gamma_beta(9200)
    d["T"], d["Z"] = class_rows(n, 9300), class_rows(n, 9400)
    if huge:
        even = (torch.arange(n) % 2 == 0).unsqueeze(1)
        d["T"] = torch.where(even, rnd(n, C) * 2.0 ** 70, d["T"]).contiguous()
        d["Z"] = torch.where(~even, rnd(n, C) * 2.0 ** 70, d["Z"]).contiguous()
    d["Y"] = torch.relu(gn_saved(d["T"], d["g1"], d["b1"]))
    d["out"] = kill_dead(torch.relu(gn_saved(d["Z"], d["g2"], d["b2"]) + d["x"]), cls)
    return d


def laneconv_stock(case, dtype, device="cpu"):
    """Stock autograd of out = (GN2(Z) + x) * (out > 0), Z <- Y W2^T, Y <- GN1(T) * (Y > 0), T <- x W1^T (ident1) with the
    saved tensors substituted for their values: the outputs of ops.laneconv_bwd by name."""
    to = lambda t: t.to(device=device, dtype=dtype)
    p = {k: to(case[k]).requires_grad_(True) for k in ("x", "w1", "w2", "g1", "b1", "g2", "b2")}
    T = to(case["T"]).requires_grad_(True)
    r_ = to(case["x"]).requires_grad_(True)          # the residual as its own leaf without ident1: its gradient is g2
    t = sub(T, p["x"] @ p["w1"].t()) if case["ident1"] else T
    y = sub(to(case["Y"]), F.group_norm(t, 1, p["g1"], p["b1"], EPS) * to(case["Y"] > 0))
    z = sub(to(case["Z"]), y @ p["w2"].t())
    o = (F.group_norm(z, 1, p["g2"], p["b2"], EPS) + (p["x"] if case["ident1"] else r_)) * to(case["out"] > 0)
    o.backward(to(case["d_out"]))
    r = dict(d_w2=p["w2"].grad, d_g2=p["g2"].grad, d_b2=p["b2"].grad, d_g1=p["g1"].grad, d_b1=p["b1"].grad)
    if case["ident1"]:
        r.update(dX=p["x"].grad, d_w1=p["w1"].grad)
    else:
        r.update(dT=T.grad, g2=r_.grad)
    return r


def laneconv_reference64(case):
    """The formulas of include/lgcn.h (lgcn_laneconv_bwd) in float64 on the saved tensors."""
    T, Y, Z, out = (case[k].double() for k in ("T", "Y", "Z", "out"))
    d_out, w2 = case["d_out"].double(), case["w2"].double()
    r = {}
    g2 = d_out * (out > 0)
    zh, rstd2 = hat64(Z)
    r["d_g2"], r["d_b2"] = (g2 * zh).sum(0), g2.sum(0)
    dZ = gn_bwd64(g2, zh, rstd2, case["g2"].double())
    r["d_w2"] = dZ.t() @ Y
    g1 = (dZ @ w2) * (Y > 0)
    th, rstd1 = hat64(T)
    r["d_g1"], r["d_b1"] = (g1 * th).sum(0), g1.sum(0)
    dT = gn_bwd64(g1, th, rstd1, case["g1"].double())
    if case["ident1"]:
        r["dX"] = dT @ case["w1"].double() + g2
        r["d_w1"] = dT.t() @ case["x"].double()
    else:
        r["dT"], r["g2"] = dT, g2
    return r


@functools.lru_cache(maxsize=None)
def gn_cl_case(n, c, l):
    """lgcn_gn_cl_bwd on [n, C, L] (one group over (C, L)): item i of class i % 5."""
    g = torch.Generator().manual_seed(10000 + n + c)
    cls = row_class(n)
    x = class_rows(n, 10100 + n, c * l).reshape(n, c, l).contiguous()
    gamma, beta = gamma_beta(10200 + c, c)
    res = torch.randn(n, c, l, generator=g)
    flat = x.reshape(n, -1)
    mu = flat.mean(1, keepdim=True)
    xh = ((flat - mu) / torch.sqrt(((flat - mu) ** 2).mean(1, keepdim=True) + EPS)).reshape(n, c, l)
    post = kill_dead(torch.relu(xh * gamma[:, None] + beta[:, None] + res), cls)
    return dict(x=x, gamma=gamma, beta=beta, res=res, post=post, dy=torch.randn(n, c, l, generator=g), cls=cls)


def gn_cl_stock(case, dtype, device="cpu"):
    to = lambda t: t.to(device=device, dtype=dtype)
    x, gamma, beta, res = (to(case[k]).requires_grad_(True) for k in ("x", "gamma", "beta", "res"))
    y = (F.group_norm(x, 1, gamma, beta, EPS) + res) * to(case["post"] > 0)
    y.backward(to(case["dy"]))
    return dict(dx=x.grad, g=res.grad, dgamma=gamma.grad, dbeta=beta.grad)


def gn_cl_reference64(case):
    """GroupNorm backward over (C, L) per item in float64 (the formula of lgcn_gn_bwd with the channel axis second)."""
    x, dy = case["x"].double(), case["dy"].double()
    n, c, l = x.shape
    g = dy * (case["post"] > 0).double()
    xh, rstd = hat64(x.reshape(n, -1))
    d = (g * case["gamma"].double()[:, None]).reshape(n, -1)
    dx = rstd * (d - d.mean(1, keepdim=True) - xh * (d * xh).mean(1, keepdim=True))
    xh = xh.reshape(n, c, l)
    return dict(dx=dx.reshape(n, c, l), g=g, dgamma=(g * xh).sum((0, 2)), dbeta=g.sum((0, 2)))


# (cin, cout, kernel, stride, residual mode: 0 none / 1 same length / 2 upsampled x2): ActorNet's first unit, a strided one and
# the lateral 1x1 with the top-down residual
CONV_UNITS = {"3-32-k3-s1": (3, 32, 3, 1, 0), "32-64-k3-s2": (32, 64, 3, 2, 1), "128-128-k1-up2": (128, 128, 1, 1, 2)}
CONV_A, CONV_L = 5, 20


@functools.lru_cache(maxsize=None)
def conv_case(unit):
    """lgcn_conv1d_gn_bwd, channels-last: x [A, L, Cin], weight [Cout, Cin, k] at 0.08-like scale, the saved pre-norm y
    [A, Lout, Cout] (actor a of class a), gamma, beta, res, out with a dead actor, d_out."""
    cin, cout, ks, stride, res_mode = CONV_UNITS[unit]
    g = torch.Generator().manual_seed(11000 + cin + cout)
    rnd = lambda *sz: torch.randn(*sz, generator=g)
    lout = (CONV_L + 2 * ((ks - 1) // 2) - ks) // stride + 1
    cls = row_class(CONV_A)
    d = dict(x=rnd(CONV_A, CONV_L, cin), w=rnd(cout, cin, ks) * (1.0 / (cin * ks) ** 0.5), d_out=rnd(CONV_A, lout, cout), cls=cls,
             unit=unit, res=rnd(CONV_A, lout // 2 if res_mode == 2 else lout, cout) if res_mode else None)
    d["gamma"], d["beta"] = gamma_beta(11100 + cout, cout)
    d["y"] = class_rows(CONV_A, 11200 + cout, lout * cout).reshape(CONV_A, lout, cout).contiguous()
    o = gn32(d["y"], d["gamma"], d["beta"])
    if res_mode:
        o = o + (up2(d["res"].transpose(1, 2)).transpose(1, 2) if res_mode == 2 else d["res"])
    d["out"] = kill_dead(torch.relu(o), cls)
    return d


def up2(x):
    """x2 linear upsampling of [A, C, L], align_corners = False (the FPN top-down step)."""
    return F.interpolate(x, scale_factor=2, mode="linear", align_corners=False)


def conv_stock(case, dtype, device="cpu"):
    """Stock autograd of the unit in NCL with the saved y substituted: {"dx", "dw", "dgamma", "dbeta", "dres"}, channels-last."""
    cin, cout, ks, stride, res_mode = CONV_UNITS[case["unit"]]
    to = lambda t: t.to(device=device, dtype=dtype)
    x = to(case["x"]).transpose(1, 2).contiguous().requires_grad_(True)
    w, gamma, beta = (to(case[k]).requires_grad_(True) for k in ("w", "gamma", "beta"))
    y = sub(to(case["y"]).transpose(1, 2), F.conv1d(x, w, stride=stride, padding=(ks - 1) // 2))
    o = F.group_norm(y, 1, gamma, beta, EPS)
    res = None
    if res_mode:
        res = to(case["res"]).transpose(1, 2).contiguous().requires_grad_(True)
        o = o + (up2(res) if res_mode == 2 else res)
    o = o * to(case["out"] > 0).transpose(1, 2)
    o.backward(to(case["d_out"]).transpose(1, 2))
    return dict(dx=x.grad.transpose(1, 2), dw=w.grad, dgamma=gamma.grad, dbeta=beta.grad,
                dres=None if res is None else res.grad.transpose(1, 2))


def conv_reference64(case):
    """The unit's backward in float64 from the formulas: the GroupNorm backward over (Lout, Cout) per actor on the saved y,
    then the transposed convolution / the correlation with x written as sums over taps."""
    cin, cout, ks, stride, res_mode = CONV_UNITS[case["unit"]]
    x, w, y, d_out = (case[k].double() for k in ("x", "w", "y", "d_out"))
    A, lout = y.shape[0], y.shape[1]
    g = d_out * (case["out"] > 0).double()
    xh, rstd = hat64(y.reshape(A, -1))
    d = (g * case["gamma"].double()).reshape(A, -1)
    dy = (rstd * (d - d.mean(1, keepdim=True) - xh * (d * xh).mean(1, keepdim=True))).reshape(A, lout, cout)
    xh = xh.reshape(A, lout, cout)
    r = dict(dgamma=(g * xh).sum((0, 1)), dbeta=g.sum((0, 1)), dx=torch.zeros_like(x), dw=torch.zeros_like(w), dres=None)
    pad = (ks - 1) // 2
    for lo in range(lout):
        for t in range(ks):
            li = lo * stride + t - pad
            if 0 <= li < x.shape[1]:
                r["dx"][:, li] += dy[:, lo] @ w[:, :, t]
                r["dw"][:, :, t] += dy[:, lo].t() @ x[:, li]
    if res_mode == 1:
        r["dres"] = g
    elif res_mode == 2:         # the transpose of up2: out[2i] = 0.25 r[i-1] + 0.75 r[i], out[2i+1] = 0.75 r[i] + 0.25 r[i+1], clamped
        half = lout // 2
        dres = torch.zeros(A, half, cout, dtype=torch.float64)
        for i in range(half):
            dres[:, max(i - 1, 0)] += 0.25 * g[:, 2 * i]
            dres[:, i] += 0.75 * g[:, 2 * i] + 0.75 * g[:, 2 * i + 1]
            dres[:, min(i + 1, half - 1)] += 0.25 * g[:, 2 * i + 1]
        r["dres"] = dres
    return r


# ------------------------------------------------------------------ the stock block of the homogeneity claim
def stock_block(x, w, gamma, beta, res):
    """ReLU(GN(x W^T) + res) on stock ATen ops."""
    return torch.relu(F.group_norm(x @ w.t(), 1, gamma, beta, EPS) + res)
