"""Float64 model of the split-precision operand formats (csrc/lgcn_mma_bf.hpp: Fmt<>, split_store) and float64
restatements of the forward kernels built on them.

Test infrastructure, like lc_plan_ref.py.  A kernel in a split mode does not compute the fp32 product: it rounds both
operands to 16-bit planes and multiplies a subset of the plane pairs.  The model does exactly that and nothing else --
RNE planes with the residual taken in fp32, subnormals kept, the products of Fmt<>'s PA / PB lists, everything behind
the rounding in float64 -- so model - fp64 is the error the FORMAT commits on a given input, and a kernel that stays
within a small factor of it is implementing its format and no worse.  Every restatement takes model=False and then
returns the exact float64 value of the same formulas on the fp32 inputs (the reference).

Inputs are numpy arrays or torch tensors; outputs are float64 numpy arrays."""
import numpy as np

C = 128
EPS = 1e-5

# mode -> (16-bit type, planes, PA, PB): the product list of Fmt<F> (A plane, B plane)
FORMATS = {
    "bf16x3": ("bf16", 3, (2, 0, 1, 1, 0, 0), (0, 2, 1, 0, 1, 0)),
    "f16x2": ("f16", 2, (1, 0, 0), (0, 1, 0)),
    "bf16": ("bf16", 1, (0,), (0,)),
}
MODES = ("f32", "bf16x3", "f16x2", "bf16")


def arr(a, dtype=None):
    if hasattr(a, "detach"):
        a = a.detach().cpu().numpy()
    a = np.asarray(a)
    return a if dtype is None else a.astype(dtype)


def f32(a):
    """Round to fp32 (where a kernel holds a value in a float register)."""
    return arr(a).astype(np.float32)


def round16(v, kind):
    """fp32 -> fp16 / bf16 -> fp32, round to nearest even, subnormals kept, overflow to inf (v_cvt_pk_*_f32)."""
    v = np.ascontiguousarray(v, np.float32)
    if kind == "f16":
        with np.errstate(over="ignore"):
            return v.astype(np.float16).astype(np.float32)
    u = v.view(np.uint32).astype(np.uint64)
    r = ((u + 0x7FFF + ((u >> 16) & 1)) >> 16) << 16
    out = (r & 0xFFFFFFFF).astype(np.uint32).view(np.float32)
    return np.where(np.isnan(v), v, out)


def planes(a, mode):
    """The planes of an fp32 array as split_store forms them: plane p = round16(residual), residual -= plane in fp32."""
    kind, n_planes = FORMATS[mode][:2]
    v = f32(a).copy()
    out = []
    for p in range(n_planes):
        q = round16(v, kind)
        out.append(q.astype(np.float64))
        if p + 1 < n_planes:
            with np.errstate(invalid="ignore"):
                v = (v - q).astype(np.float32)
    return out


def mm(a, w, mode):
    """a [n, K] x w [c, K]^T -> [n, c]: the mode's plane products summed in float64; "f32": the float64 product."""
    if mode == "f32":
        return arr(a, np.float32).astype(np.float64) @ arr(w, np.float32).astype(np.float64).T
    pa, pb = planes(a, mode), planes(w, mode)
    out = 0.0
    with np.errstate(invalid="ignore"):
        for i, j in zip(*FORMATS[mode][2:]):
            out = out + pa[i] @ pb[j].T
    return out


def rel_err(got, ref):
    got, ref = arr(got, np.float64), arr(ref, np.float64)
    return float(np.abs(got - ref).max() / np.abs(ref).max())


def gn(x, gamma, beta, eps=EPS):
    """GroupNorm(1, C) over the last axis (row_gn: biased variance)."""
    mu = x.mean(-1, keepdims=True)
    var = ((x - mu) ** 2).mean(-1, keepdims=True)
    return (x - mu) / np.sqrt(var + eps) * arr(gamma, np.float64) + arr(beta, np.float64)


def gather_sum(x, edges, n_rows, model=True):
    """A[n] = sum_{e: u[e] = n} x[v[e]], sources in ascending order of v, duplicates kept (LGCN_REL_CSR).  The kernels
    form the sum in fp32 and split the sum; model=False: the float64 sum."""
    if edges is None:
        return arr(x, np.float32 if model else None)[:n_rows]
    u, v = (arr(t, np.int64) for t in edges)
    order = np.lexsort((v, u))
    u, v = u[order], v[order]
    dt = np.float32 if model else np.float64
    out = np.zeros((n_rows, arr(x).shape[1]), dt)
    np.add.at(out, u, arr(x, np.float32 if model else None).astype(dt)[v])       # unbuffered: one addition per edge, in order
    return out


def _mm(a, w, mode, model):
    if model:
        return mm(f32(a), w, mode)
    return arr(a, np.float64) @ arr(w, np.float32).astype(np.float64).T


def _hold(a, model):
    """A value the kernel holds in fp32 before it splits it again."""
    return f32(a) if model else a


def row_block(n_rows, rels, mode, gn1=None, relu1=False, w2=None, gn2=None, res=None, relu2=False, eps=EPS, model=True):
    """lgcn_agg_mlp.  rels: (x, w [128, 128], edges (u, v) | None = IDENT).  Returns dict(pre = T, mid = Y, out):
    T = sum_r gather_r(x_r) w_r^T;  Y = act(GN1(T));  out = act(GN2(Y w2^T) + res) (one stage without w2: out = Y + res)."""
    T = 0.0
    for x, w, edges in rels:
        T = T + _mm(gather_sum(x, edges, n_rows, model), w, mode, model)
    y = gn(T, *gn1, eps) if gn1 is not None else T
    if w2 is None and res is not None:
        y = y + arr(res, np.float64)
    if relu1:
        y = np.maximum(y, 0.0)
    if w2 is None:
        return dict(pre=T, mid=y, out=y)
    z = _mm(_hold(y, model), w2, mode, model)
    if gn2 is not None:
        z = gn(z, *gn2, eps)
    if res is not None:
        z = z + arr(res, np.float64)
    if relu2:
        z = np.maximum(z, 0.0)
    return dict(pre=T, mid=y, out=z)


def lane_conv(x, units, gn1, w2, gn2, mode, eps=EPS, model=True):
    """One LaneConv layer (lgcn_laneconv_fwd == lgcn_agg_mlp with every flag): units = (w, edges | None for ctr)."""
    n = arr(x).shape[0]
    return row_block(n, [(x, w, e) for w, e in units], mode, gn1=gn1, relu1=True, w2=w2, gn2=gn2, res=x, relu2=True,
                     eps=eps, model=model)["out"]


def lin2_relu(xy, w1, b1, model):
    """ReLU(w1 xy + b1) of an [n, 2] input, held in fp32."""
    h = arr(xy, np.float64) @ arr(w1, np.float32).astype(np.float64).T + arr(b1, np.float64)
    return _hold(np.maximum(h, 0.0), model)


def att_pairs(agt_ctrs, ctx_ctrs, hi, wi, wd0, bd0, w_d2, gn_d, w_c0e, U, V, gn_c, mode, eps=EPS, model=True, exact_d=False):
    """m [P, 128] of lgcn_att_pairs / _ws / _wi (include/lgcn.h); w_c0e = columns 0:128 of ctx.0's weight.  exact_d: the
    centre offsets in float64 (what a float64 run of the reference forms) instead of the kernels' fp32 difference."""
    hi, wi = arr(hi, np.int64), arr(wi, np.int64)
    dt = np.float64 if exact_d else np.float32
    d = arr(agt_ctrs, np.float32).astype(dt)[hi] - arr(ctx_ctrs, np.float32).astype(dt)[wi]      # default: fp32, as the kernels form it
    h1 = lin2_relu(d, wd0, bd0, model)
    e = np.maximum(gn(_mm(h1, w_d2, mode, model), *gn_d, eps), 0.0)
    c = _mm(_hold(e, model), w_c0e, mode, model) + arr(U, np.float64)[hi] + arr(V, np.float64)[wi]
    return np.maximum(gn(c, *gn_c, eps), 0.0)


def mapnet_input(ctrs, feats, wa1, ba1, wa2, gn_a, ws1, bs1, ws2, gn_s, mode, eps=EPS, model=True):
    """lgcn_mapnet_input: ReLU(GN_a(W_a2 ReLU(W_a1 ctr + b_a1)) + GN_s(W_s2 ReLU(W_s1 seg + b_s1)))."""
    a = gn(_mm(lin2_relu(ctrs, wa1, ba1, model), wa2, mode, model), *gn_a, eps)
    s = gn(_mm(lin2_relu(feats, ws1, bs1, model), ws2, mode, model), *gn_s, eps)
    return np.maximum(a + s, 0.0)


def seg_sum(m, hi, n_rows, model=True):
    """S[t] = sum_{p: hi[p] = t} m[p] (LGCN_REL_RANGE / RANGE16): the float64 sum of the rows as held, then held itself.
    The kernels add in fp32 in an order that depends on the pair kernel (whole segments, or 16-aligned pieces first)."""
    out = np.zeros((n_rows, arr(m).shape[1]))
    np.add.at(out, arr(hi, np.int64), arr(_hold(m, model), np.float64))
    return _hold(out, model)


HOT_CFG = {"actor2map_dist": 7.0, "map2actor_dist": 6.0, "actor2actor_dist": 100.0, "num_scales": 6}
STAGES = ("map_net", "a2m", "m2m", "m2a", "a2a")


def hot_path(graph, actors, actor_ctrs, sd, mode, model=True, cfg=None):
    """MapNet -> A2M -> M2M -> M2A -> A2A (oracle.hot_path's arguments: the gathered graph, ActorNet's output rows, the
    per-scene actor centres, a state dict) as the launches of lanegcn.py compose them: lgcn_mapnet_input, 4 LaneConv
    layers, A2M.meta_kw (128 columns through the matrix cores, the four meta columns w4 beside them), per Att layer
    u_kw / v_kw (U per target row, V per context row), the pair stage and pairs_tail (segment sum, agt + ctx.1, norm,
    linear, residual), 4 more LaneConv layers, M2A, A2A.  Every GEMM over a 128-column block goes through mm(); a value
    one kernel hands to the next, or one GEMM of a kernel to the next, is rounded to fp32 (_hold).  The [*, 2] Linears,
    w4, GroupNorm, U[hi] + V[wi], the segment sum and the residuals are float64 behind their fp32 inputs.  Pairs come
    from oracle.pair_search (fp32, as lgcn_pairs_build).  model=False: the exact float64 value of the reference's
    formulas (centre offsets in float64 too).  Returns {stage: float64 [rows, 128]}."""
    from oracle import lanegcn_oracle as O
    cfg = cfg or HOT_CFG
    W = lambda name: arr(sd[name], np.float32)
    G = lambda name: (W(name + ".weight"), W(name + ".bias"))
    node_ctrs = graph["ctrs"]                                            # per-scene torch tensors, as the oracle takes them
    cat = lambda cs: np.concatenate([arr(c, np.float32) for c in cs], 0)
    nodes_c, actors_c = cat(node_ctrs), cat(actor_ctrs)
    keys = [(k1, i) for i in range(cfg["num_scales"]) for k1 in ("pre", "suc")]
    edges = [("%s%d" % k, (graph[k[0]][k[1]]["u"], graph[k[0]][k[1]]["v"])) for k in keys]
    edges += [(k, (graph[k]["u"], graph[k]["v"])) for k in ("left", "right")]
    edges = [(k, e) for k, e in edges if len(e[0]) > 0]

    def fuse(x, prefix):
        for i in range(4):
            units = [(W("%s.ctr.%d.weight" % (prefix, i)), None)] + [(W("%s.%s.%d.weight" % (prefix, k, i)), e) for k, e in edges]
            c2 = "%s.ctr2.%d" % (prefix, i)
            x = _hold(lane_conv(x, units, G("%s.norm.%d" % (prefix, i)), W(c2 + ".linear.weight"), G(c2 + ".norm"), mode,
                                model=model), model)
        return x

    def att(agts, agt_c, ctx, ctx_c, hi, wi, name):
        wc0 = W(name + ".ctx.0.linear.weight")
        q = np.maximum(gn(_mm(agts, W(name + ".query.linear.weight"), mode, model), *G(name + ".query.norm")), 0.0)
        U = _hold(_mm(_hold(q, model), wc0[:, C:2 * C], mode, model), model)
        V = _hold(_mm(ctx, wc0[:, 2 * C:], mode, model), model)
        m = att_pairs(agt_c, ctx_c, hi, wi, W(name + ".dist.0.weight"), W(name + ".dist.0.bias"), W(name + ".dist.2.linear.weight"),
                      G(name + ".dist.2.norm"), wc0[:, :C], U, V, G(name + ".ctx.0.norm"), mode, model=model, exact_d=not model)
        T = agts.shape[0]
        rels = [(agts, W(name + ".agt.weight"), None), (seg_sum(m, hi, T, model), W(name + ".ctx.1.weight"), None)]
        return _hold(row_block(T, rels, mode, gn1=G(name + ".norm"), relu1=True, w2=W(name + ".linear.linear.weight"),
                               gn2=G(name + ".linear.norm"), res=agts, relu2=True, model=model)["out"], model)

    def block(agts, agt_cs, agt_c, ctx, ctx_cs, ctx_c, th, prefix):
        hi, wi = O.pair_search(agt_cs, ctx_cs, th)
        for i in range(2):
            agts = att(agts, agt_c, agts if ctx is None else ctx, ctx_c, hi, wi, "%s.att.%d" % (prefix, i))
        return agts

    out = {}
    a, s = "map_net.input", "map_net.seg"
    x = mapnet_input(nodes_c, arr(graph["feats"], np.float32), W(a + ".0.weight"), W(a + ".0.bias"), W(a + ".2.linear.weight"),
                     G(a + ".2.norm"), W(s + ".0.weight"), W(s + ".0.bias"), W(s + ".2.linear.weight"), G(s + ".2.norm"), mode,
                     model=model)
    out["map_net"] = x = fuse(_hold(x, model), "map_net.fuse")
    wm = W("a2m.meta.linear.weight")
    meta4 = np.concatenate([arr(graph["turn"], np.float64), arr(graph["control"], np.float64)[:, None],
                            arr(graph["intersect"], np.float64)[:, None]], 1)
    x = _mm(x, wm[:, :C], mode, model) + meta4 @ wm[:, C:].astype(np.float64).T
    x = _hold(np.maximum(gn(x, *G("a2m.meta.norm")), 0.0), model)
    acts = arr(actors, np.float32)
    out["a2m"] = x = block(x, node_ctrs, nodes_c, acts, actor_ctrs, actors_c, cfg["actor2map_dist"], "a2m")
    out["m2m"] = x = fuse(x, "m2m.fuse")
    out["m2a"] = y = block(acts, actor_ctrs, actors_c, x, node_ctrs, nodes_c, cfg["map2actor_dist"], "m2a")
    out["a2a"] = block(y, actor_ctrs, actors_c, None, actor_ctrs, actors_c, cfg["actor2actor_dist"], "a2a")
    return {k: arr(v, np.float64) for k, v in out.items()}


def up2_linear(r):
    """F.interpolate(scale_factor=2, mode="linear", align_corners=False) along axis 1 of r [A, n, c] in float64 (up2_taps of
    csrc/lgcn_conv.hpp): source coordinate (j + 0.5) / 2 - 0.5 clamped at 0, so out[2i] = 0.25 r[i - 1] + 0.75 r[i] and
    out[2i + 1] = 0.75 r[i] + 0.25 r[i + 1], the two ends clamped (out[0] = r[0], out[2n - 1] = r[n - 1])."""
    r = arr(r, np.float64)
    n = r.shape[1]
    src = np.maximum((np.arange(2 * n) + 0.5) * 0.5 - 0.5, 0.0)
    i0 = np.floor(src).astype(np.int64)
    i1 = np.minimum(i0 + 1, n - 1)
    w1 = (src - i0)[None, :, None]
    return (1.0 - w1) * r[:, i0] + w1 * r[:, i1]


def conv1d_unit(x, w, stride, gamma, beta, mode, eps=EPS, relu=False, res=None, res_up2=False, model=True):
    """lgcn_conv1d_gn_train on channels-last x [A, L, cin], w [cout, cin, ks] (ks 1 / 3, padding (ks - 1) / 2, no bias):
    (out, y), y the convolution, out = act(GN(y) + residual) with the statistics over an actor's lout x cout values.
    res [A, lout, cout], or [A, lout / 2, cout] with res_up2 (upsampled x2, up2_linear); the model takes it as fp32, as
    the kernel holds it, and adds it in float64.
    mode "f16x2": the two-plane units; "f32": the exact units."""
    dt = np.float32 if model else np.float64
    x, w = arr(x).astype(dt), arr(w, np.float32)
    A_, lin, cin = x.shape
    cout, _, ks = w.shape
    pad = (ks - 1) // 2
    lout = (lin + 2 * pad - ks) // stride + 1
    xp = np.zeros((A_, lin + 2 * pad, cin), dt)
    xp[:, pad:pad + lin] = x
    y = np.zeros((A_ * lout, cout))
    for t in range(ks):
        rows = xp[:, t:t + (lout - 1) * stride + 1:stride].reshape(A_ * lout, cin)
        y = y + _mm(rows, w[:, :, t], mode, model)
    y = y.reshape(A_, lout, cout)
    mu = y.mean((1, 2), keepdims=True)
    var = ((y - mu) ** 2).mean((1, 2), keepdims=True)
    out = (y - mu) / np.sqrt(var + eps) * arr(gamma, np.float64) + arr(beta, np.float64)
    if res is not None:
        r = arr(_hold(res, model), np.float64)
        assert r.shape == ((A_, lout // 2, cout) if res_up2 else (A_, lout, cout)) and not (res_up2 and lout % 2)
        out = out + (up2_linear(r) if res_up2 else r)
    return (np.maximum(out, 0.0) if relu else out), y


def res1d_block(x, blk, mode, second=None, model=True):
    """layers.Res1d on channels-last x [A, L, cin] as the composition of conv1d_unit calls that ops.res1d_gn stands for
    (lgcn_res1d_gn; with `second`, a C -> C block with the identity shortcut chained behind, lgcn_res1d_pair_gn):
        out = act( GN2(conv2( relu(GN1(conv1 x)) )) + r ),   r = x, or GN_d(conv_d x) with conv_d k = 1 at conv1's stride.
    blk: dict(w1, stride, gn1 = (gamma, beta), w2, gn2, wd = None, gnd = None, eps, act = True).  What one unit hands to
    the next -- the intermediate rows the fused launches keep in LDS, the shortcut's rows, the first block's output -- is
    an fp32 value that is split again: _hold.  Mode "f32" rounds nothing anywhere (no operand format to model), so its
    model is the reference and its error 0, as hot_path_cases.model_err has it."""
    hold = model = model and mode != "f32"
    kw = dict(eps=blk.get("eps", EPS), model=model)
    x = _hold(x, hold)
    mid = _hold(conv1d_unit(x, blk["w1"], blk["stride"], *blk["gn1"], mode, relu=True, **kw)[0], hold)
    skip = x
    if blk.get("wd") is not None:
        skip = _hold(conv1d_unit(x, blk["wd"], blk["stride"], *blk["gnd"], mode, **kw)[0], hold)
    out = conv1d_unit(mid, blk["w2"], 1, *blk["gn2"], mode, relu=blk.get("act", True), res=skip, **kw)[0]
    if second is None:
        return out
    assert second.get("wd") is None and second["stride"] == 1
    return res1d_block(_hold(out, hold), second, mode, model=model)


def actor_blocks(state, eps=EPS):
    """ActorNet's state dict (groups.g.b.{conv1, bn1, conv2, bn2, downsample.0, downsample.1}, lateral.i.{conv, norm},
    output.*) as res1d_block's dicts: (groups [[blk, blk]] x 3, lateral [(w, gamma, beta)] x 3, output blk).  The strides
    are the architecture's (the first block of groups 1 and 2 halves the length)."""
    W = lambda name: arr(state[name], np.float32)
    G = lambda name: (W(name + ".weight"), W(name + ".bias"))

    def blk(p, stride):
        d = dict(w1=W(p + ".conv1.weight"), stride=stride, gn1=G(p + ".bn1"), w2=W(p + ".conv2.weight"), gn2=G(p + ".bn2"), eps=eps)
        if p + ".downsample.0.weight" in state:
            d.update(wd=W(p + ".downsample.0.weight"), gnd=G(p + ".downsample.1"))
        return d
    groups = [[blk("groups.%d.0" % g, 1 if g == 0 else 2), blk("groups.%d.1" % g, 1)] for g in range(3)]
    lateral = [(W("lateral.%d.conv.weight" % i),) + G("lateral.%d.norm" % i) for i in range(3)]
    return groups, lateral, blk("output", 1)


def actor_net(x, state, mode, model=True):
    """ActorNet on x [A, 3, L] (the module's input; L = 20): the FPN walk of ActorNet._forward_hip over conv1d_unit /
    res1d_block -- three groups of two Res1d blocks (lengths L, L / 2, L / 4), the coarsest lateral, two top-down steps
    (lateral conv + GN + the x2-upsampled coarser level, no ReLU), the output block -- returning its last step [A, 128].
    Every unit's output is held in fp32 (the launches hand fp32 tensors on; the fused launches' LDS rows are fp32 values
    too); mode "f32": nothing is rounded (res1d_block)."""
    groups, lateral, output = actor_blocks(state)
    hold = model = model and mode != "f32"
    out, pyramid = arr(x).transpose(0, 2, 1), []
    for g in groups:
        out = _hold(res1d_block(out, g[0], mode, second=g[1], model=model), hold)
        pyramid.append(out)
    w, gamma, beta = lateral[2]
    out = _hold(conv1d_unit(pyramid[2], w, 1, gamma, beta, mode, model=model)[0], hold)
    for i in (1, 0):
        w, gamma, beta = lateral[i]
        out = _hold(conv1d_unit(pyramid[i], w, 1, gamma, beta, mode, res=out, res_up2=True, model=model)[0], hold)
    return arr(res1d_block(out, output, mode, model=model)[:, -1, :], np.float64)


def bar(e_model):
    """What a kernel may show against float64 where its format's model shows e_model: twice the model, never below
    1e-6 (fp32's own reordering noise on a 128-term sum), and inside the window -- where the model stays under 5e-5 --
    never above the project's 1e-4."""
    b = max(2.0 * e_model, 1e-6)
    return min(b, 1e-4) if e_model <= 5e-5 else b
