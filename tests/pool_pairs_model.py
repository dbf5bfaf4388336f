"""Float64 model, in plain torch on the CPU, of the pair stage of the fork's LanePooling as include/lgcn.h states it for
lgcn_pool_pairs, and of the whole LanePooling built around it -- TEST INFRASTRUCTURE ONLY.  Pinned against the reference's
own capture pool/out of tests/golden/lanercnn_b3.npz by test_pool_pairs_model_host.py before any kernel is compared with
it."""
import torch

EPS = 1e-5
C = 128


def gn64(x, g, b, eps=EPS):
    """GroupNorm(1, C) of the rows of x (biased variance) with gain g and bias b."""
    mu = x.mean(1, keepdim=True)
    var = ((x - mu) ** 2).mean(1, keepdim=True)
    return (x - mu) / torch.sqrt(var + eps) * g + b


def pair_stage(ctx_pose, tgt_pose, ti, ci, wp, bp, w0h, U, g, bt, eps=EPS):
    """m [P,128] in float64.  ctx_pose [C,4], tgt_pose [T,4]: fp32 tensors -- the subtraction is done in fp32, as in the
    reference and the kernel (it is exact for the poses the tests use); ti, ci: LongTensors [P]; wp [128,4], bp [128]:
    relpose.0; w0h [128,128]: ctx.0's columns 128:256; U [C,128] the hoisted context row block; g, bt: ctx.0's norm."""
    f = lambda t: t.double()
    d = (ctx_pose.float()[ci] - tgt_pose.float()[ti]).double()
    h = torch.relu(d @ f(wp).t() + f(bp))
    z = h @ f(w0h).t() + f(U)[ci]
    return torch.relu(gn64(z, f(g), f(bt), eps))


def pair_search(context_ctrs, target_ctrs, dist_th=6.0):
    """(ci, ti) as the reference lists them (lanercnn.py:468-487): context-major per scene, a scene without a pair
    advancing neither offset; distances in the inputs' own precision."""
    ci, ti, cc, tc = [], [], 0, 0
    for c, t in zip(context_ctrs, target_ctrs):
        dist = torch.sqrt(((c.view(-1, 1, 2) - t.view(1, -1, 2)) ** 2).sum(2))
        idcs = torch.nonzero(dist <= dist_th, as_tuple=False)
        if len(idcs) == 0:
            continue
        ci.append(idcs[:, 0] + cc)
        ti.append(idcs[:, 1] + tc)
        cc += len(c)
        tc += len(t)
    return torch.cat(ci, 0), torch.cat(ti, 0)


def lane_pooling(context_feat, context_graph, target_feat, target_graph, sd, prefix="pool", dist_th=6.0):
    """LanePooling.forward (lanercnn.py:462-514) in float64 with the pair stage above: (out [T,128], ci, ti)."""
    f = lambda k: sd[prefix + "." + k].double()
    ci, ti = pair_search(context_graph["ctrs"], target_graph["ctrs"], dist_th)
    c_pose, t_pose = torch.cat(context_graph["pose"], 0), torch.cat(target_graph["pose"], 0)
    w0 = f("ctx.0.linear.weight")
    U = context_feat.double() @ w0[:, :C].t()
    m = pair_stage(c_pose, t_pose, ti, ci, f("relpose.0.weight"), f("relpose.0.bias"), w0[:, C:], U,
                   f("ctx.0.norm.weight"), f("ctx.0.norm.bias"))
    tf = target_feat.double()
    out = tf @ f("input.weight").t()
    out = out.index_add(0, ti, m @ f("ctx.1.weight").t())
    out = torch.relu(gn64(out, f("norm.weight"), f("norm.bias")))
    out = torch.relu(gn64(out @ f("mlp.0.linear.weight").t(), f("mlp.0.norm.weight"), f("mlp.0.norm.bias")))
    out = gn64(out @ f("mlp.1.linear.weight").t(), f("mlp.1.norm.weight"), f("mlp.1.norm.bias"))
    return torch.relu(out + tf), ci, ti
