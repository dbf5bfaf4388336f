"""Input side of the fork model: the per-agent lane RoIs of the reference's data_lrcnn.generate_lane_roi
(data_lrcnn.py:620-844), built on the device for a whole batch of scenes (csrc/lgcn_roi.hip).

The reference's dataset reader stays out of scope (argoverse-api); generate_lane_roi reads nothing but the preprocessed
scene dict, and that is what is ported."""
import numpy as np
import torch

from . import _lib as L
from . import ops

REL_KEYS = [("pre", i) for i in range(6)] + [("suc", i) for i in range(6)] + [("left", None), ("right", None)]


def _is_host(x):
    return not (torch.is_tensor(x) and x.is_cuda)


def _host(x, dtype):
    return np.asarray(x.detach().numpy() if torch.is_tensor(x) else x).astype(dtype, copy=False)


def _cat(parts, np_dtype, tail, dev):
    """The concatenation of `parts` (numpy arrays, CPU or GPU tensors) along axis 0 as one device tensor of np_dtype."""
    tdtype = torch.from_numpy(np.zeros(0, np_dtype)).dtype
    if all(_is_host(x) for x in parts):      # one host concatenation, one copy
        flat = np.concatenate([_host(x, np_dtype).reshape((-1,) + tail) for x in parts] + [np.zeros((0,) + tail, np_dtype)])
        return torch.from_numpy(np.ascontiguousarray(flat)).to(dev)
    return torch.cat([torch.as_tensor(x).to(dev).to(tdtype).reshape((-1,) + tail) for x in parts]
                     + [torch.zeros((0,) + tail, dtype=tdtype, device=dev)], 0).contiguous()


def _rel(graph, k1, i):
    return graph[k1] if i is None else graph[k1][i]


def _lane_counts(scenes):
    """Lanes of every scene, lane_idcs[-1] + 1 as the reference counts them (one read-back for leaves on the device)."""
    last, on_dev = [], []
    for b, s in enumerate(scenes):
        li = s["graph"]["lane_idcs"]
        if len(li) == 0:
            last.append(-1)
        elif _is_host(li):
            last.append(int(li[-1]))
        else:
            last.append(None)
            on_dev.append((b, li[-1:]))
    if on_dev:
        vals = torch.cat([x for _, x in on_dev]).cpu().tolist()
        for (b, _), v in zip(on_dev, vals):
            last[b] = int(v)
    return [v + 1 for v in last]


def generate_lane_roi_batch(scenes, horizon_buffer=20., device=False):
    """generate_lane_roi for a list of scene dicts in one pass on the device: fills scene["subgraphs"] and
    scene["valid_agent_ids"] (int16) of every scene in place and returns the list.

    Leaves of the scenes may be numpy arrays, CPU or GPU tensors, index arrays of any integer type.  With device=False
    the leaves of the RoIs are numpy arrays (the reference's dtypes); with device=True they are views into the batch's
    flat buffers on the current device, which lanercnn.subgraph_gather takes as they are.  num_nodes stays a Python int
    and agent_vel a host np.float32.  A scene whose agents all drop gets empty lists.

    Differences from the reference, both deliberate: a lane that the search lists more than once (a lane cycle shorter
    than the horizon, with no left / right neighbour outside the RoI) is kept ONCE, at its first occurrence, where the
    reference emits its nodes twice; and among eligible nodes at exactly the same distance the anchor is the one with the
    smaller index, where the reference's unstable argsort leaves the choice open.  A lane search that does not end within
    lgcn_roi_max_levels() levels (a cycle of zero-length lanes, on which the reference never returns) raises LgcnError
    ("did not end").  So does EVERY index out of range ("outside its scene"), whether or not an RoI would have reached it:
    a node index of one of the 14 relations, a lane index of suc_pairs / pre_pairs (these two are read by the searches, so
    only in a scene with a moving agent that has an anchor), and a lane_idcs value below 0 or above lane_idcs[-1] (the
    reference counts lanes as lane_idcs[-1] + 1 and would leave such a node out of every RoI in silence).  The status is
    per batch: one bad scene fails the call, and the next call starts clean (a batch without any agent launches nothing
    and checks nothing).  Lane lengths are summed as np.sum does for
    any number of nodes (pairwise in blocks of 128, through the default 8192-element buffer).
    At most ops.roi_max_lanes() = 4096 lanes per scene (LgcnError above, nothing is launched).

    11 kernel launches, one memset and two zero fills per batch, whatever the number of scenes, agents or RoIs, and two
    size read-backs (node counts, edge counts)."""
    if not torch.cuda.is_available():
        raise L.LgcnError("data_lrcnn.generate_lane_roi needs a GPU (the lane-RoI kernels have no CPU fallback)")
    scenes = list(scenes)
    S = len(scenes)
    if S == 0:
        return scenes
    n_lanes = _lane_counts(scenes)
    cap = ops.roi_max_lanes()
    for b, nl in enumerate(n_lanes):
        if nl > cap:
            raise L.LgcnError("generate_lane_roi: scene %d has %d lanes, the lane-RoI kernels take at most %d" % (b, nl, cap))
        if nl <= 0 and len(scenes[b]["graph"]["lane_idcs"]):      # lane_idcs[-1] < 0: no lane for the kernels to check against
            raise L.LgcnError("generate_lane_roi: a node, lane or pair index lies outside its scene")
    dev =torch.device("cuda", torch.cuda.current_device())
    graphs = [s["graph"] for s in scenes]
    n_nodes = [len(g["lane_idcs"]) for g in graphs]
    n_agents = [len(s["ctrs"]) for s in scenes]
    for s in scenes:
        if tuple(s["feats"].shape[1:2]) != (20,) or tuple(s["obs_trajs"].shape[1:2]) != (20,):
            raise L.LgcnError("generate_lane_roi: feats and obs_trajs must hold 20 observed steps")
    pairs = {k: [g[k + "_pairs"] for g in graphs] for k in ("suc", "pre")}
    edges = [[_rel(g, k1, i) for g in graphs] for k1, i in REL_KEYS]
    csum = lambda sizes: np.concatenate([[0], np.cumsum(sizes, dtype=np.int64)])
    tabs = [csum(n_nodes), csum(n_lanes), csum(n_agents), csum([a * l for a, l in zip(n_agents, n_lanes)]),
            csum([len(x) for x in pairs["suc"]]), csum([len(x) for x in pairs["pre"]]),
            csum([len(e["u"]) for rel in edges for e in rel])]
    off = np.concatenate(tabs)
    if off.max() > 0x7fffffff:
        raise L.LgcnError("generate_lane_roi: the batch is too large for 32-bit offsets")
    t = dict(
        ctrs=_cat([g["ctrs"] for g in graphs], np.float32, (2,), dev),
        feats=_cat([g["feats"] for g in graphs], np.float32, (2,), dev),
        turn=_cat([g["turn"] for g in graphs], np.float32, (2,), dev),
        control=_cat([g["control"] for g in graphs], np.float32, (), dev),
        intersect=_cat([g["intersect"] for g in graphs], np.float32, (), dev),
        lane_idcs=_cat([g["lane_idcs"] for g in graphs], np.int32, (), dev),
        a_ctrs=_cat([s["ctrs"] for s in scenes], np.float32, (2,), dev),
        a_feats=_cat([s["feats"][:, :, :2] for s in scenes], np.float32, (20, 2), dev),
        a_obs=_cat([s["obs_trajs"][:, :, :2] for s in scenes], np.float32, (20, 2), dev),
        suc_pairs=_cat(pairs["suc"], np.int32, (2,), dev),
        pre_pairs=_cat(pairs["pre"], np.int32, (2,), dev),
        edge_u=_cat([e["u"] for rel in edges for e in rel], np.int32, (), dev),
        edge_v=_cat([e["v"] for rel in edges for e in rel], np.int32, (), dev),
    )
    job = ops.RoiJob(t, off.astype(np.int32), horizon_buffer)
    A_ = job.A
    for s in scenes:
        s["subgraphs"], s["valid_agent_ids"] = [], np.zeros(0, np.int16)
    if A_ == 0:
        return scenes
    ops.roi_search(job)
    head = job.agent_out.cpu().numpy()                       # read-back 1: node count per agent, status, speeds
    counts, status, vel = head[:A_], int(head[A_]), head[A_ + 1:].view(np.float32)
    if status & ops.ROI_STATUS_RANGE:
        raise L.LgcnError("generate_lane_roi: a node, lane or pair index lies outside its scene")
    if status & ops.ROI_STATUS_LEVELS:
        raise L.LgcnError("generate_lane_roi: a lane search did not end (a cycle of zero-length lanes)")
    valid = np.flatnonzero(counts > 0)
    R = len(valid)
    agent_off = tabs[2]
    scene_of = np.searchsorted(agent_off, valid, side="right") - 1
    for b, s in enumerate(scenes):
        s["subgraphs"] = []
        s["valid_agent_ids"] = (valid[scene_of == b] - agent_off[b]).astype(np.int16)
    if R == 0:
        return scenes
    sizes = counts[valid].astype(np.int64)
    roi_base = csum(sizes)
    if roi_base[-1] > 0x7fffffff:
        raise L.LgcnError("generate_lane_roi: the RoIs hold more than 2^31 - 1 nodes")
    table = torch.from_numpy(np.concatenate([valid, roi_base]).astype(np.int32)).to(dev)
    node_mask, feats, agent_feat = ops.roi_nodes(job, table[:R], table[R:], int(roi_base[-1]))
    cnt = ops.roi_edge_count(job).cpu().numpy().astype(np.int64)          # read-back 2: edge counts
    rel_sizes, a2m_sizes = cnt[:, :ops.ROI_REL].reshape(-1), cnt[:, ops.ROI_REL]
    rel_base, a2m_base = csum(rel_sizes), csum(a2m_sizes)
    if rel_base[-1] > 0x7fffffff:
        raise L.LgcnError("generate_lane_roi: the RoIs hold more than 2^31 - 1 edges")
    base = np.concatenate([rel_base[:-1].reshape(R, ops.ROI_REL), a2m_base[:-1, None]], 1).astype(np.int32)
    out_u, out_v, a2m_v = ops.roi_edge_fill(job, torch.from_numpy(np.ascontiguousarray(base)).to(dev),
                                            int(rel_base[-1]), int(a2m_base[-1]))
    a2m_u = torch.zeros_like(a2m_v)
    rel_sizes, a2m_sizes, sizes = rel_sizes.tolist(), a2m_sizes.tolist(), sizes.tolist()
    if device:
        cut = lambda x, n: x.split(n)
        agent_rows = agent_feat.unbind(0)
    else:
        def cut(x, n):
            return np.split(x.cpu().numpy(), np.cumsum(n[:-1]))
        agent_rows = list(agent_feat.cpu().numpy())
    p_mask, p_feats = cut(node_mask, sizes), cut(feats, sizes)
    p_u, p_v = cut(out_u, rel_sizes), cut(out_v, rel_sizes)
    p_au, p_av = cut(a2m_u, a2m_sizes), cut(a2m_v, a2m_sizes)
    for r in range(R):
        e = [{"u": p_u[k], "v": p_v[k]} for k in range(r * ops.ROI_REL, (r + 1) * ops.ROI_REL)]
        scenes[scene_of[r]]["subgraphs"].append({
            "a2m": {"u": p_au[r], "v": p_av[r]}, "node_mask": p_mask[r], "num_nodes": sizes[r], "feats": p_feats[r],
            "agent_feat": agent_rows[r], "agent_vel": vel[valid[r]],
            "pre": e[:6], "suc": e[6:12], "left": e[12], "right": e[13]})
    return scenes


def generate_lane_roi(data, horizon_buffer=20., max_vel_threshold=2.78):
    """The reference's generate_lane_roi (data_lrcnn.py:690-844) on the device: adds data["subgraphs"] -- one RoI dict per
    kept agent: a2m {u, v} int32, node_mask int64, num_nodes int, feats fp32 [n,8], agent_feat fp32 [80], agent_vel
    np.float32, pre / suc lists of six {u, v} int64, left / right {u, v} int64, leaves numpy -- and
    data["valid_agent_ids"] (int16), and returns data.  max_vel_threshold is accepted and, as in the reference, unused.
    See generate_lane_roi_batch for the two deliberate differences (a lane listed twice is kept once, at its first
    occurrence; distance ties go to the smaller node index) and the limits."""
    generate_lane_roi_batch([data], horizon_buffer)
    return data
