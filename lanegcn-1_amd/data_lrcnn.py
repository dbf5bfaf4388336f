"""Input side of the fork model: the per-agent lane RoIs of the reference's data_lrcnn.generate_lane_roi
(data_lrcnn.py:620-844), built on the device for a whole batch of scenes (csrc/lgcn_roi.hip).
Two routes: per-RoI dicts in the reference's schema (generate_lane_roi, generate_lane_roi_batch), and the flat route
(lane_roi_flat, generate_lane_roi_flat, store_roi_inputs -> RoiBatch), in which the kernels write the batch's merged
graph and nothing is split per RoI.

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


def _roi_inputs(scenes):
    """(t, off, agent_off) of ops.RoiJob for a non-empty list of scene dicts: the leaves concatenated on the device, the
    int32 offset table and the agents' offsets [S + 1]; the lane cap and the shapes are checked before any copy."""
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
    return t, off.astype(np.int32), tabs[2]


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
    t, off, agent_off = _roi_inputs(scenes)
    job = ops.RoiJob(t, off, horizon_buffer)
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
    scene_of = np.searchsorted(agent_off, valid, side="right") - 1
    for b, s in enumerate(scenes):
        s["subgraphs"] = []
        s["valid_agent_ids"] = (valid[scene_of == b] - agent_off[b]).astype(np.int16)
    if R == 0:
        return scenes
    sizes = counts[valid].astype(np.int64)
    csum = lambda sizes: np.concatenate([[0], np.cumsum(sizes, dtype=np.int64)])
    roi_base = csum(sizes)
    if roi_base[-1] > 0x7fffffff:
        raise L.LgcnError("generate_lane_roi: the RoIs hold more than 2^31 - 1 nodes")
    dev = job.ws.device
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


# ------------------------------------------------------------------ the flat route: RoIs as one batch graph
def relation_major_tables(cnt):
    """Host tables of lgcn_roi_edge_fill_graph from the edge counts cnt [R, 15] (14 relations, then |a2m|):
    (edge_base [R, 15] int32, rel_ext [15] int64, n_a2m).  The relations are laid out RELATION-major -- relation k of
    every RoI back to back in RoI order, then relation k + 1 -- so relation k of the batch graph is
    out[rel_ext[k]:rel_ext[k + 1]], in the order a concatenation over the RoIs gives; a2m is RoI-major in arrays of its
    own.  Vectorised numpy, no loop over RoIs.  LgcnError beyond 2^31 - 1 edges."""
    cnt = np.asarray(cnt, np.int64).reshape(-1, ops.ROI_REL + 1)
    R = cnt.shape[0]
    rel = np.ascontiguousarray(cnt[:, :ops.ROI_REL].T)                   # [14, R]
    ends = np.cumsum(rel.reshape(-1), dtype=np.int64)
    a2m_ends = np.cumsum(cnt[:, ops.ROI_REL], dtype=np.int64)
    n_rel, n_a2m = (int(ends[-1]), int(a2m_ends[-1])) if R else (0, 0)
    if n_rel > 0x7fffffff or n_a2m > 0x7fffffff:
        raise L.LgcnError("generate_lane_roi: the RoIs hold more than 2^31 - 1 edges")
    base = np.empty((R, ops.ROI_REL + 1), np.int32)
    base[:, :ops.ROI_REL] = (ends - rel.reshape(-1)).reshape(ops.ROI_REL, R).T
    base[:, ops.ROI_REL] = a2m_ends - cnt[:, ops.ROI_REL]
    rel_ext = np.concatenate([[0], ends[R - 1::R]]).astype(np.int64) if R else np.zeros(ops.ROI_REL + 1, np.int64)
    return base, rel_ext, n_a2m


class RoiBatch:
    """The lane RoIs of a batch of scenes as ONE graph, as lane_roi_flat leaves them: what lanercnn.subgraph_gather
    builds from per-RoI dicts, without the dicts.

    Device (flat, RoI-major rows): feats [T, 8], node_mask [T] int64 (scene-local node of every row), agent_feat [R, 80];
    u, v [E] int64 and a2m_u, a2m_v [n_a2m] int64: indices of the merged graph (row of feats; a2m_u: row of agent_feat),
    relation k (pre 0..5, suc 0..5, left, right) at [rel_ext[k], rel_ext[k + 1]).
    Host (numpy): sizes [R], roi_base [R + 1] (first row of every RoI), scene_of [R], agents [R] (batch-wide agent row of
    every RoI), agent_off [S + 1], agent_vel [R] fp32, rel_ext [15], edge_cnt [R, 15].  Every scene holds at least one RoI
    (lane_roi_flat refuses the batch otherwise)."""

    def __init__(self, feats, node_mask, agent_feat, u, v, a2m_u, a2m_v, sizes, scene_of, agents, agent_off, agent_vel,
                 rel_ext, edge_cnt):
        self.feats, self.node_mask, self.agent_feat = feats, node_mask, agent_feat
        self.u, self.v, self.a2m_u, self.a2m_v = u, v, a2m_u, a2m_v
        i64 = lambda x: np.ascontiguousarray(x, np.int64)
        self.sizes, self.scene_of, self.agents, self.agent_off = i64(sizes), i64(scene_of), i64(agents), i64(agent_off)
        self.agent_vel = np.ascontiguousarray(agent_vel, np.float32)
        self.rel_ext, self.edge_cnt = i64(rel_ext), i64(edge_cnt).reshape(-1, ops.ROI_REL + 1)
        self.roi_base = np.concatenate([[0], np.cumsum(self.sizes, dtype=np.int64)])
        self.n_scenes, self.n_rois = len(self.agent_off) - 1, len(self.sizes)
        self.rois_per_scene = np.bincount(self.scene_of, minlength=self.n_scenes).astype(np.int64)
        if self.n_scenes == 0 or (np.diff(self.scene_of) < 0).any():
            raise L.LgcnError("RoiBatch: no scene in the batch, or RoIs out of scene order")
        empty = np.flatnonzero(self.rois_per_scene == 0)
        if len(empty):
            raise L.LgcnError("RoiBatch: scene %d has no lane RoI (every agent of the scene dropped)" % int(empty[0]))
        self.first_roi = np.concatenate([[0], np.cumsum(self.rois_per_scene)])

    def valid_agent_ids(self, b):
        """The kept agents of scene b, scene-local, int16 (the reference's data["valid_agent_ids"])."""
        lo, hi = self.first_roi[b], self.first_roi[b + 1]
        return (self.agents[lo:hi] - self.agent_off[b]).astype(np.int16)

    def bookkeeping(self):
        """lanercnn.subgraph_bookkeeping of the equivalent per-RoI lists, from the host tables."""
        base, first = self.roi_base, self.first_roi
        counts = base[:-1].tolist()
        return {"num_nodes": int(base[-1]), "counts": counts,
                "batch_spans": [[lo, hi] for lo, hi in zip(base[first[:-1]].tolist(), base[first[1:]].tolist())],
                "num_atgs_per_batch": self.rois_per_scene.tolist(),
                "roi_spans": [[lo, hi] for lo, hi in zip(counts, base[1:].tolist())],
                "interest_roi": torch.tensor(first[:-1].tolist(), dtype=torch.long)}

    def subgraphs(self):
        """The per-RoI dicts of generate_lane_roi_batch(device=True), one list per scene: views of the flat buffers, the
        RoI-local indices recovered by subtracting the RoI's base (two subtractions for the batch, then splits).  For
        callers of the list interface and for the tests; subgraph_gather does not need it."""
        R, K, dev = self.n_rois, ops.ROI_REL, self.feats.device
        rel_cnt = np.ascontiguousarray(self.edge_cnt[:, :K].T).reshape(-1)                # relation-major, as u / v lie
        a2m_cnt = self.edge_cnt[:, K]
        owner = np.concatenate([np.repeat(np.tile(self.roi_base[:-1], K), rel_cnt), np.repeat(self.roi_base[:-1], a2m_cnt)])
        owner = torch.from_numpy(owner).to(dev)
        E = int(rel_cnt.sum())
        sizes = self.sizes.tolist()
        p_u, p_v = (self.u - owner[:E]).split(rel_cnt.tolist()), (self.v - owner[:E]).split(rel_cnt.tolist())
        a2m_v = (self.a2m_v - owner[E:]).to(torch.int32)
        p_av, p_au = a2m_v.split(a2m_cnt.tolist()), torch.zeros_like(a2m_v).split(a2m_cnt.tolist())
        p_mask, p_feats, rows = self.node_mask.split(sizes), self.feats.split(sizes), self.agent_feat.unbind(0)
        out = [[] for _ in range(self.n_scenes)]
        for r in range(R):
            e = [{"u": p_u[k * R + r], "v": p_v[k * R + r]} for k in range(K)]
            out[self.scene_of[r]].append({
                "a2m": {"u": p_au[r], "v": p_av[r]}, "node_mask": p_mask[r], "num_nodes": sizes[r], "feats": p_feats[r],
                "agent_feat": rows[r], "agent_vel": self.agent_vel[r],
                "pre": e[:6], "suc": e[6:12], "left": e[12], "right": e[13]})
        return out


def lane_roi_flat(t, off, horizon_buffer=20.):
    """The lane RoIs of a batch straight from flat arrays -> RoiBatch.  t, off: the inputs of ops.RoiJob as they are (the
    scenes' arrays concatenated on the device with scene-local int32 indices, and the host offset table of
    include/lgcn.h).  roi_search / roi_nodes / roi_edge_count as generate_lane_roi_batch runs them, with its two size
    read-backs, checks and messages; then ops.roi_edge_fill_graph at a relation-major edge_base writes the indices of the
    merged graph, so that nothing is split per RoI or concatenated again: 11 kernel launches, one memset and one zero
    fill per batch.  LgcnError, naming the scene, for a scene none of whose agents keeps an RoI (the list route fails
    there later, on an assert of subgraph_bookkeeping)."""
    if not torch.cuda.is_available():
        raise L.LgcnError("data_lrcnn.lane_roi_flat needs a GPU (the lane-RoI kernels have no CPU fallback)")
    job = ops.RoiJob(t, off, horizon_buffer)
    S, A_ = job.S, job.A
    if S == 0:
        raise L.LgcnError("lane_roi_flat: no scene in the batch")
    agent_off = job.off[2 * (S + 1):3 * (S + 1)].astype(np.int64)
    dev = job.ws.device
    counts, vel = np.zeros(0, np.int32), np.zeros(0, np.float32)
    if A_ > 0:
        ops.roi_search(job)
        head = job.agent_out.cpu().numpy()                       # read-back 1: node count per agent, status, speeds
        counts, status, vel = head[:A_], int(head[A_]), head[A_ + 1:].view(np.float32)
        if status & ops.ROI_STATUS_RANGE:
            raise L.LgcnError("generate_lane_roi: a node, lane or pair index lies outside its scene")
        if status & ops.ROI_STATUS_LEVELS:
            raise L.LgcnError("generate_lane_roi: a lane search did not end (a cycle of zero-length lanes)")
    valid = np.flatnonzero(counts > 0)
    R = len(valid)
    scene_of = np.searchsorted(agent_off, valid, side="right") - 1
    per_scene = np.bincount(scene_of, minlength=S)
    if (per_scene == 0).any():
        raise L.LgcnError("lane_roi_flat: scene %d has no lane RoI (every agent dropped)" % int(np.flatnonzero(per_scene == 0)[0]))
    sizes = counts[valid].astype(np.int64)
    roi_base = np.concatenate([[0], np.cumsum(sizes, dtype=np.int64)])
    if roi_base[-1] > 0x7fffffff:
        raise L.LgcnError("generate_lane_roi: the RoIs hold more than 2^31 - 1 nodes")
    table = torch.from_numpy(np.concatenate([valid, roi_base]).astype(np.int32)).to(dev)
    node_mask, feats, agent_feat = ops.roi_nodes(job, table[:R], table[R:], int(roi_base[-1]))
    cnt = ops.roi_edge_count(job).cpu().numpy().astype(np.int64)          # read-back 2: edge counts
    base, rel_ext, n_a2m = relation_major_tables(cnt)
    u, v, a2m_u, a2m_v = ops.roi_edge_fill_graph(job, torch.from_numpy(base).to(dev), int(rel_ext[-1]), n_a2m)
    return RoiBatch(feats, node_mask, agent_feat, u, v, a2m_u, a2m_v, sizes, scene_of, valid, agent_off, vel[valid], rel_ext, cnt)


def store_roi_inputs(store):
    """(t, off) of ops.RoiJob / lane_roi_flat from a flatfile.DeviceSceneStore that data_raw.build_store(..., lanes=True)
    made, for ALL its scenes: the node and actor arrays are the store's own tensors; the int32 scene-local edges come out
    of the store's relation-major edge_u / edge_v by one concatenation of 14 relation blocks (the store orders pre0, suc0,
    pre1, ..., left, right; the RoI kernels pre 0..5, suc 0..5, left, right), the agents' steps and positions by one
    strided copy each; the offset table from the store's host tables.  Nothing per scene.  LgcnError for a store without
    the lane arrays."""
    la = getattr(store, "lane_arrays", None)
    if la is None:
        raise L.LgcnError("lane RoIs need the lane arrays of the store: build it with data_raw.build_store(..., lanes=True)")
    ns, S, a = store.num_scales, store.n_scenes, store._job.t
    if 2 * ns + 2 != ops.ROI_REL:
        raise L.LgcnError("lane RoIs need a store of 6 scales, got %d" % ns)
    order = [2 * k for k in range(ns)] + [2 * k + 1 for k in range(ns)] + [2 * ns, 2 * ns + 1]
    ro = store.rel_off.tolist()
    n_agents, n_lanes = np.diff(store.actor_off), np.diff(la["lane_off"])
    csum = lambda sizes: np.concatenate([[0], np.cumsum(sizes, dtype=np.int64)])
    off = np.concatenate([store.node_off, la["lane_off"], store.actor_off, csum(n_agents * n_lanes), la["suc_off"], la["pre_off"],
                          csum(np.diff(store.edge_off[order], axis=1).reshape(-1))])
    if off.max() > 0x7fffffff:
        raise L.LgcnError("generate_lane_roi: the batch is too large for 32-bit offsets")
    cap = ops.roi_max_lanes()
    if S and n_lanes.max() > cap:
        b = int(np.argmax(n_lanes))
        raise L.LgcnError("generate_lane_roi: scene %d has %d lanes, the lane-RoI kernels take at most %d" % (b, n_lanes[b], cap))
    t = dict(ctrs=a["node_ctrs"], feats=a["node_feats"], turn=a["turn"], control=a["control"], intersect=a["intersect"],
             lane_idcs=la["lane_idcs"].to(torch.int32), a_ctrs=a["actor_ctrs"],
             a_feats=a["actor_feats"][:, :, :2].contiguous(), a_obs=la["obs"][:, :, :2].contiguous(),
             suc_pairs=la["suc_pairs"].to(torch.int32), pre_pairs=la["pre_pairs"].to(torch.int32),
             edge_u=torch.cat([a["edge_u"][ro[k]:ro[k + 1]] for k in order]),
             edge_v=torch.cat([a["edge_v"][ro[k]:ro[k + 1]] for k in order]))
    return t, off.astype(np.int32)


def generate_lane_roi_flat(scenes, horizon_buffer=20.):
    """generate_lane_roi_batch(scenes, horizon_buffer, device=True) on the flat route: sets scene["valid_agent_ids"]
    (int16) of every scene in place and returns the batch's RoiBatch in the place of scene["subgraphs"] (which is left
    alone).  lanercnn.subgraph_gather and Net.forward take the RoiBatch where they take data["subgraphs"].  Inputs,
    limits and errors are generate_lane_roi_batch's, plus lane_roi_flat's LgcnError for a scene without an RoI."""
    if not torch.cuda.is_available():
        raise L.LgcnError("data_lrcnn.generate_lane_roi needs a GPU (the lane-RoI kernels have no CPU fallback)")
    scenes = list(scenes)
    if not scenes:
        raise L.LgcnError("lane_roi_flat: no scene in the batch")
    t, off, _ = _roi_inputs(scenes)
    rb = lane_roi_flat(t, off, horizon_buffer)
    for b, s in enumerate(scenes):
        s["valid_agent_ids"] = rb.valid_agent_ids(b)
    return rb


def generate_lane_roi(data, horizon_buffer=20., max_vel_threshold=2.78):
    """The reference's generate_lane_roi (data_lrcnn.py:690-844) on the device: adds data["subgraphs"] -- one RoI dict per
    kept agent: a2m {u, v} int32, node_mask int64, num_nodes int, feats fp32 [n,8], agent_feat fp32 [80], agent_vel
    np.float32, pre / suc lists of six {u, v} int64, left / right {u, v} int64, leaves numpy -- and
    data["valid_agent_ids"] (int16), and returns data.  max_vel_threshold is accepted and, as in the reference, unused.
    See generate_lane_roi_batch for the two deliberate differences (a lane listed twice is kept once, at its first
    occurrence; distance ties go to the smaller node index) and the limits."""
    generate_lane_roi_batch([data], horizon_buffer)
    return data
