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


def _roi_extract(t, off, horizon_buffer, allow_empty):
    """The body of lane_roi_flat -> the arguments of RoiBatch, in its order.  allow_empty (RoiStore): a scene none of whose
    agents keeps an RoI is no error -- it simply owns no RoI; without a single RoI nothing more is launched."""
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
    if (per_scene == 0).any() and not allow_empty:
        raise L.LgcnError("lane_roi_flat: scene %d has no lane RoI (every agent dropped)" % int(np.flatnonzero(per_scene == 0)[0]))
    if R == 0:
        i64 = lambda: torch.zeros(0, dtype=torch.int64, device=dev)
        f32 = lambda *shape: torch.zeros(shape, dtype=torch.float32, device=dev)
        return (f32(0, 8), i64(), f32(0, 80), i64(), i64(), i64(), i64(), np.zeros(0, np.int64), scene_of, valid, agent_off,
                np.zeros(0, np.float32), np.zeros(ops.ROI_REL + 1, np.int64), np.zeros((0, ops.ROI_REL + 1), np.int64))
    sizes = counts[valid].astype(np.int64)
    roi_base = np.concatenate([[0], np.cumsum(sizes, dtype=np.int64)])
    if roi_base[-1] > 0x7fffffff:
        raise L.LgcnError("generate_lane_roi: the RoIs hold more than 2^31 - 1 nodes")
    table = torch.from_numpy(np.concatenate([valid, roi_base]).astype(np.int32)).to(dev)
    node_mask, feats, agent_feat = ops.roi_nodes(job, table[:R], table[R:], int(roi_base[-1]))
    cnt = ops.roi_edge_count(job).cpu().numpy().astype(np.int64)          # read-back 2: edge counts
    base, rel_ext, n_a2m = relation_major_tables(cnt)
    u, v, a2m_u, a2m_v = ops.roi_edge_fill_graph(job, torch.from_numpy(base).to(dev), int(rel_ext[-1]), n_a2m)
    return feats, node_mask, agent_feat, u, v, a2m_u, a2m_v, sizes, scene_of, valid, agent_off, vel[valid], rel_ext, cnt


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
    return RoiBatch(*_roi_extract(t, off, horizon_buffer, False))


def store_roi_inputs(store, scenes=None):
    """(t, off) of ops.RoiJob / lane_roi_flat from a flatfile.DeviceSceneStore that data_raw.build_store(..., lanes=True)
    made, for ALL its scenes, or for the scenes [lo, hi) of scenes=(lo, hi): the node and actor arrays are the store's own
    tensors (slices of them); the int32 scene-local edges come out of the store's relation-major edge_u / edge_v by one
    concatenation of 14 relation blocks (the store orders pre0, suc0, pre1, ..., left, right; the RoI kernels pre 0..5,
    suc 0..5, left, right), the agents' steps and positions by one strided copy each; the offset table from the store's
    host tables.  Nothing per scene.  LgcnError for a store without the lane arrays."""
    la = getattr(store, "lane_arrays", None)
    if la is None:
        raise L.LgcnError("lane RoIs need the lane arrays of the store: build it with data_raw.build_store(..., lanes=True)")
    ns, S, a = store.num_scales, store.n_scenes, store._job.t
    if 2 * ns + 2 != ops.ROI_REL:
        raise L.LgcnError("lane RoIs need a store of 6 scales, got %d" % ns)
    lo, hi = (0, S) if scenes is None else (int(scenes[0]), int(scenes[1]))
    if not 0 <= lo <= hi <= S:
        raise L.LgcnError("store_roi_inputs: scenes [%d, %d) of a store of %d" % (lo, hi, S))
    order = [2 * k for k in range(ns)] + [2 * k + 1 for k in range(ns)] + [2 * ns, 2 * ns + 1]
    ro = store.rel_off.tolist()
    cut = lambda tab: np.asarray(tab, np.int64)[lo:hi + 1] - int(tab[lo])       # the range's own prefix sums
    node_off, actor_off, lane_off = cut(store.node_off), cut(store.actor_off), cut(la["lane_off"])
    n_agents, n_lanes = np.diff(actor_off), np.diff(lane_off)
    csum = lambda sizes: np.concatenate([[0], np.cumsum(sizes, dtype=np.int64)])
    off = np.concatenate([node_off, lane_off, actor_off, csum(n_agents * n_lanes), cut(la["suc_off"]), cut(la["pre_off"]),
                          csum(np.diff(store.edge_off[order][:, lo:hi + 1], axis=1).reshape(-1))])
    if off.max() > 0x7fffffff:
        raise L.LgcnError("generate_lane_roi: the batch is too large for 32-bit offsets")
    cap = ops.roi_max_lanes()
    if hi > lo and n_lanes.max() > cap:
        b = int(np.argmax(n_lanes))
        raise L.LgcnError("generate_lane_roi: scene %d has %d lanes, the lane-RoI kernels take at most %d" % (lo + b, n_lanes[b], cap))
    def rows(x, tab):         # rows of the range; the RoI kernels read 16-byte vectors, so a slice off that grid is copied
        x = x[int(tab[lo]):int(tab[hi])]
        return x if x.data_ptr() % 16 == 0 else x.clone()
    nodes, actors = (lambda x: rows(x, store.node_off)), (lambda x: rows(x, store.actor_off))
    eo = store.edge_off
    edges = lambda x: torch.cat([x[ro[k] + int(eo[k, lo]):ro[k] + int(eo[k, hi])] for k in order])
    t = dict(ctrs=nodes(a["node_ctrs"]), feats=nodes(a["node_feats"]), turn=nodes(a["turn"]), control=nodes(a["control"]),
             intersect=nodes(a["intersect"]), lane_idcs=nodes(la["lane_idcs"]).to(torch.int32), a_ctrs=actors(a["actor_ctrs"]),
             a_feats=actors(a["actor_feats"])[:, :, :2].contiguous(), a_obs=actors(la["obs"])[:, :, :2].contiguous(),
             suc_pairs=rows(la["suc_pairs"], la["suc_off"]).to(torch.int32),
             pre_pairs=rows(la["pre_pairs"], la["pre_off"]).to(torch.int32),
             edge_u=edges(a["edge_u"]), edge_v=edges(a["edge_v"]))
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


# ------------------------------------------------------------------ the resident RoI store
_I32_MAX = 2 ** 31 - 1
_ROI_TABLES = ("first_roi", "node_off", "edge_off", "sizes", "agent_vel", "edge_cnt", "agent_ids")


def _csum(x):
    return np.concatenate([[0], np.cumsum(x, dtype=np.int64)])


def roi_store_tables(n_scenes, sizes, scene_of, agent_ids, agent_vel, edge_cnt):
    """Host tables of a RoiStore over n_scenes scenes from the per-RoI tables of an extraction (RoIs in scene order):
    first_roi, node_off [S + 1] (first RoI / first node row of every scene), edge_off [15, S + 1] (per relation, then a2m:
    prefix sums of the scenes' edges), and the per-RoI sizes [R], agent_vel [R] fp32, edge_cnt [R, 15], agent_ids [R]
    (scene-local id of the RoI's agent).  A scene may hold 0 RoIs.  Plain numpy; needs no GPU."""
    K = ops.ROI_REL + 1
    sizes, scene_of, agent_ids = (np.asarray(x, np.int64).reshape(-1) for x in (sizes, scene_of, agent_ids))
    edge_cnt = np.asarray(edge_cnt, np.int64).reshape(-1, K)
    R, S = len(sizes), int(n_scenes)
    if not (len(scene_of) == len(agent_ids) == len(edge_cnt) == len(np.asarray(agent_vel).reshape(-1)) == R):
        raise L.LgcnError("RoiStore: the per-RoI tables must have one length")
    if R and (scene_of.min() < 0 or scene_of.max() >= S or (np.diff(scene_of) < 0).any()):
        raise L.LgcnError("RoiStore: RoIs out of scene order, or of a scene outside the store")
    first_roi = _csum(np.bincount(scene_of, minlength=S))
    node_off = _csum(sizes)[first_roi]
    ends = np.concatenate([np.zeros((1, K), np.int64), np.cumsum(edge_cnt, 0, dtype=np.int64)])[first_roi]      # [S + 1, 15]
    return dict(first_roi=first_roi, node_off=node_off, edge_off=np.ascontiguousarray(ends.T), sizes=sizes,
                agent_vel=np.ascontiguousarray(agent_vel, np.float32).reshape(-1), edge_cnt=edge_cnt, agent_ids=agent_ids)


class RoiPlan:
    """Everything of one pick of a RoiStore that is not a device array: the table lgcn_roi_store_gather reads
    (include/lgcn.h: node_off, roi_off [B + 1], node_src, roi_src [B], seg_off [30 B + 1], seg_src [30 B], int64), the
    totals, and the host tables of the pick's RoiBatch."""

    def __init__(self, **kw):
        self.__dict__.update(kw)


def plan_roi_batch(tables, indices) -> RoiPlan:
    """Host half of RoiStore.batch: from a store's tables (a dict or anything that holds them as attributes) and the picked
    scenes to a RoiPlan.  Repeats and any order are allowed.  Vectorised numpy over the tables; needs no GPU.  LgcnError
    for an empty pick, an index outside the store, a picked scene without an RoI (naming the scene) and totals beyond
    2^31 - 1."""
    get = (lambda k: tables[k]) if isinstance(tables, dict) or hasattr(tables, "files") else (lambda k: getattr(tables, k))
    first_roi, node_off, edge_off = (np.asarray(get(k), np.int64) for k in ("first_roi", "node_off", "edge_off"))
    K, Q = ops.ROI_REL, ops.ROI_STORE_SEGS
    idx = np.asarray(indices)
    if idx.size == 0:
        raise L.LgcnError("RoiStore: an empty pick has no batch")
    if idx.ndim != 1 or idx.dtype.kind not in "iu":
        raise L.LgcnError("RoiStore: indices must be a flat sequence of integers")
    idx = idx.astype(np.int64, copy=False)
    S = len(first_roi) - 1
    if int(idx.min()) < 0 or int(idx.max()) >= S:
        raise L.LgcnError("RoiStore: scene index outside [0, %d)" % S)
    roi_src, node_src = first_roi[idx], node_off[idx]
    n_roi, n_node = first_roi[idx + 1] - roi_src, node_off[idx + 1] - node_src
    if (n_roi == 0).any():
        raise L.LgcnError("RoiStore: scene %d has no lane RoI (every agent dropped)" % int(idx[np.flatnonzero(n_roi == 0)[0]]))
    B = len(idx)
    G = Q * B
    if B > _I32_MAX // 64:
        raise L.LgcnError("RoiStore: a pick of %d scenes is past 32-bit offsets" % B)
    lo = edge_off[:, idx]                                               # [15, B]
    seg_len = edge_off[:, idx + 1] - lo
    rel_at = np.concatenate([_csum(edge_off[:K, -1])[:K], [0]])         # where a relation starts in edge_u; a2m has its own arrays
    seg_src = lo + rel_at[:, None]
    runs = [slice(0, K), slice(0, K), slice(K, K + 1), slice(K, K + 1)]             # u, v, a2m_u, a2m_v
    tab = np.empty(4 * B + 2 * G + 3, np.int64)
    t_node_off, t_roi_off = tab[:B + 1], tab[B + 1:2 * B + 2]
    tab[2 * B + 2:3 * B + 2], tab[3 * B + 2:4 * B + 2] = node_src, roi_src
    t_seg_off, t_seg_src = tab[4 * B + 2:4 * B + G + 3], tab[4 * B + G + 3:]
    t_node_off[0] = t_roi_off[0] = t_seg_off[0] = 0
    np.cumsum(n_node, out=t_node_off[1:])
    np.cumsum(n_roi, out=t_roi_off[1:])
    np.cumsum(np.concatenate([seg_len[r] for r in runs]).reshape(-1), out=t_seg_off[1:])
    t_seg_src[:] = np.concatenate([seg_src[r] for r in runs]).reshape(-1)
    n_nodes, n_rois, n_elem = int(t_node_off[-1]), int(t_roi_off[-1]), int(t_seg_off[-1])
    if 2 * n_nodes > _I32_MAX or 81 * n_rois > _I32_MAX or n_elem > _I32_MAX:
        raise L.LgcnError("RoiStore: a batch of %d nodes, %d RoIs and %d index elements is past 32-bit offsets"
                          % (n_nodes, n_rois, n_elem))
    pick = np.repeat(roi_src - t_roi_off[:-1], n_roi) + np.arange(n_rois, dtype=np.int64)         # the store's RoI of every output RoI
    rel_ext = _csum(seg_len[:K].sum(1))
    return RoiPlan(n_scenes=B, n_nodes=n_nodes, n_rois=n_rois, n_edges=int(rel_ext[-1]), n_a2m=int(seg_len[K].sum()),
                   n_elem=n_elem, table=tab, first_roi=t_roi_off.copy(), rois_per_scene=n_roi, rel_ext=rel_ext,
                   scene_of=np.repeat(np.arange(B, dtype=np.int64), n_roi), sizes=np.asarray(get("sizes"), np.int64)[pick],
                   agent_vel=np.asarray(get("agent_vel"), np.float32)[pick], edge_cnt=np.asarray(get("edge_cnt"), np.int64)[pick],
                   agent_ids=np.asarray(get("agent_ids"), np.int64)[pick])


def merge_roi_tables(parts) -> dict:
    """Host half of RoiStore.concat: the tables of the store that holds the scenes of `parts` (RoiStores, dicts or loaded
    `.npz` with the tables of roi_store_tables) in part order, and the runs that merge the parts' edge_u (or edge_v)
    relation-major: seg_part, seg_at, seg_len [14 * P] in the order (relation, part).  LgcnError for an empty list."""
    parts = list(parts)
    if not parts:
        raise L.LgcnError("RoiStore: concat of an empty list")
    get = lambda p, k: p[k] if isinstance(p, dict) or hasattr(p, "files") else getattr(p, k)
    i64 = lambda p, k: np.asarray(get(p, k), np.int64)
    K, P = ops.ROI_REL, len(parts)
    ends = {k: np.stack([i64(p, k)[..., -1] for p in parts]) for k in ("first_roi", "node_off", "edge_off")}     # [P] / [P, 15]
    bases = {k: np.cumsum(v, 0) - v for k, v in ends.items()}
    chain = lambda k: np.concatenate([[0]] + [i64(p, k)[1:] + base for p, base in zip(parts, bases[k])])
    edge_off = np.concatenate([np.zeros((K + 1, 1), np.int64)] + [i64(p, "edge_off")[:, 1:] + b[:, None]
                                                                 for p, b in zip(parts, bases["edge_off"])], 1)
    rel = ends["edge_off"][:, :K]                                        # [P, 14]: a part's edges per relation
    at = np.cumsum(rel, 1) - rel                                         # where the relation starts in the part's edge_u
    out = dict(first_roi=chain("first_roi"), node_off=chain("node_off"), edge_off=edge_off,
               sizes=np.concatenate([i64(p, "sizes") for p in parts]),
               agent_vel=np.concatenate([np.asarray(get(p, "agent_vel"), np.float32).reshape(-1) for p in parts]),
               edge_cnt=np.concatenate([i64(p, "edge_cnt").reshape(-1, K + 1) for p in parts]),
               agent_ids=np.concatenate([i64(p, "agent_ids") for p in parts]))
    out.update(seg_part=np.tile(np.arange(P, dtype=np.int64), K), seg_at=np.ascontiguousarray(at.T).reshape(-1),
               seg_len=np.ascontiguousarray(rel.T).reshape(-1))
    return out


class RoiStore:
    """The lane RoIs of a split, extracted ONCE and resident in device memory: `batch(indices)` hands the RoiBatch (and
    the per-RoI agent rows) of any pick of scenes to lanercnn.Net from one small table upload and ONE launch
    (ops.roi_store_gather), on the current stream, without a synchronisation or a device -> host read.

    Device (ops.RoiStoreJob): feats [T, 8], node_mask [T] int32, agent_feat [R, 80]; edge_u, edge_v [E] int32,
    relation-major (pre 0..5, suc 0..5, left, right) with the scenes back to back inside a relation; a2m_u, a2m_v [M]
    int32; per RoI the rows of its agent: ctrs [R, 2], actor_feats, obs [R, 20, 3] and, both or neither, gt_preds
    [R, 30, 2], has_preds [R, 30].  All indices are SCENE-LOCAL (row within the block of the scene's RoI nodes; a2m_u: the
    RoI's number within the scene), so a gather is a copy plus one base per picked scene, and concat re-extracts nothing.
    Host (numpy): the tables of roi_store_tables.  A scene none of whose agents keeps an RoI is in the store with 0 RoIs;
    it cannot be picked (`usable()` lists the scenes that can)."""

    # -------------------------------------------------------------- building
    @classmethod
    def from_arrays(cls, arrays, tables):
        """A store over device tensors that already exist (nothing is copied) and the host tables that describe them."""
        self = object.__new__(cls)
        i64 = lambda x: np.ascontiguousarray(x, np.int64)
        self.first_roi, self.node_off, self.edge_off = i64(tables["first_roi"]), i64(tables["node_off"]), i64(tables["edge_off"])
        self.sizes, self.agent_ids = i64(tables["sizes"]).reshape(-1), i64(tables["agent_ids"]).reshape(-1)
        self.edge_cnt = i64(tables["edge_cnt"]).reshape(-1, ops.ROI_REL + 1)
        self.agent_vel = np.ascontiguousarray(tables["agent_vel"], np.float32).reshape(-1)
        self.n_scenes = len(self.first_roi) - 1
        arrays = dict(arrays)
        if "has_preds" in arrays and arrays["has_preds"].dtype == torch.bool:
            arrays["has_preds"] = arrays["has_preds"].view(torch.uint8)
        self._job = job = ops.RoiStoreJob(arrays, self.n_scenes)
        self.device, self.nbytes, p, K = job.device, job.nbytes, job.p, ops.ROI_REL
        R = len(self.sizes)
        if self.n_scenes < 0 or self.node_off.shape != (self.n_scenes + 1,) or self.edge_off.shape != (K + 1, self.n_scenes + 1) \
                or not (len(self.agent_ids) == len(self.edge_cnt) == len(self.agent_vel) == R) \
                or int(self.first_roi[-1]) != R or p.n_rois != R or int(self.node_off[-1]) != p.n_nodes \
                or int(self.sizes.sum()) != p.n_nodes or int(self.edge_off[:K, -1].sum()) != p.n_edges \
                or int(self.edge_off[K, -1]) != p.n_a2m or not np.array_equal(self.edge_cnt.sum(0), self.edge_off[:, -1]):
            raise L.LgcnError("RoiStore: the tables do not describe the arrays")
        return self

    @classmethod
    def from_inputs(cls, t, off, horizon_buffer=20., rows=None):
        """The store of the scenes that (t, off) describe: the inputs of ops.RoiJob / lane_roi_flat, and the launches
        lane_roi_flat runs (one shared body), once.  rows: the scenes' per-agent arrays on the device, concatenated in
        scene order -- ctrs [A, 2], feats [A, 20, 3], obs_trajs [A, 20, 3] and, both or neither, gt_preds [A, 30, 2],
        has_preds [A, 30] -- of which the store keeps the rows of the agents that keep an RoI.  rows=None: only what `t`
        holds can be kept -- ctrs, and the (x, y) columns of feats / obs_trajs with the third column (the step flag,
        which the RoI kernels do not read) zero; no gt.  Results, checks and messages are lane_roi_flat's, but for a scene
        none of whose agents keeps an RoI, which is recorded as holding 0 RoIs."""
        if not torch.cuda.is_available():
            raise L.LgcnError("data_lrcnn.RoiStore needs a GPU (the lane-RoI kernels have no CPU fallback)")
        feats, node_mask, agent_feat, u, v, a2m_u, a2m_v, sizes, scene_of, valid, agent_off, vel, _, cnt = \
            _roi_extract(t, off, horizon_buffer, True)
        S, K, dev = len(agent_off) - 1, ops.ROI_REL, feats.device
        tb = roi_store_tables(S, sizes, scene_of, valid - agent_off[scene_of], vel, cnt)
        # merged-graph indices -> scene-local: one subtraction per array, the owner's base from the host tables
        node_base, roi_base = tb["node_off"][scene_of], tb["first_roi"][scene_of]              # per RoI: its scene's bases
        rel_cnt, a2m_cnt = np.ascontiguousarray(cnt[:, :K].T).reshape(-1), cnt[:, K]
        owner = np.concatenate([np.repeat(np.tile(node_base, K), rel_cnt), np.repeat(node_base, a2m_cnt), np.repeat(roi_base, a2m_cnt)])
        owner = torch.from_numpy(owner).to(dev)
        E, M = int(rel_cnt.sum()), int(a2m_cnt.sum())
        arrays = dict(feats=feats, node_mask=node_mask.to(torch.int32), agent_feat=agent_feat,
                      edge_u=(u - owner[:E]).to(torch.int32), edge_v=(v - owner[:E]).to(torch.int32),
                      a2m_u=(a2m_u - owner[E + M:]).to(torch.int32), a2m_v=(a2m_v - owner[E:E + M]).to(torch.int32))
        keep = torch.from_numpy(np.ascontiguousarray(valid, np.int64)).to(dev)
        if rows is None:
            pad = lambda x: torch.cat([x, torch.zeros_like(x[:, :, :1])], 2)
            rows = dict(ctrs=t["a_ctrs"], feats=pad(t["a_feats"]), obs_trajs=pad(t["a_obs"]))
        if ("gt_preds" in rows) != ("has_preds" in rows):
            raise L.LgcnError("RoiStore: gt_preds and has_preds come together")
        names = dict(ctrs="ctrs", actor_feats="feats", obs="obs_trajs", gt_preds="gt_preds", has_preds="has_preds")
        for k, src in names.items():
            if src in rows:
                x = rows[src]
                if not (torch.is_tensor(x) and x.is_cuda) or x.shape[0] != int(agent_off[-1]):
                    raise L.LgcnError("RoiStore: rows[%r] must be a device tensor with one row per agent" % src)
                x = x.view(torch.uint8) if x.dtype == torch.bool else x
                arrays[k] = x.index_select(0, keep).contiguous()
        return cls.from_arrays(arrays, tb)

    @classmethod
    def from_store(cls, store, horizon_buffer=20., chunk=None):
        """The store of all scenes of a flatfile.DeviceSceneStore that data_raw.build_store(..., lanes=True) made
        (store_roi_inputs); the per-RoI agent rows come from the store's own tensors.  chunk: scenes per extraction pass,
        which bounds the workspace of lgcn_roi_search; the parts are merged by concat.  None: one pass."""
        S = len(store)
        if S == 0:
            raise L.LgcnError("lane_roi_flat: no scene in the batch")
        chunk = S if chunk is None else int(chunk)
        if chunk < 1:
            raise L.LgcnError("RoiStore.from_store: chunk must be positive")
        la, a, parts = getattr(store, "lane_arrays", None), store._job.t, []
        for lo in range(0, S, chunk):
            hi = min(S, lo + chunk)
            t, off = store_roi_inputs(store, (lo, hi))
            cut = lambda x: x[int(store.actor_off[lo]):int(store.actor_off[hi])]
            rows = dict(ctrs=cut(a["actor_ctrs"]), feats=cut(a["actor_feats"]), obs_trajs=cut(la["obs"]))
            if store.has_gt:
                rows.update(gt_preds=cut(a["gt_preds"]), has_preds=cut(a["has_preds"]))
            with torch.cuda.device(store.device):
                parts.append(cls.from_inputs(t, off, horizon_buffer, rows))
        return parts[0] if len(parts) == 1 else cls.concat(parts)

    @classmethod
    def concat(cls, stores):
        """One store that holds the scenes of `stores` in part order: the store of all those scenes extracted at once.
        The relation-major edge arrays are merged by ONE ops.store_pack launch over P x 2 x 14 runs, every other array by
        one concatenation, the tables on the host (merge_roi_tables).  LgcnError, before any launch: an empty list,
        parts on different devices, or that differ in having gt_preds."""
        stores = list(stores)
        if not stores:
            raise L.LgcnError("RoiStore: concat of an empty list")
        if len({str(s.device) for s in stores}) != 1:
            raise L.LgcnError("RoiStore: concat of parts on different devices")
        if len({bool(s.has_gt) for s in stores}) != 1:
            raise L.LgcnError("RoiStore: concat of parts with and without gt_preds")
        m = merge_roi_tables(stores)
        P, dev = len(stores), stores[0].device
        parts = [s._job.t for s in stores]
        with torch.cuda.device(dev):
            arrays = {k: torch.cat([t[k] for t in parts]) for k in parts[0] if k not in ("edge_u", "edge_v")}
            E = int(m["seg_len"].sum())
            edges = torch.empty(2 * E, dtype=torch.int32, device=dev)
            ops.store_pack([t["edge_u"] for t in parts] + [t["edge_v"] for t in parts],
                           np.concatenate([m["seg_part"], m["seg_part"] + P]), np.tile(m["seg_at"], 2), np.tile(m["seg_len"], 2), edges)
        arrays["edge_u"], arrays["edge_v"] = edges[:E], edges[E:]
        return cls.from_arrays(arrays, m)

    # -------------------------------------------------------------- the file
    def save(self, path: str) -> None:
        """Write the store as a plain `.npz` of its arrays and tables (one device -> host copy per array)."""
        out = {k: getattr(self, k) for k in _ROI_TABLES}
        for k, v in self._job.t.items():
            out[k] = v.cpu().numpy()
        if "has_preds" in out:
            out["has_preds"] = out["has_preds"].view(bool)
        np.savez(path, **out)

    @classmethod
    def load(cls, path: str, device=None):
        """The store that save() wrote, resident on `device` (None: the current one).  load followed by save reproduces the
        file's arrays byte for byte."""
        if not torch.cuda.is_available():
            raise L.LgcnError("data_lrcnn.RoiStore needs a GPU (the HIP hot path has no CPU fallback)")
        dev = torch.device("cuda" if device is None else device)
        if dev.index is None:
            dev = torch.device(dev.type, torch.cuda.current_device())
        with np.load(path) as f:
            tables = {k: f[k] for k in _ROI_TABLES}
            host = {k: np.ascontiguousarray(f[k]) for k in f.files if k not in _ROI_TABLES}
        if "has_preds" in host:
            host["has_preds"] = host["has_preds"].view(np.uint8)
        self = cls.from_arrays({k: torch.from_numpy(v).to(dev) for k, v in host.items()}, tables)
        torch.cuda.synchronize(dev)              # resident before any stream reads it
        return self

    # -------------------------------------------------------------- reading
    def __len__(self):
        return self.n_scenes

    @property
    def has_gt(self) -> bool:
        return self._job.has_gt

    @property
    def n_rois(self) -> int:
        return len(self.sizes)

    @property
    def rois_per_scene(self) -> np.ndarray:
        return np.diff(self.first_roi)

    def usable(self) -> np.ndarray:
        """The scenes that hold at least one RoI -- the ones a sampler may pick."""
        return np.flatnonzero(self.rois_per_scene > 0)

    def plan(self, indices) -> RoiPlan:
        return plan_roi_batch(self, indices)

    def batch(self, indices, plan: RoiPlan = None):
        """-> (RoiBatch, rows) of the picked scenes, as lane_roi_flat gives the RoiBatch for those scenes alone, but for
        agents = arange(R') and agent_off = first_roi' (the rows hold the kept agents only, so valid_agent_ids(b) is
        arange(R_b)).  rows: the gathered per-RoI agent arrays ctrs [R', 2], feats, obs_trajs [R', 20, 3] and, if the store
        has them, gt_preds [R', 30, 2], has_preds [R', 30] bool; and agent_ids, per picked scene the original scene-local
        ids (int16) of its kept agents.  One table upload from pinned memory and one launch on the current stream; no
        synchronisation, no device -> host read.  `plan`: this pick's plan(), if the caller already has it."""
        p = self.plan(indices) if plan is None else plan
        T, R, dev = p.n_nodes, p.n_rois, self.device
        f32, i64 = torch.float32, torch.int64
        with torch.cuda.device(dev):
            stage = torch.empty(p.table.size, dtype=i64, pin_memory=True)          # staging of its own, as DeviceSceneStore.batch
            stage.numpy()[:] = p.table
            tab_dev = torch.empty(p.table.size, dtype=i64, device=dev)
            tab_dev.copy_(stage, non_blocking=True)
            new = lambda shape, dt: torch.empty(shape, dtype=dt, device=dev)
            out = dict(feats=new((T, 8), f32), node_mask=new((T,), i64), agent_feat=new((R, 80), f32), idx=new((p.n_elem,), i64),
                       ctrs=new((R, 2), f32), actor_feats=new((R, 20, 3), f32), obs=new((R, 20, 3), f32))
            if self.has_gt:
                out.update(gt_preds=new((R, 30, 2), f32), has_preds=new((R, 30), torch.bool))
            ops.roi_store_gather(self._job, stage, tab_dev, p.n_scenes, T, R, p.n_elem, out)
        E, M, idx = p.n_edges, p.n_a2m, out["idx"]
        rb = RoiBatch(out["feats"], out["node_mask"], out["agent_feat"], idx[:E], idx[E:2 * E], idx[2 * E:2 * E + M],
                      idx[2 * E + M:], p.sizes, p.scene_of, np.arange(R, dtype=np.int64), p.first_roi, p.agent_vel, p.rel_ext,
                      p.edge_cnt)
        rows = dict(ctrs=out["ctrs"], feats=out["actor_feats"], obs_trajs=out["obs"],
                    agent_ids=np.split(p.agent_ids.astype(np.int16), p.first_roi[1:-1]))
        if self.has_gt:
            rows.update(gt_preds=out["gt_preds"], has_preds=out["has_preds"])
        return rb, rows
