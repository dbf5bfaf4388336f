"""Front end of the data path: raw tracks and map lanes to scenes, on the device for a whole batch (csrc/lgcn_scene.hip,
and with batched=True csrc/lgcn_graphbatch.hip for the dilated scales and left / right).  The
reference does this per scene in Python: ArgoDataset.get_obj_feats (data.py:148-217) and ArgoDataset.get_lane_graph
(data.py:220-361).  build_scenes returns scene dicts; build_store packs the same batch straight into a resident
flatfile.DeviceSceneStore (one more launch, no scene dicts, nothing through the host).

Neither routine needs argoverse-api once its inputs are plain arrays:
  a raw scene   {"city", "trajs": [[n_i,2] float64], "steps": [[n_i] int64]}, the agent first: what the reference's
                read_argo_data returns (that reader itself stays out of scope);
  a LaneTable   one city's lanes as flat arrays, built once from any {lane_id: lane} mapping whose lanes carry the
                attributes get_lane_graph reads (argoverse-api users pass am.city_lane_centerlines_dict[city]) and
                uploaded once with .to(device).

The module needs a GPU (no CPU fallback), like its neighbours."""
import numpy as np
import torch

from . import _lib as L
from . import ops
from . import preprocess_data

OBS, FUT = 20, 30


class LaneTable:
    """One city's lanes as flat arrays (host numpy; .to(device) adds the device copies the kernels read):
      lane_id [L] int64, unique;  pt_off [L + 1], pts [P,2] float64, world frame (every lane >= 2 points);
      turn [L] int8 (0 none, 1 LEFT, 2 RIGHT), control, intersect [L] uint8;
      pred_off [L + 1] / pred, succ_off [L + 1] / succ: neighbours as table rows, -1 where the id is not in the table, in
      the reference's list order, duplicates included;  left, right [L]: table rows or -1."""

    def __init__(self, lane_id, pt_off, pts, turn, control, intersect, pred_off, pred, succ_off, succ, left, right):
        i32 = lambda x: np.ascontiguousarray(x, np.int32).reshape(-1)
        self.lane_id = np.ascontiguousarray(lane_id, np.int64).reshape(-1)
        self.pt_off, self.pts = i32(pt_off), np.ascontiguousarray(pts, np.float64).reshape(-1, 2)
        self.turn = np.ascontiguousarray(turn, np.int8).reshape(-1)
        self.control = np.ascontiguousarray(control, np.uint8).reshape(-1)
        self.intersect = np.ascontiguousarray(intersect, np.uint8).reshape(-1)
        self.pred_off, self.pred, self.succ_off, self.succ = i32(pred_off), i32(pred), i32(succ_off), i32(succ)
        self.left, self.right = i32(left), i32(right)
        n = self.n_lanes = len(self.lane_id)
        self.n_pts, self.n_pred, self.n_succ = len(self.pts), len(self.pred), len(self.succ)
        if len(np.unique(self.lane_id)) != n:
            raise L.LgcnError("LaneTable: duplicate lane ids")
        for name, arr, size in (("pt_off", self.pt_off, n + 1), ("pred_off", self.pred_off, n + 1),
                                ("succ_off", self.succ_off, n + 1), ("turn", self.turn, n), ("control", self.control, n),
                                ("intersect", self.intersect, n), ("left", self.left, n), ("right", self.right, n)):
            if len(arr) != size:
                raise L.LgcnError("LaneTable: %s must hold %d entries, got %d" % (name, size, len(arr)))
        if n and int(np.diff(self.pt_off).min()) < 2:
            raise L.LgcnError("LaneTable: lane %d has fewer than 2 points" % int(self.lane_id[int(np.diff(self.pt_off).argmin())]))
        if not np.isfinite(self.pts).all():
            raise L.LgcnError("LaneTable: a centerline holds a non-finite coordinate")
        flags = self.turn.astype(np.int32) | (self.control.astype(np.int32) != 0) << 8 | (self.intersect.astype(np.int32) != 0) << 16
        # the int32 block of include/lgcn.h (lgcn_lane_table_t); the library validates it before every launch
        self.topo_host = np.ascontiguousarray(np.concatenate([self.pt_off, self.pred_off, self.succ_off, self.left, self.right,
                                                              flags.astype(np.int32), self.pred, self.succ]).astype(np.int32))
        self._row = None
        self.topo_dev = self.pts_dev = None

    @classmethod
    def from_lanes(cls, mapping):
        """The table of {lane_id: lane}; a lane needs centerline [n,>=2], turn_direction, has_traffic_control,
        is_intersection, predecessors, successors (lists or None), l_neighbor_id, r_neighbor_id (an id or None)."""
        ids = list(mapping.keys())
        if len(set(ids)) != len(ids):
            raise L.LgcnError("LaneTable: duplicate lane ids")
        row = {k: i for i, k in enumerate(ids)}
        pts, pt_off, pred, pred_off, succ, succ_off = [], [0], [], [0], [], [0]
        turn, control, intersect, left, right = [], [], [], [], []
        for k in ids:
            lane = mapping[k]
            c = np.asarray(lane.centerline, np.float64)
            if c.ndim != 2 or c.shape[0] < 2 or c.shape[1] < 2:
                raise L.LgcnError("LaneTable: lane %s has fewer than 2 points" % (k,))
            pts.append(c[:, :2])
            pt_off.append(pt_off[-1] + len(c))
            pred += [row.get(x, -1) for x in (lane.predecessors if lane.predecessors is not None else [])]
            succ += [row.get(x, -1) for x in (lane.successors if lane.successors is not None else [])]
            pred_off.append(len(pred))
            succ_off.append(len(succ))
            turn.append({"LEFT": 1, "RIGHT": 2}.get(lane.turn_direction, 0))
            control.append(bool(lane.has_traffic_control))
            intersect.append(bool(lane.is_intersection))
            left.append(row.get(lane.l_neighbor_id, -1) if lane.l_neighbor_id is not None else -1)
            right.append(row.get(lane.r_neighbor_id, -1) if lane.r_neighbor_id is not None else -1)
        pts = np.concatenate(pts, 0) if pts else np.zeros((0, 2))
        return cls(np.asarray(ids, np.int64), pt_off, pts, turn, control, intersect, pred_off, pred, succ_off, succ, left, right)

    def to(self, device):
        """This table with its arrays uploaded to `device` (one copy each; the host arrays are shared)."""
        out = object.__new__(LaneTable)
        out.__dict__.update(self.__dict__)
        out.topo_dev = torch.from_numpy(self.topo_host).to(device)
        out.pts_dev = torch.from_numpy(self.pts).to(device)
        return out

    def rows(self, lane_ids):
        """Table rows of a list of lane ids (LgcnError for an id that is not in the table or is listed twice)."""
        if self._row is None:
            self._row = {int(k): i for i, k in enumerate(self.lane_id.tolist())}
        try:
            rows = np.asarray([self._row[int(k)] for k in lane_ids], np.int32)
        except KeyError as e:
            raise L.LgcnError("lane id %s is not in the lane table" % (e.args[0],))
        if len(np.unique(rows)) != len(rows):
            raise L.LgcnError("lane_ids lists a lane twice")
        return rows


def _need_gpu(what):
    if not torch.cuda.is_available():
        raise L.LgcnError("data_raw.%s needs a GPU (the scene kernels have no CPU fallback)" % what)
    return torch.device("cuda", torch.cuda.current_device())


def scene_frames(raws, thetas=None):
    """(orig [B,2] fp32, theta [B] float64, rot [B,2,2] fp32) of raw scenes with the reference's own operations
    (data.py:149-159): orig = the agent's ROW 19 rounded to fp32, theta = pi - atan2 of (row 18 - orig) in float64 unless
    given, rot = cos / sin rounded to fp32.  An agent track of fewer than 20 rows is an LgcnError."""
    B = len(raws)
    a = np.zeros((B, 2, 2), np.float64)
    for b, r in enumerate(raws):
        t0 = np.asarray(r["trajs"][0], np.float64)
        if t0.ndim != 2 or t0.shape[0] < OBS or t0.shape[1] != 2:
            raise L.LgcnError("scene %d: the agent track must hold at least 20 rows of (x, y), got %s" % (b, t0.shape))
        a[b] = t0[OBS - 2:OBS]
    orig = a[:, 1].astype(np.float32)
    pre = a[:, 0] - orig
    theta = np.pi - np.arctan2(pre[:, 1], pre[:, 0])
    if thetas is not None:
        for b, th in enumerate(thetas):
            if th is not None:
                theta[b] = th
    c, s = np.cos(theta), np.sin(theta)
    rot = np.stack([c, -s, s, c], 1).astype(np.float32).reshape(B, 2, 2)
    return orig, theta, rot


def _frame_dev(orig, rot, dev):
    f = np.concatenate([np.asarray(orig, np.float32).reshape(-1, 2), np.asarray(rot, np.float32).reshape(-1, 4)], 1)
    return torch.from_numpy(np.ascontiguousarray(f)).to(dev)


def _csum(sizes):
    return np.concatenate([[0], np.cumsum(np.asarray(sizes, np.int64), dtype=np.int64)])


def _track_job(raws, frame, pred_range, head, dev):
    """The batch's tracks, flat, and their lgcn_scene_tracks job (nothing launched)."""
    trajs, steps, n_trk = [], [], []
    for b, r in enumerate(raws):
        if len(r["trajs"]) != len(r["steps"]) or len(r["trajs"]) == 0:
            raise L.LgcnError("scene %d: trajs and steps must list the same tracks, the agent first" % b)
        for k, (xy, st) in enumerate(zip(r["trajs"], r["steps"])):
            xy, st = np.asarray(xy, np.float64), np.asarray(st, np.int64).reshape(-1)
            if xy.shape != (len(st), 2):
                raise L.LgcnError("scene %d track %d: trajs must be [n,2] and steps [n]" % (b, k))
            trajs.append(xy)
            steps.append(st)
        n_trk.append(len(r["trajs"]))
    step = np.concatenate(steps)
    if len(step) and step.min() < 0:
        raise L.LgcnError("a track lists a negative step")
    off = np.concatenate([_csum(n_trk), _csum([len(s) for s in steps])])
    xy = torch.from_numpy(np.ascontiguousarray(np.concatenate(trajs, 0))).to(dev)
    step = torch.from_numpy(np.minimum(step, OBS + FUT).astype(np.int32)).to(dev)
    return ops.SceneTracksJob(xy, step, frame, off, pred_range, head), off[:len(n_trk) + 1]


def _track_status(job, head, trk_off):
    """Per-scene output offsets of the kept tracks from the read-back head; LgcnError for a repeated step."""
    S, T = job.S, job.T
    if head[S + 1]:
        t = T - int(head[S + 1])
        b = int(np.searchsorted(trk_off, t, side="right")) - 1
        raise L.LgcnError("scene %d track %d lists a step twice" % (b, t - int(trk_off[b])))
    return head[:S + 1].astype(np.int64)


def _lane_job(tabs, scene_tab, lane_ids, frame, pred_range, head):
    S = len(scene_tab)
    explicit = lane_ids is not None and any(x is not None for x in lane_ids)
    n_tab = [tabs[i].n_lanes for i in scene_tab]
    if explicit:
        cand = [tabs[i].rows(ids) if ids is not None else np.arange(tabs[i].n_lanes, dtype=np.int32)
                for i, ids in zip(scene_tab, lane_ids)]
        n_cand = [len(c) for c in cand]
    else:
        cand, n_cand = [], n_tab
    for b, n in enumerate(n_cand):
        if n == 0:
            raise L.LgcnError("scene %d: no lane survives (there is no candidate lane)" % b)
    off = np.concatenate([np.asarray(scene_tab, np.int64), _csum(n_cand), _csum(n_tab)] + [np.asarray(c, np.int64) for c in cand])
    return ops.SceneLanesJob(tabs, off, explicit, frame, pred_range, head)


def _lane_fill(job, head, dev):
    """After the first read-back: LgcnError for a scene without a lane, else the fill launches; returns (outputs, head2)."""
    h = head.reshape(job.S + 1, 4).astype(np.int64)
    n_lanes = np.diff(h[:, 0])
    if (n_lanes == 0).any():
        raise L.LgcnError("scene %d: no lane survives the pred_range rectangle" % int(np.flatnonzero(n_lanes == 0)[0]))
    head2 = torch.empty(4 * (job.S + 1), dtype=torch.int32, device=dev)
    return ops.scene_lanes_fill(job, h[-1], head2), head2, h


def _split(x, off, device):
    sizes = np.diff(off).tolist()
    if device:
        return list(x.split(sizes))
    return np.split(x.cpu().numpy(), off[1:-1])


def _cuts(h, h2):
    """Per-scene offsets [S + 1] of the batch's scale-0 edge arrays and pair lists, from the two read-back heads."""
    h2 = h2.reshape(len(h), 4).astype(np.int64)
    chain = h[:, 1] - h[:, 0]
    return dict(pre=chain + h2[:, 0], suc=chain + h2[:, 1], pre_pairs=h2[:, 0], suc_pairs=h2[:, 1], left_pairs=h2[:, 2],
                right_pairs=h2[:, 3])


def _graphs(out, h, h2, device):
    """Per-scene graph dicts (scale 0) cut out of the batch's arrays."""
    S = len(h) - 1
    cuts = _cuts(h, h2)
    used = {k: int(v[-1]) for k, v in cuts.items()}
    parts = {k: _split(out[k], h[:, 1], device) for k in ("ctrs", "feats", "turn", "control", "intersect", "lane_idcs")}
    for k in ("pre", "suc"):
        parts[k + "_u"] = _split(out[k + "_u"][:used[k]], cuts[k], device)
        parts[k + "_v"] = _split(out[k + "_v"][:used[k]], cuts[k], device)
    for k in ("pre_pairs", "suc_pairs", "left_pairs", "right_pairs"):
        parts[k] = _split(out[k][:used[k]], cuts[k], device)
    graphs = []
    for b in range(S):
        g = {k: parts[k][b] for k in ("ctrs", "feats", "turn", "control", "intersect", "lane_idcs", "pre_pairs", "suc_pairs",
                                      "left_pairs", "right_pairs")}
        g["num_nodes"] = int(h[b + 1, 1] - h[b, 1])
        g["pre"] = [{"u": parts["pre_u"][b], "v": parts["pre_v"][b]}]
        g["suc"] = [{"u": parts["suc_u"][b], "v": parts["suc_v"][b]}]
        graphs.append(g)
    return graphs


def _dilate(graph, dev_graph, num_scales, device):
    """Scales 1 .. num_scales - 1 of pre / suc from the existing device op (preprocess_data.dilated_nbrs)."""
    for k in ("pre", "suc"):
        more = preprocess_data.dilated_nbrs(dev_graph[k][0], graph["num_nodes"], num_scales)
        if not device:
            more = [{"u": e["u"].cpu().numpy(), "v": e["v"].cpu().numpy()} for e in more]
        graph[k] = graph[k] + more


def _flat_tail(out, h, h2, num_scales, cross_dist):
    """Scales 1 .. num_scales - 1 of pre / suc and, with cross_dist given, left / right for the whole batch from the flat
    arrays _lane_fill left on the device (ops.dilate_batch, ops.cross_edges_batch): no per-scene call, no concatenation,
    one host read per scale and one for the left / right counts -> (scale 0 as such a scale dict: the used parts of
    pre_u .. suc_v with pre_off / suc_off, the scales above it, (edges, offs) of cross_edges_batch or None)."""
    cuts = _cuts(h, h2)
    flat = lambda k, cut=None: out[k][:int(cuts[cut or k][-1])]      # the used part of an array sized by its upper bound
    first = {"pre_u": flat("pre_u", "pre"), "pre_v": flat("pre_v", "pre"), "suc_u": flat("suc_u", "suc"),
             "suc_v": flat("suc_v", "suc"), "pre_off": cuts["pre"], "suc_off": cuts["suc"]}
    scales = ops.dilate_batch(first["pre_u"], first["pre_v"], first["suc_u"], first["suc_v"], h[:, 1], cuts["pre"], cuts["suc"],
                              num_scales)
    cross = None
    if cross_dist is not None:
        cross = ops.cross_edges_batch(out["ctrs"], out["feats"], out["lane_idcs"], flat("pre_pairs"), flat("suc_pairs"),
                                      flat("left_pairs"), flat("right_pairs"), h[:, 1], h[:, 0], cuts["pre_pairs"],
                                      cuts["suc_pairs"], cuts["left_pairs"], cuts["right_pairs"], cross_dist)
    return first, scales, cross


def _batched_tail(graphs, out, h, h2, num_scales, cross_dist, device):
    """_flat_tail's results cut into the per-scene leaves of `graphs`."""
    _, scales, cross = _flat_tail(out, h, h2, num_scales, cross_dist)
    for sc in scales:
        for k in ("pre", "suc"):
            us, vs = _split(sc[k + "_u"], sc[k + "_off"], device), _split(sc[k + "_v"], sc[k + "_off"], device)
            for g, u, v in zip(graphs, us, vs):
                g[k] = g[k] + [{"u": u, "v": v}]
    if cross is not None:
        for g, side in zip(graphs, preprocess_data.split_cross(cross[0], cross[1], range(len(graphs)), device)):
            g["left"], g["right"] = side["left"], side["right"]


def get_obj_feats(data, config, theta=None):
    """ArgoDataset.get_obj_feats (data.py:148-217) as a function: adds feats, obs_trajs [A,20,3], ctrs [A,2], gt_preds
    [A,30,2] fp32, has_preds [A,30] bool, orig [2] fp32, theta (float64), rot [2,2] fp32 to `data` (numpy leaves) and
    returns it.  theta= replaces the heading-derived angle (the reference's rot_aug branch, the draw left to the caller).
    A step listed twice in one track and an agent track under 20 rows raise LgcnError."""
    dev = _need_gpu("get_obj_feats")
    orig, th, rot = scene_frames([data], None if theta is None else [theta])
    head = torch.zeros(3, dtype=torch.int32, device=dev)
    job, trk_off = _track_job([data], _frame_dev(orig, rot, dev), config["pred_range"], head, dev)
    ops.scene_tracks(job)
    n = int(_track_status(job, head.cpu().numpy(), trk_off)[1])
    data["feats"], data["obs_trajs"] = job.feats[:n].cpu().numpy(), job.obs[:n].cpu().numpy()
    data["ctrs"], data["orig"], data["theta"], data["rot"] = job.ctrs[:n].cpu().numpy(), orig[0], th[0], rot[0]
    data["gt_preds"], data["has_preds"] = job.gt[:n].cpu().numpy(), job.has[:n].cpu().numpy()
    return data


def get_lane_graph(data, table, config, lane_ids=None):
    """ArgoDataset.get_lane_graph (data.py:220-361) as a function of data["orig"], data["rot"] and one LaneTable: the
    reference's graph dict with numpy leaves; pre / suc hold config["num_scales"] entries, the scales above 0 from the
    device's dilated_nbrs (edges sorted by (u, v); scipy fixes no order inside a row).  Candidates are all lanes of the
    table in table order, or lane_ids in its own order (the reference's get_lane_ids_in_xy_bbox is a prefilter: any
    order-preserving superset of the lanes that pass the rectangle test gives the same graph).  A scene in which no lane
    survives raises LgcnError."""
    dev = _need_gpu("get_lane_graph")
    tab = table if table.topo_dev is not None and table.topo_dev.device == dev else table.to(dev)
    head = torch.empty(8, dtype=torch.int32, device=dev)
    job = _lane_job([tab], [0], None if lane_ids is None else [lane_ids], _frame_dev(data["orig"], data["rot"], dev),
                    config["pred_range"], head)
    ops.scene_lanes_rank(job)
    out, head2, h = _lane_fill(job, head.cpu().numpy(), dev)
    h2 = head2.cpu().numpy()
    graph = _graphs(out, h, h2, False)[0]
    _dilate(graph, _graphs(out, h, h2, True)[0], int(config["num_scales"]), False)
    return graph


def _front(raws, tables, config, lane_ids, dev):
    """The front half that build_scenes and build_store share: the frames, the track and lane launches and the two size
    read-backs of a non-empty batch -> (orig, theta, rot on the host, frame [S,6] on the device, the track job, a_off
    [S + 1], the lane fill's flat outputs, h, h2).  Raises the batch's LgcnErrors."""
    S = len(raws)
    orig, theta, rot = scene_frames(raws)
    cities, tabs, scene_tab = {}, [], []
    for r in raws:
        if r["city"] not in cities:
            tb = tables[r["city"]]
            if tb.topo_dev is None or tb.topo_dev.device != dev:
                tb = tables[r["city"]] = tb.to(dev)
            cities[r["city"]] = len(tabs)
            tabs.append(tb)
        scene_tab.append(cities[r["city"]])
    frame = _frame_dev(orig, rot, dev)
    head = torch.zeros((S + 2) + 4 * (S + 1), dtype=torch.int32, device=dev)
    tjob, trk_off = _track_job(raws, frame, config["pred_range"], head[:S + 2], dev)
    ljob = _lane_job(tabs, scene_tab, lane_ids, frame, config["pred_range"], head[S + 2:])
    ops.scene_tracks(tjob)
    ops.scene_lanes_rank(ljob)
    hh = head.cpu().numpy()                                   # read-back 1: kept tracks, status, lanes and nodes
    a_off = _track_status(tjob, hh[:S + 2], trk_off)
    out, head2, h = _lane_fill(ljob, hh[S + 2:], dev)
    h2 = head2.cpu().numpy()                                  # read-back 2: kept neighbours
    return orig, theta, rot, frame, tjob, a_off, out, h, h2


def build_scenes(raws, tables, config, device=True, cross=True, lane_ids=None, batched=False):
    """Raw scenes to scene dicts in the reference's schema, the whole batch at once: the track kernels and the lane
    kernels run once (6 launches, one memset and one zero fill whatever the number of scenes, 2 size read-backs), then per
    scene the existing device ops: preprocess_data.dilated_nbrs for scales 1 .. num_scales - 1 and, with cross=True,
    preprocess_data.preprocess for graph["left"] / graph["right"] (config["cross_dist"], default 6).  batched=True replaces
    the per-scene ops by ops.dilate_batch and ops.cross_edges_batch on the batch's flat arrays: the same leaves from a
    number of launches and host reads (num_scales - 1, plus 1 with cross=True) that does not depend on the number of scenes.

    raws: raw scenes; tables: {city: LaneTable} (uploaded on first use if .to(device) was not called; a batch may mix
    cities); lane_ids: optional per-scene candidate lists (None = the whole table).  Returns new dicts with city, idx (the
    position in the batch), feats, obs_trajs, ctrs, orig, theta, rot, gt_preds, has_preds and graph; leaves are device
    tensors, which data.collate_fn and Net.forward take as they come, or numpy arrays with device=False.  num_nodes is an
    int and theta a float.  Errors (LgcnError, nothing launched afterwards): an agent track under 20 rows (before any
    launch), a step listed twice in a track, a scene in which no lane survives."""
    dev = _need_gpu("build_scenes")
    raws = list(raws)
    S = len(raws)
    if S == 0:
        return []
    orig, theta, rot, frame, tjob, a_off, out, h, h2 = _front(raws, tables, config, lane_ids, dev)
    n_a = int(a_off[-1])
    actors = {k: _split(v[:n_a], a_off, device) for k, v in (("feats", tjob.feats), ("obs_trajs", tjob.obs), ("ctrs", tjob.ctrs),
                                                             ("gt_preds", tjob.gt), ("has_preds", tjob.has))}
    graphs = _graphs(out, h, h2, device)
    cross_dist = float(config.get("cross_dist", 6.0))
    if batched:
        _batched_tail(graphs, out, h, h2, int(config["num_scales"]), cross_dist if cross else None, device)
    else:
        dev_graphs = graphs if device else _graphs(out, h, h2, True)
    if device:
        orig_l, rot_l = frame[:, :2].unbind(0), frame[:, 2:].reshape(S, 2, 2).unbind(0)
    else:
        orig_l, rot_l = list(orig), list(rot)
    scenes = []
    for b, r in enumerate(raws):
        g = graphs[b]
        if not batched:
            dg = dev_graphs[b]
            _dilate(g, dg, int(config["num_scales"]), device)
            if cross:
                side = preprocess_data.preprocess(dict(dg, idx=b), cross_dist)
                for k in ("left", "right"):
                    g[k] = {c: torch.from_numpy(side[k][c]).to(dev) for c in "uv"} if device else side[k]
        s = {"city": r["city"], "idx": b, "orig": orig_l[b], "theta": float(theta[b]), "rot": rot_l[b], "graph": g}
        s.update({k: v[b] for k, v in actors.items()})
        scenes.append(s)
    return scenes


def build_store(raws, tables, config, lane_ids=None, lanes=False):
    """Raw scenes to a flatfile.DeviceSceneStore that holds them, without leaving the device: the launches and host
    reads of build_scenes(..., device=True, cross=True, batched=True) (2 size read-backs, ops.read_back num_scales - 1
    times for the dilation and once for left / right) and then ONE more launch, ops.store_pack, which writes the store's
    int32 relation-major edge_u / edge_v from the builder's flat edge arrays and rot / orig from the frame rows.  No scene
    dict and no per-scene view is made: inside one relation the builder's flat arrays already hold the scenes back to
    back, as the store wants them, so a relation's u (or v) is one run, and the node and actor arrays are the builder's
    own tensors, adopted as they are (the actor arrays as the first n_a rows of tensors sized for every track).
    The offset tables come from the tables the builder already holds, theta from scene_frames.

    The store equals DeviceSceneStore(path) after write_scenes(path, build_scenes(..., device=False), theta=True), byte for
    byte; plan, batch (with and without rot_dt), Net.forward_store*, evaluate_store, concat and save work on it.
    raws, tables, lane_ids and the errors: as build_scenes; an empty batch is an LgcnError.

    lanes=True also keeps, as the plain attribute store.lane_arrays (never saved, like scene_city), what the fork's lane-RoI
    extraction reads beyond the store's own arrays, all of it the builder's flat tensors as they are: lane_idcs [N] int64
    (scene-local lane of every node), suc_pairs / pre_pairs [P, 2] int64 (scene-local lane pairs, the used part) with their
    per-scene offsets suc_off / pre_off [S + 1], lane_off [S + 1] (lanes per scene) and obs [A, 20, 3] (obs_trajs of the
    kept tracks).  The store's arrays and tables are the same bytes either way."""
    from .flatfile import DeviceSceneStore
    dev = _need_gpu("build_store")
    raws = list(raws)
    S = len(raws)
    if S == 0:
        raise L.LgcnError("build_store: no scene to build a store from")
    _, theta, _, frame, tjob, a_off, out, h, h2 = _front(raws, tables, config, lane_ids, dev)
    num_scales = int(config["num_scales"])
    first, scales, (edges, offs) = _flat_tail(out, h, h2, num_scales, float(config.get("cross_dist", 6.0)))
    # the store's relations in its order: pre0, suc0, pre1, ..., left, right
    rels = [{"u": sc[k + "_u"], "v": sc[k + "_v"], "off": sc[k + "_off"]} for sc in [first] + scales for k in ("pre", "suc")]
    rels += [{"u": edges[k + "_u"], "v": edges[k + "_v"], "off": offs[k + "_off"]} for k in ("left", "right")]
    R = len(rels)
    edge_off = np.stack([np.asarray(r["off"], np.int64) for r in rels])
    rel_off = _csum(edge_off[:, -1])
    E = int(rel_off[-1])
    packed = torch.empty(2 * E, dtype=torch.int32, device=dev)
    rot, orig = torch.empty((S, 2, 2), dtype=torch.float32, device=dev), torch.empty((S, 2), dtype=torch.float32, device=dev)
    # run k < R is relation k's u of every scene, run R + k its v: 2 R runs, one source each
    ops.store_pack([r["u"] for r in rels] + [r["v"] for r in rels], np.arange(2 * R), np.zeros(2 * R, np.int64),
                   np.tile(edge_off[:, -1], 2), packed, frame, rot, orig)
    n_a = int(a_off[-1])
    arrays = dict(node_ctrs=out["ctrs"], node_feats=out["feats"], turn=out["turn"], control=out["control"],
                  intersect=out["intersect"], actor_ctrs=tjob.ctrs[:n_a], actor_feats=tjob.feats[:n_a], rot=rot, orig=orig,
                  gt_preds=tjob.gt[:n_a], has_preds=tjob.has[:n_a], edge_u=packed[:E], edge_v=packed[E:])
    store = DeviceSceneStore.from_arrays(arrays, h[:, 1], a_off, edge_off, rel_off, num_scales, theta)
    store.scene_city = [r["city"] for r in raws]      # for evaluate_store(..., drivable=): the map each scene is looked up in
    store.lane_arrays = None
    if lanes:
        cuts = _cuts(h, h2)
        store.lane_arrays = dict(lane_idcs=out["lane_idcs"], obs=tjob.obs[:n_a], lane_off=np.asarray(h[:, 0], np.int64),
                                 **{k: out[k][:int(cuts[k][-1])] for k in ("suc_pairs", "pre_pairs")},
                                 suc_off=np.asarray(cuts["suc_pairs"], np.int64), pre_off=np.asarray(cuts["pre_pairs"], np.int64))
    return store
