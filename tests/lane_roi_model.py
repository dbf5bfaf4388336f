"""CPU model of the fork's lane-RoI extraction (reference data_lrcnn.py:620-844, generate_lane_roi), in numpy over sparse
structures: adjacency lists for the lane graphs and the 14 node relations instead of the reference's dense [L,L] and
[N,N] boolean matrices.  Every float is formed by the numpy expression the reference uses (fp32 distances, fp32 lane
lengths, the fp32 horizon v * 3 + buffer of NumPy 2's scalar promotion), so on one NumPy version the result equals the
reference's leaf for leaf.

``first_occurrence=True`` (the product's rule) keeps a lane that the search lists more than once at its first
occurrence; ``first_occurrence=False`` reproduces the reference, which then emits that lane's nodes twice.

``agent_margins`` / ``on_edge`` give, in float64, how close an agent's decisions are to flipping (angle gates, distance
ties, search horizon): the comparisons of a device implementation against this model leave such agents out."""
import numpy as np

MAX_LEVELS = 4096
ANGLE_EPS, HORIZON_EPS = 1e-5, 1e-3
RELS = [("pre", i) for i in range(6)] + [("suc", i) for i in range(6)] + [("left", None), ("right", None)]


def _np(x):
    return x.detach().cpu().numpy() if hasattr(x, "detach") else np.asarray(x)


def rel_edges(graph, k1, i):
    e = graph[k1] if i is None else graph[k1][i]
    return _np(e["u"]).astype(np.int64), _np(e["v"]).astype(np.int64)


def agent_velocity(agent_feats, cycle_time=0.1):
    """Mean speed over the window from the first to the last moving step (data_lrcnn.py:666-684), fp32; 0 = never moves."""
    direct = np.sqrt((agent_feats[:, :, :2] ** 2).sum(-1))
    moving = direct > 0
    T = moving.shape[1]
    any_move = moving.any(1)
    first = moving.argmax(1)
    last = T - 1 - moving[:, ::-1].argmax(1)
    duration = (last - first + 1) * cycle_time
    vel = np.zeros(len(direct), np.float32)
    dist = direct.sum(axis=1)
    vel[any_move] = dist[any_move] / duration[any_move]
    return vel


class Scene:
    """Sparse tables of one scene dict."""

    def __init__(self, data):
        g = data["graph"]
        self.ctrs = _np(g["ctrs"]).astype(np.float32, copy=False)
        self.feats = _np(g["feats"]).astype(np.float32, copy=False)
        self.lane_idcs = _np(g["lane_idcs"]).astype(np.int64)
        self.N = len(self.lane_idcs)
        self.L = int(self.lane_idcs[-1]) + 1 if self.N else 0
        order = np.argsort(self.lane_idcs, kind="stable")
        bounds = np.searchsorted(self.lane_idcs[order], np.arange(self.L + 1))
        self.lane_nodes = [order[bounds[l]:bounds[l + 1]] for l in range(self.L)]
        # the reference's get_dist_np over feats[lane_idcs == l] (a Python 0.0 for a lane without nodes)
        self.lane_len = np.array([np.sum(np.sqrt(np.sum(np.square(self.feats[n]), axis=-1))) if len(n) else 0.0
                                  for n in self.lane_nodes], np.float32)
        self.lane_len64 = np.array([np.sqrt((self.feats[n].astype(np.float64) ** 2).sum(-1)).sum() for n in self.lane_nodes])
        self.adj = {}
        for key in ("suc", "pre"):
            pairs = _np(g[key + "_pairs"]).astype(np.int64).reshape(-1, 2)
            self.adj[key] = _adjacency(pairs[:, 0], pairs[:, 1])
        lu, lv = [], []
        for k1 in ("left", "right"):
            u, v = rel_edges(g, k1, None)
            lu.append(self.lane_idcs[u])
            lv.append(self.lane_idcs[v])
        self.adj["side"] = _adjacency(np.concatenate(lu), np.concatenate(lv))
        self.rel = [_adjacency(*rel_edges(g, k1, i)) for k1, i in RELS]
        node_feats = np.zeros((self.N, 8), np.float32)
        node_feats[:, :2], node_feats[:, 2:4], node_feats[:, 4:6] = self.ctrs, self.feats, _np(g["turn"])
        node_feats[:, 6], node_feats[:, 7] = _np(g["control"]), _np(g["intersect"])
        self.node_feats = node_feats
        self.a_feats = _np(data["feats"]).astype(np.float32, copy=False)
        self.a_ctrs = _np(data["ctrs"]).astype(np.float32, copy=False)
        self.obs = _np(data["obs_trajs"])
        self.vel = agent_velocity(self.a_feats)


def _adjacency(u, v):
    """{u: sorted unique v}"""
    adj = {}
    if len(u):
        key = np.unique(np.stack([u, v], 1), axis=0)
        cut = np.flatnonzero(np.diff(key[:, 0])) + 1
        for rows in np.split(key, cut):
            adj[int(rows[0, 0])] = rows[:, 1]
    return adj


def _step(adj, frontier):
    nxt = [adj[a] for a in frontier if a in adj]
    return np.unique(np.concatenate(nxt)) if nxt else np.zeros(0, np.int64)


def angle_gap(sc, a, dtype=np.float32):
    """|heading(agent step 19) - heading(node)| wrapped at pi, the reference's expression in `dtype`."""
    f, nf = sc.a_feats[a, -1, :2].astype(dtype), sc.feats.astype(dtype)
    t1 = np.arctan2(f[1], f[0])
    t2 = np.arctan2(nf[:, 1], nf[:, 0])
    dt = np.abs(t1 - t2)
    m = dt > np.pi
    dt[m] = np.abs(dt[m] - 2 * np.pi)
    return dt


def node_dist(sc, a):
    return np.sqrt(((sc.ctrs - sc.a_ctrs[a][None, :]) ** 2).sum(-1))


def anchor(sc, a):
    """The closest node whose heading is within pi/4 of the agent's (pi/2 when none is); -1 when none.  Ties: the smaller
    node index."""
    dt, dist = angle_gap(sc, a), node_dist(sc, a)
    for gate in (0.25 * np.pi, 0.5 * np.pi):
        idx = np.flatnonzero(dt < gate)
        if len(idx):
            return int(idx[np.argmin(dist[idx])])
    return -1


def lane_search(adj, lane_len, target, thres, trace=None):
    """Level-by-level frontier from `target` (get_lanes_with_dfs): every level's lanes ascending, until the running length
    (target lane + the shortest lane of each level) reaches thres."""
    out, frontier = [], np.array([target], np.int64)
    dist_sum = lane_len[target]
    for _ in range(MAX_LEVELS):
        if trace is not None:
            trace.append(abs(float(dist_sum) - float(thres)))
        if dist_sum >= thres:
            return out
        frontier = _step(adj, frontier)
        if len(frontier) == 0:
            return out
        out.extend(int(l) for l in frontier)
        dist_sum = dist_sum + lane_len[frontier].min()
    raise RuntimeError("lane search did not end within %d levels (a cycle of zero-length lanes)" % MAX_LEVELS)


def side_closure(adj, lanes):
    """get_nbr_set: (lanes, False) when no left/right neighbour lies outside `lanes`, else (ascending closure, True)."""
    nbrs, cur, grew = np.asarray(lanes, np.int64), np.unique(lanes), False
    while True:
        cur = _step(adj, cur)
        if np.isin(cur, nbrs).all():
            return nbrs, grew
        nbrs, grew = np.unique(np.concatenate([nbrs, cur])), True


def roi_lanes(sc, a, node_id, horizon_buffer, first_occurrence=True):
    v = sc.vel[a]
    target = int(sc.lane_idcs[node_id])
    lanes = [target]
    lanes += lane_search(sc.adj["suc"], sc.lane_len, target, v * 3.0 + horizon_buffer)
    lanes += lane_search(sc.adj["pre"], sc.lane_len, target, v * 2.0 + horizon_buffer)
    if first_occurrence:
        _, keep = np.unique(lanes, return_index=True)
        lanes = [lanes[i] for i in sorted(keep)]
    return side_closure(sc.adj["side"], lanes)


def generate_lane_roi(data, horizon_buffer=20., max_vel_threshold=2.78, first_occurrence=True):
    sc = Scene(data)
    subgraphs, valid = [], []
    for a in range(len(sc.a_ctrs)):
        if sc.vel[a] == 0:
            continue
        node_id = anchor(sc, a)
        if node_id < 0:
            continue
        lanes, _ = roi_lanes(sc, a, node_id, horizon_buffer, first_occurrence)
        node_mask = np.concatenate([sc.lane_nodes[l] for l in lanes]).astype(np.int64)
        n = len(node_mask)
        if n < 6:
            continue
        local = {}
        for i, g in enumerate(node_mask):
            local.setdefault(int(g), []).append(i)
        sg = {}
        near = node_dist(sc, a)[node_mask] < 5.0
        vs = np.flatnonzero(near).astype(np.int32)
        sg["a2m"] = {"u": np.zeros(len(vs), np.int32), "v": vs}
        sg["node_mask"], sg["num_nodes"] = node_mask, n
        sg["feats"] = sc.node_feats[node_mask]
        sg["agent_feat"] = np.concatenate([sc.obs[a, :, :2], sc.a_feats[a, :, :2]], axis=-1).reshape(-1)
        sg["agent_vel"] = sc.vel[a]
        rels = []
        for adj in sc.rel:
            us, vs = [], []
            for i, g in enumerate(node_mask):
                row = adj.get(int(g))
                if row is None:
                    continue
                lv = sorted(j for gv in row for j in local.get(int(gv), ()))
                us += [i] * len(lv)
                vs += lv
            rels.append({"u": np.asarray(us, np.int64), "v": np.asarray(vs, np.int64)})
        sg["pre"], sg["suc"], sg["left"], sg["right"] = rels[:6], rels[6:12], rels[12], rels[13]
        if len(sg["pre"][0]["u"]) == 0 and len(sg["suc"][0]["u"]) == 0:
            continue
        subgraphs.append(sg)
        valid.append(a)
    data["subgraphs"] = subgraphs
    data["valid_agent_ids"] = np.asarray(valid, np.int16)
    return data


# ------------------------------------------------------------------ decision margins (float64)
def agent_margins(data, a, horizon_buffer=20., sc=None):
    """{"angle": the smallest | dt - pi/4 | or | dt - pi/2 | over the nodes at most as far as the chosen anchor (all nodes
    when there is none), "tie": two eligible nodes share the smallest distance, "horizon": the smallest | dist_sum - thres |
    over the levels of both lane searches}, in float64.  A standing agent has no decision: all margins infinite."""
    sc = sc or Scene(data)
    out = {"angle": np.inf, "tie": False, "horizon": np.inf}
    if sc.vel[a] == 0 or sc.N == 0:
        return out
    dt = angle_gap(sc, a, np.float64)
    d32 = node_dist(sc, a)
    d64 = np.sqrt(((sc.ctrs.astype(np.float64) - sc.a_ctrs[a].astype(np.float64)[None, :]) ** 2).sum(-1))
    node_id = anchor(sc, a)
    inside = d64 <= d64[node_id] if node_id >= 0 else np.ones(sc.N, bool)
    out["angle"] = float(np.minimum(np.abs(dt - 0.25 * np.pi), np.abs(dt - 0.5 * np.pi))[inside].min())
    if node_id < 0:
        return out
    gate = 0.25 * np.pi if (dt < 0.25 * np.pi).any() else 0.5 * np.pi
    elig = dt < gate
    out["tie"] = bool((d32[elig] == d32[node_id]).sum() > 1 or (d64[elig] == d64[node_id]).sum() > 1)
    feats64 = sc.a_feats[a, :, :2].astype(np.float64)
    direct = np.sqrt((feats64 ** 2).sum(-1))
    mv = np.flatnonzero(direct > 0)
    v64 = direct.sum() / ((mv[-1] - mv[0] + 1) * 0.1)
    trace, target = [], int(sc.lane_idcs[node_id])
    lane_search(sc.adj["suc"], sc.lane_len64, target, v64 * 3.0 + horizon_buffer, trace)
    lane_search(sc.adj["pre"], sc.lane_len64, target, v64 * 2.0 + horizon_buffer, trace)
    out["horizon"] = float(min(trace))
    return out


def on_edge(margins):
    return margins["angle"] < ANGLE_EPS or margins["tie"] or margins["horizon"] < HORIZON_EPS


def edge_agents(data, horizon_buffer=20.):
    """Indices of the agents of a scene whose decisions may flip in the last bit."""
    sc = Scene(data)
    return [a for a in range(len(sc.a_ctrs)) if on_edge(agent_margins(data, a, horizon_buffer, sc))]
