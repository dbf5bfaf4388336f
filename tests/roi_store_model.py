"""A numpy model of the resident lane-RoI store (data_lrcnn.RoiStore): the resident layout with
scene-local indices, the gather of a pick (copy the run, add the base of the picked scene) and its per-batch table, all in
plain loops over scenes, RoIs and relations; and the merged graph of a list of scenes built the way lane_roi_flat lays it
out (RoI by RoI at the relation-major bases).  Inputs are scene dicts with "subgraphs" / "valid_agent_ids" in the
reference's schema (lane_roi_model.generate_lane_roi).  `tables_fn` is data_lrcnn.relation_major_tables, the same function
on both sides."""
import numpy as np

K = 14                    # relations: pre 0..5, suc 0..5, left, right
REL = [("pre", i) for i in range(6)] + [("suc", i) for i in range(6)] + [("left", None), ("right", None)]
ROW_KEYS = ("ctrs", "feats", "obs_trajs", "gt_preds", "has_preds")


def rel_of(sg, k):
    k1, i = REL[k]
    e = sg[k1] if i is None else sg[k1][i]
    return np.asarray(e["u"], np.int64), np.asarray(e["v"], np.int64)


def edge_counts(sgs):
    return np.array([[len(rel_of(sg, k)[0]) for k in range(K)] + [len(sg["a2m"]["v"])] for sg in sgs], np.int64).reshape(-1, K + 1)


def _cat(parts, tail, dtype):
    return np.concatenate([np.asarray(p, dtype).reshape((-1,) + tail) for p in parts] + [np.zeros((0,) + tail, dtype)])


def merged(scenes, tables_fn):
    """The batch graph of `scenes` (every one with an RoI) as lane_roi_flat leaves it, and the per-RoI agent rows."""
    sgs = [sg for s in scenes for sg in s["subgraphs"]]
    per = [len(s["subgraphs"]) for s in scenes]
    assert all(per)
    sizes = np.array([sg["num_nodes"] for sg in sgs], np.int64)
    roi_base = np.concatenate([[0], np.cumsum(sizes)])
    cnt = edge_counts(sgs)
    base, rel_ext, n_a2m = tables_fn(cnt)
    u, v = np.zeros(int(rel_ext[-1]), np.int64), np.zeros(int(rel_ext[-1]), np.int64)
    au, av = np.zeros(n_a2m, np.int64), np.zeros(n_a2m, np.int64)
    for r, sg in enumerate(sgs):
        for k in range(K):
            ru, rv = rel_of(sg, k)
            u[base[r, k]:base[r, k] + len(ru)] = ru + roi_base[r]
            v[base[r, k]:base[r, k] + len(rv)] = rv + roi_base[r]
        n = len(sg["a2m"]["v"])
        au[base[r, K]:base[r, K] + n] = r
        av[base[r, K]:base[r, K] + n] = np.asarray(sg["a2m"]["v"], np.int64) + roi_base[r]
    out = dict(feats=_cat([sg["feats"] for sg in sgs], (8,), np.float32), node_mask=_cat([sg["node_mask"] for sg in sgs], (), np.int64),
               agent_feat=_cat([sg["agent_feat"] for sg in sgs], (80,), np.float32), u=u, v=v, a2m_u=au, a2m_v=av, sizes=sizes,
               scene_of=np.repeat(np.arange(len(scenes)), per), agent_vel=np.array([sg["agent_vel"] for sg in sgs], np.float32),
               rel_ext=np.asarray(rel_ext, np.int64), edge_cnt=cnt, first_roi=np.concatenate([[0], np.cumsum(per)]).astype(np.int64),
               agent_ids=np.concatenate([np.asarray(s["valid_agent_ids"], np.int64) for s in scenes]))
    for key in ROW_KEYS:
        out["row_" + key] = np.concatenate([np.asarray(s[key])[np.asarray(s["valid_agent_ids"], np.int64)] for s in scenes])
    return out


def build(scenes):
    """The resident layout of `scenes` (a scene may hold no RoI): arrays with scene-local indices and the host tables."""
    S = len(scenes)
    first_roi, node_off = [0], [0]
    edge_off = np.zeros((K + 1, S + 1), np.int64)
    rel_u, rel_v = [[] for _ in range(K)], [[] for _ in range(K)]
    au, av, sgs, ids = [], [], [], []
    for s, sc in enumerate(scenes):
        at = 0                                                    # row of the RoI's first node within the scene's block
        for i, sg in enumerate(sc["subgraphs"]):
            for k in range(K):
                ru, rv = rel_of(sg, k)
                rel_u[k].append(ru + at)
                rel_v[k].append(rv + at)
                edge_off[k, s + 1] += len(ru)
            n = len(sg["a2m"]["v"])
            au.append(np.full(n, i, np.int64))
            av.append(np.asarray(sg["a2m"]["v"], np.int64) + at)
            edge_off[K, s + 1] += n
            at += sg["num_nodes"]
            sgs.append(sg)
        ids.append(np.asarray(sc["valid_agent_ids"], np.int64))
        first_roi.append(first_roi[-1] + len(sc["subgraphs"]))
        node_off.append(node_off[-1] + at)
    st = dict(feats=_cat([sg["feats"] for sg in sgs], (8,), np.float32), node_mask=_cat([sg["node_mask"] for sg in sgs], (), np.int32),
              agent_feat=_cat([sg["agent_feat"] for sg in sgs], (80,), np.float32),
              edge_u=_cat([x for k in range(K) for x in rel_u[k]], (), np.int32), edge_v=_cat([x for k in range(K) for x in rel_v[k]], (), np.int32),
              a2m_u=_cat(au, (), np.int32), a2m_v=_cat(av, (), np.int32),
              first_roi=np.asarray(first_roi, np.int64), node_off=np.asarray(node_off, np.int64), edge_off=np.cumsum(edge_off, 1),
              sizes=np.array([sg["num_nodes"] for sg in sgs], np.int64), agent_vel=np.array([sg["agent_vel"] for sg in sgs], np.float32),
              edge_cnt=edge_counts(sgs), agent_ids=_cat(ids, (), np.int64))
    for key in ROW_KEYS:
        tail = np.asarray(scenes[0][key]).shape[1:]
        st["row_" + key] = _cat([np.asarray(sc[key])[i] for sc, i in zip(scenes, ids)], tail, np.asarray(scenes[0][key]).dtype)
    return st


def usable(st):
    return [s for s in range(len(st["first_roi"]) - 1) if st["first_roi"][s + 1] > st["first_roi"][s]]


def gather(st, pick, tables_fn):
    """The pick's merged graph, host tables and per-batch table out of the resident layout: per run of a picked scene, the
    resident elements plus the base of that scene in the OUTPUT."""
    first_roi, node_off, edge_off = st["first_roi"], st["node_off"], st["edge_off"]
    S, B = len(first_roi) - 1, len(pick)
    if B == 0:
        raise ValueError("empty pick")
    for s in pick:
        if not 0 <= s < S:
            raise ValueError("scene outside the store")
        if first_roi[s + 1] == first_roi[s]:
            raise ValueError("scene %d has no lane RoI" % s)
    rel_at = np.concatenate([[0], np.cumsum(edge_off[:K, -1])])
    out_node, out_roi = [0], [0]
    for s in pick:
        out_node.append(out_node[-1] + int(node_off[s + 1] - node_off[s]))
        out_roi.append(out_roi[-1] + int(first_roi[s + 1] - first_roi[s]))
    rows = np.concatenate([np.arange(node_off[s], node_off[s + 1]) for s in pick])
    rois = np.concatenate([np.arange(first_roi[s], first_roi[s + 1]) for s in pick])
    seg_len, seg_src, idx = [], [], []
    for q in range(2 * K + 2):                                    # u of relation 0..13, v of relation 0..13, a2m_u, a2m_v
        for j, s in enumerate(pick):
            k = q % K if q < 2 * K else K
            name = "edge_u" if q < K else "edge_v" if q < 2 * K else "a2m_u" if q == 2 * K else "a2m_v"
            lo = int(edge_off[k, s]) + (int(rel_at[k]) if q < 2 * K else 0)
            n = int(edge_off[k, s + 1] - edge_off[k, s])
            seg_len.append(n)
            seg_src.append(lo)
            idx.append(st[name][lo:lo + n].astype(np.int64) + (out_roi[j] if q == 2 * K else out_node[j]))
    cnt = st["edge_cnt"][rois]
    _, rel_ext, n_a2m = tables_fn(cnt)
    idx = np.concatenate(idx)
    E = int(rel_ext[-1])
    assert len(idx) == 2 * E + 2 * n_a2m
    table = np.concatenate([out_node, out_roi, [node_off[s] for s in pick], [first_roi[s] for s in pick],
                            np.concatenate([[0], np.cumsum(seg_len)]), seg_src]).astype(np.int64)
    out = dict(feats=st["feats"][rows], node_mask=st["node_mask"][rows].astype(np.int64), agent_feat=st["agent_feat"][rois],
               u=idx[:E], v=idx[E:2 * E], a2m_u=idx[2 * E:2 * E + n_a2m], a2m_v=idx[2 * E + n_a2m:], sizes=st["sizes"][rois],
               scene_of=np.repeat(np.arange(B), np.diff(out_roi)), agent_vel=st["agent_vel"][rois],
               rel_ext=np.asarray(rel_ext, np.int64), edge_cnt=cnt, first_roi=np.asarray(out_roi, np.int64),
               agent_ids=st["agent_ids"][rois], table=table)
    for key in ROW_KEYS:
        out["row_" + key] = st["row_" + key][rois]
    return out


def picks_of(st):
    """The picks of the issue over the usable scenes: the first, the last, [2, 0, 2], all reversed, 70 entries cycling."""
    us = usable(st)
    assert len(us) >= 3
    return [[us[0]], [us[-1]], [us[2], us[0], us[2]], us[::-1], [us[i % len(us)] for i in range(70)]]
