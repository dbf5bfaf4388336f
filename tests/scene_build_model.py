"""Host model of scene construction (lanegcn_amd.data_raw, csrc/lgcn_scene.hip) in plain numpy, written from the
description of the arithmetic in include/lgcn.h:

  frame     orig = the agent's row 19 rounded to fp32; theta = pi - atan2(row 18 - orig) in float64; rot = cos / sin
            rounded to fp32.
  a point   d = p - (double)orig;  x' = r00 * dx + r01 * dy,  y' = r10 * dx + r11 * dy in float64, every product and sum
            rounded on its own (numpy's elementwise * and + are separate operations: no FMA).
  tracks    positions rounded to fp32, steps differenced in fp32;  nodes formed in float64, rounded once.

Tables are lanegcn_amd.data_raw.LaneTable objects (host arrays only: no GPU needed)."""
import numpy as np

OBS, FUT = 20, 30


class ModelError(Exception):
    pass


def frame(raw, theta=None):
    t0 = np.asarray(raw["trajs"][0], np.float64)
    if len(t0) < OBS:
        raise ModelError("agent track under 20 rows")
    orig = t0[19].astype(np.float32)
    if theta is None:
        pre = t0[18] - orig
        theta = np.pi - np.arctan2(pre[1], pre[0])
    rot = np.asarray([[np.cos(theta), -np.sin(theta)], [np.sin(theta), np.cos(theta)]], np.float32)
    return orig, theta, rot


def xform(pts, orig, rot):
    """float64 [n,2]: the points in the scene frame."""
    pts = np.asarray(pts, np.float64).reshape(-1, 2)
    o, r = orig.astype(np.float64), rot.astype(np.float64)
    dx, dy = pts[:, 0] - o[0], pts[:, 1] - o[1]
    x = r[0, 0] * dx + r[0, 1] * dy
    y = r[1, 0] * dx + r[1, 1] * dy
    return np.stack([x, y], 1)


def obj_feats(raw, pred_range, theta=None, scene=0):
    orig, theta, rot = frame(raw, theta)
    lo_x, hi_x, lo_y, hi_y = (np.float32(v) for v in pred_range)
    feats, obs_all, ctrs, gts, hass = [], [], [], [], []
    for k, (xy, st) in enumerate(zip(raw["trajs"], raw["steps"])):
        xy, st = np.asarray(xy, np.float64), np.asarray(st, np.int64)
        low = st[st < OBS + FUT]
        if len(np.unique(low)) != len(low):
            raise ModelError("scene %d track %d lists a step twice" % (scene, k))
        if 19 not in st:
            continue
        present = np.zeros(OBS, bool)
        present[st[st < OBS]] = True
        gaps = np.flatnonzero(~present)
        first = int(gaps[-1]) + 1 if len(gaps) else 0          # the run of consecutive steps that ends at 19
        pos = xform(xy, orig, rot).astype(np.float32)
        obs = np.zeros((OBS, 3), np.float32)
        sel = (st >= first) & (st < OBS)
        obs[st[sel], :2] = pos[sel]
        obs[st[sel], 2] = 1.0
        x, y = obs[19, 0], obs[19, 1]
        if x < lo_x or x > hi_x or y < lo_y or y > hi_y:
            continue
        f = np.zeros((OBS, 3), np.float32)
        f[first + 1:, :2] = obs[first + 1:, :2] - obs[first:-1, :2]
        f[first:, 2] = 1.0
        gt, has = np.zeros((FUT, 2), np.float32), np.zeros(FUT, bool)
        fut = (st >= OBS) & (st < OBS + FUT)
        gt[st[fut] - OBS] = xy[fut].astype(np.float32)
        has[st[fut] - OBS] = True
        feats.append(f); obs_all.append(obs); ctrs.append(obs[19, :2].copy()); gts.append(gt); hass.append(has)
    stack = lambda xs, tail, dt: np.stack(xs).astype(dt) if xs else np.zeros((0,) + tail, dt)
    return dict(feats=stack(feats, (OBS, 3), np.float32), obs_trajs=stack(obs_all, (OBS, 3), np.float32),
                ctrs=stack(ctrs, (2,), np.float32), orig=orig, theta=theta, rot=rot,
                gt_preds=stack(gts, (FUT, 2), np.float32), has_preds=stack(hass, (FUT,), bool))


def lane_graph(orig, rot, table, pred_range, rows=None, scene=0):
    """The scale-0 graph; rows: candidate table rows in their order (None: the whole table)."""
    x_min, x_max, y_min, y_max = (float(v) for v in pred_range)
    rows = np.arange(table.n_lanes) if rows is None else np.asarray(rows, np.int64)
    kept, lines = [], {}
    for r in rows:
        c = xform(table.pts[table.pt_off[r]:table.pt_off[r + 1]], orig, rot)
        x, y = c[:, 0], c[:, 1]
        if x.max() < x_min or x.min() > x_max or y.max() < y_min or y.min() > y_max:
            continue
        kept.append(int(r))
        lines[int(r)] = c
    if not kept:
        raise ModelError("scene %d: no lane survives" % scene)
    rank = {r: i for i, r in enumerate(kept)}
    nseg = [len(lines[r]) - 1 for r in kept]
    start = np.concatenate([[0], np.cumsum(nseg)]).astype(np.int64)
    ctrs = np.concatenate([((lines[r][:-1] + lines[r][1:]) / 2.0).astype(np.float32) for r in kept])
    feats = np.concatenate([(lines[r][1:] - lines[r][:-1]).astype(np.float32) for r in kept])
    turn = np.zeros((start[-1], 2), np.float32)
    control, intersect = np.zeros(start[-1], np.float32), np.zeros(start[-1], np.float32)
    lane_idcs = np.zeros(start[-1], np.int64)
    pre, suc = {"u": [], "v": []}, {"u": [], "v": []}
    pairs = {k: [] for k in ("pre", "suc", "left", "right")}
    for i, r in enumerate(kept):
        a, b = int(start[i]), int(start[i + 1])
        lane_idcs[a:b] = i
        if table.turn[r] == 1:
            turn[a:b, 0] = 1
        elif table.turn[r] == 2:
            turn[a:b, 1] = 1
        control[a:b], intersect[a:b] = float(table.control[r] != 0), float(table.intersect[r] != 0)
        nodes = list(range(a, b))
        pre["u"] += nodes[1:]; pre["v"] += nodes[:-1]
        for j in table.pred[table.pred_off[r]:table.pred_off[r + 1]]:
            if int(j) in rank:
                pre["u"].append(a); pre["v"].append(int(start[rank[int(j)] + 1]) - 1)
                pairs["pre"].append([i, rank[int(j)]])
        suc["u"] += nodes[:-1]; suc["v"] += nodes[1:]
        for j in table.succ[table.succ_off[r]:table.succ_off[r + 1]]:
            if int(j) in rank:
                suc["u"].append(b - 1); suc["v"].append(int(start[rank[int(j)]]))
                pairs["suc"].append([i, rank[int(j)]])
        if int(table.left[r]) in rank:
            pairs["left"].append([i, rank[int(table.left[r])]])
        if int(table.right[r]) in rank:
            pairs["right"].append([i, rank[int(table.right[r])]])
    i64 = lambda x: np.asarray(x, np.int64)
    g = dict(ctrs=ctrs, num_nodes=int(start[-1]), feats=feats, turn=turn, control=control, intersect=intersect,
             pre=[{k: i64(v) for k, v in pre.items()}], suc=[{k: i64(v) for k, v in suc.items()}], lane_idcs=lane_idcs)
    for k, v in pairs.items():
        g[k + "_pairs"] = i64(v).reshape(-1, 2)
    g["kept_rows"] = i64(kept)
    return g


def build_scenes(raws, tables, config, lane_ids=None, cross=True, dilate=True):
    """Scene dicts (numpy leaves) as lanegcn_amd.data_raw.build_scenes returns them with device=False."""
    from lanegcn_amd import data as gen
    scenes = []
    for b, raw in enumerate(raws):
        s = obj_feats(raw, config["pred_range"], scene=b)
        tab = tables[raw["city"]]
        rows = tab.rows(lane_ids[b]) if lane_ids is not None and lane_ids[b] is not None else None
        g = lane_graph(s["orig"], s["rot"], tab, config["pred_range"], rows, scene=b)
        del g["kept_rows"]
        if dilate:
            for k in ("pre", "suc"):
                g[k] = g[k] + gen.dilated_nbrs(g[k][0], g["num_nodes"], config["num_scales"])
        if cross:
            from oracle import graphgen_oracle as GO
            side = GO.preprocess(g, config["cross_dist"])
            g["left"], g["right"] = side["left"], side["right"]
        s.update(city=raw["city"], idx=b, graph=g, theta=float(s["theta"]))
        scenes.append(s)
    return scenes
