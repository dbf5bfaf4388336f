"""float64 restatement of the fork model's goal decoder (reference lanercnn.py: nms_select 687-708, Decode.forward
802-865 and 899-919) -- TEST INFRASTRUCTURE ONLY.  Written from the formulas; pinned against the reference's own captures
(tests/golden/lanercnn_decode_b3.npz) by test_decode_model_host.py, and then the yardstick of the GPU tests.

Everything real is torch in the dtype of its inputs (float64 in the tests) and differentiable; the selection is numpy."""
import numpy as np
import torch
import torch.nn.functional as F


def rank_order(logits):
    """Node order of torch.sort(descending=True) with the open cases decided as include/lgcn.h states them: NaN above every
    number, lower index first among equals."""
    lg = np.asarray(logits, dtype=np.float64)
    nan = np.isnan(lg)
    key = np.where(nan, np.inf, lg)
    return sorted(range(len(lg)), key=lambda i: (-key[i], i))


def greedy(xy, logits, threshold=2.0, min_len=6, max_keep=0):
    """The list of nms_select (:687-708): walk the nodes in rank order, keep one unless it is closer than threshold
    (strictly) to a kept one; pad with the best unlisted nodes up to min_len; cut to max_keep (<= 0: no limit)."""
    xy = np.asarray(xy, dtype=np.float64)
    order = rank_order(logits)
    kept = []
    for i in order:
        if kept and np.sqrt(((xy[kept] - xy[i]) ** 2).sum(-1)).min() < threshold:
            continue
        kept.append(i)
    for i in order:
        if len(kept) >= min_len:
            break
        if i not in kept:
            kept.append(i)
    return kept[:max_keep] if max_keep > 0 else kept


def greedy_argmax(xy, logits, threshold=2.0, min_len=6, max_keep=0):
    """The same list in the form the kernel computes it: repeatedly take the best live node and drop every live node
    closer than threshold to it; then pad by the same arg-max over the dropped nodes."""
    xy = np.asarray(xy, dtype=np.float64)
    n = len(xy)
    order = rank_order(logits)
    limit = min(max_keep, n) if max_keep > 0 else n
    state = np.zeros(n, dtype=np.int64)          # 0 live, 1 listed, 2 dropped
    out = []
    while len(out) < limit:
        live = [i for i in order if state[i] == 0]
        if not live:
            break
        b = live[0]
        d = np.sqrt(((xy - xy[b]) ** 2).sum(-1))
        state[(state == 0) & (d < threshold)] = 2
        state[b] = 1
        out.append(b)
    while len(out) < min(min_len, limit):
        dropped = [i for i in order if state[i] == 2]
        if not dropped:
            break
        state[dropped[0]] = 1
        out.append(dropped[0])
    return out


def node_fields(pred, anc_ctrs, anc_dirs):
    """Per node of one RoI: logit, goal xy, heading theta (:807-816)."""
    xy = anc_ctrs + pred[:, 1:3]
    theta = torch.atan2(anc_dirs[:, 1], anc_dirs[:, 0]) + torch.atan(pred[:, 3] / pred[:, 4])
    return pred[:, 0], xy, theta


def poly(s, c):
    """c [..., 6] = (a0, a1, a2, b0, b1, b2), s [..., S] -> points [..., S, 2] (:728-732)."""
    a0, a1, a2, b0, b1, b2 = [c[..., i:i + 1] for i in range(6)]
    return torch.stack([a0 * s ** 2 + a1 * s + a2, b0 * s ** 2 + b1 * s + b2], -1)


def poly_d1(s, c):
    a0, a1, _, b0, b1, _ = [c[..., i:i + 1] for i in range(6)]
    return torch.stack([2 * a0 * s + a1, 2 * b0 * s + b1], -1)


def decode(pred, pred_spans, anc_ctrs, anc_dirs, anc_first, agt_ctrs, agt_dir_last, agt_vel, k=6, threshold=2.0, top_idx=None):
    """:802-865 for all interest agents.  top_idx given: use those indices (gradient checks); else select them."""
    tops, goals, thetas, logits = [], [], [], []
    for a in range(len(pred_spans) - 1):
        lo, hi = pred_spans[a], pred_spans[a + 1]
        f = anc_first[a]
        lg, xy, th = node_fields(pred[lo:hi], anc_ctrs[f:f + hi - lo], anc_dirs[f:f + hi - lo])
        if top_idx is None:
            top = greedy(xy.detach().numpy(), lg.detach().numpy(), threshold, k, k)
        else:
            top = [int(i) for i in top_idx[a]]
        assert len(top) == k
        t = torch.tensor(top, dtype=torch.long)
        tops.append(top)
        goals.append(xy[t])
        thetas.append(th[t])
        logits.append(lg[t])
    goals, thetas, logits = torch.stack(goals), torch.stack(thetas), torch.stack(logits)
    p = torch.stack([torch.cos(thetas), torch.sin(thetas)], -1)                      # [A, k, 2]
    nrm = torch.sqrt((agt_dir_last ** 2).sum(1, keepdim=True))
    d = torch.where(nrm < 1e-6, torch.zeros_like(agt_dir_last), agt_dir_last / nrm).unsqueeze(1)   # [A, 1, 2]
    c = agt_ctrs.unsqueeze(1)
    q1 = (2 * goals * d + 2 * c * d) / (2 + d - p)
    q0 = goals - c - q1
    q2 = c.expand_as(goals)
    coef = torch.stack([q0[..., 0], q1[..., 0], q2[..., 0], q0[..., 1], q1[..., 1], q2[..., 1]], -1)   # [A, k, 6]
    j = torch.arange(0, 31, dtype=pred.dtype)
    pts = poly(j / 30, coef)
    length = torch.sqrt(((pts[:, :, 1:] - pts[:, :, :-1]) ** 2).sum(-1)).sum(-1)       # [A, k]
    vel = agt_vel.view(-1, 1)
    acc = 2 * (length - vel * 3.0) / 9.0
    t = j / 10
    v = (vel.unsqueeze(2) + acc.unsqueeze(2) * t).clamp_min(0.0)
    s_samples = (v[:, :, :1] + v[:, :, 1:]) * t[1:] / 2
    return {"top_idx": np.asarray(tops, dtype=np.int64), "goals": goals, "thetas": thetas, "logits": logits, "coef": coef,
            "s_samples": s_samples, "denominators": 2 + d - p}


def normalise(s):
    s = s / s.max(-1, keepdim=True)[0]
    return torch.where(s == 0.0, torch.ones_like(s), s)


def refine(s_samples, coef, traj_delta):
    """:899-919: pred_trajs [A, k, 30, 2]."""
    s = normalise(s_samples + traj_delta[..., 0])
    tangent = poly_d1(s, coef)
    normal = torch.stack([-tangent[..., 1], tangent[..., 0]], -1)
    return poly(s, coef) + normal * traj_delta[..., 1:2]


# ---------------------------------------------------------------- the modules around it, on a state_dict (any dtype)
def _gn(x, sd, name):
    return F.group_norm(x, 1, sd[name + ".weight"], sd[name + ".bias"], 1e-5)


def _block(x, sd, name, act=True):
    out = _gn(F.linear(x, sd[name + ".linear.weight"]), sd, name + ".norm")
    return F.relu(out) if act else out


def stem(xa, xs, sd, a, s):
    """ReLU(a(xa) + s(xs)), a / s = Linear(2, 128) -> ReLU -> Linear(128, 128, GN)."""
    br = lambda x, n: _block(F.relu(F.linear(x, sd[n + ".0.weight"], sd[n + ".0.bias"])), sd, n + ".2", act=False)
    return F.relu(br(xa, a) + br(xs, s))


def head(x, sd, name):
    """Linear(128, 128, GN, ReLU) -> Linear(128, out) with bias."""
    return F.linear(_block(x, sd, name + ".0"), sd[name + ".1.weight"], sd[name + ".1.bias"])


def decode_forward(sd, roi_feat, spans, anc_ctrs, anc_dirs, agt_ctrs, agt_dirs, agt_trajs, agt_vel, lane_pooling, k=6,
                   top_idx=None):
    """Decode.forward on the state_dict sd (prefix-free names) for interest RoIs `spans` (rows of roi_feat and of the
    anchors).  agt_dirs / agt_trajs [A, 20, 2].  lane_pooling = oracle.lanercnn_oracle.lane_pooling: handed the motion
    centres as [1, 20, 2] tensors it advances the context offset by 1 per scene, as the reference does (:487, :878)."""
    pred_spans = [0]
    for lo, hi in spans:
        pred_spans.append(pred_spans[-1] + hi - lo)
    feats = torch.cat([roi_feat[lo:hi] for lo, hi in spans], 0)
    pred = head(feats, sd, "pred")
    dec = decode(pred, pred_spans, anc_ctrs, anc_dirs, [lo for lo, _ in spans], agt_ctrs, agt_dirs[:, -1], agt_vel, k,
                 top_idx=top_idx)
    agt_feat = stem(agt_trajs.reshape(-1, 2), agt_dirs.reshape(-1, 2), sd, "agt_layer1", "agt_layer2")
    n_agt = len(spans)
    motion = {"ctrs": [agt_trajs[i:i + 1] for i in range(n_agt)],
              "pose": [torch.cat([agt_trajs[i], agt_dirs[i]], -1) for i in range(n_agt)]}
    roi_map = {"ctrs": [anc_ctrs[lo:hi] for lo, hi in spans],
               "pose": [torch.cat([anc_ctrs[lo:hi], anc_dirs[lo:hi]], -1) for lo, hi in spans]}
    pooled = lane_pooling(agt_feat, motion, feats, roi_map, sd, "lane_pool")[0]
    rows = torch.as_tensor(dec["top_idx"], dtype=torch.long) + torch.tensor(pred_spans[:-1]).view(-1, 1)
    traj_delta = head(pooled[rows.reshape(-1)], sd, "refinement").view(n_agt, k, 30, 2)
    dec.update(pred=pred, pooled=pooled, traj_delta=traj_delta, pred_trajs=refine(dec["s_samples"], dec["coef"], traj_delta))
    return dec


# ---------------------------------------------------------------- the fixture and the shared float64 reference
_cache = {}


def fixture():
    """tests/golden/lanercnn_decode_b3.npz (captures of the reference's Decode / Interactor) and the state names."""
    if "fx" not in _cache:
        import json
        import os
        here = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
        with np.load(os.path.join(here, "lanercnn_decode_b3.npz")) as z:
            g = {k: z[k] for k in z.files}
        _cache["fx"] = (g, json.load(open(os.path.join(here, "lanercnn_decode_state_names.json"))))
    return _cache["fx"]


def decode_args(g, dtype=torch.float64, device=None):
    """The arguments of decode() from the fixture: anchors concatenated, the interest agents' rows picked on the host."""
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dtype).to(device or "cpu")
    n_scene = len(g["dec/interest_roi"])
    spans = [tuple(int(v) for v in g["dec/roi_spans"][i]) for i in g["dec/interest_roi"]]
    first = [int(g["dec/data/valid_agent_ids/%d" % b][0]) for b in range(n_scene)]
    pick = lambda key: np.stack([g["dec/data/%s/%d" % (key, b)][first[b]] for b in range(n_scene)])
    return {"spans": spans,
            "anc_ctrs": t(np.concatenate([g["dec/anc_ctrs/%d" % b] for b in range(n_scene)])),
            "anc_dirs": t(np.concatenate([g["dec/anc_dirs/%d" % b] for b in range(n_scene)])),
            "agt_ctrs": t(pick("ctrs")), "agt_dirs": t(pick("feats")[:, :, :2]), "agt_trajs": t(pick("obs_trajs")[:, :, :2]),
            "agt_vel": t(g["dec/agent_vel"][g["dec/interest_roi"]].astype(np.float32))}


def reference64():
    """decode() and refine() in float64 on the fixture's fp32 `pred` and `traj_delta` (computed once, never modified)."""
    if "ref" not in _cache:
        g, _ = fixture()
        a = decode_args(g)
        spans = [0] + list(np.cumsum([hi - lo for lo, hi in a["spans"]]))
        dec = decode(torch.from_numpy(g["dec/pred"]).double(), [int(v) for v in spans], a["anc_ctrs"], a["anc_dirs"],
                     [lo for lo, _ in a["spans"]], a["agt_ctrs"], a["agt_dirs"][:, -1], a["agt_vel"])
        dec["pred_trajs"] = refine(dec["s_samples"], dec["coef"], torch.from_numpy(g["dec/traj_delta"]).double())
        _cache["ref"] = dec
    return _cache["ref"]


def rel_err(got, ref):
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    return float(np.abs(got - ref).max() / np.abs(ref).max())
