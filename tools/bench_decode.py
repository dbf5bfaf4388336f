"""Decode.forward (reference lanercnn.py:740-924) on 32 interest agents x ~300 RoI nodes: the HIP path of
lanegcn_amd.lanercnn.Decode beside a stock-op restatement of the reference's loop that lives in this tool -- a Python
walk over the sorted nodes of every RoI with one host read per visited node, one .item() per agent, and the trajectory
arithmetic as ~80 elementwise ATen launches.  Both share the module's weights and its LanePooling; the two heads of the
stock side are F.linear + F.group_norm.  Prints the medians and one JSON line.  A number for DESIGN.md; no bar.
The kernels' results at this shape (RoIs of 300 nodes and beyond: second passes of the 256-thread loops) are checked by
tests/test_gpu_goal_decode_edges.py, not here.

  --agents N --nodes M   interest agents and nodes per RoI (default 32 x 300)
  --steps K --warmup W   timed and untimed forwards per variant, alternating call by call
  --train                instead: forward + backward of Decode + lanercnn.Loss with Decode.train_hip off and on, alternating
                         step by step in this process after the warm-up; medians, and the kernel launches per step of each
                         path (torch.profiler; null where it is unavailable)"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import lanegcn_amd  # noqa: E402,F401
from lanegcn_amd import lanegcn as M  # noqa: E402
from lanegcn_amd import lanercnn as R  # noqa: E402
from lanegcn_amd import ops  # noqa: E402


def make_inputs(n_agt, n_nodes, seed=0):
    rng = np.random.default_rng(seed)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).cuda()
    sub = {"ctrs": [], "dirs": [], "roi_spans": [], "interest_roi": torch.arange(n_agt), "agent_vel": []}
    data = {"valid_agent_ids": [], "ctrs": [], "feats": [], "obs_trajs": []}
    row, per = 0, 30
    for _ in range(n_agt):
        heading, speed = rng.uniform(0.2, 1.3), rng.uniform(4.0, 9.0)
        u, v = np.array([np.cos(heading), np.sin(heading)]), np.array([-np.sin(heading), np.cos(heading)])
        centre = rng.normal(0, 8.0, 2)
        lane, j = np.divmod(np.arange(n_nodes), per)
        ctrs = centre + np.outer(j - 4.0, u) + np.outer(3.2 * (lane - lane.max() / 2), v) + rng.normal(0, 0.05, (n_nodes, 2))
        th = heading + 0.02 * j
        pos = centre + np.outer(np.arange(20) - 19, u * speed * 0.1) + rng.normal(0, 0.05, (20, 2))
        step = np.zeros((20, 2))
        step[1:] = pos[1:] - pos[:-1]
        one = np.ones((1, 20, 1))
        sub["ctrs"].append(t(ctrs))
        sub["dirs"].append(t(np.stack([np.cos(th), np.sin(th)], 1)))
        sub["roi_spans"].append((row, row + n_nodes))
        sub["agent_vel"].append(float(speed))
        row += n_nodes
        data["valid_agent_ids"].append(torch.zeros(1, dtype=torch.int64).cuda())
        data["ctrs"].append(t(centre[None]))
        data["feats"].append(t(np.concatenate([step[None], one], 2)))
        data["obs_trajs"].append(t(np.concatenate([pos[None], one], 2)))
    return sub, data, torch.from_numpy(rng.normal(0, 1, (row, 128)).astype(np.float32)).cuda().relu()


def stock_head(seq, x):
    lin = seq[0]
    h = F.relu(F.group_norm(F.linear(x, lin.linear.weight), 1, lin.norm.weight, lin.norm.bias, lin.norm.eps))
    return F.linear(h, seq[1].weight, seq[1].bias)


def stock_select(xy, logits, threshold=2.0, min_len=6):
    """The reference's selection, node by node: a host read decides every visited node."""
    order = logits.sort(descending=True)[1]
    kept = []
    for i in order:
        if kept and bool(torch.sqrt(((xy[torch.stack(kept)] - xy[i]) ** 2).sum(-1)).min() < threshold):
            continue
        kept.append(i)
    if len(kept) < min_len:
        have = set(int(i.item()) for i in kept)
        for i in order:
            if int(i.item()) not in have:
                kept.append(i)
                if len(kept) == min_len:
                    break
    return torch.stack(kept)


def stock_decode(m, roi_feat, sub, data, k=6):
    spans = [sub["roi_spans"][int(i.item())] for i in sub["interest_roi"]]             # one .item() per agent
    feats = torch.cat([roi_feat[lo:hi] for lo, hi in spans], 0)
    pred = stock_head(m.pred, feats)
    anc_c, anc_d = torch.cat(sub["ctrs"], 0), torch.cat(sub["dirs"], 0)
    tops, goals, thetas, logits, row = [], [], [], [], 0
    for lo, hi in spans:
        p = pred[row:row + hi - lo]
        row += hi - lo
        xy = anc_c[lo:hi] + p[:, 1:3]
        th = torch.atan2(anc_d[lo:hi, 1], anc_d[lo:hi, 0]) + torch.atan(p[:, 3] / p[:, 4])
        top = stock_select(xy, p[:, 0])[:k]
        tops.append(top)
        goals.append(xy[top])
        thetas.append(th[top])
        logits.append(p[:, 0][top])
    goals, thetas, logits = torch.stack(goals), torch.stack(thetas), torch.stack(logits)
    first = lambda key: torch.cat([x[v][:1] for v, x in zip(data["valid_agent_ids"], data[key])], 0)
    agt_ctrs = first("ctrs").view(-1, 2)
    agt_dirs, agt_trajs = first("feats").view(-1, 20, 3)[:, :, :2], first("obs_trajs").view(-1, 20, 3)[:, :, :2]
    vel = torch.tensor(sub["agent_vel"], device=pred.device)[sub["interest_roi"].to(pred.device)]
    d = agt_dirs[:, -1]
    nrm = torch.linalg.norm(d, dim=1)
    d = d / nrm.view(-1, 1)
    d[nrm < 1e-6] = 0.0
    coefs = R.compute_coefficent(agt_ctrs, d, goals, torch.stack([torch.cos(thetas), torch.sin(thetas)], -1))
    s31 = (1.0 / 30) * torch.arange(0, 31, device=pred.device).float()
    pts = R.sample_trajectory(s31, *coefs)
    length = torch.sqrt(((pts[:, :, 1:] - pts[:, :, :-1]) ** 2).sum(-1)).sum(-1)
    acc = 2 * (length - vel.view(-1, 1) * 3.0) / 9.0
    t31 = 0.1 * torch.arange(0, 31, device=pred.device).float()
    v = vel.view(-1, 1, 1) + acc.unsqueeze(2) * t31
    v[v <= 0.0] = 0.0
    s = (v[:, :, :1] + v[:, :, 1:]) * t31[1:] / 2
    # the motion graph pooled into the RoIs: the module's own LanePooling (same launches on both sides)
    n_agt = len(spans)
    rows = (torch.arange(n_agt, device=pred.device).view(-1, 1) + torch.arange(20, device=pred.device).view(1, -1)).reshape(-1)
    tq, dq = agt_trajs.reshape(-1, 2)[rows], agt_dirs.reshape(-1, 2)[rows]
    br = lambda seq, x: F.group_norm(F.linear(F.relu(seq[0](x)), seq[2].linear.weight), 1, seq[2].norm.weight, seq[2].norm.bias,
                                     seq[2].norm.eps)
    agt_feat = F.relu(br(m.agt_layer1, tq) + br(m.agt_layer2, dq))
    motion = {"ctrs": [agt_trajs[i].contiguous() for i in range(n_agt)], "pose": list(torch.cat([tq, dq], -1).split(20, 0))}
    roi_map = {"ctrs": [anc_c[lo:hi] for lo, hi in spans], "pose": [torch.cat([anc_c[lo:hi], anc_d[lo:hi]], -1) for lo, hi in spans]}
    pooled = m.lane_pool(agt_feat, motion, feats, roi_map)
    row, picked = 0, []
    for (lo, hi), top in zip(spans, tops):
        picked.append(pooled[row:row + hi - lo][top])
        row += hi - lo
    delta = stock_head(m.refinement, torch.cat(picked, 0)).view(n_agt, k, 30, 2)
    s = s + delta[..., 0]
    s = s / s.max(2)[0].unsqueeze(2)
    s[s == 0.0] = 1.0
    tan = R.sample_d1_trajectory(s, *coefs)
    rot = torch.tensor([[0.0, -1.0], [1.0, 0.0]], device=pred.device)
    shift = torch.matmul(rot, tan.reshape(-1, 2, 1)).view(n_agt, k, 30, 2) * delta[..., 1].unsqueeze(3)
    return logits, goals, R.sample_trajectory(s, *coefs) + shift, torch.stack(tops)


def count_launches(step):
    """Device kernel launches of one step() as torch.profiler sees them, or None."""
    try:
        from torch.profiler import ProfilerActivity, profile
        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            step()
            torch.cuda.synchronize()
        kernels = [e for e in prof.events() if str(e.device_type).endswith("CUDA") and "memcpy" not in e.name.lower()
                   and "memset" not in e.name.lower()]
        return len(kernels) or None
    except Exception as exc:  # noqa: BLE001  (a number for a document; never a reason to lose the timings)
        print("launch count unavailable: %r" % (exc,), flush=True)
        return None


def train_mode(args):
    """Forward + backward of Decode + Loss, Decode.train_hip off / on."""
    torch.manual_seed(0)
    cfg = dict(M.config, num_mods=6, num_preds=30)
    m = R.Decode(cfg).cuda().train()
    loss = R.Loss(cfg)
    sub, data, roi_feat = make_inputs(args.agents, args.nodes)
    rng = np.random.default_rng(1)
    data["gt_preds"], data["has_preds"] = [], []
    for c, f in zip(data["ctrs"], data["feats"]):              # the future: the last observed step continued, all observed
        step = f[0, -1, :2].cpu().numpy().astype(np.float64)
        gt = c.cpu().numpy() + np.outer(np.arange(1, 31), step) + rng.normal(0, 0.3, (30, 2))
        data["gt_preds"].append(torch.from_numpy(gt[None].astype(np.float32)).cuda())
        data["has_preds"].append(torch.ones(1, 30, dtype=torch.bool).cuda())
    x = roi_feat.clone().requires_grad_(True)

    def step(on):
        R.Decode.train_hip = on
        try:
            m.zero_grad(set_to_none=True)
            x.grad = None
            logits, goals, trajs = m(x, sub, data)
            lo = loss({"pred_logics": logits, "pred_goals": goals, "pred_trajs": trajs}, data)
            lo["loss"].backward()
            return lo["loss"].detach()
        finally:
            R.Decode.train_hip = False

    names = {"off": False, "on": True}
    times = {k: [] for k in names}
    for _ in range(max(args.warmup, 3)):
        for on in names.values():
            step(on)
    torch.cuda.synchronize()
    for _ in range(max(args.steps, 20)):
        for name, on in names.items():
            t0 = time.perf_counter()
            step(on)
            torch.cuda.synchronize()
            times[name].append((time.perf_counter() - t0) * 1e3)
    launches = {name: count_launches(lambda on=on: step(on)) for name, on in names.items()}
    values = {name: float(step(on)) for name, on in names.items()}
    res = {"metric": "Decode + Loss forward + backward, %d interest agents x %d nodes" % (args.agents, args.nodes),
           "mma": ops.get_mma(), "steps": len(times["on"]), "median_ms": {k: float(np.median(v)) for k, v in times.items()},
           "min_ms": {k: min(v) for k, v in times.items()}, "launches_per_step": launches, "loss": values}
    for name in names:
        print("Decode + Loss step, train_hip %s: median %.3f ms (min %.3f), %s launches" % (name, res["median_ms"][name],
                                                                                          res["min_ms"][name], launches[name]), flush=True)
    print(json.dumps(res), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--agents", type=int, default=32)
    ap.add_argument("--nodes", type=int, default=300)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--mma", default=None)
    ap.add_argument("--train", action="store_true")
    args = ap.parse_args()
    if args.mma:
        ops.set_mma(args.mma)
    if args.train:
        return train_mode(args)
    torch.manual_seed(0)
    m = R.Decode(M.config).cuda().eval()
    sub, data, roi_feat = make_inputs(args.agents, args.nodes)
    run = {"hip": lambda: m.decode(roi_feat, sub, data), "stock": lambda: stock_decode(m, roi_feat, sub, data)}
    times = {name: [] for name in run}
    with torch.no_grad():
        for _ in range(args.warmup):
            for f in run.values():
                f()
        torch.cuda.synchronize()
        for _ in range(args.steps):
            for name, f in run.items():
                t0 = time.perf_counter()
                f()
                torch.cuda.synchronize()
                times[name].append((time.perf_counter() - t0) * 1e3)
        hip, stock = run["hip"](), run["stock"]()
    same = bool(torch.equal(hip["top_idx"].long(), stock[3]))
    diff = float((hip["pred_trajs"] - stock[2]).abs().max())
    res = {"metric": "Decode.forward, %d interest agents x %d nodes" % (args.agents, args.nodes), "mma": ops.get_mma(),
           "steps": args.steps, "median_ms": {k: float(np.median(v)) for k, v in times.items()},
           "min_ms": {k: min(v) for k, v in times.items()}, "same_top_k": same, "max_abs_diff_pred_trajs": diff}
    for name in run:
        print("Decode.forward, %s: median %.3f ms (min %.3f)" % (name, res["median_ms"][name], res["min_ms"][name]), flush=True)
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
