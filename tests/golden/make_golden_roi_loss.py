"""Generates tests/golden/lanercnn_roi_loss.npz by running the REFERENCE's own RoiLoss and Loss (lanercnn.py:1205-1325)
on the CPU on small hand-built inputs, imported read-only with the shims of make_golden.py / make_golden_decode.py.
Run in the build container only:
    python tests/golden/make_golden_roi_loss.py
The fixture holds inputs, the two index decisions, every numeric loss_out entry and the reference's own autograd
gradients of loss_out["loss"] (data), never reference source.

The indices are captured by wrapping Tensor.max / Tensor.min while the reference's forward runs.  The script searches
seeds until no decision of the loss hangs on rounding and ASSERTS the margins it prints."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden_decode as MD  # noqa: E402  (also puts the repository and tests/ on sys.path)

A, M, T = 37, 6, 30
PATTERNS = ("all", "tail", "hole", "none", "first")


def has_pattern(rng, kind):
    h = np.ones(T, dtype=bool)
    if kind == "tail":
        h[int(rng.integers(5, T - 1)):] = False
    elif kind == "hole":
        lo = int(rng.integers(3, 12))
        h[lo:lo + int(rng.integers(2, 10))] = False
    elif kind == "none":
        h[:] = False
    elif kind == "first":
        h[1:] = False
    return h


def loss_inputs(rng):
    """A scenes; per scene 2-4 agents of which two are valid, the first valid one is the agent of interest."""
    data = {"valid_agent_ids": [], "gt_preds": [], "has_preds": []}
    out = {"pred_logics": rng.normal(0, 2.0, (A, M)).astype(np.float32),
           "pred_goals": np.zeros((A, M, 2), np.float32), "pred_trajs": np.zeros((A, M, T, 2), np.float32)}
    kinds = []
    for b in range(A):
        n_agents = 2 + b % 3
        valid = np.sort(rng.choice(n_agents, 2, replace=False)).astype(np.int64)
        heading, speed = rng.uniform(0, 2 * np.pi), rng.uniform(2.0, 12.0)
        step = np.array([np.cos(heading), np.sin(heading)]) * speed * 0.1
        gt = (rng.normal(0, 5.0, (n_agents, 1, 2)) + (np.arange(T)[None, :, None] + 1) * step[None, None]
              + rng.normal(0, 0.1, (n_agents, T, 2))).astype(np.float32)
        has = np.stack([has_pattern(rng, PATTERNS[int(rng.integers(0, 5))]) for _ in range(n_agents)])
        kind = PATTERNS[b % 5]                               # the agent of interest cycles through every pattern
        has[valid[0]] = has_pattern(rng, kind)
        kinds.append(kind)
        # residuals on both sides of the SmoothL1 knee: scenes alternate between small and large errors
        scale = 0.3 if b % 2 == 0 else 2.5
        for j in range(M):
            off = rng.normal(0, scale, 2) * (0.5 + 0.5 * j)
            out["pred_trajs"][b, j] = gt[valid[0]] + off + rng.normal(0, scale, (T, 2))
            out["pred_goals"][b, j] = gt[valid[0], -1] + off + rng.normal(0, scale, 2)
        data["valid_agent_ids"].append(valid)
        data["gt_preds"].append(gt)
        data["has_preds"].append(has)
    return out, data, kinds


def run_loss(rl, torch, loss, out, data):
    """The reference's Loss.forward with Tensor.max / Tensor.min wrapped; returns loss_out, the indices, the gradients."""
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a))
    cap = {"max": [], "min": []}
    real_max, real_min = torch.Tensor.max, torch.Tensor.min

    def spy_max(self, *a, **k):
        r = real_max(self, *a, **k)
        if a == (1,):
            cap["max"].append((self.detach().numpy().copy(), r[1].numpy().copy()))
        return r

    def spy_min(self, *a, **k):
        r = real_min(self, *a, **k)
        if a == (-1,):
            cap["min"].append((self.detach().numpy().copy(), r[1].numpy().copy()))
        return r

    o = {k: t(v).clone().requires_grad_(True) for k, v in out.items()}
    d = {k: [t(x) for x in v] for k, v in data.items()}
    torch.Tensor.max, torch.Tensor.min = spy_max, spy_min
    try:
        loss_out = loss(o, d)
    finally:
        torch.Tensor.max, torch.Tensor.min = real_max, real_min
    assert len(cap["max"]) == 1 and len(cap["min"]) == 1
    loss_out["loss"].backward()
    grads = {"d_logits": o["pred_logics"].grad.numpy().copy(), "d_goals": o["pred_goals"].grad.numpy().copy(),
             "d_trajs": o["pred_trajs"].grad.numpy().copy()}
    return loss_out, cap, grads


def main():
    rl = MD.import_lanercnn()
    import torch
    torch.set_num_threads(1)
    loss = rl.Loss(rl.config)
    for seed in range(300, 400):
        out, data, kinds = loss_inputs(np.random.default_rng(seed))
        loss_out, cap, grads = run_loss(rl, torch, loss, out, data)
        last_vals, last_idcs = cap["max"][0]
        dist, min_idcs = cap["min"][0]
        first = [int(v[0]) for v in data["valid_agent_ids"]]
        gt = np.stack([data["gt_preds"][b][first[b]] for b in range(A)])
        has = np.stack([data["has_preds"][b][first[b]] for b in range(A)])
        rows = np.arange(A)
        two = np.sort(dist.astype(np.float64), 1)[:, :2]
        gap = float((two[:, 1] - two[:, 0]).min())
        res_goal = (out["pred_goals"][rows, min_idcs].astype(np.float64) - gt[rows, last_idcs])[has[rows, last_idcs]]
        res_traj = (out["pred_trajs"][rows, min_idcs].astype(np.float64) - gt)[has]
        res = np.concatenate([res_goal.reshape(-1), res_traj.reshape(-1)])
        knee = float(np.abs(np.abs(res) - 1.0).min())
        sides = (int((np.abs(res) < 1).sum()), int((np.abs(res) > 1).sum()))
        srt = np.sort(last_vals.astype(np.float64), 1)
        last_gap = float((srt[:, -1] - srt[:, -2]).min())
        print("seed %d: dist gap %.3e, distance to the knee %.3e, residuals below / above 1: %s, last-step gap %.3e"
              % (seed, gap, knee, sides, last_gap))
        if gap >= 1e-3 and knee >= 1e-3:
            break
    assert gap >= 1e-3, "the two smallest dist_j of some agent differ by less than 1e-3"
    assert knee >= 1e-3, "a residual lies within 1e-3 of +-1"
    assert min(sides) >= 50, "the residuals do not fall on both sides of the SmoothL1 knee"
    assert sorted(set(kinds)) == sorted(PATTERNS)
    assert has.all(1).any() and (~has).all(1).any() and any(h[0] and not h[1:].any() for h in has)
    assert any(h[0] and not h[-1] and h.sum() > 1 for h in has) and any(h[0] and h[-1] and not h.all() for h in has)
    assert np.array_equal(last_idcs[(~has).all(1)], np.full(int((~has).all(1).sum()), T - 1))
    fx = {"seed": np.int64(seed), "margins": np.asarray([gap, knee]), "reg_coef": np.float64(rl.config["reg_coef"]),
          "logits": out["pred_logics"], "goals": out["pred_goals"], "trajs": out["pred_trajs"], "gt": gt, "has": has,
          "last_idcs": last_idcs.astype(np.int64), "min_idcs": min_idcs.astype(np.int64)}
    for b in range(A):
        for k in data:
            fx["data/%s/%d" % (k, b)] = data[k][b]
    for k, v in loss_out.items():
        if k in ("pred_trajs",):
            continue                                          # the input itself
        fx["loss_out/" + k] = v.detach().numpy().copy() if torch.is_tensor(v) else np.asarray(v)
    fx.update(grads)
    assert all(np.isfinite(v).all() for v in fx.values())
    path = os.path.join(HERE, "lanercnn_roi_loss.npz")
    np.savez_compressed(path, **fx)
    assert os.path.getsize(path) < 1000000
    print("wrote lanercnn_roi_loss.npz (%d bytes), seed %d: dist gap %.3e, distance to the knee %.3e" % (os.path.getsize(path), seed, gap, knee))
    print("loss_out:", {k: (float(v) if np.ndim(v) == 0 else v.shape) for k, v in fx.items() if k.startswith("loss_out/")})


if __name__ == "__main__":
    main()
