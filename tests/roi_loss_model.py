"""float64 restatement of the fork model's RoiLoss and Loss (reference lanercnn.py:1214-1325) -- TEST INFRASTRUCTURE
ONLY.  Written from the formulas; pinned against the reference's own run (tests/golden/lanercnn_roi_loss.npz) by
test_roi_loss_model_host.py, and then the yardstick of the GPU tests.

Everything real is torch in the dtype of its inputs (float64 in the tests) and differentiable.  The two index
decisions (last observed step, closest mode) can be handed in, so that a float64 run uses the fp32 run's indices."""
import os

import numpy as np
import torch
import torch.nn.functional as F


def last_step(has):
    """has [A, T] bool -> first arg-max of has + 0.1 t / T, formed in fp32 as the reference forms it (:1234-1235)."""
    T = has.shape[1]
    last = has.float() + 0.1 * torch.arange(T).float() / float(T)
    return last.max(1)[1]


def closest_mode(goals, gt, last_idcs):
    """First arg-min over the modes of the distance goal - gt[last] (:1246-1258)."""
    rows = torch.arange(len(last_idcs))
    dist = torch.sqrt(((goals - gt[rows, last_idcs].unsqueeze(1)) ** 2).sum(-1))          # [A, M]
    return dist.min(-1)[1], dist


def smooth_l1_sum(x):
    a = x.abs()
    return torch.where(a < 1.0, 0.5 * x * x, a - 0.5).sum()


def roi_loss(logits, goals, trajs, gt, has, reg_coef=1.0, last_idcs=None, min_idcs=None):
    """RoiLoss.forward on the first-agent tensors: logits [A, M], goals [A, M, 2], trajs [A, M, T, 2], gt [A, T, 2],
    has [A, T] bool.  Returns the reference's loss_out entries plus last_idcs / min_idcs."""
    A = logits.shape[0]
    rows = torch.arange(A)
    if last_idcs is None:
        last_idcs = last_step(has)
    last_idcs = torch.as_tensor(last_idcs, dtype=torch.long)
    if min_idcs is None:
        min_idcs = closest_mode(goals.detach(), gt, last_idcs)[0]
    min_idcs = torch.as_tensor(min_idcs, dtype=torch.long)
    y = torch.zeros_like(logits)
    y[rows, min_idcs] = 1
    x = logits
    mv = (-x).clamp_min(0)
    cls = ((1 - y) * x + mv + torch.log(torch.exp(-mv) + torch.exp(-x - mv))).sum()
    has_goal = has[rows, last_idcs]
    best_goals = goals[rows, min_idcs]
    goal = reg_coef * smooth_l1_sum((best_goals - gt[rows, last_idcs])[has_goal])
    traj = reg_coef * smooth_l1_sum((trajs[rows, min_idcs] - gt)[has])
    return {"cls_loss": cls, "num_cls": A, "reg_goal_loss": goal, "num_reg_goal": int(has_goal.sum()),
            "reg_traj_loss": traj, "num_reg_traj": int(has.sum()), "stage_one_loss": 0, "num_stage_one": 1,
            "pred_goals": best_goals, "pred_trajs": trajs, "last_idcs": last_idcs, "min_idcs": min_idcs}


def total(loss_out):
    """Loss.forward's combination (:1320-1323)."""
    return (loss_out["cls_loss"] / (loss_out["num_cls"] + 1e-10) + loss_out["reg_goal_loss"] / (loss_out["num_reg_goal"] + 1e-10)
            + loss_out["reg_traj_loss"] / (loss_out["num_reg_traj"] + 1e-10)
            + loss_out["stage_one_loss"] / (loss_out["num_stage_one"] + 1e-10))


def loss_and_grads(logits, goals, trajs, gt, has, reg_coef=1.0, last_idcs=None, min_idcs=None, dtype=torch.float64):
    """numpy in, numpy out: the loss entries and the gradients of `loss` with respect to logits, goals and trajs."""
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dtype)
    xs = [t(a).requires_grad_(True) for a in (logits, goals, trajs)]
    out = roi_loss(xs[0], xs[1], xs[2], t(gt), torch.from_numpy(np.ascontiguousarray(has)).bool(), reg_coef, last_idcs, min_idcs)
    out["loss"] = total(out)
    out["loss"].backward()
    res = {k: (v.detach().numpy() if torch.is_tensor(v) else v) for k, v in out.items()}
    res.update(d_logits=xs[0].grad.numpy(), d_goals=xs[1].grad.numpy(), d_trajs=xs[2].grad.numpy())
    return res


_cache = {}


def fixture():
    """tests/golden/lanercnn_roi_loss.npz: inputs, indices, loss entries and gradients of the reference's own run."""
    if "fx" not in _cache:
        here = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
        with np.load(os.path.join(here, "lanercnn_roi_loss.npz")) as z:
            _cache["fx"] = {k: z[k] for k in z.files}
    return _cache["fx"]


def tiled(rows=None):
    """The fixture's first-agent tensors, its rows repeated in order until there are `rows` of them (default: as they
    are), with the reference's indices."""
    g = fixture()
    n = g["logits"].shape[0]
    rows = n if rows is None else rows
    rep = lambda a: np.concatenate([a] * (rows // n + 1), 0)[:rows]
    return {k: rep(g[k]) for k in ("logits", "goals", "trajs", "gt", "has", "last_idcs", "min_idcs")}


def reference(rows=None, dtype=torch.float64):
    """The model on tiled(rows) with the reference's indices, in float64 (the yardstick) or in fp32 (the reference's own
    arithmetic, whose distance from the yardstick sets the bars); computed once per (rows, dtype), never modified."""
    key = ("ref", rows, dtype)
    if key not in _cache:
        a = tiled(rows)
        _cache[key] = loss_and_grads(a["logits"], a["goals"], a["trajs"], a["gt"], a["has"], float(fixture()["reg_coef"]),
                                     a["last_idcs"], a["min_idcs"], dtype=dtype)
    return _cache[key]


def rel_err(got, ref):
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    return float(np.abs(got - ref).max() / max(np.abs(ref).max(), 1e-300))
