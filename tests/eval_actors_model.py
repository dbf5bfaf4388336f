"""Float64 numpy model of the per-actor evaluation (lgcn_eval_actors' record, lgcn_eval_reduce_sel's sums), built on the
definitions of tests/eval_model.py and generalised by PredLoss's rule (reference lanegcn.py:740-807): with
O = {t < horizon : has[t]}, n_obs = |O| and t_last = max O, the final displacement is taken at t_last and the mean
displacement over O; an actor without an observed step is not evaluated; gt at an unobserved step is never looked at.

`variant` builds deliberately wrong records, which the host test uses to show that the GPU test's bars tell a wrong
kernel from a right one:
  "ade_over_horizon"   the sum over O divided by horizon instead of n_obs
  "fde_at_end"         the final displacement taken at horizon - 1 instead of t_last
  "gt_checked_always"  gt tested for finiteness at every step < horizon, observed or not"""
import numpy as np

import eval_model as EM

REC = EM.REC
WHO = {"all": 0, "agent": 1, "others": 2}


def record(reg, cls, gt, has, horizon, local=0, variant=None):
    """One actor: reg [M, T, 2], cls [M], gt [T, 2], has [T] -> the 32 floats of its record, in float64."""
    reg, cls, gt = np.asarray(reg), np.asarray(cls), np.asarray(gt)
    M, H = reg.shape[0], int(horizon)
    out = np.zeros(REC, np.float64)
    out[3] = local
    obs = np.nonzero(np.asarray(has)[:H])[0]
    if obs.size == 0:
        return out
    gt_seen = gt[:H] if variant == "gt_checked_always" else gt[obs]
    if not (np.isfinite(reg[:, :H]).all() and np.isfinite(cls).all() and np.isfinite(gt_seen).all()):
        out[0] = 2.0
        return out
    t_last = H - 1 if variant == "fde_at_end" else int(obs[-1])
    with np.errstate(invalid="ignore", over="ignore"):
        d = reg[:, :H].astype(np.float64) - gt[None, :H].astype(np.float64)
        dist = np.sqrt(d[..., 0] ** 2 + d[..., 1] ** 2)                # [M, H]
    fde = dist[:, t_last]
    # contiguous rows: numpy then adds a fully observed row in the order of eval_model's mean(1)
    ade = np.ascontiguousarray(dist[:, obs]).sum(1) / (H if variant == "ade_over_horizon" else obs.size)
    out[:3] = 1.0, M, H
    out[28], out[29] = H - obs.size, H - 1 - int(obs[-1])
    c = cls.astype(np.float64)
    for k in range(1, M + 1):
        j = 0
        for i in range(1, k):                                        # strict <: the first index wins a tie
            if fde[i] < fde[j]:
                j = i
        e = np.exp(c[:k] - c[:k].max())
        out[4 + 3 * (k - 1):7 + 3 * (k - 1)] = fde[j], ade[j], e[j] / e.sum()
    return out


def records(reg, cls, gt, has, actor_off, horizon, variant=None):
    """A batch -> [A, 32]: row a is actor a, its local index counted from its scene's first row."""
    A = len(reg)
    out = np.zeros((A, REC), np.float64)
    for b in range(len(actor_off) - 1):
        for a in range(int(actor_off[b]), int(actor_off[b + 1])):
            out[a] = record(reg[a], cls[a], gt[a], has[a], horizon, a - int(actor_off[b]), variant)
    return out


def record_f32(reg, cls, gt, t_last):
    """p_k of one evaluated actor by the same formula in numpy float32 (the yardstick of the p_k tolerance) -> [M]:
    eval_model.record_f32 with the final displacement at t_last."""
    return EM.record_f32(reg, cls, gt, t_last + 1)


def excluded(rec, who, max_missing):
    """The rows of the table [n, 32] that the selection (who: "all" / "agent" / "others"; a flag-1 record counts only with
    [28] <= max_missing) leaves out -> bool [n]."""
    rec = np.asarray(rec, np.float64).reshape(-1, REC)
    first = rec[:, 3] == 0.0
    out = ~first if who == "agent" else first.copy() if who == "others" else np.zeros(len(rec), bool)
    return out | ((rec[:, 0] == 1.0) & ~(rec[:, 28] <= max_missing))


def zeroed(rec, who, max_missing):
    """A copy of the table with the excluded rows zeroed."""
    out = np.array(rec, copy=True).reshape(-1, REC)
    out[excluded(rec, who, max_missing)] = 0
    return out


def reduce_sel(rec, who, max_missing, miss_thr=2.0):
    """-> (out [8, 6] float64, cnt [4] int64) as lgcn_eval_reduce_sel defines them; the sums run through math.fsum
    (eval_model.reduce over the kept rows)."""
    rec = np.asarray(rec, np.float64).reshape(-1, REC)
    ex = excluded(rec, who, max_missing)
    out, cnt = EM.reduce(rec[~ex], miss_thr)
    return out, np.concatenate([cnt, [ex.sum()]]).astype(np.int64)


def summary(rec, who="all", min_obs=1, horizon=None, miss_thr=2.0, ks=(6, 1)):
    out, cnt = reduce_sel(rec, who, horizon - min_obs, miss_thr)
    n = int(cnt[1])
    res = {int(k): {m: (out[k - 1, EM.COLUMN[m]] / n if n else float("nan")) for m in EM.METRICS} for k in ks}
    res.update(n_evaluated=n, n_skipped=int(cnt[0]), n_nonfinite=int(cnt[2]), n_excluded=int(cnt[3]))
    return res
