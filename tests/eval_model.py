"""Float64 numpy model of the split evaluation (lgcn_eval_scenes' record, lgcn_eval_reduce's sums, Evaluator.summary),
written from the definitions of Argoverse's get_displacement_errors_and_miss_rate:

  for K = k, over the first k modes as they come: j* = the first mode of the smallest final displacement (strict <),
  minFDE_k = that displacement, minADE_k = the mean displacement of mode j* (picked by FDE, not by ADE),
  p_k = softmax(cls[:k])[j*]; MR counts minFDE_k > miss_thr; brier-minFDE / brier-minADE add (1 - p_k)^2;
  p-minADE adds min(-log p_k, -log 0.05).

`pick` and `drop_last` build deliberately wrong variants (mode picked by ADE; the last step left out), which the host
test uses to show that the tolerances tell a wrong kernel from a right one."""
import numpy as np

REC = 32
METRICS = ("minADE", "minFDE", "MR", "p-minADE", "brier-minADE", "brier-minFDE")
COLUMN = {"minADE": 0, "minFDE": 1, "MR": 2, "brier-minFDE": 3, "brier-minADE": 4, "p-minADE": 5}


def record(reg, cls, gt, has, horizon, pick="fde", drop_last=False):
    """One agent: reg [M, T, 2], cls [M], gt [T, 2], has [T] -> the 32 floats of its record, in float64."""
    reg, cls, gt = np.asarray(reg), np.asarray(cls), np.asarray(gt)
    M, H = reg.shape[0], int(horizon)
    out = np.zeros(REC, np.float64)
    if not np.asarray(has)[:H].all():
        return out
    if not (np.isfinite(reg[:, :H]).all() and np.isfinite(cls).all() and np.isfinite(gt[:H]).all()):
        out[0] = 2.0
        return out
    steps = H - 1 if drop_last and H > 1 else H
    d = reg[:, :steps].astype(np.float64) - gt[None, :steps].astype(np.float64)
    dist = np.sqrt(d[..., 0] ** 2 + d[..., 1] ** 2)                 # [M, steps]
    fde, ade = dist[:, -1], dist.mean(1)
    out[:3] = 1.0, M, H
    c = cls.astype(np.float64)
    for k in range(1, M + 1):
        key = fde if pick == "fde" else ade
        j = 0
        for i in range(1, k):                                        # strict <: the first index wins a tie
            if key[i] < key[j]:
                j = i
        e = np.exp(c[:k] - c[:k].max())
        out[4 + 3 * (k - 1):7 + 3 * (k - 1)] = fde[j], ade[j], e[j] / e.sum()
    return out


def records(reg, cls, gt, has, actor_off, horizon, **variant):
    """A batch: reg [A, M, T, 2], ..., actor_off [B + 1] -> [B, 32]; scene b is its first actor row, a scene without one is 0."""
    B = len(actor_off) - 1
    out = np.zeros((B, REC), np.float64)
    for b in range(B):
        a = int(actor_off[b])
        if int(actor_off[b + 1]) > a:
            out[b] = record(reg[a], cls[a], gt[a], has[a], horizon, **variant)
    return out


def record_f32(reg, cls, gt, horizon):
    """p_k of one evaluated agent by the same formula in numpy float32 (the yardstick of the p_k tolerance) -> [M]."""
    reg, cls, gt = np.asarray(reg, np.float32), np.asarray(cls, np.float32), np.asarray(gt, np.float32)
    M, H = reg.shape[0], int(horizon)
    d = reg[:, H - 1] - gt[None, H - 1]
    fde = np.sqrt(d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1])
    p = np.zeros(M, np.float32)
    for k in range(1, M + 1):
        j = int(np.argmin(fde[:k]))
        e = np.exp(cls[:k] - cls[:k].max())
        p[k - 1] = e[j] / e.sum(dtype=np.float32)
    return p


def reduce(rec, miss_thr=2.0):
    """The record table [n, 32] (any float dtype) -> (out [8, 6] float64, cnt [3] int64) as lgcn_eval_reduce defines them.
    Sums run through math.fsum: the model carries no summation error of its own."""
    import math
    rec = np.asarray(rec, np.float64).reshape(-1, REC)
    flag = rec[:, 0]
    cnt = np.array([(flag != 1.0).sum() - (flag == 2.0).sum(), (flag == 1.0).sum(), (flag == 2.0).sum()], np.int64)
    ok = rec[flag == 1.0]
    if len(ok) and (np.any(ok[:, 1] != ok[0, 1]) or np.any(ok[:, 2] != ok[0, 2])):
        raise ValueError("records of different M / horizon")
    out = np.zeros((8, 6), np.float64)
    clip = -math.log(0.05)
    for k in range(1, 9):
        r = ok[ok[:, 1] >= k]
        fde, ade, p = r[:, 4 + 3 * (k - 1)], r[:, 5 + 3 * (k - 1)], r[:, 6 + 3 * (k - 1)]
        with np.errstate(divide="ignore"):
            nl = np.minimum(-np.log(p), clip)
        cols = (ade, fde, (fde > miss_thr).astype(np.float64), (1.0 - p) ** 2 + fde, (1.0 - p) ** 2 + ade, nl + ade)
        out[k - 1] = [math.fsum(c) for c in cols]
    return out, cnt


def summary(rec, miss_thr=2.0, ks=(6, 1)):
    out, cnt = reduce(rec, miss_thr)
    n = int(cnt[1])
    res = {int(k): {m: (out[k - 1, COLUMN[m]] / n if n else float("nan")) for m in METRICS} for k in ks}
    res.update(n_evaluated=n, n_skipped=int(cnt[0]), n_nonfinite=int(cnt[2]))
    return res
