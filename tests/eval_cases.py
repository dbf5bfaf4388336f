"""Generated inputs of the split-evaluation tests (numpy only; the GPU tests and the host test of the separation
conditions read the same cases).

A case is a batch: B scenes with 0 / 1 / 3 / 50 actors each (so the first row of a scene is not row 0; for B >= 5 empty
scenes sit first, last and in the middle), world-scale coordinates (|x| up to 5e3), M modes whose final displacement
from the ground truth climbs a ladder of ratio >= 1.3 between 1e-2 and 30 m in a random mode order, per-step errors that
wander by a factor 0.2 .. 3 (the mode of the best ADE is often not the mode of the best FDE), and scores of span 0 (all
equal) in the even scenes and 40 in the odd ones (softmax needs the maximum subtracted).

Guaranteed by construction and checked by tests/test_eval_model_host.py on every scene: per K the two smallest final
displacements differ by more than 1e-4 relative, and no minFDE_K lies within 1e-3 relative of the miss threshold 2.0."""
import numpy as np

SHAPES = ((1, 1, 1), (6, 30, 30), (6, 30, 10), (8, 64, 64), (3, 33, 33))      # (M, T, horizon)
BATCHES = (1, 5, 67)
ACTORS = (0, 1, 3, 50)
MISS_THR = 2.0
CASES = [(m, t, h, b) for (m, t, h) in SHAPES for b in BATCHES]


def case_id(c):
    return "M%d-T%d-H%d-B%d" % c


def _agent(rng, M, T, H, span):
    """reg [M, T, 2], cls [M], gt [T, 2] of one actor, fp32."""
    while True:
        centre = rng.uniform(-4.9e3, 4.9e3, 2)
        gt = centre + np.cumsum(rng.normal(0.0, 0.5, (T, 2)), 0)
        ratio = rng.uniform(1.3, 1.6)
        e0 = np.exp(rng.uniform(np.log(1e-2), np.log(30.0 / ratio ** (M - 1))))
        size = e0 * ratio ** rng.permutation(M)                         # final displacement per mode
        wander = rng.uniform(0.2, 3.0, (M, T))
        wander[:, H - 1] = 1.0
        ang = rng.uniform(0.0, 2.0 * np.pi, (M, T))
        err = (size[:, None] * wander)[..., None] * np.stack([np.cos(ang), np.sin(ang)], -1)
        reg = (gt[None] + err).astype(np.float32)
        gt = gt.astype(np.float32)
        if np.abs(reg).max() <= 5e3 and np.abs(gt).max() <= 5e3 and separated(reg, gt, H):
            break
    cls = (rng.uniform(0.0, 1.0, M) * span).astype(np.float32)
    if span and M > 1:
        cls[rng.integers(0, M)] = 0.0
        cls[(int(np.argmin(cls)) + 1) % M] = span                      # the span is reached
    return reg, cls, gt


def final_displacements(reg, gt, H):
    d = reg[:, H - 1].astype(np.float64) - gt[H - 1].astype(np.float64)
    return np.sqrt((d ** 2).sum(1))


def separated(reg, gt, H, rel_gap=1e-4, rel_thr=1e-3):
    """The two separation conditions for one agent, from its fp32 arrays in float64 (a margin of 10 x is kept here)."""
    f = final_displacements(reg, gt, H)
    for k in range(1, len(f) + 1):
        s = np.sort(f[:k])
        if k > 1 and s[1] - s[0] <= 10 * rel_gap * s[1]:
            return False
        if abs(s[0] - MISS_THR) <= 10 * rel_thr * MISS_THR:
            return False
    return True


def sizes_of(rng, B):
    sizes = rng.choice(ACTORS, B)
    if B == 1:
        sizes[:] = 3
    if B >= 5:
        sizes[[0, B // 2, B - 1]] = 0
        sizes[1] = 50
    return [int(s) for s in sizes]


def make_case(M, T, H, B, seed=0):
    """-> dict(reg [A, M, T, 2], cls [A, M], gt [A, T, 2] fp32, has [A, T] bool (all set), actor_off [B + 1] int32,
    M, T, horizon)."""
    rng = np.random.default_rng([seed, M, T, H, B])
    sizes = sizes_of(rng, B)
    reg, cls, gt = [], [], []
    for b, n in enumerate(sizes):
        for _ in range(n):
            r, c, g = _agent(rng, M, T, H, 0.0 if b % 2 == 0 else 40.0)
            reg.append(r), cls.append(c), gt.append(g)
    A = sum(sizes)
    stack = lambda xs, shape: np.stack(xs).astype(np.float32) if xs else np.zeros((0,) + shape, np.float32)
    return dict(reg=stack(reg, (M, T, 2)), cls=stack(cls, (M,)), gt=stack(gt, (T, 2)), has=np.ones((A, T), bool),
                actor_off=np.concatenate([[0], np.cumsum(sizes)]).astype(np.int32), M=M, T=T, horizon=H)


def make_records(n, M, H, seed=0, flags=(0, 1, 1, 1, 2)):
    """A record table [n, 32] fp32 with mixed flags for the reduce tests: plausible minFDE / minADE / p values, some p below
    0.05 (the clip of p-minADE) and some exactly 0, no minFDE within 1e-3 relative of the miss threshold."""
    rng = np.random.default_rng([seed, n, M, H])
    rec = np.zeros((n, 32), np.float32)
    flag = rng.choice(flags, n)
    rec[:, 0] = flag
    ok = flag == 1
    rec[ok, 1], rec[ok, 2] = M, H
    for k in range(M):
        fde = np.exp(rng.uniform(np.log(1e-2), np.log(30.0), n))
        near = np.abs(fde - MISS_THR) <= 2e-3 * MISS_THR
        fde[near] = MISS_THR * 1.01
        p = rng.uniform(0.0, 1.0, n) ** 3
        p[rng.random(n) < 0.05] = 0.0
        rec[ok, 4 + 3 * k] = fde[ok]
        rec[ok, 5 + 3 * k] = (fde * rng.uniform(0.3, 1.2, n))[ok]
        rec[ok, 6 + 3 * k] = p[ok]
    return rec
