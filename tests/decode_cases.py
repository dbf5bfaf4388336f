"""Synthetic inputs of the goal decoder (csrc/lgcn_goal.hip, csrc/lgcn_goal_bwd.hip) -- TEST INFRASTRUCTURE ONLY.  No GPU
and no import of the library: numpy fp32 arrays in the layout ops.goal_decode takes, from fixed seeds, built once per
process and read-only.  Pinned by test_decode_cases_host.py, used by test_gpu_goal_decode_edges.py.

Index decisions are the same in fp32 and in float64: anchor centres and the offsets pred[:, 1:3] are multiples of 0.25 m
with |coordinate| <= 50 m, so anc + pred and every squared distance are exact in fp32; sqrt is monotone and
sqrt(4) = 2, so `dist < 2.0` decides alike -- pairs exactly 2.0 apart included.  Logits are distinct unless a case
says otherwise.

Conditions the values are built to meet (asserted by the host test, so that fp32 and float64 take the same branches):
every denominator |2 + d - p| of a goal heading is >= 0.25 (every node heads within 1.2 rad of its agent), every
|pred[:, 4]| >= 0.5, and every float64 speed v_j, j >= 1, of a selected mode is at least 1e-3 from 0 (a random
velocity is redrawn until its agent's modes meet that; the fixed ones are met by the seed)."""
import numpy as np
import torch

import decode_model as DM

K = 6
GRID = 0.25
PLANTED = (256, 255, 64, 63, 0, 192)            # second pass, last thread, the wave seams, index 0, a wave's first lane
SPREAD_SIZES = (6, 7, 255, 256, 257, 300, 600, 1025)
DIR_KINDS = ("random", "zero", "below", "above")
VEL_KINDS = ("random", "zero", "fast")
SPEED_MARGIN = 1e-3

_cache = {}


def _grid(rng, shape, lim):
    """Multiples of 0.25 in [-lim, lim]."""
    q = int(round(lim / GRID))
    return rng.integers(-q, q + 1, shape) * GRID


def _logits(rng, n):
    return rng.permutation(n) * 0.01 - 3.0


def _place(lg, idx, rank):
    """Swap logits so that node idx holds the one of the given rank (0 = best)."""
    j = int(np.argsort(-lg)[rank])
    lg[idx], lg[j] = lg[j], lg[idx]


def _spread_xy(rng, n, lim=40.0):
    return _grid(rng, (n, 2), lim), _grid(rng, (n, 2), 2.0)


def _disc_xy(rng, n, bases):
    """Every node inside one of the 0.5 m squares at `bases` (chosen at random per node), zero offsets."""
    bases = np.asarray(bases, dtype=np.float64)
    which = rng.integers(0, len(bases), n)
    which[:len(bases)] = np.arange(len(bases))           # every square is used
    return bases[which] + rng.integers(0, 3, (n, 2)) * GRID, np.zeros((n, 2))


def _roi(name, xy, off, logit):
    return {"name": name, "xy": np.asarray(xy, dtype=np.float64), "off": np.asarray(off, dtype=np.float64),
            "logit": np.asarray(logit, dtype=np.float64)}


def _selection_rois(rng):
    rois = []
    for n in SPREAD_SIZES:
        xy, off = _spread_xy(rng, n)
        rois.append(_roi("spread%d" % n, xy, off, _logits(rng, n)))
    xy, off = _disc_xy(rng, 300, [(12.0, -7.0)])
    lg = _logits(rng, 300)
    _place(lg, 299, 2)                                   # pads from the second pass of the 256-thread loops
    _place(lg, 256, 4)
    rois.append(_roi("one_disc300", xy, off, lg))
    xy, off = _disc_xy(rng, 257, [(-14.0, 9.0), (-6.0, 9.0)])
    lg = _logits(rng, 257)
    _place(lg, 256, 3)                                   # the one node of the second pass is a pad
    rois.append(_roi("two_discs257", xy, off, lg))
    # the six best logits on chosen indices, far apart: all six are selected, in this order
    xy, off = _spread_xy(rng, 257)
    lg = _logits(rng, 257)
    for j, i in enumerate(PLANTED):
        xy[i] = (-30.0 + 30.0 * (j % 3), -20.0 + 40.0 * (j // 3))
        lg[i] = 20.0 - j
    rois.append(_roi("planted257", xy, off, lg))
    # all logits equal, two squares: survivors and pads both go to the lower index
    xy, off = _disc_xy(rng, 40, [(8.0, 8.0), (16.0, 8.0)])
    off = _grid(rng, (40, 2), 2.0)
    rois.append(_roi("equal40", xy, off, np.full(40, 0.5)))
    # two NaN logits, far apart: they rank first, the lower index before the higher
    xy, off = _spread_xy(rng, 12, 6.0)
    lg = _logits(rng, 12)
    xy[9], xy[4] = (-20.0, 12.0), (20.0, -12.0)
    lg[9] = lg[4] = np.nan
    rois.append(_roi("nan12", xy, off, lg))
    # nodes 0 / 1 exactly 2.0 apart (both kept: the comparison is strict), nodes 2 / 3 1.75 apart (3 is dropped)
    xy = np.array([(0, 0), (2, 0), (10, 0), (11.75, 0), (20, 0), (0, 10), (10, 10), (20, 10)], dtype=np.float64) + (-9.5, 3.25)
    lg = np.array([2.0, 1.9, 1.8, 1.7, 1.6, 1.5, 1.4, 1.3])
    rois.append(_roi("pairs8", xy, _grid(rng, (8, 2), 2.0), lg))
    return rois


def _many_rois(rng, n_agt=300):
    rois = []
    for a in range(n_agt):
        n = int(rng.integers(6, 41))
        xy, off = _spread_xy(rng, n, 6.0)
        rois.append(_roi("small%d" % a, xy, off, _logits(rng, n)))
    return rois


def _agent(rng, a):
    """Agent row a of the cycle: (centre, heading, dir_last, kind of dir_last, kind of velocity)."""
    kind_d, kind_v = DIR_KINDS[a % len(DIR_KINDS)], VEL_KINDS[a % len(VEL_KINDS)]
    ctr = _grid(rng, 2, 5.0) + 0.125                     # never on a goal: no polyline of length 0
    phi = rng.uniform(-np.pi, np.pi)
    speed = rng.uniform(0.1, 2.0)
    if kind_d == "random":
        d = speed * np.array([np.cos(phi), np.sin(phi)])
    elif kind_d == "zero":
        d = np.zeros(2)
    else:
        d = np.array([3.0, 4.0]) * (1e-7 if kind_d == "below" else 1e-6)
        phi = np.arctan2(4.0, 3.0)
    return ctr, phi, d, kind_d, kind_v


def _lengths(case):
    """float64 polyline lengths [A, K] of the selected modes (they do not depend on the velocity)."""
    t64 = lambda x: torch.from_numpy(np.ascontiguousarray(x)).double()
    dec = DM.decode(t64(case["pred"]), case["pred_spans"], t64(case["anc_ctrs"]), t64(case["anc_dirs"]), case["anc_first"],
                    t64(case["agt_ctrs"]), t64(case["dir_last"]), t64(case["agt_vel"]), K)
    pts = DM.poly(torch.arange(0, 31, dtype=torch.float64) / 30, dec["coef"])
    return torch.sqrt(((pts[:, :, 1:] - pts[:, :, :-1]) ** 2).sum(-1)).sum(-1).numpy()


def speeds(length, vel):
    """float64 v_j = vel + acc t_j before the clamp, j = 0..30: [A, K, 31]."""
    length, vel = np.asarray(length, dtype=np.float64), np.asarray(vel, dtype=np.float64).reshape(-1, 1)
    acc = 2 * (length - vel * 3.0) / 9.0
    return vel[:, :, None] + acc[:, :, None] * (np.arange(31) / 10.0)


def _pack(rois, seed, skip=()):
    """One launch: pred rows of the RoIs back to back, their anchors with unused rows between them (anc_first differs
    from the pred offset), one agent row per RoI.  RoIs named in `skip` are left out; the others keep their agent."""
    rng = np.random.default_rng(seed)
    pred, anc_c, anc_d, spans, names, agents = [], [], [], [], [], []
    n_anc = 0
    for a, r in enumerate(rois):
        ctr, phi, d, kind_d, kind_v = _agent(rng, a)
        n = len(r["xy"])
        alpha = phi + rng.uniform(-0.6, 0.6, n)
        beta = rng.uniform(-0.6, 0.6, n)
        p4 = rng.uniform(0.55, 1.5, n) * rng.choice([-1.0, 1.0], n)
        vel_draws = rng.uniform(0.0, 15.0, 64)
        filler = 3 + a % 4
        if r["name"] in skip:
            continue
        anc_c += [np.full((filler, 2), 77.0), r["xy"] - r["off"]]
        anc_d += [np.tile([[0.6, -0.8]], (filler, 1)), np.stack([np.cos(alpha), np.sin(alpha)], 1)]
        spans.append((n_anc + filler, n_anc + filler + n))
        n_anc += filler + n
        pred.append(np.concatenate([r["logit"][:, None], r["off"], (p4 * np.tan(beta))[:, None], p4[:, None]], 1))
        names.append(r["name"])
        agents.append((ctr, d, kind_v, vel_draws, kind_d))
    f = lambda x: np.ascontiguousarray(x, dtype=np.float32)
    sizes = [hi - lo for lo, hi in spans]
    case = {"names": names, "spans": spans, "pred_spans": [0] + [int(v) for v in np.cumsum(sizes)],
            "anc_first": [lo for lo, _ in spans], "pred": f(np.concatenate(pred)),
            "anc_ctrs": f(np.concatenate(anc_c + [np.full((2, 2), 77.0)])),
            "anc_dirs": f(np.concatenate(anc_d + [np.tile([[0.6, -0.8]], (2, 1))])),
            "agt_ctrs": f([g[0] for g in agents]), "dir_last": f([g[1] for g in agents]),
            "dir_kind": [g[4] for g in agents],
            "vel_kind": [g[2] for g in agents]}
    # velocities: 0, 25, or a draw from 0..15 whose speeds stay clear of 0 in every selected mode
    case["agt_vel"] = np.zeros(len(agents), dtype=np.float32)
    length = _lengths(case)
    vel = np.zeros(len(agents), dtype=np.float32)
    for a, (_, _, kind_v, draws, _) in enumerate(agents):
        if kind_v == "fast":
            vel[a] = 25.0
        elif kind_v == "random":
            ok = [v for v in draws.astype(np.float32) if np.abs(speeds(length[a:a + 1], [v])[..., 1:]).min() >= 2 * SPEED_MARGIN]
            vel[a] = ok[0]
    case["agt_vel"] = vel
    for v in case.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return case


def selection_cases(nan_roi=True):
    """One launch of 14 RoIs (13 without the RoI of NaN logits; the other RoIs and their agents are the same)."""
    key = ("selection", nan_roi)
    if key not in _cache:
        if "selection_rois" not in _cache:
            _cache["selection_rois"] = _selection_rois(np.random.default_rng(101))
        _cache[key] = _pack(_cache["selection_rois"], 102, skip=() if nan_roi else ("nan12",))
    return _cache[key]


def many_agents_case():
    """300 agents (more workgroups than the card has CUs) with RoIs of 6..40 nodes within +-6 m."""
    if "many" not in _cache:
        _cache["many"] = _pack(_many_rois(np.random.default_rng(201)), 202)
    return _cache["many"]


def xy_logit(case):
    """Goal positions [n, 2] and logits [n] in pred's row order, fp32 (the sum is exact)."""
    rows = np.concatenate([np.arange(lo, hi) for lo, hi in case["spans"]])
    return case["anc_ctrs"][rows] + case["pred"][:, 1:3], case["pred"][:, 0].copy()


REFINE_ROWS = ("plain", "replaced", "tied_max", "negative", "nan", "zero_samples")
REPLACED_AT, TIED_AT, NAN_AT = 7, (12, 29), 5


def refine_cases():
    """s_samples [6, 30], coef [6, 6], delta [6, 30, 2] (fp32), one row per entry of REFINE_ROWS:
    plain         increasing samples, small delta
    replaced      delta[7, 0] = -s_samples[7] exactly: the sum is 0, the normalised sample is replaced by 1
    tied_max      steps 12 and 29 both hold the row maximum, delta[..., 0] = 0
    negative      every sample (and every sum) negative: the row maximum is negative
    nan           delta[5, 0] = NaN: the maximum, and with it the whole row, is NaN
    zero_samples  s_samples = 0, delta non-zero: the sums are the deltas
    Besides the tie, the two largest sums of a row are >= 1e-2 apart and no sum besides the replaced one is 0."""
    if "refine" not in _cache:
        rng = np.random.default_rng(301)
        R = len(REFINE_ROWS)
        inc = np.cumsum(rng.uniform(0.3, 1.2, (R, 30)), 1)
        delta = rng.normal(0, 0.05, (R, 30, 2))
        s = inc.copy()
        s32 = lambda x: np.asarray(x, dtype=np.float32)
        delta[1, REPLACED_AT, 0] = -float(s32(s[1, REPLACED_AT]))
        s[2, TIED_AT[0]] = s[2, TIED_AT[1]] = s[2].max() + 1.0
        delta[2, :, 0] = 0.0
        s[3] = -inc[3, ::-1] - 1.0
        delta[4, NAN_AT, 0] = np.nan
        s[5] = 0.0
        delta[5, :, 0] = rng.permutation(30) * 0.05 - 0.62
        coef = rng.normal(0, 1, (R, 6)) * np.array([20.0, 10.0, 30.0, 20.0, 10.0, 30.0])
        out = {"s_samples": s32(s), "coef": s32(coef), "delta": s32(delta)}
        for v in out.values():
            v.setflags(write=False)
        _cache["refine"] = out
    return _cache["refine"]


# ---------------------------------------------------------------- the model on a case, on the CPU in float64 or float32
def _t(x, dtype):
    return torch.from_numpy(np.array(x)).to(dtype)               # a copy: the cases are read-only


def model(case, dtype=torch.float64, top_idx=None, pred=None):
    """DM.decode on a case in `dtype` (float32: the reference's formula at the kernels' own precision)."""
    pred = _t(case["pred"], dtype) if pred is None else pred
    return DM.decode(pred, case["pred_spans"], _t(case["anc_ctrs"], dtype), _t(case["anc_dirs"], dtype), case["anc_first"],
                     _t(case["agt_ctrs"], dtype), _t(case["dir_last"], dtype), _t(case["agt_vel"], dtype), K, top_idx=top_idx)


def agent_err(got, ref):
    """Largest per-agent relative error: every agent is held to its own scale."""
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    return max(DM.rel_err(got[a], ref[a]) for a in range(len(ref)))


def bar_of(e32):
    return max(4 * e32, 1e-6)


def value_reference(case, top_idx, keys=("goals", "logits", "coef", "s_samples")):
    """{tensor: (float64 values, bar)} for the given indices; bar = max(4 x per-agent error of the float32 CPU model, 1e-6)."""
    ref, m32 = model(case, torch.float64, top_idx), model(case, torch.float32, top_idx)
    return {k: (ref[k].numpy(), bar_of(agent_err(m32[k].numpy(), ref[k].numpy()))) for k in keys}


def upstream(case, seed):
    """Random upstream gradients (fp32 values) of the four outputs of goal_decode."""
    rng = np.random.default_rng(seed)
    A_ = len(case["spans"])
    return {k: rng.normal(0, 1, s).astype(np.float32)
            for k, s in (("goals", (A_, K, 2)), ("logits", (A_, K)), ("coef", (A_, K, 6)), ("s_samples", (A_, K, 30)))}


def model_d_pred(case, top_idx, w, dtype=torch.float64):
    """d_pred [n, 5] of sum(w * outputs) by CPU autograd of the model in `dtype`."""
    pred = _t(case["pred"], dtype).requires_grad_(True)
    dec = model(case, dtype, top_idx, pred)
    sum((dec[k] * _t(w[k], dtype)).sum() for k in w).backward()
    return pred.grad.numpy()


def d_pred_reference(case, top_idx, w):
    ref = model_d_pred(case, top_idx, w)
    return ref, bar_of(DM.rel_err(model_d_pred(case, top_idx, w, torch.float32), ref))


def refine_inputs(rows=None, nan=True):
    """refine_cases() restricted to `rows` (names); nan=False: the NaN of row `nan` replaced by a plain number."""
    c = refine_cases()
    sel = list(range(len(REFINE_ROWS))) if rows is None else [REFINE_ROWS.index(r) for r in rows]
    out = {k: v[sel].copy() for k, v in c.items()}
    if not nan and "nan" in (rows or REFINE_ROWS):
        out["delta"][[REFINE_ROWS[i] for i in sel].index("nan"), NAN_AT, 0] = 0.0625
    return out


def refine_model(c, dtype=torch.float64):
    return DM.refine(_t(c["s_samples"], dtype), _t(c["coef"], dtype), _t(c["delta"], dtype)).numpy()


def refine_grads(c, w, dtype=torch.float64):
    """(d_s_samples, d_coef, d_delta) of sum(w * refine) by CPU autograd of the model in `dtype`."""
    leaves = [_t(c[k], dtype).requires_grad_(True) for k in ("s_samples", "coef", "delta")]
    (DM.refine(*leaves) * _t(w, dtype)).sum().backward()
    return [x.grad.numpy() for x in leaves]
