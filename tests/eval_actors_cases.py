"""Generated inputs of the per-actor evaluation tests (numpy only; the GPU test and the host test read the same cases),
and the bars both hold records to.

A case is a batch at one (M, T, horizon) and one scene layout:
  "mixed"   scenes of 0, 1, 5, 0, 0, 9, 3, 0 actors: a first, a last and two consecutive middle scenes without actors, a
            one-actor scene, and scenes of 5 (rows 1..5) and 9 (rows 6..14) that straddle the 4-row workgroups
  "single"  a batch of one scene of 9 actors
Every actor is an eval_cases._agent (world-scale coordinates, a ladder of final displacements, the two separation
conditions) whose displacement ladder is built at ITS last observed step.  The `has` rows cycle through the patterns
below, so every case holds each of them by construction (make_case asserts it):
  full    every step < horizon            none    no step at all             first   step 0 alone
  last    step horizon - 1 alone          hole    all but one middle step    cut     a prefix: t_last < horizon - 1
  beyond  steps >= horizon alone (flag 0; needs T > horizon)                  random  a random non-empty subset
A horizon of 1 leaves no room for a hole or a cut, a horizon of 2 none for a hole: those rows fall back to `random`, and
the assertion asks only for what the shape admits.  gt at a step that is not observed is arbitrary, as datasets leave it:
NaN on the odd rows, a far-away finite point on the even ones; `has` beyond the horizon is random."""
import numpy as np

import eval_cases as EC

SHAPES = ((1, 1, 1), (6, 30, 30), (6, 30, 10), (8, 64, 64), (3, 64, 1))      # (M, T, horizon)
LAYOUTS = {"mixed": (0, 1, 5, 0, 0, 9, 3, 0), "single": (9,)}
PATTERNS = ("full", "none", "first", "last", "hole", "cut", "beyond", "random")
CASES = [s + (l,) for s in SHAPES for l in LAYOUTS]
EPS = 2.0 ** -24
MISS_THR = EC.MISS_THR


def case_id(c):
    return "M%d-T%d-H%d-%s" % c


def _has(rng, pattern, T, H):
    """-> (has [T] bool, the pattern that was built)."""
    if (pattern == "hole" and H < 3) or (pattern == "cut" and H < 2) or (pattern == "beyond" and T == H):
        pattern = "random"
    h = np.zeros(T, bool)
    h[H:] = rng.random(T - H) < 0.5
    if pattern == "full":
        h[:H] = True
    elif pattern == "none":
        h[:] = False
    elif pattern == "first":
        h[0] = True
    elif pattern == "last":
        h[H - 1] = True
    elif pattern == "hole":
        h[:H] = True
        h[rng.integers(1, H - 1)] = False
    elif pattern == "cut":
        h[:rng.integers(1, H)] = True
    elif pattern == "beyond":
        h[:] = False
        h[rng.integers(H, T)] = True
    else:
        h[:H] = rng.random(H) < 0.6
        h[rng.integers(0, H)] = True
    return h, pattern


def make_case(M, T, H, layout, seed=0):
    """-> dict(reg [A, M, T, 2], cls [A, M], gt [A, T, 2] fp32, has [A, T] bool, actor_off [B + 1] int32, M, T, horizon,
    pattern [A] (names), sizes)."""
    sizes = LAYOUTS[layout]
    rng = np.random.default_rng([seed, M, T, H, len(sizes)])
    reg, cls, gt, has, names = [], [], [], [], []
    row = 0
    for b, n in enumerate(sizes):
        for i in range(n):
            want = "full" if (layout == "mixed" and b == 6 and i == 0) else PATTERNS[row % len(PATTERNS)]
            h, name = _has(rng, want, T, H)
            obs = np.nonzero(h[:H])[0]
            t_last = int(obs[-1]) if obs.size else H - 1
            r, c, g = EC._agent(rng, M, T, t_last + 1, 0.0 if row % 2 == 0 else 40.0)
            hidden = ~h
            g[hidden] = np.nan if row % 2 else (g[hidden] + np.float32(7.5e3))
            reg.append(r), cls.append(c), gt.append(g), has.append(h), names.append(name)
            row += 1
    c = dict(reg=np.stack(reg), cls=np.stack(cls), gt=np.stack(gt), has=np.stack(has),
             actor_off=np.concatenate([[0], np.cumsum(sizes)]).astype(np.int32), M=M, T=T, horizon=H, pattern=names, sizes=sizes)
    _assert_holds_every_pattern(c)
    return c


def _assert_holds_every_pattern(c):
    H, T = c["horizon"], c["T"]
    h = c["has"][:, :H]
    n_obs = h.sum(1)
    t_last = np.where(n_obs > 0, H - 1 - np.argmax(h[:, ::-1], 1), -1)
    assert (n_obs == H).any(), "a fully observed actor"
    assert (n_obs == 0).any(), "an actor without an observed step"
    assert ((n_obs == 1) & h[:, 0]).any() and ((n_obs == 1) & h[:, H - 1]).any(), "one step, at 0 and at horizon - 1"
    if H >= 3:
        assert ((n_obs < t_last + 1) & (n_obs > 1)).any(), "a hole in the middle"
    if H >= 2:
        assert ((t_last >= 0) & (t_last < H - 1)).any(), "a future cut short"
    if T > H:
        assert ((n_obs == 0) & c["has"][:, H:].any(1)).any(), "observed only beyond the horizon"
    assert np.isnan(c["gt"][:, :H][~h]).any() or H == 1, "NaN at an unobserved step"
    first = c["actor_off"][:-1][np.diff(c["actor_off"]) > 0]
    assert (n_obs[first] == H).any(), "a fully observed first actor"
    if len(c["sizes"]) > 1:
        s = list(c["sizes"])
        assert s[0] == 0 and s[-1] == 0 and any(s[i] == 0 and s[i + 1] == 0 for i in range(1, len(s) - 2))
        assert 1 in s and 5 in s and 9 in s
        off = c["actor_off"]
        assert any(off[b] // 4 != (off[b + 1] - 1) // 4 for b in range(len(s)) if s[b] in (5, 9)), "a scene across workgroups"


def outside_bars(got, want, M, H, p_bar):
    """What of `got` [n, 32] misses the bars of the GPU test against the model's records `want`: a list of names, empty when
    all is inside.  Flags and the floats [1..3], [28], [29] exact, everything behind 4 + 3 M but those zero, a record of flag
    0 / 2 zero but for [0] and [3]; minFDE within 8 * 2^-24 relative, minADE within (horizon + 8) * 2^-24, p_k within p_bar
    (tests/test_gpu_eval.py derives them; n_obs <= horizon, so they hold unchanged)."""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    miss = []
    if not np.array_equal(got[:, 0], want[:, 0]):
        return ["flags"]
    if not np.array_equal(got[:, 3], want[:, 3]):
        miss.append("local index")
    ok = want[:, 0] == 1.0
    if got[~ok][:, [1, 2]].any() or got[~ok, 4:].any():
        miss.append("a record of flag 0 / 2 is not zero")
    if not (np.array_equal(got[ok, 1:3], want[ok, 1:3]) and np.array_equal(got[ok, 28:30], want[ok, 28:30])):
        miss.append("M / horizon / missing / cut")
    if got[ok, 4 + 3 * M:28].any() or got[ok, 30:].any():
        miss.append("not zero behind the metrics")
    g, w = got[ok, 4:4 + 3 * M].reshape(-1, M, 3), want[ok, 4:4 + 3 * M].reshape(-1, M, 3)
    for i, (name, bar) in enumerate((("minFDE", 8 * EPS), ("minADE", (H + 8) * EPS), ("p", p_bar))):
        if not np.all(np.abs(g[..., i] - w[..., i]) <= bar * w[..., i]):          # a NaN misses too
            miss.append(name)
    return miss


def worst(got, want, M):
    """Largest relative errors (minFDE, minADE, p) over the evaluated records, for the tests' printed figures."""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    ok = want[:, 0] == 1.0
    if not ok.any():
        return np.zeros(3)
    g, w = got[ok, 4:4 + 3 * M].reshape(-1, 3), want[ok, 4:4 + 3 * M].reshape(-1, 3)
    with np.errstate(invalid="ignore", divide="ignore"):
        return np.nanmax(np.abs(g - w) / w, 0)


def make_records(n, M, H, seed=0):
    """A record table [n, 32] fp32 of mixed flags for the selected reduce: eval_cases.make_records plus a local index in [3]
    (0 for about a third of the rows, every flag) and, on the evaluated rows, missing steps in [28] (0 for about half,
    else 1 .. horizon - 1) with a cut [29] <= [28]."""
    rec = EC.make_records(n, M, H, seed=seed)
    rng = np.random.default_rng([seed, n, M, H, 7])
    local = rng.integers(0, 60, n) * (rng.random(n) < 0.67)
    rec[:, 3] = local
    ok = rec[:, 0] == 1.0
    missing = rng.integers(1, max(H, 2), n) * (rng.random(n) < 0.5) if H > 1 else np.zeros(n, np.int64)
    rec[ok, 28] = missing[ok]
    rec[ok, 29] = (missing * (rng.random(n) < 0.5))[ok]
    return rec
