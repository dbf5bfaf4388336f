"""Cases that put the users of csrc/lgcn_blockscan.hpp on their workgroup seams: the pair search's row chunks and scene
trips, the CSR plan's scan tiles, and the 256-thread block scans of the batched graph ops and of scene construction.  Every
size below is derived from a constant of the kernels; tests/test_seam_cases_host.py pins those constants to the library
and proves on the host that the cases hold what they claim.  The GPU tests (tests/test_gpu_block_seams.py,
tests/test_gpu_scene_seams.py) compare against host models only: oracle/lanegcn_oracle.py, oracle/graphgen_oracle.py,
tests/scene_build_model.py and the numpy restatements in this file, none of which calls the library.

The vectorised restatements here (csr_expected, obj_feats_batch, lane_graph_one) exist because the per-item Python loops
of the models they restate take seconds at 65 536 items; the host test holds them to those models element for element."""
import numpy as np

from scene_build_cases import Pose

BLOCK = 256               # kScThreads: sc_scan_local / sc_block_base / block_base<256>
PAIR_CHUNK = 4096         # pairs_scan_bases_body: 1024 threads x 4 rows per trip
PAIR_SCENES = 1024        # pairs_scan_bases_body: scenes per trip
IDX_TILE = 4096           # k_index_scan: keys per workgroup
IDX_MAX_TILES = 1024      # k_index_scan: block_base<1024> takes one trip
PAIR_TH = 5.0             # 3-4-5 triangles on the integer grid fall exactly on it
CTX_SIZES = (0, 1, 63, 64, 65, 128, 129)       # around the 64-lane ballot loop

PRED_RANGE = [-100.0, 100.0, -100.0, 100.0]
SCENE_CONFIG = {"pred_range": PRED_RANGE, "num_scales": 1, "cross_dist": 6.0}
OBS, FUT = 20, 30


def csum(sizes):
    return np.concatenate([[0], np.cumsum(np.asarray(sizes, np.int64), dtype=np.int64)])


# ------------------------------------------------------------------ 1. pair search
PAIR_ROWS = {4095: ([1000, 0, 2000, 1095], [65, 3, 129, 64]),
             4096: ([1000, 0, 2000, 1096], [65, 3, 129, 64]),                      # ends on the chunk edge: rp[T] alone
             4097: ([1000, 0, 2000, 1096, 1], [65, 3, 129, 64, 128]),               # a scene boundary at row 4096
             8193: ([1000, 0, 2000, 1096, 4000, 97], [65, 3, 129, 64, 128, 1])}
PAIR_SCENE_COUNTS = (1023, 1024, 1025, 2049)


def _grid(rng, n):
    return rng.integers(-8, 9, (n, 2)).astype(np.float32)


def pair_case_rows(T):
    """T target rows in a handful of scenes (the second one has context rows and no target row)."""
    rows, ctx = PAIR_ROWS[T]
    rng = np.random.default_rng(T)
    return {"name": "T%d" % T, "agt": [_grid(rng, n) for n in rows], "ctx": [_grid(rng, n) for n in ctx]}


def pair_scene_kinds(B):
    """position -> kind of the scenes that hold no pair: first, last, two in a row (0 and 1, 500 and 501), 1023, 1024."""
    kinds = {0: "no_pair", 1: "no_target", 500: "no_ctx", 501: "no_pair", 777: "no_target"}
    if B > 1025:
        kinds.update({1023: "no_pair", 1024: "no_target", 2047: "no_ctx"})
    elif B > 1024:
        kinds.update({1023: "no_target"})
    kinds[B - 1] = "no_pair"
    return kinds


def pair_case_scenes(B):
    """B scenes of 3 .. 6 target rows; context sizes walk CTX_SIZES (every seventh scene has none)."""
    rng = np.random.default_rng(B)
    kinds = pair_scene_kinds(B)
    agt, ctx = [], []
    for i in range(B):
        na, nc, shift = int(rng.integers(3, 7)), CTX_SIZES[i % len(CTX_SIZES)], 0.0
        kind = kinds.get(i)
        if kind == "no_target":
            na, nc = 0, max(nc, 1)
        elif kind == "no_ctx":
            nc = 0
        elif kind == "no_pair":
            nc, shift = 65, 500.0
        agt.append(_grid(rng, na))
        ctx.append(_grid(rng, nc) + np.float32(shift))
    return {"name": "B%d" % B, "agt": agt, "ctx": ctx}


def pair_flat(case):
    """(agt [T,2], agt_off [B+1], ctx [S,2], ctx_off [B+1], capacity) as the library takes them."""
    agt = np.concatenate(case["agt"]).astype(np.float32).reshape(-1, 2)
    ctx = np.concatenate(case["ctx"]).astype(np.float32).reshape(-1, 2)
    na, nc = [len(a) for a in case["agt"]], [len(c) for c in case["ctx"]]
    return agt, csum(na).astype(np.int32), ctx, csum(nc).astype(np.int32), int(np.dot(na, nc))


def pair_counts(case, th=PAIR_TH):
    """Pairs per scene, by the oracle's arithmetic."""
    out = []
    for a, c in zip(case["agt"], case["ctx"]):
        d = a.reshape(-1, 1, 2) - c.reshape(1, -1, 2)
        sq = d * d
        out.append(int((np.sqrt(sq[..., 0] + sq[..., 1]) <= np.float32(th)).sum()))
    return np.asarray(out, np.int64)


def pair_expected(case, legacy, th=PAIR_TH):
    """(hi, wi int64, rowptr int32 [T + 1]) from oracle.lanegcn_oracle.pair_search."""
    import torch
    from oracle import lanegcn_oracle as O
    hi, wi = O.pair_search([torch.from_numpy(a) for a in case["agt"]], [torch.from_numpy(c) for c in case["ctx"]], th, legacy)
    T = sum(len(a) for a in case["agt"])
    return hi, wi, np.searchsorted(hi, np.arange(T + 1), side="left").astype(np.int32)


# ------------------------------------------------------------------ 2. CSR plan
def csr_keys1(n_nodes, n_rel):
    return (n_nodes + 15) // 16 * 16 * n_rel + 1


def csr_key(u, r, n_rel):
    return ((u >> 4) * n_rel + r) * 16 + (u & 15)


def csr_node_of_key(k, n_rel):
    """(node, relation) of key k."""
    sub, j = k // 16, k % 16
    return (sub // n_rel) * 16 + j, sub % n_rel


CSR_SMALL = ((4080, 1), (4096, 1), (8192, 1), (4096, 3))
CSR_MAX_NODES = IDX_TILE * IDX_MAX_TILES - 16        # 4 194 288: n_keys1 = 4 194 289, the 1024th tile
CSR_MAX_PLANT_TILES = (0, 255, 256, 257, 1023)


def csr_case(n_nodes, n_rel, n_random=None, plant_tiles=None):
    """Per relation (u, v) int64: random edges, duplicates, endpoints outside [0, n_nodes) and edges planted on the first
    and the last key of scan tiles (every tile, or plant_tiles)."""
    rng = np.random.default_rng(n_nodes * 8 + n_rel)
    nk = csr_keys1(n_nodes, n_rel) - 1
    n_tiles = (nk + 1 + IDX_TILE - 1) // IDX_TILE
    tiles = range(n_tiles) if plant_tiles is None else plant_tiles
    plant = [[] for _ in range(n_rel)]
    for t in tiles:
        for k in (t * IDX_TILE, t * IDX_TILE + 1, min((t + 1) * IDX_TILE, nk) - 1):
            if k < nk:
                u, r = csr_node_of_key(k, n_rel)
                if u < n_nodes:
                    plant[r] += [u, u, u]              # three edges per planted key
    us, vs = [], []
    for r in range(n_rel):
        m = (3 * n_nodes if n_random is None else n_random) // n_rel
        u, v = rng.integers(0, n_nodes, m), rng.integers(0, n_nodes, m)
        dup = rng.integers(0, m, m // 10)
        pu = np.asarray(plant[r], np.int64)
        bad_u = np.array([-1, n_nodes, n_nodes + 5, 3, 7, 2 ** 40, -2 ** 40, 0], np.int64)
        bad_v = np.array([5, 9, 2, -1, n_nodes, 1, 1, 2 ** 31], np.int64)
        u = np.concatenate([u, u[dup], pu, bad_u])
        v = np.concatenate([v, v[dup], rng.integers(0, n_nodes, len(pu)), bad_v])
        p = rng.permutation(len(u))
        us.append(u[p].astype(np.int64))
        vs.append(v[p].astype(np.int64))
    return us, vs


def csr_expected(us, vs, n_nodes, n_rel):
    """(rowptr int32 [n_keys + 1], col int32 [kept edges]): the exclusive cumsum of a bincount over the key, and the
    sources ordered by (key, v)."""
    nk = csr_keys1(n_nodes, n_rel) - 1
    keys, cols = [], []
    for r, (u, v) in enumerate(zip(us, vs)):
        ok = (u >= 0) & (u < n_nodes) & (v >= 0) & (v < n_nodes)
        keys.append(csr_key(u[ok], r, n_rel))
        cols.append(v[ok])
    key, col = np.concatenate(keys), np.concatenate(cols)
    rowptr = csum(np.bincount(key, minlength=nk))
    assert rowptr[-1] < 2 ** 31
    return rowptr.astype(np.int32), col[np.lexsort((col, key))].astype(np.int32)


def expand_plan_loop(rowptr, col, n_nodes, n_rel):
    """The plan as a sorted list of (relation, u, v), by the plain loop of tests/test_gpu_parity.py::expand_plan."""
    out = []
    for t in range((n_nodes + 15) // 16):
        for r in range(n_rel):
            for j in range(16):
                k = (t * n_rel + r) * 16 + j
                out += [(r, t * 16 + j, int(col[e])) for e in range(rowptr[k], rowptr[k + 1])]
    return sorted(out)


# ------------------------------------------------------------------ 3. / 4. the batched graph ops
GRAPH_NODES = (127, 128, 32767, 32768, 32769 + 256)       # items = 2 N + 1
DILATE_SCALES = 3


def scene_sizes(N, rng):
    """Node counts of a batch of N nodes: scenes of 20 .. 72 nodes, one boundary on node 256 (N permitting) with an empty
    scene sitting on it, empty scenes first, last and twice in a row."""
    sizes, left = [], N
    while left > 0:
        n = min(left, int(rng.integers(20, 73)))
        cum = N - left
        if cum < BLOCK < cum + n and N > 2 * BLOCK:
            n = BLOCK - cum
        sizes.append(n)
        left -= n
    out = [0]
    for i, n in enumerate(sizes):
        out.append(n)
        if sum(out) == BLOCK and N > 2 * BLOCK:
            out.append(0)                                 # equal neighbours on a block edge
        if i == len(sizes) // 2:
            out += [0, 0]
    return out + [0]


def _lanes_of(n, rng):
    """n nodes cut into lanes of 8 .. 12 (the last one takes what is left)."""
    cuts, at = [0], 0
    while at < n:
        at = min(n, at + int(rng.integers(8, 13)))
        cuts.append(at)
    return np.asarray(cuts, np.int64)


def dilate_batch(N):
    """Scenes {"n", "u", "v"} (the `pre` relation; `suc` is its transpose) as tests/graph_batch_cases.py shapes them: chains,
    links between lanes, duplicates, and edges that leave [0, n)."""
    rng = np.random.default_rng(N)
    scenes = []
    for n in scene_sizes(N, rng):
        if n == 0:
            scenes.append({"n": 0, "u": np.zeros(0, np.int64), "v": np.zeros(0, np.int64)})
            continue
        cuts = _lanes_of(n, rng)
        nl = len(cuts) - 1
        i = np.arange(n)
        chain = i[~np.isin(i, cuts[:-1])]                 # every node but a lane's first has its predecessor
        u, v = [chain], [chain - 1]
        k = int(rng.integers(0, 2 * nl + 1))
        a, b = rng.integers(0, nl, k), rng.integers(0, nl, k)
        u.append(cuts[a]); v.append(cuts[b + 1] - 1)      # first node of lane a <- last node of lane b
        if len(chain):
            d = rng.integers(0, len(chain), 3)
            u.append(chain[d]); v.append(chain[d] - 1)    # duplicates
        u.append(np.array([0, n, -1, n - 1], np.int64)); v.append(np.array([n, 0, 0, n + 7], np.int64))
        u, v = np.concatenate(u).astype(np.int64), np.concatenate(v).astype(np.int64)
        p = rng.permutation(len(u))
        scenes.append({"n": int(n), "u": u[p], "v": v[p]})
    return scenes


def inside(c):
    ok = (c["u"] >= 0) & (c["u"] < c["n"]) & (c["v"] >= 0) & (c["v"] < c["n"])
    return {"u": c["u"][ok], "v": c["v"][ok]}


def transposed(c):
    return dict(c, u=c["v"], v=c["u"])


def dilate_expected(scenes, num_scales=DILATE_SCALES):
    """Per scale {"u", "v", "off"}: oracle.lanegcn_oracle.dilated_nbrs per scene on the in-range edges, (u, v)-sorted,
    back to back."""
    from oracle import lanegcn_oracle as O
    per = []
    for c in scenes:
        if c["n"] == 0:
            per.append([{"u": np.zeros(0, np.int64), "v": np.zeros(0, np.int64)}] * (num_scales - 1))
            continue
        out = O.dilated_nbrs(inside(c), c["n"], num_scales)
        srt = []
        for e in out:
            o = np.lexsort((e["v"], e["u"]))
            srt.append({"u": e["u"][o].astype(np.int64), "v": e["v"][o].astype(np.int64)})
        per.append(srt)
    res = []
    for j in range(num_scales - 1):
        res.append({"u": np.concatenate([p[j]["u"] for p in per]), "v": np.concatenate([p[j]["v"] for p in per]),
                    "off": csum([len(p[j]["u"]) for p in per])})
    return res


def cross_batch(N):
    """Scenes of straight parallel lanes 3.5 m apart (8 m in every fifth scene with nodes: nothing within cross_dist), one
    heading per scene, left / right lane pairs between neighbours; every third such scene (from the second) has an empty left list,
    every fourth (from the third) an empty right list.  Keys as graphgen_oracle.preprocess reads them."""
    rng = np.random.default_rng(N + 1)
    scenes, k = [], 0
    for n in scene_sizes(N, rng):
        if n == 0:
            scenes.append({"n": 0})
            continue
        k += 1
        cuts = _lanes_of(n, rng)
        nl = len(cuts) - 1
        lane = np.repeat(np.arange(nl), np.diff(cuts))
        along = np.arange(n) - cuts[lane] + rng.uniform(0.0, 0.4, nl)[lane]
        gap = 8.0 if k % 5 == 0 else 3.5
        phi = rng.uniform(0, 2 * np.pi)
        d, nrm = np.array([np.cos(phi), np.sin(phi)]), np.array([-np.sin(phi), np.cos(phi)])
        ctrs = rng.uniform(-50, 50, 2)[None, :] + along[:, None] * d[None, :] + (gap * lane)[:, None] * nrm[None, :]
        feats = np.repeat(d[None, :].astype(np.float32), n, 0)           # one vector, bit for bit, for the whole scene
        nb = np.stack([np.arange(nl - 1), np.arange(1, nl)], 1).reshape(-1, 2).astype(np.int64)
        none = np.zeros((0, 2), np.int64)
        m = int(rng.integers(0, 4))
        scenes.append({"n": int(n), "ctrs": ctrs.astype(np.float32), "feats": feats, "lane_idcs": lane.astype(np.int64),
                       "pre_pairs": rng.integers(0, nl, (m, 2)).astype(np.int64),
                       "suc_pairs": rng.integers(0, nl, (m, 2)).astype(np.int64),
                       "left_pairs": none if k % 3 == 2 else nb, "right_pairs": none if k % 4 == 3 else nb[:, ::-1].copy(),
                       "far": gap > 6.0})
    return scenes


CROSS_LISTS = ("pre_pairs", "suc_pairs", "left_pairs", "right_pairs")


def cross_flat(scenes):
    """(arrays, offset tables) as ops.cross_edges_batch takes them."""
    real = [s for s in scenes if s["n"]]
    arr = {k: np.concatenate([s[k] for s in real]) for k in ("ctrs", "feats", "lane_idcs") + CROSS_LISTS}
    off = {"node": csum([s["n"] for s in scenes]), "lane": csum([int(s["lane_idcs"][-1]) + 1 if s["n"] else 0 for s in scenes])}
    for k in CROSS_LISTS:
        off[k] = csum([len(s[k]) if s["n"] else 0 for s in scenes])
    return arr, off


def cross_expected(scenes, cross_dist=6.0):
    """{"left_u", ..} int16 back to back and {"left_off", "right_off"}: graphgen_oracle.preprocess per scene."""
    from oracle import graphgen_oracle as GO
    per = [GO.preprocess(s, cross_dist) if s["n"] else None for s in scenes]
    z = np.zeros(0, np.int16)
    out = {}
    for side in ("left", "right"):
        for c in "uv":
            out["%s_%s" % (side, c)] = np.concatenate([p[side][c] if p else z for p in per]).astype(np.int16)
        out[side + "_off"] = csum([len(p[side]["u"]) if p else 0 for p in per])
    return out


# ------------------------------------------------------------------ 5. scene tracks
TRACK_COUNTS = (255, 256, 65535, 65536, 65536 + 257)      # items = T + 1
# non-agent tracks: (steps, step 19 inside pred_range)
TRACK_KINDS = (([19], True), ([18, 19], True), ([19, 20, 21], True), ([17, 18], False), ([19], False), ([16, 18, 19], True),
               ([17, 19], True), ([18, 19, 24], False), ([20, 21], False), ([19, 49], True), ([0, 19], True))


CENTRE = (2570.25, 1180.5)


def poses(S, seed):
    rng = np.random.default_rng(seed)
    return [Pose(CENTRE[0] + rng.uniform(-20, 20), CENTRE[1] + rng.uniform(-20, 20), rng.uniform(-np.pi, np.pi)) for _ in range(S)]


def small_table():
    """Three lanes around CENTRE: every scene of a track case keeps them."""
    from lanegcn_amd.data_raw import LaneTable
    pts = np.array([[0, 0], [5, 0], [10, 0], [0, 3.5], [6, 3.5], [0, -3.5], [7, -3.5], [14, -3.5]], np.float64) + np.asarray(CENTRE)
    return LaneTable([7, 8, 9], [0, 3, 5, 8], pts, [0, 1, 2], [0, 1, 0], [1, 0, 0], [0, 0, 1, 1], [0], [0, 1, 1, 1], [1], [1, -1, 0],
                     [2, 0, -1])


def track_scene_sizes(T):
    """Tracks per scene, the agent included: 8 scenes; the first ends on track 256 (T permitting)."""
    rng = np.random.default_rng(T)
    if T <= BLOCK:
        w = rng.integers(10, 40, 8)
        sizes = np.maximum(1, w * T // w.sum())
        sizes[-1] += T - sizes.sum()
        return sizes.astype(np.int64)
    w = rng.integers(10, 40, 7)
    rest = T - BLOCK
    sizes = np.maximum(1, w * rest // w.sum())
    sizes[-1] += rest - sizes.sum()
    return np.concatenate([[BLOCK], sizes]).astype(np.int64)


def track_batch(T):
    """Raw scenes for lanegcn_amd.data_raw.build_scenes with T tracks in all: the agent's 50 steps, then tracks of
    TRACK_KINDS drawn at random (no period), inside ones within 80 m, outside ones 130 .. 170 m ahead."""
    rng = np.random.default_rng(T + 7)
    sizes = track_scene_sizes(T)
    raws = []
    for pose, n in zip(poses(len(sizes), T), sizes):
        kind = rng.integers(0, len(TRACK_KINDS), n - 1)
        steps = [np.asarray(TRACK_KINDS[k][0], np.int64) for k in kind]
        inside_ = np.asarray([TRACK_KINDS[k][1] for k in kind], bool)
        start = rng.uniform(-80, 80, (n - 1, 2))
        start[~inside_, 0] = rng.uniform(130, 170, int((~inside_).sum()))
        vel = rng.uniform(-1.0, 1.0, (n - 1, 2))
        trajs = [pose.to_world(s[None, :] + (st - 19)[:, None] * v[None, :]) for s, v, st in zip(start, vel, steps)]
        a_xy, a_st = pose.agent()
        raws.append({"city": "A", "trajs": [a_xy] + trajs, "steps": [a_st] + steps})
    return raws


def frames(raws):
    """(orig [S,2] fp32, rot [S,2,2] fp32) as tests/scene_build_model.frame gives them."""
    import scene_build_model as M
    fr = [M.frame(r) for r in raws]
    return np.stack([f[0] for f in fr]), np.stack([f[2] for f in fr])


def xform_rows(pts, orig, rot):
    """scene_build_model.xform with one frame per row: float64, every product and sum rounded on its own."""
    o, r = orig.astype(np.float64), rot.astype(np.float64)
    dx, dy = pts[:, 0] - o[:, 0], pts[:, 1] - o[:, 1]
    return np.stack([r[:, 0, 0] * dx + r[:, 0, 1] * dy, r[:, 1, 0] * dx + r[:, 1, 1] * dy], 1)


def obj_feats_batch(raws, pred_range=PRED_RANGE):
    """scene_build_model.obj_feats for every scene at once (no step is listed twice in these cases):
    ({feats, obs_trajs, ctrs, gt_preds, has_preds} of the kept tracks back to back, kept tracks per scene)."""
    orig, rot = frames(raws)
    n_trk = np.asarray([len(r["steps"]) for r in raws])
    T = int(n_trk.sum())
    n_row = np.asarray([len(s) for r in raws for s in r["steps"]])
    st = np.concatenate([s for r in raws for s in r["steps"]]).astype(np.int64)
    xy = np.concatenate([t for r in raws for t in r["trajs"]]).astype(np.float64)
    trk = np.repeat(np.arange(T), n_row)
    scene = np.repeat(np.arange(len(raws)), n_trk)[trk]
    flat = trk * (OBS + FUT) + np.minimum(st, OBS + FUT - 1)
    low = st < OBS + FUT
    assert len(np.unique(flat[low])) == int(low.sum()), "a step is listed twice"
    pos = xform_rows(xy, orig[scene], rot[scene]).astype(np.float32)
    present = np.zeros((T, OBS), bool)
    o = st < OBS
    present[trk[o], st[o]] = True
    gaps = ~present
    first = np.where(gaps.any(1), OBS - np.argmax(gaps[:, ::-1], 1), 0)         # one past the last gap
    obs = np.zeros((T, OBS, 3), np.float32)
    sel = o & (st >= first[trk])
    obs[trk[sel], st[sel], :2] = pos[sel]
    obs[trk[sel], st[sel], 2] = 1.0
    lo_x, hi_x, lo_y, hi_y = (np.float32(v) for v in pred_range)
    x, y = obs[:, OBS - 1, 0], obs[:, OBS - 1, 1]
    keep = present[:, OBS - 1] & ~((x < lo_x) | (x > hi_x) | (y < lo_y) | (y > hi_y))
    k = np.arange(OBS)[None, :]
    f = np.zeros((T, OBS, 3), np.float32)
    diff = obs[:, 1:, :2] - obs[:, :-1, :2]
    f[:, 1:, :2] = np.where((k[:, 1:] > first[:, None])[..., None], diff, np.float32(0))
    f[:, :, 2] = (k >= first[:, None]).astype(np.float32)
    gt, has = np.zeros((T, FUT, 2), np.float32), np.zeros((T, FUT), bool)
    fut = (st >= OBS) & (st < OBS + FUT)
    gt[trk[fut], st[fut] - OBS] = xy[fut].astype(np.float32)
    has[trk[fut], st[fut] - OBS] = True
    counts = np.add.reduceat(keep.astype(np.int64), csum(n_trk)[:-1])
    return dict(feats=f[keep], obs_trajs=obs[keep], ctrs=obs[keep][:, OBS - 1, :2].copy(), gt_preds=gt[keep], has_preds=has[keep]), counts


# ------------------------------------------------------------------ 6. scene lanes
LANE_COUNTS = (255, 256, 65535, 65536, 65536 + 257)       # items = n_cand + 1
TABLE_NX, TABLE_NY = 128, 64                              # 8 192 lanes


def lane_table():
    """8 192 lanes of 2 .. 4 points on a 280 m x 280 m grid around CENTRE (pred_range covers 200 m x 200 m of it: about half
    survive), with random predecessors, successors (0 .. 2 each, some of them ids that are not in the table) and left / right
    neighbours anywhere in the table, so many of them point at lanes that do not survive."""
    from lanegcn_amd.data_raw import LaneTable
    rng = np.random.default_rng(64)
    L = TABLE_NX * TABLE_NY
    i, j = np.arange(L) % TABLE_NX, np.arange(L) // TABLE_NX
    x0 = CENTRE[0] + (i - TABLE_NX / 2) * (280.0 / TABLE_NX) + rng.uniform(0, 0.3, L)
    y0 = CENTRE[1] + (j - TABLE_NY / 2) * (280.0 / TABLE_NY) + rng.uniform(0, 0.3, L)
    npts = rng.integers(2, 5, L)
    pt_off = csum(npts)
    lane_of = np.repeat(np.arange(L), npts)
    k = np.arange(pt_off[-1]) - pt_off[lane_of]
    pts = np.stack([x0[lane_of] + 0.6 * k, y0[lane_of] + 0.05 * k * k], 1)
    nbr = lambda n: np.where(rng.random(n) < 0.1, -1, rng.integers(0, L, n))
    n_pred, n_succ = rng.integers(0, 3, L), rng.integers(0, 3, L)
    side = lambda: np.where(rng.random(L) < 0.4, -1, rng.integers(0, L, L))
    return LaneTable(np.arange(L) + 1000, pt_off, pts, rng.integers(0, 3, L), rng.random(L) < 0.3, rng.random(L) < 0.3,
                     csum(n_pred), nbr(int(n_pred.sum())), csum(n_succ), nbr(int(n_succ.sum())), side(), side())


def lane_batch(n_cand, table):
    """(raw scenes with the agent alone, lane_ids per scene) whose candidate lists hold n_cand lanes in all.  8 scenes share
    the table (9 for the largest case); a scene with lane_ids None lists the whole table."""
    rng = np.random.default_rng(n_cand)
    L = table.n_lanes
    if n_cand < L:                                        # every scene lists a few lanes in an order of its own
        w = rng.integers(20, 40, 8)
        sizes = w * n_cand // w.sum()
        sizes[-1] += n_cand - sizes.sum()
        ids = [table.lane_id[rng.permutation(L)[:n]].tolist() for n in sizes]
    else:
        S, extra = n_cand // L, n_cand % L
        if extra > L // 2:                                # 65 535: one scene lists all lanes but one
            S, extra = S + 1, extra - L
        ids = [None] * S
        if extra > 0:
            ids.insert(3, table.lane_id[rng.permutation(L)[:extra]].tolist())
        elif extra < 0:
            ids[3] = table.lane_id[rng.permutation(L)[:L + extra]].tolist()
    raws = []
    for pose in poses(len(ids), n_cand + 3):
        xy, st = pose.agent()
        raws.append({"city": "A", "trajs": [xy], "steps": [st]})
    return raws, ids


def lane_cand_rows(table, lane_ids):
    return [np.arange(table.n_lanes) if ids is None else table.rows(ids).astype(np.int64) for ids in lane_ids]


def _ragged(off, rows):
    """(flat element indices, owner position in `rows`) of the runs off[r] .. off[r + 1] of `rows`, in order."""
    n = (off[rows + 1] - off[rows]).astype(np.int64)
    own = np.repeat(np.arange(len(rows)), n)
    return off[rows][own] + np.arange(int(n.sum())) - csum(n)[:-1][own], own


def lane_graph_one(orig, rot, table, pred_range, rows):
    """scene_build_model.lane_graph without its per-lane loops: the same leaves (pre / suc hold scale 0 only)."""
    import scene_build_model as M
    x_min, x_max, y_min, y_max = (float(v) for v in pred_range)
    rows = np.asarray(rows, np.int64)
    L = table.n_lanes
    pt_off = table.pt_off.astype(np.int64)
    npts = np.diff(pt_off)
    c = M.xform(table.pts, orig, rot)
    first = pt_off[:-1]
    x0, x1 = np.minimum.reduceat(c[:, 0], first), np.maximum.reduceat(c[:, 0], first)
    y0, y1 = np.minimum.reduceat(c[:, 1], first), np.maximum.reduceat(c[:, 1], first)
    inside_ = ~((x1 < x_min) | (x0 > x_max) | (y1 < y_min) | (y0 > y_max))
    kept = rows[inside_[rows]]
    assert len(kept), "no lane survives"
    K = len(kept)
    rank = np.full(L + 1, -1, np.int64)                   # slot L: the id that is not in the table (-1)
    rank[kept] = np.arange(K)
    nseg = npts[kept] - 1
    start = csum(nseg)
    n = int(start[-1])
    lane_idcs = np.repeat(np.arange(K), nseg)
    a_pt = pt_off[kept][lane_idcs] + np.arange(n) - start[:-1][lane_idcs]
    ctrs = ((c[a_pt] + c[a_pt + 1]) / 2.0).astype(np.float32)
    feats = (c[a_pt + 1] - c[a_pt]).astype(np.float32)
    turn = np.zeros((n, 2), np.float32)
    turn[:, 0] = (table.turn[kept] == 1)[lane_idcs]
    turn[:, 1] = (table.turn[kept] == 2)[lane_idcs]
    control = (table.control[kept] != 0)[lane_idcs].astype(np.float32)
    intersect = (table.intersect[kept] != 0)[lane_idcs].astype(np.float32)
    g = dict(ctrs=ctrs, num_nodes=n, feats=feats, turn=turn, control=control, intersect=intersect, lane_idcs=lane_idcs)

    def neighbours(off, nb):
        e, own = _ragged(off.astype(np.int64), kept)
        j = rank[nb[e].astype(np.int64)]
        return own[j >= 0], j[j >= 0]                     # (kept lane, kept neighbour) in list order

    pi, pj = neighbours(table.pred_off, table.pred)
    si, sj = neighbours(table.succ_off, table.succ)
    # per lane: its chain edges, then its kept neighbours; a stable sort by lane restores that order
    node = np.arange(n)
    inner = node != start[:-1][lane_idcs]                 # every node but a lane's first
    def edges(chain_u, chain_v, chain_lane, nb_u, nb_v, nb_lane):
        lane = np.concatenate([chain_lane, nb_lane])
        kind = np.concatenate([np.zeros(len(chain_lane), np.int64), np.ones(len(nb_lane), np.int64)])
        pos = np.concatenate([np.arange(len(chain_lane)), np.arange(len(nb_lane))])
        o = np.lexsort((pos, kind, lane))
        return {"u": np.concatenate([chain_u, nb_u])[o].astype(np.int64), "v": np.concatenate([chain_v, nb_v])[o].astype(np.int64)}
    g["pre"] = [edges(node[inner], node[inner] - 1, lane_idcs[inner], start[:-1][pi], start[1:][pj] - 1, pi)]
    g["suc"] = [edges(node[inner] - 1, node[inner], lane_idcs[inner], start[1:][si] - 1, start[:-1][sj], si)]
    g["pre_pairs"], g["suc_pairs"] = np.stack([pi, pj], 1).astype(np.int64), np.stack([si, sj], 1).astype(np.int64)
    for k, tab in (("left", table.left), ("right", table.right)):
        j = rank[tab[kept].astype(np.int64)]
        g[k + "_pairs"] = np.stack([np.arange(K)[j >= 0], j[j >= 0]], 1).astype(np.int64)
    g["kept_rows"] = kept
    return g
