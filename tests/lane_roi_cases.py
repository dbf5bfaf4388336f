"""Scenes for the lane-RoI tests: a builder of small lane graphs with a chosen topology (chains of lanes of 1..20
nodes, parallel chains joined by left / right edges, branches, lane cycles, clusters of one-node lanes, shuffled node
order) in the reference's scene schema with pre_pairs / suc_pairs and obs_trajs, and the six random trials of
tests/test_gpu_lane_roi.py (tests/test_lane_roi_model_host.py checks the same seeds with the model alone); the named
scenes at real sizes of tests/test_gpu_lane_roi_large.py (large_scene) with the properties they must hold; the loaders
of the two recordings of the reference and the comparison helpers."""
import numpy as np

from lanegcn_amd import data as gen

TRIAL_SEEDS = (11, 12, 13, 14, 15, 16)


class Builder:
    def __init__(self, rng):
        self.rng = rng
        self.ctrs, self.feats, self.lane = [], [], []
        self.suc_u, self.suc_v, self.left_u, self.left_v = [], [], [], []
        self.n_lanes = 0

    def _lane(self, start, heading, k, spacing):
        """k nodes from `start` along `heading` (slowly turning); returns (node ids, end point, end heading)."""
        ids, p, th = [], np.asarray(start, np.float64), heading
        for _ in range(k):
            th += self.rng.normal(0.0, 0.02)
            q = p + spacing * np.array([np.cos(th), np.sin(th)])
            ids.append(len(self.lane))
            self.ctrs.append((p + q) / 2.0)
            self.feats.append(q - p)
            self.lane.append(self.n_lanes)
            p = q
        for a, b in zip(ids[:-1], ids[1:]):
            self.suc_u.append(a)
            self.suc_v.append(b)
        self.n_lanes += 1
        return ids, p, th

    def chain(self, origin, heading, sizes, n_par=1, cycle=False, spacing=None):
        """A chain of len(sizes) lanes joined end to start; n_par parallel copies 3.5 m apart joined node by node by
        left / right edges; cycle: the last lane leads back into the first.  Returns the lanes' node ids per copy."""
        spacing = spacing or self.rng.uniform(1.0, 3.0)
        copies = []
        for c in range(n_par):
            nrm = np.array([-np.sin(heading), np.cos(heading)])
            p, th, lanes = np.asarray(origin, np.float64) + 3.5 * c * nrm, heading, []
            state = self.rng.bit_generator.state            # the copies share their curvature
            for k in sizes:
                ids, p, th = self._lane(p, th, k, spacing)
                if lanes:
                    self.suc_u.append(lanes[-1][-1])
                    self.suc_v.append(ids[0])
                lanes.append(ids)
            if cycle:
                self.suc_u.append(lanes[-1][-1])
                self.suc_v.append(lanes[0][0])
            if c + 1 < n_par:
                self.rng.bit_generator.state = state
            copies.append(lanes)
        for c in range(n_par - 1):
            for la, lb in zip(copies[c], copies[c + 1]):
                self.left_u += la
                self.left_v += lb
        return copies

    def branch(self, lane_from, lane_to):
        self.suc_u.append(lane_from[-1])
        self.suc_v.append(lane_to[0])

    def cluster(self, origin, heading, n):
        """n one-node lanes side by side, joined only by left / right edges."""
        nrm = np.array([-np.sin(heading), np.cos(heading)])
        ids = [self._lane(np.asarray(origin) + 3.5 * i * nrm, heading, 1, 2.0)[0][0] for i in range(n)]
        self.left_u += ids[:-1]
        self.left_v += ids[1:]
        return ids

    def graph(self, idx_dtype=np.int64, shuffle=False, dup_edges=False, meta_p=0.3):
        N = len(self.lane)
        perm = np.arange(N)
        if shuffle:         # non-contiguous lane_idcs; a node of the last lane stays last (num_lanes = lane_idcs[-1] + 1)
            last = max(i for i in range(N) if self.lane[i] == self.n_lanes - 1)
            rest = np.array([i for i in range(N) if i != last])
            perm = np.concatenate([self.rng.permutation(rest), [last]])
        new = np.empty(N, np.int64)
        new[perm] = np.arange(N)
        suc0 = {"u": new[np.asarray(self.suc_u, np.int64)], "v": new[np.asarray(self.suc_v, np.int64)]}
        pre0 = {"u": suc0["v"].copy(), "v": suc0["u"].copy()}
        pre = [pre0] + gen.dilated_nbrs(pre0, N, 6)
        suc = [suc0] + gen.dilated_nbrs(suc0, N, 6)
        if dup_edges and len(suc0["u"]) > 3:      # pairs listed twice count once
            for rel in (pre[1], suc[0]):
                rel["u"], rel["v"] = np.concatenate([rel["u"], rel["u"][:3]]), np.concatenate([rel["v"], rel["v"][:3]])
        lu, lv = new[np.asarray(self.left_u, np.int64)], new[np.asarray(self.left_v, np.int64)]
        lane_idcs = np.asarray(self.lane, np.int64)[perm]
        cast = lambda d: {k: np.asarray(v).astype(idx_dtype) for k, v in d.items()}
        rng = self.rng
        g = dict(num_nodes=N, ctrs=np.asarray(self.ctrs, np.float64)[perm].astype(np.float32).reshape(N, 2),
                 feats=np.asarray(self.feats, np.float64)[perm].astype(np.float32).reshape(N, 2),
                 turn=(rng.random((N, 2)) < meta_p).astype(np.float32), control=(rng.random(N) < meta_p).astype(np.float32),
                 intersect=(rng.random(N) < meta_p).astype(np.float32),
                 pre=[cast(d) for d in pre], suc=[cast(d) for d in suc],
                 left=cast({"u": lu, "v": lv}), right=cast({"u": lv, "v": lu}), lane_idcs=lane_idcs.astype(idx_dtype))
        g["pre_pairs"] = gen.lane_pairs(pre[0], lane_idcs).astype(idx_dtype)
        g["suc_pairs"] = gen.lane_pairs(suc[0], lane_idcs).astype(idx_dtype)
        return g, new


def agents(rng, graph, spec):
    """spec: list of (node id in the graph, heading offset to that node's direction, speed m/s, lateral offset m)."""
    a = len(spec)
    node = np.array([s[0] for s in spec], np.int64)
    d = graph["feats"][node].astype(np.float64)
    base = np.arctan2(d[:, 1], d[:, 0])
    th = base + np.array([s[1] for s in spec])
    speed = np.array([s[2] for s in spec], np.float64)
    lat = np.array([s[3] for s in spec], np.float64)
    steps = 0.1 * speed[:, None, None] * np.stack([np.cos(th), np.sin(th)], 1)[:, None, :] * np.ones((1, 20, 1))
    steps = steps + rng.normal(0.0, 0.01, (a, 20, 2)) * (speed > 0)[:, None, None]
    steps[:, 0] = 0.0
    nrm = np.stack([-np.sin(base), np.cos(base)], 1)
    ctrs = (graph["ctrs"][node] + lat[:, None] * nrm + rng.normal(0.0, 0.2, (a, 2))).astype(np.float32)
    after = np.cumsum(steps[:, ::-1], 1)[:, ::-1] - steps
    ones = np.ones((a, 20, 1))
    return dict(feats=np.concatenate([steps, ones], 2).astype(np.float32), ctrs=ctrs,
                obs_trajs=np.concatenate([ctrs[:, None, :].astype(np.float64) - after, ones], 2).astype(np.float32),
                gt_preds=np.repeat(ctrs[:, None, :], 30, 1), has_preds=np.ones((a, 30), bool),
                orig=np.zeros(2, np.float32), theta=0.0, rot=np.eye(2, dtype=np.float32), graph=graph)


def random_agents(rng, graph, n, p_stand=0.15, p_turned=0.15):
    spec = []
    for _ in range(n):
        off = rng.uniform(0.0, 2.0 * np.pi) if rng.random() < p_turned else rng.normal(0.0, 0.2)
        speed = 0.0 if rng.random() < p_stand else rng.uniform(0.5, 15.0)
        spec.append((int(rng.integers(0, graph["num_nodes"])), off, speed, rng.normal(0.0, 1.5)))
    return agents(rng, graph, spec)


def random_scene(rng, n_lanes, n_agents, idx_dtype=np.int64, shuffle=False, dup_edges=False, cycle=False, max_size=20):
    """About n_lanes lanes of 1..max_size nodes in chains of 1..6 lanes, single or doubled, some branches; 40..400 nodes,
    not a multiple of 64.  cycle: the first chain is a ring of short lanes (18 m at most, below every horizon) without
    neighbours, with an agent driving on it."""
    n_lanes = max(n_lanes, 8) if cycle else n_lanes
    for _ in range(1000):
        b, heads, ring = Builder(rng), [], None
        while b.n_lanes < n_lanes:
            k = int(min(rng.integers(1, 7), n_lanes - b.n_lanes))
            first_ring = cycle and not heads
            if first_ring:
                k = min(max(k, 2), 4)
            n_par = 2 if (not first_ring and k * 2 <= n_lanes - b.n_lanes and rng.random() < 0.5) else 1
            sizes = [int(x) for x in (rng.integers(3, 6, k) if first_ring else rng.integers(1, max_size + 1, k))]
            copies = b.chain(rng.uniform(-40, 40, 2), rng.uniform(0, 2 * np.pi), sizes, n_par,
                             cycle=first_ring, spacing=0.6 if first_ring else None)
            if first_ring:
                ring = copies[0]
            elif heads and rng.random() < 0.5:
                b.branch(heads[int(rng.integers(len(heads)))], copies[0][0])
            heads.append(copies[0][-1])
        if 40 <= len(b.lane) <= 400 and len(b.lane) % 64:
            break
    else:
        raise RuntimeError("no scene of 40..400 nodes with %d lanes" % n_lanes)
    g, new = b.graph(idx_dtype, shuffle, dup_edges)
    scene = random_agents(rng, g, n_agents)
    if ring is not None:      # the ring's agent replaces the first one
        one = agents(rng, g, [(int(new[ring[0][0]]), 0.05, 6.0, 0.3)])
        for k in ("feats", "ctrs", "obs_trajs", "gt_preds"):
            scene[k][0] = one[k][0]
    return scene


def standing_scene(rng, idx_dtype=np.int64):
    """No agent survives: every agent stands."""
    b = Builder(rng)
    b.chain(rng.uniform(-20, 20, 2), rng.uniform(0, 2 * np.pi), [7, 9, 5, 12], 2)
    g, _ = b.graph(idx_dtype)
    return agents(rng, g, [(int(rng.integers(0, g["num_nodes"])), 0.0, 0.0, 0.5) for _ in range(4)])


def trial(seed):
    """Three scenes of one random trial.  Over the six trials: lane sizes 1..20, node counts off the multiples of 64, a
    shuffled node order (trial 1), a scene of 70 or more lanes (trial 2), a lane cycle shorter than the horizon (trial 3),
    pairs listed twice (trial 4), a scene without a surviving agent (trial 0), a scene with one agent (trial 5), and
    index arrays as int16 / int32 / int64 in turn."""
    k = TRIAL_SEEDS.index(seed)
    rng = np.random.default_rng(seed)
    dt = (np.int16, np.int32, np.int64)
    scenes = [random_scene(rng, int(rng.integers(3, 41)), int(rng.integers(2, 9)), dt[(k + i) % 3], shuffle=(k == 1 and i == 0),
                           dup_edges=(k == 4), cycle=(k == 3 and i == 1)) for i in range(3)]
    if k == 0:
        scenes[1] = standing_scene(rng, np.int32)
    if k == 2:
        scenes[2] = random_scene(rng, 75, 6, np.int16, max_size=5)
    if k == 5:
        scenes[0] = random_scene(rng, 12, 1, np.int64)
    return scenes


# ------------------------------------------------------------------ named scenes at real sizes
# name -> seed.  tests/golden/make_golden_lane_roi_large.py searches the seeds of the recorded scenes (no agent on an
# edge, no lane listed twice, every property of assert_large_properties) and refuses to write unless they stand here.
LARGE_SEEDS = dict(wide=1, chain=2, cap=1, mixed=1, crowd=1, longlane=1, fan=1, empty_agents=1)
LARGE_RECORDED = ("wide", "chain", "cap")      # in tests/golden/lane_roi_large.npz (with mixed it passes 1,000,000 bytes)
LARGE_NAMES = LARGE_RECORDED + ("mixed", "crowd", "longlane", "fan", "empty_agents")


def large_scene(name, seed=None):
    """One named scene, each the smallest at which one path of csrc/lgcn_roi.hip can go wrong:
    wide          30 lanes of 20 nodes in 3 copies, shuffled, int16: an RoI of more than 512 nodes (three chunks of 256
                  in the edge kernels), ascending lanes (the closure grew)
    chain         700 one-node lanes, 0.5 m each, no neighbours: an RoI of more than 256 lanes in search order
    cap           4096 one-node lanes in 4 copies: lane ids on both sides of bitset word 64, an RoI of over 1024 lanes
    mixed         1800 lanes of 1..3 nodes in 2 copies, shuffled: over 256 lanes with lane offsets and node ranks
    crowd         40 lanes, 72 agents, some standing and some turned: over 40 RoIs in one scene
    longlane      a chain with one lane of 130 and one of 300 nodes (numpy sums more than 128 elements in blocks)
    fan           2,020 one-node lanes far away, then a trunk lane with 80 successor chains of 3 lanes, no neighbours: one
                  search level adds 80 lanes in bitset words 63..70, which go into the search-order list by a popcount
                  prefix over the words before them, on both sides of word 64
    empty_agents  a small graph without agents"""
    rng = np.random.default_rng(LARGE_SEEDS[name] if seed is None else seed)
    b = Builder(rng)
    at = lambda new, lane, k=0: int(new[lane[k]])
    if name == "wide":
        cp = b.chain((0.0, 0.0), 0.4, [20] * 30, 3, spacing=1.0)
        g, new = b.graph(np.int16, shuffle=True)
        return agents(rng, g, [(at(new, cp[0][14], 10), 0.05, 31.0, 0.3), (at(new, cp[1][12], 5), -0.05, 25.5, -0.4),
                               (at(new, cp[2][20], 3), 0.0, 12.5, 0.2)])
    if name == "chain":
        cp = b.chain((0.0, 0.0), 1.0, [1] * 700, 1, spacing=0.5)
        g, new = b.graph(np.int64)
        return agents(rng, g, [(at(new, cp[0][300]), 0.02, 31.0, 0.3), (at(new, cp[0][640]), -0.02, 20.5, -0.3)])
    if name == "cap":
        cp = b.chain((0.0, 0.0), 0.2, [1] * 1024, 4, spacing=0.5)
        g, new = b.graph(np.int32)
        return agents(rng, g, [(at(new, cp[2][500]), 0.02, 31.0, 0.2), (at(new, cp[0][300]), -0.02, 25.5, -0.2),
                               (at(new, cp[3][900]), 0.0, 28.3, 0.1)])
    if name == "mixed":
        cp = b.chain((0.0, 0.0), 2.0, [int(x) for x in rng.integers(1, 4, 900)], 2, spacing=0.5)
        g, new = b.graph(np.int32, shuffle=True)
        return agents(rng, g, [(at(new, cp[0][450]), 0.03, 31.0, 0.3), (at(new, cp[1][200]), -0.03, 22.0, -0.3)])
    if name == "crowd":
        return random_scene(rng, 40, 72, np.int32, max_size=14)
    if name == "longlane":
        cp = b.chain((0.0, 0.0), 0.3, [6, 130, 7, 300, 6], 1, spacing=0.3)
        g, new = b.graph(np.int64)
        return agents(rng, g, [(at(new, cp[0][1], 60), 0.02, 9.0, 0.3), (at(new, cp[0][3], 150), -0.02, 14.0, -0.3)])
    if name == "fan":
        b.chain((2000.0, 0.0), 0.0, [1] * 2020, 1, spacing=0.5)
        trunk = b.chain((0.0, 0.0), 0.5, [3], 1, spacing=2.0)[0][0]
        end = b.ctrs[trunk[-1]] + b.feats[trunk[-1]] / 2.0
        for off in np.linspace(-0.6, 0.6, 80):
            b.branch(trunk, b.chain(end, 0.5 + off, [3, 3, 3], 1, spacing=2.0)[0][0])
        g, new = b.graph(np.int32)
        return agents(rng, g, [(at(new, trunk, 1), 0.02, 7.0, 0.2)])
    if name == "empty_agents":
        b.chain((0.0, 0.0), 0.5, [5, 6, 4], 2)
        g, _ = b.graph(np.int64)
        return agents(rng, g, [])
    raise KeyError(name)


def large_scenes(names=LARGE_NAMES):
    """{name: scene} of the named scenes, deterministic (LARGE_SEEDS)."""
    return {n: large_scene(n) for n in names}


def roi_properties(scene, out):
    """Per RoI of `out` (a model or reference result for `scene`): agent, node count, lanes in RoI order (each once), the
    sizes of those lanes, ascending or not, the anchor's lane, whether the left / right closure grew."""
    import lane_roi_model as M
    sc = M.Scene(scene)
    props = []
    for a, sg in zip(out["valid_agent_ids"].tolist(), out["subgraphs"]):
        ln = sc.lane_idcs[sg["node_mask"]]
        lanes = ln[np.sort(np.unique(ln, return_index=True)[1])]
        props.append(dict(agent=a, nodes=int(sg["num_nodes"]), lanes=lanes, sizes=[len(sc.lane_nodes[l]) for l in lanes],
                          ascending=bool((np.diff(lanes) > 0).all()), anchor_lane=int(sc.lane_idcs[M.anchor(sc, a)]),
                          grew=bool(M.roi_lanes(sc, a, M.anchor(sc, a), 20.0)[1])))
    return props


def assert_large_properties(name, scene, out, excluded=()):
    """The property each named scene is there for, read off a result `out`, carried by an agent outside `excluded`."""
    import lane_roi_model as M
    g = scene["graph"]
    li = np.asarray(g["lane_idcs"], np.int64)
    lane_sizes = np.bincount(li)
    props = [p for p in roi_properties(scene, out) if p["agent"] not in set(excluded)]
    some = lambda f: any(f(p) for p in props)
    if name == "wide":
        assert g["lane_idcs"].dtype == np.int16 and (np.diff(li) < 0).any() and len(scene["ctrs"]) == 3
        assert (M.agent_velocity(scene["feats"]) > 0).all()
        assert some(lambda p: p["nodes"] > 512 and p["grew"] and p["ascending"]), props
    elif name == "chain":
        assert len(lane_sizes) >= 600 and (lane_sizes == 1).all() and len(g["left"]["u"]) == 0 == len(g["right"]["u"])

        def search_order(p):
            lanes, t = p["lanes"].tolist(), p["anchor_lane"]
            n_suc = int(np.argmax(np.diff(lanes) < 0))          # lanes[:n_suc + 1] = target and its successors
            return (len(lanes) > 256 and not p["ascending"] and n_suc >= 1 and len(lanes) - n_suc - 1 >= 1
                    and lanes == list(range(t, t + n_suc + 1)) + list(range(t - 1, t - len(lanes) + n_suc, -1)))
        assert some(search_order), props
    elif name == "cap":
        assert len(lane_sizes) == 4096 and (lane_sizes == 1).all()
        assert some(lambda p: p["anchor_lane"] >= 2048 and len(p["lanes"]) > 1024 and p["lanes"].min() < 2048
                    and p["lanes"].max() >= 2080), props
        assert some(lambda p: 4095 in p["lanes"]), props
    elif name == "mixed":
        assert 1700 <= len(lane_sizes) <= 1900 and set(lane_sizes.tolist()) == {1, 2, 3} and (np.diff(li) < 0).any()
        assert some(lambda p: len(p["lanes"]) > 256 and {1, 2, 3} <= set(p["sizes"])), props
    elif name == "crowd":
        sc = M.Scene(scene)
        assert len(scene["ctrs"]) >= 70 and 30 <= len(lane_sizes) <= 50 and 200 <= len(li) <= 400
        assert len(props) >= 40
        moving = np.flatnonzero(sc.vel > 0)
        assert len(moving) < len(sc.vel)                          # some stand
        assert any(M.angle_gap(sc, a)[np.argmin(M.node_dist(sc, a))] > 0.5 * np.pi for a in moving)      # some are turned
    elif name == "longlane":
        long_ = np.flatnonzero(lane_sizes >= 300)
        mid = np.flatnonzero((lane_sizes >= 130) & (lane_sizes < 300))
        assert len(long_) and len(mid)
        assert some(lambda p: p["anchor_lane"] in long_) and some(lambda p: p["anchor_lane"] in mid), props
    elif name == "fan":
        pairs = np.asarray(g["suc_pairs"], np.int64)

        def fans_out(p):
            nxt = pairs[pairs[:, 0] == p["anchor_lane"], 1]
            return (not p["grew"] and not p["ascending"] and {63, 64, 65} <= set((nxt >> 5).tolist())
                    and set(nxt.tolist()) <= set(p["lanes"].tolist()) and len(p["lanes"]) > 160)
        assert len(g["left"]["u"]) == 0 and some(fans_out), props
    elif name == "empty_agents":
        assert len(scene["ctrs"]) == 0 and len(li) > 0 and len(out["subgraphs"]) == 0
        assert out["valid_agent_ids"].dtype == np.int16 and out["valid_agent_ids"].shape == (0,)
    else:
        raise KeyError(name)


def zero_ring_scene(on_ring=True):
    """A ring of three one-node lanes whose feats are exactly zero (a lane search on it never adds length) beside an
    ordinary chain, with one agent anchored on the ring (on_ring) or on the chain."""
    rng = np.random.default_rng(7)
    b = Builder(rng)
    ring = b.chain((0.0, 0.0), 0.0, [1, 1, 1], 1, cycle=True, spacing=0.5)
    ch = b.chain((300.0, 0.0), 0.0, [6, 7, 5], 1, spacing=1.0)
    g, new = b.graph(np.int64)
    on = [int(new[l[0]]) for l in ring[0]]
    g["feats"][on] = 0.0
    return agents(rng, g, [(on[1] if on_ring else int(new[ch[0][1][3]]), 0.01, 6.0, 0.1)])


# ------------------------------------------------------------------ fixture and comparison
def load_large_fixture():
    """({name: scene}, {name: want}): the recorded scenes of tests/golden/lane_roi_large.npz and the reference's output,
    as load_fixture gives them."""
    return _load("lane_roi_large.npz", named=True)


def load_fixture():
    """(scenes, want): the four scenes of tests/golden/lane_roi_b4.npz and the reference's recorded output per scene,
    {"subgraphs": [...], "valid_agent_ids": int16}."""
    return _load("lane_roi_b4.npz")


def _load(file, named=False):
    import os
    from golden_io import load_scenes, unflatten
    flat = dict(np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", file)))
    scenes = load_scenes(flat)
    for s in scenes:
        s["theta"] = float(s["theta"])
    want = []
    for b in range(len(scenes)):
        subs = unflatten(flat, "want/%d/subgraphs" % b) if int(flat["want/%d/n_rois" % b]) else []
        for sg in subs:
            sg["num_nodes"], sg["agent_vel"] = int(sg["num_nodes"]), np.float32(sg["agent_vel"])
        want.append({"subgraphs": subs, "valid_agent_ids": flat["want/%d/valid_agent_ids" % b]})
    if named:
        names = [str(n) for n in flat["names"]]
        return dict(zip(names, scenes)), dict(zip(names, want))
    return scenes, want


def assert_same(got, want, path="", vel_rtol=0.0):
    """Leaf for leaf: keys, lengths, dtypes, shapes and values; agent_vel to vel_rtol (0: exact)."""
    if isinstance(want, dict):
        assert isinstance(got, dict) and set(got) == set(want), (path, sorted(got), sorted(want))
        for k in want:
            assert_same(got[k], want[k], path + "/" + str(k), vel_rtol)
    elif isinstance(want, (list, tuple)):
        assert len(got) == len(want), (path, len(got), len(want))
        for i, (x, y) in enumerate(zip(got, want)):
            assert_same(x, y, "%s/%d" % (path, i), vel_rtol)
    elif path.endswith("/agent_vel"):
        assert isinstance(got, np.float32), (path, type(got))
        assert abs(float(got) - float(want)) <= vel_rtol * abs(float(want)), (path, got, want)
    elif isinstance(want, np.ndarray):
        assert isinstance(got, np.ndarray) and got.dtype == want.dtype and got.shape == want.shape, \
            (path, getattr(got, "dtype", type(got)), want.dtype, getattr(got, "shape", None), want.shape)
        assert np.array_equal(got, want), (path, got.ravel()[:8], want.ravel()[:8])
    else:
        assert type(got) is type(want) and got == want, (path, type(got), type(want), got, want)


def drop_agents(out, agents):
    """`out` ({"subgraphs", "valid_agent_ids"}) without the RoIs of the listed agents."""
    keep = [i for i, a in enumerate(out["valid_agent_ids"].tolist()) if a not in set(agents)]
    return {"subgraphs": [out["subgraphs"][i] for i in keep], "valid_agent_ids": out["valid_agent_ids"][keep]}


def to_tensors(x, move):
    """numpy leaves -> tensors through `move`, recursively."""
    import torch
    if isinstance(x, dict):
        return {k: to_tensors(v, move) for k, v in x.items()}
    if isinstance(x, list):
        return [to_tensors(v, move) for v in x]
    return move(torch.from_numpy(x)) if isinstance(x, np.ndarray) and x.ndim else x


def to_numpy(x):
    """Tensor leaves -> numpy, recursively."""
    import torch
    if isinstance(x, dict):
        return {k: to_numpy(v) for k, v in x.items()}
    if isinstance(x, list):
        return [to_numpy(v) for v in x]
    return x.cpu().numpy() if torch.is_tensor(x) else x


def assert_same_tensors(x, y, path):
    """Trees of tensors and plain values: keys, lengths, dtypes, devices and values."""
    import torch
    if isinstance(x, dict):
        assert set(x) == set(y), path
        for k in x:
            assert_same_tensors(x[k], y[k], path + "/" + str(k))
    elif isinstance(x, (list, tuple)):
        assert len(x) == len(y), path
        for i, (p, q) in enumerate(zip(x, y)):
            assert_same_tensors(p, q, "%s/%d" % (path, i))
    elif torch.is_tensor(x):
        assert x.dtype == y.dtype and x.device == y.device and torch.equal(x, y), path
    else:
        assert type(x) is type(y) and x == y, (path, x, y)


def device_leaves(sg):
    """The array leaves of one RoI dict."""
    leaves = [sg["node_mask"], sg["feats"], sg["agent_feat"], sg["a2m"]["u"], sg["a2m"]["v"]]
    return leaves + [e[k] for e in sg["pre"] + sg["suc"] + [sg["left"], sg["right"]] for k in "uv"]
