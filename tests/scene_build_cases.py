"""Raw scenes and lane maps for the scene-construction tests (lanegcn_amd.data_raw): plain arrays and small lane objects
with the attributes the reference's get_lane_graph reads.  Geometry is laid out in the SCENE frame of a chosen agent pose
and mapped back to the world, so that a lane or a track can be put a known distance from a pred_range bound."""
import numpy as np

PRED_RANGE = [-100.0, 100.0, -100.0, 100.0]
CONFIG = {"pred_range": PRED_RANGE, "num_scales": 6, "cross_dist": 6.0}


class Lane:
    def __init__(self, centerline, turn="NONE", control=False, intersect=False, pred=None, succ=None, left=None, right=None):
        self.centerline = np.asarray(centerline, np.float64)
        self.turn_direction, self.has_traffic_control, self.is_intersection = turn, control, intersect
        self.predecessors, self.successors, self.l_neighbor_id, self.r_neighbor_id = pred, succ, left, right


class Pose:
    """An agent pose: world position of step 19, heading phi.  to_world maps scene-frame points (x ahead) to the world
    approximately (the tests never rely on it being exact: margins are asserted on the transformed values)."""

    def __init__(self, x, y, phi):
        self.p, self.phi = np.array([x, y], np.float64), float(phi)

    def to_world(self, pts):
        # the reference's frame: theta = pi - atan2(p18 - p19) = -phi for an agent that moves along phi
        c, s = np.cos(self.phi), np.sin(self.phi)
        return self.p[None, :] + np.asarray(pts, np.float64).reshape(-1, 2) @ np.array([[c, s], [-s, c]])

    def agent(self, n_rows=50, speed=0.9):
        k = (np.arange(n_rows) - 19)[:, None] * speed
        return self.to_world(np.concatenate([k, 0.01 * k ** 2 / 10.0], 1)), np.arange(n_rows, dtype=np.int64)


def line(a, b, n):
    return np.linspace(np.asarray(a, np.float64), np.asarray(b, np.float64), n)


def city_a(pose, rng, n_random=40):
    """A hand-made city around `pose` (see the case list in tests/golden/make_golden_scene_build.py) plus random lanes."""
    W = pose.to_world
    lanes = {
        10: Lane(W(line((0, 0), (10, 0), 2)), pred=[999], succ=[11], left=20),                    # 2 points; pred not in the table
        11: Lane(W(line((10, 0), (50, 0), 10)), turn="LEFT", pred=[10, 10], succ=[12], left=20, right=777),   # pred twice
        12: Lane(W(line((50, 0), (90, 5), 6)), turn="RIGHT", control=True, pred=[11], succ=None),
        13: Lane(W(line((100.5, -20), (60, -20), 5)), intersect=True, pred=[14], succ=[15]),      # pred in the table, not kept
        14: Lane(W(line((130, -20), (100.5, -20), 4)), succ=[13]),                                # just outside
        15: Lane(W(line((60, -20), (20, -22), 7)), pred=[13], succ=[16, 17], control=True, intersect=True),
        16: Lane(W(line((20, -22), (-30, -22), 5)), pred=[15], right=17),
        17: Lane(W(line((20, -22), (0, -60), 5)), pred=[15], left=16, right=14),                  # right neighbour not kept
        18: Lane(W(line((99.5, 20), (130, 20), 3)), pred=None, succ=None),                        # just inside
        20: Lane(W(line((0, 3.5), (50, 3.5), 8)), right=11, succ=[12]),
        21: Lane(W(line((-99.5, 150), (-130, 99.5), 3))),                                         # corner: extents just inside
        22: Lane(W(line((-100.5, 0), (-140, 10), 3)), succ=[16]),                                 # just outside on the other side
        23: Lane(W(line((0, -40), (88, -41), 45)), pred=[17], succ=[13]),                         # 44 nodes: pre[5] / suc[5] exist
    }
    ids = list(range(100, 100 + n_random))
    for k in ids:
        a = rng.uniform(-160, 160, 2)
        th = rng.uniform(0, 2 * np.pi)
        n = int(rng.integers(2, 12))
        d = rng.uniform(2.0, 6.0)
        pts = a[None, :] + d * np.arange(n)[:, None] * np.array([np.cos(th), np.sin(th)])[None, :]
        pick = lambda m: [int(x) for x in rng.choice(ids + [10, 11, 14, 555], m)]
        lanes[k] = Lane(W(pts), turn=str(rng.choice(["NONE", "LEFT", "RIGHT"])), control=bool(rng.random() < 0.3),
                        intersect=bool(rng.random() < 0.3), pred=pick(int(rng.integers(0, 3))) if rng.random() < 0.8 else None,
                        succ=pick(int(rng.integers(0, 3))), left=int(rng.choice(ids)) if rng.random() < 0.3 else None,
                        right=int(rng.choice(ids + [556])) if rng.random() < 0.3 else None)
    return lanes


def city_b(pose, n_x=50, n_y=30):
    """1,500 short lanes on a grid of 8 m x 9 m cells around `pose`: rows chained by successors, neighbours across rows."""
    W = pose.to_world
    lanes = {}
    lid = lambda i, j: 1000 + j * n_x + i
    for j in range(n_y):
        for i in range(n_x):
            x, y = (i - n_x / 2) * 8.0 + 0.37, (j - n_y / 2) * 9.0 + 0.21
            n = 2 + (i + j) % 2
            lanes[lid(i, j)] = Lane(W(line((x, y), (x + 8.0, y), n)), turn=("NONE", "LEFT", "RIGHT")[(i * 7 + j) % 3],
                                    control=(i + 2 * j) % 5 == 0, intersect=(i * j) % 7 == 0,
                                    pred=[lid(i - 1, j)] if i > 0 else [], succ=[lid(i + 1, j)] if i + 1 < n_x else None,
                                    left=lid(i, j + 1) if j + 1 < n_y else None, right=lid(i, j - 1) if j > 0 else None)
    return lanes


def random_track(rng, pose, reach=80.0, steps=None):
    if steps is None:
        lo = int(rng.integers(0, 19))
        hi = int(rng.integers(20, 51))
        steps = np.arange(lo, hi)
        steps = steps[rng.random(len(steps)) < 0.9]
    steps = np.asarray(steps, np.int64)
    start = rng.uniform(-reach, reach, 2)
    th = rng.uniform(0, 2 * np.pi)
    v = rng.uniform(0.0, 1.5)
    pts = start[None, :] + v * (steps - 19)[:, None] * np.array([np.cos(th), np.sin(th)])[None, :] + rng.normal(0, 0.05, (len(steps), 2))
    return pose.to_world(pts), steps


def special_tracks(rng, pose):
    """name -> (xy, steps): the track cases of the issue's list."""
    t = {}
    t["only_19"] = random_track(rng, pose, steps=[19])
    t["gap_15_16_18_19"] = random_track(rng, pose, steps=[15, 16, 18, 19])
    t["no_19"] = random_track(rng, pose, steps=[12, 13, 14, 15, 16, 17, 18, 20, 21, 22])
    xy, st = random_track(rng, pose, steps=np.arange(5, 40))
    t["ends_outside"] = (xy + (pose.to_world([[150.0, 0.0]]) - pose.p), st)
    xy, st = random_track(rng, pose, steps=np.arange(50))
    perm = rng.permutation(50)
    t["shuffled_50"] = (xy[perm], st[perm])
    t["steps_over_49"] = random_track(rng, pose, steps=np.arange(10, 56))
    return t


def raw_scene(city, tracks):
    return {"city": city, "trajs": [np.asarray(xy, np.float64) for xy, _ in tracks],
            "steps": [np.asarray(st, np.int64) for _, st in tracks]}


def golden_inputs(seed):
    """(raws, lane maps {city: {id: Lane}}, lane_ids per scene, names of the special tracks of scene 0)."""
    rng = np.random.default_rng(seed)
    pa, pb = Pose(2570.25, 1180.5, 0.7), Pose(-412.0, 903.75, -2.1)
    maps = {"A": city_a(pa, rng), "B": city_b(pb)}
    special = special_tracks(rng, pa)
    s0 = raw_scene("A", [pa.agent()] + list(special.values()) + [random_track(rng, pa) for _ in range(6)])
    p1 = Pose(2570.25 + 35.0, 1180.5 - 20.0, 2.4)
    s1 = raw_scene("A", [p1.agent(40)] + [random_track(rng, p1) for _ in range(9)])
    s2 = raw_scene("A", [Pose(2560.0, 1175.0, -0.3).agent(20)])                    # the agent alone
    s3 = raw_scene("B", [pb.agent()] + [random_track(rng, pb, 130.0, steps=[[19], [18, 19], [19, 20, 21], [17, 18]][int(rng.integers(4))])
                                        for _ in range(299)])                      # 300 tracks
    ids1 = list(maps["A"].keys())
    ids1 = [ids1[i] for i in rng.permutation(len(ids1))]                           # explicit candidates, not in table order
    ids1.remove(23)
    ids1 = ([23] + ids1)[:len(ids1) - 4]
    return [s0, s1, s2, s3], maps, [None, ids1, None, None], list(special)


CASES = ("only_19", "gap_15_16_18_19", "no_19", "ends_outside", "shuffled_50", "steps_over_49", "agent_alone", "tracks_300",
         "two_point_lane", "just_inside", "just_outside", "pred_not_in_table", "pred_not_kept", "pred_twice", "no_left_right",
         "table_1500", "explicit_not_table_order", "two_cities")


def found_cases(raws, tables, lane_ids, pred_range=PRED_RANGE):
    """(name -> found, smallest distance of a keep / drop decision from a pred_range bound) over the scenes, by the host
    model's arithmetic.  `tables`: {city: LaneTable}."""
    import scene_build_model as M
    x_min, x_max, y_min, y_max = pred_range
    c = dict.fromkeys(CASES, False)
    margin = np.inf
    c["two_cities"] = len({r["city"] for r in raws}) >= 2
    for b, raw in enumerate(raws):
        orig, theta, rot = M.frame(raw)
        steps = [np.asarray(s, np.int64) for s in raw["steps"]]
        c["agent_alone"] |= len(steps) == 1
        c["tracks_300"] |= len(steps) >= 300
        for xy, s in zip(raw["trajs"], steps):
            c["only_19"] |= s.tolist() == [19]
            c["gap_15_16_18_19"] |= sorted(s.tolist()) == [15, 16, 18, 19]
            c["no_19"] |= 19 not in s
            c["shuffled_50"] |= sorted(s.tolist()) == list(range(50)) and s.tolist() != list(range(50))
            c["steps_over_49"] |= bool((s >= 50).any())
            if 19 in s:
                p = M.xform(np.asarray(xy)[s == 19], orig, rot).astype(np.float32)[0].astype(np.float64)
                d = np.array([p[0] - x_min, x_max - p[0], p[1] - y_min, y_max - p[1]])
                c["ends_outside"] |= bool((d < 0).any())
                margin = min(margin, float(np.abs(d).min()))
        tab = tables[raw["city"]]
        c["table_1500"] |= tab.n_lanes >= 1500
        rows = np.arange(tab.n_lanes) if lane_ids[b] is None else tab.rows(lane_ids[b])
        c["explicit_not_table_order"] |= lane_ids[b] is not None and bool((np.diff(rows) < 0).any())
        kept = set()
        for r in rows:
            q = M.xform(tab.pts[tab.pt_off[r]:tab.pt_off[r + 1]], orig, rot)
            d = np.array([q[:, 0].max() - x_min, x_max - q[:, 0].min(), q[:, 1].max() - y_min, y_max - q[:, 1].min()])
            margin = min(margin, float(np.abs(d).min()))
            if (d >= 0).all():
                kept.add(int(r))
                c["just_inside"] |= bool(d.min() < 1.0)
                c["two_point_lane"] |= len(q) == 2
            else:
                c["just_outside"] |= bool(-d.min() < 1.0)
        for r in kept:
            pred = tab.pred[tab.pred_off[r]:tab.pred_off[r + 1]].tolist()
            c["pred_not_in_table"] |= -1 in pred
            c["pred_not_kept"] |= any(j >= 0 and j not in kept for j in pred)
            kp = [j for j in pred if j in kept]
            c["pred_twice"] |= len(set(kp)) < len(kp)
            c["no_left_right"] |= tab.left[r] < 0 and tab.right[r] < 0
    return c, margin


def load_fixture(path):
    """(raws, {city: LaneTable}, lane_ids per scene, the reference's recorded scenes) of tests/golden/scene_build_b4.npz."""
    from golden_io import unflatten
    from lanegcn_amd.data_raw import LaneTable
    with np.load(path) as z:
        flat = {k: z[k] for k in z.files}
    raws = unflatten(flat, "raws")
    for r in raws:
        r["city"] = str(r["city"])
    tables = {city: LaneTable(**arrays) for city, arrays in unflatten(flat, "tables").items()}
    lane_ids = [flat["lane_ids/%d" % b].tolist() if "lane_ids/%d" % b in flat else None for b in range(len(raws))]
    want = unflatten(flat, "want")
    for w in want:
        w["graph"]["num_nodes"] = int(w["graph"]["num_nodes"])
    return raws, tables, lane_ids, want


def extra_scene(seed):
    """A fifth scene in city B for the mixed batch."""
    rng = np.random.default_rng(seed)
    p = Pose(-412.0 + 60.0, 903.75 + 10.0, 0.4)
    return raw_scene("B", [p.agent()] + [random_track(rng, p) for _ in range(20)])
