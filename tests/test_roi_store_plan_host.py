"""CPU: the host half of the resident lane-RoI store.  data_lrcnn.plan_roi_batch (the per-batch table of
lgcn_roi_store_gather and the host tables of the pick's RoiBatch) against a plain loop over the picked scenes on random
tables -- scenes with 0 RoIs, relations empty in every RoI, a single-scene store --, its four error paths, and
merge_roi_tables (RoiStore.concat's table merge) against tables built at once."""
import numpy as np
import pytest

K = 14
Q = 2 * K + 2


@pytest.fixture(scope="module")
def mods():
    import lanegcn_amd  # noqa: F401
    from lanegcn_amd import data_lrcnn
    from lanegcn_amd._lib import LgcnError
    return data_lrcnn, LgcnError


def random_rois(rng, per_scene, empty_rel=(3, 9, 13)):
    """Per-RoI tables of a store whose scene s holds per_scene[s] RoIs."""
    R = int(sum(per_scene))
    cnt = rng.integers(0, 40, (R, K + 1))
    cnt[:, list(empty_rel)] = 0                                  # relations without an edge in any RoI
    if R > 2:
        cnt[rng.integers(0, R, 2)] = 0                           # RoIs without an edge
    return dict(sizes=rng.integers(6, 700, R), scene_of=np.repeat(np.arange(len(per_scene)), per_scene),
                agent_ids=rng.integers(0, 60, R), agent_vel=rng.random(R).astype(np.float32), edge_cnt=cnt)


def tables(D, per_scene, r):
    return D.roi_store_tables(len(per_scene), r["sizes"], r["scene_of"], r["agent_ids"], r["agent_vel"], r["edge_cnt"])


def loop_tables(per_scene, r):
    """first_roi, node_off [S + 1] and edge_off [15, S + 1] scene by scene."""
    first, node, edge, at = [0], [0], [[0] for _ in range(K + 1)], 0
    for n in per_scene:
        first.append(first[-1] + n)
        node.append(node[-1] + int(sum(r["sizes"][at:at + n])))
        for k in range(K + 1):
            edge[k].append(edge[k][-1] + int(sum(r["edge_cnt"][at:at + n, k])))
        at += n
    return np.asarray(first, np.int64), np.asarray(node, np.int64), np.asarray(edge, np.int64)


def loop_plan(tb, pick):
    """The table and the pick's host tables, one picked scene and one segment at a time."""
    first, node, edge = tb["first_roi"], tb["node_off"], tb["edge_off"]
    rel_at = [int(sum(edge[:k, -1])) for k in range(K)]
    node_off, roi_off, rois = [0], [0], []
    for s in pick:
        node_off.append(node_off[-1] + int(node[s + 1] - node[s]))
        roi_off.append(roi_off[-1] + int(first[s + 1] - first[s]))
        rois += list(range(first[s], first[s + 1]))
    seg_off, seg_src = [0], []
    for q in range(Q):
        for s in pick:
            k = q % K if q < 2 * K else K
            seg_off.append(seg_off[-1] + int(edge[k, s + 1] - edge[k, s]))
            seg_src.append(int(edge[k, s]) + (rel_at[k] if q < 2 * K else 0))
    table = np.asarray(node_off + roi_off + [node[s] for s in pick] + [first[s] for s in pick] + seg_off + seg_src, np.int64)
    rel_ext = [0]
    for k in range(K):
        rel_ext.append(rel_ext[-1] + sum(int(edge[k, s + 1] - edge[k, s]) for s in pick))
    scene_of = [j for j, s in enumerate(pick) for _ in range(first[s], first[s + 1])]
    return dict(table=table, first_roi=np.asarray(roi_off, np.int64), rel_ext=np.asarray(rel_ext, np.int64),
                scene_of=np.asarray(scene_of, np.int64), sizes=tb["sizes"][rois], agent_vel=tb["agent_vel"][rois],
                edge_cnt=tb["edge_cnt"][rois], agent_ids=tb["agent_ids"][rois],
                n_nodes=node_off[-1], n_rois=roi_off[-1], n_elem=seg_off[-1], n_edges=rel_ext[-1],
                n_a2m=sum(int(edge[K, s + 1] - edge[K, s]) for s in pick))


def check_plan(D, tb, pick):
    p, want = D.plan_roi_batch(tb, pick), loop_plan(tb, list(pick))
    for k, w in want.items():
        g = getattr(p, k)
        if isinstance(w, np.ndarray):
            assert g.dtype == w.dtype and g.shape == w.shape and g.tobytes() == w.tobytes(), (k, list(pick))
        else:
            assert g == w and isinstance(g, int), (k, list(pick))
    assert p.n_scenes == len(pick) and p.table.size == 4 * len(pick) + 2 * Q * len(pick) + 3
    assert np.array_equal(p.rois_per_scene, np.diff(p.first_roi))


@pytest.mark.parametrize("seed", range(5))
def test_tables_and_plan_against_a_loop(mods, seed):
    D, _ = mods
    rng = np.random.default_rng(seed)
    per_scene = [int(x) for x in rng.integers(0, 7, int(rng.integers(4, 12)))]
    per_scene[1], per_scene[-1], per_scene[0] = 0, 0, max(per_scene[0], 1)      # scenes without an RoI, the last one too
    per_scene[2] = max(per_scene[2], 2)
    r = random_rois(rng, per_scene)
    tb = tables(D, per_scene, r)
    first, node, edge = loop_tables(per_scene, r)
    for k, w in (("first_roi", first), ("node_off", node), ("edge_off", edge)):
        assert tb[k].dtype == np.int64 and np.array_equal(tb[k], w), k
    us = [s for s, n in enumerate(per_scene) if n]
    for pick in ([us[0]], [us[-1]], [us[1], us[0], us[1]], us[::-1], [us[i % len(us)] for i in range(70)],
                 np.asarray(us, np.int32), tuple(us)):
        check_plan(D, tb, pick)


def test_single_scene_store_and_a_store_without_edges(mods):
    D, _ = mods
    rng = np.random.default_rng(7)
    r = random_rois(rng, [3])
    check_plan(D, tables(D, [3], r), [0])
    check_plan(D, tables(D, [3], r), [0, 0, 0])
    r = random_rois(rng, [1, 2], empty_rel=range(K + 1))        # no edge anywhere: every segment is empty
    check_plan(D, tables(D, [1, 2], r), [1, 0])
    tb = tables(D, [0, 0], random_rois(rng, [0, 0]))             # a store none of whose scenes holds an RoI
    assert tb["first_roi"].tolist() == [0, 0, 0] and tb["edge_off"].shape == (K + 1, 3) and not tb["edge_off"].any()


def test_error_paths(mods):
    D, LgcnError = mods
    rng = np.random.default_rng(3)
    per_scene = [2, 0, 3]
    tb = tables(D, per_scene, random_rois(rng, per_scene))
    with pytest.raises(LgcnError, match="empty pick"):
        D.plan_roi_batch(tb, [])
    for bad in ([3], [-1], [0, 2, 7]):
        with pytest.raises(LgcnError, match="outside"):
            D.plan_roi_batch(tb, bad)
    with pytest.raises(LgcnError, match="scene 1 has no lane RoI"):
        D.plan_roi_batch(tb, [2, 1, 0])
    # totals beyond 2^31 - 1: nodes, index elements
    big = tables(D, [1, 1], dict(sizes=[2 ** 29, 6], scene_of=[0, 1], agent_ids=[0, 0], agent_vel=np.zeros(2, np.float32),
                                 edge_cnt=np.zeros((2, K + 1), np.int64)))
    D.plan_roi_batch(big, [0])                                   # 2 * 2^29 half rows: fits
    with pytest.raises(LgcnError, match="32-bit"):
        D.plan_roi_batch(big, [0, 1, 0])
    cnt = np.zeros((2, K + 1), np.int64)
    cnt[0, 0] = 2 ** 29
    big = tables(D, [1, 1], dict(sizes=[6, 6], scene_of=[0, 1], agent_ids=[0, 0], agent_vel=np.zeros(2, np.float32), edge_cnt=cnt))
    D.plan_roi_batch(big, [0, 1])                                # u and v: 2^30 elements
    with pytest.raises(LgcnError, match="32-bit"):
        D.plan_roi_batch(big, [0, 0])                            # 2^31
    with pytest.raises(LgcnError, match="out of scene order"):
        D.roi_store_tables(2, [6, 6], [1, 0], [0, 0], np.zeros(2, np.float32), cnt)


@pytest.mark.parametrize("cuts", [(3,), (1, 4), (0, 2, 6), (6,)])
def test_concat_merges_the_tables_of_its_parts(mods, cuts):
    D, LgcnError = mods
    rng = np.random.default_rng(11)
    per_scene = [2, 0, 3, 1, 0, 4]
    r = random_rois(rng, per_scene)
    whole = tables(D, per_scene, r)
    first = whole["first_roi"]
    parts, lo = [], 0
    for hi in list(cuts) + [len(per_scene)]:                     # (a part may be empty, and may hold only empty scenes)
        a, b = int(first[lo]), int(first[hi])
        sub = {k: np.asarray(v)[a:b] for k, v in r.items()}
        sub["scene_of"] = sub["scene_of"] - lo
        parts.append(tables(D, per_scene[lo:hi], sub))
        lo = hi
    m = D.merge_roi_tables(parts)
    for k, w in whole.items():
        assert m[k].dtype == w.dtype and m[k].shape == w.shape and m[k].tobytes() == w.tobytes(), k
    # the runs put relation k of every part back to back: what one store of all scenes holds in edge_u
    P = len(parts)
    assert m["seg_part"].tolist() == list(range(P)) * K
    for k in range(K):
        for i, p in enumerate(parts):
            assert m["seg_len"][k * P + i] == p["edge_off"][k, -1] and m["seg_at"][k * P + i] == p["edge_off"][:k, -1].sum()
    with pytest.raises(LgcnError, match="empty list"):
        D.merge_roi_tables([])
