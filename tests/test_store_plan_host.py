"""CPU: the host half of flatfile.DeviceSceneStore -- plan_batch over a store's offset tables -- gives the non-array
fields and the offset arrays of FlatSceneFile.batch for every pick of the GPU test, and refuses what it must."""
import numpy as np
import pytest

import scene_store_cases as SC


@pytest.fixture(scope="module")
def store(tmp_path_factory):
    import lanegcn_amd  # noqa: F401
    from lanegcn_amd.flatfile import FlatSceneFile, write_scenes
    path = str(tmp_path_factory.mktemp("store") / "split.npz")
    write_scenes(path, SC.make_scenes())
    return FlatSceneFile(path)


def _plan(store, pick):
    from lanegcn_amd.flatfile import plan_batch
    a = store.a
    return plan_batch(a["node_off"], a["actor_off"], a["edge_off"], a["rel_off"], store.num_scales, pick)


@pytest.mark.parametrize("name", sorted(SC.PICKS))
def test_plan_equals_the_host_batch(store, name):
    pick = SC.PICKS[name]
    fb, ex = store.batch(pick, device="cpu")
    p = _plan(store, pick)
    for f in SC.FLAT_FIELDS:
        assert getattr(p, f) == getattr(fb, f), f
    assert p.sizes == ex["sizes"] and all(type(x) is int for x in p.sizes)
    for f in ("node_off", "actor_off", "seg_off", "seg_base"):
        assert np.array_equal(getattr(p, f), getattr(fb, f).numpy()), f
    assert p.n_elem == fb.idx_local.numel() and p.n_seg == fb.seg_base.numel() == 2 * 14 * len(pick)
    # the table: source runs of the picked scenes, in the layout of include/lgcn.h
    B, G, a = len(pick), p.n_seg, store.a
    assert p.table.dtype == np.int64 and p.table.size == 5 * B + 2 * G + 3
    assert np.array_equal(p.table[2 * B + 2:3 * B + 2], a["node_off"][pick])
    assert np.array_equal(p.table[3 * B + 2:4 * B + 2], a["actor_off"][pick])
    assert np.array_equal(p.table[4 * B + 2:5 * B + 2], pick)
    seg_src, seg_off = p.table[5 * B + G + 3:], p.seg_off
    runs = [a[("edge_u", "edge_v")[(k // B) & 1]][s:s + n] for k, (s, n) in enumerate(zip(seg_src, np.diff(seg_off)))]
    want = np.concatenate(runs)
    assert np.array_equal(want, fb.idx_local.numpy())
    if name == "no_left_right":
        assert p.n_edges[-2:] == [0, 0]
    if name == "seventy":
        assert B + 1 > 64 and G == 1960


def test_plan_accepts_numpy_and_refuses_bad_picks(store):
    from lanegcn_amd._lib import LgcnError
    assert _plan(store, np.array([5, 0], np.int32)).sizes == _plan(store, [5, 0]).sizes
    for bad in ([-1], [0, store.n_scenes], [store.n_scenes]):
        with pytest.raises(IndexError):
            _plan(store, bad)
    with pytest.raises(LgcnError):
        _plan(store, [])
    with pytest.raises(LgcnError):
        _plan(store, np.zeros(0, np.int64))
    with pytest.raises(TypeError):
        _plan(store, [0.5])


def test_plan_refuses_totals_past_32_bits():
    """Offset tables of a store whose scenes are too large for one batch (no arrays are needed to plan)."""
    import lanegcn_amd  # noqa: F401
    from lanegcn_amd._lib import LgcnError
    from lanegcn_amd.flatfile import plan_batch
    big = 2 ** 30
    node_off, actor_off = np.array([0, big, 2 * big], np.int64), np.array([0, 1, 2], np.int64)
    edge_off, rel_off = np.zeros((14, 3), np.int64), np.zeros(15, np.int64)
    assert plan_batch(node_off, actor_off, edge_off, rel_off, 6, [0]).n_nodes == big
    with pytest.raises(LgcnError):
        plan_batch(node_off, actor_off, edge_off, rel_off, 6, [0, 1])          # 2^31 node rows
    edge_off[3] = [0, big // 2, big]
    rel_off[4:] = big
    assert plan_batch(np.array([0, 5, 9]), actor_off, edge_off, rel_off, 6, [1]).n_elem == big
    with pytest.raises(LgcnError):
        plan_batch(np.array([0, 5, 9]), actor_off, edge_off, rel_off, 6, [1, 1])   # 2^31 index elements
    with pytest.raises(LgcnError):
        plan_batch(np.array([0, 5, 9]), np.array([0, 2 ** 26, 2 ** 27]), np.zeros((14, 3), np.int64), np.zeros(15, np.int64),
                   6, [0])                                                          # 60 floats per actor
