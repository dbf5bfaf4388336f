"""CPU: the scene-construction entries (lgcn_scene_*, csrc/lgcn_scene.hip) refuse bad arguments before launching anything,
LaneTable refuses bad lanes, the host frame arithmetic equals the model's bit for bit, and lanegcn_amd.data_raw refuses to
run without a GPU.  Nothing here launches: every call fails its validation (device pointers are made-up addresses)."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import scene_build_cases as SC
import scene_build_model as M

OK, EINVAL, ESHAPE, EALIGN = 0, -1, -2, -3
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "scene_build_b4.npz")


@pytest.fixture(scope="module")
def lib():
    import lanegcn_amd  # noqa: F401
    from lanegcn_amd import _lib
    l = _lib.load()
    assert (l.lgcn_strerror(EINVAL), l.lgcn_strerror(ESHAPE), l.lgcn_strerror(EALIGN)) != (b"ok",) * 3
    return l, _lib


def fake(k):
    return 0x7f0000100000 + 0x1000 * k      # 16-byte aligned, never dereferenced


def tracks(mod, off, S=1, T=2, R=5):
    p = mod.SceneTracks()
    p.n_scenes, p.n_tracks, p.n_rows = S, T, R
    p.pred_range[:] = SC.PRED_RANGE
    p._off = np.asarray(off, np.int32)
    p.off_host = p._off.ctypes.data
    for k, name in enumerate(("off_dev", "xy", "step", "frame", "ws", "head", "feats", "obs", "ctrs", "gt", "has")):
        setattr(p, name, fake(k))
    return p


def test_tracks_refusals(lib):
    l, mod = lib
    good = [0, 2, 0, 3, 5]
    run = lambda p: l.lgcn_scene_tracks(C.byref(p), None)
    assert l.lgcn_scene_tracks(None, None) == EINVAL
    # the base passes every check in front of the last one: only the last pointer checked is misaligned
    p = tracks(mod, good); p.gt = fake(9) + 2
    assert run(p) == EALIGN
    for name in ("n_scenes", "n_tracks", "n_rows"):
        p = tracks(mod, good); setattr(p, name, -1)
        assert run(p) == EINVAL, name
    p = tracks(mod, good); p.pred_range[2] = float("nan")
    assert run(p) == EINVAL
    for off in ([1, 2, 0, 3, 5], [0, 1, 0, 3, 5], [0, 2, 0, 6, 5], [0, 2, 1, 3, 5], [0, 2, 0, 3, 4]):
        assert run(tracks(mod, off)) == EINVAL, off
    assert run(tracks(mod, [0, 0, 2, 0, 3, 5], S=2)) == EINVAL                # a scene without its agent
    for name in ("off_host", "off_dev", "xy", "step", "frame", "ws", "head", "feats", "obs", "ctrs", "gt", "has"):
        p = tracks(mod, good); setattr(p, name, None)
        assert run(p) == EINVAL, name
    for name, by in (("xy", 8), ("ws", 4), ("step", 2), ("off_dev", 1), ("frame", 2), ("head", 2), ("feats", 2), ("obs", 1), ("ctrs", 2)):
        p = tracks(mod, good); setattr(p, name, getattr(p, name) + by)
        assert run(p) == EALIGN, name
    p = tracks(mod, good); p.n_tracks = 0x7fffffff
    assert run(p) == ESHAPE
    p = mod.SceneTracks()
    assert run(p) == OK                                                        # an empty batch: nothing to launch
    p.n_tracks = 1
    assert run(p) == EINVAL
    assert l.lgcn_scene_tracks_ws_elems(-1) == EINVAL and l.lgcn_scene_tracks_ws_elems(1 << 40) == ESHAPE
    assert 0 < l.lgcn_scene_tracks_ws_elems(0) <= l.lgcn_scene_tracks_ws_elems(300) < l.lgcn_scene_tracks_ws_elems(100000)


TOPO = dict(pt_off=[0, 2, 5, 7], pred_off=[0, 1, 1, 2], succ_off=[0, 0, 1, 1], left=[-1, 0, -1], right=[1, -1, -1],
            flags=[0, 1, 2 | 1 << 8], pred=[2, -1], succ=[0])


def lanes(mod, off=(0, 0, 3, 0, 3), explicit=0, **change):
    topo = dict(TOPO, **change)
    p = mod.SceneLanes()
    p._topo = np.concatenate([np.asarray(topo[k], np.int32) for k in ("pt_off", "pred_off", "succ_off", "left", "right", "flags",
                                                                        "pred", "succ")])
    p._tab = (mod.LaneTableC * 1)()
    t = p._tab[0]
    t.n_lanes, t.n_pts, t.n_pred, t.n_succ = 3, 7, 2, 1
    t.topo_host, t.topo_dev, t.pts = p._topo.ctypes.data, fake(20), fake(21)
    p._off = np.asarray(off, np.int32)
    p.n_scenes, p.n_tables, p.n_cand, p.n_rank, p.explicit_ids = 1, 1, int(p._off[2]), 3, explicit
    p.pred_range[:] = SC.PRED_RANGE
    p.tabs_host, p.tabs_dev, p.off_host = C.addressof(p._tab), fake(22), p._off.ctypes.data
    p.off_dev, p.frame, p.ws, p.head, p.head2 = fake(23), fake(24), fake(25), fake(26), fake(27)
    p.n_nodes, p.cap_pre, p.cap_suc, p.cap_pre_pairs, p.cap_suc_pairs, p.cap_left_pairs, p.cap_right_pairs = 4, 3, 2, 2, 1, 3, 3
    for k, name in enumerate(("ctrs", "feats", "turn", "control", "intersect", "lane_idcs", "pre_u", "pre_v", "suc_u", "suc_v",
                              "pre_pairs", "suc_pairs", "left_pairs", "right_pairs")):
        setattr(p, name, fake(30 + k))
    return p


def test_lanes_refusals(lib):
    l, mod = lib
    rank = lambda p: l.lgcn_scene_lanes_rank(C.byref(p), None)
    fill = lambda p: l.lgcn_scene_lanes_fill(C.byref(p), None)
    assert l.lgcn_scene_lanes_rank(None, None) == EINVAL and l.lgcn_scene_lanes_fill(None, None) == EINVAL
    # the base passes every check of both stages in front of the last one
    p = lanes(mod); p.right_pairs = fake(50) + 4
    assert fill(p) == EALIGN
    p = lanes(mod, (0, 0, 2, 0, 3, 2, 0), explicit=1); p.right_pairs = fake(50) + 4
    assert fill(p) == EALIGN
    for call in (rank, fill):
        for name in ("n_scenes", "n_tables", "n_cand", "n_rank"):
            p = lanes(mod); setattr(p, name, -1)
            assert call(p) == EINVAL, name
        p = lanes(mod); p.pred_range[0] = float("nan")
        assert call(p) == EINVAL
        p = lanes(mod); p.n_tables = 0
        assert call(p) == EINVAL
        # a bad table never becomes an address
        for change in (dict(pt_off=[0, 1, 5, 7]), dict(pt_off=[0, 2, 5, 8]), dict(pt_off=[1, 2, 5, 7]), dict(pred=[3, -1]),
                       dict(pred=[2, -2]), dict(succ=[3]), dict(left=[-2, 0, -1]), dict(right=[1, -1, 3]),
                       dict(pred_off=[0, 1, 1, 1]), dict(succ_off=[0, 2, 1, 1])):
            assert call(lanes(mod, **change)) == EINVAL, change
        for off in ((1, 0, 3, 0, 3), (-1, 0, 3, 0, 3), (0, 0, 2, 0, 3), (0, 0, 3, 0, 2), (0, 1, 3, 0, 3), (0, 0, 0, 0, 3)):
            assert call(lanes(mod, off)) == EINVAL, off
        for off in ((0, 0, 2, 0, 3, 3, 0), (0, 0, 2, 0, 3, -1, 0)):           # an explicit candidate outside its table
            assert call(lanes(mod, off, explicit=1)) == EINVAL, off
        for name in ("tabs_host", "tabs_dev", "off_host", "off_dev", "frame", "ws", "head"):
            p = lanes(mod); setattr(p, name, None)
            assert call(p) == EINVAL, name
        for field in ("topo_host", "topo_dev", "pts"):
            p = lanes(mod); setattr(p._tab[0], field, None)
            assert call(p) == EINVAL, field
        for field, by in (("pts", 8), ("topo_dev", 2)):
            p = lanes(mod); setattr(p._tab[0], field, getattr(p._tab[0], field) + by)
            assert call(p) == EALIGN, field
        for name, by in (("ws", 8), ("tabs_dev", 4), ("off_dev", 2), ("frame", 1), ("head", 2)):
            p = lanes(mod); setattr(p, name, getattr(p, name) + by)
            assert call(p) == EALIGN, name
        p = lanes(mod); p._tab[0].n_lanes = -1
        assert call(p) == EINVAL
    for name in ("n_nodes", "cap_pre", "cap_suc", "cap_pre_pairs", "cap_suc_pairs", "cap_left_pairs", "cap_right_pairs"):
        p = lanes(mod); setattr(p, name, -1)
        assert fill(p) == EINVAL, name
    for name in ("head2", "ctrs", "feats", "turn", "control", "intersect", "lane_idcs", "pre_u", "pre_v", "suc_u", "suc_v",
                 "pre_pairs", "suc_pairs", "left_pairs", "right_pairs"):
        p = lanes(mod); setattr(p, name, None)
        assert fill(p) == EINVAL, name
    for name, by in (("head2", 2), ("ctrs", 1), ("control", 2), ("lane_idcs", 4), ("pre_u", 4), ("suc_v", 4), ("pre_pairs", 4)):
        p = lanes(mod); setattr(p, name, getattr(p, name) + by)
        assert fill(p) == EALIGN, name
    p = mod.SceneLanes()
    assert rank(p) == OK and fill(p) == OK                                     # an empty batch
    p.n_cand = 1
    assert rank(p) == EINVAL
    assert l.lgcn_scene_topo_elems(3, 2, 1) == 3 * 4 + 3 * 3 + 3 == len(lanes(mod)._topo)
    assert l.lgcn_scene_topo_elems(-1, 0, 0) == EINVAL and l.lgcn_scene_topo_elems(1 << 31, 0, 0) == ESHAPE
    assert l.lgcn_scene_lanes_ws_elems(-1, 0) == EINVAL and l.lgcn_scene_lanes_ws_elems(0, -1) == EINVAL
    assert l.lgcn_scene_lanes_ws_elems(1 << 31, 0) == ESHAPE and l.lgcn_scene_lanes_ws_elems(0, 1 << 31) == ESHAPE
    assert 0 < l.lgcn_scene_lanes_ws_elems(1, 1) < l.lgcn_scene_lanes_ws_elems(1500, 1500) < l.lgcn_scene_lanes_ws_elems(480000, 480000)


def test_lanes_batch_beyond_the_32_bit_scans(lib):
    """The scans are int32: a batch whose tables could hold more than 2^31 - 1 points and neighbour entries is refused."""
    l, mod = lib
    S, n_pred = 1000, 2200000
    p = lanes(mod)
    p._topo = np.concatenate([np.asarray(x, np.int32) for x in ([0, 2, 5, 7], [0, n_pred, n_pred, n_pred], [0, 0, 1, 1],
                                                                 [-1, 0, -1], [1, -1, -1], [0, 0, 0])]
                             + [np.zeros(n_pred, np.int32), np.zeros(1, np.int32)])
    p._tab[0].n_pred, p._tab[0].topo_host = n_pred, p._topo.ctypes.data
    p._off = np.concatenate([np.zeros(S), 3 * np.arange(S + 1), 3 * np.arange(S + 1)]).astype(np.int32)
    p.off_host, p.n_scenes, p.n_cand, p.n_rank = p._off.ctypes.data, S, 3 * S, 3 * S
    assert l.lgcn_scene_lanes_rank(C.byref(p), None) == ESHAPE
    p.n_scenes, p.n_cand, p.n_rank = 900, 2700, 2700                           # 900 x 2.2 M fits: on to the last check
    p._off = np.concatenate([np.zeros(900), 3 * np.arange(901), 3 * np.arange(901)]).astype(np.int32)
    p.off_host, p.right_pairs = p._off.ctypes.data, fake(50) + 4
    assert l.lgcn_scene_lanes_fill(C.byref(p), None) == EALIGN


def test_lane_table_errors():
    import lanegcn_amd  # noqa: F401
    from lanegcn_amd import _lib
    from lanegcn_amd.data_raw import LaneTable
    ok = {1: SC.Lane([[0, 0], [1, 0]], succ=[2], left=7), 2: SC.Lane([[1, 0], [2, 0], [3, 1]], turn="LEFT", pred=[1, 1, 9], right=1)}
    t = LaneTable.from_lanes(ok)
    assert t.lane_id.tolist() == [1, 2] and t.pt_off.tolist() == [0, 2, 5] and t.pts.dtype == np.float64
    assert t.pred.tolist() == [0, 0, -1] and t.pred_off.tolist() == [0, 0, 3] and t.succ.tolist() == [1] and t.succ_off.tolist() == [0, 1, 1]
    assert t.left.tolist() == [-1, -1] and t.right.tolist() == [-1, 0] and t.turn.tolist() == [0, 1] and t.turn.dtype == np.int8
    assert t.control.dtype == np.uint8 and t.intersect.dtype == np.uint8
    assert t.rows([2, 1]).tolist() == [1, 0]
    with pytest.raises(_lib.LgcnError, match="fewer than 2 points"):
        LaneTable.from_lanes({1: SC.Lane([[0, 0]])})
    with pytest.raises(_lib.LgcnError, match="fewer than 2 points"):
        LaneTable([5], [0, 1], [[0.0, 0.0]], [0], [0], [0], [0, 0], [], [0, 0], [], [-1], [-1])

    class Twice(dict):
        def keys(self):
            return [1, 1]

    with pytest.raises(_lib.LgcnError, match="duplicate"):
        LaneTable.from_lanes(Twice(ok))
    with pytest.raises(_lib.LgcnError, match="duplicate"):
        LaneTable([5, 5], [0, 2, 4], np.zeros((4, 2)), [0, 0], [0, 0], [0, 0], [0, 0, 0], [], [0, 0, 0], [], [-1, -1], [-1, -1])
    with pytest.raises(_lib.LgcnError, match="not in the lane table"):
        t.rows([3])
    with pytest.raises(_lib.LgcnError, match="twice"):
        t.rows([1, 1])


def test_host_frames_equal_the_models():
    """orig, theta, rot of a batch (vectorised) are the model's per-scene values, bit for bit; the recording's too
    (tests/test_scene_build_model_host.py holds the model to the recording)."""
    import lanegcn_amd  # noqa: F401
    from lanegcn_amd import _lib
    from lanegcn_amd.data_raw import scene_frames
    raws = SC.load_fixture(GOLDEN)[0] + [SC.extra_scene(s) for s in range(5)]
    orig, theta, rot = scene_frames(raws)
    assert orig.dtype == np.float32 and theta.dtype == np.float64 and rot.dtype == np.float32 and rot.shape == (len(raws), 2, 2)
    for b, r in enumerate(raws):
        o, th, ro = M.frame(r)
        assert orig[b].tobytes() == o.tobytes() and theta[b] == th and rot[b].tobytes() == ro.tobytes(), b
    _, th, ro = scene_frames(raws[:2], [None, 0.25])
    assert th[1] == 0.25 and ro[1].tobytes() == M.frame(raws[1], 0.25)[2].tobytes() and th[0] == theta[0]
    short = dict(raws[0], trajs=[raws[0]["trajs"][0][:19]], steps=[raws[0]["steps"][0][:19]])
    with pytest.raises(_lib.LgcnError, match="scene 1.*20 rows"):
        scene_frames([raws[0], short])


def test_public_interface_needs_a_gpu():
    import inspect
    import lanegcn_amd  # noqa: F401
    from lanegcn_amd import _lib, data_raw
    assert list(inspect.signature(data_raw.get_obj_feats).parameters) == ["data", "config", "theta"]
    assert list(inspect.signature(data_raw.get_lane_graph).parameters) == ["data", "table", "config", "lane_ids"]
    sig = inspect.signature(data_raw.build_scenes)
    assert list(sig.parameters)[:5] == ["raws", "tables", "config", "device", "cross"]
    assert sig.parameters["device"].default is True and sig.parameters["cross"].default is True
    if torch.cuda.is_available():
        return                                   # with a GPU the functions run: tests/test_gpu_scene_build.py
    raws, tables, _, want = SC.load_fixture(GOLDEN)
    with pytest.raises(_lib.LgcnError, match="needs a GPU"):
        data_raw.build_scenes(raws, tables, SC.CONFIG)
    with pytest.raises(_lib.LgcnError, match="needs a GPU"):
        data_raw.get_obj_feats(dict(raws[0]), SC.CONFIG)
    with pytest.raises(_lib.LgcnError, match="needs a GPU"):
        data_raw.get_lane_graph(want[0], tables["A"], SC.CONFIG)
