"""GPU: lanegcn_amd.data_raw (csrc/lgcn_scene.hip) against the host model (tests/scene_build_model.py), bit for bit, and
against the reference's recording (tests/golden/scene_build_b4.npz) with the bounds of tests/scene_build_compare.py.

The four recorded scenes hold the cases at which the kernels can go wrong (scene_build_cases.CASES: gaps in the observed
steps, shuffled rows, tracks dropped for either reason, 300 tracks in one scene so that the compaction crosses workgroups,
2-point lanes, lanes just inside and outside the rectangle, neighbours missing / not kept / listed twice, a table of 1,500
lanes so that the lane scan crosses workgroups, explicit candidates out of table order, two cities).

Measured on an MI355X (this file's own print-out): device against the recording, 0 of 17,446 position-like elements
differ at all; the host model against the recording (tests/test_scene_build_model_host.py), 0 as well."""
import copy
import os

import numpy as np
import pytest
import torch

import lanegcn_amd  # noqa: F401
import scene_build_cases as C
import scene_build_compare as K
import scene_build_model as M

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "scene_build_b4.npz")


@pytest.fixture(scope="module")
def fixture():
    return C.load_fixture(GOLDEN)


@pytest.fixture(scope="module")
def batch5(fixture):
    """Five scenes over two cities, explicit candidates in scene 1: (raws, tables, lane_ids, model scenes without
    left / right, device scenes without left / right)."""
    from lanegcn_amd import data_raw as D
    raws, tables, lane_ids, _ = fixture
    raws, lane_ids = raws + [C.extra_scene(9)], lane_ids + [None]
    tables = {k: v.to("cuda") for k, v in tables.items()}
    want = M.build_scenes(copy.deepcopy(raws), tables, C.CONFIG, lane_ids, cross=False)
    got = D.build_scenes(copy.deepcopy(raws), tables, C.CONFIG, device=True, cross=False, lane_ids=lane_ids)
    torch.cuda.synchronize()
    return raws, tables, lane_ids, want, got


def test_device_equals_the_model_bit_for_bit(batch5):
    raws, tables, lane_ids, want, got = batch5
    assert len(got) == 5 and {r["city"] for r in raws} == {"A", "B"}
    for b, (g, w) in enumerate(zip(got, want)):
        assert g["feats"].is_cuda and g["graph"]["pre"][0]["u"].is_cuda and g["graph"]["pre"][5]["u"].is_cuda
        K.assert_same_bits(g, w, "scene %d" % b)
    assert len(got[3]["ctrs"]) > 64 and int(got[3]["graph"]["lane_idcs"][-1]) + 1 > 256       # both scans cross workgroups


def test_device_against_the_recording(batch5, fixture):
    want = fixture[3]
    n_diff = n_all = 0
    for b, w in enumerate(want):
        d, n = K.check_against_recording(batch5[4][b], w, "scene %d" % b)
        n_diff, n_all = n_diff + d, n_all + n
    print("device vs recording: %d of %d position-like elements differ at all" % (n_diff, n_all))


def test_host_leaves_with_left_and_right(batch5):
    """device=False, cross=True: numpy leaves in the reference's dtypes; left / right from the existing preprocess."""
    from lanegcn_amd import data_raw as D
    raws, tables, lane_ids, _, _ = batch5
    pick = [0, 1]
    want = M.build_scenes([copy.deepcopy(raws[b]) for b in pick], tables, C.CONFIG, [lane_ids[b] for b in pick], cross=True)
    got = D.build_scenes([copy.deepcopy(raws[b]) for b in pick], tables, C.CONFIG, device=False, lane_ids=[lane_ids[b] for b in pick])
    for b, (g, w) in enumerate(zip(got, want)):
        assert isinstance(g["feats"], np.ndarray) and g["has_preds"].dtype == bool and g["graph"]["left"]["u"].dtype == np.int16
        K.assert_same_bits(g, w, "scene %d" % b)


def test_single_scene_functions(batch5, fixture):
    """get_obj_feats / get_lane_graph with the reference's keys and dtypes; explicit lane_ids; theta=."""
    from lanegcn_amd import data_raw as D
    raws, tables, lane_ids, model, _ = batch5
    want = fixture[3]
    data = D.get_obj_feats(copy.deepcopy(raws[1]), C.CONFIG)
    assert {"feats", "obs_trajs", "ctrs", "orig", "theta", "rot", "gt_preds", "has_preds"} <= set(data)
    assert isinstance(data["theta"], np.float64) and data["orig"].shape == (2,) and data["rot"].shape == (2, 2)
    data["graph"] = D.get_lane_graph(data, tables["A"], C.CONFIG, lane_ids=lane_ids[1])
    assert isinstance(data["graph"]["num_nodes"], int) and len(data["graph"]["pre"]) == 6
    K.check_against_recording(data, want[1], "scene 1")
    K.assert_same_bits({k: data[k] for k in ("feats", "obs_trajs", "ctrs", "gt_preds", "has_preds", "graph")},
                       {k: model[1][k] for k in ("feats", "obs_trajs", "ctrs", "gt_preds", "has_preds", "graph")})
    # the same candidates in table order give another lane order, hence another graph
    other = D.get_lane_graph(data, tables["A"], C.CONFIG)
    assert not np.array_equal(other["ctrs"][:8], data["graph"]["ctrs"][:8])
    turned = D.get_obj_feats(copy.deepcopy(raws[0]), C.CONFIG, theta=0.25)
    w = M.obj_feats(raws[0], C.PRED_RANGE, theta=0.25)
    assert turned["theta"] == 0.25
    K.assert_same_bits({k: turned[k] for k in w if k != "theta"}, {k: w[k] for k in w if k != "theta"})


def test_errors_stop_the_batch(batch5, monkeypatch):
    """A repeated step, an agent track of 19 rows, a scene without a surviving lane: LgcnError that names the scene, and
    nothing is launched afterwards."""
    from lanegcn_amd import _lib, data_raw as D, ops, preprocess_data
    raws, tables, lane_ids, _, _ = batch5
    calls = []
    for mod, name in ((ops, "scene_tracks"), (ops, "scene_lanes_rank"), (ops, "scene_lanes_fill"), (preprocess_data, "dilated_nbrs"),
                      (preprocess_data, "preprocess")):
        real = getattr(mod, name)
        monkeypatch.setattr(mod, name, lambda *a, _real=real, _name=name, **k: (calls.append(_name), _real(*a, **k))[1])

    bad = copy.deepcopy(raws[:3])
    bad[1]["steps"][3] = np.concatenate([bad[1]["steps"][3], bad[1]["steps"][3][:1]])
    bad[1]["trajs"][3] = np.concatenate([bad[1]["trajs"][3], bad[1]["trajs"][3][:1]])
    with pytest.raises(_lib.LgcnError, match="scene 1 track 3 lists a step twice"):
        D.build_scenes(bad, tables, C.CONFIG)
    assert calls == ["scene_tracks", "scene_lanes_rank"]
    with pytest.raises(_lib.LgcnError, match="track 3 lists a step twice"):
        D.get_obj_feats(bad[1], C.CONFIG)

    del calls[:]
    short = copy.deepcopy(raws[:3])
    short[2]["trajs"][0], short[2]["steps"][0] = short[2]["trajs"][0][:19], short[2]["steps"][0][:19]
    with pytest.raises(_lib.LgcnError, match="scene 2.*20 rows"):
        D.build_scenes(short, tables, C.CONFIG)
    assert calls == []

    far = copy.deepcopy(raws[:3])
    far[2]["trajs"][0] = far[2]["trajs"][0] + 5000.0
    with pytest.raises(_lib.LgcnError, match="scene 2: no lane survives"):
        D.build_scenes(far, tables, C.CONFIG)
    assert calls == ["scene_tracks", "scene_lanes_rank"]
    data = D.get_obj_feats(far[2], C.CONFIG)
    del calls[:]
    with pytest.raises(_lib.LgcnError, match="no lane survives"):
        D.get_lane_graph(data, tables["A"], C.CONFIG)
    assert calls == ["scene_lanes_rank"]
    # the next call starts clean
    del calls[:]
    assert len(D.build_scenes(copy.deepcopy(raws[2:3]), tables, C.CONFIG, cross=False)) == 1
    assert calls[:3] == ["scene_tracks", "scene_lanes_rank", "scene_lanes_fill"]


def test_net_forward_end_to_end(batch5, ref_state_names):
    """Net.forward(collate_fn(build_scenes(...))) under no_grad in the default mode equals the forward on the host model's
    scenes bit for bit."""
    from lanegcn_amd import data as gen, data_raw as D, lanegcn as LG
    from oracle import lanegcn_oracle as O
    raws, tables, lane_ids, _, _ = batch5
    want = M.build_scenes(copy.deepcopy(raws), tables, C.CONFIG, lane_ids, cross=True)
    got = D.build_scenes(copy.deepcopy(raws), tables, C.CONFIG, lane_ids=lane_ids)
    for s in got:
        assert len(s["graph"]["pre"][5]["u"]) > 0 and len(s["graph"]["suc"][5]["u"]) > 0
    net = LG.Net(LG.config)
    net.load_state_dict(O.seeded_state(ref_state_names, 13), strict=True)
    net = net.cuda().eval()
    keys = ("feats", "ctrs", "orig", "theta", "rot", "gt_preds", "has_preds", "graph")
    with torch.no_grad():
        out_g = net(gen.collate_fn([{k: s[k] for k in keys} for s in got]))
        out_w = net(gen.collate_fn([{k: s[k] for k in keys} for s in want]))
    for k in ("cls", "reg"):
        for a, b in zip(out_g[k], out_w[k]):
            assert a.shape == b.shape and torch.equal(a, b), k
            assert torch.isfinite(a).all()
