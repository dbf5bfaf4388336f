"""CPU: the host model of scene construction (tests/scene_build_model.py) against the reference's recording
(tests/golden/scene_build_b4.npz, written by tests/golden/make_golden_scene_build.py), and the fixture itself: it holds
every case the GPU tests rely on, away from every pred_range bound."""
import copy
import os

import numpy as np
import pytest

import lanegcn_amd  # noqa: F401
import scene_build_cases as C
import scene_build_compare as K
import scene_build_model as M

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "scene_build_b4.npz")


@pytest.fixture(scope="module")
def fixture():
    return C.load_fixture(GOLDEN)


def test_fixture_holds_every_case_away_from_the_bounds(fixture):
    raws, tables, lane_ids, want = fixture
    found, margin = C.found_cases(raws, tables, lane_ids)
    assert sorted(found) == sorted(C.CASES) and all(found.values()), found
    assert margin >= 1e-3, margin
    for r in raws:      # the agent's heading vector is non-zero
        assert np.abs(r["trajs"][0][18] - r["trajs"][0][19].astype(np.float32)).max() > 0
    with np.load(GOLDEN) as z:
        assert str(z["numpy_version"])
    assert os.path.getsize(GOLDEN) < 1000000
    # the generator regenerates the same inputs
    again = C.golden_inputs(int(np.load(GOLDEN)["seed"]))[0]
    for a, b in zip(again, raws):
        assert all(np.array_equal(x, y) for x, y in zip(a["trajs"], b["trajs"]))
        assert all(np.array_equal(x, y) for x, y in zip(a["steps"], b["steps"]))


def test_model_against_the_recording(fixture):
    raws, tables, lane_ids, want = fixture
    got = M.build_scenes(copy.deepcopy(raws), tables, C.CONFIG, lane_ids, cross=False)
    n_diff = n_all = 0
    for b, (g, w) in enumerate(zip(got, want)):
        d, n = K.check_against_recording(g, w, "scene %d" % b)
        n_diff, n_all = n_diff + d, n_all + n
    print("model vs recording: %d of %d position-like elements differ at all" % (n_diff, n_all))
    assert len(got[3]["graph"]["pre"][5]["u"]) > 0 and len(got[3]["graph"]["suc"][5]["u"]) > 0


def test_model_theta_override(fixture):
    raws = fixture[0]
    s = M.obj_feats(raws[0], C.PRED_RANGE, theta=0.25)
    assert s["theta"] == 0.25 and s["rot"][0, 0] == np.float32(np.cos(0.25)) and s["rot"][1, 0] == np.float32(np.sin(0.25))


def test_model_errors(fixture):
    raws, tables, _, _ = fixture
    bad = copy.deepcopy(raws[0])
    bad["steps"][3] = np.concatenate([bad["steps"][3], bad["steps"][3][:1]])
    bad["trajs"][3] = np.concatenate([bad["trajs"][3], bad["trajs"][3][:1]])
    with pytest.raises(M.ModelError, match="scene 0 track 3"):
        M.obj_feats(bad, C.PRED_RANGE)
    short = copy.deepcopy(raws[2])
    short["trajs"][0], short["steps"][0] = short["trajs"][0][:19], short["steps"][0][:19]
    with pytest.raises(M.ModelError, match="20 rows"):
        M.obj_feats(short, C.PRED_RANGE)
    far = copy.deepcopy(raws[2])
    far["trajs"][0] = far["trajs"][0] + 5000.0
    s = M.obj_feats(far, C.PRED_RANGE)
    with pytest.raises(M.ModelError, match="no lane"):
        M.lane_graph(s["orig"], s["rot"], tables["A"], C.PRED_RANGE)
