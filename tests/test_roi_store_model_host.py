"""CPU: the numpy model of the resident lane-RoI store (roi_store_model) on the RoIs that lane_roi_model.generate_lane_roi
extracts.  For every pick, the model's gather out of the resident layout equals the model's merged graph of the picked
scenes alone -- arrays and host tables, exactly -- and the library's host half (data_lrcnn.roi_store_tables,
plan_roi_batch) gives the model's tables and the model's per-batch table.  data_lrcnn.relation_major_tables is the same
function on both sides."""
import copy

import numpy as np
import pytest

import lane_roi_cases as C
import lane_roi_model as M
import roi_store_model as RS

ARRAYS = ("feats", "node_mask", "agent_feat", "u", "v", "a2m_u", "a2m_v")
TABLES = ("sizes", "scene_of", "agent_vel", "rel_ext", "edge_cnt", "first_roi", "agent_ids")


@pytest.fixture(scope="module")
def D():
    import lanegcn_amd  # noqa: F401
    from lanegcn_amd import data_lrcnn
    return data_lrcnn


def batches():
    return {"shuffle": C.trial(12), "dup_edges": C.trial(15),
            "standing_added": C.trial(16) + [C.standing_scene(np.random.default_rng(5), np.int16)]}


@pytest.fixture(scope="module")
def extracted():
    return {name: [M.generate_lane_roi(copy.deepcopy(s)) for s in scenes] for name, scenes in batches().items()}


def same(got, want, keys, what):
    for k in keys:
        assert got[k].dtype == want[k].dtype and got[k].shape == want[k].shape and got[k].tobytes() == want[k].tobytes(), (what, k)


@pytest.mark.parametrize("name", ["shuffle", "dup_edges", "standing_added"])
def test_gather_equals_the_model_on_the_picked_scenes_alone(D, extracted, name):
    scenes = extracted[name]
    st = RS.build(scenes)
    tb = D.roi_store_tables(len(scenes), st["sizes"], np.repeat(np.arange(len(scenes)), np.diff(st["first_roi"])),
                            st["agent_ids"], st["agent_vel"], st["edge_cnt"])
    same(tb, st, ("first_roi", "node_off", "edge_off", "sizes", "agent_vel", "edge_cnt", "agent_ids"), name)
    for pick in RS.picks_of(st):
        got = RS.gather(st, pick, D.relation_major_tables)
        want = RS.merged([scenes[i] for i in pick], D.relation_major_tables)
        same(got, want, ARRAYS + TABLES + tuple("row_" + k for k in RS.ROW_KEYS), (name, pick))
        plan = D.plan_roi_batch(tb, pick)                         # the library's host half against the model's
        assert plan.table.dtype == np.int64 and plan.table.tobytes() == got["table"].tobytes(), (name, pick)
        for k in TABLES:
            x = getattr(plan, k)
            assert x.dtype == got[k].dtype and x.tobytes() == got[k].tobytes(), (name, pick, k)
        assert (plan.n_scenes, plan.n_nodes, plan.n_rois) == (len(pick), len(got["feats"]), len(got["sizes"]))
        assert (plan.n_edges, plan.n_a2m, plan.n_elem) == (len(got["u"]), len(got["a2m_u"]), 2 * len(got["u"]) + 2 * len(got["a2m_u"]))


def test_the_standing_scene_is_in_the_store_and_cannot_be_picked(D, extracted):
    from lanegcn_amd._lib import LgcnError
    scenes = extracted["standing_added"]
    st = RS.build(scenes)
    last = len(scenes) - 1
    assert len(scenes[last]["subgraphs"]) == 0 and len(st["first_roi"]) == len(scenes) + 1
    assert st["first_roi"][last + 1] == st["first_roi"][last] and last not in RS.usable(st)
    with pytest.raises(ValueError, match="scene %d has no lane RoI" % last):
        RS.gather(st, [0, last], D.relation_major_tables)
    with pytest.raises(LgcnError, match="scene %d has no lane RoI" % last):
        D.plan_roi_batch(st, [0, last])
