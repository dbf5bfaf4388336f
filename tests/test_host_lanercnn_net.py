"""CPU: the host side of the fork model's Net -- state_dict names and shapes and config keys against the reference's
(tests/golden/lanercnn_net_state_names.json), the plugin shim, the host bookkeeping of subgraph_gather against the
reference's own (lanercnn_net_b3.npz), and the synthetic lane-RoI generator."""
import numpy as np
import pytest
import torch

import lanercnn_net_fixture as NF


@pytest.fixture(scope="module")
def mods():
    import lanegcn_amd  # noqa: F401
    from lanegcn_amd import data as gen
    from lanegcn_amd import lanercnn as R
    return gen, R


def test_state_dict_names_and_shapes(mods):
    _, R = mods
    _, names = NF.fixture()
    net = R.Net(R.config)
    assert [[k, list(v.shape)] for k, v in net.state_dict().items()] == names["net"]
    assert [n for n, _ in net.named_children()] == ["input", "roi_net1", "interactor", "roi_net2", "decode"]


def test_config_has_the_reference_keys(mods):
    _, R = mods
    _, names = NF.fixture()
    assert sorted(R.config.keys()) == names["config"]
    c = R.config
    assert (c["opt"], c["weight_decay"], c["batch_size"], c["num_mods"], c["num_preds"], c["n_map"]) == ("adamw", 0.01, 10, 6, 30, 128)
    assert c["lr_func"](0) == 1e-3 and c["lr_func"](32) == 1e-4


def test_plugin_shim(mods):
    _, R = mods
    import lanercnn_mi355x as P
    assert P.get_model is R.get_model and P.get_model_for_torch_dist is R.get_model_for_torch_dist
    assert P.config is R.config and P.Net is R.Net and P.Loss is R.Loss and P.PostProcess is R.PostProcess


def test_host_bookkeeping_equals_the_reference(mods):
    gen, R = mods
    g, _ = NF.fixture()
    batch = gen.collate_fn(NF.scenes())
    book = R.subgraph_bookkeeping(batch["subgraphs"])
    assert sorted(book) == sorted(NF.HOST_KEYS)
    for k in NF.HOST_KEYS:
        got = book[k].tolist() if torch.is_tensor(book[k]) else book[k]
        assert got == NF.host_value(g, k), k
    assert isinstance(book["num_nodes"], int) and book["interest_roi"].dtype == torch.int64
    # numpy leaves give the same
    assert R.subgraph_bookkeeping([s["subgraphs"] for s in NF.scenes()])["roi_spans"] == book["roi_spans"]


def test_scene_without_subgraphs_is_refused(mods):
    gen, R = mods
    subs = [s["subgraphs"] for s in NF.scenes()]
    subs[1] = []
    with pytest.raises(AssertionError, match="batch 1 have empty subgraphs"):
        R.subgraph_bookkeeping(subs)
    with pytest.raises(AssertionError, match="batch 1 have empty subgraphs"):
        R.subgraph_gather(subs)


def test_synth_subgraphs(mods):
    gen, _ = mods
    rng = np.random.default_rng(5)
    scene = gen.synth_scene(rng, [4, 3], 7)
    scene["feats"][2, :, :2] = 0.0                                       # an agent that does not move gets no RoI
    assert "obs_trajs" not in scene
    out = gen.synth_subgraphs(scene, horizon_time=0.5, horizon_buffer=6.0)
    assert out is scene and scene["obs_trajs"].shape == (7, 20, 3)
    assert np.allclose(scene["obs_trajs"][:, -1, :2], scene["ctrs"], atol=1e-5)
    assert np.allclose(np.diff(scene["obs_trajs"][:, :, :2], axis=1), scene["feats"][:, 1:, :2], atol=1e-4)
    valid = scene["valid_agent_ids"]
    assert valid.dtype == np.int16 and 2 not in valid and len(valid) == len(scene["subgraphs"]) >= 1
    graph = scene["graph"]
    for a, sg in zip(valid, scene["subgraphs"]):
        n = sg["num_nodes"]
        assert n >= 6 and sg["feats"].shape == (n, 8) and sg["feats"].dtype == np.float32 and sg["agent_feat"].shape == (80,)
        assert np.array_equal(sg["feats"][:, :2], graph["ctrs"][sg["node_mask"]])
        assert np.array_equal(sg["feats"][:, 2:4], graph["feats"][sg["node_mask"]])
        assert np.array_equal(sg["agent_feat"].reshape(20, 4)[:, :2], scene["obs_trajs"][a, :, :2])
        assert float(sg["agent_vel"]) > 0
        assert len(sg["pre"]) == len(sg["suc"]) == 6
        for k1, i in NF.REL_KEYS:
            e, full = NF.rel(sg, k1, i), NF.rel(graph, k1, i)
            assert len(e["u"]) == len(e["v"])
            assert all(0 <= int(x) < n for x in e["u"]) and all(0 <= int(x) < n for x in e["v"])
            # the induced subgraph: exactly the relation's edges with both ends in the RoI
            want = {(int(u), int(v)) for u, v in zip(full["u"], full["v"])} & {(int(u), int(v)) for u in sg["node_mask"] for v in sg["node_mask"]}
            assert {(int(sg["node_mask"][u]), int(sg["node_mask"][v])) for u, v in zip(e["u"], e["v"])} == want
        assert len(sg["pre"][0]["u"]) + len(sg["suc"][0]["u"]) > 0
        assert np.all(sg["a2m"]["u"] == 0) and all(0 <= int(x) < n for x in sg["a2m"]["v"])
        near = np.sqrt(((sg["feats"][:, :2] - scene["ctrs"][a]) ** 2).sum(-1)) < 5.0
        assert np.array_equal(np.nonzero(near)[0], sg["a2m"]["v"])
    # existing valid_agent_ids / obs_trajs of a scene are kept when they are there
    keep = scene["obs_trajs"].copy()
    gen.synth_subgraphs(scene, max_rois=2)
    assert len(scene["subgraphs"]) == 2 and np.array_equal(scene["obs_trajs"], keep)


def test_collate_carries_subgraphs(mods):
    gen, _ = mods
    rng = np.random.default_rng(6)
    scenes = [gen.synth_subgraphs(gen.synth_scene(rng, [3], 4)), gen.synth_subgraphs(gen.synth_scene(rng, [4], 5))]
    batch = gen.collate_fn(scenes)
    assert len(batch["subgraphs"]) == 2 and len(batch["valid_agent_ids"]) == 2 and len(batch["obs_trajs"]) == 2
    for b, s in enumerate(scenes):
        assert len(batch["subgraphs"][b]) == len(s["subgraphs"])
        sg = batch["subgraphs"][b][0]
        assert torch.is_tensor(sg["feats"]) and torch.is_tensor(sg["pre"][0]["u"]) and torch.is_tensor(sg["a2m"]["v"])
        assert torch.equal(sg["left"]["u"], torch.from_numpy(s["subgraphs"][0]["left"]["u"]))
        assert batch["valid_agent_ids"][b].dtype == torch.int16


def test_roi_dataset_items(mods):
    gen, _ = mods
    ds = gen.SyntheticLaneRoIDataset(length=2, roads=(3,), n_actors=4)
    item = ds[1]
    assert len(ds) == 2 and item["idx"] == 1 and len(item["subgraphs"]) >= 1 and "obs_trajs" in item
