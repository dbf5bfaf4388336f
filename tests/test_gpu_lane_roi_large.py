"""GPU: the lane-RoI kernels (csrc/lgcn_roi.hip) at real scene sizes, at the lane cap and on their error paths.

The scenes are lane_roi_cases.large_scene's (tests/test_lane_roi_model_host.py asserts, on the CPU, the sizes they hold):
RoIs of 600 nodes (three chunks of 256 with a carry in k_roi_edge_count / k_roi_edge_fill), of 391 lanes in search order
(two chunks in k_roi_nodes), of 1,556 lanes out of 4,096 on both sides of bitset word 64, of 404 lanes of 1..3 nodes, 60
RoIs in one scene, lanes of 130 and 300 nodes, 80 new lanes in one search level, and scenes without agents at the head,
in the middle and at the tail of a batch of 12.  wide, chain and cap are held to the reference's own recording
(tests/golden/lane_roi_large.npz), the others to tests/lane_roi_model.py; index arrays, feats and dtypes exactly,
agent_vel to 1e-6, as in tests/test_gpu_lane_roi.py.

The 4,096-lane scene runs in three calls: alone, in the batch with numpy leaves, and in the batch with tensor leaves on
the device and device=True.  The last two are the batch twice: they must agree bit for bit."""
import copy

import numpy as np
import pytest
import torch

import lanegcn_amd  # noqa: F401
import lane_roi_cases as C
import lane_roi_model as M
from lanegcn_amd import data_lrcnn as D
from lanegcn_amd._lib import LgcnError

pytestmark = pytest.mark.gpu
VEL_RTOL = 1e-6
# empty_agents at the head, in the middle and at the tail; trial scenes are (seed, index)
BATCH = ("empty_agents", "cap", (11, 0), "wide", "chain", "empty_agents", "crowd", "standing", "mixed", (14, 1), "longlane",
         "empty_agents")


def _out(scene):
    return {"subgraphs": scene["subgraphs"], "valid_agent_ids": scene["valid_agent_ids"]}


@pytest.fixture(scope="module")
def runs():
    """Everything the tests below compare, computed once: the scenes by name, the expected result of each (the
    reference's recording, or the model's result, with the agents to leave out), each scene alone, and the batch twice."""
    recorded, want = C.load_large_fixture()
    scenes = dict(recorded)
    for n in C.LARGE_NAMES:
        if n not in scenes:
            scenes[n] = C.large_scene(n)
    scenes["standing"] = C.standing_scene(np.random.default_rng(21), np.int32)
    for seed, i in (k for k in BATCH if isinstance(k, tuple)):
        scenes[(seed, i)] = C.trial(seed)[i]
    assert len(BATCH) == 12 and set(BATCH) <= set(scenes)
    skip = {n: ([] if n in want else M.edge_agents(s)) for n, s in scenes.items()}
    for n, s in scenes.items():
        if n not in want:
            want[n] = _out(M.generate_lane_roi(copy.deepcopy(s)))
    alone = {n: _out(D.generate_lane_roi(copy.deepcopy(s))) for n, s in scenes.items()}
    batch = [scenes[n] for n in BATCH]
    host = D.generate_lane_roi_batch(copy.deepcopy(batch))
    tens = [C.to_tensors(s, lambda t: t.cuda()) for s in copy.deepcopy(batch)]
    dev = D.generate_lane_roi_batch(tens, device=True)
    return dict(scenes=scenes, want=want, skip=skip, alone=alone, host=host, dev=dev)


def _check(got, runs, name, path):
    skip = runs["skip"][name]
    C.assert_same(C.drop_agents(got, skip), C.drop_agents(runs["want"][name], skip), path, VEL_RTOL)


def test_recorded_scenes_alone_batched_and_from_device_tensors(runs):
    """wide, chain and cap against the reference's recording, every leaf: each alone, all in one batch, and in the batch
    whose scene leaves are tensors on the device."""
    for n in C.LARGE_RECORDED:
        assert runs["skip"][n] == [] and len(runs["want"][n]["subgraphs"]) >= 2
        assert runs["alone"][n]["valid_agent_ids"].dtype == np.int16
        _check(runs["alone"][n], runs, n, "alone/" + n)
        b = BATCH.index(n)
        _check(_out(runs["host"][b]), runs, n, "batch/" + n)
        _check(C.to_numpy(_out(runs["dev"][b])), runs, n, "tensors/" + n)


@pytest.mark.parametrize("name", ["mixed", "crowd", "longlane", "fan"])
def test_model_parity(runs, name):
    """mixed (lane offsets and node ranks off the identity over 404 lanes), crowd (60 RoIs in one scene) and longlane
    (lanes of 130 and 300 nodes, whose length numpy sums in blocks; the length routine itself is held to numpy bit for
    bit on the CPU, tests/test_lane_roi_model_host.py) and fan (one search level adds 80 lanes in bitset words 63..70 to
    the search-order list) against the model; agents on an edge left out (none here)."""
    assert len(runs["skip"][name]) <= 0.1 * len(runs["scenes"][name]["ctrs"])
    assert len(C.drop_agents(runs["want"][name], runs["skip"][name])["subgraphs"]) >= (1 if name == "fan" else 2)
    _check(runs["alone"][name], runs, name, name)


def test_every_scene_of_the_batch_equals_that_scene_alone(runs):
    """Twelve scenes in one call, scenes without agents first, in the middle and last (two equal entries in a row in the
    agent and slot tables that roi_find_seg searches): every scene's result is bit for bit the result of that scene
    alone, the empty ones get [] and an empty int16 array, and every scene equals its expected result."""
    assert [len(runs["scenes"][n]["ctrs"]) == 0 for n in BATCH] == [i in (0, 5, 11) for i in range(12)]
    for b, n in enumerate(BATCH):
        got = _out(runs["host"][b])
        C.assert_same(got, runs["alone"][n], "batch%d" % b)
        _check(got, runs, n, "want%d" % b)
        if n in ("empty_agents", "standing"):
            assert got["subgraphs"] == [] and got["valid_agent_ids"].dtype == np.int16 and got["valid_agent_ids"].shape == (0,)
    assert sum(len(s["subgraphs"]) for s in runs["host"]) >= 70


def test_device_views_equal_the_host_result_and_the_batch_repeats(runs):
    """The batch again, from tensor leaves on the device and with device=True: every leaf is a device tensor that equals
    the first run's numpy leaf bit for bit (agent_vel included: the batch twice gives the same bytes), and
    lanercnn.subgraph_gather of both gives equal output."""
    from lanegcn_amd import lanercnn as R
    host, dev = runs["host"], runs["dev"]
    for b, (d, a) in enumerate(zip(dev, host)):
        assert len(d["subgraphs"]) == len(a["subgraphs"])
        assert isinstance(d["valid_agent_ids"], np.ndarray) and d["valid_agent_ids"].dtype == np.int16
        for sd in d["subgraphs"]:
            assert isinstance(sd["num_nodes"], int) and isinstance(sd["agent_vel"], np.float32)
            assert all(torch.is_tensor(x) and x.is_cuda for x in C.device_leaves(sd))
        C.assert_same(C.to_numpy(_out(d)), _out(a), "device%d" % b)
    keep = [i for i, s in enumerate(host) if len(s["subgraphs"])]
    assert len(keep) == 8
    ga = R.subgraph_gather([dev[i]["subgraphs"] for i in keep])
    gb = R.subgraph_gather([host[i]["subgraphs"] for i in keep])
    assert set(ga) == set(gb)
    C.assert_same_tensors(ga, gb, "gather")


# ------------------------------------------------------------------ status paths
@pytest.fixture(scope="module")
def good():
    scenes, want = C.load_fixture()
    return scenes[0], want[0]


def _still_good(good):
    """A normal call after a refused one returns the right result: the status word does not stick."""
    C.assert_same(_out(D.generate_lane_roi(copy.deepcopy(good[0]))), good[1], "after", VEL_RTOL)


def _anchors(scene):
    sc = M.Scene(scene)
    return sc, [M.anchor(sc, a) for a in range(len(sc.a_ctrs)) if sc.vel[a] > 0]


def test_a_ring_of_zero_length_lanes_is_refused(good):
    """k_roi_search: the running length never grows on a ring of lanes of length 0, so the suc search runs its 4,096
    levels (bounded: the loop counts levels, nothing waits), sets kStLevels and returns without an RoI."""
    with pytest.raises(LgcnError, match="did not end"):
        D.generate_lane_roi(C.zero_ring_scene(True))
    _still_good(good)
    got = D.generate_lane_roi(C.zero_ring_scene(False))       # the agent beside the ring: the ring is never searched
    C.assert_same(_out(got), _out(M.generate_lane_roi(C.zero_ring_scene(False))), "off_ring", VEL_RTOL)


def test_a_lane_pair_outside_its_scene_is_refused(good):
    """suc_pairs is read in one place, the pair loop of k_roi_search, which compares both lanes with the scene's lane
    count before it touches a bitset (s_front, s_next) and reports kStRange."""
    scene = copy.deepcopy(good[0])
    n_lanes = int(scene["graph"]["lane_idcs"][-1]) + 1
    scene["graph"]["suc_pairs"][1, 1] = n_lanes
    with pytest.raises(LgcnError, match="outside its scene"):
        D.generate_lane_roi(scene)
    _still_good(good)


def test_a_relation_node_outside_its_scene_is_refused(good):
    """A pre relation whose v equals the node count.  edge_u / edge_v are read by roi_edge_key (k_roi_edge_rows reports
    kStRange, k_roi_edge_fill_rows leaves the edge out of the CSR rows, so roi_row and roi_local never meet it: roi_row
    checks its column against the node count once more before roi_local reads lane_idcs / node_rank with it) and by
    the closure and s_has loops of k_roi_search, which compare u and v with the node count before reading lane_idcs."""
    for k1, i in (("pre", 0), ("pre", 3)):
        scene = copy.deepcopy(good[0])
        scene["graph"][k1][i]["v"][2] = scene["graph"]["num_nodes"]
        with pytest.raises(LgcnError, match="outside its scene"):
            D.generate_lane_roi(scene)
        _still_good(good)


def test_a_lane_index_outside_its_scene_is_refused(good):
    """lane_idcs values above lane_idcs[-1] or below 0, on an anchor node and on a node that is no agent's anchor.  A lane
    id read from lane_idcs indexes the bitsets, lane_len, the lane table and roi_lane_off; it is compared with the scene's
    lane count first in k_roi_search (the anchor's lane, and lu / lv in the closure and s_has loops), in roi_local and in
    k_roi_nodes (the lanes of roi_lanes); k_roi_lane_count / k_roi_lane_fill only compare it with their own lane.
    k_roi_lane_fill reports every such node, anchor or not: no lane holds it, so no RoI could."""
    sc, anchors = _anchors(good[0])
    assert anchors and anchors[0] != sc.N - 1
    other = next(i for i in range(sc.N - 1) if i not in anchors)
    for node, val in ((anchors[0], sc.L), (anchors[0], sc.L + 40), (other, sc.L), (other, -1)):
        scene = copy.deepcopy(good[0])
        scene["graph"]["lane_idcs"][node] = val
        with pytest.raises(LgcnError, match="outside its scene"):
            D.generate_lane_roi(scene)
        _still_good(good)
    # in a batch, one bad scene fails the call whichever place it has
    bad = copy.deepcopy(good[0])
    bad["graph"]["lane_idcs"][other] = sc.L
    with pytest.raises(LgcnError, match="outside its scene"):
        D.generate_lane_roi_batch([copy.deepcopy(good[0]), C.large_scene("empty_agents"), bad])
    _still_good(good)
