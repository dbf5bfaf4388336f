"""CPU: tests/lane_roi_model.py against the reference's recorded generate_lane_roi output (tests/golden/lane_roi_b4.npz),
its first-occurrence rule on a hand-made lane cycle, and the share of agents of the GPU test's random trials whose
decisions hang on rounding."""
import copy

import numpy as np

import lanegcn_amd  # noqa: F401
import lane_roi_cases as C
import lane_roi_model as M


def _run(scenes, **kw):
    return [M.generate_lane_roi(copy.deepcopy(s), **kw) for s in scenes]


def _out(scene):
    return {"subgraphs": scene["subgraphs"], "valid_agent_ids": scene["valid_agent_ids"]}


def test_model_equals_the_reference_on_the_fixture():
    """Every leaf exactly (agent_vel included: the model forms it with the reference's numpy expressions), with the
    reference's duplicates switched on and, because the fixture lists no lane twice, with first occurrences too.  The
    fp32 horizon follows NumPy 2's scalar promotion, under which the fixture was recorded."""
    scenes, want = C.load_fixture()
    assert int(np.__version__.split(".")[0]) >= 2
    assert sum(len(w["subgraphs"]) for w in want) >= 8 and all(len(w["subgraphs"]) for w in want)
    for kw in (dict(first_occurrence=False), dict(first_occurrence=True)):
        for b, got in enumerate(_run(scenes, **kw)):
            C.assert_same(_out(got), want[b], "scene%d" % b)


def test_fixture_has_no_agent_on_an_edge():
    scenes, _ = C.load_fixture()
    assert all(M.edge_agents(s) == [] for s in scenes)


def test_first_occurrence_on_a_four_lane_cycle():
    """Four lanes of 3 nodes, 1.8 m each, in a ring without neighbours: the search walks the ring several times.  The
    reference's rule lists every lane once per lap; the product's rule keeps each lane once, in search order."""
    rng = np.random.default_rng(5)
    b = C.Builder(rng)
    ring = b.chain((0.0, 0.0), 0.7, [3, 3, 3, 3], 1, cycle=True, spacing=0.6)
    g, new = b.graph()
    scene = C.agents(rng, g, [(int(new[ring[0][1][1]]), 0.0, 5.0, 0.2)])
    once = M.generate_lane_roi(copy.deepcopy(scene))["subgraphs"]
    laps = M.generate_lane_roi(copy.deepcopy(scene), first_occurrence=False)["subgraphs"]
    assert len(once) == 1 and len(laps) == 1
    lanes = g["lane_idcs"][once[0]["node_mask"]]
    assert lanes.tolist() == [1] * 3 + [2] * 3 + [3] * 3 + [0] * 3          # target, then its successors round the ring
    assert once[0]["num_nodes"] == 12 and len(np.unique(once[0]["node_mask"])) == 12
    assert laps[0]["num_nodes"] > 12 and np.array_equal(laps[0]["node_mask"][:12], once[0]["node_mask"])
    assert set(laps[0]["node_mask"].tolist()) == set(once[0]["node_mask"].tolist())
    # every induced relation of the kept RoI lists each pair once, sorted by (u, v)
    for rel in once[0]["pre"] + once[0]["suc"]:
        key = rel["u"] * 12 + rel["v"]
        assert (np.diff(key) > 0).all()


def test_random_trials_leave_at_most_a_tenth_of_agents_on_an_edge():
    """The seeds of tests/test_gpu_lane_roi.py: the agents left out of its comparison are at most 10 % per trial, and the
    trials hold the sizes and topologies that test is about."""
    seen = dict(sizes=set(), dtypes=set(), shuffled=False, lanes70=False, cycle=False, empty=False, single=False)
    for seed in C.TRIAL_SEEDS:
        scenes = C.trial(seed)
        assert len(scenes) == 3
        n_agents = sum(len(s["ctrs"]) for s in scenes)
        n_edge = sum(len(M.edge_agents(s)) for s in scenes)
        assert n_edge <= 0.1 * n_agents, (seed, n_edge, n_agents)
        once, laps = _run(scenes), _run(scenes, first_occurrence=False)
        for s, o, l in zip(scenes, once, laps):
            li = np.asarray(s["graph"]["lane_idcs"], np.int64)
            assert 40 <= len(li) <= 400 and len(li) % 64 != 0
            seen["sizes"] |= set(np.bincount(li).tolist())
            seen["dtypes"].add(s["graph"]["lane_idcs"].dtype.name)
            seen["shuffled"] |= bool((np.diff(li) < 0).any())
            seen["lanes70"] |= int(li[-1]) + 1 >= 70
            seen["cycle"] |= [g["num_nodes"] for g in o["subgraphs"]] != [g["num_nodes"] for g in l["subgraphs"]]
            seen["empty"] |= len(o["subgraphs"]) == 0
            seen["single"] |= len(s["ctrs"]) == 1
    assert {1, 20} <= seen["sizes"] and seen["dtypes"] == {"int16", "int32", "int64"}
    assert all(seen[k] for k in ("shuffled", "lanes70", "cycle", "empty", "single")), seen
