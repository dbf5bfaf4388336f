"""CPU: tests/lane_roi_model.py against the reference's recorded generate_lane_roi output (tests/golden/lane_roi_b4.npz),
its first-occurrence rule on a hand-made lane cycle, and the share of agents of the GPU test's random trials whose
decisions hang on rounding; the same against tests/golden/lane_roi_large.npz on the named scenes at real sizes, the sizes
those scenes must keep, the ring of zero-length lanes, and the library's lane length against numpy's sum."""
import copy

import numpy as np
import pytest

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


# ------------------------------------------------------------------ named scenes at real sizes (lane_roi_cases.large_scene)
@pytest.fixture(scope="module")
def large():
    """(scenes, model results, excluded agents) by name, built and run once."""
    scenes = C.large_scenes()
    return scenes, {n: M.generate_lane_roi(copy.deepcopy(s)) for n, s in scenes.items()}, \
        {n: M.edge_agents(s) for n, s in scenes.items()}


def test_large_fixture_holds_the_scenes_the_builder_builds(large):
    """tests/golden/lane_roi_large.npz records large_scene(name) itself, leaf for leaf: the GPU tests may take the
    recorded scenes from either place."""
    rec, want = C.load_large_fixture()
    assert tuple(rec) == C.LARGE_RECORDED and {"wide", "chain", "cap"} <= set(rec) and set(want) == set(rec)
    for n in rec:
        C.assert_same(rec[n], large[0][n], n)


def test_model_equals_the_reference_on_the_large_fixture():
    """Every leaf exactly, with the reference's duplicates switched on and with first occurrences (no lane is listed
    twice): RoIs of 600 nodes, of 391 lanes in search order, and of 1,556 lanes out of 4,096."""
    scenes, want = C.load_large_fixture()
    assert int(np.__version__.split(".")[0]) >= 2
    for kw in (dict(first_occurrence=False), dict(first_occurrence=True)):
        for n, s in scenes.items():
            assert len(want[n]["subgraphs"]) >= 2
            C.assert_same(_out(M.generate_lane_roi(copy.deepcopy(s), **kw)), want[n], n)


def test_large_fixture_has_no_agent_on_an_edge(large):
    assert all(large[2][n] == [] for n in C.LARGE_RECORDED)


def test_large_scenes_hold_the_sizes_they_are_there_for(large):
    """What tests/test_gpu_lane_roi_large.py relies on, read off the model's output so that the scenes cannot shrink
    unnoticed; every property is carried by an agent that the GPU comparison keeps (not on an edge), and at most 10 % of
    a scene's agents are left out.
      wide: an RoI of more than 512 nodes, ascending after a closure that grew; int16 indices, shuffled nodes, 3 agents
      chain: an RoI of more than 256 one-node lanes in search order: target, successors, then predecessors
      cap: 4,096 lanes; an anchor lane >= 2,048; an RoI of more than 1,024 lanes on both sides of bitset word 64; lane 4,095
      mixed: an RoI of more than 256 lanes of 1, 2 and 3 nodes, shuffled
      crowd: 70 or more agents, standing and turned ones among them, 40 or more RoIs
      longlane: an RoI anchored on a lane of 130..299 nodes and one on a lane of 300 or more
      fan: an RoI in search order whose anchor lane has successors in bitset words 63, 64 and 65, all of them in the RoI
      empty_agents: no agent, an empty int16 valid_agent_ids"""
    scenes, outs, skip = large
    assert set(scenes) == set(C.LARGE_NAMES)
    for n, s in scenes.items():
        assert len(skip[n]) <= 0.1 * len(s["ctrs"]), (n, skip[n])
        C.assert_large_properties(n, s, outs[n], skip[n])
    # the sizes themselves, so that a smaller scene fails here by name
    sizes = {n: sorted(g["num_nodes"] for g in outs[n]["subgraphs"]) for n in scenes}
    assert sizes["wide"][-1] > 512 and sizes["cap"][-1] > 1024 and sizes["chain"][-1] > 256 and len(sizes["crowd"]) >= 40
    assert max(len(p["lanes"]) for p in C.roi_properties(scenes["mixed"], outs["mixed"])) > 256
    assert max(p["sizes"][0] for p in C.roi_properties(scenes["longlane"], outs["longlane"])) >= 300


def test_a_ring_of_zero_length_lanes_never_ends():
    """The model raises on an agent anchored on a ring of three one-node lanes of length exactly 0; the same scene with
    the agent on the chain beside the ring runs."""
    on, off = C.zero_ring_scene(True), C.zero_ring_scene(False)
    sc = M.Scene(on)
    ring = np.flatnonzero(sc.lane_len == 0)
    assert len(ring) == 3 and int(sc.lane_idcs[M.anchor(sc, 0)]) in ring
    with pytest.raises(RuntimeError, match="did not end"):
        M.generate_lane_roi(copy.deepcopy(on))
    assert int(sc.lane_idcs[M.anchor(M.Scene(off), 0)]) not in ring
    assert len(M.generate_lane_roi(copy.deepcopy(off))["subgraphs"]) == 1


def test_lane_length_of_the_library_equals_numpy_at_every_size():
    """lgcn_roi_lane_length_host is the kernels' own lane-length routine (csrc/lgcn_roi.hip, roi_lane_length) compiled
    for the host.  Bit for bit against the model's expression np.sum(np.sqrt(np.sum(np.square(feats), -1))): below 8
    elements in order, up to 128 with 8 accumulators, above in halves (numpy's pairwise_sum), above 8,192 through
    numpy's reduction buffer; node ids permuted, three scales."""
    from lanegcn_amd import _lib
    lib = _lib.load()
    assert np.getbufsize() == 8192
    rng = np.random.default_rng(0)
    sizes = list(range(0, 140)) + [255, 256, 257, 263, 264, 265, 300, 511, 512, 513, 1000, 1023, 1025, 4096, 5000, 8191, 8192,
                                   8193, 8320, 8321, 16384, 16385, 20001]
    for n in sizes:
        for scale in (0.3, 1.0, 40.0):
            feats = (rng.normal(0.0, scale, (n + 5, 2))).astype(np.float32)
            nodes = rng.permutation(n + 5)[:n].astype(np.int32)
            want = np.sum(np.sqrt(np.sum(np.square(feats[nodes]), axis=-1))) if n else np.float32(0.0)
            got = np.float32(lib.lgcn_roi_lane_length_host(feats.ctypes.data, nodes.ctypes.data, n))
            assert got == np.float32(want), (n, scale, got, want)
    assert np.isnan(lib.lgcn_roi_lane_length_host(None, None, 3)) and np.isnan(lib.lgcn_roi_lane_length_host(None, None, -1))
