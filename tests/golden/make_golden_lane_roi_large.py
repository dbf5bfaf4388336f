"""Generates tests/golden/lane_roi_large.npz by running the REFERENCE's own generate_lane_roi (data_lrcnn.py:690-844),
imported read-only through make_golden.import_reference()'s stubs, on the named scenes at real sizes that
tests/lane_roi_cases.large_scene builds (wide, chain, cap and, while the file stays below its limit, mixed).
Run in the build container only:
    python tests/golden/make_golden_lane_roi_large.py
The fixture holds the scenes' names, the scenes and the reference's output (every RoI leaf, valid_agent_ids) as data,
never reference source, the seed of every scene and the NumPy version it ran under (see make_golden_lane_roi.py).

Per scene the script searches seeds, from the one in lane_roi_cases.LARGE_SEEDS, until no agent's decision hangs on
rounding (lane_roi_model.on_edge), no lane is listed twice and the scene holds the property it is there for
(lane_roi_cases.assert_large_properties), ASSERTS all three on the reference's own output, and refuses to write unless
the seeds it found are the ones in LARGE_SEEDS: the tests build the same scenes from that table."""
import copy
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden as MG  # noqa: E402
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

LIMIT = 1000000


def sizes(out):
    return [g["num_nodes"] for g in out["subgraphs"]]


def find_seed(C, M, name):
    for seed in range(C.LARGE_SEEDS[name], C.LARGE_SEEDS[name] + 50):
        scene = C.large_scene(name, seed)
        if M.edge_agents(scene):
            continue
        once = M.generate_lane_roi(copy.deepcopy(scene))
        if sizes(once) != sizes(M.generate_lane_roi(copy.deepcopy(scene), first_occurrence=False)):
            continue                                           # a lane listed twice
        try:
            C.assert_large_properties(name, scene, once)
        except AssertionError:
            continue
        return seed, scene
    raise AssertionError("no seed for " + name)


def pack(names, scenes, outs, seeds):
    from golden_io import flatten
    out = {"names": np.asarray(names), "seeds": np.asarray(seeds, np.int64), "numpy_version": np.asarray(np.__version__)}
    flatten(scenes, "scenes/", out)
    for b, o in enumerate(outs):
        out["want/%d/valid_agent_ids" % b] = o["valid_agent_ids"]
        out["want/%d/n_rois" % b] = np.int64(len(o["subgraphs"]))
        flatten(o["subgraphs"], "want/%d/subgraphs/" % b, out)
    return out


def main():
    MG.import_reference()
    import data_lrcnn as ref
    import lanegcn_amd  # noqa: F401  (our own generator; the reference only consumes its output)
    import lane_roi_cases as C
    import lane_roi_model as M

    names, scenes, outs, seeds = [], [], [], []
    for name in ("wide", "chain", "cap", "mixed"):
        seed, scene = find_seed(C, M, name)
        out = ref.generate_lane_roi(copy.deepcopy(scene))
        assert M.edge_agents(scene) == []
        assert sizes(out) == sizes(M.generate_lane_roi(copy.deepcopy(scene)))          # no lane listed twice
        C.assert_large_properties(name, scene, out)
        print("%s: seed %d, %d nodes, %d lanes, RoI sizes %s" % (name, seed, scene["graph"]["num_nodes"],
                                                              int(scene["graph"]["lane_idcs"][-1]) + 1, sizes(out)))
        names.append(name), scenes.append(scene), outs.append(out), seeds.append(seed)
    found = dict(zip(names, seeds))
    assert found == {n: C.LARGE_SEEDS[n] for n in names}, ("set lane_roi_cases.LARGE_SEEDS to", found)
    path = os.path.join(HERE, "lane_roi_large.npz")
    while True:
        np.savez_compressed(path, **pack(names, scenes, outs, seeds))
        if os.path.getsize(path) < LIMIT or names[-1] != "mixed":
            break
        print("%d bytes with mixed: dropped" % os.path.getsize(path))
        names, scenes, outs, seeds = names[:-1], scenes[:-1], outs[:-1], seeds[:-1]
    assert os.path.getsize(path) < LIMIT and {"wide", "chain", "cap"} <= set(names)
    assert tuple(names) == C.LARGE_RECORDED, ("set lane_roi_cases.LARGE_RECORDED to", names)
    print("wrote lane_roi_large.npz (%d bytes): %s, seeds %s, NumPy %s" % (os.path.getsize(path), names, seeds, np.__version__))


if __name__ == "__main__":
    main()
