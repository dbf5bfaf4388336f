"""Generates tests/golden/lane_roi_b4.npz by running the REFERENCE's own generate_lane_roi (data_lrcnn.py:690-844),
imported read-only through make_golden.import_reference()'s stubs, on four small scenes built by tests/lane_roi_cases.py.
Run in the build container only:
    python tests/golden/make_golden_lane_roi.py
The fixture holds the scenes and the reference's output (every RoI leaf, valid_agent_ids) as data, never reference source,
and the NumPy version it ran under (the fp32 horizon v * 3 + 20 depends on NumPy 2's scalar promotion).

The script searches seeds and ASSERTS that the four scenes hold every case the tests rely on (see `cases`) and that no
agent's decision hangs on rounding (lane_roi_model.on_edge)."""
import copy
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden as MG  # noqa: E402
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

REL = [("pre", i) for i in range(6)] + [("suc", i) for i in range(6)] + [("left", None), ("right", None)]


def make_scenes(C, seed):
    rng = np.random.default_rng(seed)
    # A: a doubled chain (the closure adds the parallel lanes) and, far away, a single chain without neighbours
    b = C.Builder(rng)
    dbl = b.chain((0.0, 0.0), 0.3, [6, 7, 5, 8], 2)
    single = b.chain((400.0, 0.0), 2.0, [5, 6, 7, 6, 5], 1)
    g, new = b.graph(np.int64)
    a = C.agents(rng, g, [(int(new[dbl[0][1][3]]), 0.1, 7.0, 0.4), (int(new[single[0][2][3]]), -0.1, 9.0, 0.5),
                          (int(new[dbl[1][2][1]]), 0.0, 0.0, 0.3), (int(new[single[0][1][2]]), 0.05, 3.0, -0.6)])
    # B: every lane heads the same way: an agent against the traffic, one across it (pi/2 fallback), one along it
    b = C.Builder(rng)
    ch = b.chain((0.0, 0.0), 1.0, [8, 8, 8], 1)
    g2, new = b.graph(np.int32)
    a2 = C.agents(rng, g2, [(int(new[ch[0][1][2]]), np.pi, 5.0, 0.3), (int(new[ch[0][1][4]]), 1.1, 6.0, -0.3),
                            (int(new[ch[0][0][5]]), 0.0, 8.0, 0.2)])
    # C: a lane of 4 nodes on its own, seven one-node lanes joined only by left / right edges, and a chain whose agent
    #    drives 8 m beside it (no node within 5 m: an empty a2m)
    b = C.Builder(rng)
    short = b.chain((0.0, 0.0), 0.5, [4], 1)
    cl = b.cluster((400.0, 0.0), 1.5, 7)
    far = b.chain((0.0, 400.0), 2.5, [6, 6], 1)
    g3, new = b.graph(np.int16)
    a3 = C.agents(rng, g3, [(int(new[short[0][0][1]]), 0.0, 4.0, 0.3), (int(new[cl[3]]), 0.0, 5.0, 0.2),
                            (int(new[far[0][0][4]]), 0.05, 6.0, 8.0)])
    return [a, a2, a3, C.random_scene(rng, 14, 6, np.int64)]


def cases(M, scenes, outs):
    """name -> True for every case found in the four scenes."""
    c = dict.fromkeys(("closure_ascending", "not_ascending_no_neighbours", "standing", "no_anchor", "fallback", "under_6",
                       "no_pre0_suc0_edge", "empty_relation", "empty_a2m"), False)
    for s, out in zip(scenes, outs):
        sc = M.Scene(s)
        valid = set(out["valid_agent_ids"].tolist())
        for sg in out["subgraphs"]:
            c["empty_relation"] |= any(len((sg[k1] if i is None else sg[k1][i])["u"]) == 0 for k1, i in REL)
            c["empty_a2m"] |= len(sg["a2m"]["v"]) == 0
        for a in range(len(sc.a_ctrs)):
            if sc.vel[a] == 0:
                c["standing"] = True
                continue
            node = M.anchor(sc, a)
            if node < 0:
                c["no_anchor"] = True
                continue
            c["fallback"] |= not (M.angle_gap(sc, a) < 0.25 * np.pi).any()
            lanes, grew = M.roi_lanes(sc, a, node, 20.0)
            n = sum(len(sc.lane_nodes[l]) for l in lanes)
            c["under_6"] |= n < 6
            c["no_pre0_suc0_edge"] |= n >= 6 and a not in valid
            if a in valid:
                t = int(sc.lane_idcs[node])
                c["closure_ascending"] |= bool(grew)
                c["not_ascending_no_neighbours"] |= (not grew) and max(lanes) > t > min(lanes) and \
                    bool((np.diff(np.concatenate([sc.lane_nodes[l] for l in lanes])) < 0).any())
    return c


def main():
    MG.import_reference()
    import data_lrcnn as ref
    import lanegcn_amd  # noqa: F401  (our own generator; the reference only consumes its output)
    import lane_roi_cases as C
    import lane_roi_model as M
    from golden_io import flatten

    for seed in range(100, 400):
        scenes = make_scenes(C, seed)
        if any(M.edge_agents(s) for s in scenes):
            continue
        once = [M.generate_lane_roi(copy.deepcopy(s)) for s in scenes]
        twice = [M.generate_lane_roi(copy.deepcopy(s), first_occurrence=False) for s in scenes]
        if any([g["num_nodes"] for g in x["subgraphs"]] != [g["num_nodes"] for g in y["subgraphs"]] for x, y in zip(once, twice)):
            continue                                           # a lane listed twice
        outs = [ref.generate_lane_roi(copy.deepcopy(s)) for s in scenes]
        found = cases(M, scenes, outs)
        print("seed %d: RoI sizes %s, cases %s" % (seed, [[g["num_nodes"] for g in o["subgraphs"]] for o in outs], found))
        if all(found.values()):
            break
    assert all(found.values()), found
    assert not any(M.edge_agents(s) for s in scenes)
    out = {"seed": np.int64(seed), "numpy_version": np.asarray(np.__version__)}
    flatten(scenes, "scenes/", out)
    for b, o in enumerate(outs):
        out["want/%d/valid_agent_ids" % b] = o["valid_agent_ids"]
        out["want/%d/n_rois" % b] = np.int64(len(o["subgraphs"]))
        flatten(o["subgraphs"], "want/%d/subgraphs/" % b, out)
    path = os.path.join(HERE, "lane_roi_b4.npz")
    np.savez_compressed(path, **out)
    assert os.path.getsize(path) < 1000000
    print("wrote lane_roi_b4.npz (%d bytes), seed %d, NumPy %s" % (os.path.getsize(path), seed, np.__version__))


if __name__ == "__main__":
    main()
