"""Generates tests/golden/scene_build_b4.npz by running the REFERENCE's own ArgoDataset.get_obj_feats (data.py:148-217) and
ArgoDataset.get_lane_graph (data.py:220-361), imported read-only through make_golden.import_reference()'s stubs, on the
four raw scenes of tests/scene_build_cases.golden_inputs.  Run in the build container only:
    python tests/golden/make_golden_scene_build.py
The dataset object is made with __new__ and given config, train=False and a stand-in map object of our own (the three
members get_lane_graph touches).  The fixture holds the raw scenes, the lane tables and the reference's outputs as data,
never reference source, and the NumPy version it ran under.

The script ASSERTS that the four scenes hold every case of scene_build_cases.CASES, that no keep / drop decision lies
within 1e-3 m of a pred_range bound and that every agent's heading vector is non-zero.  It also prints the reference's
time per scene on this machine (DESIGN.md section 5b quotes it)."""
import copy
import os
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden as MG  # noqa: E402
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

TABLE_KEYS = ("lane_id", "pt_off", "pts", "turn", "control", "intersect", "pred_off", "pred", "succ_off", "succ", "left", "right")


class StandInMap:
    """What get_lane_graph asks of ArgoverseMap: the lane dict, a candidate query (table order, or the list set for the
    scene) and a lane polygon (unused by anything recorded)."""

    def __init__(self, maps):
        self.city_lane_centerlines_dict = maps
        self.order = None

    def get_lane_ids_in_xy_bbox(self, x, y, city, radius):
        return list(self.order) if self.order is not None else list(self.city_lane_centerlines_dict[city].keys())

    def get_lane_segment_polygon(self, lane_id, city):
        c = self.city_lane_centerlines_dict[city][lane_id].centerline
        return np.concatenate([np.concatenate([c, c[::-1]], 0), np.zeros((2 * len(c), 1))], 1)


def main():
    _, refdata = MG.import_reference()
    import lanegcn_amd  # noqa: F401
    from lanegcn_amd.data_raw import LaneTable
    import scene_build_cases as C
    from golden_io import flatten

    for seed in range(500, 560):
        raws, maps, lane_ids, _ = C.golden_inputs(seed)
        tables = {k: LaneTable.from_lanes(v) for k, v in maps.items()}
        found, margin = C.found_cases(raws, tables, lane_ids)
        print("seed %d: margin %.2e m, missing %s" % (seed, margin, [k for k, v in found.items() if not v]))
        if all(found.values()) and margin >= 1e-3:
            break
    assert all(found.values()), found
    assert margin >= 1e-3, margin
    for r in raws:
        assert np.abs(r["trajs"][0][18] - r["trajs"][0][19].astype(np.float32)).max() > 0

    ds = refdata.ArgoDataset.__new__(refdata.ArgoDataset)
    ds.config = dict(C.CONFIG, rot_aug=False)
    ds.train = False
    ds.am = StandInMap(maps)
    outs, t_obj, t_graph = [], [], []
    for raw, ids in zip(raws, lane_ids):
        ds.am.order = ids
        t0 = time.perf_counter()
        data = ds.get_obj_feats(copy.deepcopy(raw))
        t1 = time.perf_counter()
        data["graph"] = ds.get_lane_graph(data)
        t2 = time.perf_counter()
        t_obj.append(t1 - t0)
        t_graph.append(t2 - t1)
        outs.append({k: data[k] for k in ("feats", "obs_trajs", "ctrs", "orig", "theta", "rot", "gt_preds", "has_preds", "graph")})
        print("scene: %d tracks -> %d kept, %d lanes, %d nodes; reference get_obj_feats %.2f ms, get_lane_graph %.2f ms" % (
            len(raw["trajs"]), len(data["ctrs"]), int(data["graph"]["lane_idcs"][-1]) + 1, data["graph"]["num_nodes"],
            1e3 * t_obj[-1], 1e3 * t_graph[-1]))
    out = {"seed": np.int64(seed), "numpy_version": np.asarray(np.__version__)}
    flatten(raws, "raws/", out)
    for city, tb in tables.items():
        for k in TABLE_KEYS:
            out["tables/%s/%s" % (city, k)] = getattr(tb, k)
    for b, ids in enumerate(lane_ids):
        if ids is not None:
            out["lane_ids/%d" % b] = np.asarray(ids, np.int64)
    flatten(outs, "want/", out)
    path = os.path.join(HERE, "scene_build_b4.npz")
    np.savez_compressed(path, **out)
    assert os.path.getsize(path) < 1000000, os.path.getsize(path)
    print("wrote scene_build_b4.npz (%d bytes), seed %d, NumPy %s; reference per scene: get_obj_feats %.2f ms, "
          "get_lane_graph %.2f ms (mean of the four scenes, one run)" % (
              os.path.getsize(path), seed, np.__version__, 1e3 * np.mean(t_obj), 1e3 * np.mean(t_graph)))


if __name__ == "__main__":
    main()
