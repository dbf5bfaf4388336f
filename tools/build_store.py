"""Raw scenes to a resident store and a flat file, on the device: the job of the reference's preprocess_data.py.

    python tools/build_store.py --out split.npz [--rois rois.npz] [--raws raws.npz --tables tables.npz] [--batch 32] [--scenes 256]

Per batch of `--batch` raw scenes one data_raw.build_store, then ONE DeviceSceneStore.concat and ONE save: no scene dict
and no copy to the host before the save's one copy per array.  The file is what flatfile.write_scenes(..., theta=True)
writes for the same scenes; FlatSceneFile and DeviceSceneStore read it.

--rois OUT.npz also extracts the fork's lane RoIs: every batch is built with lanes=True and its data_lrcnn.RoiStore made
right after it, while the batch's lane arrays exist (they are never saved and do not survive the concat); ONE
RoiStore.concat and ONE save at the end.  data_lrcnn.RoiStore.load reads the file; scene i of it is scene i of --out.

Inputs are plain `.npz` files (the reader of the Argoverse CSVs and the map API stay out of scope):
  --raws    city [S] (strings), trk_off [S + 1] (tracks per scene, the agent first), row_off [T + 1] (rows per track),
            xy [rows,2] float64, step [rows] int64
  --tables  per city the arrays LaneTable's constructor takes, as "<city>/<name>": lane_id, pt_off, pts, turn, control,
            intersect, pred_off, pred, succ_off, succ, left, right
Without --raws the synthetic workload of tools/bench_scene_build.py is built: `--scenes` scenes of 40 tracks over one city
table of 13,200 lanes.  Prints one JSON line."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

TABLE_FIELDS = ("lane_id", "pt_off", "pts", "turn", "control", "intersect", "pred_off", "pred", "succ_off", "succ", "left", "right")


def synthetic(n_scenes, seed=0):
    """(raws, {city: LaneTable on the host}) of tools/bench_scene_build.py: the same city and, for seed 0, the same scenes."""
    import numpy as np
    import scene_build_cases as C
    from bench_scene_build import city
    from lanegcn_amd.data_raw import LaneTable
    rng = np.random.default_rng(seed)
    lanes, (wx, wy) = city()
    raws = []
    for _ in range(n_scenes):
        pose = C.Pose(rng.uniform(300, wx - 300), rng.uniform(300, wy - 300), rng.uniform(0, 2 * np.pi))
        raws.append(C.raw_scene("X", [pose.agent()] + [C.random_track(rng, pose) for _ in range(39)]))
    return raws, {"X": LaneTable.from_lanes(lanes)}


def read_inputs(raws_path, tables_path):
    import numpy as np
    from lanegcn_amd.data_raw import LaneTable
    with np.load(raws_path, allow_pickle=False) as z:
        city, trk_off, row_off, xy, step = z["city"], z["trk_off"], z["row_off"], z["xy"], z["step"]
    raws = []
    for s in range(len(city)):
        tracks = range(int(trk_off[s]), int(trk_off[s + 1]))
        raws.append({"city": str(city[s]), "trajs": [xy[row_off[t]:row_off[t + 1]] for t in tracks],
                     "steps": [step[row_off[t]:row_off[t + 1]] for t in tracks]})
    with np.load(tables_path, allow_pickle=False) as z:
        cities = sorted({k.split("/", 1)[0] for k in z.files})
        tables = {c: LaneTable(*[z["%s/%s" % (c, f)] for f in TABLE_FIELDS]) for c in cities}
    return raws, tables


def build(raws, tables, config, batch, rois=False):
    """-> (the store of all `raws`, its parts, the RoiStore of all `raws` or None): build_store per batch of `batch` scenes
    and, with rois, the batch's RoiStore while its lane arrays exist; one concat each."""
    from lanegcn_amd import data_raw as D
    from lanegcn_amd.data_lrcnn import RoiStore
    from lanegcn_amd.flatfile import DeviceSceneStore
    parts = [D.build_store(raws[i:i + batch], tables, config, lanes=rois) for i in range(0, len(raws), batch)]
    roi_store = RoiStore.concat([RoiStore.from_store(p) for p in parts]) if rois else None
    return DeviceSceneStore.concat(parts), parts, roi_store


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", required=True)
    ap.add_argument("--rois", help="also write the lane-RoI store of the same scenes (data_lrcnn.RoiStore) to this .npz")
    ap.add_argument("--raws")
    ap.add_argument("--tables")
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--scenes", type=int, default=256, help="synthetic scenes, without --raws")
    ap.add_argument("--num-scales", type=int, default=6)
    ap.add_argument("--pred-range", type=float, nargs=4, default=[-100.0, 100.0, -100.0, 100.0])
    ap.add_argument("--cross-dist", type=float, default=6.0)
    args = ap.parse_args()
    if (args.raws is None) != (args.tables is None):
        ap.error("--raws and --tables come together")
    if args.batch < 1:
        ap.error("--batch must be positive")
    import torch
    import lanegcn_amd  # noqa: F401
    if not torch.cuda.is_available():
        raise SystemExit("build_store.py builds on the GPU; none found")
    raws, tables = synthetic(args.scenes) if args.raws is None else read_inputs(args.raws, args.tables)
    tables = {k: v.to("cuda") for k, v in tables.items()}
    config = {"pred_range": args.pred_range, "num_scales": args.num_scales, "cross_dist": args.cross_dist}
    t0 = time.perf_counter()
    store, parts, rois = build(raws, tables, config, args.batch, rois=args.rois is not None)
    torch.cuda.synchronize()
    t1 = time.perf_counter()
    store.save(args.out)
    extra = {}
    if rois is not None:
        rois.save(args.rois)
        extra = {"rois_out": args.rois if args.rois.endswith(".npz") else args.rois + ".npz", "rois": rois.n_rois,
                 "roi_nodes": int(rois.node_off[-1]), "usable_scenes": int(len(rois.usable())),
                 "roi_store_mb": round(rois.nbytes / 1e6, 2)}
    t2 = time.perf_counter()
    print(json.dumps({**extra, "out": args.out if args.out.endswith(".npz") else args.out + ".npz", "scenes": len(store), "parts": len(parts),
                      "nodes": int(store.node_off[-1]), "actors": int(store.actor_off[-1]), "edges": int(store.rel_off[-1]),
                      "store_mb": round(store.nbytes / 1e6, 2), "build_ms": round((t1 - t0) * 1e3, 1),
                      "save_ms": round((t2 - t1) * 1e3, 1)}))


if __name__ == "__main__":
    main()
