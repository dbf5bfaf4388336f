"""Scene construction for a batch: data_raw.build_scenes on the device against the host model (tests/scene_build_model.py,
the stand-in for the reference where the reference is absent).

    python tools/bench_scene_build.py [--scenes 32] [--runs 30] [--model-scenes 2]

Argoverse-like sizes: one city table of 13,200 lane segments of 10 points each (Miami has about 12.6 k, Pittsburgh 9.6 k),
15 m long on a 15 m x 15 m grid, about 200 of which (1,800 nodes) overlap a scene's 200 m x 200 m rectangle; 32 raw scenes of
40 tracks with up to 50 rows each.  Prints one JSON line: the median of `runs` synchronised calls (ms per batch) of
  scale0_ms          tracks + lanes kernels, both read-backs, the scene dicts (num_scales = 1, cross=False)
  dilated_ms         ... plus the per-scene dilated_nbrs for scales 1..5 (cross=False)
  full_ms            ... plus the per-scene preprocess for left / right (the default call)
  full_prefiltered_ms  the default call with explicit lane_ids: the lanes within the reference's query radius, found on
                     the host outside the timed region (the map query itself is out of scope)
  dilated_batched_ms, full_batched_ms  dilated_ms and full_ms with batched=True: the scales and left / right from
                     ops.dilate_batch and ops.cross_edges_batch on the whole batch (same raws, same process); the tool
                     asserts that every pre / suc / left / right leaf of full_batched equals full's
and the host model's scale-0 time per scene (median over --model-scenes scenes)."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

# lgcn_scene_tracks: 2 kernels; lgcn_scene_lanes_rank: 1 memset + 2 kernels; lgcn_scene_lanes_fill: 2 kernels; one zero
# fill (the head buffer)
DEVICE_OPS = {"kernels": 6, "memsets": 1, "fills": 1, "size_readbacks": 2}
# batched=True adds, whatever the number of scenes: lgcn_dilate_batch_csr: 1 kernel + lgcn_csr_build's 5 to 6; per scale
# lgcn_dilate_batch_count: 2, lgcn_dilate_batch_fill: 1 and one read-back; lgcn_cross_edges_batch: 1 memset + 4 kernels and
# one read-back (num_scales = 6: 25 to 26 kernels, 1 memset, 6 read-backs, besides torch's allocations and table uploads)
BATCHED_TAIL_OPS = {"kernels": 26, "memsets": 1, "size_readbacks": 6}


def city(n_x=120, n_y=110, cell=15.0, n_pts=10):
    import numpy as np
    import scene_build_cases as C
    lanes = {}
    lid = lambda i, j: j * n_x + i
    t = np.linspace(0.0, 1.0, n_pts)[:, None]
    for j in range(n_y):
        for i in range(n_x):
            a = np.array([i * cell, j * cell + 0.3 * np.sin(i)])
            b = np.array([(i + 1) * cell, j * cell + 0.3 * np.sin(i + 1)])
            lanes[lid(i, j)] = C.Lane(a + t * (b - a), turn=("NONE", "LEFT", "RIGHT")[(i + j) % 3], control=i % 4 == 0,
                                      intersect=j % 5 == 0, pred=[lid(i - 1, j)] if i else [], succ=[lid(i + 1, j)] if i + 1 < n_x else [],
                                      left=lid(i, j + 1) if j + 1 < n_y and j % 2 == 0 else None,
                                      right=lid(i, j - 1) if j % 2 == 1 else None)
    return lanes, (n_x * cell, n_y * cell)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scenes", type=int, default=32)
    ap.add_argument("--runs", type=int, default=30)
    ap.add_argument("--model-scenes", type=int, default=2)
    args = ap.parse_args()
    import numpy as np
    import torch
    import lanegcn_amd  # noqa: F401
    from lanegcn_amd import data_raw as D
    import scene_build_cases as C
    import scene_build_model as M

    rng = np.random.default_rng(0)
    lanes, (wx, wy) = city()
    table = D.LaneTable.from_lanes(lanes)
    tables = {"X": table.to("cuda")}
    raws = []
    for _ in range(args.scenes):
        pose = C.Pose(rng.uniform(300, wx - 300), rng.uniform(300, wy - 300), rng.uniform(0, 2 * np.pi))
        raws.append(C.raw_scene("X", [pose.agent()] + [C.random_track(rng, pose) for _ in range(39)]))
    # the reference's candidate query: lanes with a point within radius = 200 m of the agent
    orig = np.stack([r["trajs"][0][19] for r in raws])
    lo = np.minimum.reduceat(table.pts, table.pt_off[:-1], 0)
    hi = np.maximum.reduceat(table.pts, table.pt_off[:-1], 0)
    near = [np.flatnonzero(((lo <= o + 200.0) & (hi >= o - 200.0)).all(1)) for o in orig]
    lane_ids = [table.lane_id[n].tolist() for n in near]
    cfg = dict(C.CONFIG)
    out = {"scenes": args.scenes, "table_lanes": table.n_lanes, "table_points": table.n_pts, "tracks_per_scene": 40,
           "candidates_prefiltered_per_scene": int(np.mean([len(n) for n in near])), "device_ops_per_batch": DEVICE_OPS,
           "batched_tail_ops_per_batch": BATCHED_TAIL_OPS}

    scenes, kept = None, {}
    for name, kw in (("scale0_ms", dict(config=dict(cfg, num_scales=1), cross=False)), ("dilated_ms", dict(cross=False)),
                     ("full_ms", dict()), ("full_prefiltered_ms", dict(lane_ids=lane_ids)),
                     ("dilated_batched_ms", dict(cross=False, batched=True)), ("full_batched_ms", dict(batched=True))):
        times = []
        for _ in range(args.runs + 3):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            scenes = D.build_scenes(raws, tables, **dict(dict(config=cfg), **kw))
            torch.cuda.synchronize()
            times.append((time.perf_counter() - t0) * 1e3)
        out[name] = round(statistics.median(times[3:]), 3)
        kept[name] = scenes
    # faster and different is not faster: at the timed size, every graph leaf of the batched call equals the per-scene call's
    for a, b in zip(kept["full_batched_ms"], kept["full_ms"]):
        for k in ("pre", "suc"):
            assert len(a["graph"][k]) == len(b["graph"][k])
            for x, y in zip(a["graph"][k], b["graph"][k]):
                assert torch.equal(x["u"], y["u"]) and torch.equal(x["v"], y["v"]), k
        for k in ("left", "right"):
            for c in "uv":
                assert a["graph"][k][c].dtype == b["graph"][k][c].dtype and torch.equal(a["graph"][k][c], b["graph"][k][c]), k
    out["batched_equals_per_scene"] = True
    out["nodes_per_scene"] = int(np.mean([s["graph"]["num_nodes"] for s in scenes]))
    out["actors_per_scene"] = int(np.mean([len(s["ctrs"]) for s in scenes]))
    times = []
    for r in raws[:args.model_scenes]:
        t0 = time.perf_counter()
        s = M.obj_feats(r, cfg["pred_range"])
        M.lane_graph(s["orig"], s["rot"], table, cfg["pred_range"])
        times.append((time.perf_counter() - t0) * 1e3)
    out["host_model_scale0_ms_per_scene"] = round(statistics.median(times), 3)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
