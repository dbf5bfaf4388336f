"""Lane-RoI extraction for a batch: data_lrcnn.generate_lane_roi_batch on the device against the host model
(tests/lane_roi_model.py, the stand-in for the reference where the reference is absent).

    python tools/bench_lane_roi.py [--scenes 32] [--runs 30] [--model-scenes 4] [--flat [--reps 3]]

32 synth_lane_scene scenes of 1,728 nodes and 20 agents.  Prints one JSON line: the median of `runs` calls with
device=True and with device=False (ms per batch, synchronised), the host model (ms per scene, median over
--model-scenes scenes), and the number of device operations per batch, which does not depend on the batch.  The
reference's own generate_lane_roi took 24 ms per scene of this size on one CPU core (NumPy 2.2.6).

--flat instead times the flat route (data_lrcnn.generate_lane_roi_flat -> RoiBatch) against the list route
(generate_lane_roi_batch(device=True)) on the same batch, alternating call by call in one process: the RoI call alone
and the RoI call followed by lanercnn.subgraph_gather, which is where the list route concatenates its R x 30 pieces
again.  --reps repetitions of the median of --runs calls each; the JSON line holds every median and lowest - highest."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

# lgcn_roi_search: 1 memset + 8 kernels (7 where one scan tile holds every row count: not at these sizes); lgcn_roi_nodes,
# lgcn_roi_edge_count, lgcn_roi_edge_fill: 1 kernel each; two zero fills (the status / count buffer, a2m.u)
DEVICE_OPS = {"kernels": 11, "memsets": 1, "fills": 2, "size_readbacks": 2}


# the flat route: lgcn_roi_edge_fill_graph in the place of lgcn_roi_edge_fill, no zero fill of a2m.u
FLAT_DEVICE_OPS = {"kernels": 11, "memsets": 1, "fills": 1, "size_readbacks": 2}


def flat_mode(args, scenes, out):
    import torch
    from lanegcn_amd import data_lrcnn as D
    from lanegcn_amd import lanercnn as R

    # subgraph_gather (both routes) takes no scene without an RoI
    scenes = [s for s, d in zip(scenes, D.generate_lane_roi_batch([dict(s) for s in scenes], device=True)) if len(d["subgraphs"])]
    out["scenes"] = len(scenes)

    def run(flat, gather):
        batch = [dict(s) for s in scenes]
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        if flat:
            subs = D.generate_lane_roi_flat(batch)
        else:
            subs = [s["subgraphs"] for s in D.generate_lane_roi_batch(batch, device=True)]
        if gather:
            R.subgraph_gather(subs)
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3, subs

    kinds = [(name + ("_gather" if g else ""), f, g) for g in (False, True) for name, f in (("list", False), ("flat", True))]
    for _ in range(3):
        for _, f, g in kinds:
            run(f, g)
    meds = {k: [] for k, _, _ in kinds}
    for _ in range(args.reps):
        times = {k: [] for k, _, _ in kinds}
        for _ in range(args.runs):
            for k, f, g in kinds:            # alternating call by call
                times[k].append(run(f, g)[0])
        for k in times:
            meds[k].append(round(statistics.median(times[k]), 3))
    out["rois_per_batch"] = run(True, False)[1].n_rois
    out["device_ops_per_batch"] = {"list": DEVICE_OPS, "flat": FLAT_DEVICE_OPS}
    out["median_ms_per_batch"] = meds
    out["lowest_highest_ms"] = {k: [min(v), max(v)] for k, v in meds.items()}
    print(json.dumps(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--flat", action="store_true")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--scenes", type=int, default=32)
    ap.add_argument("--runs", type=int, default=30)
    ap.add_argument("--model-scenes", type=int, default=4)
    args = ap.parse_args()
    import numpy as np
    import torch
    import lanegcn_amd  # noqa: F401
    from lanegcn_amd import data as gen
    from lanegcn_amd import data_lrcnn as D
    import lane_roi_model as M

    rng = np.random.default_rng(0)
    scenes = [gen.synth_lane_scene(rng, [6] * 16, 20) for _ in range(args.scenes)]
    out = {"scenes": args.scenes, "nodes_per_scene": int(scenes[0]["graph"]["num_nodes"]), "agents_per_scene": 20,
           "device_ops_per_batch": DEVICE_OPS, "reference_ms_per_scene_cpu": 24.0}
    if args.flat:
        return flat_mode(args, scenes, out)
    for name, device in (("device_true_ms_per_batch", True), ("device_false_ms_per_batch", False)):
        times = []
        for _ in range(args.runs + 3):
            batch = [dict(s) for s in scenes]
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            D.generate_lane_roi_batch(batch, device=device)
            torch.cuda.synchronize()
            times.append((time.perf_counter() - t0) * 1e3)
        out[name] = round(statistics.median(times[3:]), 3)
    out["rois_per_batch"] = sum(len(s["subgraphs"]) for s in batch)
    times = []
    for s in scenes[:args.model_scenes]:
        t0 = time.perf_counter()
        M.generate_lane_roi(dict(s))
        times.append((time.perf_counter() - t0) * 1e3)
    out["host_model_ms_per_scene"] = round(statistics.median(times), 3)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
