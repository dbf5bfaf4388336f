"""Net.forward of the fork model (lanegcn_amd.lanercnn.Net, reference lanercnn.py:85-119) on a synthetic batch with lane
RoIs (data.synth_scene + data.synth_subgraphs), with LanePooling.fused off -- the chain of generic launches -- and on --
the pair stage of every pooling as one lgcn_pool_pairs launch -- alternating call by call in one process after the warm-up.
Prints the medians, the kernel launches per forward of each path (torch.profiler; null where it is unavailable), the pair
count P of each of the three poolings, the same two timings for the largest pooling alone (Interactor.roi2graph on the
inputs it receives inside the forward, pair search included) and one JSON line.  Numbers for DESIGN.md; no bar.

  --scenes B --agents A --roads L,L,..   scenes per batch, agents (= RoIs at most) per scene, lanes per road (default
                                         10 x 12 on roads 6,6,6: 324 nodes per scene)
  --steps K --warmup W                   timed and untimed forwards per variant (default 30 / 5)
  --mma MODE                             matrix mode of everything but the fused pair stage (which is exact fp32)
  --train                                instead: forward + Loss + backward of Net on the same batch with
                                         LanePooling.train_hip off (the composed pair stage) and on (autograd.PoolPairsFn),
                                         alternating call by call in one process after the warm-up: median and minimum of
                                         --steps steps each (host clock around a step that ends in a synchronise), kernel
                                         launches of one step each (torch.profiler, after the timed steps), the peak of
                                         torch.cuda.max_memory_allocated over one step each, and the largest relative
                                         difference of the loss and of any parameter gradient between the two
  --others                               with --train: RowBlockFn.train_hip and Decode.train_hip on for both variants
  --raw                                  instead: raw tracks to predictions.  Net.forward_raw (resident store, flat RoIs) against
                                         the dict route (data_raw.build_scenes(batched=True) -> generate_lane_roi_batch(device=True)
                                         -> collate_fn -> Net.forward) on --scenes raw scenes of 21 tracks in the synthetic city of
                                         tests/scene_build_cases.py, alternating call by call in one process: --reps repetitions of
                                         the median of --steps calls, lowest - highest, and whether the outputs are equal
  --store                                instead: the resident RoI store (data_lrcnn.RoiStore) against the rebuild, on two
                                         workloads -- the --raw workload (--scenes raw scenes) and the batch of
                                         tools/bench_lane_roi.py (--roi-scenes synth_lane_scene scenes) -- alternating call by
                                         call in one process, --reps repetitions of the median of --steps calls, lowest - highest:
                                         (a) rois.batch(pick) against lane_roi_flat over the pick's scenes (the rebuild),
                                         (b) Net.forward_store against Net.forward_raw (raw workload only),
                                         (c) the lgcn_roi_store_gather launch alone between device events, behind a queued
                                         256 MB fill, with the bytes it reads and writes computed from the shapes and the
                                         resulting bytes/s next to the HBM peak (8.0 TB/s spec, 6.29 TB/s measured copy),
                                         and the resident bytes per scene (nbytes / S)"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import lanegcn_amd  # noqa: E402,F401
from bench_decode import count_launches  # noqa: E402
from lanegcn_amd import data as gen  # noqa: E402
from lanegcn_amd import lanercnn as R  # noqa: E402
from lanegcn_amd import ops  # noqa: E402


def make_batch(n_scenes, n_agents, roads, seed=0):
    rng = np.random.default_rng(seed)
    scenes = []
    while len(scenes) < n_scenes:
        s = gen.synth_subgraphs(gen.synth_scene(rng, roads, n_agents))
        if len(s["subgraphs"]) > 0:
            scenes.append(s)
    return gen.collate_fn(scenes)


def train_mode(args):
    from lanegcn_amd import autograd as A
    torch.manual_seed(0)
    net, loss_fn = R.Net(R.config).cuda().train(), R.Loss(R.config).cuda()
    data = make_batch(args.scenes, args.agents, [int(v) for v in args.roads.split(",")])
    n_rois = sum(len(s) for s in data["subgraphs"])
    A.RowBlockFn.train_hip = R.Decode.train_hip = bool(args.others)

    def step(on):
        R.LanePooling.train_hip = on
        try:
            net.zero_grad(set_to_none=True)
            loss = loss_fn(net(data), data)["loss"]
            loss.backward()
            return loss.detach()
        finally:
            R.LanePooling.train_hip = False

    pairs, real_pairs = [], R.build_pairs
    R.build_pairs = lambda *a, **k: pairs.append(real_pairs(*a, **k)) or pairs[-1]
    try:
        step(False)
    finally:
        R.build_pairs = real_pairs
    P = {name: ps.count() for name, ps in zip(("roi2graph", "graph2roi", "lane_pool"), pairs)}
    del pairs

    names = {"off": False, "on": True}
    times = {k: [] for k in names}
    for _ in range(args.warmup):
        for on in names.values():
            step(on)
    torch.cuda.synchronize()
    for _ in range(args.steps):
        for name, on in names.items():
            t0 = time.perf_counter()
            step(on)
            torch.cuda.synchronize()
            times[name].append((time.perf_counter() - t0) * 1e3)
    peak, grads, loss = {}, {}, {}
    for name, on in names.items():
        net.zero_grad(set_to_none=True)
        torch.cuda.synchronize()
        torch.cuda.empty_cache()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        loss[name] = float(step(on))
        torch.cuda.synchronize()
        peak[name] = {"max_allocated_mib": torch.cuda.max_memory_allocated() / 2 ** 20,
                      "above_resident_mib": (torch.cuda.max_memory_allocated() - base) / 2 ** 20}
        grads[name] = {k: p.grad.clone() for k, p in net.named_parameters()}
    diffs = {k: float((grads["on"][k] - g).abs().max() / g.abs().max().clamp_min(1e-30)) for k, g in grads["off"].items()}
    diff, worst = max(diffs.values()), sorted(diffs.items(), key=lambda kv: -kv[1])[:5]
    del grads
    launches = {name: count_launches(lambda on=on: step(on)) for name, on in names.items()}
    res = {"metric": "lanercnn.Net forward + Loss + backward, %d scenes, %d RoIs" % (args.scenes, n_rois),
           "mma": ops.get_mma(), "steps": args.steps, "other_train_hip_switches": bool(args.others), "pairs": P,
           "median_ms": {k: float(np.median(v)) for k, v in times.items()}, "min_ms": {k: min(v) for k, v in times.items()},
           "p10_p90_ms": {k: [float(np.percentile(v, 10)), float(np.percentile(v, 90))] for k, v in times.items()},
           "launches_per_step": launches, "peak_memory": peak, "loss": loss, "max_rel_grad_diff_on_off": diff,
           "largest_rel_grad_diffs": worst}
    print("P per pooling: %s" % P, flush=True)
    for name in names:
        print("Net step, LanePooling.train_hip %s: median %.3f ms (min %.3f), %s launches, peak %.1f MiB (%.1f above resident)"
              % (name, res["median_ms"][name], res["min_ms"][name], launches[name], peak[name]["max_allocated_mib"],
                 peak[name]["above_resident_mib"]), flush=True)
    print(json.dumps(res), flush=True)


def raw_mode(args):
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests"))
    import scene_build_cases as SC
    from lanegcn_amd import data_lrcnn as D
    from lanegcn_amd import data_raw
    torch.manual_seed(0)
    net = R.Net(R.config).cuda().eval()
    maps = SC.golden_inputs(500)[1]
    tables = {c: data_raw.LaneTable.from_lanes(m).to("cuda") for c, m in maps.items()}
    raws, seed = [], 0
    while len(raws) < args.scenes:      # scenes in which at least one agent keeps a lane RoI
        r = SC.extra_scene(seed)
        seed += 1
        if len(D.generate_lane_roi_batch(data_raw.build_scenes([r], tables, net.config, batched=True), device=True)[0]["subgraphs"]):
            raws.append(r)

    def run(flat):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        with torch.no_grad():
            if flat:
                out = net.forward_raw(raws, tables)[0]
            else:
                scenes = D.generate_lane_roi_batch(data_raw.build_scenes(raws, tables, net.config, batched=True), device=True)
                out = net(gen.collate_fn(scenes))
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3, out

    names = {"dict": False, "raw": True}
    for _ in range(args.warmup):
        for flat in names.values():
            run(flat)
    meds = {k: [] for k in names}
    for _ in range(args.reps):
        times = {k: [] for k in names}
        for _ in range(args.steps):
            for k, flat in names.items():
                times[k].append(run(flat)[0])
        for k in names:
            meds[k].append(float(np.median(times[k])))
    a, b = run(False)[1], run(True)[1]
    rb = net.forward_raw(raws, tables)[1]["subgraphs"]
    launches = {k: count_launches(lambda flat=flat: run(flat)) for k, flat in names.items()}
    res = {"metric": "raw tracks -> lanercnn.Net predictions, %d scenes, %d RoIs, %d RoI nodes" % (len(raws), rb.n_rois, int(rb.roi_base[-1])),
           "mma": ops.get_mma(), "steps": args.steps, "median_ms": meds,
           "lowest_highest_ms": {k: [min(v), max(v)] for k, v in meds.items()}, "launches_per_call": launches,
           "outputs_equal": bool(all(torch.equal(a[k], b[k]) for k in a))}
    print(json.dumps(res), flush=True)

HBM_PEAK_SPEC, HBM_PEAK_COPY = 8.0e12, 6.29e12          # bytes / s (MI355X: HBM3E spec, and a measured float4 copy)


def gather_bytes(plan, has_gt):
    """Bytes lgcn_roi_store_gather reads and writes for one pick, from the shapes: the table, the node rows (feats in and
    out, node_mask int32 -> int64), the RoI rows (agent_feat, ctrs, actor_feats, obs and with gt gt_preds, has_preds, in
    and out) and the index elements (int32 -> int64)."""
    row = 80 * 4 + 2 * 4 + 2 * 60 * 4 + ((60 * 4 + 30) if has_gt else 0)
    return plan.table.size * 8 + plan.n_nodes * (2 * 32 + 4 + 8) + plan.n_rois * 2 * row + plan.n_elem * (4 + 8)


def alternate(routes, steps, warmup, reps):
    """{name: [median ms of `steps` calls] * reps} of routes {name: fn}, alternating call by call; a call ends in a synchronise."""
    def run(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3
    for _ in range(warmup):
        for fn in routes.values():
            run(fn)
    meds = {k: [] for k in routes}
    for _ in range(reps):
        times = {k: [] for k in routes}
        for _ in range(steps):
            for k, fn in routes.items():
                times[k].append(run(fn))
        for k in routes:
            meds[k].append(float(np.median(times[k])))
    return meds


def bracket(meds, resident, rebuild):
    """Lowest - highest of every route, and the claim the brackets allow."""
    lh = {k: [min(v), max(v)] for k, v in meds.items()}
    claim = ("the resident route's bracket lies wholly below the rebuild's (%.1fx by the medians' medians)"
             % (float(np.median(meds[rebuild])) / float(np.median(meds[resident])))
             if lh[resident][1] < lh[rebuild][0] else "brackets overlap, no difference claimed")
    return {"median_ms": meds, "lowest_highest_ms": lh, "claim": claim}


def gather_launch(rois, pick, steps, warmup):
    """(c): the launch alone, us between device events, median of `steps`; behind a queued fill so that the launch is
    already in the queue when the device gets to it."""
    from lanegcn_amd import ops as O
    p = rois.plan(pick)
    dev, f32, i64 = rois.device, torch.float32, torch.int64
    T, Rn = p.n_nodes, p.n_rois
    stage = torch.from_numpy(p.table.copy())
    tab_dev = stage.to(dev)
    new = lambda shape, dt: torch.empty(shape, dtype=dt, device=dev)
    out = dict(feats=new((T, 8), f32), node_mask=new((T,), i64), agent_feat=new((Rn, 80), f32), idx=new((p.n_elem,), i64),
               ctrs=new((Rn, 2), f32), actor_feats=new((Rn, 20, 3), f32), obs=new((Rn, 20, 3), f32))
    if rois.has_gt:
        out.update(gt_preds=new((Rn, 30, 2), f32), has_preds=new((Rn, 30), torch.bool))
    ballast = torch.empty(64 * 2 ** 20, dtype=f32, device=dev)             # 256 MB
    us = []
    for i in range(warmup + steps):
        ballast.fill_(float(i))
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        O.roi_store_gather(rois._job, stage, tab_dev, p.n_scenes, T, Rn, p.n_elem, out)
        b.record()
        torch.cuda.synchronize()
        if i >= warmup:
            us.append(a.elapsed_time(b) * 1e3)
    nbytes, med = gather_bytes(p, rois.has_gt), float(np.median(us))
    return {"median_us": med, "min_us": min(us), "bytes_moved": nbytes, "bytes_per_s": nbytes / (med * 1e-6),
            "share_of_hbm_spec_peak": nbytes / (med * 1e-6) / HBM_PEAK_SPEC,
            "share_of_hbm_copy_peak": nbytes / (med * 1e-6) / HBM_PEAK_COPY}


def store_mode(args):
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests"))
    import scene_build_cases as SC
    from lanegcn_amd import data_lrcnn as D
    from lanegcn_amd import data_raw
    torch.manual_seed(0)
    net = R.Net(R.config).cuda().eval()
    res = {"mma": ops.get_mma(), "steps": args.steps, "reps": args.reps, "rocm": getattr(torch.version, "hip", None),
           "date": time.strftime("%Y-%m-%d")}

    # ---- the --raw workload: raw scenes in the synthetic city, each keeping at least one RoI
    maps = SC.golden_inputs(500)[1]
    tables = {c: data_raw.LaneTable.from_lanes(m).to("cuda") for c, m in maps.items()}
    raws, seed = [], 0
    while len(raws) < args.scenes:
        r = SC.extra_scene(seed)
        seed += 1
        if len(D.generate_lane_roi_batch(data_raw.build_scenes([r], tables, net.config, batched=True), device=True)[0]["subgraphs"]):
            raws.append(r)
    store = data_raw.build_store(raws, tables, net.config, lanes=True)
    rois = D.RoiStore.from_store(store)
    pick = np.arange(len(store))
    with torch.no_grad():
        a, b = net.forward_raw(raws, tables)[0], net.forward_store(store, rois, pick)[0]
        equal = bool(all(torch.equal(a[k], b[k]) for k in a))
        rb = rois.batch(pick)[0]
        w = {"metric": "resident RoI store against the rebuild, %d raw scenes, %d RoIs, %d RoI nodes" % (len(raws), rb.n_rois, int(rb.roi_base[-1])),
             "outputs_equal": equal, "resident_bytes": rois.nbytes, "resident_bytes_per_scene": rois.nbytes / len(rois),
             "scene_store_bytes_per_scene": store.nbytes / len(store)}
        w["roi_call"] = bracket(alternate({"rebuild": lambda: D.lane_roi_flat(*D.store_roi_inputs(store)),
                                           "resident": lambda: rois.batch(pick)}, args.steps, args.warmup, args.reps), "resident", "rebuild")
        w["forward"] = bracket(alternate({"forward_raw": lambda: net.forward_raw(raws, tables),
                                          "forward_store": lambda: net.forward_store(store, rois, pick)},
                                         args.steps, args.warmup, args.reps), "forward_store", "forward_raw")
        w["launches_per_call"] = {"forward_raw": count_launches(lambda: net.forward_raw(raws, tables)),
                                  "forward_store": count_launches(lambda: net.forward_store(store, rois, pick)),
                                  "rois.batch": count_launches(lambda: rois.batch(pick))}
    w["gather_launch"] = gather_launch(rois, pick, args.steps, args.warmup)
    res["raw_workload"] = w

    # ---- the batch of tools/bench_lane_roi.py: synth_lane_scene scenes of 1,728 nodes and 20 agents
    rng = np.random.default_rng(0)
    scenes = [gen.synth_lane_scene(rng, [6] * 16, 20) for _ in range(args.roi_scenes)]
    scenes = [s for s, d in zip(scenes, D.generate_lane_roi_batch([dict(s) for s in scenes], device=True)) if len(d["subgraphs"])]
    t, off, _ = D._roi_inputs(scenes)
    cat = lambda k, dt: torch.from_numpy(np.concatenate([np.asarray(s[k]).astype(dt, copy=False) for s in scenes])).cuda()
    rows = dict(ctrs=cat("ctrs", np.float32), feats=cat("feats", np.float32), obs_trajs=cat("obs_trajs", np.float32))
    if all("gt_preds" in s and "has_preds" in s for s in scenes):
        rows.update(gt_preds=cat("gt_preds", np.float32), has_preds=cat("has_preds", bool))
    rois2 = D.RoiStore.from_inputs(t, off, rows=rows)
    pick2 = np.arange(len(scenes))
    rb, want = rois2.batch(pick2)[0], D.lane_roi_flat(t, off)
    w = {"metric": "resident RoI store against the rebuild, %d scenes of %d nodes, %d RoIs, %d RoI nodes"
                   % (len(scenes), int(scenes[0]["graph"]["num_nodes"]), rb.n_rois, int(rb.roi_base[-1])),
         "outputs_equal": bool(all(torch.equal(getattr(rb, k), getattr(want, k)) for k in ("feats", "node_mask", "agent_feat", "u", "v", "a2m_u", "a2m_v"))),
         "resident_bytes": rois2.nbytes, "resident_bytes_per_scene": rois2.nbytes / len(rois2),
         # the rebuild from inputs that are already concatenated on the device (lane_roi_flat alone, the least the parent's
         # route does) and from the scene dicts (generate_lane_roi_flat, the call of tools/bench_lane_roi.py --flat)
         "roi_call": bracket(alternate({"rebuild": lambda: D.lane_roi_flat(t, off),
                                        "rebuild_from_dicts": lambda: D.generate_lane_roi_flat([dict(s) for s in scenes]),
                                        "resident": lambda: rois2.batch(pick2)}, args.steps, args.warmup, args.reps), "resident", "rebuild"),
         "gather_launch": gather_launch(rois2, pick2, args.steps, args.warmup)}
    res["roi_batch_workload"] = w
    print(json.dumps(res), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--raw", action="store_true")
    ap.add_argument("--store", action="store_true")
    ap.add_argument("--roi-scenes", type=int, default=32)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--scenes", type=int, default=10)
    ap.add_argument("--agents", type=int, default=12)
    ap.add_argument("--roads", default="6,6,6")
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--mma", default=None)
    ap.add_argument("--train", action="store_true")
    ap.add_argument("--others", action="store_true")
    args = ap.parse_args()
    if args.mma:
        ops.set_mma(args.mma)
    if args.train:
        return train_mode(args)
    if args.raw:
        return raw_mode(args)
    if args.store:
        return store_mode(args)
    torch.manual_seed(0)
    net = R.Net(R.config).cuda().eval()
    data = make_batch(args.scenes, args.agents, [int(v) for v in args.roads.split(",")])
    n_rois = sum(len(s) for s in data["subgraphs"])
    roi_nodes = sum(int(len(sg["feats"])) for s in data["subgraphs"] for sg in s)
    graph_nodes = sum(int(g["num_nodes"]) for g in data["graph"])

    def forward(on):
        R.LanePooling.fused = on
        try:
            with torch.no_grad():
                return net(data)
        finally:
            R.LanePooling.fused = False

    pairs, real_pairs, pool_args = [], R.build_pairs, []
    R.build_pairs = lambda *a, **k: pairs.append(real_pairs(*a, **k)) or pairs[-1]
    hook = net.interactor.roi2graph.register_forward_pre_hook(lambda m, a: pool_args.append(a))
    try:
        forward(False)
    finally:
        R.build_pairs = real_pairs
        hook.remove()
    P = {name: ps.count() for name, ps in zip(("roi2graph", "graph2roi", "lane_pool"), pairs)}

    def pooling(on):
        R.LanePooling.fused = on
        try:
            with torch.no_grad():
                return net.interactor.roi2graph(*pool_args[0])
        finally:
            R.LanePooling.fused = False

    names = {"off": False, "on": True}

    def timed(fn):
        times = {k: [] for k in names}
        for _ in range(args.warmup):
            for on in names.values():
                fn(on)
        torch.cuda.synchronize()
        for _ in range(args.steps):
            for name, on in names.items():
                t0 = time.perf_counter()
                fn(on)
                torch.cuda.synchronize()
                times[name].append((time.perf_counter() - t0) * 1e3)
        return times

    times, pool_times = timed(forward), timed(pooling)
    launches = {name: count_launches(lambda on=on: forward(on)) for name, on in names.items()}
    off, on = forward(False), forward(True)
    diff = {k: float((off[k] - on[k]).abs().max() / off[k].abs().max()) for k in off}
    pool_launches = {name: count_launches(lambda on=on: pooling(on)) for name, on in names.items()}
    res = {"metric": "lanercnn.Net.forward, %d scenes, %d RoIs, %d RoI nodes, %d graph nodes" % (args.scenes, n_rois, roi_nodes, graph_nodes),
           "mma": ops.get_mma(), "steps": args.steps, "pairs": P,
           "median_ms": {k: float(np.median(v)) for k, v in times.items()}, "min_ms": {k: min(v) for k, v in times.items()},
           "launches_per_forward": launches, "max_rel_diff_on_off": diff,
           "roi2graph_median_ms": {k: float(np.median(v)) for k, v in pool_times.items()},
           "roi2graph_min_ms": {k: min(v) for k, v in pool_times.items()}, "roi2graph_launches": pool_launches}
    print("P per pooling: %s" % P, flush=True)
    for name in names:
        print("Net.forward, LanePooling.fused %s: median %.3f ms (min %.3f), %s launches"
              % (name, res["median_ms"][name], res["min_ms"][name], launches[name]), flush=True)
        print("roi2graph alone (P = %d), fused %s: median %.3f ms (min %.3f), %s launches"
              % (P["roi2graph"], name, res["roi2graph_median_ms"][name], res["roi2graph_min_ms"][name], pool_launches[name]), flush=True)
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
