"""A fresh batch per step: flatfile.DeviceSceneStore.batch (one table upload + one launch out of a device-resident
store) against flatfile.FlatSceneFile.batch (host slicing + one upload per array).

    python tools/bench_store.py [--scenes 256] [--batch 32] [--rounds 30] [--warmup 5] [--reps 3] [--ragged] [--replay]

A store of `scenes` synthetic scenes of S2's per-scene size (324 nodes, 50 actors), random picks of `batch`.  One
process measures, the two paths alternating on the same picks, `reps` times over:
  (a) host_ms           FlatSceneFile.batch(pick) until its arrays are on the device (ends with a synchronise)
  (b) store_ms          DeviceSceneStore.batch(pick), the same
  (c) store_enqueue_ms  host time of (b) alone, no synchronise inside the timed region
  (d) scenes_per_s      FullNetEngine.forward with a fresh pick every step, through (a) and through (b): `rounds` steps
                        per window, one synchronise at the end of the window
Every figure is the median over `rounds` after `warmup`; per figure the JSON line carries the median of the `reps`
medians and their lowest and highest value (the spread between repetitions).  The GPU time of the gather launch
itself is not measured here: it is k_store_gather in a kernel trace of this tool.
--ragged: the scenes' sizes differ (2..4 roads, 20..80 actors drawn per scene: 216..432 nodes), as a real split's do.
--replay: also (e) scenes_per_s_checked, Net.forward_store_flat on a fresh pick every step (the eager route WITH its one
host read per batch), and (f) scenes_per_s_replay, engine.StoreReplay.forward on the same kind of picks (padded to
StoreCaps.for_size, one captured graph, the same host read) -- (e) of the same run is (f)'s baseline.  With them the
line carries replay_stats (routes taken, mean pad shares), replay_host_ms (host time per batch up to the host read) and
graph_pool_mb (memory the capture reserved)."""
import argparse
import json
import os
import statistics
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scenes", type=int, default=256)
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--rounds", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--ragged", action="store_true")
    ap.add_argument("--replay", action="store_true")
    args = ap.parse_args()
    import numpy as np
    import torch
    import lanegcn_amd  # noqa: F401
    from lanegcn_amd import data as gen
    from lanegcn_amd import lanegcn as M
    from lanegcn_amd.engine import FullNetEngine
    from lanegcn_amd.flatfile import DeviceSceneStore, FlatSceneFile, write_scenes

    if not torch.cuda.is_available():
        raise SystemExit("bench_store.py measures on the GPU; none found")
    with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, "split.npz")
        if args.ragged:
            srng = np.random.default_rng(0)
            scenes = [gen.synth_scene(srng, [6] * int(srng.integers(2, 5)), int(srng.integers(20, 81))) for _ in range(args.scenes)]
        else:
            scenes = gen.synth_batch("S2", seed=0, n_scenes=args.scenes)
        write_scenes(path, scenes)
        host = FlatSceneFile(path)
    dev = DeviceSceneStore(host)
    torch.manual_seed(0)
    net = M.Net(M.config).cuda().eval()
    eng = FullNetEngine(net)
    rng = np.random.default_rng(1)
    draw = lambda: [int(i) for i in rng.integers(0, args.scenes, args.batch)]
    sync = torch.cuda.synchronize
    paths = {"host": lambda p: host.batch(p), "store": lambda p: dev.batch(p)}
    replay = None
    if args.replay:
        from lanegcn_amd.engine import StoreReplay
        from lanegcn_amd.flatfile import StoreCaps
        replay = StoreReplay(net, dev, StoreCaps.for_size(dev, args.batch))
        routes = {"checked": lambda p: net.forward_store_flat(dev, p), "replay": lambda p: replay.forward(p)}

    def batch_times():
        """-> medians (ms) of host, store, store enqueue over `rounds` picks; each pick goes through both paths."""
        t = {"host": [], "store": [], "enqueue": []}
        for i in range(args.warmup + args.rounds):
            pick = draw()
            for name in (("host", "store") if i % 2 else ("store", "host")):
                sync()
                t0 = time.perf_counter()
                out = paths[name](pick)
                t1 = time.perf_counter()
                sync()
                t2 = time.perf_counter()
                del out
                if i >= args.warmup:
                    t[name].append((t2 - t0) * 1e3)
                    if name == "store":
                        t["enqueue"].append((t1 - t0) * 1e3)
        return {k: statistics.median(v) for k, v in t.items()}

    def forward_rate(name):
        """scenes/s of `rounds` forwards, each on a fresh pick through path `name`."""
        with torch.no_grad():
            for i in range(args.warmup + args.rounds):
                if i == args.warmup:
                    sync()
                    t0 = time.perf_counter()
                fb, ex = paths[name](draw())
                eng.forward(fb, ex["actor_feats"], ex["rot"], ex["orig"], ex["sizes"])
            sync()
        return args.rounds * args.batch / (time.perf_counter() - t0)

    def routed_rate(name):
        """scenes/s of `rounds` whole forwards behind their host read, each on a fresh pick through route `name`."""
        for i in range(args.warmup + args.rounds):
            if i == args.warmup:
                sync()
                t0 = time.perf_counter()
            routes[name](draw())
        sync()
        return args.rounds * args.batch / (time.perf_counter() - t0)

    reps = {"host_ms": [], "store_ms": [], "store_enqueue_ms": [], "scenes_per_s_host": [], "scenes_per_s_store": []}
    for r in range(args.reps):
        t = batch_times()
        reps["host_ms"].append(t["host"])
        reps["store_ms"].append(t["store"])
        reps["store_enqueue_ms"].append(t["enqueue"])
        for name in (("host", "store") if r % 2 else ("store", "host")):
            reps["scenes_per_s_" + name].append(forward_rate(name))
        if replay is not None:
            for name in (("checked", "replay") if r % 2 else ("replay", "checked")):
                reps.setdefault("scenes_per_s_" + name, []).append(routed_rate(name))
    fb, _ = dev.batch(draw())
    out = {"scenes": args.scenes, "batch": args.batch, "rounds": args.rounds, "warmup": args.warmup, "reps": args.reps,
           "store_mb": round(dev.nbytes / 1e6, 2), "batch_nodes": fb.n_nodes, "batch_index_elems": int(fb.idx_local.numel()),
           "batch_kb": round(fb.buf_view().numel() / 1e3, 1), "ragged": args.ragged}
    if replay is not None:
        out.update(replay_stats={k: (round(v, 4) if isinstance(v, float) else v) for k, v in replay.stats.items()},
                   graph_pool_mb=round(replay.graph_pool_bytes() / 1e6, 2),
                   caps={"nodes": replay.caps.nodes, "actors": replay.caps.actors, "edges": sum(replay.caps.edges)})
    for k, v in reps.items():
        digits = 1 if k.startswith("scenes") else 4
        out[k] = {"median": round(statistics.median(v), digits), "min": round(min(v), digits), "max": round(max(v), digits)}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
