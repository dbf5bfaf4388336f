"""Raw scenes to a resident store on the device (data_raw.build_store, DeviceSceneStore.concat, Net.forward_raw) against
the routes that existed before, side by side in one process.

    python tools/bench_build_store.py [--scenes 32] [--rounds 30] [--warmup 3] [--reps 3] [--parts 64]

The workload of tools/bench_scene_build.py (32 raw scenes of 40 tracks, one city table of 13,200 lanes) and the protocol of
tools/bench_store.py: every figure is the median of `rounds` synchronised calls after `warmup`, the routes of a pair
alternating call by call; `reps` repetitions; the JSON line carries the median of the repetitions' medians and their
lowest and highest value.
  (a) scenes_ms        build_scenes(batched=True): scene dicts with device leaves        } per batch
  (b) store_ms         build_store: a DeviceSceneStore                                    }
  (c) forward_dicts_ms Net.forward(collate_fn(build_scenes(batched=True))): raw -> outputs as before
  (d) forward_raw_ms   Net.forward_raw: raw -> outputs through the store
  (e) split_file_ms    a split of `parts` batches made resident through the file: per batch build_scenes(device=False,
                       batched=True), then write_scenes and DeviceSceneStore(path)
  (f) split_store_ms   the same split: `parts` x build_store, one concat
      (e) and (f) run ONCE per repetition (one (e) is `parts` batches and a file of the whole split), so their figure
      is the median of `reps` single runs; both use the same batch `parts` times
  pack_batch_us, pack_concat_us   the lgcn_store_pack launch alone between device events, behind a queued 256 MB fill (so
                       that the launch is queued before the GPU reaches it): one batch's 28 runs, the concat's parts x 28
The tool asserts that (b)'s store holds (a)'s node rows, futures and edge counts, that (c) and (d) return the same bits
and that (e) and (f) hold the same arrays."""
import argparse
import json
import os
import statistics
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scenes", type=int, default=32)
    ap.add_argument("--rounds", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--parts", type=int, default=64)
    args = ap.parse_args()
    import numpy as np
    import torch
    import lanegcn_amd  # noqa: F401
    from build_store import synthetic
    from lanegcn_amd import data as gen, data_raw as D, lanegcn as M, ops
    from lanegcn_amd.flatfile import DeviceSceneStore, write_scenes
    import scene_build_cases as C

    if not torch.cuda.is_available():
        raise SystemExit("bench_build_store.py measures on the GPU; none found")
    raws, tables = synthetic(args.scenes)
    tables = {k: v.to("cuda") for k, v in tables.items()}
    torch.manual_seed(0)
    net = M.Net(dict(M.config, **C.CONFIG)).cuda().eval()
    cfg = net.config
    keys = ("feats", "ctrs", "orig", "theta", "rot", "gt_preds", "has_preds", "graph")
    sync = torch.cuda.synchronize

    def forward_dicts():
        scenes = D.build_scenes(raws, tables, cfg, batched=True)
        return net(gen.collate_fn([{k: s[k] for k in keys} for s in scenes]))

    def split_file(tmp):
        path = os.path.join(tmp, "split.npz")
        scenes = []
        for _ in range(args.parts):
            scenes += D.build_scenes(raws, tables, cfg, device=False, batched=True)
        write_scenes(path, scenes, theta=True)
        return DeviceSceneStore(path)

    def split_store():
        return DeviceSceneStore.concat([D.build_store(raws, tables, cfg) for _ in range(args.parts)])

    routes = {"scenes_ms": lambda: D.build_scenes(raws, tables, cfg, batched=True), "store_ms": lambda: D.build_store(raws, tables, cfg),
              "forward_dicts_ms": forward_dicts, "forward_raw_ms": lambda: net.forward_raw(raws, tables)}

    def pair(x, y):
        """-> medians (ms) of routes x and y over `rounds` calls each, alternating."""
        t = {x: [], y: []}
        with torch.no_grad():
            for i in range(args.warmup + args.rounds):
                for name in ((x, y) if i % 2 else (y, x)):
                    sync()
                    t0 = time.perf_counter()
                    out = routes[name]()
                    sync()
                    t1 = time.perf_counter()
                    del out
                    if i >= args.warmup:
                        t[name].append((t1 - t0) * 1e3)
        return {k: statistics.median(v) for k, v in t.items()}

    def once(fn, *a):
        sync()
        t0 = time.perf_counter()
        out = fn(*a)
        sync()
        return (time.perf_counter() - t0) * 1e3, out

    def pack_us(job, big):
        """The launch of `job` between device events, queued behind a fill of `big`."""
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t = []
        for i in range(args.warmup + args.rounds):
            sync()
            big.fill_(float(i))
            e0.record()
            ops.store_pack_launch(job)
            e1.record()
            sync()
            if i >= args.warmup:
                t.append(e0.elapsed_time(e1) * 1e3)
        return statistics.median(t)

    # the jobs of the two pack launches, taken from one build_store and one concat as they make them
    jobs = []
    real = ops.StorePackJob

    class Keep(real):
        def __init__(self, *a, **k):
            real.__init__(self, *a, **k)
            jobs.append(self)
    ops.StorePackJob = Keep
    part = D.build_store(raws, tables, cfg)
    whole = DeviceSceneStore.concat([part] * args.parts)
    ops.StorePackJob = real
    sync()
    assert len(jobs) == 2 and jobs[0].p.n_seg == 28 and jobs[1].p.n_seg == 28 * args.parts

    # the same data on both sides of every pair
    scenes = D.build_scenes(raws, tables, cfg, batched=True)
    fb, ex = part.batch(np.arange(len(part)))
    assert torch.equal(fb.node_ctrs, torch.cat([s["graph"]["ctrs"] for s in scenes]))
    assert torch.equal(ex["gt_preds"], torch.cat([s["gt_preds"] for s in scenes]))
    assert fb.n_edges == [sum(len(e["u"]) for e in rel) for rel in
                          zip(*[[x for i in range(6) for x in (s["graph"]["pre"][i], s["graph"]["suc"][i])] +
                                [s["graph"]["left"], s["graph"]["right"]] for s in scenes])]
    with torch.no_grad():
        o1, o2 = forward_dicts(), net.forward_raw(raws, tables)
    assert all(torch.equal(a, b) for k in ("cls", "reg") for a, b in zip(o1[k], o2[k]))
    del scenes, fb, ex, o1, o2

    reps = {k: [] for k in ("scenes_ms", "store_ms", "forward_dicts_ms", "forward_raw_ms", "split_file_ms", "split_store_ms",
                            "pack_batch_us", "pack_concat_us")}
    big = torch.empty(64 << 20, dtype=torch.float32, device="cuda")
    for r in range(args.reps):
        for x, y in (("scenes_ms", "store_ms"), ("forward_dicts_ms", "forward_raw_ms")):
            for k, v in pair(x, y).items():
                reps[k].append(v)
        with tempfile.TemporaryDirectory() as tmp:
            order = ("file", "store") if r % 2 else ("store", "file")
            for name in order:
                ms, out = once(split_file, tmp) if name == "file" else once(split_store)
                reps["split_%s_ms" % name].append(ms)
                if name == "file":
                    by_file = out
                else:
                    by_store = out
            if r == 0:
                assert all(torch.equal(by_file._job.t[k], by_store._job.t[k]) for k in by_file._job.t)
                assert np.array_equal(by_file.edge_off, by_store.edge_off) and np.array_equal(by_file.theta, by_store.theta)
            del by_file, by_store, out
        reps["pack_batch_us"].append(pack_us(jobs[0], big))
        reps["pack_concat_us"].append(pack_us(jobs[1], big))
    out = {"scenes": args.scenes, "rounds": args.rounds, "warmup": args.warmup, "reps": args.reps, "parts": args.parts,
           "nodes_per_batch": int(part.node_off[-1]), "actors_per_batch": int(part.actor_off[-1]),
           "edge_words_per_batch": 2 * int(part.rel_off[-1]), "edge_words_concat": 2 * int(whole.rel_off[-1]),
           "part_store_mb": round(part.nbytes / 1e6, 2), "split_store_mb": round(whole.nbytes / 1e6, 2),
           "rocm": getattr(torch.version, "hip", None), "equal": True}
    for k, v in reps.items():
        out[k] = {"median": round(statistics.median(v), 3), "min": round(min(v), 3), "max": round(max(v), 3)}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
