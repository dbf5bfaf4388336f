"""Evaluating a split: lanegcn_amd.evaluate.evaluate_store against the loop a user had to write without it, and the two
evaluation launches alone.

    python tools/bench_eval.py [--scenes 256] [--batch 32] [--rounds 30] [--warmup 5] [--reps 3] [--slots 39472]
    python tools/bench_eval.py --actors [--actor-slots 631552]
    python tools/bench_eval.py --ragged [--replay]

The store and the protocol of tools/bench_store.py: `scenes` synthetic scenes of S2's per-scene size (324 nodes, 50
actors), batches of `batch`; one process measures, the two loops alternating, `reps` times over.
  (a) scenes_per_s_evaluate  evaluate_store over `rounds` batches + summary() (one reduce launch, one read)
  (b) scenes_per_s_manual    the same batches through Net.forward_store, PostProcess.forward's per-scene host copies of
                             reg[i][0:1] / gt_preds / has_preds, and pred_metrics at the end
      each window starts and ends with a synchronise; scenes/s = rounds * batch / window
  (c) eval_scenes_us         lgcn_eval_scenes for one batch between device events
  (d) eval_reduce_us         lgcn_eval_reduce over `slots` records (39,472: the Argoverse validation split) between events
  (c) and (d) are medians over `rounds` launches after `warmup`, each behind a queued 256 MB fill (the stream is busy while
  the host enqueues, so the interval is the launch and not the host's call).  Per figure the JSON line carries the median of the `reps`
values and their lowest and highest (the spread between repetitions).

--ragged: the scenes' sizes differ (2..4 roads, 20..80 actors drawn per scene), as a real split's do.
--replay (without --actors): also (a') scenes_per_s_replay, evaluate_store(..., replay=StoreReplay) over the same
windows, alternating with (a) -- (a) of the same run is its baseline; the line then carries replay_stats (routes, mean
pad shares, host ms per batch) and graph_pool_mb of the last window.  The StoreReplay is made per window (capacities
over the window's batches) before the timed region; its warm-up batches capture the graph.

--actors: the same store and protocol for the evaluation of EVERY actor (evaluate.ActorEvaluator; every actor of the
synthetic store is fully observed, the most work a row can be):
  (e) scenes_per_s_actors    evaluate_store(actors=True) + summary(), alternating with (a) in the same process
  (f) eval_actors_us         lgcn_eval_actors for one batch (1,600 actor rows) next to (c) on the same batch
  (g) eval_reduce_sel_us     lgcn_eval_reduce_sel (who = others, every evaluated record kept) over `actor-slots` records
                             (631,552 = 16 per scene of (d)'s split), next to lgcn_eval_reduce over the same table

--dac (with or without --actors): drivable-area compliance on a synthetic raster (two cities of 2,048 x 2,048 cells, 16 m
blocks of which about two in three are drivable, the scenes alternating between them):
  (h) scenes_per_s_dac       evaluate_store + summary() with drivable=, alternating with the same loop without it ((a) or (e))
  (i) eval_*_da_us           the _da launch for one batch next to the plain launch on the same batch
  (j) eval_dac_reduce_us     lgcn_eval_dac_reduce over `slots` (`actor-slots`) records next to the plain reduce"""
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
    ap.add_argument("--slots", type=int, default=39472)
    ap.add_argument("--actors", action="store_true", help="measure the evaluation of every actor against the agent-only one")
    ap.add_argument("--actor-slots", type=int, default=16 * 39472)
    ap.add_argument("--dac", action="store_true", help="measure drivable-area compliance against the same evaluation without it")
    ap.add_argument("--ragged", action="store_true")
    ap.add_argument("--replay", action="store_true")
    args = ap.parse_args()
    import numpy as np
    import torch
    import lanegcn_amd  # noqa: F401
    from lanegcn_amd import data as gen
    from lanegcn_amd import lanegcn as M
    from lanegcn_amd import ops
    from lanegcn_amd.evaluate import ActorEvaluator, Evaluator, evaluate_store
    from lanegcn_amd.flatfile import DeviceSceneStore, write_scenes

    if not torch.cuda.is_available():
        raise SystemExit("bench_eval.py measures on the GPU; none found")
    with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, "split.npz")
        if args.ragged:
            srng = np.random.default_rng(0)
            scenes = [gen.synth_scene(srng, [6] * int(srng.integers(2, 5)), int(srng.integers(20, 81))) for _ in range(args.scenes)]
        else:
            scenes = gen.synth_batch("S2", seed=0, n_scenes=args.scenes)
        write_scenes(path, scenes)
        store = DeviceSceneStore(path)
    torch.manual_seed(0)
    net = M.Net(M.config).cuda().eval()
    post = M.PostProcess(M.config)
    cfg = M.config
    sync = torch.cuda.synchronize
    rng = np.random.default_rng(1)
    n_batches = args.warmup + args.rounds

    def picks():
        """The scene indices of one window: `n_batches` batches without a repeat inside a batch."""
        return [rng.permutation(args.scenes)[:args.batch].astype(np.int64) for _ in range(n_batches)]

    last_replay = []

    def drivable_area():
        from lanegcn_amd.evaluate import DrivableArea
        drng = np.random.default_rng(2)
        se2 = np.array([[1., 0., 1024.], [0., 1., 1024.], [0., 0., 1.]])
        da = DrivableArea({c: (np.kron(drng.random((128, 128)) < 2 / 3, np.ones((16, 16), bool)), se2) for c in ("A", "B")})
        return dict(drivable=da.to("cuda"), scene_city=np.arange(len(store), dtype=np.int32) % 2)

    da_kw = drivable_area() if args.dac else {}

    def evaluate_rate(window, actors=False, replay=False, dac=False):
        kw = da_kw if dac else {}
        ev = ActorEvaluator.for_store(store, cfg, **kw) if actors else Evaluator(len(store), cfg["num_mods"], cfg["num_preds"], **kw)
        if replay:
            from lanegcn_amd.engine import StoreReplay
            from lanegcn_amd.flatfile import StoreCaps
            replay = StoreReplay(net, store, StoreCaps.for_picks(store, window))
            last_replay[:] = [replay]
        evaluate_store(net, store, args.batch, ev, indices=np.concatenate(window[:args.warmup]), replay=replay)
        sync()
        t0 = time.perf_counter()
        evaluate_store(net, store, args.batch, ev, indices=np.concatenate(window[args.warmup:]), replay=replay)
        res = ev.summary()
        sync()
        return args.rounds * args.batch / (time.perf_counter() - t0), res

    def manual_rate(window):
        """forward_store + PostProcess.forward's host copies + pred_metrics: what scoring a split took without the evaluator."""
        first = store.actor_off[:-1]
        gt_all, has_all = store._job.t["gt_preds"], store._job.t["has_preds"].bool()
        metrics = {"preds": [], "gt_preds": [], "has_preds": []}
        with torch.no_grad():
            for i, pick in enumerate(window):
                if i == args.warmup:
                    metrics = {"preds": [], "gt_preds": [], "has_preds": []}
                    sync()
                    t0 = time.perf_counter()
                out = net.forward_store(store, pick)
                rows = torch.from_numpy(first[pick]).cuda()          # one gather + one copy per tensor, as train_dp.first_rows_on_host
                data = {"gt_preds": list(gt_all[rows].cpu().split(1)), "has_preds": list(has_all[rows].cpu().split(1))}
                po = post(out, data)
                for k in metrics:
                    metrics[k] += po[k]
            ade1, fde1, ade, fde, _ = M.pred_metrics(np.concatenate(metrics["preds"], 0), np.concatenate(metrics["gt_preds"], 0),
                                                     np.concatenate(metrics["has_preds"], 0))
            sync()
        return args.rounds * args.batch / (time.perf_counter() - t0), (ade1, fde1, ade, fde)

    busy = torch.empty(1 << 28, dtype=torch.uint8, device="cuda")

    def launch_us(fn):
        """Median device time of fn() between two events, in microseconds.  A 256 MB fill is queued first, so the stream is
        still busy while the host enqueues event, launch, event: the interval holds the launch, not the host's call."""
        ts = []
        for i in range(n_batches):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            busy.zero_()
            a.record()
            fn()
            b.record()
            b.synchronize()
            if i >= args.warmup:
                ts.append(a.elapsed_time(b) * 1e3)
        return statistics.median(ts)

    def filled(n):
        """A record table of n evaluated records (an ActorEvaluator of one scene), every third one a first actor."""
        big = ActorEvaluator(np.array([0, n], np.int64), cfg["num_mods"], cfg["num_preds"])
        big.rec[:, 0] = 1.0
        big.rec[:, 1], big.rec[:, 2] = cfg["num_mods"], cfg["num_preds"]
        big.rec[:, 3] = (torch.arange(n, device="cuda") % 3).float()
        big.rec[:, 4:4 + 3 * cfg["num_mods"]] = torch.rand((n, 3 * cfg["num_mods"]), device="cuda")
        return big

    if args.dac:
        base = "actors" if args.actors else "evaluate"
        launch = "eval_actors" if args.actors else "eval_scenes"
        plain_reduce = "eval_reduce_sel" if args.actors else "eval_reduce"
        n_red = args.actor_slots if args.actors else args.slots
        reps = {"scenes_per_s_" + base: [], "scenes_per_s_dac": [], launch + "_us": [], launch + "_da_us": [],
                plain_reduce + "_us": [], "eval_dac_reduce_us": []}
        got = {}
        for r in range(args.reps):
            window = picks()
            for dac in ((False, True) if r % 2 else (True, False)):
                rate, got[dac] = evaluate_rate(window, actors=args.actors, dac=dac)
                reps["scenes_per_s_" + ("dac" if dac else base)].append(rate)
            n_mod = cfg["num_mods"]
            if got[True][n_mod]["minFDE"] != got[False][n_mod]["minFDE"]:
                raise SystemExit("bench_eval.py: the evaluation with a map scored other records than the one without")
            pick = window[0]
            with torch.no_grad():
                fb, ex, out = net.forward_store_flat(store, pick)
            ev = ActorEvaluator.for_store(store, cfg, **da_kw) if args.actors else Evaluator(len(store), n_mod, cfg["num_preds"], **da_kw)
            rows = torch.from_numpy(store.actor_off[pick] if args.actors else pick).cuda()
            city = torch.from_numpy(da_kw["scene_city"][pick]).cuda()
            tensors = (out["reg"], out["cls"], ex["gt_preds"], ex["has_preds"], fb.actor_off, rows, ev.horizon, ev.rec, None, None, ev._err_slot)
            plain_fn, da_fn = (ops.eval_actors, ops.eval_actors_da) if args.actors else (ops.eval_scenes, ops.eval_scenes_da)
            reps[launch + "_us"].append(launch_us(lambda: plain_fn(*tensors)))
            reps[launch + "_da_us"].append(launch_us(lambda: da_fn(*tensors, da_kw["drivable"], city)))
            big = filled(n_red)
            big.rec[:, 30] = torch.randint(0, 1 << n_mod, (n_red,), device="cuda").float()
            big.rec[:, 31] = 1.0
            dac_out = torch.zeros(ops.EVAL_DAC_OUT, dtype=torch.int64, device="cuda")
            if args.actors:
                reps[plain_reduce + "_us"].append(launch_us(lambda: ops.eval_reduce_sel(
                    big.rec, 2.0, ops.EVAL_WHO["others"], big.horizon - 1, big._out, big._cnt4, big._err_mix)))
                reps["eval_dac_reduce_us"].append(launch_us(lambda: ops.eval_dac_reduce(big.rec, ops.EVAL_WHO["others"], big.horizon - 1, dac_out)))
            else:
                reps[plain_reduce + "_us"].append(launch_us(lambda: ops.eval_reduce(big.rec, 2.0, big._out, big._cnt, big._err_mix)))
                reps["eval_dac_reduce_us"].append(launch_us(lambda: ops.eval_dac_reduce(big.rec, 0, ops.EVAL_MAX_T, dac_out)))
        res = {"scenes": args.scenes, "batch": args.batch, "rounds": args.rounds, "warmup": args.warmup, "reps": args.reps,
               "actors": args.actors, "rows_per_batch": int(fb.n_actors if args.actors else fb.n_scenes), "reduce_slots": n_red,
               "DAC": {k: float("%.6g" % got[True][k]["DAC"]) for k in (n_mod, 1)}, "n_dac": got[True]["n_dac"]}
        for k, v in reps.items():
            digits = 1 if k.startswith("scenes") else 2
            res[k] = {"median": round(statistics.median(v), digits), "min": round(min(v), digits), "max": round(max(v), digits)}
        print(json.dumps(res))
        return

    if args.actors:
        reps = {"scenes_per_s_evaluate": [], "scenes_per_s_actors": [], "eval_scenes_us": [], "eval_actors_us": [],
                "eval_reduce_us": [], "eval_reduce_sel_us": []}
        agree = None
        for r in range(args.reps):
            window = picks()
            got = {}
            for name in (("evaluate", "actors") if r % 2 else ("actors", "evaluate")):
                rate, got[name] = evaluate_rate(window, actors=name == "actors")
                reps["scenes_per_s_" + name].append(rate)
            n_mod = cfg["num_mods"]
            agree = (got["evaluate"][n_mod]["minFDE"], got["actors"][n_mod]["minFDE"], got["actors"]["n_evaluated"])
            pick = window[0]
            with torch.no_grad():
                fb, ex, out = net.forward_store_flat(store, pick)
            ev, av = Evaluator(len(store), n_mod, cfg["num_preds"]), ActorEvaluator.for_store(store, cfg)
            slot = torch.from_numpy(pick).cuda()
            base = torch.from_numpy(store.actor_off[pick]).cuda()
            reps["eval_scenes_us"].append(launch_us(lambda: ops.eval_scenes(
                out["reg"], out["cls"], ex["gt_preds"], ex["has_preds"], fb.actor_off, slot, ev.horizon, ev.rec, None, None, ev._err_slot)))
            reps["eval_actors_us"].append(launch_us(lambda: ops.eval_actors(
                out["reg"], out["cls"], ex["gt_preds"], ex["has_preds"], fb.actor_off, base, av.horizon, av.rec, None, None, av._err_slot)))
            big = filled(args.actor_slots)
            reps["eval_reduce_us"].append(launch_us(lambda: ops.eval_reduce(big.rec, 2.0, big._out, big._cnt, big._err_mix)))
            reps["eval_reduce_sel_us"].append(launch_us(lambda: ops.eval_reduce_sel(
                big.rec, 2.0, ops.EVAL_WHO["others"], big.horizon - 1, big._out, big._cnt4, big._err_mix)))
        res = {"scenes": args.scenes, "batch": args.batch, "rounds": args.rounds, "warmup": args.warmup, "reps": args.reps,
               "actor_rows_per_batch": int(fb.n_actors), "reduce_slots": args.actor_slots,
               "minFDE_agents": float("%.6g" % agree[0]), "minFDE_all_actors": float("%.6g" % agree[1]), "actors_evaluated": agree[2]}
        for k, v in reps.items():
            digits = 1 if k.startswith("scenes") else 2
            res[k] = {"median": round(statistics.median(v), digits), "min": round(min(v), digits), "max": round(max(v), digits)}
        print(json.dumps(res))
        return

    reps = {"scenes_per_s_evaluate": [], "scenes_per_s_manual": [], "eval_scenes_us": [], "eval_reduce_us": []}
    agree = None
    for r in range(args.reps):
        window = picks()
        got = {}
        names = ("evaluate", "manual") + (("replay",) if args.replay else ())
        for name in (names if r % 2 else names[::-1]):
            rate, got[name] = manual_rate(window) if name == "manual" else evaluate_rate(window, replay=name == "replay")
            reps.setdefault("scenes_per_s_" + name, []).append(rate)
        if args.replay and got["replay"] != got["evaluate"]:
            raise SystemExit("bench_eval.py: the replay route's summary differs from the eager one's")
        # the two loops scored the same scenes: K = 1 / K = num_mods minADE, minFDE against ade1, fde1, ade, fde
        s, m = got["evaluate"], got["manual"]
        mine = (s[1]["minADE"], s[1]["minFDE"], s[cfg["num_mods"]]["minADE"], s[cfg["num_mods"]]["minFDE"])
        # (a scene picked in several batches counts once in the table and once per batch in the manual loop: a loose check)
        agree = max(abs(a - float(b)) / abs(float(b)) for a, b in zip(mine, m))
        # the launches alone, on one batch of this store
        pick = window[0]
        with torch.no_grad():
            fb, ex, out = net.forward_store_flat(store, pick)
        ev = Evaluator(len(store), cfg["num_mods"], cfg["num_preds"])
        slot = torch.from_numpy(pick).cuda()
        reps["eval_scenes_us"].append(launch_us(lambda: ops.eval_scenes(
            out["reg"], out["cls"], ex["gt_preds"], ex["has_preds"], fb.actor_off, slot, ev.horizon, ev.rec, None, None, ev._err_slot)))
        big = Evaluator(args.slots, cfg["num_mods"], cfg["num_preds"])
        big.rec[:, 0] = 1.0
        big.rec[:, 1], big.rec[:, 2] = cfg["num_mods"], cfg["num_preds"]
        big.rec[:, 4:4 + 3 * cfg["num_mods"]] = torch.rand((args.slots, 3 * cfg["num_mods"]), device="cuda")
        reps["eval_reduce_us"].append(launch_us(lambda: ops.eval_reduce(big.rec, 2.0, big._out, big._cnt, big._err_mix)))
    res = {"scenes": args.scenes, "batch": args.batch, "rounds": args.rounds, "warmup": args.warmup, "reps": args.reps,
           "reduce_slots": args.slots, "metrics_rel_diff_between_loops": float("%.3g" % agree), "ragged": args.ragged}
    if last_replay:
        rp = last_replay[0]
        res.update(replay_stats={k: (round(v, 4) if isinstance(v, float) else v) for k, v in rp.stats.items()},
                   graph_pool_mb=round(rp.graph_pool_bytes() / 1e6, 2))
    for k, v in reps.items():
        digits = 1 if k.startswith("scenes") else 2
        res[k] = {"median": round(statistics.median(v), digits), "min": round(min(v), digits), "max": round(max(v), digits)}
    print(json.dumps(res))


if __name__ == "__main__":
    main()
