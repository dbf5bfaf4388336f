"""Training-step timing (BASELINE.json config 3: end-to-end lanegcn.py training step, batch = 32, fp32):
Net forward + loss + backward + Adam step on one 32-scene synthetic batch (S2), HIP hot path fwd/bwd, against
the same step on the CPU with the oracle's stock-ATen statement of the hot path (reference-equivalent)."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import lanegcn_amd  # noqa: E402,F401
from lanegcn_amd import autograd as A  # noqa: E402
from lanegcn_amd import data as gen  # noqa: E402
from lanegcn_amd import lanegcn as M  # noqa: E402
from lanegcn_amd import layers  # noqa: E402
from lanegcn_amd import ops  # noqa: E402
from lanegcn_amd import utils  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--mma", default=None)
    ap.add_argument("--cpu-steps", type=int, default=2)
    ap.add_argument("--actor-impl", default=None, choices=["hip", "miopen", "ab"],
                    help="ActorNet.impl for the step; 'ab': both, alternating step by step after a warm-up of each")
    ap.add_argument("--pred-impl", default=None, choices=["hip", "stock", "ab"],
                    help="PredNet's training tail: 'hip' sets PredNet.train_hip, 'stock' leaves the ATen tail; 'ab': both, "
                         "alternating step by step after a warm-up of each")
    ap.add_argument("--att-impl", default=None, choices=["hip", "stock", "ab"],
                    help="Att's training pair stage: 'hip' sets Att.train_hip (AttPairsFn), 'stock' leaves the composed row "
                         "blocks; 'ab': both, alternating step by step after a warm-up of each")
    ap.add_argument("--lc-impl", default=None, choices=["hip", "stock", "ab"],
                    help="LaneConv / LinearRes backward: 'hip' sets MapNet.train_hip, M2M.train_hip and LinearRes.train_hip "
                         "(lgcn_laneconv_bwd), 'stock' leaves the composed launches; 'ab': both, alternating step by step after "
                         "a warm-up of each")
    ap.add_argument("--rb-impl", default=None, choices=["hip", "stock", "ab"],
                    help="Row-block backward (layers.Linear, the input stems, A2M.meta, AttDest, the node side of Att): 'hip' sets "
                         "autograd.RowBlockFn.train_hip (lgcn_rowblock_bwd), 'stock' leaves the composed launches; 'ab': both, "
                         "alternating step by step after a warm-up of each")
    ap.add_argument("--opt-impl", default="stock", choices=["hip", "stock"],
                    help="the optimizer step: 'hip' sets utils.Optimizer.train_hip (lgcn_opt_step), 'stock' leaves torch.optim.  A "
                         "choice for the whole process, not 'ab': the optimizer's state makes interleaved steps meaningless")
    ap.add_argument("--actor-exact", action="store_true",
                    help="ActorNet.exact: the 'hip' ActorNet on the exact-fp32 units (any --mma)")
    args = ap.parse_args()
    M.ActorNet.exact = args.actor_exact
    if args.mma:
        ops.set_mma(args.mma)
    if [args.actor_impl, args.pred_impl, args.att_impl, args.lc_impl, args.rb_impl].count("ab") > 1:
        ap.error("one of --actor-impl / --pred-impl / --att-impl / --lc-impl / --rb-impl can alternate at a time")
    actor_impls = ["hip", "miopen"] if args.actor_impl == "ab" else [args.actor_impl or M.ActorNet.impl]
    pred_impls = ["hip", "stock"] if args.pred_impl == "ab" else [args.pred_impl or "stock"]
    att_impls = ["hip", "stock"] if args.att_impl == "ab" else [args.att_impl or "stock"]
    lc_impls = ["hip", "stock"] if args.lc_impl == "ab" else [args.lc_impl or "stock"]
    rb_impls = ["hip", "stock"] if args.rb_impl == "ab" else [args.rb_impl or "stock"]
    # a variant of the step: (ActorNet.impl, PredNet's training tail, Att's pair stage, the LaneConv / LinearRes backward, the
    # row-block backward); its name is the side that alternates
    impls = [(a, p, t, c, r) for a in actor_impls for p in pred_impls for t in att_impls for c in lc_impls for r in rb_impls]
    name = lambda v: (v[4] if args.rb_impl == "ab" else v[3] if args.lc_impl == "ab" else v[2] if args.att_impl == "ab"
                      else v[1] if args.pred_impl == "ab" else v[0])

    def select(v):
        M.ActorNet.impl, M.PredNet.train_hip, M.Att.train_hip = v[0], v[1] == "hip", v[2] == "hip"
        M.MapNet.train_hip = M.M2M.train_hip = layers.LinearRes.train_hip = v[3] == "hip"
        A.RowBlockFn.train_hip = v[4] == "hip"

    select(impls[0])
    if args.actor_impl:
        M.ActorNet.train_hip = True          # "hip": ActorNet's training units on Conv1dGNFn; "miopen": the stock path
    torch.manual_seed(0)
    torch.autograd.set_multithreading_enabled(False)      # what train_dp.py does for its loop
    net = M.Net(M.config).cuda().train()
    loss_fn = M.Loss(M.config).cuda()
    utils.Optimizer.train_hip = args.opt_impl == "hip"
    opt = M.Optimizer(net.parameters(), M.config)
    assert opt.fused == (args.opt_impl == "hip")
    opt_host, opt_dev = [], []           # of opt.step alone: host time to enqueue it (no sync), device time between two events
    batch = gen.collate_fn(gen.synth_batch("S2", seed=5))
    stages = {}

    def step(i, timed=False):
        marks = [time.perf_counter()]
        out = net(batch)
        if timed:
            torch.cuda.synchronize(); marks.append(time.perf_counter())
        lo = loss_fn(out, batch)
        opt.zero_grad()
        lo["loss"].backward()
        if timed:
            torch.cuda.synchronize(); marks.append(time.perf_counter())
        if timed:
            ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
            ev[0].record()
            t_opt = time.perf_counter()
        opt.step(i / 6436.0)
        if timed:
            opt_host.append((time.perf_counter() - t_opt) * 1e3)
            ev[1].record()
            torch.cuda.synchronize(); marks.append(time.perf_counter())
            opt_dev.append(ev[0].elapsed_time(ev[1]))
            for k, a, b in zip(("forward", "loss+backward", "adam"), marks[:-1], marks[1:]):
                stages.setdefault(k, []).append((b - a) * 1e3)
        return float(lo["loss"].detach())

    losses = []
    for impl in impls:
        select(impl)
        losses += [step(i) for i in range(args.warmup)]
    torch.cuda.synchronize()
    # per-step times (synchronised), the implementations interleaved step by step
    per_step = {name(impl): [] for impl in impls}
    t0 = time.perf_counter()
    for i in range(args.steps):
        for impl in impls:
            select(impl)
            t1 = time.perf_counter()
            losses.append(step(args.warmup + i))
            torch.cuda.synchronize()
            per_step[name(impl)].append((time.perf_counter() - t1) * 1e3)
    ms = (time.perf_counter() - t0) / (args.steps * len(impls)) * 1e3
    select(impls[0])
    for i in range(max(5, args.steps)):
        step(args.warmup + args.steps + i, timed=True)
    res = {"metric": "training step (forward + loss + backward + Adam), batch 32, S2", "mma": ops.get_mma(),
           "ms_per_step": ms, "scenes_per_s": 32e3 / ms, "loss_first": losses[0], "loss_last": losses[-1],
           "stage_ms": {k: float(np.median(v)) for k, v in stages.items()},
           "actor_impl": actor_impls[0] if len(actor_impls) == 1 else "ab", "actor_exact": M.ActorNet.exact,
           "pred_impl": pred_impls[0] if len(pred_impls) == 1 else "ab",
           "att_impl": att_impls[0] if len(att_impls) == 1 else "ab",
           "lc_impl": lc_impls[0] if len(lc_impls) == 1 else "ab",
           "rb_impl": rb_impls[0] if len(rb_impls) == 1 else "ab",
           "opt_impl": args.opt_impl,
           "opt_step_host_ms": {"median": float(np.median(opt_host)), "p25": float(np.percentile(opt_host, 25)),
                                "p75": float(np.percentile(opt_host, 75))},
           "opt_step_device_ms": {"median": float(np.median(opt_dev)), "p25": float(np.percentile(opt_dev, 25)),
                                  "p75": float(np.percentile(opt_dev, 75))},
           "spread_step_ms": {k: [float(np.percentile(v, 25)), float(np.percentile(v, 75))] for k, v in per_step.items()},
           "median_step_ms": {k: float(np.median(v)) for k, v in per_step.items()}}
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
