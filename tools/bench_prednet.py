"""PredNet (reference lanegcn.py:575-631) forward + backward time on the S2 actor batch (1,600 actors): what the stock
training tail (six nn.Linear heads, stack, AttDest's first Linear, the score Linear, sort, indexed gather and their autograd)
costs, and what the HIP tail (PredNet.train_hip: PredRegFn / PredFinalFn) costs beside it.  The LinearRes / AttDest row blocks
are the same Functions in both.

  --impl stock   PredNet.train_hip = False
  --impl hip     PredNet.train_hip = True
  --impl ab      both, alternating call by call after a warm-up of each (medians per variant)
  --repeat N     the whole measurement N times in one process: the spread of a repeated identical run"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import lanegcn_amd  # noqa: E402,F401
from lanegcn_amd import lanegcn as M  # noqa: E402
from lanegcn_amd import ops  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--impl", default="ab", choices=["stock", "hip", "ab"])
    ap.add_argument("--mma", default=None)
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--actors", type=int, default=1600)
    ap.add_argument("--repeat", type=int, default=1)
    args = ap.parse_args()
    if args.mma:
        ops.set_mma(args.mma)
    torch.manual_seed(0)
    torch.autograd.set_multithreading_enabled(False)
    net = M.PredNet(M.config).cuda().train()
    actors = torch.randn(args.actors, 128, device="cuda").relu().requires_grad_(True)
    ctrs = [torch.randn(args.actors, 2, device="cuda") * 30]
    idcs = [torch.arange(args.actors, device="cuda")]
    names = ["hip", "stock"] if args.impl == "ab" else [args.impl]
    w = {}

    def fwd_bwd(name):
        M.PredNet.train_hip = name == "hip"
        net.zero_grad(set_to_none=True)
        actors.grad = None
        out = net(actors, idcs, ctrs)
        cls, reg = out["cls"][0], out["reg"][0]
        if not w:
            w["cls"], w["reg"] = torch.randn_like(cls), torch.randn_like(reg)
        ((cls * w["cls"]).sum() + (reg * w["reg"]).sum()).backward()

    res = {"metric": "PredNet forward + backward, %d actors" % args.actors, "mma": ops.get_mma(), "steps": args.steps,
           "median_ms": {name: [] for name in names}, "min_ms": {name: [] for name in names}}
    for name in names:
        for _ in range(args.warmup):
            fwd_bwd(name)
    torch.cuda.synchronize()
    for _ in range(args.repeat):
        times = {name: [] for name in names}
        for _ in range(args.steps):
            for name in names:
                t0 = time.perf_counter()
                fwd_bwd(name)
                torch.cuda.synchronize()
                times[name].append((time.perf_counter() - t0) * 1e3)
        for name in names:
            res["median_ms"][name].append(float(np.median(times[name])))
            res["min_ms"][name].append(min(times[name]))
            print("forward+backward, %s: median %.3f ms (min %.3f)" % (name, res["median_ms"][name][-1], min(times[name])), flush=True)
    res["spread_ms"] = {name: max(v) - min(v) for name, v in res["median_ms"].items()}
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
