"""ActorNet (the Conv1d FPN, reference lanegcn.py:213-263) forward / forward+backward time on the S2 actor batch
[1600, 3, 20]: what MIOpen costs in a training step, and what the HIP units cost beside it.

  --impl stock   the stock path (MIOpen convolutions; channels-last + lgcn_gn_cl under no_grad)
  --impl hip     the f16x2 HIP units (fused Res1d blocks under no_grad, Conv1dGNFn under autograd)
  --impl exact   the exact-fp32 HIP units (ActorNet.exact)
  --impl all     the three interleaved step by step in one process (medians per variant)
  --mma MODE     the matrix mode around it (the hip / exact variants are forced on whatever it is)

Env knobs are MIOpen's own (MIOPEN_DEBUG_CONV_GEMM=0 ...); --find turns on torch.backends.cudnn.benchmark (MIOpen find)."""
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

# variant -> (ActorNet.impl, ActorNet.exact, matrix mode it needs or None)
VARIANTS = {"stock": ("miopen", False, None), "hip": ("hip", False, "f16x2"), "exact": ("hip", True, None)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--impl", default="stock", choices=["stock", "hip", "exact", "all"])
    ap.add_argument("--mma", default=None)
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--actors", type=int, default=1600)
    ap.add_argument("--find", action="store_true")
    args = ap.parse_args()
    if args.mma:
        ops.set_mma(args.mma)
    mode = ops.get_mma()
    torch.backends.cudnn.benchmark = args.find
    torch.manual_seed(0)
    net = M.ActorNet(M.config).cuda().train()
    x = torch.randn(args.actors, 3, 20, device="cuda")
    M.ActorNet.train_hip = True
    names = list(VARIANTS) if args.impl == "all" else [args.impl]

    def select(name):
        impl, exact, need = VARIANTS[name]
        M.ActorNet.impl, M.ActorNet.exact = impl, exact
        ops.set_mma(need or mode)          # the f16x2 units exist in that mode only

    def fwd():
        with torch.no_grad():
            return net(x)

    def fwd_bwd():
        net.zero_grad(set_to_none=True)
        net(x).square().mean().backward()

    res = {"metric": "ActorNet, %d actors" % args.actors, "mma": mode, "steps": args.steps, "median_ms": {}}
    for what, fn in (("forward (no_grad)", fwd), ("forward+backward", fwd_bwd)):
        for name in names:
            select(name)
            for _ in range(args.warmup):
                fn()
        torch.cuda.synchronize()
        times = {name: [] for name in names}
        for _ in range(args.steps):
            for name in names:
                select(name)
                t0 = time.perf_counter()
                fn()
                torch.cuda.synchronize()
                times[name].append((time.perf_counter() - t0) * 1e3)
        for name in names:
            print("%s, %s: median %.3f ms (min %.3f)" % (what, name, float(np.median(times[name])), min(times[name])), flush=True)
        res["median_ms"][what] = {name: float(np.median(times[name])) for name in names}
    ops.set_mma(mode)
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
