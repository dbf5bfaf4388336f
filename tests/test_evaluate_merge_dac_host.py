"""CPU, world_size 2, gloo: Evaluator.merge() of an evaluator with a DrivableArea.  The compliance floats [30], [31] of a
record are zero on the rank that did not write the slot, like the rest of it, so the summed table is the full table bit
for bit and merge() needed no change."""
import os
import sys

import numpy as np
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
from test_evaluate_merge_host import M, N, T, _free_port, _full_tables      # noqa: E402


def _dac_tables():
    rec = _full_tables()[0].clone()
    g = torch.Generator().manual_seed(1)
    ok = rec[:, 0] == 1
    rec[ok, 30] = torch.randint(0, 1 << M, (int(ok.sum()),), generator=g).float()
    rec[ok, 31] = 1.0
    return rec


def _worker(rank, world, port, q):
    sys.path.insert(0, ROOT)
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world), LOCAL_RANK=str(rank))
    import lanegcn_amd  # noqa: F401
    from lanegcn_amd.evaluate import DrivableArea, Evaluator
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        rec = _dac_tables()
        assert (rec[:, 31] == 1).sum() > 5 and (rec[:, 31] == 0).sum() > 0
        mine = list(range(rank, N, world))
        da = DrivableArea({"P": (np.ones((7, 9)), np.eye(3))})
        ev = Evaluator(N, M, T, device="cpu", drivable=da, scene_city=["P"] * N)
        ev.rec[mine] = rec[mine]
        ev.merge()
        assert np.array_equal(ev.rec.numpy().view(np.uint32), rec.numpy().view(np.uint32))
        q.put((rank, "ok"))
    except Exception as e:  # noqa: BLE001
        q.put((rank, repr(e)))
        raise
    finally:
        dist.destroy_process_group()


def test_merge_keeps_the_compliance_floats():
    world = 2
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_worker, args=(r, world, port, q)) for r in range(world)]
    for p in procs:
        p.start()
    res = [q.get(timeout=180) for _ in range(world)]
    for p in procs:
        p.join(timeout=60)
    assert sorted(res) == [(0, "ok"), (1, "ok")], res
