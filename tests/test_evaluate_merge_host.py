"""CPU, world_size 2, gloo: Evaluator.merge() of two half-filled tables (every slot written by exactly one rank, zero on
the other) equals the full table bit for bit -- records, trajectories and scores."""
import os
import socket

import numpy as np
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N, M, T = 37, 6, 30


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _full_tables():
    import sys
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import eval_cases as EC
    rec = torch.from_numpy(EC.make_records(N, M, T, seed=3))
    g = torch.Generator().manual_seed(0)
    traj = (torch.rand((N, M, T, 2), generator=g) - 0.5) * 1e4
    score = torch.randn((N, M), generator=g) * 10
    empty = rec[:, 0] == 0                      # a slot nobody evaluated holds no prediction either
    traj[empty], score[empty] = 0.0, 0.0
    return rec, traj, score


def _worker(rank, world, port, q):
    import sys
    sys.path.insert(0, ROOT)
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world),
                      LOCAL_RANK=str(rank))
    import lanegcn_amd  # noqa: F401
    from lanegcn_amd import dist as D
    from lanegcn_amd.evaluate import Evaluator
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        rec, traj, score = _full_tables()
        mine = list(range(rank, N, world))         # the shard of train_dp.py --eval-store: no tail dropped, 19 + 18 slots
        ev = Evaluator(N, M, T, keep_preds=True, device="cpu")
        ev.rec[mine], ev.traj[mine], ev.score[mine] = rec[mine], traj[mine], score[mine]
        assert not torch.equal(ev.rec, rec)
        ev.merge()
        same = lambda a, b: np.array_equal(a.numpy().view(np.uint32), b.numpy().view(np.uint32))
        assert same(ev.rec, rec) and same(ev.traj, traj) and same(ev.score, score)
        ev._err_slot[0] = rank                     # a slot error seen by one rank reaches every rank
        ev.merge()
        assert int(ev._err_slot[0]) == 1
        D.barrier()
        q.put((rank, "ok"))
    except Exception as e:  # noqa: BLE001
        q.put((rank, repr(e)))
        raise
    finally:
        dist.destroy_process_group()


def test_merge_of_two_half_tables_is_the_full_table():
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


def test_merge_without_a_process_group_is_a_no_op():
    import lanegcn_amd  # noqa: F401
    from lanegcn_amd.evaluate import Evaluator
    ev = Evaluator(N, M, T, device="cpu")
    ev.rec[:] = _full_tables()[0]
    before = ev.rec.clone()
    ev.merge()
    assert torch.equal(ev.rec, before)
