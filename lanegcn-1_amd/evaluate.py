"""Evaluate a whole split on the device: the reference's test.py loop (test.py:60-100) and Argoverse's forecasting
metrics (eval_forecasting.get_displacement_errors_and_miss_rate) on the resident scene store.

    ev = evaluate_store(net, DeviceSceneStore(path), batch_size=32)
    ev.summary()            # {6: {"minADE": ..., "minFDE": ..., "MR": ..., ...}, 1: {...}, "n_evaluated": ...}

Per batch: one launch of lgcn_eval_scenes behind the forward writes a 32-float record per scene (its agent, the first actor
row) into a table that holds one row per scene of the split -- no host read, no synchronise.  Per summary: one launch of
lgcn_eval_reduce sums the table in float64 in a fixed order and one device-to-host read brings the sums back.  The table
makes the result independent of the batch size, the order of the batches and the number of ranks: every slot is written
by one wave from that scene's rows alone."""
from typing import Dict, Optional, Sequence

import numpy as np
import torch

from . import ops
from ._lib import LgcnError

METRICS = ("minADE", "minFDE", "MR", "p-minADE", "brier-minADE", "brier-minFDE")      # Argoverse's key order
_COLUMN = {"minADE": 0, "minFDE": 1, "MR": 2, "brier-minFDE": 3, "brier-minADE": 4, "p-minADE": 5}      # of lgcn_eval_reduce's out
# one byte buffer behind summary()'s single read: out [8, 6] float64 | cnt [3] int64 | slot error int32 | mixed-records error int32
_AT_CNT, _AT_ERR_SLOT, _AT_ERR_MIX, _STATUS_BYTES = 384, 416, 432, 448


class Evaluator:
    """The record table of a split of `n_scenes` scenes (row = scene index) and, with keep_preds, the agent's num_mods
    trajectories and scores per scene.  `horizon`: the steps that count (default: all num_preds); `miss_thr`: a miss is
    minFDE > miss_thr metres.  The buffers live on `device` (default: the current GPU; "cpu" holds tables to merge only)."""

    def __init__(self, n_scenes: int, num_mods: int, num_preds: int, horizon: Optional[int] = None, miss_thr: float = 2.0,
                 keep_preds: bool = False, device=None):
        horizon = num_preds if horizon is None else horizon
        if n_scenes < 0 or not 1 <= num_mods <= ops.EVAL_MAX_MOD or not 1 <= num_preds <= 64 or not 1 <= horizon <= num_preds:
            raise LgcnError("Evaluator: need n_scenes >= 0, 1 <= num_mods <= 8, 1 <= horizon <= num_preds <= 64, got %s"
                            % ((n_scenes, num_mods, num_preds, horizon),))
        self.n_scenes, self.num_mods, self.num_preds, self.horizon = int(n_scenes), int(num_mods), int(num_preds), int(horizon)
        self.miss_thr, self.keep_preds = float(miss_thr), bool(keep_preds)
        self.device = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
        f32 = dict(dtype=torch.float32, device=self.device)
        self.rec = torch.zeros((self.n_scenes, ops.EVAL_REC), **f32)
        self.traj = torch.zeros((self.n_scenes, self.num_mods, self.num_preds, 2), **f32) if keep_preds else None
        self.score = torch.zeros((self.n_scenes, self.num_mods), **f32) if keep_preds else None
        st = self._status = torch.zeros(_STATUS_BYTES, dtype=torch.uint8, device=self.device)
        self._out = st[:_AT_CNT].view(torch.float64).view(ops.EVAL_MAX_MOD, 6)
        self._cnt = st[_AT_CNT:_AT_CNT + 24].view(torch.int64)
        self._err_slot = st[_AT_ERR_SLOT:_AT_ERR_SLOT + 4].view(torch.int32)
        self._err_mix = st[_AT_ERR_MIX:_AT_ERR_MIX + 4].view(torch.int32)

    def update(self, out_reg_flat, out_cls_flat, fb, ex: Dict, indices) -> None:
        """One launch on the current stream: the records of the batch `fb` / `ex` (DeviceSceneStore.batch) whose scenes are
        the rows `indices` of the split, from the flat outputs reg [A, M, T, 2] (world frame) and cls [A, M] of its forward."""
        if "gt_preds" not in ex or "has_preds" not in ex:
            raise LgcnError("Evaluator.update: the batch holds no gt_preds / has_preds to evaluate against")
        idx = np.ascontiguousarray(indices, dtype=np.int64).reshape(-1)
        if idx.size != fb.n_scenes:
            raise LgcnError("Evaluator.update: %d indices for a batch of %d scenes" % (idx.size, fb.n_scenes))
        A = fb.n_actors
        if tuple(out_reg_flat.shape) != (A, self.num_mods, self.num_preds, 2):
            raise LgcnError("Evaluator.update: reg must be %s, got %s" % ((A, self.num_mods, self.num_preds, 2), tuple(out_reg_flat.shape)))
        with torch.cuda.device(self.device):
            stage = torch.empty(idx.size, dtype=torch.int64, pin_memory=True)      # as the store's table: no synchronising copy
            stage.numpy()[:] = idx
            slot = stage.to(self.device, non_blocking=True)
            ops.eval_scenes(out_reg_flat, out_cls_flat, ex["gt_preds"], ex["has_preds"], fb.actor_off, slot, self.horizon,
                            self.rec, self.traj, self.score, self._err_slot)

    def merge(self) -> None:
        """Sum the tables over the ranks of torch.distributed, one all-reduce each.  Every slot is written by exactly one
        rank and is zero on the others, so the sum adds zeros: every rank then holds the single-process table, and its
        summary() is the single-process one bit for bit.  No-op without a process group."""
        import torch.distributed as dist
        if not (dist.is_available() and dist.is_initialized()) or dist.get_world_size() == 1:
            return
        for t in (self.rec, self.traj, self.score):
            if t is not None:
                dist.all_reduce(t, op=dist.ReduceOp.SUM)
        dist.all_reduce(self._err_slot, op=dist.ReduceOp.MAX)

    def summary(self, ks: Sequence[int] = (6, 1), strict: bool = False) -> Dict:
        """One reduce launch and one device-to-host read -> {k: {metric: mean over the evaluated scenes}} for every k of
        `ks`, plus n_evaluated / n_skipped / n_nonfinite (scenes of flag 1 / 0 / 2).  strict: LgcnError unless every scene
        of the split was evaluated (the reference's `assert has_preds.all()`)."""
        ks = [int(k) for k in ks]
        if any(not 1 <= k <= self.num_mods for k in ks):
            raise LgcnError("summary: K must lie in 1..%d, got %s" % (self.num_mods, ks))
        with torch.cuda.device(self.device):
            ops.eval_reduce(self.rec, self.miss_thr, self._out, self._cnt, self._err_mix)
        host = self._status.cpu().numpy()
        if int(host[_AT_ERR_SLOT:_AT_ERR_SLOT + 4].view(np.int32)[0]) != 0:
            raise LgcnError("Evaluator: a scene index outside [0, %d) was passed to update(); its scene was not recorded" % self.n_scenes)
        if int(host[_AT_ERR_MIX:_AT_ERR_MIX + 4].view(np.int32)[0]) != 0:
            raise LgcnError("Evaluator: the table holds records of different num_mods / horizon")
        out = host[:_AT_CNT].view(np.float64).reshape(ops.EVAL_MAX_MOD, 6)
        n_skip, n_eval, n_bad = (int(c) for c in host[_AT_CNT:_AT_CNT + 24].view(np.int64))
        if strict and (n_skip or n_bad):
            raise LgcnError("Evaluator: %d scenes were not evaluated (no agent, or its future is not fully observed) and %d hold "
                            "non-finite values" % (n_skip, n_bad))
        res = {}
        for k in ks:
            res[k] = {m: (float(out[k - 1, _COLUMN[m]]) / n_eval if n_eval else float("nan")) for m in METRICS}
        res.update(n_evaluated=n_eval, n_skipped=n_skip, n_nonfinite=n_bad)
        return res

    def records(self) -> np.ndarray:
        """The raw record table [n_scenes, 32] (layout: include/lgcn.h, lgcn_eval_scenes)."""
        return self.rec.cpu().numpy()

    def predictions(self):
        """(index [n], preds [n, M, T, 2], scores [n, M]) of the scenes with a record of flag 1 or 2: the agent's
        trajectories (world frame, sorted by score) and scores -- the `preds` table of test.py:79-90.  Needs keep_preds."""
        if not self.keep_preds:
            raise LgcnError("Evaluator.predictions: built without keep_preds")
        index = torch.nonzero(self.rec[:, 0] >= 1.0).reshape(-1)
        return index.cpu().numpy(), self.traj[index].cpu().numpy(), self.score[index].cpu().numpy()


def evaluate_store(net, store, batch_size: int, evaluator: Optional[Evaluator] = None, indices=None, on_batch=None) -> Evaluator:
    """Run `net` over the scenes `indices` (default: all) of a flatfile.DeviceSceneStore in batches of `batch_size` (the
    last one may be shorter) and record every scene in `evaluator` (default: a new one for the whole store, sized by
    net.config).  Per batch: store.plan, store.batch, the whole-Net forward of Net.forward_store with its one host read
    and its error behaviour (KeyError / RuntimeError, the pair-capacity regrow, the range guard's re-run), one
    Evaluator.update.  A batch whose scenes hold no actor at all is skipped: its slots stay `not evaluated`.
    `on_batch(out, fb, ex)`, if given, sees every evaluated batch's flat outputs (train_dp.py takes the validation loss there)."""
    if not store.has_gt:
        raise LgcnError("evaluate_store: the store holds no gt_preds / has_preds to evaluate against")
    if batch_size < 1:
        raise LgcnError("evaluate_store: batch_size must be positive")
    if evaluator is None:
        evaluator = Evaluator(len(store), net.config["num_mods"], net.config["num_preds"], device=store.device)
    if evaluator.n_scenes != len(store):
        raise LgcnError("evaluate_store: the evaluator holds %d slots for a store of %d scenes" % (evaluator.n_scenes, len(store)))
    idx = np.arange(len(store), dtype=np.int64) if indices is None else np.asarray(indices, dtype=np.int64).reshape(-1)
    with torch.no_grad():
        for i in range(0, len(idx), batch_size):
            pick = idx[i:i + batch_size]
            plan = store.plan(pick)
            if plan.n_actors == 0:
                continue
            fb, ex, out = net.forward_store_flat(store, pick, plan=plan)
            evaluator.update(out["reg"], out["cls"], fb, ex, pick)
            if on_batch is not None:
                on_batch(out, fb, ex)
    return evaluator
