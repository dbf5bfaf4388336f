"""Evaluate a whole split on the device: the reference's test.py loop (test.py:60-100) and Argoverse's forecasting
metrics (eval_forecasting.get_displacement_errors_and_miss_rate) on the resident scene store.

    ev = evaluate_store(net, DeviceSceneStore(path), batch_size=32)
    ev.summary()            # {6: {"minADE": ..., "minFDE": ..., "MR": ..., ...}, 1: {...}, "n_evaluated": ...}

Per batch: one launch of lgcn_eval_scenes behind the forward writes a 32-float record per scene (its agent, the first actor
row) into a table that holds one row per scene of the split -- no host read, no synchronise.  Per summary: one launch of
lgcn_eval_reduce sums the table in float64 in a fixed order and one device-to-host read brings the sums back.  The table
makes the result independent of the batch size, the order of the batches and the number of ranks: every slot is written
by one wave from that scene's rows alone.

    ev = evaluate_store(net, store, batch_size=32, actors=True)       # an ActorEvaluator: one row per ACTOR of the split
    ev.summary(who="others", min_obs=10)

scores every actor with at least one observed future step by PredLoss's rule (final displacement at the last observed
step, mean over the observed steps): lgcn_eval_actors per batch, lgcn_eval_reduce_sel per summary.

    da = DrivableArea.from_files({"MIA": (mat_path, se2_path), "PIT": (...)})
    ev = evaluate_store(net, store, 32, drivable=da, scene_city=cities)      # one city name / id / None per scene
    ev.summary()[6]["DAC"]

adds Argoverse's drivable-area compliance: the share of the first K modes whose every step lies on the drivable area of the
scene's city.  The lookup rides in the launch that writes the record (lgcn_eval_scenes_da / lgcn_eval_actors_da); the counts
are summed as integers (lgcn_eval_dac_reduce) into the buffer of the summary's one read."""
from typing import Dict, Optional, Sequence

import numpy as np
import torch

from . import _lib as L
from . import ops
from ._lib import LgcnError

METRICS = ("minADE", "minFDE", "MR", "p-minADE", "brier-minADE", "brier-minFDE")      # Argoverse's key order
_COLUMN = {"minADE": 0, "minFDE": 1, "MR": 2, "brier-minFDE": 3, "brier-minADE": 4, "p-minADE": 5}      # of lgcn_eval_reduce's out
# one byte buffer behind summary()'s single read: out [8, 6] float64 | cnt [3] int64 ([4] with a selection) | slot error int32 |
# mixed-records error int32
_AT_CNT, _AT_ERR_SLOT, _AT_ERR_MIX, _STATUS_BYTES = 384, 416, 432, 448
# with a DrivableArea the buffer goes on: dac [9] int64 (lgcn_eval_dac_reduce), padded to 16 bytes
_AT_DAC, _STATUS_BYTES_DAC = 448, 528


class DrivableArea:
    """The drivable areas of a split's cities, as Argoverse ships them: {city: (da_mat [H, W], se2 [3, 3])} with a cell
    drivable iff da_mat == 1 and se2 = npyimage_to_city_se2, applied as stored to city coordinates.  `cities` gives the order,
    which is the id a scene_city entry may name.  The rule of `inside` is include/lgcn.h's."""

    def __init__(self, areas: Dict):
        if len(areas) < 1:
            raise LgcnError("DrivableArea: needs at least one city")
        self.cities = [str(c) for c in areas]
        self.table = (L.DaCity * len(self.cities))()      # the host copy of the device table
        flat, off = [], 0
        for i, (mat, se2) in enumerate(areas.values()):
            mat, se2 = np.asarray(mat), np.asarray(se2, dtype=np.float64)
            if mat.ndim != 2 or mat.shape[0] < 1 or mat.shape[1] < 1:
                raise LgcnError("DrivableArea: the raster of %s must be [H, W] with H, W >= 1, got %s" % (self.cities[i], mat.shape))
            if se2.shape != (3, 3) or not np.isfinite(se2).all():
                raise LgcnError("DrivableArea: se2 of %s must be a finite 3 x 3 matrix" % self.cities[i])
            t = self.table[i]
            t.off, t.h, t.w = off, mat.shape[0], mat.shape[1]
            t.m[:] = [float(x) for x in se2[:2].reshape(-1)]
            flat.append(np.ascontiguousarray(mat == 1).reshape(-1).view(np.uint8))
            off += flat[-1].size
        self.raster = np.concatenate(flat)
        self.raster_dev = self.table_dev = None

    @classmethod
    def from_files(cls, paths: Dict):
        """{city: (path of the raster .npy, path of the se2 .npy)}, each through np.load."""
        return cls({c: (np.load(m), np.load(s)) for c, (m, s) in paths.items()})

    def to(self, device):
        """Copy the rasters and the city table to `device` (once per device); returns self."""
        device = torch.device(device)
        if device.type == "cuda" and device.index is None:
            device = torch.device("cuda", torch.cuda.current_device())
        if self.raster_dev is None or self.raster_dev.device != device:
            self.raster_dev = torch.from_numpy(self.raster).to(device)
            self.table_dev = torch.from_numpy(np.frombuffer(self.table, dtype=np.uint8).copy()).to(device)
        return self

    def city_id(self, city) -> int:
        """The id of a city name or id; -1 for None / -1 (no map).  LgcnError for a name or an id that is not held."""
        if city is None:
            return -1
        if isinstance(city, (str, bytes, np.str_)):
            city = city.decode() if isinstance(city, bytes) else str(city)
            if city not in self.cities:
                raise LgcnError("DrivableArea: no city %r (have %s)" % (city, self.cities))
            return self.cities.index(city)
        c = int(city)
        if c != city or not -1 <= c < len(self.cities):
            raise LgcnError("DrivableArea: a city id must lie in -1..%d, got %r" % (len(self.cities) - 1, city))
        return c

    def scene_cities(self, scene_city, n_scenes: int) -> np.ndarray:
        """`scene_city` (one name, id or None per scene) as the int32 [n_scenes] ids the kernels read."""
        if scene_city is None or len(scene_city) != n_scenes:
            raise LgcnError("scene_city must hold one entry per scene (%d), got %s"
                            % (n_scenes, "none" if scene_city is None else len(scene_city)))
        return np.array([self.city_id(c) for c in scene_city], dtype=np.int32).reshape(n_scenes)

    def inside(self, points, city) -> np.ndarray:
        """points [..., 2] (fp32, world frame) -> bool [...]: the host lookup, the kernels' rule in numpy."""
        c = self.city_id(city)
        p = np.asarray(points, dtype=np.float32)
        if c < 0:
            return np.zeros(p.shape[:-1], dtype=bool)
        t = self.table[c]
        m = list(t.m)
        r = np.rint(p).astype(np.float64)
        with np.errstate(all="ignore"):
            iu = np.trunc(r[..., 0] * m[0] + r[..., 1] * m[1] + m[2])
            iv = np.trunc(r[..., 0] * m[3] + r[..., 1] * m[4] + m[5])
            ok = (iu > 0) & (iu < t.w) & (iv > 0) & (iv < t.h)
            at = np.where(ok, iv * t.w + iu, 0.0).astype(np.int64)
        return ok & (self.raster[t.off + at] != 0)


class Evaluator:
    """The record table of a split of `n_scenes` scenes (row = scene index) and, with keep_preds, the agent's num_mods
    trajectories and scores per scene.  `horizon`: the steps that count (default: all num_preds); `miss_thr`: a miss is
    minFDE > miss_thr metres.  The buffers live on `device` (default: the current GPU; "cpu" holds tables to merge only)."""

    def __init__(self, n_scenes: int, num_mods: int, num_preds: int, horizon: Optional[int] = None, miss_thr: float = 2.0,
                 keep_preds: bool = False, device=None, drivable: Optional[DrivableArea] = None, scene_city=None):
        horizon = num_preds if horizon is None else horizon
        if n_scenes < 0 or not 1 <= num_mods <= ops.EVAL_MAX_MOD or not 1 <= num_preds <= 64 or not 1 <= horizon <= num_preds:
            raise LgcnError("Evaluator: need n_scenes >= 0, 1 <= num_mods <= 8, 1 <= horizon <= num_preds <= 64, got %s"
                            % ((n_scenes, num_mods, num_preds, horizon),))
        self.n_scenes, self.num_mods, self.num_preds, self.horizon = int(n_scenes), int(num_mods), int(num_preds), int(horizon)
        self.miss_thr, self.keep_preds = float(miss_thr), bool(keep_preds)
        self.device = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
        self.drivable, self.scene_city = drivable, None
        if drivable is not None:
            self.scene_city = drivable.scene_cities(scene_city, self.n_scenes)
            if self.device.type == "cuda":
                drivable.to(self.device)
        elif scene_city is not None:
            raise LgcnError("%s: scene_city without a DrivableArea" % type(self).__name__)
        self._tables(self._n_rows())

    def _n_rows(self) -> int:
        return self.n_scenes

    def _tables(self, n_rows: int) -> None:
        f32 = dict(dtype=torch.float32, device=self.device)
        self.rec = torch.zeros((n_rows, ops.EVAL_REC), **f32)
        self.traj = torch.zeros((n_rows, self.num_mods, self.num_preds, 2), **f32) if self.keep_preds else None
        self.score = torch.zeros((n_rows, self.num_mods), **f32) if self.keep_preds else None
        st = self._status = torch.zeros(_STATUS_BYTES if self.drivable is None else _STATUS_BYTES_DAC, dtype=torch.uint8,
                                        device=self.device)
        self._out = st[:_AT_CNT].view(torch.float64).view(ops.EVAL_MAX_MOD, 6)
        self._cnt = st[_AT_CNT:_AT_CNT + 24].view(torch.int64)
        self._cnt4 = st[_AT_CNT:_AT_CNT + 32].view(torch.int64)
        self._err_slot = st[_AT_ERR_SLOT:_AT_ERR_SLOT + 4].view(torch.int32)
        self._err_mix = st[_AT_ERR_MIX:_AT_ERR_MIX + 4].view(torch.int32)
        self._dac = None if self.drivable is None else st[_AT_DAC:_AT_DAC + 8 * ops.EVAL_DAC_OUT].view(torch.int64)

    def _upload(self, rows: np.ndarray, idx: np.ndarray):
        """The table rows of a batch through pinned memory, as the store's table: one copy that does not synchronise ->
        (rows int64 [B], None) on the device.  With a DrivableArea the same buffer and the same copy also carry the scenes'
        city ids, from a 16-byte boundary behind the rows -> (rows, scene_city[idx] int32 [B])."""
        B = rows.size
        if self.drivable is None:
            stage = torch.empty(B, dtype=torch.int64, pin_memory=True)
            stage.numpy()[:] = rows
            return stage.to(self.device, non_blocking=True), None
        at = (B + 1) // 2 * 2
        stage = torch.empty(at + (B + 1) // 2, dtype=torch.int64, pin_memory=True)
        stage.numpy()[:B] = rows
        ok = (idx >= 0) & (idx < self.n_scenes)              # a scene outside the split has no city; the kernel flags its slot
        stage.numpy()[at:].view(np.int32)[:B] = np.where(ok, self.scene_city[np.where(ok, idx, 0)], -1) if self.n_scenes else -1
        dev = stage.to(self.device, non_blocking=True)
        return dev[:B], dev[at:].view(torch.int32)[:B]

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
            slot, city = self._upload(idx, idx)
            args = (out_reg_flat, out_cls_flat, ex["gt_preds"], ex["has_preds"], fb.actor_off, slot, self.horizon,
                    self.rec, self.traj, self.score, self._err_slot)
            if self.drivable is None:
                ops.eval_scenes(*args)
            else:
                ops.eval_scenes_da(*args, self.drivable, city)

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
        def reduce():
            ops.eval_reduce(self.rec, self.miss_thr, self._out, self._cnt, self._err_mix)
            if self.drivable is not None:          # one more launch into the same buffer; still one read
                ops.eval_dac_reduce(self.rec, 0, ops.EVAL_MAX_T, self._dac)
        return self._summarise(ks, strict, reduce, 3,
                               "a scene index outside [0, %d) or a city id the DrivableArea does not hold was passed to update()" % self.n_scenes
                               if self.drivable is not None else
                               "a scene index outside [0, %d) was passed to update(); its scene was not recorded" % self.n_scenes,
                               "%d scenes were not evaluated (no agent, or its future is not fully observed)")

    def _summarise(self, ks, strict, reduce, n_cnt, slot_msg, skipped_msg) -> Dict:
        """`reduce()` (one launch into the status buffer) and the one read behind every summary; n_cnt: counts it writes."""
        name = type(self).__name__
        ks = [int(k) for k in ks]
        if any(not 1 <= k <= self.num_mods for k in ks):
            raise LgcnError("summary: K must lie in 1..%d, got %s" % (self.num_mods, ks))
        with torch.cuda.device(self.device):
            reduce()
        host = self._status.cpu().numpy()
        if int(host[_AT_ERR_SLOT:_AT_ERR_SLOT + 4].view(np.int32)[0]) != 0:
            raise LgcnError("%s: %s" % (name, slot_msg))
        if int(host[_AT_ERR_MIX:_AT_ERR_MIX + 4].view(np.int32)[0]) != 0:
            raise LgcnError("%s: the table holds records of different num_mods / horizon" % name)
        out = host[:_AT_CNT].view(np.float64).reshape(ops.EVAL_MAX_MOD, 6)
        n_skip, n_eval, n_bad, *rest = (int(c) for c in host[_AT_CNT:_AT_CNT + 8 * n_cnt].view(np.int64))
        if strict and (n_skip or n_bad):
            raise LgcnError(("%s: " + skipped_msg + " and %d hold non-finite values") % (name, n_skip, n_bad))
        res = {}
        for k in ks:
            res[k] = {m: (float(out[k - 1, _COLUMN[m]]) / n_eval if n_eval else float("nan")) for m in METRICS}
        res.update(n_evaluated=n_eval, n_skipped=n_skip, n_nonfinite=n_bad)
        if rest:
            res.update(n_excluded=rest[0])
        if self.drivable is not None:
            dac = [int(c) for c in host[_AT_DAC:_AT_DAC + 8 * ops.EVAL_DAC_OUT].view(np.int64)]
            n_dac = dac[ops.EVAL_MAX_MOD]
            for k in ks:          # DAC_k = mean over the counted records of (compliant modes among the first k) / k
                res[k]["DAC"] = dac[k - 1] / (k * n_dac) if n_dac else float("nan")
            res.update(n_dac=n_dac)
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


class ActorEvaluator(Evaluator):
    """The record table of every actor of a split: row actor_off[s] + i is the i-th actor of scene s (`actor_off`: the
    split's int64 [S + 1] prefix sums, DeviceSceneStore.actor_off).  An actor with at least one observed step t < horizon is
    evaluated over its observed steps (lgcn_eval_actors; include/lgcn.h has the record).  Other arguments as Evaluator."""

    def __init__(self, actor_off, num_mods: int, num_preds: int, horizon: Optional[int] = None, miss_thr: float = 2.0,
                 keep_preds: bool = False, device=None, drivable: Optional[DrivableArea] = None, scene_city=None):
        off = np.ascontiguousarray(actor_off, dtype=np.int64).reshape(-1)
        if off.size < 1 or off[0] != 0 or np.any(np.diff(off) < 0):
            raise LgcnError("ActorEvaluator: actor_off must be prefix sums [S + 1] that start at 0")
        if off.size > 1 and int(np.diff(off).max()) > 1 << 24:
            raise LgcnError("ActorEvaluator: a scene of more than 2^24 actors (the record holds the local index in fp32)")
        self.actor_off, self.n_slots = off, int(off[-1])
        Evaluator.__init__(self, off.size - 1, num_mods, num_preds, horizon, miss_thr, keep_preds, device, drivable, scene_city)

    def _n_rows(self) -> int:
        return self.n_slots

    @classmethod
    def for_store(cls, store, config, **kw):
        """The evaluator of every actor of a flatfile.DeviceSceneStore, sized by `config` (num_mods, num_preds)."""
        kw.setdefault("device", store.device)
        if kw.get("drivable") is not None and kw.get("scene_city") is None:
            kw["scene_city"] = getattr(store, "scene_city", None)
        return cls(store.actor_off, config["num_mods"], config["num_preds"], **kw)

    def update(self, out_reg_flat, out_cls_flat, fb, ex: Dict, indices) -> None:
        """One launch on the current stream: the records of every actor of the batch `fb` / `ex` whose scenes are the rows
        `indices` of the split.  Arguments as Evaluator.update."""
        if "gt_preds" not in ex or "has_preds" not in ex:
            raise LgcnError("ActorEvaluator.update: the batch holds no gt_preds / has_preds to evaluate against")
        idx = np.ascontiguousarray(indices, dtype=np.int64).reshape(-1)
        if idx.size != fb.n_scenes:
            raise LgcnError("ActorEvaluator.update: %d indices for a batch of %d scenes" % (idx.size, fb.n_scenes))
        if idx.size and (int(idx.min()) < 0 or int(idx.max()) >= self.n_scenes):
            raise LgcnError("ActorEvaluator.update: a scene index outside [0, %d)" % self.n_scenes)
        A = fb.n_actors
        if tuple(out_reg_flat.shape) != (A, self.num_mods, self.num_preds, 2):
            raise LgcnError("ActorEvaluator.update: reg must be %s, got %s"
                            % ((A, self.num_mods, self.num_preds, 2), tuple(out_reg_flat.shape)))
        if A != int((self.actor_off[idx + 1] - self.actor_off[idx]).sum()):
            raise LgcnError("ActorEvaluator.update: the batch holds %d actors, the split's table has %d for these scenes"
                            % (A, int((self.actor_off[idx + 1] - self.actor_off[idx]).sum())))
        with torch.cuda.device(self.device):
            base, city = self._upload(self.actor_off[idx], idx)
            args = (out_reg_flat, out_cls_flat, ex["gt_preds"], ex["has_preds"], fb.actor_off, base, self.horizon,
                    self.rec, self.traj, self.score, self._err_slot)
            if self.drivable is None:
                ops.eval_actors(*args)
            else:
                ops.eval_actors_da(*args, self.drivable, city)

    def summary(self, ks: Sequence[int] = (6, 1), who: str = "all", min_obs: int = 1, strict: bool = False) -> Dict:
        """One reduce launch and one device-to-host read -> Evaluator.summary's dict over the actors the selection keeps,
        plus n_excluded.  who: "all", "agent" (the first actor of each scene) or "others"; min_obs: an evaluated actor
        counts only with at least that many observed steps (1..horizon; horizon: fully observed futures only).  strict:
        LgcnError unless no kept actor was skipped or non-finite."""
        if who not in ops.EVAL_WHO:
            raise LgcnError("summary: who must be one of %s, got %r" % (sorted(ops.EVAL_WHO), who))
        if not 1 <= int(min_obs) <= self.horizon:
            raise LgcnError("summary: min_obs must lie in 1..%d, got %s" % (self.horizon, min_obs))
        def reduce():
            ops.eval_reduce_sel(self.rec, self.miss_thr, ops.EVAL_WHO[who], self.horizon - int(min_obs), self._out, self._cnt4,
                                self._err_mix)
            if self.drivable is not None:
                ops.eval_dac_reduce(self.rec, ops.EVAL_WHO[who], self.horizon - int(min_obs), self._dac)
        return self._summarise(ks, strict, reduce,
                               4, "update() was given a batch whose actor rows do not match the split's table; some actors were "
                               "not recorded", "%d actors were not evaluated (no observed step, or never recorded)")

    def actor_index(self):
        """(scene [n], local [n]) int64: the scene and the index inside it of every row of the table."""
        scene = np.repeat(np.arange(self.n_scenes, dtype=np.int64), np.diff(self.actor_off))
        return scene, np.arange(self.n_slots, dtype=np.int64) - self.actor_off[scene]


def evaluate_store(net, store, batch_size: int, evaluator: Optional[Evaluator] = None, indices=None, on_batch=None,
                   actors: bool = False, replay: bool = False, drivable: Optional[DrivableArea] = None,
                   scene_city=None) -> Evaluator:
    """Run `net` over the scenes `indices` (default: all) of a flatfile.DeviceSceneStore in batches of `batch_size` (the
    last one may be shorter) and record every scene in `evaluator` (default: a new one for the whole store, sized by
    net.config).  Per batch: store.plan, store.batch, the whole-Net forward of Net.forward_store with its one host read
    and its error behaviour (KeyError / RuntimeError, the pair-capacity regrow, the range guard's re-run), one
    Evaluator.update.  A batch whose scenes hold no actor at all is skipped: its slots stay `not evaluated`.
    `on_batch(out, fb, ex)`, if given, sees every evaluated batch's flat outputs (train_dp.py takes the validation loss there).
    actors=True: the default evaluator is an ActorEvaluator.for_store (every actor of the split); an evaluator passed in, of
    either class, is used as it is.
    replay=True: the full batches are padded to the capacities flatfile.StoreCaps.for_picks finds over them (so every one
    fits) and run through one engine.StoreReplay -- a captured graph replayed per batch; a shorter last batch goes the
    eager way.  Same records; Evaluator.update stays outside the graph.  `replay` may also be a StoreReplay of this net,
    this store and this batch size, to be reused across calls.
    drivable, scene_city: the default evaluator also scores drivable-area compliance (Evaluator's arguments); without
    scene_city the store's own (`store.scene_city`, left there by data_raw.build_store) is taken."""
    if not store.has_gt:
        raise LgcnError("evaluate_store: the store holds no gt_preds / has_preds to evaluate against")
    if batch_size < 1:
        raise LgcnError("evaluate_store: batch_size must be positive")
    if evaluator is not None and (drivable is not None or scene_city is not None):
        raise LgcnError("evaluate_store: drivable / scene_city belong to the evaluator that was passed in")
    if drivable is not None and scene_city is None:
        scene_city = getattr(store, "scene_city", None)
    if evaluator is None and actors:
        evaluator = ActorEvaluator.for_store(store, net.config, drivable=drivable, scene_city=scene_city)
    if evaluator is None:
        evaluator = Evaluator(len(store), net.config["num_mods"], net.config["num_preds"], device=store.device,
                              drivable=drivable, scene_city=scene_city)
    if evaluator.n_scenes != len(store):
        raise LgcnError("evaluate_store: the evaluator holds %d slots for a store of %d scenes" % (evaluator.n_scenes, len(store)))
    if isinstance(evaluator, ActorEvaluator) and not np.array_equal(evaluator.actor_off, store.actor_off):
        raise LgcnError("evaluate_store: the evaluator's actor_off is not the store's")
    idx = np.arange(len(store), dtype=np.int64) if indices is None else np.asarray(indices, dtype=np.int64).reshape(-1)
    if replay is True:
        from .engine import StoreReplay
        from .flatfile import StoreCaps
        full = idx[:len(idx) // batch_size * batch_size].reshape(-1, batch_size)
        replay = StoreReplay(net, store, StoreCaps.for_picks(store, full)) if len(full) else None
    replay = replay or None
    if replay is not None and (replay.net is not net or replay.store is not store):
        raise LgcnError("evaluate_store: the StoreReplay was made for another net or another store")
    with torch.no_grad():
        for i in range(0, len(idx), batch_size):
            pick = idx[i:i + batch_size]
            plan = store.plan(pick)
            if plan.n_actors == 0:
                continue
            if replay is not None and len(pick) == replay.caps.batch:
                fb, ex, out = replay.forward(pick)
            else:
                fb, ex, out = net.forward_store_flat(store, pick, plan=plan)
            evaluator.update(out["reg"], out["cls"], fb, ex, pick)
            if on_batch is not None:
                on_batch(out, fb, ex)
    return evaluator
