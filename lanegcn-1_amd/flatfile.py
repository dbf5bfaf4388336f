"""Flat scene store: the on-disk counterpart of engine.FlatBatch.

The reference keeps preprocessed scenes as a pickle of nested dicts with int16 index arrays
(preprocess_data.py:230-263) and rebuilds batches from ~40 small arrays per scene.  Here a split is ONE
`.npz` of concatenated arrays plus per-scene offset tables; a batch is cut out with a handful of slices and
goes to the device as one copy per array.  Everything is plain numpy (loadable with allow_pickle=False).

Layout (S scenes, R = 2 * num_scales + 2 relations in the order pre0, suc0, ..., left, right):
  node_off [S+1], actor_off [S+1]                      int64 prefix sums of nodes / actors per scene
  node_ctrs, node_feats, turn [N,2]; control, intersect [N]     float32
  actor_ctrs [A,2], actor_feats [A,20,3], rot [S,2,2], orig [S,2]   float32
  gt_preds [A,30,2] float32, has_preds [A,30] bool
  theta [S] float64, only with write_scenes(..., theta=True): the scenes' headings, for the rotation augmentation
  edge_off [R, S+1] int64: edges of relation r of scene s are  u[r][edge_off[r,s]:edge_off[r,s+1]]
  edge_u, edge_v [sum E] int32 (scene-local node indices), stored relation-major: rel_off [R+1]

FlatSceneFile cuts a batch on the host.  DeviceSceneStore keeps the arrays in device memory and cuts the same batch
there with one launch; plan_batch is its host half.  With `rot_dt` both turn the picked scenes as the
reference's rot_aug does (data.py:39-65), the device store inside that same launch.

A DeviceSceneStore is also made on the device: from_arrays wraps existing device tensors (data_raw.build_store ends
there), concat merges stores (merge_tables is its host half; one ops.store_pack launch merges the edge arrays), and save
writes the file that write_scenes would write for the store's scenes.

Padded batches: StoreCaps fixes the sizes of a batch, plan_batch(..., caps=) / batch_padded cut a
pick plus one filler scene to exactly those sizes, and PaddedSlot holds the buffers that every such batch reuses -- what
engine.StoreReplay needs to replay one captured graph for ragged picks.
"""
from dataclasses import dataclass
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np
import torch

from . import ops
from ._lib import LgcnError
from .engine import FlatBatch, _FLAT_ARRAYS

_NODE = ("ctrs", "feats", "turn", "control", "intersect")


def _npy(x):
    return x.numpy() if torch.is_tensor(x) else np.asarray(x)


def _relations(graph) -> List[Dict]:
    rels = []
    for i in range(len(graph["pre"])):
        rels += [graph["pre"][i], graph["suc"][i]]
    return rels + [graph["left"], graph["right"]]


def write_scenes(path: str, scenes: Sequence[Dict], theta: bool = False) -> None:
    """Write scene dicts (reference schema) as one flat store.  theta: also keep every scene's heading `theta` [S]
    float64, which the training rotation (rot_aug_tables) starts from."""
    S = len(scenes)
    graphs = [s["graph"] for s in scenes]
    R = 2 * len(graphs[0]["pre"]) + 2
    node_off = np.zeros(S + 1, np.int64)
    np.cumsum([int(g["num_nodes"]) for g in graphs], out=node_off[1:])
    actor_off = np.zeros(S + 1, np.int64)
    np.cumsum([len(s["ctrs"]) for s in scenes], out=actor_off[1:])
    edge_off = np.zeros((R, S + 1), np.int64)
    us, vs = [[] for _ in range(R)], [[] for _ in range(R)]
    for j, g in enumerate(graphs):
        for r, rel in enumerate(_relations(g)):
            u, v = _npy(rel["u"]).reshape(-1), _npy(rel["v"]).reshape(-1)
            us[r].append(u.astype(np.int32))
            vs[r].append(v.astype(np.int32))
            edge_off[r, j + 1] = edge_off[r, j] + len(u)
    rel_off = np.zeros(R + 1, np.int64)
    np.cumsum(edge_off[:, -1], out=rel_off[1:])
    cat = lambda parts, dt: np.concatenate(parts).astype(dt) if parts else np.zeros(0, dt)
    out = dict(
        num_scales=np.int64(len(graphs[0]["pre"])), node_off=node_off, actor_off=actor_off, edge_off=edge_off,
        rel_off=rel_off,
        edge_u=cat([x for r in range(R) for x in us[r]], np.int32), edge_v=cat([x for r in range(R) for x in vs[r]], np.int32),
        actor_ctrs=cat([_npy(s["ctrs"]) for s in scenes], np.float32),
        actor_feats=cat([_npy(s["feats"]) for s in scenes], np.float32),
        rot=np.stack([_npy(s["rot"]) for s in scenes]).astype(np.float32),
        orig=np.stack([_npy(s["orig"]) for s in scenes]).astype(np.float32),
    )
    for k in _NODE:
        out["node_" + k if k in ("ctrs", "feats") else k] = cat([_npy(g[k]) for g in graphs], np.float32)
    if "gt_preds" in scenes[0]:
        out["gt_preds"] = cat([_npy(s["gt_preds"]) for s in scenes], np.float32)
        out["has_preds"] = cat([_npy(s["has_preds"]) for s in scenes], bool)
    if theta:
        out["theta"] = np.array([float(s["theta"]) for s in scenes], np.float64)
    np.savez(path, **out)


def rot_aug_tables(theta, dt):
    """The reference's training rotation (data.py:45-54) of B picked scenes with headings `theta`, turned by `dt` (both
    float64 [B]) -> (theta' = theta + dt float64 [B], aug float32 [B, 8]): per scene Rm = the rotation by -dt, row-major,
    then rot' = the rotation by theta', row-major -- each entry a float64 cos / sin rounded to float32, as the reference
    forms them.  The table lgcn_store_gather_aug reads."""
    theta, dt = np.asarray(theta, np.float64).reshape(-1), np.asarray(dt, np.float64).reshape(-1)
    new = theta + dt
    aug = np.empty((len(dt), 8), np.float32)
    aug[:, 0], aug[:, 1], aug[:, 2], aug[:, 3] = np.cos(-dt), -np.sin(-dt), np.sin(-dt), np.cos(-dt)
    aug[:, 4], aug[:, 5], aug[:, 6], aug[:, 7] = np.cos(new), -np.sin(new), np.sin(new), np.cos(new)
    return new, aug


def draw_rot_dt(n: int, rot_size: float, rng=None) -> np.ndarray:
    """`n` angles rand() * rot_size (data.py:45), one per picked scene in pick order.  rng=None draws from np.random, one
    np.random.rand() per scene: a seeded global generator gives the reference's sequence for scenes visited in that
    order.  Otherwise `rng` is a np.random.Generator."""
    if rng is None:
        return np.array([np.random.rand() * rot_size for _ in range(int(n))], np.float64)
    return rng.random(int(n)) * rot_size


def _pick_aug(theta, idx, rot_dt):
    """The rot_dt rules of both batch() methods, before anything is launched -> rot_aug_tables of the pick."""
    try:
        dt = np.asarray(rot_dt, np.float64)
    except (TypeError, ValueError):
        raise ValueError("store: rot_dt must be a sequence of finite floats") from None
    if dt.ndim != 1 or len(dt) != len(idx) or not np.isfinite(dt).all():
        raise ValueError("store: rot_dt must hold one finite angle per picked scene (%d)" % len(idx))
    if theta is None:
        raise LgcnError("store: rot_dt needs the scenes' theta; write the store with write_scenes(..., theta=True)")
    return rot_aug_tables(theta[np.asarray(idx, np.int64)], dt)


def _turn(xy: np.ndarray, rm: np.ndarray) -> np.ndarray:
    """Rows (x, y) of float32 `xy` [..., 2] times Rm (`rm` [..., 4] row-major, broadcast): two rounded float32 products
    and one float32 add per output -- the arithmetic of the gather kernel, bit for bit."""
    x, y = xy[..., 0], xy[..., 1]
    return np.stack([x * rm[..., 0] + y * rm[..., 2], x * rm[..., 1] + y * rm[..., 3]], -1)


class FlatSceneFile:
    """Read side: `batch(indices)` cuts a FlatBatch (+ actor tracks) for any list of scene indices."""

    def __init__(self, path: str):
        with np.load(path, allow_pickle=False) as z:
            self.a = {k: z[k] for k in z.files}
        self.n_scenes = len(self.a["node_off"]) - 1
        self.num_scales = int(self.a["num_scales"])
        self.theta = np.asarray(self.a["theta"], np.float64) if "theta" in self.a else None

    def __len__(self):
        return self.n_scenes

    def _rows(self, off, idx):
        return np.concatenate([np.arange(off[i], off[i + 1]) for i in idx]) if len(idx) else np.zeros(0, np.int64)

    def batch(self, indices: Sequence[int], device=None, rot_dt=None):
        """-> (FlatBatch, extras) with extras = {actor_feats [A,3,20], rot [A,2,2], orig [A,2], sizes,
        gt_preds, has_preds}: everything FullNetEngine / HotPathEngine need, no per-scene dicts.
        rot_dt: one angle per picked scene; the scenes come out turned as the reference's rot_aug turns them
        (rot_aug_tables, _turn), rot is rot' and extras["theta"] holds the new headings (host float64 [B])."""
        a = self.a
        idx = list(indices)
        theta_new, aug = (None, None) if rot_dt is None else _pick_aug(self.theta, idx, rot_dt)
        dev = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
        up = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(dev)
        n_nodes = np.array([a["node_off"][i + 1] - a["node_off"][i] for i in idx], np.int64)
        n_act = np.array([a["actor_off"][i + 1] - a["actor_off"][i] for i in idx], np.int64)
        node_off = np.zeros(len(idx) + 1, np.int64)
        np.cumsum(n_nodes, out=node_off[1:])
        actor_off = np.zeros(len(idx) + 1, np.int64)
        np.cumsum(n_act, out=actor_off[1:])
        nrow, arow = self._rows(a["node_off"], idx), self._rows(a["actor_off"], idx)
        R = a["edge_off"].shape[0]
        pieces, seg_len, seg_base, rel_slices, n_edges = [], [], [], [], []
        pos = 0
        for r in range(R):
            spans = []
            for which in ("edge_u", "edge_v"):
                begin = pos
                for j, i in enumerate(idx):
                    lo, hi = a["rel_off"][r] + a["edge_off"][r, i], a["rel_off"][r] + a["edge_off"][r, i + 1]
                    pieces.append(a[which][lo:hi].astype(np.int64))
                    seg_len.append(hi - lo)
                    seg_base.append(node_off[j])
                    pos += hi - lo
                spans.append((int(begin), int(pos)))
            rel_slices.append((spans[0], spans[1]))
            n_edges.append(spans[0][1] - spans[0][0])
        seg_off = np.zeros(len(seg_len) + 1, np.int64)
        np.cumsum(seg_len, out=seg_off[1:])
        rep = np.repeat(np.asarray(idx), n_act)
        node_ctrs, node_feats, actor_ctrs = a["node_ctrs"][nrow], a["node_feats"][nrow], a["actor_ctrs"][arow]
        actor_feats, rot = a["actor_feats"][arow], a["rot"][rep]
        if aug is not None:
            by_node, by_actor = np.repeat(aug, n_nodes, 0), np.repeat(aug, n_act, 0)
            node_ctrs, node_feats = _turn(node_ctrs, by_node[:, :4]), _turn(node_feats, by_node[:, :4])
            actor_ctrs = _turn(actor_ctrs, by_actor[:, :4])
            actor_feats[:, :, :2] = _turn(actor_feats[:, :, :2], by_actor[:, None, :4])     # (fancy indexing made a copy)
            rot = by_actor[:, 4:].reshape(-1, 2, 2)
        fb = FlatBatch(
            n_scenes=len(idx), n_nodes=int(node_off[-1]), n_actors=int(actor_off[-1]), num_scales=self.num_scales,
            node_ctrs=up(node_ctrs), node_feats=up(node_feats), turn=up(a["turn"][nrow]),
            control=up(a["control"][nrow]), intersect=up(a["intersect"][nrow]), actor_ctrs=up(actor_ctrs),
            node_off=up(node_off.astype(np.int32)), actor_off=up(actor_off.astype(np.int32)),
            idx_local=up(np.concatenate(pieces) if pieces else np.zeros(0, np.int64)), seg_off=up(seg_off),
            seg_base=up(np.asarray(seg_base, np.int64)), rel_slices=rel_slices,
            cap_a2m=int(np.dot(n_nodes, n_act)), cap_a2a=int(np.dot(n_act, n_act)), n_edges=n_edges,
            node_sizes=n_nodes.tolist())
        extras = {"actor_feats": up(actor_feats.transpose(0, 2, 1)), "rot": up(rot),
                  "orig": up(a["orig"][rep]), "sizes": [int(x) for x in n_act]}
        if "gt_preds" in a:
            extras["gt_preds"], extras["has_preds"] = up(a["gt_preds"][arow]), up(a["has_preds"][arow])
        if aug is not None:
            extras["theta"] = theta_new
        return fb, extras


@dataclass
class StorePlan:
    """Everything of one batch that is not an array (the non-array fields of FlatBatch + `sizes`), and the table that
    lgcn_store_gather reads (include/lgcn.h): int64, node_off [B+1], actor_off [B+1], node_src [B], actor_src [B],
    scene [B], seg_off [G+1], seg_src [G] with G = 2 * n_rel * B segments ordered (relation, u|v, scene)."""
    n_scenes: int
    n_nodes: int
    n_actors: int
    num_scales: int
    rel_slices: List[tuple]
    n_edges: List[int]
    cap_a2m: int
    cap_a2a: int
    sizes: List[int]
    n_rel: int
    n_elem: int
    table: np.ndarray
    # a padded plan (plan_batch(..., caps=)): n_scenes counts the filler scene, the totals above are the capacities, and
    # these are the totals of the picked scenes alone
    real_nodes: Optional[int] = None
    real_actors: Optional[int] = None
    real_edges: Optional[List[int]] = None

    @property
    def n_seg(self) -> int:
        return 2 * self.n_rel * self.n_scenes

    @property
    def node_off(self) -> np.ndarray:
        return self.table[:self.n_scenes + 1]

    @property
    def actor_off(self) -> np.ndarray:
        return self.table[self.n_scenes + 1:2 * self.n_scenes + 2]

    @property
    def seg_off(self) -> np.ndarray:
        at = 5 * self.n_scenes + 2
        return self.table[at:at + self.n_seg + 1]

    @property
    def seg_base(self) -> np.ndarray:
        return np.tile(self.node_off[:-1], 2 * self.n_rel)


_I32_MAX = 2 ** 31 - 1


def _tables(src):
    """(node_off, actor_off, edge_off) int64 of a store or of anything that holds its tables as keys or attributes."""
    get = (lambda k: src[k]) if isinstance(src, dict) or hasattr(src, "files") else (lambda k: getattr(src, k))
    return tuple(np.asarray(get(k), np.int64) for k in ("node_off", "actor_off", "edge_off"))


def _pick_totals(tables, picks):
    """Totals of every pick of `picks` [P, B] (scene indices): nodes [P], actors [P], edges [P, R]."""
    node_off, actor_off, edge_off = tables
    picks = np.asarray(picks, np.int64)
    return ((node_off[picks + 1] - node_off[picks]).sum(1), (actor_off[picks + 1] - actor_off[picks]).sum(1),
            (edge_off[:, picks + 1] - edge_off[:, picks]).sum(2).T)


class StoreFitError(LgcnError):
    """A pick that does not fit a StoreCaps (its length, or a total beyond a capacity)."""


@dataclass(frozen=True)
class StoreCaps:
    """Fixed sizes of a PADDED batch: `batch` picked scenes plus one filler scene hold exactly
    `nodes` nodes, `actors` actors and `edges[r]` edges in relation r.  A pick of totals N, A, E_r fits when it has `batch`
    scenes, N + 1 <= nodes, A + 1 <= actors (the filler always owns one node and one actor) and E_r <= edges[r].  The
    constructors return the exact maxima, not rounded up."""
    batch: int
    nodes: int
    actors: int
    edges: Tuple[int, ...]

    @classmethod
    def _over(cls, tables, picks):
        picks = np.asarray(picks, np.int64)
        if picks.ndim != 2 or picks.shape[0] == 0 or picks.shape[1] == 0:
            raise LgcnError("StoreCaps: picks must be a non-empty list of picks of one positive length")
        S = len(tables[0]) - 1
        if int(picks.min()) < 0 or int(picks.max()) >= S:
            raise IndexError("store: scene index outside [0, %d)" % S)
        n, a, e = _pick_totals(tables, picks)
        return cls(batch=int(picks.shape[1]), nodes=int(n.max()) + 1, actors=int(a.max()) + 1,
                   edges=tuple(int(x) for x in e.max(0)))

    @classmethod
    def for_picks(cls, store_or_tables, picks) -> "StoreCaps":
        """The smallest capacities that every pick of `picks` (each of the same length B) fits."""
        return cls._over(_tables(store_or_tables), picks)

    @classmethod
    def for_size(cls, store_or_tables, batch_size: int, draws: int = 1000, seed: int = 0) -> "StoreCaps":
        """for_picks over `draws` picks of `batch_size` scenes drawn uniformly (with repeats) by default_rng(seed): the
        same capacities for the same arguments.  A later pick may still exceed them (it then does not fit)."""
        tables = _tables(store_or_tables)
        if int(batch_size) < 1 or int(draws) < 1:
            raise LgcnError("StoreCaps.for_size: batch_size and draws must be positive")
        picks = np.random.default_rng(seed).integers(0, len(tables[0]) - 1, (int(draws), int(batch_size)))
        return cls._over(tables, picks)

    def misfit(self, n_scenes: int, nodes: int, actors: int, edges) -> Optional[str]:
        """What of a pick with these totals does not fit (None: it fits)."""
        if n_scenes != self.batch:
            return "%d scenes for a batch of %d" % (n_scenes, self.batch)
        if len(edges) != len(self.edges):
            return "%d relations for capacities of %d" % (len(edges), len(self.edges))
        if nodes + 1 > self.nodes:
            return "%d nodes (+ 1 of the filler) for a capacity of %d" % (nodes, self.nodes)
        if actors + 1 > self.actors:
            return "%d actors (+ 1 of the filler) for a capacity of %d" % (actors, self.actors)
        for r, (e, cap) in enumerate(zip(edges, self.edges)):
            if e > cap:
                return "%d edges in relation %d for a capacity of %d" % (e, r, cap)
        return None


def plan_batch(node_off, actor_off, edge_off, rel_off, num_scales: int, indices, caps: Optional[StoreCaps] = None) -> StorePlan:
    """Host half of DeviceSceneStore.batch: from a store's offset tables (the arrays of the same names in the file) and
    the picked scenes to a StorePlan.  Vectorised numpy over small tables; needs no GPU.
    caps: the plan of the PADDED batch -- the picked scenes and, last, the filler scene that brings every total to its
    capacity (its table entries: source -1).  rel_slices are then the fixed blocks of caps.edges[r] elements, sizes has
    B + 1 entries, real_nodes / real_actors / real_edges are the picked scenes' totals.  StoreFitError (an LgcnError) names
    what does not fit."""
    if len(indices) == 0:
        raise LgcnError("store: an empty pick has no batch")
    idx = np.asarray(indices)
    if idx.ndim != 1 or idx.dtype.kind not in "iu":
        raise TypeError("store: indices must be a flat sequence of integers")
    idx = idx.astype(np.int64, copy=False)
    S = len(node_off) - 1
    if int(idx.min()) < 0 or int(idx.max()) >= S:
        raise IndexError("store: scene index outside [0, %d)" % S)
    R = int(edge_off.shape[0])
    node_src, actor_src, scene = node_off[idx], actor_off[idx], idx
    n_nodes, n_act = node_off[idx + 1] - node_src, actor_off[idx + 1] - actor_src
    lo = edge_off[:, idx]                                               # [R, B]
    seg_len, seg_src = edge_off[:, idx + 1] - lo, lo + np.asarray(rel_off)[:R, None]
    real = {}
    if caps is not None:
        N, A, E = int(n_nodes.sum()), int(n_act.sum()), seg_len.sum(1)
        why = caps.misfit(len(idx), N, A, E.tolist())
        if why is not None:
            raise StoreFitError("store: the pick does not fit the capacities: " + why)
        real = dict(real_nodes=N, real_actors=A, real_edges=[int(e) for e in E])
        minus = np.array([-1], np.int64)
        node_src, actor_src, scene = (np.concatenate([x, minus]) for x in (node_src, actor_src, scene))
        n_nodes, n_act = np.append(n_nodes, caps.nodes - N), np.append(n_act, caps.actors - A)
        seg_len = np.concatenate([seg_len, (np.asarray(caps.edges, np.int64) - E)[:, None]], 1)
        seg_src = np.concatenate([seg_src, np.full((R, 1), -1, np.int64)], 1)
    B = len(scene)
    G = 2 * R * B
    tab = np.empty(5 * B + 2 * G + 3, np.int64)
    t_node_off, t_actor_off = tab[:B + 1], tab[B + 1:2 * B + 2]
    t_node_src, t_actor_src, t_scene = tab[2 * B + 2:3 * B + 2], tab[3 * B + 2:4 * B + 2], tab[4 * B + 2:5 * B + 2]
    t_seg_off, t_seg_src = tab[5 * B + 2:5 * B + G + 3], tab[5 * B + G + 3:]
    t_node_src[:], t_actor_src[:], t_scene[:] = node_src, actor_src, scene
    t_node_off[0] = t_actor_off[0] = t_seg_off[0] = 0
    np.cumsum(n_nodes, out=t_node_off[1:])
    np.cumsum(n_act, out=t_actor_off[1:])
    t_seg_src.reshape(R, 2, B)[:] = seg_src[:, None, :]
    np.cumsum(np.broadcast_to(seg_len[:, None, :], (R, 2, B)).reshape(-1), out=t_seg_off[1:])
    total_n, total_a, n_elem = int(t_node_off[-1]), int(t_actor_off[-1]), int(t_seg_off[-1])
    if total_n > _I32_MAX or 60 * total_a > _I32_MAX or n_elem > _I32_MAX or G > _I32_MAX:
        raise LgcnError("store: a batch of %d nodes, %d actors and %d index elements is past 32-bit offsets"
                        % (total_n, total_a, n_elem))
    cut = t_seg_off[::B].tolist()                                       # the 2 R + 1 ends of the u / v blocks
    rel_slices = [((cut[2 * r], cut[2 * r + 1]), (cut[2 * r + 1], cut[2 * r + 2])) for r in range(R)]
    return StorePlan(
        n_scenes=B, n_nodes=total_n, n_actors=total_a, num_scales=int(num_scales), rel_slices=rel_slices,
        n_edges=[u[1] - u[0] for u, _ in rel_slices], cap_a2m=int(np.dot(n_nodes, n_act)), cap_a2a=int(np.dot(n_act, n_act)),
        sizes=n_act.tolist(), n_rel=R, n_elem=n_elem, table=tab, **real)


def merge_tables(parts) -> Dict:
    """Host half of DeviceSceneStore.concat: the tables of the store that holds the scenes of `parts` in part order.
    A part is anything with node_off, actor_off, edge_off, rel_off, num_scales and (optionally, None = absent) theta as
    keys or as attributes: a DeviceSceneStore, FlatSceneFile(path).a, a loaded `.npz`.  Returns node_off, actor_off,
    edge_off, rel_off, num_scales, theta (None if the parts have none) and the runs that merge the parts' edge_u (or
    edge_v, the same runs) relation-major: seg_part, seg_at, seg_len [R * P] int64 in the order (relation, part) -- run k is
    edge_u of part seg_part[k] from seg_at[k] on.  LgcnError for an empty list, parts that differ in num_scales or in
    having theta.  Plain numpy; needs no GPU."""
    def get(p, k):
        if isinstance(p, dict) or hasattr(p, "files"):
            return p[k] if k in p else None
        return getattr(p, k, None)
    parts = list(parts)
    if not parts:
        raise LgcnError("store: concat of an empty list")
    scales = [int(get(p, "num_scales")) for p in parts]
    if len(set(scales)) != 1:
        raise LgcnError("store: concat of parts with different num_scales: %s" % sorted(set(scales)))
    thetas = [get(p, "theta") for p in parts]
    if len({t is None for t in thetas}) != 1:
        raise LgcnError("store: concat of parts with and without theta")
    R = 2 * scales[0] + 2
    i64 = lambda p, k: np.asarray(get(p, k), np.int64)
    for p in parts:
        if i64(p, "edge_off").shape[0] != R or i64(p, "rel_off").shape != (R + 1,):
            raise LgcnError("store: a part's edge tables do not hold 2 * num_scales + 2 relations")
    ends = {k: np.stack([i64(p, k)[..., -1] for p in parts]) for k in ("node_off", "actor_off", "edge_off")}    # [P] / [P, R]
    bases = {k: np.cumsum(v, 0) - v for k, v in ends.items()}
    chain = lambda k: np.concatenate([[0]] + [i64(p, k)[1:] + base for p, base in zip(parts, bases[k])])
    node_off, actor_off = chain("node_off"), chain("actor_off")
    edge_off = np.concatenate([np.zeros((R, 1), np.int64)] + [i64(p, "edge_off")[:, 1:] + b[:, None]
                                                             for p, b in zip(parts, bases["edge_off"])], 1)
    rel_off = np.zeros(R + 1, np.int64)
    np.cumsum(edge_off[:, -1], out=rel_off[1:])
    rel = np.stack([i64(p, "rel_off") for p in parts], 1)                  # [R + 1, P]
    return dict(node_off=node_off, actor_off=actor_off, edge_off=edge_off, rel_off=rel_off, num_scales=scales[0],
                theta=None if thetas[0] is None else np.concatenate([np.asarray(t, np.float64).reshape(-1) for t in thetas]),
                seg_part=np.tile(np.arange(len(parts), dtype=np.int64), R), seg_at=rel[:-1].reshape(-1).copy(),
                seg_len=np.diff(rel, axis=0).reshape(-1))


def _carve(spec, device):
    """One device byte buffer that holds the arrays (name, dtype, shape) of `spec` in order, each at a 256-byte aligned
    offset (the layout of engine.collate_flat_host), and the arrays as views of it."""
    at, off = [], 0
    for _, dt, shp in spec:
        at.append(off)
        off = (off + int(np.prod(shp)) * dt.itemsize + 255) & ~255
    buf = torch.empty(max(off, 256), dtype=torch.uint8, device=device)
    typed, views = {}, {}
    for (name, dt, shp), o in zip(spec, at):
        if dt not in typed:
            typed[dt] = buf.view(dt)
        strides, step = [], 1
        for d in reversed(shp):
            strides.append(step)
            step *= d
        # one op per array (a slice, a dtype view and a reshape are three, and sixteen arrays make them the call's cost)
        views[name] = typed[dt].as_strided(shp, strides[::-1], o // dt.itemsize)
    return buf, views


def _batch_spec(B, N, A, E, G, has_gt):
    """(name, dtype, shape) of the arrays of a batch's two carved buffers: the FlatBatch arrays and the extras."""
    f32, i32, i64 = torch.float32, torch.int32, torch.int64
    flat = (("node_ctrs", f32, (N, 2)), ("node_feats", f32, (N, 2)), ("turn", f32, (N, 2)), ("control", f32, (N,)),
            ("intersect", f32, (N,)), ("actor_ctrs", f32, (A, 2)), ("node_off", i32, (B + 1,)),
            ("actor_off", i32, (B + 1,)), ("idx_local", i64, (E,)), ("seg_off", i64, (G + 1,)), ("seg_base", i64, (G,)))
    assert tuple(n for n, _, _ in flat) == _FLAT_ARRAYS
    extra = (("actor_feats", f32, (A, 3, 20)), ("rot", f32, (A, 2, 2)), ("orig", f32, (A, 2)))
    if has_gt:
        extra += (("gt_preds", f32, (A, 30, 2)), ("has_preds", torch.bool, (A, 30)))
    return flat, extra


class DeviceSceneStore:
    """A flat store resident in device memory: `batch(indices)` assembles the FlatBatch (+ actor tracks) of any list of
    scenes with one small upload (the offset table of the pick, from pinned memory) and ONE kernel launch
    (ops.store_gather), on the current stream and without synchronising.  Same results as FlatSceneFile.batch, byte for
    byte.  The offset tables stay on the host (numpy); `plan(indices)` is the host half and needs no GPU."""

    def __init__(self, source, device=None):
        source = source if isinstance(source, FlatSceneFile) else FlatSceneFile(source)
        a, self.theta = source.a, source.theta       # theta stays on the host, next to the offset tables
        self.n_scenes = len(a["node_off"]) - 1
        self.num_scales = int(a["num_scales"])
        self.node_off, self.actor_off = np.asarray(a["node_off"], np.int64), np.asarray(a["actor_off"], np.int64)
        self.edge_off, self.rel_off = np.asarray(a["edge_off"], np.int64), np.asarray(a["rel_off"], np.int64)
        self.scene_city = None                       # the file format holds no cities (data_raw.build_store knows them)
        self.lane_arrays = None                      # nor the lane arrays of the fork (data_raw.build_store(..., lanes=True))
        if not torch.cuda.is_available():
            raise LgcnError("DeviceSceneStore needs a GPU (the HIP hot path has no CPU fallback); plan_batch does not")
        self.device = torch.device("cuda" if device is None else device)
        if self.device.index is None:
            self.device = torch.device(self.device.type, torch.cuda.current_device())
        names = list(ops.STORE_FLOATS) + ["edge_u", "edge_v"] + (["gt_preds", "has_preds"] if "gt_preds" in a else [])
        host = {k: np.ascontiguousarray(a[k]) for k in names}
        if "has_preds" in host:
            host["has_preds"] = host["has_preds"].view(np.uint8)
        self._job = ops.StoreJob({k: torch.from_numpy(v).to(self.device) for k, v in host.items()})
        torch.cuda.synchronize(self.device)      # resident before any stream reads it
        self.nbytes = self._job.nbytes

    @classmethod
    def from_arrays(cls, arrays, node_off, actor_off, edge_off, rel_off, num_scales: int, theta=None):
        """A store over device tensors that already exist (nothing is copied; data_raw.build_store and concat end here).
        arrays: the tensors ops.StoreJob takes (has_preds may be bool); node_off, actor_off [S + 1], edge_off [R, S + 1],
        rel_off [R + 1]: the host tables of the file layout; theta: the scenes' headings [S] or None.  The tensors may be
        views of larger allocations: `nbytes` counts the storages they keep alive, once each."""
        self = object.__new__(cls)
        i64 = lambda x: np.ascontiguousarray(x, np.int64)
        self.node_off, self.actor_off, self.edge_off, self.rel_off = i64(node_off), i64(actor_off), i64(edge_off), i64(rel_off)
        self.n_scenes, self.num_scales = len(self.node_off) - 1, int(num_scales)
        self.theta = None if theta is None else np.ascontiguousarray(theta, np.float64).reshape(-1)
        self.scene_city = None                       # a plain attribute, never saved: one city name per scene, or None
        self.lane_arrays = None                      # likewise: the fork's lane arrays, or None
        arrays = dict(arrays)
        if "has_preds" in arrays and arrays["has_preds"].dtype == torch.bool:
            arrays["has_preds"] = arrays["has_preds"].view(torch.uint8)
        self._job = job = ops.StoreJob(arrays)
        self.device = job.device
        R, S, p = 2 * self.num_scales + 2, self.n_scenes, job.p
        if self.edge_off.shape != (R, S + 1) or self.actor_off.shape != (S + 1,) or self.rel_off.shape != (R + 1,) \
                or (self.theta is not None and self.theta.shape != (S,)) or p.n_scenes != S \
                or int(self.node_off[-1]) != p.n_nodes or int(self.actor_off[-1]) != p.n_actors \
                or int(self.rel_off[-1]) != p.n_edges or not np.array_equal(np.diff(self.rel_off), self.edge_off[:, -1]):
            raise LgcnError("store: the offset tables do not describe the arrays")
        held = {t.untyped_storage().data_ptr(): t.untyped_storage().nbytes() for t in job.t.values() if t.numel()}
        self.nbytes = sum(held.values())
        return self

    @classmethod
    def concat(cls, stores):
        """One store that holds the scenes of `stores` in part order: the store of all those scenes written at once.  The
        edge arrays are merged relation-major by ONE ops.store_pack launch over P x 2R runs, every other array by one
        concatenation, the tables on the host (merge_tables).  LgcnError, before any launch: an empty list, parts on
        different devices, with different num_scales, or that differ in having gt_preds or in having theta."""
        stores = list(stores)
        if not stores:
            raise LgcnError("store: concat of an empty list")
        if len({str(s.device) for s in stores}) != 1:
            raise LgcnError("store: concat of parts on different devices")
        if len({bool(s.has_gt) for s in stores}) != 1:
            raise LgcnError("store: concat of parts with and without gt_preds")
        m = merge_tables(stores)
        P, dev = len(stores), stores[0].device
        parts = [s._job.t for s in stores]
        with torch.cuda.device(dev):
            arrays = {k: torch.cat([t[k] for t in parts]) for k in parts[0] if k not in ("edge_u", "edge_v")}
            E = int(m["rel_off"][-1])
            edges = torch.empty(2 * E, dtype=torch.int32, device=dev)
            ops.store_pack([t["edge_u"].reshape(-1) for t in parts] + [t["edge_v"].reshape(-1) for t in parts],
                           np.concatenate([m["seg_part"], m["seg_part"] + P]), np.tile(m["seg_at"], 2), np.tile(m["seg_len"], 2), edges)
        arrays["edge_u"], arrays["edge_v"] = edges[:E], edges[E:]
        self = cls.from_arrays(arrays, m["node_off"], m["actor_off"], m["edge_off"], m["rel_off"], m["num_scales"], m["theta"])
        if all(getattr(s, "scene_city", None) is not None for s in stores):
            self.scene_city = [c for s in stores for c in s.scene_city]
        return self

    def save(self, path: str) -> None:
        """Write the store as the `.npz` that write_scenes(path, scenes, theta=...) writes for its scenes: same keys, dtypes,
        shapes and bytes (theta if the store has it).  One device->host copy per array."""
        t = self._job.t
        out = dict(num_scales=np.int64(self.num_scales), node_off=self.node_off, actor_off=self.actor_off, edge_off=self.edge_off,
                   rel_off=self.rel_off)
        for k, v in t.items():
            out[k] = v.cpu().numpy()
        if "has_preds" in out:
            out["has_preds"] = out["has_preds"].view(bool)
        if self.theta is not None:
            out["theta"] = self.theta
        np.savez(path, **out)

    def __len__(self):
        return self.n_scenes

    @property
    def has_gt(self) -> bool:
        """Whether the store holds gt_preds / has_preds (a training step needs them)."""
        return self._job.has_gt

    def plan(self, indices, caps: Optional[StoreCaps] = None) -> StorePlan:
        return plan_batch(self.node_off, self.actor_off, self.edge_off, self.rel_off, self.num_scales, indices, caps=caps)

    def batch_padded(self, indices, caps: StoreCaps, slot: "PaddedSlot" = None, plan: StorePlan = None):
        """-> (FlatBatch, extras) of the pick PADDED to `caps`: the B picked scenes and one filler scene (DESIGN.md section
        3.10) that brings every total to its capacity -- byte for byte FlatSceneFile.batch(pick + [F]) of a store that also
        holds that filler scene as scene F.  Every padded batch of one `caps` has the same sizes.  slot: a PaddedSlot of
        this store and these capacities, filled in place (one host-to-device copy of the table, one launch, nothing
        allocated; the arrays returned are the slot's, valid until it is filled again); None: a new one.  plan: this
        pick's plan(indices, caps=caps).  StoreFitError when the pick does not fit."""
        p = self.plan(indices, caps=caps) if plan is None else plan
        if p.real_nodes is None:
            raise LgcnError("store: batch_padded needs the plan of a padded batch (plan(indices, caps=caps))")
        slot = PaddedSlot(self, caps) if slot is None else slot
        if slot.store is not self or slot.caps != caps:
            raise LgcnError("store: the slot was made for another store or other capacities")
        with torch.cuda.device(self.device):
            slot.upload(p)
            slot.launch()
        return slot.flat_batch(p), slot.extras(p)

    def batch(self, indices, plan: StorePlan = None, rot_dt=None):
        """-> (FlatBatch, extras) as FlatSceneFile.batch(indices, device, rot_dt) returns them.  The FlatBatch arrays are
        views of one device byte buffer (`buf_view()`) at the 256-byte aligned offsets of engine.HostFlatBatch; the extras
        are views of a second one.  `plan`: this pick's plan(), if the caller already has it.  `rot_dt`: one angle per
        picked scene; the rotation happens inside the same launch, and its table rides in the offset table's upload."""
        p = self.plan(indices) if plan is None else plan
        B, N, A, E, G = p.n_scenes, p.n_nodes, p.n_actors, p.n_elem, p.n_seg
        theta_new, aug = (None, None) if rot_dt is None else _pick_aug(self.theta, p.table[4 * B + 2:5 * B + 2], rot_dt)
        i64, f32 = torch.int64, torch.float32
        flat, extra = _batch_spec(B, N, A, E, G, self._job.has_gt)
        with torch.cuda.device(self.device):
            # the table goes through pinned memory of its own: the host allocator hands a block out again only after the
            # copies queued from it have run, so back-to-back calls never share staging
            # the rotation table, 8 floats = 4 int64 words per scene, rides behind the offset table (from an even word on:
            # 16-byte aligned): still one upload and one launch per batch
            T = p.table.size
            at = T + (T & 1)
            words = T if aug is None else at + 4 * B
            stage = torch.empty(words, dtype=i64, pin_memory=True)
            stage.numpy()[:T] = p.table
            tab_dev = torch.empty(words, dtype=i64, device=self.device)
            tabs = (stage, tab_dev, None, None)
            if aug is not None:
                stage.numpy()[T:at] = 0
                tabs = (stage[:T], tab_dev[:T], stage[at:].view(f32), tab_dev[at:].view(f32))
                tabs[2].numpy()[:] = aug.reshape(-1)
            tab_dev.copy_(stage, non_blocking=True)
            fbuf, out = _carve(flat, self.device)
            out.update(_carve(extra, self.device)[1])
            ops.store_gather(self._job, tabs[0], tabs[1], B, p.n_rel, N, A, E, out, tabs[2], tabs[3])
        fb = FlatBatch(n_scenes=B, n_nodes=N, n_actors=A, num_scales=p.num_scales, rel_slices=p.rel_slices,
                       cap_a2m=p.cap_a2m, cap_a2a=p.cap_a2a, n_edges=p.n_edges, _buf=fbuf,
                       node_sizes=np.diff(p.node_off).tolist(),
                       **{n: out[n] for n in _FLAT_ARRAYS})
        extras = {n: out[n] for n, _, _ in extra}
        extras["sizes"] = list(p.sizes)
        if aug is not None:
            extras["theta"] = theta_new
        return fb, extras


class PaddedSlot:
    """Everything a padded batch of one store and one StoreCaps needs, made once: the pinned stage of the per-batch table,
    the device table, the two carved buffers (FlatBatch arrays, extras) and the launch's arguments.  upload(plan) checks
    the plan's table (lgcn_store_pad_check) and queues its copy to the device; launch() queues the gather.  Both on the
    current stream; neither allocates.  Since all sizes are the capacities, the launch is the same for every pick and can
    be captured in a graph once -- a replay reads whatever table the last upload left on the device.
    Staging rule: the pinned stage is reused, so an event is recorded behind every copy and upload() waits for it on the
    host before it rewrites the stage -- a second upload cannot overwrite words that a queued copy has not read yet."""

    def __init__(self, store: DeviceSceneStore, caps: StoreCaps):
        R = 2 * store.num_scales + 2
        if len(caps.edges) != R or caps.batch < 1 or caps.nodes < 1 or caps.actors < 1 or min(caps.edges) < 0:
            raise LgcnError("store: capacities of %d relations for a store of %d, or a capacity below the filler's one node "
                            "and one actor" % (len(caps.edges), R))
        self.store, self.caps = store, caps
        B1, N, A, E = caps.batch + 1, caps.nodes, caps.actors, 2 * int(sum(caps.edges))
        G = 2 * R * B1
        self._spec = _batch_spec(B1, N, A, E, G, store.has_gt)
        with torch.cuda.device(store.device):
            T = ops.store_table_elems(B1, R)
            self.stage = torch.empty(T, dtype=torch.int64, pin_memory=True)
            self.tab_dev = torch.empty(T, dtype=torch.int64, device=store.device)
            self.buf, self.out = _carve(self._spec[0], store.device)
            self.extra_buf, ex = _carve(self._spec[1], store.device)
            self.out.update(ex)
            # node_off[B] and actor_off[B] of the table: the real scenes' rows, where the range guard reads them
            self.real_rows = (self.tab_dev[B1 - 1:B1], self.tab_dev[2 * B1:2 * B1 + 1])
            self._copied = torch.cuda.Event()
            self._pending = False
            self.job = ops.StorePadJob(store._job, self.tab_dev, B1, R, N, A, E, self.out)

    def upload(self, plan: StorePlan) -> None:
        if plan.real_nodes is None or plan.table.size != self.stage.numel() or plan.n_nodes != self.caps.nodes \
                or plan.n_actors != self.caps.actors or tuple(plan.n_edges) != tuple(self.caps.edges):
            raise LgcnError("store: the plan is not a padded plan of this slot's capacities")
        if self._pending:
            self._copied.synchronize()      # the staging rule: the queued copy has read the stage
        self.stage.numpy()[:] = plan.table
        self.job.check(self.stage)
        self.tab_dev.copy_(self.stage, non_blocking=True)
        self._copied.record()
        self._pending = True

    def launch(self) -> None:
        self.job.launch()

    def flat_batch(self, plan: StorePlan) -> FlatBatch:
        """The padded batch's FlatBatch over the slot's arrays (its host-side fields are the plan's)."""
        return FlatBatch(n_scenes=plan.n_scenes, n_nodes=plan.n_nodes, n_actors=plan.n_actors, num_scales=plan.num_scales,
                         rel_slices=plan.rel_slices, cap_a2m=plan.cap_a2m, cap_a2a=plan.cap_a2a, n_edges=plan.n_edges,
                         _buf=self.buf, node_sizes=np.diff(plan.node_off).tolist(), real_rows=self.real_rows,
                         **{n: self.out[n] for n in _FLAT_ARRAYS})

    def extras(self, plan: StorePlan) -> Dict:
        ex = {n: self.out[n] for n, _, _ in self._spec[1]}
        ex["sizes"] = list(plan.sizes)
        return ex
