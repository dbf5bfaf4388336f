"""Lean forward engine of the hot path: flat, pre-collated device batch in, stage features out.

``collate_flat`` does on the host, once per batch, what the reference spreads over ~1.3 k tiny
H2D copies and casts (utils.gpu / utils.to_long, lanegcn.py:129-134): every per-scene array is
concatenated into one flat buffer and uploaded with one copy per array.  ``HotPathEngine.forward``
then runs graph_gather -> CSR plan -> MapNet -> A2M -> M2M -> M2A -> A2A with no host
synchronisation and no data-dependent host control flow, so the whole forward can be captured in
a hipGraph (``capture``) and replayed with one host call.
"""
from dataclasses import dataclass
from typing import Dict, List, Optional

import os
import time

import numpy as np
import torch

from . import ops
from . import lanegcn as M
from ._lib import LgcnError


@dataclass
class FlatBatch:
    """One batch of scenes, flat and device resident."""
    n_scenes: int
    n_nodes: int
    n_actors: int
    num_scales: int
    node_ctrs: torch.Tensor     # [N,2]
    node_feats: torch.Tensor    # [N,2]
    turn: torch.Tensor          # [N,2]
    control: torch.Tensor       # [N]
    intersect: torch.Tensor     # [N]
    actor_ctrs: torch.Tensor    # [A,2]
    node_off: torch.Tensor      # [B+1] int32
    actor_off: torch.Tensor     # [B+1] int32
    idx_local: torch.Tensor     # [2*sumE] int64: scene-local u/v of every (relation, u|v, scene) segment
    seg_off: torch.Tensor       # [S+1] int64
    seg_base: torch.Tensor      # [S] int64: node offset of the segment's scene
    rel_slices: List[tuple]     # per relation: ((u_begin, u_end), (v_begin, v_end)) into idx_local
    cap_a2m: int                # sum_i n_i * a_i   (upper bound of the pair counts)
    cap_a2a: int                # sum_i a_i * a_i
    n_edges: List[int]
    _buf: Optional[torch.Tensor] = None     # the one device byte buffer the arrays are views of (collate_flat)
    node_sizes: Optional[List[int]] = None  # nodes per scene, on the host (what flat_graph splits by)
    # a padded batch (flatfile.PaddedSlot): (nodes, actors) of its REAL scenes as one-element int64 device tensors (words of
    # the slot's table) -- the range guard looks at those rows only; the filler's rows are never anyone's result
    real_rows: Optional[tuple] = None

    def buf_view(self) -> Optional[torch.Tensor]:
        return self._buf


def flat_graph(fb: FlatBatch) -> Dict:
    """The dict lanegcn.graph_gather returns (idcs, ctrs per scene; feats, turn, control, intersect; pre, suc, left,
    right with int64 global u / v), out of a FlatBatch: one lgcn_graph_gather launch over idx_local, then views.  No
    per-segment host work, no upload and no read-back -- the per-scene sizes are the batch's host-side node_sizes."""
    if fb.node_sizes is None:
        raise LgcnError("flat_graph: the FlatBatch carries no node_sizes (collate_flat and the scene stores set it)")
    g64, _ = ops.graph_gather_indices(fb.idx_local, fb.seg_off, fb.seg_base)
    sizes, ns = list(fb.node_sizes), fb.num_scales
    rel = [{"u": g64[a:b], "v": g64[c:d]} for (a, b), (c, d) in fb.rel_slices]
    return {"idcs": list(torch.split(torch.arange(fb.n_nodes, device=fb.node_ctrs.device), sizes)),
            "ctrs": list(torch.split(fb.node_ctrs, sizes)), "feats": fb.node_feats, "turn": fb.turn, "control": fb.control,
            "intersect": fb.intersect, "pre": rel[0:2 * ns:2], "suc": rel[1:2 * ns:2], "left": rel[2 * ns],
            "right": rel[2 * ns + 1]}


_FLAT_ARRAYS = ("node_ctrs", "node_feats", "turn", "control", "intersect", "actor_ctrs", "node_off", "actor_off",
                "idx_local", "seg_off", "seg_base")


@dataclass
class HostFlatBatch:
    """One batch of scenes, flat, on the HOST: every array of FlatBatch packed at 256-byte aligned offsets into ONE
    byte buffer (pinned when a GPU is present), so that uploading a batch is one host-to-device copy
    (the reference does ~1.3 k per batch, utils.py:74-96).  Built by ``collate_flat_host`` -- plain
    numpy, so a DataLoader worker can do it (``collate_fn`` of this package attaches it as data["_flat"])."""
    buf: torch.Tensor                      # uint8 [nbytes]
    layout: Dict[str, tuple]               # name -> (offset, numpy dtype str, shape)
    meta: Dict                             # the non-array fields of FlatBatch

    def to(self, device=None) -> "FlatBatch":
        """Upload (one copy) and cut the device buffer into FlatBatch views (256-byte aligned)."""
        dev = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
        dbuf = self.buf if dev.type == "cpu" else self.buf.to(dev, non_blocking=True)
        arrs = {}
        for name, (off, dt, shape) in self.layout.items():
            cnt = int(np.prod(shape)) if len(shape) else 1
            tdt = {"float32": torch.float32, "int32": torch.int32, "int64": torch.int64}[dt]
            arrs[name] = dbuf[off:off + cnt * np.dtype(dt).itemsize].view(tdt).view(*shape)
        return FlatBatch(**self.meta, **arrs, _buf=dbuf)


def collate_flat_host(scenes: List[Dict], pin: Optional[bool] = None) -> HostFlatBatch:
    """Host collate of scene dicts (numpy or CPU torch leaves) into one staging buffer."""

    def npy(x):
        return x.numpy() if torch.is_tensor(x) else np.asarray(x)

    graphs = [s["graph"] for s in scenes]
    B = len(scenes)
    ns = len(graphs[0]["pre"])
    n_nodes = np.array([int(g["num_nodes"]) for g in graphs], np.int64)
    n_act = np.array([len(s["ctrs"]) for s in scenes], np.int64)
    node_off = np.zeros(B + 1, np.int64)
    np.cumsum(n_nodes, out=node_off[1:])
    actor_off = np.zeros(B + 1, np.int64)
    np.cumsum(n_act, out=actor_off[1:])

    pieces, seg_len, seg_base, rel_slices, n_edges = [], [], [], [], []
    pos = 0

    def add(getter):
        nonlocal pos
        begin = pos
        for j, g in enumerate(graphs):
            x = npy(getter(g)).astype(np.int64, copy=False).reshape(-1)   # 0-dim guard (lanegcn.py:203-207) + to_long
            pieces.append(x)
            seg_len.append(len(x))
            seg_base.append(node_off[j])
            pos += len(x)
        return (begin, pos)

    keys = []
    for i in range(ns):
        keys += [("pre", i), ("suc", i)]
    for k1, i in keys:
        su = add(lambda g: g[k1][i]["u"])
        sv = add(lambda g: g[k1][i]["v"])
        rel_slices.append((su, sv))
        n_edges.append(su[1] - su[0])
    for k1 in ("left", "right"):
        su = add(lambda g: g[k1]["u"])
        sv = add(lambda g: g[k1]["v"])
        rel_slices.append((su, sv))
        n_edges.append(su[1] - su[0])
    seg_off = np.zeros(len(seg_len) + 1, np.int64)
    np.cumsum(seg_len, out=seg_off[1:])

    cat = lambda key, src: np.concatenate([npy(s[key]) for s in src], 0)
    arrays = {
        "node_ctrs": cat("ctrs", graphs).astype(np.float32, copy=False), "node_feats": cat("feats", graphs).astype(np.float32, copy=False),
        "turn": cat("turn", graphs).astype(np.float32, copy=False), "control": cat("control", graphs).astype(np.float32, copy=False),
        "intersect": cat("intersect", graphs).astype(np.float32, copy=False), "actor_ctrs": cat("ctrs", scenes).astype(np.float32, copy=False),
        "node_off": node_off.astype(np.int32), "actor_off": actor_off.astype(np.int32),
        "idx_local": np.concatenate(pieces) if pieces else np.zeros(0, np.int64),
        "seg_off": seg_off, "seg_base": np.asarray(seg_base, np.int64),
    }
    layout, off = {}, 0
    for name in _FLAT_ARRAYS:
        a = arrays[name]
        layout[name] = (off, str(a.dtype), tuple(a.shape))
        off = (off + a.nbytes + 255) & ~255
    pin = torch.cuda.is_available() if pin is None else pin
    buf = torch.empty(max(off, 256), dtype=torch.uint8, pin_memory=bool(pin))
    view = buf.numpy()
    for name in _FLAT_ARRAYS:
        o, _, _ = layout[name]
        a = np.ascontiguousarray(arrays[name])
        view[o:o + a.nbytes] = a.view(np.uint8).reshape(-1)
    meta = dict(n_scenes=B, n_nodes=int(node_off[-1]), n_actors=int(actor_off[-1]), num_scales=ns,
                rel_slices=rel_slices, cap_a2m=int(np.dot(n_nodes, n_act)), cap_a2a=int(np.dot(n_act, n_act)),
                n_edges=n_edges, node_sizes=n_nodes.tolist())
    return HostFlatBatch(buf, layout, meta)


def collate_flat(scenes: List[Dict], device=None, pin: Optional[bool] = None) -> FlatBatch:
    """Host collate of scene dicts into a FlatBatch on `device`: one staging buffer, ONE host-to-device copy.
    (Round 1 reported that packing the arrays as views of staging buffers halved the throughput of four captured
    forwards in flight; with every view 256-byte aligned in one buffer that does not reproduce: DESIGN.md 5c.)"""
    on_cpu = device is not None and torch.device(device).type == "cpu"
    return collate_flat_host(scenes, pin=False if on_cpu else pin).to(device)


def host_actor_inputs(scenes):
    """[A,3,20] actor tracks (actor_gather, lanegcn.py:155-168) and the per-actor world-frame transform rot [A,2,2] /
    orig [A,2] (the scene's, repeated for its actors) as host tensors + the actors-per-scene list."""
    npy = lambda x: x.numpy() if torch.is_tensor(x) else np.asarray(x)
    feats = np.concatenate([npy(s["feats"]).transpose(0, 2, 1) for s in scenes], 0).astype(np.float32)
    rot = np.concatenate([np.repeat(npy(s["rot"])[None], len(s["ctrs"]), 0) for s in scenes]).astype(np.float32)
    orig = np.concatenate([np.repeat(npy(s["orig"])[None], len(s["ctrs"]), 0) for s in scenes]).astype(np.float32)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a))
    return t(feats), t(rot), t(orig), [len(s["ctrs"]) for s in scenes]


# stage name -> the state key of its output (forward(stages=True) returns them under the stage's name)
_STAGE_OUT = {"map_net": "nodes", "a2m": "nodes_a2m", "m2m": "nodes_m2m", "m2a": "actors_m2a", "a2a": "actors_a2a"}


class HotPathEngine:
    """graph_gather -> MapNet -> A2M -> M2M -> M2A -> A2A on the HIP kernels, sync-free."""

    def __init__(self, map_net: M.MapNet, a2m: M.A2M, m2m: M.M2M, m2a: M.M2A, a2a: M.A2A, config=None,
                 legacy_offsets: bool = True, branches: bool = False, lane_impl: Optional[str] = None):
        self.map_net, self.a2m, self.m2m, self.m2a, self.a2a = map_net, a2m, m2m, m2a, a2a
        self.config = config or M.config
        self.legacy_offsets = legacy_offsets
        # LaneConv implementation (lanegcn.lane_conv): None = the package default ("tiled": weight-stationary row
        # blocks, the faster one for ONE forward at a time); "fused" = one elastic launch per layer, which packs
        # better when several captured forwards share the GPU (bench.py --streams > 1)
        self.lane_impl = lane_impl
        # optional parallel graph branches: the three pair searches (index work that depends only on the centres)
        # and every Att's V GEMM on a side stream, forked / joined with events (captured as graph edges).
        # Measured on MI355X / ROCm 7.2: bitwise the same result, no single-stream gain (38.9 k vs 39.4 k
        # scenes/s) and a loss with four graphs in flight (61 k vs 90 k) -> off by default.
        self.branches = branches
        self._side = None
        self._cnt_capture = None      # counter buffer of the forward being captured (capture(); it lives with the graph)
        # Pair capacities (rows of hi / wi and of every [cap, 128] pair-row buffer of a forward).  "bound": sum_i t_i s_i,
        # can never overflow (265 MB of pair rows per A2M layer at S2, untouched but reserved).  "tight" (default):
        # 1.25 x the largest pair count this engine has seen per set, at least 4,096 (the bound until a count is known)
        # -- learnt by capture() from its eager warm-up forwards (one host read each) and by host_checks() behind
        # forward_guarded() / Net.forward; a forward whose count exceeds it comes back with a negative n_pairs (the
        # kernels keep to the capacity), learn_pair_counts(out) says so and grows the capacity, the caller runs again;
        # a captured graph has to be captured again.
        self.pair_caps = os.environ.get("LGCN_PAIR_CAPS", "tight")
        self._pair_seen = [0, 0, 0]

    def _counters(self, fb: FlatBatch) -> torch.Tensor:
        """Key counters of lgcn_index_build (zero before, zero after).  A captured forward owns a buffer of its own
        (capture() sets it); eager forwards share one per FlatBatch -- do not run two eager forwards of the SAME
        FlatBatch concurrently on different streams."""
        if self._cnt_capture is not None:
            return self._cnt_capture
        cnt = fb.__dict__.get("_idx_cnt")
        if cnt is None:
            cnt = ops.index_counters(fb.n_nodes, len(fb.rel_slices), fb.node_ctrs.device)
            fb.__dict__["_idx_cnt"] = cnt
        return cnt

    @torch.no_grad()
    def forward(self, fb: FlatBatch, actors: torch.Tensor, stages: bool = False,
                mapnet_only: bool = False) -> Dict[str, torch.Tensor]:
        """actors: [A,128] ActorNet output.  Returns {"nodes", "actors"} (+ every stage if stages).
        mapnet_only: stop after MapNet (BASELINE config "MapNet LaneConv only"): graph_gather + plan + MapNet."""
        if mapnet_only:
            st, fns = self.stage_functions(fb, actors, plan_only=True)
            for _, fn in fns[:2]:
                fn()
            return {"nodes": st["nodes"], "actors": actors}
        if self.branches and self._side is None:
            self._side = torch.cuda.Stream()
        st, fns = self.stage_functions(fb, actors, tight=True, counters=self._counters, guard=True,
                                       side=self._side if self.branches else None)
        out = {}
        for name, fn in fns:
            fn()
            if stages and name in _STAGE_OUT:
                out[name] = st[_STAGE_OUT[name]]
        out["nodes"], out["actors"] = st["nodes_m2m"], st["actors_a2a"]
        out["n_pairs"] = [p.n_pairs for p in st["pairs"]]
        # range check of the 16-bit-plane modes, on the device and part of every (captured) forward: bit 0 of
        # out["nonfinite"] is set when a feature row came out NaN / inf (ops.guarded / host_checks act on it)
        ops.check_finite(st["flag"], out["nodes"], out["actors"], rows=fb.real_rows)
        out["nonfinite"] = st["flag"]
        return out

    @torch.no_grad()
    def stage_functions(self, fb: FlatBatch, actors: torch.Tensor, tight: bool = False, counters=None,
                        guard: bool = False, side: Optional[torch.cuda.Stream] = None, plan_only: bool = False):
        """The forward cut at the reference's module boundaries: returns (state, [(name, fn)]); fn() runs one stage on
        the tensors the previous stages left in `state`.  forward() runs them in order; called as (fb, actors) they are
        what a per-stage measurement captures (run them in order once before capturing any of them in a graph): pair
        buffers of the bound capacities and key counters of the stages' own (state["_cnt"]: a stage's captured graph is
        replayed alone).  forward()'s arguments -- tight: pair buffers of the tight capacities; counters: fb -> the
        key-counter buffer; guard: state["flag"], the range guard's word, cleared by the index stage; side: the stream
        of the parallel branches; plan_only: the index stage builds the CSR plan alone (mapnet_only)."""
        cfg, st = self.config, {}
        dev = fb.node_ctrs.device
        main = torch.cuda.current_stream() if side is not None else None
        searches = ((fb.node_ctrs, fb.node_off, fb.actor_ctrs, fb.actor_off, cfg["actor2map_dist"], fb.cap_a2m),
                    (fb.actor_ctrs, fb.actor_off, fb.node_ctrs, fb.node_off, cfg["map2actor_dist"], fb.cap_a2m),
                    (fb.actor_ctrs, fb.actor_off, fb.actor_ctrs, fb.actor_off, cfg["actor2actor_dist"], fb.cap_a2a))
        if tight and self.pair_caps == "tight":      # nothing seen yet for a set: the bound (the first forward cannot overflow)
            searches = tuple(s[:5] + (min(s[5], self._cap(i)) if self._pair_seen[i] > 0 else s[5],) for i, s in enumerate(searches))
        # launches folded across the Att layers of the three blocks (lanegcn.att_block): 7 row-block launches + M2A's
        # ctx-heads; one rule for the whole pipeline
        fold = side is None and M._fold_ok(actors) and fb.n_nodes > 0

        def index():
            if plan_only:
                return gather_plan()
            bufs = [ops.pairs_alloc(s[0].shape[0], fb.n_scenes, s[5], dev) for s in searches]   # on the main stream
            if side is not None:
                side.wait_stream(main)
            if side is None and ops.index_fused_ok(fb.n_nodes, len(fb.rel_slices), sum(fb.n_edges)):
                # graph_gather (lanegcn.py:171-209) + CSR plan + the three pair searches: four launches in all
                if guard:
                    st["flag"] = torch.empty(1, dtype=torch.int32, device=dev)      # cleared by the first launch
                cnt = counters(fb) if counters is not None else st.get("_cnt")
                if cnt is None:
                    cnt = st["_cnt"] = ops.index_counters(fb.n_nodes, len(fb.rel_slices), dev)
                st["plan"], st["pairs"] = ops.index_build(fb.idx_local, fb.seg_off, fb.seg_base, fb.rel_slices, fb.n_nodes,
                                                          searches, self.legacy_offsets, bufs=bufs, cnt=cnt,
                                                          clear_word=st.get("flag"))
                return
            if guard:
                st["flag"] = torch.zeros(1, dtype=torch.int32, device=dev)
            with torch.cuda.stream(side):      # (None: the current stream)
                st["pairs"] = ops.pairs_build_multi(searches, self.legacy_offsets, bufs=bufs)   # three sets, three launches
            gather_plan()

        def gather_plan():
            g64, _ = ops.graph_gather_indices(fb.idx_local, fb.seg_off, fb.seg_base)
            st["plan"] = ops.csr_build([g64[a:b] for (a, b), _ in fb.rel_slices],
                                       [g64[a:b] for _, (a, b) in fb.rel_slices], fb.n_nodes)

        def lane(fuse, feat):
            return M.lane_conv(fuse, feat, st["plan"], fb.num_scales, impl=self.lane_impl)

        def layers(atts, act, ctx, ps):      # the per-layer route; ctx None: the targets are their own context (A2A)
            for att in atts:
                act = att.run(act, act if ctx is None else ctx, ps, side)
            return act

        def map_net():      # lanegcn.py:311-363
            st["nodes"] = lane(self.map_net.fuse, self.map_net.stem(fb.node_ctrs, fb.node_feats))

        def a2m():      # lanegcn.py:385-407
            if fold:      # M2A's U of layer 0 depends on `actors` alone: it rides in A2M's first launch, off M2A's critical path
                st["nodes_a2m"], st["u_m2a"] = self.a2m.run(st["nodes"], fb.turn, fb.control, fb.intersect, actors,
                                                            st["pairs"][0], extra=self.m2a.att[0].u_kw(actors))
                return
            feat = self.a2m.fuse_meta(st["nodes"], fb.turn, fb.control, fb.intersect)
            if side is not None:
                main.wait_stream(side)            # the pair sets are needed from here on
            st["nodes_a2m"], st["u_m2a"] = layers(self.a2m.att, feat, actors, st["pairs"][0]), None

        def m2m():      # lanegcn.py:445-480
            st["nodes_m2m"] = lane(self.m2m.fuse, st["nodes_a2m"])

        def m2a():      # lanegcn.py:502-513
            if fold:
                # M2A's last tail also emits U / V of A2A's first layer (its targets and context are M2A's output rows)
                # (it starts with the V rows of both layers: one weight-stationary launch over the lane nodes)
                st["actors_m2a"], st["uv_a2a"] = M.att_block(self.m2a.att, actors, st["nodes_m2m"], st["pairs"][1],
                                                             next_att=self.a2a.att[0], next_ctx_is_out=True, u0=st["u_m2a"])
                return
            st["actors_m2a"], st["uv_a2a"] = layers(self.m2a.att, actors, st["nodes_m2m"], st["pairs"][1]), None

        def a2a():      # lanegcn.py:534-545
            act = st["actors_m2a"]
            if fold:
                st["actors_a2a"] = M.att_block(self.a2a.att, act, act, st["pairs"][2], uv=st["uv_a2a"], ctx_is_agts=True)[0]
                return
            st["actors_a2a"] = layers(self.a2a.att, act, None, st["pairs"][2])

        return st, [("index", index), ("map_net", map_net), ("a2m", a2m), ("m2m", m2m), ("m2a", m2a), ("a2a", a2a)]

    def _cap(self, i: int) -> int:
        """Tight capacity of pair set i (A2M, M2A, A2A): 1.25 x the largest count seen, at least 4,096, in 1,024s."""
        want = max(4096, int(self._pair_seen[i] * 1.25) + 1)
        return (want + 1023) // 1024 * 1024

    def _record(self, counts) -> bool:
        """Keep the largest magnitude per pair set; True when a count is negative (its capacity was exceeded)."""
        over = False
        for i, c in enumerate(counts):
            over = over or c < 0
            self._pair_seen[i] = max(self._pair_seen[i], abs(int(c)))
        return over

    def learn_pair_counts(self, out: Dict[str, torch.Tensor]) -> bool:
        """Host side of the tight pair capacities: reads the forward's three pair counts (one device->host copy), keeps
        the largest per set; True when a count exceeded its capacity (negative n_pairs: the forward's features are
        those of a truncated pair set and must be recomputed with the grown capacity)."""
        return self._record(torch.stack([c.view(()) for c in out["n_pairs"]]).tolist())

    def host_checks(self, out: Dict, rerun, strict: bool = False, on_regrow=None) -> Dict:
        """The host side of a forward's device-side checks -> the output that passed them.  `out`: a forward's output
        with its range-guard flag ("nonfinite") and pair counts ("n_pairs"): one device->host read of the four words;
        an output without them (the map-only forward) has nothing to check.  rerun() runs the same forward again in
        the matrix mode current at the call and returns its output.
          tight pair capacities: the counts are recorded; a forward that overflowed (negative count: the features of
            a truncated pair set) calls on_regrow() and runs again with the grown capacities;
          range guard (ops.set_guard): an f16x2 forward that left fp16's range runs again in bf16x3, or raises.  The
            re-run has fp32's exponent range in every stage: non-finite values that survive it were in the inputs or
            the weights, and are returned as they are -- what the reference does with them;
          strict: a pair set without a pair raises like torch.cat([]) at the reference's lanegcn.py:688."""
        if "nonfinite" not in out or "n_pairs" not in out:
            return out
        read = lambda o: torch.cat([o["nonfinite"].view(1)] + [c.view(1) for c in o["n_pairs"]]).tolist()
        flag, *counts = read(out)
        if self.pair_caps == "tight" and self._record(counts):
            if on_regrow is not None:
                on_regrow()
            out = rerun()
            flag, *counts = read(out)
            if self._record(counts):
                raise LgcnError("pair capacity still exceeded after growing it")
        if flag != 0 and ops.get_mma() == "f16x2" and ops.get_guard() != "off":
            if ops.get_guard() == "raise":
                raise LgcnError("non-finite features in f16x2 mode: an operand left fp16's range (|x| >= 65520)")
            with ops.mma_scope("bf16x3"):
                out = rerun()
            counts = read(out)[1:]
        if strict and 0 in counts:
            raise RuntimeError("torch.cat(): expected a non-empty list of Tensors")
        return out

    def forward_guarded(self, fb: FlatBatch, actors: torch.Tensor, **kw) -> Dict[str, torch.Tensor]:
        """forward() behind host_checks(): one 16-byte device->host read."""
        return self.host_checks(self.forward(fb, actors, **kw), lambda: self.forward(fb, actors, **kw))

    def capture(self, fb: FlatBatch, actors: torch.Tensor, warmup: int = 2, **fwd_kw):
        """Capture one forward into a hipGraph.  Returns (graph, outputs); ``graph.replay()`` re-runs
        the whole forward on the captured buffers (refill fb's tensors / `actors` in place first)."""
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            for _ in range(max(warmup, 2 if self.pair_caps == "tight" else 0)):
                o = self.forward(fb, actors, **fwd_kw)   # also fills the weight-pack caches outside the capture
                if self.pair_caps == "tight" and not fwd_kw.get("mapnet_only"):
                    self.learn_pair_counts(o)           # the captured buffers are sized for THIS batch's counts x 1.25
        torch.cuda.current_stream().wait_stream(side)
        torch.cuda.synchronize()
        with self.own_counters(fb) as cnt:
            graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graph):
                out = self.forward(fb, actors, **fwd_kw)
        # a graph holds ADDRESSES: the captured inputs (and its counter buffer) must outlive it -- a freed FlatBatch's
        # memory is handed to the next allocation, and the replay then builds its plan from whatever lies there
        graph._lgcn_inputs = (fb, actors, cnt)
        return graph, out

    def own_counters(self, fb: FlatBatch):
        """Context: forwards inside it use a fresh, zeroed counter buffer (yielded: keep it alive as long as what was
        captured) -- for a forward that is being captured: several captured forwards may replay concurrently."""
        import contextlib

        @contextlib.contextmanager
        def cm():
            cnt = ops.index_counters(fb.n_nodes, len(fb.rel_slices), fb.node_ctrs.device)
            torch.cuda.synchronize()         # zeroed before anything captured can run
            prev, self._cnt_capture = self._cnt_capture, cnt
            try:
                yield cnt
            finally:
                self._cnt_capture = prev
        return cm()


class FullNetEngine:
    """Whole Net.forward (lanegcn.py:127-151) on flat device inputs, capturable in one hipGraph: ActorNet (stock
    conv ops) -> hot path (HotPathEngine) -> PredNet (HIP row blocks + stock heads) -> world-frame transform."""

    def __init__(self, net: "M.Net"):
        self.net = net
        self.hot = HotPathEngine(net.map_net, net.a2m, net.m2m, net.m2a, net.a2a, net.config)

    @staticmethod
    def actor_inputs(scenes, device=None):
        """Device copies of host_actor_inputs(scenes): (feats [A,3,20], rot [A,2,2], orig [A,2])."""
        dev = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
        feats, rot, orig, _ = host_actor_inputs(scenes)
        return feats.to(dev), rot.to(dev), orig.to(dev)

    @torch.no_grad()
    def forward(self, fb: FlatBatch, actor_feats: torch.Tensor, rot: torch.Tensor, orig: torch.Tensor,
                sizes: List[int]) -> Dict[str, torch.Tensor]:
        """Returns {"cls": [A,6], "reg": [A,6,30,2]} for all actors of the batch (scene i = rows
        sum(sizes[:i]) .. sum(sizes[:i+1])), reg already in world coordinates."""
        net = self.net
        actors = net.actor_net(actor_feats)
        hot = self.hot.forward(fb, actors)
        actors = hot["actors"]
        if net.pred_net._hip_ok(actors):
            cls, reg = net.pred_net.forward_flat(actors, fb.actor_ctrs, rot, orig)     # world frame inside the last launch
        else:
            idcs, ctrs, st = [], [], 0
            for n in sizes:
                idcs.append(slice(st, st + n))
                ctrs.append(fb.actor_ctrs[st:st + n])
                st += n
            out = net.pred_net(actors, idcs, ctrs)
            reg = torch.cat(out["reg"], 0)
            cls = torch.cat(out["cls"], 0)
            reg = torch.einsum("amtk,akj->amtj", reg, rot) + orig.view(-1, 1, 1, 2)
        res = {"cls": cls, "reg": reg, "nonfinite": hot["nonfinite"]}
        if fb.real_rows is None:
            ops.check_finite(hot["nonfinite"], reg.reshape(-1), cls.reshape(-1), bit=2)      # PredNet's row blocks too
        else:
            ops.check_finite(hot["nonfinite"], reg, cls, bit=2, rows=(fb.real_rows[1], fb.real_rows[1]))
        # device counts of the three pair sets (A2M, M2A, A2A): Att.strict's check and the tight pair capacities
        # (negative = capacity exceeded, HotPathEngine.learn_pair_counts)
        res["n_pairs"] = hot["n_pairs"]
        return res

    def capture(self, fb, actor_feats, rot, orig, sizes, warmup: int = 3, tune_convs: bool = True,
                capture_error_mode: str = "global", **fwd_kw):
        """Capture the whole Net forward.  tune_convs: let MIOpen search its solvers for ActorNet's 17 Conv1d shapes
        during the warm-up (torch.backends.cudnn.benchmark): the shapes of a captured graph are fixed, and the
        default heuristic picks were measured 11 % slower end to end (2.34 vs 2.10 ms per batch)."""
        prev = torch.backends.cudnn.benchmark
        torch.backends.cudnn.benchmark = bool(tune_convs)
        try:
            side = torch.cuda.Stream()
            side.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(side):
                for _ in range(warmup):
                    o = self.forward(fb, actor_feats, rot, orig, sizes, **fwd_kw)
                    if self.hot.pair_caps == "tight" and self.hot.learn_pair_counts(o):      # sized for this batch x 1.25
                        self.forward(fb, actor_feats, rot, orig, sizes, **fwd_kw)
            torch.cuda.current_stream().wait_stream(side)
            torch.cuda.synchronize()
            with self.hot.own_counters(fb) as cnt:
                graph = torch.cuda.CUDAGraph()
                with torch.cuda.graph(graph, capture_error_mode=capture_error_mode):
                    out = self.forward(fb, actor_feats, rot, orig, sizes, **fwd_kw)
            graph._lgcn_inputs = (fb, actor_feats, rot, orig, cnt)      # the graph holds their addresses: keep them alive
        finally:
            torch.backends.cudnn.benchmark = prev
        return graph, out


class StoreReplay:
    """Whole-Net no-grad forwards of picks of a flatfile.DeviceSceneStore through ONE captured graph: every pick is padded
    to the fixed capacities `caps` (flatfile.StoreCaps), so the padded gather and
    FullNetEngine.forward are captured once and replayed for any pick that fits -- per pick one plan, one table check,
    one upload and one graph.replay(), then the one 16-byte host read of the device-side checks.

    forward(indices) -> (fb, ex, out) with the meaning of Net.forward_store_flat, restricted to the REAL rows: fb describes
    the B picked scenes (n_scenes, n_nodes, n_actors, node_off / actor_off [B + 1] and the node / actor arrays cut to the
    real rows; its index arrays -- idx_local, seg_off, seg_base, rel_slices -- stay the padded batch's), ex and out["cls"],
    out["reg"] are views of the first A rows.  They are valid until the next forward() of this object; own=True returns
    clones.  The first `warm` fitting picks (at least one: the weight packs are made outside a capture) run eagerly on
    the padded batch and teach the pair capacities; the next one captures.  A pick that does not fit or has another
    length, a pair capacity exceeded and the range guard's flag send the pick to net.forward_store_flat (which regrows /
    reroutes as ever); after an overflow the graph is dropped and captured again with the grown capacity.  The graph is
    also dropped when the matrix mode, a kernel implementation switch, Att.strict or a parameter's version changes.
    Errors are forward_store's, decided from the real totals before any launch.  `stats` counts the routes (captures,
    replays, eager_warm, eager_nofit, eager_overflow, eager_guard) and holds, as means over the padded runs, the pad share
    (filler rows / capacity) of nodes, actors and edges and the host's milliseconds per pick up to the host read."""

    def __init__(self, net, store, caps, warm: int = 2):
        from .flatfile import PaddedSlot
        self.net, self.store, self.caps = net, store, caps
        self.warm = max(int(warm), 1)
        self.slot = PaddedSlot(store, caps)
        self._graph = self._sig = None
        self._warm_left = self.warm
        self.stats = dict(captures=0, replays=0, eager_warm=0, eager_nofit=0, eager_overflow=0, eager_guard=0,
                          pad_nodes=0.0, pad_actors=0.0, pad_edges=0.0, host_ms=0.0)
        self._padded = 0
        self._pad_sum = [0.0, 0.0, 0.0, 0.0]

    def _signature(self):
        A, N = M.ActorNet, M.PredNet
        return (ops.get_mma(), ops.att_pairs_impl(), ops.laneconv_impl(), M.Att.strict, A.impl, A.exact, N.impl,
                self.net._full_engine().hot.pair_caps, sum(p._version for p in ops.module_params(self.net)))

    def graph_pool_bytes(self) -> int:
        """Bytes allocated in the capture's private memory pool (the graph's buffers; 0 before a capture)."""
        return 0 if self._graph is None else self._graph[3]

    def _padded_batch(self, plan):
        """The padded FlatBatch / extras over the slot's arrays.  Pair capacities: the bound of ANY pick that fits (a
        capture must hold for the next pick too), which the engine cuts to its tight capacity."""
        fb, ex = self.slot.flat_batch(plan), self.slot.extras(plan)
        fb.cap_a2m, fb.cap_a2a = self.caps.nodes * self.caps.actors, self.caps.actors * self.caps.actors
        return fb, ex

    @staticmethod
    def _stable_convs():
        """Context of this object's own forwards, eager and captured: no solver search (tune_convs=False) and MIOpen's
        deterministic solvers only.  Where ActorNet runs on MIOpen (the matrix modes other than f16x2 without
        ActorNet.exact) its default solvers differ from call to call on the same input (1e-6 in the features, 3e-5 in reg
        measured); with this a replayed graph equals the eager forward of the same padded batch bit for bit."""
        import contextlib

        @contextlib.contextmanager
        def cm():
            cd = torch.backends.cudnn
            prev = cd.benchmark, cd.deterministic
            cd.benchmark, cd.deterministic = False, True
            try:
                yield
            finally:
                cd.benchmark, cd.deterministic = prev
        return cm()

    def _capture(self, eng, fb, ex):
        torch.cuda.synchronize()
        before = torch.cuda.memory_allocated()
        with self._stable_convs(), eng.hot.own_counters(fb) as cnt:
            graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graph, capture_error_mode="thread_local"):
                self.slot.launch()
                out = eng.forward(fb, ex["actor_feats"], ex["rot"], ex["orig"], ex["sizes"])
        pool = max(torch.cuda.memory_allocated() - before, 0)      # what the capture's private pool holds for the graph
        self._graph = (graph, out, (fb, ex, cnt), pool)      # the graph holds their addresses
        self.stats["captures"] += 1

    def _eager(self, indices, why: str, own: bool):
        self.stats[why] += 1
        fb, ex, out = self.net.forward_store_flat(self.store, indices)
        return fb, ex, ({"cls": out["cls"].clone(), "reg": out["reg"].clone()} if own else out)

    @torch.no_grad()
    def forward(self, indices, own: bool = False):
        from .flatfile import StoreFitError
        t0 = time.perf_counter()
        net, hot = self.net, self.net._full_engine().hot
        eng = net._full_engine()
        if eng.hot.branches:
            raise LgcnError("StoreReplay: HotPathEngine.branches must stay off (one stream, one captured graph)")
        try:
            plan = self.store.plan(indices, caps=self.caps)
        except StoreFitError:
            return self._eager(indices, "eager_nofit", own)
        M._need_nodes(plan.real_nodes, plan.real_edges, plan.num_scales)
        if plan.real_actors == 0:
            raise LgcnError("forward_store: the picked scenes hold no actor")
        sig = self._signature()
        if sig != self._sig:
            self._graph, self._sig = None, sig
            self._warm_left = max(self._warm_left, 1)         # new packs / kernels: once eagerly before a capture
        B, N, A = self.caps.batch, plan.real_nodes, plan.real_actors
        with torch.cuda.device(self.store.device):
            self.slot.upload(plan)
            fb, ex = self._padded_batch(plan)
            if self._graph is None and self._warm_left > 0:
                self._warm_left -= 1
                route = "eager_warm"
                self.slot.launch()
                with self._stable_convs():
                    out = eng.forward(fb, ex["actor_feats"], ex["rot"], ex["orig"], ex["sizes"])
            else:
                route = "replays"
                if self._graph is None:
                    self._capture(eng, fb, ex)
                graph, out = self._graph[0], self._graph[1]
                graph.replay()
            host_ms = (time.perf_counter() - t0) * 1e3        # the host's work of this pick, up to the read that waits
            # the one host read: the range guard's word and the three pair counts
            flag, *counts = torch.cat([out["nonfinite"].view(1)] + [c.view(1) for c in out["n_pairs"]]).tolist()
        if hot.pair_caps == "tight" and hot._record(counts):
            self._graph = None                                # sized for fewer pairs: capture again, later
            return self._eager(indices, "eager_overflow", own)
        if flag != 0 and ops.get_mma() == "f16x2" and ops.get_guard() != "off":
            return self._eager(indices, "eager_guard", own)
        a_f = self.caps.actors - A                            # the filler's A2A self-pairs are nobody's context
        if M.Att.strict and (counts[0] == 0 or counts[1] == 0 or counts[2] - a_f == 0):
            raise RuntimeError("torch.cat(): expected a non-empty list of Tensors")
        self.stats[route] += 1
        self._padded += 1
        for i, share in enumerate(((self.caps.nodes - N) / self.caps.nodes, a_f / self.caps.actors,
                                   1.0 - sum(plan.real_edges) / max(sum(self.caps.edges), 1), host_ms)):
            self._pad_sum[i] += share
            self.stats[("pad_nodes", "pad_actors", "pad_edges", "host_ms")[i]] = self._pad_sum[i] / self._padded
        cut = lambda t, n: t[:n].clone() if own else t[:n]
        real = FlatBatch(n_scenes=B, n_nodes=N, n_actors=A, num_scales=plan.num_scales, rel_slices=plan.rel_slices,
                         cap_a2m=plan.cap_a2m - (self.caps.nodes - N) * a_f, cap_a2a=plan.cap_a2a - a_f * a_f,
                         n_edges=plan.real_edges,
                         node_sizes=np.diff(plan.node_off[:B + 1]).tolist(),
                         **{k: cut(getattr(fb, k), N) for k in ("node_ctrs", "node_feats", "turn", "control", "intersect")},
                         actor_ctrs=cut(fb.actor_ctrs, A), node_off=cut(fb.node_off, B + 1), actor_off=cut(fb.actor_off, B + 1),
                         idx_local=fb.idx_local, seg_off=fb.seg_off, seg_base=fb.seg_base)
        rex = {k: (cut(v, A) if torch.is_tensor(v) else v) for k, v in ex.items()}
        rex["sizes"] = list(plan.sizes[:B])
        return real, rex, {"cls": cut(out["cls"], A), "reg": cut(out["reg"], A), "nonfinite": out["nonfinite"],
                           "n_pairs": out["n_pairs"]}
