"""Model plugin with the reference's interface (lanegcn.py): ``get_model()``, ``Net``, ``graph_gather``,
``actor_gather``, ``MapNet``, ``A2M``, ``M2M``, ``M2A``, ``A2A``, ``Att`` -- same class names, constructor
arguments, forward signatures and parameter names (state_dict compatible), re-implemented on the
MI355X HIP kernels of ``csrc/`` behind the C ABI of ``include/lgcn.h``.

Hot path: graph_gather -> MapNet -> A2M -> M2M -> M2A -> A2A.  Their CUDA forward
never touches ATen arithmetic; on CPU tensors they raise (no fallback).  ActorNet / PredNet / loss are
outside the hot path and use stock PyTorch-ROCm ops.
"""
import os
from math import gcd
from typing import Dict, List, Optional

import numpy as np
import torch
from torch import Tensor, nn
from torch.nn import functional as F

from . import _lib as L
from . import autograd as A
from . import ops
from .data import collate_fn
from .layers import Conv1d, Linear, LinearRes, Res1d, group_norm1
from .utils import Optimizer, StepLR, gpu, to_long

file_path = os.path.abspath(__file__)
root_path = os.path.dirname(file_path)
model_name = os.path.basename(file_path).split(".")[0]

# Same keys and values as the reference's module-level config (lanegcn.py:27-92).
config = dict(
    display_iters=205942, val_iters=205942 * 2, save_freq=1.0, epoch=0, horovod=True, opt="adam",
    num_epochs=36, lr=[1e-3, 1e-4], lr_epochs=[32],
    batch_size=32, val_batch_size=32, workers=0, val_workers=0,
    preprocess=True, rot_aug=False, pred_range=[-100.0, 100.0, -100.0, 100.0],
    num_scales=6, n_actor=128, n_map=128,
    actor2map_dist=7.0, map2actor_dist=6.0, actor2actor_dist=100.0,
    pred_size=30, pred_step=1, num_mods=6, cls_coef=1.0, reg_coef=1.0, mgn=0.2, cls_th=2.0, cls_ignore=0.2,
)
config["lr_func"] = StepLR(config["lr"], config["lr_epochs"])
config["num_preds"] = config["pred_size"] // config["pred_step"]
config["save_dir"] = os.path.join(root_path, "results", model_name)
for _k, _p in (("train_split", "dataset/train/data"), ("val_split", "dataset/val/data"),
               ("test_split", "dataset/test_obs/data"),
               ("preprocess_train", "dataset/preprocess/train_crs_dist6_angle90.p"),
               ("preprocess_val", "dataset/preprocess/val_crs_dist6_angle90.p"),
               ("preprocess_test", "dataset/preprocess/test_test.p")):
    config[_k] = os.path.join(root_path, _p)

_FULL = L.F_GN1 | L.F_RELU1 | L.F_GEMM2 | L.F_GN2 | L.F_RES | L.F_RELU2


def _gn(m: nn.GroupNorm):
    return (m.weight, m.bias)


def _hot_guard(*tensors) -> bool:
    """The hot path is HIP-only: refuse CPU tensors loudly.  Returns True when autograd must record the
    call (then the differentiable composition of autograd.py runs instead of the fused inference kernels)."""
    for t in tensors:
        if isinstance(t, Tensor) and not t.is_cuda:
            raise L.LgcnError("LaneGCN hot-path modules need CUDA tensors (HIP kernels, no CPU fallback)")
    return ops.wants_grad(*[t for t in tensors if isinstance(t, Tensor)])


# ------------------------------------------------------------------ gathers
def actor_gather(actors: List[Tensor]):
    """[a_i,20,3] per scene -> ([A,3,20], per-scene index ranges) (reference lanegcn.py:155-168)."""
    sizes = [len(x) for x in actors]
    feats = torch.cat([x.transpose(1, 2) for x in actors], 0)
    idcs, start = [], 0
    for n in sizes:
        idcs.append(torch.arange(start, start + n, device=feats.device))
        start += n
    return feats, idcs


def rel_keys(num_scales: int) -> List[str]:
    """Relation order of the lane plan: pre0, suc0, ..., pre5, suc5, left, right (lanegcn.py:333-354)."""
    keys = []
    for i in range(num_scales):
        keys += ["pre%d" % i, "suc%d" % i]
    return keys + ["left", "right"]


def graph_gather(graphs: List[Dict]) -> Dict:
    """Merge per-scene lane graphs into one block-diagonal graph (reference lanegcn.py:171-209).

    Same output dict as the reference (idcs, ctrs, feats, turn, control, intersect, pre, suc, left,
    right with int64 u/v).  All 28 x B index arrays are offset by ONE lgcn_graph_gather launch over
    their concatenation instead of 28 x B adds and 28 cats; scenes may arrive on CPU or GPU."""
    B = len(graphs)
    dev = torch.device("cuda", torch.cuda.current_device())
    counts, node_idcs, n = [], [], 0
    for g in graphs:
        counts.append(n)
        node_idcs.append(torch.arange(n, n + g["num_nodes"], device=dev))
        n += g["num_nodes"]
    graph = dict()
    graph["idcs"] = node_idcs
    graph["ctrs"] = [g["ctrs"].to(dev, non_blocking=True) for g in graphs]
    for key in ("feats", "turn", "control", "intersect"):
        graph[key] = torch.cat([g[key] for g in graphs], 0).to(dev, non_blocking=True)

    num_scales = len(graphs[0]["pre"])
    pieces, seg_len, seg_base, slots = [], [], [], []
    empty = torch.zeros(0, dtype=torch.int64)

    def add(getter):
        start = len(pieces)
        for j, g in enumerate(graphs):
            x = getter(g)
            if x.dim() == 0:           # 0-dim guard of lanegcn.py:203-207
                x = empty.to(x.device)
            pieces.append(x.long() if x.dtype != torch.int64 else x)
            seg_len.append(int(x.numel()))
            seg_base.append(counts[j])
        slots.append((start, len(pieces)))

    for k1 in ("pre", "suc"):
        for i in range(num_scales):
            for k2 in ("u", "v"):
                add(lambda g, k1=k1, i=i, k2=k2: g[k1][i][k2])
    for k1 in ("left", "right"):
        for k2 in ("u", "v"):
            add(lambda g, k1=k1, k2=k2: g[k1][k2])

    flat = torch.cat(pieces, 0)
    if not flat.is_cuda:
        flat = flat.pin_memory().to(dev, non_blocking=True)
    off = np.zeros(len(seg_len) + 1, np.int64)
    np.cumsum(seg_len, out=off[1:])
    tables = torch.from_numpy(np.stack([off[:-1], np.asarray(seg_base, np.int64)])).to(dev)
    seg_off = torch.cat([tables[0], torch.tensor([off[-1]], device=dev)])
    out64, _ = ops.graph_gather_indices(flat, seg_off, tables[1].contiguous())

    views = [out64[off[a]:off[b]] for a, b in slots]
    it = iter(views)
    for k1 in ("pre", "suc"):
        graph[k1] = []
        for i in range(num_scales):
            graph[k1].append({"u": next(it), "v": next(it)})
    for k1 in ("left", "right"):
        graph[k1] = {"u": next(it), "v": next(it)}
    return graph


def _n_nodes(graph: Dict) -> int:
    """Rows of the merged graph: of its feature tensor, or (the fork's RoI graph keeps per-scene lists) its node count."""
    return int(graph["feats"].shape[0]) if torch.is_tensor(graph["feats"]) else int(graph["num_nodes"])


def lane_plan(graph: Dict) -> ops.LanePlan:
    """CSR-by-destination plan of the 14 relations, built once per batch and cached on the graph
    dict (the graph is identical for the 8 LaneConv layers of MapNet and M2M)."""
    plan = graph.get("_plan")
    if plan is None:
        ns = len(graph["pre"])
        us, vs = [], []
        for i in range(ns):
            for k1 in ("pre", "suc"):
                us.append(graph[k1][i]["u"])
                vs.append(graph[k1][i]["v"])
        for k1 in ("left", "right"):
            us.append(graph[k1]["u"])
            vs.append(graph[k1]["v"])
        plan = ops.csr_build(us, vs, _n_nodes(graph))
        graph["_plan"] = plan
    return plan


def _coo_lists(graph: Dict):
    us, vs = [], []
    for i in range(len(graph["pre"])):
        for k1 in ("pre", "suc"):
            us.append(graph[k1][i]["u"])
            vs.append(graph[k1][i]["v"])
    for k1 in ("left", "right"):
        us.append(graph[k1]["u"])
        vs.append(graph[k1]["v"])
    return us, vs


def lane_plan_t(graph: Dict) -> ops.LanePlan:
    """The same relations keyed by SOURCE (u and v swapped): the backward of a gather-by-destination is a
    gather-by-source of the output gradients.  Built on first use in training, cached on the graph dict."""
    plan = graph.get("_plan_t")
    if plan is None:
        us, vs = _coo_lists(graph)
        plan = ops.csr_build(vs, us, _n_nodes(graph))
        graph["_plan_t"] = plan
    return plan


def lane_conv_train(fuse: nn.ModuleDict, feat: Tensor, plan: ops.LanePlan, plan_t: ops.LanePlan,
                    num_scales: int, fused_bwd: bool = False) -> Tensor:
    """lane_conv with autograd (LaneConvFn: fused forward launch, composed HIP backward; fused_bwd: lgcn_laneconv_bwd
    for everything below the relation stage)."""
    keys = rel_keys(num_scales)
    for i in range(len(fuse["ctr"])):
        rels, weights = [A.Rel(0, 0, L.REL_IDENT)], [fuse["ctr"][i].weight]
        for r, key in enumerate(keys):
            if plan.n_edges[r] > 0:
                rels.append(A.Rel(0, len(weights), L.REL_CSR, r))
                weights.append(fuse[key][i].weight)
        spec = A.BlockSpec(n_rows=feat.shape[0], rels=rels, gn=True, relu=True, has_res=True, eps=fuse["norm"][i].eps,
                           plan=plan, plan_t=plan_t, fused_bwd=fused_bwd)
        c2 = fuse["ctr2"][i]
        feat = A.LaneConvFn.apply(spec, feat, fuse["norm"][i].weight, fuse["norm"][i].bias, c2.linear.weight,
                                  c2.norm.weight, c2.norm.bias, *weights)
    return feat


def _fuse_modules(n_map: int, num_scales: int, ng: int = 1) -> nn.ModuleDict:
    """The reference's ``fuse`` ModuleDict (lanegcn.py:288-308): 4 layers of ctr/norm/ctr2/left/right/
    pre{i}/suc{i}; key order and module types fix the state_dict names."""
    keys = ["ctr", "norm", "ctr2", "left", "right"]
    for i in range(num_scales):
        keys += ["pre%d" % i, "suc%d" % i]
    fuse = {}
    for key in keys:
        if key == "norm":
            mods = [nn.GroupNorm(gcd(ng, n_map), n_map) for _ in range(4)]
        elif key == "ctr2":
            mods = [Linear(n_map, n_map, norm="GN", ng=ng, act=False) for _ in range(4)]
        else:
            mods = [nn.Linear(n_map, n_map, bias=False) for _ in range(4)]
        fuse[key] = nn.ModuleList(mods)
    return nn.ModuleDict(fuse)


def lane_conv(fuse: nn.ModuleDict, feat: Tensor, plan: ops.LanePlan, num_scales: int, tile_rb: int = 0,
              impl: Optional[str] = None) -> Tensor:
    """4 LaneConv layers (reference lanegcn.py:331-362 == 448-479).
    impl "tiled" (default in the split-precision matrix modes): lgcn_laneconv_fwd, weight-stationary row blocks
    over LDS-resident source rows + a combine launch; "fused": one lgcn_agg_mlp launch per layer (the only
    implementation of the exact-f32 mode, and the one the autograd path records)."""
    keys = rel_keys(num_scales)
    if impl is None:      # three-plane operands leave the tiled kernel too little LDS per row block to pay (measured)
        impl = "fused" if ops.get_mma() == "bf16x3" else ops.laneconv_impl()
    lcp = ops.lc_plan(plan) if impl == "tiled" and tile_rb == 0 and plan.n_nodes > 0 else None
    if lcp is not None:
        part = ops.lc_part(lcp)
        for i in range(len(fuse["ctr"])):
            wps = [ops.packed(fuse["ctr"][i].weight)]
            wps += [ops.packed(fuse[key][i].weight) if plan.n_edges[r] > 0 else None for r, key in enumerate(keys)]
            c2 = fuse["ctr2"][i]
            feat = ops.laneconv_fwd(feat, lcp, wps, _gn(fuse["norm"][i]), ops.packed(c2.linear.weight), _gn(c2.norm),
                                    eps=fuse["norm"][i].eps, part=part)
        return feat
    for i in range(len(fuse["ctr"])):
        rels = [ops.RelSpec(feat, ops.packed(fuse["ctr"][i].weight), L.REL_IDENT)]
        for r, key in enumerate(keys):
            if plan.n_edges[r] > 0:
                rels.append(ops.RelSpec(feat, ops.packed(fuse[key][i].weight), L.REL_CSR, r))
        c2 = fuse["ctr2"][i]
        feat = ops.agg_mlp(feat.shape[0], rels, _FULL, rowptr=plan.rowptr, col=plan.col, n_rel_csr=plan.n_rel,
                           gn1=_gn(fuse["norm"][i]), wp2=ops.packed(c2.linear.weight), gn2=_gn(c2.norm),
                           res=feat, eps=fuse["norm"][i].eps, tag="laneconv", tile_rb=tile_rb)
    return feat


class MapNet(nn.Module):
    """Map Graph feature extractor with LaneGraphCNN (reference lanegcn.py:266-363)."""
    # Train the 4 LaneConv layers with the fused exact-fp32 backward (autograd.BlockSpec.fused_bwd: lgcn_laneconv_bwd, then
    # the relation stage's two launches) instead of the ten composed launches per layer.  Opt-in, like Att.train_hip.
    train_hip = False

    def __init__(self, config):
        super().__init__()
        self.config = config
        n_map = config["n_map"]
        self.input = nn.Sequential(nn.Linear(2, n_map), nn.ReLU(inplace=True),
                                   Linear(n_map, n_map, norm="GN", ng=1, act=False))
        self.seg = nn.Sequential(nn.Linear(2, n_map), nn.ReLU(inplace=True),
                                 Linear(n_map, n_map, norm="GN", ng=1, act=False))
        self.fuse = _fuse_modules(n_map, config["num_scales"])
        self.relu = nn.ReLU(inplace=True)

    def stem(self, ctrs: Tensor, feats: Tensor) -> Tensor:
        """ReLU(input(ctrs) + seg(feats)), one launch (reference lanegcn.py:324-327)."""
        a, s = self.input, self.seg
        return ops.mapnet_input(ctrs, feats,
                                a[0].weight, a[0].bias, ops.packed(a[2].linear.weight), _gn(a[2].norm),
                                s[0].weight, s[0].bias, ops.packed(s[2].linear.weight), _gn(s[2].norm),
                                eps=a[2].norm.eps)

    def forward(self, graph):
        if (len(graph["feats"]) == 0 or len(graph["pre"][-1]["u"]) == 0 or len(graph["suc"][-1]["u"]) == 0):
            # the reference's early-return branch reads a key that graph_gather never sets
            # (lanegcn.py:312-322) and therefore raises KeyError; kept for error parity
            raise KeyError("node_idcs")
        ctrs = torch.cat(graph["ctrs"], 0)
        if _hot_guard(graph["feats"], *ops.module_params(self)):
            a, s = self.input, self.seg      # the two nn.Linear(2,128) are [N,2]-shaped: stock ops
            fa = A.linear_gn(F.relu(a[0](ctrs)), a[2].linear.weight, gn=a[2].norm)
            fs = A.linear_gn(F.relu(s[0](graph["feats"])), s[2].linear.weight, gn=s[2].norm)
            feat = lane_conv_train(self.fuse, F.relu(fa + fs), lane_plan(graph), lane_plan_t(graph), len(graph["pre"]),
                                   fused_bwd=MapNet.train_hip)
            return feat, graph["idcs"], graph["ctrs"]
        feat = ops.guarded(lambda: lane_conv(self.fuse, self.stem(ctrs, graph["feats"]), lane_plan(graph), len(graph["pre"])))
        return feat, graph["idcs"], graph["ctrs"]


class M2M(nn.Module):
    """Lane to lane block: 4 more LaneConv layers (reference lanegcn.py:410-480)."""
    train_hip = False       # as MapNet.train_hip

    def __init__(self, config):
        super().__init__()
        self.config = config
        self.fuse = _fuse_modules(config["n_map"], config["num_scales"])
        self.relu = nn.ReLU(inplace=True)

    def forward(self, feat: Tensor, graph: Dict) -> Tensor:
        if _hot_guard(feat, *ops.module_params(self)):
            return lane_conv_train(self.fuse, feat, lane_plan(graph), lane_plan_t(graph), len(graph["pre"]),
                                   fused_bwd=M2M.train_hip)
        return ops.guarded(lambda: lane_conv(self.fuse, feat, lane_plan(graph), len(graph["pre"])))


# ------------------------------------------------------------------ attention blocks
def build_pairs(agt_idcs, agt_ctrs, ctx_idcs, ctx_ctrs, dist_th, legacy_offsets=True) -> ops.PairSet:
    """Distance-gated (target, context) pairs of one fusion block (reference lanegcn.py:672-689),
    searched once per block on the GPU and reused by both of its Att layers."""
    ta = [int(len(x)) for x in agt_idcs]
    tc = [int(len(x)) for x in ctx_idcs]
    dev = agt_ctrs[0].device
    off = np.zeros((2, len(ta) + 1), np.int32)
    np.cumsum(ta, out=off[0, 1:])
    np.cumsum(tc, out=off[1, 1:])
    off_d = torch.from_numpy(off).to(dev)
    cap = int(np.dot(np.asarray(ta, np.int64), np.asarray(tc, np.int64)))
    return ops.pairs_build(torch.cat(agt_ctrs, 0), off_d[0], torch.cat(ctx_ctrs, 0), off_d[1],
                           dist_th, cap, legacy_offsets)


class Att(nn.Module):
    """Distance-gated attention block (reference lanegcn.py:634-710).

    ``strict`` (default True) keeps the reference's error behaviour -- a batch without a single
    pair raises like ``torch.cat([])`` at lanegcn.py:688 -- at the price of one device->host read of
    P per pair set; the benchmark engine switches it off to run sync-free."""
    strict = True
    legacy_offsets = True   # zero-pair scenes do not advance hi/wi offsets (lanegcn.py:681-687)
    fold = True             # att_block: row-block launches folded across the Att layers
    # Train the pair stage (lanegcn.py:691-703) on the fused exact-fp32 pair of autograd.AttPairsFn (lgcn_att_pairs_train /
    # lgcn_att_pairs_bwd) instead of the composition of row blocks below: no [P,128] tensor is saved, one is written in the
    # backward.  Opt-in, like ActorNet.train_hip / PredNet.train_hip: the default training path stays the composed one.
    train_hip = False

    def __init__(self, n_agt: int, n_ctx: int) -> None:
        super().__init__()
        self.dist = nn.Sequential(nn.Linear(2, n_ctx), nn.ReLU(inplace=True),
                                  Linear(n_ctx, n_ctx, norm="GN", ng=1))
        self.query = Linear(n_agt, n_ctx, norm="GN", ng=1)
        self.ctx = nn.Sequential(Linear(3 * n_ctx, n_agt, norm="GN", ng=1), nn.Linear(n_agt, n_agt, bias=False))
        self.agt = nn.Linear(n_agt, n_agt, bias=False)
        self.norm = nn.GroupNorm(gcd(1, n_agt), n_agt)
        self.linear = Linear(n_agt, n_agt, norm="GN", ng=1, act=False)
        self.relu = nn.ReLU(inplace=True)

    def forward(self, agts: Tensor, agt_idcs: List[Tensor], agt_ctrs: List[Tensor], ctx: Tensor,
                ctx_idcs: List[Tensor], ctx_ctrs: List[Tensor], dist_th: float,
                pairs: Optional[ops.PairSet] = None) -> Tensor:
        train = _hot_guard(agts, ctx, *ops.module_params(self))
        T = agts.shape[0]
        lin = self.linear
        if len(ctx) == 0:   # lanegcn.py:664-670: no GroupNorm before the ReLU
            if train:
                a = A.linear_gn(agts, self.agt.weight, relu=True)
                return A.linear_gn(a, lin.linear.weight, gn=lin.norm, relu=True, res=agts)
            return ops.guarded(lambda: ops.agg_mlp(T, [ops.RelSpec(agts, ops.packed(self.agt.weight))],
                                                   L.F_RELU1 | L.F_GEMM2 | L.F_GN2 | L.F_RES | L.F_RELU2,
                                                   wp2=ops.packed(lin.linear.weight), gn2=_gn(lin.norm), res=agts,
                                                   eps=lin.norm.eps))
        ps = pairs if pairs is not None else build_pairs(agt_idcs, agt_ctrs, ctx_idcs, ctx_ctrs, dist_th,
                                                         self.legacy_offsets)
        if (self.strict or train) and ps.count() == 0:
            raise RuntimeError("torch.cat(): expected a non-empty list of Tensors")
        return self.run_train(agts, ctx, ps) if train else ops.guarded(lambda: self.run(agts, ctx, ps))

    def _train_hip_ok(self, agts: Tensor, ctx: Tensor, ps: ops.PairSet) -> bool:
        rows_ok = max(agts.shape[0], ctx.shape[0]) < (1 << 23)
        return (Att.train_hip and agts.is_cuda and agts.dtype == torch.float32 and ctx.dtype == torch.float32
                and agts.shape[1] == ops.C_FEAT and ctx.shape[1] == ops.C_FEAT and self.agt.weight.shape[0] == ops.C_FEAT
                and rows_ok and ps.count() > 0 and not (ps.agt_ctrs.requires_grad or ps.ctx_ctrs.requires_grad))

    def run_train_hip(self, agts: Tensor, ctx: Tensor, ps: ops.PairSet) -> Tensor:
        """run_train with the pair stage on AttPairsFn: U, V and the node epilogue are the same row blocks; the segment
        sum S comes out of the pair stage, and ctx.1 (linear) is applied to it as in pairs_tail."""
        T = agts.shape[0]
        lin, c0, d = self.linear, self.ctx[0], self.dist
        q = A.linear_gn(agts, self.query.linear.weight, gn=self.query.norm, relu=True)
        U = A.linear_gn(q, c0.linear.weight, col0=128)
        V = A.linear_gn(ctx, c0.linear.weight, col0=256)
        S = A.AttPairsFn.apply(ps, d[0].weight, d[0].bias, d[2].linear.weight, d[2].norm.weight, d[2].norm.bias,
                               c0.linear.weight, U, V, c0.norm.weight, c0.norm.bias, c0.norm.eps)
        y = A.row_block([agts, S], [self.agt.weight, self.ctx[1].weight], [A.Rel(0, 0, L.REL_IDENT), A.Rel(1, 1, L.REL_IDENT)],
                        T, gn=self.norm, relu=True, tag="att_post")
        return A.linear_gn(y, lin.linear.weight, gn=lin.norm, relu=True, res=agts)

    def run_train(self, agts: Tensor, ctx: Tensor, ps: ops.PairSet) -> Tensor:
        """Differentiable composition of the same arithmetic as run() (lanegcn.py:691-709): per-pair tensors are
        sized by the exact pair count (one host read per pair set, already paid by the emptiness check)."""
        if self._train_hip_ok(agts, ctx, ps):
            return self.run_train_hip(agts, ctx, ps)
        P, T = ps.count(), agts.shape[0]
        lin, c0 = self.linear, self.ctx[0]
        hi, wi = ps.hi[:P].long(), ps.wi[:P].long()
        delta = ps.agt_ctrs[hi] - ps.ctx_ctrs[wi]                                   # [P,2]; centres carry no gradient
        h1 = F.relu(self.dist[0](delta))                                           # nn.Linear(2,128): stock op
        e = A.linear_gn(h1, self.dist[2].linear.weight, gn=self.dist[2].norm, relu=True)
        q = A.linear_gn(agts, self.query.linear.weight, gn=self.query.norm, relu=True)
        U = A.linear_gn(q, c0.linear.weight, col0=128)
        V = A.linear_gn(ctx, c0.linear.weight, col0=256)
        c = A.PairAddFn.apply(A.linear_gn(e, c0.linear.weight, col0=0), U, V, ps)
        m = A.gn_act(c, gn=c0.norm, relu=True)
        spec_kw = dict(rowptr=ps.rowptr, seg_ids=ps.hi, n_seg_rows=ps.n_pairs, tag="att_post")
        y = A.row_block([agts, m], [self.agt.weight, self.ctx[1].weight],
                        [A.Rel(0, 0, L.REL_IDENT), A.Rel(1, 1, L.REL_RANGE)], T, gn=self.norm, relu=True, **spec_kw)
        return A.linear_gn(y, lin.linear.weight, gn=lin.norm, relu=True, res=agts)

    def run(self, agts: Tensor, ctx: Tensor, ps: ops.PairSet, side: Optional[torch.cuda.Stream] = None) -> Tensor:
        """The pair MLP + segment reduce + node epilogue for a given pair set (lanegcn.py:691-709).
        `side`: a second stream for V (independent of U) -- fork/join around it, buffers allocated here."""
        # row-wise Linears commute with the gathers agts[hi] / ctx[wi]: evaluate them per node.  U (per target:
        # query -> GN -> ReLU -> ctx.0[:,128:256]) and V (per context row: ctx.0[:,256:384]) are independent:
        # one dual-problem launch
        u_kw, v_kw = self.u_kw(agts), self.v_kw(ctx)
        if side is not None:
            main = torch.cuda.current_stream()
            V = torch.empty((ctx.shape[0], ops.C_FEAT), dtype=torch.float32, device=ctx.device)
            side.wait_stream(main)
            with torch.cuda.stream(side):
                ops.agg_mlp(out=V, **v_kw)
            U = ops.agg_mlp(**u_kw)
            main.wait_stream(side)
        else:
            U, V = ops.agg_mlp_pair(u_kw, v_kw)
        return self.pairs_tail(agts, ctx.shape[0], ps, U, V)

    # ---- the pieces of run(), also used by att_block (launch folding across the Att layers of a fusion block)
    def u_kw(self, agts: Tensor) -> dict:
        """U = ReLU(GN_q(agts W_q^T)) W_c0[:,128:256]^T per target row, as an agg_mlp problem."""
        return dict(n_rows=agts.shape[0], rels=[ops.RelSpec(agts, ops.packed(self.query.linear.weight))],
                    flags=L.F_GN1 | L.F_RELU1 | L.F_GEMM2, gn1=_gn(self.query.norm),
                    wp2=ops.packed(self.ctx[0].linear.weight, 128, 128), eps=self.query.norm.eps)

    def v_kw(self, ctx: Tensor) -> dict:
        """V = ctx W_c0[:,256:384]^T per context row, as an agg_mlp problem."""
        return dict(n_rows=ctx.shape[0], rels=[ops.RelSpec(ctx, ops.packed(self.ctx[0].linear.weight, 256, 128))], flags=0)

    def chain_u(self):
        """What a row block that PRODUCES this layer's target rows needs to emit its U as well (ops.agg_mlp chain_u)."""
        return (ops.packed(self.query.linear.weight), _gn(self.query.norm), ops.packed(self.ctx[0].linear.weight, 128, 128))

    def chain_v(self):
        return ops.packed(self.ctx[0].linear.weight, 256, 128)

    def pairs_tail(self, agts: Tensor, n_ctx: int, ps: ops.PairSet, U: Tensor, V: Tensor, chain_u=None, chain_v=None):
        """Pair MLP + segment sum + node epilogue for given U / V (lanegcn.py:693-709); the tail's launch can emit the
        NEXT layer's U / V from its output rows (chain_u / chain_v).  Returns out or (out, U'[, V'])."""
        T = agts.shape[0]
        lin, c0 = self.linear, self.ctx[0]
        # few targets with many pairs each (M2A, A2A: at least as many context rows as targets): the pair kernel
        # sums the rows of a target inside every 16-aligned group, and the tail reads one row per piece
        seg = 16 if ops.att_pairs_impl() in ("ws", "wi") and n_ctx >= T else 0
        m = ops.att_pairs(ps, self.dist[0].weight, self.dist[0].bias, (self.dist[2].linear.weight, 0),
                          _gn(self.dist[2].norm), (c0.linear.weight, 0), U, V, _gn(c0.norm),
                          eps=c0.norm.eps, seg=seg)
        # ctx.1 is linear: apply it to the per-target segment sum instead of every pair
        rels = [ops.RelSpec(agts, ops.packed(self.agt.weight)),
                ops.RelSpec(m, ops.packed(self.ctx[1].weight), L.REL_RANGE16 if seg else L.REL_RANGE)]
        # many targets (A2M: the lane nodes), no V to emit: the weight-stationary launch, same bits
        tail = ops.node_tail if seg == 0 and chain_v is None and ops.node_tail_ok() else ops.agg_mlp
        return tail(T, rels, _FULL, rowptr=ps.rowptr, gn1=_gn(self.norm),
                    wp2=ops.packed(lin.linear.weight), gn2=_gn(lin.norm), res=agts, eps=self.norm.eps,
                    tag="att_post", chain_u=chain_u, chain_v=chain_v)


def att_block(atts, agts: Optional[Tensor], ctx: Tensor, ps: ops.PairSet, head: Optional[dict] = None, uv=None,
              ctx_is_agts: bool = False, next_att: Optional["Att"] = None, next_ctx_is_out: bool = False,
              u0: Optional[Tensor] = None, extra: Optional[dict] = None):
    """The Att layers of one fusion block (reference lanegcn.py:397-406, 506-512, 537-544) with the row-block launches
    folded: a layer's tail also emits the next layer's U (and V, when the context rows are the targets: A2A) from its
    output rows before they leave the CU, the V rows of every layer whose context does not change are computed up
    front, and the block's first launch carries them together with U of layer 0 -- chained onto `head`, the row block
    that produces the targets (A2M.meta), when there is one (that launch is then the weight-stationary ops.node_head in
    f16x2 / bf16, the multi-problem row block otherwise).  Same arithmetic as Att.run per layer.
      head: agg_mlp keywords of a row block whose output is the block's target rows (agts is then ignored);
      uv: (U, V) of layer 0 when a previous block's tail has already emitted them;
      next_att: first Att of the FOLLOWING block when this block's output rows are its targets (and, with
                next_ctx_is_out, its context rows): the last tail emits its U (and V);
      u0: U of layer 0 when an earlier launch has computed it (it depends on the targets alone: HotPathEngine puts M2A's
          into A2M's first launch); the block then starts with its V rows;
      extra: one more agg_mlp problem for the block's first launch (A2M carrying M2A's U of layer 0); its output is
             returned as a third value.
    V rows that are still missing once U of layer 0 is known (context rows that are not the targets) come from one
    weight-stationary launch that reads the context rows once (ops.ctx_heads: f16x2 / bf16) or, in the other modes,
    from a multi-problem row-block launch.
    Returns (out, uv_next) -- uv_next is None without next_att -- or (out, uv_next, extra's output)."""
    n = len(atts)
    Vs = [None] * n
    x_out = None
    if uv is not None:
        U, Vs[0] = uv
    elif u0 is not None:
        U = u0
    else:
        first = dict(head, chain_u=atts[0].chain_u()) if head is not None else atts[0].u_kw(agts)
        probs = [first] + [atts[i].v_kw(ctx) for i in range(1 if ctx_is_agts else n)]
        probs_all = probs + ([extra] if extra is not None else [])
        # targets produced by `head` (A2M: the lane nodes): the weight-stationary launch, same bits
        ws = head is not None and ops.node_head_ok() and all(ops.node_head_form(kw) is not None for kw in probs_all)
        res = (ops.node_head if ws else ops.agg_mlp_multi)(probs_all, tag="att_head")
        if extra is not None:
            x_out, extra = res[-1], None
        if head is not None:
            agts, U = res[0]
        else:
            U = res[0]
        for i in range(len(probs) - 1):
            Vs[i] = res[1 + i]
    if extra is not None:
        x_out = ops.agg_mlp(**extra)
    if not ctx_is_agts and any(v is None for v in Vs):      # U of layer 0 came with uv / u0: the V rows on their own
        todo = [i for i in range(n) if Vs[i] is None]
        if ops.ctx_heads_ok():
            for k in range(0, len(todo), 2):
                part = todo[k:k + 2]
                for i, v in zip(part, ops.ctx_heads(ctx, [atts[i].chain_v() for i in part])):
                    Vs[i] = v
        else:
            for i, v in zip(todo, ops.agg_mlp_multi([atts[i].v_kw(ctx) for i in todo], tag="att_head")):
                Vs[i] = v
    uv_next = None
    for i, att in enumerate(atts):
        nxt = atts[i + 1] if i + 1 < n else next_att
        want_v = nxt is not None and (ctx_is_agts if i + 1 < n else next_ctx_is_out)
        n_ctx = agts.shape[0] if ctx_is_agts else ctx.shape[0]
        res = att.pairs_tail(agts, n_ctx, ps, U, Vs[i], chain_u=nxt.chain_u() if nxt is not None else None,
                             chain_v=nxt.chain_v() if want_v else None)
        if nxt is None:
            agts = res
        elif i + 1 < n:
            agts, U = res[0], res[1]
            if want_v:
                Vs[i + 1] = res[2]
        else:
            agts, uv_next = res[0], (res[1], res[2] if want_v else None)
    return (agts, uv_next) if x_out is None else (agts, uv_next, x_out)


def _fold_ok(ctx: Tensor) -> bool:
    return Att.fold and ctx.shape[0] > 0


def _strict_check(ps: ops.PairSet):
    """Att.strict: a batch without a single pair raises like torch.cat([]) at lanegcn.py:688 (one host read of P)."""
    if Att.strict and ps.count() == 0:
        raise RuntimeError("torch.cat(): expected a non-empty list of Tensors")


class A2M(nn.Module):
    """Actor to Map fusion (reference lanegcn.py:366-407)."""

    def __init__(self, config):
        super().__init__()
        self.config = config
        n_map = config["n_map"]
        self.meta = Linear(n_map + 4, n_map, norm="GN", ng=1)
        self.att = nn.ModuleList([Att(n_map, config["n_actor"]) for _ in range(2)])

    def fuse_meta(self, feat: Tensor, turn: Tensor, control: Tensor, intersect: Tensor) -> Tensor:
        """meta = Linear(132 -> 128)+GN+ReLU over cat(feat, turn, control, intersect) without
        materialising the cat (reference lanegcn.py:387-395)."""
        return ops.agg_mlp(**self.meta_kw(feat, turn, control, intersect))

    def meta_kw(self, feat: Tensor, turn: Tensor, control: Tensor, intersect: Tensor) -> dict:
        w = self.meta.linear.weight
        return dict(n_rows=feat.shape[0], rels=[ops.RelSpec(feat, ops.packed(w, 0, 128))], flags=L.F_GN1 | L.F_RELU1,
                    x4=(turn, control, intersect), w4=ops.cols4(w, 128), gn1=_gn(self.meta.norm), eps=self.meta.norm.eps)

    def run(self, feat: Tensor, turn: Tensor, control: Tensor, intersect: Tensor, actors: Tensor, ps: ops.PairSet,
            extra: Optional[dict] = None):
        """meta + both Att layers for given pairs, launches folded (att_block): inference only.
        extra: one more agg_mlp problem that rides in the first launch (meta + chained U0 | V0 | V1 | extra: the four
        problems of lgcn_agg_mlp_multi) -- a row block that depends on the forward's inputs alone, such as M2A's U of
        layer 0 over the actors; the result is then (feat, extra's output)."""
        if not _fold_ok(actors):
            feat = self.fuse_meta(feat, turn, control, intersect)
            for att in self.att:
                feat = att.run(feat, actors, ps)
            return feat if extra is None else (feat, ops.agg_mlp(**extra))
        res = att_block(self.att, None, actors, ps, head=self.meta_kw(feat, turn, control, intersect), extra=extra)
        return res[0] if extra is None else (res[0], res[2])

    def forward(self, feat: Tensor, graph: Dict, actors: Tensor, actor_idcs: List[Tensor],
                actor_ctrs: List[Tensor]) -> Tensor:
        if _hot_guard(feat, actors, *ops.module_params(self)):
            w = self.meta.linear.weight       # 132 = 128 (HIP row block) + 4 meta columns ([N,4]: stock op)
            meta4 = torch.cat((graph["turn"], graph["control"].unsqueeze(1), graph["intersect"].unsqueeze(1)), 1)
            feat = A.gn_act(A.linear_gn(feat, w, col0=0) + F.linear(meta4, w[:, 128:132]), gn=self.meta.norm, relu=True)
        else:
            x_in = feat
            if len(actors) > 0 and _fold_ok(actors):      # inference: meta + both Att layers with folded launches
                ps = build_pairs(graph["idcs"], graph["ctrs"], actor_idcs, actor_ctrs, self.config["actor2map_dist"],
                                 Att.legacy_offsets)
                _strict_check(ps)
                return ops.guarded(lambda: self.run(x_in, graph["turn"], graph["control"], graph["intersect"], actors, ps))
            feat = ops.guarded(lambda: self.fuse_meta(x_in, graph["turn"], graph["control"], graph["intersect"]))
        th = self.config["actor2map_dist"]
        ps = None
        if len(actors) > 0:
            ps = build_pairs(graph["idcs"], graph["ctrs"], actor_idcs, actor_ctrs, th, Att.legacy_offsets)
        for att in self.att:
            feat = att(feat, graph["idcs"], graph["ctrs"], actors, actor_idcs, actor_ctrs, th, pairs=ps)
        return feat


class M2A(nn.Module):
    """Lane to actor fusion (reference lanegcn.py:483-513)."""

    def __init__(self, config):
        super().__init__()
        self.config = config
        self.att = nn.ModuleList([Att(config["n_actor"], config["n_map"]) for _ in range(2)])

    def forward(self, actors: Tensor, actor_idcs: List[Tensor], actor_ctrs: List[Tensor], nodes: Tensor,
                node_idcs: List[Tensor], node_ctrs: List[Tensor]) -> Tensor:
        th = self.config["map2actor_dist"]
        ps = None
        if len(nodes) > 0:
            ps = build_pairs(actor_idcs, actor_ctrs, node_idcs, node_ctrs, th, Att.legacy_offsets)
            if _fold_ok(nodes) and not _hot_guard(actors, nodes, *ops.module_params(self)):
                _strict_check(ps)
                x_in = actors
                return ops.guarded(lambda: att_block(self.att, x_in, nodes, ps)[0])
        for att in self.att:
            actors = att(actors, actor_idcs, actor_ctrs, nodes, node_idcs, node_ctrs, th, pairs=ps)
        return actors


class A2A(nn.Module):
    """Actor to actor interaction (reference lanegcn.py:516-545)."""

    def __init__(self, config):
        super().__init__()
        self.config = config
        self.att = nn.ModuleList([Att(config["n_actor"], config["n_actor"]) for _ in range(2)])

    def forward(self, actors: Tensor, actor_idcs: List[Tensor], actor_ctrs: List[Tensor]) -> Tensor:
        th = self.config["actor2actor_dist"]
        ps = None
        if len(actors) > 0:
            ps = build_pairs(actor_idcs, actor_ctrs, actor_idcs, actor_ctrs, th, Att.legacy_offsets)
            if _fold_ok(actors) and not _hot_guard(actors, *ops.module_params(self)):
                _strict_check(ps)
                x_in = actors
                return ops.guarded(lambda: att_block(self.att, x_in, x_in, ps, ctx_is_agts=True)[0])
        for att in self.att:
            actors = att(actors, actor_idcs, actor_ctrs, actors, actor_idcs, actor_ctrs, th, pairs=ps)
        return actors


# ------------------------------------------------------------------ rest of the plugin (outside the hot path)
def upsample2_linear(x: Tensor) -> Tensor:
    """F.interpolate(x, scale_factor=2, mode="linear", align_corners=False) on [N, C, L] written with slices:
    out[2i] = 0.25 x[i-1] + 0.75 x[i], out[2i+1] = 0.75 x[i] + 0.25 x[i+1] (edges clamped).  The stock ROCm
    upsample_linear1d kernels take 30 ms forward / 81 ms backward at [1600,128,10] on MI355X (88 % of a training
    step); this is a handful of elementwise ops."""
    left = torch.cat((x[..., :1], x[..., :-1]), -1)
    right = torch.cat((x[..., 1:], x[..., -1:]), -1)
    even, odd = 0.25 * left + 0.75 * x, 0.75 * x + 0.25 * right
    return torch.stack((even, odd), -1).reshape(*x.shape[:-1], 2 * x.shape[-1])


class ActorNet(nn.Module):
    """1-D conv FPN over the 20-step actor tracks (reference lanegcn.py:212-263); stock ATen ops."""

    def __init__(self, config):
        super().__init__()
        self.config = config
        n_in, widths = 3, [32, 64, 128]
        groups = []
        for i, w in enumerate(widths):
            blocks = [Res1d(n_in, w, norm="GN", ng=1) if i == 0 else Res1d(n_in, w, stride=2, norm="GN", ng=1),
                      Res1d(w, w, norm="GN", ng=1)]
            groups.append(nn.Sequential(*blocks))
            n_in = w
        self.groups = nn.ModuleList(groups)
        n = config["n_actor"]
        self.lateral = nn.ModuleList([Conv1d(w, n, norm="GN", ng=1, act=False) for w in widths])
        self.output = Res1d(n, n, norm="GN", ng=1)

    def _forward_channels_last(self, actors: Tensor) -> Tensor:
        """Inference path: the same FPN on [A, C, 1, L] tensors in torch.channels_last (memory [A, L, C]).  MIOpen
        runs these convolutions 2-3x faster than the NCL ones (no layout transposes around its NHWC kernels:
        128->128 at L = 20 takes 35 us instead of 59), and every norm / residual / ReLU / upsampling step in
        between is one lgcn_gn_cl launch."""
        cl = torch.channels_last

        def conv(m: nn.Conv1d, x: Tensor) -> Tensor:
            w = ops._cached(m.weight, ("cl4",), lambda: m.weight.detach().unsqueeze(2).contiguous(memory_format=cl))
            return F.conv2d(x, w, stride=(1, m.stride[0]), padding=(0, m.padding[0]))

        def gn(x, norm, **kw):
            return ops.gn_cl(x, norm.weight, norm.bias, norm.eps, **kw)

        def res1d(b: Res1d, x: Tensor) -> Tensor:
            out = gn(conv(b.conv1, x), b.bn1, relu=True)
            skip = x if b.downsample is None else gn(conv(b.downsample[0], x), b.downsample[1])
            return gn(conv(b.conv2, out), b.bn2, relu=b.act, res=skip)

        out, pyramid = actors.unsqueeze(2).contiguous(memory_format=cl), []
        for g in self.groups:
            for b in g:
                out = res1d(b, out)
            pyramid.append(out)
        lat = self.lateral[-1]
        out = gn(conv(lat.conv, pyramid[-1]), lat.norm, relu=lat.act)
        for i in range(len(pyramid) - 2, -1, -1):
            lat = self.lateral[i]
            out = gn(conv(lat.conv, pyramid[i]), lat.norm, res=out, res_up2=True)
        return res1d(self.output, out)[:, :, 0, -1]

    def _forward_hip(self, actors: Tensor) -> Tensor:
        """The FPN on lgcn_conv1d_gn: every Conv1d + GroupNorm (+ residual, + x2 upsampling, + ReLU) of the FPN is
        ONE launch on [A, L, C] tensors: 20 launches instead of 20 stock convolutions + 20 norm launches.  Under autograd
        the same 20 units run as Conv1dGNFn (lgcn_conv1d_gn_train forward, lgcn_conv1d_gn_bwd backward), unfused.  With
        ActorNet.exact the 20 units are lgcn_conv1d_gn_f32 launches (fp32 operands), unfused in inference too."""
        train = ops.wants_grad(actors, *ops.module_params(self))
        exact = ActorNet.exact

        def cg(conv: nn.Conv1d, norm: nn.GroupNorm, x: Tensor, **kw) -> Tensor:
            if exact:
                kw["exact"] = True
            if train:
                return A.conv1d_gn(x, conv, norm, **kw)
            return ops.conv1d_gn(x, conv.weight, conv.stride[0], norm.weight, norm.bias, norm.eps, **kw)

        def fusable(b: Res1d) -> bool:
            return not train and not exact and ActorNet.fuse_blocks and b.act and b.conv1.kernel_size[0] == 3 and b.conv2.kernel_size[0] == 3 and \
                b.conv2.stride[0] == 1 and b.bn1.eps == b.bn2.eps and \
                (b.downsample is None or (b.downsample[0].kernel_size[0] == 1 and b.downsample[1].eps == b.bn1.eps))

        def group(g, x: Tensor) -> Tensor:
            # two blocks (the second with the identity shortcut) in one launch
            if len(g) == 2 and fusable(g[0]) and fusable(g[1]) and g[1].downsample is None and g[1].conv1.stride[0] == 1 and \
                    g[1].bn1.eps == g[0].bn1.eps and ActorNet.fuse_groups:
                return ops.res1d_gn(x, g[0], second=g[1])
            for b in g:
                x = res1d(b, x)
            return x

        def res1d(b: Res1d, x: Tensor) -> Tensor:
            if fusable(b):
                return ops.res1d_gn(x, b)                                 # the whole block in one launch
            out = cg(b.conv1, b.bn1, x, relu=True)
            skip = x if b.downsample is None else cg(b.downsample[0], b.downsample[1], x)
            return cg(b.conv2, b.bn2, out, res=skip, relu=b.act)

        out, pyramid = actors.transpose(1, 2).contiguous(), []          # [A, 3, 20] -> [A, 20, 3]
        for g in self.groups:
            out = group(g, out)
            pyramid.append(out)
        lat = self.lateral[-1]
        out = cg(lat.conv, lat.norm, pyramid[-1], relu=lat.act)
        for i in range(len(pyramid) - 2, -1, -1):
            lat = self.lateral[i]
            out = cg(lat.conv, lat.norm, pyramid[i], res=out, res_up2=True)
        return res1d(self.output, out)[:, -1, :].contiguous()        # a view would be copied again by every op that takes it

    def _hip_ok(self, actors: Tensor) -> bool:
        # lgcn_conv1d_gn / lgcn_res1d_gn take no matrix-mode argument: they always split operands into two fp16 planes.
        # In the exact-f32 and bf16x3 modes (and inside the range guard's bf16x3 re-run, which must cure an overflow that
        # starts in ActorNet too) the MIOpen channels-last path runs instead -- unless ActorNet.exact is set: the fp32
        # units (lgcn_conv1d_gn_f32) take fp32's whole operand range and serve every matrix mode.  Their GroupNorm (and
        # lgcn_gn_cl's, the norm of the MIOpen path) follows convolutions of any finite size: where the squares of the
        # centred values leave fp32 (beyond ~2^58) the variance is summed over scaled values (conv_gn_stats<true>,
        # gn_cl_rstd_wide; measured at 2^100, DESIGN.md 5c "ActorNet").  Before that path they returned beta there.
        if ActorNet.impl != "hip" or not (ActorNet.exact or ops.get_mma() == "f16x2") or not self._channels_last_shape_ok(actors):
            return False
        if not ActorNet.train_hip and ops.wants_grad(actors, *ops.module_params(self)):
            return False
        convs = [c for g in self.groups for b in g for c in ([b.conv1, b.conv2] + ([b.downsample[0]] if b.downsample is not None else []))]
        convs += [l.conv for l in self.lateral] + [self.output.conv1, self.output.conv2]
        ok = all(c.bias is None and c.padding[0] == (c.kernel_size[0] - 1) // 2 and c.dilation[0] == 1 and c.groups == 1 for c in convs)
        lens, lin = [], actors.shape[2]
        for g in self.groups:                       # lengths along the FPN: stride-2 groups halve them
            lin = (lin + 2 * 1 - 3) // g[0].conv1.stride[0] + 1
            lens.append(lin)
        # every level's length is one lgcn_conv1d_gn takes (5, 10, 20), consecutive levels halve (the x2 upsampling)
        return ok and all(n in (5, 10, 20) for n in lens) and all(lens[i] == 2 * lens[i + 1] for i in range(len(lens) - 1)) and \
            all(c.in_channels <= 128 and c.out_channels in (32, 64, 128) and c.kernel_size[0] in (1, 3) and c.stride[0] in (1, 2) for c in convs)

    # "hip": lgcn_conv1d_gn / lgcn_res1d_gn launches (training: Conv1dGNFn); "miopen": stock channels-last convolutions +
    # lgcn_gn_cl for inference, the stock NCL path for training
    impl = "hip"
    # training (autograd recording) on the HIP units too: Conv1dGNFn forward and backward instead of the stock NCL path.
    # Off by default: the f16x2 forward moves the actor features by fp32 rounding, which is enough to change which
    # knife-edge ReLUs of the graph hot path flip against the reference in the batch-32 training check.
    train_hip = False
    # the units in exact fp32 (lgcn_conv1d_gn_f32: fp32 operands on v_mfma_f32_16x16x4_f32) in every matrix mode, one launch
    # per unit (no fused Res1d blocks).  Off by default: the f16x2 units and their fused blocks stay the f16x2-mode path and
    # MIOpen the path of the other modes.
    exact = False
    # a Res1d block (conv + GN + ReLU + conv + GN + shortcut + ReLU) in ONE launch (lgcn_res1d_gn) instead of two or three
    fuse_blocks = True
    # the two Res1d blocks of a group in ONE launch (lgcn_res1d_pair_gn)
    fuse_groups = True

    def _channels_last_shape_ok(self, actors: Tensor) -> bool:
        mods = [b for g in self.groups for b in g] + [self.output]
        norms = [m for b in mods for m in (b.bn1, b.bn2)] + [l.norm for l in self.lateral]
        return (actors.is_cuda and actors.dtype == torch.float32 and actors.dim() == 3 and actors.shape[0] > 0
                and actors.shape[2] % 4 == 0
                and all(isinstance(n, nn.GroupNorm) and n.num_groups == 1 for n in norms)
                and not any(l.act for l in self.lateral[:-1]))

    def _channels_last_ok(self, actors: Tensor) -> bool:
        return self._channels_last_shape_ok(actors) and not ops.wants_grad(actors, *ops.module_params(self))

    def forward(self, actors: Tensor) -> Tensor:
        if self._hip_ok(actors):
            return self._forward_hip(actors)
        if self._channels_last_ok(actors):
            return self._forward_channels_last(actors)
        pyramid, out = [], actors
        for g in self.groups:
            out = g(out)
            pyramid.append(out)
        out = self.lateral[-1](pyramid[-1])
        for i in range(len(pyramid) - 2, -1, -1):
            lat = self.lateral[i]
            if (out.is_cuda and not ops.wants_grad(out, pyramid[i], *ops.module_params(lat))
                    and isinstance(lat.norm, nn.GroupNorm) and lat.norm.num_groups == 1 and not lat.act
                    and pyramid[i].shape[2] == 2 * out.shape[2]):
                # lateral norm + x2 upsampling of the coarser level + add: one launch
                out = ops.gn_cl(lat.conv(pyramid[i]).contiguous(), lat.norm.weight, lat.norm.bias, lat.norm.eps,
                                res=out.contiguous(), res_up2=True)
            else:
                out = upsample2_linear(out) + lat(pyramid[i])
        return self.output(out)[:, :, -1]


class AttDest(nn.Module):
    """Destination-conditioned actor feature for the mode scores (reference lanegcn.py:713-737)."""

    def __init__(self, n_agt: int):
        super().__init__()
        self.dist = nn.Sequential(nn.Linear(2, n_agt), nn.ReLU(inplace=True), Linear(n_agt, n_agt, norm="GN", ng=1))
        self.agt = Linear(2 * n_agt, n_agt, norm="GN", ng=1)

    def forward(self, agts: Tensor, agt_ctrs: Tensor, dest_ctrs: Tensor) -> Tensor:
        num_mods = dest_ctrs.size(1)
        d = (agt_ctrs.unsqueeze(1) - dest_ctrs).reshape(-1, 2)
        h = F.relu(self.dist[0](d))                                   # nn.Linear(2,128): [rows,2]-shaped, stock op
        return self.from_dist(agts, h, num_mods)

    def from_dist(self, agts: Tensor, h: Tensor, num_mods: int) -> Tensor:
        """The rest of forward() from h = relu(dist[0](agt_ctrs - dest_ctrs)) [A num_mods, n_agt]."""
        n_agt = agts.size(1)
        a = agts.unsqueeze(1).expand(-1, num_mods, -1).reshape(-1, n_agt)
        if agts.is_cuda and n_agt == ops.C_FEAT:
            # dist.2 = Linear+GN+ReLU (one row block); agt = Linear(256 -> 128)+GN+ReLU over cat(dist, agts) = a
            # two-relation row block on the two 128-column halves of its weight (no cat)
            d = A.linear_gn(h, self.dist[2].linear.weight, gn=self.dist[2].norm, relu=True) \
                if ops.wants_grad(h, *self.dist[2].parameters()) else self.dist[2](h)
            w, a = self.agt.linear.weight, a.contiguous()
            if ops.wants_grad(d, a, *self.agt.parameters()):
                return A.row_block([d, a], [w], [A.Rel(0, 0, L.REL_IDENT, 0, 0), A.Rel(1, 0, L.REL_IDENT, 0, 128)],
                                   d.shape[0], gn=self.agt.norm, relu=True)
            return ops.agg_mlp(d.shape[0], [ops.RelSpec(d, ops.packed(w, 0, 128)), ops.RelSpec(a, ops.packed(w, 128, 128))],
                               L.F_GN1 | L.F_RELU1, gn1=_gn(self.agt.norm), eps=self.agt.norm.eps)
        d = group_norm1(F.linear(h, self.dist[2].linear.weight), self.dist[2].norm, relu=True)
        return self.agt(torch.cat((d, a), 1))


class PredNet(nn.Module):
    """6-mode trajectory regression + scoring head (reference lanegcn.py:575-631); stock ATen ops."""

    def __init__(self, config):
        super().__init__()
        self.config = config
        n = config["n_actor"]
        self.pred = nn.ModuleList([nn.Sequential(LinearRes(n, n, norm="GN", ng=1), nn.Linear(n, 2 * config["num_preds"]))
                                   for _ in range(config["num_mods"])])
        self.att_dest = AttDest(n)
        self.cls = nn.Sequential(LinearRes(n, n, norm="GN", ng=1), nn.Linear(n, 1))

    impl = "hip"      # "hip": the stock-op tail on lgcn_pred_reg / lgcn_pred_final (inference); "stock": ATen only
    # training (autograd recording) on the HIP tail too: PredRegFn / PredFinalFn forward and backward instead of the stock
    # GEMM, sort and index ops.  Opt-in, like ActorNet.train_hip: the default training path stays the stock one.
    train_hip = False

    def _shape_ok(self, actors: Tensor) -> bool:
        cfg = self.config
        return (PredNet.impl == "hip" and actors.is_cuda and actors.dtype == torch.float32 and actors.shape[0] > 0
                and cfg["n_actor"] == ops.C_FEAT and cfg["num_mods"] <= 8 and 2 * cfg["num_preds"] <= 64)

    def _hip_ok(self, actors: Tensor) -> bool:
        return self._shape_ok(actors) and not ops.wants_grad(actors, *ops.module_params(self))

    def _train_hip_ok(self, actors: Tensor, actor_ctrs: List[Tensor]) -> bool:
        return (PredNet.train_hip and self._shape_ok(actors) and ops.wants_grad(actors, *ops.module_params(self))
                and not any(c.requires_grad for c in actor_ctrs))

    def forward_flat_train(self, actors: Tensor, ctrs: Tensor):
        """forward_flat (without rot / orig) recorded by autograd, on the same kernels: the heads' LinearRes (LaneConvFn),
        PredRegFn, AttDest's two row blocks, the score head's LinearRes, PredFinalFn."""
        actors = actors.contiguous()
        h = [head[0](actors) for head in self.pred]
        reg, hd = A.PredRegFn.apply(*h, *[head[1].weight for head in self.pred], *[head[1].bias for head in self.pred],
                                    ctrs, self.att_dest.dist[0].weight, self.att_dest.dist[0].bias)
        f = self.cls[0](self.att_dest.from_dist(actors, hd, len(self.pred)))
        return A.PredFinalFn.apply(f, self.cls[1].weight, self.cls[1].bias, reg)

    def forward_flat(self, actors: Tensor, ctrs: Tensor, rot: Optional[Tensor] = None, orig: Optional[Tensor] = None):
        """Inference on the HIP tail: (cls [A, M] descending, reg [A, M, T, 2] in that order) for all actors of the batch;
        with rot [A, 2, 2] / orig [A, 2] (each actor's scene rotation / origin) reg comes out in world coordinates
        (Net.forward's loop, lanegcn.py:147-150).  Launches: the heads' row blocks (two per launch), lgcn_pred_reg,
        AttDest's two row blocks, the score head's LinearRes, lgcn_pred_final."""
        actors = actors.contiguous()
        kws = [head[0].block_kw(actors) for head in self.pred]            # the heads' LinearRes row blocks, two per launch
        h = []
        for i in range(0, len(kws) - 1, 2):
            h += list(ops.agg_mlp_pair(kws[i], kws[i + 1]))
        if len(kws) % 2:
            h.append(ops.agg_mlp(**kws[-1]))
        reg, hd = ops.pred_reg(h, [head[1].weight for head in self.pred], [head[1].bias for head in self.pred],
                               ctrs, self.att_dest.dist[0].weight, self.att_dest.dist[0].bias)
        f = self.cls[0](self.att_dest.from_dist(actors, hd, len(self.pred)))
        return ops.pred_final(f, self.cls[1].weight, self.cls[1].bias, reg, rot, orig)

    def forward(self, actors: Tensor, actor_idcs: List[Tensor], actor_ctrs: List[Tensor]) -> Dict[str, List[Tensor]]:
        if self._hip_ok(actors):
            cls, reg = self.forward_flat(actors, torch.cat(actor_ctrs, 0))
            return {"cls": [cls[i] for i in actor_idcs], "reg": [reg[i] for i in actor_idcs]}
        if self._train_hip_ok(actors, actor_ctrs):
            cls, reg = self.forward_flat_train(actors, torch.cat(actor_ctrs, 0))
            return {"cls": [cls[i] for i in actor_idcs], "reg": [reg[i] for i in actor_idcs]}
        reg = torch.stack([head(actors) for head in self.pred], 1)
        reg = reg.view(reg.size(0), reg.size(1), -1, 2)
        ctrs = torch.cat(actor_ctrs, 0)
        reg = reg + ctrs.view(-1, 1, 1, 2)        # the per-scene loop of :609-612 in one op (idcs partition the rows)
        dest = reg[:, :, -1].detach()
        cls = self.cls(self.att_dest(actors, ctrs, dest)).view(-1, self.config["num_mods"])
        cls, order = cls.sort(1, descending=True)
        rows = torch.arange(len(order), device=order.device).view(-1, 1).expand_as(order)
        reg = reg[rows.reshape(-1), order.reshape(-1)].view(cls.size(0), cls.size(1), -1, 2)
        return {"cls": [cls[i] for i in actor_idcs], "reg": [reg[i] for i in actor_idcs]}


def _own_outputs(gout: Dict) -> Dict:
    """cls / reg of a replayed whole-Net graph live in the graph's static pool: the next replay overwrites them.  The
    caller gets copies (two small device-to-device copies), like the fresh tensors every other path returns."""
    out = dict(gout)
    out["cls"], out["reg"] = gout["cls"].clone(), gout["reg"].clone()
    return out


def _need_nodes(n_nodes: int, n_edges, num_scales: int):
    """The reference's MapNet fails with KeyError("node_idcs") on a batch without a lane node or without an edge in its
    widest pre / suc relation (lanegcn.py:312-322): decided here from the counts, before any launch."""
    if n_nodes == 0 or n_edges[2 * num_scales - 2] == 0 or n_edges[2 * num_scales - 1] == 0:
        raise KeyError("node_idcs")


def _net_replay_or_run(self, eng, hfb, feats, rot, orig, sizes):
    """Whole-Net forward for one host-packed batch (engine.HostFlatBatch + host actor tensors).  A batch whose shapes
    (and the weights' versions) equal the previous call's is captured in a hipGraph once and replayed from then on
    (fixed-size evaluation batches: ~120 eager launches become one replay behind four input copies); anything else
    is uploaded and run eagerly.  Net.graph_cache = False disables it."""
    m = hfb.meta
    sig = (m["n_nodes"], m["n_actors"], tuple(m["n_edges"]), tuple(sizes), m["cap_a2m"], m["cap_a2a"], ops.get_mma(),
           ops.att_pairs_impl(), ops.laneconv_impl(), Att.strict, ActorNet.impl, ActorNet.exact, PredNet.impl,
           sum(p._version for p in ops.module_params(self)))
    st = self.__dict__.setdefault("_graph_state", {"last": None, "sig": None, "graph": None})
    if Net.graph_cache and st["graph"] is not None and st["sig"] == sig:
        g, gfb, gin, gout = st["graph"]
        gfb.buf_view().copy_(hfb.buf, non_blocking=True)
        for dst, src in zip(gin, (feats, rot, orig)):
            dst.copy_(src, non_blocking=True)
        g.replay()
        return gfb, _own_outputs(gout)
    fb = hfb.to()
    dev = fb.node_ctrs.device
    _need_nodes(fb.n_nodes, fb.n_edges, fb.num_scales)
    gin = tuple(t.to(dev, non_blocking=True) for t in (feats, rot, orig))
    if Net.graph_cache and st["last"] == sig:      # second time in a row: worth capturing
        # thread_local: CUDA activity of OTHER threads (a DataLoader's pin_memory thread) must not abort the capture
        g, gout = eng.capture(fb, *gin, sizes, warmup=1, tune_convs=False, capture_error_mode="thread_local")
        st.update(sig=sig, graph=(g, fb, gin, gout))
        g.replay()
        return fb, _own_outputs(gout)
    st["last"] = sig
    return fb, eng.forward(fb, *gin, sizes)


class Net(nn.Module):
    """ActorNet -> [graph_gather -> MapNet -> A2M -> M2M -> M2A -> A2A] -> PredNet (reference lanegcn.py:94-151).
    The bracketed part is the HIP hot path; input and output formats are the reference's."""

    def __init__(self, config):
        super().__init__()
        self.config = config
        self.actor_net = ActorNet(config)
        self.map_net = MapNet(config)
        self.a2m = A2M(config)
        self.m2m = M2M(config)
        self.m2a = M2A(config)
        self.a2a = A2A(config)
        self.pred_net = PredNet(config)

    def forward(self, data: Dict) -> Dict[str, List[Tensor]]:
        if not ops.wants_grad(*ops.module_params(self)) and len(data["feats"]) > 0 and sum(len(x) for x in data["ctrs"]) > 0:
            return self._forward_inference(data)
        actors, actor_idcs = actor_gather(gpu(data["feats"]))
        # graph_gather takes the scenes as they come (CPU or GPU, int16 or int64): one concatenation and
        # one H2D per array instead of utils.gpu's per-leaf copies (lanegcn.py:134)
        out = self._modules_forward(actors, actor_idcs, gpu(data["ctrs"]), graph_gather(to_long(data["graph"])))
        rot, orig = gpu(data["rot"]), gpu(data["orig"])
        for i in range(len(out["reg"])):        # back to world coordinates (:147-150)
            out["reg"][i] = torch.matmul(out["reg"][i], rot[i]) + orig[i].view(1, 1, 1, -1)
        return out

    def _modules_forward(self, actors: Tensor, actor_idcs, actor_ctrs, graph: Dict) -> Dict[str, List[Tensor]]:
        """The seven modules in the reference's order (lanegcn.py:135-146), recorded by autograd -> PredNet's output in
        the scenes' own frames."""
        actors = self.actor_net(actors)
        nodes, node_idcs, node_ctrs = self.map_net(graph)
        nodes = self.a2m(nodes, graph, actors, actor_idcs, actor_ctrs)
        nodes = self.m2m(nodes, graph)
        actors = self.m2a(actors, actor_idcs, actor_ctrs, nodes, node_idcs, node_ctrs)
        actors = self.a2a(actors, actor_idcs, actor_ctrs)
        return self.pred_net(actors, actor_idcs, actor_ctrs)

    graph_cache = True
    _replay_or_run = _net_replay_or_run

    def _full_engine(self):
        """This net's engine.FullNetEngine, made on first use (kept out of the module tree: net.__dict__["_engine"])."""
        eng = self.__dict__.get("_engine")
        if eng is None:
            from .engine import FullNetEngine
            eng = self.__dict__["_engine"] = FullNetEngine(self)
        return eng

    def _forward_inference(self, data: Dict) -> Dict[str, List[Tensor]]:
        """No-grad fast path of forward(): the batch is collated flat on the host (one H2D per array) and run
        through engine.FullNetEngine -- same arithmetic and same outputs as the module path, without its
        per-scene tensor ops.  Error behaviour is kept: KeyError when pre[5] / suc[5] is empty
        (lanegcn.py:312-322) and, while Att.strict, RuntimeError when a fusion block has no pair (:688)."""
        eng = self._full_engine()
        flat = getattr(data, "flat", None)
        if flat is not None:      # packed by this package's collate_fn (in the DataLoader worker)
            hfb, (feats, rot, orig, sizes) = flat
        else:
            from .engine import collate_flat_host, host_actor_inputs
            n = len(data["feats"])
            scenes = [{k: data[k][i] for k in ("feats", "ctrs", "rot", "orig", "graph")} for i in range(n)]
            cpu = lambda t: t.cpu() if torch.is_tensor(t) and t.is_cuda else t
            scenes = [{"feats": cpu(s["feats"]), "ctrs": cpu(s["ctrs"]), "rot": cpu(s["rot"]), "orig": cpu(s["orig"]),
                       "graph": _tree_cpu(s["graph"])} for s in scenes]
            hfb = collate_flat_host(scenes)
            feats, rot, orig, sizes = host_actor_inputs(scenes)
        _need_nodes(hfb.meta["n_nodes"], hfb.meta["n_edges"], hfb.meta["num_scales"])
        fb, out = self._replay_or_run(eng, hfb, feats, rot, orig, sizes)
        return self._finish_inference(eng, fb, out, feats, rot, orig, sizes)

    def _finish_inference(self, eng, fb, out, feats, rot, orig, sizes) -> Dict[str, List[Tensor]]:
        """The host-side checks behind a whole-Net forward `out` of the device batch `fb` (feats / rot / orig: its actor
        inputs, on the host or on the device), then the per-scene lists."""
        out = self._check_inference(eng, fb, out, feats, rot, orig, sizes)
        # per-scene views in two calls (a Python slice per scene and tensor costs ~2 us each: 0.13 ms at batch 32)
        sizes = [int(a) for a in sizes]
        return {"cls": list(torch.split(out["cls"], sizes)), "reg": list(torch.split(out["reg"], sizes))}

    def _check_inference(self, eng, fb, out, feats, rot, orig, sizes) -> Dict:
        """The host-side checks of _finish_inference (engine.HotPathEngine.host_checks: one device->host read; the
        pair-capacity regrow, which drops the cached graph, and the range guard run the forward again -- outside f16x2
        ActorNet runs its exact fp32 units when ActorNet.exact is set and the MIOpen path otherwise, see
        ActorNet._hip_ok) -> the flat engine output that passed them: cls [A, M], reg [A, M, T, 2]."""
        dev = fb.node_ctrs.device
        return eng.hot.host_checks(
            out, lambda: eng.forward(fb, feats.to(dev), rot.to(dev), orig.to(dev), sizes), strict=Att.strict,
            on_regrow=lambda: self.__dict__.get("_graph_state", {}).update(sig=None, graph=None, last=None))

    def forward_store(self, store, indices, replay=None) -> Dict[str, List[Tensor]]:
        """No-grad forward of the scenes `indices` of a flatfile.DeviceSceneStore: the batch is cut out of the resident
        store by one launch (no per-scene host work, no scene dicts) and run eagerly through engine.FullNetEngine.
        Output and error behaviour are those of forward(data) on the same scenes: per-scene lists in world coordinates,
        KeyError when pre[5] / suc[5] is empty, RuntimeError under Att.strict when a fusion block has no pair.
        replay: an engine.StoreReplay of this net and this store -- the pick is padded to its fixed capacities and runs
        through its one captured graph (same outputs; the lists are views that the next call with `replay` overwrites)."""
        if replay is not None:
            if replay.net is not self or replay.store is not store:
                raise L.LgcnError("forward_store: the StoreReplay was made for another net or another store")
            fb, ex, out = replay.forward(indices)
        else:
            fb, ex, out = self.forward_store_flat(store, indices)
        sizes = [int(a) for a in ex["sizes"]]
        return {"cls": list(torch.split(out["cls"], sizes)), "reg": list(torch.split(out["reg"], sizes))}

    def forward_raw(self, raws, tables, lane_ids=None) -> Dict[str, List[Tensor]]:
        """No-grad forward of raw scenes (data_raw's raw-scene dicts and {city: LaneTable}): data_raw.build_store with
        this net's config (pred_range, num_scales, cross_dist), then forward_store over all its scenes -- raw tracks to
        predictions without a scene dict and without a trip through the host.  Output and errors are forward_store's,
        after build_store's own."""
        from . import data_raw
        store = data_raw.build_store(raws, tables, self.config, lane_ids=lane_ids)
        return self.forward_store(store, np.arange(len(store)))

    def forward_store_flat(self, store, indices, plan=None):
        """forward_store before its outputs are cut into per-scene lists -> (fb, ex, out): the FlatBatch and the extras of
        store.batch(indices), and the flat engine output behind the host-side checks (out["cls"] [A, M], out["reg"]
        [A, M, T, 2] in world coordinates, actor rows in batch order).  Errors as forward_store's."""
        eng = self._full_engine()
        plan = store.plan(indices) if plan is None else plan
        _need_nodes(plan.n_nodes, plan.n_edges, plan.num_scales)
        if plan.n_actors == 0:
            raise L.LgcnError("forward_store: the picked scenes hold no actor")
        with torch.no_grad():
            fb, ex = store.batch(indices, plan=plan)
            feats, rot, orig, sizes = ex["actor_feats"], ex["rot"], ex["orig"], ex["sizes"]
            out = eng.forward(fb, feats, rot, orig, sizes)
            return fb, ex, self._check_inference(eng, fb, out, feats, rot, orig, sizes)

    def forward_store_train(self, store, indices, rot_dt=None):
        """Training forward of the scenes `indices` of a flatfile.DeviceSceneStore -> (out, data): the modules of
        forward(data)'s grad branch in the same order, fed with the flat tensors of the store's batch (one launch; with
        `rot_dt`, one angle per pick, turned inside it as the reference's rot_aug turns a scene) -- no scene dicts, no
        actor_gather / graph_gather / utils.gpu.  `out`: per-scene cls / reg lists in world coordinates, recorded by
        autograd.  `data`: what Loss.forward reads (gt_preds, has_preds: per-scene lists of device views) and the frame
        (rot, orig per scene -- None for a scene without actors, which has no row in the batch -- and ctrs).  Errors as
        forward_store's, decided from the plan before any launch; a store without gt_preds raises LgcnError."""
        from .engine import flat_graph
        plan = store.plan(indices)
        _need_nodes(plan.n_nodes, plan.n_edges, plan.num_scales)
        if plan.n_actors == 0:
            raise L.LgcnError("forward_store_train: the picked scenes hold no actor")
        if not store.has_gt:
            raise L.LgcnError("forward_store_train: the store holds no gt_preds / has_preds to train against")
        fb, ex = store.batch(indices, plan=plan, rot_dt=rot_dt)
        sizes = ex["sizes"]
        actor_idcs = list(torch.split(torch.arange(fb.n_actors, device=fb.actor_ctrs.device), sizes))
        actor_ctrs = list(torch.split(fb.actor_ctrs, sizes))
        out = self._modules_forward(ex["actor_feats"], actor_idcs, actor_ctrs, flat_graph(fb))
        # the scene's rot / orig: the row of its first actor (the batch holds them per actor)
        first = plan.actor_off[:-1].tolist()
        rot = [ex["rot"][o] if n else None for o, n in zip(first, sizes)]
        orig = [ex["orig"][o] if n else None for o, n in zip(first, sizes)]
        for i in range(len(out["reg"])):        # back to world coordinates, as forward(data) does
            if sizes[i]:
                out["reg"][i] = torch.matmul(out["reg"][i], rot[i]) + orig[i].view(1, 1, 1, -1)
        data = {"gt_preds": list(torch.split(ex["gt_preds"], sizes)), "has_preds": list(torch.split(ex["has_preds"], sizes)),
                "rot": rot, "orig": orig, "ctrs": actor_ctrs}
        if "theta" in ex:
            data["theta"] = ex["theta"]
        return out, data


def _tree_cpu(x):
    if isinstance(x, dict):
        return {k: _tree_cpu(v) for k, v in x.items()}
    if isinstance(x, (list, tuple)):
        return [_tree_cpu(v) for v in x]
    return x.cpu() if torch.is_tensor(x) and x.is_cuda else x


class PredLoss(nn.Module):
    """Max-margin mode classification + SmoothL1 regression of the closest mode (reference lanegcn.py:740-807)."""

    impl = "hip"      # "stock": the ATen composition below

    def __init__(self, config):
        super().__init__()
        self.config = config
        self.reg_loss = nn.SmoothL1Loss(reduction="sum")

    def forward(self, out, gt_preds, has_preds):
        cfg = self.config
        cls, reg = torch.cat(list(out["cls"]), 0), torch.cat(list(out["reg"]), 0)
        gt_preds, has_preds = torch.cat(list(gt_preds), 0), torch.cat(list(has_preds), 0)
        if (PredLoss.impl == "hip" and cls.is_cuda and cls.dtype == torch.float32 and reg.dim() == 4 and cls.shape[1] <= 8
                and reg.shape[2] <= 64 and has_preds.dtype == torch.bool):
            # one launch forward, one backward (csrc/lgcn_loss.hip); the counts come back in ONE 8-byte read -- the
            # reference reads them with two .item() calls (:801, :807)
            c_loss, r_loss, counts = A.PredLossFn.apply(cls, reg, gt_preds.float().contiguous(), has_preds.contiguous(), cfg)
            n_cls, n_reg = counts.tolist()
            return {"cls_loss": c_loss, "num_cls": n_cls, "reg_loss": r_loss, "num_reg": n_reg}
        zero = 0.0 * (cls.sum() + reg.sum())
        loss_out = {"cls_loss": zero.clone(), "num_cls": 0, "reg_loss": zero.clone(), "num_reg": 0}
        num_mods, num_preds = cfg["num_mods"], cfg["num_preds"]
        # last observed step per actor; actors whose only observed step is t=0 are dropped
        last = has_preds.float() + 0.1 * torch.arange(num_preds, device=has_preds.device).float() / float(num_preds)
        max_last, last_idcs = last.max(1)
        keep = max_last > 1.0
        cls, reg, gt_preds, has_preds, last_idcs = cls[keep], reg[keep], gt_preds[keep], has_preds[keep], last_idcs[keep]
        rows = torch.arange(len(last_idcs), device=last_idcs.device)
        dist = torch.stack([torch.sqrt(((reg[rows, j, last_idcs] - gt_preds[rows, last_idcs]) ** 2).sum(1))
                            for j in range(num_mods)], 1)
        min_dist, min_idcs = dist.min(1)
        mgn = cls[rows, min_idcs].unsqueeze(1) - cls
        mask0 = (min_dist < cfg["cls_th"]).view(-1, 1)
        mask1 = dist - min_dist.view(-1, 1) > cfg["cls_ignore"]
        mgn = mgn[mask0 * mask1]
        hit = mgn < cfg["mgn"]
        loss_out["cls_loss"] += cfg["cls_coef"] * (cfg["mgn"] * hit.sum() - mgn[hit].sum())
        loss_out["num_cls"] += hit.sum().item()
        best = reg[rows, min_idcs]
        loss_out["reg_loss"] += cfg["reg_coef"] * self.reg_loss(best[has_preds], gt_preds[has_preds])
        loss_out["num_reg"] += has_preds.sum().item()
        return loss_out


class Loss(nn.Module):
    def __init__(self, config):
        super().__init__()
        self.config = config
        self.pred_loss = PredLoss(config)

    def forward(self, out: Dict, data: Dict) -> Dict:
        loss_out = self.pred_loss(out, gpu(data["gt_preds"]), gpu(data["has_preds"]))
        loss_out["loss"] = (loss_out["cls_loss"] / (loss_out["num_cls"] + 1e-10)
                            + loss_out["reg_loss"] / (loss_out["num_reg"] + 1e-10))
        return loss_out


def pred_metrics(preds, gt_preds, has_preds):
    """ade1, fde1, ade, fde, min_idcs (reference lanegcn.py:883-899)."""
    assert has_preds.all()
    preds, gt_preds = np.asarray(preds, np.float32), np.asarray(gt_preds, np.float32)
    err = np.sqrt(((preds - np.expand_dims(gt_preds, 1)) ** 2).sum(3))
    ade1, fde1 = err[:, 0].mean(), err[:, 0, -1].mean()
    min_idcs = err[:, :, -1].argmin(1)
    best = err[np.arange(len(min_idcs)), min_idcs]
    return ade1, fde1, best.mean(), best[:, -1].mean(), min_idcs


class PostProcess(nn.Module):
    """Collects the first actor's predictions per scene and prints ADE/FDE (reference lanegcn.py:824-880)."""

    def __init__(self, config):
        super().__init__()
        self.config = config

    def forward(self, out, data):
        return {"preds": [x[0:1].detach().cpu().numpy() for x in out["reg"]],
                "gt_preds": [x[0:1].numpy() for x in data["gt_preds"]],
                "has_preds": [x[0:1].numpy() for x in data["has_preds"]]}

    def append(self, metrics: Dict, loss_out: Dict, post_out=None) -> Dict:
        if len(metrics.keys()) == 0:
            for key in loss_out:
                if key != "loss":
                    metrics[key] = 0.0
            for key in post_out:
                metrics[key] = []
        for key, val in loss_out.items():
            if key != "loss":
                metrics[key] += val.item() if isinstance(val, torch.Tensor) else val
        for key in post_out:
            metrics[key] += post_out[key]
        return metrics

    def display(self, metrics, dt, epoch, lr=None):
        if lr is not None:
            print("Epoch %3.3f, lr %.5f, time %3.2f" % (epoch, lr, dt))
        else:
            print("************************* Validation, time %3.2f *************************" % dt)
        cls = metrics["cls_loss"] / (metrics["num_cls"] + 1e-10)
        reg = metrics["reg_loss"] / (metrics["num_reg"] + 1e-10)
        ade1, fde1, ade, fde, _ = pred_metrics(np.concatenate(metrics["preds"], 0), np.concatenate(metrics["gt_preds"], 0),
                                               np.concatenate(metrics["has_preds"], 0))
        print("loss %2.4f %2.4f %2.4f, ade1 %2.4f, fde1 %2.4f, ade %2.4f, fde %2.4f"
              % (cls + reg, cls, reg, ade1, fde1, ade, fde))
        print()


def get_model():
    """The reference's plugin entry point (lanegcn.py:902-913; called by train.py:63-64, test.py:57):
    (config, Dataset, collate_fn, net, loss, post_process, opt)."""
    from .data import SyntheticArgoDataset
    # Dataset: the reference returns its ArgoDataset (needs argoverse-api and the dataset, both absent here).  A caller
    # that has them injects the class as config["dataset_cls"]; the synthetic generator is the explicit fallback and
    # says so when it is handed a split path (data.SyntheticArgoDataset).  No process-wide switches are flipped here
    # (train_dp.py turns off autograd's device thread for its own loop).
    Dataset = config.get("dataset_cls") or SyntheticArgoDataset
    net = Net(config).cuda()
    loss = Loss(config).cuda()
    post_process = PostProcess(config).cuda()
    opt = Optimizer(net.parameters(), config)
    return config, Dataset, collate_fn, net, loss, post_process, opt
