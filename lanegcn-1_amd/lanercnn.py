"""Second consumer of the two hot kernels: the graph modules of the reference's fork
model lanercnn.py on the same HIP row-block / LaneConv / pair kernels.

Same class names, constructor arguments, forward signatures and state_dict names as the reference:
  LaneInput      lanercnn.py:280-351  map_fc(8 -> 128) + index_add_ of agt_fc(80 -> 128) over a2m edges -> GN -> ReLU
  LaneRoI        lanercnn.py:354-430  Linear(input_dim -> 128, GN, ReLU) + 4 LaneConv layers
  GlobalGraphNet lanercnn.py:517-600  4 LaneConv layers on a given feature
  LanePooling    lanercnn.py:433-514  distance-gated pooling between two lane graphs: the Att pattern with a 4-d
                                      relative pose instead of the 2-d offset and without a query term
  Interactor     lanercnn.py:603-642  stem (MapNet's input form) -> LanePooling -> GlobalGraphNet -> LanePooling
  Decode         lanercnn.py:740-924  goal head, NMS + trajectory coefficients (lgcn_goal_decode), pooling of the agent's
                                      motion into its RoI, refinement head, refined trajectories (lgcn_goal_refine)
  RoiLoss / Loss :1205-1325           BCE of the mode logits against the mode closest to the last observed step +
                                      SmoothL1 of that mode's goal and trajectory: lgcn_roi_loss_fwd / _bwd, one launch each
  PostProcess    :1328-1423           and pred_metrics / pred_metrics_ade (:1426-1463), host-side bookkeeping
and the module-level nms_select / compute_coefficent / sample_trajectory / sample_d1_trajectory (:687-737); on top of
them the whole model:
  config         :30-82               the reference's keys and values
  Net            :85-119              input -> roi_net1 -> interactor -> roi_net2 -> decode on a collated batch
  subgraph_gather / graph_gather :122-277   lane RoIs / scenes merged into one block-diagonal graph each; every index
                                      array offset by one lgcn_graph_gather launch
  get_model / get_model_for_torch_dist :1466-1490   the plugin entry points (lanercnn_mi355x.py loads them by name)

Inference (no_grad) runs on the HIP kernels; under autograd LaneRoI / GlobalGraphNet train through the LaneConv
autograd path of lanegcn.py, LanePooling and LaneInput through the row-block / pair / gather Functions of autograd.py
(the same composition as Att.run_train): every 128-d contraction of the backward is a HIP launch as well.
"""
import os
from math import gcd
from typing import Dict, List, Tuple

import numpy as np
import torch
from torch import Tensor, nn
from torch.nn import functional as F

from . import _lib as L
from . import autograd as A
from . import ops
from . import lanegcn as _base
from .data import collate_fn
from .data_lrcnn import RoiBatch
from .lanegcn import _fuse_modules, _gn, build_pairs, lane_conv, lane_conv_train, lane_plan, lane_plan_t, rel_keys
from .layers import Linear
from .utils import Optimizer, StepLR, gpu, to_long

file_path = os.path.abspath(__file__)
root_path = os.path.dirname(file_path)
model_name = os.path.basename(file_path).split(".")[0]

# Same keys and values as the reference's module-level config (lanercnn.py:30-82).
config = dict(
    display_iters=205942, val_iters=205942 * 2, save_freq=1.0, epoch=0, horovod=True, opt="adamw",
    num_epochs=36, lr=[1e-3, 1e-4], lr_epochs=[32], weight_decay=0.01,
    batch_size=10, val_batch_size=10, workers=0, val_workers=0,
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


def _need_cuda(*ts):
    for t in ts:
        if torch.is_tensor(t) and not t.is_cuda:
            raise L.LgcnError("lanercnn modules need CUDA tensors (the HIP hot path has no CPU fallback)")


# ------------------------------------------------------------------ gathers (reference lanercnn.py:122-277)
def subgraph_bookkeeping(subgraphs_in_batch) -> Dict:
    """The host side of subgraph_gather (lanercnn.py:125-163): everything that is a Python int or list in the reference's
    dict -- num_nodes, counts (node offset per RoI), batch_spans, num_atgs_per_batch, roi_spans -- plus interest_roi (the
    first RoI of every scene, a CPU LongTensor).  Reads only the RoI sizes; touches no GPU."""
    counts, num_atgs, batch_spans, interest, count = [], [], [], [], 0
    for b, subgraphs in enumerate(subgraphs_in_batch):
        assert len(subgraphs) > 0, "batch {} have empty subgraphs".format(b)               # lanercnn.py:180
        interest.append(len(counts))
        num_atgs.append(len(subgraphs))
        start = count
        for sg in subgraphs:
            counts.append(count)
            count += int(len(sg["feats"]))
        batch_spans.append([start, count])
    ends = counts[1:] + [count]
    return {"num_nodes": count, "counts": counts, "batch_spans": batch_spans, "num_atgs_per_batch": num_atgs,
            "roi_spans": [[lo, hi] for lo, hi in zip(counts, ends)],
            "interest_roi": torch.tensor(interest, dtype=torch.long)}


def _as_tensor(x) -> Tensor:
    return x if torch.is_tensor(x) else torch.from_numpy(np.ascontiguousarray(x))


def _offset_indices(pieces: List, bases: List[int], dev) -> Tuple[Tensor, np.ndarray]:
    """out[e] = piece(e)[.] + base(piece) for the concatenation of `pieces` (numpy arrays, CPU or GPU tensors of any
    integer type) with ONE lgcn_graph_gather launch: (int64 device tensor, element offsets of the pieces)."""
    pieces = [_as_tensor(x).reshape(-1) for x in pieces]
    off = np.zeros(len(pieces) + 1, np.int64)
    np.cumsum([int(x.numel()) for x in pieces], out=off[1:])
    if any(x.is_cuda for x in pieces):
        flat = torch.cat([x.to(dev).long() for x in pieces], 0)
    else:      # one host concatenation, one copy
        flat = torch.from_numpy(np.concatenate([x.numpy().astype(np.int64, copy=False) for x in pieces]
                                              + [np.zeros(0, np.int64)])).to(dev, non_blocking=True)
    if flat.numel() == 0:
        return flat, off
    tables = torch.from_numpy(np.stack([off, np.asarray(list(bases) + [0], np.int64)])).to(dev)
    out64, _ = ops.graph_gather_indices(flat, tables[0].contiguous(), tables[1, :-1].contiguous())
    return out64, off


def subgraph_gather(subgraphs_in_batch) -> Dict:
    """Merge the lane RoIs of a batch into one block-diagonal graph (reference lanercnn.py:122-231): the reference's
    dict, key for key.  The 28 local index arrays of every RoI and its two a2m arrays are offset by ONE
    lgcn_graph_gather launch over one concatenation (segment base: the RoI's node offset, or the RoI's number for
    a2m.u) instead of hundreds of adds and cats.  Leaves may be numpy arrays, CPU or GPU tensors, int16 / int32 / int64.
    A relation without edges comes out as an empty int64 tensor (the reference's float zeros((0,)) is not mirrored).

    A data_lrcnn.RoiBatch in the place of the lists (the flat route) already holds the merged graph: the same dict comes
    out of views of its buffers, without a launch or a concatenation (_subgraph_views)."""
    if isinstance(subgraphs_in_batch, RoiBatch):
        return _subgraph_views(subgraphs_in_batch)
    graph = subgraph_bookkeeping(subgraphs_in_batch)
    dev = torch.device("cuda", torch.cuda.current_device())
    counts = graph["counts"]
    rois = [sg for subgraphs in subgraphs_in_batch for sg in subgraphs]
    graph["node_idcs"] = torch.arange(graph["num_nodes"], device=dev)
    fdev = lambda x: _as_tensor(x).to(dev, non_blocking=True)
    feats, agt_feat = [], []
    for subgraphs in subgraphs_in_batch:
        feats.append(torch.cat([fdev(sg["feats"]) for sg in subgraphs], 0))
        agt_feat.append(torch.cat([fdev(sg["agent_feat"]).view(1, -1) for sg in subgraphs], 0))
    graph["feats"], graph["agent_feat"] = feats, agt_feat
    graph["ctrs"] = [f[:, :2] for f in feats]
    graph["dirs"] = [f[:, 2:4] for f in feats]
    graph["pose"] = [f[:, :4] for f in feats]
    graph["agent_vel"] = [sg["agent_vel"] for sg in rois]

    num_scales = len(rois[0]["pre"])
    getters = [lambda sg, k1=k1, i=i, k2=k2: sg[k1][i][k2] for k1 in ("pre", "suc") for i in range(num_scales) for k2 in "uv"]
    getters += [lambda sg, k1=k1, k2=k2: sg[k1][k2] for k1 in ("left", "right") for k2 in "uv"]
    getters += [lambda sg: sg["a2m"]["u"], lambda sg: sg["a2m"]["v"]]
    pieces = [get(sg) for get in getters for sg in rois]
    bases = [list(range(len(rois))) if j == len(getters) - 2 else counts for j in range(len(getters))]
    out64, off = _offset_indices(pieces, [b for bs in bases for b in bs], dev)
    R = len(rois)
    it = iter(out64[off[j * R]:off[(j + 1) * R]] for j in range(len(getters)))
    for k1 in ("pre", "suc"):
        graph[k1] = [{"u": next(it), "v": next(it)} for _ in range(num_scales)]
    for k1 in ("left", "right"):
        graph[k1] = {"u": next(it), "v": next(it)}
    graph["a2m"] = {"u": next(it), "v": next(it)}
    return graph


def _subgraph_views(rb: RoiBatch) -> Dict:
    """subgraph_gather's dict out of a RoiBatch: its host bookkeeping, S-way splits of the flat feature buffers and one
    slice per relation of the four index arrays.  The number of tensor ops depends on the scenes, never on the RoIs."""
    graph = rb.bookkeeping()
    nodes = [hi - lo for lo, hi in graph["batch_spans"]]
    graph["node_idcs"] = torch.arange(graph["num_nodes"], device=rb.feats.device)
    graph["feats"] = list(rb.feats.split(nodes))
    graph["agent_feat"] = list(rb.agent_feat.split(graph["num_atgs_per_batch"]))
    graph["ctrs"] = list(rb.feats[:, :2].split(nodes))
    graph["dirs"] = list(rb.feats[:, 2:4].split(nodes))
    graph["pose"] = list(rb.feats[:, :4].split(nodes))
    graph["agent_vel"] = list(rb.agent_vel)
    ext = rb.rel_ext.tolist()
    rel = [{"u": rb.u[lo:hi], "v": rb.v[lo:hi]} for lo, hi in zip(ext[:-1], ext[1:])]
    graph["pre"], graph["suc"], graph["left"], graph["right"] = rel[0:6], rel[6:12], rel[12], rel[13]
    graph["a2m"] = {"u": rb.a2m_u, "v": rb.a2m_v}
    return graph


def graph_gather(graphs: List[Dict]) -> Dict:
    """lanegcn.graph_gather plus the fork's num_nodes, counts and pose = cat(ctrs, feats) per scene (reference
    lanercnn.py:234-277)."""
    graph = _base.graph_gather(graphs)
    dev = graph["feats"].device
    graph["num_nodes"] = [int(g["num_nodes"]) for g in graphs]
    graph["counts"] = [int(v) for v in np.cumsum([0] + graph["num_nodes"][:-1])]
    graph["pose"] = [torch.cat([c, g["feats"].to(dev, non_blocking=True)], -1) for c, g in zip(graph["ctrs"], graphs)]
    return graph


class LaneInput(nn.Module):
    """Lane-RoI input encoder (reference lanercnn.py:280-351)."""

    def __init__(self, config):
        super().__init__()
        map_dim = config["n_map"]
        self.map_fc = nn.Linear(8, map_dim, bias=False)
        self.agt_fc = nn.Linear(80, map_dim, bias=False)
        self.bn = nn.GroupNorm(gcd(1, map_dim), map_dim)
        self.relu = nn.ReLU(inplace=True)

    def forward(self, graph: Dict) -> Tensor:
        map_feats = torch.cat(graph["feats"], 0)            # [nodes, 8]
        agt_feats = torch.cat(graph["agent_feat"], 0)       # [agts, 80]
        _need_cuda(map_feats, agt_feats)
        train = ops.wants_grad(map_feats, agt_feats, *ops.module_params(self))
        n = map_feats.shape[0]
        # the two Linears have K = 8 / 80 (not 128-d contractions): stock ops; agt_fc commutes with the gather
        base = self.map_fc(map_feats)
        agt = self.agt_fc(agt_feats)
        u, v = graph["a2m"]["u"].long(), graph["a2m"]["v"].long()
        if u.numel() > 0:
            # one relation: key(n, 0) = n, i.e. a plain CSR by node (sized for the larger index space: the builder
            # bounds-checks sources and destinations against the same count)
            rows = max(n, agt.shape[0])
            plan = ops.csr_build([v], [u], rows)
            if train:      # the gather's transpose = the same gather over the CSR by source
                base = base + A.GatherSumFn.apply(agt, plan, ops.csr_build([u], [v], rows), n)
            else:
                base = base + ops.gather_sum(agt, plan.rowptr, plan.col, n)
        if train:
            return A.gn_act(base.contiguous(), gn=self.bn, relu=True)
        return ops.gn_fwd(base.contiguous(), _gn(self.bn), relu=True, eps=self.bn.eps)


class _UnusedParamsFn(torch.autograd.Function):
    """Identity on x that hands zero gradients to parameters the forward did not read.  lane_conv_train leaves out a
    relation without a single edge in the batch (its term is an empty sum); the reference's empty index_add_ leaves a
    zero gradient on that relation's weights, not None, so every parameter of the fork's Net receives a gradient and the
    optimizer's weight decay reaches it."""

    @staticmethod
    def forward(ctx, x, *params):
        ctx.save_for_backward(*params)
        return x.view_as(x)

    @staticmethod
    def backward(ctx, g):
        return (g, *[torch.zeros_like(p) for p in ctx.saved_tensors])


def _lane_conv_train(fuse: nn.ModuleDict, feat: Tensor, graph: Dict) -> Tensor:
    plan, num_scales = lane_plan(graph), len(graph["pre"])
    out = lane_conv_train(fuse, feat, plan, lane_plan_t(graph), num_scales)
    unused = [m.weight for r, key in enumerate(rel_keys(num_scales)) if plan.n_edges[r] == 0 for m in fuse[key]]
    return _UnusedParamsFn.apply(out, *unused) if unused else out


class LaneRoI(nn.Module):
    """Lane-RoI encoder: input Linear + 4 LaneConv layers (reference lanercnn.py:354-430)."""

    def __init__(self, config, input_dim):
        super().__init__()
        self.config = config
        map_dim = config["n_map"]
        self.input = Linear(input_dim, map_dim, norm="GN", ng=1, act=True)
        self.fuse = _fuse_modules(map_dim, config["num_scales"])
        self.relu = nn.ReLU(inplace=True)

    def forward(self, feat: Tensor, graph: Dict) -> Tensor:
        _need_cuda(feat)
        feat = self.input(feat)
        if ops.wants_grad(feat, *ops.module_params(self)):
            return _lane_conv_train(self.fuse, feat, graph)
        return ops.guarded(lambda: lane_conv(self.fuse, feat, lane_plan(graph), len(graph["pre"])))


class GlobalGraphNet(nn.Module):
    """4 LaneConv layers over the global lane graph (reference lanercnn.py:517-600)."""

    def __init__(self, config):
        super().__init__()
        self.config = config
        self.fuse = _fuse_modules(config["n_map"], config["num_scales"])
        self.relu = nn.ReLU(inplace=True)

    def forward(self, feat: Tensor, graph: Dict):
        if len(graph["feats"]) == 0 or len(graph["pre"][-1]["u"]) == 0 or len(graph["suc"][-1]["u"]) == 0:
            temp = graph["feats"]                            # the reference returns a 1-tuple here (:538-544)
            return (temp.new().resize_(0),)
        _need_cuda(feat)
        if ops.wants_grad(feat, *ops.module_params(self)):
            return _lane_conv_train(self.fuse, feat, graph)
        return ops.guarded(lambda: lane_conv(self.fuse, feat, lane_plan(graph), len(graph["pre"])))


class LanePooling(nn.Module):
    """Distance-gated pooling of a context lane graph into a target lane graph (reference lanercnn.py:433-514)."""
    legacy_offsets = True     # scenes without a pair do not advance the index offsets (lanercnn.py:476-483)
    # Run the pair stage (:492-499: relative pose, relpose.0, ctx.0's pose half + the context row block, GroupNorm, ReLU)
    # of a forward that needs no gradient as ONE exact-fp32 launch (lgcn_pool_pairs) instead of the chain of generic
    # ones; only m [P,128] reaches memory.  Under autograd this switch is ignored (train_hip below decides).  Opt-in; read
    # on each forward.
    fused = False
    # Train the pair stage on the fused exact-fp32 pair of autograd.PoolPairsFn (lgcn_pool_pairs_train /
    # lgcn_pool_pairs_bwd) instead of the composition of row blocks in _run: no [P,128] tensor is saved, one (dz) is written
    # in the backward, and the pair stage's training forward is bit for bit the launch of `fused`.  The tail then takes the
    # segment sum S as a plain source, so its backward is eligible for RowBlockFn.train_hip; it sums m before ctx.1 in
    # another order than the inference tail's RANGE relation, so the MODULE's training forward may still differ from its
    # no_grad forward in the last bits.  Opt-in, like Att.train_hip: the default training path stays the composed one.
    # Read on each forward.
    train_hip = False

    def __init__(self, in_dim: int, out_dim: int) -> None:
        super().__init__()
        in_dim, mid_dim, out_dim = 128, 128, 128             # the reference overrides its arguments (:438)
        self.input = nn.Linear(in_dim, mid_dim, bias=False)
        self.relpose = nn.Sequential(nn.Linear(4, in_dim), nn.ReLU(inplace=True))
        self.ctx = nn.Sequential(Linear(in_dim * 2, mid_dim, norm="GN", ng=1), nn.Linear(mid_dim, mid_dim, bias=False))
        self.mlp = nn.Sequential(Linear(mid_dim, mid_dim, norm="GN", ng=1),
                                 Linear(mid_dim, out_dim, norm="GN", ng=1, act=False))
        self.norm = nn.GroupNorm(gcd(1, 128), 128)
        self.relu = nn.ReLU(inplace=True)

    def forward(self, context_feat: Tensor, context_graph: Dict, target_feat: Tensor, target_graph: Dict,
                dist_th: float = 6.0, g2r: bool = False) -> Tensor:
        _need_cuda(context_feat, target_feat)
        if ops.wants_grad(context_feat, target_feat, *ops.module_params(self)):
            return self._run(context_feat, context_graph, target_feat, target_graph, dist_th, train=True)
        return ops.guarded(lambda: self._run(context_feat, context_graph, target_feat, target_graph, dist_th))

    def _run(self, context_feat, context_graph, target_feat, target_graph, dist_th, train=False):
        c_ctrs, t_ctrs = context_graph["ctrs"], target_graph["ctrs"]
        # The reference lists the pairs context-major (hi = context row, wi = target row) and index_add_s them by
        # TARGET (:509): for one target the contributions arrive in ascending context order.  Searching with the
        # target as the row side gives exactly those segments, contiguous and in that order (and the same numbering
        # quirk: a scene without pairs advances neither offset).
        idc = lambda ctrs: [torch.arange(len(c)) for c in ctrs]
        ps = build_pairs(idc(t_ctrs), t_ctrs, idc(c_ctrs), c_ctrs, dist_th, self.legacy_offsets)
        P = ps.count()
        if P == 0:
            raise RuntimeError("torch.cat(): expected a non-empty list of Tensors")          # lanercnn.py:484
        T = target_feat.shape[0]
        c_pose = torch.cat(context_graph["pose"], 0)
        t_pose = torch.cat(target_graph["pose"], 0)
        w0 = self.ctx[0].linear.weight                                                     # [128, 256] = [feat | pose]
        if not train and LanePooling.fused:
            per_ctx = ops.agg_mlp(context_feat.shape[0], [ops.RelSpec(context_feat, ops.packed(w0, 0, 128))], 0)
            m = ops.pool_pairs(ps, c_pose, t_pose, self.relpose[0].weight, self.relpose[0].bias, w0, per_ctx,
                               _gn(self.ctx[0].norm), cap=P, eps=self.ctx[0].norm.eps)
            return self._tail(m, ps, target_feat)
        if train and self._train_hip_ok(context_feat, target_feat, c_pose, t_pose, ps):
            return self.run_train_hip(context_feat, target_feat, c_pose, t_pose, ps)
        t_idx, c_idx = ps.hi[:P].long(), ps.wi[:P].long()
        h = F.relu(self.relpose[0](c_pose[c_idx] - t_pose[t_idx]))                        # [P,128]; K = 4: stock op
        if train:      # the differentiable composition of the same arithmetic (cf. Att.run_train)
            m0, m1 = self.mlp[0], self.mlp[1]
            per_ctx = A.linear_gn(context_feat, w0, col0=0)
            per_pair = A.linear_gn(h.contiguous(), w0, col0=128)
            no_query = torch.zeros((T, ops.C_FEAT), dtype=torch.float32, device=per_pair.device)
            pre = A.PairAddFn.apply(per_pair, no_query, per_ctx, ps)                    # + per_ctx[context row of the pair]
            m = A.gn_act(pre, gn=self.ctx[0].norm, relu=True)
            y = A.row_block([target_feat, m], [self.input.weight, self.ctx[1].weight],
                            [A.Rel(0, 0, L.REL_IDENT), A.Rel(1, 1, L.REL_RANGE)], T, gn=self.norm, relu=True,
                            rowptr=ps.rowptr, seg_ids=ps.hi, n_seg_rows=ps.n_pairs)
            y = A.linear_gn(y, m0.linear.weight, gn=m0.norm, relu=True)
            return A.linear_gn(y, m1.linear.weight, gn=m1.norm, relu=True, res=target_feat)
        per_ctx = ops.agg_mlp(context_feat.shape[0], [ops.RelSpec(context_feat, ops.packed(w0, 0, 128))], 0)
        per_pair = ops.agg_mlp(P, [ops.RelSpec(h.contiguous(), ops.packed(w0, 128, 128))], 0)
        zero_row = torch.zeros((1, ops.C_FEAT), dtype=torch.float32, device=per_pair.device)
        zero_idx = torch.zeros(P, dtype=torch.int32, device=per_pair.device)
        pre = ops.pair_add(per_pair, per_ctx, ps.wi, zero_row, zero_idx, ps.n_pairs, P)
        m = ops.gn_fwd(pre, _gn(self.ctx[0].norm), relu=True, eps=self.ctx[0].norm.eps)
        return self._tail(m, ps, target_feat)

    def _train_hip_ok(self, context_feat, target_feat, c_pose, t_pose, ps) -> bool:
        rows_ok = max(context_feat.shape[0], target_feat.shape[0]) < (1 << 23)
        return (LanePooling.train_hip and context_feat.is_cuda and context_feat.dtype == torch.float32
                and target_feat.dtype == torch.float32 and context_feat.shape[1] == ops.C_FEAT
                and target_feat.shape[1] == ops.C_FEAT and c_pose.dtype == torch.float32 and t_pose.dtype == torch.float32
                and c_pose.dim() == 2 and t_pose.dim() == 2 and c_pose.shape[1] == 4 and t_pose.shape[1] == 4
                and rows_ok and ps.count() > 0 and not (c_pose.requires_grad or t_pose.requires_grad))

    def run_train_hip(self, context_feat, target_feat, c_pose, t_pose, ps):
        """The training path of _run with the pair stage on PoolPairsFn: U and the two mlp blocks are the same row blocks;
        the segment sum S comes out of the pair stage, and ctx.1 (linear) is applied to it as an IDENT relation."""
        T = target_feat.shape[0]
        w0, c0, rp = self.ctx[0].linear.weight, self.ctx[0].norm, self.relpose[0]
        m0, m1 = self.mlp[0], self.mlp[1]
        U = A.linear_gn(context_feat, w0, col0=0)
        S = A.PoolPairsFn.apply(ps, c_pose, t_pose, rp.weight, rp.bias, w0, U, c0.weight, c0.bias, c0.eps)
        y = A.row_block([target_feat, S], [self.input.weight, self.ctx[1].weight],
                        [A.Rel(0, 0, L.REL_IDENT), A.Rel(1, 1, L.REL_IDENT)], T, gn=self.norm, relu=True)
        y = A.linear_gn(y, m0.linear.weight, gn=m0.norm, relu=True)
        return A.linear_gn(y, m1.linear.weight, gn=m1.norm, relu=True, res=target_feat)

    def _tail(self, m, ps, target_feat):
        T = target_feat.shape[0]
        m0, m1 = self.mlp[0], self.mlp[1]
        # ctx.1 is linear: applied to the per-target segment sum (pairs sorted by target: a RANGE relation)
        y = ops.agg_mlp(T, [ops.RelSpec(target_feat, ops.packed(self.input.weight)),
                            ops.RelSpec(m, ops.packed(self.ctx[1].weight), L.REL_RANGE)],
                        L.F_GN1 | L.F_RELU1 | L.F_GEMM2 | L.F_GN2 | L.F_RELU2, rowptr=ps.rowptr, gn1=_gn(self.norm),
                        wp2=ops.packed(m0.linear.weight), gn2=_gn(m0.norm), eps=self.norm.eps)
        return ops.agg_mlp(T, [ops.RelSpec(y, ops.packed(m1.linear.weight))], L.F_GN1 | L.F_RES | L.F_RELU1,
                           gn1=_gn(m1.norm), res=target_feat, eps=m1.norm.eps)


def _stem_train(a: nn.Sequential, s: nn.Sequential, xa: Tensor, xs: Tensor) -> Tensor:
    """_stem composed of differentiable ops, as MapNet.forward composes it."""
    fa = A.linear_gn(F.relu(a[0](xa)), a[2].linear.weight, gn=a[2].norm)
    fs = A.linear_gn(F.relu(s[0](xs)), s[2].linear.weight, gn=s[2].norm)
    return F.relu(fa + fs)


def _stem_infer(a: nn.Sequential, s: nn.Sequential, xa: Tensor, xs: Tensor) -> Tensor:
    return ops.mapnet_input(xa, xs, a[0].weight, a[0].bias, ops.packed(a[2].linear.weight), _gn(a[2].norm),
                            s[0].weight, s[0].bias, ops.packed(s[2].linear.weight), _gn(s[2].norm), eps=a[2].norm.eps)


class _StemInferFn(torch.autograd.Function):
    """_stem for inputs that need no gradient, with the inference launch as its forward (Decode.train_hip: the K = 2
    Linears of the composed path run on ATen and round differently from lgcn_mapnet_input, which would make the
    training forward differ from the no_grad one in the last bit).  The backward re-runs the composed path and
    differentiates that: the parameters' gradients are those of _stem_train at the same inputs."""

    @staticmethod
    def forward(ctx, a, s, xa, xs, *params):
        ctx.mods = (a, s)
        ctx.save_for_backward(xa, xs)
        return _stem_infer(a, s, xa, xs)

    @staticmethod
    def backward(ctx, g):
        a, s = ctx.mods
        xa, xs = ctx.saved_tensors
        params = [*ops.module_params(a), *ops.module_params(s)]
        need = [p for p in params if p.requires_grad]
        with torch.enable_grad():
            grads = iter(torch.autograd.grad(_stem_train(a, s, xa, xs), need, g.contiguous()))
        return (None, None, None, None, *[next(grads) if p.requires_grad else None for p in params])


def _stem(a: nn.Sequential, s: nn.Sequential, xa: Tensor, xs: Tensor, infer_fwd: bool = False) -> Tensor:
    """ReLU(a(xa) + s(xs)) for two Linear(2,128) -> ReLU -> Linear(128,128,GN) branches: MapNet's stem form
    (lgcn_mapnet_input, one launch); under autograd composed as MapNet.forward composes it, or with infer_fwd (and
    inputs that need no gradient) the same launch with a recomputing backward."""
    xa, xs = xa.contiguous(), xs.contiguous()
    params = (*ops.module_params(a), *ops.module_params(s))
    if ops.wants_grad(xa, xs, *params):
        if infer_fwd and not (xa.requires_grad or xs.requires_grad):
            return _StemInferFn.apply(a, s, xa, xs, *params)
        return _stem_train(a, s, xa, xs)
    return _stem_infer(a, s, xa, xs)


def _stem_branch(n: int) -> nn.Sequential:
    return nn.Sequential(nn.Linear(2, n), nn.ReLU(inplace=True), Linear(n, n, norm="GN", ng=1, act=False))


class Interactor(nn.Module):
    """Exchange between the lane RoIs and the global lane graph (reference lanercnn.py:603-642): the RoI features are
    pooled into the graph's stem features, run through GlobalGraphNet and pooled back into the RoIs."""

    def __init__(self, config):
        super().__init__()
        self.config = config
        n_map = config["n_map"]
        self.input = _stem_branch(n_map)
        self.seg = _stem_branch(n_map)
        self.relu = nn.ReLU(inplace=True)
        self.roi2graph = LanePooling(in_dim=128, out_dim=128)
        self.global_graph_net = GlobalGraphNet(config)
        self.graph2roi = LanePooling(in_dim=128, out_dim=128)

    def graph_input(self, graph: Dict) -> Tensor:
        return _stem(self.input, self.seg, torch.cat(graph["ctrs"], 0), graph["feats"])

    def forward(self, graph: Dict, subgraph: Dict, roi_feat: Tensor) -> Tensor:
        _need_cuda(roi_feat, graph["feats"])
        graph_feat = self.roi2graph(roi_feat, subgraph, self.graph_input(graph), graph)
        graph_feat = self.global_graph_net(graph_feat, graph)
        return self.graph2roi(graph_feat, graph, roi_feat, subgraph)


class Net(nn.Module):
    """The fork model (reference lanercnn.py:85-119): LaneInput -> LaneRoI -> Interactor -> LaneRoI -> Decode on a batch
    as collate_fn delivers it (per-scene lists, on the CPU or the GPU; data["subgraphs"] may be a data_lrcnn.RoiBatch, the
    flat route, and forward_raw starts from raw tracks).  Under no_grad every stage runs its inference
    launches (with the modules' own range guard); under autograd their Functions, honouring Decode.train_hip and the
    other *.train_hip switches."""

    def __init__(self, config):
        super().__init__()
        self.config = config
        self.input = LaneInput(config)
        self.roi_net1 = LaneRoI(config, input_dim=config["n_map"])
        self.interactor = Interactor(config)
        self.roi_net2 = LaneRoI(config, input_dim=config["n_map"])
        self.decode = Decode(config)

    def forward(self, data: Dict) -> Dict[str, Tensor]:
        return self._modules_forward(graph_gather(data["graph"]), subgraph_gather(data["subgraphs"]), data)

    def forward_raw(self, raws, tables, lane_ids=None, horizon_buffer=20.):
        """Raw scenes (data_raw's raw-scene dicts and {city: LaneTable}) to the fork's predictions without a scene dict,
        a per-RoI view or a host collate -> (out, data).  data_raw.build_store(..., lanes=True) with this net's config,
        the lane RoIs of all its scenes as one data_lrcnn.RoiBatch (store_roi_inputs + lane_roi_flat), the main graph from
        engine.flat_graph of the store's batch plus the fork's num_nodes / counts / pose, then the modules of forward() in
        its order -- under no_grad their inference launches, under autograd their Functions, as in forward().
        `out`: forward()'s dict, equal to forward(collate_fn(generate_lane_roi_batch(build_scenes(...), device=True))).
        `data`: what Decode read and Loss reads -- ctrs, feats, obs_trajs, gt_preds, has_preds per scene as views of the
        store's arrays, valid_agent_ids (int16, S views of one upload) -- and "subgraphs", the RoiBatch.  Errors: build_store's, the RoI
        stage's, and LgcnError naming the scene when every agent of a scene drops."""
        from . import data_lrcnn, data_raw
        store = data_raw.build_store(raws, tables, self.config, lane_ids=lane_ids, lanes=True)
        rb = data_lrcnn.lane_roi_flat(*data_lrcnn.store_roi_inputs(store), horizon_buffer)
        graph, fb = self._store_graph(store, np.arange(len(store)))
        a, n_act = store._job.t, np.diff(store.actor_off).tolist()
        ids = torch.from_numpy((rb.agents - rb.agent_off[rb.scene_of]).astype(np.int16)).to(fb.node_ctrs.device)
        data = {"ctrs": list(a["actor_ctrs"].split(n_act)), "feats": list(a["actor_feats"].split(n_act)),
                "obs_trajs": list(store.lane_arrays["obs"].split(n_act)),
                "valid_agent_ids": list(ids.split(rb.rois_per_scene.tolist())), "subgraphs": rb}
        if store.has_gt:
            data["gt_preds"] = list(a["gt_preds"].split(n_act))
            data["has_preds"] = list(a["has_preds"].view(torch.bool).split(n_act))
        return self._modules_forward(graph, subgraph_gather(rb), data), data

    @staticmethod
    def _store_graph(store, indices):
        """The main graph of a pick of a DeviceSceneStore as the modules read it: engine.flat_graph of store.batch(indices)
        plus the fork's num_nodes / counts / pose -> (graph, the FlatBatch)."""
        from .engine import flat_graph
        fb, _ = store.batch(indices)
        graph = flat_graph(fb)
        sizes = [int(n) for n in fb.node_sizes]
        graph["num_nodes"] = sizes
        graph["counts"] = [int(v) for v in np.cumsum([0] + sizes[:-1])]
        graph["pose"] = list(torch.cat([fb.node_ctrs, fb.node_feats], -1).split(sizes))
        return graph, fb

    def forward_store(self, store, rois, indices):
        """The fork's predictions for a pick of scenes from two RESIDENT stores -> (out, data): `store`, a
        flatfile.DeviceSceneStore (the main graph: store.batch(indices), one launch), and `rois`, the data_lrcnn.RoiStore
        of the same scenes (the lane RoIs: rois.batch(indices), one launch) -- no lane search, no device -> host read
        before the modules.  Repeats and any order are allowed; every picked scene must hold an RoI (rois.usable()).
        `out`: what forward_raw gives for the picked scenes alone.  `data`: ctrs, feats, obs_trajs and, with gt,
        gt_preds / has_preds as per-scene views of the gathered per-RoI rows (the kept agents only, so valid_agent_ids
        is an int16 arange per scene), agent_ids (the original scene-local ids) and "subgraphs", the RoiBatch; Loss works
        on the pair.  Follows the autograd context as forward() does."""
        if len(store) != len(rois):
            raise L.LgcnError("forward_store: the scene store holds %d scenes, the RoI store %d" % (len(store), len(rois)))
        plan = rois.plan(indices)                 # first: it names a picked scene without an RoI before anything is launched
        graph, fb = self._store_graph(store, indices)
        rb, rows = rois.batch(indices, plan=plan)
        per = rb.rois_per_scene.tolist()
        ids = np.arange(rb.n_rois, dtype=np.int64) - np.repeat(rb.first_roi[:-1], rb.rois_per_scene)
        ids = torch.from_numpy(ids.astype(np.int16)).to(fb.node_ctrs.device)
        data = {k: list(rows[k].split(per)) for k in ("ctrs", "feats", "obs_trajs", "gt_preds", "has_preds") if k in rows}
        data.update(valid_agent_ids=list(ids.split(per)), agent_ids=rows["agent_ids"], subgraphs=rb)
        return self._modules_forward(graph, subgraph_gather(rb), data), data

    def _modules_forward(self, graph: Dict, graph_roi: Dict, data: Dict) -> Dict[str, Tensor]:
        roi_feat = self.input(graph_roi)
        roi_feat = self.roi_net1(roi_feat, graph_roi)
        roi_feat = self.interactor(graph, graph_roi, roi_feat)
        roi_feat = self.roi_net2(roi_feat, graph_roi)
        pred_logics, pred_goals, pred_trajs = self.decode(roi_feat, graph_roi, data)
        return {"pred_logics": pred_logics, "pred_goals": pred_goals, "pred_trajs": pred_trajs}


# ------------------------------------------------------------------ goal decoding (reference lanercnn.py:683-924)
def nms_select(xys: Tensor, logits: Tensor, threshold: float = 2.0, min_len: int = 6) -> Tensor:
    """The full list of the reference's nms_select (:687-708) for one RoI: greedy survivors in descending logit order,
    padded with the best dropped nodes up to min_len.  One launch (lgcn_nms_select); the length is read from the
    device (this function returns a list of data-dependent length; Decode does not use it)."""
    _need_cuda(xys, logits)
    n = logits.shape[0]
    idx, count = ops.nms_select_segments(xys.detach().float(), logits.detach().float(), [0, n], threshold, min_len, 0)
    return idx[:int(count.item())].long()


def compute_coefficent(agt_ctrs: Tensor, agt_dirs: Tensor, pred_ctrs: Tensor, pred_dirs: Tensor):
    """Coefficients of the quadratic x(s) = a0 s^2 + a1 s + a2, y(s) = b0 s^2 + b1 s + b2 from the agent's centre and
    unit direction to each goal with its unit direction (:710-723).  pred_*: [A, k, 2]; returns six [A, k, 1]."""
    c, d = agt_ctrs.view(-1, 1, 2), agt_dirs.view(-1, 1, 2)
    out = []
    for ax in (0, 1):
        g, p = pred_ctrs[:, :, ax], pred_dirs[:, :, ax]
        c_, d_ = c[:, :, ax], d[:, :, ax]
        q1 = (2 * g * d_ + 2 * c_ * d_) / (2 + d_ - p)
        q0 = g - c_ - q1
        q2 = c_.expand_as(g)
        out += [q0.unsqueeze(2), q1.unsqueeze(2), q2.unsqueeze(2)]
    return tuple(out)


def sample_trajectory(s_samples: Tensor, a0, a1, a2, b0, b1, b2) -> Tensor:
    """Points of the quadratic at s_samples: [..., S] -> [..., S, 2] (:728-732)."""
    x = a0 * s_samples ** 2 + a1 * s_samples + a2
    y = b0 * s_samples ** 2 + b1 * s_samples + b2
    return torch.stack([x, y], -1)


def sample_d1_trajectory(s_samples: Tensor, a0, a1, a2, b0, b1, b2) -> Tensor:
    """First derivative of the quadratic at s_samples (:734-737)."""
    return torch.stack([2 * a0 * s_samples + a1, 2 * b0 * s_samples + b1], -1)


class Decode(nn.Module):
    """Goal decoder (reference lanercnn.py:740-924).  Inference: goal head (row block + Linear(128, 5)), one
    lgcn_goal_decode launch for NMS, goals, coefficients and arc-length samples of all interest agents, the agent's
    observed motion (stem form) pooled into its RoI, the refinement head on the k gathered rows and one
    lgcn_goal_refine launch -- no device -> host read besides the pair count inside LanePooling.  Under autograd the
    indices still come from lgcn_nms_select (the reference does not propagate through the selection either) and
    everything else runs on differentiable ops; with Decode.train_hip set the decode and refine stages stay on the
    inference launches and their backward is lgcn_goal_refine_bwd + lgcn_goal_decode_bwd.

    The reference hands the motion graph's centres to LanePooling as [1, 20, 2] tensors, whose len() is 1, so its
    context row offset grows by 1 per scene, not by 20: scene b pools rows b .. b + 19 of the concatenated [A * 20]
    motion features and poses (distances still come from scene b's own trajectory).  That numbering is reproduced
    here: the stem and pose rows are gathered in that order before LanePooling sees [20, 2] centres."""
    # Train the decode and refine stages on the inference launches (autograd.GoalDecodeFn / GoalRefineFn): the training
    # forward is lgcn_goal_decode + lgcn_goal_refine, their backward lgcn_goal_refine_bwd + lgcn_goal_decode_bwd, instead
    # of the stock ops of _decode_torch and of the tail of decode(); the motion stem keeps the inference launch as its
    # forward too (_StemInferFn), so the whole training forward is the no_grad forward bit for bit.  Opt-in, like
    # Att.train_hip; read on each forward.
    train_hip = False

    def __init__(self, config):
        super().__init__()
        self.config = config
        n_actor = config["n_actor"]
        self.pred = nn.Sequential(Linear(n_actor, n_actor, norm="GN", ng=1), nn.Linear(n_actor, 5))
        self.agt_layer1 = _stem_branch(n_actor)
        self.agt_layer2 = _stem_branch(n_actor)
        self.relu = nn.ReLU(inplace=True)
        self.lane_pool = LanePooling(n_actor, n_actor)
        self.refinement = nn.Sequential(Linear(n_actor, n_actor, norm="GN", ng=1), nn.Linear(n_actor, 30 * 2))

    @staticmethod
    def _interest(subgraph: Dict) -> Tuple[List[int], List[Tuple[int, int]]]:
        ids = subgraph["interest_roi"]
        ids = [int(i) for i in (ids.tolist() if torch.is_tensor(ids) or isinstance(ids, np.ndarray) else ids)]
        spans = [(int(subgraph["roi_spans"][i][0]), int(subgraph["roi_spans"][i][1])) for i in ids]
        return ids, spans

    def forward(self, roi_feat: Tensor, subgraph: Dict, data: Dict):
        out = self.decode(roi_feat, subgraph, data)
        return out["logits"], out["goals"], out["pred_trajs"]

    def decode(self, roi_feat: Tensor, subgraph: Dict, data: Dict) -> Dict[str, Tensor]:
        """forward() with its intermediates: pred [n, 5], top_idx [A, k] (RoI-local), goals, logits, s_samples
        (un-normalised), pooled [n, 128], traj_delta [A, k, 30, 2] and pred_trajs."""
        _need_cuda(roi_feat)
        k, dev = self.config["num_mods"], roi_feat.device
        if self.config["num_preds"] != ops.GOAL_STEPS:
            raise L.LgcnError("Decode: num_preds must be %d" % ops.GOAL_STEPS)
        ids, spans = self._interest(subgraph)                       # host integers
        n_agt = len(ids)
        pred_spans = [0]
        for lo, hi in spans:
            pred_spans.append(pred_spans[-1] + hi - lo)
        feats = torch.cat([roi_feat[lo:hi] for lo, hi in spans], 0)
        pred = self.pred(feats)                                       # [n, 5]
        anchor_ctrs = torch.cat(subgraph["ctrs"], 0)
        anchor_dirs = torch.cat(subgraph["dirs"], 0)
        # the first valid agent of every scene: centre, observed steps and their directions (:835-841)
        first = lambda key: torch.cat([x.to(dev).index_select(0, v.to(dev).long()[:1]) for v, x in
                                       zip(data["valid_agent_ids"], data[key])], 0)
        agt_ctrs = first("ctrs").view(-1, 2).float()
        agt_dirs = first("feats").view(-1, 20, 3)[:, :, :2]
        agt_trajs = first("obs_trajs").view(-1, 20, 3)[:, :, :2]
        vel = subgraph["agent_vel"]
        agt_vels = torch.tensor([float(vel[i]) for i in ids], dtype=torch.float32).to(dev, non_blocking=True)
        dir_last = agt_dirs[:, -1, :].float()
        train = ops.wants_grad(roi_feat, *ops.module_params(self))

        fused = train and Decode.train_hip
        if fused:
            top, goals, logits, coef, s_samples = A.GoalDecodeFn.apply(pred, pred_spans, anchor_ctrs, anchor_dirs,
                                                                       [lo for lo, _ in spans], agt_ctrs, dir_last, agt_vels,
                                                                       k, 2.0)
        elif train:
            top, goals, logits, coefs, s_samples = self._decode_torch(pred, pred_spans, anchor_ctrs, anchor_dirs, spans,
                                                                      agt_ctrs, dir_last, agt_vels, k)
        else:
            top, goals, logits, coef, s_samples = ops.goal_decode(pred, pred_spans, anchor_ctrs, anchor_dirs,
                                                                  [lo for lo, _ in spans], agt_ctrs, dir_last, agt_vels, k)

        # the agent's observed motion, pooled into its RoI (:873-887); row order: see the class docstring
        rows = (torch.arange(n_agt, device=dev).view(-1, 1) + torch.arange(20, device=dev).view(1, -1)).reshape(-1)
        trajs_q = agt_trajs.reshape(-1, 2).float().index_select(0, rows)
        dirs_q = agt_dirs.reshape(-1, 2).float().index_select(0, rows)
        agt_feat = _stem(self.agt_layer1, self.agt_layer2, trajs_q, dirs_q, infer_fwd=Decode.train_hip)
        pose_q = torch.cat([trajs_q, dirs_q], -1)
        motion = {"ctrs": [agt_trajs[i].float() for i in range(n_agt)], "pose": list(pose_q.split(20, 0))}
        roi_map = {"ctrs": [anchor_ctrs[lo:hi] for lo, hi in spans],
                   "pose": [torch.cat([anchor_ctrs[lo:hi], anchor_dirs[lo:hi]], -1) for lo, hi in spans]}
        pooled = self.lane_pool(agt_feat, motion, feats, roi_map)

        base = torch.tensor(pred_spans[:-1], dtype=torch.int32).to(dev, non_blocking=True)
        flat = (top + base.view(-1, 1)).reshape(-1)                   # rows of `pooled`, [A * k]
        if train:
            traj_feats = pooled.index_select(0, flat.long())
        else:
            n_rows = torch.tensor([n_agt * k], dtype=torch.int32).to(dev, non_blocking=True)
            traj_feats = ops.gather_rows(pooled, flat.contiguous(), n_rows, n_agt * k)
        traj_delta = self.refinement(traj_feats).view(n_agt, k, ops.GOAL_STEPS, 2)

        if fused:
            pred_trajs = A.GoalRefineFn.apply(s_samples, coef, traj_delta)
        elif train:
            s = s_samples + traj_delta[..., 0]
            s = s / s.max(2, keepdim=True)[0]
            s = torch.where(s == 0.0, torch.ones_like(s), s)
            tangent = sample_d1_trajectory(s, *coefs)
            normal = torch.stack([-tangent[..., 1], tangent[..., 0]], -1)
            pred_trajs = sample_trajectory(s, *coefs) + normal * traj_delta[..., 1:2]
        else:
            pred_trajs = ops.goal_refine(s_samples, coef, traj_delta)
        return {"pred": pred, "top_idx": top, "goals": goals, "logits": logits, "s_samples": s_samples, "pooled": pooled,
                "traj_delta": traj_delta, "pred_trajs": pred_trajs}

    def _decode_torch(self, pred, pred_spans, anchor_ctrs, anchor_dirs, spans, agt_ctrs, dir_last, agt_vels, k):
        """The differentiable restatement of :802-865 on stock ops; the indices come from lgcn_nms_select."""
        dev = pred.device
        n_agt = len(spans)
        for a in range(n_agt):
            if pred_spans[a + 1] - pred_spans[a] < k:
                raise L.LgcnError("Decode: interest RoI %d has fewer than %d nodes" % (a, k))
        anc_rows = torch.cat([torch.arange(lo, hi) for lo, hi in spans]).to(dev, non_blocking=True)
        anc_c, anc_d = anchor_ctrs.index_select(0, anc_rows), anchor_dirs.index_select(0, anc_rows)
        xy = anc_c + pred[:, 1:3]
        theta = torch.atan2(anc_d[:, 1], anc_d[:, 0]) + torch.atan(pred[:, 3] / pred[:, 4])
        idx, _ = ops.nms_select_segments(xy.detach(), pred[:, 0].detach(), pred_spans, 2.0, k, k)
        off = torch.tensor(pred_spans[:-1]).to(dev, non_blocking=True)
        sel = off.view(-1, 1) + torch.arange(k, device=dev).view(1, -1)          # list positions [A, k]
        top = idx.index_select(0, sel.reshape(-1)).view(n_agt, k)
        flat = (top.long() + off.view(-1, 1)).reshape(-1)
        goals = xy.index_select(0, flat).view(n_agt, k, 2)
        thetas = theta.index_select(0, flat).view(n_agt, k)
        logits = pred[:, 0].index_select(0, flat).view(n_agt, k)
        pdirs = torch.stack([torch.cos(thetas), torch.sin(thetas)], -1)
        nrm = torch.linalg.norm(dir_last, dim=1)
        adir = torch.where((nrm < 1e-6).view(-1, 1), torch.zeros_like(dir_last), dir_last / nrm.view(-1, 1))
        coefs = compute_coefficent(agt_ctrs, adir, goals, pdirs)
        s31 = (1.0 / 30) * torch.arange(0, 31, device=dev).float()
        pts = sample_trajectory(s31, *coefs)
        length = torch.sqrt(((pts[:, :, 1:] - pts[:, :, :-1]) ** 2).sum(-1)).sum(-1)
        acc = 2 * (length - agt_vels.view(-1, 1) * 3.0) / 9.0
        t31 = 0.1 * torch.arange(0, 31, device=dev).float()
        v = (agt_vels.view(-1, 1, 1) + acc.unsqueeze(2) * t31).clamp_min(0.0)
        s_samples = (v[:, :, :1] + v[:, :, 1:]) * t31[1:] / 2
        return top, goals, logits, coefs, s_samples


# ------------------------------------------------------------------ loss and metrics (reference lanercnn.py:1205-1463)
class RoiLoss(nn.Module):
    """Goal / trajectory loss of the fork model (reference lanercnn.py:1205-1301): per scene the first valid agent's
    future is compared with the mode whose goal is closest to its last observed step.  The first valid agents are
    picked on the device, the three sums and their gradients are one launch each (autograd.RoiLossFn), and the only
    device -> host read is the one of the two counts the reference reads with .item() (:1284, :1294)."""

    def __init__(self, config):
        super().__init__()
        self.config = config
        self.num_mods = config["num_mods"]
        self.bce_loss = nn.BCELoss()
        self.reg_loss = nn.SmoothL1Loss(reduction="sum")

    def forward(self, data: Dict, out: Dict, gt_preds: List[Tensor], has_preds: List[Tensor]) -> Dict:
        pred_logics, pred_goals, pred_trajs = out["pred_logics"], out["pred_goals"], out["pred_trajs"]
        valid_agent_ids = to_long(gpu(data["valid_agent_ids"]))
        _need_cuda(pred_logics, pred_goals, pred_trajs, *gt_preds, *has_preds)
        num_preds = pred_trajs.shape[2]
        first = lambda xs, tail: torch.cat([x.index_select(0, ids.long()[:1]).view(-1, *tail)
                                            for ids, x in zip(valid_agent_ids, xs)], 0)
        gt = first(gt_preds, (num_preds, 2)).float().contiguous()             # [bs, 30, 2]
        has = first(has_preds, (num_preds,)).bool().contiguous()              # [bs, 30]
        cls_loss, goal_loss, traj_loss, counts, best_goals = A.RoiLossFn.apply(
            pred_logics.float(), pred_goals.float(), pred_trajs.float(), gt, has, float(self.config["reg_coef"]))
        _, n_goal, n_traj = counts.tolist()
        return {"cls_loss": cls_loss, "num_cls": len(pred_logics), "pred_goals": best_goals,
                "reg_goal_loss": goal_loss, "num_reg_goal": n_goal, "pred_trajs": pred_trajs,
                "reg_traj_loss": traj_loss, "num_reg_traj": n_traj, "stage_one_loss": 0, "num_stage_one": 1}


class Loss(nn.Module):
    """loss = cls / num_cls + reg_goal / num_reg_goal + reg_traj / num_reg_traj (reference lanercnn.py:1305-1325)."""

    def __init__(self, config):
        super().__init__()
        self.config = config
        self.pred_loss = RoiLoss(config)

    def forward(self, out: Dict, data: Dict) -> Dict:
        loss_out = self.pred_loss(data, out, gpu(data["gt_preds"]), gpu(data["has_preds"]))
        loss_out["loss"] = (loss_out["cls_loss"] / (loss_out["num_cls"] + 1e-10)
                            + loss_out["reg_goal_loss"] / (loss_out["num_reg_goal"] + 1e-10)
                            + loss_out["reg_traj_loss"] / (loss_out["num_reg_traj"] + 1e-10)
                            + loss_out["stage_one_loss"] / (loss_out["num_stage_one"] + 1e-10))
        return loss_out


def pred_metrics_ade(goals, gt_preds, has_preds):
    """Mean distance of the chosen goals to the last ground-truth step (reference lanercnn.py:1426-1444)."""
    assert has_preds.all()
    goals = np.asarray(goals, np.float32).reshape(-1, 2)
    gt_preds = np.asarray(gt_preds, np.float32)
    return np.sqrt(((goals - gt_preds[:, -1]) ** 2).sum(-1)).mean()


def pred_metrics(preds, gt_preds, has_preds):
    """ade1, fde1, ade, fde, min_idcs (reference lanercnn.py:1446-1463)."""
    assert has_preds.all()
    preds, gt_preds = np.asarray(preds, np.float32), np.asarray(gt_preds, np.float32)
    err = np.sqrt(((preds - np.expand_dims(gt_preds, 1)) ** 2).sum(3))
    ade1, fde1 = err[:, 0].mean(), err[:, 0, -1].mean()
    min_idcs = err[:, :, -1].argmin(1)
    best = err[np.arange(len(min_idcs)).astype(np.int64), min_idcs]
    return ade1, fde1, best.mean(), best[:, -1].mean(), min_idcs


class PostProcess(nn.Module):
    """Collects the chosen goals, all trajectories and the first agent's ground truth per scene, and prints the
    running losses with ADE / FDE (reference lanercnn.py:1328-1423)."""

    def __init__(self, config):
        super().__init__()
        self.config = config

    def forward(self, out, data, loss_out):
        return {"goals": [loss_out["pred_goals"].detach().cpu().numpy()],
                "trajs": [loss_out["pred_trajs"].detach().cpu().numpy()],
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
            if key in ("loss", "pred_goals", "pred_trajs"):
                continue
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
        reg_goal = metrics["reg_goal_loss"] / (metrics["num_reg_goal"] + 1e-10)
        reg_traj = metrics["reg_traj_loss"] / (metrics["num_reg_traj"] + 1e-10)
        stg1_cls = metrics["stage_one_loss"] / (metrics["num_stage_one"] + 1e-10)
        loss = cls + reg_goal + reg_traj + stg1_cls
        ade1, fde1, ade, fde, _ = pred_metrics(np.concatenate(metrics["trajs"], 0), np.concatenate(metrics["gt_preds"], 0),
                                               np.concatenate(metrics["has_preds"], 0))
        print("loss %2.4f - %2.4f %2.4f %2.4f, %2.4f - ade1=%2.4f fde1=%2.4f ade=%2.4f fde=%2.4f"
              % (loss, cls, reg_goal, reg_traj, stg1_cls, ade1, fde1, ade, fde))
        print()


def _plugin_parts():
    from .data import SyntheticLaneRoIDataset
    # Dataset: the reference returns its ArgoDataset (needs argoverse-api and the dataset, both absent here); a caller that
    # has them injects the class as config["dataset_cls"], as for lanegcn.get_model
    dataset = config.get("dataset_cls") or SyntheticLaneRoIDataset
    return dataset, Net(config).cuda(), Loss(config).cuda(), PostProcess(config).cuda()


def get_model():
    """The reference's plugin entry point (lanercnn.py:1466-1477): (config, Dataset, collate_fn, net, loss, post_process,
    opt)."""
    dataset, net, loss, post_process = _plugin_parts()
    return config, dataset, collate_fn, net, loss, post_process, Optimizer(net.parameters(), config)


def get_model_for_torch_dist():
    """get_model without the optimizer (lanercnn.py:1479-1490): the caller builds it after wrapping the net."""
    dataset, net, loss, post_process = _plugin_parts()
    return config, dataset, collate_fn, net, loss, post_process
