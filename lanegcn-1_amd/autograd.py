"""Differentiable versions of the hot-path row blocks (training path).

Forward = the fused HIP kernels of ops.py (saving the pre-normalisation tensors); backward = the same
kernels on transposed plans / transposed weights plus three backward kernels:
  row-GEMMs of the backward  -> lgcn_agg_mlp  (dx = dy W is a Linear with weight W^T; the transpose of a
                                 gather-by-destination is a gather-by-source on the transposed plan)
  GroupNorm / ReLU backward  -> lgcn_gn_bwd   (deterministic dgamma / dbeta)
  weight gradients           -> lgcn_wgrad    (dW_r = dT^T (G_r src_r), fp32-input MFMA)
Every Function also has a fused exact-fp32 backward, opt-in: RowBlockFn with RowBlockFn.train_hip (one or two IDENT
relations: lgcn_rowblock_bwd does the whole backward in one launch pair; blocks with a RANGE or CSR relation keep the
composition above) and LaneConvFn with BlockSpec.fused_bwd (lgcn_laneconv_bwd).
Att's pair stage has a fused pair of its own (Att.train_hip): AttPairsFn on lgcn_att_pairs_train / lgcn_att_pairs_bwd,
and so has the pair stage of the fork's LanePooling (LanePooling.train_hip): PoolPairsFn on lgcn_pool_pairs_train /
lgcn_pool_pairs_bwd.
PredNet's tail (the heads' nn.Linear(128, 2 T), AttDest's first layer, the score Linear, the sort and the gather) has
its own pair: PredRegFn / PredFinalFn on lgcn_pred_reg / lgcn_pred_final_train and their backward entries.
Only the K = 2 / K = 4 input Linears (nn.Linear(2,128) of the stems, the 4 meta columns) stay on stock
ATen ops in the training path: they are [N,2]-shaped, not 128-d contractions.
"""
from dataclasses import dataclass
from typing import List, Optional

import torch
from torch.autograd import Function

from . import _lib as L
from . import ops

C_FEAT = ops.C_FEAT


@dataclass
class Rel:
    """One relation of a row block: which source tensor / weight (indices into the Function's tensor
    arguments), how it is gathered and (for weight slices) the first input column of the 128-wide block."""
    src: int                    # index into `srcs`
    w: int                      # index into `weights`
    mode: int = L.REL_IDENT
    ridx: int = 0
    col0: int = 0


@dataclass
class BlockSpec:
    n_rows: int
    rels: List[Rel]
    gn: bool = False
    relu: bool = False
    has_res: bool = False
    eps: float = ops.EPS
    plan: Optional[ops.LanePlan] = None        # CSR relations: plan by destination ...
    plan_t: Optional[ops.LanePlan] = None      # ... and by source (for d src)
    rowptr: Optional[torch.Tensor] = None      # RANGE relation: segments [n_rows+1]
    seg_ids: Optional[torch.Tensor] = None     # RANGE relation: segment id of every source row (int32)
    n_seg_rows: Optional[torch.Tensor] = None  # device count of valid source rows (int32 [1])
    tag: Optional[str] = None
    fused_bwd: bool = False                    # backward on lgcn_laneconv_bwd (LaneConvFn) / lgcn_rowblock_bwd (RowBlockFn), exact
                                               # fp32, instead of the composed one


def _fwd_rels(spec: BlockSpec, srcs, weights):
    return [ops.RelSpec(srcs[r.src], ops.packed(weights[r.w], r.col0, C_FEAT), r.mode, r.ridx) for r in spec.rels]


def _csr_kw(spec: BlockSpec, plan):
    if plan is not None:
        return dict(rowptr=plan.rowptr, col=plan.col, n_rel_csr=plan.n_rel)
    if spec.rowptr is not None:
        return dict(rowptr=spec.rowptr)
    return {}


def _stage_backward(spec: BlockSpec, srcs, weights, dT, need_src, need_w, res_grad=None):
    """Gradients of T = sum_r (G_r src_r) W_r^T given dT.  Returns (d_srcs list, d_weights list)."""
    d_srcs: List[Optional[torch.Tensor]] = [None] * len(srcs)
    d_ws: List[Optional[torch.Tensor]] = [None] * len(weights)
    # ---- d src: one launch per source for the IDENT / CSR relations, gather for RANGE
    for si in range(len(srcs)):
        if not need_src[si]:
            continue
        same = [r for r in spec.rels if r.src == si]
        lin = [r for r in same if r.mode != L.REL_RANGE]
        acc = None
        if lin:
            rels = []
            for r in lin:
                wp = ops.packed_t(weights[r.w], r.col0)
                rels.append(ops.RelSpec(dT, wp, L.REL_CSR if r.mode == L.REL_CSR else L.REL_IDENT, r.ridx))
            flags = L.F_RES if (res_grad is not None and si == 0) else 0
            acc = ops.agg_mlp(srcs[si].shape[0], rels, flags, res=res_grad if flags else None,
                              **_csr_kw(spec, spec.plan_t if any(r.mode == L.REL_CSR for r in lin) else None))
        for r in same:
            if r.mode == L.REL_RANGE:   # d src[p] = (dT W_r)[seg(p)]
                tmp = ops.agg_mlp(dT.shape[0], [ops.RelSpec(dT, ops.packed_t(weights[r.w], r.col0))], 0)
                rows = srcs[si].shape[0]
                g = ops.gather_rows(tmp, spec.seg_ids, spec.n_seg_rows, rows)
                acc = g if acc is None else acc + g
        d_srcs[si] = acc
    # ---- d W
    if any(need_w):
        rels = [ops.RelSpec(srcs[r.src], None, r.mode, r.ridx) for r in spec.rels]
        dW = ops.wgrad(spec.n_rows, rels, dT, **_csr_kw(spec, spec.plan))
        for i, r in enumerate(spec.rels):
            if not need_w[r.w]:
                continue
            w = weights[r.w]
            if w.shape[1] == C_FEAT:
                d_ws[r.w] = dW[i] if d_ws[r.w] is None else d_ws[r.w] + dW[i]
            else:                           # a 128-column block of a wider weight (ctx.0 [128,384], meta [128,132])
                if d_ws[r.w] is None:
                    d_ws[r.w] = torch.zeros_like(w)
                d_ws[r.w][:, r.col0:r.col0 + C_FEAT] += dW[i]
    return d_srcs, d_ws


class RowBlockFn(Function):
    """out = [ReLU]( [GN]( sum_r (G_r src_r) W_r^T ) [+ res] )  -- layers.Linear, Att.query / agt+ctx.1 tail,
    the pure Linear stages (gn = relu = False).  Backward is composed, or with spec.fused_bwd, for the blocks that
    _fused_ok() accepts, the fused lgcn_rowblock_bwd."""
    # Default of BlockSpec.fused_bwd for the blocks built by row_block(): one switch for every module behind it
    # (layers.Linear, the input stems, A2M.meta, AttDest, the node side of Att, lanercnn.py).  Opt-in, like Att.train_hip.
    train_hip = False

    @staticmethod
    def forward(ctx, spec: BlockSpec, n_src: int, n_w: int, *tensors):
        srcs, weights = list(tensors[:n_src]), list(tensors[n_src:n_src + n_w])
        gn_w, gn_b, res = tensors[n_src + n_w:n_src + n_w + 3]
        flags = (L.F_GN1 if spec.gn else 0) | (L.F_RELU1 if spec.relu else 0) | (L.F_RES if spec.has_res else 0)
        need_pre = spec.gn or spec.relu
        pre = torch.empty((spec.n_rows, C_FEAT), dtype=torch.float32, device=srcs[0].device) if need_pre else None
        out = ops.agg_mlp(spec.n_rows, _fwd_rels(spec, srcs, weights), flags,
                          gn1=(gn_w, gn_b) if spec.gn else None, res=res if spec.has_res else None, out_pre=pre,
                          eps=spec.eps, tag=spec.tag, **_csr_kw(spec, spec.plan))
        ctx.spec, ctx.n_src, ctx.n_w = spec, n_src, n_w
        ctx.save_for_backward(*srcs, *weights, *(t for t in (gn_w, pre, out) if t is not None))
        ctx.has = (gn_w is not None, pre is not None)
        return out

    @staticmethod
    def backward(ctx, d_out):
        spec, n_src, n_w = ctx.spec, ctx.n_src, ctx.n_w
        saved = list(ctx.saved_tensors)
        srcs, weights = saved[:n_src], saved[n_src:n_src + n_w]
        rest = saved[n_src + n_w:]
        gn_w = rest.pop(0) if ctx.has[0] else None
        pre = rest.pop(0) if ctx.has[1] else None
        out = rest.pop(0)
        d_out = d_out.contiguous()
        ni = ctx.needs_input_grad          # (spec, n_src, n_w, *tensors)
        need_src = [ni[3 + i] for i in range(n_src)]
        need_w = [ni[3 + n_src + i] for i in range(n_w)]
        if spec.fused_bwd and RowBlockFn._fused_ok(spec, d_out, weights):
            return RowBlockFn._backward_fused(spec, ni, d_out, srcs, weights, gn_w, pre, out)
        d_gw = d_gb = d_res = None
        if spec.gn or spec.relu:
            dT, g, d_gw, d_gb = ops.gn_bwd(d_out, pre, out if spec.relu else None, gn_w if spec.gn else None,
                                           eps=spec.eps, want_g=spec.has_res)
            d_res = g if spec.has_res else None
        else:
            dT = d_out
            d_res = d_out if spec.has_res else None
        with ops.backward_mma():
            d_srcs, d_ws = _stage_backward(spec, srcs, weights, dT, need_src, need_w)
        return (None, None, None, *d_srcs, *d_ws, d_gw, d_gb, d_res)

    @staticmethod
    def _fused_ok(spec, d_out, weights):
        """What lgcn_rowblock_bwd covers: CUDA fp32 rows, one or two IDENT relations on distinct sources and distinct
        128-column blocks ([128, K] weights, K and col0 multiples of 4: the block's gradient is written in place)."""
        rels = spec.rels
        if not (d_out.is_cuda and d_out.dtype == torch.float32 and spec.n_rows > 0 and 1 <= len(rels) <= 2):
            return False
        if any(r.mode != L.REL_IDENT for r in rels) or len({r.src for r in rels}) != len(rels):
            return False
        if len(rels) == 2 and rels[0].w == rels[1].w and abs(rels[0].col0 - rels[1].col0) < C_FEAT:
            return False                      # the same (or an overlapping) block twice: its gradient is a sum
        if len(rels) == 2 and rels[0].w != rels[1].w and weights[rels[0].w].data_ptr() == weights[rels[1].w].data_ptr():
            return False                      # one parameter passed as two weight arguments: autograd adds their gradients
        for r in rels:
            w = weights[r.w]
            if w.dim() != 2 or w.shape[0] != C_FEAT or r.col0 < 0 or r.col0 + C_FEAT > w.shape[1] or w.shape[1] % 4 or r.col0 % 4:
                return False
        return True

    @staticmethod
    def _backward_fused(spec, ni, d_out, srcs, weights, gn_w, pre, out):
        """BlockSpec.fused_bwd: the whole backward in one launch pair (lgcn_rowblock_bwd); inputs that need no gradient
        cost nothing."""
        n_src, n_w = len(srcs), len(weights)
        i_gn = 3 + n_src + n_w
        need_w = [ni[3 + n_src + i] for i in range(n_w)]
        want_res = spec.has_res and spec.relu and ni[i_gn + 2]
        g = ops.rowblock_bwd(d_out, out if spec.relu else None, pre if spec.gn else None, gn_w if spec.gn else None,
                             [(srcs[r.src], weights[r.w], r.col0) for r in spec.rels],
                             want_src=[ni[3 + r.src] for r in spec.rels], want_w=[need_w[r.w] for r in spec.rels],
                             want_gn=spec.gn and (ni[i_gn] or ni[i_gn + 1]), want_res=want_res, eps=spec.eps)
        d_srcs: List[Optional[torch.Tensor]] = [None] * n_src
        d_ws: List[Optional[torch.Tensor]] = [None] * n_w
        for i, r in enumerate(spec.rels):
            d_srcs[r.src] = g["d_src"][i]
            d_ws[r.w] = g["d_w"][g["w_index"][i]]
        d_res = g["d_res"] if spec.relu else (d_out if spec.has_res else None)
        return (None, None, None, *d_srcs, *d_ws, g["d_gamma"], g["d_beta"], d_res)


class LaneConvFn(Function):
    """One fused LaneConv layer (lanegcn.py:331-362): X' = ReLU(GN2(ReLU(GN1(sum_r (G_r X) W_r^T)) W2^T) + X).
    Forward is the single fused launch of inference (saving T, Y, Z); backward is composed, or with spec.fused_bwd
    the fused lgcn_laneconv_bwd."""

    @staticmethod
    def forward(ctx, spec: BlockSpec, feat, gn1_w, gn1_b, w2, gn2_w, gn2_b, *weights):
        N = spec.n_rows
        T, Y, Z = (torch.empty((N, C_FEAT), dtype=torch.float32, device=feat.device) for _ in range(3))
        flags = L.F_GN1 | L.F_RELU1 | L.F_GEMM2 | L.F_GN2 | L.F_RES | L.F_RELU2
        out = ops.agg_mlp(N, _fwd_rels(spec, [feat], list(weights)), flags, gn1=(gn1_w, gn1_b), wp2=ops.packed(w2),
                          gn2=(gn2_w, gn2_b), res=feat, out_pre=T, out_mid=Y, out_pre2=Z, eps=spec.eps, tag="laneconv",
                          **_csr_kw(spec, spec.plan))
        ctx.spec = spec
        ctx.save_for_backward(feat, gn1_w, w2, gn2_w, T, Y, Z, out, *weights)
        return out

    @staticmethod
    def backward(ctx, d_out):
        spec = ctx.spec
        feat, gn1_w, w2, gn2_w, T, Y, Z, out, *weights = ctx.saved_tensors
        ni = ctx.needs_input_grad
        N = spec.n_rows
        if (spec.fused_bwd and d_out.is_cuda and d_out.dtype == torch.float32 and N > 0
                and all(tuple(w.shape) == (C_FEAT, C_FEAT) for w in (w2, *weights))):
            return LaneConvFn._backward_fused(spec, ni, d_out, feat, gn1_w, w2, gn2_w, T, Y, Z, out, weights)
        # out = ReLU(GN2(Z) + X)
        dZ, g2, d_g2w, d_g2b = ops.gn_bwd(d_out.contiguous(), Z, out, gn2_w, eps=spec.eps, want_g=True)
        # Z = Y W2^T
        with ops.backward_mma():
            dY = ops.agg_mlp(N, [ops.RelSpec(dZ, ops.packed_t(w2))], 0)
        d_w2 = ops.wgrad(N, [ops.RelSpec(Y, None)], dZ)[0] if ni[4] else None
        # Y = ReLU(GN1(T))
        dT, _, d_g1w, d_g1b = ops.gn_bwd(dY, T, Y, gn1_w, eps=spec.eps)
        # T = sum_r (G_r X) W_r^T ; the residual branch adds g2 to dX inside the same launch
        need_w = [ni[7 + i] for i in range(len(weights))]
        with ops.backward_mma():
            d_srcs, d_ws = _stage_backward(spec, [feat], list(weights), dT, [ni[1]], need_w, res_grad=g2)
        return (None, d_srcs[0], d_g1w, d_g1b, d_w2, d_g2w, d_g2b, *d_ws)

    @staticmethod
    def _backward_fused(spec, ni, d_out, feat, gn1_w, w2, gn2_w, T, Y, Z, out, weights):
        """BlockSpec.fused_bwd: everything below the relation stage in one launch pair (lgcn_laneconv_bwd); with one IDENT
        relation (LinearRes) that is the whole backward, otherwise dX and dW_r stay the two launches of _stage_backward."""
        names = {2: "d_g1", 3: "d_b1", 4: "d_w2", 5: "d_g2", 6: "d_b2"}
        want = [n for i, n in names.items() if ni[i]]
        need_w = [ni[7 + i] for i in range(len(weights))]
        r0 = spec.rels[0]
        if len(spec.rels) == 1 and r0.mode == L.REL_IDENT and r0.col0 == 0:
            g = ops.laneconv_bwd(d_out, out, Z, Y, T, gn1_w, w2, gn2_w, x=feat, w1=weights[0],
                                 want=want + (["d_w1"] if need_w[0] else []), want_dx=ni[1], eps=spec.eps)
            d_x, d_ws = g["dX"], [g.get("d_w1")]
        else:
            g = ops.laneconv_bwd(d_out, out, Z, Y, T, gn1_w, w2, gn2_w, want=want, want_dx=ni[1], eps=spec.eps)
            with ops.backward_mma():
                d_srcs, d_ws = _stage_backward(spec, [feat], list(weights), g["dT"], [ni[1]], need_w, res_grad=g["g2"])
            d_x = d_srcs[0]
        return (None, d_x, g.get("d_g1"), g.get("d_b1"), g.get("d_w2"), g.get("d_g2"), g.get("d_b2"), *d_ws)


class GNActFn(Function):
    """out = [ReLU](GN(x) [+ res]) on rows (stand-alone; the per-pair composition of Att)."""

    @staticmethod
    def forward(ctx, x, gn_w, gn_b, res, relu: bool, eps: float):
        out = ops.gn_fwd(x, (gn_w, gn_b) if gn_w is not None else None, res, relu, eps)
        ctx.relu, ctx.eps, ctx.has_res, ctx.has_gn = relu, eps, res is not None, gn_w is not None
        ctx.save_for_backward(x, out, *([gn_w] if gn_w is not None else []))
        return out

    @staticmethod
    def backward(ctx, d_out):
        x, out, *gw = ctx.saved_tensors
        dx, g, d_gw, d_gb = ops.gn_bwd(d_out.contiguous(), x, out if ctx.relu else None, gw[0] if ctx.has_gn else None,
                                       eps=ctx.eps, want_g=ctx.has_res)
        return dx, d_gw, d_gb, (g if ctx.has_res else None), None, None


class GNCLFn(Function):
    """out = [ReLU](GroupNorm(1 group over (C, L))(x) [+ res]) on [n, C, L]: ActorNet's conv norms (one launch
    forward, one backward, instead of ~30 ATen launches of the explicit mean / var formula)."""

    @staticmethod
    def forward(ctx, x, gn_w, gn_b, res, relu: bool, eps: float):
        x = x.contiguous()
        out = ops.gn_cl(x, gn_w, gn_b, eps, res=res, relu=relu)
        ctx.relu, ctx.eps, ctx.has_res = relu, eps, res is not None
        ctx.save_for_backward(x, out, gn_w)
        return out

    @staticmethod
    def backward(ctx, d_out):
        x, out, gw = ctx.saved_tensors
        dx, g, d_gw, d_gb = ops.gn_cl_bwd(d_out, x, out if ctx.relu else None, gw, eps=ctx.eps, want_g=ctx.has_res)
        return dx, d_gw, d_gb, (g if ctx.has_res else None), None, None


def gn_cl_act(x, gn, relu=False, res=None):
    return GNCLFn.apply(x, gn.weight, gn.bias, res, relu, gn.eps)


class Conv1dGNFn(Function):
    """out = [ReLU](GroupNorm(1 group)(conv1d(x, weight)) [+ res | + up2(res)]) on channels-last tensors x [A, L, Cin] ->
    [A, Lout, Cout]: one unit of ActorNet (reference layers.py:40-62, 142-190).  Forward = lgcn_conv1d_gn_train (saving the
    pre-norm y), backward = lgcn_conv1d_gn_bwd (dx, dW, dgamma, dbeta, dres; exact fp32).  exact: the forward in exact fp32
    too (lgcn_conv1d_gn_f32); the backward is the same."""

    @staticmethod
    def forward(ctx, x, weight, gamma, beta, res, stride: int, res_mode: int, relu: bool, eps: float, exact: bool = False):
        out, y = ops.conv1d_gn_train(x, weight, stride, gamma, beta, eps, res=res if res_mode else None,
                                     res_up2=res_mode == 2, relu=relu, exact=exact)
        ctx.stride, ctx.res_mode, ctx.relu, ctx.eps = stride, res_mode, relu, eps
        ctx.save_for_backward(x, y, out, weight, gamma)
        return out

    @staticmethod
    def backward(ctx, d_out):
        x, y, out, weight, gamma = ctx.saved_tensors
        ni = ctx.needs_input_grad
        dx, dw, dg, db, dres = ops.conv1d_gn_bwd(d_out.contiguous(), x, y, out, weight, ctx.stride, gamma, ctx.eps,
                                                 res_mode=ctx.res_mode, relu=ctx.relu, want_dx=ni[0],
                                                 want_dres=ctx.res_mode != 0 and ni[4])
        return (dx, dw if ni[1] else None, dg if ni[2] else None, db if ni[3] else None, dres,
                None, None, None, None, None)


def conv1d_gn(x, conv, gn, res=None, res_up2=False, relu=False, exact=False):
    """Differentiable ops.conv1d_gn for an nn.Conv1d (no bias, padding (k - 1) / 2) and its nn.GroupNorm(1, C)."""
    mode = 0 if res is None else (2 if res_up2 else 1)
    return Conv1dGNFn.apply(x, conv.weight, gn.weight, gn.bias, res, conv.stride[0], mode, bool(relu), gn.eps, bool(exact))


class PredRegFn(Function):
    """(reg [A, M, T, 2], hd [A M, 128]) = lgcn_pred_reg of (h_0 .. h_{M-1}, W_0 .., b_0 .., ctrs, wd, bd): the M heads'
    nn.Linear(128, 2 T) + centre and AttDest's first layer on the detached destinations (reference lanegcn.py:601-614,
    725-729).  Backward = lgcn_pred_reg_bwd.  hd carries gradient to wd / bd only (the reference detaches the destination);
    ctrs gets none and must not ask for one."""

    @staticmethod
    def forward(ctx, *tensors):
        M = (len(tensors) - 3) // 3
        if M < 1 or len(tensors) != 3 * M + 3:
            raise L.LgcnError("PredRegFn: expected (h_0 .., W_0 .., b_0 .., ctrs, wd, bd)")
        if ctx.needs_input_grad[3 * M]:
            raise L.LgcnError("PredRegFn: no gradient with respect to ctrs")
        h = [t.contiguous() for t in tensors[:M]]
        w, b = tensors[M:2 * M], tensors[2 * M:3 * M]
        ctrs, wd, bd = tensors[3 * M:]
        reg, hd = ops.pred_reg(h, w, b, ctrs, wd, bd)
        ctx.n_mod = M
        ctx.set_materialize_grads(False)
        ctx.save_for_backward(*h, *w, ctrs, reg, hd)
        return reg, hd

    @staticmethod
    def backward(ctx, g_reg, g_hd):
        M, ni = ctx.n_mod, ctx.needs_input_grad
        saved = ctx.saved_tensors
        h, w = saved[:M], saved[M:2 * M]
        ctrs, reg, hd = saved[2 * M:]
        if g_reg is None:
            g_reg = torch.zeros_like(reg)
        want_w, want_d = any(ni[M:3 * M]), ni[3 * M + 1] or ni[3 * M + 2]
        d_h, d_w, d_b, d_wd, d_bd = ops.pred_reg_bwd(g_reg, g_hd, h, w, hd, reg, ctrs, want_h=ni[:M], want_w=want_w,
                                                     want_d=want_d)
        return (*d_h, *(d_w[m] if ni[M + m] else None for m in range(M)),
                *(d_b[m] if ni[2 * M + m] else None for m in range(M)), None,
                d_wd if ni[3 * M + 1] else None, d_bd if ni[3 * M + 2] else None)


class PredFinalFn(Function):
    """(cls [A, M] descending, out [A, M, T, 2] in that order) = lgcn_pred_final_train of (f, wc, bc, reg): the score
    nn.Linear(128, 1), the sort and the gather of reference lanegcn.py:616-622.  The order is saved, not returned; backward
    = lgcn_pred_final_bwd."""

    @staticmethod
    def forward(ctx, f, wc, bc, reg):
        f, reg = f.contiguous(), reg.contiguous()
        cls, out, order = ops.pred_final_train(f, wc, bc, reg)
        ctx.set_materialize_grads(False)
        ctx.save_for_backward(f, wc, order)
        ctx.n_pred = reg.shape[2]
        return cls, out

    @staticmethod
    def backward(ctx, g_cls, g_out):
        f, wc, order = ctx.saved_tensors
        ni = ctx.needs_input_grad
        g_reg, d_f, d_wc, d_bc = ops.pred_final_bwd(g_cls, g_out, order, f, wc, ctx.n_pred, want_reg=ni[3], want_f=ni[0])
        return d_f, d_wc.view_as(wc) if ni[1] else None, d_bc if ni[2] else None, g_reg


class PairAddFn(Function):
    """out[p] = c[p] + U[hi[p]] + V[wi[p]] (the hoisted query / context terms of lanegcn.py:696-699)."""

    @staticmethod
    def forward(ctx, c, U, V, pairs):
        P = c.shape[0]
        out = ops.pair_add(c, U, pairs.hi, V, pairs.wi, pairs.n_pairs, P)
        ctx.pairs, ctx.n_u, ctx.n_v = pairs, U.shape[0], V.shape[0]
        return out

    @staticmethod
    def backward(ctx, g):
        g = g.contiguous()
        ps = ctx.pairs
        dU = ops.gather_sum(g, ps.rowptr, None, ctx.n_u) if ctx.needs_input_grad[1] else None       # sorted by hi
        dV = None
        if ctx.needs_input_grad[2]:
            rp, col = ps.csr_by_wi(ctx.n_v)
            dV = ops.gather_sum(g, rp, col, ctx.n_v)
        return g, dU, dV, None


class AttPairsFn(Function):
    """S [T,128] = per-target sum of the pair MLP of Att (reference lanegcn.py:691-703; formulas: include/lgcn.h,
    lgcn_att_pairs_train) of (pairs, dist.0 weight / bias, dist.2 weight, dist.2 norm weight / bias, ctx.0 weight
    [128,384], U, V, ctx.0 norm weight / bias).  Exact fp32 in every matrix mode.  Forward = lgcn_att_pairs_train + the
    segment sum; only the inputs and the ReLU masks (48 B per pair) are saved -- m is not.  Backward =
    lgcn_att_pairs_bwd, then dU / dV as segment sums of dc.  The gradient of ctx.0's weight fills columns 0:128 of a zero
    [128,384]; the U / V row blocks add their own column blocks.  The centres of `pairs` get no gradient."""

    @staticmethod
    def forward(ctx, pairs, wd0, bd0, w_d2, gd_w, gd_b, w_c0, U, V, gc_w, gc_b, eps: float = ops.EPS):
        U, V = U.contiguous(), V.contiguous()
        m, masks = ops.att_pairs_train(pairs, wd0, bd0, w_d2, (gd_w, gd_b), w_c0, U, V, (gc_w, gc_b), eps=eps)
        ctx.pairs, ctx.eps = pairs, eps
        ctx.set_materialize_grads(False)
        ctx.save_for_backward(wd0, bd0, w_d2, gd_w, gd_b, w_c0, U, V, gc_w, gc_b, masks)
        return ops.gather_sum(m, pairs.rowptr, None, U.shape[0])

    @staticmethod
    def backward(ctx, dS):
        if dS is None:
            return (None,) * 12
        wd0, bd0, w_d2, gd_w, gd_b, w_c0, U, V, gc_w, gc_b, masks = ctx.saved_tensors
        ps, ni = ctx.pairs, ctx.needs_input_grad
        names = {1: "d_wd0", 2: "d_bd0", 3: "d_wd2", 4: "d_gd", 5: "d_btd", 6: "d_wc0e", 9: "d_gc", 10: "d_btc"}
        want = [n for i, n in names.items() if ni[i]]
        g = ops.att_pairs_bwd(ps, dS.contiguous(), masks, wd0, bd0, w_d2, (gd_w, gd_b), w_c0, U, V, (gc_w, gc_b), want=want,
                              want_dc=ni[7] or ni[8], eps=ctx.eps)
        out = [None] * 12
        for i, n in names.items():
            out[i] = g.get(n)
        if ni[6]:
            out[6] = torch.zeros_like(w_c0)
            out[6][:, :C_FEAT] = g["d_wc0e"]
        if ni[7]:
            out[7] = ops.gather_sum(g["dc"], ps.rowptr, None, U.shape[0])          # sorted by hi
        if ni[8]:
            rp, col = ps.csr_by_wi(V.shape[0])
            out[8] = ops.gather_sum(g["dc"], rp, col, V.shape[0])
        return tuple(out)


class PoolPairsFn(Function):
    """S [T,128] = per-target sum of the pair stage of the fork's LanePooling (reference lanercnn.py:492-499; formulas:
    include/lgcn.h, lgcn_pool_pairs_train) of (pairs with hi = target row and wi = context row, context poses [C,4],
    target poses [T,4], relpose.0 weight / bias, ctx.0 weight [128,256], U [C,128], ctx.0 norm weight / bias).  Exact fp32
    in every matrix mode.  Forward = lgcn_pool_pairs_train + the segment sum; only the inputs and the ReLU masks (32 B per
    pair) are saved -- m is not.  Backward = lgcn_pool_pairs_bwd, then dU as the segment sum of dz over the pairs by
    context row.  The gradient of ctx.0's weight fills columns 128:256 of a zero [128,256]; the U row block adds columns
    0:128.  The poses get no gradient."""

    @staticmethod
    def forward(ctx, pairs, ctx_pose, tgt_pose, wp, bp, w_c0, U, g_w, g_b, eps: float = ops.EPS):
        ctx_pose, tgt_pose, U = ctx_pose.contiguous(), tgt_pose.contiguous(), U.contiguous()
        P = pairs.count()
        m, masks = ops.pool_pairs_train(pairs, ctx_pose, tgt_pose, wp, bp, w_c0, U, (g_w, g_b), cap=P, eps=eps)
        ctx.pairs, ctx.eps, ctx.P = pairs, eps, P
        ctx.set_materialize_grads(False)
        ctx.save_for_backward(ctx_pose, tgt_pose, wp, bp, w_c0, U, g_w, g_b, masks)
        return ops.gather_sum(m, pairs.rowptr, None, tgt_pose.shape[0])

    @staticmethod
    def backward(ctx, dS):
        if dS is None:
            return (None,) * 10
        ctx_pose, tgt_pose, wp, bp, w_c0, U, g_w, g_b, masks = ctx.saved_tensors
        ps, ni = ctx.pairs, ctx.needs_input_grad
        names = {3: "d_wp", 4: "d_bp", 5: "d_w0h", 7: "d_g", 8: "d_bt"}
        want = [n for i, n in names.items() if ni[i]]
        g = ops.pool_pairs_bwd(ps, dS.contiguous(), masks, ctx_pose, tgt_pose, wp, bp, w_c0, U, (g_w, g_b), want=want,
                               want_dz=ni[6], cap=ctx.P, eps=ctx.eps)
        out = [None] * 10
        for i, n in names.items():
            out[i] = g.get(n)
        if ni[5]:
            out[5] = torch.zeros_like(w_c0)
            out[5][:, C_FEAT:] = g["d_w0h"]
        if ni[6]:
            rp, col = ps.csr_by_wi(U.shape[0])
            out[6] = ops.gather_sum(g["dz"], rp, col, U.shape[0])
        return tuple(out)


class GatherSumFn(Function):
    """out[n] = sum of src rows over a CSR (rowptr, col) by destination: the differentiable index_add_ of a gathered
    tensor (reference lanercnn.py:343: out.index_add_(0, v, agt_fc(agt[u]))).  Backward = the same gather over the
    transposed CSR (plan_t: rows = sources)."""

    @staticmethod
    def forward(ctx, src, plan, plan_t, n_rows: int):
        ctx.plan_t, ctx.n_src = plan_t, src.shape[0]
        return ops.gather_sum(src.contiguous(), plan.rowptr, plan.col, n_rows)

    @staticmethod
    def backward(ctx, g):
        return ops.gather_sum(g.contiguous(), ctx.plan_t.rowptr, ctx.plan_t.col, ctx.n_src), None, None, None


# ------------------------------------------------------------------ convenience wrappers
def row_block(srcs, weights, rels, n_rows, gn=None, relu=False, res=None, **kw):
    """Differentiable row block.  gn: nn.GroupNorm or None.  fused_bwd (default: RowBlockFn.train_hip): see BlockSpec."""
    kw.setdefault("fused_bwd", RowBlockFn.train_hip)
    spec = BlockSpec(n_rows=n_rows, rels=rels, gn=gn is not None, relu=relu, has_res=res is not None,
                     eps=gn.eps if gn is not None else ops.EPS, **kw)
    gw, gb = (gn.weight, gn.bias) if gn is not None else (None, None)
    return RowBlockFn.apply(spec, len(srcs), len(weights), *srcs, *weights, gw, gb, res)


def linear_gn(x, weight, gn=None, relu=False, res=None, col0=0):
    """[ReLU]([GN](x W[:, col0:col0+128]^T) [+ res])."""
    return row_block([x], [weight], [Rel(0, 0, L.REL_IDENT, 0, col0)], x.shape[0], gn=gn, relu=relu, res=res)


def gn_act(x, gn=None, relu=False, res=None):
    gw, gb = (gn.weight, gn.bias) if gn is not None else (None, None)
    return GNActFn.apply(x, gw, gb, res, relu, gn.eps if gn is not None else ops.EPS)


class PredLossFn(torch.autograd.Function):
    """PredLoss's two sums (reference lanegcn.py:740-807) in one launch, gradients in one more (csrc/lgcn_loss.hip).
    Returns (cls_loss, reg_loss, counts [2] int32 on the device: num_cls, num_reg)."""

    @staticmethod
    def forward(ctx, cls, reg, gt, has, cfg):
        cls, reg = cls.contiguous(), reg.contiguous()
        sums, counts, sel = ops.pred_loss_fwd(cls, reg, gt, has, cfg)
        ctx.save_for_backward(cls, reg, gt, has, sel)
        ctx.cfg = cfg
        ctx.mark_non_differentiable(counts)
        return sums[0], sums[1], counts

    @staticmethod
    def backward(ctx, g_cls, g_reg, _):
        cls, reg, gt, has, sel = ctx.saved_tensors
        z = lambda g: torch.zeros(1, dtype=torch.float32, device=cls.device) if g is None else g.reshape(1).float().contiguous()
        dcls, dreg = ops.pred_loss_bwd(cls, reg, gt, has, ctx.cfg, sel, z(g_cls), z(g_reg))
        return dcls, dreg, None, None, None


class GoalDecodeFn(Function):
    """lgcn_goal_decode under autograd (Decode.train_hip): the forward is the inference launch, the backward one
    lgcn_goal_decode_bwd launch.  Returns (top_idx, goals, logits, coef, s_samples); only pred receives a gradient and
    the selection top_idx is not differentiated."""

    @staticmethod
    def forward(ctx, pred, pred_spans, anc_ctrs, anc_dirs, anc_first, agt_ctrs, agt_dir_last, agt_vel, k, threshold):
        pred = pred.contiguous()
        top, goals, logits, coef, ss = ops.goal_decode(pred, pred_spans, anc_ctrs, anc_dirs, anc_first, agt_ctrs, agt_dir_last,
                                                       agt_vel, k, threshold)
        ctx.save_for_backward(pred, anc_ctrs, anc_dirs, agt_ctrs, agt_dir_last, agt_vel, top)
        ctx.tables = (list(pred_spans), list(anc_first))
        ctx.mark_non_differentiable(top)
        return top, goals, logits, coef, ss

    @staticmethod
    def backward(ctx, _, d_goals, d_logits, d_coef, d_ss):
        pred, anc_ctrs, anc_dirs, agt_ctrs, agt_dir_last, agt_vel, top = ctx.saved_tensors
        pred_spans, anc_first = ctx.tables
        d_pred = ops.goal_decode_bwd(pred, pred_spans, anc_ctrs, anc_dirs, anc_first, agt_ctrs, agt_dir_last, agt_vel, top,
                                     d_goals, d_logits, d_coef, d_ss)
        return (d_pred,) + (None,) * 9


class GoalRefineFn(Function):
    """lgcn_goal_refine under autograd: pred_trajs = refine(s_samples, coef, traj_delta); backward = one
    lgcn_goal_refine_bwd launch."""

    @staticmethod
    def forward(ctx, s_samples, coef, traj_delta):
        s_samples, coef, traj_delta = s_samples.contiguous(), coef.contiguous(), traj_delta.contiguous()
        ctx.save_for_backward(s_samples, coef, traj_delta)
        return ops.goal_refine(s_samples, coef, traj_delta)

    @staticmethod
    def backward(ctx, d_out):
        s_samples, coef, traj_delta = ctx.saved_tensors
        return ops.goal_refine_bwd(s_samples, coef, traj_delta, d_out.contiguous())


class RoiLossFn(Function):
    """RoiLoss's three sums (reference lanercnn.py:1214-1301) in one launch, gradients in one more (csrc/lgcn_loss.hip).
    Returns (cls_loss, reg_goal_loss, reg_traj_loss, counts [3] int32 on the device: num_cls, num_reg_goal,
    num_reg_traj, pred_goals [A, 2] = the goal of the selected mode, not differentiated)."""

    @staticmethod
    def forward(ctx, logits, goals, trajs, gt, has, reg_coef):
        logits, goals, trajs = logits.contiguous(), goals.contiguous(), trajs.contiguous()
        sums, counts, sel, pred_goals = ops.roi_loss_fwd(logits, goals, trajs, gt, has, reg_coef)
        ctx.save_for_backward(logits, goals, trajs, gt, has, sel)
        ctx.reg_coef = reg_coef
        ctx.mark_non_differentiable(counts, pred_goals)
        return sums[0], sums[1], sums[2], counts, pred_goals

    @staticmethod
    def backward(ctx, g_cls, g_goal, g_traj, _c, _p):
        logits, goals, trajs, gt, has, sel = ctx.saved_tensors
        z = lambda g: torch.zeros(1, dtype=torch.float32, device=logits.device) if g is None else g.reshape(1).float().contiguous()
        dlogits, dgoals, dtrajs = ops.roi_loss_bwd(logits, goals, trajs, gt, has, ctx.reg_coef, sel, z(g_cls), z(g_goal), z(g_traj))
        return dlogits, dgoals, dtrajs, None, None, None
