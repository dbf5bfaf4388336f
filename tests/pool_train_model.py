"""Float64 model, in plain torch autograd on the CPU, of the training of LanePooling's pair stage as include/lgcn.h states
it for lgcn_pool_pairs_train / lgcn_pool_pairs_bwd -- TEST INFRASTRUCTURE ONLY.  The forward is pool_pairs_model.pair_stage
with its two ReLUs replaced by multiplications with given masks (the backward kernel reads the stored masks, it does not
re-derive them); with the masks of the pre-activations' own signs it is pair_stage to the bit
(test_host_pool_train_cabi.py)."""
import torch

from pool_pairs_model import C, EPS, gn64

NAMES = ("wp", "bp", "w0h", "U", "g", "bt")


def pre_activations(ctx_pose, tgt_pose, ti, ci, x, mask0, eps=EPS):
    """(y0, y1 = GN(z)) [P,128] in float64 and z, for leaves x (a dict over NAMES of float64 tensors); mask0 [P,128] is
    the first ReLU, None for the sign of y0 itself.  The pose subtraction is done in fp32, as in the kernel."""
    d = (ctx_pose.float()[ci] - tgt_pose.float()[ti]).double()
    y0 = d @ x["wp"].t() + x["bp"]
    h = torch.relu(y0) if mask0 is None else y0 * mask0.double()
    z = h @ x["w0h"].t() + x["U"][ci]
    return y0, gn64(z, x["g"], x["bt"], eps), z


def true_masks(ctx_pose, tgt_pose, ti, ci, inp, eps=EPS):
    """bool [P,2,128]: the signs of the model's own pre-activations."""
    x = {k: inp[k].double() for k in NAMES}
    y0, y1, _ = pre_activations(ctx_pose, tgt_pose, ti, ci, x, None, eps)
    return torch.stack([y0 > 0, y1 > 0], 1)


def forward(ctx_pose, tgt_pose, ti, ci, inp, masks, n_tgt, eps=EPS):
    """(m [P,128], S [n_tgt,128]) in float64 with the ReLUs as the given masks [P,2,128]."""
    x = {k: inp[k].double() for k in NAMES}
    _, y1, _ = pre_activations(ctx_pose, tgt_pose, ti, ci, x, masks[:, 0], eps)
    m = y1 * masks[:, 1].double()
    return m, torch.zeros(n_tgt, C, dtype=torch.float64).index_add(0, ti, m)


def train_step(ctx_pose, tgt_pose, ti, ci, inp, masks, dS, eps=EPS):
    """Forward and backward for the loss sum(S * dS): (S, gradients by NAMES + "dz", (y0, y1)).  inp: fp32 or fp64 tensors
    over NAMES (w0h [128,128] = ctx.0's columns 128:256); masks bool [P,2,128]; dS [T,128]."""
    x = {k: inp[k].double().clone().requires_grad_(True) for k in NAMES}
    y0, y1, z = pre_activations(ctx_pose, tgt_pose, ti, ci, x, masks[:, 0], eps)
    z.retain_grad()
    S = torch.zeros(dS.shape[0], C, dtype=torch.float64).index_add(0, ti, y1 * masks[:, 1].double())
    (S * dS.double()).sum().backward()
    grads = {k: v.grad for k, v in x.items()}
    grads["dz"] = z.grad
    return S.detach(), grads, (y0.detach(), y1.detach())
