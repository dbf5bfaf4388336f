"""GPU: the fork model's loss (lgcn_roi_loss_fwd / lgcn_roi_loss_bwd in csrc/lgcn_loss.hip, autograd.RoiLossFn,
lanercnn.RoiLoss / Loss) on the reference's recorded run (tests/golden/lanercnn_roi_loss.npz) against the float64
restatement (tests/roi_loss_model.py, pinned by test_roi_loss_model_host.py).

Bars: per quantity max(4 x the relative error of the reference's own fp32 result against the same float64 model, 1e-6),
the convention of test_gpu_goal_decode.bars.  For the tiled sizes, where the reference was not run, its fp32 result is
the model evaluated in fp32 on the CPU (the same ATen operations; pinned to the recording at 1e-6 by the host test)."""
import numpy as np
import pytest
import torch

import roi_loss_model as RM

pytestmark = pytest.mark.gpu
SUMS = ("cls_loss", "reg_goal_loss", "reg_traj_loss")
GRADS = ("d_logits", "d_goals", "d_trajs")


@pytest.fixture(scope="module")
def ops():
    import lanegcn_amd  # noqa: F401
    from lanegcn_amd import ops
    return ops


def device_inputs(a):
    t = lambda x: torch.from_numpy(np.ascontiguousarray(x)).cuda()
    return [t(a[k]) for k in ("logits", "goals", "trajs", "gt", "has")]


def upstream(ref):
    """d loss / d (cls, reg_goal, reg_traj) as Loss combines them: 1 / (count + 1e-10), rounded to fp32."""
    return [torch.tensor([1.0 / (ref[k] + 1e-10)], dtype=torch.float32).cuda() for k in ("num_cls", "num_reg_goal", "num_reg_traj")]


def scalar_err(got, ref):
    return abs(float(got) - float(ref)) / max(abs(float(ref)), 1e-300)


def bars(ref32, ref64):
    bar = {k: max(4 * scalar_err(ref32[k], ref64[k]), 1e-6) for k in SUMS}
    bar.update({k: max(4 * RM.rel_err(ref32[k], ref64[k]), 1e-6) for k in GRADS})
    return bar


def check(ops, rows, ref32, ref64, what):
    a = RM.tiled(rows)
    ins = device_inputs(a)
    keep = [t.clone() for t in ins]
    coef = float(RM.fixture()["reg_coef"])
    sums, counts, sel, pred_goals = ops.roi_loss_fwd(*ins, coef)
    g = upstream(ref64)
    grads = ops.roi_loss_bwd(*ins, coef, sel, *g)
    has_goal = a["has"][np.arange(len(a["has"])), a["last_idcs"]]
    assert np.array_equal(sel.cpu().numpy(), a["min_idcs"] | (has_goal.astype(np.int64) << 8))
    assert counts.tolist() == [int(ref64[k]) for k in ("num_cls", "num_reg_goal", "num_reg_traj")]
    assert np.array_equal(pred_goals.cpu().numpy(), a["goals"][np.arange(len(a["goals"])), a["min_idcs"]])
    bar = bars(ref32, ref64)
    errs = {k: scalar_err(sums[i].item(), ref64[k]) for i, k in enumerate(SUMS)}
    errs.update({k: RM.rel_err(grads[i].cpu().numpy(), ref64[k]) for i, k in enumerate(GRADS)})
    for k, e in errs.items():
        print("%s %-14s rel error %.2e (bar %.2e)" % (what, k, e, bar[k]))
    for k, e in errs.items():
        assert e <= bar[k], (what, k, e, bar[k])
    for i, k in enumerate(GRADS):                          # zeros off the selected mode / unobserved steps: exactly
        assert np.array_equal(grads[i].cpu().numpy() == 0, ref64[k] == 0), k
    # bitwise repeatable; inputs unmodified
    again = ops.roi_loss_fwd(*ins, coef)
    assert all(torch.equal(x, y) for x, y in zip(again, (sums, counts, sel, pred_goals)))
    assert all(torch.equal(x, y) for x, y in zip(ops.roi_loss_bwd(*ins, coef, sel, *g), grads))
    assert all(torch.equal(x, y) for x, y in zip(ins, keep))


def test_roi_loss_kernels_on_the_reference_run(ops):
    g = RM.fixture()
    ref32 = {k: g["loss_out/" + k] for k in SUMS}
    ref32.update({k: g[k] for k in GRADS})
    check(ops, None, ref32, RM.reference(), "A=37")


@pytest.mark.parametrize("rows", [1, 1025, 4097])
def test_roi_loss_kernels_on_tiled_rows(ops, rows):
    """1025 agents: more than one agent per thread of the 1024-thread block, and the whole cross-thread tree.  4097 agents:
    one more than the 4096 workgroups of k_roi_loss_bwd, so workgroup 0 strides on to a second agent."""
    check(ops, rows, RM.reference(rows, torch.float32), RM.reference(rows), "A=%d" % rows)


def test_roi_loss_of_an_empty_batch(ops):
    a = RM.tiled(0)
    ins = device_inputs(a)
    sums, counts, sel, pred_goals = ops.roi_loss_fwd(*ins, 1.0)
    assert sums.tolist() == [0.0, 0.0, 0.0] and counts.tolist() == [0, 0, 0]
    assert tuple(sel.shape) == (0,) and tuple(pred_goals.shape) == (0, 2)
    one = torch.ones(1, device="cuda")
    grads = ops.roi_loss_bwd(*ins, 1.0, sel, one, one, one)
    assert [tuple(x.shape) for x in grads] == [(0, 6), (0, 6, 2), (0, 6, 30, 2)]


def test_loss_module_on_the_reference_run():
    import lanegcn_amd  # noqa: F401
    from lanegcn_amd import _lib
    from lanegcn_amd import lanegcn as M
    from lanegcn_amd import lanercnn as R
    g = RM.fixture()
    ref = RM.reference()
    ref32 = {k: g["loss_out/" + k] for k in SUMS + ("loss",)}
    ref32.update({k: g[k] for k in GRADS})
    bar = bars(ref32, ref)
    bar["loss"] = max(4 * scalar_err(ref32["loss"], ref["loss"]), 1e-6)
    t = lambda x: torch.from_numpy(np.ascontiguousarray(x))
    data = {k: [t(g["data/%s/%d" % (k, b)]) for b in range(37)] for k in ("valid_agent_ids", "gt_preds", "has_preds")}   # on the CPU
    out = {"pred_logics": t(g["logits"]).cuda().requires_grad_(True), "pred_goals": t(g["goals"]).cuda().requires_grad_(True),
           "pred_trajs": t(g["trajs"]).cuda().requires_grad_(True)}
    loss = R.Loss(dict(M.config, num_mods=6, num_preds=30))
    lo = loss(out, data)
    assert set(lo) == {"cls_loss", "num_cls", "reg_goal_loss", "num_reg_goal", "reg_traj_loss", "num_reg_traj", "stage_one_loss",
                       "num_stage_one", "pred_goals", "pred_trajs", "loss"}
    for k in ("num_cls", "num_reg_goal", "num_reg_traj", "num_stage_one", "stage_one_loss"):
        assert not torch.is_tensor(lo[k]) and lo[k] == int(g["loss_out/" + k]), k
    assert np.array_equal(lo["pred_goals"].cpu().numpy(), g["loss_out/pred_goals"])
    assert lo["pred_trajs"] is out["pred_trajs"]
    for k in SUMS + ("loss",):
        e = scalar_err(lo[k].item(), ref[k])
        print("module %-14s rel error %.2e (bar %.2e)" % (k, e, bar[k]))
        assert e <= bar[k], k
    lo["loss"].backward()
    for k, name in zip(GRADS, ("pred_logics", "pred_goals", "pred_trajs")):
        e = RM.rel_err(out[name].grad.cpu().numpy(), ref[k])
        print("module %-14s rel error %.2e (bar %.2e)" % (k, e, bar[k]))
        assert e <= bar[k], k
    # host-side bookkeeping on the result
    post = R.PostProcess(loss.config)
    po = post(out, data, lo)
    assert po["goals"][0].shape == (37, 2) and po["trajs"][0].shape == (37, 6, 30, 2) and len(po["gt_preds"]) == 37
    m = post.append({}, lo, po)
    assert m["num_cls"] == 37 and abs(m["cls_loss"] - float(g["loss_out/cls_loss"])) <= 1e-3
    # CPU tensors are refused
    with pytest.raises(_lib.LgcnError):
        loss({k: v.detach().cpu() for k, v in out.items()}, data)
