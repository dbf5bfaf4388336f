"""CPU: the float64 restatement of RoiLoss / Loss (tests/roi_loss_model.py) reproduces the reference's own run recorded
in tests/golden/lanercnn_roi_loss.npz: the same indices, its sums and its gradients to 1e-6 relative (the reference ran
in fp32; the comparison is model-in-fp32 against it, and model-in-float64 within fp32's reach of it)."""
import numpy as np
import torch

import roi_loss_model as RM

SUMS = ("cls_loss", "reg_goal_loss", "reg_traj_loss", "loss")
COUNTS = ("num_cls", "num_reg_goal", "num_reg_traj", "num_stage_one")


def test_fixture_holds_what_the_tests_need():
    g = RM.fixture()
    assert g["logits"].shape == (37, 6) and g["goals"].shape == (37, 6, 2) and g["trajs"].shape == (37, 6, 30, 2)
    assert g["gt"].shape == (37, 30, 2) and g["has"].shape == (37, 30) and g["has"].dtype == np.bool_
    has = g["has"]
    assert has.all(1).any() and (~has).all(1).any()                              # all true, all false
    assert any(h[0] and not h[1:].any() for h in has)                            # only step 0
    assert any(h[0] and not h[-1] and h.sum() > 1 for h in has)                  # a false tail
    assert any(h[0] and h[-1] and not h.all() for h in has)                      # a hole in the middle
    assert g["margins"][0] >= 1e-3 and g["margins"][1] >= 1e-3
    for b in range(37):                                                          # the first valid agent's rows
        first = int(g["data/valid_agent_ids/%d" % b][0])
        assert np.array_equal(g["data/gt_preds/%d" % b][first], g["gt"][b])
        assert np.array_equal(g["data/has_preds/%d" % b][first], g["has"][b])


def test_model_selects_the_reference_indices():
    g = RM.fixture()
    has = torch.from_numpy(g["has"])
    last = RM.last_step(has)
    assert np.array_equal(last.numpy(), g["last_idcs"])
    assert (g["last_idcs"][~g["has"].any(1)] == 29).all()                        # no observed step: T - 1
    for dtype in (torch.float32, torch.float64):
        mins, _ = RM.closest_mode(torch.from_numpy(g["goals"]).to(dtype), torch.from_numpy(g["gt"]).to(dtype), last)
        assert np.array_equal(mins.numpy(), g["min_idcs"]), dtype


def test_model_reproduces_the_reference_sums_and_gradients():
    g = RM.fixture()
    args = (g["logits"], g["goals"], g["trajs"], g["gt"], g["has"], float(g["reg_coef"]))
    for dtype, given in ((torch.float32, False), (torch.float64, False), (torch.float64, True)):
        idx = dict(last_idcs=g["last_idcs"], min_idcs=g["min_idcs"]) if given else {}
        r = RM.loss_and_grads(*args, dtype=dtype, **idx)
        assert np.array_equal(r["last_idcs"], g["last_idcs"]) and np.array_equal(r["min_idcs"], g["min_idcs"])
        for k in COUNTS:
            assert int(r[k]) == int(g["loss_out/" + k]), k
        assert r["stage_one_loss"] == 0 and int(g["loss_out/stage_one_loss"]) == 0
        for k in SUMS:
            assert abs(float(r[k]) - float(g["loss_out/" + k])) <= 1e-6 * abs(float(g["loss_out/" + k])), (k, dtype)
        assert RM.rel_err(r["pred_goals"], g["loss_out/pred_goals"]) == 0.0
        for k in ("d_logits", "d_goals", "d_trajs"):
            assert RM.rel_err(r[k], g[k]) <= 1e-6, (k, dtype, RM.rel_err(r[k], g[k]))
            assert np.array_equal(r[k] == 0, g[k] == 0), k                       # the same elements carry no gradient


def test_shared_reference_is_tiled_consistently():
    one, three = RM.reference(), RM.reference(111)
    assert three["d_trajs"].shape[0] == 111 and int(three["num_reg_traj"]) == 3 * int(one["num_reg_traj"])
    assert abs(float(three["cls_loss"]) - 3 * float(one["cls_loss"])) <= 1e-12 * float(three["cls_loss"])
    assert RM.tiled(40)["logits"].shape == (40, 6) and np.array_equal(RM.tiled(40)["gt"][37:], RM.fixture()["gt"][:3])
    assert RM.reference(1)["num_cls"] == 1
