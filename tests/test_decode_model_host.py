"""CPU: the float64 restatement of the goal decoder (tests/decode_model.py) against the reference's own captures
(tests/golden/lanercnn_decode_b3.npz): it is the yardstick of the GPU tests, so it is pinned here first."""
import numpy as np
import pytest
import torch

import decode_model as DM

TOL = 1e-5


@pytest.fixture(scope="module")
def fx():
    return DM.fixture()[0]


def test_restatement_reproduces_the_reference_indices(fx):
    ref = DM.reference64()
    assert np.array_equal(ref["top_idx"], fx["dec/top_k"])
    for a in range(len(fx["dec/interest_roi"])):
        got = DM.greedy(fx["dec/nms_xy/%d" % a], fx["dec/nms_logits/%d" % a], 2.0, 6, 0)
        assert got == fx["dec/nms_list/%d" % a].tolist(), a


def test_argmax_form_equals_the_recorded_lists(fx):
    sizes = []
    for a in range(len(fx["dec/interest_roi"])):
        xy, lg, want = fx["dec/nms_xy/%d" % a], fx["dec/nms_logits/%d" % a], fx["dec/nms_list/%d" % a].tolist()
        assert DM.greedy_argmax(xy, lg, 2.0, 6, 0) == want, a
        assert DM.greedy_argmax(xy, lg, 2.0, 6, 6) == want[:6], a
        sizes.append(len(xy))
    assert sorted(sizes) == [6, 7, 64, 160]


def test_restatement_reproduces_the_reference_values(fx):
    ref = DM.reference64()
    pairs = {"goals": "dec/out_goals", "logits": "dec/out_logits", "thetas": "dec/thetas", "coef": "dec/coef",
             "s_samples": "dec/s_samples", "pred_trajs": "dec/out_trajs"}
    for mine, theirs in pairs.items():
        e = DM.rel_err(ref[mine].numpy(), fx[theirs])
        print("%-10s rel error of the reference's fp32 against float64: %.2e" % (mine, e))
        assert e <= TOL, (mine, e)
    # the normalised samples of both stages, and the refined un-normalised ones
    s2 = ref["s_samples"] + torch.from_numpy(fx["dec/traj_delta"]).double()[..., 0]
    assert DM.rel_err(s2.numpy(), fx["dec/s_samples_refined"]) <= TOL
    assert DM.rel_err(DM.normalise(ref["s_samples"]).numpy(), fx["dec/s_norm"]) <= TOL
    assert DM.rel_err(DM.normalise(s2).numpy(), fx["dec/s_norm_refined"]) <= TOL
    assert float(ref["denominators"].min()) >= 1.0


def test_module_restatement_reproduces_the_reference_stages(fx):
    """decode_forward (fp32 here, same ATen ops) against the captured stages: it is the float64 reference of the
    gradient tests, and this pins the reference's pooling row numbering (context offset + 1 per scene)."""
    from oracle import lanercnn_oracle as OR
    names = DM.fixture()[1]
    sd = OR.seeded_state([(k, tuple(s)) for k, s in names["decode"]], int(fx["seed"]))
    a = DM.decode_args(fx, torch.float32)
    out = DM.decode_forward(sd, torch.from_numpy(fx["dec/roi_feat"]), a["spans"], a["anc_ctrs"], a["anc_dirs"], a["agt_ctrs"],
                            a["agt_dirs"], a["agt_trajs"], a["agt_vel"], OR.lane_pooling)
    assert np.array_equal(out["top_idx"], fx["dec/top_k"])
    for mine, theirs in (("pred", "dec/pred"), ("pooled", "dec/pooled"), ("traj_delta", "dec/traj_delta"),
                         ("pred_trajs", "dec/out_trajs")):
        assert float(np.abs(out[mine].numpy() - fx[theirs]).max()) <= 1e-5 * max(1.0, float(np.abs(fx[theirs]).max())), mine
