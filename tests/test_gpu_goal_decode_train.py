"""GPU: training the goal decoder on its inference launches (Decode.train_hip): autograd.GoalDecodeFn / GoalRefineFn on
lgcn_goal_decode_bwd / lgcn_goal_refine_bwd (csrc/lgcn_goal_bwd.hip) against CPU float64 autograd of the restatement
(tests/decode_model.py), on the inputs of tests/golden/lanercnn_decode_b3.npz (interest RoIs of 6, 7, 64 and 160 nodes;
with 6 nodes every node is selected and the padding path runs) and on one synthetic decelerating agent.

Bar per gradient tensor: max(4 x the error of the stock-op training path (Decode with train_hip = False: _decode_torch
and the elementwise tail of Decode.decode) against the same float64 gradients, 1e-6)."""
import numpy as np
import pytest
import torch

import decode_model as DM
from test_gpu_lanercnn_heads import GTOL, decode_inputs, decode_module, f32, rel, state  # noqa: F401  (f32: a fixture)

pytestmark = pytest.mark.gpu
K = 6


@pytest.fixture(scope="module")
def mods():
    import lanegcn_amd  # noqa: F401
    from lanegcn_amd import autograd, lanercnn, ops
    return ops, autograd, lanercnn


def fixture_case():
    g = DM.fixture()[0]
    a = DM.decode_args(g)
    spans = a["spans"]
    f = lambda t: t.numpy().astype(np.float32)             # fp32 values held in float64: the cast is exact
    case = {"pred": g["dec/pred"], "spans": spans, "anc_ctrs": f(a["anc_ctrs"]), "anc_dirs": f(a["anc_dirs"]),
            "agt_ctrs": f(a["agt_ctrs"]), "dir_last": f(a["agt_dirs"][:, -1]), "agt_vel": f(a["agt_vel"]),
            "delta": g["dec/traj_delta"]}
    return case, g["dec/top_k"]


def synthetic_case():
    """One agent at 14 m/s whose goals lie 4-9 m ahead: the constant deceleration that covers so short a curve in 3 s
    stops it early, so the later v_j clamp to 0."""
    rng = np.random.default_rng(41)
    n, heading = 9, 0.6
    ahead = np.array([np.cos(heading), np.sin(heading)])
    side = np.array([-np.sin(heading), np.cos(heading)])
    anc = np.stack([ahead * (4.0 + 2.5 * (i % 3)) + side * 2.5 * (i // 3 - 1) for i in range(n)]) + rng.normal(0, 0.05, (n, 2))
    th = heading + rng.normal(0, 0.05, n)
    pred = np.concatenate([rng.permutation(n)[:, None] * 0.3 - 1.0, rng.normal(0, 0.2, (n, 2)), rng.normal(0, 0.2, (n, 1)),
                           1.0 + rng.normal(0, 0.1, (n, 1))], 1)
    f = lambda x: np.ascontiguousarray(x, dtype=np.float32)
    return {"pred": f(pred), "spans": [(3, 3 + n)], "anc_ctrs": f(np.concatenate([np.zeros((3, 2)), anc])),
            "anc_dirs": f(np.concatenate([np.ones((3, 2)), np.stack([np.cos(th), np.sin(th)], 1)])),
            "agt_ctrs": f([[0.2, -0.1]]), "dir_last": f([ahead * 1.4]), "agt_vel": f([14.0]),
            "delta": f(rng.normal(0, 0.05, (1, K, 30, 2)))}


def gradient_errors(mods, case, seed, want_top=None):
    """Gradients of sum(w * outputs) through the decode and the refine stage: HIP Functions and the stock ops against CPU
    float64 autograd.  Returns (errors of the HIP path, errors of the stock path, details)."""
    ops, A, R = mods
    spans = case["spans"]
    pred_spans = [0] + [int(v) for v in np.cumsum([hi - lo for lo, hi in spans])]
    first = [lo for lo, _ in spans]
    n_agt = len(spans)
    cu = lambda x: torch.from_numpy(np.ascontiguousarray(x)).cuda()
    fixed = [cu(case[k]) for k in ("anc_ctrs", "anc_dirs")], [cu(case[k]) for k in ("agt_ctrs", "dir_last", "agt_vel")]
    (anc_c, anc_d), (agt_c, dir_last, vel) = fixed
    rng = np.random.default_rng(seed)
    w = {k: rng.normal(0, 1, s) for k, s in (("goals", (n_agt, K, 2)), ("logits", (n_agt, K)), ("coef", (n_agt, K, 6)),
                                              ("s_samples", (n_agt, K, 30)), ("trajs", (n_agt, K, 30, 2)))}
    wc = {k: cu(v.astype(np.float32)) for k, v in w.items()}
    w64 = {k: torch.from_numpy(v.astype(np.float32)).double() for k, v in w.items()}

    # ---- HIP: the inference launches under autograd
    pred = cu(case["pred"]).requires_grad_(True)
    top, goals, logits, coef, ss = A.GoalDecodeFn.apply(pred, pred_spans, anc_c, anc_d, first, agt_c, dir_last, vel, K, 2.0)
    assert not top.requires_grad and goals.requires_grad
    ((goals * wc["goals"]).sum() + (logits * wc["logits"]).sum() + (coef * wc["coef"]).sum() + (ss * wc["s_samples"]).sum()).backward()
    top_np = top.cpu().numpy()
    if want_top is not None:
        assert np.array_equal(top_np, want_top)
    ss0, coef0 = ss.detach().clone(), coef.detach().clone()
    leaves = [ss0.clone().requires_grad_(True), coef0.clone().requires_grad_(True), cu(case["delta"]).requires_grad_(True)]
    trajs = A.GoalRefineFn.apply(*leaves)
    (trajs * wc["trajs"]).sum().backward()
    hip = {"d_pred": pred.grad, "d_s_samples": leaves[0].grad, "d_coef": leaves[1].grad, "d_traj_delta": leaves[2].grad}
    # the forward under autograd is the inference forward, bit for bit
    with torch.no_grad():
        plain = ops.goal_decode(pred.detach(), pred_spans, anc_c, anc_d, first, agt_c, dir_last, vel, K, 2.0)
        assert all(torch.equal(x, y) for x, y in zip(plain, (top, goals, logits, coef, ss)))
        assert torch.equal(ops.goal_refine(ss0, coef0, leaves[2].detach()), trajs)

    # ---- the stock-op training path (Decode with train_hip = False), restated stage by stage
    pred_s = cu(case["pred"]).requires_grad_(True)
    top_s, goals_s, logits_s, coefs_s, ss_s = R.Decode._decode_torch(None, pred_s, pred_spans, anc_c, anc_d, spans, agt_c, dir_last, vel, K)
    assert np.array_equal(top_s.cpu().numpy(), top_np)
    ((goals_s * wc["goals"]).sum() + (logits_s * wc["logits"]).sum() + (torch.cat(coefs_s, 2) * wc["coef"]).sum()
     + (ss_s * wc["s_samples"]).sum()).backward()
    lv = [ss0.clone().requires_grad_(True), coef0.clone().requires_grad_(True), cu(case["delta"]).requires_grad_(True)]
    s = lv[0] + lv[2][..., 0]
    s = s / s.max(2, keepdim=True)[0]
    s = torch.where(s == 0.0, torch.ones_like(s), s)
    cs = tuple(lv[1][..., i:i + 1] for i in range(6))
    tangent = R.sample_d1_trajectory(s, *cs)
    normal = torch.stack([-tangent[..., 1], tangent[..., 0]], -1)
    ((R.sample_trajectory(s, *cs) + normal * lv[2][..., 1:2]) * wc["trajs"]).sum().backward()
    stock = {"d_pred": pred_s.grad, "d_s_samples": lv[0].grad, "d_coef": lv[1].grad, "d_traj_delta": lv[2].grad}

    # ---- CPU float64 autograd of the restatement, the same indices
    t64 = lambda x: torch.from_numpy(np.ascontiguousarray(x)).double()
    pred64 = t64(case["pred"]).requires_grad_(True)
    dec = DM.decode(pred64, pred_spans, t64(case["anc_ctrs"]), t64(case["anc_dirs"]), first, t64(case["agt_ctrs"]),
                    t64(case["dir_last"]), t64(case["agt_vel"]), K, top_idx=top_np)
    ((dec["goals"] * w64["goals"]).sum() + (dec["logits"] * w64["logits"]).sum() + (dec["coef"] * w64["coef"]).sum()
     + (dec["s_samples"] * w64["s_samples"]).sum()).backward()
    l64 = [ss0.cpu().double().requires_grad_(True), coef0.cpu().double().requires_grad_(True), t64(case["delta"]).requires_grad_(True)]
    (DM.refine(*l64) * w64["trajs"]).sum().backward()
    ref = {"d_pred": pred64.grad, "d_s_samples": l64[0].grad, "d_coef": l64[1].grad, "d_traj_delta": l64[2].grad}

    e_hip = {k: DM.rel_err(hip[k].cpu().numpy(), ref[k].numpy()) for k in ref}
    e_stock = {k: DM.rel_err(stock[k].cpu().numpy(), ref[k].numpy()) for k in ref}
    return e_hip, e_stock, {"hip": hip, "top": top_np, "pred_spans": pred_spans, "dec64": dec, "l64": l64, "ref": ref}


def assert_under_bars(e_hip, e_stock, what):
    bar = {k: max(4 * e_stock[k], 1e-6) for k in e_hip}
    for k in e_hip:
        print("%s %-13s rel error %.2e (stock path %.2e, bar %.2e)" % (what, k, e_hip[k], e_stock[k], bar[k]))
    for k in e_hip:
        assert e_hip[k] <= bar[k], (what, k, e_hip[k], bar[k])


def test_decode_and_refine_gradients_on_the_reference_inputs(mods):
    case, top_k = fixture_case()
    e_hip, e_stock, d = gradient_errors(mods, case, 29, want_top=top_k)
    assert_under_bars(e_hip, e_stock, "fixture")
    # (d) rows of d_pred outside top_idx are exactly 0 -- and with 6 nodes every row is selected
    d_pred = d["hip"]["d_pred"].cpu().numpy()
    chosen = np.zeros(len(d_pred), dtype=bool)
    for a, lo in enumerate(d["pred_spans"][:-1]):
        chosen[lo + d["top"][a]] = True
    assert (d_pred[~chosen] == 0).all() and (~chosen).sum() == len(d_pred) - 4 * K
    sizes = np.diff(d["pred_spans"]).tolist()
    assert sorted(sizes) == [6, 7, 64, 160]
    assert (np.abs(d_pred[chosen]).max(1) > 0).all()
    # (e) two runs are bitwise equal
    again = gradient_errors(mods, case, 29)[2]["hip"]
    assert all(torch.equal(again[k], d["hip"][k]) for k in again)


def test_gradients_of_a_decelerating_agent(mods):
    case = synthetic_case()
    e_hip, e_stock, d = gradient_errors(mods, case, 31)
    # the float64 model's speeds: some clamp to 0, none within 1e-3 of it
    dec = d["dec64"]
    j = torch.arange(0, 31, dtype=torch.float64)
    pts = DM.poly(j / 30, dec["coef"].detach())
    length = torch.sqrt(((pts[:, :, 1:] - pts[:, :, :-1]) ** 2).sum(-1)).sum(-1)
    vel = torch.from_numpy(case["agt_vel"]).double().view(-1, 1)
    v = vel.unsqueeze(2) + (2 * (length - vel * 3.0) / 9.0).unsqueeze(2) * (j / 10)
    assert float(v.abs().min()) >= 1e-3, float(v.abs().min())
    assert int((v < 0).sum(-1).min()) >= 1 and int((v > 0).sum(-1).min()) >= 5          # every mode: some steps clamp, some do not
    u = DM.normalise(d["l64"][0].detach() + d["l64"][2].detach()[..., 0])
    two = torch.sort(u, -1)[0][..., -2:]
    assert float((two[..., 1] - two[..., 0]).min()) >= 1e-4
    print("decelerating agent: min |v_j| %.3e, clamped steps per mode %s, top-two gap %.3e"
          % (float(v.abs().min()), (v < 0).sum(-1).tolist(), float((two[..., 1] - two[..., 0]).min())))
    assert_under_bars(e_hip, e_stock, "decelerating")
    # a clamped step passes nothing to pred: d_pred from d_s_samples of the clamped steps alone is exactly 0
    ops = mods[0]
    cu = lambda x: torch.from_numpy(np.ascontiguousarray(x)).cuda()
    g_ss = torch.zeros(1, K, 30)
    g_ss[(v[:, :, 1:] < 0)] = 1.0
    d_pred = ops.goal_decode_bwd(cu(case["pred"]), d["pred_spans"], cu(case["anc_ctrs"]), cu(case["anc_dirs"]),
                                 [lo for lo, _ in case["spans"]], cu(case["agt_ctrs"]), cu(case["dir_last"]), cu(case["agt_vel"]),
                                 cu(d["top"].astype(np.int32)), d_s_samples=g_ss.cuda())
    assert (d_pred == 0).all()


def test_decode_module_trains_on_the_inference_launches(mods, f32):
    _, _, R = mods
    from oracle import lanercnn_oracle as OR
    g, names = DM.fixture()
    seed = int(g["seed"])
    m = decode_module(names, seed).train()
    sub, data, roi_feat = decode_inputs(g)
    rng = np.random.default_rng(23)
    w = [torch.from_numpy(rng.normal(0, 1, s)) for s in ((4, 6), (4, 6, 2), (4, 6, 30, 2))]
    sd = {k: v.requires_grad_(True) for k, v in state(names, "decode", seed, torch.float64).items()}
    a = DM.decode_args(g)
    x64 = torch.from_numpy(g["dec/roi_feat"]).double().requires_grad_(True)
    r = DM.decode_forward(sd, x64, a["spans"], a["anc_ctrs"], a["anc_dirs"], a["agt_ctrs"], a["agt_dirs"], a["agt_trajs"],
                          a["agt_vel"], OR.lane_pooling, top_idx=g["dec/top_k"])
    ((r["logits"] * w[0]).sum() + (r["goals"] * w[1]).sum() + (r["pred_trajs"] * w[2]).sum()).backward()
    with torch.no_grad():
        plain = m.decode(roi_feat, sub, data)
    x = roi_feat.clone().requires_grad_(True)
    m.zero_grad()
    assert R.Decode.train_hip is False
    R.Decode.train_hip = True
    try:
        out = m.decode(x, sub, data)
        assert type(out["pred_trajs"].grad_fn).__name__.startswith("GoalRefineFn")
        assert type(out["goals"].grad_fn).__name__.startswith("GoalDecodeFn")
        wc = [t.float().cuda() for t in w]
        ((out["logits"] * wc[0]).sum() + (out["goals"] * wc[1]).sum() + (out["pred_trajs"] * wc[2]).sum()).backward()
    finally:
        R.Decode.train_hip = False
    assert np.array_equal(out["top_idx"].cpu().numpy(), g["dec/top_k"])
    for k in ("logits", "goals", "pred_trajs", "top_idx", "s_samples"):
        assert torch.equal(out[k], plain[k]), k               # the training forward is the no_grad forward, bit for bit
    worst = {"roi_feat": rel(x.grad, x64.grad)}
    for k, prm in m.named_parameters():
        assert prm.grad is not None, k
        worst[k] = rel(prm.grad, sd[k].grad)
    print("largest relative gradient errors:", sorted(worst.items(), key=lambda kv: -kv[1])[:4])
    assert all(v <= GTOL for v in worst.values()), {k: v for k, v in worst.items() if v > GTOL}
    # with the switch off the stock path runs, as before
    out_off = m.decode(roi_feat.clone().requires_grad_(True), sub, data)
    assert not type(out_off["pred_trajs"].grad_fn).__name__.startswith("GoalRefineFn")
