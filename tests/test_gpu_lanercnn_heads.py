"""GPU: Interactor and Decode of the fork model (lanegcn_amd.lanercnn) against the reference's captures
(tests/golden/lanercnn_decode_b3.npz): module stages in every matrix mode that claims fp32 parity, the whole
Decode.forward, and gradients against CPU float64 autograd of the restatement (tests/decode_model.py)."""
import numpy as np
import pytest
import torch

import decode_model as DM
from conftest import to_torch_scene
from golden_io import load_scenes
from oracle import lanegcn_oracle as O
from oracle import lanercnn_oracle as OR

pytestmark = pytest.mark.gpu
FTOL = 1e-4            # the bar of test_lanercnn.py
GTOL = 2e-4            # its gradient bar


def err(got, want):
    return float((got.detach().cpu() - torch.from_numpy(np.ascontiguousarray(want))).abs().max())


def rel(a, b):
    return float((a.detach().cpu().double() - b).abs().max()) / max(1e-6, float(b.abs().max()))


def state(names, key, seed, dtype=torch.float32):
    return {k: v.to(dtype) for k, v in OR.seeded_state([(k, tuple(s)) for k, s in names[key]], seed).items()}


def decode_module(names, seed):
    import lanegcn_amd  # noqa: F401
    from lanegcn_amd import lanegcn as M
    from lanegcn_amd import lanercnn as R
    m = R.Decode(M.config)
    m.load_state_dict(state(names, "decode", seed), strict=True)
    return m.cuda().eval()


def decode_inputs(g, device="cuda"):
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(device)
    n = len(g["dec/interest_roi"])
    sub = {"ctrs": [t(g["dec/anc_ctrs/%d" % b]) for b in range(n)], "dirs": [t(g["dec/anc_dirs/%d" % b]) for b in range(n)],
           "roi_spans": [tuple(int(v) for v in s) for s in g["dec/roi_spans"]],
           "interest_roi": torch.from_numpy(g["dec/interest_roi"]), "agent_vel": [float(v) for v in g["dec/agent_vel"]]}
    data = {k: [t(g["dec/data/%s/%d" % (k, b)]) for b in range(n)] for k in ("valid_agent_ids", "ctrs", "feats", "obs_trajs")}
    return sub, data, t(g["dec/roi_feat"])


def interactor_inputs(g, device="cuda"):
    import lanegcn_amd  # noqa: F401
    from lanegcn_amd import lanegcn as M
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(device)
    scenes = [to_torch_scene(s) for s in load_scenes(g, "ia/scenes")]
    graphs = [s["graph"] for s in scenes]
    pose = [torch.cat([gr["ctrs"].float(), gr["feats"].float()], 1) for gr in graphs]
    if device == "cuda":
        graph = M.graph_gather(graphs)
        graph["ctrs"] = [c.float().cuda() for c in graph["ctrs"]]
    else:
        graph = O.graph_gather(graphs)
    graph["pose"] = [p.to(device) for p in pose]
    sub = {"ctrs": [t(g["ia/roi_ctrs/%d" % i]) for i in range(3)], "pose": [t(g["ia/roi_pose/%d" % i]) for i in range(3)]}
    return graph, sub, t(g["ia/roi_feat"])


@pytest.fixture(params=["f32", "bf16x3", "f16x2"])
def mma(request):
    import lanegcn_amd  # noqa: F401
    from lanegcn_amd import ops
    prev = ops.get_mma()
    ops.set_mma(request.param)
    yield request.param
    ops.set_mma(prev)


@pytest.fixture
def f32():
    import lanegcn_amd  # noqa: F401
    from lanegcn_amd import ops
    prev = ops.get_mma()
    ops.set_mma("f32")
    yield
    ops.set_mma(prev)


def test_module_stages_vs_reference_captures(mma):
    g, names = DM.fixture()
    seed = int(g["seed"])
    m = decode_module(names, seed)
    sub, data, roi_feat = decode_inputs(g)
    a = DM.decode_args(g, torch.float32, "cuda")
    spans = a["spans"]
    with torch.no_grad():
        feats = torch.cat([roi_feat[lo:hi] for lo, hi in spans], 0)
        assert err(m.pred(feats), g["dec/pred"]) <= FTOL
        # the refinement head fed the reference's pooled rows
        pooled = torch.from_numpy(g["dec/pooled"]).cuda()
        base = np.cumsum([0] + [hi - lo for lo, hi in spans])[:-1]
        rows = torch.from_numpy((g["dec/top_k"] + base[:, None]).reshape(-1)).cuda()
        assert err(m.refinement(pooled[rows]).view(-1, 6, 30, 2), g["dec/traj_delta"]) <= FTOL
        # the whole forward's pooled features: the reference's row numbering of the motion graph included
        out = m.decode(roi_feat, sub, data)
        assert err(out["pooled"], g["dec/pooled"]) <= FTOL
        assert err(out["pred"], g["dec/pred"]) <= FTOL
        assert err(out["traj_delta"], g["dec/traj_delta"]) <= 2 * FTOL           # pooled (FTOL) through one more head
    # Interactor
    from lanegcn_amd import lanegcn as M
    from lanegcn_amd import lanercnn as R
    ia = R.Interactor(M.config)
    ia.load_state_dict(state(names, "interactor", seed + 1), strict=True)
    ia.cuda().eval()
    graph, isub, iroi = interactor_inputs(g)
    keep = iroi.clone()
    with torch.no_grad():
        assert err(ia.graph_input(graph), g["ia/graph_input"]) <= FTOL
        assert err(ia(graph, isub, iroi), g["ia/out"]) <= FTOL
    assert torch.equal(iroi, keep)


def test_decode_forward_vs_reference(f32):
    g, names = DM.fixture()
    m = decode_module(names, int(g["seed"]))
    sub, data, roi_feat = decode_inputs(g)
    keep = [roi_feat.clone()] + [c.clone() for c in sub["ctrs"]] + [x.clone() for v in data.values() for x in v]
    with torch.no_grad():
        out = m.decode(roi_feat, sub, data)
        logits, goals, trajs = m(roi_feat, sub, data)
    assert np.array_equal(out["top_idx"].cpu().numpy(), g["dec/top_k"])
    assert err(logits, g["dec/out_logits"]) <= FTOL and err(goals, g["dec/out_goals"]) <= FTOL
    # bar of pred_trajs, from the reference side alone: 2 x the largest change of the restatement's output when pred and
    # traj_delta move by +-FTOL (8 random sign draws), plus the entry-level bar of test_gpu_goal_decode.py
    ref = DM.reference64()
    a = DM.decode_args(g)
    pred_spans = [0] + [int(v) for v in np.cumsum([hi - lo for lo, hi in a["spans"]])]
    pred64, delta64 = torch.from_numpy(g["dec/pred"]).double(), torch.from_numpy(g["dec/traj_delta"]).double()
    rng = np.random.default_rng(17)
    change = 0.0
    for _ in range(8):
        sp = torch.from_numpy(rng.choice([-FTOL, FTOL], tuple(pred64.shape)))
        sd_ = torch.from_numpy(rng.choice([-FTOL, FTOL], tuple(delta64.shape)))
        dec = DM.decode(pred64 + sp, pred_spans, a["anc_ctrs"], a["anc_dirs"], [lo for lo, _ in a["spans"]], a["agt_ctrs"],
                        a["agt_dirs"][:, -1], a["agt_vel"], top_idx=g["dec/top_k"])
        moved = DM.refine(dec["s_samples"], dec["coef"], delta64 + sd_)
        change = max(change, float((moved - ref["pred_trajs"]).abs().max()))
    entry = max(4 * DM.rel_err(g["dec/out_trajs"], ref["pred_trajs"].numpy()), 1e-6) * float(ref["pred_trajs"].abs().max())
    bar = 2 * change + entry
    e = float((trajs.cpu().double() - ref["pred_trajs"]).abs().max())
    print("pred_trajs: max|got - ref64| %.3e, bar %.3e (change %.3e, entry %.3e)" % (e, bar, change, entry))
    assert e <= bar
    # two runs are bitwise equal; the inputs are unmodified
    with torch.no_grad():
        again = m(roi_feat, sub, data)
    assert all(torch.equal(x, y) for x, y in zip(again, (logits, goals, trajs)))
    now = [roi_feat] + list(sub["ctrs"]) + [x for v in data.values() for x in v]
    assert all(torch.equal(x, y) for x, y in zip(now, keep))


def test_decode_gradients_vs_float64_autograd(f32):
    g, names = DM.fixture()
    seed = int(g["seed"])
    m = decode_module(names, seed).train()
    sub, data, roi_feat = decode_inputs(g)
    rng = np.random.default_rng(23)
    w = [torch.from_numpy(rng.normal(0, 1, s)) for s in ((4, 6), (4, 6, 2), (4, 6, 30, 2))]
    # reference: CPU float64 autograd of the restatement with the same indices
    sd = {k: v.requires_grad_(True) for k, v in state(names, "decode", seed, torch.float64).items()}
    a = DM.decode_args(g)
    x64 = torch.from_numpy(g["dec/roi_feat"]).double().requires_grad_(True)
    r = DM.decode_forward(sd, x64, a["spans"], a["anc_ctrs"], a["anc_dirs"], a["agt_ctrs"], a["agt_dirs"], a["agt_trajs"],
                          a["agt_vel"], OR.lane_pooling, top_idx=g["dec/top_k"])
    ((r["logits"] * w[0]).sum() + (r["goals"] * w[1]).sum() + (r["pred_trajs"] * w[2]).sum()).backward()
    x = roi_feat.clone().requires_grad_(True)
    m.zero_grad()
    out = m.decode(x, sub, data)
    assert np.array_equal(out["top_idx"].cpu().numpy(), g["dec/top_k"])
    assert err(out["logits"], g["dec/out_logits"]) <= FTOL and err(out["goals"], g["dec/out_goals"]) <= FTOL
    wc = [t.float().cuda() for t in w]
    ((out["logits"] * wc[0]).sum() + (out["goals"] * wc[1]).sum() + (out["pred_trajs"] * wc[2]).sum()).backward()
    worst = {"roi_feat": rel(x.grad, x64.grad)}
    for k, prm in m.named_parameters():
        assert prm.grad is not None, k
        worst[k] = rel(prm.grad, sd[k].grad)
    print("largest relative gradient errors:", sorted(worst.items(), key=lambda kv: -kv[1])[:4])
    assert all(v <= GTOL for v in worst.values()), {k: v for k, v in worst.items() if v > GTOL}


def test_interactor_gradients_vs_float64_autograd(f32):
    g, names = DM.fixture()
    seed = int(g["seed"]) + 1
    import lanegcn_amd  # noqa: F401
    from lanegcn_amd import lanegcn as M
    from lanegcn_amd import lanercnn as R
    ia = R.Interactor(M.config)
    ia.load_state_dict(state(names, "interactor", seed), strict=True)
    ia.cuda().train()
    w = torch.from_numpy(np.random.default_rng(29).normal(0, 1, g["ia/out"].shape))
    # reference: the oracle's lane_pooling and global_graph_net composed in float64 on the CPU
    sd = {k: v.requires_grad_(True) for k, v in state(names, "interactor", seed, torch.float64).items()}
    graph, sub, roi = interactor_inputs(g, "cpu")
    f64 = lambda d: {"ctrs": [c.double() for c in d["ctrs"]], "pose": [p.double() for p in d["pose"]]}
    x64 = roi.double().requires_grad_(True)
    gi = DM.stem(torch.cat(graph["ctrs"], 0).double(), graph["feats"].double(), sd, "input", "seg")
    gf = OR.lane_pooling(x64, f64(sub), gi, f64(graph), sd, "roi2graph")[0]
    gf = OR.global_graph_net(gf, graph, sd, "global_graph_net")
    out64 = OR.lane_pooling(gf, f64(graph), x64, f64(sub), sd, "graph2roi")[0]
    assert float((out64.detach() - torch.from_numpy(g["ia/out"])).abs().max()) <= 1e-4
    (out64 * w).sum().backward()
    graph_d, sub_d, roi_d = interactor_inputs(g)
    x = roi_d.clone().requires_grad_(True)
    ia.zero_grad()
    out = ia(graph_d, sub_d, x)
    assert err(out, g["ia/out"]) <= FTOL
    (out * w.float().cuda()).sum().backward()
    worst = {"roi_feat": rel(x.grad, x64.grad)}
    for k, prm in ia.named_parameters():
        assert prm.grad is not None, k
        worst[k] = rel(prm.grad, sd[k].grad)
    print("largest relative gradient errors:", sorted(worst.items(), key=lambda kv: -kv[1])[:4])
    assert all(v <= GTOL for v in worst.values()), {k: v for k, v in worst.items() if v > GTOL}
