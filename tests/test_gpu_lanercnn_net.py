"""GPU: the fork model end to end against the reference's own run (tests/golden/lanercnn_net_b3.npz, written by
make_golden_lanercnn_net.py): subgraph_gather and the fork's graph_gather (every index array array_equal, features equal;
numpy, int16, int64 and GPU-resident inputs), Net.forward with LanePooling.fused off and on in the three matrix modes
that claim fp32 parity (pair sets and NMS top-k array_equal, stage captures and pred_logics within FTOL relative,
pred_goals and pred_trajs within the trajectory bar of test_gpu_lanercnn_heads.py, built the same way), and one training
step of Net + Loss with the train_hip switches off and on against a float64 autograd run composed of
oracle.lanercnn_oracle, tests/decode_model.py and tests/roi_loss_model.py with the forward's NMS indices."""
import numpy as np
import pytest
import torch

import decode_model as DM
import lanercnn_net_fixture as NF
import roi_loss_model as RL
from oracle import lanercnn_oracle as OR
from test_gpu_lanercnn_heads import FTOL, GTOL, f32, mma, rel  # noqa: F401  (mma, f32: fixtures)

pytestmark = pytest.mark.gpu
SUB_KEYS = ["num_nodes", "node_idcs", "counts", "batch_spans", "num_atgs_per_batch", "roi_spans", "interest_roi", "feats",
            "agent_feat", "ctrs", "dirs", "pose", "agent_vel", "a2m", "pre", "suc", "left", "right"]
_cache = {}


@pytest.fixture(scope="module")
def mods():
    import lanegcn_amd  # noqa: F401
    from lanegcn_amd import autograd as A
    from lanegcn_amd import data as gen
    from lanegcn_amd import lanercnn as R
    from lanegcn_amd import ops
    from lanegcn_amd.utils import gpu
    return A, gen, R, ops, gpu


def cast_ints(tree, dtype):
    if isinstance(tree, dict):
        return {k: cast_ints(v, dtype) for k, v in tree.items()}
    if isinstance(tree, list):
        return [cast_ints(v, dtype) for v in tree]
    if torch.is_tensor(tree) and not tree.is_floating_point() and tree.dtype != torch.bool:
        return tree.to(dtype)
    return tree


# ------------------------------------------------------------------ gathers
def check_subgraph(got, g):
    assert sorted(got.keys()) == sorted(SUB_KEYS)
    for k in NF.HOST_KEYS:
        v = got[k].tolist() if torch.is_tensor(got[k]) else got[k]
        assert v == NF.host_value(g, k), k
    assert got["node_idcs"].dtype == torch.int64 and np.array_equal(got["node_idcs"].cpu().numpy(), g["sub/node_idcs"])
    for k in ("feats", "agent_feat", "ctrs", "dirs", "pose"):
        assert len(got[k]) == 3
        for b in range(3):
            assert got[k][b].is_cuda and np.array_equal(got[k][b].cpu().numpy(), g["sub/%s/%d" % (k, b)]), (k, b)
    assert np.array_equal(np.asarray([float(v) for v in got["agent_vel"]]), g["sub/agent_vel"])
    for k1, i in NF.REL_KEYS:
        for k2 in "uv":
            x = NF.rel(got, k1, i)[k2]
            assert x.dtype == torch.int64 and x.is_cuda, (k1, i, k2)      # an empty relation too: int64, not the float zeros((0,))
            assert np.array_equal(x.cpu().numpy(), g["sub/%s/%s" % (NF.rel_name(k1, i), k2)]), (k1, i, k2)
    for k2 in "uv":
        assert got["a2m"][k2].dtype == torch.int64 and np.array_equal(got["a2m"][k2].cpu().numpy(), g["sub/a2m/" + k2])


@pytest.mark.parametrize("kind", ["cpu", "numpy", "int16", "int64", "gpu"])
def test_subgraph_gather_vs_reference(mods, kind):
    _, gen, R, _, gpu = mods
    g, _ = NF.fixture()
    assert any(g["sub/%s/u" % NF.rel_name(k1, i)].size == 0 for k1, i in NF.REL_KEYS)
    subs = [s["subgraphs"] for s in NF.scenes()] if kind == "numpy" else gen.collate_fn(NF.scenes())["subgraphs"]
    if kind in ("int16", "int64"):
        subs = cast_ints(subs, getattr(torch, kind))
    if kind == "gpu":
        subs = gpu(subs)
    check_subgraph(R.subgraph_gather(subs), g)


@pytest.mark.parametrize("kind", ["cpu", "int16", "gpu"])
def test_graph_gather_vs_reference(mods, kind):
    _, gen, R, _, gpu = mods
    g, _ = NF.fixture()
    graphs = gen.collate_fn(NF.scenes())["graph"]
    if kind == "int16":
        graphs = cast_ints(graphs, torch.int16)
    if kind == "gpu":
        graphs = gpu(graphs)
    got = R.graph_gather(graphs)
    assert got["num_nodes"] == g["graph/num_nodes"].tolist() and got["counts"] == g["graph/counts"].tolist()
    for b in range(3):
        for k in ("idcs", "ctrs", "pose"):
            assert np.array_equal(got[k][b].cpu().numpy(), g["graph/%s/%d" % (k, b)]), (k, b)
        assert got["pose"][b].is_cuda and got["pose"][b].shape[1] == 4
    for k in ("feats", "turn", "control", "intersect"):
        assert np.array_equal(got[k].cpu().numpy(), g["graph/" + k]), k
    for k1, i in NF.REL_KEYS:
        for k2 in "uv":
            x = NF.rel(got, k1, i)[k2]
            assert x.dtype == torch.int64 and np.array_equal(x.cpu().numpy(), g["graph/%s/%s" % (NF.rel_name(k1, i), k2)])


# ------------------------------------------------------------------ Net.forward
def make_net(R, train=False):
    g, names = NF.fixture()
    net = R.Net(R.config)
    net.load_state_dict(OR.seeded_state([(k, tuple(s)) for k, s in names["net"]], int(g["seed"])), strict=True)
    net.cuda()
    return net.train() if train else net.eval()


def run_captured(R, net, data):
    """net(data) with every pooling's pair set, the stage outputs and the decoder's intermediates recorded."""
    cap = {"pairs": [], "stages": {}}
    real_pairs, real_decode = R.build_pairs, net.decode.decode
    R.build_pairs = lambda *a, **k: cap["pairs"].append(real_pairs(*a, **k)) or cap["pairs"][-1]
    net.decode.decode = lambda *a, **k: cap.__setitem__("dec", real_decode(*a, **k)) or cap["dec"]
    hooks = [getattr(net, n).register_forward_hook(lambda m, i, o, n=n: cap["stages"].__setitem__(n, o.detach()))
             for n in ("input", "roi_net1", "interactor", "roi_net2")]
    try:
        cap["out"] = net(data)
    finally:
        for h in hooks:
            h.remove()
        R.build_pairs = real_pairs
        del net.decode.decode
    return cap


def check_pairs(cap, g):
    """The reference lists a pooling's pairs context-major (hi = context, wi = target); the product target-major."""
    assert len(cap["pairs"]) == 3
    for name, ps in zip(NF.POOLS, cap["pairs"]):
        P = ps.count()
        tgt, ctx = ps.hi[:P].cpu().numpy().astype(np.int64), ps.wi[:P].cpu().numpy().astype(np.int64)
        if name == "lane_pool":      # the product numbers scene b's motion rows 20 b + j, the reference b + j (Decode's docstring)
            ctx = ctx // 20 + ctx % 20
        hi, wi = g["pool/%s/hi" % name], g["pool/%s/wi" % name]
        order = np.lexsort((hi, wi))
        assert P == len(hi), name
        assert np.array_equal(tgt, wi[order]) and np.array_equal(ctx, hi[order]), name


def traj_bars(g):
    """The bar of pred_trajs of test_gpu_lanercnn_heads.py, built the same way from the reference side alone -- 2 x the
    largest change of the float64 restatement's output when pred and traj_delta move by +-FTOL (8 random sign draws) plus
    max(4 x the reference's own distance from the restatement, 1e-6) x max |ref| -- and the same for pred_goals."""
    if "bars" not in _cache:
        a = DM.decode_args(g)
        spans = [0] + [int(v) for v in np.cumsum([hi - lo for lo, hi in a["spans"]])]
        pred64, delta64 = torch.from_numpy(g["dec/pred"]).double(), torch.from_numpy(g["dec/traj_delta"]).double()
        args = (spans, a["anc_ctrs"], a["anc_dirs"], [lo for lo, _ in a["spans"]], a["agt_ctrs"], a["agt_dirs"][:, -1], a["agt_vel"])
        ref = DM.decode(pred64, *args)
        assert np.array_equal(ref["top_idx"], g["dec/top_k"])
        ref["pred_trajs"] = DM.refine(ref["s_samples"], ref["coef"], delta64)
        rng = np.random.default_rng(17)
        change = {"goals": 0.0, "pred_trajs": 0.0}
        for _ in range(8):
            sp = torch.from_numpy(rng.choice([-FTOL, FTOL], tuple(pred64.shape)))
            sd_ = torch.from_numpy(rng.choice([-FTOL, FTOL], tuple(delta64.shape)))
            dec = DM.decode(pred64 + sp, *args, top_idx=g["dec/top_k"])
            moved = {"goals": dec["goals"], "pred_trajs": DM.refine(dec["s_samples"], dec["coef"], delta64 + sd_)}
            for k in change:
                change[k] = max(change[k], float((moved[k] - ref[k]).abs().max()))
        bars = {}
        for k, own in (("goals", g["out/pred_goals"]), ("pred_trajs", g["out/pred_trajs"])):
            entry = max(4 * DM.rel_err(own, ref[k].numpy()), 1e-6) * float(ref[k].abs().max())
            bars[k] = (2 * change[k] + entry, change[k], entry)
        _cache["bars"] = (ref, bars)
    return _cache["bars"]


@pytest.mark.parametrize("fused", [False, True], ids=["composed", "fused"])
def test_net_forward_vs_reference(mods, mma, fused, monkeypatch):  # noqa: F811
    _, gen, R, ops, _ = mods
    g, _ = NF.fixture()
    net = make_net(R)
    data = gen.collate_fn(NF.scenes())
    calls, real = [], ops.pool_pairs
    monkeypatch.setattr(ops, "pool_pairs", lambda *a, **k: calls.append(1) or real(*a, **k))
    R.LanePooling.fused = fused
    try:
        with torch.no_grad():
            cap = run_captured(R, net, data)
    finally:
        R.LanePooling.fused = False
    assert len(calls) == (3 if fused else 0)
    check_pairs(cap, g)
    assert np.array_equal(cap["dec"]["top_idx"].cpu().numpy(), g["dec/top_k"])
    out = cap["out"]
    assert list(out.keys()) == ["pred_logics", "pred_goals", "pred_trajs"]
    errs = {n: rel(cap["stages"][n], torch.from_numpy(g["stage/" + n]).double()) for n in cap["stages"]}
    errs["pred_logics"] = rel(out["pred_logics"], torch.from_numpy(g["out/pred_logics"]).double())
    print("%s fused=%s P=%s relative errors %s" % (mma, fused, [ps.count() for ps in cap["pairs"]],
                                                    {k: "%.2e" % v for k, v in errs.items()}))
    assert all(v <= FTOL for v in errs.values()), errs
    ref, bars = traj_bars(g)
    for k, got in (("goals", out["pred_goals"]), ("pred_trajs", out["pred_trajs"])):
        e = float((got.cpu().double() - ref[k]).abs().max())
        print("%s: max|got - ref64| %.3e, bar %.3e (change %.3e, entry %.3e)" % ((k, e) + bars[k]))
        assert e <= bars[k][0], k


def test_net_takes_a_gpu_resident_batch(mods, f32):  # noqa: F811
    _, gen, R, _, gpu = mods
    net = make_net(R)
    with torch.no_grad():
        a = net(gen.collate_fn(NF.scenes()))
        b = net(gpu(dict(gen.collate_fn(NF.scenes()))))
        c = net(gen.collate_fn(NF.scenes()))
    for k in a:
        assert torch.equal(a[k], b[k]) and torch.equal(a[k], c[k]), k


# ------------------------------------------------------------------ one training step
def forward64(g, sd, top_idx):
    """Net.forward and Loss in float64 on the CPU: the oracle's modules on the reference's own gathered graphs."""
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a))
    rels = lambda name: {**{k1: [{k2: t(g["%s/%s/%d/%s" % (name, k1, i, k2)]) for k2 in "uv"} for i in range(6)] for k1 in ("pre", "suc")},
                         **{k1: {k2: t(g["%s/%s/%s" % (name, k1, k2)]) for k2 in "uv"} for k1 in ("left", "right")}}
    sub = rels("sub")
    sub.update(feats=[t(g["sub/feats/%d" % b]).double() for b in range(3)],
               agent_feat=[t(g["sub/agent_feat/%d" % b]).double() for b in range(3)],
               a2m={"u": t(g["sub/a2m/u"]), "v": t(g["sub/a2m/v"])})
    graph = rels("graph")
    graph["feats"] = t(g["graph/feats"]).double()
    sub_p = {"ctrs": [t(g["sub/ctrs/%d" % b]).double() for b in range(3)], "pose": [t(g["sub/pose/%d" % b]).double() for b in range(3)]}
    graph_p = {"ctrs": [t(g["graph/ctrs/%d" % b]).double() for b in range(3)], "pose": [t(g["graph/pose/%d" % b]).double() for b in range(3)]}
    x = OR.lane_input(sub, sd, "input")
    x = OR.lane_roi(x, sub, sd, "roi_net1")
    gi = DM.stem(torch.cat(graph_p["ctrs"], 0), graph["feats"], sd, "interactor.input", "interactor.seg")
    gf = OR.lane_pooling(x, sub_p, gi, graph_p, sd, "interactor.roi2graph")[0]
    gf = OR.global_graph_net(gf, graph, sd, "interactor.global_graph_net")
    x = OR.lane_pooling(gf, graph_p, x, sub_p, sd, "interactor.graph2roi")[0]
    x = OR.lane_roi(x, sub, sd, "roi_net2")
    a = DM.decode_args(g)
    sd_dec = {k[len("decode."):]: v for k, v in sd.items() if k.startswith("decode.")}
    r = DM.decode_forward(sd_dec, x, a["spans"], a["anc_ctrs"], a["anc_dirs"], a["agt_ctrs"], a["agt_dirs"], a["agt_trajs"],
                          a["agt_vel"], OR.lane_pooling, top_idx=top_idx)
    first = [int(g["dec/data/valid_agent_ids/%d" % b][0]) for b in range(3)]
    gt = torch.stack([t(g["scenes/%d/gt_preds" % b][first[b]]).double() for b in range(3)])
    has = torch.stack([t(g["scenes/%d/has_preds" % b][first[b]]).bool() for b in range(3)])
    loss_out = RL.roi_loss(r["logits"], r["goals"], r["pred_trajs"], gt, has, 1.0)
    return r, RL.total(loss_out)


def reference_step(g, names):
    if "step" not in _cache:
        sd = {k: v.double().requires_grad_(True)
              for k, v in OR.seeded_state([(k, tuple(s)) for k, s in names["net"]], int(g["seed"])).items()}
        r, loss = forward64(g, sd, g["dec/top_k"])
        loss.backward()
        _cache["step"] = (float(loss.detach()), {k: v.grad for k, v in sd.items()}, r)
    return _cache["step"]


@pytest.mark.parametrize("hip", [False, True], ids=["composed", "train_hip"])
def test_training_step_vs_float64_autograd(mods, f32, hip):  # noqa: F811
    A, gen, R, _, _ = mods
    g, names = NF.fixture()
    loss64, grads64, r64 = reference_step(g, names)
    assert float((r64["logits"].detach() - torch.from_numpy(g["out/pred_logics"])).abs().max()) <= FTOL
    net, loss_fn = make_net(R, train=True), R.Loss(R.config).cuda()
    data = gen.collate_fn(NF.scenes())
    prev = (A.RowBlockFn.train_hip, R.Decode.train_hip)
    A.RowBlockFn.train_hip = R.Decode.train_hip = hip
    try:
        cap = run_captured(R, net, data)
        loss_out = loss_fn(cap["out"], data)
        loss_out["loss"].backward()
    finally:
        A.RowBlockFn.train_hip, R.Decode.train_hip = prev
    assert np.array_equal(cap["dec"]["top_idx"].cpu().numpy(), g["dec/top_k"])      # the indices the float64 run used
    loss = float(loss_out["loss"].detach())
    print("train_hip=%s loss %.6f float64 %.6f" % (hip, loss, loss64))
    assert np.isfinite(loss)
    worst = {}
    for k, prm in net.named_parameters():
        assert prm.grad is not None and bool(torch.isfinite(prm.grad).all()), k
        worst[k] = rel(prm.grad, grads64[k])
    print("largest relative gradient errors:", sorted(worst.items(), key=lambda kv: -kv[1])[:4])
    assert all(v <= GTOL for v in worst.values()), {k: v for k, v in worst.items() if v > GTOL}
