"""Generates tests/golden/lanercnn_net_b3.npz and lanercnn_net_state_names.json by running the REFERENCE's own
subgraph_gather (lanercnn.py:122-231), graph_gather (:234-277) and Net.forward (:85-119) on three small synthetic scenes
with lane RoIs (lanegcn_amd.data.synth_scene / synth_subgraphs), imported read-only with the shims of
make_golden_decode.py.  Run in the build container only:
    python tests/golden/make_golden_lanercnn_net.py
The fixture holds inputs, the gathered index arrays, the host bookkeeping, the stage captures (input, roi_net1, interactor,
roi_net2, every pooling's hi / wi, the decoder's intermediates) and the three outputs -- data, never reference source;
weights are not stored: both sides regenerate them with oracle.lanercnn_oracle.seeded_state.

The script searches seeds until no comparison hangs on rounding and ASSERTS the margins it prints: every pooling's
min |dist - dist_th| >= 1e-3 and the decoder margins of make_golden_decode.margins_ok."""
import copy
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden_decode as MGD  # noqa: E402  (also puts the repository and tests/ on sys.path)

POOLS = ("roi2graph", "graph2roi", "lane_pool")
DIST_TH = 6.0
REL_KEYS = [("pre", i) for i in range(6)] + [("suc", i) for i in range(6)] + [("left", None), ("right", None)]


def make_scenes(gen, seed):
    """Three scenes with 3 / 2 / 3 RoIs; the second scene's lanes are cut into pieces of 3 nodes so that a short horizon
    gives RoIs of a few nodes; node centres are jittered by 5 cm."""
    rng = np.random.default_rng(seed)
    scenes = [gen.synth_scene(rng, [4, 3], 6), gen.synth_scene(rng, [3], 5), gen.synth_scene(rng, [3, 3], 6)]
    for s in scenes:       # off the 2 m grid of synth_scene, on which RoI and graph nodes lie exactly dist_th = 3 x 2 m apart
        s["graph"]["ctrs"] = (s["graph"]["ctrs"] + rng.normal(0, 0.05, s["graph"]["ctrs"].shape)).astype(np.float32)
    g1 = scenes[1]["graph"]
    g1["lane_idcs"] = (np.arange(g1["num_nodes"]) // 3).astype(np.int64)
    gen.synth_subgraphs(scenes[0], horizon_time=0.5, horizon_buffer=11.0, max_rois=3)
    gen.synth_subgraphs(scenes[1], horizon_time=0.0, horizon_buffer=2.0, max_rois=2)
    gen.synth_subgraphs(scenes[2], horizon_time=0.5, horizon_buffer=4.0, max_rois=3)
    for s in scenes:
        for sg in s["subgraphs"]:
            del sg["node_mask"]                                # not read by the model
    return scenes


def run_net(rl, torch, net, scenes):
    """The reference's Net.forward with its gathers, stages and poolings captured."""
    cap = {"pools": []}
    real_sub, real_graph, real_fwd = rl.subgraph_gather, rl.graph_gather, rl.LanePooling.forward
    real_cat, real_sqrt = torch.cat, torch.sqrt

    def spy_sub(x):
        cap["sub"] = real_sub(x)
        return cap["sub"]

    def spy_graph(x):
        cap["graph"] = real_graph(x)
        return cap["graph"]

    def pool_forward(self, *a, **k):
        # inside LanePooling.forward the only torch.cat calls on int64 tensors are hi and wi (:489-490) and the only
        # torch.sqrt calls are the per-scene distance matrices (:478)
        rec = {"cats": [], "margin": np.inf}

        def spy_cat(tensors, *aa, **kk):
            r = real_cat(tensors, *aa, **kk)
            if r.dtype == torch.int64:
                rec["cats"].append(r.numpy().copy())
            return r

        def spy_sqrt(x, *aa, **kk):
            r = real_sqrt(x, *aa, **kk)
            rec["margin"] = min(rec["margin"], float((r - DIST_TH).abs().min()))
            return r

        torch.cat, torch.sqrt = spy_cat, spy_sqrt
        try:
            out = real_fwd(self, *a, **k)
        finally:
            torch.cat, torch.sqrt = real_cat, real_sqrt
        assert len(rec["cats"]) == 2
        cap["pools"].append({"hi": rec["cats"][0], "wi": rec["cats"][1], "margin": rec["margin"]})
        return out

    hooks, stages = [], {}
    for name in ("input", "roi_net1", "interactor", "roi_net2"):
        hooks.append(getattr(net, name).register_forward_hook(
            lambda m, i, o, name=name: stages.__setitem__(name, o.detach().numpy().copy())))
    rl.subgraph_gather, rl.graph_gather, rl.LanePooling.forward = spy_sub, spy_graph, pool_forward
    try:
        data = rl.collate_fn(copy.deepcopy(scenes))
        with torch.no_grad():
            out = net(data)
    finally:
        rl.subgraph_gather, rl.graph_gather, rl.LanePooling.forward = real_sub, real_graph, real_fwd
        for h in hooks:
            h.remove()
    assert len(cap["pools"]) == 3
    cap["stages"], cap["out"] = stages, {k: v.numpy().copy() for k, v in out.items()}
    return cap


def decode_view(cap, scenes):
    """The decoder's inputs in the layout of make_golden_decode.run_decode, from the reference's gathered RoI graph."""
    sub = cap["sub"]
    n = lambda t: t.numpy().copy()
    return ({"ctrs": [n(c) for c in sub["ctrs"]], "dirs": [n(d) for d in sub["dirs"]],
             "roi_spans": [tuple(s) for s in sub["roi_spans"]], "interest_roi": n(sub["interest_roi"]),
             "agent_vel": [float(v) for v in sub["agent_vel"]]},
            {k: [np.asarray(s[k]) for s in scenes] for k in ("valid_agent_ids", "ctrs", "feats", "obs_trajs")})


def main():
    rl = MGD.import_lanercnn()
    import torch
    import lanegcn_amd  # noqa: F401  (our own generator; the reference only consumes its output)
    from lanegcn_amd import data as gen
    from golden_io import flatten
    from oracle.lanercnn_oracle import seeded_state
    torch.set_num_threads(1)
    net = rl.Net(rl.config).eval()
    shapes = [(k, tuple(v.shape)) for k, v in net.state_dict().items()]
    for seed in range(300, 4000):
        scenes = make_scenes(gen, seed)
        sizes = [[int(sg["num_nodes"]) for sg in s["subgraphs"]] for s in scenes]
        interest = sorted(sz[0] for sz in sizes if sz)
        if [len(sz) for sz in sizes] != [3, 2, 3] or interest[0] != 6 or not 40 <= interest[-1] <= 72:
            continue
        net.load_state_dict(seeded_state(shapes, seed))
        try:
            cap = run_net(rl, torch, net, scenes)
        except RuntimeError as e:                                 # a pooling without a pair
            print("seed %d: %s" % (seed, e))
            continue
        sub, data = decode_view(cap, scenes)
        dcap, m = MGD.run_decode(rl, torch, net.decode, sub, data, cap["stages"]["roi_net2"])
        m["pool_dist"] = [p["margin"] for p in cap["pools"]]
        print("seed %d: RoI sizes %s, margins %s" % (seed, sizes, m))
        if MGD.margins_ok(m) and min(m["pool_dist"]) >= 1e-3:
            break
    assert MGD.margins_ok(m) and min(m["pool_dist"]) >= 1e-3, "no seed in range gives the margins"
    # the decoder run on the captured roi_net2 output is the Net's own decoder run
    assert np.array_equal(dcap["out_logits"], cap["out"]["pred_logics"]) and np.array_equal(dcap["out_trajs"], cap["out"]["pred_trajs"])
    assert np.array_equal(dcap["out_goals"], cap["out"]["pred_goals"])
    rois = [sg for s in scenes for sg in s["subgraphs"]]
    rel = lambda sg, k1, i: sg[k1] if i is None else sg[k1][i]
    assert any(len(rel(sg, k1, i)["u"]) == 0 for sg in rois for k1, i in REL_KEYS), "no RoI has a relation without edges"

    out = {"seed": np.int64(seed), "margins": np.asarray([m["dist"], m["logit_gap"], m["denominator"], m["max_val"]] + m["pool_dist"])}
    flatten(scenes, "scenes/", out)
    sub, graph = cap["sub"], cap["graph"]
    for k in ("num_nodes", "counts", "batch_spans", "num_atgs_per_batch", "roi_spans", "interest_roi"):
        out["sub/host/" + k] = np.asarray(sub[k].numpy() if torch.is_tensor(sub[k]) else sub[k], np.int64)
    out["sub/node_idcs"] = sub["node_idcs"].numpy()
    out["sub/agent_vel"] = np.asarray([float(v) for v in sub["agent_vel"]], np.float64)
    for k in ("feats", "agent_feat", "ctrs", "dirs", "pose"):
        for b, t in enumerate(sub[k]):
            out["sub/%s/%d" % (k, b)] = t.numpy().copy()
    for name, g in (("sub", sub), ("graph", graph)):
        for k1, i in REL_KEYS:
            for k2 in "uv":
                out["%s/%s%s/%s" % (name, k1, "" if i is None else "/%d" % i, k2)] = rel(g, k1, i)[k2].numpy().astype(np.int64)
    out["sub/a2m/u"], out["sub/a2m/v"] = sub["a2m"]["u"].numpy(), sub["a2m"]["v"].numpy()
    out["graph/num_nodes"], out["graph/counts"] = np.asarray(graph["num_nodes"], np.int64), np.asarray(graph["counts"], np.int64)
    for b in range(len(scenes)):
        out["graph/idcs/%d" % b], out["graph/ctrs/%d" % b] = graph["idcs"][b].numpy(), graph["ctrs"][b].numpy()
        out["graph/pose/%d" % b] = graph["pose"][b].numpy()
    for k in ("feats", "turn", "control", "intersect"):
        out["graph/" + k] = graph[k].numpy()
    for name, v in cap["stages"].items():
        out["stage/" + name] = v
    for name, p in zip(POOLS, cap["pools"]):
        out["pool/%s/hi" % name], out["pool/%s/wi" % name] = p["hi"], p["wi"]
    out.update({"out/" + k: v for k, v in cap["out"].items()})
    # the decoder's view in the key layout of lanercnn_decode_b3.npz (decode_model.decode_args reads it)
    out.update({"dec/" + k: v for k, v in dcap.items()})
    out["dec/roi_spans"] = np.asarray(sub["roi_spans"], np.int64)
    out["dec/interest_roi"] = sub["interest_roi"].numpy()
    out["dec/agent_vel"] = out["sub/agent_vel"]
    dsub, ddata = decode_view(cap, scenes)
    for b in range(len(scenes)):
        out["dec/anc_ctrs/%d" % b], out["dec/anc_dirs/%d" % b] = dsub["ctrs"][b], dsub["dirs"][b]
        for k in ddata:
            out["dec/data/%s/%d" % (k, b)] = ddata[k][b]
    names = {"net": [[k, list(s)] for k, s in shapes], "config": sorted(rl.config.keys())}
    with open(os.path.join(HERE, "lanercnn_net_state_names.json"), "w") as f:
        json.dump(names, f)
    path = os.path.join(HERE, "lanercnn_net_b3.npz")
    np.savez_compressed(path, **out)
    assert os.path.getsize(path) < 1000000
    print("wrote lanercnn_net_b3.npz (%d bytes), seed %d, RoI sizes %s, pooling pairs %s, margins %s"
          % (os.path.getsize(path), seed, sizes, [len(p["hi"]) for p in cap["pools"]], m))


if __name__ == "__main__":
    main()
