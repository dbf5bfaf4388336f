"""Generates tests/golden/hotpath_wide_b4.npz by running the REFERENCE's own MapNet / A2M / M2M / M2A / A2A (imported
read-only with the shims of make_golden.py) in fp32 AND in float64 (net.double(), the batch's floats cast to double) on
the scenes and ActorNet rows of hotpath_b4.npz, at two states of oracle.wide_state (seed 3): the wide one
(e_lo = -8, e_hi = 2) and the uniform one (every matrix of K >= 128 times 2^-8).  Run in the build container only:
    python tests/golden/make_golden_wide.py            (--check: regenerate and compare with the committed file, bit for bit)
The fixture holds the reference's float64 outputs and its own fp32-vs-float64 error (data), never reference source;
weights are not stored: both sides regenerate them with oracle.wide_state.

Per state (prefix "wide/" and "u-8/"):
    m2a, a2a                          float64 [42, 128]
    <stage>/rows8, <stage>/colsum     map_net, a2m, m2m: every 8th row and the float64 column sums
    rel32/<stage>                     max |fp32 run - float64 run| / max |float64 run| of the reference itself
    params                            seed, e_lo, e_hi, g_lo, g_hi, neg (g_lo = nan: GroupNorm parameters as seeded)
pair_margin/<block>: the smallest |distance - threshold| over every (target, context) of a scene, in float64.  The
script ASSERTS that the fp32 and the float64 run used identical pair sets (recorded from torch.cat / index_add_ while the
blocks run, as make_golden.py does)."""
import copy
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden as MG  # noqa: E402  (also puts the repository and tests/ on sys.path)

SEED = 3
STATES = {"wide": dict(e_lo=-8, e_hi=2, g_lo=0.05, g_hi=8.0, neg=0.1), "u-8": dict(e_lo=-8, e_hi=-8, g_lo=None, g_hi=8.0, neg=0.1)}
NODE_STAGES, ACTOR_STAGES = ("map_net", "a2m", "m2m"), ("m2a", "a2a")
OUT = os.path.join(HERE, "hotpath_wide_b4.npz")


def rel_err(got, ref):
    return float(np.abs(got.astype(np.float64) - ref).max() / np.abs(ref).max())


def run_stages(torch, net, graph, actors, actor_idcs, actor_ctrs):
    """The five stages as Net.forward runs them (lanegcn.py:134-141) + the index tensors of every Att block."""
    captured = []
    real_cat, real_index_add = torch.cat, torch.Tensor.index_add_

    def spy_cat(tensors, *a, **k):
        r = real_cat(tensors, *a, **k)
        if r.dtype == torch.int64 and r.dim() == 1:
            captured.append(("cat", r.numpy().copy()))
        return r

    def spy_index_add(self, dim, index, source, *a, **k):
        captured.append(("index_add_", index.numpy().copy()))
        return real_index_add(self, dim, index, source, *a, **k)

    pairs = {}

    def run_block(fn, name):
        del captured[:]
        torch.cat, torch.Tensor.index_add_ = spy_cat, spy_index_add
        try:
            res = fn()
        finally:
            torch.cat, torch.Tensor.index_add_ = real_cat, real_index_add
        cats = [c for kind, c in captured if kind == "cat"]
        adds = [c for kind, c in captured if kind == "index_add_"]
        assert len(cats) == 4 and len(adds) == 2, (name, len(cats), len(adds))         # two Att layers per block
        assert np.array_equal(cats[0], cats[2]) and np.array_equal(cats[1], cats[3]) and np.array_equal(cats[0], adds[0])
        pairs[name] = (cats[0], cats[1])
        return res

    out = {}
    with torch.no_grad():
        nodes, node_idcs, node_ctrs = net.map_net(graph)
        out["map_net"] = nodes.numpy().copy()
        nodes = run_block(lambda: net.a2m(nodes, graph, actors, actor_idcs, actor_ctrs), "a2m")
        out["a2m"] = nodes.numpy().copy()
        nodes = net.m2m(nodes, graph)
        out["m2m"] = nodes.numpy().copy()
        act = run_block(lambda: net.m2a(actors, actor_idcs, actor_ctrs, nodes, node_idcs, node_ctrs), "m2a")
        out["m2a"] = act.numpy().copy()
        act = run_block(lambda: net.a2a(act, actor_idcs, actor_ctrs), "a2a")
        out["a2a"] = act.numpy().copy()
    return out, pairs


def generate():
    import torch
    import lanegcn_amd  # noqa: F401
    from golden_io import load_scenes
    from oracle.lanegcn_oracle import wide_state

    torch.manual_seed(0)
    torch.set_num_threads(1)
    ref, refdata = MG.import_reference()
    with np.load(os.path.join(HERE, "hotpath_b4.npz")) as z:
        flat = {k: z[k] for k in z.files}
    scenes = load_scenes(flat)
    net = ref.Net(ref.config).eval()
    shapes = [(k, tuple(v.shape)) for k, v in net.state_dict().items()]

    def inputs(double):
        batch = refdata.collate_fn(copy.deepcopy(scenes))
        _, actor_idcs = ref.actor_gather(batch["feats"])
        graph = ref.graph_gather(ref.to_long(batch["graph"]))
        actors, actor_ctrs = torch.from_numpy(flat["actors_in"].copy()), batch["ctrs"]
        if double:
            actors, actor_ctrs = actors.double(), [c.double() for c in actor_ctrs]
            graph["ctrs"] = [c.double() for c in graph["ctrs"]]
            for k in ("feats", "turn", "control", "intersect"):
                graph[k] = graph[k].double()
        return graph, actors, actor_idcs, actor_ctrs

    out = {}
    for name, kw in STATES.items():
        sd = wide_state(shapes, SEED, **kw)
        net.float().load_state_dict(sd)
        got32, pairs32 = run_stages(torch, net, *inputs(False))
        net.double()                                                # fp32 values, exactly, in double
        for k, v in net.state_dict().items():
            assert torch.equal(v, sd[k].double()), k
        got64, pairs64 = run_stages(torch, net, *inputs(True))
        for blk in pairs32:       # the float64 run must have decided every pair as the fp32 run (and the kernels) did
            assert np.array_equal(pairs32[blk][0], pairs64[blk][0]) and np.array_equal(pairs32[blk][1], pairs64[blk][1]), blk
        for k in NODE_STAGES:
            assert got64[k].dtype == np.float64
            out["%s/%s/rows8" % (name, k)], out["%s/%s/colsum" % (name, k)] = got64[k][::8].copy(), got64[k].sum(0)
        for k in ACTOR_STAGES:
            assert got64[k].dtype == np.float64
            out["%s/%s" % (name, k)] = got64[k]
        for k in NODE_STAGES + ACTOR_STAGES:
            out["%s/rel32/%s" % (name, k)] = np.float64(rel_err(got32[k], got64[k]))
        out[name + "/params"] = np.array([SEED, kw["e_lo"], kw["e_hi"], np.nan if kw["g_lo"] is None else kw["g_lo"],
                                          kw["g_hi"], kw["neg"]], np.float64)
        print(name, {k: "%.2e" % out["%s/rel32/%s" % (name, k)] for k in NODE_STAGES + ACTOR_STAGES},
              {b: len(p[0]) for b, p in pairs64.items()})

    cfg = ref.config
    node_c, act_c = [s["graph"]["ctrs"].astype(np.float64) for s in scenes], [s["ctrs"].astype(np.float64) for s in scenes]
    for blk, a, c, th in (("a2m", node_c, act_c, cfg["actor2map_dist"]), ("m2a", act_c, node_c, cfg["map2actor_dist"]),
                          ("a2a", act_c, act_c, cfg["actor2actor_dist"])):
        margin = min(float(np.abs(np.sqrt(((x[:, None] - y[None]) ** 2).sum(2)) - th).min()) for x, y in zip(a, c))
        out["pair_margin/" + blk] = np.float64(margin)
        print("pair margin %s: %.3e" % (blk, margin))
        assert margin > 1e-4, blk                                   # far from fp32's rounding of a distance (~1e-6 at 10 m)
    return out


def main(argv):
    out = generate()
    if "--check" in argv:
        with np.load(OUT) as z:
            assert sorted(z.files) == sorted(out), "key sets differ"
            for k in z.files:
                assert z[k].dtype == out[k].dtype and z[k].shape == out[k].shape and z[k].tobytes() == out[k].tobytes(), k
        print("hotpath_wide_b4.npz regenerates bit for bit (%d arrays)" % len(out))
        return 0
    np.savez_compressed(OUT, **out)
    print("wrote hotpath_wide_b4.npz: %d bytes" % os.path.getsize(OUT))
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
