"""GPU: the HIP hot path (through the C ABI / ctypes) against the oracle and the reference captures.

Bars: index work bit-exact; fp32 features max|delta| <= 1e-4 (BASELINE.json north_star)."""
import numpy as np
import pytest
import torch

from conftest import to_torch_scene
from golden_io import load_scenes
from oracle import lanegcn_oracle as O

pytestmark = pytest.mark.gpu
FTOL = 1e-4


@pytest.fixture(scope="module")
def hip():
    import lanegcn_amd  # noqa: F401
    from lanegcn_amd import lanegcn as M
    from lanegcn_amd import ops
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return M, ops


@pytest.fixture(autouse=True, params=["f32", "bf16x3", "f16x2"])
def mma_mode(request, hip):
    """Every test runs on all matrix-core modes that claim fp32 parity: the exact f32 MFMA chain, the
    3-way bf16 split (6 products) and the 2-way fp16 split (3 products).  Same 1e-4 bar for all."""
    _, ops = hip
    prev = ops.get_mma()
    ops.set_mma(request.param)
    yield request.param
    ops.set_mma(prev)


def make_modules(M, sd, device="cuda"):
    mods = {}
    for name, cls in (("map_net", M.MapNet), ("a2m", M.A2M), ("m2m", M.M2M), ("m2a", M.M2A), ("a2a", M.A2A)):
        m = cls(M.config)
        sub = {k[len(name) + 1:]: v for k, v in sd.items() if k.startswith(name + ".")}
        m.load_state_dict(sub, strict=True)
        mods[name] = m.to(device).eval()
    return mods


def run_hot_path(M, mods, scenes, actors):
    """Device forward of the five stages; returns dict of CPU numpy outputs + the graph dict."""
    with torch.no_grad():
        graph = M.graph_gather([s["graph"] for s in scenes])
        actor_ctrs = [s["ctrs"].cuda() for s in scenes]
        sizes = [len(c) for c in actor_ctrs]
        actor_idcs, st = [], 0
        for n in sizes:
            actor_idcs.append(torch.arange(st, st + n, device="cuda"))
            st += n
        actors = actors.cuda()
        out = {}
        nodes, node_idcs, node_ctrs = mods["map_net"](graph)
        out["map_net"] = nodes
        nodes = mods["a2m"](nodes, graph, actors, actor_idcs, actor_ctrs)
        out["a2m"] = nodes
        nodes = mods["m2m"](nodes, graph)
        out["m2m"] = nodes
        act = mods["m2a"](actors, actor_idcs, actor_ctrs, nodes, node_idcs, node_ctrs)
        out["m2a"] = act
        act = mods["a2a"](act, actor_idcs, actor_ctrs)
        out["a2a"] = act
        torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in out.items()}, graph


@pytest.fixture(scope="module")
def gcase(golden, ref_state_names, hip):
    M, _ = hip
    scenes = [to_torch_scene(s) for s in load_scenes(golden)]
    sd = O.seeded_state(ref_state_names, int(golden["seed"]))
    return scenes, sd, make_modules(M, sd)


def test_graph_gather_bit_exact(gcase, golden, hip):
    M, _ = hip
    scenes, _, _ = gcase
    graph = M.graph_gather([s["graph"] for s in scenes])
    for k1 in ("pre", "suc"):
        for i in range(6):
            for k2 in ("u", "v"):
                got = graph[k1][i][k2]
                assert got.dtype == torch.int64
                assert np.array_equal(got.cpu().numpy(), golden["gg/%s/%d/%s" % (k1, i, k2)])
    for k1 in ("left", "right"):
        for k2 in ("u", "v"):
            assert np.array_equal(graph[k1][k2].cpu().numpy(), golden["gg/%s/%s" % (k1, k2)])
    assert [len(x) for x in graph["idcs"]] == [s["graph"]["num_nodes"] for s in scenes]


def test_graph_gather_int16_and_gpu_inputs(gcase, golden, hip):
    """int16 on-disk indices (preprocess_data.py:230-238) through to_long, and scenes already on the GPU."""
    M, _ = hip
    from lanegcn_amd.utils import gpu, to_long
    scenes, _, _ = gcase

    def cast16(g):
        g = dict(g)
        for k1 in ("pre", "suc"):
            g[k1] = [{k: v.to(torch.int16) for k, v in d.items()} for d in g[k1]]
        for k1 in ("left", "right"):
            g[k1] = {k: v.to(torch.int16) for k, v in g[k1].items()}
        return g

    graph = M.graph_gather(to_long(gpu([cast16(s["graph"]) for s in scenes])))
    assert np.array_equal(graph["pre"][3]["u"].cpu().numpy(), golden["gg/pre/3/u"])
    assert np.array_equal(graph["right"]["v"].cpu().numpy(), golden["gg/right/v"])


def expand_plan(plan):
    """CSR plan -> sorted list of (relation, u, v)."""
    rp = plan.rowptr.cpu().numpy().astype(np.int64)
    col = plan.col.cpu().numpy()
    out = []
    n_sub = (plan.n_nodes + 15) // 16
    for t in range(n_sub):
        for r in range(plan.n_rel):
            for j in range(16):
                k = (t * plan.n_rel + r) * 16 + j
                for e in range(rp[k], rp[k + 1]):
                    out.append((r, t * 16 + j, int(col[e])))
    return sorted(out)


def test_csr_plan_is_the_coo_multiset(gcase, hip):
    M, _ = hip
    scenes, _, _ = gcase
    graph = M.graph_gather([s["graph"] for s in scenes])
    plan = M.lane_plan(graph)
    want = []
    r = 0
    for i in range(6):
        for k1 in ("pre", "suc"):
            u, v = graph[k1][i]["u"].cpu().numpy(), graph[k1][i]["v"].cpu().numpy()
            want += [(r, int(a), int(b)) for a, b in zip(u, v)]
            r += 1
    for k1 in ("left", "right"):
        u, v = graph[k1]["u"].cpu().numpy(), graph[k1]["v"].cpu().numpy()
        want += [(r, int(a), int(b)) for a, b in zip(u, v)]
        r += 1
    assert expand_plan(plan) == sorted(want)
    rp = plan.rowptr.cpu().numpy()
    assert rp[0] == 0 and rp[-1] == len(want) and np.all(np.diff(rp) >= 0)


def test_csr_duplicates_and_unsorted_edges(hip):
    _, ops = hip
    rng = np.random.default_rng(5)
    n = 77
    us = [torch.from_numpy(rng.integers(0, n, m)).cuda() for m in (0, 40, 300)]
    vs = [torch.from_numpy(rng.integers(0, n, m)).cuda() for m in (0, 40, 300)]
    plan = ops.csr_build(us, vs, n)
    want = sorted((r, int(a), int(b)) for r in range(3) for a, b in zip(us[r].cpu().numpy(), vs[r].cpu().numpy()))
    assert expand_plan(plan) == want


def test_pairs_bit_exact_vs_reference(gcase, golden, hip):
    M, _ = hip
    scenes, _, _ = gcase
    graph = M.graph_gather([s["graph"] for s in scenes])
    actor_ctrs = [s["ctrs"].cuda() for s in scenes]
    actor_idcs = [torch.arange(len(c)) for c in actor_ctrs]
    cases = {"a2m": (graph["idcs"], graph["ctrs"], actor_idcs, actor_ctrs, 7.0),
             "m2a": (actor_idcs, actor_ctrs, graph["idcs"], graph["ctrs"], 6.0),
             "a2a": (actor_idcs, actor_ctrs, actor_idcs, actor_ctrs, 100.0)}
    for name, (ai, ac, ci, cc, th) in cases.items():
        ps = M.build_pairs(ai, ac, ci, cc, th)
        hi, wi = ps.hi_wi_long()
        assert hi.dtype == torch.int64
        assert np.array_equal(hi.cpu().numpy(), golden["pairs/%s/hi" % name]), name
        assert np.array_equal(wi.cpu().numpy(), golden["pairs/%s/wi" % name]), name
        # rowptr = segments of index_add_(0, hi, .)
        rp = ps.rowptr.cpu().numpy()
        want = np.searchsorted(golden["pairs/%s/hi" % name], np.arange(len(rp)), side="left")
        assert np.array_equal(rp, want), name


def test_pairs_threshold_boundary_and_modes(hip):
    """Integer-grid centres put many distances exactly ON the threshold (3-4-5 triangles): the fp32
    no-FMA evaluation must agree with the oracle pair for pair, in legacy and fixed offset modes."""
    M, _ = hip
    rng = np.random.default_rng(9)
    agt = [torch.from_numpy(rng.integers(-6, 7, (n, 2)).astype(np.float32)) for n in (70, 3, 130, 1)]
    ctx = [torch.from_numpy(rng.integers(-6, 7, (n, 2)).astype(np.float32)) for n in (65, 4, 200, 2)]
    ctx[1] = ctx[1] + 500.0   # scene 1 without pairs
    ai = [torch.arange(len(a)) for a in agt]
    ci = [torch.arange(len(c)) for c in ctx]
    for legacy in (True, False):
        hi_o, wi_o = O.pair_search(agt, ctx, 5.0, legacy)
        ps = M.build_pairs(ai, [a.cuda() for a in agt], ci, [c.cuda() for c in ctx], 5.0, legacy)
        hi, wi = ps.hi_wi_long()
        assert np.array_equal(hi.cpu().numpy(), hi_o) and np.array_equal(wi.cpu().numpy(), wi_o)
    # random real-valued centres, non-representable threshold
    agt = [torch.from_numpy(rng.normal(0, 4, (n, 2)).astype(np.float32)) for n in (257, 64)]
    ctx = [torch.from_numpy(rng.normal(0, 4, (n, 2)).astype(np.float32)) for n in (300, 129)]
    hi_o, wi_o = O.pair_search(agt, ctx, 0.1 * 37)
    ps = M.build_pairs([torch.arange(len(a)) for a in agt], [a.cuda() for a in agt],
                       [torch.arange(len(c)) for c in ctx], [c.cuda() for c in ctx], 0.1 * 37)
    hi, wi = ps.hi_wi_long()
    assert np.array_equal(hi.cpu().numpy(), hi_o) and np.array_equal(wi.cpu().numpy(), wi_o)


def test_stages_vs_reference_captures(gcase, golden, hip):
    M, _ = hip
    scenes, _, mods = gcase
    out, _ = run_hot_path(M, mods, scenes, torch.from_numpy(golden["actors_in"]))
    for k in ("map_net", "a2m", "m2m", "m2a", "a2a"):
        err = float(np.abs(out[k] - golden[k]).max())
        assert np.isfinite(out[k]).all() and err <= FTOL, (k, err)


def test_each_stage_from_reference_inputs(gcase, golden, hip):
    """Stage-by-stage: every module fed with the REFERENCE's input for that stage (no error carry-over)."""
    M, _ = hip
    scenes, _, mods = gcase
    with torch.no_grad():
        graph = M.graph_gather([s["graph"] for s in scenes])
        actor_ctrs = [s["ctrs"].cuda() for s in scenes]
        actor_idcs = [torch.arange(len(c), device="cuda") for c in actor_ctrs]
        actors = torch.from_numpy(golden["actors_in"]).cuda()
        g = lambda k: torch.from_numpy(golden[k]).cuda()
        got = {
            "a2m": mods["a2m"](g("map_net"), graph, actors, actor_idcs, actor_ctrs),
            "m2m": mods["m2m"](g("a2m"), graph),
            "m2a": mods["m2a"](actors, actor_idcs, actor_ctrs, g("m2m"), graph["idcs"], graph["ctrs"]),
            "a2a": mods["a2a"](g("m2a"), actor_idcs, actor_ctrs),
        }
    for k, v in got.items():
        err = float(np.abs(v.cpu().numpy() - golden[k]).max())
        assert err <= FTOL, (k, err)


def test_att_empty_context_branch(gcase, golden, hip):
    M, _ = hip
    scenes, _, mods = gcase
    with torch.no_grad():
        graph = M.graph_gather([s["graph"] for s in scenes])
        nodes = torch.from_numpy(golden["map_net"]).cuda()
        out = mods["a2m"].att[0](nodes, graph["idcs"], graph["ctrs"], torch.zeros(0, 128, device="cuda"), [], [], 7.0)
    assert float(np.abs(out.cpu().numpy() - golden["att_empty_ctx"]).max()) <= FTOL


def test_error_behaviour_matches_reference(gcase, hip):
    M, _ = hip
    scenes, sd, mods = gcase
    from lanegcn_amd import data as gen
    with torch.no_grad():
        # all scenes pair-less -> RuntimeError like torch.cat([]) (lanegcn.py:688)
        graph = M.graph_gather([s["graph"] for s in scenes])
        far = [s["ctrs"].cuda() + 1.0e4 for s in scenes]
        idcs = [torch.arange(len(c)) for c in far]
        nodes = torch.zeros(sum(len(x) for x in graph["idcs"]), 128, device="cuda")
        with pytest.raises(RuntimeError):
            mods["a2m"].att[0](nodes, graph["idcs"], graph["ctrs"], torch.zeros(sum(len(c) for c in far), 128, device="cuda"),
                               idcs, far, 7.0)
        # chains shorter than 33 nodes -> KeyError (lanegcn.py:312-322)
        short = to_torch_scene(gen.synth_scene(np.random.default_rng(0), [2], 3))
        with pytest.raises(KeyError):
            mods["map_net"](M.graph_gather([short["graph"]]))
    # CPU tensors are refused: there is no CPU fallback
    from lanegcn_amd._lib import LgcnError
    with pytest.raises(LgcnError):
        mods["m2m"].cpu()(torch.zeros(4, 128), {})
    mods["m2m"].cuda()
    # one rowptr per launch: CSR and RANGE relations cannot be mixed (LGCN_EINVAL from the C ABI)
    from lanegcn_amd import _lib as L
    from lanegcn_amd import ops
    x = torch.zeros(16, 128, device="cuda")
    w = ops.packed(mods["m2m"].fuse["ctr"][0].weight)
    rp = torch.zeros(64, dtype=torch.int32, device="cuda")
    with pytest.raises(LgcnError):
        ops.agg_mlp(16, [ops.RelSpec(x, w, L.REL_CSR, 0), ops.RelSpec(x, w, L.REL_RANGE)], 0, rowptr=rp, col=rp, n_rel_csr=1)


def test_s2_batch_vs_oracle_and_properties(hip, ref_state_names):
    """BASELINE size (32 scenes, 10,368 nodes, 1,600 actors): HIP vs oracle within 1e-4, bitwise
    run-to-run repeatability, and scene-order equivariance (scenes are independent graphs)."""
    M, _ = hip
    from lanegcn_amd import data as gen
    sd = O.seeded_state(ref_state_names, 3)
    mods = make_modules(M, sd)
    scenes_np = gen.synth_batch("S2", seed=1)
    scenes = [to_torch_scene(s) for s in scenes_np]
    A = sum(len(s["ctrs"]) for s in scenes)
    actors = torch.from_numpy(np.random.default_rng(2).normal(0, 1, (A, 128)).astype(np.float32)).relu()
    out, graph = run_hot_path(M, mods, scenes, actors)
    assert out["map_net"].shape == (10368, 128) and out["a2a"].shape == (1600, 128)

    torch.set_num_threads(max(1, (torch.get_num_threads())))
    want = O.hot_path(O.graph_gather([s["graph"] for s in scenes]), actors, [s["ctrs"] for s in scenes], sd)
    for k in ("map_net", "a2m", "m2m", "m2a", "a2a"):
        err = float(np.abs(out[k] - want[k].numpy()).max())
        assert err <= FTOL, (k, err)

    out2, _ = run_hot_path(M, mods, scenes, actors)
    for k in out:
        assert np.array_equal(out[k], out2[k]), "not bitwise repeatable: " + k

    # reverse the scene order: per-scene outputs must come back identical
    rev = scenes[::-1]
    a_rev = torch.cat([actors[50 * i:50 * (i + 1)] for i in range(31, -1, -1)])
    out_r, _ = run_hot_path(M, mods, rev, a_rev)
    for i in (0, 7, 31):
        j = 31 - i
        assert np.allclose(out["m2m"][324 * i:324 * (i + 1)], out_r["m2m"][324 * j:324 * (j + 1)], atol=2e-5)
        assert np.allclose(out["a2a"][50 * i:50 * (i + 1)], out_r["a2a"][50 * j:50 * (j + 1)], atol=2e-5)


def test_ragged_tail_tile(hip, ref_state_names):
    """Node / actor counts that are not multiples of the 32-row tile, single scene."""
    M, _ = hip
    from lanegcn_amd import data as gen
    sd = O.seeded_state(ref_state_names, 5)
    mods = make_modules(M, sd)
    sc = to_torch_scene(gen.synth_scene(np.random.default_rng(4), [5, 4], 7))   # 162 nodes, 7 actors
    actors = torch.from_numpy(np.random.default_rng(6).normal(0, 1, (7, 128)).astype(np.float32))
    out, _ = run_hot_path(M, mods, [sc], actors)
    want = O.hot_path(O.graph_gather([sc["graph"]]), actors, [sc["ctrs"]], sd)
    for k in out:
        assert float(np.abs(out[k] - want[k].numpy()).max()) <= FTOL, k


def test_full_net_forward_vs_reference(golden, ref_state_names, hip):
    """Drop-in Net.forward(data) on the reference's batch format: cls / reg against the reference's own
    output (ActorNet / PredNet are stock ATen; the hot path in between is HIP)."""
    M, _ = hip
    from lanegcn_amd import data as gen
    scenes = load_scenes(golden)
    net = M.Net(M.config)
    net.load_state_dict(O.seeded_state(ref_state_names, int(golden["seed"])), strict=True)
    net = net.cuda().eval()
    batch = gen.collate_fn(scenes)
    with torch.no_grad():
        out = net(batch)
    assert sorted(out.keys()) == ["cls", "reg"]
    for i in range(len(scenes)):
        cls, reg = out["cls"][i].cpu().numpy(), out["reg"][i].cpu().numpy()
        assert cls.shape == golden["net/cls/%d" % i].shape and reg.shape == golden["net/reg/%d" % i].shape
        assert float(np.abs(cls - golden["net/cls/%d" % i]).max()) <= 2e-4, i
        # reg carries world coordinates up to ~1e3 m (scene 1 is offset by 1000 m): fp32 ulp there is 6e-5
        assert np.allclose(reg, golden["net/reg/%d" % i], rtol=1e-6, atol=5e-4), i


def test_bf16_single_product_mode(gcase, golden, hip):
    """BASELINE config "bf16" (one bf16 product, fp32 accumulate / GN): no fp32 parity claim; over the whole
    16-layer path the features stay within 2e-2 relative (Frobenius) / 0.2 absolute of the reference
    (SURVEY.md hard part 6 suggests 2e-2 relative)."""
    M, ops = hip
    scenes, _, mods = gcase
    prev = ops.get_mma()
    ops.set_mma("bf16")
    try:
        out, _ = run_hot_path(M, mods, scenes, torch.from_numpy(golden["actors_in"]))
    finally:
        ops.set_mma(prev)
    for k in ("map_net", "a2m", "m2m", "m2a", "a2a"):
        err = float(np.abs(out[k] - golden[k]).max())
        rel = float(np.linalg.norm(out[k] - golden[k]) / np.linalg.norm(golden[k]))
        assert np.isfinite(out[k]).all() and 1e-5 < err <= 0.2 and rel <= 2e-2, (k, err, rel)


def test_tile_heights_agree(hip, ref_state_names):
    """Every tile height (16/32/48/64 rows) of the split-bf16 LaneConv kernel gives the same layer output
    (same per-row arithmetic; only the work decomposition changes)."""
    M, ops = hip
    if ops.get_mma() == "f32":
        pytest.skip("tile height is a split-bf16 kernel parameter")
    from lanegcn_amd import data as gen
    sd = O.seeded_state(ref_state_names, 5)
    mods = make_modules(M, sd)
    scenes = [to_torch_scene(s) for s in gen.synth_batch("S2", seed=3, n_scenes=3)]
    with torch.no_grad():
        graph = M.graph_gather([s["graph"] for s in scenes])
        feat = mods["map_net"].stem(torch.cat(graph["ctrs"], 0), graph["feats"])
        plan = M.lane_plan(graph)
        outs = [M.lane_conv(mods["map_net"].fuse, feat, plan, 6, tile_rb=rb).cpu().numpy() for rb in (1, 2, 3, 4)]
    for o in outs[1:]:
        assert np.array_equal(outs[0], o)


def test_engine_matches_modules_and_graph_replay(hip, ref_state_names):
    """The flat-batch engine (side-stream branches on and off, eager and hipGraph replay) gives bitwise the
    features of the module-level path."""
    M, _ = hip
    from lanegcn_amd import data as gen
    from lanegcn_amd.engine import HotPathEngine, collate_flat
    sd = O.seeded_state(ref_state_names, 11)
    mods = make_modules(M, sd)
    scenes_np = gen.synth_batch("S2", seed=2, n_scenes=5)
    scenes = [to_torch_scene(s) for s in scenes_np]
    actors = torch.from_numpy(np.random.default_rng(1).normal(0, 1, (250, 128)).astype(np.float32)).relu()
    want, _ = run_hot_path(M, mods, scenes, actors)
    fb = collate_flat(scenes_np)
    for branches in (False, True):
        eng = HotPathEngine(mods["map_net"], mods["a2m"], mods["m2m"], mods["m2a"], mods["a2a"], branches=branches)
        out = eng.forward(fb, actors.cuda(), stages=True)
        torch.cuda.synchronize()
        for k in ("map_net", "a2m", "m2m", "m2a", "a2a"):
            assert np.array_equal(out[k].cpu().numpy(), want[k]), (branches, k)
        graph, gout = eng.capture(fb, actors.cuda())
        for _ in range(3):
            graph.replay()
        torch.cuda.synchronize()
        assert np.array_equal(gout["nodes"].cpu().numpy(), want["m2m"]) and np.array_equal(gout["actors"].cpu().numpy(), want["a2a"])


def test_tight_pair_capacities_overflow_is_flagged_safe_and_regrown(hip, ref_state_names):
    """Pair buffers sized below sum_i t_i s_i (engine default: 1.25 x the counts it has seen): a forward whose pair sets
    outgrow them reports NEGATIVE counts, its segment tables stay inside the capacity (nothing reads or writes past the
    [cap, .] buffers), learn_pair_counts() grows the capacities and the next forward equals the one with the bound
    capacities bit for bit; forward_guarded does the whole loop; lgcn_pairs_build alone: first cap pairs, clamped rowptr."""
    M, ops = hip
    from lanegcn_amd import data as gen
    from lanegcn_amd.engine import HotPathEngine, collate_flat
    sd = O.seeded_state(ref_state_names, 11)
    mods = make_modules(M, sd)
    scenes_np = gen.synth_batch("S2", seed=3, n_scenes=16)
    fb = collate_flat(scenes_np)
    actors = torch.from_numpy(np.random.default_rng(2).normal(0, 1, (fb.n_actors, 128)).astype(np.float32)).relu().cuda()
    args = (mods["map_net"], mods["a2m"], mods["m2m"], mods["m2a"], mods["a2a"])
    bound = HotPathEngine(*args)
    bound.pair_caps = "bound"
    want = bound.forward(fb, actors)
    counts = [int(c) for c in torch.stack(want["n_pairs"]).flatten().tolist()]
    assert min(counts) > 4096
    eng = HotPathEngine(*args)
    eng.pair_caps = "tight"                                # the default unless LGCN_PAIR_CAPS says otherwise
    first = eng.forward(fb, actors)                       # nothing seen yet: the bound, cannot overflow
    assert not eng.learn_pair_counts(first) and eng._pair_seen == counts
    assert torch.equal(first["nodes"], want["nodes"]) and torch.equal(first["actors"], want["actors"])
    tight = eng.forward(fb, actors)                       # 1.25 x the counts
    assert torch.equal(tight["nodes"], want["nodes"]) and torch.equal(tight["actors"], want["actors"])
    assert [int(c) for c in torch.stack(tight["n_pairs"]).flatten().tolist()] == counts
    # a batch with more pairs than the engine has seen: pretend it has only seen a tenth
    eng._pair_seen = [max(c // 10, 1) for c in counts]
    caps = [eng._cap(i) for i in range(3)]
    assert all(cap < c for cap, c in zip(caps, counts))
    over = eng.forward(fb, actors)
    assert [int(c) for c in torch.stack(over["n_pairs"]).flatten().tolist()] == [-c for c in counts]
    assert torch.isfinite(over["nodes"]).all() and torch.isfinite(over["actors"]).all()
    assert eng.learn_pair_counts(over) and eng._pair_seen == counts
    again = eng.forward(fb, actors)
    assert torch.equal(again["nodes"], want["nodes"]) and torch.equal(again["actors"], want["actors"])
    eng._pair_seen = [max(c // 10, 1) for c in counts]
    auto = eng.forward_guarded(fb, actors)
    assert torch.equal(auto["nodes"], want["nodes"]) and torch.equal(auto["actors"], want["actors"])
    # a captured forward is sized from its warm-up forwards
    eng2 = HotPathEngine(*args)
    eng2.pair_caps = "tight"
    graph, gout = eng2.capture(fb, actors)
    graph.replay()
    torch.cuda.synchronize()
    assert eng2._pair_seen == counts
    assert torch.equal(gout["nodes"], want["nodes"]) and torch.equal(gout["actors"], want["actors"])
    # the search alone
    full = ops.pairs_build(fb.node_ctrs, fb.node_off, fb.actor_ctrs, fb.actor_off, M.config["actor2map_dist"], fb.cap_a2m, True)
    P = full.count()
    cap = P // 3
    cut = ops.pairs_build(fb.node_ctrs, fb.node_off, fb.actor_ctrs, fb.actor_off, M.config["actor2map_dist"], cap, True)
    assert int(cut.n_pairs.item()) == -P and cut.hi.numel() == cap
    assert torch.equal(cut.hi, full.hi[:cap]) and torch.equal(cut.wi, full.wi[:cap])
    assert torch.equal(cut.rowptr, full.rowptr.clamp(max=cap))


def test_captured_forwards_keep_their_inputs_and_counters(hip, ref_state_names):
    """A hipGraph holds addresses, not references: capture() must keep the FlatBatch, the actor tensor and the index
    counters of a captured forward alive.  Two lanes are captured, every outside reference to their inputs is dropped,
    the freed memory is given to other tensors and overwritten -- the replays (one at a time and both in flight) must
    still equal the eager forwards, and the counters must be zero afterwards."""
    M, ops = hip
    import gc
    from lanegcn_amd import data as gen
    from lanegcn_amd.engine import HotPathEngine, collate_flat
    sd = O.seeded_state(ref_state_names, 5)
    mods = {}
    for name, cls in (("map_net", M.MapNet), ("a2m", M.A2M), ("m2m", M.M2M), ("m2a", M.M2A), ("a2a", M.A2A)):
        m = cls(M.config)
        m.load_state_dict({k[len(name) + 1:]: v for k, v in sd.items() if k.startswith(name + ".")})
        mods[name] = m.cuda().eval()
    eng = HotPathEngine(mods["map_net"], mods["a2m"], mods["m2m"], mods["m2a"], mods["a2a"])
    lanes, want = [], []
    for j in range(2):
        fb = collate_flat(gen.synth_batch("S2", seed=40 + j, n_scenes=4))
        actors = torch.randn(fb.n_actors, 128, device="cuda").relu()
        o = eng.forward(fb, actors)
        want.append((o["nodes"].clone(), o["actors"].clone()))
        g, out = eng.capture(fb, actors)
        lanes.append((torch.cuda.Stream(), g, out))
        del fb, actors, o
    gc.collect()
    torch.cuda.empty_cache()
    junk = [torch.full((1 << 20,), -7, dtype=torch.int64, device="cuda") for _ in range(8)]      # lands on freed memory, if any
    for st, g, out in lanes:
        g.replay()
        torch.cuda.synchronize()
    for rep in range(6):
        st, g, _ = lanes[rep % 2]
        with torch.cuda.stream(st):
            g.replay()
    torch.cuda.synchronize()
    for (st, g, out), (nodes, acts) in zip(lanes, want):
        assert torch.allclose(out["nodes"], nodes, rtol=0, atol=1e-5) and torch.allclose(out["actors"], acts, rtol=0, atol=1e-5)
        assert int(out["nonfinite"]) == 0
        assert int(g._lgcn_inputs[-1].abs().sum()) == 0          # the graph's index counters came back to zero
    del junk


def test_full_net_engine_matches_net_forward(golden, ref_state_names, hip):
    """FullNetEngine (flat inputs, one hipGraph) == Net.forward on the reference's batch format."""
    M, _ = hip
    from lanegcn_amd import data as gen
    from lanegcn_amd.engine import FullNetEngine, collate_flat
    scenes = load_scenes(golden)
    net = M.Net(M.config)
    net.load_state_dict(O.seeded_state(ref_state_names, int(golden["seed"])), strict=True)
    net = net.cuda().eval()
    with torch.no_grad():
        want = net(gen.collate_fn(scenes))
    eng = FullNetEngine(net)
    fb = collate_flat(scenes)
    feats, rot, orig = eng.actor_inputs(scenes)
    sizes = [len(s["ctrs"]) for s in scenes]
    graph, out = eng.capture(fb, feats, rot, orig, sizes)
    graph.replay()
    torch.cuda.synchronize()
    # eager vs captured run may pick different MIOpen conv solvers for ActorNet (stock ops): 1e-5 .. 6e-5 seen
    assert float((out["cls"] - torch.cat(want["cls"], 0)).abs().max()) <= 1e-4
    assert torch.allclose(out["reg"], torch.cat(want["reg"], 0), rtol=1e-6, atol=2e-4)
    for i in range(len(scenes)):     # and against the reference itself
        a = sum(sizes[:i])
        assert float(np.abs(out["cls"][a:a + sizes[i]].cpu().numpy() - golden["net/cls/%d" % i]).max()) <= 2e-4


def test_engine_at_twice_the_baseline_batch_vs_oracle(hip, ref_state_names):
    """64 scenes (20,736 nodes, 3,200 actors, ~215 k pairs) through the flat engine vs the oracle: guards the
    index arithmetic (offsets, caps, scans over several blocks) beyond the BASELINE size."""
    M, ops = hip
    if ops.get_mma() != "f16x2":
        pytest.skip("one mode is enough for the scale check")
    from lanegcn_amd import data as gen
    from lanegcn_amd.engine import HotPathEngine, collate_flat
    sd = O.seeded_state(ref_state_names, 13)
    mods = make_modules(M, sd)
    scenes_np = gen.synth_batch("S2", seed=21, n_scenes=64)
    scenes = [to_torch_scene(s) for s in scenes_np]
    actors = torch.from_numpy(np.random.default_rng(5).normal(0, 1, (3200, 128)).astype(np.float32)).relu()
    eng = HotPathEngine(mods["map_net"], mods["a2m"], mods["m2m"], mods["m2a"], mods["a2a"])
    out = eng.forward(collate_flat(scenes_np), actors.cuda(), stages=True)
    torch.cuda.synchronize()
    want = O.hot_path(O.graph_gather([s["graph"] for s in scenes]), actors, [s["ctrs"] for s in scenes], sd)
    for k in ("map_net", "a2m", "m2m", "m2a", "a2a"):
        assert float((out[k].cpu() - want[k]).abs().max()) <= FTOL, k
    counts = [int(c) for c in torch.stack(out["n_pairs"]).flatten().tolist()]
    for got, (a, c, th) in zip(counts, ((0, 1, 7.0), (1, 0, 6.0), (1, 1, 100.0))):
        ctr = [[s["graph"]["ctrs"] for s in scenes], [s["ctrs"] for s in scenes]]
        assert got == len(O.pair_search(ctr[a], ctr[c], th)[0])


def test_laneconv_on_a_multigraph_vs_oracle(hip, ref_state_names):
    """Lane graphs branch rarely, real maps do merge: rows with in-degree 2, 3..9 and duplicate edges under one
    relation, relations without edges, a node count that is no multiple of the tile.  Exercises the second-edge
    loads and the > 2 tail of the gather (forward M2M = 4 LaneConv layers) against the oracle's index_add_ chain,
    in the engine's fused path and at every tile height."""
    M, ops = hip
    rng = np.random.default_rng(17)
    n = 16 * 23 + 5
    sd = O.seeded_state(ref_state_names, 11)
    m2m = make_modules(M, sd)["m2m"]

    def edges(m, hot=False):
        u = rng.integers(0, n, m)
        if hot:                                   # a few destination rows collect most edges
            u = np.where(rng.random(m) < 0.5, rng.integers(0, 12, m), u)
        v = rng.integers(0, n, m)
        return {"u": torch.from_numpy(u), "v": torch.from_numpy(v)}

    graph = {"pre": [edges(m, hot=(i == 0)) for i, m in enumerate((900, 700, 0, 350, 40, 500))],
             "suc": [edges(m) for m in (800, 0, 600, 300, 3, 450)],
             "left": edges(260, hot=True), "right": edges(0)}
    feat = torch.from_numpy(rng.normal(0, 1, (n, 128)).astype(np.float32)).relu()
    want = O.m2m(feat, graph, sd).numpy()
    deg = np.bincount(graph["pre"][0]["u"].numpy(), minlength=n)
    assert deg.max() >= 9 and (deg == 2).any()
    us, vs = [], []
    for i in range(6):
        for k1 in ("pre", "suc"):
            us.append(graph[k1][i]["u"].cuda())
            vs.append(graph[k1][i]["v"].cuda())
    for k1 in ("left", "right"):
        us.append(graph[k1]["u"].cuda())
        vs.append(graph[k1]["v"].cuda())
    with torch.no_grad():
        plan = ops.csr_build(us, vs, n)
        for rb in (0, 1, 2, 3, 4):
            if rb and ops.get_mma() == "f32":
                continue
            got = M.lane_conv(m2m.fuse, feat.cuda(), plan, 6, tile_rb=rb).cpu().numpy()
            err = float(np.abs(got - want).max())
            assert err <= FTOL, (rb, err)


def test_pairs_build_multi_equals_single_searches(hip):
    """The three pair sets of a forward in one launch triple must be bit-identical to three single searches
    (legacy and fixed offsets; a scene without pairs; different T / S / thresholds per job)."""
    M, ops = hip
    rng = np.random.default_rng(23)
    na, nc = (70, 3, 130, 1), (65, 4, 200, 2)
    agt = torch.cat([torch.from_numpy(rng.integers(-6, 7, (n, 2)).astype(np.float32)) for n in na]).cuda()
    ctx = torch.cat([torch.from_numpy(rng.integers(-6, 7, (n, 2)).astype(np.float32)) + (500.0 if i == 1 else 0.0)
                     for i, n in enumerate(nc)]).cuda()
    a_off = torch.tensor(np.concatenate([[0], np.cumsum(na)]), dtype=torch.int32).cuda()
    c_off = torch.tensor(np.concatenate([[0], np.cumsum(nc)]), dtype=torch.int32).cuda()
    cap_ac = int(np.dot(na, nc))
    searches = [(agt, a_off, ctx, c_off, 5.0, cap_ac), (ctx, c_off, agt, a_off, 3.0, cap_ac),
                (agt, a_off, agt, a_off, 100.0, int(np.dot(na, na)))]
    for legacy in (True, False):
        multi = ops.pairs_build_multi(searches, legacy)
        for s, pm in zip(searches, multi):
            ps = ops.pairs_build(*s, legacy)
            P = ps.count()
            assert pm.count() == P and P > 0
            assert torch.equal(pm.hi[:P], ps.hi[:P]) and torch.equal(pm.wi[:P], ps.wi[:P])
            assert torch.equal(pm.rowptr, ps.rowptr)


def test_fused_index_stage_is_bit_identical(hip):
    """lgcn_index_build (graph_gather + CSR plan + pair searches in three launches, self-cleaning counters) against the
    separate entry points: same rowptr / col / pairs bit for bit; twice in a row (the counters must come back to
    zero); on ragged scenes, a multigraph with duplicate edges and in-degree > 2, and a batch without any pair job."""
    M, ops = hip
    from lanegcn_amd import data as gen
    from lanegcn_amd.engine import collate_flat
    cfg = M.config
    for seed, n_scenes in ((5, 3), (6, 7)):
        fb = collate_flat(gen.synth_batch("S2", seed=seed, n_scenes=n_scenes))
        g64, _ = ops.graph_gather_indices(fb.idx_local, fb.seg_off, fb.seg_base)
        want = ops.csr_build([g64[a:b] for (a, b), _ in fb.rel_slices], [g64[a:b] for _, (a, b) in fb.rel_slices], fb.n_nodes)
        searches = ((fb.node_ctrs, fb.node_off, fb.actor_ctrs, fb.actor_off, cfg["actor2map_dist"], fb.cap_a2m),
                    (fb.actor_ctrs, fb.actor_off, fb.node_ctrs, fb.node_off, cfg["map2actor_dist"], fb.cap_a2m),
                    (fb.actor_ctrs, fb.actor_off, fb.actor_ctrs, fb.actor_off, cfg["actor2actor_dist"], fb.cap_a2a))
        want_pairs = ops.pairs_build_multi(searches, True)
        assert ops.index_fused_ok(fb.n_nodes, len(fb.rel_slices), sum(fb.n_edges))
        cnt = ops.index_counters(fb.n_nodes, len(fb.rel_slices), fb.node_ctrs.device)
        for rep in range(2):
            plan, pairs = ops.index_build(fb.idx_local, fb.seg_off, fb.seg_base, fb.rel_slices, fb.n_nodes, searches, True,
                                          cnt=cnt)
            assert torch.equal(plan.rowptr, want.rowptr) and torch.equal(plan.col, want.col), (seed, rep)
            assert plan.n_edges == want.n_edges
            for got, ref in zip(pairs, want_pairs):
                P = ref.count()
                assert got.count() == P
                assert torch.equal(got.hi[:P], ref.hi[:P]) and torch.equal(got.wi[:P], ref.wi[:P])
                assert torch.equal(got.rowptr, ref.rowptr)
            assert int(cnt.abs().sum()) == 0
    # a multigraph given as ONE segment per run (local = global), no pair job
    rng = np.random.default_rng(3)
    n, us, vs = 16 * 9 + 3, [], []
    for r in range(5):
        m = 0 if r == 3 else int(rng.integers(40, 400))
        us.append(torch.from_numpy(rng.integers(0, n, m)))
        vs.append(torch.from_numpy(rng.integers(0, n, m)))
    flat = torch.cat([t for pair in zip(us, vs) for t in pair]).cuda()
    lens = [len(t) for pair in zip(us, vs) for t in pair]
    offs = np.concatenate([[0], np.cumsum(lens)])
    rel_slices = [((int(offs[2 * r]), int(offs[2 * r + 1])), (int(offs[2 * r + 1]), int(offs[2 * r + 2]))) for r in range(5)]
    seg_off = torch.tensor(offs[:-1], dtype=torch.int64).cuda()
    seg_base = torch.zeros(len(lens), dtype=torch.int64).cuda()
    want = ops.csr_build([u.cuda() for u in us], [v.cuda() for v in vs], n)
    plan, pairs = ops.index_build(flat, seg_off, seg_base, rel_slices, n)
    assert pairs == [] and torch.equal(plan.rowptr, want.rowptr) and torch.equal(plan.col, want.col)


@pytest.mark.parametrize("shape", [(1600, 32, 20), (37, 64, 10), (5, 128, 5), (130, 128, 20), (3, 7, 3)])
def test_gn_cl_vs_torch_group_norm(hip, shape):
    """lgcn_gn_cl = GroupNorm(1 group over (C, L)) [+ res] [ReLU] in one launch vs torch's fp64 GroupNorm on the CPU."""
    M, ops = hip
    torch.manual_seed(shape[0])
    n, C_, L_ = shape
    x = torch.randn(n, C_, L_) * 3.0 + 0.7
    res = torch.randn(n, C_, L_)
    gn = torch.nn.GroupNorm(1, C_)
    with torch.no_grad():
        gn.weight.uniform_(0.5, 1.5)
        gn.bias.uniform_(-0.5, 0.5)
    ref = torch.nn.functional.group_norm(x.double(), 1, gn.weight.double(), gn.bias.double(), gn.eps)
    for use_res in (False, True):
        for relu in (False, True):
            want = ref + res.double() if use_res else ref
            want = want.relu() if relu else want
            got = ops.gn_cl(x.cuda(), gn.weight.cuda(), gn.bias.cuda(), gn.eps, res=res.cuda() if use_res else None, relu=relu)
            assert float((got.cpu().double() - want).abs().max()) <= 2e-5, (use_res, relu)


def test_gn_cl_with_upsampled_residual(hip):
    """res_up2: the FPN top-down step "interpolate(coarse, x2, linear) + lateral norm" in one launch vs torch."""
    M, ops = hip
    torch.manual_seed(5)
    for n, C_, L_ in ((1600, 128, 10), (9, 128, 20), (4, 16, 2)):
        x, coarse = torch.randn(n, C_, L_), torch.randn(n, C_, L_ // 2)
        gn = torch.nn.GroupNorm(1, C_)
        with torch.no_grad():
            gn.weight.uniform_(0.5, 1.5)
            gn.bias.uniform_(-0.5, 0.5)
        up = torch.nn.functional.interpolate(coarse.double(), scale_factor=2, mode="linear", align_corners=False)
        want = up + torch.nn.functional.group_norm(x.double(), 1, gn.weight.double(), gn.bias.double(), gn.eps)
        got = ops.gn_cl(x.cuda(), gn.weight.cuda(), gn.bias.cuda(), gn.eps, res=coarse.cuda(), res_up2=True)
        assert float((got.cpu().double() - want).abs().max()) <= 2e-5
        assert float((M.upsample2_linear(coarse).double() - up).abs().max()) <= 1e-6      # the op-level fallback agrees too


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_random_ragged_batches_engine_vs_oracle(hip, ref_state_names, seed):
    """Fuzz: 5-8 scenes of random size (road layouts, 1..37 actors), one scene shifted 5 km away from its actors
    (no A2M / M2A pairs there: the legacy offset quirk in the middle of a batch), int16 indices; the flat engine
    (batched pair search, CSR plan, fused kernels) against the oracle, every stage and the pair counts."""
    M, ops = hip
    from lanegcn_amd import data as gen
    from lanegcn_amd.engine import HotPathEngine, collate_flat
    rng = np.random.default_rng(100 + seed)
    sd = O.seeded_state(ref_state_names, 20 + seed)
    mods = make_modules(M, sd)
    scenes_np = []
    for j in range(int(rng.integers(5, 9))):
        roads = [int(r) for r in rng.integers(4, 7, int(rng.integers(1, 4)))]
        sc = gen.synth_scene(rng, roads, int(rng.integers(1, 38)), idx_dtype=np.int16)
        if j == 2:
            sc["ctrs"] = sc["ctrs"] + np.float32(5000.0)          # actors far from their map
        scenes_np.append(sc)
    scenes = [to_torch_scene(s) for s in scenes_np]
    A_ = sum(len(s["ctrs"]) for s in scenes)
    actors = torch.from_numpy(rng.normal(0, 1, (A_, 128)).astype(np.float32)).relu()
    from lanegcn_amd.utils import to_long
    want = O.hot_path(O.graph_gather([to_long(dict(s["graph"])) for s in scenes]), actors, [s["ctrs"] for s in scenes], sd)
    eng = HotPathEngine(mods["map_net"], mods["a2m"], mods["m2m"], mods["m2a"], mods["a2a"])
    got = eng.forward(collate_flat(scenes_np), actors.cuda(), stages=True)
    for k in ("map_net", "a2m", "m2m", "m2a", "a2a"):
        err = float((got[k].cpu() - want[k]).abs().max())
        assert err <= FTOL, (k, err)
    node_ctrs, actor_ctrs = [s["graph"]["ctrs"] for s in scenes], [s["ctrs"] for s in scenes]
    for n_dev, (a, c, th) in zip(got["n_pairs"], ((node_ctrs, actor_ctrs, 7.0), (actor_ctrs, node_ctrs, 6.0),
                                                   (actor_ctrs, actor_ctrs, 100.0))):
        assert int(n_dev.item()) == len(O.pair_search(a, c, th)[0])


def test_actor_net_channels_last_path_equals_stock_path(hip):
    """ActorNet inference path (channels_last convolutions + lgcn_gn_cl glue) vs the stock NCL module path
    (taken when autograd records) vs a CPU fp32 run of the same module."""
    M, ops = hip
    torch.manual_seed(11)
    net = M.ActorNet(M.config).eval()
    with torch.no_grad():
        for p in net.parameters():
            if p.dim() == 1:
                p.uniform_(0.5, 1.5) if p.mean() > 0.5 else p.uniform_(-0.3, 0.3)
    x = torch.randn(333, 3, 20)
    with torch.no_grad():
        want = net(x)                                   # CPU: stock path
    net = net.cuda()
    with torch.no_grad():
        got = net(x.cuda())                             # HIP glue + channels_last convolutions
        assert net._channels_last_ok(x.cuda())
    stock = net(x.cuda().requires_grad_(True)).detach() # autograd records: stock NCL path on the GPU
    assert got.shape == (333, 128)
    assert float((got.cpu() - want).abs().max()) <= 2e-4
    assert float((got - stock).abs().max()) <= 2e-4


def test_actor_net_hip_conv_path(hip, mma_mode):
    """ActorNet on lgcn_conv1d_gn (conv + GroupNorm + residual / x2-upsampled residual + ReLU in one launch) against the
    CPU fp32 run of the same module and the channels-last stock path, actor counts that are not a multiple of the
    workgroup's 4 / 8 / 16 actors included; and the single op against torch for every shape ActorNet uses.  Bit for bit:
    a fused Res1d launch against its composition of single units, and (f16x2 mode, where the HIP path runs) the whole
    net with fuse_blocks / fuse_groups on against off.
    The HIP convolutions always split their operands into two fp16 planes, so they are the path of the f16x2 mode only:
    in the exact-f32 and bf16x3 modes (and inside the range guard's bf16x3 re-run) ActorNet takes the MIOpen path."""
    M, ops = hip
    import torch.nn.functional as F
    torch.manual_seed(13)
    net = M.ActorNet(M.config).eval()
    with torch.no_grad():
        for p in net.parameters():
            if p.dim() == 1:
                p.uniform_(0.5, 1.5) if p.mean() > 0.5 else p.uniform_(-0.3, 0.3)
    for n in (333, 1, 1600):
        x = torch.randn(n, 3, 20) * 3.0
        with torch.no_grad():
            want = net(x)
        net = net.cuda()
        prev = M.ActorNet.impl
        try:
            with torch.no_grad():
                M.ActorNet.impl = "hip"
                assert net._hip_ok(x.cuda()) == (mma_mode == "f16x2")
                got = net(x.cuda())
                M.ActorNet.impl = "miopen"
                other = net(x.cuda())
        finally:
            M.ActorNet.impl = prev
        net = net.cpu()
        assert got.shape == (n, 128)
        assert float((got.cpu() - want).abs().max()) <= 1e-4, n
        assert float((got - other).abs().max()) <= 2e-4, n
    # whole Res1d blocks in one launch (lgcn_res1d_gn) against the same module on the CPU, and bit for bit against its
    # composition of single units (one definition of staging, tap GEMM and GroupNorm serves both kernels)
    from lanegcn_amd.layers import Res1d

    def unit(conv, norm, x, **kw):
        return ops.conv1d_gn(x, conv.weight, conv.stride[0], norm.weight, norm.bias, norm.eps, **kw)
    for cin, c, stride, lin in ((3, 32, 1, 20), (32, 32, 1, 20), (32, 64, 2, 20), (64, 64, 1, 10), (64, 128, 2, 10),
                                (128, 128, 1, 5), (128, 128, 1, 20), (96, 128, 2, 20)):
        torch.manual_seed(cin + c)
        blk = Res1d(cin, c, stride=stride, norm="GN", ng=1).eval()
        with torch.no_grad():
            for q in blk.parameters():
                if q.dim() == 1:
                    q.uniform_(0.5, 1.5) if q.mean() > 0.5 else q.uniform_(-0.3, 0.3)
        for A_ in (37, 1):
            x = torch.randn(A_, cin, lin) * 2.0
            with torch.no_grad():
                want = blk(x)
            blk = blk.cuda()
            xg = x.transpose(1, 2).contiguous().cuda()
            got = ops.res1d_gn(xg, blk)
            skip = xg if blk.downsample is None else unit(blk.downsample[0], blk.downsample[1], xg)
            units = unit(blk.conv2, blk.bn2, unit(blk.conv1, blk.bn1, xg, relu=True), res=skip, relu=True)
            blk = blk.cpu()
            assert got.shape == (A_, want.shape[2], c)
            err = float((got.cpu().transpose(1, 2) - want).abs().max())
            assert err <= 1e-4, (cin, c, stride, lin, A_, err)
            assert torch.equal(got, units), (cin, c, stride, lin, A_, float((got - units).abs().max()))
    # two blocks of a group in one launch (lgcn_res1d_pair_gn) against the CPU modules
    for cin, c, stride, lin in ((3, 32, 1, 20), (32, 64, 2, 20), (64, 128, 2, 10), (64, 64, 1, 10)):
        torch.manual_seed(7 * cin + c)
        b0, b1 = Res1d(cin, c, stride=stride, norm="GN", ng=1).eval(), Res1d(c, c, norm="GN", ng=1).eval()
        with torch.no_grad():
            for q in list(b0.parameters()) + list(b1.parameters()):
                if q.dim() == 1:
                    q.uniform_(0.5, 1.5) if q.mean() > 0.5 else q.uniform_(-0.3, 0.3)
        for A_ in (37, 1):
            x = torch.randn(A_, cin, lin) * 2.0
            with torch.no_grad():
                want = b1(b0(x))
            b0, b1 = b0.cuda(), b1.cuda()
            got = ops.res1d_gn(x.transpose(1, 2).contiguous().cuda(), b0, second=b1)
            b0, b1 = b0.cpu(), b1.cpu()
            err = float((got.cpu().transpose(1, 2) - want).abs().max())
            assert got.shape == (A_, want.shape[2], c) and err <= 1e-4, (cin, c, stride, lin, A_, err)
    net = net.cuda()
    x = (torch.randn(333, 3, 20) * 3.0).cuda()
    prev = M.ActorNet.fuse_blocks, M.ActorNet.fuse_groups
    try:
        with torch.no_grad():
            M.ActorNet.fuse_blocks, M.ActorNet.fuse_groups = True, True
            y2 = net(x)
            M.ActorNet.fuse_blocks, M.ActorNet.fuse_groups = True, False
            y1 = net(x)
            M.ActorNet.fuse_blocks = False
            y0 = net(x)
    finally:
        M.ActorNet.fuse_blocks, M.ActorNet.fuse_groups = prev
    net = net.cpu()
    assert float((y1 - y0).abs().max()) <= 1e-4 and float((y2 - y0).abs().max()) <= 1e-4
    if mma_mode == "f16x2":             # the HIP path (elsewhere the switches select nothing: three MIOpen runs)
        assert torch.equal(y1, y0) and torch.equal(y2, y0), (float((y1 - y0).abs().max()), float((y2 - y0).abs().max()))
    # the op alone
    gen = torch.Generator().manual_seed(3)
    for cin, cout, ks, stride, lin, mode in ((3, 32, 3, 1, 20, 0), (3, 32, 1, 1, 20, 0), (32, 32, 3, 1, 20, 1), (32, 64, 3, 2, 20, 0),
                                              (32, 64, 1, 2, 20, 0), (64, 64, 3, 1, 10, 1), (64, 128, 3, 2, 10, 0), (128, 128, 3, 1, 5, 1),
                                              (64, 128, 3, 1, 10, 2), (32, 128, 3, 1, 20, 2), (128, 128, 3, 1, 20, 1),
                                              (96, 64, 3, 1, 10, 1), (70, 32, 1, 2, 20, 0), (128, 128, 1, 1, 20, 0)):
        A_ = 37
        x = torch.randn(A_, cin, lin, generator=gen)
        w = torch.randn(cout, cin, ks, generator=gen) * (1.0 / (cin * ks) ** 0.5)
        g, b = torch.rand(cout, generator=gen) + 0.5, torch.randn(cout, generator=gen) * 0.2
        y = F.group_norm(F.conv1d(x, w, stride=stride, padding=(ks - 1) // 2), 1, g, b, 1e-5)
        lout = y.shape[2]
        res = None
        if mode == 1:
            res = torch.randn(A_, cout, lout, generator=gen)
            y = y + res
        elif mode == 2:
            res = torch.randn(A_, cout, lout // 2, generator=gen)
            y = y + F.interpolate(res, scale_factor=2, mode="linear", align_corners=False)
        y = torch.relu(y)
        wp = torch.nn.Parameter(w.cuda())
        got = ops.conv1d_gn(x.transpose(1, 2).contiguous().cuda(), wp, stride, g.cuda(), b.cuda(), 1e-5,
                            res=None if res is None else res.transpose(1, 2).contiguous().cuda(), res_up2=mode == 2, relu=True)
        err = float((got.cpu().transpose(1, 2) - y).abs().max())
        assert err <= 1e-4, (cin, cout, ks, stride, lin, mode, err)


def test_pred_net_hip_tail(hip):
    """PredNet with its stock-op tail on lgcn_pred_reg / lgcn_pred_final against the CPU fp32 run of the same module
    (scores, their order, the gathered trajectories), against the stock path on the device, and the world-frame
    transform of the last launch against matmul + orig; the two ops alone against torch, equal scores included."""
    M, ops = hip
    torch.manual_seed(21)
    net = M.PredNet(M.config).eval()
    for n, sizes in ((333, (100, 33, 200)), (1, (1,)), (1600, (800, 800))):
        actors = torch.randn(n, 128).relu()
        ctrs = torch.randn(n, 2) * 30.0
        idcs, cl, st = [], [], 0
        for k in sizes:
            idcs.append(torch.arange(st, st + k))
            cl.append(ctrs[st:st + k])
            st += k
        with torch.no_grad():
            want = net(actors, idcs, cl)
        net = net.cuda()
        prev = M.PredNet.impl
        try:
            with torch.no_grad():
                M.PredNet.impl = "hip"
                assert net._hip_ok(actors.cuda())
                got = net(actors.cuda(), [i.cuda() for i in idcs], [c.cuda() for c in cl])
                rot = torch.randn(n, 2, 2).cuda()
                orig = (torch.randn(n, 2) * 100.0).cuda()
                cls_w, reg_w = net.forward_flat(actors.cuda(), ctrs.cuda(), rot, orig)
                M.PredNet.impl = "stock"
                assert not net._hip_ok(actors.cuda())
                other = net(actors.cuda(), [i.cuda() for i in idcs], [c.cuda() for c in cl])
        finally:
            M.PredNet.impl = prev
        net = net.cpu()
        for i in range(len(sizes)):
            assert got["cls"][i].shape == want["cls"][i].shape and got["reg"][i].shape == want["reg"][i].shape
            assert float((got["cls"][i].cpu() - want["cls"][i]).abs().max()) <= 1e-4
            assert float((got["reg"][i].cpu() - want["reg"][i]).abs().max()) <= 1e-4
            assert float((got["cls"][i] - other["cls"][i]).abs().max()) <= 1e-4
            assert float((got["reg"][i] - other["reg"][i]).abs().max()) <= 1e-4
        reg_all = torch.cat(got["reg"], 0)
        ref_w = torch.matmul(reg_all.double(), rot.double().unsqueeze(1)) + orig.double().view(-1, 1, 1, 2)
        assert float((reg_w.double() - ref_w).abs().max()) <= 1e-4 * 10       # values up to a few hundred: fp32 ulp 3e-5
        assert torch.equal(cls_w, torch.cat(got["cls"], 0))
    # the ops alone
    gen = torch.Generator().manual_seed(5)
    for A_, Mo, T in ((70, 6, 30), (33, 3, 7), (5, 8, 32)):
        h = [torch.randn(A_, 128, generator=gen) for _ in range(Mo)]
        w = [torch.randn(2 * T, 128, generator=gen) * 0.1 for _ in range(Mo)]
        b = [torch.randn(2 * T, generator=gen) for _ in range(Mo)]
        ctrs = torch.randn(A_, 2, generator=gen) * 10
        wd, bd = torch.randn(128, 2, generator=gen), torch.randn(128, generator=gen)
        reg = torch.stack([h[m].double() @ w[m].double().t() + b[m].double() for m in range(Mo)], 1).view(A_, Mo, T, 2) \
            + ctrs.double().view(-1, 1, 1, 2)
        hd = torch.relu((ctrs.double().unsqueeze(1) - reg[:, :, -1]).reshape(-1, 2) @ wd.double().t() + bd.double())
        g_reg, g_hd = ops.pred_reg([t.cuda() for t in h], [t.cuda() for t in w], [t.cuda() for t in b], ctrs.cuda(), wd.cuda(), bd.cuda())
        assert float((g_reg.cpu().double() - reg).abs().max()) <= 2e-5
        assert float((g_hd.cpu().double() - hd).abs().max()) <= 2e-4
        f = torch.randn(A_ * Mo, 128, generator=gen)
        f[Mo:2 * Mo] = f[Mo]                                  # one actor with all scores equal: mode order is kept
        wc, bc = torch.randn(1, 128, generator=gen), torch.randn(1, generator=gen)
        cls = (f.double() @ wc.double().t() + bc.double()).view(A_, Mo)
        scls, order = cls.sort(dim=1, descending=True, stable=True)
        rot, orig = torch.randn(A_, 2, 2, generator=gen), torch.randn(A_, 2, generator=gen) * 50
        regf = g_reg.cpu()
        want = torch.matmul(torch.gather(regf.double(), 1, order.view(A_, Mo, 1, 1).expand(-1, -1, T, 2)), rot.double().unsqueeze(1)) \
            + orig.double().view(-1, 1, 1, 2)
        g_cls, g_out = ops.pred_final(f.cuda(), wc.cuda(), bc.cuda(), g_reg, rot.cuda(), orig.cuda())
        assert float((g_cls.cpu().double() - scls).abs().max()) <= 2e-5
        assert float((g_out.cpu().double() - want).abs().max()) <= 1e-4
        g_cls2, g_out2 = ops.pred_final(f.cuda(), wc.cuda(), bc.cuda(), g_reg)
        assert torch.equal(g_cls2, g_cls)
        assert torch.equal(g_out2.cpu(), torch.gather(regf, 1, order.view(A_, Mo, 1, 1).expand(-1, -1, T, 2)))


@pytest.mark.parametrize("shape", [(1600, 128, 20), (77, 32, 20), (9, 64, 10), (4, 128, 5), (3, 6, 4)])
def test_gn_cl_channels_last_layout(hip, shape):
    """lgcn_gn_cl on [n, C, 1, L] channels_last tensors (memory [n, L, C]), incl. the upsampled residual, vs torch."""
    M, ops = hip
    torch.manual_seed(shape[1])
    n, C_, L_ = shape
    cl = torch.channels_last
    x = torch.randn(n, C_, 1, L_) * 2 + 0.5
    res = torch.randn(n, C_, 1, L_)
    gn = torch.nn.GroupNorm(1, C_)
    with torch.no_grad():
        gn.weight.uniform_(0.5, 1.5)
        gn.bias.uniform_(-0.5, 0.5)
    ref = torch.nn.functional.group_norm(x.double(), 1, gn.weight.double(), gn.bias.double(), gn.eps)
    xc = x.cuda().contiguous(memory_format=cl)
    got = ops.gn_cl(xc, gn.weight.cuda(), gn.bias.cuda(), gn.eps, res=res.cuda().contiguous(memory_format=cl), relu=True)
    assert got.is_contiguous(memory_format=cl) and got.shape == x.shape
    assert float((got.cpu().double() - (ref + res.double()).relu()).abs().max()) <= 2e-5
    if L_ % 2 == 0:
        coarse = torch.randn(n, C_, 1, L_ // 2)
        up = torch.nn.functional.interpolate(coarse.double().squeeze(2), scale_factor=2, mode="linear",
                                             align_corners=False).unsqueeze(2)
        got = ops.gn_cl(xc, gn.weight.cuda(), gn.bias.cuda(), gn.eps, res=coarse.cuda().contiguous(memory_format=cl),
                        res_up2=True)
        assert float((got.cpu().double() - (up + ref)).abs().max()) <= 2e-5


def test_att_pairs_ws_wi_agree_and_pieces(gcase, golden, hip, mma_mode):
    """lgcn_att_pairs_ws (weights in registers, 64-pair tiles) and lgcn_att_pairs_wi (weights in LDS, wave-independent
    16-pair blocks): (1) seg = 0 writes the same pair rows as the other kernel of the mode (ws against wi in f16x2 /
    bf16; in bf16x3, which has ws only, against the exact-f32 kernel lgcn_att_pairs); (2) seg = 16 writes exactly the
    per-target sums of the 16-aligned pieces, at the piece's first row, and touches no other row; (3) the whole hot path
    with every pair kernel of the mode meets the reference captures."""
    M, ops = hip
    if mma_mode == "f32":
        pytest.skip("split-precision kernel")
    scenes, _, mods = gcase
    actors = torch.from_numpy(golden["actors_in"])
    # (3) every implementation of the mode end to end
    try:
        for impl in ("ws", "wi"):
            ops.set_att_pairs_impl(impl)
            if ops.att_pairs_impl() != impl:
                continue                      # wi: two- / one-plane modes only
            out, _ = run_hot_path(M, mods, scenes, actors)
            for k in ("a2m", "m2m", "m2a", "a2a"):
                err = float(np.abs(out[k] - golden[k]).max())
                assert err <= FTOL, (impl, k, err)
    finally:
        ops.set_att_pairs_impl("wi")
    # (1), (2) on the A2A pair set of the fixture (ragged: 5 scenes, several pairs per target)
    att = mods["a2a"].att[0]
    ctrs = [s["ctrs"].cuda() for s in scenes]
    idcs, n = [], 0
    for c in ctrs:
        idcs.append(torch.arange(n, n + len(c), device="cuda"))
        n += len(c)
    with torch.no_grad():
        ps = M.build_pairs(idcs, ctrs, idcs, ctrs, M.config["actor2actor_dist"])
        P = ps.count()
        assert P > 64
        x = torch.from_numpy(golden["m2a"]).cuda()
        c0 = att.ctx[0]
        U = ops.agg_mlp(n, [ops.RelSpec(x, ops.packed(att.query.linear.weight))], M.L.F_GN1 | M.L.F_RELU1 | M.L.F_GEMM2,
                        gn1=M._gn(att.query.norm), wp2=ops.packed(c0.linear.weight, 128, 128))
        V = ops.agg_mlp(n, [ops.RelSpec(x, ops.packed(c0.linear.weight, 256, 128))], 0)
        args = (ps, att.dist[0].weight, att.dist[0].bias, (att.dist[2].linear.weight, 0), M._gn(att.dist[2].norm),
                (c0.linear.weight, 0), U, V, M._gn(c0.norm))
        try:
            m = {}
            for impl in ("ws", "wi"):
                ops.set_att_pairs_impl(impl)
                if ops.att_pairs_impl() == impl:      # wi: two- / one-plane modes only
                    m[impl] = ops.att_pairs(*args)[:P].cpu().numpy()
            if "wi" in m:
                m_ref = m["wi"]
            else:
                with ops.mma_scope("f32"):            # lgcn_att_pairs on f32-packed images of the same weights
                    m_ref = ops.att_pairs(*args)[:P].cpu().numpy()
            err = float(np.abs(m["ws"] - m_ref).max()) / max(1.0, float(np.abs(m_ref).max()))
            assert err <= 2e-5, err
            hi = ps.hi[:P].cpu().numpy()
            first = np.ones(P, bool)
            first[1:] = (hi[1:] != hi[:-1]) | (np.arange(1, P) % 16 == 0)
            starts = np.flatnonzero(first)
            untouched = np.ones(ps.cap, bool)
            untouched[starts] = False
            for impl, m_k in m.items():
                ops.set_att_pairs_impl(impl)
                canary = torch.full((ps.cap, 128), 7777.0, device="cuda")
                m_seg = ops.att_pairs(*args, m=canary, seg=16).cpu().numpy()
                want = np.add.reduceat(m_k.astype(np.float64), starts, axis=0)
                assert float(np.abs(m_seg[starts] - want).max()) <= 1e-4 * max(1.0, float(np.abs(want).max())), impl
                assert (m_seg[untouched] == 7777.0).all(), impl
        finally:
            ops.set_att_pairs_impl("wi")


def test_net_forward_graph_cache(golden, ref_state_names, hip):
    """Drop-in Net.forward(data) under no_grad: eager, then captured on the second identical-shape call, then
    replayed -- same outputs each time; a batch of another shape in between runs eagerly; a weight update drops
    the captured graph."""
    M, _ = hip
    from lanegcn_amd import data as gen
    net = M.Net(M.config)
    net.load_state_dict(O.seeded_state(ref_state_names, int(golden["seed"])), strict=True)
    net = net.cuda().eval()
    scenes = load_scenes(golden)
    batch, other = gen.collate_fn(scenes), gen.collate_fn(scenes[:3])
    with torch.no_grad():
        outs = [net(batch) for _ in range(4)]                      # eager, eager -> capture, replay, replay
        assert net.__dict__["_graph_state"]["graph"] is not None
        close = lambda a, b: torch.allclose(a, b, rtol=1e-5, atol=2e-4)
        for i in range(len(scenes)):      # eager vs captured: same arithmetic up to the stock ops' (MIOpen, sort) own noise
            assert close(outs[3]["cls"][i], outs[0]["cls"][i]) and close(outs[3]["reg"][i], outs[0]["reg"][i])
        keep = [[t.clone() for t in outs[3]["reg"]], [t.clone() for t in outs[3]["cls"]]]
        o3 = net(other)                                            # other shapes: eager, the captured graph stays
        assert len(o3["cls"]) == 3 and net.__dict__["_graph_state"]["graph"] is not None
        o4 = net(batch)                                            # replayed again (ActorNet's stock convolutions are
        for i in range(len(scenes)):                               # not bitwise repeatable: 1 ulp of a ~1000 m coordinate)
            assert close(o4["reg"][i], keep[0][i]) and close(o4["cls"][i], keep[1][i])
        for i in range(len(scenes)):
            assert float(np.abs(o4["cls"][i].cpu().numpy() - golden["net/cls/%d" % i]).max()) <= 2e-4
        net.pred_net.cls[1].weight.add_(0.01)                     # a weight changed: replaying would be stale
        o5 = net(batch)
        assert not torch.equal(o5["cls"][0], keep[1][0])


def test_net_forward_graph_replay_with_other_content(golden, ref_state_names, hip):
    """The captured whole-Net graph replayed on a batch of the SAME signature (shapes, per-scene sizes) but other content --
    actor tracks and centres moved, so the pair sets change too: equal to the eager forward of that batch; results handed
    out earlier stay what they were (the caller owns them).  (Pair sets that outgrow a captured graph's capacities:
    test_tight_pair_capacities_overflow_is_flagged_safe_and_regrown, on the engine.)"""
    M, _ = hip
    import copy
    from lanegcn_amd import data as gen
    net = M.Net(M.config)
    net.load_state_dict(O.seeded_state(ref_state_names, int(golden["seed"])), strict=True)
    net = net.cuda().eval()
    scenes = load_scenes(golden)
    rng = np.random.default_rng(9)

    def moved(scale, one_spot=False):
        out = copy.deepcopy(scenes)
        for sc in out:
            f, c = np.asarray(sc["feats"], np.float32), np.asarray(sc["ctrs"], np.float32)
            sc["feats"] = (f * 0.9).astype(np.float32)
            c = c + rng.normal(0, scale, c.shape).astype(np.float32)
            if one_spot:          # every actor of a scene on the first lane node: far more pairs of every kind
                c = c * 0 + np.asarray(sc["graph"]["ctrs"], np.float32)[:1]
            sc["ctrs"] = c.astype(np.float32)
        return out

    a, b, far = gen.collate_fn(scenes), gen.collate_fn(moved(0.3)), gen.collate_fn(moved(0.0, one_spot=True))
    close = lambda x, y: torch.allclose(x, y, rtol=1e-5, atol=2e-4)
    with torch.no_grad():
        M.Net.graph_cache = False
        try:
            want_b, want_far = net(b), net(far)
        finally:
            M.Net.graph_cache = True
        net.__dict__.pop("_graph_state", None)
        net.__dict__["_engine"].hot._pair_seen = [0, 0, 0]          # forget the counts the eager runs have taught the engine
        first = net(a)
        held = net(a)                                    # captured here
        assert net.__dict__["_graph_state"]["graph"] is not None
        keep = [t.clone() for t in held["reg"]]
        got_b = net(b)                                   # same signature, other content: replay
        assert net.__dict__["_graph_state"]["graph"] is not None
        for i in range(len(scenes)):
            assert close(got_b["reg"][i], want_b["reg"][i]) and close(got_b["cls"][i], want_b["cls"][i]), i
            assert torch.equal(held["reg"][i], keep[i]), "a result handed out earlier was overwritten by the replay"
            assert close(first["reg"][i], held["reg"][i])
        got_far = net(far)                               # every actor of a scene on one spot: other pair sets again
        for i in range(len(scenes)):
            assert close(got_far["reg"][i], want_far["reg"][i]) and close(got_far["cls"][i], want_far["cls"][i]), i


# ------------------------------------------------------------------ round 3: folded row-block launches of the Att blocks
def test_chained_outputs_and_multi_launch_equal_separate_launches(hip):
    """lgcn_agg_mlp's chained outputs (ch_*: the NEXT Att layer's U / V computed from a row block's output rows before
    they leave the CU) and lgcn_agg_mlp_multi (several row blocks in one launch) give bit for bit what separate
    launches give -- ragged row counts, one- and two-stage blocks, U only / V only / both."""
    M, ops = hip
    from lanegcn_amd import _lib as L
    g = torch.Generator().manual_seed(5)
    w = lambda: ops.packed((torch.randn(128, 128, generator=g) * 0.09).cuda())
    gn = lambda: ((1 + 0.1 * torch.randn(128, generator=g)).cuda(), (0.1 * torch.randn(128, generator=g)).cuda())
    full = L.F_GN1 | L.F_RELU1 | L.F_GEMM2 | L.F_GN2 | L.F_RES | L.F_RELU2
    for n_rows in (1, 37, 250, 1041):
        x = torch.randn(n_rows, 128, generator=g).cuda()
        w1, w2, wq, wu, wv, g1, g2, gq = w(), w(), w(), w(), w(), gn(), gn(), gn()
        for flags, kw in ((full, dict(gn1=g1, wp2=w2, gn2=g2, res=x)), (L.F_GN1 | L.F_RELU1, dict(gn1=g1)), (0, {})):
            base = ops.agg_mlp(n_rows, [ops.RelSpec(x, w1)], flags, **kw)
            u_sep = ops.agg_mlp(n_rows, [ops.RelSpec(base, wq)], L.F_GN1 | L.F_RELU1 | L.F_GEMM2, gn1=gq, wp2=wu)
            v_sep = ops.agg_mlp(n_rows, [ops.RelSpec(base, wv)], 0)
            for cu, cv in ((True, False), (False, True), (True, True)):
                res = ops.agg_mlp(n_rows, [ops.RelSpec(x, w1)], flags, chain_u=(wq, gq, wu) if cu else None,
                                  chain_v=wv if cv else None, **kw)
                assert torch.equal(res[0], base), (n_rows, flags, cu, cv)
                if cu:
                    assert torch.equal(res[1], u_sep), (n_rows, flags, cu, cv)
                if cv:
                    assert torch.equal(res[-1], v_sep), (n_rows, flags, cu, cv)
    # several problems of different heights in one launch, one of them with chained outputs
    xa, xb, xc = (torch.randn(n, 128, generator=g).cuda() for n in (700, 33, 129))
    w1, w2, w3, wq, wu, g1, gq = w(), w(), w(), w(), w(), gn(), gn()
    pa = dict(n_rows=700, rels=[ops.RelSpec(xa, w1)], flags=L.F_GN1 | L.F_RELU1, gn1=g1, chain_u=(wq, gq, wu))
    pb = dict(n_rows=33, rels=[ops.RelSpec(xb, w2)], flags=0)
    pc = dict(n_rows=129, rels=[ops.RelSpec(xc, w3)], flags=0)
    for probs in ([pa, pb, pc], [pb, pa], [pc, pb, pa, pb]):
        got = ops.agg_mlp_multi(probs)
        for q, o in zip(probs, got):
            want = ops.agg_mlp(**q)
            if isinstance(want, tuple):
                assert all(torch.equal(a, b) for a, b in zip(o, want))
            else:
                assert torch.equal(o, want)
    # two two-stage + residual problems in one launch, as PredNet builds them for two heads (LinearRes.block_kw): the
    # smallest row counts that put the boundary between the problems inside, at and past a 16-row sub-tile with a
    # different tile count per problem; at the library's tile height and at every forced one
    from lanegcn_amd.layers import LinearRes
    heads = [LinearRes(128, 128, norm="GN", ng=1).cuda().eval() for _ in range(2)]
    with torch.no_grad():
        for h in heads:
            for p in h.parameters():      # norm gains around 1, everything else around 0
                p.copy_((1.0 if p.dim() == 1 else 0.0) + 0.09 * torch.randn(p.shape, generator=g))
        for na, nb in ((1, 33), (17, 49), (250, 37)):
            xa, xb = torch.randn(na, 128, generator=g).cuda(), torch.randn(nb, 128, generator=g).cuda()
            for rb in (0, 1, 2, 3, 4):
                probs = [dict(h.block_kw(x), tile_rb=rb) for h, x in zip(heads, (xa, xb))]
                want = [ops.agg_mlp(**q) for q in probs]
                for got in (ops.agg_mlp_multi(probs), ops.agg_mlp_pair(*probs)):      # (pair: one launch at rb = 0 only)
                    for o, t in zip(got, want):
                        assert torch.equal(o, t), (na, nb, rb)


@pytest.mark.parametrize("rb", [1, 2, 3, 4])
def test_row_blocks_at_every_tile_height(hip, rb):
    """lgcn_agg_mlp in its Linear / Att roles (plain, two stages + residual, RANGE / RANGE16 segment sums, an Att tail with
    chained U and V, A2M.meta's rank-4 update with a chained U, several problems in one launch) at a forced tile height of
    16 rb rows: bit for bit what the library's own pick gives (pick_rb takes 48-row tiles for these roles at some batch
    sizes, e.g. 54 S2 scenes; the fixtures and S2 itself only ever run 16- and 32-row tiles)."""
    import os
    import sys
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
    import check_tile_rb
    assert check_tile_rb.run(rb, verbose=False) == []


def test_folded_att_blocks_equal_per_layer_launches(gcase, hip):
    """lanegcn.att_block (a layer's tail emits the next layer's U / V, V rows up front, A2M.meta chained into the first
    U, M2A's last tail feeding A2A) against Att.run layer by layer: bit for bit, on the reference's fixture scenes
    (incl. the scene without A2M pairs) and through the engine."""
    M, ops = hip
    from lanegcn_amd.engine import HotPathEngine, collate_flat
    scenes, sd, mods = gcase
    fb = collate_flat(scenes)
    actors = torch.from_numpy(np.random.default_rng(4).normal(0, 1, (fb.n_actors, 128)).astype(np.float32)).relu().cuda()
    eng = HotPathEngine(mods["map_net"], mods["a2m"], mods["m2m"], mods["m2a"], mods["a2a"])
    prev = M.Att.fold
    try:
        M.Att.fold = True
        got = eng.forward(fb, actors, stages=True)
        M.Att.fold = False
        want = eng.forward(fb, actors, stages=True)
    finally:
        M.Att.fold = prev
    torch.cuda.synchronize()
    for k in ("map_net", "a2m", "m2m", "m2a", "a2a"):
        assert torch.equal(got[k], want[k]), k


def test_forward_bitwise_repeatable_alone_and_with_four_in_flight(hip, ref_state_names):
    """The S2 forward (32 scenes) repeated on one stream and with four forwards in flight on four streams gives, every
    time, bit for bit the stage outputs of the first run.  This is the signature test of the wrong rows investigated in
    rounds 2 / 3 (a few rows of a stage differing from run to run, first seen on a build whose
    ReLU was compare + select; tools/relu_variant_check.py is the same loop on that diagnostic build)."""
    M, ops = hip
    from lanegcn_amd import data as gen
    from lanegcn_amd.engine import HotPathEngine, collate_flat
    sd = O.seeded_state(ref_state_names, 3)
    mods = make_modules(M, sd)
    scenes = gen.synth_batch("S2", seed=1)
    fb = collate_flat(scenes)
    actors = torch.from_numpy(np.random.default_rng(2).normal(0, 1, (fb.n_actors, 128)).astype(np.float32)).relu().cuda()
    keys = ("map_net", "a2m", "m2m", "m2a", "a2a")
    eng = HotPathEngine(mods["map_net"], mods["a2m"], mods["m2m"], mods["m2a"], mods["a2a"])
    first = {k: v.clone() for k, v in eng.forward(fb, actors, stages=True).items() if k in keys}
    for r in range(10):
        out = eng.forward(fb, actors, stages=True)
        for k in keys:
            assert torch.equal(out[k], first[k]), ("one stream", r, k)
    streams = [torch.cuda.Stream() for _ in range(4)]
    engs = [HotPathEngine(mods["map_net"], mods["a2m"], mods["m2m"], mods["m2a"], mods["a2a"]) for _ in streams]
    fbs = [collate_flat(scenes) for _ in streams]
    for r in range(4):
        outs = []
        for st, e, f in zip(streams, engs, fbs):
            st.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(st):
                outs.append(e.forward(f, actors, stages=True))
        torch.cuda.synchronize()
        for j, o in enumerate(outs):
            for k in keys:
                assert torch.equal(o[k], first[k]), ("four in flight", r, j, k)
