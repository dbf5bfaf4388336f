"""GPU: HotPathEngine's one pipeline and one host-check loop on the device -- a forward that outgrows its tight pair
capacities is regrown by forward_guarded with exactly one more forward (and the map-only forward, which has no flag and no
counts, passes the same loop); forward() launches what the six stage functions launch, in the same order; and on an empty
actor or lane-node set, where the launches are not folded, forward(stages=True) and the stage functions agree bit for bit."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

STAGES = (("map_net", "nodes"), ("a2m", "nodes_a2m"), ("m2m", "nodes_m2m"), ("m2a", "actors_m2a"), ("a2a", "actors_a2a"))


@pytest.fixture(scope="module")
def hip():
    import lanegcn_amd  # noqa: F401
    from lanegcn_amd import lanegcn as M
    from lanegcn_amd import ops
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return M, ops


@pytest.fixture
def f16x2(hip):
    _, ops = hip
    prev = ops.get_mma()
    ops.set_mma("f16x2")
    yield
    ops.set_mma(prev)


def bits(t):
    return t.contiguous().view(torch.int32)


def engine(M, seed=21):
    from lanegcn_amd.engine import HotPathEngine
    torch.manual_seed(seed)
    return HotPathEngine(*[cls(M.config).cuda().eval() for cls in (M.MapNet, M.A2M, M.M2M, M.M2A, M.A2A)])


def actor_rows(n, seed=5):
    return torch.from_numpy(np.random.default_rng(seed).normal(0, 1, (n, 128)).astype(np.float32)).relu().cuda()


def test_overflow_is_regrown_with_one_more_forward_and_the_map_only_forward_passes(hip, f16x2):
    M, ops = hip
    from lanegcn_amd import data as gen
    from lanegcn_amd.engine import collate_flat
    fb = collate_flat(gen.synth_batch("S2", seed=3, n_scenes=8))
    assert fb.n_actors == 400
    actors = actor_rows(400)
    eng = engine(M)
    eng.pair_caps = "bound"
    want = eng.forward(fb, actors, stages=True)
    counts = [int(c) for c in torch.stack(want["n_pairs"]).flatten().tolist()]
    print("pair counts", counts)                          # numpy gives (5082, 4191, 14966)
    assert min(counts) > 4096                              # above the floor of a tight capacity
    assert int(want["nonfinite"].item()) == 0
    eng.pair_caps = "tight"
    calls, real = [], eng.forward
    eng.forward = lambda *a, **k: (calls.append(k), real(*a, **k))[1]
    tenth = [max(c // 10, 1) for c in counts]
    eng._pair_seen = list(tenth)
    assert all(eng._cap(i) < c for i, c in enumerate(counts))
    got = eng.forward_guarded(fb, actors)
    assert len(calls) == 2, calls                          # the overflowing forward + one with the grown capacities
    assert eng._pair_seen == counts
    assert [int(c) for c in torch.stack(got["n_pairs"]).flatten().tolist()] == counts
    for k in ("nodes", "actors"):
        assert torch.equal(bits(got[k]), bits(want[k])), k
    # the map-only forward: no flag, no counts -- nothing to read, nothing learnt, no second forward
    calls.clear()
    eng._pair_seen = list(tenth)
    only = eng.forward_guarded(fb, actors, mapnet_only=True)
    assert len(calls) == 1 and eng._pair_seen == tenth
    assert sorted(only) == ["actors", "nodes"] and only["actors"] is actors
    assert torch.equal(bits(only["nodes"]), bits(want["map_net"]))


def run_stages(eng, fb, actors):
    st, fns = eng.stage_functions(fb, actors)
    assert [n for n, _ in fns] == ["index", "map_net", "a2m", "m2m", "m2a", "a2a"]
    for _, fn in fns:
        fn()
    return st


def test_forward_launches_what_the_stage_functions_launch(hip, f16x2):
    M, ops = hip
    from lanegcn_amd import data as gen
    from lanegcn_amd.engine import collate_flat
    fb = collate_flat(gen.synth_batch("S0", seed=3))
    assert (fb.n_scenes, fb.n_nodes, fb.n_actors) == (1, 648, 50)
    actors = actor_rows(50)
    eng = engine(M)
    eng.forward(fb, actors)                                # weight images packed outside the recorded runs
    with ops.kernel_timer() as t:
        eng.forward(fb, actors)
    fwd = [tag for tag, _, _ in t.recs]
    with ops.kernel_timer() as t:
        run_stages(eng, fb, actors)
    cut = [tag for tag, _, _ in t.recs]
    torch.cuda.synchronize()
    print("forward", fwd)
    print("stages ", cut)
    if fwd and fwd[-1] == "check_finite":                  # the forward's epilogue
        fwd = fwd[:-1]
    assert fwd == cut
    assert {"laneconv", "att_head", "att_pairs", "att_post", "ctx_heads"} <= set(cut)


def empty_actor_batch():
    from lanegcn_amd import data as gen
    scene = dict(gen.synth_batch("S0", seed=3)[0])
    for k in ("feats", "ctrs", "gt_preds", "has_preds"):
        scene[k] = scene[k][:0]
    return [scene]


def empty_node_batch():
    from lanegcn_amd import data as gen
    scene = dict(gen.synth_batch("S0", seed=3)[0])
    g = scene["graph"]
    none = lambda: {"u": np.zeros(0, np.int64), "v": np.zeros(0, np.int64)}
    scene["graph"] = dict(num_nodes=0, ctrs=g["ctrs"][:0], feats=g["feats"][:0], turn=g["turn"][:0], control=g["control"][:0],
                          intersect=g["intersect"][:0], pre=[none() for _ in g["pre"]], suc=[none() for _ in g["suc"]],
                          left=none(), right=none(), lane_idcs=g["lane_idcs"][:0])
    return [scene]


@pytest.mark.parametrize("which", ["no_actors", "no_nodes"])
def test_empty_sets_forward_and_stage_functions_agree(hip, f16x2, which):
    """No actor row, or no lane node: no launch is folded (one rule for the whole pipeline), every stage runs, and the two
    entry points give the same bits."""
    M, ops = hip
    from lanegcn_amd.engine import collate_flat
    fb = collate_flat(empty_actor_batch() if which == "no_actors" else empty_node_batch())
    assert (fb.n_nodes, fb.n_actors) == ((648, 0) if which == "no_actors" else (0, 50))
    actors = actor_rows(fb.n_actors)
    eng = engine(M)
    out = eng.forward(fb, actors, stages=True)
    st = run_stages(eng, fb, actors)
    torch.cuda.synchronize()
    assert st["u_m2a"] is None and st["uv_a2a"] is None          # the per-layer route
    assert [int(c) for c in torch.stack(out["n_pairs"]).flatten().tolist()] == [int(p.n_pairs.item()) for p in st["pairs"]]
    for name, key in STAGES:
        rows = fb.n_nodes if key.startswith("nodes") else fb.n_actors
        assert out[name].shape == st[key].shape == (rows, 128), name
        assert torch.equal(bits(out[name]), bits(st[key])), name
    assert torch.equal(bits(out["nodes"]), bits(st["nodes_m2m"])) and torch.equal(bits(out["actors"]), bits(st["actors_a2a"]))
