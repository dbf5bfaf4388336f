"""GPU: the PADDED scene-store batch (lgcn_store_gather_pad, DeviceSceneStore.batch_padded) against its host model, the
independence of the real rows from the filler scene, and engine.StoreReplay (one captured graph replayed for every pick
that fits) against the eager route, with its fallbacks, its errors and evaluate_store(..., replay=True)."""
import copy

import numpy as np
import pytest
import torch

import scene_store_cases as SC
from oracle import lanegcn_oracle as O
from store_pad_model import padded_batch_host, pick_totals

pytestmark = pytest.mark.gpu

NO_SCALE5, HOT = 6, 7          # scene 6: no pre[5] / suc[5] edge; scene 7: lane nodes far outside fp16's range after the stem
GATHER_PICKS = ("repeat", "all", "no_left_right", "no_actors", "seventy")
# slack over the pick's totals (nodes, actors, edges per relation): n_f = a_f = 1 with nine filler edges per relation on the
# one filler node; n_f = 300 > 256 (the filler crosses a block); n_f = 3 with eleven filler edges (the modulo)
SLACKS = {"one_node": (1, 1, 9), "wide": (300, 5, 7), "modulo": (3, 2, 11)}


@pytest.fixture(scope="module")
def fx(tmp_path_factory):
    import lanegcn_amd  # noqa: F401
    from lanegcn_amd.flatfile import DeviceSceneStore, write_scenes
    scenes = SC.make_scenes()
    bare = copy.deepcopy(scenes[0])
    for k in ("pre", "suc"):
        bare["graph"][k][5] = {"u": np.zeros(0, np.int64), "v": np.zeros(0, np.int64)}
    hot = copy.deepcopy(scenes[5])
    hot["graph"]["ctrs"] = np.asarray(hot["graph"]["ctrs"], np.float32) * 4096.0
    scenes = scenes + [bare, hot]
    tmp = tmp_path_factory.mktemp("store_pad")
    path = str(tmp / "split.npz")
    write_scenes(path, scenes)
    return dict(scenes=scenes, dev=DeviceSceneStore(path), tmp=tmp)


@pytest.fixture(scope="module")
def net(ref_state_names):
    import lanegcn_amd  # noqa: F401
    from lanegcn_amd import lanegcn as M
    n = M.Net(M.config)
    n.load_state_dict(O.seeded_state(ref_state_names, 3), strict=True)
    return n.cuda().eval()


def caps_of(fx, pick, slack):
    from lanegcn_amd.flatfile import StoreCaps
    n, a, e = pick_totals(fx["scenes"], pick)
    return StoreCaps(len(pick), n + slack[0], a + slack[1], tuple(x + slack[2] for x in e))


def raw(t):
    return t.contiguous().view(torch.uint8).reshape(-1)


def check_padded(got, want, what):
    """Every array of the padded batch equals the host model's, byte for byte, and nothing of a 0xFF pre-fill is left."""
    (fb, ex), (wfb, wex) = got, want
    for f in SC.FLAT_FIELDS:
        assert getattr(fb, f) == getattr(wfb, f), (what, f)
    arrays = [(f, getattr(fb, f), getattr(wfb, f)) for f in SC.FLAT_ARRAYS] + [(k, ex[k], wex[k]) for k in wex if k != "sizes"]
    assert sorted(ex) == sorted(wex) and ex["sizes"] == wex["sizes"], what
    for name, g, w in arrays:
        assert g.dtype == w.dtype and tuple(g.shape) == tuple(w.shape), (what, name, g.dtype, g.shape, w.dtype, w.shape)
        assert torch.equal(raw(g), raw(w)), (what, name)
        b = raw(g)
        if g.element_size() >= 4:
            assert not bool((b.reshape(-1, 4) == 0xFF).all(1).any()), (what, name, "a word of the pre-fill is left")
        else:
            assert not bool((b == 0xFF).any()), (what, name, "a byte of the pre-fill is left")


def filled_slot(dev, caps):
    from lanegcn_amd.flatfile import PaddedSlot
    slot = PaddedSlot(dev, caps)
    slot.buf.fill_(0xFF)
    slot.extra_buf.fill_(0xFF)
    return slot


# ------------------------------------------------------------------ the gather
@pytest.mark.parametrize("slack", sorted(SLACKS))
@pytest.mark.parametrize("name", GATHER_PICKS)
def test_padded_batch_equals_the_host_model(fx, name, slack):
    pick = SC.PICKS[name]
    caps = caps_of(fx, pick, SLACKS[slack])
    want = padded_batch_host(fx["scenes"], pick, caps, fx["tmp"], device="cuda")
    got = fx["dev"].batch_padded(pick, caps, slot=filled_slot(fx["dev"], caps))
    torch.cuda.synchronize()
    check_padded(got, want, (name, slack))
    fb, ex = got
    assert fb.n_scenes == len(pick) + 1 and fb.n_nodes == caps.nodes and fb.n_actors == caps.actors
    assert fb.n_edges == list(caps.edges) and fb.idx_local.numel() == 2 * sum(caps.edges)
    if name == "no_left_right":                      # two relations hold filler edges only
        (a, b), (c, d) = fb.rel_slices[-1]
        n_f = SLACKS[slack][0]
        assert b - a == SLACKS[slack][2] and torch.equal(fb.idx_local[a:b].cpu(), torch.arange(b - a) % n_f)
    if name == "seventy":
        assert fb.node_off.numel() == 72 > 64
    check_padded(fx["dev"].batch_padded(pick, caps), want, (name, slack, "a slot of its own"))


def test_stale_rows_do_not_survive_in_a_slot(fx):
    """One slot filled with a large pick and then with a small one holds the small pick's padded batch and nothing else;
    and two fills back to back without a synchronise each leave their own batch (the staging rule)."""
    dev = fx["dev"]
    big, small = [1, 3, 1, 3], [0, 5, 2, 0]
    caps = caps_of(fx, big, (2, 2, 3))
    slot = filled_slot(dev, caps)
    want = {k: padded_batch_host(fx["scenes"], p, caps, fx["tmp"], device="cuda") for k, p in (("big", big), ("small", small))}
    torch.cuda.synchronize()
    fb, ex = dev.batch_padded(big, caps, slot=slot)
    first = slot.buf.clone(), slot.extra_buf.clone()
    got = dev.batch_padded(small, caps, slot=slot)             # no synchronise in between
    torch.cuda.synchronize()
    check_padded(got, want["small"], "small after big")
    # the first fill, as it was before the second overwrote the slot: compare through a slot-shaped view of the clones
    slot.buf.copy_(first[0])
    slot.extra_buf.copy_(first[1])
    torch.cuda.synchronize()
    check_padded((slot.flat_batch(dev.plan(big, caps=caps)), slot.extras(dev.plan(big, caps=caps))), want["big"], "big")


# ------------------------------------------------------------------ the real rows do not depend on the filler
def modes():
    from lanegcn_amd import lanegcn as M
    from lanegcn_amd import ops
    import contextlib

    @contextlib.contextmanager
    def exact_f32():
        keep = M.ActorNet.exact
        M.ActorNet.exact = True
        try:
            with ops.mma_scope("f32"):
                yield
        finally:
            M.ActorNet.exact = keep
    return {"f16x2": contextlib.nullcontext, "f32_exact": exact_f32}


@pytest.mark.parametrize("mode", ["f16x2", "f32_exact"])
def test_real_rows_do_not_depend_on_the_filler(fx, net, mode):
    """The eager forward on the padded batch gives, in the real rows, bitwise what forward_store_flat gives on the
    unpadded pick; the filler adds no A2M and no M2A pair and exactly its a_f A2A self-pairs; the range guard's word,
    which looks at the real rows only, stays clear."""
    from lanegcn_amd import ops
    from lanegcn_amd.engine import FullNetEngine
    if mode == "f16x2":
        assert ops.get_mma() == "f16x2"
    dev = fx["dev"]
    eng = FullNetEngine(net)
    with modes()[mode](), torch.no_grad():
        for pick, slack in (([3, 1, 1, 0], (1, 1, 0)), ([0, 1, 2, 3, 4, 5], (300, 5, 7)), ([4, 4, 5], (37, 3, 2))):
            caps = caps_of(fx, pick, slack)
            fb, ex = dev.batch_padded(pick, caps)
            out = eng.forward(fb, ex["actor_feats"], ex["rot"], ex["orig"], ex["sizes"])
            wfb, wex, want = net.forward_store_flat(dev, pick)
            A, a_f = wfb.n_actors, caps.actors - wfb.n_actors
            assert out["cls"].shape[0] == caps.actors and A == sum(wex["sizes"])
            assert torch.equal(out["cls"][:A], want["cls"]), (mode, pick, "cls")
            assert torch.equal(out["reg"][:A], want["reg"]), (mode, pick, "reg")
            got_pairs, want_pairs = [int(c) for c in out["n_pairs"]], [int(c) for c in want["n_pairs"]]
            assert got_pairs == [want_pairs[0], want_pairs[1], want_pairs[2] + a_f], (mode, pick)
            assert int(out["nonfinite"].item()) == 0, (mode, pick)


# ------------------------------------------------------------------ StoreReplay
REPLAY_PICKS = [[3, 1, 1, 0], [0, 5, 2, 0], [1, 3, 1, 3], [4, 4, 5, 2], [5, 0, 3, 1], [3, 1, 1, 0], [2, 2, 4, 1], [0, 0, 0, 5]]


def eager(net, dev, pick):
    out = net.forward_store(dev, pick)
    return {k: [t.clone() for t in v] for k, v in out.items()}


def same_lists(got, want, what):
    assert len(got["cls"]) == len(want["cls"]) and len(got["reg"]) == len(want["reg"]), what
    for k in ("cls", "reg"):
        for i, (g, w) in enumerate(zip(got[k], want[k])):
            assert g.dtype == w.dtype and g.shape == w.shape and torch.equal(g, w), (what, k, i)


def fresh(net):
    """Forget the pair counts and graphs this net's engine has learnt, so that a test's route does not depend on its
    predecessors."""
    net.__dict__.pop("_engine", None)
    net.__dict__.pop("_graph_state", None)


def test_eight_picks_replay_one_graph(fx, net):
    from lanegcn_amd.engine import StoreReplay
    from lanegcn_amd.flatfile import StoreCaps
    dev = fx["dev"]
    fresh(net)
    want = [eager(net, dev, p) for p in REPLAY_PICKS]
    fresh(net)
    rp = StoreReplay(net, dev, StoreCaps.for_picks(dev, REPLAY_PICKS), warm=1)
    for i, p in enumerate(REPLAY_PICKS):
        same_lists(net.forward_store(dev, p, replay=rp), want[i], i)
    st = rp.stats
    assert st["captures"] == 1 and st["eager_warm"] == 1 and st["replays"] == 7, st
    assert st["eager_nofit"] == st["eager_overflow"] == st["eager_guard"] == 0, st
    assert 0 < st["pad_nodes"] < 1 and 0 < st["pad_actors"] < 1 and 0 <= st["pad_edges"] < 1 and rp.graph_pool_bytes() >= 0
    # the flat form: the real scenes' batch, views of the first A rows
    fb, ex, out = rp.forward(REPLAY_PICKS[3])
    wfb, wex, wout = net.forward_store_flat(dev, REPLAY_PICKS[3])
    assert (fb.n_scenes, fb.n_nodes, fb.n_actors, fb.n_edges) == (4, wfb.n_nodes, wfb.n_actors, wfb.n_edges)
    assert (fb.cap_a2m, fb.cap_a2a, ex["sizes"]) == (wfb.cap_a2m, wfb.cap_a2a, wex["sizes"])
    for k in ("node_ctrs", "node_feats", "turn", "control", "intersect", "actor_ctrs", "node_off", "actor_off"):
        assert torch.equal(getattr(fb, k), getattr(wfb, k)), k
    for k in ("actor_feats", "rot", "orig", "gt_preds", "has_preds"):
        assert torch.equal(ex[k], wex[k]), k
    assert torch.equal(out["cls"], wout["cls"]) and torch.equal(out["reg"], wout["reg"])


def test_back_to_back_forwards_keep_their_results(fx, net):
    """Two forwards with no synchronise in between: the first one's own copies and the second one's views are both right."""
    from lanegcn_amd.engine import StoreReplay
    from lanegcn_amd.flatfile import StoreCaps
    dev = fx["dev"]
    fresh(net)
    a, b = REPLAY_PICKS[2], REPLAY_PICKS[1]
    want = [net.forward_store_flat(dev, p)[2] for p in (a, b)]
    want = [{k: o[k].clone() for k in ("cls", "reg")} for o in want]
    rp = StoreReplay(net, dev, StoreCaps.for_picks(dev, [a, b]), warm=1)
    rp.forward(a)
    rp.forward(b)                                       # warm-up and capture are behind us
    first = rp.forward(a, own=True)[2]
    second = rp.forward(b)[2]
    torch.cuda.synchronize()
    assert rp.stats["replays"] == 3
    for got, w in ((first, want[0]), (second, want[1])):
        assert torch.equal(got["cls"], w["cls"]) and torch.equal(got["reg"], w["reg"])


def test_miopen_actornet_replay_equals_eager_on_the_same_padded_batch(fx, net):
    """f32 without ActorNet.exact runs ActorNet's convolutions on MIOpen: there the replayed graph is held to the eager
    forward of the SAME padded batch, bitwise.  (MIOpen's default solvers are not repeatable there -- the same input gave
    features 1.4e-6 and reg 3e-5 apart from call to call -- so StoreReplay runs its own forwards, eager and captured, with
    MIOpen's deterministic solvers.)"""
    from lanegcn_amd import lanegcn as M
    from lanegcn_amd import ops
    from lanegcn_amd.engine import StoreReplay
    from lanegcn_amd.flatfile import StoreCaps
    dev = fx["dev"]
    caps = StoreCaps.for_picks(dev, REPLAY_PICKS[:4])
    keep = M.ActorNet.exact
    M.ActorNet.exact = False
    try:
        with ops.mma_scope("f32"):
            fresh(net)
            always_eager, replayed = StoreReplay(net, dev, caps, warm=1000), StoreReplay(net, dev, caps, warm=1)
            for p in REPLAY_PICKS[:4]:
                w = {k: v.clone() for k, v in always_eager.forward(p)[2].items() if k in ("cls", "reg")}
                g = replayed.forward(p)[2]
                assert torch.equal(g["cls"], w["cls"]) and torch.equal(g["reg"], w["reg"]), p
            assert always_eager.stats["eager_warm"] == 4 and replayed.stats["replays"] == 3 and replayed.stats["captures"] == 1
    finally:
        M.ActorNet.exact = keep
        fresh(net)


# ------------------------------------------------------------------ fallbacks
def test_picks_that_do_not_fit_go_the_eager_way(fx, net):
    from lanegcn_amd.engine import StoreReplay
    from lanegcn_amd.flatfile import StoreCaps
    dev = fx["dev"]
    fresh(net)
    small, big, three = [0, 5, 2, 0], [1, 3, 1, 3], [3, 1, 0]
    want = {k: eager(net, dev, p) for k, p in (("small", small), ("big", big), ("three", three))}
    fresh(net)
    rp = StoreReplay(net, dev, StoreCaps.for_picks(dev, [small]), warm=1)
    same_lists(net.forward_store(dev, small, replay=rp), want["small"], "warm")
    same_lists(net.forward_store(dev, big, replay=rp), want["big"], "too large")
    same_lists(net.forward_store(dev, three, replay=rp), want["three"], "length 3")
    same_lists(net.forward_store(dev, small, replay=rp), want["small"], "replay")
    st = rp.stats
    assert (st["eager_nofit"], st["eager_warm"], st["captures"], st["replays"]) == (2, 1, 1, 1), st


def test_pair_overflow_falls_back_and_captures_again(fx, net, monkeypatch):
    """A capture sized for few pairs (HotPathEngine._cap cut to the counts seen, no headroom), then a pick with more:
    its count comes back negative, the pick runs the eager route, the graph is dropped, and the next pick captures again
    with the grown capacity."""
    from lanegcn_amd.engine import HotPathEngine, StoreReplay
    from lanegcn_amd.flatfile import StoreCaps
    dev = fx["dev"]
    small, big = [0, 0, 0, 0], [1, 3, 1, 3]
    fresh(net)
    want = {k: eager(net, dev, p) for k, p in (("small", small), ("big", big))}
    fresh(net)
    monkeypatch.setattr(HotPathEngine, "_cap", lambda self, i: max(8, (self._pair_seen[i] + 7) // 8 * 8))
    rp = StoreReplay(net, dev, StoreCaps.for_picks(dev, [small, big]), warm=1)
    same_lists(net.forward_store(dev, small, replay=rp), want["small"], "warm")
    same_lists(net.forward_store(dev, small, replay=rp), want["small"], "captured for the small pick")
    assert rp.stats["captures"] == 1 and rp.stats["replays"] == 1
    same_lists(net.forward_store(dev, big, replay=rp), want["big"], "overflow")
    assert rp.stats["eager_overflow"] == 1 and rp.stats["replays"] == 1
    same_lists(net.forward_store(dev, big, replay=rp), want["big"], "captured again")
    same_lists(net.forward_store(dev, small, replay=rp), want["small"], "replayed")
    st = rp.stats
    assert (st["captures"], st["replays"], st["eager_overflow"], st["eager_guard"], st["eager_nofit"]) == (2, 3, 1, 0, 0), st
    monkeypatch.undo()
    fresh(net)


def test_range_guard_sends_the_pick_to_the_eager_route(fx, net):
    """A real scene whose lane nodes leave fp16's range in the stem (f16x2): the guard's word is set by REAL rows, the
    pick is rerouted by the eager route as forward_store reroutes it, and the graph stays for the next pick.  ActorNet.exact:
    the re-run in bf16x3 then keeps ActorNet on this library's units, whose results do not depend on the call's history."""
    from lanegcn_amd import lanegcn as M
    from lanegcn_amd import ops
    from lanegcn_amd.engine import StoreReplay
    from lanegcn_amd.flatfile import StoreCaps
    assert ops.get_mma() == "f16x2" and ops.get_guard() == "reroute"
    dev = fx["dev"]
    cool, hot = [3, 1, 1, 0], [3, HOT, 1, 0]
    keep = M.ActorNet.exact
    M.ActorNet.exact = True
    try:
        fresh(net)
        want = {k: eager(net, dev, p) for k, p in (("cool", cool), ("hot", hot))}
        assert all(bool(torch.isfinite(t).all()) for t in want["hot"]["reg"])
        fresh(net)
        rp = StoreReplay(net, dev, StoreCaps.for_picks(dev, [cool, hot]), warm=1)
        same_lists(net.forward_store(dev, cool, replay=rp), want["cool"], "warm")
        same_lists(net.forward_store(dev, cool, replay=rp), want["cool"], "captured")
        same_lists(net.forward_store(dev, hot, replay=rp), want["hot"], "guard")
        same_lists(net.forward_store(dev, cool, replay=rp), want["cool"], "replayed")
    finally:
        M.ActorNet.exact = keep
        fresh(net)
    st = rp.stats
    assert (st["captures"], st["replays"], st["eager_guard"], st["eager_overflow"]) == (1, 2, 1, 0), st


# ------------------------------------------------------------------ errors
def test_errors_are_forward_stores_and_come_before_any_launch(fx, net):
    from lanegcn_amd._lib import LgcnError
    from lanegcn_amd.engine import StoreReplay
    from lanegcn_amd.flatfile import StoreCaps
    dev = fx["dev"]
    bare, empty = [NO_SCALE5] * 4, [SC.NO_ACTORS] * 4
    with pytest.raises(KeyError):
        net.forward_store(dev, bare)
    with pytest.raises(LgcnError):
        net.forward_store(dev, empty)
    caps = StoreCaps.for_picks(dev, [bare, empty, REPLAY_PICKS[0]])
    caps = StoreCaps(caps.batch, caps.nodes, caps.actors, tuple(e + 5 for e in caps.edges))      # filler edges in pre[5] / suc[5] too
    rp = StoreReplay(net, dev, caps, warm=1)
    rp.slot.buf.fill_(0xFF)
    torch.cuda.synchronize()
    before = rp.slot.buf.clone()
    with pytest.raises(KeyError):
        rp.forward(bare)
    with pytest.raises(LgcnError):
        rp.forward(empty)
    with pytest.raises(IndexError):
        rp.forward([0, 1, 2, len(dev)])
    torch.cuda.synchronize()
    assert torch.equal(rp.slot.buf, before) and sum(v for k, v in rp.stats.items() if isinstance(v, int)) == 0
    with pytest.raises(LgcnError):                                      # a StoreReplay of another net
        net.forward_store(dev, REPLAY_PICKS[0], replay=type("R", (), {"net": None, "store": dev})())


# ------------------------------------------------------------------ evaluation
@pytest.mark.parametrize("actors", [False, True])
def test_evaluate_store_with_replay_records_the_same(fx, net, actors):
    from lanegcn_amd.evaluate import evaluate_store
    dev = fx["dev"]
    idx = np.random.default_rng(26).integers(0, 6, 26)                   # six full batches of 4 and one of 2
    fresh(net)
    want = evaluate_store(net, dev, 4, indices=idx, actors=actors)
    fresh(net)
    seen = []
    got = evaluate_store(net, dev, 4, indices=idx, actors=actors, replay=True, on_batch=lambda out, fb, ex: seen.append(fb.n_scenes))
    assert seen == [4] * 6 + [2]
    assert np.array_equal(got.records(), want.records())
    np.testing.assert_equal(got.summary(), want.summary())              # (NaN-aware: a split without an evaluated scene)


def test_train_driver_eval_replay_writes_the_same_predictions(tmp_path, capsys, monkeypatch):
    """train_dp.py --eval --eval-store PATH --eval-replay: the metric lines and the prediction table of the run without
    the flag, through a captured graph (three batches of 2: two eager warm-ups, then a capture and a replay)."""
    import importlib
    from lanegcn_amd import engine
    from lanegcn_amd import lanegcn as M
    from lanegcn_amd.flatfile import write_scenes
    path = str(tmp_path / "six.npz")
    write_scenes(path, SC.make_scenes())
    captures = []
    capture = engine.StoreReplay._capture
    monkeypatch.setattr(engine.StoreReplay, "_capture", lambda self, *a: (captures.append(1), capture(self, *a))[1])
    train_dp = importlib.import_module("train_dp")
    saved = dict(M.config)                # the driver writes into the shared config
    got = {}
    try:
        for flag in ((), ("--eval-replay",)):
            M.config["val_batch_size"] = 2
            preds = str(tmp_path / ("preds%d.npz" % len(flag)))
            assert train_dp.main(["--eval", "--eval-store", path, "--save-preds", preds, "--dataset-len", "4", *flag]) == 0
            lines = capsys.readouterr().out.strip().splitlines()[-3:]
            with np.load(preds) as z:
                got[flag] = (lines, {k: z[k] for k in z.files})
            assert len(captures) == len(flag)
    finally:
        M.config.clear()
        M.config.update(saved)
    (lines, tab), (rlines, rtab) = got[()], got[("--eval-replay",)]
    assert rlines == lines and lines[-1].startswith("evaluated ") and sorted(rtab) == sorted(tab)
    for k in tab:
        assert np.array_equal(rtab[k], tab[k]), k
