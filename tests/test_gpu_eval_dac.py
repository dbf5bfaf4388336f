"""GPU: drivable-area compliance (lgcn_eval_scenes_da, lgcn_eval_actors_da, lgcn_eval_dac_reduce, evaluate.DrivableArea)
against the loop-level model of tests/eval_dac_model.py on its fixture.  The record floats [30] (the bitmask) and [31] are
integers and are compared exactly; the other 30 floats, traj and score are compared bit for bit with what the entries
without a map write from the same inputs (those are held to their own models in test_gpu_eval.py and
test_gpu_eval_actors.py; the flag the model needs is read from there).  DAC_k of a summary is compared exactly with
counts / (k n_dac) in Python: the counts are integers and the one division is the same float64 division."""
import os
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import eval_dac_model as DM

pytestmark = pytest.mark.gpu
SENTINEL = -7.25
SHAPES = [(M, T, H) for M in (1, 6, 8) for T, H in ((30, 30), (30, 7), (64, 64), (64, 7))]
B_MAX = 70                                # more than one workgroup of 4 waves, not a multiple of 4


def bits(x):
    x = x.cpu().numpy() if torch.is_tensor(x) else np.asarray(x)
    return np.ascontiguousarray(x).view(np.uint32)


def cu(x):
    return torch.from_numpy(np.ascontiguousarray(x)).cuda()


def make_batch(M, T, H):
    """B_MAX scenes from the fixture's records (scene i's first actor is record i, cycled), most with one actor, some with
    five, two without any; an agent with an incomplete future (flag 0), one with a NaN in reg (flag 2), one scene of city -1
    (the fixture's last record); a few other actors observed in part.  The first B scenes are a batch of their own."""
    f = DM.fixture(M, T, H, seed=M * 1000 + T * 10 + H)
    A0 = len(f["reg"])
    assert A0 < B_MAX and f["city"][A0 - 1] == -1
    rng = np.random.default_rng(M + T + H)
    n_act = np.ones(B_MAX, np.int64)
    n_act[[4, 11, 40]] = 5
    n_act[[6, B_MAX - 1]] = 0
    off = np.concatenate([[0], np.cumsum(n_act)]).astype(np.int32)
    A = int(off[-1])
    src = np.zeros(A, np.int64)                                            # the fixture record behind every actor row
    scene_of = np.repeat(np.arange(B_MAX), n_act)
    city = f["city"][np.arange(B_MAX) % A0].copy()
    for a in range(A):
        b, i = scene_of[a], a - off[scene_of[a]]
        same = np.nonzero(f["city"] == f["city"][b % A0])[0]               # the other actors: records of the scene's own city
        src[a] = b % A0 if i == 0 else same[(b + 7 * i) % len(same)]
    reg = f["reg"][src].copy()
    gt = (reg[:, 0] + rng.normal(0, 1, (A, T, 2))).astype(np.float32)
    gt[np.abs(gt) > 1e6] = 0.0                                             # next to the 1e30 points: gt itself stays finite (flag 1)
    cls = rng.normal(0, 1, (A, M)).astype(np.float32)
    has = np.ones((A, T), bool)
    has[off[13], H - 1] = False                                            # the agent of scene 13: future not whole
    reg[off[17], M - 1, 0, 0] = np.nan                                     # the agent of scene 17: non-finite
    has[off[4] + 1, :] = False                                             # never observed
    has[off[4] + 2, H // 2:] = False                                       # cut short
    has[off[11] + 3, 0] = False                                            # a hole (with H = 7 still 6 observed steps)
    has[off[40] + 4, :H - 1] = False                                       # the last counted step alone
    return dict(reg=reg, cls=cls, gt=gt, has=has, actor_off=off, city=city.astype(np.int32), scene_of=scene_of, M=M, T=T,
                horizon=H, areas=f["areas"], names=f["names"])


@pytest.fixture(scope="module")
def batches():
    """Every shape's batch with the model's masks of every actor row given flag 1 (computed once, never modified)."""
    out = {}
    for M, T, H in SHAPES:
        c = make_batch(M, T, H)
        A = len(c["reg"])
        c["mask1"], c["has1"] = DM.masks(c["reg"], np.ones(A, np.float32), c["city"][c["scene_of"]], H, c["areas"])
        out[(M, T, H)] = c
    return out


@pytest.fixture(scope="module")
def drivable():
    import lanegcn_amd  # noqa: F401
    from lanegcn_amd.evaluate import DrivableArea
    return DrivableArea(DM.fixture_areas()).to("cuda")


def head(c, B):
    """The first B scenes of batch c as a batch of their own."""
    A = int(c["actor_off"][B])
    d = {k: c[k][:A] for k in ("reg", "cls", "gt", "has", "mask1", "has1", "scene_of")}
    d.update(actor_off=c["actor_off"][:B + 1], city=c["city"][:B], M=c["M"], T=c["T"], horizon=c["horizon"])
    return d


def tables(n, M, T, fill=SENTINEL):
    return (torch.full((n, 32), fill, dtype=torch.float32, device="cuda"), torch.full((n, M, T, 2), fill, dtype=torch.float32, device="cuda"),
            torch.full((n, M), fill, dtype=torch.float32, device="cuda"), torch.zeros(1, dtype=torch.int32, device="cuda"))


def run(c, da=None, actors=False, slot=None, n_slots=None, city=None):
    from lanegcn_amd import ops
    B = len(c["actor_off"]) - 1
    if slot is None:
        slot = c["actor_off"][:-1].astype(np.int64) if actors else np.arange(B, dtype=np.int64)
    n = (len(c["reg"]) if actors else B) if n_slots is None else n_slots
    t = tables(n, c["M"], c["T"])
    args = (cu(c["reg"]), cu(c["cls"]), cu(c["gt"]), cu(c["has"]), cu(c["actor_off"]), cu(np.asarray(slot, np.int64)), c["horizon"]) + t
    if da is None:
        (ops.eval_actors if actors else ops.eval_scenes)(*args)
    else:
        (ops.eval_actors_da if actors else ops.eval_scenes_da)(*args, da, cu(np.asarray(c["city"] if city is None else city, np.int32)))
    return t


def want_dac(plain_rec, mask1, has1):
    """The model's floats [30], [31] of the rows whose record (from the entry without a map) has flag 1."""
    ok = plain_rec[:, 0] == 1.0
    return np.where(ok, mask1, 0.0).astype(np.float32), np.where(ok, has1, 0.0).astype(np.float32)


@pytest.mark.parametrize("B", [1, 3, B_MAX])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "M%d-T%d-H%d" % s)
def test_scene_records(batches, drivable, shape, B):
    c = head(batches[shape], B)
    first = c["actor_off"][:-1].clip(max=max(len(c["reg"]) - 1, 0))
    some = np.diff(c["actor_off"]) > 0
    plain, got = run(c), run(c, drivable)
    assert int(plain[3].item()) == 0 and int(got[3].item()) == 0
    rec0, rec = plain[0].cpu().numpy(), got[0].cpu().numpy()
    assert np.array_equal(bits(rec[:, :30]), bits(rec0[:, :30])) and not rec0[:, 30:].any()
    assert np.array_equal(bits(got[1]), bits(plain[1])) and np.array_equal(bits(got[2]), bits(plain[2]))
    mask, has = want_dac(rec0, np.where(some, c["mask1"][first], 0.0), np.where(some, c["has1"][first], 0.0))
    assert np.array_equal(rec[:, 30], mask) and np.array_equal(rec[:, 31], has), np.nonzero(rec[:, 30] != mask)[0]
    if B == B_MAX:                                                        # every case of the issue is in the batch
        assert (rec0[:, 0] == 0.0).sum() == 3 and rec0[13, 0] == 0.0 and rec0[17, 0] == 2.0 and not rec[[6, 13, 17, B - 1], 1:].any()
        assert (c["city"] == -1).sum() >= 1 and not rec[c["city"] == -1, 30:].any() and (rec[c["city"] == -1, 0] == 1.0).all()
        assert len(set(c["city"][has == 1.0].tolist())) == 2              # the two-city batch
        full = float((1 << shape[0]) - 1)
        assert (mask[has == 1.0] == full).sum() >= 5 and (mask[has == 1.0] != full).sum() >= 20


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "M%d-T%d-H%d" % s)
def test_actor_records(batches, drivable, shape):
    c = batches[shape]
    plain, got = run(c, actors=True), run(c, drivable, actors=True)
    assert int(plain[3].item()) == 0 and int(got[3].item()) == 0
    rec0, rec = plain[0].cpu().numpy(), got[0].cpu().numpy()
    assert np.array_equal(bits(rec[:, :30]), bits(rec0[:, :30])) and not rec0[:, 30:].any()
    assert np.array_equal(bits(got[1]), bits(plain[1])) and np.array_equal(bits(got[2]), bits(plain[2]))
    mask, has = want_dac(rec0, c["mask1"], c["has1"])
    assert np.array_equal(rec[:, 30], mask) and np.array_equal(rec[:, 31], has), np.nonzero(rec[:, 30] != mask)[0]
    off = c["actor_off"]
    assert rec0[off[4] + 1, 0] == 0.0 and rec0[off[17], 0] == 2.0 and (rec0[[off[4] + 2, off[11] + 3, off[40] + 4, off[13]], 0] == 1.0).all()
    assert has[off[13]] == 1.0                                            # has_preds plays no part: the whole trajectory counts
    # the first actor of a scene the agents' entry evaluates: the same two floats
    srec = run(c, drivable)[0].cpu().numpy()
    ev = np.nonzero(srec[:, 0] == 1.0)[0]
    assert np.array_equal(bits(rec[off[ev]]), bits(srec[ev]))


def fake_batch(c):
    fb = SimpleNamespace(n_scenes=len(c["actor_off"]) - 1, n_actors=len(c["reg"]), actor_off=cu(c["actor_off"]))
    return fb, {"gt_preds": cu(c["gt"]), "has_preds": cu(c["has"])}


def part(c, order):
    """The batch `c` reduced to its scenes `order`, in that order."""
    off = c["actor_off"]
    rows = np.concatenate([np.arange(off[b], off[b + 1]) for b in order] + [np.zeros(0, np.int64)]).astype(np.int64)
    d = {k: c[k][rows] for k in ("reg", "cls", "gt", "has")}
    d.update(actor_off=np.concatenate([[0], np.cumsum([off[b + 1] - off[b] for b in order])]).astype(np.int32))
    return d


def feed(ev, c, groups):
    for g in groups:
        d = part(c, g)
        fb, ex = fake_batch(d)
        ev.update(cu(d["reg"]), cu(d["cls"]), fb, ex, np.asarray(g, np.int64))


def test_actor_evaluator_selections(batches, drivable):
    """Scenes of 0, 1 and 5 actors: every who, min_obs in {1, horizon}; DAC_k = counts / (k n_dac), exactly."""
    from lanegcn_amd.evaluate import ActorEvaluator
    M, T, H = 6, 30, 7
    c = batches[(M, T, H)]
    names = [None if i < 0 else c["names"][i] for i in c["city"]]          # by name, None for the scene without a map
    ev = ActorEvaluator(c["actor_off"], M, T, horizon=H, drivable=drivable, scene_city=names)
    feed(ev, c, [list(range(0, 30)), list(range(30, B_MAX))])
    rec = ev.records()
    assert sorted(set(np.diff(c["actor_off"]).tolist())) == [0, 1, 5]
    mask, has = want_dac(rec, c["mask1"], c["has1"])
    assert np.array_equal(rec[:, 30], mask) and np.array_equal(rec[:, 31], has)
    seen = set()
    for who in ("all", "agent", "others"):
        for min_obs in (1, H):
            keep = (rec[:, 28] <= H - min_obs) & {"all": rec[:, 3] >= 0, "agent": rec[:, 3] == 0, "others": rec[:, 3] > 0}[who]
            counts, n = DM.counts(mask, has, M, keep)
            got = ev.summary(ks=(6, 3, 1), who=who, min_obs=min_obs)
            assert got["n_dac"] == n and n > 0, (who, min_obs)
            assert list(got[6]) == ["minADE", "minFDE", "MR", "p-minADE", "brier-minADE", "brier-minFDE", "DAC"]
            for k in (6, 3, 1):
                assert got[k]["DAC"] == counts[k - 1] / (k * n), (who, min_obs, k)
            assert 0.0 < got[6]["DAC"] < 1.0                                # compliant and other modes among the counted ones
            seen.add((n, tuple(counts)))
    assert len(seen) == 6                                                 # every selection counts other records
    # the same table without a map: every other number of the summary is the same, DAC is absent
    plain = ActorEvaluator(c["actor_off"], M, T, horizon=H)
    feed(plain, c, [list(range(B_MAX))])
    a, b = ev.summary(who="others"), plain.summary(who="others")
    assert "DAC" not in b[6] and "n_dac" not in b and plain._status.numel() == 448
    assert a.pop("n_dac") > 0 and all(0.0 <= a[k].pop("DAC") <= 1.0 for k in (6, 1))
    assert repr(a) == repr(b)


def test_summary_is_independent_of_batching_and_makes_one_read(batches, drivable, monkeypatch):
    from lanegcn_amd.evaluate import Evaluator
    M, T, H = 8, 64, 7
    c = batches[(M, T, H)]
    one = Evaluator(B_MAX, M, T, horizon=H, drivable=drivable, scene_city=c["city"])
    two = Evaluator(B_MAX, M, T, horizon=H, drivable=drivable, scene_city=c["city"])
    feed(one, c, [list(range(B_MAX))])
    order = np.random.default_rng(2).permutation(B_MAX).tolist()
    feed(two, c, [order[:1], order[1:4], order[4:33], order[33:]])
    assert np.array_equal(bits(one.rec), bits(two.rec))
    reads = []
    real = torch.Tensor.cpu
    monkeypatch.setattr(torch.Tensor, "cpu", lambda t, *a, **k: (reads.append(tuple(t.shape)), real(t, *a, **k))[1])
    s1, s2 = one.summary(ks=tuple(range(1, M + 1))), two.summary(ks=tuple(range(1, M + 1)))
    monkeypatch.undo()
    assert reads == [(528,), (528,)]                                      # the status buffer, once per summary
    assert repr(s1) == repr(s2)
    rec = one.records()
    first = c["actor_off"][:-1].clip(max=len(c["reg"]) - 1)
    some = np.diff(c["actor_off"]) > 0
    mask, has = want_dac(rec, np.where(some, c["mask1"][first], 0.0), np.where(some, c["has1"][first], 0.0))
    counts, n = DM.counts(mask, has, M)
    assert s1["n_dac"] == n == int((rec[:, 31] == 1.0).sum()) and s1["n_evaluated"] == n + int((c["city"][rec[:, 0] == 1.0] == -1).sum())
    for k in range(1, M + 1):
        assert s1[k]["DAC"] == counts[k - 1] / (k * n), k
    # nothing counted: NaN
    none = Evaluator(B_MAX, M, T, horizon=H, drivable=drivable, scene_city=[None] * B_MAX)
    feed(none, c, [list(range(B_MAX))])
    s0 = none.summary()
    assert s0["n_dac"] == 0 and np.isnan(s0[1]["DAC"]) and s0["n_evaluated"] == s1["n_evaluated"] and s0[1]["minFDE"] == s1[1]["minFDE"]
    assert not none.records()[:, 30:].any()


def test_argument_errors_are_flagged_and_raise_at_summary(batches, drivable):
    """A city id the table does not hold and a slot outside the table: both set err, neither touches another row."""
    from lanegcn_amd._lib import LgcnError
    from lanegcn_amd.evaluate import ActorEvaluator, Evaluator
    M, T, H = 6, 30, 30
    c = head(batches[(M, T, H)], 12)
    good = run(c, drivable)[0].cpu().numpy()
    plain = run(c)[0].cpu().numpy()
    city = c["city"].copy()
    city[[2, 5]] = 2, 1 << 20                                             # n_cities = 2
    rec, traj, score, err = run(c, drivable, city=city)
    rec = rec.cpu().numpy()
    assert int(err.item()) == 1
    rest = [b for b in range(12) if b not in (2, 5)]
    assert np.array_equal(bits(rec[rest]), bits(good[rest]))
    assert np.array_equal(bits(rec[[2, 5]]), bits(plain[[2, 5]])) and not rec[[2, 5], 30:].any()      # the record, without DAC
    arec = run(c, drivable, actors=True, city=city)
    assert int(arec[3].item()) == 1
    rows = np.concatenate([np.arange(c["actor_off"][b], c["actor_off"][b + 1]) for b in (2, 5)])
    assert not arec[0].cpu().numpy()[rows, 30:].any()
    # a slot outside the table: nothing is written for that scene, the others are as before
    slot = np.arange(12, dtype=np.int64)
    slot[3], slot[8] = 12, -1
    rec, traj, score, err = run(c, drivable, slot=slot)
    assert int(err.item()) == 1
    rest = [b for b in range(12) if b not in (3, 8)]
    assert np.array_equal(bits(rec[rest]), bits(good[rest])) and bool((rec[[3, 8]] == SENTINEL).all())
    assert bool((traj[[3, 8]] == SENTINEL).all()) and bool((score[[3, 8]] == SENTINEL).all())
    # the public interface raises at summary()
    fb, ex = fake_batch(c)
    ev = Evaluator(12, M, T, drivable=drivable, scene_city=c["city"])
    ev.update(cu(c["reg"]), cu(c["cls"]), fb, ex, np.arange(12))
    assert ev.summary()["n_dac"] > 0
    ev.scene_city[4] = 2                                                  # past the validation at construction
    ev.update(cu(c["reg"]), cu(c["cls"]), fb, ex, np.arange(12))
    with pytest.raises(LgcnError):
        ev.summary()
    ev2 = Evaluator(12, M, T, drivable=drivable, scene_city=c["city"])
    ev2.update(cu(c["reg"]), cu(c["cls"]), fb, ex, slot)
    with pytest.raises(LgcnError):
        ev2.summary()
    assert np.array_equal(bits(ev2.rec[rest]), bits(good[rest])) and not ev2.rec[[3, 8]].any()
    av = ActorEvaluator(c["actor_off"], M, T, drivable=drivable, scene_city=c["city"])
    av.scene_city[0] = 7
    av.update(cu(c["reg"]), cu(c["cls"]), fb, ex, np.arange(12))
    with pytest.raises(LgcnError):
        av.summary()


def test_dac_reduce_counts(drivable):
    """lgcn_eval_dac_reduce alone on generated tables: sizes around the 1,024 threads, M below 8, every flag."""
    from lanegcn_amd import ops
    for n, M in ((1, 8), (1023, 6), (1024, 1), (1025, 8), (5000, 6)):
        rng = np.random.default_rng(n)
        rec = np.zeros((n, 32), np.float32)
        rec[:, 0] = rng.choice([0.0, 1.0, 1.0, 1.0, 2.0], n)
        rec[:, 1], rec[:, 2] = M, 30
        rec[:, 3] = rng.integers(0, 3, n)
        rec[:, 28] = rng.integers(0, 30, n)
        rec[:, 30] = rng.integers(0, 1 << M, n)
        rec[:, 31] = rng.integers(0, 2, n)
        for who, max_missing in ((0, 64), (1, 29), (2, 0), (0, 10)):
            keep = (rec[:, 0] == 1.0) & (rec[:, 28] <= max_missing) & [rec[:, 3] >= 0, rec[:, 3] == 0, rec[:, 3] > 0][who]
            counts, cnt = DM.counts(rec[:, 30], rec[:, 31], M, keep)
            dac = torch.full((9,), -1, dtype=torch.int64, device="cuda")
            ops.eval_dac_reduce(cu(rec), who, max_missing, dac)
            assert dac.tolist() == counts + [0] * (8 - M) + [cnt], (n, M, who, max_missing)


@pytest.fixture(scope="module")
def e2e(tmp_path_factory):
    """A store of 6 small synthetic scenes (scene 1 holds no actor), a randomly initialised Net, and a map per scene
    around it; the last scene has no map."""
    import lanegcn_amd  # noqa: F401
    from lanegcn_amd import data as gen
    from lanegcn_amd import lanegcn as M
    from lanegcn_amd.evaluate import DrivableArea
    from lanegcn_amd.flatfile import DeviceSceneStore, write_scenes
    rng = np.random.default_rng(11)
    scenes = [gen.synth_scene(rng, [4, 4] if i % 2 else [5], n) for i, n in enumerate([5, 0, 9, 1, 7, 3])]
    path = str(tmp_path_factory.mktemp("eval_dac") / "split.npz")
    write_scenes(path, scenes)
    store = DeviceSceneStore(path)
    torch.manual_seed(0)
    net = M.Net(M.config).cuda().eval()
    # a city per scene, rasters of different sizes; the odd ones are drivable but for the cell where mode 0 of their scene
    # ends (that mode leaves the road there, whatever the others do), the even ones everywhere inside
    from lanegcn_amd.evaluate import Evaluator, evaluate_store
    sc = ["c0", "c1", "c2", "c3", "c4", None]
    traj = evaluate_store(net, store, 2, evaluator=Evaluator(6, 6, 30, keep_preds=True)).traj.cpu().numpy()
    maps = {}
    for i, c in enumerate(sc[:5]):
        mat, tx, ty = np.ones((600 + 10 * i, 500 - 10 * i), np.uint8 if i % 2 else np.float32), 250. - i, 300. + i
        if i % 2:
            x, y = np.rint(traj[i, 0, 29])
            mat[int(y + ty), int(x + tx)] = 0
        maps[c] = (mat, np.array([[1., 0., tx], [0., 1., ty], [0., 0., 1.]]))
    da = DrivableArea(maps)
    return dict(store=store, net=net, da=da, scene_city=sc, path=path)


def test_evaluate_store_end_to_end_eager_and_replay(e2e):
    from lanegcn_amd.evaluate import Evaluator, evaluate_store
    net, store, da, sc = e2e["net"], e2e["store"], e2e["da"], e2e["scene_city"]
    eager = evaluate_store(net, store, 2, drivable=da, scene_city=sc)
    replay = evaluate_store(net, store, 2, drivable=da, scene_city=sc, replay=True)
    assert type(eager) is Evaluator and eager.drivable is da
    assert np.array_equal(bits(eager.rec), bits(replay.rec))
    s = eager.summary()
    assert repr(s) == repr(replay.summary()) and s["n_dac"] == 4 and s["n_evaluated"] == 5
    # against the model, from the kept predictions
    kept = Evaluator(6, 6, 30, keep_preds=True, drivable=da, scene_city=sc)
    assert evaluate_store(net, store, 2, evaluator=kept) is kept           # the same batches: the same forward, bit for bit
    rec = kept.records()
    assert np.array_equal(bits(rec), bits(eager.rec))
    ids = kept.scene_city
    areas = [(da.raster[t.off:t.off + t.h * t.w].reshape(t.h, t.w), np.array(list(t.m) + [0., 0., 1.]).reshape(3, 3)) for t in da.table]
    mask, has = DM.masks(kept.traj.cpu().numpy(), rec[:, 0], ids, 30, areas)
    assert np.array_equal(rec[:, 30], mask) and np.array_equal(rec[:, 31], has) and has.tolist() == [1, 0, 1, 1, 1, 0]
    counts, n = DM.counts(mask, has, 6)
    print("end to end: masks", mask.tolist(), "counts", counts, "n_dac", n)
    assert s[6]["DAC"] == counts[5] / (6 * n) and s[1]["DAC"] == counts[0] / n
    assert [int(m) for m in mask[[0, 2, 4]]] == [63, 63, 63] and int(mask[3]) & 1 == 0      # see the fixture's maps
    # every actor of the split
    every = evaluate_store(net, store, 2, actors=True, drivable=da, scene_city=sc)
    sa = every.summary(who="agent", min_obs=30)
    assert sa["n_dac"] == 4 and sa[6]["DAC"] == s[6]["DAC"] and sa[1]["DAC"] == s[1]["DAC"]
    assert every.summary()["n_dac"] == 5 + 9 + 1 + 7
    # without a map: the records of before, nothing in [30], [31]
    plain = evaluate_store(net, store, 2)
    assert np.array_equal(bits(plain.rec[:, :30]), bits(eager.rec[:, :30])) and not plain.rec[:, 30:].any()
    assert "DAC" not in plain.summary()[6]


def test_train_driver_prints_dac(e2e, tmp_path, capsys):
    """train_dp.py --eval --eval-store --eval-drivable FILE.npz: DAC behind the six metrics of every K."""
    import importlib
    import re
    from lanegcn_amd import lanegcn as M
    train_dp = importlib.import_module("train_dp")
    da = e2e["da"]
    npz = str(tmp_path / "drivable.npz")
    arrays = {"cities": np.array(da.cities), "scene_city": np.array([0, 1, 2, 3, 4, -1], np.int32)}
    for t, c in zip(da.table, da.cities):
        arrays["raster/" + c] = da.raster[t.off:t.off + t.h * t.w].reshape(t.h, t.w)
        arrays["se2/" + c] = np.array(list(t.m) + [0., 0., 1.]).reshape(3, 3)
    np.savez(npz, **arrays)
    saved = dict(M.config)
    try:
        assert train_dp.main(["--eval", "--eval-store", e2e["path"], "--eval-drivable", npz, "--dataset-len", "4"]) == 0
    finally:
        M.config.clear()
        M.config.update(saved)
    k6, k1, tail = capsys.readouterr().out.strip().splitlines()[-3:]
    keys = "minADE, minFDE, MR, p-minADE, brier-minADE, brier-minFDE, DAC".split(", ")
    for line, k in ((k6, 6), (k1, 1)):
        assert line.startswith("K=%d " % k) and re.findall(r"([A-Za-z-]+) \d+\.\d{4}", line) == keys, line
    assert tail == "evaluated 5 scenes, skipped 1, non-finite 0"


def test_build_store_leaves_the_cities_on_the_store():
    import copy
    import scene_build_cases as C
    from conftest import GOLDEN_DIR
    from lanegcn_amd import data_raw as D
    from lanegcn_amd import lanegcn as M
    from lanegcn_amd.evaluate import DrivableArea, evaluate_store
    from lanegcn_amd.flatfile import DeviceSceneStore
    raws, tables, lane_ids, _ = C.load_fixture(os.path.join(GOLDEN_DIR, "scene_build_b4.npz"))
    raws, lane_ids = raws[:3], lane_ids[:3]
    tables = {k: v.to("cuda") for k, v in tables.items()}
    store = D.build_store(copy.deepcopy(raws), tables, C.CONFIG, lane_ids=lane_ids)
    assert store.scene_city == [r["city"] for r in raws]
    parts = [D.build_store(copy.deepcopy(raws[a:b]), tables, C.CONFIG, lane_ids=lane_ids[a:b]) for a, b in ((0, 1), (1, 3))]
    whole = DeviceSceneStore.concat(parts)
    assert whole.scene_city == store.scene_city
    parts[0].scene_city = None
    assert DeviceSceneStore.concat(parts).scene_city is None
    cities = sorted(set(store.scene_city), reverse=True)                  # an order of its own: the ids follow the DrivableArea
    da = DrivableArea({c: (np.ones((50, 60)), np.eye(3)) for c in cities})
    torch.manual_seed(0)
    net = M.Net(dict(M.config, **C.CONFIG)).cuda().eval()
    ev = evaluate_store(net, store, 3, drivable=da)
    assert ev.scene_city.tolist() == [cities.index(c) for c in store.scene_city]
    assert ev.summary()["n_dac"] == ev.summary()["n_evaluated"]
