"""GPU: the per-actor evaluation (lgcn_eval_actors, lgcn_eval_reduce_sel, evaluate.ActorEvaluator) against the float64 model
of tests/eval_actors_model.py on the generated cases of tests/eval_actors_cases.py.

Tolerances are those tests/test_gpu_eval.py derives, unchanged because n_obs <= horizon: |minFDE - model| <= 8 * 2^-24 *
model, |minADE - model| <= (horizon + 8) * 2^-24 * model, p_k within 4 x the error of the same formula in numpy float32
(floor 1e-6, relative); flags and the floats [1..3], [28], [29] exact, everything else zero.  The selected reduce equals its
float64 model within 1e-12 relative with exact counts, and lgcn_eval_reduce on the zeroed copy bit for bit.  The agents'
summary of an ActorEvaluator equals Evaluator.summary() within 1e-12 relative (the two tables put an agent on different
threads of the reduce), n_evaluated exactly."""
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import eval_actors_cases as AC
import eval_actors_model as AM
import eval_model as EM

pytestmark = pytest.mark.gpu
SENTINEL = -7.25


@pytest.fixture(scope="module")
def cases():
    """Every generated case with the model's records (computed once, never modified)."""
    out = {}
    for c in AC.CASES:
        d = AC.make_case(*c)
        d["want"] = AM.records(d["reg"], d["cls"], d["gt"], d["has"], d["actor_off"], d["horizon"])
        out[c] = d
    return out


def bits(x):
    x = x.cpu().numpy() if torch.is_tensor(x) else np.asarray(x)
    return np.ascontiguousarray(x).view(np.uint32)


def cu(x):
    return torch.from_numpy(np.ascontiguousarray(x)).cuda()


def tables(n_slots, M, T, keep=True, fill=0.0):
    rec = torch.full((n_slots, 32), fill, dtype=torch.float32, device="cuda")
    traj = torch.full((n_slots, M, T, 2), fill, dtype=torch.float32, device="cuda") if keep else None
    score = torch.full((n_slots, M), fill, dtype=torch.float32, device="cuda") if keep else None
    return rec, traj, score, torch.zeros(1, dtype=torch.int32, device="cuda")


def launch_into(c, slot_base, rec, traj, score, err):
    from lanegcn_amd import ops
    ops.eval_actors(cu(c["reg"]), cu(c["cls"]), cu(c["gt"]), cu(c["has"]), cu(c["actor_off"]), cu(np.asarray(slot_base, np.int64)),
                    c["horizon"], rec, traj, score, err)


def launch(c, slot_base=None, n_slots=None, keep=True, fill=0.0):
    """One lgcn_eval_actors launch of the batch `c` into fresh tables (default: row = the batch's own actor row)."""
    slot_base = c["actor_off"][:-1] if slot_base is None else slot_base
    t = tables(len(c["reg"]) if n_slots is None else n_slots, c["M"], c["T"], keep, fill)
    launch_into(c, slot_base, *t)
    return t


def p_bar(c, want):
    """4 x the largest relative error of p_k by the same formula in numpy float32 against the model, floor 1e-6."""
    H, worst = c["horizon"], 0.0
    for a in np.nonzero(want[:, 0] == 1.0)[0]:
        t_last = H - 1 - int(want[a, 29])
        gt = np.nan_to_num(c["gt"][a])                                    # unobserved steps hold NaN; the yardstick reads t_last alone
        p32 = AM.record_f32(c["reg"][a], c["cls"][a], gt, t_last).astype(np.float64)
        p = want[a, 6:6 + 3 * c["M"]:3]
        worst = max(worst, float(np.max(np.abs(p32 - p) / p)))
    return max(4 * worst, 1e-6)


def check(got, want, c, what):
    M, H = c["M"], c["horizon"]
    bar = p_bar(c, want)
    w = AC.worst(got, want, M)
    print("%s: worst relative error minFDE %.3g (bar %.3g) minADE %.3g (bar %.3g) p %.3g (bar %.3g)"
          % (what, w[0], 8 * AC.EPS, w[1], (H + 8) * AC.EPS, w[2], bar))
    assert AC.outside_bars(got, want, M, H, bar) == [], what


def subset(c, order):
    """The batch `c` reduced to its scenes `order`, in that order."""
    off = c["actor_off"]
    rows = np.concatenate([np.arange(off[b], off[b + 1]) for b in order] + [np.zeros(0, np.int64)]).astype(np.int64)
    d = {k: c[k][rows] for k in ("reg", "cls", "gt", "has")}
    d.update(actor_off=np.concatenate([[0], np.cumsum([off[b + 1] - off[b] for b in order])]).astype(np.int32),
             M=c["M"], T=c["T"], horizon=c["horizon"])
    return d


@pytest.mark.parametrize("case", AC.CASES, ids=AC.case_id)
def test_kernel_against_the_model(cases, case):
    c = cases[case]
    want = c["want"]
    rec, traj, score, err = launch(c, fill=SENTINEL)
    assert int(err.item()) == 0
    check(rec.cpu().numpy(), want, c, AC.case_id(case))
    for a in range(len(want)):
        if want[a, 0] >= 1.0:
            assert np.array_equal(bits(traj[a]), bits(c["reg"][a])) and np.array_equal(bits(score[a]), bits(c["cls"][a]))
        else:                                                             # no prediction is kept of an actor that was not evaluated
            assert bool((traj[a] == SENTINEL).all()) and bool((score[a] == SENTINEL).all())
    rec2 = launch(c, keep=False)[0]                                       # without the prediction tables: the same records
    assert np.array_equal(bits(rec2), bits(rec))


@pytest.mark.parametrize("case", AC.CASES, ids=AC.case_id)
def test_a_fully_observed_first_actor_is_the_scene_record(cases, case):
    from lanegcn_amd import ops
    c = cases[case]
    M, T, H = c["M"], c["T"], c["horizon"]
    B = len(c["actor_off"]) - 1
    rec = launch(c)[0].cpu().numpy()
    srec, straj, sscore, serr = tables(B, M, T)
    ops.eval_scenes(cu(c["reg"]), cu(c["cls"]), cu(c["gt"]), cu(c["has"]), cu(c["actor_off"]), cu(np.arange(B, dtype=np.int64)), H,
                    srec, straj, sscore, serr)
    srec = srec.cpu().numpy()
    full = [b for b in range(B) if c["actor_off"][b + 1] > c["actor_off"][b] and c["has"][c["actor_off"][b], :H].all()]
    assert full and all(srec[b, 0] == 1.0 for b in full)
    for b in full:
        assert np.array_equal(bits(rec[c["actor_off"][b]]), bits(srec[b])), b
    assert not srec[[b for b in range(B) if b not in full]].any()          # a partly observed agent: nothing there, a record here


def test_flags(cases):
    """One scene of variations of the same fully observed actor (M 6, T 30, horizon 10)."""
    M, T, H = 6, 30, 10
    base = cases[(6, 30, 10, "single")]
    assert base["has"][0, :H].all()
    nan, inf = np.nan, np.inf
    edits = [("has", (H - 1,), False, 1), ("has", (H,), False, 1), ("reg", (3, H - 1, 0), nan, 2), ("reg", (0, 0, 1), inf, 2),
             ("cls", (M - 1,), nan, 2), ("cls", (0,), -inf, 2), ("gt", (H - 1, 1), nan, 2), ("gt", (0, 0), inf, 2),
             ("reg", (5, H, 0), nan, 1), ("gt", (T - 1, 1), inf, 1), ("has", (0,), False, 1), (None, None, None, 1),
             ("reg", (2, T - 1, 1), -inf, 1), ("has", (T - 1,), False, 1),
             ("gt+has", (4, 0), nan, 1), ("gt", (4, 0), nan, 2), ("has", slice(0, H), False, 0), ("reg-unobserved", (1, 4, 1), nan, 2)]
    n = len(edits)
    c = {k: np.repeat(base[k][0:1], n, 0).copy() for k in ("reg", "cls", "gt", "has")}
    for i, (name, at, val, _) in enumerate(edits):
        if name == "gt+has":                                              # a NaN in gt at a step that is not observed: never looked at
            c["gt"][(i,) + at] = val
            c["has"][i, at[0]] = False
        elif name == "reg-unobserved":                                    # reg counts at every step < horizon, observed or not
            c["reg"][(i,) + at] = val
            c["has"][i, at[1]] = False
        elif name == "has":
            c["has"][i, at] = val
        elif name is not None:
            c[name][(i,) + at] = val
    c.update(actor_off=np.array([0, n], np.int32), M=M, T=T, horizon=H)
    want = AM.records(c["reg"], c["cls"], c["gt"], c["has"], c["actor_off"], H)
    assert want[:, 0].tolist() == [float(f) for *_, f in edits]
    assert want[0, 28:30].tolist() == [1.0, 1.0] and want[10, 28:30].tolist() == [1.0, 0.0] and want[14, 28:30].tolist() == [1.0, 0.0]
    rec, traj, score, err = launch(c, fill=SENTINEL)
    assert int(err.item()) == 0
    check(rec.cpu().numpy(), want, c, "flags")
    for i, (*_, flag) in enumerate(edits):
        if flag == 0:
            assert bool((traj[i] == SENTINEL).all()) and bool((score[i] == SENTINEL).all())
        else:
            assert np.array_equal(bits(traj[i]), bits(c["reg"][i])) and np.array_equal(bits(score[i]), bits(c["cls"][i]))


def test_tables_untouched_slots_permutation_and_split(cases):
    c = cases[(6, 30, 10, "mixed")]
    M, T = c["M"], c["T"]
    off, B = c["actor_off"].astype(np.int64), len(c["actor_off"]) - 1
    # the scenes at scattered bases of a larger table, 3 free rows in front of each
    base = off[:-1] + 3 * (np.arange(B) + 1)
    n_slots = int(off[-1]) + 3 * (B + 1)
    rows = np.concatenate([base[b] + np.arange(off[b + 1] - off[b]) for b in range(B)]).astype(np.int64)
    one = launch(c, base, n_slots, fill=SENTINEL)
    assert int(one[3].item()) == 0
    rest = np.setdiff1d(np.arange(n_slots), rows)
    assert len(rest) == 3 * (B + 1)
    assert all(bool((t[rest] == SENTINEL).all()) for t in one[:3])
    check(one[0][rows].cpu().numpy(), c["want"], c, "scattered bases")
    # the scenes in another order, and in two launches: the same tables
    order = np.array([5, 0, 2, 7, 6, 1, 3, 4])
    perm = launch(subset(c, order), base[order], n_slots, fill=SENTINEL)
    two = tables(n_slots, M, T, fill=SENTINEL)
    for part in (np.arange(0, 3), np.arange(3, B)):
        launch_into(subset(c, part), base[part], *two)
    single = tables(n_slots, M, T, fill=SENTINEL)
    launch_into(subset(c, [5]), base[[5]], *single)                       # a batch of one scene (9 actors)
    for other, what in ((perm, "permuted"), (two, "two batches")):
        for x, y, name in zip(one[:3], other[:3], ("rec", "traj", "score")):
            assert np.array_equal(bits(x), bits(y)), (what, name)
        assert int(other[3].item()) == 0
    mine = base[5] + np.arange(9)
    assert np.array_equal(bits(single[0][mine]), bits(one[0][mine]))
    assert bool((single[0][np.setdiff1d(np.arange(n_slots), mine)] == SENTINEL).all()) and int(single[3].item()) == 0


def test_a_slot_outside_the_table_is_flagged_and_not_written(cases):
    from lanegcn_amd._lib import LgcnError
    from lanegcn_amd.evaluate import ActorEvaluator
    c = cases[(6, 30, 30, "mixed")]
    A = len(c["reg"])
    good = launch(c)[0]
    assert c["actor_off"].tolist() == [0, 0, 1, 6, 6, 6, 15, 18, 18]
    # scene 5 (9 actors, rows 6..14) pushed so that its last 4 rows fall off the end; scene 6 (3 actors, rows 15..17) at a
    # negative base, so that only its last actor has a slot; scene 1 (row 0) moved out of that actor's way
    base = c["actor_off"][:-1].astype(np.int64)
    base[1], base[5], base[6] = 6, A - 5, -2
    rec, traj, score, err = launch(c, base, A, fill=SENTINEL)
    assert int(err.item()) == 1
    src = np.concatenate([[0], np.arange(1, 6), np.arange(6, 11), [17]])      # the batch rows that have a slot ...
    dst = np.concatenate([[6], np.arange(1, 6), np.arange(A - 5, A), [0]])    # ... and the slot of each
    landed = {int(d): int(s) for s, d in zip(src, dst)}
    assert len(landed) == 12
    for d, s in landed.items():
        assert np.array_equal(bits(rec[d]), bits(good[s])), (d, s)
    rest = [i for i in range(A) if i not in landed]
    assert bool((rec[rest] == SENTINEL).all()) and bool((traj[rest] == SENTINEL).all()) and bool((score[rest] == SENTINEL).all())
    # the public interface: a batch whose actor count is not the table's is refused on the host
    d = subset(c, [1, 2])
    fb = SimpleNamespace(n_scenes=2, n_actors=int(d["actor_off"][-1]), actor_off=cu(d["actor_off"]))
    ex = {"gt_preds": cu(d["gt"]), "has_preds": cu(d["has"])}
    ev = ActorEvaluator(c["actor_off"], 6, 30)
    with pytest.raises(LgcnError):
        ev.update(cu(d["reg"]), cu(d["cls"]), fb, ex, [2, 5])             # scenes of 5 and 9 actors; the batch holds 1 + 5
    with pytest.raises(LgcnError):
        ev.update(cu(d["reg"]), cu(d["cls"]), fb, ex, [1, 8])             # no such scene
    with pytest.raises(LgcnError):
        ev.update(cu(d["reg"]), cu(d["cls"]), fb, {}, [1, 2])             # a batch without ground truth
    assert not ev.rec.any()
    ev.update(cu(d["reg"]), cu(d["cls"]), fb, ex, [1, 2])
    assert np.array_equal(bits(ev.rec[:6]), bits(good[:6])) and not ev.rec[6:].any()
    # a device actor_off that disagrees with the split's (same total, other cut): rows past a scene's slots are flagged
    fb.actor_off = cu(np.array([0, 6, 6], np.int32))
    ev2 = ActorEvaluator(np.array([0, 1, 6], np.int64), 6, 30)
    ev2.update(cu(d["reg"]), cu(d["cls"]), fb, ex, [0, 1])                # scene 0 claims 6 rows at base 0: all inside the table
    ev2.summary()
    fb.actor_off = cu(np.array([0, 0, 6], np.int32))
    ev2.update(cu(d["reg"]), cu(d["cls"]), fb, ex, [0, 1])                # scene 1 claims 6 rows at base 1: the last falls off
    with pytest.raises(LgcnError):
        ev2.summary()


def reduce_sel_on_device(rec, who, max_missing, miss_thr=2.0):
    from lanegcn_amd import ops
    out = torch.full((8, 6), -1.0, dtype=torch.float64, device="cuda")
    cnt = torch.full((4,), -1, dtype=torch.int64, device="cuda")
    err = torch.zeros(1, dtype=torch.int32, device="cuda")
    ops.eval_reduce_sel(torch.from_numpy(rec).cuda(), miss_thr, AM.WHO[who], max_missing, out, cnt, err)
    return out.cpu().numpy(), cnt.cpu().numpy(), int(err.item())


def reduce_on_device(rec, miss_thr=2.0):
    from lanegcn_amd import ops
    out = torch.full((8, 6), -1.0, dtype=torch.float64, device="cuda")
    cnt = torch.full((3,), -1, dtype=torch.int64, device="cuda")
    err = torch.zeros(1, dtype=torch.int32, device="cuda")
    ops.eval_reduce(torch.from_numpy(rec).cuda(), miss_thr, out, cnt, err)
    return out.cpu().numpy(), cnt.cpu().numpy(), int(err.item())


@pytest.mark.parametrize("n_slots", [1, 127, 128, 129, 6 * 128 + 5])
def test_selected_reduce(n_slots):
    M, H = 6, 30
    rec = AC.make_records(n_slots, M, H, seed=n_slots)
    if n_slots == 1:
        rec[0] = 0.0
        rec[0, :3] = 1.0, M, H
        rec[0, 4:4 + 3 * M] = np.tile([1.5, 1.25, 0.25], M)
    for who in ("all", "agent", "others"):
        for max_missing in (0, H - 1):
            want, want_cnt = AM.reduce_sel(rec, who, max_missing, AC.MISS_THR)
            out, cnt, err = reduce_sel_on_device(rec, who, max_missing)
            what = (n_slots, who, max_missing)
            assert err == 0 and cnt.tolist() == want_cnt.tolist() and cnt.sum() == n_slots, what
            assert np.array_equal(out[:, 2], want[:, 2]) and not out[M:].any(), what      # MR numerators: exact
            assert np.all(np.abs(out - want) <= 1e-12 * np.abs(want)), what
            zero = AM.zeroed(rec, who, max_missing)
            out0, cnt0, err0 = reduce_on_device(zero)
            assert np.array_equal(out.view(np.uint64), out0.view(np.uint64)), what        # bit for bit the plain reduce of the zeroed copy
            assert err0 == 0 and cnt0[1:].tolist() == cnt[1:3].tolist() and cnt0[0] == cnt[0] + cnt[3], what
    # nothing excluded: the plain reduce of the table itself, counts included
    out, cnt, _ = reduce_sel_on_device(rec, "all", H - 1)
    out0, cnt0, _ = reduce_on_device(rec)
    assert np.array_equal(out.view(np.uint64), out0.view(np.uint64)) and cnt[:3].tolist() == cnt0.tolist() and cnt[3] == 0


def test_mixed_records_raise_only_when_kept():
    M, H = 6, 30
    rec = AC.make_records(129, M, H, seed=3)
    others = np.nonzero((rec[:, 0] == 1.0) & (rec[:, 3] > 0))[0]
    rec[others[0], 1] = M - 1                                             # one evaluated record of another M, not an agent
    assert reduce_sel_on_device(rec, "all", H - 1)[2] == 1 and reduce_sel_on_device(rec, "others", H - 1)[2] == 1
    assert reduce_sel_on_device(rec, "agent", H - 1)[2] == 0


@pytest.fixture(scope="module")
def e2e(tmp_path_factory):
    """A store of 6 small synthetic scenes (scene 1 holds no actor) in which has_preds of some actors that are not the agent
    was edited before write_scenes, a randomly initialised Net, and both evaluators of the same store."""
    import lanegcn_amd  # noqa: F401
    from lanegcn_amd import data as gen
    from lanegcn_amd import lanegcn as M
    from lanegcn_amd.evaluate import Evaluator, evaluate_store
    from lanegcn_amd.flatfile import DeviceSceneStore, write_scenes
    rng = np.random.default_rng(11)
    actors = [5, 0, 9, 1, 7, 3]
    scenes = [gen.synth_scene(rng, [4, 4] if i % 2 else [5], n) for i, n in enumerate(actors)]
    has = [np.array(s["has_preds"], dtype=bool, copy=True) for s in scenes]
    has[0][1, :] = False                                                  # never observed
    has[0][2, 10:] = False                                                # cut short
    has[2][3, 5] = False                                                  # a hole
    has[2][8, :] = False
    has[2][8, 0] = True                                                   # the first step alone
    has[4][6, :29] = False                                                # the last step alone
    has[5][1, 7:19] = False
    for s, h in zip(scenes, has):
        s["has_preds"] = h
    n_obs = np.concatenate([h.sum(1) for h in has if len(h)])
    assert (n_obs == 0).sum() == 1 and ((n_obs > 0) & (n_obs < 30)).sum() == 5 and all(h[0].all() for h in has if len(h))
    tmp = tmp_path_factory.mktemp("eval_actors")
    path = str(tmp / "split.npz")
    write_scenes(path, scenes)
    store = DeviceSceneStore(path)
    torch.manual_seed(0)
    net = M.Net(M.config).cuda().eval()
    ev = evaluate_store(net, store, 3, actors=True)
    agents = evaluate_store(net, store, 3, evaluator=Evaluator(6, 6, 30, keep_preds=True))
    reg, cls = [], []
    with torch.no_grad():
        for pick in ([0, 1, 2], [3, 4, 5]):
            out = net.forward_store_flat(store, pick)[2]
            reg.append(out["reg"].cpu().numpy()), cls.append(out["cls"].cpu().numpy())
    return dict(store=store, net=net, ev=ev, agents=agents, reg=np.concatenate(reg), cls=np.concatenate(cls), actors=actors,
                has=np.concatenate([h for h in has if len(h)]), path=path)


def test_evaluate_store_actors_end_to_end(e2e):
    from lanegcn_amd._lib import LgcnError
    from lanegcn_amd.evaluate import ActorEvaluator, Evaluator, evaluate_store
    ev, store, agents = e2e["ev"], e2e["store"], e2e["agents"]
    assert type(ev) is ActorEvaluator and ev.n_slots == 25 and ev.n_scenes == 6 and ev.traj is None
    gt = store._job.t["gt_preds"].cpu().numpy()
    has_dev = store._job.t["has_preds"].cpu().numpy().astype(bool)
    assert np.array_equal(has_dev, e2e["has"])                            # the store kept the edited rows
    c = dict(reg=e2e["reg"], cls=e2e["cls"], gt=gt, has=has_dev, M=6, T=30, horizon=30)
    want = AM.records(c["reg"], c["cls"], gt, has_dev, store.actor_off, 30)
    assert sorted(want[:, 0].tolist()) == [0.0] + [1.0] * 24 and (want[:, 28] > 0).sum() == 5
    check(ev.records(), want, c, "end to end")
    scene, local = ev.actor_index()
    assert np.array_equal(local, want[:, 3]) and scene.tolist() == np.repeat(np.arange(6), e2e["actors"]).tolist()
    # the agents' summary of the actor table is the agent-only evaluator's
    mine, theirs = ev.summary(who="agent", min_obs=30), agents.summary()
    assert mine["n_evaluated"] == theirs["n_evaluated"] == 5 and mine["n_excluded"] == 20
    assert (mine["n_skipped"], mine["n_nonfinite"], theirs["n_skipped"]) == (0, 0, 1)
    for k in (6, 1):
        for m in EM.METRICS:
            assert abs(mine[k][m] - theirs[k][m]) <= 1e-12 * abs(theirs[k][m]), (k, m, mine[k][m], theirs[k][m])
    first = store.actor_off[:-1][np.diff(store.actor_off) > 0]
    assert np.array_equal(bits(ev.records()[first]), bits(agents.records()[[0, 2, 3, 4, 5]]))
    # the summaries against the model of the selected reduce
    for who, min_obs in (("all", 1), ("others", 1), ("others", 30), ("all", 12), ("agent", 1)):
        got, model = ev.summary(who=who, min_obs=min_obs), AM.summary(ev.records(), who, min_obs, 30)
        assert list(got) == [6, 1, "n_evaluated", "n_skipped", "n_nonfinite", "n_excluded"]
        for k in (6, 1):
            for m in EM.METRICS:
                assert abs(got[k][m] - model[k][m]) <= 1e-12 * abs(model[k][m]), (who, min_obs, k, m)
        assert all(got[n] == model[n] for n in ("n_evaluated", "n_skipped", "n_nonfinite", "n_excluded")), (who, min_obs)
    assert ev.summary()["n_evaluated"] == 24 and ev.summary(min_obs=30)["n_evaluated"] == 19
    assert ev.summary(who="others")["n_skipped"] == 1
    with pytest.raises(LgcnError):
        ev.summary(strict=True)                                           # one actor without an observed step
    assert ev.summary(who="agent", strict=True)["n_evaluated"] == 5
    # the default call: an Evaluator with the records of before; either class passed in is used as it is
    again = evaluate_store(e2e["net"], store, 3)
    assert type(again) is Evaluator and np.array_equal(bits(again.records()), bits(agents.records()))
    kept = ActorEvaluator.for_store(store, e2e["net"].config, keep_preds=True)
    assert evaluate_store(e2e["net"], store, 3, evaluator=kept) is kept
    assert np.array_equal(bits(kept.records()), bits(ev.records()))
    index, preds, scores = kept.predictions()
    assert index.tolist() == np.nonzero(want[:, 0] >= 1.0)[0].tolist()
    assert np.array_equal(bits(preds), bits(e2e["reg"][index])) and np.array_equal(bits(scores), bits(e2e["cls"][index]))
    assert evaluate_store(e2e["net"], store, 3, evaluator=agents, actors=True) is agents
    with pytest.raises(LgcnError):
        evaluate_store(e2e["net"], store, 3, evaluator=ActorEvaluator([0, 5, 5, 14, 15, 22, 26], 6, 30))


def test_train_driver_evaluates_every_actor(e2e, tmp_path, capsys):
    """train_dp.py --eval --eval-store --eval-actors: the three summaries and the prediction table of every actor."""
    import importlib
    import re
    from lanegcn_amd import lanegcn as M
    train_dp = importlib.import_module("train_dp")
    preds = str(tmp_path / "preds.npz")
    saved = dict(M.config)                                                # the driver writes into the shared config
    try:
        assert train_dp.main(["--eval", "--eval-store", e2e["path"], "--eval-actors", "--min-obs", "2", "--save-preds", preds,
                              "--dataset-len", "4"]) == 0
    finally:
        M.config.clear()
        M.config.update(saved)
    lines = capsys.readouterr().out.strip().splitlines()[-12:]
    keys = "minADE, minFDE, MR, p-minADE, brier-minADE, brier-minFDE".split(", ")
    counts = {"all": (22, 1, 0, 2), "agent": (5, 0, 0, 20), "others": (17, 1, 0, 7)}
    for i, who in enumerate(("all", "agent", "others")):
        head, k6, k1, tail = lines[4 * i:4 * i + 4]
        assert head == "actors: %s, at least 2 observed steps" % who
        for line, k in ((k6, 6), (k1, 1)):
            assert line.startswith("K=%d " % k) and re.findall(r"([A-Za-z-]+) \d+\.\d{4}", line) == keys, line
        assert tail == "evaluated %d actors, skipped %d, non-finite %d, excluded %d" % counts[who]
    with np.load(preds) as z:
        assert z["index"].tolist() == [i for i in range(25) if i != 1]
        assert z["scene"].tolist() == [0] * 4 + [2] * 9 + [3] + [4] * 7 + [5] * 3
        assert z["local"].tolist() == [0, 2, 3, 4] + list(range(9)) + [0] + list(range(7)) + [0, 1, 2]
        assert z["preds"].shape == (24, 6, 30, 2) and z["scores"].shape == (24, 6)
        assert z["preds"].dtype == np.float32 and np.isfinite(z["preds"]).all()
        assert np.all(np.diff(z["scores"], axis=1) <= 0)                  # the modes come sorted by score
