"""GPU: the split evaluation (lgcn_eval_scenes, lgcn_eval_reduce, lanegcn_amd.evaluate) against the float64 model of
tests/eval_model.py on the generated cases of tests/eval_cases.py.

Tolerances (derived, not measured): inputs are fp32; dx, dy are one rounding each, the norm three more, the sum over t at
most `horizon` more (the butterfly over the lanes is shallower), so |minFDE - model| <= 8 * 2^-24 * model and
|minADE - model| <= (horizon + 8) * 2^-24 * model.  p_k depends on the device's expf: the bar is 4 x the error of the
same formula in numpy float32 against the model (floor 1e-6, relative).  The summary equals the float64 model of the
reduce within 1e-12 relative; counts and MR numerators are exact."""
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import eval_cases as EC
import eval_model as EM

pytestmark = pytest.mark.gpu
EPS = 2.0 ** -24
SENTINEL = -7.25


@pytest.fixture(scope="module")
def cases():
    """Every generated case with the model's records (computed once, never modified)."""
    out = {}
    for c in EC.CASES:
        d = EC.make_case(*c)
        d["want"] = EM.records(d["reg"], d["cls"], d["gt"], d["has"], d["actor_off"], d["horizon"])
        out[c] = d
    return out


def bits(x):
    x = x.cpu().numpy() if torch.is_tensor(x) else np.asarray(x)
    return np.ascontiguousarray(x).view(np.uint32)


def launch(c, slot, n_slots, keep=True, fill=0.0):
    """One lgcn_eval_scenes launch of the batch `c` into fresh tables filled with `fill` -> (rec, traj, score, err)."""
    M, T = c["M"], c["T"]
    rec = torch.full((n_slots, 32), fill, dtype=torch.float32, device="cuda")
    traj = torch.full((n_slots, M, T, 2), fill, dtype=torch.float32, device="cuda") if keep else None
    score = torch.full((n_slots, M), fill, dtype=torch.float32, device="cuda") if keep else None
    err = torch.zeros(1, dtype=torch.int32, device="cuda")
    launch_into(c, slot, rec, traj, score, err)
    return rec, traj, score, err


def launch_into(c, slot, rec, traj, score, err, actor_off=None):
    from lanegcn_amd import ops
    cu = lambda x: torch.from_numpy(np.ascontiguousarray(x)).cuda()
    off = c["actor_off"] if actor_off is None else np.asarray(actor_off, np.int32)
    ops.eval_scenes(cu(c["reg"]), cu(c["cls"]), cu(c["gt"]), cu(c["has"]), cu(off), cu(np.asarray(slot, np.int64)),
                    c["horizon"], rec, traj, score, err)


def p_yardstick(c, want):
    """Largest relative error of p_k by the same formula in numpy float32 against the model, over the evaluated scenes."""
    worst = 0.0
    for b in np.nonzero(want[:, 0] == 1.0)[0]:
        a = c["actor_off"][b]
        p32 = EM.record_f32(c["reg"][a], c["cls"][a], c["gt"][a], c["horizon"]).astype(np.float64)
        p = want[b, 6:6 + 3 * c["M"]:3]
        worst = max(worst, float(np.max(np.abs(p32 - p) / p)))
    return worst


def check_records(got, want, M, H, p_bar, what=""):
    """`got` (fp32 records of the kernel) against the model's `want` within the bars of the module docstring."""
    got = np.asarray(got, np.float64)
    assert np.array_equal(got[:, 0], want[:, 0]), (what, "flags")
    ok = want[:, 0] == 1.0
    assert not got[~ok, 1:].any(), (what, "a record that was not evaluated must be zero behind its flag")
    assert np.array_equal(got[ok, 1:4], want[ok, 1:4]) and not got[ok, 4 + 3 * M:].any(), what
    g, w = got[ok, 4:4 + 3 * M].reshape(-1, M, 3), want[ok, 4:4 + 3 * M].reshape(-1, M, 3)
    rel = np.abs(g - w) / w
    worst = rel.reshape(-1, 3).max(0) if ok.any() else np.zeros(3)
    print("%s: worst relative error minFDE %.3g (bar %.3g) minADE %.3g (bar %.3g) p %.3g (bar %.3g)"
          % (what, worst[0], 8 * EPS, worst[1], (H + 8) * EPS, worst[2], p_bar))
    assert np.all(np.abs(g[..., 0] - w[..., 0]) <= 8 * EPS * w[..., 0]), (what, "minFDE", worst[0])
    assert np.all(np.abs(g[..., 1] - w[..., 1]) <= (H + 8) * EPS * w[..., 1]), (what, "minADE", worst[1])
    assert np.all(np.abs(g[..., 2] - w[..., 2]) <= p_bar * w[..., 2]), (what, "p", worst[2])


@pytest.mark.parametrize("case", EC.CASES, ids=EC.case_id)
def test_kernel_against_the_model(cases, case):
    c = cases[case]
    M, T, H, B = case
    rec, traj, score, err = launch(c, np.arange(B), B)
    assert int(err.item()) == 0
    err32 = p_yardstick(c, c["want"])
    print("%s: numpy float32 p error %.3g" % (EC.case_id(case), err32))
    check_records(rec.cpu().numpy(), c["want"], M, H, max(4 * err32, 1e-6), EC.case_id(case))
    first = c["actor_off"][:-1]
    for b in range(B):
        if c["want"][b, 0] >= 1.0:
            assert np.array_equal(bits(traj[b]), bits(c["reg"][first[b]])) and np.array_equal(bits(score[b]), bits(c["cls"][first[b]]))
        else:
            assert not traj[b].any() and not score[b].any()
    rec2 = launch(c, np.arange(B), B, keep=False)[0]                    # without the prediction tables: the same records
    assert np.array_equal(bits(rec2), bits(rec))


def test_flags(cases):
    """One batch of one-actor scenes, each a variation of the same agent (M 6, T 30, horizon 10)."""
    M, T, H = 6, 30, 10
    base = cases[(6, 30, 10, 5)]
    a = int(base["actor_off"][1])
    nan, inf = np.nan, np.inf
    edits = [("has", (H - 1,), False, 0), ("has", (H,), False, 1), ("reg", (3, H - 1, 0), nan, 2), ("reg", (0, 0, 1), inf, 2),
             ("cls", (M - 1,), nan, 2), ("cls", (0,), -inf, 2), ("gt", (H - 1, 1), nan, 2), ("gt", (0, 0), inf, 2),
             ("reg", (5, H, 0), nan, 1), ("gt", (T - 1, 1), inf, 1), ("has", (0,), False, 0), (None, None, None, 1),
             ("reg", (2, T - 1, 1), -inf, 1), ("has", (T - 1,), False, 1)]
    n = len(edits)
    c = {k: np.repeat(base[k][a:a + 1], n, 0).copy() for k in ("reg", "cls", "gt", "has")}
    for i, (name, at, val, _) in enumerate(edits):
        if name is not None:
            c[name][(i,) + at] = val
    c.update(actor_off=np.arange(n + 1, dtype=np.int32), M=M, T=T, horizon=H)
    want = EM.records(c["reg"], c["cls"], c["gt"], c["has"], c["actor_off"], H)
    assert want[:, 0].tolist() == [float(f) for *_, f in edits]
    rec, traj, score, err = launch(c, np.arange(n), n, fill=SENTINEL)
    assert int(err.item()) == 0
    check_records(rec.cpu().numpy(), want, M, H, max(4 * p_yardstick(c, want), 1e-6), "flags")
    for i, (*_, flag) in enumerate(edits):
        if flag == 0:                                                     # no prediction is kept of a scene that was not evaluated
            assert bool((traj[i] == SENTINEL).all()) and bool((score[i] == SENTINEL).all())
        else:
            assert np.array_equal(bits(traj[i]), bits(c["reg"][i])) and np.array_equal(bits(score[i]), bits(c["cls"][i]))


def test_untouched_slots_keep_their_contents(cases):
    c = cases[(6, 30, 30, 67)]
    B, n_slots = 67, 301
    slot = np.random.default_rng(5).permutation(n_slots)[:B]
    rec, traj, score, err = launch(c, slot, n_slots, fill=SENTINEL)
    assert int(err.item()) == 0
    rest = np.setdiff1d(np.arange(n_slots), slot)
    assert bool((rec[rest] == SENTINEL).all()) and bool((traj[rest] == SENTINEL).all()) and bool((score[rest] == SENTINEL).all())
    check_records(rec[slot].cpu().numpy(), c["want"], 6, 30, max(4 * p_yardstick(c, c["want"]), 1e-6), "sparse slots")


def reordered(c, order):
    """The batch `c` with its scenes in the order `order`."""
    off = c["actor_off"]
    rows = np.concatenate([np.arange(off[b], off[b + 1]) for b in order]).astype(np.int64)
    d = {k: c[k][rows] for k in ("reg", "cls", "gt", "has")}
    d.update(actor_off=np.concatenate([[0], np.cumsum([off[b + 1] - off[b] for b in order])]).astype(np.int32),
             M=c["M"], T=c["T"], horizon=c["horizon"])
    return d


@pytest.mark.parametrize("shape", [(6, 30, 30), (8, 64, 64)], ids=lambda s: "M%d-T%d-H%d" % s)
def test_a_record_depends_on_its_scene_alone(cases, shape):
    c = cases[shape + (67,)]
    B = 67
    one = launch(c, np.arange(B), B)
    again = launch(c, np.arange(B), B)
    order = np.arange(B)[::-1]
    rev = launch(reordered(c, order), order, B)
    M, T = c["M"], c["T"]
    single = (torch.zeros((B, 32), device="cuda"), torch.zeros((B, M, T, 2), device="cuda"), torch.zeros((B, M), device="cuda"),
              torch.zeros(1, dtype=torch.int32, device="cuda"))
    for b in range(B):                                                    # launches of one scene, the rows left where they are
        launch_into(c, [b], *single, actor_off=c["actor_off"][b:b + 2])
    for other, what in ((again, "second run"), (rev, "reversed"), (single, "launches of one")):
        for x, y, name in zip(one[:3], other[:3], ("rec", "traj", "score")):
            assert np.array_equal(bits(x), bits(y)), (what, name)
        assert int(other[3].item()) == 0


def reduce_on_device(rec, miss_thr=2.0):
    from lanegcn_amd import ops
    out = torch.full((8, 6), -1.0, dtype=torch.float64, device="cuda")
    cnt = torch.full((3,), -1, dtype=torch.int64, device="cuda")
    err = torch.zeros(1, dtype=torch.int32, device="cuda")
    ops.eval_reduce(torch.from_numpy(rec).cuda(), miss_thr, out, cnt, err)
    return out.cpu().numpy(), cnt.cpu().numpy(), int(err.item())


@pytest.mark.parametrize("n_slots", [1, 257, 4099])
def test_reduce_against_the_model(n_slots):
    M, H = 6, 30
    rec = EC.make_records(n_slots, M, H, seed=n_slots)
    if n_slots == 1:
        rec[0, 0], rec[0, 1], rec[0, 2] = 1.0, M, H
    want, want_cnt = EM.reduce(rec, EC.MISS_THR)
    out, cnt, err = reduce_on_device(rec)
    assert err == 0 and cnt.tolist() == want_cnt.tolist() and cnt.sum() == n_slots
    assert np.array_equal(out[:, 2], want[:, 2])                          # MR numerators: exact
    assert not out[M:].any()
    rel = np.abs(out[:M] - want[:M]) / np.maximum(np.abs(want[:M]), 1e-300)
    print("reduce n_slots %d: worst relative error %.3g" % (n_slots, rel[want[:M] != 0].max() if (want[:M] != 0).any() else 0.0))
    assert np.all(np.abs(out - want) <= 1e-12 * np.abs(want))
    out2, cnt2, _ = reduce_on_device(rec)
    assert np.array_equal(out.view(np.uint64), out2.view(np.uint64)) and np.array_equal(cnt, cnt2)


def test_summary_against_the_model_and_mixed_records_raise():
    from lanegcn_amd._lib import LgcnError
    from lanegcn_amd.evaluate import Evaluator
    n, M, H = 4099, 6, 30
    rec = EC.make_records(n, M, H, seed=1)
    ev = Evaluator(n, M, H)
    ev.rec.copy_(torch.from_numpy(rec))
    got, want = ev.summary(ks=(6, 1, 3)), EM.summary(rec, EC.MISS_THR, ks=(6, 1, 3))
    assert list(got) == [6, 1, 3, "n_evaluated", "n_skipped", "n_nonfinite"]
    for k in (6, 1, 3):
        assert list(got[k]) == list(EM.METRICS)
        for m in EM.METRICS:
            assert abs(got[k][m] - want[k][m]) <= 1e-12 * abs(want[k][m]), (k, m)
    assert all(got[k] == want[k] for k in ("n_evaluated", "n_skipped", "n_nonfinite"))
    assert got["n_skipped"] > 0 and got["n_nonfinite"] > 0
    with pytest.raises(LgcnError):
        ev.summary(strict=True)
    with pytest.raises(LgcnError):
        ev.summary(ks=(7,))
    assert np.array_equal(ev.records().view(np.uint32), rec.view(np.uint32))
    bad = int(np.nonzero(rec[:, 0] == 1.0)[0][-1])
    ev.rec[bad, 1] = M - 1                                                # one evaluated record of another M
    with pytest.raises(LgcnError):
        ev.summary()
    empty = Evaluator(0, M, H).summary()
    assert empty["n_evaluated"] == 0 and np.isnan(empty[6]["minADE"])


def test_a_slot_outside_the_table_is_refused_and_not_written(cases):
    from lanegcn_amd._lib import LgcnError
    from lanegcn_amd.evaluate import Evaluator
    c = cases[(6, 30, 30, 5)]
    off = c["actor_off"]
    assert off[2] > off[1]                                                # scene 1 holds actors
    n_slots = 9
    pairs = [(1, 3), (1, n_slots), (3, -1), (1, 5)]                       # (scene, slot): launches of one, rows left in place
    rec = torch.full((n_slots, 32), SENTINEL, device="cuda")
    traj = torch.full((n_slots, 6, 30, 2), SENTINEL, device="cuda")
    score = torch.full((n_slots, 6), SENTINEL, device="cuda")
    err = torch.zeros(1, dtype=torch.int32, device="cuda")
    for b, s in pairs:
        launch_into(c, [s], rec, traj, score, err, actor_off=off[b:b + 2])
    assert int(err.item()) == 1
    rest = [i for i in range(n_slots) if i not in (3, 5)]
    assert bool((rec[rest] == SENTINEL).all()) and bool((traj[rest] == SENTINEL).all()) and bool((score[rest] == SENTINEL).all())
    assert np.array_equal(bits(rec[3]), bits(rec[5])) and float(rec[3, 0]) == c["want"][1, 0]
    # one launch that names a bad slot between two good ones
    rec2, _, _, err2 = launch(reordered(c, [1, 3, 1]), [0, 1 << 40, 2], 3, fill=SENTINEL)
    assert int(err2.item()) == 1 and bool((rec2[1] == SENTINEL).all()) and np.array_equal(bits(rec2[0]), bits(rec[3]))
    # the public interface turns the flag into an error
    d = reordered(c, [1, 3])
    cu = lambda x: torch.from_numpy(np.ascontiguousarray(x)).cuda()
    fb = SimpleNamespace(n_scenes=2, n_actors=int(d["actor_off"][-1]), actor_off=cu(d["actor_off"]))
    ex = {"gt_preds": cu(d["gt"]), "has_preds": cu(d["has"])}
    ev = Evaluator(4, 6, 30)
    ev.update(cu(d["reg"]), cu(d["cls"]), fb, ex, [2, 4])
    with pytest.raises(LgcnError):
        ev.summary()
    assert not ev.rec[3].any() and float(ev.rec[2, 0]) == 1.0
    with pytest.raises(LgcnError):
        ev.update(cu(d["reg"]), cu(d["cls"]), fb, {}, [0, 1])          # a batch without ground truth


@pytest.fixture(scope="module")
def e2e(tmp_path_factory):
    """A store of 7 small synthetic scenes (scene 1 and scene 6 hold no actor), a randomly initialised Net, the evaluator
    of evaluate_store(batch_size=3) and forward_store's per-scene outputs on the same picks."""
    import lanegcn_amd  # noqa: F401
    from lanegcn_amd import data as gen
    from lanegcn_amd import lanegcn as M
    from lanegcn_amd.evaluate import Evaluator, evaluate_store
    from lanegcn_amd.flatfile import DeviceSceneStore, write_scenes
    rng = np.random.default_rng(11)
    actors = [5, 0, 9, 1, 7, 3, 0]
    scenes = [gen.synth_scene(rng, [4, 4] if i % 2 else [5], n) for i, n in enumerate(actors)]
    tmp = tmp_path_factory.mktemp("eval")
    write_scenes(str(tmp / "split.npz"), scenes)
    store = DeviceSceneStore(str(tmp / "split.npz"))
    torch.manual_seed(0)
    net = M.Net(M.config).cuda().eval()
    ev = evaluate_store(net, store, 3, evaluator=Evaluator(7, 6, 30, keep_preds=True))
    reg, cls = [None] * 7, [None] * 7
    for pick in ([0, 1, 2], [3, 4, 5]):
        out = net.forward_store(store, pick)
        for i, r, c in zip(pick, out["reg"], out["cls"]):
            reg[i], cls[i] = r, c
    for s in scenes:
        s.pop("gt_preds"), s.pop("has_preds")
    write_scenes(str(tmp / "nogt.npz"), scenes[:2])
    return dict(scenes=scenes, store=store, net=net, ev=ev, reg=reg, cls=cls, actors=actors, nogt=str(tmp / "nogt.npz"),
                path=str(tmp / "split.npz"))


def test_evaluate_store_end_to_end(e2e):
    from lanegcn_amd._lib import LgcnError
    from lanegcn_amd.evaluate import evaluate_store
    from lanegcn_amd.flatfile import DeviceSceneStore
    from lanegcn_amd.lanegcn import pred_metrics
    ev, store, actors = e2e["ev"], e2e["store"], e2e["actors"]
    seen = [i for i in range(6) if actors[i]]
    a_off = store.actor_off
    gt = np.stack([store._job.t["gt_preds"][a_off[i]].cpu().numpy() for i in seen])
    preds = np.stack([e2e["reg"][i][0].cpu().numpy() for i in seen])
    scores = np.stack([e2e["cls"][i][0].cpu().numpy() for i in seen])
    want = np.zeros((7, 32))
    for n, i in enumerate(seen):
        want[i] = EM.record(preds[n], scores[n], gt[n], np.ones(30, bool), 30)
    err32 = max(float(np.max(np.abs(EM.record_f32(preds[n], scores[n], gt[n], 30) - want[i, 6:24:3]) / want[i, 6:24:3]))
                for n, i in enumerate(seen))
    check_records(ev.records(), want, 6, 30, max(4 * err32, 1e-6), "end to end")
    s = ev.summary()
    assert (s["n_evaluated"], s["n_skipped"], s["n_nonfinite"]) == (len(seen), 2, 0)
    ade1, fde1, ade, fde, _ = pred_metrics(preds, gt, np.ones((len(seen), 30), bool))
    assert s[1]["minADE"] == pytest.approx(ade1, rel=1e-5) and s[1]["minFDE"] == pytest.approx(fde1, rel=1e-5)
    assert s[6]["minADE"] == pytest.approx(ade, rel=1e-5) and s[6]["minFDE"] == pytest.approx(fde, rel=1e-5)
    with pytest.raises(LgcnError):
        ev.summary(strict=True)                                           # two scenes without an agent
    index, p, sc = ev.predictions()
    assert index.tolist() == seen and np.array_equal(bits(p), bits(preds)) and np.array_equal(bits(sc), bits(scores))
    # a shard of the split into the same table: the other slots stay as they are; the default evaluator covers the store
    ev2 = evaluate_store(e2e["net"], store, 3, indices=[3, 4, 5])
    r2 = ev2.records()
    assert np.array_equal(bits(r2[3:6]), bits(ev.records()[3:6])) and not r2[[0, 1, 2, 6]].any()
    assert ev2.n_scenes == 7 and ev2.traj is None
    with pytest.raises(LgcnError):
        evaluate_store(e2e["net"], DeviceSceneStore(e2e["nogt"]), 2)
    with pytest.raises(LgcnError):
        evaluate_store(e2e["net"], store, 3, evaluator=type(ev)(5, 6, 30))


def test_forward_store_is_unchanged_by_the_refactor(e2e):
    """forward_store returns what forward(data) returns on the same scenes (per-scene lists, world frame)."""
    from lanegcn_amd import data as gen
    net, store = e2e["net"], e2e["store"]
    fb, ex, flat = net.forward_store_flat(store, [3, 4, 5])
    out = net.forward_store(store, [3, 4, 5])
    assert [tuple(r.shape) for r in out["reg"]] == [(n, 6, 30, 2) for n in (1, 7, 3)]
    assert torch.equal(torch.cat(out["reg"]), flat["reg"]) and torch.equal(torch.cat(out["cls"]), flat["cls"])
    assert ex["sizes"] == [1, 7, 3] and fb.n_scenes == 3


def run_driver(argv):
    """train_dp.main(argv) in-process, like the other driver tests; the shared config is put back afterwards."""
    import importlib
    from lanegcn_amd import lanegcn as M
    train_dp = importlib.import_module("train_dp")
    saved = dict(M.config)     # the driver writes batch_size / save_dir / epoch into the shared config
    try:
        return train_dp.main(argv)
    finally:
        M.config.clear()
        M.config.update(saved)


def test_train_driver_evaluates_a_store(e2e, tmp_path, capsys):
    """train_dp.py --eval --eval-store: one line per K in Argoverse's key order, the counts, and the prediction table."""
    import re
    preds = str(tmp_path / "preds.npz")
    assert run_driver(["--eval", "--eval-store", e2e["path"], "--save-preds", preds, "--dataset-len", "4"]) == 0
    lines = capsys.readouterr().out.strip().splitlines()
    keys = "minADE, minFDE, MR, p-minADE, brier-minADE, brier-minFDE".split(", ")
    for line, k in zip(lines[-3:-1], (6, 1)):
        assert line.startswith("K=%d " % k) and re.findall(r"([A-Za-z-]+) \d+\.\d{4}", line) == keys, line
    assert lines[-1] == "evaluated 5 scenes, skipped 2, non-finite 0"
    with np.load(preds) as z:
        assert z["index"].tolist() == [0, 2, 3, 4, 5] and z["preds"].shape == (5, 6, 30, 2) and z["scores"].shape == (5, 6)
        assert z["preds"].dtype == np.float32 and np.isfinite(z["preds"]).all()
        assert np.all(np.diff(z["scores"], axis=1) <= 0)                  # the modes come sorted by score


def test_train_driver_validates_from_a_store(e2e, tmp_path, capsys):
    """train_dp.py --eval-store without --eval: validation runs from the store and prints the reference's validation line."""
    import re
    assert run_driver(["--eval-store", e2e["path"], "--max-iters", "1", "--batch-size", "2", "--dataset-len", "4",
                       "--save-dir", str(tmp_path / "run")]) == 0
    out = capsys.readouterr().out
    assert "Validation, time" in out
    assert re.search(r"loss \d+\.\d{4} \d+\.\d{4} \d+\.\d{4}, ade1 \d+\.\d{4}, fde1 \d+\.\d{4}, ade \d+\.\d{4}, fde \d+\.\d{4}", out)
