"""CPU: the float64 model of the per-actor evaluation (tests/eval_actors_model.py): it is eval_model.record on fully
observed rows, follows PredLoss's rule on partial ones, its selected reduce is eval_model.reduce on the zeroed copy, and
the bars of tests/test_gpu_eval_actors.py reject each of its deliberately wrong variants on the generated cases."""
import numpy as np
import pytest

import eval_actors_cases as AC
import eval_actors_model as AM
import eval_model as EM

VARIANTS = ("ade_over_horizon", "fde_at_end", "gt_checked_always")


@pytest.fixture(scope="module")
def cases():
    out = {}
    for c in AC.CASES:
        d = AC.make_case(*c)
        d["want"] = AM.records(d["reg"], d["cls"], d["gt"], d["has"], d["actor_off"], d["horizon"])
        out[c] = d
    return out


@pytest.mark.parametrize("case", AC.CASES, ids=AC.case_id)
def test_fully_observed_rows_are_the_scene_model(cases, case):
    c = cases[case]
    H = c["horizon"]
    full = np.nonzero(c["has"][:, :H].all(1))[0]
    assert full.size
    for a in full:
        want = EM.record(c["reg"][a], c["cls"][a], c["gt"][a], c["has"][a], H)
        got = c["want"][a].copy()
        assert got[28] == 0.0 and got[29] == 0.0
        got[3] = 0.0                                                      # the local index is the one float the scene record lacks
        assert np.array_equal(got, want), a
    # and the scene model on the first rows: a partially observed agent is `not evaluated` there, evaluated here
    scene = EM.records(c["reg"], c["cls"], c["gt"], c["has"], c["actor_off"], H)
    for b, a in enumerate(c["actor_off"][:-1]):
        if c["actor_off"][b + 1] > a and scene[b, 0] == 1.0:
            assert np.array_equal(c["want"][a], scene[b])


def test_partial_rows_follow_the_loss_rule():
    """One actor by hand: gt on the x axis, two modes displaced along y by a constant each; steps 1 and 3 of 5 observed."""
    T = 5
    gt = np.stack([np.arange(T, dtype=np.float64), np.zeros(T)], 1)
    reg = np.repeat(gt[None], 2, 0)
    reg[0, :, 1] = [9.0, 4.0, 9.0, 2.0, 9.0]
    reg[1, :, 1] = [9.0, 1.0, 9.0, 3.0, 0.0]
    has = np.array([False, True, False, True, False])
    gt[[0, 2, 4]] = np.nan                                                # never looked at
    r = AM.record(reg, np.zeros(2), gt, has, 5, local=3)
    assert r[:4].tolist() == [1.0, 2.0, 5.0, 3.0] and r[28] == 3.0 and r[29] == 1.0
    assert r[4:7].tolist() == [2.0, 3.0, 1.0]                             # K = 1: mode 0: FDE at step 3, ADE (4 + 2) / 2
    assert r[7:10].tolist() == [2.0, 3.0, 0.5]                            # K = 2: mode 0 still (2 < 3), although mode 1 ends on gt
    assert not r[10:28].any() and not r[30:].any()
    assert AM.record(reg, np.zeros(2), gt, has, 1, local=3).tolist() == [0.0, 0.0, 0.0, 3.0] + [0.0] * 28      # nothing observed before 1
    reg[1, 4, 0] = np.inf                                                 # inside the horizon, at an unobserved step: counts
    bad = AM.record(reg, np.zeros(2), gt, has, 5, local=3)
    assert bad[0] == 2.0 and bad[3] == 3.0 and not bad[[1, 2]].any() and not bad[4:].any()
    assert AM.record(reg, np.zeros(2), gt, has, 4, local=3)[0] == 1.0     # outside it: does not


@pytest.mark.parametrize("case", AC.CASES, ids=AC.case_id)
def test_the_bars_tell_wrong_from_right(cases, case):
    c = cases[case]
    M, T, H, _ = case
    want = c["want"]
    args = (c["reg"], c["cls"], c["gt"], c["has"], c["actor_off"], H)
    assert AC.outside_bars(want.astype(np.float32), want, M, H, 1e-6) == []      # rounding the model to fp32 stays inside
    for v in VARIANTS:
        miss = AC.outside_bars(AM.records(*args, variant=v), want, M, H, 1e-6)
        if H > 1:
            assert miss, v
            print("%s %s: %s" % (AC.case_id(case), v, miss))
        else:                      # one step: every evaluated actor is fully observed, the variants are the model
            assert miss == [], v


@pytest.mark.parametrize("who", sorted(AM.WHO))
@pytest.mark.parametrize("n", [1, 129, 773])
def test_selected_reduce_is_the_reduce_of_the_zeroed_copy(n, who):
    M, H = 6, 30
    rec = AC.make_records(n, M, H, seed=n)
    for max_missing in (0, H - 1):
        out, cnt = AM.reduce_sel(rec, who, max_missing, AC.MISS_THR)
        zero = AM.zeroed(rec, who, max_missing)
        want, want_cnt = EM.reduce(zero, AC.MISS_THR)
        assert np.array_equal(out, want)
        assert cnt[1:3].tolist() == want_cnt[1:].tolist() and cnt[0] + cnt[3] == want_cnt[0] and cnt.sum() == n
        ex = AM.excluded(rec, who, max_missing)
        assert cnt[3] == ex.sum() and not zero[ex].any() and np.array_equal(zero[~ex], rec[~ex])
        if n > 1:
            assert 0 < ex.sum() < n or (who == "all" and max_missing == H - 1 and not ex.any())
    s = AM.summary(rec, who, 1, H, AC.MISS_THR)
    assert list(s) == [6, 1, "n_evaluated", "n_skipped", "n_nonfinite", "n_excluded"]


def test_make_records_covers_the_selection():
    rec = AC.make_records(773, 6, 30, seed=773)
    ok = rec[:, 0] == 1.0
    for flag in (0.0, 1.0, 2.0):
        f = rec[:, 0] == flag
        assert (rec[f, 3] == 0).any() and (rec[f, 3] > 0).any()
    assert (rec[ok, 28] == 0).any() and (rec[ok, 28] > 0).any()
    assert not rec[~ok, 28:30].any() and np.all(rec[ok, 29] <= rec[ok, 28])
