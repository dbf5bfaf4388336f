"""GPU: the goal decoder's kernels (csrc/lgcn_goal.hip, csrc/lgcn_goal_bwd.hip) at the sizes and on the branches the
reference's captures do not reach -- RoIs of up to 1025 nodes (second and later passes of the 256-thread loops), one
and two survivors with padding, ties, NaN logits, pairs exactly at the threshold, stopped agents, zero and clamping
velocities, 300 agents in one launch; refine rows with a replaced sample, a tied, a negative and a NaN maximum.  Inputs:
tests/decode_cases.py (pinned by test_decode_cases_host.py).  Yardstick: tests/decode_model.py in float64.

Indices are compared exactly (the cases make every index decision the same in fp32 and float64).  Bar of a value or
gradient tensor: max(4 x the error of the same model run in float32 on the CPU against its float64 run, 1e-6)."""
import numpy as np
import pytest
import torch

import decode_cases as DC
import decode_model as DM

pytestmark = pytest.mark.gpu
K = DC.K
CASES = {"selection": DC.selection_cases, "selection_no_nan": lambda: DC.selection_cases(nan_roi=False),
         "many_agents": DC.many_agents_case}
OUT = ("top_idx", "goals", "logits", "coef", "s_samples")
INS = ("pred", "anc_ctrs", "anc_dirs", "agt_ctrs", "dir_last", "agt_vel")


@pytest.fixture(scope="module")
def ops():
    import lanegcn_amd  # noqa: F401
    from lanegcn_amd import ops
    return ops


def cu(x):
    return torch.from_numpy(np.array(x)).cuda()


def bits(t):
    """NaNs compare by their bits."""
    t = t.detach().cpu().contiguous()
    return t.view(torch.int32) if t.dtype == torch.float32 else t


def same_bits(a, b):
    return a.shape == b.shape and torch.equal(bits(a), bits(b))


def decode(ops, case, dev):
    return ops.goal_decode(dev["pred"], case["pred_spans"], dev["anc_ctrs"], dev["anc_dirs"], case["anc_first"], dev["agt_ctrs"],
                           dev["dir_last"], dev["agt_vel"], K, 2.0)


@pytest.fixture(scope="module")
def runs(ops):
    """Every launch once: the device inputs, the outputs of goal_decode, and the same launch a second time."""
    out = {}
    for name, make in CASES.items():
        case = make()
        dev = {k: cu(case[k]) for k in INS}
        first = decode(ops, case, dev)
        again = decode(ops, case, dev)
        torch.cuda.synchronize()
        out[name] = {"case": case, "dev": dev, "got": dict(zip(OUT, first)), "again": dict(zip(OUT, again)),
                     "top": first[0].cpu().numpy().astype(np.int64)}
    return out


@pytest.mark.parametrize("name", ["selection", "many_agents"])
def test_three_routes_select_the_same_nodes(ops, runs, name):
    r = runs[name]
    case, got, top = r["case"], r["got"], r["top"]
    off = case["pred_spans"]
    xy, lg = DC.xy_logit(case)
    want = np.array([DM.greedy(xy[off[a]:off[a + 1]], lg[off[a]:off[a + 1]], 2.0, K, K) for a in range(len(off) - 1)])
    idx, count = ops.nms_select_segments(cu(xy), cu(lg), off, 2.0, K, K)
    idx = idx.cpu().numpy()
    nms = np.array([idx[off[a]:off[a] + K] for a in range(len(off) - 1)])
    assert (count.cpu().numpy() == K).all()
    wrong = [case["names"][a] for a in range(len(want)) if not (np.array_equal(top[a], want[a]) and np.array_equal(nms[a], want[a]))]
    for a in range(len(want)):
        if case["names"][a] in wrong:
            print("%s: float64 %s, goal_decode %s, nms_select %s" % (case["names"][a], want[a], top[a], nms[a]))
    assert not wrong, wrong
    assert got["top_idx"].dtype == torch.int32 and tuple(got["top_idx"].shape) == (len(want), K)
    # goals and logits are the selected rows, bit for bit
    rows = np.asarray(off[:-1])[:, None] + top
    assert np.array_equal(got["goals"].cpu().numpy().view(np.int32), xy[rows].view(np.int32))
    assert np.array_equal(got["logits"].cpu().numpy().view(np.int32), case["pred"][rows, 0].view(np.int32))
    # inputs unmodified, and a second run is bitwise equal
    assert all(same_bits(r["dev"][k], torch.from_numpy(np.array(case[k]))) for k in INS)
    assert all(same_bits(got[k], r["again"][k]) for k in OUT)
    if name == "selection":
        a = case["names"].index("nan12")
        assert np.isnan(got["logits"][a].cpu().numpy()).tolist() == [True, True] + [False] * (K - 2)
        same = runs["selection_no_nan"]
        keep = [i for i in range(len(want)) if i != a]
        assert np.array_equal(same["top"], top[keep])               # the launch without that RoI selects the same nodes


@pytest.mark.parametrize("name", ["selection_no_nan", "many_agents"])
def test_coefficients_and_samples_against_float64(runs, name):
    r = runs[name]
    case, got = r["case"], r["got"]
    ref = DC.value_reference(case, r["top"])
    err = {k: DC.agent_err(got[k].cpu().numpy(), ref[k][0]) for k in ref}
    for k in ref:
        print("%-16s %-9s rel error %.2e (bar %.2e)" % (name, k, err[k], ref[k][1]))
    coef = got["coef"].cpu().numpy()
    assert np.isfinite(coef).all() and np.isfinite(got["s_samples"].cpu().numpy()).all()
    stopped = [a for a, k in enumerate(case["dir_kind"]) if k in ("zero", "below")]
    moving = [a for a, k in enumerate(case["dir_kind"]) if k in ("random", "above")]
    assert len(stopped) >= 6 and (coef[stopped][..., 1] == 0).all() and (coef[stopped][..., 4] == 0).all()
    assert (np.abs(coef[moving][..., [1, 4]]).max(-1) > 0).all()
    for k in ref:
        assert err[k] <= ref[k][1], (name, k, err[k], ref[k][1])


@pytest.mark.parametrize("name", ["selection", "selection_no_nan", "many_agents"])
def test_training_route_against_inference_route(runs, name):
    from lanegcn_amd import lanercnn as R
    r = runs[name]
    case, dev = r["case"], r["dev"]
    with torch.no_grad():
        top, goals, logits, coefs, ss = R.Decode._decode_torch(None, dev["pred"], case["pred_spans"], dev["anc_ctrs"], dev["anc_dirs"],
                                                               case["spans"], dev["agt_ctrs"], dev["dir_last"], dev["agt_vel"], K)
    assert np.array_equal(top.cpu().numpy(), r["top"])
    if name == "selection":                                            # NaN logits: the indices are the whole check
        return
    got = {"goals": goals, "logits": logits, "coef": torch.cat(coefs, 2), "s_samples": ss}
    ref = DC.value_reference(case, r["top"])
    err = {k: DC.agent_err(got[k].cpu().numpy(), ref[k][0]) for k in ref}
    for k in ref:
        print("%-16s %-9s rel error of the stock-op route %.2e (bar %.2e)" % (name, k, err[k], ref[k][1]))
    for k in ref:
        assert err[k] <= ref[k][1], (name, k, err[k], ref[k][1])


def refine(ops, c):
    return ops.goal_refine(cu(c["s_samples"][None]), cu(c["coef"][None]), cu(c["delta"][None]))[0]


def test_refine_forward_on_the_edge_rows(ops):
    with_nan, without = DC.refine_inputs(), DC.refine_inputs(nan=False)
    got, got_plain = refine(ops, with_nan), refine(ops, without)
    e = DC.REFINE_ROWS.index("nan")
    others = [i for i in range(len(DC.REFINE_ROWS)) if i != e]
    # one NaN in: its row is NaN throughout, as in float64, and no other row changes
    assert np.isnan(DC.refine_model(with_nan)[e]).all()
    assert bool(torch.isnan(got[e]).all()) and bool(torch.isfinite(got_plain).all())
    assert torch.equal(got[others], got_plain[others])
    assert same_bits(refine(ops, with_nan), got)
    ref, m32 = DC.refine_model(without), DC.refine_model(without, torch.float32)
    out = got_plain.cpu().numpy()
    err = [DM.rel_err(out[i], ref[i]) for i in range(len(ref))]
    bar = [DC.bar_of(DM.rel_err(m32[i], ref[i])) for i in range(len(ref))]
    for i, n in enumerate(DC.REFINE_ROWS):
        print("refine %-12s rel error %.2e (bar %.2e)" % (n, err[i], bar[i]))
    # the replaced step is evaluated at s = 1, as the model does: the curve's end point plus the normal offset
    b = DC.REFINE_ROWS.index("replaced")
    c64 = without["coef"][b].astype(np.float64)
    dn = float(without["delta"][b, DC.REPLACED_AT, 1])
    end = np.array([c64[0] + c64[1] + c64[2] - (2 * c64[3] + c64[4]) * dn, c64[3] + c64[4] + c64[5] + (2 * c64[0] + c64[1]) * dn])
    assert np.abs(ref[b, DC.REPLACED_AT] - end).max() <= 1e-12 * np.abs(end).max()
    assert np.abs(out[b, DC.REPLACED_AT] - end).max() <= bar[b] * np.abs(ref[b]).max()
    for i, n in enumerate(DC.REFINE_ROWS):
        assert err[i] <= bar[i], (n, err[i], bar[i])


def test_refine_backward_on_the_edge_rows(ops):
    rows = [n for n in DC.REFINE_ROWS if n != "nan"]
    c = DC.refine_inputs(rows)
    w = np.random.default_rng(5).normal(0, 1, c["delta"].shape).astype(np.float32)
    run = lambda: ops.goal_refine_bwd(cu(c["s_samples"][None]), cu(c["coef"][None]), cu(c["delta"][None]), cu(w[None]))
    got = run()
    assert all(same_bits(x, y) for x, y in zip(got, run()))
    got = [g[0].cpu().numpy() for g in got]
    g64, g32 = DC.refine_grads(c, w), DC.refine_grads(c, w, torch.float32)
    names = ("d_s_samples", "d_coef", "d_traj_delta")
    err = [DM.rel_err(g, r) for g, r in zip(got, g64)]
    bar = [DC.bar_of(DM.rel_err(a, r)) for a, r in zip(g32, g64)]
    for n, e, b in zip(names, err, bar):
        print("refine %-12s rel error %.2e (bar %.2e)" % (n, e, b))
    # per row too, by the same rule: a row's error is not hidden behind a row of larger gradients
    row_miss = []
    for i, n in enumerate(rows):
        for k in range(3):
            e_row, b_row = DM.rel_err(got[k][i], g64[k][i]), DC.bar_of(DM.rel_err(g32[k][i], g64[k][i]))
            print("refine %-12s %-12s rel error %.2e (bar %.2e)" % (n, names[k], e_row, b_row))
            if not e_row <= b_row:
                row_miss.append((n, names[k], e_row, b_row))
    # the replaced step: its own path is cut, and it is not the maximum, so it receives exactly nothing
    i = rows.index("replaced")
    assert got[0][i, DC.REPLACED_AT] == 0 and got[2][i, DC.REPLACED_AT, 0] == 0 and got[2][i, DC.REPLACED_AT, 1] != 0
    assert g64[0][i, DC.REPLACED_AT] == 0
    # d_s_samples and d_traj_delta[..., 0] are the same numbers
    assert np.array_equal(got[0], got[2][..., 0])
    for n, e, b in zip(names, err, bar):
        assert e <= b, (n, e, b)
    assert not row_miss, row_miss


@pytest.mark.parametrize("name", ["selection_no_nan", "many_agents"])
def test_decode_backward_against_float64_autograd(ops, runs, name):
    r = runs[name]
    case, dev = r["case"], r["dev"]
    w = DC.upstream(case, 7)
    ups = {k: cu(v) for k, v in w.items()}
    top_dev = r["got"]["top_idx"]
    run = lambda: ops.goal_decode_bwd(dev["pred"], case["pred_spans"], dev["anc_ctrs"], dev["anc_dirs"], case["anc_first"],
                                      dev["agt_ctrs"], dev["dir_last"], dev["agt_vel"], top_dev, d_goals=ups["goals"],
                                      d_logits=ups["logits"], d_coef=ups["coef"], d_s_samples=ups["s_samples"])
    junk = torch.full_like(dev["pred"], float("nan"))      # d_pred is torch.empty_like(pred): let it start from NaNs,
    del junk                                               # not from a block that happens to hold zeros
    got_dev = run()
    assert same_bits(got_dev, run())
    got = got_dev.cpu().numpy()
    ref, bar = DC.d_pred_reference(case, r["top"], w)
    err = DM.rel_err(got, ref)
    print("%-16s d_pred    rel error %.2e (bar %.2e)" % (name, err, bar))
    chosen = np.zeros(len(got), dtype=bool)
    for a, lo in enumerate(case["pred_spans"][:-1]):
        chosen[lo + r["top"][a]] = True
    assert chosen.sum() == len(r["top"]) * K and (got[~chosen] == 0).all()         # the zeroing loop, past 256 x 5 floats
    rows = np.asarray(case["pred_spans"][:-1])[:, None] + r["top"]
    assert np.array_equal(got[rows, 0], w["logits"])                               # d_logits lands on the selected rows
    assert np.isfinite(got).all() and (np.abs(got[chosen]).max(1) > 0).all()
    assert all(same_bits(dev[k], torch.from_numpy(np.array(case[k]))) for k in INS)
    assert err <= bar, (name, err, bar)
