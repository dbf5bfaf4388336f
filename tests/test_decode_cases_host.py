"""CPU: the synthetic inputs of the goal-decoder edge tests (tests/decode_cases.py) hold what they claim, so that
test_gpu_goal_decode_edges.py cannot pass vacuously: sizes, grid exactness, the survivor counts, the planted winners,
ties, NaNs, the exact-2.0 pair, and the conditioning bounds.  Also prints the fp32-model bars the GPU test uses."""
import numpy as np
import pytest
import torch

import decode_cases as DC
import decode_model as DM

K = DC.K


@pytest.fixture(scope="module", params=["selection", "many"])
def case(request):
    return DC.selection_cases() if request.param == "selection" else DC.many_agents_case()


def rois(case):
    xy, lg = DC.xy_logit(case)
    off = case["pred_spans"]
    return {n: (xy[off[a]:off[a + 1]], lg[off[a]:off[a + 1]]) for a, n in enumerate(case["names"])}


@pytest.fixture(scope="module")
def full_lists():
    """The uncut float64 list of every RoI of selection_cases(), computed once."""
    return {n: DM.greedy(xy, lg, 2.0, K, 0) for n, (xy, lg) in rois(DC.selection_cases()).items()}


def test_sizes_and_layout():
    c = DC.selection_cases()
    sizes = dict(zip(c["names"], np.diff(c["pred_spans"]).tolist()))
    assert [sizes["spread%d" % n] for n in DC.SPREAD_SIZES] == [6, 7, 255, 256, 257, 300, 600, 1025]
    assert (sizes["one_disc300"], sizes["two_discs257"], sizes["planted257"]) == (300, 257, 257)
    assert (sizes["equal40"], sizes["nan12"], sizes["pairs8"]) == (40, 12, 8)
    assert len(c["names"]) == 14 and c["pred_spans"][-1] <= 4000
    no_nan = DC.selection_cases(nan_roi=False)
    assert no_nan["names"] == [n for n in c["names"] if n != "nan12"] and not np.isnan(no_nan["pred"]).any()
    keep = [a for a, n in enumerate(c["names"]) if n != "nan12"]
    for k in ("agt_ctrs", "dir_last", "agt_vel"):
        assert np.array_equal(no_nan[k], c[k][keep]), k
    m = DC.many_agents_case()
    sizes = np.diff(m["pred_spans"])
    assert len(sizes) == 300 and sizes.min() == 6 and sizes.max() == 40 and m["pred_spans"][-1] <= 8000
    for c in (c, no_nan, m):
        assert c["pred"].dtype == np.float32 and c["pred"].shape == (c["pred_spans"][-1], 5)
        # unused anchor rows between the RoIs: no RoI's anchors start at its pred offset
        assert all(f != p for f, p in zip(c["anc_first"], c["pred_spans"][:-1]))
        assert all(hi - lo == n for (lo, hi), n in zip(c["spans"], np.diff(c["pred_spans"])))
        assert c["spans"][-1][1] <= len(c["anc_ctrs"]) and c["anc_dirs"].shape == c["anc_ctrs"].shape
    assert DC.selection_cases() is DC.selection_cases() and not DC.selection_cases()["pred"].flags.writeable


def test_agent_rows_cover_every_kind():
    for c in (DC.selection_cases(nan_roi=False), DC.many_agents_case()):
        assert {(d, v) for d, v in zip(c["dir_kind"], c["vel_kind"])} >= {(d, v) for d in DC.DIR_KINDS for v in DC.VEL_KINDS}
        nrm = np.sqrt((c["dir_last"].astype(np.float64) ** 2).sum(1))
        for a, (d, v) in enumerate(zip(c["dir_kind"], c["vel_kind"])):
            assert {"random": nrm[a] > 0.05, "zero": nrm[a] == 0, "below": 0 < nrm[a] < 0.9e-6, "above": 1.1e-6 < nrm[a] < 1e-5}[d]
            assert {"random": 0 < c["agt_vel"][a] <= 15, "zero": c["agt_vel"][a] == 0, "fast": c["agt_vel"][a] == 25}[v]
        # the norm as the kernel forms it (fp32, products rounded on their own) falls on the same side of 1e-6
        d32 = c["dir_last"]
        n32 = np.sqrt(d32[:, 0] * d32[:, 0] + d32[:, 1] * d32[:, 1])
        assert np.array_equal(n32 < np.float32(1e-6), nrm < 1e-6)


def test_grid_exactness(case):
    rows = np.concatenate([np.arange(lo, hi) for lo, hi in case["spans"]])
    anc, off = case["anc_ctrs"][rows], case["pred"][:, 1:3]
    for v in (anc, off):
        assert np.array_equal(v * 4, np.round(v * 4)) and np.abs(v).max() <= 50
    xy32 = anc + off
    assert xy32.dtype == np.float32 and np.array_equal(xy32.astype(np.float64), anc.astype(np.float64) + off.astype(np.float64))
    assert np.array_equal(DC.xy_logit(case)[0], xy32)
    assert (np.abs(off).max(1) > 0).sum() > len(off) // 2              # the offsets matter
    # squared distances to a RoI's first node are exact too (fp32 arithmetic gives the float64 numbers)
    for xy, _ in list(rois(case).values())[:14]:
        d32 = (xy[:, 0] - xy[0, 0]) * (xy[:, 0] - xy[0, 0]) + (xy[:, 1] - xy[0, 1]) * (xy[:, 1] - xy[0, 1])
        x64 = xy.astype(np.float64)
        assert np.array_equal(d32.astype(np.float64), ((x64 - x64[0]) ** 2).sum(1))


def test_both_forms_of_the_greedy_agree(case, full_lists):
    for name, (xy, lg) in rois(case).items():
        cut = DM.greedy(xy, lg, 2.0, K, K)
        assert len(cut) == K and cut == DM.greedy_argmax(xy, lg, 2.0, K, K), name
        if name in full_lists:
            assert full_lists[name][:K] == cut and full_lists[name] == DM.greedy_argmax(xy, lg, 2.0, K, 0), name


def survivors(xy, lg):
    return len(DM.greedy(xy, lg, 2.0, 0, 0))


def test_survivor_counts_and_planted_lists(full_lists):
    r = rois(DC.selection_cases())
    assert survivors(*r["one_disc300"]) == 1 and survivors(*r["two_discs257"]) == 2
    assert survivors(*r["spread600"]) > 256 and survivors(*r["spread1025"]) > 256
    assert all(survivors(*r["spread%d" % n]) >= K for n in (255, 256, 257, 300))
    # distinct logits everywhere but in equal40 (NaNs aside)
    for name, (_, lg) in r.items():
        fin = lg[~np.isnan(lg)]
        assert len(np.unique(fin)) == (1 if name == "equal40" else len(fin)), name
    # one disc: the best node, then the next five by logit; two discs: the pads interleave the two squares
    xy, lg = r["one_disc300"]
    assert full_lists["one_disc300"] == np.argsort(-lg)[:K].tolist()
    assert full_lists["one_disc300"][2] == 299 and full_lists["one_disc300"][4] == 256      # pads from the second pass
    xy, lg = r["two_discs257"]
    top = full_lists["two_discs257"]
    side = (xy[:, 0] > -10).astype(int)
    assert side[top[0]] != side[top[1]] and len(set(side[top[2:]].tolist())) == 2
    assert top[2:] == [i for i in np.argsort(-lg).tolist() if i not in top[:2]][:K - 2] and 256 in top[2:]
    # planted winners; equal logits: lower index first among survivors and among pads
    assert full_lists["planted257"][:K] == list(DC.PLANTED)
    xy, lg = r["equal40"]
    second = int(np.argmax(xy[:, 0] >= 15))
    assert survivors(xy, lg) == 2 and second > 0
    assert full_lists["equal40"] == [0, second] + [i for i in range(40) if i not in (0, second)][:K - 2]
    # NaN logits rank first, the lower index before the higher
    xy, lg = r["nan12"]
    assert np.isnan(lg).sum() == 2 and full_lists["nan12"][:2] == [4, 9] == DM.rank_order(lg)[:2]
    # exactly 2.0 apart: both kept; 1.75 apart: the lower logit is dropped, and there is no padding to bring it back
    xy, lg = r["pairs8"]
    d = lambda i, j: float(np.sqrt(((xy[i].astype(np.float64) - xy[j]) ** 2).sum()))
    assert d(0, 1) == 2.0 and d(2, 3) == 1.75
    assert full_lists["pairs8"] == [0, 1, 2, 4, 5, 6, 7] and full_lists["pairs8"][:K] == [0, 1, 2, 4, 5, 6]


def test_conditioning(case):
    dec = DC.model(case)
    top = dec["top_idx"]
    den = dec["denominators"].abs().numpy()
    finite = ~np.isnan(case["pred"][:, 0])
    assert np.abs(case["pred"][:, 4]).min() >= 0.5
    assert den.min() >= 0.25, den.min()
    coef = dec["coef"]
    pts = DM.poly(torch.arange(0, 31, dtype=torch.float64) / 30, coef)
    seg = torch.sqrt(((pts[:, :, 1:] - pts[:, :, :-1]) ** 2).sum(-1))
    assert float(seg.min()) > 1e-4                                     # no polyline segment of length 0
    v = DC.speeds(seg.sum(-1).numpy(), case["agt_vel"])
    assert np.abs(v[..., 1:]).min() >= DC.SPEED_MARGIN, np.abs(v[..., 1:]).min()
    clamped = (v[..., 1:] < 0).sum(-1)                                  # [A, K]
    fast = [a for a, k in enumerate(case["vel_kind"]) if k == "fast"]
    assert clamped[fast].max() >= 5 and (clamped.sum(1) > 0).sum() >= 1
    assert (clamped == 0).any() and (clamped[fast] < 30).all()          # and unclamped steps remain
    stopped = [a for a, k in enumerate(case["dir_kind"]) if k in ("zero", "below")]
    assert (coef[stopped][..., 1] == 0).all() and (coef[stopped][..., 4] == 0).all() and bool(torch.isfinite(coef).all())
    print("%d agents: min |2 + d - p| %.3f, min |v_j| %.2e, clamped steps %d (most on one agent: %d), NaN logits %d"
          % (len(top), den.min(), np.abs(v[..., 1:]).min(), clamped.sum(), clamped.sum(1).max(), (~finite).sum()))


def test_fp32_model_takes_the_float64_branches_and_sets_the_bars():
    """The bars of the GPU test: 4 x the error of the model run in float32 on the CPU, against float64."""
    for what, c in (("selection", DC.selection_cases(nan_roi=False)), ("many agents", DC.many_agents_case())):
        top = DC.model(c)["top_idx"]
        assert np.array_equal(DC.model(c, torch.float32)["top_idx"], top)          # fp32 selects the same nodes
        for k, (ref, bar) in DC.value_reference(c, top).items():
            print("%-11s %-9s fp32 CPU model bar %.2e" % (what, k, bar))
            assert 1e-6 <= bar <= 1e-4, (what, k, bar)
        ref, bar = DC.d_pred_reference(c, top, DC.upstream(c, 7))
        print("%-11s %-9s fp32 CPU autograd bar %.2e" % (what, "d_pred", bar))
        assert np.isfinite(ref).all() and 1e-6 <= bar <= 1e-3
        chosen = np.zeros(len(ref), dtype=bool)
        for a, lo in enumerate(c["pred_spans"][:-1]):
            chosen[lo + top[a]] = True
        assert (ref[~chosen] == 0).all() and (np.abs(ref[chosen]).max(1) > 0).all()


def test_refine_cases():
    c = DC.refine_cases()
    R = len(DC.REFINE_ROWS)
    assert c["s_samples"].shape == (R, 30) and c["coef"].shape == (R, 6) and c["delta"].shape == (R, 30, 2) and R % K == 0
    assert all(v.dtype == np.float32 for v in c.values())
    row = {n: i for i, n in enumerate(DC.REFINE_ROWS)}
    s32 = c["s_samples"] + c["delta"][..., 0]                                       # the kernel's sum
    s = torch.from_numpy(np.array(c["s_samples"])).double() + torch.from_numpy(np.array(c["delta"])).double()[..., 0]
    u = DM.normalise(s)
    # replaced: the sum is exactly 0 at one step, in fp32 as in float64; that step is not the maximum and becomes 1
    b = row["replaced"]
    assert (s[b] == 0).nonzero().flatten().tolist() == [DC.REPLACED_AT] == np.flatnonzero(s32[b] == 0).tolist()
    assert float(u[b, DC.REPLACED_AT]) == 1.0 and int(s[b].argmax()) != DC.REPLACED_AT
    assert (u[b] == 1).nonzero().flatten().tolist() == sorted([DC.REPLACED_AT, int(s[b].argmax())])
    for n in DC.REFINE_ROWS:
        if n not in ("replaced", "nan"):
            assert (s[row[n]] != 0).all() and (s32[row[n]] != 0).all(), n
    # tied maximum: two arg-max positions; torch.max hands the gradient to the first
    t = row["tied_max"]
    assert (s[t] == s[t].max()).nonzero().flatten().tolist() == list(DC.TIED_AT) and int(s[t].max(-1)[1]) == DC.TIED_AT[0]
    assert (c["delta"][t, :, 0] == 0).all()
    assert float(s[row["negative"]].max()) < 0 and (c["s_samples"][row["negative"]] < 0).all()
    assert (c["s_samples"][row["zero_samples"]] == 0).all() and (c["delta"][row["zero_samples"], :, 0] != 0).all()
    assert float(s[row["zero_samples"]].max()) > 0
    # NaN: one element in, the whole row out
    e = row["nan"]
    assert np.isnan(c["delta"]).sum() == 1 and np.isnan(c["delta"][e, DC.NAN_AT, 0])
    out = DC.refine_model(c)
    assert np.isnan(out[e]).all() and np.isfinite(np.delete(out, e, 0)).all()
    assert np.isfinite(DC.refine_model(DC.refine_inputs(nan=False))).all()
    # besides the tie the two largest sums are well apart, so fp32 and float64 agree on the maximum
    for n in DC.REFINE_ROWS:
        if n not in ("tied_max", "nan"):
            two = torch.sort(s[row[n]])[0][-2:]
            assert float(two[1] - two[0]) >= 1e-2, n
    # the bars of the GPU test
    rows = [n for n in DC.REFINE_ROWS if n != "nan"]
    ci = DC.refine_inputs(rows)
    ref, m32 = DC.refine_model(ci), DC.refine_model(ci, torch.float32)
    for i, n in enumerate(rows):
        print("refine %-12s fp32 CPU model bar %.2e" % (n, DC.bar_of(DM.rel_err(m32[i], ref[i]))))
    w = np.random.default_rng(5).normal(0, 1, ref.shape).astype(np.float32)
    g64, g32 = DC.refine_grads(ci, w), DC.refine_grads(ci, w, torch.float32)
    for name, a, b_ in zip(("d_s_samples", "d_coef", "d_delta"), g32, g64):
        print("refine %-12s fp32 CPU autograd bar %.2e" % (name, DC.bar_of(DM.rel_err(a, b_))))
        assert np.isfinite(b_).all()
    # the replaced step receives nothing: its own path is cut and it is not the maximum
    i = rows.index("replaced")
    assert g64[0][i, DC.REPLACED_AT] == 0 and g64[2][i, DC.REPLACED_AT, 0] == 0 and g64[2][i, DC.REPLACED_AT, 1] != 0
    # the first of the tied maxima carries the maximum's share: the same upstream gradient on both, different results
    i = rows.index("tied_max")
    w2 = w.copy()
    w2[i, DC.TIED_AT[1]] = w2[i, DC.TIED_AT[0]]
    g = DC.refine_grads(ci, w2)[0][i]
    assert g[DC.TIED_AT[0]] != g[DC.TIED_AT[1]]
