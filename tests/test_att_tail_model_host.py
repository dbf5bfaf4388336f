"""CPU: the Att tail problem of tests/test_gpu_att_tail_scale.py (att_tail_cases) before any kernel sees it.

(1) Every case's model and float64 reference are finite -- the case itself stays inside its format's range (the 40-pair
    target is left out in f16x2 at s_x = 2^12, where its sum passes 65504) -- and the pair counts are the ones the
    kernels' gather loops branch on.
(2) split_model.bar separates the bf16 model -- the weakest format, so the widest bar -- from a wrong kernel: a GEMM
    that drops one K-step (32 weight columns) and a GroupNorm that returns beta land far above twice the model's
    error.  (The bar does NOT separate truncation from round-to-nearest in this mode -- 1.14 x measured -- and this file
    does not claim so: the elementwise check of the GPU test does that.)
(3) The RANGE16 source: its piece sums restate the same segment sums."""
import numpy as np
import pytest

import att_tail_cases as A
import split_model as S


@pytest.mark.parametrize("mode,ex,ew", A.CASES, ids=A.IDS)
def test_every_case_stays_in_range(mode, ex, ew):
    for T in A.ROWS:
        c = A.problem(mode, ex, ew, T)
        cnt = np.diff(c["rowptr"].numpy())
        assert c["P"] == len(c["hi"]) == cnt.sum() and c["res"].abs().max() < 8 and not c["res"].equal(c["a"])
        if T >= 49:
            assert set(A.COUNTS) <= set(cnt.tolist())
            assert (A.BIG in cnt) == (not (mode == "f16x2" and ex == 12))
        for rel16 in (False, True):
            model, ref = A.tail(mode, ex, ew, T, True, rel16), A.tail(mode, ex, ew, T, False)
            for k in A.TENSORS:
                assert np.isfinite(model[k]).all() and np.isfinite(ref[k]).all(), (T, rel16, k)
                assert np.abs(ref[k]).max() > 0
        if mode == "f16x2":
            assert float(S.seg_sum(c["m"][:c["P"]], c["hi"], T).max(initial=0)) < 65504
    if mode == "f16x2" and ex == 12:                      # the sum that was left out does leave fp16's range
        for T in A.ROWS[1:]:
            b = int(A.counts(T)[:T // 2].sum())
            assert float(A.tail_draw()["m"][b:b + A.BIG].double().sum(0).max()) * 2.0 ** ex > 65504


@pytest.mark.parametrize("ex,ew", A.WIDE_GRID, ids=["x2^%d-w2^%d" % c for c in A.WIDE_GRID])
def test_bar_rejects_broken_variants_of_the_bf16_model(ex, ew):
    T = 130
    c = A.problem("bf16", ex, ew, T)
    ref, good = A.tail("bf16", ex, ew, T, False), A.tail("bf16", ex, ew, T)
    e_m = S.rel_err(good["out"], ref["out"])
    print("\nATTTAIL bf16 x2^%d w2^%d out: model %.2e bar %.2e" % (ex, ew, e_m, S.bar(e_m)))
    assert 1e-4 <= e_m <= 1e-2                               # 8 significand bits per operand, damped where eps weighs in
    # stage 1 is live only where GN1's variance stands above eps: at (2^-100, 2^80) and (2^-8, 2^-8) the stage-1 sums are
    # ~2^-20 / ~2^-16, GN1 returns ~beta in float64 too, and a K-step dropped there cannot show
    live1 = ex + ew > 0
    broken = {"%s K-step %d dropped" % (w, s): dict(drop_kstep=(w, s)) for w in ("w_agt", "w2")[0 if live1 else 1:] for s in (0, 3)}
    broken["GN2 returns beta"] = dict(gn2_is_beta=True)
    for what, kw in broken.items():
        e = S.rel_err(A.tail_values(c, "bf16", **kw)["out"], ref["out"])
        print("ATTTAIL bf16 x2^%d w2^%d out: %s %.2e" % (ex, ew, what, e))
        assert e > 10 * S.bar(e_m), what
    # the chained outputs sit behind `out`: a tail that is wrong there is wrong in U and V too
    bad = A.tail_values(c, "bf16", gn2_is_beta=True)
    for k in ("U", "V"):
        assert S.rel_err(bad[k], ref[k]) > 10 * S.bar(S.rel_err(good[k], ref[k])), k


@pytest.mark.parametrize("T", A.ROWS)
def test_range16_pieces_hold_the_segment_sums(T):
    c = A.problem("bf16x3", -8, -8, T)
    m16, starts = c["m16"].numpy(), c["pieces"]
    rp = c["rowptr"].numpy()
    want = sorted({int(b) for b, e in zip(rp[:-1], rp[1:]) if b < e} |
                  {r for b, e in zip(rp[:-1], rp[1:]) for r in range(int(b) + 1, int(e)) if r % 16 == 0})
    assert starts.tolist() == want
    if c["P"]:
        assert np.isnan(np.delete(m16, starts, 0)).all() and np.isfinite(m16[starts]).all()
        assert T < 49 or len(starts) < c["P"] and any(s % 16 == 0 and s not in rp for s in starts)     # a segment is cut
    full, pieces = A.seg(c, True), A.seg(c, True, rel16=True)
    assert np.abs(full - pieces).max() <= 2.0 ** -22 * max(np.abs(full).max(), 1e-30)
