"""CPU: the whole-hot-path operand-format model (split_model.hot_path) and its float64 truth, pinned.

(1) split_model.hot_path(model=False) -- the launches of lanegcn.py restated in float64 -- equals the oracle run on double
    tensors to 1e-10 relative: the restatement computes the reference's function (U / V hoisted out of the pair loop, ctx.1
    behind the segment sum, the meta columns beside the 128-column block).
(2) the oracle on double tensors equals the REFERENCE's own float64 run (tests/golden/hotpath_wide_b4.npz) to 1e-10: both
    sides are float64 and differ in operation order only; the smallest effect under test is 1e-7.
(3) the f16x2 model's error per stage over the grid of tests/test_gpu_hot_path_scale.py, within a factor 1.5 of the
    recorded table, and the window it implies: every stage <= 1e-4 while s_w >= 2^-8 (max |W| >= 0.70 * 2^-8), some stage
    above 1e-4 at 2^-10.  The GPU test's bar is built from these figures, so it cannot drift with the model.
(4) oracle.wide_state: what it promises, and a pinned checksum (bit-stable like seeded_state)."""
import os

import numpy as np
import pytest

import hot_path_cases as H
import split_model as S
from conftest import GOLDEN_DIR
from oracle import lanegcn_oracle as O

U = lambda e: ("uniform", e)

# (scenes, state) -> f16x2 model error per stage (map_net, a2m, m2m, m2a, a2a), recorded from this file's own run
TABLE = {
    ("b4", U(0)): (3.27e-7, 4.75e-7, 3.54e-7, 3.59e-7, 2.91e-7),
    ("b4", U(-2)): (1.09e-6, 1.47e-6, 1.06e-6, 1.12e-6, 1.59e-6),
    ("b4", U(-4)): (3.88e-6, 6.34e-6, 4.88e-6, 4.45e-6, 5.15e-6),
    ("b4", U(-6)): (1.63e-5, 2.54e-5, 1.88e-5, 1.92e-5, 2.14e-5),
    ("b4", U(-8)): (6.23e-5, 9.52e-5, 7.46e-5, 6.99e-5, 9.53e-5),
    ("b4", U(-10)): (1.63e-4, 1.71e-4, 1.55e-4, 8.75e-5, 9.67e-5),
    ("b4", H.WIDE): (1.06e-5, 4.24e-5, 4.66e-5, 5.27e-5, 4.28e-5),
    ("b4", ("blocks", -9)): (6.90e-5, 8.23e-5, 8.07e-5, 6.97e-5, 6.48e-5),
    ("s0", U(0)): (3.18e-7, 4.26e-7, 3.19e-7, 3.96e-7, 2.72e-7),
    ("s0", U(-6)): (1.47e-5, 2.78e-5, 1.89e-5, 2.22e-5, 1.83e-5),
}
IDS = ["%s-%s" % (w, H.case_id(s)) for w, s in TABLE]


@pytest.mark.parametrize("which,state", [("b4", U(0)), ("b4", U(-8)), ("b4", H.WIDE), ("s0", U(0))],
                         ids=["b4-seeded", "b4-w2^-8", "b4-wide", "s0-seeded"])
def test_exact_restatement_equals_the_oracle_in_float64(which, state):
    graph, actors, ctrs = H.oracle_inputs(which)
    got = S.hot_path(graph, actors, ctrs, H.state_dict(state), "f32", model=False)
    truth = H.cpu(which, state)["truth"]
    assert truth["map_net"].shape[0] == (486 if which == "b4" else 648) and truth["a2a"].shape[0] == (42 if which == "b4" else 50)
    for k in H.STAGES:
        e = S.rel_err(got[k], truth[k])
        print("HOTPATH exact %s %s %s: %.2e" % (which, H.case_id(state), k, e))
        assert truth[k].dtype == np.float64 and e <= 1e-10, (k, e)


@pytest.mark.parametrize("name,state", [("wide", H.WIDE), ("u-8", U(-8))])
def test_oracle_in_float64_equals_the_reference_fixture(name, state):
    with np.load(os.path.join(GOLDEN_DIR, "hotpath_wide_b4.npz")) as z:
        fx = {k: z[k] for k in z.files if k.startswith(name + "/")}
        margins = {k: float(z[k]) for k in z.files if k.startswith("pair_margin/")}
    seed, e_lo, e_hi, g_lo = fx[name + "/params"][:4]
    assert (seed, e_lo, e_hi) == ((H.SEED, -8, 2) if state == H.WIDE else (H.SEED, -8, -8)) and np.isnan(g_lo) == (state != H.WIDE)
    assert min(margins.values()) > 1e-4        # no pair of the fixture hangs on how a distance is rounded
    c = H.cpu("b4", state)
    for k in H.STAGES:
        t = c["truth"][k]
        if k in ("m2a", "a2a"):
            errs = [S.rel_err(t, fx["%s/%s" % (name, k)])]
        else:
            errs = [S.rel_err(t[::8], fx["%s/%s/rows8" % (name, k)]), S.rel_err(t.sum(0), fx["%s/%s/colsum" % (name, k)])]
        r32 = float(fx["%s/rel32/%s" % (name, k)])
        print("HOTPATH fixture %s %s: oracle64 vs reference64 %s; fp32 vs float64: reference %.2e, oracle %.2e"
              % (name, k, " ".join("%.2e" % e for e in errs), r32, c["e_ref32"][k]))
        assert max(errs) <= 1e-10, (k, errs)
        # the term 4 e_ref32 of the GPU bar: the reference's own fp32 run lies 1e-7 .. 2e-6 from its float64 run
        assert 5e-8 <= r32 <= 2e-6 and 5e-8 <= c["e_ref32"][k] <= 2e-6


@pytest.mark.parametrize("which,state", list(TABLE), ids=IDS)
def test_f16x2_model_table(which, state):
    got = H.model_err(which, state, "f16x2")
    e32 = H.cpu(which, state)["e_ref32"]
    for k, want in zip(H.STAGES, TABLE[(which, state)]):
        print("HOTPATH model %s %s %s: f16x2 %.2e (table %.2e), fp32 oracle %.2e" % (which, H.case_id(state), k, got[k], want, e32[k]))
    for k, want in zip(H.STAGES, TABLE[(which, state)]):
        assert want / 1.5 <= got[k] <= want * 1.5, (k, got[k], want)
        assert e32[k] <= 2e-6, (k, e32[k])


def test_f16x2_whole_path_window():
    """Inside: every stage <= 1e-4 for s_w >= 2^-8, and the heterogeneous state.  Outside: some stage above 1e-4 at 2^-10."""
    for state in [U(e) for e in (0, -2, -4, -6, -8)] + [H.WIDE]:
        worst = max(H.model_err("b4", state, "f16x2").values())
        print("HOTPATH window %s: worst stage %.2e" % (H.case_id(state), worst))
        assert worst <= 1e-4, (state, worst)
    assert max(H.model_err("b4", U(-10), "f16x2").values()) > 1e-4
    # what tools/check_weight_scale.py warns below: EVERY 128-column block at max |W| = 2^-9 is still inside, by 1.2 x
    from tools import check_weight_scale as W
    assert W.W_LOW == 2.0 ** -9 and W.small_blocks(H.state_dict(("blocks", -9))) == []
    assert len(W.small_blocks(H.state_dict(("blocks", -10)))) == 179
    assert max(H.model_err("b4", ("blocks", -9), "f16x2").values()) <= 1e-4
    for which, state in (("s0", U(0)), ("s0", U(-6))):
        assert max(H.model_err(which, state, "f16x2").values()) <= 1e-4


@pytest.mark.parametrize("state", [U(0), U(-10), U(-20), H.WIDE], ids=H.case_id)
def test_bf16x3_model_is_scale_free(state):
    got = H.model_err("b4", state, "bf16x3")
    print("HOTPATH model b4 %s bf16x3: %s" % (H.case_id(state), " ".join("%.2e" % got[k] for k in H.STAGES)))
    assert max(got.values()) <= 3e-7         # fp32 holds between the GEMMs (2^-24 each), no plane effect


def test_bf16_model_is_scale_free():
    """The single-product mode (one bf16 plane: fp32's exponent range, 8 significand bits) over EXACT_GRID: 4e-3 .. 8e-3
    per stage at s_w = 2^0, inside the 2e-2 the project allows that mode, and -- unlike f16x2, whose error grows like
    1 / s_w -- no larger at 2^-10 and 2^-20 (it shrinks there: the float64 function's GroupNorms meet eps and the
    residuals take over)."""
    errs = {st: H.model_err("b4", st, "bf16") for st in H.EXACT_GRID}
    for st, e in errs.items():
        print("HOTPATH model b4 %s bf16: %s" % (H.case_id(st), " ".join("%.2e" % e[k] for k in H.STAGES)))
    base = errs[U(0)]
    assert all(1e-3 <= base[k] <= 2e-2 for k in H.STAGES)               # the model really rounds to 8 bits
    for st, e in errs.items():
        assert all(e[k] <= 1.5 * base[k] for k in H.STAGES), (st, e)


def test_bar():
    assert H.bar(0.0, 0.0) == 1e-6 and H.bar(0.0, 5e-7) == pytest.approx(2e-6)
    assert H.bar(2e-5, 5e-7) == pytest.approx(4e-5) and H.bar(5e-5, 1e-6) == pytest.approx(1e-4)
    assert H.bar(4e-5, 3e-5) == 1e-4                                  # capped inside the window
    assert H.bar(9.5e-5, 5e-7) == pytest.approx(1.9e-4)


def test_wide_state():
    shapes = O.hot_state_shapes()
    base, wide = O.seeded_state(shapes, 3), O.wide_state(shapes, 3, -8, 2)
    again = O.wide_state(list(reversed(shapes))[::2], 3, -8, 2)           # any subset, any order: the same tensors
    assert all(np.array_equal(again[k].numpy(), wide[k].numpy()) for k in again)
    exps, gammas = [], []
    for name, shape in shapes:
        b, w = base[name].numpy().astype(np.float64), wide[name].numpy().astype(np.float64)
        if len(shape) == 2 and shape[1] >= 128:
            r = w / b
            assert np.ptp(r) <= 2e-7 * r.max()                             # one scale per tensor
            exps.append(np.log2(r.mean()))
        elif len(shape) == 2:
            assert shape[1] == 2 and np.array_equal(w, b)                  # the [128, 2] input layers
        elif name.endswith(".weight"):
            gammas.append(w)
        else:
            assert np.array_equal(w, (base[name].numpy() * np.float32(5.0)).astype(np.float64))
    exps, gammas = np.asarray(exps), np.concatenate(gammas)
    assert len(exps) == 167 and -8 <= exps.min() < -7.5 and 1.5 < exps.max() <= 2
    assert 0.05 <= np.abs(gammas).min() < 0.052 and 7.8 < np.abs(gammas).max() <= 8.0
    assert 0.08 <= (gammas < 0).mean() <= 0.12
    assert abs(np.log(np.abs(gammas)).mean() - 0.5 * (np.log(0.05) + np.log(8.0))) <= 0.1
    # the uniform grid: an exact power of two on the matrices, everything else as seeded
    uni = O.wide_state(shapes, 3, -8, -8, g_lo=None)
    for name, shape in shapes:
        scale = 2.0 ** -8 if len(shape) == 2 and shape[1] >= 128 else 1.0
        assert np.array_equal(uni[name].numpy().astype(np.float64), base[name].numpy().astype(np.float64) * scale)
    # pinned: float64 sums of three tensors of the wide state
    pins = {k: float(wide[k].double().sum()) for k in ("m2m.fuse.ctr.0.weight", "a2a.att.1.norm.weight", "map_net.seg.2.norm.bias")}
    print("HOTPATH wide_state pins", {k: "%.17g" % v for k, v in pins.items()})
    assert pins == pytest.approx(PINS, rel=1e-13)          # fp32 values are pinned; only the order of the float64 sum is free


PINS = {"m2m.fuse.ctr.0.weight": -0.058687156226968185, "a2a.att.1.norm.weight": 162.89572195708752,
        "map_net.seg.2.norm.bias": 4.4710897613840643}
