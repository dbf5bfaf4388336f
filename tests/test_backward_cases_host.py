"""CPU: the builders and float64 references of backward_cases.py -- every reference is stock float64 autograd to 1e-12, every
row class has the statistic it is named for, stock fp32 autograd stays within 1e-5 of float64 on every row tensor (so the inputs excuse
no failure of a kernel there), and the stock fp32 block is bitwise homogeneous in its incoming gradient at the three scales."""
import math

import pytest
import torch

import backward_cases as B


def worst(ref, stock):
    assert set(k for k, v in ref.items() if v is not None) == set(k for k, v in stock.items() if v is not None)
    return max(B.rel_err(ref[k], stock[k]) for k in ref if ref[k] is not None)


def assert_classes(rows, cls):
    """rows [n, width]: variance and mean per class."""
    rows = rows.double().reshape(rows.shape[0], -1)
    var, mean = rows.var(1, unbiased=False), rows.mean(1)
    sel = lambda name: cls == B.CLASSES.index(name)
    assert bool((var[sel("ordinary")] > 1000 * B.EPS).all()) and bool((var[sel("dead")] > 1000 * B.EPS).all())
    assert bool((var[sel("flat")] < B.EPS / 10).all()) and bool((var[sel("flat")] > 0).all())
    assert bool((mean[sel("offset")].abs() > 500 * var[sel("offset")].sqrt()).all())
    assert bool((var[sel("constant")] == 0).all())
    assert sel("constant").sum() < 2 or bool((rows[sel("constant")] == 0).all(1).any())


def test_row_classes_have_their_statistics():
    cls = B.row_class(B.N_ROWS)
    for c in range(len(B.CLASSES)):
        for tile in range(0, B.N_ROWS, 32):
            assert bool((cls[tile:tile + 32] == c).any()) or tile + 32 > B.N_ROWS        # every class in every full tile
    assert_classes(B.class_rows(B.N_ROWS, 1), cls)
    assert_classes(B.gn_case()["x"], cls)
    assert_classes(B.rowblock_case("b")["pre"], cls)
    lc = B.laneconv_case(True)
    assert_classes(lc["T"], cls)
    assert_classes(lc["Z"], cls)
    for shape in ((5, 128, 5), (37, 64, 10)):
        case = B.gn_cl_case(*shape)
        assert_classes(case["x"], case["cls"])
    for unit in B.CONV_UNITS:
        case = B.conv_case(unit)
        assert_classes(case["y"], case["cls"])


def test_gamma_and_masks_are_mixed():
    gamma, beta = B.gamma_beta(3)
    mag = gamma[gamma != 0].abs()
    assert int((gamma == 0).sum()) == 2 and bool((gamma < 0).any()) and bool((gamma > 0).any())
    assert float(mag.min()) >= 2.0 ** -8 and float(mag.max()) <= 4.0 and float(mag.min()) < 2.0 ** -6 and float(mag.max()) > 1.0
    for case, key in ((B.gn_case(), "post"), (B.rowblock_case("b"), "out"), (B.laneconv_case(True), "out"), (B.laneconv_case(True), "Y")):
        live = case[key][case["cls"] != B.CLASSES.index("dead")] > 0
        assert 0.2 < float(live.float().mean()) < 0.8
        if key != "Y":
            assert bool((case[key][case["cls"] == B.CLASSES.index("dead")] <= 0).all())


@pytest.mark.parametrize("build,stock,ref", [
    (lambda: B.gn_case(), B.gn_stock, B.gn_reference64),
    (lambda: B.rowblock_case("a"), B.rowblock_stock, B.rowblock_reference64),
    (lambda: B.rowblock_case("b", 2.0 ** -12), B.rowblock_stock, B.rowblock_reference64),
    (lambda: B.rowblock_case("d", 2.0 ** 4), B.rowblock_stock, B.rowblock_reference64),
    (lambda: B.rowblock_case("g"), B.rowblock_stock, B.rowblock_reference64),
    (lambda: B.laneconv_case(True), B.laneconv_stock, B.laneconv_reference64),
    (lambda: B.laneconv_case(False, 2.0 ** -12), B.laneconv_stock, B.laneconv_reference64),
    (lambda: B.laneconv_case(True, 2.0 ** 4), B.laneconv_stock, B.laneconv_reference64),
    (lambda: B.gn_cl_case(5, 128, 5), B.gn_cl_stock, B.gn_cl_reference64),
    (lambda: B.gn_cl_case(37, 64, 10), B.gn_cl_stock, B.gn_cl_reference64),
    (lambda: B.conv_case("3-32-k3-s1"), B.conv_stock, B.conv_reference64),
    (lambda: B.conv_case("32-64-k3-s2"), B.conv_stock, B.conv_reference64),
    (lambda: B.conv_case("128-128-k1-up2"), B.conv_stock, B.conv_reference64),
], ids=["gn", "rb-a", "rb-b-w2^-12", "rb-d-w2^4", "rb-g", "lc-ident1", "lc-rel-w2^-12", "lc-ident1-w2^4", "gn_cl-5", "gn_cl-37",
        "conv-3-32", "conv-32-64-s2", "conv-128-up2"])
def test_references_are_stock_float64_autograd(build, stock, ref):
    """The header's formulas in float64 against stock float64 autograd to 1e-12; stock fp32 autograd against them per tensor,
    printed: the comparison path's error on these statistics."""
    case = build()
    r64, s64, s32 = ref(case), stock(case, torch.float64), stock(case, torch.float32)
    e = worst(r64, s64)
    assert e <= 1e-12, e
    for k, v in r64.items():
        if v is None:
            continue
        e32 = B.rel_err(s32[k], v)
        print("%-8s stock fp32 against float64 %.3e" % (k, e32))
        # row tensors: the inputs excuse no failure.  Parameter gradients sum g * xhat over the rows, and on the offset rows
        # the fp32 mean alone is off by up to half an ulp of 2^10 (6e-5) against a spread of 1, which goes straight into xhat
        assert e32 <= (1e-5 if v.dim() > 1 and v.shape[0] == case["cls"].shape[0] else 1e-3), (k, e32)
    dead = case["cls"] == B.CLASSES.index("dead")
    for k in ("dx", "g", "d res", "dT", "g2", "dX"):
        if r64.get(k) is not None and r64[k].shape[0] == dead.shape[0]:
            assert bool((r64[k][dead] == 0).all()), k


def test_huge_rows_have_a_finite_reference():
    """Part C's rows of magnitude 2^70: the float64 reference is finite and non-zero, while stock fp32 (whose sum of squares
    overflows) is not a usable comparison, so the bar of that case is its 1e-4 ceiling."""
    for case, ref in ((B.gn_case(huge=True), B.gn_reference64), (B.rowblock_case("b", huge=True), B.rowblock_reference64),
                      (B.laneconv_case(False, huge=True), B.laneconv_reference64)):
        r = ref(case)
        assert all(bool(torch.isfinite(v).all()) and float(v.abs().max()) > 0 for v in r.values())
    r = B.gn_reference64(B.gn_case(huge=True))
    assert 1e-23 < float(r["dx"].abs().max()) < 1e-18                 # rstd ~ 2^-70: inside fp32's normal range
    r = B.laneconv_reference64(B.laneconv_case(False, huge=True))
    live = r["dT"][r["dT"] != 0].abs()
    assert float(live.min()) > 1e-30 and 1e-24 < float(r["dT"].abs().max()) < 1e-15      # never rstd1 rstd2 = 2^-140 in one row
    assert math.isfinite(B.bar(1e-7)) and B.bar(float("nan")) == 1e-4 and B.bar(float("inf")) == 1e-4


@pytest.mark.parametrize("kind", ["ordinary", "flat", "offset", "constant"])
def test_stock_fp32_block_is_bitwise_homogeneous(kind):
    """Stock fp32 autograd of ReLU(GN(x W^T) + res) on 130 rows: grad(2^k d_out) == 2^k grad(d_out) bit for bit at k = -40,
    -20, +20, and the smallest non-zero entry at k = -40 is far above fp32's subnormals."""
    g = torch.Generator().manual_seed(5)
    n = 130
    x = torch.randn(n, B.C, generator=g)
    w = torch.randn(B.C, B.C, generator=g) * 0.08
    if kind == "flat":
        x = torch.randn(n, 1, generator=g) + 2.0 ** -12 * x
        w = torch.eye(B.C)
    elif kind == "offset":
        x, w = 2.0 ** 10 + x, torch.eye(B.C)
    elif kind == "constant":
        x, w = torch.randn(n, 1, generator=g).expand(n, B.C).contiguous(), torch.eye(B.C)
    gamma, beta = B.gamma_beta(17)
    leaves = dict(x=x, w=w, gamma=gamma, beta=beta, res=torch.randn(n, B.C, generator=g))
    leaves = {k: v.clone().requires_grad_(True) for k, v in leaves.items()}
    out = B.stock_block(*leaves.values())
    d_out = torch.randn(n, B.C, generator=g)
    bad, base = B.homogeneous([out], leaves, [d_out])
    assert not bad, bad
    small = min(float(v[v != 0].abs().min()) for v in base.values() if bool((v != 0).any()))
    assert small * 2.0 ** -40 > 1e-30, small


def test_homogeneous_sees_an_absolute_threshold():
    """The check's own control on the CPU: a backward that flushes gradients below 1e-10 is reported at k = -40 only."""

    class Flush(torch.autograd.Function):
        @staticmethod
        def forward(ctx, x):
            return x * 2

        @staticmethod
        def backward(ctx, g):
            return torch.where(g.abs() < 1e-10, torch.zeros_like(g), g * 2)

    x = torch.randn(8, 4).requires_grad_(True)
    bad, _ = B.homogeneous([Flush.apply(x)], dict(x=x), [torch.randn(8, 4)])
    assert bad == [(-40, "x")]
