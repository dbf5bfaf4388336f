"""CPU: the float64 model of the split-precision operand formats (tests/split_model.py) pinned against the figures the
operand-scale work started from, so that the bar of tests/test_gpu_operand_scale.py cannot drift with the model.

The case: a 96 x 128 post-ReLU N(0, 1) input times a 128 x 128 weight N(0, 1 / 128) * 1.5 (oracle.seeded_state's
matrices), one of them scaled by an exact power of two; error = max |model - fp64| / max |fp64|.  TABLE_W / TABLE_X are
the recorded figures; the draw is np.random.RandomState(13) (max |W| = 0.500 as in the table's header).  Over the seeds
0..39 the same figures move by a factor 0.85 .. 1.8 of the table (they are maxima over 12,288 outputs), so the factor 1.5
pins this draw, not every draw."""
import numpy as np
import pytest

import split_model as S

# s -> model error of f16x2, weight scaled (max |W| = s / 2) / input scaled
TABLE_W = {0: 1.2e-7, -4: 1.7e-6, -6: 6.4e-6, -8: 3.2e-5, -10: 9.3e-5, -12: 4.2e-4, -16: 6.2e-3}
TABLE_X = {-2: 1.2e-7, -8: 3.8e-6, -12: 5.7e-5, -14: 2.0e-4}


@pytest.fixture(scope="module")
def draw():
    rs = np.random.RandomState(13)
    x = np.maximum(rs.standard_normal((96, 128)), 0).astype(np.float32)
    w = (rs.standard_normal((128, 128)) * 1.5 / np.sqrt(128)).astype(np.float32)
    return x, w


def scaled(a, e):
    out = a * np.float32(2.0 ** e)
    assert np.array_equal(out.astype(np.float64), a.astype(np.float64) * 2.0 ** e)       # exact: no fp32 underflow
    return out


def model_err(x, w, mode):
    return S.rel_err(S.mm(x, w, mode), S.mm(x, w, "f32"))


@pytest.mark.parametrize("e,want", sorted(TABLE_W.items()))
def test_f16x2_weight_scale_table(draw, e, want):
    x, w = draw
    got = model_err(x, scaled(w, e), "f16x2")
    print("f16x2 s_w = 2^%d: model %.2e, table %.2e" % (e, got, want))
    assert want / 1.5 <= got <= want * 1.5


@pytest.mark.parametrize("e,want", sorted(TABLE_X.items()))
def test_f16x2_input_scale_table(draw, e, want):
    x, w = draw
    got = model_err(scaled(x, e), w, "f16x2")
    print("f16x2 s_x = 2^%d: model %.2e, table %.2e" % (e, got, want))
    assert want / 1.5 <= got <= want * 1.5


def test_bf16x3_is_scale_free(draw):
    x, w = draw
    errs = {e: model_err(x, scaled(w, e), "bf16x3") for e in range(-40, 17, 4)}
    errs.update({("x", e): model_err(scaled(x, e), w, "bf16x3") for e in range(-40, 17, 4)})
    print("bf16x3 model: %.2e .. %.2e" % (min(errs.values()), max(errs.values())))
    assert max(errs.values()) <= 2e-8


def test_bf16_is_one_rne_plane_and_one_product(draw):
    """LGCN_MMA_BF16 (Fmt<2>): NP = 1, PA = PB = {0} -- the one plane is the RNE rounding itself, nothing is left over."""
    assert S.FORMATS["bf16"] == ("bf16", 1, (0,), (0,)) and "bf16" in S.MODES
    x, w = draw
    v = np.concatenate([x.ravel(), w.ravel(), np.array([1.0 + 2.0 ** -8, 1.0 + 3 * 2.0 ** -8, 1.2345678 * 2.0 ** -100, 2.0 ** -130],
                                                       np.float32)])
    p = S.planes(v, "bf16")
    assert len(p) == 1 and np.array_equal(p[0], S.round16(v, "bf16").astype(np.float64))
    assert p[0][-4:-2].tolist() == [1.0, 1.0 + 2.0 ** -6] and p[0][-1] == 2.0 ** -130       # ties to even; a bf16 subnormal survives
    assert abs(p[0][-2] / (1.2345678 * 2.0 ** -100) - 1) <= 2.0 ** -9 and p[0][-2] * 2.0 ** 100 * 128 % 1 == 0     # 8 bits at 2^-100
    # the product is that of the rounded operands, in float64
    want = S.round16(x, "bf16").astype(np.float64) @ S.round16(w, "bf16").astype(np.float64).T
    assert np.array_equal(S.mm(x, w, "bf16"), want)


def test_bf16_is_scale_free(draw):
    """One bf16 plane has fp32's exponent range: the model's error (8 significand bits per operand) does not move with a
    power-of-two scale on either operand, as bf16x3's does not."""
    x, w = draw
    base = model_err(x, w, "bf16")
    errs = {(ex, ew): model_err(scaled(x, ex), scaled(w, ew), "bf16") for ex, ew in ((0, 0), (-100, 80), (-8, -8))}
    print("bf16 model: %s" % " ".join("%.3e" % e for e in errs.values()))
    assert 5e-4 <= base <= 1e-2                            # 2^-9 per operand over a 128-term sum of mixed signs
    assert all(abs(e - base) <= 1e-12 * base for e in errs.values())


def test_planes_are_rne_with_fp32_residual_and_subnormals():
    # fp16: 2049 is a tie (2048 | 2050) -> even 2048, residual 1; 2^-20 is subnormal in fp16 and must survive;
    # 2^-25 rounds to zero in the first plane (half the smallest subnormal: tie to even) and is gone
    p = S.planes(np.array([2049.0, 2.0 ** -20, 2.0 ** -25, 65504.0, 65519.0], np.float32), "f16x2")
    assert p[0].tolist() == [2048.0, 2.0 ** -20, 0.0, 65504.0, 65504.0]
    assert p[1].tolist() == [1.0, 0.0, 0.0, 0.0, 15.0]
    # 65520 is the first fp32 value that rounds to fp16's infinity
    assert np.isinf(S.planes(np.array([65520.0], np.float32), "f16x2")[0][0])
    # bf16: 1 + 2^-8 is a tie -> 1; three planes carry 24 bits exactly
    v = np.array([1.0 + 2.0 ** -8, 1.0 + 2.0 ** -8 + 2.0 ** -16 + 2.0 ** -23, 1.2345678 * 2.0 ** -100], np.float32)
    q = S.planes(v, "bf16x3")
    assert q[0][0] == 1.0 and q[1][0] == 2.0 ** -8
    assert (q[0] + q[1] + q[2]).tolist() == v.astype(np.float64).tolist()


def test_restatements_reduce_to_the_reference_in_f32():
    """Every restatement with model=False is the float64 value; the f32 model differs from it only where a kernel holds
    an intermediate in fp32 (2^-24 relative)."""
    rs = np.random.RandomState(5)
    n = 33
    x = rs.standard_normal((n, 128)).astype(np.float32)
    w = [(rs.standard_normal((128, 128)) * 0.13).astype(np.float32) for _ in range(3)]
    g = (1 + 0.1 * rs.standard_normal(128)).astype(np.float32), (0.1 * rs.standard_normal(128)).astype(np.float32)
    edges = (rs.randint(0, n, 90), rs.randint(0, n, 90))
    units = [(w[0], None), (w[1], edges)]
    ref = S.lane_conv(x, units, g, w[2], g, "f32", model=False)
    assert S.rel_err(S.lane_conv(x, units, g, w[2], g, "f32"), ref) <= 2e-7
    assert 1e-8 <= S.rel_err(S.lane_conv(x, units, g, w[2], g, "f16x2"), ref) <= 1e-5
    # the gathered sum against a plain loop
    want = np.zeros((n, 128))
    for u, v in zip(*edges):
        want[u] += x[v]
    assert np.abs(S.gather_sum(x, edges, n, model=False) - want).max() <= 1e-12
    # a k = 3, stride 2 convolution against a plain loop
    xa = rs.standard_normal((2, 20, 5)).astype(np.float32)
    wc = rs.standard_normal((32, 5, 3)).astype(np.float32)
    _, y = S.conv1d_unit(xa, wc, 2, np.ones(32), np.zeros(32), "f32", model=False)
    assert y.shape == (2, 10, 32)
    for l in (0, 9):
        acc = np.zeros(32)
        for t in range(3):
            li = 2 * l + t - 1
            if 0 <= li < 20:
                acc += wc[:, :, t].astype(np.float64) @ xa[1, li].astype(np.float64)
        assert np.abs(y[1, l] - acc).max() <= 1e-12


def test_bar():
    assert S.bar(0.0) == 1e-6 and S.bar(1e-7) == 1e-6
    assert S.bar(2e-5) == pytest.approx(4e-5)
    assert S.bar(5e-5) == pytest.approx(1e-4)
    assert S.bar(6e-3) == pytest.approx(1.2e-2)
