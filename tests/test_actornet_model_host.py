"""CPU: the float64 model of ActorNet's conv path (split_model.conv1d_unit with residuals, res1d_block, actor_net) pinned
against the stock modules, so that the bars of tests/test_gpu_actornet_scale.py cannot drift with the model.

  model=False   equals layers.Res1d / layers.Conv1d / ActorNet run in double: both sides are float64 evaluations of the same
                formulas on the same fp32 parameters and differ by the rounding of float64 sums only (ATen's convolution
                and GroupNorm sum in another order).  Bar 1e-12; measured 1.2e-15 for a unit, 7.5e-16 for a block or a
                group, 1.2e-15 for the whole module (max |diff| / max |ref|).
  mode "f32"    the model IS the reference: error exactly 0 (nothing is rounded to 16-bit planes).
  mode "f16x2"  at scale 1 the model sits in the 1e-7 range (5e-8 .. 1e-6 asserted), as the conv rows of DESIGN.md 5c do;
                at w x 2^-16 it has left the 1e-4 window, which is why the GPU bars follow the model and not a constant.
Also here: the x2 upsampling against F.interpolate, the range condition of the cases (reference and model finite at every
state) and that the states are what actornet_cases says they are."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import actornet_cases as AC
import split_model as S

STATE0 = ("uniform", 0)


def test_up2_linear_is_interpolate():
    for n in (1, 2, 5, 10):
        r = torch.randn(3, n, 4, dtype=torch.float64)
        want = F.interpolate(r.transpose(1, 2), scale_factor=2, mode="linear", align_corners=False).transpose(1, 2)
        got = S.up2_linear(r)
        assert got.shape == (3, 2 * n, 4) and np.abs(got - want.numpy()).max() <= 1e-15
    r = np.arange(5, dtype=np.float64).reshape(1, 5, 1)
    up = S.up2_linear(r)[0, :, 0]
    assert up[0] == 0.0 and up[1] == 0.25 and up[2] == 0.75 and up[-1] == 4.0 and up[-2] == 3.75      # 0.75 / 0.25, ends clamped


def unit_shapes():
    import test_gpu_actornet_train as T
    return sorted(set(T.unit_shapes(AC.modules())))


def test_unit_shapes_are_actornets():
    shapes = unit_shapes()
    assert len(shapes) == 12 and (3, 32, 1, 1, 20) in shapes and (128, 128, 3, 1, 5) in shapes and (64, 128, 1, 2, 10) in shapes


@pytest.mark.parametrize("res_mode", [0, 1, 2])
@pytest.mark.parametrize("relu", [False, True])
def test_unit_reference_is_the_stock_unit_in_double(res_mode, relu):
    worst = 0.0
    for shape in unit_shapes():
        cin, cout, ks, stride, lin = shape
        lout = (lin + 2 * ((ks - 1) // 2) - ks) // stride + 1
        if res_mode == 2 and lout % 2:
            continue
        x, w, stride, gamma, beta, res = AC.unit_case(shape, 3, STATE0, res_mode)
        out, y = S.conv1d_unit(x, w, stride, gamma, beta, "f32", relu=relu, res=res, res_up2=res_mode == 2, model=False)
        yd = F.conv1d(x.double().transpose(1, 2), w.double(), stride=stride, padding=(ks - 1) // 2)
        want = F.group_norm(yd, 1, gamma.double(), beta.double(), S.EPS)
        if res is not None:
            r = res.double().transpose(1, 2)
            want = want + (F.interpolate(r, scale_factor=2, mode="linear", align_corners=False) if res_mode == 2 else r)
        want = want.relu() if relu else want
        worst = max(worst, S.rel_err(out, want.transpose(1, 2)), S.rel_err(y, yd.transpose(1, 2)))
        # mode "f32" as a model is the same float64 value: error exactly 0
        m_out, m_y = S.conv1d_unit(x, w, stride, gamma, beta, "f32", relu=relu, res=res, res_up2=res_mode == 2)
        assert np.array_equal(m_out, out) and np.array_equal(m_y, y)
    print("units res_mode %d relu %d: reference against stock double %.2e" % (res_mode, relu, worst))
    assert worst <= 1e-12


@pytest.mark.parametrize("path,lin", AC.BLOCKS + AC.GROUPS, ids=[p for p, _ in AC.BLOCKS + AC.GROUPS])
def test_block_reference_and_model(path, lin):
    """Identity shortcut (groups.*.1, output), k = 1 downsample shortcut (groups.*.0) and the chained C -> C block."""
    sd = AC.state_dict(STATE0)
    x = AC.block_input(path, lin, 5, STATE0)
    d = AC.block_dicts(sd, path)
    second = d[1] if len(d) == 2 else None
    assert (d[0].get("wd") is not None) == path.endswith(".0") or len(d) == 2
    with torch.no_grad():
        want = AC.submodule(AC.make_net(sd, double=True), path)(x.transpose(1, 2).double()).transpose(1, 2).numpy()
    ref = S.res1d_block(x, d[0], "f32", second=second, model=False)
    e_ref = S.rel_err(ref, want)
    assert np.array_equal(S.res1d_block(x, d[0], "f32", second=second), ref)                   # mode f32: error 0
    e_model = S.rel_err(S.res1d_block(x, d[0], "f16x2", second=second), want)
    print("%s: reference against stock double %.2e, f16x2 model %.2e" % (path, e_ref, e_model))
    assert ref.shape == want.shape and e_ref <= 1e-12
    assert 5e-8 <= e_model <= 1e-6


@pytest.mark.parametrize("draw", AC.DRAWS)
def test_actor_net_reference_and_model(draw):
    sd, x = AC.state_dict(STATE0), AC.inputs(draw, 17)
    with torch.no_grad():
        want = AC.make_net(sd, double=True)(x.double()).numpy()
    ref = S.actor_net(x, sd, "f32", model=False)
    e_ref = S.rel_err(ref, want)
    assert np.array_equal(S.actor_net(x, sd, "f32"), ref)                                      # mode f32: error 0
    c = AC.net_cpu(draw, 17, STATE0)
    print("ActorNet %s: reference against stock double %.2e, f16x2 model %.2e, fp32 stock %.2e" % (draw, e_ref, c["e_model"],
                                                                                                 c["e_ref32"]))
    assert ref.shape == (17, 128) and e_ref <= 1e-12
    assert np.array_equal(c["truth"], want)
    assert 5e-8 <= c["e_model"] <= 1e-6


def test_a_dropped_plane_or_swapped_taps_leaves_the_model():
    """What the GPU bars must catch, on the model itself: the second plane of the intermediate rows dropped (its rows
    rounded to ONE fp16 plane), and the 0.75 / 0.25 taps swapped, both move the result by far more than any bar.  (On
    the GPU the dropped plane also fails the older absolute 1e-4 of test_actor_net_hip_conv_path: DESIGN.md 5c.)"""
    sd = AC.state_dict(STATE0)
    d = AC.block_dicts(sd, "groups.1.1")[0]
    x = AC.block_input("groups.1.1", 10, 5, STATE0)
    ref = S.res1d_block(x, d, "f32", model=False)
    mid = S.conv1d_unit(x, d["w1"], 1, *d["gn1"], "f16x2", relu=True)[0]
    one_plane = S.round16(S.f32(mid), "f16")
    out = S.conv1d_unit(one_plane, d["w2"], 1, *d["gn2"], "f16x2", relu=True, res=x)[0]
    e = S.rel_err(out, ref)
    print("one plane of the intermediate rows: %.2e" % e)
    assert 2e-5 <= e <= 5e-4                                    # fp16's 2^-11 through one GEMM + GroupNorm: 1.3e-4 here
    assert e > 10 * AC.bar(S.rel_err(S.res1d_block(x, d, "f16x2"), ref), 1e-7)
    r = np.random.RandomState(0).standard_normal((2, 5, 4))
    up = S.up2_linear(r)
    swapped = up.copy()
    swapped[:, 1:-1] = up[:, 1:-1].reshape(2, 4, 2, 4)[:, :, ::-1].reshape(2, 8, 4)
    assert S.rel_err(swapped, up) > 0.1


@pytest.mark.parametrize("state", AC.STATES, ids=[AC.case_id(s) for s in AC.STATES])
def test_range_condition_and_model_figures(state):
    """Every state keeps the reference and the model finite (net_cpu / block_cpu assert it) at A = 17; prints the figures
    the GPU bars are built from."""
    for draw in AC.DRAWS:
        c = AC.net_cpu(draw, 17, state)
        print("ActorNet %s %s: model %.3e fp32 stock %.3e" % (AC.case_id(state), draw, c["e_model"], c["e_ref32"]))
        assert np.isfinite(c["e_model"]) and np.isfinite(c["e_ref32"])
    for path, lin in AC.GROUPS:
        c = AC.block_cpu(path, lin, 17, state)
        print("%s %s: model %.3e fp32 stock %.3e" % (path, AC.case_id(state), c["e_model"], c["e_ref32"]))
    assert float(AC.scaled_input("randn", 17, state).abs().max()) < 65520.0


def test_states_are_what_they_say():
    base = AC.state_dict(STATE0)
    convs = [k for k, v in base.items() if v.dim() == 3]
    assert len(convs) == 20 and len(base) == 60
    for e in (-4, -16):
        sd = AC.state_dict(("uniform", e))
        assert all(torch.equal(sd[k], base[k] * 2.0 ** e) for k in convs)
        assert all(torch.equal(sd[k], base[k]) for k in base if k not in convs)
    assert all(torch.equal(AC.state_dict(("input", 12))[k], base[k]) for k in base)
    assert torch.equal(AC.scaled_input("randn", 17, ("input", 12)), AC.inputs("randn", 17) * 4096.0)
    wide = AC.state_dict(AC.WIDE)
    ratios = [float((wide[k] / base[k]).median()) for k in convs]
    assert all(2.0 ** -8 <= r <= 4.0 for r in ratios) and len(set(ratios)) == 20                # one scale per tensor
    gam = torch.cat([wide[k] for k in wide if wide[k].dim() == 1 and k.endswith(".weight")])
    assert 0.05 <= float(gam.abs().min()) and float(gam.abs().max()) <= 8.0 and 0.03 < float((gam < 0).float().mean()) < 0.2
    x = AC.inputs("track", 17)
    assert float(x[0, :, :19].abs().max()) == 0 and float(x[2, :, :13].abs().max()) == 0 and float(x[2, 2, 13:].min()) == 1
    assert torch.equal(x[3, :2], torch.zeros(2, 20)) and set(x[:, 2].unique().tolist()) == {0.0, 1.0}
