"""GPU: lgcn_pool_pairs, the pair stage of the fork's LanePooling in one exact-fp32 launch, against the float64 model of
tests/pool_pairs_model.py at the project's bar for exact-fp32 kernels (test_gpu_att_train.py): rel_err <= min(max(2 x the
error of today's composed path in f32 mode on the same inputs, 1e-6), 1e-4), both errors printed; rows past the pair count
untouched; repeatable and independent of the matrix mode; and LanePooling.fused at module level against the reference's
captures pool/out, ia/out and dec/pooled and against the switch-off output.

Pair sets are made by hand: T = 5 target rows and S = 9 context rows with repeated indices, cap = P + 7 with far-out-of-range
garbage indices and sentinel rows of m past the count; P = 1, 31, 32, 33 (one side of, and across, the 32-pair tile), 95
(three tiles, the last ragged) and 65537 (2049 tiles on the 2048 workgroups of the launch's grid-stride loop: workgroup 0
runs a second tile).  Poses are multiples of 1/64 m in [0, 4), so every difference is exact in fp32 with or without the
shift by 1e3 m."""
import json
import os

import numpy as np
import pytest
import torch

import decode_model as DM
import pool_pairs_model as PM
import test_gpu_lanercnn_heads as TH
from conftest import GOLDEN_DIR
from oracle import lanercnn_oracle as OR
from test_gpu_lanercnn_heads import mma  # noqa: F401  (fixture: the three matrix modes that claim fp32 parity)
from test_lanercnn import inputs

pytestmark = pytest.mark.gpu
T, S, C = 5, 9, 128
PAD, GARBAGE, SENTINEL = 7, 1 << 30, -777.0
FTOL = 1e-4
EPS = 1e-5


@pytest.fixture(scope="module")
def mods():
    import lanegcn_amd  # noqa: F401
    from lanegcn_amd import _lib as L
    from lanegcn_amd import lanegcn as M
    from lanegcn_amd import lanercnn as R
    from lanegcn_amd import ops
    return L, M, R, ops


@pytest.fixture
def set_mma(mods):
    ops = mods[3]
    prev = ops.get_mma()
    yield ops.set_mma
    ops.set_mma(prev)


@pytest.fixture
def fused_on(mods):
    R = mods[2]
    prev = R.LanePooling.fused
    R.LanePooling.fused = True
    yield
    R.LanePooling.fused = prev


def make_case(ops, P, scale=1.0, shift=0.0, count=None, valid_pad=False, seed=0):
    """(PairSet on the device, inputs on the CPU in fp32, ti, ci as CPU LongTensors over the rows the launch processes)."""
    g = torch.Generator().manual_seed(100 * P + seed)
    ti = torch.sort(torch.randint(T, (P,), generator=g))[0]
    ci = torch.randint(S, (P,), generator=g)
    if valid_pad:
        pad_t, pad_c = torch.randint(T, (PAD,), generator=g), torch.randint(S, (PAD,), generator=g)
    else:
        pad_t, pad_c = torch.full((PAD,), GARBAGE), -torch.full((PAD,), GARBAGE)
    cap = P + PAD
    rowptr = torch.zeros(T + 1, dtype=torch.int64)
    rowptr[1:] = torch.cumsum(torch.bincount(ti, minlength=T), 0)
    grid = lambda n: torch.randint(256, (n, 4), generator=g).float() / 64 + shift
    tgt_pose, ctx_pose = grid(T), grid(S)
    i32 = lambda t: t.to(torch.int32).cuda()
    ps = ops.PairSet(i32(torch.cat([ti, pad_t])), i32(torch.cat([ci, pad_c])), i32(torch.tensor([P if count is None else count])),
                     i32(rowptr), cap, T, tgt_pose[:, :2].contiguous().cuda(), ctx_pose[:, :2].contiguous().cuda())
    rn = lambda *shape, fan: torch.randn(*shape, generator=g) * (scale * 1.5 / fan ** 0.5)
    w0 = rn(C, 2 * C, fan=2 * C)
    cfeat = torch.randn(S, C, generator=g)
    inp = dict(wp=rn(C, 4, fan=4), bp=rn(C, fan=4), w0=w0, U=(cfeat.double() @ w0[:, :C].double().t()).float(),
               g=1 + 0.1 * (2 * torch.rand(C, generator=g) - 1), bt=0.1 * torch.randn(C, generator=g),
               ctx_pose=ctx_pose, tgt_pose=tgt_pose)
    if valid_pad:
        ti, ci = torch.cat([ti, pad_t]), torch.cat([ci, pad_c])
    return ps, inp, ti, ci


def run(ops, ps, inp, m=None):
    x = {k: v.cuda() for k, v in inp.items()}
    return ops.pool_pairs(ps, x["ctx_pose"], x["tgt_pose"], x["wp"], x["bp"], x["w0"], x["U"], (x["g"], x["bt"]), m=m, eps=EPS)


def model(inp, ti, ci):
    return PM.pair_stage(inp["ctx_pose"], inp["tgt_pose"], ti, ci, inp["wp"], inp["bp"], inp["w0"][:, C:], inp["U"], inp["g"],
                         inp["bt"], EPS)


def composed(ops, ps, inp, n):
    """The pair stage as LanePooling._run composes it with the switch off (the lines from `h` to `m`), first n pairs."""
    x = {k: v.cuda() for k, v in inp.items()}
    t_idx, c_idx = ps.hi[:n].long(), ps.wi[:n].long()
    h = torch.relu(torch.nn.functional.linear(x["ctx_pose"][c_idx] - x["tgt_pose"][t_idx], x["wp"], x["bp"]))
    per_pair = ops.agg_mlp(n, [ops.RelSpec(h.contiguous(), ops.packed(x["w0"], 128, 128))], 0)
    zero_row = torch.zeros((1, C), dtype=torch.float32, device="cuda")
    zero_idx = torch.zeros(n, dtype=torch.int32, device="cuda")
    n_dev = torch.tensor([n], dtype=torch.int32, device="cuda")
    pre = ops.pair_add(per_pair, x["U"], ps.wi, zero_row, zero_idx, n_dev, n)
    return ops.gn_fwd(pre, (x["g"], x["bt"]), relu=True, eps=EPS)


def rel_err(got, want):
    return float((got.detach().double().cpu() - want).abs().max() / (want.abs().max() + 1e-12))


def check_against_model(ops, tag, ps, inp, ti, ci):
    n = len(ti)
    m = torch.full((ps.cap, C), SENTINEL, device="cuda")
    out = run(ops, ps, inp, m)
    assert out is m
    want = model(inp, ti, ci)
    e_new, e_cmp = rel_err(m[:n], want), rel_err(composed(ops, ps, inp, n)[:n], want)
    print("%s rows=%d fused %.3e composed %.3e" % (tag, n, e_new, e_cmp))
    assert bool(torch.isfinite(m).all())
    assert bool((m[n:] == SENTINEL).all())                               # rows at or past the count stay untouched
    assert e_new <= min(max(2 * e_cmp, 1e-6), 1e-4), (e_new, e_cmp)
    return m


@pytest.mark.parametrize("P", [1, 31, 32, 33, 95, 65537])
def test_against_fp64(mods, set_mma, P):
    ops = mods[3]
    set_mma("f32")
    check_against_model(ops, "P=%d" % P, *make_case(ops, P))


@pytest.mark.parametrize("scale,shift", [(0.1, 0.0), (8.0, 0.0), (1.0, 1e3), (0.1, 1e3), (8.0, 1e3)])
def test_over_weight_scale_and_pose_offset(mods, set_mma, scale, shift):
    ops = mods[3]
    set_mma("f32")
    ps, inp, ti, ci = make_case(ops, 95, scale=scale, shift=shift)
    d = inp["ctx_pose"][ci] - inp["tgt_pose"][ti]
    assert float(d.abs().max()) < 6.0
    assert torch.equal(d.double(), inp["ctx_pose"].double()[ci] - inp["tgt_pose"].double()[ti])      # the subtraction is exact
    check_against_model(ops, "scale=%g shift=%g" % (scale, shift), ps, inp, ti, ci)


def test_negative_count_processes_cap_rows(mods, set_mma):
    """The pair search reports an overflow as a negative count: the launch then processes all cap rows."""
    ops = mods[3]
    set_mma("f32")
    ps, inp, ti, ci = make_case(ops, 33, count=-50, valid_pad=True)
    assert len(ti) == ps.cap == 40
    check_against_model(ops, "count=-50", ps, inp, ti, ci)
    ps, inp, ti, ci = make_case(ops, 33, count=1000, valid_pad=True)     # a count past cap is clamped as well
    check_against_model(ops, "count=1000", ps, inp, ti, ci)


def test_zero_row_gives_relu_beta(mods, set_mma):
    """A pair whose z is exactly zero (U[c] = 0 and h = 0): GroupNorm of a constant row is its bias, finite."""
    ops = mods[3]
    set_mma("f32")
    ps, inp, ti, ci = make_case(ops, 33)
    inp["bp"] = -torch.ones(C)                                           # h = ReLU(W_p 0 - 1) = 0 where the poses coincide
    inp["U"][int(ci[7])] = 0.0
    inp["ctx_pose"][int(ci[7])] = inp["tgt_pose"][int(ti[7])]
    m = check_against_model(ops, "zero row", ps, inp, ti, ci)
    assert torch.equal(m[7].cpu(), torch.relu(inp["bt"]))


@pytest.mark.parametrize("P", [33, 95])
def test_repeatable_and_mode_independent(mods, set_mma, P):
    ops = mods[3]
    ps, inp, _, _ = make_case(ops, P)
    outs = []
    for mode in ("f32", "f32", "bf16x3", "f16x2"):
        set_mma(mode)
        outs.append(run(ops, ps, inp)[:P].clone())
    for o in outs[1:]:
        assert torch.equal(o.view(torch.int32), outs[0].view(torch.int32))


def test_rows_of_m_are_checked(mods):
    L, _, _, ops = mods
    ps, inp, _, _ = make_case(ops, 33)
    with pytest.raises(L.LgcnError):
        run(ops, ps, inp, torch.empty((ps.cap - 1, C), device="cuda"))
    assert run(ops, ps, {**inp}, None).shape == (ps.cap, C)


# ------------------------------------------------------------------ LanePooling.fused at module level
def load(name):
    with np.load(os.path.join(GOLDEN_DIR, name + ".npz")) as z:
        return {k: z[k] for k in z.files}


def err(got, want):
    return float((got.detach().cpu() - torch.from_numpy(np.ascontiguousarray(want))).abs().max())


def count_launches(ops, monkeypatch):
    calls, real = [], ops.pool_pairs
    monkeypatch.setattr(ops, "pool_pairs", lambda *a, **k: calls.append(1) or real(*a, **k))
    return calls


def test_lane_pooling_fused_vs_reference_capture(mods, mma, monkeypatch):  # noqa: F811
    _, M, R, ops = mods
    g = load("lanercnn_b3")
    names = json.load(open(os.path.join(GOLDEN_DIR, "lanercnn_state_names.json")))
    _, _, ctx_g, tgt_g, dev = inputs(g, "cuda")
    pool = R.LanePooling(128, 128)
    pool.load_state_dict(OR.seeded_state([(k, tuple(s)) for k, s in names["pool"]], int(g["seed"]) + 2), strict=True)
    pool.cuda().eval()
    calls = count_launches(ops, monkeypatch)
    tfeat = dev(g["pool/tfeat"])
    keep = tfeat.clone()
    with torch.no_grad():
        off = pool(dev(g["pool/cfeat"]), ctx_g, tfeat, tgt_g, 6.0)
        assert not calls
        R.LanePooling.fused = True
        try:
            on = pool(dev(g["pool/cfeat"]), ctx_g, tfeat, tgt_g, 6.0)
        finally:
            R.LanePooling.fused = False
    assert len(calls) == 1 and torch.equal(tfeat, keep)
    print("%s pool/out: fused %.3e composed %.3e, fused - composed %.3e"
          % (mma, err(on, g["pool/out"]), err(off, g["pool/out"]), float((on - off).abs().max())))
    assert err(on, g["pool/out"]) <= FTOL
    assert float((on - off).abs().max()) <= FTOL


def test_fused_is_ignored_under_autograd(mods, set_mma, fused_on, monkeypatch):
    _, M, R, ops = mods
    set_mma("f32")
    g = load("lanercnn_b3")
    names = json.load(open(os.path.join(GOLDEN_DIR, "lanercnn_state_names.json")))
    _, _, ctx_g, tgt_g, dev = inputs(g, "cuda")
    pool = R.LanePooling(128, 128)
    pool.load_state_dict(OR.seeded_state([(k, tuple(s)) for k, s in names["pool"]], int(g["seed"]) + 2), strict=True)
    pool.cuda().train()
    calls = count_launches(ops, monkeypatch)
    out = pool(dev(g["pool/cfeat"]), ctx_g, dev(g["pool/tfeat"]), tgt_g, 6.0)
    assert not calls and out.requires_grad
    assert err(out, g["pool/out"]) <= FTOL
    out.sum().backward()
    assert all(p.grad is not None for p in pool.parameters())


def test_interactor_and_decode_fused_vs_reference_captures(mods, mma, monkeypatch):  # noqa: F811
    _, M, R, ops = mods
    g, names = DM.fixture()
    seed = int(g["seed"])
    ia = R.Interactor(M.config)
    ia.load_state_dict(TH.state(names, "interactor", seed + 1), strict=True)
    ia.cuda().eval()
    graph, isub, iroi = TH.interactor_inputs(g)
    dec = TH.decode_module(names, seed)
    sub, data, roi_feat = TH.decode_inputs(g)
    calls = count_launches(ops, monkeypatch)
    with torch.no_grad():
        off, off_pooled = ia(graph, isub, iroi), dec.decode(roi_feat, sub, data)["pooled"]
        assert not calls
        R.LanePooling.fused = True
        try:
            on, on_pooled = ia(graph, isub, iroi), dec.decode(roi_feat, sub, data)["pooled"]
        finally:
            R.LanePooling.fused = False
    assert len(calls) == 3                                               # roi2graph, graph2roi, Decode.lane_pool
    print("%s ia/out: fused %.3e composed %.3e; dec/pooled: fused %.3e composed %.3e"
          % (mma, err(on, g["ia/out"]), err(off, g["ia/out"]), err(on_pooled, g["dec/pooled"]), err(off_pooled, g["dec/pooled"])))
    assert err(on, g["ia/out"]) <= FTOL and float((on - off).abs().max()) <= FTOL
    assert err(on_pooled, g["dec/pooled"]) <= FTOL and float((on_pooled - off_pooled).abs().max()) <= FTOL
