"""GPU: the WHOLE hot path (MapNet -> A2M -> M2M -> M2A -> A2A, 14 stacked GEMM + GroupNorm layers) against float64, over
weight scale and trained-looking statistics, every matrix mode held to a model of its own operand format.

Every other whole-path test draws oracle.seeded_state (max |W| 0.55 .. 0.70, GroupNorm scales 1 +- 0.1, all positive) and
compares with fp32 captures at an absolute 1e-4.  Every 128-wide Linear of the path feeds a GroupNorm, so the float64
function does not move when such a weight shrinks by a power of two -- weight decay does that freely -- while the f16x2
error grows like 1 / scale.  tests/test_gpu_operand_scale.py pins that per kernel; this file pins what the stack does, and
replaces the flat 1e-4 by a bar that a dropped plane product or a stale weight image in ONE layer cannot pass:

    rel_err(kernel) <= max(2 e_model, 4 e_ref32, 1e-6)     per stage;  rel_err = max |x - fp64| / max |fp64|
    (capped at 1e-4 wherever e_model <= 5e-5)

e_model: split_model.hot_path in the case's mode against float64 (0 for f32); e_ref32: the fp32 oracle against the
float64 oracle on the same input.  Both are computed on the CPU at test time (hot_path_cases.cpu / model_err, cached per
state and shared by the modes); nothing comes from the kernels.  2 x the model is the project's rule;
4 x e_ref32 because the model sums in float64 while the kernels carry fp32 accumulation noise through 14 layers in an
order of their own (two independent noises of the oracle's size, and the tail of a maximum over 62 k entries).

Cases (hot_path_cases): f16x2 at s_w = 2^{0, -2, -4, -6, -8, -10}, every 128-column block at max |W| = 2^-9 (the
threshold of tools/check_weight_scale.py), the wide state, and the one-scene S0 batch at 2^0 and
2^-6; bf16x3, f32 and the single-product bf16 mode at 2^{0, -10, -20} and the wide state; HotPathEngine
(forward_guarded and one captured replay) in f16x2 at 2^0, 2^-8 and the wide state, with the same bars and bitwise the module path.  Fresh modules per case (no packed
image is reused), ops.set_guard("raise") throughout: a silent bf16x3 re-run must not satisfy an f16x2 bar.
Measured figures: DESIGN.md section 5c, "whole hot path"."""
import numpy as np
import pytest
import torch

import hot_path_cases as H
import split_model as S
from test_gpu_parity import make_modules, run_hot_path

pytestmark = pytest.mark.gpu

U = lambda e: ("uniform", e)
CASES = [("f16x2", "b4", st) for st in H.F16_GRID + [("blocks", -9), H.WIDE]] + [("f16x2", "s0", U(0)), ("f16x2", "s0", U(-6))]
CASES += [(m, "b4", st) for m in ("bf16x3", "f32") for st in H.EXACT_GRID + [H.WIDE]]
CASES += [("bf16", "b4", st) for st in H.EXACT_GRID + [H.WIDE]]
ENGINE_STATES = [U(0), U(-8), H.WIDE]


@pytest.fixture(scope="module")
def hip():
    import lanegcn_amd  # noqa: F401
    from lanegcn_amd import lanegcn as M
    from lanegcn_amd import ops
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return M, ops


@pytest.fixture(autouse=True)
def guard_raises(hip):
    _, ops = hip
    prev = ops.get_guard()
    ops.set_guard("raise")
    yield
    ops.set_guard(prev)


def check(head, mode, which, state, got):
    """Prints stage: model / fp32-oracle / kernel for every stage, then asserts the bar of every stage."""
    c, e_m = H.cpu(which, state), H.model_err(which, state, mode)
    bad = []
    for k in H.STAGES:
        assert got[k].dtype == np.float32 and got[k].shape == c["truth"][k].shape, k
        e_k, b = S.rel_err(got[k], c["truth"][k]), H.bar(e_m[k], c["e_ref32"][k])
        print("\nHOTPATH %s %s %s %s %s: %.3e / %.3e / %.3e  bar %.3e" % (head, mode, which, H.case_id(state), k, e_m[k],
                                                                        c["e_ref32"][k], e_k, b), end="")
        if not e_k <= b:                      # a NaN fails
            bad.append((k, e_m[k], c["e_ref32"][k], e_k, b))
    assert not bad, "%s %s %s %s (stage, model, fp32 oracle, kernel, bar): %s" % (head, mode, which, H.case_id(state), bad)


@pytest.mark.parametrize("mode,which,state", CASES, ids=["%s-%s-%s" % (m, w, H.case_id(s)) for m, w, s in CASES])
def test_modules_over_weight_scale(hip, mode, which, state):
    M, ops = hip
    _, scenes, actors = H.scenes(which)
    with ops.mma_scope(mode):
        assert ops.get_mma() == mode and ops.get_guard() == "raise"
        got, _ = run_hot_path(M, make_modules(M, H.state_dict(state)), scenes, actors)
    check("modules", mode, which, state, got)


@pytest.mark.parametrize("state", ENGINE_STATES, ids=[H.case_id(s) for s in ENGINE_STATES])
def test_engine_over_weight_scale(hip, state):
    """HotPathEngine on the fixture's scenes: forward_guarded with every stage, and one captured replay (nodes = m2m,
    actors = a2a): the same bars, and bitwise the module path."""
    M, ops = hip
    from lanegcn_amd.engine import HotPathEngine, collate_flat
    scenes_np, scenes, actors = H.scenes("b4")
    names = ("map_net", "a2m", "m2m", "m2a", "a2a")
    with ops.mma_scope("f16x2"):
        mods = make_modules(M, H.state_dict(state))
        want, _ = run_hot_path(M, mods, scenes, actors)
        eng = HotPathEngine(*(mods[k] for k in names))
        fb, act_d = collate_flat(scenes_np), actors.cuda()
        out = eng.forward_guarded(fb, act_d, stages=True)
        torch.cuda.synchronize()
        got = {k: out[k].cpu().numpy() for k in names}
        graph, gout = eng.capture(fb, act_d)
        graph.replay()
        torch.cuda.synchronize()
        replay = {"m2m": gout["nodes"].cpu().numpy(), "a2a": gout["actors"].cpu().numpy()}
        assert int(gout["nonfinite"].item()) == 0
    check("engine", "f16x2", "b4", state, got)
    for k in names:
        assert np.array_equal(got[k], want[k]), "engine differs from the module path: " + k
    for k in replay:
        assert np.array_equal(replay[k], want[k]), "captured replay differs from the module path: " + k
