"""The whole hot path (MapNet -> A2M -> M2M -> M2A -> A2A) over weight scale and statistics: the cases, and the three CPU
evaluations every check of them shares -- the float64 truth (the oracle on double tensors), the fp32 oracle, and the
operand-format model (split_model.hot_path) -- computed once per (scenes, state) and cached.

Test infrastructure for tests/test_hot_path_model_host.py and tests/test_gpu_hot_path_scale.py.

States (all from oracle.seeded_state / wide_state at seed 3, regenerated, never stored):
    ("uniform", e)   every matrix of K >= 128 times 2^e, GroupNorm parameters as seeded (max |W| = 0.70 * 2^e)
    ("blocks", e)    every 128-column block of those matrices rescaled to max |W| = 2^e exactly -- the quantity that
                     tools/check_weight_scale.py looks at (A2M.meta's four columns go with their block)
    ("wide",)        per-tensor scales 2^U[-8, 2], GroupNorm scales log-uniform in [0.05, 8] with 10 % negative, shifts x 5
Scenes:
    "b4"   the reference fixture's four scenes (486 nodes, 42 actors; a scene without pairs, a scene without left / right)
    "s0"   data.synth_batch("S0", seed=0): one scene, 648 nodes, 50 actors
"""
import functools
import os

import numpy as np
import torch

import split_model as S
from conftest import GOLDEN_DIR, to_torch_scene
from golden_io import load_scenes
from oracle import lanegcn_oracle as O

SEED = 3
STAGES = S.STAGES
WIDE = ("wide",)
WIDE_KW = dict(e_lo=-8, e_hi=2)
F16_GRID = [("uniform", e) for e in (0, -2, -4, -6, -8, -10)]
EXACT_GRID = [("uniform", e) for e in (0, -10, -20)]


def case_id(state):
    return "wide" if state == WIDE else ("w2^%d" if state[0] == "uniform" else "blockmax2^%d") % state[1]


def state_dict(state):
    shapes = O.hot_state_shapes()
    if state == WIDE:
        return O.wide_state(shapes, SEED, **WIDE_KW)
    if state[0] == "blocks":
        sd = O.seeded_state(shapes, SEED)
        for w in sd.values():
            if w.dim() == 2 and w.shape[1] >= 128:
                for c in range(0, w.shape[1] - 127, 128):
                    end = w.shape[1] if c + 256 > w.shape[1] else c + 128
                    top, scale = float(w[:, c:c + 128].abs().max()), np.float32(2.0 ** state[1] / float(w[:, c:c + 128].abs().max()))
                    while np.float32(top) * scale < np.float32(2.0 ** state[1]):       # the product is rounded: not below 2^e
                        scale = np.nextafter(scale, np.float32(np.inf))
                    w[:, c:end] *= scale
        return sd
    return O.wide_state(shapes, SEED, state[1], state[1], g_lo=None)


@functools.lru_cache(maxsize=None)
def scenes(which):
    """(numpy scenes, torch scenes, actors [A, 128] fp32 CPU tensor)."""
    if which == "b4":
        with np.load(os.path.join(GOLDEN_DIR, "hotpath_b4.npz")) as z:
            flat = {k: z[k] for k in z.files}
        sc, actors = load_scenes(flat), torch.from_numpy(flat["actors_in"])
    else:
        import lanegcn_amd  # noqa: F401
        from lanegcn_amd import data as gen
        sc = gen.synth_batch("S0", seed=0)
        n_act = sum(len(s["ctrs"]) for s in sc)
        actors = torch.from_numpy(np.random.default_rng(2).normal(0, 1, (n_act, 128)).astype(np.float32)).relu()
    return sc, [to_torch_scene(s) for s in sc], actors


def double_tree(x):
    if isinstance(x, dict):
        return {k: double_tree(v) for k, v in x.items()}
    if isinstance(x, list):
        return [double_tree(v) for v in x]
    return x.double() if isinstance(x, torch.Tensor) and x.is_floating_point() else x


def oracle_inputs(which):
    _, sc, actors = scenes(which)
    return O.graph_gather([s["graph"] for s in sc]), actors, [s["ctrs"] for s in sc]


def oracle_f64(which, sd):
    """The oracle -- the reference's operators in the reference's order -- on double tensors."""
    graph, actors, ctrs = oracle_inputs(which)
    with torch.no_grad():
        out = O.hot_path(double_tree(graph), actors.double(), double_tree(ctrs), double_tree(sd))
    return {k: v.numpy() for k, v in out.items()}


@functools.lru_cache(maxsize=None)
def cpu(which, state):
    """dict(truth = float64 stages, e_ref32 = {stage: the fp32 oracle's error}, ref32 = its stages)."""
    sd = state_dict(state)
    graph, actors, ctrs = oracle_inputs(which)
    truth = oracle_f64(which, sd)
    with torch.no_grad():
        ref32 = {k: v.numpy() for k, v in O.hot_path(graph, actors, ctrs, sd).items()}
    return dict(truth=truth, ref32=ref32, e_ref32={k: S.rel_err(ref32[k], truth[k]) for k in STAGES})


@functools.lru_cache(maxsize=None)
def model_err(which, state, mode):
    """{stage: rel_err(model, truth)} of a split mode; 0 for "f32" (nothing is rounded to 16-bit planes)."""
    if mode == "f32":
        return {k: 0.0 for k in STAGES}
    graph, actors, ctrs = oracle_inputs(which)
    got = S.hot_path(graph, actors, ctrs, state_dict(state), mode)
    truth = cpu(which, state)["truth"]
    return {k: S.rel_err(got[k], truth[k]) for k in STAGES}


def bar(e_model, e_ref32):
    """rel_err(kernel) <= max(2 e_model, 4 e_ref32, 1e-6), and never above 1e-4 where the model stays under 5e-5:
    split_model.bar with the floor widened by the fp32 oracle's own error (the model sums in float64; the kernels carry
    fp32 accumulation noise through 14 layers, in another order than the oracle)."""
    b = max(2.0 * e_model, 4.0 * e_ref32, 1e-6)
    return min(b, 1e-4) if e_model <= 5e-5 else b
