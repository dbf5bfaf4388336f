"""CPU: the fused optimizer step (lgcn_opt_step and its chunk-length helper) is exported and bound, its ctypes struct matches
the header, the entry refuses an unknown kind, negative counts, a non-finite lr, clip bounds in the wrong order, an Adam bias
correction that is not positive and null tables before launching anything, and does nothing for zero chunks (no GPU needed).
optim_hip.chunk_rows covers every element of every tensor exactly once, in order.  utils.Optimizer.train_hip exists and is off
by default, and ops.refresh_packed takes force.

ref_step below is the float64 numpy statement of the three update rules of include/lgcn.h (lgcn_opt_step), which the GPU
tests (tests/test_gpu_opt_step.py) measure against; here it is checked against torch.optim.Adam / AdamW / SGD on float64 CPU
tensors to 1e-12 over 5 steps, with a change of lr, two groups with different coef, and the clamp on."""
import ctypes as C
import inspect
import math

import numpy as np
import pytest
import torch

EINVAL = -1
NEW = ("lgcn_opt_chunk_elems", "lgcn_opt_step")
HYPER = {"adam": dict(wd=0.0), "adam_wd": dict(wd=0.02), "adamw": dict(wd=0.01), "sgd": dict(wd=1e-4, momentum=0.9),
         "sgd_plain": dict(wd=1e-4, momentum=0.0)}
KIND_OF = {"adam": "adam", "adam_wd": "adam", "adamw": "adamw", "sgd": "sgd", "sgd_plain": "sgd"}


# ------------------------------------------------------------------ the float64 reference
def ref_state(kind, params):
    """Fresh optimizer state of float64 copies of `params` (numpy arrays): {"p", "m", "v", "t"} lists."""
    return dict(p=[np.array(x, dtype=np.float64) for x in params], m=[np.zeros(np.shape(x)) for x in params],
                v=[np.zeros(np.shape(x)) for x in params], t=[0] * len(params), kind=kind)


def ref_step(st, grads, lr, *, wd=0.0, momentum=0.0, beta1=0.9, beta2=0.999, eps=1e-8, clip=None):
    """One step of include/lgcn.h's formulas in float64, in place on st; grads: float64 arrays or None (the tensor is left
    out: not touched, step count not advanced); lr: one value or one per tensor.  Returns the gradients as the step leaves
    them (clamped when clip = (low, high))."""
    kind, out = st["kind"], []
    lrs = lr if isinstance(lr, (list, tuple)) else [lr] * len(grads)
    for i, g in enumerate(grads):
        if g is None:
            out.append(None)
            continue
        g = np.array(g, dtype=np.float64)
        if clip is not None:
            g = np.where(g < clip[0], clip[0], np.where(g > clip[1], clip[1], g))          # a NaN stays a NaN
        out.append(g)
        p, m, v, a = st["p"][i], st["m"][i], st["v"][i], lrs[i]
        st["t"][i] += 1
        t = st["t"][i]
        if kind == "sgd":
            ge = g + wd * p if wd else g
            if momentum:
                m[...] = ge if t == 1 else momentum * m + ge
                ge = m
            p -= a * ge
            continue
        ge = g
        if kind == "adamw":
            if wd:
                p *= 1 - a * wd
        elif wd:
            ge = g + wd * p
        m += (1 - beta1) * (ge - m)
        v[...] = beta2 * v + (1 - beta2) * ge * ge
        bc1, bc2 = 1 - beta1 ** t, 1 - beta2 ** t
        p -= (a / bc1) * m / (np.sqrt(v) / math.sqrt(bc2) + eps)
    return out


def stock_optimizer(name, groups):
    """torch.optim's optimizer for a HYPER name over `groups` ([{"params": [...], "lr": 0}])."""
    h = HYPER[name]
    if KIND_OF[name] == "sgd":
        return torch.optim.SGD(groups, momentum=h["momentum"], weight_decay=h["wd"])
    return (torch.optim.AdamW if KIND_OF[name] == "adamw" else torch.optim.Adam)(groups, weight_decay=h["wd"])


def ref_kwargs(name):
    h = HYPER[name]
    return dict(wd=h["wd"], momentum=h.get("momentum", 0.0))


@pytest.mark.parametrize("clip", [None, (-0.4, 0.7)])
@pytest.mark.parametrize("name", sorted(HYPER))
def test_reference_is_torch_optim_in_float64(name, clip):
    rng = np.random.default_rng(3)
    shapes = [(5,), (3, 4), (1,), (7, 2)]
    coef = [1.0, 1.0, 0.1, 0.1]                                          # two groups of two tensors
    p0 = [rng.normal(0, 1, s) for s in shapes]
    tp = [torch.tensor(x, dtype=torch.float64, requires_grad=True) for x in p0]
    opt = stock_optimizer(name, [{"params": tp[:2], "lr": 0}, {"params": tp[2:], "lr": 0}])
    st = ref_state(KIND_OF[name], p0)
    for step in range(5):
        lr = 1e-2 if step < 2 else 3e-3                                  # lr changes at step 3
        grads = [rng.normal(0, 1, s) for s in shapes]
        for t, g in zip(tp, grads):
            t.grad = torch.tensor(g, dtype=torch.float64)
            if clip is not None:
                t.grad.clamp_(*clip)
        for c, g in zip((1.0, 0.1), opt.param_groups):
            g["lr"] = lr * c
        opt.step()
        left = ref_step(st, grads, [lr * c for c in coef], clip=clip, **ref_kwargs(name))
        for i, t in enumerate(tp):
            e = np.abs(t.detach().numpy() - st["p"][i]).max() / np.abs(st["p"][i]).max()
            assert e <= 1e-12, (name, step, i, e)
            assert np.array_equal(t.grad.numpy(), left[i])
            s = opt.state[t]
            if KIND_OF[name] != "sgd":
                assert np.abs(s["exp_avg"].numpy() - st["m"][i]).max() <= 1e-12 * np.abs(st["m"][i]).max()
                assert np.abs(s["exp_avg_sq"].numpy() - st["v"][i]).max() <= 1e-12 * np.abs(st["v"][i]).max()
            elif HYPER[name]["momentum"]:
                assert np.abs(s["momentum_buffer"].numpy() - st["m"][i]).max() <= 1e-12 * np.abs(st["m"][i]).max()


def test_reference_leaves_a_tensor_without_gradient_alone():
    st = ref_state("adam", [np.ones(3), np.ones(2)])
    ref_step(st, [np.ones(3), None], 0.1)
    assert st["t"] == [1, 0] and np.array_equal(st["p"][1], np.ones(2)) and not np.array_equal(st["p"][0], np.ones(3))
    nan = ref_step(st, [np.array([np.nan, 2.0, -2.0]), None], 0.1, clip=(-1.0, 1.0))[0]
    assert np.isnan(nan[0]) and nan[1] == 1.0 and nan[2] == -1.0


# ------------------------------------------------------------------ the C ABI
@pytest.fixture(scope="module")
def lib():
    import lanegcn_amd  # noqa: F401
    from lanegcn_amd import _lib
    return _lib.load(), _lib


def test_symbols_are_exported_and_bound(lib):
    l, mod = lib
    for n in NEW:
        assert hasattr(l, n), "liblgcn.so does not export " + n
        assert n in mod.SIGNATURES
    assert l.lgcn_version() == 100
    assert (mod.OPT_ADAM, mod.OPT_ADAMW, mod.OPT_SGD) == (0, 1, 2)
    assert mod.OPT_KINDS == {"adam": 0, "adamw": 1, "sgd": 2}


def test_switch_is_opt_in():
    import lanegcn_amd  # noqa: F401
    from lanegcn_amd import lanegcn as M
    from lanegcn_amd import ops, optim_hip, utils
    assert utils.Optimizer.train_hip is False and M.Optimizer is utils.Optimizer
    assert inspect.signature(ops.refresh_packed).parameters["force"].default is False
    assert ops.refresh_packed() >= 0 and ops.refresh_packed(force=True) >= 0      # the count of rebuilt images, as before
    # CPU parameters are not eligible: the stock optimizer, as without the switch
    p = torch.nn.Parameter(torch.zeros(3))
    utils.Optimizer.train_hip = True
    try:
        opt = utils.Optimizer([p], dict(opt="adam", lr_func=lambda e: 1e-3))
    finally:
        utils.Optimizer.train_hip = False
    assert isinstance(opt.opt, torch.optim.Adam) and not opt.fused
    assert not optim_hip.eligible([]) and not optim_hip.eligible([p])
    with pytest.raises(_lib_error()):
        optim_hip.FusedOptim([{"params": [p], "lr": 0}], "adam")


def _lib_error():
    from lanegcn_amd import _lib
    return _lib.LgcnError


def test_struct_layout_matches_header(lib):
    _, mod = lib
    S = mod.OptTensor                                                    # lgcn_opt_tensor_t: float *p, *g, *m, *v; int64_t n
    assert [f[0] for f in S._fields_] == ["p", "g", "m", "v", "n"]
    assert [getattr(S, n).offset for n in ("p", "g", "m", "v", "n")] == [0, 8, 16, 24, 32]
    assert S.n.size == 8 and C.sizeof(S) == 40


def test_chunk_helper(lib):
    l, _ = lib
    c = l.lgcn_opt_chunk_elems()
    assert c > 0 and c % 4 == 0 and c % 256 == 0


def test_entry_validates_before_launching(lib):
    l, mod = lib
    inf, nan = float("inf"), float("nan")

    def call(tensors=256, n_tensors=3, chunks=256, n_chunks=2, kind=0, lr=1e-3, beta1=0.9, beta2=0.999, eps=1e-8, wd=0.0,
             momentum=0.0, first_step=0, bc1=0.1, bc2=0.001, clip_on=0, clip_low=-1.0, clip_high=1.0):
        return l.lgcn_opt_step(tensors, n_tensors, chunks, n_chunks, kind, lr, beta1, beta2, eps, wd, momentum, first_step, bc1,
                               bc2, clip_on, clip_low, clip_high, None)

    for kind in (mod.OPT_ADAM, mod.OPT_ADAMW, mod.OPT_SGD):
        assert call(kind=kind, n_chunks=0) == 0                          # nothing to do: no launch
        assert call(kind=kind, n_chunks=0, tensors=None, chunks=None, n_tensors=0) == 0
        assert call(kind=kind, tensors=None) == EINVAL and call(kind=kind, chunks=None) == EINVAL
        assert call(kind=kind, n_tensors=0) == EINVAL                    # chunks of no tensor
        assert call(kind=kind, n_chunks=-1) == EINVAL and call(kind=kind, n_tensors=-1) == EINVAL
        for lr in (inf, -inf, nan):
            assert call(kind=kind, lr=lr) == EINVAL and call(kind=kind, lr=lr, n_chunks=0) == EINVAL
        assert call(kind=kind, clip_on=1, clip_low=1.0, clip_high=-1.0) == EINVAL
        assert call(kind=kind, clip_on=1, clip_low=nan) == EINVAL and call(kind=kind, clip_on=1, clip_high=nan) == EINVAL
        assert call(kind=kind, clip_on=1, clip_low=1.0, clip_high=-1.0, n_chunks=0) == EINVAL
        assert call(kind=kind, clip_on=0, clip_low=1.0, clip_high=-1.0, n_chunks=0) == 0      # bounds unused without the clamp
        assert call(kind=kind, clip_on=1, clip_low=0.5, clip_high=0.5, n_chunks=0) == 0
    for kind in (-1, 3, 7):
        assert call(kind=kind) == EINVAL and call(kind=kind, n_chunks=0) == EINVAL
    for kind in (mod.OPT_ADAM, mod.OPT_ADAMW):
        assert call(kind=kind, bc1=0.0) == EINVAL and call(kind=kind, bc2=0.0) == EINVAL and call(kind=kind, bc1=nan) == EINVAL
    assert call(kind=mod.OPT_SGD, bc1=0.0, bc2=0.0, n_chunks=0) == 0     # read by the Adam kinds only


# ------------------------------------------------------------------ the chunk table
def test_chunk_rows_cover_every_element_once_in_order(lib):
    l, _ = lib
    from lanegcn_amd import optim_hip
    c = optim_hip.chunk_elems()
    assert c == l.lgcn_opt_chunk_elems()
    sizes = [0, 1, 3, 4, c - 1, c, c + 1, 2 * c + 5]
    for order in (sizes, sizes[::-1], [0, 0], [], [2 * c + 5]):
        rows = optim_hip.chunk_rows(order, c)
        seen = [[] for _ in order]
        for t, first in rows:
            assert 0 <= t < len(order) and first % c == 0 and first % 4 == 0 and 0 <= first < order[t]
            seen[t].append(first)
        assert [t for t, _ in rows] == sorted(t for t, _ in rows)         # tensors in order
        for t, n in enumerate(order):
            assert seen[t] == list(range(0, n, c)), (t, n)                # its chunks in order, none twice
            covered = sum(min(c, n - f) for f in seen[t])
            assert covered == n
        assert len(rows) == sum((n + c - 1) // c for n in order)
    assert optim_hip.chunk_rows([5, 9], 4) == [(0, 0), (0, 4), (1, 0), (1, 4), (1, 8)]
