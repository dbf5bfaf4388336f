"""CPU: the split-evaluation entry points (lgcn_eval_scenes, lgcn_eval_reduce) are exported, bound and declared, refuse bad
arguments before launching anything (placeholder device addresses: a launch would fault), and accept empty problems."""
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("lgcn_eval_scenes", "lgcn_eval_reduce")
OK, EINVAL, ESHAPE, EALIGN = 0, -1, -2, -3
PTRS = ("reg", "cls", "gt", "has", "actor_off", "slot", "rec", "traj", "score", "err")


@pytest.fixture(scope="module")
def lib():
    import lanegcn_amd  # noqa: F401
    from lanegcn_amd import _lib
    return _lib.load(), _lib


def scenes(l, **kw):
    a = dict(reg=256, cls=512, gt=768, has=1024, actor_off=1280, slot=1536, B=4, M=6, T=30, H=30, n_slots=10, rec=2048,
             traj=4096, score=8192, err=16384)
    a.update(kw)
    return l.lgcn_eval_scenes(a["reg"], a["cls"], a["gt"], a["has"], a["actor_off"], a["slot"], a["B"], a["M"], a["T"], a["H"],
                              a["n_slots"], a["rec"], a["traj"], a["score"], a["err"], None)


def reduce(l, **kw):
    a = dict(rec=256, n_slots=10, thr=2.0, out=512, cnt=1024, err=2048)
    a.update(kw)
    return l.lgcn_eval_reduce(a["rec"], a["n_slots"], a["thr"], a["out"], a["cnt"], a["err"], None)


def test_symbols_are_exported_bound_and_declared(lib):
    l, mod = lib
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "lgcn.h")).read(), flags=re.S)
    for n in NAMES:
        assert hasattr(l, n) and n in mod.SIGNATURES and re.search(r"\b%s\s*\(" % n, header), n
    assert len(mod.SIGNATURES["lgcn_eval_scenes"][1]) == 16 and len(mod.SIGNATURES["lgcn_eval_reduce"][1]) == 7
    from lanegcn_amd import evaluate, ops
    assert callable(ops.eval_scenes) and callable(ops.eval_reduce) and callable(evaluate.evaluate_store)
    src = open(os.path.join(ROOT, "lanegcn-1_amd", "csrc", "Makefile")).read()
    assert "lgcn_eval.hip" in src


def test_eval_scenes_refuses_bad_arguments(lib):
    l, _ = lib
    for name in PTRS:
        if name in ("traj", "score"):
            continue
        assert scenes(l, **{name: None}) == EINVAL, name
    assert scenes(l, traj=None) == EINVAL and scenes(l, score=None) == EINVAL      # one of the pair alone
    for kw in (dict(B=-1), dict(n_slots=-1), dict(M=0), dict(M=-3), dict(T=0), dict(H=0), dict(H=31), dict(T=10, H=11),
               dict(H=-1)):
        assert scenes(l, **kw) == EINVAL, kw
    for kw in (dict(M=9), dict(T=65, H=65), dict(T=65, H=1), dict(B=1 << 31), dict(n_slots=1 << 31), dict(B=1 << 40)):
        assert scenes(l, **kw) == ESHAPE, kw
    for name in PTRS:
        if name == "has":
            continue
        assert scenes(l, **{name: 256 + 8}) == EALIGN, name
        assert scenes(l, **{name: 256 + 4}) == EALIGN, name


def test_eval_reduce_refuses_bad_arguments(lib):
    l, _ = lib
    for name in ("rec", "out", "cnt", "err"):
        assert reduce(l, **{name: None}) == EINVAL, name
        assert reduce(l, **{name: 256 + 8}) == EALIGN, name
    assert reduce(l, n_slots=-1) == EINVAL
    assert reduce(l, n_slots=1 << 31) == ESHAPE


def test_empty_problems_launch_nothing(lib):
    l, _ = lib
    assert scenes(l, B=0) == OK
    assert scenes(l, B=0, reg=None, cls=None, gt=None, has=None, actor_off=None, slot=None) == OK
    assert scenes(l, B=0, traj=None, score=None) == OK
    assert reduce(l, n_slots=0) == OK and reduce(l, n_slots=0, rec=None) == OK


def test_wrappers_take_device_tensors_only():
    import torch
    import lanegcn_amd  # noqa: F401
    from lanegcn_amd import ops
    from lanegcn_amd._lib import LgcnError
    from lanegcn_amd.evaluate import Evaluator
    z = torch.zeros
    with pytest.raises(LgcnError):
        ops.eval_scenes(z(1, 6, 30, 2), z(1, 6), z(1, 30, 2), z(1, 30, dtype=torch.bool), z(2, dtype=torch.int32),
                        z(1, dtype=torch.int64), 30, z(4, 32), err=z(1, dtype=torch.int32))
    with pytest.raises(LgcnError):
        ops.eval_reduce(z(4, 32), 2.0, z(8, 6, dtype=torch.float64), z(3, dtype=torch.int64), z(1, dtype=torch.int32))
    for bad in (dict(num_mods=9), dict(num_preds=65), dict(horizon=31), dict(horizon=0), dict(n_scenes=-1)):
        kw = dict(n_scenes=4, num_mods=6, num_preds=30, device="cpu")
        kw.update(bad)
        with pytest.raises(LgcnError):
            Evaluator(**kw)
    ev = Evaluator(4, 6, 30, keep_preds=True, device="cpu")
    assert ev.rec.shape == (4, 32) and ev.traj.shape == (4, 6, 30, 2) and ev.score.shape == (4, 6) and ev.horizon == 30
    assert not ev.rec.any()
    with pytest.raises(LgcnError):
        Evaluator(4, 6, 30, device="cpu").predictions()
