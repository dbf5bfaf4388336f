"""CPU: the per-actor evaluation entry points (lgcn_eval_actors, lgcn_eval_reduce_sel) are exported, bound and declared,
refuse bad arguments before launching anything (placeholder device addresses: a launch would fault), and accept empty
problems; the Python surface refuses what it can on the host."""
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("lgcn_eval_actors", "lgcn_eval_reduce_sel")
OK, EINVAL, ESHAPE, EALIGN = 0, -1, -2, -3
PTRS = ("reg", "cls", "gt", "has", "actor_off", "slot_base", "rec", "traj", "score", "err")


@pytest.fixture(scope="module")
def lib():
    import lanegcn_amd  # noqa: F401
    from lanegcn_amd import _lib
    return _lib.load(), _lib


def actors(l, **kw):
    a = dict(reg=256, cls=512, gt=768, has=1024, actor_off=1280, slot_base=1536, A=9, B=4, M=6, T=30, H=30, n_slots=10, rec=2048,
             traj=4096, score=8192, err=16384)
    a.update(kw)
    return l.lgcn_eval_actors(a["reg"], a["cls"], a["gt"], a["has"], a["actor_off"], a["slot_base"], a["A"], a["B"], a["M"], a["T"],
                              a["H"], a["n_slots"], a["rec"], a["traj"], a["score"], a["err"], None)


def reduce_sel(l, **kw):
    a = dict(rec=256, n_slots=10, thr=2.0, who=0, max_missing=29, out=512, cnt=1024, err=2048)
    a.update(kw)
    return l.lgcn_eval_reduce_sel(a["rec"], a["n_slots"], a["thr"], a["who"], a["max_missing"], a["out"], a["cnt"], a["err"], None)


def test_symbols_are_exported_bound_and_declared(lib):
    l, mod = lib
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "lgcn.h")).read(), flags=re.S)
    for n in NAMES:
        assert hasattr(l, n) and n in mod.SIGNATURES and re.search(r"\b%s\s*\(" % n, header), n
    assert len(mod.SIGNATURES["lgcn_eval_actors"][1]) == 17 and len(mod.SIGNATURES["lgcn_eval_reduce_sel"][1]) == 9
    from lanegcn_amd import evaluate, ops
    assert callable(ops.eval_actors) and callable(ops.eval_reduce_sel) and callable(evaluate.ActorEvaluator.for_store)


def test_eval_actors_refuses_bad_arguments(lib):
    l, _ = lib
    for name in PTRS:
        if name in ("traj", "score"):
            continue
        assert actors(l, **{name: None}) == EINVAL, name
    assert actors(l, traj=None) == EINVAL and actors(l, score=None) == EINVAL      # one of the pair alone
    for kw in (dict(A=-1), dict(B=-1), dict(n_slots=-1), dict(M=0), dict(M=-3), dict(T=0), dict(H=0), dict(H=31), dict(T=10, H=11),
               dict(H=-1)):
        assert actors(l, **kw) == EINVAL, kw
    for kw in (dict(M=9), dict(T=65, H=65), dict(T=65, H=1), dict(B=1 << 31), dict(n_slots=1 << 31), dict(B=1 << 40),
               dict(A=(1 << 24) + 1), dict(A=1 << 40)):
        assert actors(l, **kw) == ESHAPE, kw
    for name in PTRS:
        if name == "has":
            continue
        assert actors(l, **{name: 256 + 8}) == EALIGN, name
        assert actors(l, **{name: 256 + 4}) == EALIGN, name


def test_eval_reduce_sel_refuses_bad_arguments(lib):
    l, _ = lib
    for name in ("rec", "out", "cnt", "err"):
        assert reduce_sel(l, **{name: None}) == EINVAL, name
        assert reduce_sel(l, **{name: 256 + 8}) == EALIGN, name
    for kw in (dict(n_slots=-1), dict(who=-1), dict(who=3), dict(max_missing=-1)):
        assert reduce_sel(l, **kw) == EINVAL, kw
    assert reduce_sel(l, n_slots=1 << 31) == ESHAPE


def test_empty_problems_launch_nothing(lib):
    l, _ = lib
    assert actors(l, B=0) == OK and actors(l, A=0) == OK
    assert actors(l, B=0, A=0, reg=None, cls=None, gt=None, has=None, actor_off=None, slot_base=None) == OK
    assert actors(l, A=0, traj=None, score=None) == OK
    assert actors(l, n_slots=0, A=0) == OK
    assert reduce_sel(l, n_slots=0) == OK and reduce_sel(l, n_slots=0, rec=None) == OK


def test_the_python_surface_checks_on_the_host():
    import torch
    import lanegcn_amd  # noqa: F401
    from lanegcn_amd import ops
    from lanegcn_amd._lib import LgcnError
    from lanegcn_amd.evaluate import ActorEvaluator, Evaluator
    z = torch.zeros
    with pytest.raises(LgcnError):
        ops.eval_actors(z(1, 6, 30, 2), z(1, 6), z(1, 30, 2), z(1, 30, dtype=torch.bool), z(2, dtype=torch.int32),
                        z(1, dtype=torch.int64), 30, z(4, 32), err=z(1, dtype=torch.int32))
    with pytest.raises(LgcnError):
        ops.eval_reduce_sel(z(4, 32), 2.0, 0, 0, z(8, 6, dtype=torch.float64), z(4, dtype=torch.int64), z(1, dtype=torch.int32))
    off = np.array([0, 3, 3, 4, 9], np.int64)
    for bad in (dict(num_mods=9), dict(num_preds=65), dict(horizon=31), dict(horizon=0), dict(actor_off=[1, 2]),
                dict(actor_off=[0, 3, 2]), dict(actor_off=[]), dict(actor_off=[0, (1 << 24) + 1])):
        kw = dict(actor_off=off, num_mods=6, num_preds=30, device="cpu")
        kw.update(bad)
        with pytest.raises(LgcnError):
            ActorEvaluator(**kw)
    ev = ActorEvaluator(off, 6, 30, horizon=10, keep_preds=True, device="cpu")
    assert isinstance(ev, Evaluator) and ev.n_scenes == 4 and ev.n_slots == 9 and ev.horizon == 10
    assert ev.rec.shape == (9, 32) and ev.traj.shape == (9, 6, 30, 2) and ev.score.shape == (9, 6) and not ev.rec.any()
    scene, local = ev.actor_index()
    assert scene.tolist() == [0, 0, 0, 2, 3, 3, 3, 3, 3] and local.tolist() == [0, 1, 2, 0, 0, 1, 2, 3, 4]
    for kw in (dict(who="scene"), dict(min_obs=0), dict(min_obs=11), dict(ks=(7,))):
        with pytest.raises(LgcnError):
            ev.summary(**kw)
    with pytest.raises(LgcnError):
        ActorEvaluator(off, 6, 30, device="cpu").predictions()
    empty = ActorEvaluator([0], 6, 30, device="cpu")
    assert empty.n_scenes == 0 and empty.n_slots == 0 and empty.rec.shape == (0, 32)
