"""CPU: the drivable-area entry points (lgcn_eval_scenes_da, lgcn_eval_actors_da, lgcn_eval_dac_reduce) are exported, bound
and declared, refuse bad arguments before launching anything (placeholder device addresses: a launch would fault; the
city table's host copy is real memory, it is what the checks read), and accept empty problems."""
import ctypes as C
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("lgcn_eval_scenes_da", "lgcn_eval_actors_da", "lgcn_eval_dac_reduce")
OK, EINVAL, ESHAPE, EALIGN = 0, -1, -2, -3
PTRS = ("reg", "cls", "gt", "has", "actor_off", "slot", "rec", "traj", "score", "err")
ARGS = dict(reg=256, cls=512, gt=768, has=1024, actor_off=1280, slot=1536, A=9, B=4, M=6, T=30, H=30, n_slots=10, rec=2048,
            traj=4096, score=8192, err=16384)


@pytest.fixture(scope="module")
def lib():
    import lanegcn_amd  # noqa: F401
    from lanegcn_amd import _lib
    return _lib.load(), _lib


def drivable(mod, cities=((0, 7, 9), (63, 5, 4)), m=(1., 0., -3., 0., 1., -2.), raster=32768, raster_bytes=83, city=65536,
             scene_city=131072, host=True, n_cities=None):
    """A lgcn_drivable_t over placeholder device addresses; -> (the struct, what keeps its host table alive)."""
    table = (mod.DaCity * max(len(cities), 1))()
    for t, (off, h, w) in zip(table, cities):
        t.off, t.h, t.w = off, h, w
        t.m[:] = m
    d = mod.Drivable(raster, raster_bytes, city, C.addressof(table) if host else None,
                     len(cities) if n_cities is None else n_cities, scene_city)
    return d, table


def scenes(l, d, **kw):
    a = dict(ARGS)
    a.update(kw)
    return l.lgcn_eval_scenes_da(a["reg"], a["cls"], a["gt"], a["has"], a["actor_off"], a["slot"], a["B"], a["M"], a["T"], a["H"],
                                 a["n_slots"], a["rec"], a["traj"], a["score"], a["err"], d if d is None else C.byref(d), None)


def actors(l, d, **kw):
    a = dict(ARGS)
    a.update(kw)
    return l.lgcn_eval_actors_da(a["reg"], a["cls"], a["gt"], a["has"], a["actor_off"], a["slot"], a["A"], a["B"], a["M"], a["T"],
                                 a["H"], a["n_slots"], a["rec"], a["traj"], a["score"], a["err"], d if d is None else C.byref(d), None)


def dac_reduce(l, **kw):
    a = dict(rec=256, n_slots=10, who=0, max_missing=29, dac=512)
    a.update(kw)
    return l.lgcn_eval_dac_reduce(a["rec"], a["n_slots"], a["who"], a["max_missing"], a["dac"], None)


def test_symbols_are_exported_bound_and_declared(lib):
    l, mod = lib
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "lgcn.h")).read(), flags=re.S)
    for n in NAMES:
        assert hasattr(l, n) and n in mod.SIGNATURES and re.search(r"\b%s\s*\(" % n, header), n
    assert "lgcn_drivable_t" in header and "lgcn_da_city_t" in header
    assert len(mod.SIGNATURES["lgcn_eval_scenes_da"][1]) == len(mod.SIGNATURES["lgcn_eval_scenes"][1]) + 1
    assert len(mod.SIGNATURES["lgcn_eval_actors_da"][1]) == len(mod.SIGNATURES["lgcn_eval_actors"][1]) + 1
    assert C.sizeof(mod.DaCity) == 72 and C.sizeof(mod.Drivable) == 48      # the layouts of include/lgcn.h
    from lanegcn_amd import evaluate, ops
    assert callable(ops.eval_scenes_da) and callable(ops.eval_actors_da) and callable(ops.eval_dac_reduce)
    assert callable(evaluate.DrivableArea.from_files)


@pytest.mark.parametrize("entry", [scenes, actors], ids=["scenes", "actors"])
def test_the_siblings_checks_still_apply(lib, entry):
    l, mod = lib
    d, keep = drivable(mod)
    for name in PTRS:
        if name in ("traj", "score"):
            continue
        assert entry(l, d, **{name: None}) == EINVAL, name
    assert entry(l, d, traj=None) == EINVAL and entry(l, d, score=None) == EINVAL
    for kw in (dict(B=-1), dict(n_slots=-1), dict(M=0), dict(T=0), dict(H=0), dict(H=31), dict(T=10, H=11), dict(H=-1)):
        assert entry(l, d, **kw) == EINVAL, kw
    for kw in (dict(M=9), dict(T=65, H=65), dict(T=65, H=1), dict(B=1 << 31), dict(n_slots=1 << 31)):
        assert entry(l, d, **kw) == ESHAPE, kw
    for name in PTRS:
        if name != "has":
            assert entry(l, d, **{name: 256 + 8}) == EALIGN, name
    if entry is actors:
        assert actors(l, d, A=-1) == EINVAL and actors(l, d, A=(1 << 24) + 1) == ESHAPE


@pytest.mark.parametrize("entry", [scenes, actors], ids=["scenes", "actors"])
def test_a_bad_drivable_is_refused_before_any_launch(lib, entry):
    l, mod = lib
    inf, nan = float("inf"), float("nan")
    assert entry(l, None) == EINVAL                                       # no lgcn_drivable_t at all
    for kw in (dict(raster=None), dict(city=None), dict(host=False), dict(scene_city=None), dict(n_cities=0), dict(n_cities=-1),
               dict(raster_bytes=-1),
               dict(cities=((0, 0, 9),)), dict(cities=((0, 7, 0),)), dict(cities=((0, -1, 9),)), dict(cities=((0, 7, 9), (63, 5, -4))),
               dict(cities=((-1, 7, 9),)),
               dict(m=(nan, 0., 0., 0., 1., 0.)), dict(m=(1., 0., inf, 0., 1., 0.)), dict(m=(1., 0., 0., 0., 1., -inf)),
               dict(cities=((0, 7, 9), (63, 5, 5))),                      # the second raster ends behind the buffer
               dict(cities=((21, 7, 9),), raster_bytes=83), dict(raster_bytes=82), dict(cities=((84, 1, 1),))):
        d, keep = drivable(mod, **kw)
        assert entry(l, d) == EINVAL, kw
    for kw in (dict(cities=((0, 1 << 31, 1),)), dict(cities=((0, 1, 1 << 31),)), dict(cities=((0, 7, 9), (63, 1 << 40, 1 << 40)))):
        d, keep = drivable(mod, **kw)
        assert entry(l, d) == ESHAPE, kw
    for kw in (dict(city=65536 + 8), dict(scene_city=131072 + 4), dict(scene_city=131072 + 8)):
        d, keep = drivable(mod, **kw)
        assert entry(l, d) == EALIGN, kw
    d, keep = drivable(mod, raster=32768 + 1)                             # bytes: the raster needs no alignment; the next check fails
    assert entry(l, d, reg=None) == EINVAL


def test_dac_reduce_refuses_bad_arguments(lib):
    l, _ = lib
    for name in ("rec", "dac"):
        assert dac_reduce(l, **{name: None}) == EINVAL, name
        assert dac_reduce(l, **{name: 256 + 8}) == EALIGN, name
    for kw in (dict(n_slots=-1), dict(who=-1), dict(who=3), dict(max_missing=-1)):
        assert dac_reduce(l, **kw) == EINVAL, kw
    assert dac_reduce(l, n_slots=1 << 31) == ESHAPE


def test_empty_problems_launch_nothing(lib):
    l, mod = lib
    d, keep = drivable(mod)
    assert scenes(l, d, B=0) == OK and actors(l, d, B=0) == OK and actors(l, d, A=0) == OK
    assert scenes(l, None, B=0) == OK and actors(l, None, A=0) == OK      # `da` is not looked at
    assert scenes(l, d, B=0, reg=None, cls=None, gt=None, has=None, actor_off=None, slot=None) == OK
    assert actors(l, d, A=0, traj=None, score=None) == OK
    assert dac_reduce(l, n_slots=0) == OK and dac_reduce(l, n_slots=0, rec=None, dac=None) == OK


def test_the_python_surface_checks_on_the_host():
    import numpy as np
    import torch
    import lanegcn_amd  # noqa: F401
    from lanegcn_amd import ops
    from lanegcn_amd._lib import LgcnError
    from lanegcn_amd.evaluate import DrivableArea
    z = torch.zeros
    da = DrivableArea({"P": (np.ones((7, 9)), np.eye(3))})
    for fn in (ops.eval_scenes_da, ops.eval_actors_da):
        with pytest.raises(LgcnError):                                    # host tensors: no CPU fallback
            fn(z(1, 6, 30, 2), z(1, 6), z(1, 30, 2), z(1, 30, dtype=torch.bool), z(2, dtype=torch.int32), z(1, dtype=torch.int64),
               30, z(4, 32), err=z(1, dtype=torch.int32), da=da, scene_city=z(1, dtype=torch.int32))
    with pytest.raises(LgcnError):
        ops.eval_dac_reduce(z(4, 32), 0, 0, z(9, dtype=torch.int64))
