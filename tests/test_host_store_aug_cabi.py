"""CPU: lgcn_store_gather_aug is exported, bound and declared; it refuses everything lgcn_store_gather refuses, with the
same code, and the three conditions of its own (a NULL table, a non-finite entry, a misaligned device table) -- all before
anything is launched: the jobs point at placeholder addresses, and this test runs without a GPU."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import test_host_store_cabi as T

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL, ESHAPE, EALIGN = -1, -2, -3
NAME = "lgcn_store_gather_aug"


@pytest.fixture(scope="module")
def lib():
    import lanegcn_amd  # noqa: F401
    from lanegcn_amd import _lib
    return _lib.load(), _lib


def _aug(n=3):
    rng = np.random.default_rng(0)
    return np.ascontiguousarray(rng.uniform(-1, 1, (n, 8)).astype(np.float32))


def run_aug(l, s, b, aug_host, aug_dev=512):
    host = None if aug_host is None else aug_host.ctypes.data
    return l.lgcn_store_gather_aug(None if s is None else C.byref(s), None if b is None else C.byref(b), host, aug_dev, None)


def run_plain(l, s, b):
    return l.lgcn_store_gather(None if s is None else C.byref(s), None if b is None else C.byref(b), None)


def test_symbol_is_exported_bound_and_declared(lib):
    l, mod = lib
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "lgcn.h")).read(), flags=re.S)
    assert hasattr(l, NAME) and NAME in mod.SIGNATURES
    m = re.search(r"\bint\s+%s\s*\(([^)]*)\)" % NAME, header)
    assert m, "not declared"
    args = [re.sub(r"\s+", " ", a.strip()) for a in m.group(1).split(",")]
    assert args == ["const lgcn_store_t *s", "const lgcn_store_batch_t *b", "const float *aug_host", "const float *aug_dev",
                    "void *stream"]
    restype, argtypes = mod.SIGNATURES[NAME]
    assert restype is C.c_int and len(argtypes) == 5
    # the two structs are those of lgcn_store_gather, unchanged
    assert C.sizeof(mod.Store) == 4 * 8 + 13 * 8 and C.sizeof(mod.StoreBatch) == 2 * 4 + 3 * 8 + 18 * 8


def _mutations(mod):
    """Every refused job of test_host_store_cabi.test_bad_arguments_are_refused_before_any_launch, as (label, make) with
    make() -> (store, batch, the table that batch points into)."""
    B, G = 3, 12
    out = []

    def add(label, change):
        def make():
            s, b, tab = T._job(mod)
            change(s, b, tab)
            return s, b, tab
        out.append((label, make))

    for field in ("n_scenes", "n_nodes", "n_actors", "n_edges"):
        add(("store size", field), lambda s, b, tab, f=field: setattr(s, f, -1))
    for field in ("n_scenes", "n_rel", "n_nodes", "n_actors", "n_elem"):
        add(("batch size", field), lambda s, b, tab, f=field: setattr(b, f, -1))
    for field in T.STORE_PTRS:
        add(("store null", field), lambda s, b, tab, f=field: setattr(s, f, None))
    for field in ("tab_host",) + T.BATCH_PTRS:
        add(("batch null", field), lambda s, b, tab, f=field: setattr(b, f, None))
    for start, n, total in ((0, B, "n_nodes"), (B + 1, B, "n_actors"), (5 * B + 2, G, "n_elem")):
        for at, val in ((0, 1), (1, -1), (2, 1 << 20)):
            add(("prefix", start, at), lambda s, b, tab, i=start + at, v=val: tab.__setitem__(i, v))
        add(("prefix end", start), lambda s, b, tab, i=start + n: tab.__setitem__(i, tab[i] + 1))
        add(("total", total), lambda s, b, tab, f=total: setattr(b, f, getattr(b, f) + 1))
    n_edges = T._job(mod)[0].n_edges
    for at, val in ((2 * B + 2, -1), (2 * B + 2, 6), (2 * B + 3, 13), (3 * B + 2, -1), (3 * B + 3, 4), (3 * B + 4, 1 << 40),
                    (4 * B + 2, -1), (4 * B + 2, 3), (5 * B + G + 3, -1), (5 * B + 2 * G + 2, 1 << 33),
                    (5 * B + 2 * G + 2, n_edges)):
        add(("source", at, val), lambda s, b, tab, i=at, v=val: tab.__setitem__(i, v))
    for field, val in (("n_nodes", 1 << 31), ("n_elem", 1 << 31), ("n_actors", (1 << 31) // 60 + 1), ("n_rel", 1 << 30)):
        add(("too large", field), lambda s, b, tab, f=field, v=val: setattr(b, f, v))
    for obj, field, val in (("s", "node_ctrs", 264), ("s", "rot", 264), ("s", "control", 258), ("s", "edge_v", 258),
                            ("s", "gt_preds", 258), ("b", "tab_dev", 264), ("b", "turn", 264), ("b", "idx_local", 264),
                            ("b", "seg_base", 264), ("b", "orig", 264), ("b", "node_off", 258), ("b", "actor_feats", 258),
                            ("b", "gt_preds", 258)):
        add(("alignment", obj, field), lambda s, b, tab, o=obj, f=field, v=val: setattr(s if o == "s" else b, f, v))
    add(("only has_preds",), lambda s, b, tab: setattr(s, "gt_preds", None))
    add(("only gt_preds",), lambda s, b, tab: setattr(s, "has_preds", None))
    return out


def test_every_refusal_of_the_plain_entry_is_a_refusal_of_this_one(lib):
    l, mod = lib
    aug = _aug()
    assert run_aug(l, None, T._job(mod)[1], aug) == run_plain(l, None, T._job(mod)[1]) == EINVAL
    assert run_aug(l, T._job(mod)[0], None, aug) == run_plain(l, T._job(mod)[0], None) == EINVAL
    e = mod.StoreBatch()
    e.n_nodes = 1
    assert run_aug(l, T._job(mod)[0], e, aug) == run_plain(l, T._job(mod)[0], e) == EINVAL
    muts = _mutations(mod)
    assert len(muts) > 80
    codes = set()
    for label, make in muts:
        s, b, tab = make()
        want = run_plain(l, s, b)
        assert want in (EINVAL, ESHAPE, EALIGN), label
        s, b, tab = make()
        assert run_aug(l, s, b, aug) == want, label
        codes.add(want)
    assert codes == {EINVAL, ESHAPE, EALIGN}


def test_the_refusals_of_its_own(lib):
    l, mod = lib
    s, b, tab = T._job(mod)
    aug = _aug()
    assert run_aug(l, s, b, None) == EINVAL
    assert run_aug(l, s, b, aug, aug_dev=None) == EINVAL
    for bad in (float("nan"), float("inf"), -float("inf")):
        for at in (0, 7, 8 * 3 - 1):
            a = _aug()
            a.reshape(-1)[at] = bad
            assert run_aug(l, s, b, a) == EINVAL, (bad, at)
    for ptr in (264, 516, 520, 513):
        assert run_aug(l, s, b, aug, aug_dev=ptr) == EALIGN, ptr
    # a refusal of the shared checks comes first: a misaligned batch pointer with a NULL table is EALIGN, not EINVAL
    s2, b2, tab2 = T._job(mod)
    b2.turn = 264
    assert run_aug(l, s2, b2, None) == EALIGN


def test_an_empty_job_returns_as_the_plain_entry_does(lib):
    l, mod = lib
    s, b, tab = T._job(mod)
    assert run_aug(l, mod.Store(), mod.StoreBatch(), None, aug_dev=None) == run_plain(l, mod.Store(), mod.StoreBatch()) == 0
    assert run_aug(l, s, mod.StoreBatch(), None, aug_dev=None) == run_plain(l, s, mod.StoreBatch()) == 0


def test_public_wrapper_takes_both_tables_or_neither():
    import inspect
    import lanegcn_amd  # noqa: F401
    from lanegcn_amd import ops
    from lanegcn_amd.flatfile import DeviceSceneStore, FlatSceneFile
    p = inspect.signature(ops.store_gather).parameters
    assert p["aug_host"].default is None and p["aug_dev"].default is None
    assert inspect.signature(DeviceSceneStore.batch).parameters["rot_dt"].default is None
    assert inspect.signature(FlatSceneFile.batch).parameters["rot_dt"].default is None
