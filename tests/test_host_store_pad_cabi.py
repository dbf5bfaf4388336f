"""CPU: the padded-gather entry points (lgcn_store_pad_check, lgcn_store_gather_pad) are exported, bound and declared and
refuse bad arguments before launching anything; lgcn_store_pad_check decides the fit of a pick on the host."""
import ctypes as C
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("lgcn_store_pad_check", "lgcn_store_gather_pad")
OK, EINVAL, ESHAPE, EALIGN = 0, -1, -2, -3
STORE_PTRS = ("node_ctrs", "node_feats", "turn", "control", "intersect", "actor_ctrs", "actor_feats", "rot", "orig", "gt_preds",
              "has_preds", "edge_u", "edge_v")
BATCH_PTRS = ("tab_dev", "node_ctrs", "node_feats", "turn", "control", "intersect", "actor_ctrs", "node_off", "actor_off",
              "idx_local", "seg_off", "seg_base", "actor_feats", "rot", "orig", "gt_preds", "has_preds")
N_REL = 2
NODE_OFF, ACTOR_OFF = np.array([0, 5, 12, 12]), np.array([0, 2, 2, 5])
EDGE_OFF = np.array([[0] + list(np.cumsum([s + r for s in range(3)])) for r in range(N_REL)])


@pytest.fixture(scope="module")
def lib():
    import lanegcn_amd  # noqa: F401
    from lanegcn_amd import _lib
    return _lib.load(), _lib


def _job(mod, pick=(1, 0, 1), slack=(3, 2, (4, 0))):
    """A three-scene store (5 / 7 / 0 nodes, 2 / 0 / 3 actors, relation r of scene s has s + r edges) and the padded batch
    of `pick` over placeholder device pointers: capacities = the pick's totals + slack (nodes, actors, edges per relation).
    The table is flatfile.plan_batch's."""
    from lanegcn_amd.flatfile import StoreCaps, plan_batch
    rel_off = np.concatenate([[0], np.cumsum(EDGE_OFF[:, -1])])
    s = mod.Store()
    s.n_scenes, s.n_nodes, s.n_actors, s.n_edges = 3, 12, 5, int(rel_off[-1])
    for name in STORE_PTRS:
        setattr(s, name, 256)
    idx = np.asarray(pick, np.int64)
    n, a = int((NODE_OFF[idx + 1] - NODE_OFF[idx]).sum()), int((ACTOR_OFF[idx + 1] - ACTOR_OFF[idx]).sum())
    e = (EDGE_OFF[:, idx + 1] - EDGE_OFF[:, idx]).sum(1)
    caps = StoreCaps(len(idx), n + slack[0], a + slack[1], tuple(int(x + y) for x, y in zip(e, slack[2])))
    plan = plan_batch(NODE_OFF, ACTOR_OFF, EDGE_OFF, rel_off, 0, idx, caps=caps)
    tab = plan.table.copy()
    b = mod.StoreBatch()
    b.n_scenes, b.n_rel = len(idx) + 1, N_REL
    b.n_nodes, b.n_actors, b.n_elem = caps.nodes, caps.actors, 2 * sum(caps.edges)
    for name in BATCH_PTRS:
        setattr(b, name, 256)
    return s, b, tab


def _check(l, s, b, tab):
    return l.lgcn_store_pad_check(C.byref(s), C.byref(b), tab.ctypes.data)


def _launch(l, s, b):
    return l.lgcn_store_gather_pad(C.byref(s), C.byref(b), None)


def _both(l, s, b, tab):
    return _check(l, s, b, tab), _launch(l, s, b)


def test_symbols_are_exported_bound_and_declared(lib):
    l, mod = lib
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "lgcn.h")).read(), flags=re.S)
    for n in NAMES:
        assert hasattr(l, n) and n in mod.SIGNATURES and re.search(r"\b%s\s*\(" % n, header), n


def test_a_good_table_passes_the_check(lib):
    l, mod = lib
    s, b, tab = _job(mod)
    assert tab.size == l.lgcn_store_table_elems(4, N_REL)
    assert _check(l, s, b, tab) == OK
    assert b.tab_host is None                       # the check reads its own argument, the launch no host table at all


def test_bad_arguments_are_refused_by_both_entries(lib):
    """Sizes, pointers and alignment: the check and the launch give the same code, and the launch returns before it
    launches (there is no GPU here, and the pointers are placeholders)."""
    l, mod = lib
    s, b, tab = _job(mod)
    assert l.lgcn_store_pad_check(None, C.byref(b), tab.ctypes.data) == EINVAL
    assert l.lgcn_store_pad_check(C.byref(s), None, tab.ctypes.data) == EINVAL
    assert l.lgcn_store_pad_check(C.byref(s), C.byref(b), None) == EINVAL
    assert l.lgcn_store_gather_pad(None, C.byref(b), None) == EINVAL and l.lgcn_store_gather_pad(C.byref(s), None, None) == EINVAL
    # a padded batch always holds a picked scene and the filler, and the filler one node and one actor
    assert _both(l, mod.Store(), mod.StoreBatch(), tab) == (EINVAL, EINVAL)
    for field, val in (("n_scenes", 1), ("n_scenes", 0), ("n_nodes", 0), ("n_actors", 0)):
        s, b, tab = _job(mod)
        setattr(b, field, val)
        assert _both(l, s, b, tab) == (EINVAL, EINVAL), field
    for field in ("n_scenes", "n_nodes", "n_actors", "n_edges"):
        s, b, tab = _job(mod)
        setattr(s, field, -1)
        assert _both(l, s, b, tab) == (EINVAL, EINVAL), field
    for field in ("n_scenes", "n_rel", "n_nodes", "n_actors", "n_elem"):
        s, b, tab = _job(mod)
        setattr(b, field, -1)
        assert _both(l, s, b, tab) == (EINVAL, EINVAL), field
    for field in STORE_PTRS:
        s, b, tab = _job(mod)
        setattr(s, field, None)
        assert _both(l, s, b, tab) == (EINVAL, EINVAL), field
    for field in BATCH_PTRS:
        s, b, tab = _job(mod)
        setattr(b, field, None)
        assert _both(l, s, b, tab) == (EINVAL, EINVAL), field
    for field, val in (("n_nodes", 1 << 31), ("n_elem", 1 << 31), ("n_actors", (1 << 31) // 60 + 1)):
        s, b, tab = _job(mod)
        setattr(b, field, val)
        assert _both(l, s, b, tab) == (ESHAPE, ESHAPE), field
    for obj, field, val in (("s", "node_ctrs", 264), ("s", "rot", 264), ("s", "control", 258), ("s", "edge_v", 258),
                            ("s", "gt_preds", 258), ("b", "tab_dev", 264), ("b", "turn", 264), ("b", "idx_local", 264),
                            ("b", "seg_base", 264), ("b", "orig", 264), ("b", "node_off", 258), ("b", "actor_feats", 258),
                            ("b", "gt_preds", 258)):
        s, b, tab = _job(mod)
        setattr(s if obj == "s" else b, field, val)
        assert _both(l, s, b, tab) == (EALIGN, EALIGN), field
    s, b, tab = _job(mod)
    odd = np.zeros(tab.size * 8 + 8, np.uint8)
    view = odd[4:4 + tab.size * 8]
    view[:] = tab.view(np.uint8)
    assert l.lgcn_store_pad_check(C.byref(s), C.byref(b), view.ctypes.data) == EALIGN      # tab_host: 8 bytes


def test_the_table_is_checked_on_the_host(lib):
    l, mod = lib
    B1, G1 = 4, 2 * N_REL * 4
    at_node_src, at_actor_src, at_scene = 2 * B1 + 2, 3 * B1 + 2, 4 * B1 + 2
    at_seg_off, at_seg_src = 5 * B1 + 2, 5 * B1 + G1 + 3
    # a table that does not end at the capacities
    for field in ("n_nodes", "n_actors", "n_elem"):
        s, b, tab = _job(mod)
        setattr(b, field, getattr(b, field) + 1)
        assert _check(l, s, b, tab) == EINVAL, field
    for at in (B1, 2 * B1 + 1, at_seg_off + G1):
        s, b, tab = _job(mod)
        tab[at] += 1
        assert _check(l, s, b, tab) == EINVAL, at
    # prefix sums that do not start at 0 or decrease among the picked scenes
    for start in (0, B1 + 1, at_seg_off):
        for at, val in ((0, 1), (1, -1), (2, 1 << 20)):
            s, b, tab = _job(mod)
            tab[start + at] = val
            assert _check(l, s, b, tab) == EINVAL, (start, at)
    # a missing filler entry: the last scene with a source inside the store
    for at in (at_node_src + 3, at_actor_src + 3, at_scene + 3, at_seg_src + 3, at_seg_src + G1 - 1):
        s, b, tab = _job(mod)
        assert tab[at] == -1
        tab[at] = 0
        assert _check(l, s, b, tab) == EINVAL, at
    # a filler entry that is not the last one; a source outside the store
    for at, val in ((at_node_src, -1), (at_actor_src + 1, -1), (at_scene + 2, -1), (at_seg_src, -1), (at_seg_src + 5, -1),
                    (at_node_src, 13), (at_actor_src, 6), (at_scene, 3), (at_seg_src, 1 << 33)):
        s, b, tab = _job(mod)
        tab[at] = val
        assert _check(l, s, b, tab) == EINVAL, (at, val)


def test_fit_is_decided_by_the_check(lib):
    """A pick one node / actor / edge too large for the capacities is LGCN_ESHAPE, the exact fit LGCN_OK."""
    l, mod = lib
    s, b, tab = _job(mod, slack=(1, 1, (0, 0)))          # n_f = a_f = 1, every filler segment empty
    assert _check(l, s, b, tab) == OK
    B1 = 4
    for less in (1, 2):                                  # capacities of N and N - 1 nodes: the filler has none / the pick is too large
        s, b, tab = _job(mod, slack=(1, 1, (0, 0)))
        b.n_nodes -= less
        tab[B1] -= less
        assert _check(l, s, b, tab) == ESHAPE, less
        s, b, tab = _job(mod, slack=(1, 1, (0, 0)))
        b.n_actors -= less
        tab[B1 + 1 + B1] -= less
        assert _check(l, s, b, tab) == ESHAPE, less
    s, b, tab = _job(mod, slack=(1, 1, (0, 0)))
    at_seg_off = 5 * B1 + 2
    tab[at_seg_off + B1 - 1:at_seg_off + B1] += 1        # relation 0's u: one edge more than its block holds
    assert _check(l, s, b, tab) == ESHAPE
    # the plan refuses the same picks by name before a table exists
    from lanegcn_amd.flatfile import StoreFitError
    for slack in ((0, 1, (0, 0)), (1, 0, (0, 0)), (1, 1, (0, -1))):
        with pytest.raises(StoreFitError):
            _job(mod, slack=slack)


def test_check_finite_rows_refuses_bad_arguments(lib):
    """The range guard over the real rows of a padded batch: exported, bound, declared, and refused before a launch."""
    l, mod = lib
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "lgcn.h")).read(), flags=re.S)
    assert "lgcn_check_finite_rows" in mod.SIGNATURES and re.search(r"\blgcn_check_finite_rows\s*\(", header)
    f = l.lgcn_check_finite_rows
    good = dict(a=256, na=128 * 5, row_a=128, rows_a=512, b=1024, nb=6 * 5, row_b=6, rows_b=520, flag=64, bit=1)
    call = lambda **kw: f(*[{**good, **kw}[k] for k in good], None)
    assert call(na=0, nb=0) == OK                                       # nothing to look at: no launch
    for kw in (dict(na=-1), dict(nb=-128), dict(bit=0), dict(flag=None), dict(a=None), dict(rows_a=None), dict(b=None),
               dict(rows_b=None), dict(row_a=0), dict(row_b=-6), dict(row_a=96), dict(row_b=4)):
        assert call(**kw) == EINVAL, kw
    for kw in (dict(a=260), dict(b=1032), dict(rows_a=516), dict(rows_b=524)):
        assert call(**kw) == EALIGN, kw
