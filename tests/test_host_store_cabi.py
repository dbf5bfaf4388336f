"""CPU: the scene-store entry points (lgcn_store_*) are exported, bound and declared, refuse bad arguments before
launching anything, size the per-batch table monotonically, and flatfile.DeviceSceneStore refuses to run without a GPU."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("lgcn_store_table_elems", "lgcn_store_gather")
EINVAL, ESHAPE, EALIGN = -1, -2, -3
STORE_PTRS = ("node_ctrs", "node_feats", "turn", "control", "intersect", "actor_ctrs", "actor_feats", "rot", "orig", "gt_preds",
              "has_preds", "edge_u", "edge_v")
BATCH_PTRS = ("tab_dev", "node_ctrs", "node_feats", "turn", "control", "intersect", "actor_ctrs", "node_off", "actor_off",
              "idx_local", "seg_off", "seg_base", "actor_feats", "rot", "orig", "gt_preds", "has_preds")


@pytest.fixture(scope="module")
def lib():
    import lanegcn_amd  # noqa: F401
    from lanegcn_amd import _lib
    return _lib.load(), _lib


def test_symbols_are_exported_bound_and_declared(lib):
    l, mod = lib
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "lgcn.h")).read(), flags=re.S)
    for n in NAMES:
        assert hasattr(l, n) and n in mod.SIGNATURES and re.search(r"\b%s\s*\(" % n, header), n
    assert "lgcn_store_t" in header and "lgcn_store_batch_t" in header
    # lgcn_store_t: 4 int64 sizes, then 13 pointers; lgcn_store_batch_t: 2 int32 + 3 int64 sizes, then 18 pointers
    assert C.sizeof(mod.Store) == 4 * 8 + 13 * 8 and mod.Store.node_ctrs.offset == 32
    assert [n for n, _ in mod.Store._fields_[4:]] == list(STORE_PTRS)
    assert C.sizeof(mod.StoreBatch) == 2 * 4 + 3 * 8 + 18 * 8 and mod.StoreBatch.tab_host.offset == 32
    assert [n for n, _ in mod.StoreBatch._fields_[5:]] == ["tab_host"] + list(BATCH_PTRS)


def test_table_size_helper(lib):
    l, _ = lib
    te = l.lgcn_store_table_elems
    assert te(0, 0) >= 0 and te(-1, 14) == EINVAL and te(32, -1) == EINVAL
    base = te(32, 14)
    assert base == 5 * 32 + 2 * (2 * 14 * 32) + 3
    assert te(33, 14) > base and te(32, 15) > base and te(70, 14) > te(64, 14)
    assert te(1 << 40, 14) == ESHAPE and te(32, 1 << 40) == ESHAPE and te(1 << 24, 1 << 6) == ESHAPE


def _job(mod, pick=(1, 0, 1), n_rel=2):
    """A three-scene store and a batch of `pick` over placeholder device pointers (nothing is launched on a refused
    call): scenes of 5 / 7 / 0 nodes and 2 / 0 / 3 actors, relation r of scene s has s + r edges."""
    node_off, actor_off = np.array([0, 5, 12, 12]), np.array([0, 2, 2, 5])
    edge_off = np.array([[0] + list(np.cumsum([s + r for s in range(3)])) for r in range(n_rel)])
    rel_off = np.concatenate([[0], np.cumsum(edge_off[:, -1])])
    s = mod.Store()
    s.n_scenes, s.n_nodes, s.n_actors, s.n_edges = 3, 12, 5, int(rel_off[-1])
    for name in STORE_PTRS:
        setattr(s, name, 256)
    idx = np.asarray(pick, np.int64)
    B, G = len(idx), 2 * n_rel * len(idx)
    cs = lambda x: np.concatenate([[0], np.cumsum(x)])
    lo = rel_off[:n_rel, None] + edge_off[:, idx]
    ln = edge_off[:, idx + 1] - edge_off[:, idx]
    tab = np.concatenate([cs(node_off[idx + 1] - node_off[idx]), cs(actor_off[idx + 1] - actor_off[idx]), node_off[idx],
                          actor_off[idx], idx, cs(np.repeat(ln[:, None, :], 2, 1).reshape(-1)),
                          np.repeat(lo[:, None, :], 2, 1).reshape(-1)]).astype(np.int64)
    b = mod.StoreBatch()
    b.n_scenes, b.n_rel = B, n_rel
    b.n_nodes, b.n_actors, b.n_elem = int(tab[B]), int(tab[2 * B + 1]), int(tab[5 * B + 2 + G])
    b.tab_host = tab.ctypes.data
    for name in BATCH_PTRS:
        setattr(b, name, 256)
    return s, b, tab


def _run(l, s, b):
    return l.lgcn_store_gather(C.byref(s), C.byref(b), None)


def test_bad_arguments_are_refused_before_any_launch(lib):
    l, mod = lib
    s, b, tab = _job(mod)
    assert tab.size == l.lgcn_store_table_elems(3, 2)
    assert l.lgcn_store_gather(None, C.byref(b), None) == EINVAL and l.lgcn_store_gather(C.byref(s), None, None) == EINVAL
    assert _run(l, mod.Store(), mod.StoreBatch()) == 0                 # an empty job: nothing to do
    assert _run(l, s, mod.StoreBatch()) == 0
    e = mod.StoreBatch()
    e.n_nodes = 1
    assert _run(l, s, e) == EINVAL                                      # rows without a scene
    for field in ("n_scenes", "n_nodes", "n_actors", "n_edges"):
        s, b, tab = _job(mod)
        setattr(s, field, -1)
        assert _run(l, s, b) == EINVAL, field
    for field in ("n_scenes", "n_rel", "n_nodes", "n_actors", "n_elem"):
        s, b, tab = _job(mod)
        setattr(b, field, -1)
        assert _run(l, s, b) == EINVAL, field
    # a null pointer next to a non-zero size
    for field in STORE_PTRS:
        s, b, tab = _job(mod)
        setattr(s, field, None)
        assert _run(l, s, b) == EINVAL, field
    for field in ("tab_host",) + BATCH_PTRS:
        s, b, tab = _job(mod)
        setattr(b, field, None)
        assert _run(l, s, b) == EINVAL, field
    # the table's prefix sums: not from 0, decreasing, wrong total -- for nodes, actors and segments
    B, G = 3, 12
    for start, n, total in ((0, B, "n_nodes"), (B + 1, B, "n_actors"), (5 * B + 2, G, "n_elem")):
        for at, val in ((0, 1), (1, -1), (2, 1 << 20)):
            s, b, tab = _job(mod)
            tab[start + at] = val
            assert _run(l, s, b) == EINVAL, (start, at)
        s, b, tab = _job(mod)
        tab[start + n] += 1
        assert _run(l, s, b) == EINVAL, start
        s, b, tab = _job(mod)
        setattr(b, total, getattr(b, total) + 1)
        assert _run(l, s, b) == EINVAL, total
    # a source offset outside the store: negative, past the end, a run that ends past the end; a scene outside [0, S)
    for at, val in ((2 * B + 2, -1), (2 * B + 2, 6), (2 * B + 3, 13), (3 * B + 2, -1), (3 * B + 3, 4), (3 * B + 4, 1 << 40),
                    (4 * B + 2, -1), (4 * B + 2, 3), (5 * B + G + 3, -1), (5 * B + 2 * G + 2, 1 << 33),
                    (5 * B + 2 * G + 2, s.n_edges)):
        s, b, tab = _job(mod)
        tab[at] = val
        assert _run(l, s, b) == EINVAL, (at, val)
    # totals past 2^31 - 1: refused by size, before the table is looked at
    for field, val in (("n_nodes", 1 << 31), ("n_elem", 1 << 31), ("n_actors", (1 << 31) // 60 + 1)):
        s, b, tab = _job(mod)
        setattr(b, field, val)
        assert _run(l, s, b) == ESHAPE, field
    s, b, tab = _job(mod)
    b.n_rel = 1 << 30
    assert _run(l, s, b) == ESHAPE
    # alignment: 16 bytes for the [.,2] arrays, rot, orig and the int64 arrays, 4 for the other words
    for obj, field, val, rc in (("s", "node_ctrs", 264, EALIGN), ("s", "rot", 264, EALIGN), ("s", "control", 258, EALIGN),
                                ("s", "edge_v", 258, EALIGN), ("s", "gt_preds", 258, EALIGN), ("b", "tab_dev", 264, EALIGN),
                                ("b", "turn", 264, EALIGN), ("b", "idx_local", 264, EALIGN), ("b", "seg_base", 264, EALIGN),
                                ("b", "orig", 264, EALIGN), ("b", "node_off", 258, EALIGN), ("b", "actor_feats", 258, EALIGN),
                                ("b", "gt_preds", 258, EALIGN)):
        s, b, tab = _job(mod)
        setattr(s if obj == "s" else b, field, val)
        assert _run(l, s, b) == rc, field
    # a store without gt_preds / has_preds: both null is a store that has none, one alone is refused
    s, b, tab = _job(mod)
    s.gt_preds = None
    assert _run(l, s, b) == EINVAL
    s, b, tab = _job(mod)
    s.has_preds = None
    assert _run(l, s, b) == EINVAL


def test_public_interface_refuses_to_run_without_a_gpu(tmp_path):
    import lanegcn_amd  # noqa: F401
    from lanegcn_amd import data as gen
    from lanegcn_amd import lanegcn as M
    from lanegcn_amd import ops
    from lanegcn_amd._lib import LgcnError
    from lanegcn_amd.flatfile import DeviceSceneStore, write_scenes
    assert callable(DeviceSceneStore.plan) and callable(DeviceSceneStore.batch) and callable(M.Net.forward_store)
    assert ops.store_table_elems(32, 14) == 5 * 32 + 4 * 14 * 32 + 3
    with pytest.raises(LgcnError):
        ops.store_table_elems(-1, 14)
    if torch.cuda.is_available():
        return          # with a GPU the calls run: tests/test_gpu_scene_store.py
    path = str(tmp_path / "split.npz")
    write_scenes(path, [gen.synth_scene(np.random.default_rng(0), [4], 3)])
    with pytest.raises(LgcnError):
        DeviceSceneStore(path)
    with pytest.raises(LgcnError):                                      # the wrapper takes device tensors only
        ops.StoreJob({k: torch.zeros(0) for k in ops.STORE_FLOATS + ("edge_u", "edge_v")})
