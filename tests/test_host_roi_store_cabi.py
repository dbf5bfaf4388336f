"""CPU: the RoI-store entry points (lgcn_roi_store_table_elems, lgcn_roi_store_gather) are exported, bound and declared,
refuse every bad argument with its code before launching anything, and data_lrcnn.RoiStore refuses to run without a
GPU while its host half (plan_roi_batch) does not need one."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("lgcn_roi_store_table_elems", "lgcn_roi_store_gather")
EINVAL, ESHAPE, EALIGN = -1, -2, -3
K, Q = 14, 30
STORE_PTRS = ("feats", "node_mask", "agent_feat", "edge_u", "edge_v", "a2m_u", "a2m_v", "ctrs", "actor_feats", "obs", "gt_preds",
              "has_preds")
BATCH_PTRS = ("tab_dev", "feats", "node_mask", "agent_feat", "idx", "ctrs", "actor_feats", "obs", "gt_preds", "has_preds")


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
    assert "lgcn_roi_store_t" in header and "lgcn_roi_store_batch_t" in header
    # lgcn_roi_store_t: 5 int64 sizes, then 12 pointers; lgcn_roi_store_batch_t: 4 int64 sizes, then 11 pointers
    assert C.sizeof(mod.RoiStore) == 5 * 8 + 12 * 8 and mod.RoiStore.feats.offset == 40
    assert [n for n, _ in mod.RoiStore._fields_[5:]] == list(STORE_PTRS)
    assert C.sizeof(mod.RoiStoreBatch) == 4 * 8 + 11 * 8 and mod.RoiStoreBatch.tab_host.offset == 32
    assert [n for n, _ in mod.RoiStoreBatch._fields_[4:]] == ["tab_host"] + list(BATCH_PTRS)


def test_table_size_helper(lib):
    l, _ = lib
    te = l.lgcn_roi_store_table_elems
    assert te(0) == 3 and te(-1) == EINVAL and te(-(1 << 40)) == EINVAL
    assert te(32) == 4 * 32 + 2 * Q * 32 + 3 and te(33) > te(32) and te(70) == 64 * 70 + 3
    assert te(1 << 40) == ESHAPE and te(1 << 62) == ESHAPE and te((1 << 31) // 64) == ESHAPE
    assert te(((1 << 31) - 1 - 3) // 64) > 0


def _job(mod, pick=(2, 0, 2)):
    """A three-scene store (scene 1 holds no RoI) and a batch of `pick` over placeholder device pointers (nothing is
    launched on a refused call): scenes of 2 / 0 / 3 RoIs and 13 / 0 / 20 nodes; relation k of scene s has s + k edges
    and relations 5 and 13 none, a2m 4 / 0 / 6."""
    first_roi, node_off = np.array([0, 2, 2, 5]), np.array([0, 13, 13, 33])
    per = np.array([[0 if k in (5, 13) or s == 1 else s + k for s in range(3)] for k in range(K)] + [[4, 0, 6]])
    edge_off = np.concatenate([np.zeros((K + 1, 1), np.int64), np.cumsum(per, 1)], 1)
    rel_at = np.concatenate([np.cumsum(edge_off[:K, -1]) - edge_off[:K, -1], [0]])
    s = mod.RoiStore()
    s.n_scenes, s.n_nodes, s.n_rois, s.n_edges, s.n_a2m = 3, 33, 5, int(edge_off[:K, -1].sum()), int(edge_off[K, -1])
    for name in STORE_PTRS:
        setattr(s, name, 256)
    idx = np.asarray(pick, np.int64)
    B = len(idx)
    cs = lambda x: np.concatenate([[0], np.cumsum(x)])
    ln, lo = edge_off[:, idx + 1] - edge_off[:, idx], edge_off[:, idx] + rel_at[:, None]
    runs = lambda x: np.concatenate([x[:K], x[:K], x[K:], x[K:]]).reshape(-1)
    tab = np.concatenate([cs(node_off[idx + 1] - node_off[idx]), cs(first_roi[idx + 1] - first_roi[idx]), node_off[idx],
                          first_roi[idx], cs(runs(ln)), runs(lo)]).astype(np.int64)
    b = mod.RoiStoreBatch()
    b.n_scenes, b.n_nodes, b.n_rois, b.n_elem = B, int(tab[B]), int(tab[2 * B + 1]), int(tab[4 * B + 2 + Q * B])
    b.tab_host = tab.ctypes.data
    for name in BATCH_PTRS:
        setattr(b, name, 256)
    return s, b, tab


def _run(l, s, b):
    return l.lgcn_roi_store_gather(C.byref(s), C.byref(b), None)


def test_the_plan_of_the_library_is_the_table_the_entry_point_checks(lib):
    """The table of _job is plan_roi_batch's for the same tables (so the refusals below start from a valid call)."""
    _, mod = lib
    from lanegcn_amd import data_lrcnn as D
    s, b, tab = _job(mod)
    first_roi, node_off = np.array([0, 2, 2, 5]), np.array([0, 13, 13, 33])
    per = np.array([[0 if k in (5, 13) or s_ == 1 else s_ + k for s_ in range(3)] for k in range(K)] + [[4, 0, 6]])
    edge_off = np.concatenate([np.zeros((K + 1, 1), np.int64), np.cumsum(per, 1)], 1)
    tb = dict(first_roi=first_roi, node_off=node_off, edge_off=edge_off, sizes=np.array([6, 7, 6, 7, 7]),
              agent_vel=np.zeros(5, np.float32), edge_cnt=np.zeros((5, K + 1), np.int64), agent_ids=np.arange(5))
    p = D.plan_roi_batch(tb, [2, 0, 2])
    assert p.table.tobytes() == tab.tobytes() and (p.n_nodes, p.n_rois, p.n_elem) == (b.n_nodes, b.n_rois, b.n_elem)


def test_bad_arguments_are_refused_before_any_launch(lib):
    l, mod = lib
    s, b, tab = _job(mod)
    B, G = 3, 3 * Q
    assert tab.size == l.lgcn_roi_store_table_elems(B)
    assert l.lgcn_roi_store_gather(None, C.byref(b), None) == EINVAL and l.lgcn_roi_store_gather(C.byref(s), None, None) == EINVAL
    assert _run(l, mod.RoiStore(), mod.RoiStoreBatch()) == 0          # a pick of 0 scenes, all totals 0: nothing to do
    assert _run(l, s, mod.RoiStoreBatch()) == 0
    for field in ("n_nodes", "n_rois", "n_elem"):
        e = mod.RoiStoreBatch()
        setattr(e, field, 1)
        assert _run(l, s, e) == EINVAL, field                         # rows without a scene
    for field in ("n_scenes", "n_nodes", "n_rois", "n_edges", "n_a2m"):
        s, b, tab = _job(mod)
        setattr(s, field, -1)
        assert _run(l, s, b) == EINVAL, field
    for field in ("n_scenes", "n_nodes", "n_rois", "n_elem"):
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
    # only one of gt_preds / has_preds; neither is a store without gt (the batch's pointers for them are then not used)
    for one in ("gt_preds", "has_preds"):
        s, b, tab = _job(mod)
        setattr(s, one, None)
        b.tab_dev = 264                                                # (every call here is refused: nothing may launch)
        assert _run(l, s, b) == EINVAL, one
    s, b, tab = _job(mod)
    s.gt_preds = s.has_preds = None
    b.gt_preds = b.has_preds = None
    b.tab_dev = 264
    assert _run(l, s, b) == EALIGN                                     # it got past the pointer checks to the alignment
    # the table's prefix sums: not from 0, decreasing, wrong total -- for nodes, RoIs and segments
    for start, n, total in ((0, B, "n_nodes"), (B + 1, B, "n_rois"), (4 * B + 2, G, "n_elem")):
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
    # a source run outside the store: negative, past the end, a run that ends past the end -- node rows, RoIs, the u / v
    # segments (against n_edges) and the a2m segments (against n_a2m)
    s0 = _job(mod)[0]
    seg = 4 * B + G + 3
    for at, val in ((2 * B + 2, -1), (2 * B + 2, 14), (2 * B + 3, 34), (2 * B + 3, 21), (3 * B + 2, -1), (3 * B + 2, 3),
                    (3 * B + 3, 6), (3 * B + 4, 1 << 40), (seg, -1), (seg + 1, 1 << 33), (seg + 1, s0.n_edges + 1),
                    (seg + 3 * 12 + 2, s0.n_edges - 1), (seg + 28 * B, -1), (seg + 28 * B, s0.n_a2m - 1),
                    (seg + 29 * B + 2, s0.n_a2m), (seg + 29 * B + 1, s0.n_edges)):
        s, b, tab = _job(mod)
        tab[at] = val
        assert _run(l, s, b) == EINVAL, (at, val)
    # totals past 2^31 - 1: refused by size, before the table is looked at
    for field, val in (("n_nodes", 1 << 30), ("n_elem", 1 << 31), ("n_rois", (1 << 31) // 81 + 1), ("n_scenes", 1 << 26),
                       ("n_scenes", 1 << 40)):
        s, b, tab = _job(mod)
        setattr(b, field, val)
        assert _run(l, s, b) == ESHAPE, field
    # alignment: 16 bytes for the float rows and tab_dev, 8 for ctrs / node_mask / idx of the batch and tab_host, 4 for the
    # resident int32 arrays, 2 for has_preds
    for obj, field, val in (("s", "feats", 264), ("s", "agent_feat", 264), ("s", "actor_feats", 264), ("s", "obs", 264),
                            ("s", "gt_preds", 264), ("s", "ctrs", 260), ("s", "node_mask", 258), ("s", "edge_u", 258),
                            ("s", "edge_v", 258), ("s", "a2m_u", 258), ("s", "a2m_v", 258), ("s", "has_preds", 257),
                            ("b", "tab_dev", 264), ("b", "feats", 264), ("b", "agent_feat", 264), ("b", "actor_feats", 264),
                            ("b", "obs", 264), ("b", "gt_preds", 264), ("b", "ctrs", 260), ("b", "node_mask", 260),
                            ("b", "idx", 260), ("b", "has_preds", 257)):
        s, b, tab = _job(mod)
        setattr(s if obj == "s" else b, field, val)
        assert _run(l, s, b) == EALIGN, field
    s, b, tab = _job(mod)
    b.tab_host = tab.ctypes.data + 4
    assert _run(l, s, b) == EALIGN


def test_public_interface_refuses_to_run_without_a_gpu(tmp_path):
    import lanegcn_amd  # noqa: F401
    from lanegcn_amd import data_lrcnn as D
    from lanegcn_amd import lanercnn as R
    from lanegcn_amd import ops
    from lanegcn_amd._lib import LgcnError
    for name in ("from_inputs", "from_store", "concat", "load", "save", "plan", "batch", "usable"):
        assert callable(getattr(D.RoiStore, name)), name
    assert callable(R.Net.forward_store) and callable(ops.roi_store_gather)
    assert ops.roi_store_table_elems(32) == 64 * 32 + 3
    with pytest.raises(LgcnError):
        ops.roi_store_table_elems(-1)
    if torch.cuda.is_available():
        return          # with a GPU the calls run: tests/test_gpu_roi_store.py
    with pytest.raises(LgcnError, match="needs a GPU"):
        D.RoiStore.from_inputs({}, np.zeros(7, np.int32))
    with pytest.raises(LgcnError, match="needs a GPU"):
        D.RoiStore.load(str(tmp_path / "none.npz"))
    with pytest.raises(LgcnError):                                      # the wrapper takes device tensors only
        ops.RoiStoreJob({k: torch.zeros(0) for k in ops.RoiStoreJob.FLOATS + ops.RoiStoreJob.INTS}, 0)
