"""CPU: the batched graph-construction entries (lgcn_dilate_batch_*, lgcn_cross_edges_batch, csrc/lgcn_graphbatch.hip)
refuse bad arguments before launching anything, and the Python wrappers refuse CPU tensors.  Nothing here launches: every
call fails its validation (device pointers are made-up addresses)."""
import ctypes as C

import numpy as np
import pytest
import torch

OK, EINVAL, ESHAPE, EALIGN = 0, -1, -2, -3


@pytest.fixture(scope="module")
def lib():
    import lanegcn_amd  # noqa: F401
    from lanegcn_amd import _lib
    return _lib.load(), _lib


def fake(k):
    return 0x7f0000100000 + 0x1000 * k      # 16-byte aligned, never dereferenced


DIL_OFF = ([0, 3, 3, 8], [0, 2, 2, 6], [0, 1, 1, 4])      # node, pre, suc offsets of 3 scenes, the middle one empty
DIL_PTRS = ("off_dev", "pre_u", "pre_v", "suc_u", "suc_v", "ws", "rowptr", "col", "out_rowptr", "bounds", "out_col", "out_u", "out_v")


def dilate(mod, off=DIL_OFF):
    p = mod.DilateBatch()
    p._off = np.ascontiguousarray(np.asarray(off, np.int32))
    p.n_scenes, p.n_nodes, p.n_pre, p.n_suc, p.nnz = 3, 8, 6, 4, 5
    p.off_host = p._off.ctypes.data
    for k, name in enumerate(DIL_PTRS):
        setattr(p, name, fake(k))
    return p


def test_dilate_refusals(lib):
    l, mod = lib
    entries = (l.lgcn_dilate_batch_csr, l.lgcn_dilate_batch_count, l.lgcn_dilate_batch_fill)
    calls = [lambda p, _f=f: _f(C.byref(p), None) for f in entries]
    needs = [("off_host", "off_dev", "ws", "rowptr", "col", "pre_u", "pre_v", "suc_u", "suc_v"),
             ("off_host", "off_dev", "ws", "rowptr", "col", "out_rowptr", "bounds"),
             ("off_host", "off_dev", "ws", "rowptr", "col", "out_rowptr", "bounds", "out_col", "out_u", "out_v")]
    for entry, call, need in zip(entries, calls, needs):
        assert entry(None, None) == EINVAL
        # the base passes every check in front of the last one: only the last pointer checked is misaligned
        p = dilate(mod); p.out_v = fake(40) + 4
        assert call(p) == EALIGN
        for name in ("n_scenes", "n_nodes", "n_pre", "n_suc"):
            p = dilate(mod); setattr(p, name, -1)
            assert call(p) == EINVAL, name
        for name in ("n_nodes", "n_pre", "n_suc"):
            p = dilate(mod); setattr(p, name, 1 << 32)
            assert call(p) == ESHAPE, name
        p = dilate(mod); p.n_scenes = 0x7fffffff
        assert call(p) == ESHAPE
        # a bad offset table never becomes an address: a start other than 0, a decrease, an end that is not the array size
        for off in (([1, 3, 3, 8], DIL_OFF[1], DIL_OFF[2]), ([0, 4, 3, 8], DIL_OFF[1], DIL_OFF[2]), ([0, 3, 3, 9], DIL_OFF[1], DIL_OFF[2]),
                    (DIL_OFF[0], [0, 3, 2, 6], DIL_OFF[2]), (DIL_OFF[0], [0, 2, 2, 5], DIL_OFF[2]), (DIL_OFF[0], [-1, 2, 2, 6], DIL_OFF[2]),
                    (DIL_OFF[0], DIL_OFF[1], [0, 1, 0, 4]), (DIL_OFF[0], DIL_OFF[1], [0, 1, 1, 3])):
            assert call(dilate(mod, off)) == EINVAL, off
        for name in need:
            p = dilate(mod); setattr(p, name, None)
            assert call(p) == EINVAL, name
        for name, by in (("ws", 8), ("off_dev", 2), ("rowptr", 1), ("col", 2), ("out_rowptr", 2), ("bounds", 2), ("out_col", 2),
                         ("pre_u", 4), ("pre_v", 4), ("suc_u", 4), ("suc_v", 4), ("out_u", 4)):
            p = dilate(mod); setattr(p, name, getattr(p, name) + by)
            assert call(p) == EALIGN, name
        p = mod.DilateBatch()
        assert call(p) == OK                                           # an empty batch: nothing to launch
        p.n_pre = 1
        assert call(p) == EINVAL
    fill = calls[2]
    p = dilate(mod); p.nnz = -1
    assert fill(p) == EINVAL
    p = dilate(mod); p.nnz = 1 << 31
    assert fill(p) == ESHAPE
    assert l.lgcn_dilate_batch_ws_elems(-1, 0) == EINVAL and l.lgcn_dilate_batch_ws_elems(0, -1) == EINVAL
    assert l.lgcn_dilate_batch_ws_elems(1 << 31, 0) == ESHAPE and l.lgcn_dilate_batch_ws_elems(0, 1 << 31) == ESHAPE
    assert 0 < l.lgcn_dilate_batch_ws_elems(1, 0) < l.lgcn_dilate_batch_ws_elems(915, 2000) < l.lgcn_dilate_batch_ws_elems(60000, 130000)


# node, lane, pre, suc, left, right offsets of 2 scenes (3 and 2 lanes), then what they imply: lanes^2, side * (pre + suc + 1)
CROSS_OFF = ([0, 5, 9], [0, 3, 5], [0, 2, 3], [0, 1, 3], [0, 2, 2], [0, 1, 3], [0, 9, 13], [0, 8, 8], [0, 4, 12])
CROSS_PTRS = ("off_dev", "ctrs", "feats", "lane_idcs", "pre_pairs", "suc_pairs", "left_pairs", "right_pairs", "mat", "ws", "counts",
              "out_u", "out_v")


def cross(mod, off=CROSS_OFF, totals=(9, 5, 3, 3, 2, 3)):
    p = mod.CrossBatch()
    p._off = np.ascontiguousarray(np.asarray(off, np.int32))
    p.n_scenes, p.cross_dist = p._off.shape[1] - 1, 6.0
    p.n_nodes, p.n_lanes, p.n_pre, p.n_suc, p.n_left, p.n_right = totals
    p.off_host = p._off.ctypes.data
    for k, name in enumerate(CROSS_PTRS):
        setattr(p, name, fake(k))
    return p


def change(row, value):
    off = [list(r) for r in CROSS_OFF]
    off[row] = value
    return off


def test_cross_refusals(lib):
    l, mod = lib
    call = lambda p: l.lgcn_cross_edges_batch(C.byref(p), None)
    assert l.lgcn_cross_edges_batch(None, None) == EINVAL
    p = cross(mod); p.out_v = fake(40) + 1                             # the last check
    assert call(p) == EALIGN
    for name in ("n_scenes", "n_nodes", "n_lanes", "n_pre", "n_suc", "n_left", "n_right"):
        p = cross(mod); setattr(p, name, -1)
        assert call(p) == EINVAL, name
    for name in ("n_nodes", "n_lanes", "n_pre", "n_suc", "n_left", "n_right"):
        p = cross(mod); setattr(p, name, 1 << 32)
        assert call(p) == ESHAPE, name
    p = cross(mod); p.cross_dist = float("nan")
    assert call(p) == EINVAL
    for off in (change(0, [1, 5, 9]), change(0, [0, 10, 9]), change(0, [0, 5, 8]), change(1, [0, 6, 5]), change(1, [0, 3, 4]),
                change(2, [0, 4, 3]), change(3, [-1, 1, 3]), change(4, [0, 2, 3]), change(5, [0, 4, 3]),
                change(6, [0, 9, 12]), change(6, [0, 8, 13]), change(7, [0, 8, 9]), change(7, [0, 6, 8]), change(8, [0, 5, 12]),
                change(8, [1, 4, 12])):
        assert call(cross(mod, off)) == EINVAL, off
    for name in ("off_host",) + CROSS_PTRS:
        p = cross(mod); setattr(p, name, None)
        assert call(p) == EINVAL, name
    for name, by in (("ws", 8), ("off_dev", 2), ("counts", 2), ("ctrs", 4), ("feats", 4), ("lane_idcs", 4), ("pre_pairs", 4),
                     ("suc_pairs", 4), ("left_pairs", 4), ("right_pairs", 4), ("out_u", 1)):
        p = cross(mod); setattr(p, name, getattr(p, name) + by)
        assert call(p) == EALIGN, name
    p = mod.CrossBatch()
    assert call(p) == OK                                               # an empty batch: nothing to launch
    p.n_lanes = 1
    assert call(p) == EINVAL
    assert l.lgcn_cross_edges_batch_ws_elems(-1) == EINVAL and l.lgcn_cross_edges_batch_ws_elems(1 << 31) == ESHAPE
    assert 0 < l.lgcn_cross_edges_batch_ws_elems(1) < l.lgcn_cross_edges_batch_ws_elems(60000)


def test_cross_mask_bytes_over_the_limit(lib):
    """Two masks of lanes^2 bytes per scene: 2 * 32,768^2 = 2^31 bytes are refused, 2 * 32,767^2 pass on to the last check."""
    l, mod = lib
    for lanes, want in ((32768, ESHAPE), (32767, EALIGN)):
        off = [[0, lanes], [0, lanes], [0, 0], [0, 0], [0, 0], [0, 0], [0, lanes * lanes], [0, 0], [0, 0]]
        p = cross(mod, off, (lanes, lanes, 0, 0, 0, 0)); p.out_v = fake(40) + 1
        assert l.lgcn_cross_edges_batch(C.byref(p), None) == want, lanes
    # many scenes: the sum counts, not the largest scene
    S, lanes = 64, 4096 + 1
    six = [np.arange(S + 1) * lanes] * 2 + [np.zeros(S + 1)] * 4
    off = np.stack(six + [np.arange(S + 1) * lanes * lanes, np.zeros(S + 1), np.zeros(S + 1)]).astype(np.int64)
    assert off.max() < 2 ** 31
    assert l.lgcn_cross_edges_batch(C.byref(cross(mod, off, (S * lanes, S * lanes, 0, 0, 0, 0))), None) == ESHAPE


def test_python_wrappers_refuse_cpu_tensors(lib):
    _, mod = lib
    from lanegcn_amd import ops, preprocess_data as P
    i64 = lambda *x: torch.tensor(x, dtype=torch.int64)
    off = np.array([0, 2])
    with pytest.raises(mod.LgcnError, match="CUDA tensor"):
        ops.dilate_batch(i64(1), i64(0), i64(0), i64(1), off, np.array([0, 1]), np.array([0, 1]), 3)
    with pytest.raises(mod.LgcnError, match="CUDA tensor"):
        ops.cross_edges_batch(torch.zeros(2, 2), torch.zeros(2, 2), i64(0, 0), i64(0, 0).reshape(1, 2), i64(0, 0).reshape(1, 2),
                              i64(0, 0).reshape(1, 2), i64(0, 0).reshape(1, 2), off, *[np.array([0, 1])] * 5, 6.0)
    with pytest.raises(mod.LgcnError, match="CUDA tensors"):
        P.dilated_nbrs_batch([{"u": i64(1), "v": i64(0)}], [2], 3)
    g = dict(ctrs=torch.zeros(2, 2), feats=torch.zeros(2, 2), lane_idcs=i64(0, 0), pre_pairs=i64(0, 0).reshape(1, 2),
             suc_pairs=i64(0, 0).reshape(1, 2), left_pairs=i64(0, 0).reshape(1, 2), right_pairs=i64(0, 0).reshape(1, 2), idx=0)
    with pytest.raises(mod.LgcnError, match="CUDA tensors"):
        P.preprocess_batch([g], 6.0)
    with pytest.raises(NameError):
        P.preprocess_batch([g], 6.0, cross_angle=0.5)
    # offset tables that do not fit the arrays are refused in Python, before the library sees them
    with pytest.raises(mod.LgcnError, match="do not end at the edge counts"):
        ops.dilate_batch(i64(1), i64(0), i64(0), i64(1), off, np.array([0, 2]), np.array([0, 1]), 3)
