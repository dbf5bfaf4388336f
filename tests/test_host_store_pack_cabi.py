"""CPU: lgcn_store_pack is exported, bound and declared, sizes its table, refuses every bad argument before anything is
launched (the calls below hand it placeholder device addresses: an accepted job would fault, a refused one launches
nothing), and n_seg == 0 returns without a launch."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL, ESHAPE, EALIGN = -1, -2, -3
PTRS = ("tab_host", "tab_dev", "dst", "frame", "rot", "orig")


@pytest.fixture(scope="module")
def lib():
    import lanegcn_amd  # noqa: F401
    from lanegcn_amd import _lib
    return _lib.load(), _lib


def test_symbols_are_exported_bound_and_declared(lib):
    l, mod = lib
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "lgcn.h")).read(), flags=re.S)
    for n in ("lgcn_store_pack_table_elems", "lgcn_store_pack"):
        assert hasattr(l, n) and n in mod.SIGNATURES and re.search(r"\b%s\s*\(" % n, header), n
    assert "lgcn_store_pack_t" in header
    assert C.sizeof(mod.StorePack) == 4 * 8 + 6 * 8 and mod.StorePack.tab_host.offset == 32
    assert [n for n, _ in mod.StorePack._fields_[4:]] == list(PTRS)


def test_table_size_helper(lib):
    l, _ = lib
    te = l.lgcn_store_pack_table_elems
    assert te(0, 0) == 1 and te(-1, 3) == EINVAL and te(3, -1) == EINVAL
    assert te(28, 28) == 3 * 28 + 1 + 3 * 28 and te(1792, 128) == 3 * 1792 + 1 + 3 * 128
    assert te(29, 28) > te(28, 28) and te(28, 29) > te(28, 28)
    assert te(1 << 40, 2) == ESHAPE and te(2, 1 << 40) == ESHAPE and te(1 << 29, 4) == ESHAPE


def _job(mod, n_scenes=2):
    """Four runs (3, 0, 5 and 2 words) out of three sources: int64 [8], int16 [5], int32 [2]; placeholder addresses."""
    seg_len, seg_src, seg_at = [3, 0, 5, 2], [0, 2, 1, 2], [5, 2, 0, 0]
    tab = np.concatenate([[0], np.cumsum(seg_len), seg_src, seg_at, [4096, 4098, 4100], [8, 2, 4], [8, 5, 2]]).astype(np.int64)
    p = mod.StorePack()
    p.n_seg, p.n_src, p.n_dst, p.n_scenes = 4, 3, 10, n_scenes
    p.tab_host = tab.ctypes.data
    p.tab_dev, p.dst, p.frame, p.rot, p.orig = 256, 260, 264, 272, 264
    return p, tab


def _run(l, p):
    return l.lgcn_store_pack(C.byref(p), None)


OFF, SRC, AT, PTR, KIND, LEN = 0, 5, 9, 13, 16, 19          # where the table's parts begin for G = 4, K = 3


def test_bad_arguments_are_refused_before_any_launch(lib):
    l, mod = lib
    p, tab = _job(mod)
    assert tab.size == l.lgcn_store_pack_table_elems(4, 3)
    assert l.lgcn_store_pack(None, None) == EINVAL
    for field in ("n_seg", "n_src", "n_dst", "n_scenes"):
        p, tab = _job(mod)
        setattr(p, field, -1)
        assert _run(l, p) == EINVAL, field
    # a null pointer next to a non-zero size
    for field in PTRS:
        p, tab = _job(mod)
        setattr(p, field, None)
        assert _run(l, p) == EINVAL, field
    p, tab = _job(mod)
    tab[PTR + 1] = 0
    assert _run(l, p) == EINVAL                                        # a source of 5 elements at address 0
    # misaligned: the device table and rot to 16, the host table, frame and orig to 8, dst to 4, a source to its element
    for field, val in (("tab_dev", 264), ("rot", 264), ("frame", 260), ("orig", 260), ("dst", 258)):
        p, tab = _job(mod)
        setattr(p, field, val)
        assert _run(l, p) == EALIGN, field
    p, tab = _job(mod)
    odd = np.zeros(tab.size + 1, np.int64)
    view = odd.view(np.uint8)[4:4 + 8 * tab.size].view(np.int64)      # the same table, 4 bytes off an int64 boundary
    view[:] = tab
    p.tab_host = view.ctypes.data
    assert p.tab_host % 8 == 4 and _run(l, p) == EALIGN
    for src, addr in ((0, 4100), (1, 4097), (2, 4098)):
        p, tab = _job(mod)
        tab[PTR + src] = addr
        assert _run(l, p) == EALIGN, src
    # the run table: not from 0, decreasing, an end that is not the destination size
    for at, val in ((OFF, 1), (OFF + 2, 2), (OFF + 3, 1 << 20), (OFF + 4, 11), (OFF + 4, 9), (OFF + 1, -1), (OFF + 2, -(1 << 63)),
                    (OFF + 3, (1 << 63) - 1)):
        p, tab = _job(mod)
        tab[at] = val
        assert _run(l, p) == EINVAL, (at, val)
    p, tab = _job(mod)
    p.n_dst = 11
    assert _run(l, p) == EINVAL
    # a run past its source: begins before it, begins past it, ends past it; a source index out of range
    for at, val in ((AT, -1), (AT, 9), (AT, 6), (AT + 2, 1), (AT + 3, 1), (AT + 1, 3), (SRC, -1), (SRC, 3), (SRC + 1, 1 << 40),
                    (LEN, 7), (LEN + 1, 4), (LEN + 2, -1)):
        p, tab = _job(mod)
        tab[at] = val
        assert _run(l, p) == EINVAL, (at, val)
    # an element size that is none of 2, 4, 8
    for val in (0, 1, 3, 16, -2):
        p, tab = _job(mod)
        tab[KIND] = val
        assert _run(l, p) == EINVAL, val
    # sizes beyond 2^31 - 1, refused by size before the table is looked at
    for field, val in (("n_dst", 1 << 31), ("n_scenes", 1 << 31), ("n_seg", 1 << 40), ("n_src", 1 << 40)):
        p, tab = _job(mod)
        setattr(p, field, val)
        assert _run(l, p) == ESHAPE, field
    p, tab = _job(mod)
    tab[LEN] = 1 << 31
    assert _run(l, p) == ESHAPE


def test_no_run_means_no_launch(lib):
    l, mod = lib
    assert _run(l, mod.StorePack()) == 0                                # nothing to do; no pointer is looked at
    p = mod.StorePack()
    p.n_src = 3
    assert _run(l, p) == 0
    for field in ("n_dst", "n_scenes"):                                 # words or frame rows without a run to carry them
        p = mod.StorePack()
        setattr(p, field, 1)
        assert _run(l, p) == EINVAL, field


def test_wrapper_refuses_without_a_gpu():
    import lanegcn_amd  # noqa: F401
    from lanegcn_amd import data_raw, lanegcn as M, ops
    from lanegcn_amd._lib import LgcnError
    from lanegcn_amd.flatfile import DeviceSceneStore
    assert callable(data_raw.build_store) and callable(M.Net.forward_raw) and callable(DeviceSceneStore.from_arrays)
    assert callable(DeviceSceneStore.concat) and callable(DeviceSceneStore.save)
    assert ops.store_pack_table_elems(28, 28) == 169
    with pytest.raises(LgcnError):
        ops.store_pack_table_elems(-1, 1)
    with pytest.raises(LgcnError):                                      # the wrapper takes device tensors only
        ops.store_pack([torch.zeros(4, dtype=torch.int64)], [0], [0], [4], torch.zeros(4, dtype=torch.int32))
    if not torch.cuda.is_available():
        with pytest.raises(LgcnError):
            data_raw.build_store([{"city": "A", "trajs": [np.zeros((20, 2))], "steps": [np.arange(20)]}], {}, M.config)
