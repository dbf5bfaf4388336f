"""CPU: the context-heads launch (lgcn_ctx_heads) is exported and bound, and the entry refuses an unsupported matrix mode,
a negative or too large row count, a weight count out of range, missing and misaligned pointers before launching anything;
an empty problem returns LGCN_OK without a launch (no GPU needed)."""
import ctypes as C

import pytest

EINVAL, ESHAPE, EALIGN = -1, -2, -3


@pytest.fixture(scope="module")
def lib():
    import lanegcn_amd  # noqa: F401
    from lanegcn_amd import _lib
    return _lib.load(), _lib


def test_symbol_is_exported_and_bound(lib):
    l, mod = lib
    assert hasattr(l, "lgcn_ctx_heads"), "liblgcn.so does not export lgcn_ctx_heads"
    assert "lgcn_ctx_heads" in mod.SIGNATURES
    from lanegcn_amd import ops
    assert callable(ops.ctx_heads) and callable(ops.ctx_heads_ok)


def test_wrapper_follows_the_mode():
    import lanegcn_amd  # noqa: F401
    from lanegcn_amd import ops
    prev = ops.get_mma()
    try:
        for mode, ok in (("f16x2", True), ("bf16", True), ("bf16x3", False), ("f32", False)):
            ops.set_mma(mode)
            assert ops.ctx_heads_ok() is ok, mode
    finally:
        ops.set_mma(prev)


@pytest.mark.parametrize("n_w", [1, 2])
@pytest.mark.parametrize("mode", ["f16x2", "bf16"])
def test_entry_validates_before_launching(lib, mode, n_w):
    l, mod = lib
    mma = mod.MMA_NAMES[mode]

    def call(x=256, n_rows=96, w=(256, 256), out=(256, 256), n=n_w, m=mma, w_arr=True, out_arr=True):
        wa = (C.c_void_p * 2)(*w) if w_arr else None
        oa = (C.c_void_p * 2)(*out) if out_arr else None
        return l.lgcn_ctx_heads(x, n_rows, wa, n, m, oa, None)

    # the matrix mode is looked at first, as lgcn_laneconv_fwd does
    for bad in ("bf16x3", "f32"):
        assert call(m=mod.MMA_NAMES[bad]) == ESHAPE, bad
        assert call(m=mod.MMA_NAMES[bad], n_rows=0) == ESHAPE and call(m=mod.MMA_NAMES[bad], x=None) == ESHAPE, bad
    assert call(m=17) == ESHAPE and call(m=-1) == ESHAPE
    assert call(n_rows=-1) == EINVAL
    assert call(n_rows=0x80000000) == ESHAPE and call(n_rows=1 << 40) == ESHAPE
    assert call(n=0) == EINVAL and call(n=3) == EINVAL and call(n=-1) == EINVAL
    assert call(w_arr=False) == EINVAL and call(out_arr=False) == EINVAL
    # nothing to do: no launch, the row pointers are not looked at
    assert call(n_rows=0) == 0 and call(n_rows=0, x=None, w=(None, None), out=(None, None)) == 0
    assert call(n_rows=0, n=3) == EINVAL and call(n_rows=0, w_arr=False) == EINVAL
    assert call(x=None) == EINVAL
    for j in range(n_w):
        ptrs = [256, 256]
        ptrs[j] = None
        assert call(w=tuple(ptrs)) == EINVAL and call(out=tuple(ptrs)) == EINVAL, j
    # a missing pointer comes before a misaligned one
    assert call(x=None, w=(260, 256)) == EINVAL and call(x=260, out=(None, None)) == EINVAL
    assert call(x=260) == EALIGN and call(x=264) == EALIGN
    for j in range(n_w):
        ptrs = [256, 256]
        ptrs[j] = 260
        assert call(w=tuple(ptrs)) == EALIGN and call(out=tuple(ptrs)) == EALIGN, j
    if n_w == 1:      # the unused second slot is not looked at
        assert call(n_rows=0, w=(256, 260), out=(256, None)) == 0


def test_kernel_resources():
    """The kernel's budget: at most 128 VGPRs (a second workgroup, or another forward's kernel, shares the CU), no scratch,
    about 26 KB of LDS in the two-plane mode."""
    import os
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path.insert(0, os.path.join(root, "tools"))
    from kernel_resources import kernels
    ks = [k for k in kernels(os.path.join(root, "lanegcn-1_amd", "liblgcn.so")) if "k_ctx_heads" in k["name"]]
    assert len(ks) == 2, [k["name"] for k in ks]
    for k in ks:
        assert k["vgprs"] <= 128 and k["scratch"] == 0 and k["spills"] == 0 and k["lds"] <= 27 * 1024, k
