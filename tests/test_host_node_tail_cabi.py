"""CPU: the node-side tail launch (lgcn_node_tail) is exported and bound, the entry refuses every shape but the one it
implements and missing or misaligned pointers before launching anything, an empty problem returns LGCN_OK without a
launch, and the kernels keep their resource budget (no GPU needed)."""
import ctypes as C

import pytest

EINVAL, ESHAPE, EALIGN = -1, -2, -3
PTRS = ("rowptr", "gn1_g", "gn1_b", "wp2", "gn2_g", "gn2_b", "res", "out")
CHAIN = ("ch_wq", "ch_gq_g", "ch_gq_b", "ch_wu", "ch_u_out")


@pytest.fixture(scope="module")
def lib():
    import lanegcn_amd  # noqa: F401
    from lanegcn_amd import _lib
    return _lib.load(), _lib


def problem(mod, mode="f16x2", chain=False, **over):
    """The tail's problem with dummy, 16-byte aligned addresses (nothing is launched in these tests)."""
    p = mod.AggMlp()
    p.n_rows, p.n_rel, p.eps, p.mma = 96, 2, 1e-5, mod.MMA_NAMES[mode]
    p.flags = mod.F_GN1 | mod.F_RELU1 | mod.F_GEMM2 | mod.F_GN2 | mod.F_RES | mod.F_RELU2
    p.rel[0].src, p.rel[0].wp, p.rel[0].mode = 256, 256, mod.REL_IDENT
    p.rel[1].src, p.rel[1].wp, p.rel[1].mode = 256, 256, mod.REL_RANGE
    for k in PTRS + (CHAIN if chain else ()):
        setattr(p, k, 256)
    for k, v in over.items():
        setattr(p, k, v)
    return p


def test_symbol_is_exported_and_bound(lib):
    l, mod = lib
    assert hasattr(l, "lgcn_node_tail"), "liblgcn.so does not export lgcn_node_tail"
    assert "lgcn_node_tail" in mod.SIGNATURES
    from lanegcn_amd import ops
    assert callable(ops.node_tail) and callable(ops.node_tail_ok)


def test_wrapper_follows_the_mode():
    import lanegcn_amd  # noqa: F401
    from lanegcn_amd import ops
    prev = ops.get_mma()
    try:
        for mode, ok in (("f16x2", True), ("bf16", True), ("bf16x3", False), ("f32", False)):
            ops.set_mma(mode)
            assert ops.node_tail_ok() is ok, mode
    finally:
        ops.set_mma(prev)


@pytest.mark.parametrize("chain", [False, True])
@pytest.mark.parametrize("mode", ["f16x2", "bf16"])
def test_entry_validates_before_launching(lib, mode, chain):
    l, mod = lib

    def call(**over):
        return l.lgcn_node_tail(C.byref(problem(mod, mode, chain, **over)), None)

    assert l.lgcn_node_tail(None, None) == EINVAL
    # the matrix mode is looked at first
    for bad in ("bf16x3", "f32"):
        assert call(mma=mod.MMA_NAMES[bad]) == ESHAPE and call(mma=mod.MMA_NAMES[bad], n_rows=0) == ESHAPE, bad
    assert call(mma=17) == ESHAPE
    # exactly the tail's shape
    full = problem(mod).flags
    for flags in (0, full & ~mod.F_RELU2, full & ~mod.F_RES, full & ~mod.F_GN1):
        assert call(flags=flags) == ESHAPE, flags
    assert call(n_rel=1) == ESHAPE and call(n_rel=3) == ESHAPE
    for r, m in ((0, mod.REL_RANGE), (1, mod.REL_IDENT), (1, mod.REL_RANGE16), (1, mod.REL_CSR)):
        p = problem(mod, mode, chain)
        p.rel[r].mode = m
        assert l.lgcn_node_tail(C.byref(p), None) == ESHAPE, (r, m)
    for k in ("ch_wv", "ch_v_out", "w4", "out_pre", "out_mid", "out_pre2"):
        assert call(**{k: 256}) == ESHAPE, k
    assert call(tile_rb=2) == ESHAPE
    assert call(n_rows=-1) == EINVAL
    assert call(n_rows=0x80000000) == ESHAPE and call(n_rows=1 << 40) == ESHAPE
    # nothing to do: no launch, the pointers are not looked at
    assert call(n_rows=0) == 0 and call(n_rows=0, out=None, res=None, rowptr=None) == 0
    for k in PTRS + (CHAIN if chain else ()):
        if k == "ch_wu":      # the switch of the chained output itself
            continue
        assert call(**{k: None}) == EINVAL, k
        if k != "rowptr":
            assert call(**{k: 260}) == EALIGN, k
    for r in (0, 1):
        for f in ("src", "wp"):
            p = problem(mod, mode, chain)
            setattr(p.rel[r], f, None)
            assert l.lgcn_node_tail(C.byref(p), None) == EINVAL, (r, f)
            p = problem(mod, mode, chain)
            setattr(p.rel[r], f, 264)
            assert l.lgcn_node_tail(C.byref(p), None) == EALIGN, (r, f)
    # a missing pointer comes before a misaligned one
    assert call(out=None, res=260) == EINVAL


def test_kernel_resources():
    """The kernels' budget: at most 128 VGPRs and at most half a CU's LDS (a second workgroup, or another forward's kernel,
    shares the CU), no scratch."""
    import os
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path.insert(0, os.path.join(root, "tools"))
    from kernel_resources import kernels
    ks = [k for k in kernels(os.path.join(root, "lanegcn-1_amd", "liblgcn.so")) if "k_node_tail" in k["name"]]
    assert len(ks) == 2, [k["name"] for k in ks]
    for k in ks:
        assert k["vgprs"] <= 128 and k["scratch"] == 0 and k["spills"] == 0 and k["lds"] <= 80 * 1024, k
