"""CPU: the node-side head launch (lgcn_node_head) is exported and bound, the entry refuses every problem but the three
forms it implements and missing or misaligned pointers before launching anything, empty problems return LGCN_OK without a
launch, and the kernels keep their resource budget (no GPU needed)."""
import ctypes as C

import pytest

EINVAL, ESHAPE, EALIGN = -1, -2, -3
CHAIN = ("ch_wq", "ch_gq_g", "ch_gq_b", "ch_wu", "ch_u_out")
FORMS = ("head", "head+chain", "head+w4", "u-chain", "plain")


@pytest.fixture(scope="module")
def lib():
    import lanegcn_amd  # noqa: F401
    from lanegcn_amd import _lib
    return _lib.load(), _lib


def required(form):
    """The pointer fields of lgcn_agg_mlp_t a form needs (rel[0].src / wp come on top)."""
    if form == "plain":
        return ("out",)
    if form == "u-chain":
        return ("gn1_g", "gn1_b", "wp2", "out")
    return ("gn1_g", "gn1_b", "out") + (CHAIN if form == "head+chain" else ()) + (("w4",) if form == "head+w4" else ())


def problem(mod, form, mode="f16x2", **over):
    """A problem of one form with dummy, 16-byte aligned addresses (nothing is launched in these tests)."""
    p = mod.AggMlp()
    p.n_rows, p.n_rel, p.eps, p.mma = 96, 1, 1e-5, mod.MMA_NAMES[mode]
    p.flags = {"plain": 0, "u-chain": mod.F_GN1 | mod.F_RELU1 | mod.F_GEMM2}.get(form, mod.F_GN1 | mod.F_RELU1)
    p.rel[0].src, p.rel[0].wp, p.rel[0].mode = 256, 256, mod.REL_IDENT
    for k in required(form) + (("x4_a", "x4_b", "x4_c") if form == "head+w4" else ()):
        setattr(p, k, 256)
    for k, v in over.items():
        setattr(p, k, v)
    return p


def call(l, mod, ps, n=None):
    arr = (C.POINTER(mod.AggMlp) * max(len(ps), 1))(*[C.pointer(p) for p in ps])
    return l.lgcn_node_head(arr, len(ps) if n is None else n, None)


def test_symbol_is_exported_and_bound(lib):
    l, mod = lib
    assert hasattr(l, "lgcn_node_head"), "liblgcn.so does not export lgcn_node_head"
    assert "lgcn_node_head" in mod.SIGNATURES
    from lanegcn_amd import ops
    assert callable(ops.node_head) and callable(ops.node_head_ok)


def test_wrapper_follows_the_mode():
    import lanegcn_amd  # noqa: F401
    from lanegcn_amd import ops
    prev = ops.get_mma()
    try:
        for mode, ok in (("f16x2", True), ("bf16", True), ("bf16x3", False), ("f32", False)):
            ops.set_mma(mode)
            assert ops.node_head_ok() is ok, mode
    finally:
        ops.set_mma(prev)


@pytest.mark.parametrize("mode", ["f16x2", "bf16"])
def test_the_list_is_validated_first(lib, mode):
    l, mod = lib
    mk = lambda form="plain", **over: problem(mod, form, mode, **over)
    assert l.lgcn_node_head(None, 1, None) == EINVAL
    for n in (0, 5, -1):
        assert call(l, mod, [mk() for _ in range(4)], n=n) == EINVAL, n
    arr = (C.POINTER(mod.AggMlp) * 2)(C.pointer(mk()), None)
    assert l.lgcn_node_head(arr, 2, None) == EINVAL
    # the matrix mode is looked at before anything in the problems, empty ones included
    for bad in ("bf16x3", "f32"):
        assert call(l, mod, [mk(mma=mod.MMA_NAMES[bad])]) == ESHAPE, bad
        assert call(l, mod, [mk(mma=mod.MMA_NAMES[bad], n_rows=0)]) == ESHAPE, bad
        assert call(l, mod, [mk(mma=mod.MMA_NAMES[bad], n_rows=-1)]) == ESHAPE, bad
        assert call(l, mod, [mk(), mk(mma=mod.MMA_NAMES[bad])]) == ESHAPE, bad
    assert call(l, mod, [mk(mma=17)]) == ESHAPE
    other = "bf16" if mode == "f16x2" else "f16x2"
    assert call(l, mod, [mk(), mk(mma=mod.MMA_NAMES[other])]) == ESHAPE


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("mode", ["f16x2", "bf16"])
def test_entry_validates_before_launching(lib, mode, form):
    l, mod = lib
    mk = lambda **over: problem(mod, form, mode, **over)
    one = lambda **over: call(l, mod, [mk(**over)])
    # a form, or nothing
    full = mk().flags
    for flags in (full | mod.F_GN2, full | mod.F_RES, full | mod.F_RELU2, mod.F_GN1, mod.F_RELU1, mod.F_GEMM2):
        assert one(flags=flags) == ESHAPE, flags
    assert one(n_rel=2) == ESHAPE and one(n_rel=0) == ESHAPE
    for m in (mod.REL_RANGE, mod.REL_RANGE16, mod.REL_CSR):
        p = mk()
        p.rel[0].mode = m
        assert call(l, mod, [p]) == ESHAPE, m
    for k in ("ch_wv", "ch_v_out", "out_pre", "out_mid", "out_pre2"):
        assert one(**{k: 256}) == ESHAPE, k
    assert one(tile_rb=3) == ESHAPE
    if not form.startswith("head"):
        assert one(w4=256) == ESHAPE and one(ch_wu=256) == ESHAPE
    # the shape comes before the row count, the row count before the pointers
    assert one(n_rel=2, n_rows=-1) == ESHAPE
    assert one(n_rows=-1) == EINVAL and one(n_rows=-1, out=None) == EINVAL
    assert one(n_rows=0x80000000) == ESHAPE and one(n_rows=1 << 40) == ESHAPE
    # nothing to do: no launch, the pointers are not looked at
    assert one(n_rows=0) == 0 and one(n_rows=0, out=None, gn1_g=None) == 0
    assert call(l, mod, [mk(n_rows=0), mk(n_rows=0, out=260)]) == 0
    # an empty problem beside a faulty one does not hide it
    assert call(l, mod, [mk(n_rows=0), mk(out=None)]) == EINVAL
    for k in required(form):
        if k == "ch_wu" or k == "w4":      # the switches of the chained output and of the rank-4 update themselves
            assert one(**{k: 260}) == EALIGN, k
            continue
        assert one(**{k: None}) == EINVAL, k
        assert one(**{k: 260}) == EALIGN, k
    if form == "head+w4":
        for k in ("x4_a", "x4_b", "x4_c"):
            assert one(**{k: None}) == EINVAL, k
    for f in ("src", "wp"):
        p = mk()
        setattr(p.rel[0], f, None)
        assert call(l, mod, [p]) == EINVAL, f
        p = mk()
        setattr(p.rel[0], f, 264)
        assert call(l, mod, [p]) == EALIGN, f
    # a missing pointer comes before a misaligned one, across the problems of a list too
    assert one(out=None, wp2=260) == EINVAL
    p = mk()
    p.rel[0].src = 264
    assert call(l, mod, [p, mk(out=None)]) == EINVAL


def test_kernel_resources():
    """The kernels' budget: at most 128 VGPRs, no scratch, and no more LDS than the node tail's kernel of the same format
    (two workgroups, or another forward's kernel, share the CU)."""
    import os
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path.insert(0, os.path.join(root, "tools"))
    from kernel_resources import kernels
    found = kernels(os.path.join(root, "lanegcn-1_amd", "liblgcn.so"))
    for tag in ("ILi1E", "ILi2E"):      # f16x2, bf16
        head = [k for k in found if "k_node_head" + tag in k["name"]]
        tail = [k for k in found if "k_node_tail" + tag in k["name"]]
        assert len(head) == 1 and len(tail) == 1, [k["name"] for k in head + tail]
        k = head[0]
        assert k["vgprs"] <= 128 and k["scratch"] == 0 and k["spills"] == 0 and k["lds"] <= tail[0]["lds"] <= 80 * 1024, k
