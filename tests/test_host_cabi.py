"""CPU: the C-ABI library loads, exports every symbol include/lgcn.h declares, and rejects bad
arguments before launching anything (no compute calls: there is no GPU in the build container)."""
import ctypes as C
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lib():
    import lanegcn_amd  # noqa: F401
    from lanegcn_amd import _lib
    return _lib.load(), _lib


def header_symbols():
    text = open(os.path.join(ROOT, "include", "lgcn.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(lgcn_[a-z0-9_]+)\s*\(", text)))


def test_every_declared_symbol_is_exported_and_bound(lib):
    l, mod = lib
    names = header_symbols()
    assert len(names) >= 12
    for n in names:
        assert hasattr(l, n), "liblgcn.so does not export " + n
    assert sorted(mod.SIGNATURES) == names, "ctypes binding and header disagree"


def test_version_and_strerror(lib):
    l, _ = lib
    assert l.lgcn_version() == 100
    assert l.lgcn_strerror(0) == b"ok"
    assert b"invalid" in l.lgcn_strerror(-1)


def test_struct_layout_matches_header(lib):
    _, mod = lib
    # lgcn_rel_t: 2 pointers + 2 int32; lgcn_agg_mlp_t: 32-byte head, 16 rels, 16 + 7 pointers (the library
    # static_asserts the same number: csrc/lgcn_rowmlp.hpp)
    assert C.sizeof(mod.Rel) == 24
    assert mod.AggMlp.rel.offset == 32
    assert C.sizeof(mod.AggMlp) == 32 + 16 * 24 + 23 * 8
    assert mod.AggMlp.ch_wq.offset == 32 + 16 * 24 + 16 * 8


def test_no_shipped_kernel_uses_scratch():
    """Every kernel of liblgcn.so keeps its working set in registers: private segment (scratch) 0 bytes, no spilled
    VGPR -- read from the code objects embedded in the library (tools/kernel_resources.py).  Register spills were the one
    thing common to every kernel that produced the unexplained wrong rows of rounds 2 / 3."""
    import sys
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    from kernel_resources import kernels
    ks = kernels(os.path.join(ROOT, "lanegcn-1_amd", "liblgcn.so"))
    assert len(ks) >= 100 and all(k["arch"] == "gfx950" for k in ks)
    bad = [(k["name"], k["scratch"], k["spills"]) for k in ks if k["scratch"] or k["spills"]]
    assert not bad, bad


def test_no_shipped_kernel_holds_the_miscomputed_packed_form():
    """MI355X returns wrong low halves in lanes 48-63 for a packed fp32 instruction whose low result lane reads the high
    half of its second source (op_sel[1] = 1: v_pk_mul_f32 / v_pk_add_f32 d, a, b op_sel:[0,1] ...) while other waves of
    the CU issue MFMA / LDS instructions (tools/micro/pk_opsel.hip; the cause of the wrong rows of rounds 2 / 3,
    DESIGN.md section 3.1).  The library is built without the SLP vectoriser that emits it; this disassembles the shipped
    code objects and checks."""
    import sys
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import kernel_resources as kr
    if not os.path.exists(kr.OBJDUMP):
        pytest.skip("llvm-objdump not found")
    # the line classifier on the forms tools/micro/pk_opsel.hip measured (llvm-objdump's layout, with and without its comment)
    bad = ["\tv_pk_mul_f32 v[22:23], v[20:21], v[50:51] op_sel:[0,1] op_sel_hi:[1,0]// 000000004368: D3B1 0816",
           "  v_pk_add_f32 v[74:75], v[74:75], v[78:79] op_sel:[0,1] op_sel_hi:[1,0]",
           "\tv_pk_mul_f32 v[0:1], v[2:3], v[4:5] op_sel:[0,1]",
           "\tv_pk_fma_f32 v[0:1], v[2:3], v[4:5], v[6:7] op_sel:[0,1,0] op_sel_hi:[1,0,1]"]
    good = ["\tv_pk_add_f32 v[124:125], v[120:121], v[120:121] op_sel:[0,1] op_sel_hi:[1,0]",      # one pair's horizontal add
            "\tv_pk_mul_f32 v[0:1], v[2:3], v[4:5] op_sel_hi:[1,0]", "\tv_pk_mul_f32 v[0:1], v[2:3], v[4:5]",
            "\tv_pk_mul_f32 v[0:1], v[2:3], v[4:5] op_sel:[1,0] op_sel_hi:[0,1]",
            "\tv_pk_fma_f32 v[0:1], v[2:3], v[4:5], v[6:7] op_sel:[1,0,0]", "\tv_pk_mov_b32 v[0:1], v[2:3], v[4:5] op_sel:[1,0]",
            "\tv_mfma_f32_16x16x32_f16 v[0:3], v[4:7], v[8:11], v[0:3]"]
    assert all(kr._risky_line(l) for l in bad) and not any(kr._risky_line(l) for l in good)
    found = kr.risky_packed(os.path.join(ROOT, "lanegcn-1_amd", "liblgcn.so"))
    assert not found, found[:5]
    # the detector itself: the compare + select diagnostic build (SLP on) is where the form was first seen
    diag = os.path.join(ROOT, "lanegcn-1_amd", "liblgcn_relucnd.so")
    if os.path.exists(diag):
        assert kr.risky_packed(diag), "detector finds nothing in the build that is known to hold the form"


def test_size_helpers(lib):
    l, _ = lib
    assert l.lgcn_csr_rowptr_elems(10368, 14) == 648 * 14 * 16 + 1
    assert l.lgcn_csr_rowptr_elems(33, 14) == 3 * 14 * 16 + 1
    assert l.lgcn_packed_bytes(128, 0) == 65536 and l.lgcn_packed_bytes(136, 0) == 128 * 136 * 4
    assert l.lgcn_packed_bytes(128, 1) == 3 * 32768 and l.lgcn_packed_bytes(128, 2) == 32768
    assert l.lgcn_packed_bytes(128, 3) == 2 * 32768
    assert l.lgcn_packed_bytes(136, 1) < 0 and l.lgcn_packed_bytes(128, 9) < 0
    assert l.lgcn_csr_rowptr_elems(10, 17) < 0
    assert l.lgcn_csr_ws_elems(10368, 14) > l.lgcn_csr_rowptr_elems(10368, 14)
    assert l.lgcn_pairs_ws_elems(1600, 32) == 1601 + 2 * 32 + 1 and l.lgcn_pairs_ws_elems(-1, 2) < 0


def test_bad_arguments_are_refused_without_launching(lib):
    l, mod = lib
    EINVAL, EALIGN = -1, -3
    assert l.lgcn_graph_gather(None, 5, None, None, 1, None, None, None) == EINVAL
    assert l.lgcn_graph_gather(None, 0, None, None, 0, None, None, None) == 0          # empty: nothing to do
    assert l.lgcn_graph_gather(None, -1, None, None, 0, None, None, None) == EINVAL
    assert l.lgcn_pack_weight(None, 128, 128, 128, 0, None, None) == EINVAL
    assert l.lgcn_pack_weight(C.c_void_p(64), 128, 128, 130, 0, C.c_void_p(64), None) == EINVAL   # k_pad % 8
    assert l.lgcn_pack_weight(C.c_void_p(64), 128, 128, 128, 0, C.c_void_p(68), None) == EALIGN
    assert l.lgcn_pack_weight(C.c_void_p(64), 128, 128, 128, 5, C.c_void_p(64), None) == EINVAL   # unknown mma
    assert l.lgcn_pack_weight(C.c_void_p(64), 136, 132, 136, 1, C.c_void_p(64), None) == -2       # bf16 modes: K = 128 only
    p = mod.AggMlp()
    assert l.lgcn_agg_mlp(None, None) == EINVAL
    p.n_rows, p.n_rel = 10, 0
    assert l.lgcn_agg_mlp(C.byref(p), None) == EINVAL
    p.n_rel = 17
    assert l.lgcn_agg_mlp(C.byref(p), None) == EINVAL
    p.n_rows, p.n_rel = 0, 1
    assert l.lgcn_agg_mlp(C.byref(p), None) == 0                                         # no rows: no launch
    p.n_rows = 10
    assert l.lgcn_agg_mlp(C.byref(p), None) == EINVAL                                    # null out / src
    p.out = 256
    p.rel[0].src, p.rel[0].wp, p.rel[0].mode = 256, 256, 7
    assert l.lgcn_agg_mlp(C.byref(p), None) == EINVAL                                    # unknown mode
    p.rel[0].mode = mod.REL_CSR
    assert l.lgcn_agg_mlp(C.byref(p), None) == EINVAL                                    # ridx >= n_rel_csr
    p.rel[0].mode, p.flags = mod.REL_IDENT, mod.F_GN2
    assert l.lgcn_agg_mlp(C.byref(p), None) == EINVAL                                    # GN2 without GEMM2
    p.flags = 0
    p.rel[0].src = 260
    assert l.lgcn_agg_mlp(C.byref(p), None) == EALIGN
    assert l.lgcn_pairs_build(None, None, None, None, 0, 0, 0, 1.0, 1, None, None, 0, None, None, None, None) == EINVAL
    assert l.lgcn_att_pairs(*([None] * 5), -1, *([None] * 10), 1e-5, 0, None, None) == EINVAL
    assert l.lgcn_att_pairs(*([None] * 5), 0, *([None] * 10), 1e-5, 0, None, None) == 0
    assert l.lgcn_att_pairs(*([None] * 5), 0, *([None] * 10), 1e-5, 9, None, None) == EINVAL
    assert l.lgcn_mapnet_input(None, None, 5, *([None] * 10), 1e-5, 1, None, None) == EINVAL
    # one rowptr per launch: CSR and RANGE relations cannot be mixed
    q = mod.AggMlp()
    q.n_rows, q.n_rel, q.n_rel_csr, q.out, q.rowptr, q.col = 10, 2, 1, 256, 256, 256
    q.rel[0].src, q.rel[0].wp, q.rel[0].mode, q.rel[0].ridx = 256, 256, mod.REL_CSR, 0
    q.rel[1].src, q.rel[1].wp, q.rel[1].mode = 256, 256, mod.REL_RANGE
    assert l.lgcn_agg_mlp(C.byref(q), None) == EINVAL
    # batched weight pack: job count and table pointer
    assert l.lgcn_pack_weight_batch(None, 0, 3, None) == 0
    assert l.lgcn_pack_weight_batch(None, 4, 3, None) == EINVAL
    assert l.lgcn_pack_weight_batch(C.c_void_p(256), -1, 3, None) == EINVAL
    assert l.lgcn_pack_weight_batch(C.c_void_p(256), 4, 7, None) == EINVAL
    # weight gradient: chunk count 1..1024
    w = mod.AggMlp()
    w.n_rows, w.n_rel = 64, 1
    for bad in (0, 1025):
        assert l.lgcn_wgrad(C.byref(w), C.c_void_p(256), C.c_void_p(256), C.c_void_p(256), bad, None) == EINVAL


def test_unknown_flag_bits_and_laneconv_arguments(lib):
    """lgcn_agg_mlp refuses flag bits it does not know (the timing-only work-skipping bits exist in the
    diagnostic build only); the LaneConv entry points validate geometry, groups and pointers before launching."""
    l, mod = lib
    EINVAL, ESHAPE, EALIGN = -1, -2, -3
    p = mod.AggMlp()
    p.n_rows, p.n_rel, p.out, p.mma = 10, 1, 256, 3
    p.rel[0].src, p.rel[0].wp, p.rel[0].mode = 256, 256, mod.REL_IDENT
    for bad in (1 << 8, 1 << 9, 1 << 6, 1 << 20):
        p.flags = bad
        assert l.lgcn_agg_mlp(C.byref(p), None) == EINVAL
    m, c = C.c_int32(), C.c_int32()
    assert l.lgcn_lc_config(mod.MMA_F32, 0, C.byref(m), C.byref(c)) == ESHAPE          # exact f32: lgcn_agg_mlp path
    assert l.lgcn_lc_config(mod.MMA_BF16X3, 0, C.byref(m), C.byref(c)) == ESHAPE       # three planes: lgcn_agg_mlp path too
    assert l.lgcn_lc_config(mod.MMA_F16X2, 3, C.byref(m), C.byref(c)) == EINVAL
    geoms = {}
    for mma in (mod.MMA_F16X2, mod.MMA_BF16):
        for v in (0, 1, 2):
            assert l.lgcn_lc_config(mma, v, C.byref(m), C.byref(c)) == 0
            assert m.value % 16 == 0 and c.value >= m.value
            geoms[(mma, v)] = (m.value, c.value)
            assert l.lgcn_lc_plan_elems(1000, m.value, c.value) > 0
            assert l.lgcn_lc_part_elems(1000, m.value, 1) == 0                           # one group: no partial sums
            assert l.lgcn_lc_part_elems(1000, m.value, 4) == ((1000 + m.value - 1) // m.value) * 4 * m.value * 128
    assert l.lgcn_lc_plan_elems(1000, 100, 200) == EINVAL                               # row block not supported
    assert l.lgcn_lc_plan_elems(1000, 96, 64) == EINVAL                                 # cap < rows per block
    M_, cap = geoms[(mod.MMA_F16X2, 0)]
    gs = (C.c_int32 * 3)(0, 8, 15)
    assert l.lgcn_lc_plan_build(None, None, 0, 14, M_, cap, 2, gs, None, None) == 0     # no nodes: nothing to do
    assert l.lgcn_lc_plan_build(C.c_void_p(256), C.c_void_p(256), 100, 14, M_, cap, 2, gs, None, None) == EINVAL   # null plan
    assert l.lgcn_lc_plan_build(C.c_void_p(256), C.c_void_p(256), 100, 14, M_, cap, 2, gs, C.c_void_p(260), None) == EALIGN
    bad = (C.c_int32 * 3)(0, 8, 14)                                                     # groups must end at n_units
    assert l.lgcn_lc_plan_build(C.c_void_p(256), C.c_void_p(256), 100, 14, M_, cap, 2, bad, C.c_void_p(256), None) == EINVAL
    # the weight-stationary pair kernel: split-precision modes only, seg in {0, 16}; RANGE16 relations likewise
    pa = [C.c_void_p(256)] * 5 + [64] + [C.c_void_p(256)] * 10 + [1e-5]
    assert l.lgcn_att_pairs_ws(*pa, mod.MMA_F32, 0, C.c_void_p(256), None) == ESHAPE
    for mma in (mod.MMA_BF16X3, mod.MMA_F16X2, mod.MMA_BF16):                          # and the streaming one: f32 only
        assert l.lgcn_att_pairs(*pa, mma, C.c_void_p(256), None) == ESHAPE
    assert l.lgcn_att_pairs_ws(*pa, mod.MMA_F16X2, 8, C.c_void_p(256), None) == EINVAL
    assert l.lgcn_att_pairs_ws(*pa, mod.MMA_F16X2, 16, C.c_void_p(260), None) == EALIGN
    pa[5] = 0
    assert l.lgcn_att_pairs_ws(*pa, mod.MMA_F16X2, 16, C.c_void_p(256), None) == 0      # no capacity: nothing to do
    p.flags, p.mma = 0, mod.MMA_F32
    p.rel[0].mode = mod.REL_RANGE16
    assert l.lgcn_agg_mlp(C.byref(p), None) == ESHAPE
    q = mod.LaneConv()
    assert l.lgcn_laneconv_fwd(None, None) == EINVAL
    q.mma = mod.MMA_F32
    assert l.lgcn_laneconv_fwd(C.byref(q), None) == ESHAPE
    q.mma, q.n_rows, q.rows_per_block, q.cap, q.n_units, q.n_groups = mod.MMA_F16X2, 100, M_, cap, 15, 1
    q.gstart[0], q.gstart[1] = 0, 15
    assert l.lgcn_laneconv_fwd(C.byref(q), None) == EINVAL                               # null pointers
    q.rows_per_block = 80
    assert l.lgcn_laneconv_fwd(C.byref(q), None) == EINVAL                               # not a geometry of this mode
    q.rows_per_block, q.n_rows = M_, 0
    assert l.lgcn_laneconv_fwd(C.byref(q), None) == 0                                    # no rows: no launch


def test_conv_entry_points_validate_before_launching(lib):
    """lgcn_conv1d_gn / lgcn_conv_pack_weight (ActorNet's blocks): sizes, shapes, pointers and alignment are checked on
    the host before anything is launched."""
    l, mod = lib
    EINVAL, ESHAPE, EALIGN = -1, -2, -3
    assert l.lgcn_conv_packed_bytes(128, 128, 3) == 3 * 4 * 8 * 2 * 64 * 16
    assert l.lgcn_conv_packed_bytes(3, 32, 3) == 3 * 1 * 2 * 2 * 64 * 16           # K padded to one 32-channel chunk
    assert l.lgcn_conv_packed_bytes(64, 128, 1) == 1 * 2 * 8 * 2 * 64 * 16
    for cin, cout, ks in ((0, 32, 3), (129, 32, 3), (32, 48, 3), (32, 32, 2), (32, 32, 5)):
        assert l.lgcn_conv_packed_bytes(cin, cout, ks) < 0
        assert l.lgcn_conv_pack_weight(256, cin, cout, ks, 256, None) == EINVAL
    assert l.lgcn_conv_pack_weight(None, 32, 32, 3, 256, None) == EINVAL
    assert l.lgcn_conv_pack_weight(256, 32, 32, 3, 264, None) == EALIGN

    def call(x=256, n=8, lin=20, cin=32, wp=256, cout=32, ks=3, stride=1, g=256, b=256, res=None, mode=0, out=256):
        return l.lgcn_conv1d_gn(x, n, lin, cin, wp, cout, ks, stride, g, b, 1e-5, res, mode, 1, out, None)

    assert call(n=0) == 0                                                            # nothing to do: no launch
    assert call(n=-1) == EINVAL and call(mode=3) == EINVAL and call(mode=-1) == EINVAL
    assert call(lin=8) == ESHAPE and call(lin=40) == ESHAPE                          # lout must be 5, 10 or 20
    # n = 0: the shapes are checked first, then nothing is launched (a valid call with n > 0 would launch on the
    # placeholder pointers)
    assert call(n=0, lin=20, stride=2, ks=1) == 0 and call(stride=3) == ESHAPE and call(stride=0) == ESHAPE
    assert call(cin=200) == ESHAPE and call(cout=96) == ESHAPE and call(ks=2) == ESHAPE
    assert call(lin=10, stride=2, mode=2, res=256) == ESHAPE                          # x2 upsampling needs an even lout
    assert call(x=None) == EINVAL and call(out=None) == EINVAL and call(g=None) == EINVAL
    assert call(mode=1) == EINVAL and call(mode=1, res=260) == EALIGN                 # a residual mode needs its tensor
    assert call(x=264) == EALIGN and call(wp=8) == EALIGN
    assert call(n=1 << 40) == ESHAPE

    def blk(x=256, n=8, lin=20, cin=32, c=32, stride=1, w1=256, g1=256, b1=256, w2=256, g2=256, b2=256, wd=None, gd=None, bd=None,
            out=256):
        return l.lgcn_res1d_gn(x, n, lin, cin, c, stride, w1, g1, b1, w2, g2, b2, wd, gd, bd, 1e-5, out, None)

    assert blk(n=0) == 0 and blk(n=0, cin=64, c=128, stride=2, lin=10, wd=256, gd=256, bd=256) == 0
    assert blk(n=-1) == EINVAL
    assert blk(cin=64, c=32) == ESHAPE and blk(stride=2) == ESHAPE            # an identity shortcut needs the same shape
    assert blk(wd=256) == EINVAL and blk(gd=256) == EINVAL                     # shortcut weights: all three or none
    assert blk(c=48, cin=48) == ESHAPE and blk(lin=8) == ESHAPE and blk(stride=3, wd=256, gd=256, bd=256) == ESHAPE
    assert blk(x=None) == EINVAL and blk(w2=None) == EINVAL and blk(out=260) == EALIGN
    assert blk(cin=64, c=128, wd=260, gd=256, bd=256) == EALIGN

    def pair(n=8, q=(256,) * 6, **kw):
        a = dict(x=256, lin=20, cin=32, c=32, stride=1, w1=256, g1=256, b1=256, w2=256, g2=256, b2=256, wd=None, gd=None, bd=None)
        a.update(kw)
        return l.lgcn_res1d_pair_gn(a["x"], n, a["lin"], a["cin"], a["c"], a["stride"], a["w1"], a["g1"], a["b1"], a["w2"], a["g2"],
                                    a["b2"], a["wd"], a["gd"], a["bd"], *q, 1e-5, 256, None)

    assert pair(n=0) == 0 and pair(n=-1) == EINVAL
    assert pair(q=(256, 256, None, 256, 256, 256)) == EINVAL and pair(q=(260, 256, 256, 256, 256, 256)) == EALIGN
    assert pair(cin=64, c=32) == ESHAPE and pair(lin=7) == ESHAPE


def test_pred_tail_entry_points_validate_before_launching(lib):
    """lgcn_pred_reg / lgcn_pred_final (PredNet's tail): mode and horizon limits, pointers and alignment."""
    l, mod = lib
    EINVAL, ESHAPE, EALIGN = -1, -2, -3

    def reg(n_act=10, n_mod=6, np2=60, **kw):
        q = mod.PredReg()
        for m in range(8):
            q.h[m], q.w[m], q.b[m] = 256, 256, 256
        q.ctrs, q.wd, q.bd, q.reg, q.hd = 256, 256, 256, 256, 256
        q.n_act, q.n_mod, q.np2 = n_act, n_mod, np2
        for k, v in kw.items():
            if isinstance(v, tuple):
                getattr(q, k)[v[0]] = v[1]
            else:
                setattr(q, k, v)
        return l.lgcn_pred_reg(C.byref(q), None)

    assert l.lgcn_pred_reg(None, None) == EINVAL
    assert reg(n_act=0) == 0
    assert reg(n_mod=0) == EINVAL and reg(n_mod=9) == EINVAL and reg(n_act=-1) == EINVAL
    assert reg(np2=66) == ESHAPE and reg(np2=59) == ESHAPE and reg(np2=0) == ESHAPE
    assert reg(h=(3, None)) == EINVAL and reg(w=(5, None)) == EINVAL and reg(b=(0, None)) == EINVAL
    assert reg(h=(2, 260)) == EALIGN and reg(hd=264) == EALIGN and reg(wd=260) == EALIGN
    assert reg(ctrs=None) == EINVAL and reg(reg=None) == EINVAL

    def fin(f=256, wc=256, bc=256, reg_=256, rot=None, orig=None, n=0, m=6, t=30, cls=256, out=256):
        return l.lgcn_pred_final(f, wc, bc, reg_, rot, orig, n, m, t, cls, out, None)

    assert fin() == 0
    assert fin(m=0) == EINVAL and fin(m=9) == EINVAL and fin(t=0) == EINVAL and fin(n=-1) == EINVAL
    assert fin(t=5000) == ESHAPE
    assert fin(f=None) == EINVAL and fin(cls=None) == EINVAL
    assert fin(rot=256) == EINVAL and fin(orig=256) == EINVAL          # both or neither
    assert fin(rot=264, orig=256) == EALIGN and fin(reg_=260) == EALIGN and fin(out=260) == EALIGN


def test_shipped_library_reads_no_environment():
    """No build of the library reads the environment or skips work: nothing under csrc/ (sources and Makefile) names
    getenv or the retired LGCN_TUNING / LGCN_ABLATE switches; a tile height is forced through lgcn_agg_mlp_t.tile_rb.
    The one diagnostic switch left, LGCN_STAMPS (timing stamps, same results), is not among the product's flags."""
    csrc = os.path.join(ROOT, "lanegcn-1_amd", "csrc")
    seen = 0
    for f in sorted(os.listdir(csrc)):
        path = os.path.join(csrc, f)
        if not os.path.isfile(path) or f.endswith((".o", ".so")):
            continue
        text = open(path, errors="replace").read()
        seen += f.endswith((".hip", ".hpp"))
        for word in ("getenv", "LGCN_TUNING", "LGCN_ABLATE"):
            assert word not in text, f + ": " + word
        assert "static int n = 0" not in text, f + ": function-local cache"
    assert seen >= 10
    mk = open(os.path.join(csrc, "Makefile")).read()
    flags = [ln for ln in mk.splitlines() if ln.startswith("CXXFLAGS")][0]
    assert "LGCN_STAMPS" not in flags


def test_product_never_imports_the_oracle():
    pkg = os.path.join(ROOT, "lanegcn-1_amd")
    for dirpath, _, files in os.walk(pkg):
        for f in files:
            if f.endswith((".py", ".hip", ".hpp", ".cpp")):
                text = open(os.path.join(dirpath, f)).read()
                assert "oracle" not in text.replace("no oracle", ""), f + " mentions the oracle"


def test_cpu_tensors_are_refused():
    import torch
    import lanegcn_amd  # noqa: F401
    from lanegcn_amd import lanegcn as M
    from lanegcn_amd._lib import LgcnError
    m = M.M2M(M.config)
    with torch.no_grad(), pytest.raises(LgcnError):
        m(torch.zeros(4, 128), {})
    with torch.no_grad(), pytest.raises(LgcnError):
        M.Linear(128, 128, ng=1)(torch.zeros(4, 128))
