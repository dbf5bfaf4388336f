"""CPU: the training entry points of PredNet's tail (lgcn_pred_final_train, lgcn_pred_final_bwd, lgcn_pred_reg_bwd and their
workspace helpers) are exported, and refuse null and misaligned pointers and out-of-set shapes before launching anything
(no GPU needed).  PredNet.train_hip exists and is off by default."""
import ctypes as C

import pytest

EINVAL, ESHAPE, EALIGN = -1, -2, -3
NEW = ("lgcn_pred_final_train", "lgcn_pred_final_bwd_ws_elems", "lgcn_pred_final_bwd", "lgcn_pred_reg_bwd_ws_elems",
       "lgcn_pred_reg_bwd")


@pytest.fixture(scope="module")
def lib():
    import lanegcn_amd  # noqa: F401
    from lanegcn_amd import _lib
    return _lib.load(), _lib


def test_training_symbols_are_exported_and_bound(lib):
    l, mod = lib
    for n in NEW:
        assert hasattr(l, n), "liblgcn.so does not export " + n
        assert n in mod.SIGNATURES
    assert l.lgcn_version() == 100


def test_train_hip_is_opt_in():
    import lanegcn_amd  # noqa: F401
    from lanegcn_amd import lanegcn as M
    assert M.PredNet.train_hip is False
    assert M.ActorNet.train_hip is False


def test_workspace_helpers(lib):
    l, _ = lib
    # final: one record of 132 floats (d wc [128], d bc, padding) per workgroup of 16 actors, never more than 256 records
    assert l.lgcn_pred_final_bwd_ws_elems(0) == 0
    assert l.lgcn_pred_final_bwd_ws_elems(1) == 132 and l.lgcn_pred_final_bwd_ws_elems(16) == 132
    assert l.lgcn_pred_final_bwd_ws_elems(17) == 2 * 132 and l.lgcn_pred_final_bwd_ws_elems(1600) == 100 * 132
    for n in (4096, 4097, 100000, 2000000):
        assert 0 < l.lgcn_pred_final_bwd_ws_elems(n) <= 256 * 132
    assert l.lgcn_pred_final_bwd_ws_elems(-1) < 0 and l.lgcn_pred_final_bwd_ws_elems(1 << 40) < 0
    # reg: one record per (chunk of 64 actors, mode): d W [np2, 128], 64 slots of d b, d wd [128, 2], d bd [128]
    rec = 60 * 128 + 64 + 384
    assert l.lgcn_pred_reg_bwd_ws_elems(0, 6, 60) == 0
    assert l.lgcn_pred_reg_bwd_ws_elems(1, 6, 60) == 6 * rec and l.lgcn_pred_reg_bwd_ws_elems(64, 6, 60) == 6 * rec
    assert l.lgcn_pred_reg_bwd_ws_elems(65, 6, 60) == 2 * 6 * rec and l.lgcn_pred_reg_bwd_ws_elems(1600, 6, 60) == 25 * 6 * rec
    assert l.lgcn_pred_reg_bwd_ws_elems(333, 3, 14) == 6 * 3 * (14 * 128 + 64 + 384)
    for n in (4096, 4097, 100000, 2000000):                                         # never more than 64 chunks
        assert 0 < l.lgcn_pred_reg_bwd_ws_elems(n, 8, 64) <= 64 * 8 * (64 * 128 + 64 + 384)
    for n, m, np2 in ((-1, 6, 60), (8, 0, 60), (8, 9, 60), (8, 6, 61), (8, 6, 66), (8, 6, 0), (1 << 40, 6, 60)):
        assert l.lgcn_pred_reg_bwd_ws_elems(n, m, np2) < 0


def test_final_train_validates_before_launching(lib):
    l, _ = lib

    def call(f=256, wc=256, bc=256, reg=256, n=8, m=6, np2=60, cls=256, out=256, order=256):
        return l.lgcn_pred_final_train(f, wc, bc, reg, n, m, np2, cls, out, order, None)

    assert call(n=0) == 0                                                            # nothing to do: no launch
    assert call(n=-1) == EINVAL and call(m=0) == EINVAL and call(m=9) == EINVAL
    assert call(np2=61) == ESHAPE and call(np2=66) == ESHAPE and call(np2=0) == ESHAPE
    assert call(n=1 << 40) == ESHAPE
    for k in ("f", "wc", "bc", "reg", "cls", "out", "order"):
        assert call(**{k: None}) == EINVAL, k
    assert call(reg=260) == EALIGN and call(out=260) == EALIGN


def test_final_bwd_validates_before_launching(lib):
    l, _ = lib

    def call(g_cls=256, g_out=256, order=256, f=256, wc=256, n=8, m=6, np2=60, g_reg=256, d_f=256, d_wc=256, d_bc=256,
             part=256):
        return l.lgcn_pred_final_bwd(g_cls, g_out, order, f, wc, n, m, np2, g_reg, d_f, d_wc, d_bc, part, None)

    assert call(n=0) == 0
    assert call(n=-1) == EINVAL and call(m=0) == EINVAL and call(m=9) == EINVAL
    assert call(np2=61) == ESHAPE and call(np2=66) == ESHAPE and call(np2=0) == ESHAPE
    assert call(n=1 << 40) == ESHAPE
    for k in ("order", "f", "wc", "d_wc", "d_bc", "part"):
        assert call(**{k: None}) == EINVAL, k
    # either gradient may be absent, g_reg / d_f need not be computed
    assert call(n=0, g_cls=None, g_out=None, g_reg=None, d_f=None) == 0
    for k in ("g_out", "f", "wc", "g_reg", "d_f"):
        assert call(**{k: 260}) == EALIGN, k


def test_reg_bwd_validates_before_launching(lib):
    l, mod = lib

    def call(n=8, m=6, np2=60, **kw):
        q = mod.PredRegBwd()
        for i in range(8):
            q.h[i] = q.w[i] = q.d_h[i] = q.d_w[i] = q.d_b[i] = 256
        q.g_reg = q.g_hd = q.hd = q.reg = q.ctrs = q.d_wd = q.d_bd = q.part = 256
        q.n_act, q.n_mod, q.np2 = n, m, np2
        for k, v in kw.items():
            if "_at_" in k:                                                      # h_at_5 = None: one slot of an array
                name, i = k.split("_at_")
                getattr(q, name)[int(i)] = v
            else:
                setattr(q, k, v)
        return l.lgcn_pred_reg_bwd(C.byref(q), None)

    assert l.lgcn_pred_reg_bwd(None, None) == EINVAL
    assert call(n=0) == 0
    assert call(n=-1) == EINVAL and call(m=0) == EINVAL and call(m=9) == EINVAL
    assert call(np2=61) == ESHAPE and call(np2=66) == ESHAPE and call(np2=0) == ESHAPE
    assert call(n=1 << 40) == ESHAPE
    for k in ("g_reg", "hd", "reg", "ctrs", "part", "h_at_0", "h_at_5", "w_at_0", "w_at_5"):
        assert call(**{k: None}) == EINVAL, k
    assert call(n=0, m=5, h_at_5=None, w_at_5=None) == 0                            # slots beyond n_mod are not read
    # every output and g_hd may be absent
    assert call(n=0, g_hd=None, d_wd=None, d_bd=None, d_h_at_0=None, d_w_at_3=None, d_b_at_5=None) == 0
    for k in ("part", "h_at_0", "h_at_5", "w_at_2", "d_h_at_1"):
        assert call(**{k: 260}) == EALIGN, k
