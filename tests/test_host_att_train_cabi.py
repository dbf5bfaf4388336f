"""CPU: the training entry points of Att's pair stage (lgcn_att_pairs_train, lgcn_att_pairs_bwd and its workspace helper)
are exported and bound, and refuse null and misaligned pointers, a negative capacity and an out-of-range chunk count before
launching anything (no GPU needed).  Att.train_hip exists and is off by default."""
import ctypes as C

import pytest

EINVAL, ESHAPE, EALIGN = -1, -2, -3
NEW = ("lgcn_att_pairs_train", "lgcn_att_pairs_bwd_ws_elems", "lgcn_att_pairs_bwd")
REC = 2 * 128 * 128 + 7 * 128          # floats of one chunk record: dW_d2, dW_c0e and seven [128] vectors


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
    assert M.Att.train_hip is False


def test_struct_layout_matches_header(lib):
    _, mod = lib
    # lgcn_att_pairs_bwd_t: 5 pointers, cap, 24 pointers, eps, n_chunks
    assert mod.AttPairsBwd.cap.offset == 5 * 8
    assert mod.AttPairsBwd.eps.offset == 30 * 8
    assert C.sizeof(mod.AttPairsBwd) == 31 * 8


def test_workspace_helper(lib):
    l, _ = lib
    ws = l.lgcn_att_pairs_bwd_ws_elems
    assert ws(0, 1) == 0 and ws(0, 1024) == 0
    # one record per workgroup, never more workgroups than 32-pair tiles
    assert ws(1, 1) == REC and ws(32, 8) == REC and ws(33, 8) == 2 * REC and ws(130, 3) == 3 * REC and ws(130, 8) == 5 * REC
    assert ws(100000, 256) == 256 * REC and ws(0x7ffffff0, 1024) == 1024 * REC
    caps = (0, 1, 31, 32, 33, 64, 65, 130, 1000, 100000)
    for n in (1, 2, 3, 256, 1024):
        v = [ws(c, n) for c in caps]
        assert v == sorted(v), (n, v)                                # monotone in cap
    for c in caps:
        v = [ws(c, n) for n in (1, 2, 3, 4, 5, 256, 1024)]
        assert v == sorted(v), (c, v)                                # monotone in n_chunks
    assert ws(-1, 4) < 0 and ws(1 << 40, 4) < 0 and ws(0x7ffffff1, 4) < 0
    assert ws(64, 0) < 0 and ws(64, -1) < 0 and ws(64, 1025) < 0


def test_pairs_train_validates_before_launching(lib):
    l, _ = lib
    names = ("agt_ctrs", "ctx_ctrs", "hi", "wi", "n_pairs", "wd0", "bd0", "wpd2", "gd", "btd", "wpc0e", "U", "V", "gc", "btc",
             "m", "masks")

    def call(cap=64, **kw):
        a = {n: 256 for n in names}
        a.update(kw)
        return l.lgcn_att_pairs_train(a["agt_ctrs"], a["ctx_ctrs"], a["hi"], a["wi"], a["n_pairs"], cap,
                                      *(a[n] for n in names[5:15]), 1e-5, a["m"], a["masks"], None)

    assert call(cap=0) == 0                                              # nothing to do: no launch
    assert call(cap=-1) == EINVAL and call(cap=1 << 40) == ESHAPE
    for n in names:
        assert call(**{n: None}) == EINVAL, n
    for n in names[5:]:
        assert call(**{n: 260}) == EALIGN, n


def test_pairs_bwd_validates_before_launching(lib):
    l, mod = lib
    required = ("agt_ctrs", "ctx_ctrs", "hi", "wi", "n_pairs", "wd0", "bd0", "wpd2", "gd", "btd", "wpc0e", "U", "V", "gc", "btc",
                "masks", "dS")
    outs = ("d_wd2", "d_wc0e", "d_wd0", "d_bd0", "d_gd", "d_btd", "d_gc", "d_btc")

    def call(cap=64, n_chunks=2, **kw):
        q = mod.AttPairsBwd()
        for n in required + outs + ("wptd2", "wptc0e", "dc", "ws"):
            setattr(q, n, 256)
        q.cap, q.n_chunks, q.eps = cap, n_chunks, 1e-5
        for k, v in kw.items():
            setattr(q, k, v)
        return l.lgcn_att_pairs_bwd(C.byref(q), None)

    assert l.lgcn_att_pairs_bwd(None, None) == EINVAL
    assert call(cap=0) == 0                                              # nothing to do: no launch
    assert call(cap=-1) == EINVAL and call(cap=1 << 40) == ESHAPE
    assert call(n_chunks=0) == EINVAL and call(n_chunks=-3) == EINVAL and call(n_chunks=1025) == EINVAL
    for n in required:
        assert call(**{n: None}) == EINVAL, n
    # the transposed images and the workspace are required by the outputs that need them
    assert call(wptd2=None) == EINVAL and call(wptc0e=None) == EINVAL and call(ws=None) == EINVAL
    for n in required[5:] + outs + ("wptd2", "wptc0e", "dc", "ws"):
        assert call(**{n: 260}) == EALIGN, n
    # every output absent: nothing to compute, no launch
    assert call(dc=None, ws=None, wptd2=None, wptc0e=None, **{n: None for n in outs}) == 0
