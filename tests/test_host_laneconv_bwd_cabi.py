"""CPU: the fused LaneConv / LinearRes backward (lgcn_laneconv_bwd and its workspace helper) is exported and bound, its
ctypes struct matches the header, the workspace helper counts one record per workgroup, and both variants of the entry
(ident1 = 0: any relations, ident1 = 1: one IDENT relation) refuse null and misaligned pointers, a negative or too large row
count and an out-of-range chunk count before launching anything (no GPU needed).  MapNet.train_hip, M2M.train_hip and
LinearRes.train_hip exist and are off by default."""
import ctypes as C

import pytest

EINVAL, ESHAPE, EALIGN = -1, -2, -3
NEW = ("lgcn_laneconv_bwd_ws_elems", "lgcn_laneconv_bwd")
REC = {0: 128 * 128 + 4 * 128, 1: 2 * 128 * 128 + 4 * 128}      # floats of one chunk record: dW2 [, dW1], four [128] vectors

INPUTS = ("d_out", "out", "Z", "Y", "T", "gamma1", "gamma2", "wpt2")
INPUTS_IDENT = ("X", "wpt1")
PARAM_OUTS = {0: ("d_w2", "d_g2", "d_b2", "d_g1", "d_b1"), 1: ("d_w2", "d_w1", "d_g2", "d_b2", "d_g1", "d_b1")}
ROW_OUTS = {0: ("dT", "g2"), 1: ("dX",)}


@pytest.fixture(scope="module")
def lib():
    import lanegcn_amd  # noqa: F401
    from lanegcn_amd import _lib
    return _lib.load(), _lib


def test_symbols_are_exported_and_bound(lib):
    l, mod = lib
    for n in NEW:
        assert hasattr(l, n), "liblgcn.so does not export " + n
        assert n in mod.SIGNATURES
    assert l.lgcn_version() == 100


def test_switches_are_opt_in():
    import lanegcn_amd  # noqa: F401
    from lanegcn_amd import autograd as A
    from lanegcn_amd import lanegcn as M
    from lanegcn_amd import layers
    assert M.MapNet.train_hip is False and M.M2M.train_hip is False and layers.LinearRes.train_hip is False
    assert A.BlockSpec(n_rows=1, rels=[]).fused_bwd is False
    from lanegcn_amd import ops
    assert callable(ops.laneconv_bwd)


def test_struct_layout_matches_header(lib):
    _, mod = lib
    # lgcn_laneconv_bwd_t: 6 + 4 input pointers, 3 + 7 output pointers, n_rows, eps, n_chunks, ident1, pad
    S = mod.LaneConvBwd
    assert [f[0] for f in S._fields_[:20]] == ["d_out", "out", "Z", "Y", "T", "X", "gamma1", "gamma2", "wpt2", "wpt1", "dT", "g2",
                                               "dX", "d_w2", "d_w1", "d_g2", "d_b2", "d_g1", "d_b1", "ws"]
    assert S.X.offset == 5 * 8 and S.dT.offset == 10 * 8 and S.ws.offset == 19 * 8
    assert S.n_rows.offset == 20 * 8 and S.eps.offset == 21 * 8 and S.n_chunks.offset == 21 * 8 + 4
    assert S.ident1.offset == 22 * 8
    assert C.sizeof(S) == 23 * 8


def test_workspace_helper(lib):
    l, _ = lib
    ws = l.lgcn_laneconv_bwd_ws_elems
    for ident1 in (0, 1):
        R = REC[ident1]
        assert ws(0, 1, ident1) == 0 and ws(0, 1024, ident1) == 0
        # one record per workgroup, never more workgroups than 32-row tiles
        assert ws(1, 1, ident1) == R and ws(1, 7, ident1) == R
        assert ws(32, 1, ident1) == R and ws(32, 8, ident1) == R
        assert ws(33, 1, ident1) == R and ws(33, 2, ident1) == 2 * R and ws(33, 8, ident1) == 2 * R
        assert ws(130, 1, ident1) == R and ws(130, 3, ident1) == 3 * R and ws(130, 5, ident1) == 5 * R
        assert ws(130, 8, ident1) == 5 * R and ws(130, 1024, ident1) == 5 * R
        assert ws(100000, 256, ident1) == 256 * R and ws(0x7fffffff, 1024, ident1) == 1024 * R
        rows = (0, 1, 31, 32, 33, 64, 65, 130, 1000, 100000)
        for n in (1, 2, 3, 256, 1024):
            v = [ws(r, n, ident1) for r in rows]
            assert v == sorted(v), (n, v)                                # monotone in n_rows
        for r in rows:
            v = [ws(r, n, ident1) for n in (1, 2, 3, 4, 5, 256, 1024)]
            assert v == sorted(v), (r, v)                                # monotone in n_chunks
        assert ws(-1, 4, ident1) < 0 and ws(1 << 40, 4, ident1) < 0 and ws(0x80000000, 4, ident1) < 0
        assert ws(64, 0, ident1) < 0 and ws(64, -1, ident1) < 0 and ws(64, 1025, ident1) < 0
    assert ws(64, 4, 2) < 0 and ws(64, 4, -1) < 0
    assert ws(130, 3, 1) - ws(130, 3, 0) == 3 * 128 * 128


@pytest.mark.parametrize("ident1", [0, 1])
def test_entry_validates_before_launching(lib, ident1):
    l, mod = lib
    required = INPUTS + (INPUTS_IDENT if ident1 else ())
    outs = PARAM_OUTS[ident1] + ROW_OUTS[ident1]

    def call(n_rows=64, n_chunks=2, **kw):
        q = mod.LaneConvBwd()
        for n in required + outs + ("ws",):
            setattr(q, n, 256)
        q.n_rows, q.n_chunks, q.eps, q.ident1 = n_rows, n_chunks, 1e-5, ident1
        for k, v in kw.items():
            setattr(q, k, v)
        return l.lgcn_laneconv_bwd(C.byref(q), None)

    assert l.lgcn_laneconv_bwd(None, None) == EINVAL
    assert call(n_rows=0) == 0                                           # nothing to do: no launch
    assert call(n_rows=-1) == EINVAL and call(n_rows=1 << 40) == ESHAPE and call(n_rows=0x80000000) == ESHAPE
    assert call(n_chunks=0) == EINVAL and call(n_chunks=-3) == EINVAL and call(n_chunks=1025) == EINVAL
    assert call(ident1=2) == EINVAL and call(ident1=-1) == EINVAL
    for n in required:
        assert call(**{n: None}) == EINVAL, n
    assert call(ws=None) == EINVAL                                       # required by any parameter gradient
    # an output of the other variant is an error, not a silent no-op
    for n in ROW_OUTS[1 - ident1] + (() if ident1 else ("d_w1",)):
        assert call(**{n: 256}) == EINVAL, n
    for n in required + outs + ("ws",):
        assert call(**{n: 260}) == EALIGN, n
    if not ident1:                                                       # X / wpt1 are not read, but must not be misaligned
        assert call(X=260) == EALIGN and call(wpt1=260) == EALIGN
    # every output absent: nothing to compute, no launch
    assert call(ws=None, **{n: None for n in outs}) == 0
    assert call(n_rows=0, ws=None, **{n: None for n in outs}) == 0
