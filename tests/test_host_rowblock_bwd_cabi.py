"""CPU: the fused row-block backward (lgcn_rowblock_bwd and its workspace helper) is exported and bound, its ctypes struct
matches the header, the workspace helper counts one record per workgroup, and the entry refuses a null struct, a negative or
too large row count, a relation or chunk count out of range, missing inputs, a GroupNorm gradient without a norm, a missing
workspace, a bad row stride and misaligned pointers before launching anything (no GPU needed).  RowBlockFn.train_hip exists and
is off by default."""
import ctypes as C

import pytest

EINVAL, ESHAPE, EALIGN = -1, -2, -3
NEW = ("lgcn_rowblock_bwd_ws_elems", "lgcn_rowblock_bwd")


def REC(n_rel):      # floats of one chunk record: dW_0 [, dW_1], dgamma, dbeta
    return n_rel * 16384 + 256


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


def test_switch_is_opt_in():
    import lanegcn_amd  # noqa: F401
    from lanegcn_amd import autograd as A
    from lanegcn_amd import ops
    assert A.RowBlockFn.train_hip is False
    assert A.BlockSpec(n_rows=1, rels=[]).fused_bwd is False
    assert callable(ops.rowblock_bwd)


def test_struct_layout_matches_header(lib):
    _, mod = lib
    # lgcn_rowblock_bwd_t: 4 input pointers, src[2], wpt[2], d_src[2], d_w[2], 4 output pointers, n_rows, ld_w[2], eps, n_rel,
    # n_chunks, pad
    S = mod.RowBlockBwd
    assert [f[0] for f in S._fields_] == ["d_out", "out", "pre", "gamma", "src", "wpt", "d_src", "d_w", "d_res", "d_gamma",
                                          "d_beta", "ws", "n_rows", "ld_w", "eps", "n_rel", "n_chunks", "pad_"]
    assert S.gamma.offset == 3 * 8 and S.src.offset == 4 * 8 and S.wpt.offset == 6 * 8 and S.d_src.offset == 8 * 8
    assert S.d_w.offset == 10 * 8 and S.d_res.offset == 12 * 8 and S.ws.offset == 15 * 8
    assert S.n_rows.offset == 16 * 8 and S.ld_w.offset == 17 * 8 and S.eps.offset == 18 * 8 and S.n_rel.offset == 18 * 8 + 4
    assert S.n_chunks.offset == 19 * 8 and S.pad_.offset == 19 * 8 + 4
    assert S.src.size == 16 and S.d_w.size == 16 and S.ld_w.size == 8
    assert C.sizeof(S) == 20 * 8


def test_workspace_helper(lib):
    l, _ = lib
    ws = l.lgcn_rowblock_bwd_ws_elems
    for n_rel in (1, 2):
        R = REC(n_rel)
        for c in (1, 2, 3, 7, 256, 1024):
            assert ws(0, c, n_rel) == 0
            # one record per workgroup, never more workgroups than 32-row tiles
            for n in (1, 32, 33, 130, 100000, 0x7fffffff):
                assert ws(n, c, n_rel) == min(c, (n + 31) // 32) * R, (n, c, n_rel)
        rows = (0, 1, 31, 32, 33, 64, 65, 130, 1000, 100000)
        for c in (1, 2, 3, 256, 1024):
            v = [ws(r, c, n_rel) for r in rows]
            assert v == sorted(v), (c, v)                                # monotone in n_rows
        for r in rows:
            v = [ws(r, c, n_rel) for c in (1, 2, 3, 4, 5, 256, 1024)]
            assert v == sorted(v), (r, v)                                # monotone in n_chunks
        assert ws(-1, 4, n_rel) < 0 and ws(1 << 40, 4, n_rel) < 0 and ws(0x80000000, 4, n_rel) < 0
        assert ws(64, 0, n_rel) < 0 and ws(64, -1, n_rel) < 0 and ws(64, 1025, n_rel) < 0
    assert ws(64, 4, 0) < 0 and ws(64, 4, 3) < 0 and ws(64, 4, -1) < 0
    assert ws(130, 3, 2) - ws(130, 3, 1) == 3 * 128 * 128


@pytest.mark.parametrize("n_rel", [1, 2])
@pytest.mark.parametrize("gn", [True, False])
def test_entry_validates_before_launching(lib, n_rel, gn):
    l, mod = lib

    def call(n_rows=64, n_chunks=2, **kw):
        """Every pointer 256 (pre, gamma and the GroupNorm gradients only with gn); keywords override a field, for an array
        field as (index, value)."""
        q = mod.RowBlockBwd()
        for n in ("d_out", "out", "d_res", "ws") + (("pre", "gamma", "d_gamma", "d_beta") if gn else ()):
            setattr(q, n, 256)
        for n in ("src", "wpt", "d_src", "d_w"):
            for r in range(n_rel):
                getattr(q, n)[r] = 256
        for r in range(2):
            q.ld_w[r] = 128
        q.n_rows, q.n_chunks, q.eps, q.n_rel = n_rows, n_chunks, 1e-5, n_rel
        for k, v in kw.items():
            if isinstance(v, tuple):
                getattr(q, k)[v[0]] = v[1]
            else:
                setattr(q, k, v)
        return l.lgcn_rowblock_bwd(C.byref(q), None)

    assert l.lgcn_rowblock_bwd(None, None) == EINVAL
    assert call(n_rows=0) == 0                                           # nothing to do: no launch
    assert call(n_rows=-1) == EINVAL and call(n_rows=1 << 40) == ESHAPE and call(n_rows=0x80000000) == ESHAPE
    assert call(n_rel=0) == EINVAL and call(n_rel=3) == EINVAL and call(n_rel=-1) == EINVAL
    assert call(n_chunks=0) == EINVAL and call(n_chunks=-3) == EINVAL and call(n_chunks=1025) == EINVAL
    # the row count is looked at first, then the relation count, then the chunk count, all before the pointers
    assert call(n_rows=1 << 40, n_rel=0) == ESHAPE and call(n_rel=0, d_out=260) == EINVAL and call(n_chunks=0, d_out=260) == EINVAL
    assert call(d_out=None) == EINVAL
    for r in range(n_rel):
        assert call(src=(r, None)) == EINVAL and call(wpt=(r, None)) == EINVAL, r
    if gn:
        assert call(pre=None) == EINVAL and call(gamma=None) == EINVAL   # both or neither
    else:
        assert call(pre=256) == EINVAL and call(gamma=256) == EINVAL
        assert call(d_gamma=256) == EINVAL and call(d_beta=256) == EINVAL      # no norm, no norm gradient
    assert call(ws=None) == EINVAL                                       # required by any parameter gradient
    for r in range(n_rel):
        for ld in (0, 127, 124, 130, 133, -128):
            assert call(ld_w=(r, ld)) == EINVAL, (r, ld)
    # a missing input comes before a misaligned pointer
    assert call(d_out=None, out=260) == EINVAL and call(ws=None, d_res=260) == EINVAL and call(ld_w=(0, 127), out=260) == EINVAL
    scalars = ("d_out", "out", "d_res", "ws") + (("pre", "gamma", "d_gamma", "d_beta") if gn else ())
    for n in scalars:
        assert call(**{n: 260}) == EALIGN, n
    for n in ("src", "wpt", "d_src", "d_w"):
        for r in range(2):                                               # an unused second relation must not be misaligned either
            assert call(**{n: (r, 260)}) == EALIGN, (n, r)
    # every output absent: nothing to compute, no launch
    none = dict(d_res=None, d_gamma=None, d_beta=None, ws=None)
    if n_rel == 1:
        assert call(d_src=(0, None), d_w=(0, None), **none) == 0
        assert call(n_rows=0, d_src=(0, None), d_w=(0, None), **none) == 0


def test_nothing_to_do_returns_ok(lib):
    l, mod = lib
    for n_rel in (1, 2):
        for gn in (True, False):
            for n_rows in (0, 64):
                q = mod.RowBlockBwd()
                q.d_out = q.out = 256
                if gn:
                    q.pre = q.gamma = 256
                for r in range(n_rel):
                    q.src[r] = q.wpt[r] = 256
                q.n_rows, q.n_chunks, q.eps, q.n_rel = n_rows, 3, 1e-5, n_rel
                assert l.lgcn_rowblock_bwd(C.byref(q), None) == 0, (n_rel, gn, n_rows)      # every output NULL, no workspace
