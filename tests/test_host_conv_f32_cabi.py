"""CPU: the exact-fp32 entry points of ActorNet's conv unit (lgcn_conv_packed_f32_bytes, lgcn_conv_pack_weight_f32,
lgcn_conv1d_gn_f32) are exported and bound, and refuse out-of-set shapes, null and misaligned pointers before launching
anything (no GPU needed); the Python switch that selects them is off by default."""
import inspect

import pytest

EINVAL, ESHAPE, EALIGN = -1, -2, -3
NEW = ("lgcn_conv_packed_f32_bytes", "lgcn_conv_pack_weight_f32", "lgcn_conv1d_gn_f32")


@pytest.fixture(scope="module")
def lib():
    import lanegcn_amd  # noqa: F401
    from lanegcn_amd import _lib
    return _lib.load(), _lib


def test_exact_symbols_are_exported_and_bound(lib):
    l, mod = lib
    for n in NEW:
        assert hasattr(l, n), "liblgcn.so does not export " + n
        assert n in mod.SIGNATURES
    assert l.lgcn_version() == 100


def test_packed_f32_bytes(lib):
    l, _ = lib
    # [ks][cin padded to 32][cout] fp32 values
    assert l.lgcn_conv_packed_f32_bytes(128, 128, 3) == 3 * 128 * 128 * 4
    assert l.lgcn_conv_packed_f32_bytes(3, 32, 3) == 3 * 32 * 32 * 4                  # input channels padded to 32
    assert l.lgcn_conv_packed_f32_bytes(64, 128, 1) == 64 * 128 * 4
    assert l.lgcn_conv_packed_f32_bytes(33, 64, 3) == 3 * 64 * 64 * 4
    for cin, cout, ks in ((3, 32, 3), (32, 64, 1), (128, 128, 3)):                   # the traffic of the two fp16 planes
        assert l.lgcn_conv_packed_f32_bytes(cin, cout, ks) == l.lgcn_conv_packed_bytes(cin, cout, ks)
    for cin, cout, ks in ((0, 32, 3), (129, 32, 3), (32, 48, 3), (32, 32, 2)):
        assert l.lgcn_conv_packed_f32_bytes(cin, cout, ks) < 0
        assert l.lgcn_conv_pack_weight_f32(256, cin, cout, ks, 256, None) == EINVAL


def test_pack_weight_f32_validates_before_launching(lib):
    l, _ = lib
    assert l.lgcn_conv_pack_weight_f32(None, 32, 32, 3, 256, None) == EINVAL
    assert l.lgcn_conv_pack_weight_f32(256, 32, 32, 3, None, None) == EINVAL
    assert l.lgcn_conv_pack_weight_f32(256, 32, 32, 3, 260, None) == EALIGN


def test_forward_f32_validates_before_launching(lib):
    l, _ = lib

    def call(x=256, n=8, lin=20, cin=32, wp=256, cout=32, ks=3, stride=1, g=256, b=256, res=None, mode=0, out=256, y=256):
        return l.lgcn_conv1d_gn_f32(x, n, lin, cin, wp, cout, ks, stride, g, b, 1e-5, res, mode, 1, out, y, None)

    assert call(n=0) == 0 and call(n=0, y=None) == 0                                 # nothing to do: no launch
    assert call(n=-1) == EINVAL and call(mode=3) == EINVAL and call(mode=-1) == EINVAL
    assert call(lin=8) == ESHAPE and call(cin=200) == ESHAPE and call(cout=96) == ESHAPE and call(ks=2) == ESHAPE
    assert call(cin=0) == ESHAPE and call(lin=40) == ESHAPE and call(stride=0) == ESHAPE
    assert call(stride=3) == ESHAPE and call(lin=10, stride=2, mode=2, res=256) == ESHAPE
    assert call(n=1 << 40) == ESHAPE
    # shapes before pointers
    assert call(x=None, lin=8) == ESHAPE
    for k in ("x", "wp", "g", "b", "out"):
        assert call(**{k: None}) == EINVAL, k
        assert call(**{k: None}, y=None) == EINVAL, k
    assert call(mode=1) == EINVAL and call(mode=2) == EINVAL                         # a residual mode without a residual
    for k in ("x", "wp", "g", "b", "out", "y"):
        assert call(**{k: 264 if k == "x" else 260}) == EALIGN, k
    assert call(mode=1, res=260) == EALIGN and call(mode=1, res=260, y=None) == EALIGN


def test_exact_is_opt_in():
    import lanegcn_amd  # noqa: F401
    from lanegcn_amd import autograd as A
    from lanegcn_amd import lanegcn as M
    from lanegcn_amd import ops
    assert M.ActorNet.exact is False
    assert M.ActorNet.train_hip is False
    for fn in (ops.conv1d_gn, ops.conv1d_gn_train, A.conv1d_gn):
        assert inspect.signature(fn).parameters["exact"].default is False
    assert callable(ops.conv_packed_f32)
