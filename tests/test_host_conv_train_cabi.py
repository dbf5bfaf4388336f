"""CPU: the training entry points of ActorNet's conv unit (lgcn_conv1d_gn_train, lgcn_conv1d_gn_bwd and their size helpers)
are exported, and refuse out-of-set shapes, null and misaligned pointers before launching anything (no GPU needed)."""
import ctypes as C

import pytest

EINVAL, ESHAPE, EALIGN = -1, -2, -3
NEW = ("lgcn_conv1d_gn_train", "lgcn_conv_packed_t_bytes", "lgcn_conv_pack_weight_t", "lgcn_conv1d_gn_bwd_ws_bytes",
       "lgcn_conv1d_gn_bwd")


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


def test_size_helpers(lib):
    l, _ = lib
    assert l.lgcn_conv_packed_t_bytes(128, 128, 3) == 3 * 128 * 128 * 4
    assert l.lgcn_conv_packed_t_bytes(3, 32, 3) == 3 * 16 * 32 * 4                    # input channels padded to 16
    assert l.lgcn_conv_packed_t_bytes(64, 128, 1) == 64 * 128 * 4
    for cin, cout, ks in ((0, 32, 3), (129, 32, 3), (32, 48, 3), (32, 32, 2)):
        assert l.lgcn_conv_packed_t_bytes(cin, cout, ks) < 0
        assert l.lgcn_conv_pack_weight_t(256, cin, cout, ks, 256, None) == EINVAL
    assert l.lgcn_conv_pack_weight_t(None, 32, 32, 3, 256, None) == EINVAL
    assert l.lgcn_conv_pack_weight_t(256, 32, 32, 3, None, None) == EINVAL
    assert l.lgcn_conv_pack_weight_t(256, 32, 32, 3, 260, None) == EALIGN
    # workspace: dy [A, lout, cout] + [n_wg, 2, cout] GroupNorm partials + [n_chunks, ks, cout, cin16] weight partials
    A = 1600
    ws = l.lgcn_conv1d_gn_bwd_ws_bytes(A, 20, 128, 128, 3, 1)
    assert ws >= 4 * (A * 20 * 128 + (A // 4) * 2 * 128 + 128 * 128 * 3)
    assert ws % 16 == 0
    assert l.lgcn_conv1d_gn_bwd_ws_bytes(333, 20, 3, 32, 3, 1) > 4 * 333 * 20 * 32
    assert l.lgcn_conv1d_gn_bwd_ws_bytes(0, 20, 32, 32, 3, 1) >= 0
    for lin, cin, cout, ks, stride in ((8, 32, 32, 3, 1), (20, 200, 32, 3, 1), (20, 32, 96, 3, 1), (20, 32, 32, 2, 1),
                                       (20, 32, 32, 3, 3), (40, 32, 32, 3, 1)):
        assert l.lgcn_conv1d_gn_bwd_ws_bytes(A, lin, cin, cout, ks, stride) == ESHAPE
    assert l.lgcn_conv1d_gn_bwd_ws_bytes(1 << 40, 20, 32, 32, 3, 1) == ESHAPE


def test_train_forward_validates_before_launching(lib):
    l, _ = lib

    def call(x=256, n=8, lin=20, cin=32, wp=256, cout=32, ks=3, stride=1, g=256, b=256, res=None, mode=0, out=256, y=256):
        return l.lgcn_conv1d_gn_train(x, n, lin, cin, wp, cout, ks, stride, g, b, 1e-5, res, mode, 1, out, y, None)

    assert call(n=0) == 0
    assert call(n=-1) == EINVAL and call(mode=3) == EINVAL
    assert call(lin=8) == ESHAPE and call(cin=200) == ESHAPE and call(cout=96) == ESHAPE and call(ks=2) == ESHAPE
    assert call(stride=3) == ESHAPE and call(lin=10, stride=2, mode=2, res=256) == ESHAPE
    assert call(n=1 << 40) == ESHAPE
    assert call(x=None) == EINVAL and call(out=None) == EINVAL and call(y=None) == EINVAL and call(mode=1) == EINVAL
    assert call(x=264) == EALIGN and call(y=260) == EALIGN and call(mode=1, res=260) == EALIGN


def test_backward_validates_before_launching(lib):
    l, _ = lib

    def call(g=256, x=256, y=256, out=256, n=8, lin=20, cin=32, wt=256, cout=32, ks=3, stride=1, gamma=256, mode=0, relu=1,
             dx=256, dw=256, dg=256, db=256, dres=None, ws=256):
        return l.lgcn_conv1d_gn_bwd(g, x, y, out, n, lin, cin, wt, cout, ks, stride, gamma, 1e-5, mode, relu, dx, dw, dg, db,
                                    dres, ws, None)

    assert call(n=0) == 0                                                            # nothing to do: no launch
    assert call(n=-1) == EINVAL and call(mode=3) == EINVAL and call(mode=-1) == EINVAL
    # exactly the forward's shape set
    assert call(lin=8) == ESHAPE and call(lin=40) == ESHAPE
    assert call(cin=0) == ESHAPE and call(cin=129) == ESHAPE and call(cout=16) == ESHAPE and call(cout=96) == ESHAPE
    assert call(ks=2) == ESHAPE and call(ks=5) == ESHAPE and call(stride=3) == ESHAPE and call(stride=0) == ESHAPE
    assert call(lin=10, stride=2, mode=2, dres=256) == ESHAPE                        # x2 upsampling needs an even lout
    assert call(n=1 << 40) == ESHAPE
    # null pointers: the inputs always, out with the ReLU, x with dW
    for k in ("g", "y", "wt", "gamma", "ws"):
        assert call(**{k: None}) == EINVAL, k
    assert call(out=None) == EINVAL and call(x=None) == EINVAL
    # misaligned pointers
    for k in ("g", "x", "y", "out", "wt", "gamma", "ws", "dx", "dw", "dg", "db"):
        assert call(**{k: 260}) == EALIGN, k
    assert call(mode=1, dres=264) == EALIGN
