"""CPU: the C entries that train the goal decoder and the fork model's loss (lgcn_goal_refine_bwd, lgcn_goal_decode_bwd,
lgcn_roi_loss_fwd, lgcn_roi_loss_bwd) are exported and refuse bad arguments before launching anything; the Python names
around them exist."""
import ctypes as C

import numpy as np
import pytest

EINVAL, ESHAPE = -1, -2
FAKE = C.c_void_p(0x1000)        # a non-null "device pointer": every call below is refused before it could be used
NULL = C.c_void_p(0)


@pytest.fixture(scope="module")
def lib():
    import lanegcn_amd  # noqa: F401
    from lanegcn_amd import _lib
    return _lib.load()


def host_i32(values):
    a = np.asarray(values, dtype=np.int32)
    return a, C.c_void_p(a.ctypes.data)


def test_entries_are_exported_and_bound(lib):
    from lanegcn_amd import _lib, autograd, lanercnn, ops
    for name in ("lgcn_goal_refine_bwd", "lgcn_goal_decode_bwd", "lgcn_roi_loss_fwd", "lgcn_roi_loss_bwd"):
        assert hasattr(lib, name) and name in _lib.SIGNATURES
    for name in ("goal_decode_bwd", "goal_refine_bwd", "roi_loss_fwd", "roi_loss_bwd"):
        assert callable(getattr(ops, name))
    for name in ("GoalDecodeFn", "GoalRefineFn", "RoiLossFn"):
        assert hasattr(autograd, name)
    for name in ("RoiLoss", "Loss", "PostProcess", "pred_metrics", "pred_metrics_ade"):
        assert callable(getattr(lanercnn, name))
    assert lanercnn.Decode.train_hip is False


def test_goal_refine_bwd_refuses_bad_arguments(lib):
    f = lib.lgcn_goal_refine_bwd
    assert f(FAKE, FAKE, FAKE, FAKE, -1, FAKE, FAKE, FAKE, None) == EINVAL
    for hole in range(7):                                                               # each tensor null in turn
        p = [FAKE] * 7
        p[hole] = NULL
        assert f(p[0], p[1], p[2], p[3], 12, p[4], p[5], p[6], None) == EINVAL, hole
    assert f(FAKE, FAKE, FAKE, FAKE, 1 << 40, FAKE, FAKE, FAKE, None) == ESHAPE
    assert f(NULL, NULL, NULL, NULL, 0, NULL, NULL, NULL, None) == 0                    # nothing to do: no launch


def decode_bwd_call(lib, pred_off, anc_off, n, n_anc, k, ptr=FAKE, off_ptrs=None, hole=None):
    a, pa = host_i32(pred_off)
    b, pb = host_i32(anc_off)
    if off_ptrs is not None:
        pa, pb = off_ptrs
    p = [ptr] * 14
    if hole is not None:
        p[hole] = NULL
    return lib.lgcn_goal_decode_bwd(p[0], p[1], pa, n, p[2], p[3], n_anc, p[4], pb, p[5], p[6], p[7], len(anc_off), k,
                                    p[8], p[9], p[10], p[11], p[12], p[13], None)


def test_goal_decode_bwd_refuses_bad_arguments(lib):
    ok = dict(pred_off=[0, 6, 13], anc_off=[4, 20], n=13, n_anc=40)
    assert decode_bwd_call(lib, k=6, ptr=NULL, **ok) == EINVAL                          # null tensors
    for hole in range(14):
        assert decode_bwd_call(lib, k=6, hole=hole, **ok) == EINVAL, hole
    assert decode_bwd_call(lib, k=9, **ok) == EINVAL                                    # k > 8
    assert decode_bwd_call(lib, k=0, **ok) == EINVAL
    assert decode_bwd_call(lib, k=7, **ok) == EINVAL                                    # the first RoI has 6 nodes < k
    assert decode_bwd_call(lib, [0, 6, 13], [4, 20], 12, 40, 6) == EINVAL               # span past pred
    assert decode_bwd_call(lib, [0, 6, 13], [4, 20], 14, 40, 6) == EINVAL               # spans do not cover d_pred
    assert decode_bwd_call(lib, [0, 6, 13], [4, 34], 13, 40, 6) == EINVAL               # anchors past their tensor
    assert decode_bwd_call(lib, [0, 6, 13], [-1, 20], 13, 40, 6) == EINVAL
    assert decode_bwd_call(lib, [1, 7, 14], [4, 20], 14, 40, 6) == EINVAL               # the table starts at 0
    assert decode_bwd_call(lib, [0, 6, 13], [4, 20], -1, 40, 6) == EINVAL               # negative sizes
    assert decode_bwd_call(lib, [0, 6, 13], [4, 20], 13, -1, 6) == EINVAL
    assert decode_bwd_call(lib, k=6, off_ptrs=(NULL, NULL), **ok) == EINVAL             # null host tables
    assert decode_bwd_call(lib, [0], [], 0, 0, 6, ptr=NULL) == 0                        # no agents: no launch
    a, pa = host_i32([0])
    assert lib.lgcn_goal_decode_bwd(*([NULL] * 2), pa, 0, NULL, NULL, 0, NULL, pa, NULL, NULL, NULL, -1, 6,
                                    *([NULL] * 6), None) == EINVAL                      # n_agt < 0


def roi_fwd(lib, n_agt, n_mod, n_t, p=None):
    p = p or [FAKE] * 9
    return lib.lgcn_roi_loss_fwd(p[0], p[1], p[2], p[3], p[4], n_agt, n_mod, n_t, 1.0, p[5], p[6], p[7], p[8], None)


def roi_bwd(lib, n_agt, n_mod, n_t, p=None):
    p = p or [FAKE] * 12
    return lib.lgcn_roi_loss_bwd(p[0], p[1], p[2], p[3], p[4], n_agt, n_mod, n_t, 1.0, *p[5:12], None)


@pytest.mark.parametrize("call,n_ptr", [(roi_fwd, 9), (roi_bwd, 12)])
def test_roi_loss_refuses_bad_arguments(lib, call, n_ptr):
    assert call(lib, -1, 6, 30) == EINVAL                                               # negative size
    assert call(lib, 4, 9, 30) == EINVAL                                                # M > 8
    assert call(lib, 4, 0, 30) == EINVAL
    assert call(lib, 4, 6, 65) == EINVAL                                                # T > 64
    assert call(lib, 4, 6, 0) == EINVAL
    assert call(lib, 4, -6, 30) == EINVAL
    for hole in range(n_ptr):
        p = [FAKE] * n_ptr
        p[hole] = NULL
        assert call(lib, 4, 6, 30, p) == EINVAL, hole
    assert call(lib, 1 << 40, 6, 30) == ESHAPE
    assert call(lib, 0, 6, 30, [NULL] * n_ptr) == 0                                     # nothing to do: no launch
    assert call(lib, 0, 9, 30, [NULL] * n_ptr) == EINVAL                                # ... but the sizes still count


def test_cpu_tensors_are_refused():
    import torch
    import lanegcn_amd  # noqa: F401
    from lanegcn_amd import _lib, lanegcn, lanercnn, ops
    z = torch.zeros
    with pytest.raises(_lib.LgcnError):
        ops.goal_refine_bwd(z(1, 6, 30), z(1, 6, 6), z(1, 6, 30, 2), z(1, 6, 30, 2))
    with pytest.raises(_lib.LgcnError):
        ops.roi_loss_fwd(z(2, 6), z(2, 6, 2), z(2, 6, 30, 2), z(2, 30, 2), z(2, 30, dtype=torch.bool))
    with pytest.raises(_lib.LgcnError):
        ops.goal_decode_bwd(z(6, 5), [0, 6], z(6, 2), z(6, 2), [0], z(1, 2), z(1, 2), z(1), z(1, 6, dtype=torch.int32))


def test_metrics_follow_the_formulas():
    import lanegcn_amd  # noqa: F401
    from lanegcn_amd import lanercnn as R
    rng = np.random.default_rng(2)
    gt = rng.normal(0, 3, (5, 30, 2)).astype(np.float32)
    preds = gt[:, None] + rng.normal(0, 1, (5, 6, 30, 2)).astype(np.float32)
    has = np.ones((5, 30), dtype=bool)
    ade1, fde1, ade, fde, idx = R.pred_metrics(preds, gt, has)
    err = np.sqrt(((preds.astype(np.float64) - gt[:, None]) ** 2).sum(-1))
    assert np.array_equal(idx, err[:, :, -1].argmin(1))
    assert abs(ade1 - err[:, 0].mean()) < 1e-5 and abs(fde1 - err[:, 0, -1].mean()) < 1e-5
    assert abs(ade - err[np.arange(5), idx].mean()) < 1e-5 and abs(fde - err[np.arange(5), idx, -1].mean()) < 1e-5
    goals = preds[np.arange(5), idx, -1]
    assert abs(R.pred_metrics_ade(goals, gt, has) - fde) < 1e-5
    with pytest.raises(AssertionError):
        R.pred_metrics(preds, gt, ~has)
