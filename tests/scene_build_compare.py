"""Comparisons shared by the scene-construction tests: bit equality of two scene trees, and a scene against the reference's
recording with the bounds the feature was specified with:

  integer / boolean leaves, orig, theta, rot, gt_preds (and the exact 0 / 1 node attributes): array_equal;
  position-like floats (ctrs, obs_trajs[:, :, :2], node ctrs, node feats): within 1 fp32 ulp of the scene's largest
      coordinate magnitude -- a BLAS dgemm may fuse the multiply-add, which moves the float64 value by its last bits and
      the fp32 rounding by at most one step;
  feats[:, :, :2]: within 2 such ulps (an fp32 difference of two such values).
"""
import numpy as np
import torch


def host(x):
    return x.detach().cpu().numpy() if torch.is_tensor(x) else np.asarray(x)


def leaves(tree, prefix=""):
    if isinstance(tree, dict):
        for k in sorted(tree):
            yield from leaves(tree[k], prefix + str(k) + "/")
    elif isinstance(tree, (list, tuple)):
        for i, v in enumerate(tree):
            yield from leaves(v, prefix + str(i) + "/")
    else:
        yield prefix[:-1], tree


def assert_same_bits(got, want, what=""):
    """Every leaf of two scene trees: same keys, shapes, dtypes and bytes."""
    g, w = dict(leaves(got)), dict(leaves(want))
    assert sorted(g) == sorted(w), (what, sorted(set(g) ^ set(w)))
    for k in w:
        a, b = host(g[k]), host(w[k])
        if isinstance(w[k], (str, int, float)) or b.ndim == 0:
            assert a.tolist() == b.tolist(), (what, k, a, b)
            continue
        assert a.shape == b.shape and a.dtype == b.dtype, (what, k, a.shape, b.shape, a.dtype, b.dtype)
        assert a.tobytes() == b.tobytes(), (what, k, int((a != b).sum()))


def edge_set(e):
    u, v = host(e["u"]).astype(np.int64), host(e["v"]).astype(np.int64)
    uv = np.stack([u, v], 1)
    return uv[np.lexsort((uv[:, 1], uv[:, 0]))]


def check_against_recording(got, want, what=""):
    """Asserts the bounds above for one scene; returns (position-like elements that differ at all, elements compared)."""
    exact = lambda k, a, b: np.testing.assert_array_equal(host(a), host(b), err_msg="%s %s" % (what, k))
    gg, wg = got["graph"], want["graph"]
    for k in ("has_preds", "gt_preds", "orig", "rot"):
        assert host(got[k]).dtype == host(want[k]).dtype, (what, k)
        exact(k, got[k], want[k])
    assert float(got["theta"]) == float(want["theta"]), (what, "theta")
    assert host(got["feats"]).shape == host(want["feats"]).shape, (what, "kept tracks")
    assert int(gg["num_nodes"]) == int(wg["num_nodes"]), (what, "num_nodes")
    for k in ("lane_idcs", "turn", "control", "intersect"):
        assert host(gg[k]).dtype == host(wg[k]).dtype, (what, k)
        exact(k, gg[k], wg[k])
    for k in ("pre_pairs", "suc_pairs", "left_pairs", "right_pairs"):
        assert host(gg[k]).dtype == np.int64
        exact(k, host(gg[k]).reshape(-1, 2), host(wg[k]).reshape(-1, 2))
    assert len(gg["pre"]) == len(wg["pre"]) and len(gg["suc"]) == len(wg["suc"])
    for k in ("pre", "suc"):
        for c in "uv":
            assert host(gg[k][0][c]).dtype == np.int64
            exact("%s[0][%s]" % (k, c), gg[k][0][c], wg[k][0][c])
        for i in range(1, len(wg[k])):      # the dilated scales: scipy fixes no order inside a row
            exact("%s[%d]" % (k, i), edge_set(gg[k][i]), edge_set(wg[k][i]))
    obs_w = host(want["obs_trajs"])
    mag = max(float(np.abs(host(want["ctrs"])).max(initial=0)), float(np.abs(obs_w[:, :, :2]).max(initial=0)),
              float(np.abs(host(wg["ctrs"])).max()), float(np.abs(host(wg["feats"])).max()))
    ulp = float(np.spacing(np.float32(mag)))
    n_diff = n_all = 0
    for k, a, b, n_ulp in (("ctrs", got["ctrs"], want["ctrs"], 1), ("obs_trajs", host(got["obs_trajs"])[:, :, :2], obs_w[:, :, :2], 1),
                           ("graph ctrs", gg["ctrs"], wg["ctrs"], 1), ("graph feats", gg["feats"], wg["feats"], 1),
                           ("feats", host(got["feats"])[:, :, :2], host(want["feats"])[:, :, :2], 2)):
        a, b = host(a), host(b)
        assert a.shape == b.shape and a.dtype == np.float32 and b.dtype == np.float32, (what, k, a.shape, b.shape)
        err = np.abs(a.astype(np.float64) - b.astype(np.float64))
        n_diff += int((err > 0).sum())
        n_all += err.size
        assert float(err.max(initial=0)) <= n_ulp * ulp, (what, k, float(err.max()), ulp)
    exact("obs_trajs flag", host(got["obs_trajs"])[:, :, 2], obs_w[:, :, 2])
    exact("feats flag", host(got["feats"])[:, :, 2], host(want["feats"])[:, :, 2])
    return n_diff, n_all
