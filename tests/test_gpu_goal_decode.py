"""GPU: the goal decoder's kernels (csrc/lgcn_goal.hip) alone.  lgcn_nms_select against the reference's recorded lists
and against the float64 greedy on synthetic segments; lgcn_goal_decode / lgcn_goal_refine on the reference's captured
inputs against the float64 restatement (tests/decode_model.py, pinned by test_decode_model_host.py)."""
import ctypes as C

import numpy as np
import pytest
import torch

import decode_model as DM

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ops():
    import lanegcn_amd  # noqa: F401
    from lanegcn_amd import ops
    return ops


def run_nms(ops, xys, logits, sizes, threshold=2.0, min_len=6, max_keep=0):
    off = [0] + [int(v) for v in np.cumsum(sizes)]
    xy_d = torch.from_numpy(np.ascontiguousarray(xys, dtype=np.float32)).cuda().reshape(-1, 2)
    lg_d = torch.from_numpy(np.ascontiguousarray(logits, dtype=np.float32)).cuda()
    keep = (xy_d.clone(), lg_d.clone())
    idx, count = ops.nms_select_segments(xy_d, lg_d, off, threshold, min_len, max_keep)
    bits = lambda t: t.view(torch.int32)                                        # NaN logits compare by their bits
    assert torch.equal(bits(xy_d), bits(keep[0])) and torch.equal(bits(lg_d), bits(keep[1]))     # inputs are not modified
    idx, count = idx.cpu().numpy(), count.cpu().numpy()
    lists = []
    for s, n in enumerate(sizes):
        seg = idx[off[s]:off[s + 1]]
        assert (seg[count[s]:] == -1).all(), "rows past the count must be -1"
        lists.append(seg[:count[s]].tolist())
    return lists


def test_nms_select_reproduces_the_reference_lists(ops):
    g = DM.fixture()[0]
    n_agt = len(g["dec/interest_roi"])
    xy = np.concatenate([g["dec/nms_xy/%d" % a] for a in range(n_agt)])
    lg = np.concatenate([g["dec/nms_logits/%d" % a] for a in range(n_agt)])
    sizes = [len(g["dec/nms_logits/%d" % a]) for a in range(n_agt)]
    want = [g["dec/nms_list/%d" % a].tolist() for a in range(n_agt)]
    assert run_nms(ops, xy, lg, sizes) == want
    assert run_nms(ops, xy, lg, sizes, max_keep=6) == [w[:6] for w in want]


SIZES = [1, 6, 7, 0, 64, 65, 257, 700]


@pytest.fixture(scope="module")
def synthetic():
    """Points on a 0.25 m grid (squared distances are exact in fp32 and never within rounding of threshold^2), distinct
    logits; the float64 greedy of every segment, computed once."""
    rng = np.random.default_rng(11)
    n = sum(SIZES)
    xy = (rng.integers(0, 120, (n, 2)) * 0.25).astype(np.float32)
    lg = rng.permutation(n).astype(np.float32) * 0.01 - 3.0
    off = np.cumsum([0] + SIZES)
    full = [DM.greedy(xy[off[s]:off[s + 1]], lg[off[s]:off[s + 1]], 2.0, 6, 0) for s in range(len(SIZES))]
    return xy, lg, full


@pytest.mark.parametrize("max_keep", [0, 6, 1000])
def test_nms_select_segments_of_many_sizes(ops, synthetic, max_keep):
    xy, lg, full = synthetic
    got = run_nms(ops, xy, lg, SIZES, max_keep=max_keep)
    assert got == [w[:max_keep] if max_keep > 0 else w for w in full]
    assert got[3] == [] and len(got[0]) == 1 and len(got[1]) == 6            # empty segment; fewer nodes than min_len
    if max_keep == 0:
        assert len(full[7]) > 256 or len(full[6]) > 64                         # survivors well past one pass per wave


def test_nms_select_boundary_and_order_rules(ops):
    # exactly 2.0 apart: both kept (the comparison is strict); 1.5 apart: the lower logit is dropped
    assert run_nms(ops, [[0, 0], [2, 0]], [1.0, 2.0], [2], min_len=0) == [[1, 0]]
    assert run_nms(ops, [[0, 0], [1.5, 0]], [1.0, 2.0], [2], min_len=0) == [[1]]
    assert run_nms(ops, [[0, 0], [1.5, 0]], [1.0, 2.0], [2], min_len=6) == [[1, 0]]     # ... and comes back as padding
    # every node inside one 1 m disc: one survivor, then 5 pads in logit order
    rng = np.random.default_rng(3)
    ang, rad = rng.uniform(0, 2 * np.pi, 40), rng.uniform(0, 0.5, 40)
    disc = np.stack([rad * np.cos(ang), rad * np.sin(ang)], 1)
    lg = rng.permutation(40).astype(np.float32)
    assert run_nms(ops, disc, lg, [40]) == [np.argsort(-lg)[:6].tolist()]
    # equal logits: the lower index comes first; in both phases
    far = np.stack([np.arange(8) * 3.0, np.zeros(8)], 1)
    assert run_nms(ops, far, np.zeros(8), [8]) == [list(range(8))]
    assert run_nms(ops, np.zeros((8, 2)), np.ones(8), [8]) == [[0, 1, 2, 3, 4, 5]]
    # NaN logits rank above every number, the lower index first among them
    assert run_nms(ops, far[:5], [0.5, np.nan, 7.0, np.nan, -1.0], [5], min_len=0) == [[1, 3, 2, 0, 4]]
    # max_keep below the survivor count, and min_len above max_keep
    assert run_nms(ops, far, np.arange(8.0), [8], min_len=6, max_keep=3) == [[7, 6, 5]]
    assert run_nms(ops, np.zeros((8, 2)), np.arange(8.0), [8], min_len=6, max_keep=3) == [[7, 6, 5]]


def test_nms_select_leaves_other_rows_untouched(ops):
    """A call over the middle segment alone writes that segment's rows only."""
    from lanegcn_amd import _lib
    lib = _lib.load()
    rng = np.random.default_rng(5)
    xy = torch.from_numpy((rng.integers(0, 40, (30, 2)) * 0.25).astype(np.float32)).cuda()
    lg = torch.from_numpy(rng.permutation(30).astype(np.float32)).cuda()
    off = torch.tensor([10, 20], dtype=torch.int32).cuda()
    idx = torch.full((30,), 77, dtype=torch.int32).cuda()
    count = torch.full((1,), -5, dtype=torch.int32).cuda()
    p = lambda t: C.c_void_p(t.data_ptr())
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    assert lib.lgcn_nms_select(p(xy), p(lg), p(off), 30, 1, 2.0, 6, 0, p(idx), p(count), stream) == 0
    torch.cuda.synchronize()
    idx, c = idx.cpu().numpy(), int(count.cpu()[0])
    want = DM.greedy(xy.cpu().numpy()[10:20], lg.cpu().numpy()[10:20], 2.0, 6, 0)
    assert (idx[:10] == 77).all() and (idx[20:] == 77).all()
    assert idx[10:10 + c].tolist() == want and (idx[10 + c:20] == -1).all()


def bars(g, ref):
    """Per tensor: max(4 x the rel error of the reference's own fp32 output against the float64 restatement, 1e-6)."""
    pairs = {"goals": "dec/out_goals", "logits": "dec/out_logits", "coef": "dec/coef", "s_samples": "dec/s_samples",
             "pred_trajs": "dec/out_trajs"}
    return {k: max(4 * DM.rel_err(g[v], ref[k].numpy()), 1e-6) for k, v in pairs.items()}


def test_goal_decode_and_refine_on_the_reference_inputs(ops):
    g = DM.fixture()[0]
    ref = DM.reference64()
    bar = bars(g, ref)
    a = DM.decode_args(g, torch.float32, "cuda")
    spans = a["spans"]
    pred_spans = [0] + [int(v) for v in np.cumsum([hi - lo for lo, hi in spans])]
    pred = torch.from_numpy(g["dec/pred"]).cuda()
    ins = [pred, a["anc_ctrs"], a["anc_dirs"], a["agt_ctrs"], a["agt_dirs"][:, -1].contiguous(), a["agt_vel"]]
    keep = [t.clone() for t in ins]
    run = lambda: ops.goal_decode(ins[0], pred_spans, ins[1], ins[2], [lo for lo, _ in spans], ins[3], ins[4], ins[5], 6, 2.0)
    top, goals, logits, coef, ss = run()
    assert np.array_equal(top.cpu().numpy(), g["dec/top_k"])
    got = {"goals": goals, "logits": logits, "coef": coef, "s_samples": ss}
    delta = torch.from_numpy(g["dec/traj_delta"]).cuda()
    # the refinement on the REFERENCE's fp32 coefficients and samples: its error alone
    got["pred_trajs"] = ops.goal_refine(torch.from_numpy(g["dec/s_samples"]).cuda(), torch.from_numpy(g["dec/coef"]).cuda(), delta)
    chained = ops.goal_refine(ss, coef, delta)
    for k, v in got.items():
        e = DM.rel_err(v.cpu().numpy(), ref[k].numpy())
        print("%-10s rel error %.2e (bar %.2e)" % (k, e, bar[k]))
    e = DM.rel_err(chained.cpu().numpy(), ref["pred_trajs"].numpy())
    print("%-10s rel error %.2e (bar %.2e), refine fed by goal_decode" % ("pred_trajs", e, bar["pred_trajs"]))
    for k, v in got.items():
        assert DM.rel_err(v.cpu().numpy(), ref[k].numpy()) <= bar[k], k
    assert e <= bar["pred_trajs"]
    again = run()
    assert all(torch.equal(x, y) for x, y in zip(again, (top, goals, logits, coef, ss)))     # bitwise repeatable
    assert torch.equal(ops.goal_refine(ss, coef, delta), chained)
    assert all(torch.equal(x, y) for x, y in zip(ins, keep))                                  # inputs unmodified


def test_goal_decode_refuses_a_short_roi(ops):
    from lanegcn_amd import _lib
    z = lambda *s: torch.zeros(*s, device="cuda")
    with pytest.raises(_lib.LgcnError):
        ops.goal_decode(z(11, 5), [0, 6, 11], z(20, 2), z(20, 2), [0, 6], z(2, 2), z(2, 2), z(2), 6, 2.0)
