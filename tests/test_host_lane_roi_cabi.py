"""CPU: the lane-RoI entry points (lgcn_roi_*) are exported, bound and declared, refuse bad arguments before launching
anything, size their workspace monotonically, and lanegcn_amd.data_lrcnn refuses to run without a GPU."""
import ctypes as C
import inspect
import os
import re

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("lgcn_roi_max_lanes", "lgcn_roi_max_levels", "lgcn_roi_lane_length_host", "lgcn_roi_ws_elems", "lgcn_roi_search",
         "lgcn_roi_nodes", "lgcn_roi_edge_count", "lgcn_roi_edge_fill")
EINVAL, ESHAPE, EALIGN = -1, -2, -3


@pytest.fixture(scope="module")
def lib():
    import lanegcn_amd  # noqa: F401
    from lanegcn_amd import _lib
    return _lib.load(), _lib


def test_symbols_are_exported_bound_and_declared(lib):
    l, mod = lib
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "lgcn.h")).read(), flags=re.S)
    for n in NAMES:
        assert hasattr(l, n) and n in mod.SIGNATURES and re.search(r"\b%s\s*\(" % n, header), n
    # lgcn_roi_t: 14 int32 / float words, then 29 pointers
    assert C.sizeof(mod.Roi) == 14 * 4 + 29 * 8 and mod.Roi.off_host.offset == 56
    assert l.lgcn_roi_max_lanes() == 4096 >= 1024 and l.lgcn_roi_max_levels() >= 1024


def test_workspace_helper(lib):
    l, _ = lib
    ws = l.lgcn_roi_ws_elems
    assert ws(0, 0, 0, 0, 0) >= 0 and ws(-1, 0, 0, 0, 0) == EINVAL and ws(0, 0, 0, 0, -1) == EINVAL
    base = ws(1000, 100, 20000, 2000, 20)
    assert base >= 2 * 14 * 1000 + 2 * 100 + 2 * 1000 + 20000 + 20 + 2 * 2000
    for bigger in ((1001, 100, 20000, 2000, 20), (1000, 101, 20000, 2000, 20), (1000, 100, 20004, 2000, 20),
                   (1000, 100, 20000, 2004, 20), (1000, 100, 20000, 2000, 24)):
        assert ws(*bigger) >= base
    assert ws(1 << 30, 0, 0, 0, 0) == ESHAPE and ws(0, 0, 1 << 40, 0, 0) == ESHAPE


def _job(mod, n_lanes=(3, 2), n_agents=(2, 1), n_nodes=(10, 7)):
    """A two-scene lgcn_roi_t over placeholder device pointers (nothing is launched on a refused call)."""
    S = len(n_lanes)
    cs = lambda x: np.concatenate([[0], np.cumsum(x)])
    off = np.concatenate([cs(n_nodes), cs(n_lanes), cs(n_agents), cs([a * l for a, l in zip(n_agents, n_lanes)]),
                          cs([2] * S), cs([1] * S), cs([3] * (14 * S))]).astype(np.int32)
    p = mod.Roi()
    p.n_scenes, p.n_agents, p.n_nodes, p.n_lanes = S, sum(n_agents), sum(n_nodes), sum(n_lanes)
    p.n_edges, p.n_slots, p.n_suc, p.n_pre = 3 * 14 * S, int(off[4 * S + 3]), 2 * S, S
    p.horizon_buffer = 20.0
    p.off_host = off.ctypes.data
    for name, _ in mod.Roi._fields_[15:]:
        setattr(p, name, 256)
    return p, off


def test_bad_arguments_are_refused_before_any_launch(lib):
    l, mod = lib
    calls = (l.lgcn_roi_search, l.lgcn_roi_nodes, l.lgcn_roi_edge_count, l.lgcn_roi_edge_fill)
    for f in calls:
        assert f(None, None) == EINVAL
        assert f(C.byref(mod.Roi()), None) == 0                       # an empty batch: nothing to do
    for field in ("n_scenes", "n_agents", "n_nodes", "n_edges", "n_rois", "n_out_nodes", "n_out_edges", "n_out_a2m"):
        p, off = _job(mod)
        setattr(p, field, -1)
        assert all(f(C.byref(p), None) == EINVAL for f in calls), field
    p, off = _job(mod)
    p.off_host = None
    assert l.lgcn_roi_search(C.byref(p), None) == EINVAL
    for at, val in ((0, 1), (1, -1), (2, 16)):                          # not from 0, decreasing, wrong total
        p, off = _job(mod)
        off[at] = val
        assert l.lgcn_roi_search(C.byref(p), None) == EINVAL, (at, val)
    p, off = _job(mod)
    off[-1] += 1                                                        # edge table ends past n_edges
    assert l.lgcn_roi_edge_count(C.byref(p), None) == EINVAL
    p, off = _job(mod)
    off[3 * 3 + 1] += 1                                                 # slots of scene 0 != agents * lanes
    assert l.lgcn_roi_search(C.byref(p), None) == EINVAL
    p, off = _job(mod, n_lanes=(4097, 2))
    assert all(f(C.byref(p), None) == ESHAPE for f in calls)            # above the lane cap
    p, off = _job(mod, n_lanes=(4096, 2))
    p.ws = None
    assert l.lgcn_roi_search(C.byref(p), None) == EINVAL                # at the cap: the next check answers
    for field in ("off_dev", "ws", "ctrs", "lane_idcs", "a_feats", "edge_u", "agent_nodes", "agent_vel"):
        p, off = _job(mod)
        setattr(p, field, None)
        assert l.lgcn_roi_search(C.byref(p), None) == EINVAL, field
    for field, rc in (("ws", EALIGN), ("ctrs", EALIGN), ("a_ctrs", EALIGN), ("lane_idcs", None), ("edge_v", None)):
        p, off = _job(mod)
        setattr(p, field, 264 if rc else 258)
        assert l.lgcn_roi_search(C.byref(p), None) == EALIGN, field
    p, off = _job(mod)
    p.n_rois, p.n_out_nodes, p.n_out_edges, p.n_out_a2m = 2, 12, 5, 3
    for f, field in ((l.lgcn_roi_nodes, "roi_base"), (l.lgcn_roi_nodes, "node_mask"), (l.lgcn_roi_edge_count, "edge_cnt"),
                     (l.lgcn_roi_edge_fill, "edge_base"), (l.lgcn_roi_edge_fill, "out_v"), (l.lgcn_roi_edge_fill, "a2m_v")):
        keep = getattr(p, field)
        setattr(p, field, None)
        assert f(C.byref(p), None) == EINVAL, field
        setattr(p, field, keep)
    p.node_mask = 260
    assert l.lgcn_roi_nodes(C.byref(p), None) == EALIGN
    p.node_mask, p.horizon_buffer = 256, float("nan")
    assert l.lgcn_roi_nodes(C.byref(p), None) == EINVAL


def test_public_interface_refuses_to_run_without_a_gpu():
    import lanegcn_amd  # noqa: F401
    from lanegcn_amd import data as gen
    from lanegcn_amd import data_lrcnn, ops
    from lanegcn_amd._lib import LgcnError
    assert list(inspect.signature(data_lrcnn.generate_lane_roi).parameters) == ["data", "horizon_buffer", "max_vel_threshold"]
    sig = inspect.signature(data_lrcnn.generate_lane_roi_batch)
    assert list(sig.parameters) == ["scenes", "horizon_buffer", "device"] and sig.parameters["device"].default is False
    assert sig.parameters["horizon_buffer"].default == 20.0
    scene = gen.synth_lane_scene(np.random.default_rng(0), [2], 3)
    assert scene["graph"]["pre_pairs"].shape[1] == 2 and scene["obs_trajs"].shape == (3, 20, 3)
    if torch.cuda.is_available():
        return          # with a GPU the calls run: tests/test_gpu_lane_roi.py
    with pytest.raises(LgcnError):
        data_lrcnn.generate_lane_roi(scene)
    with pytest.raises(LgcnError):
        data_lrcnn.generate_lane_roi_batch([scene], device=True)
    with pytest.raises(LgcnError):                                      # the wrappers take device tensors only
        ops.RoiJob({k: torch.zeros(0) for k in ("ctrs",)}, np.zeros(7, np.int32), 20.0)
