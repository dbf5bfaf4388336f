"""CPU: lgcn_roi_edge_fill_graph (the lane-RoI fill that writes the merged batch graph) is exported, bound and declared,
and refuses bad arguments with the codes of its sibling lgcn_roi_edge_fill on the same malformed input.  Every call
here is refused by the host-side checks (or is an empty batch), so no kernel is launched."""
import ctypes as C
import os
import re

import pytest

from test_host_lane_roi_cabi import EALIGN, EINVAL, ESHAPE, _job

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "lgcn_roi_edge_fill_graph"
PTR = 256          # a placeholder device pointer, 8-byte aligned; never dereferenced by a refused call


@pytest.fixture(scope="module")
def lib():
    import lanegcn_amd  # noqa: F401
    from lanegcn_amd import _lib
    return _lib.load(), _lib


def both(l, p, a2m_u=PTR, a2m_v=PTR):
    """(code of the graph entry, code of the sibling) on the same struct."""
    ref = C.byref(p) if p is not None else None
    return l.lgcn_roi_edge_fill_graph(ref, a2m_u, a2m_v, None), l.lgcn_roi_edge_fill(ref, None)


def test_symbol_is_exported_bound_and_declared(lib):
    l, mod = lib
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "lgcn.h")).read(), flags=re.S)
    assert hasattr(l, NAME) and NAME in mod.SIGNATURES and re.search(r"\b%s\s*\(" % NAME, header)
    assert len(mod.SIGNATURES[NAME][1]) == 4                     # struct, a2m_u, a2m_v, stream
    assert C.sizeof(mod.Roi) == 14 * 4 + 29 * 8                  # lgcn_roi_t is unchanged
    import inspect
    from lanegcn_amd import ops
    assert list(inspect.signature(ops.roi_edge_fill_graph).parameters) == ["job", "edge_base", "n_out_edges", "n_out_a2m"]


def filled(mod):
    p, off = _job(mod)
    p.n_rois, p.n_out_nodes, p.n_out_edges, p.n_out_a2m = 2, 12, 5, 3
    return p, off


def test_null_struct_and_empty_batch(lib):
    l, mod = lib
    assert both(l, None) == (EINVAL, EINVAL)
    assert both(l, mod.Roi()) == (0, 0)                         # an empty batch: nothing to do
    assert both(l, mod.Roi(), None, None) == (0, 0)
    p, off = _job(mod)                                           # scenes, but no RoI: no output is needed
    p.edge_base = p.out_u = p.out_v = p.a2m_v = None
    assert both(l, p, None, None) == (0, 0)


def test_negative_counts(lib):
    l, mod = lib
    for field in ("n_scenes", "n_agents", "n_nodes", "n_edges", "n_rois", "n_out_nodes", "n_out_edges", "n_out_a2m"):
        p, off = filled(mod)
        setattr(p, field, -1)
        assert both(l, p) == (EINVAL, EINVAL), field


def test_null_outputs_with_nonzero_counts(lib):
    l, mod = lib
    for field in ("edge_base", "out_u", "out_v"):
        p, off = filled(mod)
        setattr(p, field, None)
        assert both(l, p) == (EINVAL, EINVAL), field
    # the int64 a2m_v of the entry stands where the sibling's int32 a2m_v stands; a2m_u is checked like it
    p, off = filled(mod)
    assert l.lgcn_roi_edge_fill_graph(C.byref(p), PTR, None, None) == EINVAL
    assert l.lgcn_roi_edge_fill_graph(C.byref(p), None, PTR, None) == EINVAL
    p.a2m_v = None
    assert l.lgcn_roi_edge_fill(C.byref(p), None) == EINVAL
    # the same tables and sizes are checked first
    p, off = filled(mod)
    off[-1] += 1                                                 # the edge table ends past n_edges
    assert both(l, p) == (EINVAL, EINVAL)
    p, off = _job(mod, n_lanes=(4097, 2))
    p.n_rois, p.n_out_nodes, p.n_out_edges, p.n_out_a2m = 2, 12, 5, 3
    assert both(l, p) == (ESHAPE, ESHAPE)


def test_misaligned_outputs(lib):
    l, mod = lib
    for field in ("out_u", "out_v"):
        p, off = filled(mod)
        setattr(p, field, PTR + 4)
        assert both(l, p) == (EALIGN, EALIGN), field
    p, off = filled(mod)
    assert l.lgcn_roi_edge_fill_graph(C.byref(p), PTR + 4, PTR, None) == EALIGN
    assert l.lgcn_roi_edge_fill_graph(C.byref(p), PTR, PTR + 4, None) == EALIGN
    p.a2m_v = PTR + 2                                            # the sibling's int32 array: 4-byte alignment
    assert l.lgcn_roi_edge_fill(C.byref(p), None) == EALIGN
