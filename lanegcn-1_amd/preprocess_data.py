"""Graph construction on the GPU: the two producers of the lane relations the hot path
consumes, behind the reference's function names.

  preprocess(graph, cross_dist, cross_angle=None)   reference preprocess_data.py:287-392: left / right node adjacency of
      one scene from the lane-level left / right / pre / suc pairs (dense N x N distance + lane-pair mask + row argmin
      + 6 m and pi / 4 tests there; one wave per node here, lgcn_cross_edges).
  dilated_nbrs(nbr, num_nodes, num_scales)          reference data.py:520-534: A^(2^i) by repeated boolean squaring
      (lgcn_bool_square*), device tensors in and out.
  dilated_nbrs_batch(nbrs, num_nodes, num_scales), preprocess_batch(graphs, cross_dist, cross_angle=None, device=False)
      the same for S scenes at once (csrc/lgcn_graphbatch.hip): per scene what the two functions above return, from a
      number of launches and host reads that does not depend on S.

All need CUDA tensors (no CPU fallback).  `cross_angle`: the reference's optional sector test reads a module global
`config` (preprocess_data.py:310-312) that the module never defines -- `config` is a local of its main() (:44) -- so
passing it raises NameError there; it raises the same here, and the reference's own call (:250) never passes it.
"""
from typing import Dict

import numpy as np
import torch

from . import _lib as L
from . import ops


def dilated_nbrs(nbr: Dict, num_nodes: int, num_scales: int):
    u, v = torch.as_tensor(nbr["u"]), torch.as_tensor(nbr["v"])
    if not (u.is_cuda and v.is_cuda):
        raise L.LgcnError("dilated_nbrs: the HIP path needs CUDA tensors (host arrays: lanegcn_amd.data.dilated_nbrs)")
    return ops.dilated_nbrs(u.long(), v.long(), int(num_nodes), int(num_scales))


def preprocess(graph: Dict, cross_dist: float, cross_angle=None) -> Dict:
    """Same inputs and outputs as the reference: graph holds ctrs, feats [N,2], lane_idcs [N], pre_pairs, suc_pairs,
    left_pairs, right_pairs [k,2] (LongTensors on the GPU, as after to_long(gpu(.))) and idx; returns
    {"left": {"u", "v"}, "right": {"u", "v"}, "idx"} with int16 numpy index arrays."""
    if cross_angle is not None:        # as the reference: its branch dies on an undefined global (see the module docstring)
        raise NameError("name 'config' is not defined")
    lane_idcs = graph["lane_idcs"]
    if not (torch.is_tensor(lane_idcs) and lane_idcs.is_cuda):
        raise L.LgcnError("preprocess: the HIP path needs CUDA tensors (no CPU fallback)")
    num_lanes = int(lane_idcs[-1].item()) + 1                      # :292
    out = {}
    for side in ("left", "right"):
        pairs = graph[side + "_pairs"]
        if len(pairs) > 0:                                         # :317 / :355
            u, v = ops.cross_edges(graph["ctrs"], graph["feats"], lane_idcs, num_lanes, pairs, graph["pre_pairs"],
                                   graph["suc_pairs"], cross_dist)
            out[side] = {"u": u.cpu().numpy().astype(np.int16), "v": v.cpu().numpy().astype(np.int16)}
        else:
            out[side] = {"u": np.zeros(0, np.int16), "v": np.zeros(0, np.int16)}
    out["idx"] = graph["idx"]
    return out


def _csum(sizes):
    return np.concatenate([[0], np.cumsum(np.asarray(sizes, np.int64), dtype=np.int64)])


def dilated_nbrs_batch(nbrs, num_nodes, num_scales: int):
    """dilated_nbrs for S scenes at once (ops.dilate_batch: every scale is one squaring of the whole batch and one host
    read).  nbrs: S {"u", "v"} dicts of device tensors, num_nodes: S ints.  Returns S lists of num_scales - 1 {"u", "v"}
    dicts (int64 device tensors): for every scene what dilated_nbrs returns for it."""
    us = [torch.as_tensor(n["u"]) for n in nbrs]
    vs = [torch.as_tensor(n["v"]) for n in nbrs]
    if not all(t.is_cuda for t in us + vs):
        raise L.LgcnError("dilated_nbrs_batch: the HIP path needs CUDA tensors (host arrays: lanegcn_amd.data.dilated_nbrs)")
    S = len(us)
    if S == 0:
        return []
    if len(num_nodes) != S or any(len(u) != len(v) for u, v in zip(us, vs)):
        raise L.LgcnError("dilated_nbrs_batch: one num_nodes per scene, and u and v of equal length")
    off = _csum([len(u) for u in us])
    none = us[0].new_empty(0, dtype=torch.int64)
    scales = ops.dilate_batch(torch.cat([u.reshape(-1).long() for u in us]), torch.cat([v.reshape(-1).long() for v in vs]),
                              none, none, _csum([int(n) for n in num_nodes]), off, np.zeros(S + 1, np.int64), int(num_scales))
    out = [[] for _ in range(S)]
    for sc in scales:
        sizes = np.diff(sc["pre_off"]).tolist()
        for b, (u, v) in enumerate(zip(sc["pre_u"].split(sizes), sc["pre_v"].split(sizes))):
            out[b].append({"u": u, "v": v})
    return out


def preprocess_batch(graphs, cross_dist: float, cross_angle=None, device: bool = False):
    """preprocess for S scenes at once (ops.cross_edges_batch: both sides of all scenes in the same launches).  graphs: S
    graph dicts as preprocess takes them.  Returns S dicts {"left", "right", "idx"}; the leaves are int16 numpy arrays,
    or with device=True int16 device tensors (then nothing is copied to the host).  Two host reads per batch: the scenes'
    lane counts (their last lane_idcs entry, as preprocess reads it) and the edge counts."""
    if cross_angle is not None:        # as preprocess
        raise NameError("name 'config' is not defined")
    graphs = list(graphs)
    for g in graphs:
        if not (torch.is_tensor(g["lane_idcs"]) and g["lane_idcs"].is_cuda):
            raise L.LgcnError("preprocess_batch: the HIP path needs CUDA tensors (no CPU fallback)")
    S = len(graphs)
    if S == 0:
        return []
    if any(len(g["lane_idcs"]) == 0 for g in graphs):
        raise L.LgcnError("preprocess_batch: a scene without a node has no lane count")
    last = ops.read_back(torch.stack([g["lane_idcs"][-1] for g in graphs]))      # :292, for every scene
    pairs = {k: [g[k + "_pairs"].reshape(-1, 2) for g in graphs] for k in ("pre", "suc", "left", "right")}
    edges, offs = ops.cross_edges_batch(
        torch.cat([g["ctrs"] for g in graphs]), torch.cat([g["feats"] for g in graphs]),
        torch.cat([g["lane_idcs"] for g in graphs]), *[torch.cat(pairs[k]) for k in pairs],
        _csum([len(g["lane_idcs"]) for g in graphs]), _csum(last.astype(np.int64) + 1),
        *[_csum([len(x) for x in pairs[k]]) for k in pairs], cross_dist)
    return split_cross(edges, offs, [g["idx"] for g in graphs], device)


def split_cross(edges, offs, idx, device):
    """Per-scene {"left", "right", "idx"} dicts out of the flat result of ops.cross_edges_batch."""
    out = [{"idx": i, "left": {}, "right": {}} for i in idx]
    for side in ("left", "right"):
        off = offs[side + "_off"]
        for c in "uv":
            x = edges[side + "_" + c]
            cut = x.split(np.diff(off).tolist()) if device else np.split(x.cpu().numpy(), off[1:-1])
            for o, part in zip(out, cut):
                o[side][c] = part
    return out
