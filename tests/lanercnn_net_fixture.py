"""Loader of tests/golden/lanercnn_net_b3.npz (the reference's own subgraph_gather, graph_gather and Net.forward on three
synthetic scenes with lane RoIs, written by tests/golden/make_golden_lanercnn_net.py) -- TEST INFRASTRUCTURE ONLY."""
import copy
import json
import os

import numpy as np

from golden_io import load_scenes

GOLDEN_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
POOLS = ("roi2graph", "graph2roi", "lane_pool")
REL_KEYS = [("pre", i) for i in range(6)] + [("suc", i) for i in range(6)] + [("left", None), ("right", None)]
HOST_KEYS = ("num_nodes", "counts", "batch_spans", "num_atgs_per_batch", "roi_spans", "interest_roi")
_cache = {}


def fixture():
    """(arrays by key, {"net": state_dict names and shapes, "config": the reference's config keys})."""
    if "fx" not in _cache:
        with np.load(os.path.join(GOLDEN_DIR, "lanercnn_net_b3.npz")) as z:
            g = {k: z[k] for k in z.files}
        _cache["fx"] = (g, json.load(open(os.path.join(GOLDEN_DIR, "lanercnn_net_state_names.json"))))
    return _cache["fx"]


def scenes():
    """The fixture's scenes as numpy trees (a fresh copy per call), scalars back to Python numbers."""
    if "scenes" not in _cache:
        out = load_scenes(fixture()[0])
        for s in out:
            s["theta"] = float(s["theta"])
            for sg in s["subgraphs"]:
                sg["num_nodes"], sg["agent_vel"] = int(sg["num_nodes"]), np.float32(sg["agent_vel"])
        _cache["scenes"] = out
    return copy.deepcopy(_cache["scenes"])


def rel(graph, k1, i):
    return graph[k1] if i is None else graph[k1][i]


def rel_name(k1, i):
    return k1 if i is None else "%s/%d" % (k1, i)


def host_value(g, key):
    """An entry of the reference's host bookkeeping as the Python value the reference holds."""
    v = g["sub/host/" + key]
    return int(v) if v.ndim == 0 else v.tolist()
