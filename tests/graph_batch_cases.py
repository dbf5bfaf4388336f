"""The crafted batch of the batched graph construction (csrc/lgcn_graphbatch.hip): five scenes, in this order, each a
relation {"u", "v"} (row u, column v) over n nodes.  tests/test_graph_batch_cases_host.py proves on the host that they are
what they claim; tests/test_gpu_graph_batch.py runs them as one batch (as `pre`, and transposed as `suc`)."""
import numpy as np

NUM_SCALES = 6


def _case(name, n, u, v):
    return {"name": name, "n": int(n), "u": np.asarray(u, np.int64).reshape(-1), "v": np.asarray(v, np.int64).reshape(-1)}


def cases():
    out = []
    # 1. two lanes of 3 nodes: scale 1 has 2 edges, every later scale is empty
    out.append(_case("two_lanes", 6, [1, 2, 4, 5], [0, 1, 3, 4]))
    # 2. one node and no edge: an empty scene in the middle of the batch
    out.append(_case("one_node", 1, [], []))
    # 3. a 5-cycle: never empty at any scale
    out.append(_case("cycle5", 5, np.arange(5), (np.arange(5) + 1) % 5))
    # 4. the random multigraph of test_gpu_graphgen.py (duplicates, self loops): rows grow to hundreds of entries
    rng = np.random.default_rng(12)
    n, m = 203, 700
    u, v = rng.integers(0, n, m), rng.integers(0, n, m)
    out.append(_case("multigraph", n, u, v))
    # 5. a 700-node chain (rows cross workgroups); node 400 is a second way from 102 to 100, so 102 reaches 100 twice in
    #    two steps (the duplicate must go); the edge (5, 700) points outside the scene
    i = np.arange(699)
    out.append(_case("chain_diamond", 700, np.concatenate([i + 1, [102, 400, 5]]), np.concatenate([i, [400, 100, 700]])))
    return out


def inside(c):
    """The case without the edges that leave [0, n): what both device paths keep."""
    ok = (c["u"] >= 0) & (c["u"] < c["n"]) & (c["v"] >= 0) & (c["v"] < c["n"])
    return {"u": c["u"][ok], "v": c["v"][ok]}


def transposed(c):
    return dict(c, u=c["v"], v=c["u"])


def offsets(sizes):
    return np.concatenate([[0], np.cumsum(np.asarray(sizes, np.int64), dtype=np.int64)])
