"""CPU: the host tables of the flat lane-RoI route.  data_lrcnn.relation_major_tables (the edge_base of
lgcn_roi_edge_fill_graph and the per-relation extents) against a plain double loop over (relation, RoI), and
RoiBatch's host bookkeeping against lanercnn.subgraph_bookkeeping of the equivalent per-RoI lists."""
import numpy as np
import pytest
import torch

K = 14


@pytest.fixture(scope="module")
def mods():
    import lanegcn_amd  # noqa: F401
    from lanegcn_amd import data_lrcnn, lanercnn
    from lanegcn_amd._lib import LgcnError
    return data_lrcnn, lanercnn, LgcnError


def loop_tables(cnt):
    """Relation k of every RoI back to back in RoI order, then relation k + 1; a2m RoI-major in arrays of its own."""
    R = len(cnt)
    base = np.zeros((R, K + 1), np.int64)
    ext, at = [0], 0
    for k in range(K):
        for r in range(R):
            base[r, k] = at
            at += int(cnt[r][k])
        ext.append(at)
    at = 0
    for r in range(R):
        base[r, K] = at
        at += int(cnt[r][K])
    return base, np.asarray(ext, np.int64), at


def check(D, cnt):
    base, ext, n_a2m = D.relation_major_tables(cnt)
    wb, we, wa = loop_tables(cnt)
    assert base.dtype == np.int32 and base.shape == (len(cnt), K + 1) and base.flags["C_CONTIGUOUS"]
    assert ext.dtype == np.int64 and ext.shape == (K + 1,)
    assert np.array_equal(base, wb) and np.array_equal(ext, we) and n_a2m == wa and isinstance(n_a2m, int)


@pytest.mark.parametrize("seed", range(6))
def test_random_count_tables(mods, seed):
    D = mods[0]
    rng = np.random.default_rng(seed)
    R = int(rng.integers(2, 70))
    cnt = rng.integers(0, 900, (R, K + 1))
    cnt[:, rng.integers(0, K, 3)] = 0                            # relations without an edge in any RoI
    cnt[rng.integers(0, R, 2)] = 0                               # RoIs without an edge
    check(D, cnt)
    check(D, cnt.astype(np.int32))


def test_edge_cases(mods):
    D = mods[0]
    check(D, np.zeros((5, K + 1), np.int64))                     # nothing at all
    check(D, np.arange(K + 1)[None, :])                          # R = 1
    check(D, np.zeros((1, K + 1), np.int64))
    one = np.zeros((3, K + 1), np.int64)
    one[1, 7] = 4                                                # one relation of one RoI
    check(D, one)
    base, ext, n_a2m = D.relation_major_tables(np.zeros((0, K + 1), np.int64))
    assert base.shape == (0, K + 1) and not ext.any() and n_a2m == 0


def test_totals_around_int32(mods):
    D, _, LgcnError = mods
    lim = 2 ** 31 - 1
    cnt = np.zeros((2, K + 1), np.int64)
    cnt[0, 0], cnt[1, 0], cnt[0, 13], cnt[1, 13] = 2 ** 30, 2 ** 29, 2 ** 28, lim - 2 ** 30 - 2 ** 29 - 2 ** 28
    check(D, cnt)                                                # exactly 2^31 - 1 edges: every base fits int32
    assert int(D.relation_major_tables(cnt)[1][-1]) == lim
    cnt[1, 13] -= 1
    check(D, cnt)                                                # just under
    cnt[1, 13] += 2
    with pytest.raises(LgcnError, match="more than 2\\^31 - 1 edges"):      # just over: the existing error
        D.relation_major_tables(cnt)
    cnt = np.zeros((2, K + 1), np.int64)
    cnt[:, K] = 2 ** 30                                          # a2m alone passes the limit
    with pytest.raises(LgcnError, match="more than 2\\^31 - 1 edges"):
        D.relation_major_tables(cnt)


def roi_batch(D, rng, per_scene, n_agents):
    """A RoiBatch over host tables only (its device buffers are never touched by the bookkeeping) and the equivalent
    lists: scene b keeps per_scene[b] of its n_agents[b] agents."""
    agent_off = np.concatenate([[0], np.cumsum(n_agents)])
    agents = np.concatenate([agent_off[b] + np.sort(rng.choice(n_agents[b], per_scene[b], replace=False))
                             for b in range(len(per_scene))]).astype(np.int64)
    scene_of = np.repeat(np.arange(len(per_scene)), per_scene)
    sizes = rng.integers(6, 700, len(agents))
    cnt = rng.integers(0, 50, (len(agents), K + 1))
    _, ext, _ = D.relation_major_tables(cnt)
    rb = D.RoiBatch(None, None, None, None, None, None, None, sizes, scene_of, agents, agent_off,
                    rng.random(len(agents)).astype(np.float32), ext, cnt)
    lists, r = [], 0
    for n in per_scene:
        lists.append([{"feats": np.zeros((int(sizes[r + i]), 8), np.float32)} for i in range(n)])
        r += n
    return rb, lists, agents, agent_off


@pytest.mark.parametrize("per_scene, n_agents", [([3, 1, 5], [4, 1, 9]), ([1], [1]), ([2, 2], [2, 40]), ([60, 1], [72, 3])])
def test_bookkeeping_equals_the_list_route(mods, per_scene, n_agents):
    D, R, _ = mods
    rb, lists, agents, agent_off = roi_batch(D, np.random.default_rng(len(per_scene)), per_scene, n_agents)
    got, want = rb.bookkeeping(), R.subgraph_bookkeeping(lists)
    assert sorted(got) == sorted(want)
    for k in want:
        if torch.is_tensor(want[k]):
            assert got[k].dtype == want[k].dtype and torch.equal(got[k], want[k]), k
        else:
            assert got[k] == want[k], k
    assert all(type(v) is int for v in got["counts"]) and type(got["num_nodes"]) is int
    r = 0
    for b, n in enumerate(per_scene):
        ids = rb.valid_agent_ids(b)
        assert ids.dtype == np.int16 and np.array_equal(ids, agents[r:r + n] - agent_off[b])
        r += n


def test_a_scene_without_an_roi_is_refused(mods):
    D, _, LgcnError = mods
    cnt = np.zeros((2, K + 1), np.int64)
    ext = D.relation_major_tables(cnt)[1]
    args = (None,) * 7
    with pytest.raises(LgcnError, match="scene 1 has no lane RoI"):
        D.RoiBatch(*args, [6, 7], [0, 2], [0, 5], [0, 2, 4, 6], np.zeros(2, np.float32), ext, cnt)
    with pytest.raises(LgcnError, match="no scene in the batch"):
        D.RoiBatch(*args, [], [], [], [0], np.zeros(0, np.float32), ext, cnt[:0])
