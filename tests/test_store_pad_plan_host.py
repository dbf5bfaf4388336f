"""CPU: the host half of the PADDED scene-store batch -- StoreCaps, the fit rule and plan_batch(..., caps=) against the
host model (store_pad_model: FlatSceneFile.batch over a store that also holds the filler scene)."""
import numpy as np
import pytest

from scene_store_cases import PICKS, make_scenes
from store_pad_model import padded_batch_host, pick_totals


@pytest.fixture(scope="module")
def split(tmp_path_factory):
    import lanegcn_amd  # noqa: F401
    from lanegcn_amd.flatfile import FlatSceneFile, write_scenes
    scenes = make_scenes()
    d = tmp_path_factory.mktemp("pad_plan")
    path = str(d / "split.npz")
    write_scenes(path, scenes)
    return scenes, FlatSceneFile(path), d


def _plan(f, pick, caps=None):
    from lanegcn_amd.flatfile import plan_batch
    a = f.a
    return plan_batch(a["node_off"], a["actor_off"], a["edge_off"], a["rel_off"], f.num_scales, pick, caps=caps)


def _caps(scenes, pick, dn=1, da=1, de=0):
    from lanegcn_amd.flatfile import StoreCaps
    n, a, e = pick_totals(scenes, pick)
    return StoreCaps(batch=len(pick), nodes=n + dn, actors=a + da, edges=tuple(x + de for x in e))


@pytest.mark.parametrize("name", sorted(PICKS))
@pytest.mark.parametrize("slack", [(1, 1, 0), (300, 5, 7)])
def test_padded_plan_matches_the_host_model(split, name, slack):
    scenes, f, d = split
    pick = PICKS[name]
    caps = _caps(scenes, pick, *slack)
    p = _plan(f, pick, caps)
    fb, ex = padded_batch_host(scenes, pick, caps, d)
    B, R = len(pick), 2 * f.num_scales + 2
    assert (p.n_scenes, p.n_nodes, p.n_actors, p.num_scales) == (B + 1, caps.nodes, caps.actors, f.num_scales)
    assert (fb.n_scenes, fb.n_nodes, fb.n_actors) == (B + 1, caps.nodes, caps.actors)
    assert p.n_edges == list(caps.edges) == fb.n_edges
    assert [tuple(map(tuple, s)) for s in p.rel_slices] == [tuple(map(tuple, s)) for s in fb.rel_slices]
    at = 0
    for r in range(R):                                  # the fixed blocks: u then v of relation r, caps.edges[r] each
        assert p.rel_slices[r] == ((at, at + caps.edges[r]), (at + caps.edges[r], at + 2 * caps.edges[r]))
        at += 2 * caps.edges[r]
    assert p.n_elem == at == 2 * sum(caps.edges)
    assert p.sizes == ex["sizes"] and len(p.sizes) == B + 1
    assert (p.cap_a2m, p.cap_a2a) == (fb.cap_a2m, fb.cap_a2a)
    n, a, e = pick_totals(scenes, pick)
    assert (p.real_nodes, p.real_actors, p.real_edges) == (n, a, e)
    assert np.array_equal(p.node_off, fb.node_off.numpy()) and np.array_equal(p.actor_off, fb.actor_off.numpy())
    assert np.array_equal(p.seg_off, fb.seg_off.numpy()) and np.array_equal(p.seg_base, fb.seg_base.numpy())
    # the table: the picked scenes' entries are those of the unpadded plan, the filler's sources are negative
    q = _plan(f, pick)
    B1, G1 = B + 1, 2 * R * (B + 1)
    assert p.table.size == 5 * B1 + 2 * G1 + 3
    src = p.table[2 * B1 + 2:5 * B1 + 2].reshape(3, B1)
    assert np.array_equal(src[:, :B], q.table[2 * B + 2:5 * B + 2].reshape(3, B)) and (src[:, B] == -1).all()
    seg_src = p.table[5 * B1 + G1 + 3:].reshape(2 * R, B1)
    assert np.array_equal(seg_src[:, :B], q.table[5 * B + 2 * R * B + 3:].reshape(2 * R, B)) and (seg_src[:, B] == -1).all()
    assert int(p.node_off[B]) == n and int(p.actor_off[B]) == a


def test_fit_rule_at_its_edges(split):
    from lanegcn_amd._lib import LgcnError
    from lanegcn_amd.flatfile import StoreCaps, StoreFitError
    scenes, f, _ = split
    pick = PICKS["repeat"]
    n, a, e = pick_totals(scenes, pick)
    exact = _caps(scenes, pick)
    p = _plan(f, pick, exact)                                            # N + 1 == nodes, A + 1 == actors, E_r == edges[r]
    assert p.node_off[-1] - p.node_off[-2] == 1 and p.actor_off[-1] - p.actor_off[-2] == 1
    B1 = len(pick) + 1
    seg = np.diff(p.seg_off).reshape(-1, B1)
    assert (seg[:, -1] == 0).all()                                       # every filler segment is empty
    assert exact.misfit(len(pick), n, a, e) is None
    for bad, word in ((StoreCaps(len(pick), n, a + 1, tuple(e)), "nodes"), (StoreCaps(len(pick), n + 1, a, tuple(e)), "actors"),
                      (StoreCaps(len(pick), n + 1, a + 1, tuple(e[:3] + [e[3] - 1] + e[4:])), "relation 3"),
                      (StoreCaps(len(pick) + 1, n + 9, a + 9, tuple(e)), "scenes"),
                      (StoreCaps(len(pick) - 1, n + 9, a + 9, tuple(e)), "scenes")):
        with pytest.raises(StoreFitError) as err:
            _plan(f, pick, bad)
        assert word in str(err.value) and isinstance(err.value, LgcnError)


def test_caps_constructors(split):
    from lanegcn_amd.flatfile import StoreCaps
    scenes, f, _ = split
    rng = np.random.default_rng(5)
    picks = rng.integers(0, 6, (17, 4)).tolist()
    caps = StoreCaps.for_picks(f.a, picks)
    tot = [pick_totals(scenes, p) for p in picks]
    assert caps.batch == 4 and caps.nodes == max(t[0] for t in tot) + 1 and caps.actors == max(t[1] for t in tot) + 1
    assert caps.edges == tuple(max(t[2][r] for t in tot) for r in range(len(tot[0][2])))
    for p in picks:
        _plan(f, p, caps)                                                # every one of them fits
    a, b = StoreCaps.for_size(f.a, 4, draws=40, seed=3), StoreCaps.for_size(f.a, 4, draws=40, seed=3)
    assert a == b and a.batch == 4
    drawn = np.random.default_rng(3).integers(0, 6, (40, 4)).tolist()
    assert a == StoreCaps.for_picks(f.a, drawn)
    with pytest.raises(IndexError):
        StoreCaps.for_picks(f.a, [[0, 6]])


@pytest.mark.parametrize("name", sorted(PICKS))
def test_plans_without_caps_are_unchanged(split, name):
    """plan_batch without caps against the batch FlatSceneFile cuts: the fields of today's plan, and no real totals."""
    _, f, _ = split
    pick = PICKS[name]
    p = _plan(f, pick)
    fb, ex = f.batch(pick, device="cpu")
    assert (p.n_scenes, p.n_nodes, p.n_actors, p.n_edges) == (len(pick), fb.n_nodes, fb.n_actors, fb.n_edges)
    assert p.rel_slices == [tuple(map(tuple, s)) for s in fb.rel_slices] and p.sizes == ex["sizes"]
    assert (p.cap_a2m, p.cap_a2a) == (fb.cap_a2m, fb.cap_a2a)
    assert np.array_equal(p.seg_off, fb.seg_off.numpy()) and np.array_equal(p.node_off, fb.node_off.numpy())
    assert p.table.size == 5 * len(pick) + 2 * p.n_seg + 3 and (p.table >= 0).all()
    assert p.real_nodes is None and p.real_actors is None and p.real_edges is None
