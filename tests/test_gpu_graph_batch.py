"""GPU: graph construction for a whole batch of scenes (csrc/lgcn_graphbatch.hip) against the reference's recordings and
against the per-scene device path, element for element: every output is an integer array, so every comparison is exact,
order and dtype included."""
import copy
import os

import numpy as np
import pytest
import torch

import lanegcn_amd  # noqa: F401
import graph_batch_cases as GC
import scene_build_cases as C
import scene_build_compare as K
import scene_build_model as M
from conftest import GOLDEN_DIR
from golden_io import load_scenes

pytestmark = pytest.mark.gpu
SCENE_GOLDEN = os.path.join(GOLDEN_DIR, "scene_build_b4.npz")
GRAPH_KEYS = ("ctrs", "feats", "lane_idcs", "pre_pairs", "suc_pairs", "left_pairs", "right_pairs")


def cuda(x):
    return torch.from_numpy(np.ascontiguousarray(x)).cuda()


def same(a, b, what):
    """Two index arrays (device tensor or numpy): same dtype, same length, same elements in the same order."""
    a, b = K.host(a), K.host(b)
    assert a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a, b), (what, a.dtype, b.dtype, a.shape, b.shape)


# ------------------------------------------------------------------ dilation
def test_dilation_golden_scenes_as_one_batch(golden):
    """The four fixture scenes as one batch: the reference's recorded dil/{i}/{pre,suc}/{1..5} edge sets, 40 arrays, and
    the emitted order is (u, v)-sorted."""
    from lanegcn_amd import preprocess_data as P
    scenes = load_scenes(golden)
    nums = [int(sc["graph"]["num_nodes"]) for sc in scenes]
    seen = 0
    for k1 in ("pre", "suc"):
        nbrs = [{k: cuda(np.asarray(v, np.int64)) for k, v in sc["graph"][k1][0].items()} for sc in scenes]
        got = P.dilated_nbrs_batch(nbrs, nums, 6)
        assert len(got) == len(scenes) == 4
        for i, per_scene in enumerate(got):
            assert len(per_scene) == 5
            for j, e in enumerate(per_scene):
                assert e["u"].dtype == torch.int64 and e["u"].is_cuda and e["v"].dtype == torch.int64
                uv = np.stack([K.host(e["u"]), K.host(e["v"])], 1)
                assert np.array_equal(uv, golden["dil/%d/%s/%d" % (i, k1, j + 1)]), (i, k1, j + 1)     # sorted as emitted
                seen += 1
    assert seen == 40


@pytest.fixture(scope="module")
def crafted():
    """The crafted batch and, computed once, the per-scene device path's answer for every scene and both relations."""
    from lanegcn_amd import preprocess_data as P
    cs = GC.cases()
    rel = {"pre": cs, "suc": [GC.transposed(c) for c in cs]}
    want = {k: [P.dilated_nbrs({"u": cuda(c["u"]), "v": cuda(c["v"])}, c["n"], GC.NUM_SCALES) for c in v] for k, v in rel.items()}
    return cs, rel, want


def test_dilation_crafted_batch_equals_per_scene(crafted):
    from lanegcn_amd import ops
    cs, rel, want = crafted
    flat = {k: (cuda(np.concatenate([c["u"] for c in v])), cuda(np.concatenate([c["v"] for c in v]))) for k, v in rel.items()}
    off = {k: GC.offsets([len(c["u"]) for c in v]) for k, v in rel.items()}
    got = ops.dilate_batch(*flat["pre"], *flat["suc"], GC.offsets([c["n"] for c in cs]), off["pre"], off["suc"], GC.NUM_SCALES)
    assert len(got) == GC.NUM_SCALES - 1
    for j, sc in enumerate(got):
        for k in ("pre", "suc"):
            o = sc[k + "_off"]
            assert o.shape == (len(cs) + 1,) and o[0] == 0 and o[-1] == len(sc[k + "_u"]) == len(sc[k + "_v"])
            for b, c in enumerate(cs):
                w = want[k][b][j]
                for x in "uv":
                    g = sc[k + "_" + x][o[b]:o[b + 1]]
                    assert g.is_cuda
                    same(g, w[x], (c["name"], k, j + 1, x))
                if c["name"] == "one_node" or (c["name"] == "two_lanes" and j >= 1):
                    assert o[b + 1] == o[b] and len(w["u"]) == 0, (c["name"], k, j + 1)            # empty results are empty
                if c["name"] in ("cycle5", "chain_diamond", "multigraph"):
                    assert o[b + 1] > o[b], (c["name"], k, j + 1)
    # the rows of the multigraph did grow to hundreds of entries
    sc, o = got[3], got[3]["pre_off"]
    assert np.bincount(K.host(sc["pre_u"][o[3]:o[4]])).max() > 100


def test_dilated_nbrs_batch_equals_per_scene(crafted):
    from lanegcn_amd import preprocess_data as P
    cs, rel, want = crafted
    scales = 4                   # the flat op above went to 6; the scales are prefixes of one another
    got = P.dilated_nbrs_batch([{"u": cuda(c["u"]), "v": cuda(c["v"])} for c in cs], [c["n"] for c in cs], scales)
    assert len(got) == len(cs)
    for b, c in enumerate(cs):
        assert len(got[b]) == scales - 1
        for j in range(scales - 1):
            for x in "uv":
                same(got[b][j][x], want["pre"][b][j][x], (c["name"], j + 1, x))


# ------------------------------------------------------------------ left / right
def b6_graphs():
    with np.load(os.path.join(GOLDEN_DIR, "graphgen_b6.npz")) as z:
        z = {k: z[k] for k in z.files}
    graphs = []
    for i in range(int(z["n_scenes"])):
        g = {k: cuda(z["g%d/%s" % (i, k)]) for k in GRAPH_KEYS}
        g["idx"] = i
        graphs.append(g)
    return z, graphs


def test_left_right_six_topologies_as_one_batch():
    """The reference's recorded u / v of the six fixture topologies, element for element: ties, the empty-side branch, a
    scene without any edge within 6 m, a one-lane scene.  No row is excluded."""
    from lanegcn_amd import preprocess_data as P
    z, graphs = b6_graphs()
    got = P.preprocess_batch(graphs, float(z["cross_dist"]))
    assert len(got) == 6
    for i, out in enumerate(got):
        assert out["idx"] == i
        for side in ("left", "right"):
            for c in "uv":
                assert isinstance(out[side][c], np.ndarray)
                same(out[side][c], z["g%d/%s/%s" % (i, side, c)].astype(np.int16), (i, side, c))
    dev = P.preprocess_batch(graphs, float(z["cross_dist"]), device=True)
    for i, out in enumerate(dev):
        for side in ("left", "right"):
            for c in "uv":
                assert torch.is_tensor(out[side][c]) and out[side][c].is_cuda and out[side][c].dtype == torch.int16
                same(out[side][c], got[i][side][c], (i, side, c))
    with pytest.raises(NameError):
        P.preprocess_batch(graphs, 6.0, cross_angle=0.5)


def test_left_right_scenes_do_not_see_each_other():
    """A topology next to a copy of itself, 0.36 m away, with the same lane numbering: a neighbour from the other scene
    would be nearer than any of the scene's own."""
    from lanegcn_amd import preprocess_data as P
    z, graphs = b6_graphs()
    g = graphs[1]
    twin = dict(g, ctrs=g["ctrs"] + torch.tensor([0.3, 0.2], device="cuda"), idx=1)
    g = dict(g, idx=0)
    got = P.preprocess_batch([g, twin], 6.0)
    for b, one in enumerate((g, twin)):
        want = P.preprocess(one, 6.0)
        assert len(want["left"]["u"]) > 0 and len(want["right"]["u"]) > 0
        for side in ("left", "right"):
            for c in "uv":
                same(got[b][side][c], want[side][c], (b, side, c))


def test_left_right_random_topologies_equal_per_scene():
    """The four random topologies of test_preprocess_random_topologies_vs_oracle (same generator, seed 8) as one batch
    against the per-scene device preprocess: device against device needs no heading-margin exclusion."""
    from lanegcn_amd import preprocess_data as P
    rng = np.random.default_rng(8)
    graphs = []
    for trial in range(4):
        n, nl = int(rng.integers(40, 400)), int(rng.integers(3, 30))
        lane = np.sort(rng.integers(0, nl, n))
        lane[-1] = nl - 1
        g = dict(ctrs=np.round(rng.normal(0, 8, (n, 2)), 1).astype(np.float32),
                 feats=rng.normal(0, 1, (n, 2)).astype(np.float32), lane_idcs=lane.astype(np.int64),
                 pre_pairs=rng.integers(0, nl, (int(rng.integers(0, 40)), 2)).astype(np.int64),
                 suc_pairs=rng.integers(0, nl, (int(rng.integers(0, 40)), 2)).astype(np.int64),
                 left_pairs=rng.integers(0, nl, (int(rng.integers(1, 30)), 2)).astype(np.int64),
                 right_pairs=rng.integers(0, nl, (int(rng.integers(1, 30)), 2)).astype(np.int64))
        graphs.append(dict({k: cuda(v) for k, v in g.items()}, idx=trial))
    got = P.preprocess_batch(graphs, 6.0)
    n_edges = 0
    for b, g in enumerate(graphs):
        want = P.preprocess(g, 6.0)
        for side in ("left", "right"):
            for c in "uv":
                same(got[b][side][c], want[side][c], (b, side, c))
            n_edges += len(want[side]["u"])
    assert n_edges > 0


# ------------------------------------------------------------------ build_scenes(batched=True)
@pytest.fixture(scope="module")
def batch5():
    """The five-scene, two-city batch of test_gpu_scene_build.py."""
    raws, tables, lane_ids, _ = C.load_fixture(SCENE_GOLDEN)
    raws, lane_ids = raws + [C.extra_scene(9)], lane_ids + [None]
    return raws, {k: v.to("cuda") for k, v in tables.items()}, lane_ids


@pytest.mark.parametrize("device", [True, False])
@pytest.mark.parametrize("cross", [True, False])
def test_build_scenes_batched_equals_per_scene(batch5, device, cross):
    from lanegcn_amd import data_raw as D
    raws, tables, lane_ids = batch5
    want = D.build_scenes(copy.deepcopy(raws), tables, C.CONFIG, device=device, cross=cross, lane_ids=lane_ids)
    got = D.build_scenes(copy.deepcopy(raws), tables, C.CONFIG, device=device, cross=cross, lane_ids=lane_ids, batched=True)
    assert len(got) == len(want) == 5
    for b, (g, w) in enumerate(zip(got, want)):
        K.assert_same_bits(g, w, "scene %d" % b)
        leaf = g["graph"]["pre"][5]["u"]
        assert (torch.is_tensor(leaf) and leaf.is_cuda and leaf.dtype == torch.int64) if device else leaf.dtype == np.int64
        assert len(g["graph"]["pre"]) == len(g["graph"]["suc"]) == 6 and ("left" in g["graph"]) == cross
        if cross:
            leaf = g["graph"]["left"]["u"]
            assert (torch.is_tensor(leaf) and leaf.is_cuda and leaf.dtype == torch.int16) if device else leaf.dtype == np.int16


def test_build_scenes_batched_equals_the_model(batch5):
    """Scenes 0 and 1 with host leaves against the host model, the pair the per-scene host-leaves test checks."""
    from lanegcn_amd import data_raw as D
    raws, tables, lane_ids = batch5
    pick = [0, 1]
    want = M.build_scenes([copy.deepcopy(raws[b]) for b in pick], tables, C.CONFIG, [lane_ids[b] for b in pick], cross=True)
    got = D.build_scenes([copy.deepcopy(raws[b]) for b in pick], tables, C.CONFIG, device=False, lane_ids=[lane_ids[b] for b in pick],
                         batched=True)
    for b, (g, w) in enumerate(zip(got, want)):
        K.assert_same_bits(g, w, "scene %d" % b)


WRAPPED = (("ops", "scene_tracks"), ("ops", "scene_lanes_rank"), ("ops", "scene_lanes_fill"), ("ops", "dilate_batch"),
           ("ops", "cross_edges_batch"), ("ops", "read_back"), ("preprocess_data", "dilated_nbrs"), ("preprocess_data", "preprocess"))


@pytest.fixture
def calls(monkeypatch):
    from lanegcn_amd import ops, preprocess_data
    mods, seen = {"ops": ops, "preprocess_data": preprocess_data}, []
    for mod, name in WRAPPED:
        real = getattr(mods[mod], name)
        monkeypatch.setattr(mods[mod], name, lambda *a, _real=real, _name=name, **k: (seen.append(_name), _real(*a, **k))[1])
    return seen


def test_build_scenes_batched_budget(batch5, calls):
    """No per-scene call, each flat op once, and a number of read-backs that does not depend on the number of scenes."""
    from lanegcn_amd import data_raw as D
    raws, tables, lane_ids = batch5
    num_scales = int(C.CONFIG["num_scales"])
    for n in (2, 5):
        del calls[:]
        D.build_scenes(copy.deepcopy(raws[:n]), tables, C.CONFIG, lane_ids=lane_ids[:n], batched=True)
        assert "dilated_nbrs" not in calls and "preprocess" not in calls
        assert calls.count("dilate_batch") == 1 and calls.count("cross_edges_batch") == 1
        assert calls.count("read_back") == (num_scales - 1) + 1, (n, calls)
    del calls[:]
    D.build_scenes(copy.deepcopy(raws[:2]), tables, C.CONFIG, lane_ids=lane_ids[:2], batched=True, cross=False, device=False)
    assert calls.count("cross_edges_batch") == 0 and calls.count("read_back") == num_scales - 1
    del calls[:]
    D.build_scenes(copy.deepcopy(raws[:2]), tables, C.CONFIG, lane_ids=lane_ids[:2])
    assert calls.count("dilated_nbrs") == 4 and calls.count("preprocess") == 2 and "dilate_batch" not in calls


def test_build_scenes_batched_errors_come_first(batch5, calls):
    """The three errors raise the same messages with batched=True, with neither flat op called."""
    from lanegcn_amd import _lib, data_raw as D
    raws, tables, lane_ids = batch5
    bad = copy.deepcopy(raws[:3])
    bad[1]["steps"][3] = np.concatenate([bad[1]["steps"][3], bad[1]["steps"][3][:1]])
    bad[1]["trajs"][3] = np.concatenate([bad[1]["trajs"][3], bad[1]["trajs"][3][:1]])
    with pytest.raises(_lib.LgcnError, match="scene 1 track 3 lists a step twice"):
        D.build_scenes(bad, tables, C.CONFIG, batched=True)
    assert calls == ["scene_tracks", "scene_lanes_rank"]

    del calls[:]
    short = copy.deepcopy(raws[:3])
    short[2]["trajs"][0], short[2]["steps"][0] = short[2]["trajs"][0][:19], short[2]["steps"][0][:19]
    with pytest.raises(_lib.LgcnError, match="scene 2.*20 rows"):
        D.build_scenes(short, tables, C.CONFIG, batched=True)
    assert calls == []

    far = copy.deepcopy(raws[:3])
    far[2]["trajs"][0] = far[2]["trajs"][0] + 5000.0
    with pytest.raises(_lib.LgcnError, match="scene 2: no lane survives"):
        D.build_scenes(far, tables, C.CONFIG, batched=True)
    assert calls == ["scene_tracks", "scene_lanes_rank"]


def test_net_forward_is_bit_equal(batch5, ref_state_names):
    """Net.forward(collate_fn(build_scenes(...))) under no_grad: batched=True and batched=False give the same bits."""
    from lanegcn_amd import data as gen, data_raw as D, lanegcn as LG
    from oracle import lanegcn_oracle as O
    raws, tables, lane_ids = batch5
    net = LG.Net(LG.config)
    net.load_state_dict(O.seeded_state(ref_state_names, 13), strict=True)
    net = net.cuda().eval()
    keys = ("feats", "ctrs", "orig", "theta", "rot", "gt_preds", "has_preds", "graph")
    outs = []
    for batched in (True, False):
        scenes = D.build_scenes(copy.deepcopy(raws), tables, C.CONFIG, lane_ids=lane_ids, batched=batched)
        with torch.no_grad():
            outs.append(net(gen.collate_fn([{k: s[k] for k in keys} for s in scenes])))
    for k in ("cls", "reg"):
        for a, b in zip(outs[0][k], outs[1][k]):
            assert a.shape == b.shape and torch.equal(a, b), k
            assert torch.isfinite(a).all()
