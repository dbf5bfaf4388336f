"""GPU: the resident lane-RoI store -- data_lrcnn.RoiStore (from_inputs, from_store, concat, save / load, batch) with
lgcn_roi_store_gather, and lanercnn.Net.forward_store -- against the rebuild of the picked scenes alone
(data_lrcnn.lane_roi_flat, Net.forward_raw).  Integers and copied floats: every comparison is exact."""
import numpy as np
import pytest
import torch

import lanegcn_amd  # noqa: F401
import lane_roi_cases as C
import lanercnn_net_fixture as NF
import scene_build_cases as SC
from lanegcn_amd import data_lrcnn as D
from lanegcn_amd import data_raw
from lanegcn_amd import lanercnn as R
from lanegcn_amd._lib import LgcnError
from oracle.lanercnn_oracle import seeded_state

pytestmark = pytest.mark.gpu
RAW_SEED = 500          # every scene of golden_inputs(500) keeps an RoI (asserted below)
RAW_SEED_DROP = 1       # scene 2 of golden_inputs(1): its only agent drops (asserted below)
DEV_ARRAYS = ("feats", "node_mask", "agent_feat", "u", "v", "a2m_u", "a2m_v")
HOST_TABLES = ("sizes", "roi_base", "scene_of", "agent_vel", "rel_ext", "edge_cnt", "first_roi", "rois_per_scene")
ROW_KEYS = ("ctrs", "feats", "obs_trajs", "gt_preds", "has_preds")
ROW_TYPES = dict(ctrs=np.float32, feats=np.float32, obs_trajs=np.float32, gt_preds=np.float32, has_preds=bool)


# ------------------------------------------------------------------ the batches of test_gpu_roi_flat.py, re-stated
def one_roi_scene(n_par=2):
    rng = np.random.default_rng(21)
    b = C.Builder(rng)
    cp = b.chain((0.0, 0.0), 0.3, [7, 9, 5], n_par, spacing=2.0)
    g, new = b.graph(np.int32)
    return C.agents(rng, g, [(int(new[cp[0][1][2]]), 0.02, 6.0, 0.2)])


def no_side_scenes():
    """Two scenes of single chains: no left / right edge in any RoI."""
    rng = np.random.default_rng(22)
    out = []
    for sizes in ([6, 8, 7, 9], [12, 5, 10]):
        b = C.Builder(rng)
        cp = b.chain(rng.uniform(-10, 10, 2), 0.5, sizes, 1, spacing=2.0)
        g, new = b.graph(np.int64)
        out.append(C.agents(rng, g, [(int(new[cp[0][1][1]]), 0.02, 5.0, 0.2), (int(new[cp[0][2][0]]), -0.03, 9.0, -0.3)]))
    return out


def batches():
    return {"fixture": C.load_fixture()[0], "shuffle": C.trial(12), "dup_edges": C.trial(15), "no_side": no_side_scenes(),
            "one_roi": [one_roi_scene()], "standing_added": C.trial(16) + [C.standing_scene(np.random.default_rng(5), np.int16)]}


BATCHES = ("fixture", "shuffle", "dup_edges", "no_side", "one_roi", "standing_added")


@pytest.fixture(scope="module")
def cases():
    return batches()


def _rows(scenes):
    """The scenes' per-agent arrays, concatenated on the device."""
    return {k: torch.from_numpy(np.concatenate([np.asarray(s[k]).astype(ROW_TYPES[k], copy=False) for s in scenes])).cuda()
            for k in ROW_KEYS}


def _roi_inputs(scenes):
    t, off, _ = D._roi_inputs(scenes)
    return t, off, _rows(scenes)


def store_of(scenes):
    t, off, rows = _roi_inputs(scenes)
    return D.RoiStore.from_inputs(t, off, rows=rows)


def rebuild(scenes):
    t, off, _ = _roi_inputs(scenes)
    return D.lane_roi_flat(t, off)


def assert_batch_equals_rebuild(rois, scenes, pick, what, result=None, row_keys=ROW_KEYS):
    """rois.batch(pick) (or `result`, what it returned) against lane_roi_flat of the picked scenes alone, and the rows
    against the scenes' arrays at their valid_agent_ids."""
    got, rows = rois.batch(pick) if result is None else result
    want = rebuild([scenes[i] for i in pick])
    for k in DEV_ARRAYS:
        x, y = getattr(got, k), getattr(want, k)
        assert x.dtype == y.dtype and x.shape == y.shape and x.device == y.device and torch.equal(x, y), (what, pick, k)
    for k in HOST_TABLES:
        x, y = getattr(got, k), getattr(want, k)
        assert x.dtype == y.dtype and x.shape == y.shape and x.tobytes() == y.tobytes(), (what, pick, k)
    assert got.n_scenes == want.n_scenes == len(pick) and got.n_rois == want.n_rois
    assert np.array_equal(got.agents, np.arange(got.n_rois)) and np.array_equal(got.agent_off, got.first_roi)
    assert sorted(rows) == sorted(tuple(row_keys) + ("agent_ids",)) and len(rows["agent_ids"]) == len(pick)
    at = 0
    for j, i in enumerate(pick):
        ids = want.valid_agent_ids(j)
        n = len(ids)
        assert rows["agent_ids"][j].dtype == np.int16 and np.array_equal(rows["agent_ids"][j], ids), (what, pick, j)
        assert np.array_equal(got.valid_agent_ids(j), np.arange(n))
        for k in row_keys:
            w = np.asarray(scenes[i][k]).astype(ROW_TYPES[k], copy=False)[ids.astype(np.int64)]
            g = rows[k][at:at + n].cpu().numpy()
            assert g.dtype == w.dtype and g.shape == w.shape and g.tobytes() == w.tobytes(), (what, pick, j, k)
        at += n
    assert at == got.n_rois
    return got, want


def picks_of(rois):
    """A pick that starts at a scene other than 0, [2, 0, 2], all usable scenes reversed, and a single scene."""
    us = rois.usable().tolist()
    n = len(us)
    return [us[1:] if n > 1 else [us[0], us[0]], [us[2 % n], us[0], us[2 % n]], us[::-1], [us[-1]]]


# ------------------------------------------------------------------ 1: a pick equals the rebuild
@pytest.mark.parametrize("name", BATCHES)
def test_pick_equals_the_rebuild(cases, name):
    scenes = cases[name]
    rois = store_of(scenes)
    assert len(rois) == len(scenes) and rois.nbytes > 0 and rois.has_gt
    if name == "standing_added":
        last = len(scenes) - 1
        assert last not in rois.usable() and rois.rois_per_scene[last] == 0 and len(rois.usable()) == last
        with pytest.raises(LgcnError, match="scene %d has no lane RoI" % last):
            rois.batch([0, last])
    else:
        assert rois.usable().tolist() == list(range(len(scenes)))
    for pick in picks_of(rois):
        got, _ = assert_batch_equals_rebuild(rois, scenes, pick, name)
        if name == "no_side":                                     # segments that are empty everywhere, the table's last too
            assert got.rel_ext[13] == got.rel_ext[12] == got.rel_ext[14] and got.u.numel() > 0
    for k in ("edge_u", "edge_v", "a2m_u", "a2m_v", "node_mask"):
        assert rois._job.t[k].dtype == torch.int32             # resident indices: scene-local int32
    if rois.n_rois > 1:                                           # scene-local: no index reaches past the largest scene's block
        assert int(rois._job.t["edge_u"].max()) < np.diff(rois.node_off).max()
        assert int(rois._job.t["a2m_u"].max()) < rois.rois_per_scene.max()


# ------------------------------------------------------------------ 2: seams, and no element left unwritten
def poisoned_batch(rois, pick, monkeypatch):
    """rois.batch(pick) with every output buffer pre-filled with 0xA5 bytes."""
    real = torch.empty

    def empty(*a, **kw):
        x = real(*a, **kw)
        if x.is_cuda and x.numel():
            x.view(torch.uint8).fill_(0xA5)
        return x
    with monkeypatch.context() as m:
        m.setattr(torch, "empty", empty)
        return rois.batch(pick)


@pytest.mark.parametrize("name", ["wide", "crowd"])
def test_seams_of_large_rois_and_many_rois(name, monkeypatch):
    scenes = [one_roi_scene(), C.large_scene(name)]
    rois = store_of(scenes)
    if name == "wide":
        assert rois.sizes.max() > 512
    else:
        assert rois.n_rois >= 40 and rois.node_off[-1] > 10 * scenes[1]["graph"]["num_nodes"]
    for pick in ([0], [1], [1, 0]):
        # equal to the rebuild in every element, so no poison survives (0xA5A5A5A5 is an ordinary float, not a NaN)
        assert_batch_equals_rebuild(rois, scenes, pick, name, result=poisoned_batch(rois, pick, monkeypatch))


def test_more_segments_than_a_block_has_threads(monkeypatch):
    scenes = no_side_scenes() + [one_roi_scene()]
    rois = store_of(scenes)
    pick = [i % 3 for i in range(70)]
    assert 30 * len(pick) > 1024
    assert_batch_equals_rebuild(rois, scenes, pick, "70", result=poisoned_batch(rois, pick, monkeypatch))


# ------------------------------------------------------------------ 3: concat, chunk, save / load
def same_store(a, b, what):
    assert sorted(a._job.t) == sorted(b._job.t), what
    for k, x in a._job.t.items():
        y = b._job.t[k]
        assert x.dtype == y.dtype and x.shape == y.shape and torch.equal(x, y), (what, k)
    for k in ("first_roi", "node_off", "edge_off", "sizes", "agent_vel", "edge_cnt", "agent_ids"):
        x, y = getattr(a, k), getattr(b, k)
        assert x.dtype == y.dtype and x.shape == y.shape and x.tobytes() == y.tobytes(), (what, k)
    assert a.n_scenes == b.n_scenes and a.nbytes == b.nbytes and a.has_gt == b.has_gt


@pytest.fixture(scope="module")
def raw():
    raws, maps, lane_ids, _ = SC.golden_inputs(RAW_SEED)
    return raws, {c: data_raw.LaneTable.from_lanes(m) for c, m in maps.items()}, lane_ids


@pytest.fixture(scope="module")
def stores(raw):
    raws, tables, lane_ids = raw
    store = data_raw.build_store(raws, tables, R.config, lane_ids=lane_ids, lanes=True)
    return store, D.RoiStore.from_store(store)


def test_chunked_extraction_equals_one_pass(stores):
    store, rois = stores
    assert len(rois) == len(store) and rois.usable().tolist() == list(range(len(store)))
    same_store(D.RoiStore.from_store(store, chunk=1), rois, "chunk=1")
    same_store(D.RoiStore.from_store(store, chunk=3), rois, "chunk=3")
    want = D.lane_roi_flat(*D.store_roi_inputs(store))            # and the store is the flat route's result, scene-local
    got, _ = rois.batch(np.arange(len(store)))
    for k in DEV_ARRAYS:
        assert torch.equal(getattr(got, k), getattr(want, k)), k


def test_concat_equals_one_store_over_all_scenes(cases, tmp_path):
    a_scenes, b_scenes = cases["standing_added"], cases["dup_edges"]
    scenes = a_scenes + b_scenes
    whole = store_of(scenes)
    cat = D.RoiStore.concat([store_of(a_scenes), store_of(b_scenes)])
    same_store(cat, whole, "concat")
    us = whole.usable().tolist()
    for pick in (us[::-1], [us[-1], us[0], us[-1]]):
        assert_batch_equals_rebuild(cat, scenes, pick, "concat")
    with pytest.raises(LgcnError, match="empty list"):
        D.RoiStore.concat([])
    # save / load: equal stores, and load followed by save reproduces the file's arrays byte for byte
    p1, p2 = str(tmp_path / "rois.npz"), str(tmp_path / "again.npz")
    cat.save(p1)
    back = D.RoiStore.load(p1)
    same_store(back, whole, "load")
    back.save(p2)
    with np.load(p1) as f1, np.load(p2) as f2:
        assert sorted(f1.files) == sorted(f2.files)
        for k in f1.files:
            assert f1[k].dtype == f2[k].dtype and f1[k].shape == f2[k].shape and f1[k].tobytes() == f2[k].tobytes(), k
    assert_batch_equals_rebuild(back, scenes, us[1:3], "load")


def test_a_store_without_gt(cases):
    scenes = cases["shuffle"]
    t, off, rows = _roi_inputs(scenes)
    rows = {k: v for k, v in rows.items() if k not in ("gt_preds", "has_preds")}
    rois = D.RoiStore.from_inputs(t, off, rows=rows)
    assert not rois.has_gt
    for pick in ([1, 0], [2, 2]):
        assert_batch_equals_rebuild(rois, scenes, pick, "no gt", row_keys=ROW_KEYS[:3])
    # rows=None: what the RoI inputs hold themselves -- ctrs, and the (x, y) columns of feats / obs_trajs over a zero flag
    bare = D.RoiStore.from_inputs(t, off)
    assert not bare.has_gt
    (got, out), (_, full) = bare.batch([1, 0]), rois.batch([1, 0])
    assert torch.equal(got.u, rois.batch([1, 0])[0].u) and torch.equal(out["ctrs"], full["ctrs"])
    for k in ("feats", "obs_trajs"):
        assert torch.equal(out[k][:, :, :2], full[k][:, :, :2]) and not bool(out[k][:, :, 2].any()), k
    with pytest.raises(LgcnError, match="with and without gt_preds"):
        D.RoiStore.concat([rois, store_of(scenes)])
    with pytest.raises(LgcnError, match="come together"):
        D.RoiStore.from_inputs(t, off, rows=dict(rows, gt_preds=_rows(scenes)["gt_preds"]))


# ------------------------------------------------------------------ 4: one launch, no read-back
def device_events(rois, pick):
    from torch.profiler import ProfilerActivity, profile
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
        rois.batch(pick)
        torch.cuda.synchronize()
    return [e.name for e in prof.events() if str(e.device_type).endswith("CUDA")]


def test_one_launch_and_no_read_back(cases):
    scenes = cases["shuffle"] + cases["dup_edges"]
    rois = store_of(scenes)
    us = rois.usable().tolist()
    small, large = us[:2], [us[i % len(us)] for i in range(40)]
    names = []
    for pick in (small, large):
        device_events(rois, pick)                                 # warm: library load, allocator
        names.append(device_events(rois, pick))
    print("device events of a 2-scene pick:", names[0], "\nof a 40-scene pick:", names[1])
    is_copy = lambda n: "memcpy" in n.lower() or "copy" in n.lower()
    is_set = lambda n: "memset" in n.lower() or "fill" in n.lower()
    for ev in names:
        kernels = [n for n in ev if not is_copy(n) and not is_set(n)]
        assert len(kernels) == 1 and "roi_store_gather" in kernels[0], ev
        assert not any("dtoh" in n.lower() or "devicetohost" in n.lower().replace(" ", "") for n in ev), ev
        assert sum(1 for n in ev if is_copy(n)) == 1, ev          # the table's upload
    assert len(names[0]) == len(names[1])


# ------------------------------------------------------------------ 5: the net from the two stores
def make_net(train=False):
    g, names = NF.fixture()
    net = R.Net(R.config)
    net.load_state_dict(seeded_state([(k, tuple(s)) for k, s in names["net"]], int(g["seed"])), strict=True)
    net.cuda()
    return net.train() if train else net.eval()


OUT_KEYS = ("pred_logics", "pred_goals", "pred_trajs")


# (scene 2 holds one agent alone: picked by itself its poolings find no pair, and forward_raw raises as the reference does)
@pytest.mark.parametrize("pick", [[3, 1, 1, 0], [3], [0, 1, 2, 3], [2, 2, 0]])
def test_forward_store_equals_forward_raw(raw, stores, pick):
    raws, tables, lane_ids = raw
    store, rois = stores
    net = make_net()
    with torch.no_grad():
        want, wdata = net.forward_raw([raws[i] for i in pick], tables, lane_ids=[lane_ids[i] for i in pick])
        want = {k: v.clone() for k, v in want.items()}
        got, data = net.forward_store(store, rois, pick)
    assert sorted(got) == sorted(want) == sorted(OUT_KEYS)
    for k in OUT_KEYS:
        assert got[k].dtype == want[k].dtype and got[k].shape == want[k].shape and torch.equal(got[k], want[k]), k
    assert sorted(data) == sorted(list(ROW_KEYS) + ["valid_agent_ids", "agent_ids", "subgraphs"])
    for b in range(len(pick)):
        ids = wdata["valid_agent_ids"][b].long()
        assert data["valid_agent_ids"][b].dtype == torch.int16
        assert data["valid_agent_ids"][b].tolist() == list(range(len(ids)))
        assert np.array_equal(data["agent_ids"][b], ids.cpu().numpy())
        for k in ROW_KEYS:
            w = wdata[k][b][ids]
            assert data[k][b].dtype == w.dtype and torch.equal(data[k][b], w), (k, b)


def grads(net, loss_mod, run):
    net.zero_grad(set_to_none=True)
    out, data = run()
    loss_mod(out, data)["loss"].backward()
    return {k: p.grad.detach().clone() for k, p in net.named_parameters() if p.grad is not None}


def test_forward_store_loss_backward(raw, stores):
    raws, tables, lane_ids = raw
    store, rois = stores
    pick = [3, 1, 1, 0]
    net, loss_mod = make_net(train=True), R.Loss(R.config)
    by_raw = lambda: net.forward_raw([raws[i] for i in pick], tables, lane_ids=[lane_ids[i] for i in pick])
    a, b = grads(net, loss_mod, by_raw), grads(net, loss_mod, by_raw)
    f = grads(net, loss_mod, lambda: net.forward_store(store, rois, pick))
    assert sorted(a) == sorted(b) == sorted(f) and len(a) > 20
    own = {k: float((a[k] - b[k]).abs().max()) for k in a}       # forward_raw against itself: expected 0
    diff = {k: float((a[k] - f[k]).abs().max()) for k in a}
    print("run-to-run of forward_raw: max %.3e; forward_store against forward_raw: max %.3e" % (max(own.values()), max(diff.values())))
    for k in a:
        assert diff[k] <= own[k], (k, diff[k], own[k])


def test_a_scene_without_an_roi_is_stored_and_named():
    raws, maps, lane_ids, _ = SC.golden_inputs(RAW_SEED_DROP)
    tables = {c: data_raw.LaneTable.from_lanes(m) for c, m in maps.items()}
    store = data_raw.build_store(raws, tables, R.config, lane_ids=lane_ids, lanes=True)
    rois = D.RoiStore.from_store(store)
    assert len(rois) == len(store) and 2 not in rois.usable() and rois.rois_per_scene[2] == 0 and len(rois.usable()) == len(store) - 1
    with pytest.raises(LgcnError, match="scene 2 has no lane RoI"):
        rois.batch([0, 2])
    with pytest.raises(LgcnError, match="scene 2 has no lane RoI"):
        with torch.no_grad():
            make_net().forward_store(store, rois, [2])
    with torch.no_grad():
        out, _ = make_net().forward_store(store, rois, rois.usable())
    assert all(torch.isfinite(out[k]).all() for k in OUT_KEYS)


# ------------------------------------------------------------------ 6: repeatability
def test_batch_is_repeatable(cases):
    scenes = cases["dup_edges"] + [C.large_scene("crowd")]
    rois = store_of(scenes)
    pick = rois.usable().tolist()[::-1]
    (a, ra), (b, rb) = rois.batch(pick), rois.batch(pick)
    for k in DEV_ARRAYS:
        x, y = getattr(a, k), getattr(b, k)
        assert x.data_ptr() != y.data_ptr() or x.numel() == 0
        assert torch.equal(x.contiguous().view(torch.uint8), y.contiguous().view(torch.uint8)), k
    for k in ROW_KEYS:
        assert ra[k].data_ptr() != rb[k].data_ptr() and torch.equal(ra[k].view(torch.uint8), rb[k].view(torch.uint8)), k
    for k in HOST_TABLES:
        assert getattr(a, k).tobytes() == getattr(b, k).tobytes(), k
