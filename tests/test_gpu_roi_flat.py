"""GPU: the flat lane-RoI route -- data_lrcnn.lane_roi_flat / generate_lane_roi_flat -> RoiBatch (the merged batch graph
written by lgcn_roi_edge_fill_graph), lanercnn.subgraph_gather(RoiBatch), Net.forward on a RoiBatch and
Net.forward_raw -- against the list route of the same package (generate_lane_roi_batch(device=True) -> per-RoI dicts ->
subgraph_gather -> Net.forward).  Integers and copied floats: every comparison is exact."""
import copy

import numpy as np
import pytest
import torch

import lanegcn_amd  # noqa: F401
import lane_roi_cases as C
import lanercnn_net_fixture as NF
import scene_build_cases as SC
from lanegcn_amd import data as gen
from lanegcn_amd import data_lrcnn as D
from lanegcn_amd import data_raw
from lanegcn_amd import lanercnn as R
from lanegcn_amd._lib import LgcnError
from oracle.lanercnn_oracle import seeded_state

pytestmark = pytest.mark.gpu
RAW_SEED = 500          # every scene of golden_inputs(500) keeps an RoI (searched on the CPU models; asserted below)
RAW_SEED_DROP = 1       # scene 2 of golden_inputs(1): its only agent drops (lane_roi_model), asserted below


def list_route(scenes):
    """Today's route on copies of `scenes` -> (the scenes that keep an RoI, with subgraphs / valid_agent_ids; their positions)."""
    out = D.generate_lane_roi_batch(copy.deepcopy(scenes), device=True)
    keep = [i for i, s in enumerate(out) if len(s["subgraphs"])]
    return [out[i] for i in keep], keep


def both_gathers(scenes):
    """(subgraph_gather of the flat route, of the list route, the RoiBatch, the list route's scenes); scenes whose agents all
    drop are removed from both sides."""
    listed, keep = list_route(scenes)
    flat_scenes = copy.deepcopy([scenes[i] for i in keep])
    rb = D.generate_lane_roi_flat(flat_scenes)
    for s, w in zip(flat_scenes, listed):
        assert s["valid_agent_ids"].dtype == np.int16 and np.array_equal(s["valid_agent_ids"], w["valid_agent_ids"])
    return R.subgraph_gather(rb), R.subgraph_gather([s["subgraphs"] for s in listed]), rb, listed


def assert_same_graph(got, want, what):
    assert sorted(got) == sorted(want), what
    C.assert_same_tensors(got, want, what)      # tensors: dtype, device, torch.equal; lists: lengths; ints / np.float32: equal


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
    seeds = {"shuffle": 12, "cycle": 14, "dup_edges": 15, "standing": 11}        # lane_roi_cases.trial's docstring
    out = {"fixture": C.load_fixture()[0]}
    for name, seed in seeds.items():
        out[name] = C.trial(seed)
    out["standing_added"] = C.trial(16) + [C.standing_scene(np.random.default_rng(5), np.int16)]
    out["one_roi"] = [one_roi_scene()]
    out["no_side"] = no_side_scenes()
    return out


BATCHES = ("fixture", "shuffle", "cycle", "dup_edges", "standing", "standing_added", "one_roi", "no_side")


@pytest.fixture(scope="module")
def cases():
    return batches()


# ------------------------------------------------------------------ 1, 2: the batch graph and the per-RoI views
@pytest.mark.parametrize("name", BATCHES)
def test_batch_graph_equals_the_list_route(cases, name):
    scenes = cases[name]
    if name in ("shuffle", "cycle", "dup_edges"):
        dts = {np.asarray(s["graph"]["lane_idcs"]).dtype for s in scenes}
        assert np.dtype(np.int16) in dts                          # int16 index arrays ride along in every trial
    got, want, rb, listed = both_gathers(scenes)
    assert_same_graph(got, want, name)
    if name in ("standing", "standing_added"):
        assert len(listed) < len(scenes)                          # a scene whose agents all drop was removed
    if name == "one_roi":
        assert rb.n_rois == 1 and got["counts"] == [0]
    if name == "no_side":
        assert rb.n_rois > 1 and got["left"]["u"].numel() == 0 and got["right"]["v"].numel() == 0 and got["suc"][0]["u"].numel() > 0
    # 2: the compatibility views are today's per-RoI dicts
    subs = rb.subgraphs()
    assert len(subs) == len(listed)
    for b, (x, y) in enumerate(zip(subs, listed)):
        C.assert_same_tensors(x, y["subgraphs"], "%s/subgraphs/%d" % (name, b))
        assert np.array_equal(rb.valid_agent_ids(b), y["valid_agent_ids"])


# ------------------------------------------------------------------ 3: sizes at which the fill can go wrong
@pytest.mark.parametrize("name", ["wide", "crowd"])
def test_large_rois_and_many_rois(name):
    scene = C.large_scene(name)
    got, want, rb, _ = both_gathers([one_roi_scene(), scene])      # a scene in front: no base is 0 in the scene under test
    if name == "wide":
        assert rb.sizes.max() > 2 * 256                           # more than two chunks of kRoiThreads rows: the carry runs
    else:
        assert rb.n_rois >= 40 and rb.roi_base[-2] > 10 * scene["graph"]["num_nodes"]      # bases far above the node count
    assert_same_graph(got, want, name)


# ------------------------------------------------------------------ 4: the op count does not depend on the RoIs
def count_ops(t, off):
    from torch.profiler import ProfilerActivity, profile
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
        rb = D.lane_roi_flat(t, off)
        R.subgraph_gather(rb)
        torch.cuda.synchronize()
    ev = list(prof.events())
    aten = sum(1 for e in ev if e.name.startswith("aten::"))
    dev = sum(1 for e in ev if str(e.device_type).endswith("CUDA"))       # kernels, memsets and copies on the device
    return aten, dev, rb.n_rois


def test_op_count_does_not_depend_on_the_number_of_rois():
    crowd = C.large_scene("crowd")
    kept = list_route([crowd])[0][0]["valid_agent_ids"].tolist()
    few = copy.deepcopy(crowd)
    pick = kept[:2]
    for k in ("feats", "ctrs", "obs_trajs", "gt_preds", "has_preds"):
        few[k] = few[k][pick]
    counts = []
    for scenes in ([one_roi_scene(), few], [one_roi_scene(), crowd]):
        t, off, _ = D._roi_inputs(scenes)
        count_ops(t, off)                                         # warm: library load, allocator
        counts.append(count_ops(t, off))
    print("aten ops, device events, RoIs:", counts)
    assert counts[0][2] == 3 and counts[1][2] >= 40
    assert counts[0][0] == counts[1][0] and counts[0][0] > 0
    assert counts[0][1] == counts[1][1]


# ------------------------------------------------------------------ 5: the net on a RoiBatch
def make_net(train=False):
    g, names = NF.fixture()
    net = R.Net(R.config)
    net.load_state_dict(seeded_state([(k, tuple(s)) for k, s in names["net"]], int(g["seed"])), strict=True)
    net.cuda()
    return net.train() if train else net.eval()


def net_scenes():
    """The fixture's scenes with the lane pairs the RoI search reads (the recording holds the RoIs, not the pairs)."""
    scenes = NF.scenes()
    for s in scenes:
        g = s["graph"]
        g["pre_pairs"] = gen.lane_pairs(g["pre"][0], g["lane_idcs"])
        g["suc_pairs"] = gen.lane_pairs(g["suc"][0], g["lane_idcs"])
    return scenes


def net_inputs(flat):
    scenes = net_scenes()
    if flat:
        rb = D.generate_lane_roi_flat(scenes)
        data = gen.collate_fn(scenes)
        data["subgraphs"] = rb
        return data
    scenes = D.generate_lane_roi_batch(scenes, device=True)
    assert all(len(s["subgraphs"]) for s in scenes)
    return gen.collate_fn(scenes)


OUT_KEYS = ("pred_logics", "pred_goals", "pred_trajs")


def test_net_forward_on_a_roi_batch():
    net = make_net()
    with torch.no_grad():
        want = {k: v.clone() for k, v in net(net_inputs(False)).items()}
        got = net(net_inputs(True))
    assert sorted(got) == sorted(want) == sorted(OUT_KEYS)
    for k in OUT_KEYS:
        assert got[k].dtype == want[k].dtype and torch.equal(got[k], want[k]), k


def grads(net, loss_mod, flat):
    net.zero_grad(set_to_none=True)
    data = net_inputs(flat)
    out = net(data)
    loss_mod(out, data)["loss"].backward()
    return {k: p.grad.detach().clone() for k, p in net.named_parameters() if p.grad is not None}


def test_net_loss_backward_on_a_roi_batch():
    net, loss_mod = make_net(train=True), R.Loss(R.config)
    a, b, f = grads(net, loss_mod, False), grads(net, loss_mod, False), grads(net, loss_mod, True)
    assert sorted(a) == sorted(b) == sorted(f) and len(a) > 20
    own = {k: float((a[k] - b[k]).abs().max()) for k in a}       # the list route against itself: expected 0
    diff = {k: float((a[k] - f[k]).abs().max()) for k in a}
    print("run-to-run of the list route: max %.3e; flat against list: max %.3e" % (max(own.values()), max(diff.values())))
    for k in a:
        assert diff[k] <= own[k], (k, diff[k], own[k])


# ------------------------------------------------------------------ 6: raw tracks to predictions
@pytest.fixture(scope="module")
def raw():
    raws, maps, lane_ids, _ = SC.golden_inputs(RAW_SEED)
    return raws, {c: data_raw.LaneTable.from_lanes(m) for c, m in maps.items()}, lane_ids


def test_forward_raw_equals_the_dict_route(raw):
    raws, tables, lane_ids = raw
    net = make_net()
    scenes = D.generate_lane_roi_batch(data_raw.build_scenes(raws, tables, net.config, batched=True, lane_ids=lane_ids), device=True)
    assert all(len(s["subgraphs"]) >= 1 for s in scenes), [len(s["subgraphs"]) for s in scenes]
    with torch.no_grad():
        want = {k: v.clone() for k, v in net(gen.collate_fn(scenes)).items()}
        got, data = net.forward_raw(raws, tables, lane_ids=lane_ids)
    for k in OUT_KEYS:
        assert got[k].dtype == want[k].dtype and torch.equal(got[k], want[k]), k
    for b, s in enumerate(scenes):
        assert np.array_equal(data["valid_agent_ids"][b].cpu().numpy(), s["valid_agent_ids"])
        for k in ("ctrs", "feats", "obs_trajs", "gt_preds", "has_preds"):
            assert data[k][b].dtype == s[k].dtype and torch.equal(data[k][b], s[k]), (k, b)
    # the grad-enabled route runs the modules' Functions, and Loss works on what forward_raw returns
    net = make_net(train=True)
    out, data = net.forward_raw(raws, tables, lane_ids=lane_ids)
    loss = R.Loss(R.config)(out, data)["loss"]
    loss.backward()
    assert torch.isfinite(loss) and any(p.grad is not None and bool(p.grad.abs().sum() > 0) for p in net.parameters())


def test_forward_raw_names_a_scene_without_an_roi():
    raws, maps, lane_ids, _ = SC.golden_inputs(RAW_SEED_DROP)
    tables = {c: data_raw.LaneTable.from_lanes(m) for c, m in maps.items()}
    net = make_net()
    scenes = D.generate_lane_roi_batch(data_raw.build_scenes(raws, tables, net.config, batched=True, lane_ids=lane_ids), device=True)
    assert [b for b, s in enumerate(scenes) if not len(s["subgraphs"])] == [2]
    with pytest.raises(LgcnError, match="scene 2 has no lane RoI"):
        with torch.no_grad():
            net.forward_raw(raws, tables, lane_ids=lane_ids)


def test_store_with_and_without_lanes(raw):
    raws, tables, lane_ids = raw
    plain = data_raw.build_store(raws, tables, R.config, lane_ids=lane_ids)
    lanes = data_raw.build_store(raws, tables, R.config, lane_ids=lane_ids, lanes=True)
    assert plain.lane_arrays is None and sorted(lanes.lane_arrays) == sorted(
        ["lane_idcs", "obs", "lane_off", "suc_pairs", "pre_pairs", "suc_off", "pre_off"])
    with pytest.raises(LgcnError, match="lanes=True"):
        D.store_roi_inputs(plain)
    assert sorted(plain._job.t) == sorted(lanes._job.t)
    for k, x in plain._job.t.items():
        y = lanes._job.t[k]
        assert x.dtype == y.dtype and x.shape == y.shape and torch.equal(x, y), k
    for k in ("node_off", "actor_off", "edge_off", "rel_off", "theta"):
        x, y = getattr(plain, k), getattr(lanes, k)
        assert x.dtype == y.dtype and x.tobytes() == y.tobytes(), k
    assert plain.num_scales == lanes.num_scales and plain.scene_city == lanes.scene_city and plain.nbytes == lanes.nbytes


# ------------------------------------------------------------------ 7: repeatability
def test_lane_roi_flat_is_repeatable():
    scenes = C.trial(15) + [C.large_scene("crowd")]
    listed, keep = list_route(scenes)
    t, off, _ = D._roi_inputs([scenes[i] for i in keep])
    a, b = D.lane_roi_flat(t, off), D.lane_roi_flat(t, off)
    for k in ("feats", "node_mask", "agent_feat", "u", "v", "a2m_u", "a2m_v"):
        x, y = getattr(a, k), getattr(b, k)
        assert x.data_ptr() != y.data_ptr() or x.numel() == 0
        assert torch.equal(x.view(torch.uint8) if x.dtype != torch.float32 else x.view(torch.int32),
                           y.view(torch.uint8) if y.dtype != torch.float32 else y.view(torch.int32)), k
    for k in ("sizes", "roi_base", "scene_of", "agents", "agent_vel", "rel_ext", "edge_cnt"):
        assert getattr(a, k).tobytes() == getattr(b, k).tobytes(), k
