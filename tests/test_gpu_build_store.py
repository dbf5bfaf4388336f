"""GPU: data_raw.build_store, lgcn_store_pack, DeviceSceneStore.concat / save and Net.forward_raw against the existing
route build_scenes(device=False, cross=True, batched=True) -> write_scenes(theta=True) -> FlatSceneFile / DeviceSceneStore(path),
which the existing tests pin to the reference's recording.  Pure data movement and the same kernels on both routes: every
comparison is equality of bytes, dtype and shape included.  The pack launch alone is held against numpy's astype(int32)
and concatenate."""
import copy
import os

import numpy as np
import pytest
import torch

import lanegcn_amd  # noqa: F401
import scene_build_cases as C
import scene_store_cases as SC
from conftest import GOLDEN_DIR
from oracle import lanegcn_oracle as O

pytestmark = pytest.mark.gpu
SCENE_GOLDEN = os.path.join(GOLDEN_DIR, "scene_build_b4.npz")
PICKS = {"all": [0, 1, 2, 3, 4], "single": [3], "repeat": [4, 1, 1, 0], "reversed": [4, 3, 2, 1, 0]}
ROT_DT = {k: [0.3 * (i + 1) - 0.7 for i in range(len(v))] for k, v in PICKS.items()}
PARTS = ((0, 2), (2, 3), (3, 5))
POISON = 0x5A5A5A5A


@pytest.fixture(scope="module")
def batch5():
    """The five-scene, two-city batch of test_gpu_scene_build.py (300 tracks in scene 3, a table of 1,500 lanes)."""
    raws, tables, lane_ids, _ = C.load_fixture(SCENE_GOLDEN)
    raws, lane_ids = raws + [C.extra_scene(9)], lane_ids + [None]
    return raws, {k: v.to("cuda") for k, v in tables.items()}, lane_ids


def file_route(batch5, config, path):
    """The yardstick: scenes with host leaves, written as a flat file -> (its arrays, the store loaded from it)."""
    from lanegcn_amd import data_raw as D
    from lanegcn_amd.flatfile import DeviceSceneStore, write_scenes
    raws, tables, lane_ids = batch5
    scenes = D.build_scenes(copy.deepcopy(raws), tables, config, device=False, cross=True, lane_ids=lane_ids, batched=True)
    write_scenes(path, scenes, theta=True)
    with np.load(path, allow_pickle=False) as z:
        return {k: z[k] for k in z.files}, DeviceSceneStore(path)


@pytest.fixture(scope="module")
def fx(batch5, tmp_path_factory):
    """Per num_scales (6 and 1): the file route's arrays and store, and build_store's store.  Computed once, not modified."""
    from lanegcn_amd import data_raw as D
    raws, tables, lane_ids = batch5
    d = tmp_path_factory.mktemp("build_store")
    out = {"dir": d}
    for ns in (6, 1):
        config = dict(C.CONFIG, num_scales=ns)
        want, dev = file_route(batch5, config, str(d / ("file_%d.npz" % ns)))
        out[ns] = dict(config=config, want=want, file_store=dev,
                       store=D.build_store(copy.deepcopy(raws), tables, config, lane_ids=lane_ids))
    torch.cuda.synchronize()
    return out


def same_file(got, want, what=""):
    assert sorted(got) == sorted(want), (what, sorted(got), sorted(want))
    for k in want:
        g, w = got[k], want[k]
        assert g.dtype == w.dtype and g.shape == w.shape and g.tobytes() == w.tobytes(), (what, k, g.dtype, w.dtype, g.shape, w.shape)


def same(got, want, what):
    assert got.dtype == want.dtype and tuple(got.shape) == tuple(want.shape), (what, got.dtype, got.shape, want.dtype, want.shape)
    assert got.device == want.device and torch.equal(got, want), what


def check_batch(got, want, what=""):
    (fb, ex), (wfb, wex) = got, want
    for f in SC.FLAT_FIELDS:
        assert getattr(fb, f) == getattr(wfb, f), (what, f)
    for f in SC.FLAT_ARRAYS:
        same(getattr(fb, f), getattr(wfb, f), (what, f))
    assert sorted(ex) == sorted(wex), what
    assert ex["sizes"] == wex["sizes"] and type(ex["sizes"]) is list
    for k in wex:
        if k == "theta":
            assert ex[k].dtype == wex[k].dtype == np.float64 and ex[k].tobytes() == wex[k].tobytes(), what
        elif k != "sizes":
            same(ex[k], wex[k], (what, k))


def load(path):
    with np.load(path, allow_pickle=False) as z:
        return {k: z[k] for k in z.files}


# ------------------------------------------------------------------ 1. the store equals the file route
@pytest.mark.parametrize("ns", [6, 1])
def test_store_equals_the_file_route(fx, ns):
    from lanegcn_amd.flatfile import DeviceSceneStore, FlatSceneFile
    f = fx[ns]
    store, want = f["store"], f["want"]
    assert isinstance(store, DeviceSceneStore) and len(store) == 5 and store.num_scales == ns and store.has_gt
    assert store.edge_off.shape == (2 * ns + 2, 6) and store.theta.dtype == np.float64
    path = str(fx["dir"] / ("saved_%d.npz" % ns))
    store.save(path)
    got = load(path)
    same_file(got, want, ns)
    assert got["has_preds"].dtype == bool and got["edge_u"].dtype == np.int32 and "theta" in got
    assert got["node_off"][-1] > 1000 and got["actor_off"][-1] > 64 and got["rel_off"][-1] > 4096      # many workgroups
    # what is held: at least the arrays themselves (the actor arrays are the first rows of tensors sized for every track)
    arrays = [k for k in want if k not in ("num_scales", "node_off", "actor_off", "edge_off", "rel_off", "theta")]
    assert store.nbytes >= sum(want[k].nbytes for k in arrays)
    # both readers take the saved file
    assert len(FlatSceneFile(path)) == 5
    again = DeviceSceneStore(path)
    check_batch(again.batch(PICKS["repeat"]), f["file_store"].batch(PICKS["repeat"]), "reloaded")


# ------------------------------------------------------------------ 2. batches
@pytest.mark.parametrize("name", sorted(PICKS))
@pytest.mark.parametrize("ns", [6, 1])
def test_batches_equal_the_file_stores(fx, ns, name):
    store, ref = fx[ns]["store"], fx[ns]["file_store"]
    pick = PICKS[name]
    check_batch(store.batch(pick), ref.batch(pick), (ns, name))
    got, want = store.batch(pick, rot_dt=ROT_DT[name]), ref.batch(pick, rot_dt=ROT_DT[name])
    assert "theta" in got[1]
    check_batch(got, want, (ns, name, "rot_dt"))
    p, q = store.plan(pick), ref.plan(pick)
    assert np.array_equal(p.table, q.table) and p.rel_slices == q.rel_slices


# ------------------------------------------------------------------ 3. launches and host reads
WRAPPED = ("scene_tracks", "scene_lanes_rank", "scene_lanes_fill", "dilate_batch", "cross_edges_batch", "read_back", "store_pack")


@pytest.fixture
def calls(monkeypatch):
    from lanegcn_amd import data_raw, ops, preprocess_data
    seen = []
    for name in WRAPPED:
        real = getattr(ops, name)
        monkeypatch.setattr(ops, name, lambda *a, _real=real, _name=name, **k: (seen.append(_name), _real(*a, **k))[1])

    def never(name):
        def f(*a, **k):
            raise AssertionError("build_store reached %s" % name)
        return f
    for mod, name in ((data_raw, "_graphs"), (data_raw, "_split"), (preprocess_data, "split_cross"),
                      (preprocess_data, "dilated_nbrs"), (preprocess_data, "preprocess")):
        monkeypatch.setattr(mod, name, never(name))
    return seen


def test_launch_and_read_budget(batch5, calls):
    from lanegcn_amd import data_raw as D
    raws, tables, lane_ids = batch5
    num_scales = int(C.CONFIG["num_scales"])
    for n in (2, 5):
        del calls[:]
        store = D.build_store(copy.deepcopy(raws[:n]), tables, C.CONFIG, lane_ids=lane_ids[:n])
        assert len(store) == n
        assert calls.count("store_pack") == 1 and calls.count("dilate_batch") == 1 and calls.count("cross_edges_batch") == 1
        assert calls.count("read_back") == (num_scales - 1) + 1, (n, calls)
        assert calls[-1] == "store_pack" and calls[:3] == ["scene_tracks", "scene_lanes_rank", "scene_lanes_fill"]


# ------------------------------------------------------------------ 4. the pack launch alone
def run_pack(sources, seg_src, seg_at, seg_len, lead=32, tail=64, frame=None):
    """ops.store_pack on numpy sources into the middle of a poisoned buffer; checks the runs against numpy and that no
    word before or after them changed.  Sources may be (base, start, stop) triples: views of one device array."""
    from lanegcn_amd import ops
    bases, dev_src, np_src = {}, [], []
    for s in sources:
        if isinstance(s, tuple):
            base, a, b = s
            if id(base) not in bases:
                bases[id(base)] = torch.from_numpy(base).cuda()
            dev_src.append(bases[id(base)][a:b])
            np_src.append(base[a:b])
        else:
            dev_src.append(torch.from_numpy(s).cuda())
            np_src.append(s)
    runs = [np_src[s][a:a + n].astype(np.int32) for s, a, n in zip(seg_src, seg_at, seg_len)]
    want = np.concatenate(runs) if runs else np.zeros(0, np.int32)
    n = len(want)
    buf = torch.full((lead + n + tail,), POISON, dtype=torch.int32, device="cuda")
    extra = {}
    if frame is not None:
        S = len(frame)
        extra = dict(frame=torch.from_numpy(frame).cuda(), rot=torch.full((S, 2, 2), -7.0, device="cuda"),
                     orig=torch.full((S, 2), -7.0, device="cuda"))
    assert ops.store_pack(dev_src, seg_src, seg_at, seg_len, buf[lead:], **extra) == n
    got = buf.cpu().numpy()
    assert (got[:lead] == POISON).all() and (got[lead + n:] == POISON).all()
    assert np.array_equal(got[lead:lead + n], want)
    if frame is not None:
        assert np.array_equal(extra["orig"].cpu().numpy(), frame[:, :2])
        assert np.array_equal(extra["rot"].cpu().numpy(), frame[:, 2:].reshape(-1, 2, 2))
    return want


def wide(rng, n):
    """int64 values that do not fit int32: beyond 2^31, negative, and a few that do fit."""
    x = rng.integers(-2 ** 40, 2 ** 40, n).astype(np.int64)
    x[::7] = rng.integers(-5, 5, len(x[::7]))
    if n > 3:
        x[:4] = [2 ** 31, -2 ** 31 - 1, 2 ** 32 + 5, -1]
    return x


def test_pack_run_lengths_around_a_workgroup():
    rng = np.random.default_rng(0)
    lens = [0, 1, 255, 256, 257, 70001]
    want = run_pack([wide(rng, n) for n in lens], range(6), [0] * 6, lens)
    assert len(want) == sum(lens) and (want[1:] != 0).any()
    # the same runs out of ONE int64 array, every run from an element that is no multiple of a workgroup
    base = wide(rng, sum(lens) + 100)
    at = np.cumsum([3] + [n + 5 for n in lens[:-1]])
    run_pack([base], [0] * 6, at, lens)


def test_pack_empty_runs_first_last_and_in_a_row():
    rng = np.random.default_rng(1)
    src = [wide(rng, 40), rng.integers(-32768, 32768, 40).astype(np.int16), np.zeros(0, np.int64)]
    run_pack(src, [0, 2, 1, 2, 0, 1, 0, 2], [0, 0, 3, 0, 40, 40, 7, 0], [0, 0, 5, 0, 0, 0, 7, 0])
    run_pack(src, [2, 2, 2], [0, 0, 0], [0, 0, 0])                       # nothing but empty runs: nothing is written
    run_pack(src, [], [], [])                                            # no run at all: no launch
    run_pack(src, [1], [0], [40])                                        # a single run
    run_pack(src, [0], [39], [1])


def test_pack_three_thousand_runs_of_all_kinds():
    """3,000 runs of 0..40 elements from int16, int32 and int64 sources in random order: the run table spans many
    workgroups and consecutive threads change source and element size."""
    rng = np.random.default_rng(2)
    i16 = rng.integers(-32768, 32768, 500).astype(np.int16)
    i16[:4] = [32767, -32767, -32768, -1]
    src = [i16, rng.integers(-2 ** 31, 2 ** 31, 300).astype(np.int32), wide(rng, 400), i16[::-1].copy()]
    G = 3000
    seg_len = rng.integers(0, 41, G)
    seg_src = rng.integers(0, len(src), G)
    seg_at = np.array([rng.integers(0, len(src[s]) - n + 1) for s, n in zip(seg_src, seg_len)])
    want = run_pack(src, seg_src, seg_at, seg_len)
    assert len(want) > 256 * 100 and (want < 0).any()
    frame = rng.normal(0, 100, (700, 6)).astype(np.float32)              # frame rows past one workgroup, in the same launch
    run_pack(src, seg_src[:50], seg_at[:50], seg_len[:50], frame=frame)


def test_pack_int16_sign_and_int64_truncation():
    i16 = np.array([32767, -32767, -32768, -1, 0, 1, -2, 12345, -12345], np.int16)
    want = run_pack([i16], [0], [0], [len(i16)])
    assert want.tolist() == [32767, -32767, -32768, -1, 0, 1, -2, 12345, -12345]
    i64 = np.array([2 ** 31, 2 ** 31 - 1, -2 ** 31, -2 ** 31 - 1, 2 ** 32, 2 ** 32 + 7, -2 ** 40 + 3, -1, 2 ** 62 + 9], np.int64)
    want = run_pack([i64], [0], [0], [len(i64)])
    assert want.tolist() == [-2 ** 31, 2 ** 31 - 1, -2 ** 31, 2 ** 31 - 1, 0, 7, 3, -1, 9]
    i32 = np.array([2 ** 31 - 1, -2 ** 31, -1, 0, 77], np.int32)
    assert run_pack([i32], [0, 0], [3, 0], [2, 5]).tolist() == [0, 77, 2 ** 31 - 1, -2 ** 31, -1, 0, 77]


def test_pack_sources_that_share_a_base():
    rng = np.random.default_rng(3)
    base64, base16 = wide(rng, 600), rng.integers(-32768, 32768, 600).astype(np.int16)
    src = [(base64, 0, 600), (base64, 3, 300), (base64, 299, 600), (base16, 1, 2), (base16, 7, 600), (base16, 0, 600)]
    run_pack(src, [2, 0, 1, 3, 4, 5, 1], [0, 590, 290, 0, 500, 1, 0], [301, 10, 7, 1, 93, 0, 297])


def test_pack_refuses_a_bad_table_and_writes_nothing():
    from lanegcn_amd import ops
    from lanegcn_amd._lib import LgcnError
    src = [torch.arange(10, dtype=torch.int64, device="cuda")]
    buf = torch.full((32,), POISON, dtype=torch.int32, device="cuda")
    for seg_src, seg_at, seg_len in (([0], [5], [6]), ([1], [0], [1]), ([0], [-1], [2]), ([0, 0], [0, 0], [4, -1]), ([0], [0], [33])):
        with pytest.raises(LgcnError):
            ops.store_pack(src, seg_src, seg_at, seg_len, buf)
    with pytest.raises(LgcnError):
        ops.store_pack([src[0].float()], [0], [0], [1], buf)
    with pytest.raises(LgcnError):
        ops.store_pack(src, [0], [0], [1], buf[::2])
    torch.cuda.synchronize()
    assert bool((buf == POISON).all())


# ------------------------------------------------------------------ 5. concat
@pytest.fixture(scope="module")
def parts(batch5, fx):
    from lanegcn_amd import data_raw as D
    raws, tables, lane_ids = batch5
    return [D.build_store(copy.deepcopy(raws[a:b]), tables, C.CONFIG, lane_ids=lane_ids[a:b]) for a, b in PARTS]


def test_concat_equals_the_one_shot_store(fx, parts, monkeypatch):
    from lanegcn_amd import ops
    from lanegcn_amd.flatfile import DeviceSceneStore
    seen = []
    real = ops.store_pack
    monkeypatch.setattr(ops, "store_pack", lambda *a, **k: (seen.append(len(a[1])), real(*a, **k))[1])
    whole = DeviceSceneStore.concat(parts)
    assert seen == [len(PARTS) * 2 * 14]                                  # ONE launch over P x 2R runs
    assert [len(p) for p in parts] == [2, 1, 2] and len(whole) == 5
    counts = np.concatenate([np.diff(p.edge_off, axis=1) for p in parts], 1)
    print("edges per relation (rows) and scene (columns):\n%s" % counts)
    path = str(fx["dir"] / "concat.npz")
    whole.save(path)
    same_file(load(path), fx[6]["want"], "concat")
    for name in ("all", "repeat", "reversed"):                           # [4, 1, 1, 0] and the others cross part boundaries
        check_batch(whole.batch(PICKS[name]), fx[6]["store"].batch(PICKS[name]), name)
        check_batch(whole.batch(PICKS[name], rot_dt=ROT_DT[name]), fx[6]["file_store"].batch(PICKS[name], rot_dt=ROT_DT[name]), name)
    one = DeviceSceneStore.concat(parts[1:2])                            # a single part is a copy of it
    check_batch(one.batch([0]), fx[6]["store"].batch([2]), "single part")


def test_concat_refusals_launch_nothing(fx, parts, batch5, monkeypatch):
    from lanegcn_amd import data_raw as D, ops
    from lanegcn_amd._lib import LgcnError
    from lanegcn_amd.flatfile import DeviceSceneStore
    raws, tables, lane_ids = batch5
    narrow = D.build_store(copy.deepcopy(raws[:1]), tables, fx[1]["config"], lane_ids=lane_ids[:1])
    t = parts[1]._job.t
    no_gt = DeviceSceneStore.from_arrays({k: v for k, v in t.items() if k not in ("gt_preds", "has_preds")}, parts[1].node_off,
                                         parts[1].actor_off, parts[1].edge_off, parts[1].rel_off, 6, parts[1].theta)
    no_theta = DeviceSceneStore.from_arrays(t, parts[1].node_off, parts[1].actor_off, parts[1].edge_off, parts[1].rel_off, 6)
    assert not no_gt.has_gt and no_theta.theta is None

    def never(*a, **k):
        raise AssertionError("a refused concat reached a launch")
    monkeypatch.setattr(ops, "store_pack", never)
    monkeypatch.setattr(torch, "cat", never)
    for bad in ([], [parts[0], narrow], [parts[0], no_gt], [no_theta, parts[2]]):
        with pytest.raises(LgcnError):
            DeviceSceneStore.concat(bad)
    if torch.cuda.device_count() > 1:
        other = types_namespace_on(parts[1], "cuda:1")
        with pytest.raises(LgcnError):
            DeviceSceneStore.concat([parts[0], other])


def types_namespace_on(store, device):
    """A stand-in for `store` that says it lives on `device` (concat refuses before it touches an array)."""
    import types
    return types.SimpleNamespace(device=torch.device(device), has_gt=store.has_gt, node_off=store.node_off,
                                 actor_off=store.actor_off, edge_off=store.edge_off, rel_off=store.rel_off,
                                 num_scales=store.num_scales, theta=store.theta)


# ------------------------------------------------------------------ 6. end to end
@pytest.fixture(scope="module")
def net(ref_state_names):
    from lanegcn_amd import lanegcn as M
    n = M.Net(dict(M.config, **C.CONFIG))
    n.load_state_dict(O.seeded_state(ref_state_names, 3), strict=True)
    return n.cuda().eval()


def test_forward_raw_end_to_end(batch5, fx, net):
    from lanegcn_amd import data as gen, data_raw as D
    raws, tables, lane_ids = batch5
    keys = ("feats", "ctrs", "orig", "theta", "rot", "gt_preds", "has_preds", "graph")
    with torch.no_grad():
        got = net.forward_raw(copy.deepcopy(raws), tables, lane_ids=lane_ids)
        want = net.forward_store(fx[6]["file_store"], range(5))
        scenes = D.build_scenes(copy.deepcopy(raws), tables, C.CONFIG, device=True, lane_ids=lane_ids, batched=True)
        dicts = net(gen.collate_fn([{k: s[k] for k in keys} for s in scenes]))
    for k in ("cls", "reg"):
        assert len(got[k]) == len(want[k]) == len(dicts[k]) == 5
        for i in range(5):
            same(got[k][i], want[k][i], (k, i, "file store"))
            same(got[k][i], dicts[k][i], (k, i, "scene dicts"))
            assert bool(torch.isfinite(got[k][i]).all())
    assert got["reg"][3].shape[0] > 64 and not got["reg"][0].requires_grad


def test_evaluate_store_records(fx, net):
    from lanegcn_amd.evaluate import evaluate_store
    got = evaluate_store(net, fx[6]["store"], 2).records()
    want = evaluate_store(net, fx[6]["file_store"], 2).records()
    assert got.dtype == want.dtype and got.shape == want.shape and got.shape[0] == 5
    assert got.tobytes() == want.tobytes()


def test_builder_errors_arrive_before_the_pack(batch5, net, monkeypatch):
    from lanegcn_amd import _lib, data_raw as D, ops
    raws, tables, lane_ids = batch5
    seen = []
    real = ops.store_pack
    monkeypatch.setattr(ops, "store_pack", lambda *a, **k: (seen.append("store_pack"), real(*a, **k))[1])
    bad = copy.deepcopy(raws[:3])
    bad[1]["steps"][3] = np.concatenate([bad[1]["steps"][3], bad[1]["steps"][3][:1]])
    bad[1]["trajs"][3] = np.concatenate([bad[1]["trajs"][3], bad[1]["trajs"][3][:1]])
    far = copy.deepcopy(raws[:3])
    far[2]["trajs"][0] = far[2]["trajs"][0] + 5000.0
    short = copy.deepcopy(raws[:3])
    short[2]["trajs"][0], short[2]["steps"][0] = short[2]["trajs"][0][:19], short[2]["steps"][0][:19]
    for scenes, msg in ((bad, "scene 1 track 3 lists a step twice"), (far, "scene 2: no lane survives"), (short, "scene 2.*20 rows")):
        with pytest.raises(_lib.LgcnError, match=msg):
            net.forward_raw(copy.deepcopy(scenes), tables, lane_ids=lane_ids[:3])
        with pytest.raises(_lib.LgcnError, match=msg):
            D.build_store(copy.deepcopy(scenes), tables, C.CONFIG, lane_ids=lane_ids[:3])
    with pytest.raises(_lib.LgcnError):
        D.build_store([], tables, C.CONFIG)
    assert seen == []
    assert len(D.build_store(copy.deepcopy(raws[2:3]), tables, C.CONFIG)) == 1 and seen == ["store_pack"]     # the next call starts clean
