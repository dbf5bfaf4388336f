"""GPU: DeviceSceneStore.batch(pick, rot_dt=...) -- lgcn_store_gather_aug, the gather launch with the reference's training
rotation inside -- against the host path FlatSceneFile.batch(pick, "cuda", rot_dt=...) and against the independent numpy
model of store_aug_model.py.  The arithmetic is fixed (two rounded fp32 products, one rounded add), so every comparison is
torch.equal with matching dtype and shape, or bytes."""
import numpy as np
import pytest
import torch

import scene_store_cases as SC
import store_aug_cases as AC
import store_aug_model as AM

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def fx(tmp_path_factory):
    """The six scenes with theta as scene dicts, as a host store and as a device store; per pick the host path's batch
    with and without the pick's angles (computed once, never modified)."""
    import lanegcn_amd  # noqa: F401
    from lanegcn_amd.flatfile import DeviceSceneStore, FlatSceneFile, write_scenes
    scenes = AC.make_scenes()
    d = tmp_path_factory.mktemp("store_aug")
    path, plain = str(d / "theta.npz"), str(d / "plain.npz")
    write_scenes(path, scenes, theta=True)
    write_scenes(plain, scenes)
    host = FlatSceneFile(path)
    want = {name: host.batch(pick, "cuda", rot_dt=AC.ROT_DT[name]) for name, pick in SC.PICKS.items()}
    today = {name: host.batch(pick, "cuda") for name, pick in SC.PICKS.items()}
    return dict(scenes=scenes, host=host, dev=DeviceSceneStore(path), plain=DeviceSceneStore(plain), want=want, today=today)


def same(got, want, what):
    assert got.dtype == want.dtype and tuple(got.shape) == tuple(want.shape), (what, got.dtype, got.shape, want.dtype, want.shape)
    assert got.device == want.device and torch.equal(got, want), what


def check_batch(got, want, what=""):
    """The criterion of test_gpu_scene_store.check_batch: every field, array and extra; `theta` is a host float64 array."""
    (fb, ex), (wfb, wex) = got, want
    for f in SC.FLAT_FIELDS:
        assert getattr(fb, f) == getattr(wfb, f), (what, f)
    for f in SC.FLAT_ARRAYS:
        same(getattr(fb, f), getattr(wfb, f), (what, f))
    assert sorted(ex) == sorted(wex), what
    assert ex["sizes"] == wex["sizes"] and type(ex["sizes"]) is list and all(type(x) is int for x in ex["sizes"])
    for k in wex:
        if k == "theta":
            assert isinstance(ex[k], np.ndarray) and ex[k].dtype == np.float64 and np.array_equal(ex[k], wex[k]), what
        elif k != "sizes":
            same(ex[k], wex[k], (what, k))


def check_model(got, scenes, what=""):
    """Against scene dicts (the model's), collated as the dict path collates them."""
    from lanegcn_amd.engine import collate_flat_host, host_actor_inputs
    fb, ex = got
    wfb = collate_flat_host(scenes).to()
    for f in SC.FLAT_ARRAYS:
        same(getattr(fb, f), getattr(wfb, f), (what, f))
    feats, rot, orig, sizes = host_actor_inputs(scenes)
    assert ex["sizes"] == sizes
    for k, w in (("actor_feats", feats), ("rot", rot), ("orig", orig),
                 ("gt_preds", torch.from_numpy(np.concatenate([s["gt_preds"] for s in scenes]))),
                 ("has_preds", torch.from_numpy(np.concatenate([s["has_preds"] for s in scenes])))):
        same(ex[k], w.cuda(), (what, k))


@pytest.mark.parametrize("name", sorted(SC.PICKS))
def test_augmented_batch_equals_the_host_path_and_the_model(fx, name):
    pick, dts = SC.PICKS[name], AC.ROT_DT[name]
    got = fx["dev"].batch(pick, rot_dt=dts)
    check_batch(got, fx["want"][name], name)
    check_batch(fx["dev"].batch(np.asarray(pick), rot_dt=list(dts)), fx["want"][name], name)
    turned = AM.rotate_pick(fx["scenes"], pick, dts)
    check_model(got, turned, name)
    assert got[1]["theta"].tolist() == [s["theta"] for s in turned]
    if name == "repeat":      # scene 1 twice, by two angles; the last pick by 0.0 exactly; Rm with off-diagonals of both signs
        assert pick[1] == pick[2] and dts[1] != dts[2] and dts[3] == 0.0
        rm = AM.matrices(0.0, dts[0])[2]
        assert min(rm[0, 1], rm[1, 0]) < 0 < max(rm[0, 1], rm[1, 0])
        off = np.cumsum([0] + got[1]["sizes"])
        a, b = got[0].actor_ctrs[off[1]:off[2]], got[0].actor_ctrs[off[2]:off[3]]
        assert a.shape == b.shape and not torch.equal(a, b)
        assert not torch.equal(got[1]["rot"][off[1]], got[1]["rot"][off[2]])
        # dt = 0.0 goes through the arithmetic and gives the stored values back
        same(got[0].actor_ctrs[off[3]:], fx["today"][name][0].actor_ctrs[off[3]:], "dt = 0")
        # what the rotation does not touch is today's
        for f in ("turn", "control", "intersect", "node_off", "actor_off", "idx_local", "seg_off", "seg_base"):
            same(getattr(got[0], f), getattr(fx["today"][name][0], f), f)
        for k in ("orig", "gt_preds", "has_preds"):
            same(got[1][k], fx["today"][name][1][k], k)
        same(got[1]["actor_feats"][:, 2], fx["today"][name][1]["actor_feats"][:, 2], "feats[:, :, 2]")
        assert not torch.equal(got[0].node_ctrs, fx["today"][name][0].node_ctrs)
    if name == "seventy":
        assert got[0].node_off.numel() > 64 and got[0].seg_base.numel() == 1960 > 1024
    if name == "no_actors":
        assert got[0].n_actors == 0 and got[1]["actor_feats"].shape == (0, 3, 20) and got[1]["rot"].shape == (0, 2, 2)


@pytest.mark.parametrize("name", ["repeat", "all", "no_actors"])
def test_layout_is_still_the_host_staging_layout(fx, name):
    """The flat buffer holds, at the 256-byte aligned offsets of engine._FLAT_ARRAYS, the bytes that collate_flat_host packs
    for the model's rotated scenes."""
    from lanegcn_amd.engine import _FLAT_ARRAYS, collate_flat_host
    pick, dts = SC.PICKS[name], AC.ROT_DT[name]
    fb, _ = fx["dev"].batch(pick, rot_dt=dts)
    hfb = collate_flat_host(AM.rotate_pick(fx["scenes"], pick, dts))
    buf = fb.buf_view()
    assert buf is not None and buf.dtype == torch.uint8 and buf.is_cuda and buf.numel() == hfb.buf.numel()
    got, at = buf.cpu(), 0
    for f in _FLAT_ARRAYS:
        off, dt, shape = hfb.layout[f]
        t = getattr(fb, f)
        nbytes = t.numel() * t.element_size()
        assert off % 256 == 0 and off >= at and tuple(t.shape) == shape and str(t.dtype) == "torch." + dt, f
        assert t.storage_offset() * t.element_size() == buf.storage_offset() + off and t.is_contiguous(), f
        assert t.untyped_storage().data_ptr() == buf.untyped_storage().data_ptr(), f
        assert torch.equal(got[off:off + nbytes], hfb.buf[off:off + nbytes]), f
        at = off + nbytes
    assert at <= buf.numel()


def test_back_to_back_augmented_calls_do_not_alias(fx):
    """Eight augmented batches with no synchronisation in between, on the current stream and on a side stream: each equals
    the host path's afterwards -- outputs do not alias, and no call reuses the staging (offset table and rotation table in
    one pinned block) that an earlier copy may still read."""
    dev, host = fx["dev"], fx["host"]
    rng = np.random.default_rng(6)
    picks = [[int(i) for i in rng.integers(0, 6, n)] for n in (4, 1, 9, 33, 2, 70, 5, 4)]
    dts = [rng.uniform(0, 2 * np.pi, len(p)) for p in picks]
    want = [host.batch(p, "cuda", rot_dt=d) for p, d in zip(picks, dts)]
    torch.cuda.synchronize()
    got = [dev.batch(p, rot_dt=d) for p, d in zip(picks, dts)]
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        got_side = [dev.batch(p, rot_dt=d) for p, d in zip(picks, dts)]
    torch.cuda.synchronize()
    for i, w in enumerate(want):
        check_batch(got[i], w, ("current", i))
        check_batch(got_side[i], w, ("side", i))
    bufs = [g[0].buf_view() for g in got + got_side] + [g[1]["actor_feats"] for g in got + got_side if g[0].n_actors]
    spans = sorted((b.data_ptr(), b.data_ptr() + b.numel() * b.element_size()) for b in bufs)
    assert all(a[1] <= b[0] for a, b in zip(spans, spans[1:]))


@pytest.mark.parametrize("name", sorted(SC.PICKS))
def test_without_rot_dt_the_batch_is_todays(fx, name):
    pick = SC.PICKS[name]
    for store in (fx["dev"], fx["plain"]):
        check_batch(store.batch(pick), fx["today"][name], name)
        check_batch(store.batch(pick, rot_dt=None), fx["today"][name], name)
    check_model(fx["dev"].batch(pick), [fx["scenes"][i] for i in pick], name)


def test_bad_rot_dt_raises_and_launches_nothing(fx):
    from lanegcn_amd._lib import LgcnError
    dev, pick, dts = fx["dev"], SC.PICKS["repeat"], AC.ROT_DT["repeat"]
    fb, ex = dev.batch(pick, rot_dt=dts)
    torch.cuda.synchronize()
    before = fb.buf_view().clone(), ex["actor_feats"].clone(), ex["rot"].clone()
    for bad in ([0.1, 0.2, 0.3], [0.1] * 5, [0.1, 0.2, float("nan"), 0.3], [0.1, float("-inf"), 0.2, 0.3], 0.5,
                [[0.1, 0.2, 0.3, 0.4]], ["a", "b", "c", "d"]):
        with pytest.raises(ValueError):
            dev.batch(pick, rot_dt=bad)
        with pytest.raises(ValueError):
            fx["host"].batch(pick, "cuda", rot_dt=bad)
    with pytest.raises(LgcnError):
        fx["plain"].batch(pick, rot_dt=dts)
    with pytest.raises(IndexError):
        dev.batch([0, 6], rot_dt=[0.1, 0.2])
    torch.cuda.synchronize()
    assert torch.equal(fb.buf_view(), before[0]) and torch.equal(ex["actor_feats"], before[1]) and torch.equal(ex["rot"], before[2])
    check_batch((fb, ex), fx["want"]["repeat"])


def test_wrapper_refuses_half_a_table(fx):
    from lanegcn_amd import ops
    from lanegcn_amd._lib import LgcnError
    dev = fx["dev"]
    p = dev.plan([0])
    tab = torch.from_numpy(p.table.copy())
    with pytest.raises(LgcnError):
        ops.store_gather(dev._job, tab, tab.cuda(), 1, p.n_rel, p.n_nodes, p.n_actors, p.n_elem, {}, aug_host=torch.zeros(8))
    with pytest.raises(LgcnError):
        ops.store_gather(dev._job, tab, tab.cuda(), 1, p.n_rel, p.n_nodes, p.n_actors, p.n_elem, {}, aug_host=torch.zeros(7),
                         aug_dev=torch.zeros(7, device="cuda"))
