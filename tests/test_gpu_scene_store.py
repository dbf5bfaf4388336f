"""GPU: flatfile.DeviceSceneStore (lgcn_store_gather: one launch cuts a batch out of the device-resident store) against
the host path FlatSceneFile.batch.  Pure data movement: every comparison is torch.equal with matching dtype and shape."""
import numpy as np
import pytest
import torch

import scene_store_cases as SC
from oracle import lanegcn_oracle as O

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def fx(tmp_path_factory):
    """The six-scene fixture as scene dicts, as a host store and as a device store, and the host path's batch per pick
    (computed once, never modified)."""
    import lanegcn_amd  # noqa: F401
    from lanegcn_amd.flatfile import DeviceSceneStore, FlatSceneFile, write_scenes
    scenes = SC.make_scenes()
    path = str(tmp_path_factory.mktemp("store") / "split.npz")
    write_scenes(path, scenes)
    host = FlatSceneFile(path)
    want = {name: host.batch(pick, "cuda") for name, pick in SC.PICKS.items()}
    return dict(scenes=scenes, path=path, host=host, dev=DeviceSceneStore(path), want=want)


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
    assert ex["sizes"] == wex["sizes"] and type(ex["sizes"]) is list and all(type(x) is int for x in ex["sizes"])
    for k in wex:
        if k != "sizes":
            same(ex[k], wex[k], (what, k))


def test_store_attributes(fx):
    dev, host = fx["dev"], fx["host"]
    assert len(dev) == dev.n_scenes == 6 and dev.num_scales == host.num_scales == 6
    arrays = [k for k in host.a if k not in ("num_scales", "node_off", "actor_off", "edge_off", "rel_off")]
    assert dev.nbytes == sum(host.a[k].nbytes for k in arrays)
    assert all(isinstance(getattr(dev, k), np.ndarray) for k in ("node_off", "actor_off", "edge_off", "rel_off"))
    from lanegcn_amd.flatfile import DeviceSceneStore
    again = DeviceSceneStore(host)                                   # from a FlatSceneFile instead of a path
    check_batch(again.batch([5, 2]), host.batch([5, 2], "cuda"))


@pytest.mark.parametrize("name", sorted(SC.PICKS))
def test_batch_equals_the_host_path(fx, name):
    pick = SC.PICKS[name]
    got = fx["dev"].batch(pick)
    check_batch(got, fx["want"][name], name)
    check_batch(fx["dev"].batch(np.asarray(pick)), fx["want"][name], name)
    if name == "seventy":
        assert got[0].node_off.numel() > 64 and got[0].seg_base.numel() == 1960 > 1024
    if name == "no_left_right":
        assert got[0].n_edges[-2:] == [0, 0] and got[0].idx_local.numel() > 0
    if name == "no_actors":
        assert got[0].n_actors == 0 and got[1]["actor_feats"].shape == (0, 3, 20) and got[1]["sizes"] == [0]


@pytest.mark.parametrize("name", ["repeat", "all", "no_actors"])
def test_layout_is_the_host_staging_layout(fx, name):
    """The arrays are views of buf_view() at the 256-byte aligned offsets of engine._FLAT_ARRAYS, and hold the bytes
    that collate_flat_host packs for the same scenes at the same offsets."""
    from lanegcn_amd.engine import _FLAT_ARRAYS, collate_flat_host
    pick = SC.PICKS[name]
    fb, _ = fx["dev"].batch(pick)
    hfb = collate_flat_host([fx["scenes"][i] for i in pick])
    buf = fb.buf_view()
    assert buf is not None and buf.dtype == torch.uint8 and buf.is_cuda and buf.numel() == hfb.buf.numel()
    assert list(hfb.layout) == list(_FLAT_ARRAYS) == list(SC.FLAT_ARRAYS)
    got, at = buf.cpu(), 0
    for f in _FLAT_ARRAYS:
        off, dt, shape = hfb.layout[f]
        t = getattr(fb, f)
        nbytes = t.numel() * t.element_size()
        assert off % 256 == 0 and off >= at and tuple(t.shape) == shape and str(t.dtype) == "torch." + dt, f
        # (an empty tensor's data_ptr() is 0: the place of a view is its storage offset)
        assert t.storage_offset() * t.element_size() == buf.storage_offset() + off and t.is_contiguous(), f
        assert nbytes == 0 or t.data_ptr() == buf.data_ptr() + off, f
        assert t.untyped_storage().data_ptr() == buf.untyped_storage().data_ptr(), f
        assert torch.equal(got[off:off + nbytes], hfb.buf[off:off + nbytes]), f
        at = off + nbytes
    assert at <= buf.numel()


def test_back_to_back_calls_do_not_alias(fx):
    """Eight batches with no synchronisation in between, on the current stream and on a side stream: each equals the host
    path's afterwards -- outputs do not alias and no call reuses staging that an earlier copy may still read."""
    dev, host = fx["dev"], fx["host"]
    rng = np.random.default_rng(5)
    picks = [[int(i) for i in rng.integers(0, 6, n)] for n in (4, 1, 9, 33, 2, 70, 5, 4)]
    want = [host.batch(p, "cuda") for p in picks]
    torch.cuda.synchronize()
    got = [dev.batch(p) for p in picks]
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        got_side = [dev.batch(p) for p in picks]
    torch.cuda.synchronize()
    for i, w in enumerate(want):
        check_batch(got[i], w, ("current", i))
        check_batch(got_side[i], w, ("side", i))
    bufs = [g[0].buf_view() for g in got + got_side] + [g[1]["actor_feats"] for g in got + got_side if g[0].n_actors]
    spans = sorted((b.data_ptr(), b.data_ptr() + b.numel() * b.element_size()) for b in bufs)
    assert all(a[1] <= b[0] for a, b in zip(spans, spans[1:]))


def test_store_without_gt_preds(tmp_path):
    import lanegcn_amd  # noqa: F401
    from lanegcn_amd.flatfile import DeviceSceneStore, FlatSceneFile, write_scenes
    path = str(tmp_path / "nogt.npz")
    write_scenes(path, SC.make_scenes(gt=False))
    host, dev = FlatSceneFile(path), DeviceSceneStore(path)
    for pick in (SC.PICKS["repeat"], SC.PICKS["all"]):
        got = dev.batch(pick)
        assert sorted(got[1]) == ["actor_feats", "orig", "rot", "sizes"]
        check_batch(got, host.batch(pick, "cuda"))


@pytest.fixture(scope="module")
def net(ref_state_names):
    import lanegcn_amd  # noqa: F401
    from lanegcn_amd import lanegcn as M
    n = M.Net(M.config)
    n.load_state_dict(O.seeded_state(ref_state_names, 3), strict=True)
    return n.cuda().eval()


def test_engine_forward_is_bitwise_that_of_the_host_batch(fx, net):
    from lanegcn_amd.engine import FullNetEngine
    eng = FullNetEngine(net)
    with torch.no_grad():
        for name in ("repeat", "all"):
            outs = []
            for fb, ex in (fx["dev"].batch(SC.PICKS[name]), fx["want"][name]):
                outs.append(eng.forward(fb, ex["actor_feats"], ex["rot"], ex["orig"], ex["sizes"]))
            assert outs[0]["cls"].shape == (sum(fx["want"][name][1]["sizes"]), 6)
            same(outs[0]["cls"], outs[1]["cls"], (name, "cls"))
            same(outs[0]["reg"], outs[1]["reg"], (name, "reg"))
            assert bool(torch.isfinite(outs[0]["reg"]).all())


@pytest.mark.parametrize("cache", [True, False])
def test_net_forward_store_equals_net_forward(fx, net, cache):
    """Net.forward_store(store, pick) == Net.forward(collate_fn(scenes)) list by list, in the default f16x2 mode, with
    Net's graph cache on (eager, captured, replayed) and off."""
    from lanegcn_amd import data as gen
    from lanegcn_amd import lanegcn as M
    from lanegcn_amd import ops
    assert ops.get_mma() == "f16x2"
    pick = SC.PICKS["repeat"]
    keep = M.Net.graph_cache
    M.Net.graph_cache = cache
    net.__dict__.pop("_graph_state", None)
    try:
        with torch.no_grad():
            got = net.forward_store(fx["dev"], pick)
            for _ in range(3 if cache else 1):
                want = net(gen.collate_fn([fx["scenes"][i] for i in pick]))
                assert len(got["cls"]) == len(want["cls"]) == len(got["reg"]) == len(want["reg"]) == len(pick)
                for i in range(len(pick)):
                    same(got["cls"][i], want["cls"][i], ("cls", i))
                    same(got["reg"][i], want["reg"][i], ("reg", i))
            assert (net.__dict__["_graph_state"]["graph"] is not None) == cache
    finally:
        M.Net.graph_cache = keep
        net.__dict__.pop("_graph_state", None)
    assert got["reg"][0].shape == (7, 6, 30, 2) and not got["reg"][0].requires_grad


def test_bad_picks_raise_and_launch_nothing(fx):
    from lanegcn_amd._lib import LgcnError
    dev = fx["dev"]
    fb, ex = dev.batch(SC.PICKS["all"])
    torch.cuda.synchronize()
    before = fb.buf_view().clone(), ex["actor_feats"].clone()
    for bad in ([-1], [0, dev.n_scenes], [dev.n_scenes]):
        with pytest.raises(IndexError):
            dev.batch(bad)
        with pytest.raises(IndexError):
            dev.plan(bad)
    with pytest.raises(LgcnError):
        dev.batch([])
    torch.cuda.synchronize()
    assert torch.equal(fb.buf_view(), before[0]) and torch.equal(ex["actor_feats"], before[1])
    check_batch((fb, ex), fx["want"]["all"])
