"""GPU: a training step fed from the device scene store.  engine.flat_graph against lanegcn.graph_gather, and
Net.forward_store_train(store, pick[, rot_dt]) against Net.forward(collate_fn(scene dicts)) -- the same modules in the
same order on the same values, so outputs are compared with torch.equal and gradients against the dict path's OWN
run-to-run spread (expected 0: the library is bitwise repeatable).  Seeded state, f16x2, default switches.

With the default switches ActorNet trains on the stock NCL convolutions, and MIOpen's default choice of algorithm for them
is not repeatable on MI355X: Net.forward(data) under autograd differs from ITSELF run to run (actor_net's output by
~1e-6, measured; every later stage follows), while map_net, which runs no stock convolution, is bit-identical.  The
comparisons therefore run under torch.backends.cudnn.deterministic = True (the `repeatable` fixture, restored afterwards):
PyTorch's own setting, no switch of this package, and the one under which the dict path equals itself -- the premise of
an exact comparison."""
import os

import numpy as np
import pytest
import torch

import scene_store_cases as SC
import store_aug_cases as AC
import store_aug_model as AM
from oracle import lanegcn_oracle as O

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def fx(tmp_path_factory):
    import lanegcn_amd  # noqa: F401
    from lanegcn_amd.flatfile import DeviceSceneStore, write_scenes
    scenes = AC.make_scenes()
    d = tmp_path_factory.mktemp("store_train")
    path = str(d / "theta.npz")
    write_scenes(path, scenes, theta=True)
    write_scenes(str(d / "nogt.npz"), AC.make_scenes(gt=False), theta=True)
    return dict(scenes=scenes, path=path, dev=DeviceSceneStore(path), nogt=DeviceSceneStore(str(d / "nogt.npz")))


@pytest.fixture(scope="module")
def net(ref_state_names):
    import lanegcn_amd  # noqa: F401
    from lanegcn_amd import lanegcn as M
    from lanegcn_amd import ops
    assert ops.get_mma() == "f16x2"
    n = M.Net(M.config)
    n.load_state_dict(O.seeded_state(ref_state_names, 3), strict=True)
    n = n.cuda().train()
    assert len(list(n.parameters())) == 405
    return n


@pytest.fixture()
def repeatable():
    keep = torch.backends.cudnn.deterministic
    torch.backends.cudnn.deterministic = True
    yield
    torch.backends.cudnn.deterministic = keep


def same(got, want, what):
    assert got.dtype == want.dtype and tuple(got.shape) == tuple(want.shape), (what, got.dtype, got.shape, want.dtype, want.shape)
    assert got.device == want.device and torch.equal(got, want), what


def batch_of(scenes):
    from lanegcn_amd import data as gen
    return gen.collate_fn([gen.from_numpy(s) for s in scenes])


def test_flat_graph_equals_graph_gather(fx):
    from lanegcn_amd import lanegcn as M
    from lanegcn_amd.engine import collate_flat, flat_graph
    from lanegcn_amd.utils import to_long
    for name in ("repeat", "all", "no_left_right"):
        scenes = [fx["scenes"][i] for i in SC.PICKS[name]]
        want = M.graph_gather(to_long(batch_of(scenes)["graph"]))
        for got in (flat_graph(collate_flat(scenes)), flat_graph(fx["dev"].batch(SC.PICKS[name])[0])):
            assert sorted(got) == sorted(want) == sorted(["idcs", "ctrs", "feats", "turn", "control", "intersect", "pre", "suc",
                                                          "left", "right"])
            for k in ("idcs", "ctrs"):
                assert type(got[k]) is list and len(got[k]) == len(want[k]) == len(scenes)
                for i in range(len(scenes)):
                    same(got[k][i], want[k][i], (name, k, i))
            for k in ("feats", "turn", "control", "intersect"):
                same(got[k], want[k], (name, k))
            for k in ("pre", "suc"):
                assert type(got[k]) is list and len(got[k]) == len(want[k]) == 6
                for i in range(6):
                    for w in "uv":
                        same(got[k][i][w], want[k][i][w], (name, k, i, w))
            for k in ("left", "right"):
                for w in "uv":
                    same(got[k][w], want[k][w], (name, k, w))
                    assert got[k][w].dtype == torch.int64


def grads(net):
    return {n: (None if p.grad is None else p.grad.detach().clone()) for n, p in net.named_parameters()}


def dict_step(net, scenes):
    from lanegcn_amd import lanegcn as M
    data = batch_of(scenes)
    net.zero_grad(set_to_none=True)
    out = net(data)
    M.Loss(M.config).cuda()(out, data)["loss"].backward()
    return out, grads(net)


def store_step(net, store, pick, rot_dt=None):
    from lanegcn_amd import lanegcn as M
    net.zero_grad(set_to_none=True)
    out, data = net.forward_store_train(store, pick, rot_dt=rot_dt)
    M.Loss(M.config).cuda()(out, data)["loss"].backward()
    return out, data, grads(net)


def compare_steps(net, fx, pick, rot_dt=None):
    """Outputs torch.equal and recorded by autograd; every gradient within the dict path's own run-to-run difference."""
    scenes = [fx["scenes"][i] for i in pick] if rot_dt is None else AM.rotate_pick(fx["scenes"], pick, rot_dt)
    want, g0 = dict_step(net, scenes)
    _, g1 = dict_step(net, scenes)
    got, data, g = store_step(net, fx["dev"], pick, rot_dt)
    assert len(got["cls"]) == len(want["cls"]) == len(got["reg"]) == len(want["reg"]) == len(pick)
    for i in range(len(pick)):
        same(got["cls"][i], want["cls"][i], ("cls", i))
        same(got["reg"][i], want["reg"][i], ("reg", i))
        assert got["cls"][i].requires_grad and got["reg"][i].requires_grad, i
    assert len(g) == len(g0) == 405
    worst = 0.0
    for n in g0:
        assert (g0[n] is None) == (g1[n] is None) == (g[n] is None), n
        if g0[n] is None:
            continue
        d0 = float((g0[n] - g1[n]).abs().max())
        d = float((g[n] - g0[n]).abs().max())
        worst = max(worst, d0)
        assert bool(torch.isfinite(g[n]).all()), n
        assert d <= d0, (n, d, d0)
        if bool((g0[n] != 0).any()):
            assert bool((g[n] != 0).any()), n
    print("largest run-to-run difference of the dict path over the parameters: %.3e" % worst)
    assert sum(1 for n in g0 if g0[n] is not None and bool((g0[n] != 0).any())) > 350
    return got, data


def test_forward_and_gradients_equal_the_dict_path(fx, net, repeatable):
    pick = SC.PICKS["repeat"]
    got, data = compare_steps(net, fx, pick)
    assert got["reg"][0].shape == (7, 6, 30, 2) and sorted(data) == ["ctrs", "gt_preds", "has_preds", "orig", "rot"]
    for i, j in enumerate(pick):
        s = fx["scenes"][j]
        same(data["gt_preds"][i], torch.from_numpy(s["gt_preds"]).cuda(), ("gt_preds", i))
        same(data["has_preds"][i], torch.from_numpy(s["has_preds"]).cuda(), ("has_preds", i))
        same(data["rot"][i], torch.from_numpy(s["rot"]).cuda(), ("rot", i))
        same(data["orig"][i], torch.from_numpy(s["orig"]).cuda(), ("orig", i))
        same(data["ctrs"][i], torch.from_numpy(s["ctrs"]).cuda(), ("ctrs", i))


def test_forward_and_gradients_with_rot_dt_equal_the_dict_path_on_the_models_scenes(fx, net, repeatable):
    pick, dts = SC.PICKS["repeat"], AC.ROT_DT["repeat"]
    got, data = compare_steps(net, fx, pick, dts)
    turned = AM.rotate_pick(fx["scenes"], pick, dts)
    assert data["theta"].tolist() == [s["theta"] for s in turned]
    for i, s in enumerate(turned):
        same(data["rot"][i], torch.from_numpy(s["rot"]).cuda(), ("rot", i))
        same(data["ctrs"][i], torch.from_numpy(s["ctrs"]).cuda(), ("ctrs", i))
    plain, _ = net.forward_store_train(fx["dev"], pick)
    assert not torch.equal(plain["reg"][0], got["reg"][0])             # the rotation reaches the outputs


def test_a_batch_with_the_zero_actor_scene_does_what_the_dict_path_does(fx, net, repeatable):
    from lanegcn_amd import lanegcn as M
    pick = SC.PICKS["all"]
    scenes = [fx["scenes"][i] for i in pick]
    try:
        want = net(batch_of(scenes))
    except Exception as e:      # noqa: BLE001  (whatever the dict path raises is the expectation)
        with pytest.raises(type(e)):
            net.forward_store_train(fx["dev"], pick)
        return
    got, data = net.forward_store_train(fx["dev"], pick)
    for i in range(len(pick)):
        same(got["cls"][i], want["cls"][i], ("cls", i))
        same(got["reg"][i], want["reg"][i], ("reg", i))
    assert got["reg"][SC.NO_ACTORS].shape[0] == 0 and data["rot"][SC.NO_ACTORS] is None
    loss = M.Loss(M.config).cuda()(got, data)["loss"]
    assert bool(torch.isfinite(loss))


def test_forward_store_is_untouched(fx, net):
    pick = SC.PICKS["repeat"]
    with torch.no_grad():
        got = net.forward_store(fx["dev"], pick)
        want = net(batch_of([fx["scenes"][i] for i in pick]))
    for i in range(len(pick)):
        same(got["cls"][i], want["cls"][i], ("cls", i))
        same(got["reg"][i], want["reg"][i], ("reg", i))
        assert not got["reg"][i].requires_grad


def test_errors_come_before_any_launch(fx, net, tmp_path):
    from lanegcn_amd._lib import LgcnError
    from lanegcn_amd.flatfile import DeviceSceneStore, write_scenes
    fb, ex = fx["dev"].batch(SC.PICKS["all"])
    torch.cuda.synchronize()
    before = fb.buf_view().clone()
    calls = []
    for store in (fx["dev"], fx["nogt"]):
        keep = store.batch
        store.batch = lambda *a, _k=keep, **kw: (calls.append(1), _k(*a, **kw))[1]
    try:
        with pytest.raises(LgcnError, match="no actor"):
            net.forward_store_train(fx["dev"], SC.PICKS["no_actors"])
        with pytest.raises(LgcnError, match="gt_preds"):
            net.forward_store_train(fx["nogt"], SC.PICKS["repeat"])
        # a store whose scenes have no pre[5] / suc[5] edge: the reference's KeyError
        short = AC.make_scenes()[:1]
        for k in ("pre", "suc"):
            short[0]["graph"][k][5] = {"u": np.zeros(0, np.int64), "v": np.zeros(0, np.int64)}
        path = str(tmp_path / "short.npz")
        write_scenes(path, short, theta=True)
        s = DeviceSceneStore(path)
        keep = s.batch
        s.batch = lambda *a, **kw: (calls.append(1), keep(*a, **kw))[1]
        with pytest.raises(KeyError, match="node_idcs"):
            net.forward_store_train(s, [0])
        with pytest.raises(ValueError):
            net.forward_store_train(fx["dev"], SC.PICKS["repeat"], rot_dt=[0.1])
        with pytest.raises(IndexError):
            net.forward_store_train(fx["dev"], [6])
    finally:
        for store in (fx["dev"], fx["nogt"]):
            del store.batch
    assert calls == [1]                        # only the bad rot_dt got as far as batch(), which refuses it before launching
    torch.cuda.synchronize()
    assert torch.equal(fb.buf_view(), before)


def test_train_driver_from_a_store(fx, tmp_path):
    """train_dp.py --store: two iterations out of the resident store with rot_dt drawn per step, a checkpoint in the
    reference's format (in-process, like the driver test of test_gpu_training.py)."""
    import importlib
    import lanegcn_amd  # noqa: F401
    from lanegcn_amd import lanegcn as M
    train_dp = importlib.import_module("train_dp")
    save = str(tmp_path / "run")
    saved = dict(M.config)     # the driver writes batch_size / save_dir / epoch into the shared config
    try:
        rc = train_dp.main(["--store", fx["path"], "--rot-size", "6.28", "--max-iters", "2", "--batch-size", "2",
                            "--save-dir", save, "--dataset-len", "8"])
        assert rc == 0
        ckpts = sorted(os.listdir(save))
        assert len(ckpts) == 1 and ckpts[0].endswith(".ckpt")
        ck = torch.load(os.path.join(save, ckpts[0]), map_location="cpu", weights_only=True)
        assert set(ck) == {"epoch", "state_dict", "opt_state"} and len(ck["state_dict"]) == 405
    finally:
        M.config.clear()
        M.config.update(saved)
