"""CPU: the training rotation of a stored scene (reference data.py:45-63).  The numpy model of store_aug_model.py against
the recording of the reference's own __getitem__ (tests/golden/store_rot_aug.npz), then lanegcn_amd.flatfile against the
model: the tables bit for bit, the host batch byte for byte.

Bound of a rotated coordinate against the reference's np.matmul, whose evaluation order is BLAS's: derived, not measured
(store_aug_model.bound): 4.5 * 2^-24 * (|x Rm0c| + |y Rm1c|) + 2^-23 * (|x| + |y|)."""
import os

import numpy as np
import pytest
import torch

import scene_store_cases as SC
import store_aug_cases as AC
import store_aug_model as AM
from golden_io import load_scenes, unflatten

HERE = os.path.dirname(os.path.abspath(__file__))
ROTATED = (("feats",), ("ctrs",), ("graph", "ctrs"), ("graph", "feats"))


@pytest.fixture(scope="module")
def rec():
    with np.load(os.path.join(HERE, "golden", "store_rot_aug.npz"), allow_pickle=False) as z:
        flat = {k: z[k] for k in z.files}
    return dict(scenes=load_scenes(flat, "scenes"), want=load_scenes(flat, "want"), dt=flat["dt"], rot_size=float(flat["rot_size"]))


def get(tree, path):
    for k in path:
        tree = tree[k]
    return tree


def leaves(tree, prefix=()):
    if isinstance(tree, dict):
        for k, v in tree.items():
            yield from leaves(v, prefix + (k,))
    elif isinstance(tree, (list, tuple)):
        for i, v in enumerate(tree):
            yield from leaves(v, prefix + (i,))
    else:
        yield prefix, tree


def test_model_against_the_reference_recording(rec):
    assert len(rec["scenes"]) == len(rec["want"]) == len(rec["dt"]) == 3
    seen = 0
    for s, w, dt in zip(rec["scenes"], rec["want"], rec["dt"]):
        m = AM.rotate_scene(s, dt)
        new, rot, rm = AM.matrices(s["theta"], dt)
        assert m["theta"] == new == float(w["theta"])
        assert w["rot"].dtype == np.float32 and np.abs(m["rot"].astype(np.float64) - w["rot"]).max() <= 2.0 ** -23
        todo = dict(leaves(w))
        del todo[("theta",)], todo[("rot",)]
        for path in ROTATED:
            src = np.asarray(get(s, path), np.float32)
            got, want = get(m, path), todo.pop(path)
            assert got.dtype == want.dtype == np.float32 and got.shape == want.shape == src.shape, path
            err = np.abs(got[..., :2].astype(np.float64) - want[..., :2])
            assert (err <= AM.bound(src[..., :2], rm)).all(), (path, float(err.max()))
            if src.shape[-1] == 3:      # feats[:, :, 2] is not a coordinate
                assert np.array_equal(got[..., 2], src[..., 2]) and np.array_equal(want[..., 2], src[..., 2])
            seen += got.size
        # everything else: the reference hands the scene's own values on, and so does the model
        assert {p for p in todo} == {p for p, _ in leaves(s)} - set(ROTATED) - {("theta",), ("rot",)}
        for path, want in todo.items():
            got, src = np.asarray(get(m, path)), np.asarray(get(s, path))
            assert got.dtype == src.dtype and np.array_equal(got, want) and np.array_equal(src, want), path
            seen += got.size
        assert seen > 0
    assert {p for p, _ in leaves(rec["want"][0])} >= {("orig",), ("gt_preds",), ("has_preds",), ("graph", "turn"),
                                                      ("graph", "control"), ("graph", "intersect"), ("graph", "left", "u")}


def test_tables_agree_with_the_model_bit_for_bit(rec):
    from lanegcn_amd.flatfile import rot_aug_tables
    scenes = AC.make_scenes()
    cases = [(float(s["theta"]), float(dt)) for s, dt in zip(rec["scenes"], rec["dt"])]
    for name, pick in SC.PICKS.items():
        cases += [(scenes[i]["theta"], dt) for i, dt in zip(pick, AC.ROT_DT[name])]
    cases += [(0.3, 0.0), (-2.0, np.pi), (1.0, 2.0 * np.pi), (0.0, 1e-9)]
    theta, dt = np.array([c[0] for c in cases]), np.array([c[1] for c in cases])
    new, aug = rot_aug_tables(theta, dt)
    assert new.dtype == np.float64 and new.shape == (len(cases),) and aug.dtype == np.float32 and aug.shape == (len(cases), 8)
    for k, (th, d) in enumerate(cases):
        want_new, rot, rm = AM.matrices(th, d)
        assert new[k] == want_new
        assert aug[k, :4].tobytes() == rm.tobytes() and aug[k, 4:].tobytes() == rot.tobytes(), k


def test_draw_rot_dt(rec):
    from lanegcn_amd.flatfile import draw_rot_dt
    for k, dt in enumerate(rec["dt"]):
        np.random.seed(k)
        got = draw_rot_dt(1, rec["rot_size"])
        assert got.dtype == np.float64 and got.shape == (1,) and got[0] == dt
    np.random.seed(4)
    want = [np.random.rand() * 0.5 for _ in range(5)]
    np.random.seed(4)
    assert draw_rot_dt(5, 0.5).tolist() == want                      # one rand() per scene, in pick order
    a = draw_rot_dt(7, 3.0, np.random.default_rng(2))
    assert a.shape == (7,) and np.array_equal(a, np.random.default_rng(2).random(7) * 3.0) and (a >= 0).all() and (a < 3.0).all()


@pytest.fixture(scope="module")
def store(tmp_path_factory):
    import lanegcn_amd  # noqa: F401
    from lanegcn_amd.flatfile import FlatSceneFile, write_scenes
    scenes = AC.make_scenes()
    d = tmp_path_factory.mktemp("store_aug")
    write_scenes(str(d / "theta.npz"), scenes, theta=True)
    write_scenes(str(d / "plain.npz"), scenes)
    return dict(scenes=scenes, host=FlatSceneFile(str(d / "theta.npz")), plain=FlatSceneFile(str(d / "plain.npz")))


def same(got, want, what):
    assert got.dtype == want.dtype and tuple(got.shape) == tuple(want.shape), (what, got.dtype, got.shape, want.dtype, want.shape)
    assert got.numpy().tobytes() == want.numpy().tobytes(), what


def check_host_batch(got, scenes, what=""):
    """(FlatBatch, extras) on the CPU against scene dicts collated by collate_flat_host / host_actor_inputs, byte for byte."""
    from lanegcn_amd.engine import collate_flat_host, host_actor_inputs
    fb, ex = got
    hfb = collate_flat_host(scenes, pin=False)
    wfb = hfb.to("cpu")
    for f in SC.FLAT_FIELDS:
        assert getattr(fb, f) == getattr(wfb, f), (what, f)
    for f in SC.FLAT_ARRAYS:
        same(getattr(fb, f), getattr(wfb, f), (what, f))
    feats, rot, orig, sizes = host_actor_inputs(scenes)
    assert ex["sizes"] == sizes
    same(ex["actor_feats"], feats, (what, "actor_feats"))
    same(ex["rot"], rot, (what, "rot"))
    same(ex["orig"], orig, (what, "orig"))
    same(ex["gt_preds"], torch.from_numpy(np.concatenate([s["gt_preds"] for s in scenes])), (what, "gt_preds"))
    same(ex["has_preds"], torch.from_numpy(np.concatenate([s["has_preds"] for s in scenes])), (what, "has_preds"))


@pytest.mark.parametrize("name", sorted(SC.PICKS))
def test_host_batch_equals_the_model(store, name):
    pick, dts = SC.PICKS[name], AC.ROT_DT[name]
    got = store["host"].batch(pick, device="cpu", rot_dt=dts)
    turned = AM.rotate_pick(store["scenes"], pick, dts)
    check_host_batch(got, turned, name)
    assert sorted(got[1]) == ["actor_feats", "gt_preds", "has_preds", "orig", "rot", "sizes", "theta"]
    theta = got[1]["theta"]
    assert isinstance(theta, np.ndarray) and theta.dtype == np.float64 and theta.tolist() == [s["theta"] for s in turned]
    # a list, a tuple and an array of angles are the same thing
    again = store["host"].batch(np.asarray(pick), device="cpu", rot_dt=list(dts))
    for f in SC.FLAT_ARRAYS:
        same(getattr(again[0], f), getattr(got[0], f), f)
    if name == "repeat":
        assert pick[1] == pick[2] and dts[1] != dts[2] and dts[3] == 0.0
        a0, a1, a2 = np.cumsum([0] + got[1]["sizes"])[1:4]
        assert not torch.equal(got[0].actor_ctrs[a0:a1], got[0].actor_ctrs[a1:a2])


def test_rot_dt_none_is_todays_path(store):
    for src in (store["host"], store["plain"]):
        for name in ("repeat", "all", "no_actors"):
            pick = SC.PICKS[name]
            a, b = src.batch(pick, device="cpu"), src.batch(pick, device="cpu", rot_dt=None)
            check_host_batch(a, [store["scenes"][i] for i in pick], name)
            check_host_batch(b, [store["scenes"][i] for i in pick], name)
            assert sorted(a[1]) == sorted(b[1]) == ["actor_feats", "gt_preds", "has_preds", "orig", "rot", "sizes"]


def test_write_scenes_default_keeps_todays_keys(store):
    today = {"num_scales", "node_off", "actor_off", "edge_off", "rel_off", "edge_u", "edge_v", "actor_ctrs", "actor_feats", "rot",
             "orig", "node_ctrs", "node_feats", "turn", "control", "intersect", "gt_preds", "has_preds"}
    assert set(store["plain"].a) == today and store["plain"].theta is None
    assert set(store["host"].a) == today | {"theta"}
    th = store["host"].theta
    assert th.dtype == np.float64 and th.tolist() == [s["theta"] for s in store["scenes"]]
    for k in today:
        assert store["host"].a[k].tobytes() == store["plain"].a[k].tobytes() and store["host"].a[k].dtype == store["plain"].a[k].dtype


def test_refusals(store):
    from lanegcn_amd._lib import LgcnError
    host, pick = store["host"], SC.PICKS["repeat"]
    for bad in ([0.1, 0.2, 0.3], [0.1] * 5, [0.1, 0.2, float("nan"), 0.3], [0.1, float("inf"), 0.2, 0.3], 0.5,
                [[0.1, 0.2, 0.3, 0.4]], ["a", "b", "c", "d"], [0.1, None, 0.2, 0.3]):
        with pytest.raises(ValueError):
            host.batch(pick, device="cpu", rot_dt=bad)
    with pytest.raises(LgcnError):
        store["plain"].batch(pick, device="cpu", rot_dt=[0.1, 0.2, 0.3, 0.4])
    with pytest.raises(ValueError):                                     # the shape of rot_dt is judged first
        store["plain"].batch(pick, device="cpu", rot_dt=[0.1])
