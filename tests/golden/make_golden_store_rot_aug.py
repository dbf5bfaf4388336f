"""Generates tests/golden/store_rot_aug.npz by running the REFERENCE's own ArgoDataset.__getitem__ with rot_aug set
(data.py:35-65), imported read-only through make_golden.import_reference()'s stubs, on three small scenes in the
preprocessed schema.  Run in the build container only:
    python tests/golden/make_golden_store_rot_aug.py
The dataset object is made with __new__ and given train=True, config = {preprocess, rot_aug, rot_size = 2 pi} and the
three scenes as its `split`; np.random.seed(k) is set before item k, and the same seed gives the recorded dt.  The
fixture holds the input scenes, dt, the reference's outputs and the NumPy version it ran under as data, never reference
source.

The script ASSERTS that the model of tests/store_aug_model.py lies within its derived bound of the reference's np.matmul
on every rotated coordinate, and prints how much of the bound's first term the largest difference uses."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden as MG  # noqa: E402
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

ROT_SIZE = 2.0 * np.pi
ROTATED = (("feats",), ("ctrs",), ("graph", "ctrs"), ("graph", "feats"))


def input_scenes():
    """Three synth_scene scenes (36 / 90 / 72 nodes, 5 / 0 / 9 actors) with a heading, the rot that belongs to it, a
    world origin and the graph keys that the reference's rot_aug branch copies."""
    from lanegcn_amd import data as gen
    rng = np.random.default_rng(45)
    scenes = [gen.synth_scene(rng, roads, a) for roads, a in (([2], 5), ([5], 0), ([2, 2], 9))]
    for s in scenes:
        theta = float(rng.uniform(-np.pi, np.pi))
        s["theta"] = theta
        s["rot"] = np.asarray([[np.cos(theta), -np.sin(theta)], [np.sin(theta), np.cos(theta)]], np.float32)
        s["orig"] = rng.uniform(-500, 500, 2).astype(np.float32)
        s["has_preds"] = rng.random(s["has_preds"].shape) < 0.7
        s["graph"]["left_pairs"] = np.zeros((0, 2), np.int64)
        s["graph"]["right_pairs"] = np.zeros((0, 2), np.int64)
    return scenes


def get(tree, path):
    for k in path:
        tree = tree[k]
    return tree


def main():
    _, refdata = MG.import_reference()
    import lanegcn_amd  # noqa: F401
    import store_aug_model as AM
    from golden_io import flatten

    scenes = input_scenes()
    ds = refdata.ArgoDataset.__new__(refdata.ArgoDataset)
    ds.config = {"preprocess": True, "rot_aug": True, "rot_size": ROT_SIZE}
    ds.train = True
    ds.split = scenes
    outs, dts = [], []
    for k in range(len(scenes)):
        np.random.seed(k)
        outs.append(ds[k])
        np.random.seed(k)
        dts.append(np.random.rand() * ROT_SIZE)
    used, count = 0.0, 0
    for s, o, dt in zip(scenes, outs, dts):
        new, rot, rm = AM.matrices(s["theta"], dt)
        assert new == o["theta"] and np.array_equal(rot, o["rot"])
        m = AM.rotate_scene(s, dt)
        for path in ROTATED:
            src = np.asarray(get(s, path), np.float32)[..., :2]
            got, want = get(m, path)[..., :2].astype(np.float64), np.asarray(get(o, path))[..., :2].astype(np.float64)
            assert (np.abs(got - want) <= AM.bound(src, rm)).all(), path
            first = 4.5 * 2.0 ** -24 * (np.abs(src[..., :1].astype(np.float64) * rm[0]) + np.abs(src[..., 1:].astype(np.float64) * rm[1]))
            ok = first > 0
            used = max(used, float((np.abs(got - want)[ok] / first[ok]).max()) if ok.any() else 0.0)
            count += got.size
    out = {"numpy_version": np.asarray(np.__version__), "dt": np.asarray(dts, np.float64), "rot_size": np.float64(ROT_SIZE)}
    flatten(scenes, "scenes/", out)
    flatten(outs, "want/", out)
    path = os.path.join(HERE, "store_rot_aug.npz")
    np.savez_compressed(path, **out)
    assert os.path.getsize(path) < 1000000, os.path.getsize(path)
    print("wrote store_rot_aug.npz (%d bytes), NumPy %s; %d rotated coordinates, the reference's np.matmul uses %.2f of the "
          "bound's first term at most" % (os.path.getsize(path), np.__version__, count, used))


if __name__ == "__main__":
    main()
