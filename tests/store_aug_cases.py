"""Fixture of the rotation-augmentation tests (test_store_aug_model_host.py, test_gpu_store_aug.py, test_gpu_store_train.py):
the six scenes of scene_store_cases with a heading `theta` each and the `rot` that belongs to it, formed as the reference
forms rot (data.py:163-166: float64 cos / sin, rounded to float32), and the angles of every pick."""
import numpy as np

import scene_store_cases as SC


def make_scenes(gt=True):
    scenes = SC.make_scenes(gt)
    rng = np.random.default_rng(33)
    for s in scenes:
        theta = float(rng.uniform(-np.pi, np.pi))
        s["theta"] = theta
        s["rot"] = np.asarray([[np.cos(theta), -np.sin(theta)], [np.sin(theta), np.cos(theta)]], np.float32)
    return scenes


def _angles():
    """Per pick of SC.PICKS, one angle per picked scene from a seeded generator over [0, 2 pi).  "repeat" = [3, 1, 1, 0]
    turns scene 1 by two different angles and ends with dt = 0.0 exactly; every other angle gives an Rm whose off-diagonal
    entries are one positive and one negative."""
    out = {}
    for k, name in enumerate(sorted(SC.PICKS)):
        out[name] = np.random.default_rng(900 + k).uniform(0.0, 2.0 * np.pi, len(SC.PICKS[name]))
    out["repeat"][3] = 0.0
    assert out["repeat"][1] != out["repeat"][2]
    return out


ROT_DT = _angles()
