"""Independent numpy model of the training rotation of a preprocessed scene (reference data.py:45-63), on scene dicts, one
scene at a time.  Shares no code with lanegcn_amd.flatfile.

theta' = theta + dt; rot' and Rm (the rotation by -dt) are float64 cos / sin rounded to float32, as the reference forms
them.  Where the reference multiplies by Rm with np.matmul (evaluation order left to BLAS), the project fixes the
arithmetic: out = x * Rm[0, c] + y * Rm[1, c] in float32 arrays -- two rounded products, one rounded add."""
import numpy as np


def matrices(theta, dt):
    """-> (theta', rot' float32 [2,2], Rm float32 [2,2])."""
    theta, dt = float(theta), float(dt)
    new = theta + dt
    rot = np.asarray([[np.cos(new), -np.sin(new)], [np.sin(new), np.cos(new)]], np.float32)
    rm = np.asarray([[np.cos(-dt), -np.sin(-dt)], [np.sin(-dt), np.cos(-dt)]], np.float32)
    return new, rot, rm


def turn(xy, rm):
    xy = np.asarray(xy, np.float32)
    out = np.empty_like(xy)
    for c in range(2):
        out[..., c] = xy[..., 0] * rm[0, c] + xy[..., 1] * rm[1, c]
    return out


def bound(xy, rm):
    """The derived bound on |model - reference| per rotated coordinate (float64): 4.5 u (|x Rm0c| + |y Rm1c|) for two
    correctly rounded evaluations of the two-term dot product, fused or not, u = 2^-24, plus 2^-23 (|x| + |y|) for one ulp
    in an entry of Rm."""
    xy, rm = np.asarray(xy, np.float64), np.asarray(rm, np.float64)
    x, y = np.abs(xy[..., 0]), np.abs(xy[..., 1])
    out = np.empty_like(xy)
    for c in range(2):
        out[..., c] = 4.5 * 2.0 ** -24 * (x * abs(rm[0, c]) + y * abs(rm[1, c])) + 2.0 ** -23 * (x + y)
    return out


def rotate_scene(scene, dt):
    """The scene as the augmentation leaves it: a new dict (and graph dict); untouched values are the scene's own."""
    new, rot, rm = matrices(scene["theta"], dt)
    out = dict(scene)
    out["theta"], out["rot"] = new, rot
    feats = np.array(scene["feats"], np.float32)
    feats[:, :, :2] = turn(feats[:, :, :2], rm)
    out["feats"] = feats
    out["ctrs"] = turn(scene["ctrs"], rm)
    graph = dict(scene["graph"])
    graph["ctrs"], graph["feats"] = turn(scene["graph"]["ctrs"], rm), turn(scene["graph"]["feats"], rm)
    out["graph"] = graph
    return out


def rotate_pick(scenes, pick, dts):
    return [rotate_scene(scenes[i], dt) for i, dt in zip(pick, dts)]
