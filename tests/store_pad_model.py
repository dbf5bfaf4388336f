"""Host model of a PADDED batch of the scene store, shared by the padded-store tests: the filler
scene as a scene dict, and the padded batch as FlatSceneFile.batch over a store that holds the scenes plus that filler."""
import os

import numpy as np


def pick_totals(scenes, pick):
    """(N, A, [E_r]) of the pick: nodes, actors and edges per relation (pre0, suc0, ..., left, right)."""
    from lanegcn_amd.flatfile import _relations
    n = sum(int(scenes[i]["graph"]["num_nodes"]) for i in pick)
    a = sum(len(scenes[i]["ctrs"]) for i in pick)
    R = 2 * len(scenes[0]["graph"]["pre"]) + 2
    e = [sum(len(np.asarray(_relations(scenes[i]["graph"])[r]["u"]).reshape(-1)) for i in pick) for r in range(R)]
    return n, a, e


def filler_scene(caps, totals, num_scales, gt=True):
    """The filler scene of a pick with `totals` = (N, A, [E_r]) under `caps`: n_f = caps.nodes - N nodes at (1e6, 1e6)
    with zero features, a_f = caps.actors - A actors at (-1e6 - 256 i, -1e6) with zero tracks, identity rot, zero orig,
    zero gt_preds, no has_preds; caps.edges[r] - E_r self-loops u = v = k mod n_f per relation."""
    N, A, E = totals
    n_f, a_f = caps.nodes - N, caps.actors - A
    assert n_f >= 1 and a_f >= 1 and all(c >= e for c, e in zip(caps.edges, E))
    loops = [np.arange(c - e, dtype=np.int64) % n_f for c, e in zip(caps.edges, E)]
    rel = [{"u": k.copy(), "v": k.copy()} for k in loops]
    graph = {"num_nodes": n_f, "ctrs": np.full((n_f, 2), 1e6, np.float32), "feats": np.zeros((n_f, 2), np.float32),
             "turn": np.zeros((n_f, 2), np.float32), "control": np.zeros(n_f, np.float32),
             "intersect": np.zeros(n_f, np.float32), "pre": rel[0:2 * num_scales:2], "suc": rel[1:2 * num_scales:2],
             "left": rel[2 * num_scales], "right": rel[2 * num_scales + 1]}
    ctrs = np.stack([(-1e6 - 256.0 * np.arange(a_f)).astype(np.float32), np.full(a_f, -1e6, np.float32)], 1)
    scene = {"graph": graph, "ctrs": ctrs, "feats": np.zeros((a_f, 20, 3), np.float32), "rot": np.eye(2, dtype=np.float32),
             "orig": np.zeros(2, np.float32)}
    if gt:
        scene["gt_preds"], scene["has_preds"] = np.zeros((a_f, 30, 2), np.float32), np.zeros((a_f, 30), bool)
    return scene


def padded_batch_host(scenes, pick, caps, tmp_dir, device="cpu"):
    """(FlatBatch, extras) = FlatSceneFile.batch(pick + [F]) over write_scenes(scenes + [filler]); tensors on `device`."""
    from lanegcn_amd.flatfile import FlatSceneFile, write_scenes
    ns = len(scenes[0]["graph"]["pre"])
    fill = filler_scene(caps, pick_totals(scenes, pick), ns, gt="gt_preds" in scenes[0])
    path = os.path.join(str(tmp_dir), "padded_%d.npz" % abs(hash((tuple(pick), caps))))
    write_scenes(path, list(scenes) + [fill])
    return FlatSceneFile(path).batch(list(pick) + [len(scenes)], device=device)
