"""Fixture and picks shared by the scene-store tests (test_gpu_scene_store.py, test_store_plan_host.py)."""
import numpy as np

FLAT_ARRAYS = ("node_ctrs", "node_feats", "turn", "control", "intersect", "actor_ctrs", "node_off", "actor_off",
               "idx_local", "seg_off", "seg_base")
FLAT_FIELDS = ("n_scenes", "n_nodes", "n_actors", "num_scales", "rel_slices", "n_edges", "cap_a2m", "cap_a2a")
NO_ACTORS, NO_LEFT_RIGHT = 2, 4          # scene 2 has no actor, scene 4 neither left nor right edges

# out of order with a repeat; the zero-actor scene alone; all six; 70 indices (B + 1 > 64 and 2 * 14 * 70 = 1,960 segments:
# past one wave and past a 1,024-entry table); only the scene without left / right edges (two relations empty in the batch)
PICKS = {
    "repeat": [3, 1, 1, 0],
    "no_actors": [NO_ACTORS],
    "all": [0, 1, 2, 3, 4, 5],
    "seventy": [int(i) for i in np.random.default_rng(70).integers(0, 6, 70)],
    "no_left_right": [NO_LEFT_RIGHT, NO_LEFT_RIGHT],
}


def make_scenes(gt=True):
    """Six synth_scene scenes of 72 / 144 / 90 nodes (no run a multiple of 64) with 3..11 actors, one with none, one
    without left / right edges; every scene gets its own rot / orig and a has_preds pattern, so that a row taken from the
    wrong scene or actor shows."""
    from lanegcn_amd import data as gen
    rng = np.random.default_rng(21)
    scenes = [gen.synth_scene(rng, roads, a) for roads, a in
              (([4], 3), ([4, 4], 11), ([5], 0), ([4, 4], 7), ([5], 5), ([4], 9))]
    for k in ("left", "right"):
        scenes[NO_LEFT_RIGHT]["graph"][k] = {"u": np.zeros(0, np.int64), "v": np.zeros(0, np.int64)}
    for s in scenes:
        th = rng.uniform(0, 2 * np.pi)
        s["rot"] = np.array([[np.cos(th), -np.sin(th)], [np.sin(th), np.cos(th)]], np.float32)
        s["orig"] = rng.uniform(-500, 500, 2).astype(np.float32)
        s["has_preds"] = rng.random(s["has_preds"].shape) < 0.7
        if not gt:
            del s["gt_preds"], s["has_preds"]
    return scenes
