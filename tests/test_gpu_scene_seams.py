"""GPU: scene construction (csrc/lgcn_scene.hip) at the seams of its block scans (tests/seam_cases.py; proven on the host by
tests/test_seam_cases_host.py): lgcn_scene_tracks (sc_scan_local<1>, T + 1 items) and lgcn_scene_lanes_rank / _fill
(sc_scan_local<4>, n_cand + 1 items, four interleaved scans of stride 4) at one block, one block and a lone item, 256
blocks, and past block 256, where block_base takes its second trip.  Driven through data_raw.build_scenes, compared bit for
bit with the host model (tests/scene_build_model.py, in the vectorised form the host test holds to it).

If the totals in front of block 256 were dropped, every track (candidate lane) from item 65 536 on would be written over
the batch's first rows: the last scenes' feats / nodes and their per-scene counts differ; with the stride of the four lane
scans wrong, num_nodes or the pre / suc pair lists of every scene behind the first block differ."""
import numpy as np
import pytest

import lanegcn_amd  # noqa: F401
import scene_build_compare as K
import seam_cases as S

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("T", S.TRACK_COUNTS)
def test_scene_tracks_at_the_block_seams(T):
    from lanegcn_amd import data_raw as D
    raws = S.track_batch(T)
    want, counts = S.obj_feats_batch(raws)
    got = D.build_scenes(raws, {"A": S.small_table()}, S.SCENE_CONFIG, device=False, cross=False)
    assert [len(s["feats"]) for s in got] == counts.tolist()
    off = S.csum(counts)
    for b, s in enumerate(got):
        K.assert_same_bits({k: s[k] for k in want}, {k: v[off[b]:off[b + 1]] for k, v in want.items()}, "T %d scene %d" % (T, b))


@pytest.fixture(scope="module")
def table():
    return S.lane_table()


@pytest.mark.parametrize("n_cand", S.LANE_COUNTS)
def test_scene_lanes_at_the_block_seams(n_cand, table):
    from lanegcn_amd import data_raw as D
    raws, ids = S.lane_batch(n_cand, table)
    rows = S.lane_cand_rows(table, ids)
    orig, rot = S.frames(raws)
    got = D.build_scenes(raws, {"A": table}, S.SCENE_CONFIG, device=False, cross=False, lane_ids=ids)
    assert len(got) == len(raws)
    for b, s in enumerate(got):
        want = S.lane_graph_one(orig[b], rot[b], table, S.PRED_RANGE, rows[b])
        del want["kept_rows"]
        K.assert_same_bits(s["graph"], want, "n_cand %d scene %d" % (n_cand, b))
        assert s["feats"].shape == (1, 20, 3) and np.array_equal(s["orig"], orig[b]) and np.array_equal(s["rot"], rot[b])
