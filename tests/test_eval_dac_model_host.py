"""CPU: evaluate.DrivableArea.inside against the loop-level model of tests/eval_dac_model.py; the fixture tells every wrong
variant of the rule from the right one; mask, counts and DAC_k; the validation of scene_city."""
import numpy as np
import pytest

import eval_dac_model as DM


def drivable():
    import lanegcn_amd  # noqa: F401
    from lanegcn_amd.evaluate import DrivableArea
    return DrivableArea(DM.fixture_areas())


def test_the_fixture_points_are_what_the_definition_says():
    areas = DM.fixture_areas()
    for c, pt, want in DM.POINTS:
        assert DM.inside(pt[0], pt[1], *areas[c]) is want, (c, pt)
    for c, pt in DM.SAFE.items():
        assert DM.inside(pt[0], pt[1], *areas[c])
    # round half to even in fp32, as the definition spells it out
    assert [float(np.round(np.float32(v))) for v in (2.5, 3.5, -0.5)] == [2.0, 4.0, -0.0]
    assert np.signbit(np.round(np.float32(-0.5)))
    for mat, _ in areas.values():
        assert mat.shape[0] != mat.shape[1] and (mat[0] == 1).any() and (mat[:, 0] == 1).any() and (mat[1:, 1:] != 1).any()


def test_inside_equals_the_model_on_the_fixture_and_on_random_points():
    da, areas = drivable(), DM.fixture_areas()
    assert da.cities == ["P", "Q"]
    for c, pt, want in DM.POINTS:
        assert bool(da.inside(np.array(pt, np.float32), c)) is want, (c, pt)
    rng = np.random.default_rng(5)
    for i, c in enumerate(da.cities):
        pts = rng.uniform(-4, 15, (10000, 2)).astype(np.float32)
        pts[:2000] = np.round(pts[:2000] * 2) / 2                          # many exact .5 ties and integers
        pts[2000:2010] = [[np.nan, 1], [1, np.nan], [np.inf, 1], [1, -np.inf], [3e38, 3e38], [-3e38, 1], [1e30, 1], [-0.0, 0.0],
                          [2 ** 31, 1], [1, -2.0 ** 63]]
        got = da.inside(pts, c)
        want = np.array([DM.inside(x, y, *areas[c]) for x, y in pts])
        assert got.shape == (10000,) and got.dtype == bool and np.array_equal(got, want), c
        assert 100 < got.sum() < 9900                                     # both answers occur often
        assert np.array_equal(da.inside(pts, i), got)                     # by id
        assert np.array_equal(da.inside(pts.reshape(100, 100, 2), c), got.reshape(100, 100))
    assert not da.inside(np.ones((3, 2), np.float32), None).any() and not da.inside(np.ones((3, 2), np.float32), -1).any()


@pytest.mark.parametrize("variant", DM.VARIANTS)
def test_the_fixture_tells_every_wrong_variant_apart(variant):
    f = DM.fixture(6, 12, 7)
    flag = np.ones(len(f["reg"]), np.float32)
    right = DM.masks(f["reg"], flag, f["city"], 7, f["areas"])[0]
    wrong = DM.masks(f["reg"], flag, f["city"], 7, f["areas"], **{variant: True})[0]
    differ = np.nonzero(right != wrong)[0]
    print(variant, "changes records", differ.tolist())
    assert len(differ) >= 1


@pytest.mark.parametrize("M", [1, 6, 8])
def test_mask_counts_and_dac(M):
    T, H = 12, 7
    f = DM.fixture(M, T, H)
    A = len(f["reg"])
    flag = np.ones(A, np.float32)
    flag[3], flag[5] = 0.0, 2.0                                           # not evaluated / non-finite: no DAC
    mask, has = DM.masks(f["reg"], flag, f["city"], H, f["areas"])
    da = drivable()
    full = (1 << M) - 1
    for a in range(A):
        j, t = f["edit"][a]
        if flag[a] != 1.0 or f["city"][a] < 0:
            assert mask[a] == 0.0 and has[a] == 0.0
            continue
        assert has[a] == 1.0
        # the production lookup, step by step: the same mask
        bits = sum(1 << m for m in range(M) if da.inside(f["reg"][a, m, :H], int(f["city"][a])).all())
        assert bits == int(mask[a]), a
        want = f["want_inside"][a]
        if want is not None:                                              # one edited point at a counted step of mode j
            assert int(mask[a]) == (full if want else full & ~(1 << j)), a
        else:                                                             # edited behind the horizon only
            assert t >= H and int(mask[a]) == full
    c, n = DM.counts(mask, has, M)
    assert n == A - 3 and len(c) == M                                     # flag 0, flag 2 and the scene without a map
    for k in range(1, M + 1):
        per_record = [bin(int(m) & ((1 << k) - 1)).count("1") / k for m, h in zip(mask, has) if h == 1.0]
        assert abs(DM.dac(mask, has, M)[0][k] - float(np.mean(per_record))) <= 1e-15
    keep = np.arange(A) % 2 == 0
    assert DM.counts(mask, has, M, keep)[1] == int(((has == 1.0) & keep).sum())
    assert np.isnan(DM.dac(mask, np.zeros(A), M)[0][1]) and DM.dac(mask, np.zeros(A), M)[1] == 0


def test_scene_city_is_validated_at_construction():
    import lanegcn_amd  # noqa: F401
    from lanegcn_amd._lib import LgcnError
    from lanegcn_amd.evaluate import ActorEvaluator, DrivableArea, Evaluator
    da = drivable()
    ev = Evaluator(5, 6, 30, device="cpu", drivable=da, scene_city=["P", "Q", None, -1, 1])
    assert ev.scene_city.tolist() == [0, 1, -1, -1, 1] and ev.scene_city.dtype == np.int32
    assert Evaluator(3, 6, 30, device="cpu", drivable=da, scene_city=np.array([0, 1, -1], np.int32)).scene_city.tolist() == [0, 1, -1]
    off = np.array([0, 2, 2, 5], np.int64)
    av = ActorEvaluator(off, 6, 30, device="cpu", drivable=da, scene_city=["Q", "Q", "P"])
    assert av.scene_city.tolist() == [1, 1, 0] and av.n_slots == 5
    for bad in (["P", "Q"], ["P", "Q", "P", "P"], ["P", "Q", "MIA"], [0, 1, 2], [0, 1, -2], [0, 1, 0.5], None):
        with pytest.raises(LgcnError):
            Evaluator(3, 6, 30, device="cpu", drivable=da, scene_city=bad)
        with pytest.raises(LgcnError):
            ActorEvaluator(off, 6, 30, device="cpu", drivable=da, scene_city=bad)
    with pytest.raises(LgcnError):
        Evaluator(3, 6, 30, device="cpu", scene_city=[0, 1, 0])           # cities without a map to look them up in
    for areas in ({}, {"P": (np.ones((3,)), np.eye(3))}, {"P": (np.ones((0, 4)), np.eye(3))}, {"P": (np.ones((3, 4)), np.eye(2))},
                  {"P": (np.ones((3, 4)), np.full((3, 3), np.nan))}):
        with pytest.raises(LgcnError):
            DrivableArea(areas)
    # without a DrivableArea the evaluator is what it was: the status buffer, the keys
    plain = Evaluator(3, 6, 30, device="cpu")
    assert plain._status.numel() == 448 and plain.drivable is None and plain.scene_city is None and plain._dac is None
    assert ev._status.numel() == 528 and ev._dac.shape == (9,) and ev._dac.data_ptr() == ev._status.data_ptr() + 448


def test_from_files_and_reduction_to_equals_one(tmp_path):
    import lanegcn_amd  # noqa: F401
    from lanegcn_amd.evaluate import DrivableArea
    areas = DM.fixture_areas()
    paths = {}
    for c, (mat, se2) in areas.items():
        paths[c] = (str(tmp_path / (c + "_mat.npy")), str(tmp_path / (c + "_se2.npy")))
        np.save(paths[c][0], mat.astype(np.float32) if c == "P" else mat.astype(bool))
        np.save(paths[c][1], se2)
    da, ref = DrivableArea.from_files(paths), drivable()
    assert da.cities == ref.cities and np.array_equal(da.raster, ref.raster) and da.raster.dtype == np.uint8
    assert set(np.unique(da.raster)) == {0, 1} and da.raster.size == 7 * 9 + 5 * 4
    assert bytes(da.table) == bytes(ref.table)
    assert (da.table[1].off, da.table[1].h, da.table[1].w, list(da.table[1].m)) == (63, 5, 4, [0., -1., 2.5, 1., 0., 0.5])
