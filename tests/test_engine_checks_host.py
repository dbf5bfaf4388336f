"""CPU: HotPathEngine.host_checks -- the one host-side loop behind a forward (pair-capacity regrow, range guard, Att.strict's
empty-pair error) -- driven with stub forwards: plain callables that return CPU int32 words and note the matrix mode they
were called in.  No kernel runs; the engine is a bare HotPathEngine(None, ...), whose constructor only stores its arguments."""
import re

import pytest
import torch


def words(flag, counts):
    """A forward's output as far as host_checks reads it."""
    i32 = lambda v: torch.tensor([v], dtype=torch.int32)
    return {"nonfinite": i32(flag), "n_pairs": [i32(c) for c in counts]}


OK, BIG = (5000, 6000, 7000), (9000, 6000, 7000)
NEG = tuple(-c for c in BIG)
ZERO = (5000, 0, 7000)
REGROW = "pair capacity still exceeded"
RANGE = "fp16's range"
CAT = r"torch\.cat\(\): expected a non-empty list"

# name: (mode, guard, pair_caps, strict, first output, outputs of the reruns in order,
#        expected: index of the returned output (0 = first, k = k-th rerun) or (exception, match), modes the reruns saw,
#        _pair_seen afterwards (it starts at [1, 1, 1] and keeps the largest magnitude per set), calls of on_regrow)
CASES = {
    "clean":                    ("f16x2", "reroute", "tight", False, (0, OK), [], 0, [], list(OK), 0),
    "overflow_once":            ("f16x2", "reroute", "tight", False, (0, NEG), [(0, BIG)], 1, ["f16x2"], list(BIG), 1),
    "overflow_once_bf16":       ("bf16", "reroute", "tight", False, (0, NEG), [(0, BIG)], 1, ["bf16"], list(BIG), 1),
    "overflow_twice":           ("f16x2", "reroute", "tight", False, (0, NEG), [(0, NEG)], ("lgcn", REGROW), ["f16x2"], list(BIG), 1),
    "one_set_over":             ("f16x2", "reroute", "tight", False, (0, (5000, -6000, 7000)), [(0, OK)], 1, ["f16x2"], [5000, 6000, 7000], 1),
    "bound_records_nothing":    ("f16x2", "reroute", "bound", False, (0, NEG), [], 0, [], [1, 1, 1], 0),
    "flag_reroute":             ("f16x2", "reroute", "tight", False, (1, OK), [(1, OK)], 1, ["bf16x3"], list(OK), 0),
    "flag_raise":               ("f16x2", "raise", "tight", False, (1, OK), [], ("lgcn", RANGE), [], list(OK), 0),
    "flag_off":                 ("f16x2", "off", "tight", False, (1, OK), [], 0, [], list(OK), 0),
    "flag_other_bits":          ("f16x2", "reroute", "tight", False, (4, OK), [(0, OK)], 1, ["bf16x3"], list(OK), 0),
    "flag_in_bf16x3":           ("bf16x3", "raise", "tight", False, (1, OK), [], 0, [], list(OK), 0),
    "flag_in_bf16":             ("bf16", "reroute", "tight", False, (1, OK), [], 0, [], list(OK), 0),
    "flag_in_f32":              ("f32", "reroute", "tight", False, (1, OK), [], 0, [], list(OK), 0),
    "overflow_and_flag":        ("f16x2", "reroute", "tight", False, (1, NEG), [(1, BIG), (0, BIG)], 2, ["f16x2", "bf16x3"], list(BIG), 1),
    "overflow_and_flag_raise":  ("f16x2", "raise", "tight", False, (1, NEG), [(1, BIG)], ("lgcn", RANGE), ["f16x2"], list(BIG), 1),
    "flag_gone_after_regrow":   ("f16x2", "reroute", "tight", False, (1, NEG), [(0, BIG)], 1, ["f16x2"], list(BIG), 1),
    "strict_zero":              ("f16x2", "reroute", "tight", True, (0, ZERO), [], ("runtime", CAT), [], [5000, 1, 7000], 0),
    "strict_zero_bound":        ("f16x2", "reroute", "bound", True, (0, ZERO), [], ("runtime", CAT), [], [1, 1, 1], 0),
    "strict_zero_after_reroute": ("f16x2", "reroute", "tight", True, (1, OK), [(0, ZERO)], ("runtime", CAT), ["bf16x3"], list(OK), 0),
    "strict_zero_before_reroute_only": ("f16x2", "reroute", "tight", True, (1, ZERO), [(0, OK)], 1, ["bf16x3"], [5000, 1, 7000], 0),
    "strict_zero_after_regrow": ("f16x2", "reroute", "tight", True, (0, NEG), [(0, (9000, 0, 7000))], ("runtime", CAT), ["f16x2"], list(BIG), 1),
    "strict_nonzero":           ("f16x2", "reroute", "tight", True, (0, OK), [], 0, [], list(OK), 0),
    "strict_off_zero":          ("f16x2", "reroute", "tight", False, (0, ZERO), [], 0, [], [5000, 1, 7000], 0),
}


def run_case(mode, guard, caps, strict, first, reruns):
    """-> (engine, first output, rerun outputs, modes seen, regrow calls, result or exception, mode / guard afterwards)"""
    import lanegcn_amd  # noqa: F401
    from lanegcn_amd import ops
    from lanegcn_amd.engine import HotPathEngine
    eng = HotPathEngine(None, None, None, None, None)
    eng.pair_caps, eng._pair_seen = caps, [1, 1, 1]
    outs = [words(*r) for r in reruns]
    seen, regrown = [], []

    def rerun():
        seen.append(ops.get_mma())
        assert len(seen) <= len(outs), "more reruns than the case allows"
        return outs[len(seen) - 1]

    out0 = words(*first)
    prev = ops.get_mma(), ops.get_guard()
    try:
        ops.set_mma(mode)
        ops.set_guard(guard)
        try:
            got = eng.host_checks(out0, rerun, strict=strict, on_regrow=lambda: regrown.append(1))
        except Exception as e:      # noqa: BLE001 -- the table says which one it has to be
            got = e
        after = ops.get_mma(), ops.get_guard()
    finally:
        ops.set_mma(prev[0])
        ops.set_guard(prev[1])
    return eng, out0, outs, seen, len(regrown), got, after


@pytest.mark.parametrize("name", sorted(CASES))
def test_host_checks_table(name):
    from lanegcn_amd._lib import LgcnError
    mode, guard, caps, strict, first, reruns, want, want_modes, want_seen, want_regrow = CASES[name]
    eng, out0, outs, seen, regrown, got, after = run_case(mode, guard, caps, strict, first, reruns)
    assert after == (mode, guard), "matrix mode / guard policy not restored"
    assert seen == want_modes
    assert regrown == want_regrow
    assert eng._pair_seen == want_seen
    if isinstance(want, tuple):
        kind, match = want
        assert type(got) is {"lgcn": LgcnError, "runtime": RuntimeError}[kind], repr(got)      # LgcnError is a RuntimeError
        assert re.search(match, str(got)), str(got)
    else:
        assert got is ([out0] + outs)[want], repr(got)


def test_an_output_without_flag_and_counts_is_returned_untouched():
    """The map-only forward returns {"nodes", "actors"}: nothing to check, whatever the mode and the policy."""
    import lanegcn_amd  # noqa: F401
    from lanegcn_amd.engine import HotPathEngine
    for drop in ("nonfinite", "n_pairs", None):
        out = {"nodes": torch.zeros(2, 128), "actors": torch.zeros(1, 128)}
        if drop is not None:
            out.update({k: v for k, v in words(1, NEG).items() if k != drop})
        else:
            drop = "both"
        keys = sorted(out)
        eng = HotPathEngine(None, None, None, None, None)
        eng.pair_caps, eng._pair_seen = "tight", [1, 1, 1]
        got = eng.host_checks(out, lambda: pytest.fail("rerun called"), strict=True, on_regrow=lambda: pytest.fail("regrow called"))
        assert got is out and sorted(got) == keys and eng._pair_seen == [1, 1, 1], drop


def test_on_regrow_is_optional_and_learn_pair_counts_keeps_its_meaning():
    import lanegcn_amd  # noqa: F401
    from lanegcn_amd.engine import HotPathEngine
    eng = HotPathEngine(None, None, None, None, None)
    eng.pair_caps, eng._pair_seen = "tight", [1, 1, 1]
    second = words(0, BIG)
    assert eng.host_checks(words(0, NEG), lambda: second) is second and eng._pair_seen == list(BIG)
    assert eng.learn_pair_counts(words(0, (-9500, 10, 10))) and eng._pair_seen == [9500, 6000, 7000]
    assert not eng.learn_pair_counts(words(0, OK)) and eng._pair_seen == [9500, 6000, 7000]
    assert [eng._cap(i) for i in range(3)] == [12288, 8192, 9216]      # 1.25 x, + 1, up to the next 1,024
