"""GPU: the range guard's detector (k_check_finite<ROWS> in csrc/lgcn_bwd.hip behind lgcn_check_finite and
lgcn_check_finite_rows) with ONE value planted at a chosen place (cases and model: tests/glue_cases.py, pinned by
test_glue_cases_host.py).  Every tensor lies inside an arena of NaN, 64 floats in front of it and behind it, so a read
outside a tensor raises the flag of a run that must stay clear.  Per launch the flag word is preset to 0x50 and has
its own address; the bit walks through 1, 2 and 1 << 30; a run over a finite background must leave the word as it was
and a non-finite value anywhere must give exactly 0x50 | bit.

Places: every float of every (na, nb) in 0..9 x 0..9; around one and two workgroups with the tensors joined at an odd
size; and at the grid cap of 2048 workgroups (8 388 608 floats: four trips; 10 485 767: five whole trips, one float4 of
a sixth and a leftover of 3) the first floats, the last float4, every leftover float and both sides of every trip
boundary of both tensors.  Values: three NaN encodings and both infinities must flag; +-FLT_MAX, the smallest
denormal and -0.0 must not.  The ROWS form: every row from the clamped device count on is NaN and the word stays clear,
then an inf in the last column of the last looked-at row sets it -- for counts below, at and beyond both clamps."""
import numpy as np
import pytest
import torch

import glue_cases as G

pytestmark = pytest.mark.gpu
PAD = 64
VALUES = list(G.BAD.items()) + list(G.GOOD.items())


@pytest.fixture(scope="module")
def dev():
    import lanegcn_amd  # noqa: F401
    from lanegcn_amd import _lib as L
    from lanegcn_amd import ops
    return L.load(), L, ops


def signed(bits):
    return bits - (1 << 32) if bits >= 1 << 31 else bits


class Placed:
    """A host array on the device, NaN in front of it and behind it; 16-byte aligned."""

    def __init__(self, x):
        self.host = np.ascontiguousarray(x, np.float32)
        self.n = self.host.size
        self.arena = torch.full((PAD + self.n + PAD,), float("nan"), dtype=torch.float32, device="cuda")
        self.t = self.arena[PAD:PAD + self.n].view(self.host.shape)
        self.t.copy_(torch.from_numpy(self.host))
        self.i32 = self.arena.view(torch.int32)
        self.bits = self.host.reshape(-1).view(np.uint32)
        assert self.t.data_ptr() % 16 == 0

    def ptr(self):
        return self.t.data_ptr() if self.n else None

    def plant(self, i, bits):
        self.i32[PAD + i] = signed(int(bits))

    def restore(self, i):
        self.i32[PAD + i] = signed(int(self.bits[i]))

    def unchanged(self):
        return np.array_equal(self.arena.cpu().numpy().view(np.uint32)[PAD:PAD + self.n], self.bits)


def new_words(n):
    return torch.full((n,), G.WORD, dtype=torch.int32, device="cuda")


def launch(dev, ta, tb, words, k, bit):
    lib, L, ops = dev
    L.check(lib.lgcn_check_finite(ta.ptr(), ta.n, tb.ptr(), tb.n, words.data_ptr() + 4 * k, bit, ops._stream()), "lgcn_check_finite")


def sweep(dev, a, b, positions):
    """One clean launch, then one launch per (position, value) with that value planted alone."""
    assert not G.finite_flag(a, b)
    ta, tb = Placed(a), Placed(b)
    cases = [(w, i, name, bits) for w, i, _ in positions for name, bits in VALUES]
    words = new_words(len(cases) + 1)
    want = np.full(len(cases) + 1, G.WORD, np.int32)
    launch(dev, ta, tb, words, 0, G.BITS[0])
    for k, (w, i, name, bits) in enumerate(cases, 1):
        t = ta if w == "a" else tb
        t.plant(i, bits)
        launch(dev, ta, tb, words, k, G.BITS[k % 3])
        t.restore(i)
        if G.finite_flag(np.array([G.as_f32(bits)])):
            want[k] |= G.BITS[k % 3]
    got = words.cpu().numpy()
    bad = [(("clean",) if k == 0 else cases[k - 1], hex(got[k]), hex(want[k])) for k in np.flatnonzero(got != want)]
    assert not bad, (len(a), len(b), len(bad), bad[:12])
    assert ta.unchanged() and tb.unchanged()
    return len(cases) + 1


@pytest.mark.parametrize("na", G.TINY)
def test_every_float_of_the_tiny_sizes(dev, na):
    for nb in G.TINY:
        sweep(dev, G.background(na, 10 + na), G.background(nb, 30 + nb), G.cf_positions(na, nb, every=True))


def test_nothing_to_look_at_leaves_the_word(dev):
    lib, L, ops = dev
    words = new_words(2)
    assert lib.lgcn_check_finite(None, 0, None, 0, words.data_ptr(), 1, ops._stream()) == 0
    assert lib.lgcn_check_finite_rows(None, 0, 1, None, None, 0, 1, None, words.data_ptr() + 4, 2, ops._stream()) == 0
    assert words.tolist() == [G.WORD, G.WORD]


@pytest.mark.parametrize("total", G.SEAM_TOTALS)
@pytest.mark.parametrize("how", ["a", "b", "ab"])
def test_one_to_two_workgroups(dev, total, how):
    na, nb = G.cf_split(total, how)
    sweep(dev, G.background(na, total), G.background(nb, total + 1), G.cf_positions(na, nb))


@pytest.mark.parametrize("total", G.CAP_TOTALS)
def test_the_grid_cap(dev, total):
    na, nb = G.CAP_NA, total - G.CAP_NA
    n = sweep(dev, G.background(na, 7), G.background(nb, 8), G.cf_positions(na, nb))
    print("%d floats: %d launches, %d trips of %d float4" % (total, n, G.cf_trips(na, nb), G.cf_stride(total)))


@pytest.mark.parametrize("bit", G.BITS)
@pytest.mark.parametrize("na,nb", [(9, 6), (1027, 3077)])
def test_the_word(dev, bit, na, nb):
    """0x50 | bit exactly, whichever tensor holds the value, in its float4 part or its leftover, and with one in both."""
    ta, tb = Placed(G.background(na, 1)), Placed(G.background(nb, 2))
    plans = [[], [("a", 0)], [("a", na - 1)], [("b", 0)], [("b", nb - 1)], [("a", 5), ("b", nb - 1)], [("a", na - 1), ("b", 1)]]
    words = new_words(len(plans))
    for k, plan in enumerate(plans):
        for j, (w, i) in enumerate(plan):
            (ta if w == "a" else tb).plant(i, list(G.BAD.values())[(k + j) % 5])
        launch(dev, ta, tb, words, k, bit)
        for w, i in plan:
            (ta if w == "a" else tb).restore(i)
    assert words.tolist() == [G.WORD] + [G.WORD | bit] * (len(plans) - 1)
    # a second find ORs the same bit in again: no change; another bit joins it
    ta.plant(2, G.BAD["+inf"])
    launch(dev, ta, tb, words, 1, bit)
    launch(dev, ta, tb, words, 2, 4)
    assert words.tolist()[:3] == [G.WORD, G.WORD | bit, G.WORD | bit | 4]


def test_ops_check_finite_without_rows(dev):
    lib, L, ops = dev
    ta, tb = Placed(G.background(11 * 360, 3).reshape(11, 360)), Placed(G.background(11 * 6, 4).reshape(11, 6))
    flag = new_words(1)
    ops.check_finite(flag, ta.t, tb.t, bit=2)
    ops.check_finite(flag, ta.t)
    assert flag.item() == G.WORD
    tb.plant(65, G.BAD["quiet NaN"])                       # the last float of cls: one of its two leftover floats
    ops.check_finite(flag, ta.t, tb.t, bit=2)
    assert flag.item() == G.WORD | 2
    ops.check_finite(flag, tb.t)
    assert flag.item() == G.WORD | 3


# ------------------------------------------------------------------ the ROWS form
def rows_launch(dev, route, ta, tb, ra, rb, words, k, bit):
    """route "ops": ops.check_finite(rows=...); "direct": the C entry."""
    lib, L, ops = dev
    flag = words[k:k + 1]
    if route == "ops":
        ops.check_finite(flag, ta.t, None if tb is None else tb.t, bit=bit, rows=(ra, rb))
        return
    row = lambda t: t.host.shape[1]
    L.check(lib.lgcn_check_finite_rows(ta.ptr(), ta.n, row(ta), ra.data_ptr(), None if tb is None else tb.ptr(), 0 if tb is None else tb.n,
                                       1 if tb is None else row(tb), None if tb is None else rb.data_ptr(), flag.data_ptr(), bit,
                                       ops._stream()), "lgcn_check_finite_rows")


def count(r):
    return torch.tensor([r], dtype=torch.int64, device="cuda")


@pytest.mark.parametrize("route", ["ops", "direct"])
@pytest.mark.parametrize("shapes", G.ROW_SHAPES, ids=lambda s: "a%dx%d-b%dx%d" % (s[0] + s[1]))
def test_rows_clamp(dev, route, shapes):
    bg = [G.background(s[0] * s[1], 5 + k).reshape(s) for k, s in enumerate(shapes)]
    got, want, what = [], [], []
    words = new_words(2 * 2 * 7)
    k = 0
    for which in (0, 1):
        cap = shapes[which][0]
        other = count(shapes[1 - which][0])                 # the other tensor: all of its rows, all finite
        for r in G.row_counts(cap):
            m = G.clamp_rows(r, cap)
            x = bg[which].copy()
            x[m:] = np.nan                                  # every row that must not be looked at
            host = [bg[0], bg[1]]
            host[which] = x
            placed = [Placed(h) for h in host]
            rr = [other, other]
            rr[which] = count(r)
            rows_of = lambda: dict(rows_a=int(rr[0].item()), row_a=shapes[0][1], rows_b=int(rr[1].item()), row_b=shapes[1][1])
            rows_launch(dev, route, placed[0], placed[1], rr[0], rr[1], words, k, 2)
            want.append(G.WORD | 2 if G.finite_flag(host[0], host[1], **rows_of()) else G.WORD)
            what.append((which, r, "rows beyond are NaN"))
            assert want[-1] == G.WORD
            k += 1
            if m >= 1:
                x[m - 1, -1] = np.inf
                placed[which].plant(m * shapes[which][1] - 1, G.BAD["+inf"])
            rows_launch(dev, route, placed[0], placed[1], rr[0], rr[1], words, k, 1)
            want.append(G.WORD | 1 if G.finite_flag(host[0], host[1], **rows_of()) else G.WORD)
            what.append((which, r, "inf in the last looked-at row"))
            assert (want[-1] != G.WORD) == (m >= 1)
            k += 1
    got = words.tolist()
    bad = [(w, hex(g), hex(e)) for w, g, e in zip(what, got, want) if g != e]
    assert not bad, bad


@pytest.mark.parametrize("route", ["ops", "direct"])
def test_rows_are_independent_and_optional(dev, route):
    sa, sb = (11, 360), (11, 6)
    a, b = G.background(sa[0] * sa[1], 1).reshape(sa), G.background(sb[0] * sb[1], 2).reshape(sb)
    nan_a, nan_b = np.full(sa, np.nan, np.float32), np.full(sb, np.nan, np.float32)
    words = new_words(8)
    # a whole, b not looked at and all NaN; and the other way round
    rows_launch(dev, route, Placed(a), Placed(nan_b), count(sa[0]), count(0), words, 0, 1)
    rows_launch(dev, route, Placed(nan_a), Placed(b), count(0), count(sb[0]), words, 1, 1)
    # each count belongs to its own tensor: 3 rows of a, 7 of b
    x, y = a.copy(), b.copy()
    x[3:], y[7:] = np.nan, np.nan
    rows_launch(dev, route, Placed(x), Placed(y), count(3), count(7), words, 2, 1)
    rows_launch(dev, route, Placed(x), Placed(y), count(7), count(3), words, 3, 1)           # swapped: a's NaN rows are looked at
    rows_launch(dev, route, Placed(x), Placed(y), count(3), count(8), words, 4, 2)           # b's first NaN row
    # one count for both tensors, as the engine passes fb.real_rows[1] for reg and cls
    both = count(3)
    y[3:] = np.nan
    rows_launch(dev, route, Placed(x), Placed(y), both, both, words, 5, 2)
    # b absent
    rows_launch(dev, route, Placed(x), None, count(3), count(0), words, 6, 1)
    rows_launch(dev, route, Placed(x), None, count(4), count(0), words, 7, 1)
    assert words.tolist() == [G.WORD, G.WORD, G.WORD, G.WORD | 1, G.WORD | 2, G.WORD, G.WORD, G.WORD | 1]
    assert not G.finite_flag(x, y, 3, 360, 3, 6) and G.finite_flag(x, y, 7, 360, 3, 6) and G.finite_flag(x, None, 4, 360)


@pytest.mark.parametrize("route", ["ops", "direct"])
def test_rows_from_a_slice_of_a_table(dev, route):
    """The counts as FlatBatch.real_rows holds them: one-element slices of a larger int64 table whose other entries say
    'every row'."""
    sa, sb = (37, 128), (11, 6)
    x, y = G.background(sa[0] * sa[1], 1).reshape(sa), G.background(sb[0] * sb[1], 2).reshape(sb)
    x[20:], y[5:] = np.nan, np.nan
    table = torch.full((9,), 2 ** 40, dtype=torch.int64, device="cuda")
    table[3], table[7] = 20, 5
    words = new_words(2)
    rows_launch(dev, route, Placed(x), Placed(y), table[3:4], table[7:8], words, 0, 1)
    table[7] = 6
    rows_launch(dev, route, Placed(x), Placed(y), table[3:4], table[7:8], words, 1, 1)
    assert words.tolist() == [G.WORD, G.WORD | 1]
