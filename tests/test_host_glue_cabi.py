"""CPU: lgcn_check_finite, lgcn_check_finite_rows, lgcn_gather_sum, lgcn_pair_add, lgcn_gather_rows and lgcn_widen_i32 are
exported, bound and declared in the header, and refuse a negative count, a null required pointer, a misaligned pointer, a zero
bit and a row length that does not divide its tensor before anything is launched (no GPU needed); an empty call returns
LGCN_OK without looking at its pointers."""
import os
import re

import pytest

OK, EINVAL, EALIGN = 0, -1, -3
ENTRIES = ("lgcn_check_finite", "lgcn_check_finite_rows", "lgcn_gather_sum", "lgcn_pair_add", "lgcn_gather_rows", "lgcn_widen_i32")
HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "lgcn.h")
P = 0x7f0000100000                     # a 16-byte aligned address nothing dereferences: every check comes before the launch


@pytest.fixture(scope="module")
def lib():
    import lanegcn_amd  # noqa: F401
    from lanegcn_amd import _lib
    return _lib.load(), _lib


def test_entries_are_exported_bound_and_declared(lib):
    l, mod = lib
    text = open(HEADER).read()
    for n in ENTRIES:
        assert hasattr(l, n), "liblgcn.so does not export " + n
        assert n in mod.SIGNATURES
        assert re.search(r"\bint %s\(" % n, text), "include/lgcn.h does not declare " + n


def test_check_finite_validates_before_launching(lib):
    l, _ = lib

    def call(a=P, na=64, b=P + 4096, nb=24, flag=P + 8192, bit=1):
        return l.lgcn_check_finite(a, na, b, nb, flag, bit, None)

    assert call(na=-1) == EINVAL and call(nb=-1) == EINVAL and call(na=0, nb=-1) == EINVAL
    assert call(bit=0) == EINVAL and call(na=0, nb=0, bit=0) == EINVAL
    assert call(a=None, na=0, b=None, nb=0, flag=None) == OK                        # nothing to look at: no launch, no pointer read
    assert call(flag=None) == EINVAL and call(a=None) == EINVAL and call(b=None) == EINVAL
    assert call(a=P + 4) == EALIGN and call(b=P + 4100) == EALIGN and call(a=P + 8) == EALIGN
    # a tensor of no elements is not looked at: its pointer may be null or anything else
    assert call(a=None, na=0, b=P + 4, nb=8) == EALIGN and call(a=P + 4, na=8, b=None, nb=0) == EALIGN


def test_check_finite_rows_validates_before_launching(lib):
    l, _ = lib

    def call(a=P, na=64, row_a=16, rows_a=P + 16384, b=P + 4096, nb=24, row_b=6, rows_b=P + 16392, flag=P + 8192, bit=2):
        return l.lgcn_check_finite_rows(a, na, row_a, rows_a, b, nb, row_b, rows_b, flag, bit, None)

    assert call(na=-16) == EINVAL and call(nb=-6) == EINVAL and call(bit=0) == EINVAL
    assert call(a=None, na=0, rows_a=None, b=None, nb=0, rows_b=None, flag=None, row_a=0, row_b=0) == OK
    for name in ("a", "rows_a", "b", "rows_b", "flag"):
        assert call(**{name: None}) == EINVAL, name
    assert call(row_a=0) == EINVAL and call(row_a=-16) == EINVAL and call(row_a=3) == EINVAL and call(row_a=128) == EINVAL
    assert call(row_b=0) == EINVAL and call(row_b=-6) == EINVAL and call(row_b=5) == EINVAL and call(row_b=48) == EINVAL
    assert call(a=P + 4) == EALIGN and call(b=P + 4100) == EALIGN
    assert call(rows_a=P + 16388) == EALIGN and call(rows_b=P + 16396) == EALIGN     # int64 counts: 8-byte aligned
    # an empty tensor's row length, count pointer and address are not looked at
    assert call(a=None, na=0, row_a=0, rows_a=None, b=P + 4) == EALIGN
    assert call(b=None, nb=0, row_b=-1, rows_b=P + 4, a=P + 4) == EALIGN


def test_gather_sum_validates_before_launching(lib):
    l, _ = lib

    def call(src=P, rowptr=P + 4096, col=P + 8192, n_rows=9, out=P + 16384):
        return l.lgcn_gather_sum(src, rowptr, col, n_rows, out, None)

    assert call(n_rows=-1) == EINVAL
    assert call(src=None, rowptr=None, col=None, n_rows=0, out=None) == OK
    for name in ("src", "rowptr", "out"):
        assert call(**{name: None}) == EINVAL, name
    assert call(src=P + 4) == EALIGN and call(out=P + 16388) == EALIGN
    # the int32 tables need no 16-byte alignment, and col == NULL is the contiguous form: past every check, so not called here
    assert call(src=P + 4, rowptr=P + 4100, col=None) == EALIGN


def test_pair_add_validates_before_launching(lib):
    l, _ = lib
    names = ("c", "U", "hi", "V", "wi", "n_dev", "out")

    def call(cap=9, **kw):
        a = {n: P + 4096 * k for k, n in enumerate(names)}
        a.update(kw)
        return l.lgcn_pair_add(a["c"], a["U"], a["hi"], a["V"], a["wi"], a["n_dev"], cap, a["out"], None)

    assert call(cap=-1) == EINVAL
    assert call(cap=0, **{n: None for n in names}) == OK
    for n in names:
        assert call(**{n: None}) == EINVAL, n
    for k, n in enumerate(names):
        if n in ("c", "U", "V", "out"):
            assert call(**{n: P + 4096 * k + 4}) == EALIGN, n


def test_gather_rows_validates_before_launching(lib):
    l, _ = lib
    names = ("src", "idx", "n_dev", "out")

    def call(cap=9, **kw):
        a = {n: P + 4096 * k for k, n in enumerate(names)}
        a.update(kw)
        return l.lgcn_gather_rows(a["src"], a["idx"], a["n_dev"], cap, a["out"], None)

    assert call(cap=-1) == EINVAL
    assert call(cap=0, **{n: None for n in names}) == OK
    for n in names:
        assert call(**{n: None}) == EINVAL, n
    assert call(src=P + 4) == EALIGN and call(out=P + 3 * 4096 + 4) == EALIGN


def test_widen_validates_before_launching(lib):
    l, _ = lib
    assert l.lgcn_widen_i32(P, P + 4096, -1, P + 8192, None) == EINVAL
    assert l.lgcn_widen_i32(None, None, 0, None, None) == OK
    assert l.lgcn_widen_i32(None, P + 4096, 9, P + 8192, None) == EINVAL
    assert l.lgcn_widen_i32(P, None, 9, P + 8192, None) == EINVAL
    assert l.lgcn_widen_i32(P, P + 4096, 9, None, None) == EINVAL
