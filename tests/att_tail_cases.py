"""The Att tail roles over operand scale: the one problem every check of them shares, its float64 restatement in every
matrix mode (split_model), and the elementwise accumulation bound of the flags-0 roles.

Test infrastructure for tests/test_att_tail_model_host.py and tests/test_gpu_att_tail_scale.py.

The problem is what Att.pairs_tail hands its tail launch: T target rows a, P pair rows m in segments per target, and
    out = ReLU(GN2(ReLU(GN1(a W_agt^T + S W_c1^T)) W_2^T) + res),   S[t] = sum of the pair rows of target t (fp32)
    U   = ReLU(GN_q(out W_q^T)) W_u^T       V = out W_v^T           (the chained outputs, from the fp32-held out)
Everything comes from test_gpu_operand_scale.draw() and one more seeded draw.  s_x = 2^ex scales a and m, s_w = 2^ew
every 128-wide weight.  The residual rows are a separate O(1) draw that is NOT scaled: with res = a at 2^60 GN2's
output vanishes under the residual's ulp and a GroupNorm that returned beta would pass (model error 5e-20).

Pairs per target cycle through COUNTS and one target gets 40 (T >= 49): 0 .. 2 pairs end at lgcn_node_tail's two up-front
loads, 3 reach its scalar tail only, 6 take one four-load step, 9 and 40 a four-load step plus a remainder.  In f16x2
at s_x = 2^12 the 40-pair sum leaves fp16's range (1e5 > 65504: the guard's case, test_f16x2_upper_edge), so that
target is left out at that one scale; with at most 9 pairs the largest sum stays under 65504."""
import functools

import numpy as np
import torch

import split_model as S
from test_gpu_operand_scale import F16_GRID, WIDE_GRID, draw, p2

C = 128
ROWS = (1, 49, 130)
COUNTS = (0, 1, 2, 3, 6, 0, 1, 9)
BIG = 40
CASES = [("f16x2", ex, ew) for ex, ew in F16_GRID] + [(m, ex, ew) for m in ("bf16x3", "f32", "bf16") for ex, ew in WIDE_GRID]
IDS = ["%s-x2^%d-w2^%d" % c for c in CASES]
TENSORS = ("out", "U", "V")


def counts(T, big=True):
    c = np.array([COUNTS[i % len(COUNTS)] for i in range(T)], np.int64)
    if big and T >= 49:
        c[T // 2] = BIG
    return c


@functools.lru_cache(maxsize=None)
def tail_draw():
    """CPU fp32, unscaled.  The pair rows are post-ReLU N(0, 1), as the pair stage leaves them."""
    d = draw()
    g = torch.Generator().manual_seed(20261)
    rn = lambda *s: torch.randn(*s, generator=g)
    n = max(ROWS)
    return dict(a=d["x"], w_agt=d["w"][0], w_c1=d["w"][1], w2=d["w2"], wq=d["w"][2], wu=d["w"][3],
                wv=d["w384"][:, 2 * C:].contiguous(), gn1=d["gn1"], gn2=d["gn2"], gq=(1 + 0.1 * rn(C), 0.1 * rn(C)),
                m=rn(int(counts(n).sum()), C).relu(), res=rn(n, C))


WEIGHTS = ("w_agt", "w_c1", "w2", "wq", "wu", "wv")


@functools.lru_cache(maxsize=None)
def problem(mode, ex, ew, T):
    """The scaled problem: CPU fp32 tensors, hi [P] int64, rowptr [T + 1] int32, pieces (the rows of a RANGE16 source
    that hold data)."""
    d = tail_draw()
    cnt = counts(T, big=not (mode == "f16x2" and ex >= 12))
    rowptr = np.zeros(T + 1, np.int64)
    rowptr[1:] = np.cumsum(cnt)
    P = int(rowptr[-1])
    c = dict(T=T, P=P, hi=np.repeat(np.arange(T), cnt), rowptr=torch.from_numpy(rowptr).to(torch.int32),
             a=p2(d["a"][:T], ex).contiguous(), m=p2(d["m"][:max(P, 1)], ex).contiguous(), res=d["res"][:T].contiguous(),
             gn1=d["gn1"], gn2=d["gn2"], gq=d["gq"])
    c.update({k: p2(d[k], ew) for k in WEIGHTS})
    # RANGE16: of a segment [b, e) the rows b and the multiples of 16 inside (b, e) hold the fp32 sums, in pair order, of
    # the rows up to the next such row; every other row is never read (NaN here)
    m16 = torch.full_like(c["m"], float("nan"))
    starts = []
    for t in range(T):
        b, e = int(rowptr[t]), int(rowptr[t + 1])
        cut = [b] + [r for r in range(16 * (b // 16 + 1), e, 16)] + [e] if b < e else []
        for s, nxt in zip(cut[:-1], cut[1:]):
            acc = c["m"][s].clone()
            for r in range(s + 1, nxt):
                acc += c["m"][r]
            m16[s] = acc
            starts.append(s)
    if P == 0:
        m16[:] = c["m"]
    c["m16"], c["pieces"] = m16, np.asarray(starts, np.int64)
    return c


def seg(c, model, rel16=False):
    """The segment sums as the row block holds them (fp32) / in float64.  rel16: from the fp32 piece sums."""
    if rel16 and model:
        return S.seg_sum(S.arr(c["m16"])[c["pieces"]], c["hi"][c["pieces"]], c["T"], True)
    return S.seg_sum(c["m"][:c["P"]], c["hi"], c["T"], model)


def tail_values(c, mode, model=True, rel16=False, drop_kstep=None, gn2_is_beta=False):
    """dict(out, U, V) of the tail with both chained outputs.  drop_kstep = (weight name, s): that weight with the 32
    columns of K-step s zeroed; gn2_is_beta: GN2 returns beta -- the broken variants the bar has to reject."""
    w = {k: S.arr(c[k], np.float32) for k in WEIGHTS}
    if drop_kstep is not None:
        name, s = drop_kstep
        w[name] = w[name].copy()
        w[name][:, 32 * s:32 * s + 32] = 0
    gn2 = (np.zeros(C, np.float32), S.arr(c["gn2"][1])) if gn2_is_beta else c["gn2"]
    T = c["T"]
    out = S.row_block(T, [(c["a"], w["w_agt"], None), (seg(c, model, rel16), w["w_c1"], None)], mode, gn1=c["gn1"], relu1=True,
                      w2=w["w2"], gn2=gn2, res=c["res"], relu2=True, model=model)["out"]
    held = S._hold(out, model)
    U = S.row_block(T, [(held, w["wq"], None)], mode, gn1=c["gq"], relu1=True, w2=w["wu"], model=model)["out"]
    return dict(out=out, U=U, V=S._mm(held, w["wv"], mode, model))


@functools.lru_cache(maxsize=None)
def tail(mode, ex, ew, T, model=True, rel16=False):
    """tail_values of a case, computed once and shared (treat as read-only)."""
    return tail_values(problem(mode, ex, ew, T), mode, model, rel16)


def head_rows(c):
    """Context rows for the head pair: pair rows, as many as another entry of ROWS."""
    n = {1: 49, 49: 130, 130: 1}[c["T"]]
    return tail_draw()["m"][:n]


# ------------------------------------------------------------------ flags 0: kernel against its own model, elementwise
def abs_products(a, w, mode):
    """sum over the mode's plane products of |A_p| |B_q|^T."""
    pa, pb = S.planes(a, mode), S.planes(w, mode)
    return sum(np.abs(pa[i]) @ np.abs(pb[j]).T for i, j in zip(*S.FORMATS[mode][2:]))


def accumulation_bound(operands, mode):
    """What an fp32 accumulation of the exact plane products may differ by from their float64 sum:
    2 K NPROD 2^-24 sum |A_p| |B_q|^T, K = 128 -- the textbook bound, times 2 for an accumulator that truncates.
    operands: (A rows as the kernel splits them, weight) per relation."""
    n_prod = len(S.FORMATS[mode][2])
    return 2.0 * C * n_prod * 2.0 ** -24 * sum(abs_products(a, w, mode) for a, w in operands)
