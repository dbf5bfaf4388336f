"""Cases and plain numpy models for the small kernels every other test uses but none tests: the range guard's detector
(lgcn_check_finite / lgcn_check_finite_rows), lgcn_gather_sum, lgcn_pair_add, lgcn_gather_rows (csrc/lgcn_bwd.hip) and
lgcn_widen_i32 (csrc/lgcn_index.hip).  test_glue_cases_host.py pins the models to loops and the launch constants below
to the source text; test_gpu_finite_guard.py and test_gpu_gather_glue.py run the kernels on the cases.

The detector: blocks = clamp(((na + nb) / 4 + 1023) / 1024, 1, 2048) workgroups of 256 threads walk the float4s of a,
then of b, as ONE index space joined at na / 4, with a stride of blocks * 256 float4; the <= 3 floats either tensor
has beyond its whole float4s are read by the first threads of workgroup 0.  The row kernels: 8 rows of 128 floats per
workgroup, at most 4096 workgroups, so row 32768 is the first of a second trip."""
import numpy as np

C = 128                                                    # floats of a feature row (32 float4, one per lane of a half wave)
CF_THREADS, CF_F4_PER_BLOCK, CF_MAX_BLOCKS = 256, 1024, 2048
ROWS_PER_BLOCK, ROW_MAX_BLOCKS = 8, 4096
ROW_SPAN = ROWS_PER_BLOCK * ROW_MAX_BLOCKS                 # 32768 rows per trip of the capped grid
WIDEN_THREADS, WIDEN_MAX_BLOCKS = 256, 1024
WIDEN_SPAN = WIDEN_THREADS * WIDEN_MAX_BLOCKS              # 262144 elements per trip
LOSS_MAX_BLOCKS = 4096                                     # k_pred_loss_bwd / k_roi_loss_bwd: one agent per workgroup and trip

# ------------------------------------------------------------------ the detector
BAD = {"quiet NaN": 0x7fc00000, "payload NaN": 0x7f800001, "negative NaN": 0xffc00000, "+inf": 0x7f800000, "-inf": 0xff800000}
GOOD = {"+FLT_MAX": 0x7f7fffff, "-FLT_MAX": 0xff7fffff, "denormal": 0x00000001, "-0.0": 0x80000000}
WORD, BITS = 0x50, (1, 2, 1 << 30)
TINY = range(10)
SEAM_TOTALS = (4096, 4099, 4100, 4103, 4104)               # one workgroup holds 1024 float4 = 4096 floats
CAP_TOTALS = (8388608, 10485767)                           # exactly 2048 workgroups; beyond the cap with a leftover of 3
CAP_NA = 5000003
ROW_SHAPES = (((37, 128), (11, 6)), ((11, 360), (11, 6)), ((13, 1), (7, 1)), ((13, 2), (7, 2)), ((13, 3), (7, 3)), ((13, 5), (7, 5)))


def as_f32(bits):
    return np.array([bits], np.uint32).view(np.float32)[0]


def cf_blocks(total):
    return min(max((total // 4 + CF_F4_PER_BLOCK - 1) // CF_F4_PER_BLOCK, 1), CF_MAX_BLOCKS)


def cf_stride(total):
    """float4s between two trips of one thread."""
    return cf_blocks(total) * CF_THREADS


def cf_trips(na, nb):
    """Trips of the float4 loop that thread 0 makes (the other threads make this many or one fewer)."""
    return -(-(na // 4 + nb // 4) // cf_stride(na + nb))


def clamp_rows(r, cap_rows):
    """include/lgcn.h: the device count, clamped to [0, cap_rows]."""
    return 0 if r <= 0 else (cap_rows if r >= cap_rows else int(r))


def finite_flag(a, b=None, rows_a=None, row_a=1, rows_b=None, row_b=1):
    """True when the looked-at part of a or of b holds a NaN or an infinity.  rows_*: only the first clamp(rows_*) rows of
    row_* floats are looked at (None: all of it)."""
    bad = False
    for x, r, w in ((a, rows_a, row_a), (b, rows_b, row_b)):
        if x is None or np.size(x) == 0:
            continue
        x = np.asarray(x, np.float32).reshape(-1)
        assert w > 0 and x.size % w == 0
        n = x.size if r is None else clamp_rows(r, x.size // w) * w
        bad = bad or not bool(np.isfinite(x[:n]).all())
    return bad


def background(n, seed):
    """n finite floats over 40 binades with +-FLT_MAX, denormals and -0.0 sprinkled in and, from 4 floats on, one aligned
    float4 of four FLT_MAX (a detector that adds the values up instead of their differences overflows on it)."""
    rng = np.random.default_rng(seed)
    x = (rng.standard_normal(n) * 2.0 ** rng.integers(-20, 21, n)).astype(np.float32)
    bits = x.view(np.uint32)
    good = np.array(list(GOOD.values()), np.uint32)
    at = np.arange(seed % 5, n, 5)
    bits[at] = good[(at // 5 + seed) % len(good)]
    if n >= 4:
        q = 4 * ((n // 4) // 2)
        bits[q:q + 4] = GOOD["+FLT_MAX"]
    return x


def cf_split(total, how):
    """(na, nb) of a seam total: all in a, all in b, or a odd-sized so that b's float4s follow a's last whole float4."""
    return {"a": (total, 0), "b": (0, total), "ab": (1027, total - 1027)}[how]


def cf_positions(na, nb, every=False):
    """[(tensor, float index, tag)]: per tensor the floats 0, 1, 3, 4, the last float of the float4 part, every leftover
    float, and for every trip k >= 1 of the grid one float of the float4s k * stride - 1 (last thread of trip k - 1) and
    k * stride (first thread of trip k) of the joined index space.  every: all floats of both tensors (the tiny sizes)."""
    na4, nb4, stride = na // 4, nb // 4, cf_stride(na + nb)
    out, seen = [], set()

    def add(which, i, tag):
        if (which, i) not in seen:
            seen.add((which, i))
            out.append((which, i, tag))

    for which, n, n4, base in (("a", na, na4, 0), ("b", nb, nb4, na4)):
        for i in (0, 1, 3, 4):
            if i < n:
                add(which, i, "head" if i < 4 * n4 else "leftover")
        if n4:
            add(which, 4 * n4 - 1, "body_last")
        for i in range(n if every else 0):
            add(which, i, "head" if i < 4 * n4 else "leftover")
        for i in range(4 * n4, n):
            add(which, i, "leftover")
        for k in range(1, cf_trips(na, nb) + 1):
            for f4, tag in ((k * stride - 1, "trip_last"), (k * stride, "trip_first")):
                if f4 < na4 + nb4 and 0 <= f4 - base < n4:
                    add(which, 4 * (f4 - base) + (k + f4) % 4, tag)
    return out


def f4_thread(which, i, na, nb):
    """(global thread, trip) of the float4 loop that reads float i of a tensor; None for a leftover float."""
    n4 = (na if which == "a" else nb) // 4
    if i >= 4 * n4:
        return None
    f4 = i // 4 + (0 if which == "a" else na // 4)
    return f4 % cf_stride(na + nb), f4 // cf_stride(na + nb)


def row_counts(cap_rows):
    """The device row counts of the ROWS form around both clamps."""
    return (-3, 0, 1, cap_rows - 1, cap_rows, cap_rows + 1, 2 ** 40)


# ------------------------------------------------------------------ the row kernels
SUM_ROWS = (1, 7, 8, 9, ROW_SPAN - 1, ROW_SPAN, ROW_SPAN + 1, 2 * ROW_SPAN + 1)
PAIR_CAPS = (1, 7, 8, 9, ROW_SPAN - 1, ROW_SPAN, ROW_SPAN + 1)
WIDEN_CAPS = (1, 255, 256, 257, WIDEN_SPAN - 1, WIDEN_SPAN, WIDEN_SPAN + 1)
LONG_ROW, SRC_ROWS, GUARD_ROWS = 1000, 1000, 8
SMALL_LENS = tuple(range(10)) + (LONG_ROW,)                 # every tail length of the 4-way walk in eleven rows
SENTINEL = 0x7fc00abc                                      # a NaN no kernel produces: rows that must be left alone hold it
SENTINEL64 = 0x5a5a5a5a5a5a5a5a
U = 2.0 ** -24


def row_blocks(rows):
    return min((rows + ROWS_PER_BLOCK - 1) // ROWS_PER_BLOCK, ROW_MAX_BLOCKS)


def row_trips(rows):
    return -(-rows // (row_blocks(rows) * ROWS_PER_BLOCK)) if rows else 0


def widen_trips(cap):
    blocks = min(max((cap + WIDEN_THREADS - 1) // WIDEN_THREADS, 1), WIDEN_MAX_BLOCKS)
    return -(-cap // (blocks * WIDEN_THREADS))


def dev_count(n, cap):
    """The kernels' rule for a device count: anything outside [0, cap] means cap."""
    return cap if (n < 0 or n > cap) else int(n)


def device_counts(cap):
    return sorted({0, 1, cap - 1, cap, cap + 1, -1, -cap})


def sum_row_lengths(n_rows, sparse):
    """Lengths cycling through 0..9 (sparse: every 32nd row, the others 0 or 1 long, so that a col-less src stays small),
    one row of LONG_ROW a third of the way in, and fixed non-zero lengths on both sides of the trip boundary and at the end."""
    i = np.arange(n_rows)
    lens = np.where(i % 32 == 0, ((i // 32) * 7 + 3) % 10, i & 1) if sparse else (i * 7 + 3) % 10
    if n_rows >= 7:
        lens[n_rows // 3] = LONG_ROW
    for r, k in ((n_rows - 1, 5), (ROW_SPAN - 1, 7), (ROW_SPAN, 6)):
        if 0 <= r < n_rows and lens[r] != LONG_ROW:
            lens[r] = k
    return lens.astype(np.int64)


def features(rng, rows):
    """[rows, 128] fp32 over 16 binades, both signs: sums whose low bits depend on the order of the additions."""
    return (rng.standard_normal((rows, C)) * 2.0 ** rng.integers(-8, 9, (rows, C))).astype(np.float32)


def gather_sum_case(n_rows, with_col, lens=None):
    """src, rowptr, col (None: contiguous segments) of one lgcn_gather_sum call."""
    rng = np.random.default_rng(1000 + n_rows + int(with_col))
    lens = sum_row_lengths(n_rows, sparse=not with_col and n_rows > 1024) if lens is None else np.asarray(lens, np.int64)
    rowptr = np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)
    nnz = int(rowptr[-1])
    if not with_col:
        return dict(src=features(rng, max(nnz, 1)), rowptr=rowptr, col=None)
    col = rng.integers(0, SRC_ROWS, nnz)
    if nnz >= 4:
        col[0], col[1], col[2], col[-1] = 0, SRC_ROWS - 1, 0, SRC_ROWS - 1       # row 0, the last row, a repeat in one segment
    return dict(src=features(rng, SRC_ROWS), rowptr=rowptr, col=col.astype(np.int32))


def gather_sum_seq(src, rowptr, col=None, dtype=np.float32):
    """out[n] = (((0 + x_0) + x_1) + ...) over the entries of row n in their order, every addition rounded to dtype;
    x_k = src[col[j]], or src[j] where col is None.  Step k adds the k-th entry of every row that has one."""
    src, rowptr = np.asarray(src, dtype), np.asarray(rowptr, np.int64)
    deg = np.diff(rowptr)
    out = np.zeros((len(deg), src.shape[1]), dtype)
    order = np.argsort(-deg, kind="stable")
    n_live = np.searchsorted(-deg[order], -np.arange(1, int(deg.max(initial=0)) + 1), side="right")     # rows longer than k
    for k in range(int(deg.max(initial=0))):
        rows = order[:n_live[k]]
        j = rowptr[rows] + k
        out[rows] = out[rows] + src[j if col is None else np.asarray(col, np.int64)[j]]
    return out


def gather_sum_f64(src, rowptr, col=None):
    """(the sums, the sums of the magnitudes) in float64."""
    return gather_sum_seq(src, rowptr, col, np.float64), gather_sum_seq(np.abs(np.asarray(src, np.float64)), rowptr, col, np.float64)


def gamma(n):
    """Higham's gamma_n = n u / (1 - n u): n fp32 additions in any order are within gamma_n sum|x| of the exact sum."""
    return n * U / (1 - n * U)


def sentinel_rows(rows):
    return np.full((rows, C), SENTINEL, np.uint32).view(np.float32)


def index_case(cap, n_src, seed):
    """cap row indices into n_src rows: repeats, row 0 and the last row, both at the ends and in the middle."""
    rng = np.random.default_rng(seed)
    idx = rng.integers(0, n_src, cap)
    idx[cap // 2] = (n_src - 1) * (cap & 1)
    idx[0] = 0
    idx[-1] = n_src - 1
    return idx.astype(np.int32)


def pair_case(cap):
    rng = np.random.default_rng(2000 + cap)
    return dict(c=features(rng, cap), U=features(rng, 37), hi=index_case(cap, 37, cap), V=features(rng, 23), wi=index_case(cap, 23, cap + 1))


def pair_add(c, U, hi, V, wi, n, cap, out):
    """out[p] = (c[p] + U[hi[p]]) + V[wi[p]] for p < dev_count(n, cap), in fp32 and in that order; the other rows of out
    (a copy) are as they were."""
    out, m = np.array(out, np.float32), dev_count(n, cap)
    out[:m] = (np.asarray(c, np.float32)[:m] + np.asarray(U, np.float32)[hi[:m]]) + np.asarray(V, np.float32)[wi[:m]]
    return out


def gather_rows(src, idx, n, cap, out):
    out, m = np.array(out, np.float32), dev_count(n, cap)
    out[:m] = np.asarray(src, np.float32)[idx[:m]]
    return out


def widen_case(cap):
    rng = np.random.default_rng(3000 + cap)
    x = rng.integers(-2 ** 31, 2 ** 31, cap).astype(np.int32)
    x[cap // 2] = 2 ** 31 - 1
    x[0] = -1
    x[-1] = -2 ** 31
    return x


def widen(x, n, cap, out):
    out, m = np.array(out, np.int64), dev_count(n, cap)
    out[:m] = np.asarray(x, np.int32)[:m]                  # sign-extended
    return out
