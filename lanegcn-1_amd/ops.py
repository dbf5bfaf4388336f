"""Tensor-level wrappers over the C ABI (include/lgcn.h).

Every function takes CUDA (ROCm) tensors, enqueues on the current torch stream and returns
without synchronising.  CPU tensors are rejected: the product path has no CPU fallback.
"""
import ctypes as C
from dataclasses import dataclass
from typing import List, Optional, Sequence, Tuple

import torch

from . import _lib as L

import os

C_FEAT = 128
EPS = 1e-5

# How the 128-d contractions run on the matrix cores (include/lgcn.h, LGCN_MMA_*):
#   "f32"    exact fp32 fma chain (v_mfma_f32_32x32x2_f32)
#   "bf16x3" 3-way bf16 split, 6 products, fp32 accumulate: fp32-grade over fp32's exponent range, 2.67x the f32 MFMA rate
#   "f16x2"  2-way fp16 split, 3 products, fp32 accumulate, 5.3x the f32 rate: fp32-grade inside a window -- operands
#            below 65520 (the first value that rounds to fp16's infinity), and within 1e-4 while a block's max |W| >= 2^-9
#            (2e-3) and max |x| >= 2^-10 with the other operand O(1); below it the fp16 planes run out of bits (1e-3 at
#            max |W| = 2^-13, 1e-2 at 2^-17: DESIGN.md "Operand scale"; tools/check_weight_scale.py lists such blocks)
#   "bf16"   single bf16 product (BASELINE config "bf16"; not within 1e-4: 8 significand bits, 1e-3 .. 1e-2 against float64
#            at any operand scale -- fp32's exponent range, like bf16x3)
_mma = L.MMA_NAMES[os.environ.get("LGCN_MMA", "f16x2")]


def set_mma(name: str):
    """Select the matrix-core mode for subsequent launches ("f32" | "bf16x3" | "f16x2" | "bf16")."""
    global _mma
    _mma = L.MMA_NAMES[name]


def get_mma() -> str:
    return {v: k for k, v in L.MMA_NAMES.items()}[_mma]


class backward_mma:
    """Matrix-core mode for the row-GEMMs of a backward pass: gradients routinely sit below fp16's normal
    range (6e-5), where the 2-way fp16 split loses its second plane, so f16x2 forwards run their backward
    GEMMs on the range-safe 3-way bf16 split (same fp32-grade accuracy, fp32 exponent range)."""

    def __enter__(self):
        global _mma
        self.prev = _mma
        if _mma == L.MMA_F16X2:
            _mma = L.MMA_BF16X3
        return self

    def __exit__(self, *a):
        global _mma
        _mma = self.prev


class mma_scope:
    """``with ops.mma_scope("bf16x3"):`` -- matrix-core mode for the launches inside the block."""

    def __init__(self, name: str):
        self.name = name

    def __enter__(self):
        global _mma
        self.prev = _mma
        _mma = L.MMA_NAMES[self.name]
        return self

    def __exit__(self, *a):
        global _mma
        _mma = self.prev


def exact_mma() -> mma_scope:
    """``with ops.exact_mma():`` -- exact fp32 (LGCN_MMA_F32) for the launches and the weight images inside the block,
    whatever set_mma() says: the training pair stage of Att (att_pairs_train / att_pairs_bwd) runs in it like
    ActorNet.exact's conv units.  The images are cached per mode and registered like every other one, so
    refresh_packed() rebuilds them too."""
    return mma_scope("f32")


# What happens when a forward in the range-restricted default mode (f16x2: operands below 65520) comes back with
# non-finite features: "reroute" (default) runs it again in bf16x3 (fp32's exponent range, same fp32-grade
# accuracy), "raise" raises LgcnError, "off" returns it as it is.
_guard = os.environ.get("LGCN_GUARD", "reroute")


def set_guard(policy: str):
    global _guard
    if policy not in ("reroute", "raise", "off"):
        raise L.LgcnError("guard policy must be 'reroute', 'raise' or 'off'")
    _guard = policy


def get_guard() -> str:
    return _guard


def check_finite(flag: torch.Tensor, a: torch.Tensor, b: Optional[torch.Tensor] = None, bit: int = 1, rows=None):
    """flag[0] |= bit when a (or b) holds a NaN / inf (lgcn_check_finite); enqueued, no synchronisation.
    rows: (rows_a, rows_b), one-element int64 device tensors -- only the first rows_a[0] rows of a (dimension 0) and
    rows_b[0] of b are looked at, the counts read on the device (lgcn_check_finite_rows: the real rows of a padded batch,
    engine.FlatBatch.real_rows)."""
    lib = L.load()
    a = _dev(a, torch.float32, "a")
    b = None if b is None else _dev(b, torch.float32, "b")
    if rows is not None:
        ra, rb = (_dev(r, torch.int64, "rows") for r in rows)
        row = lambda t: t.numel() // t.shape[0] if t.numel() else 1
        L.check(lib.lgcn_check_finite_rows(_ptr(a), a.numel(), row(a), _ptr(ra), _ptr(b), 0 if b is None else b.numel(),
                                           1 if b is None else row(b), _ptr(rb), _ptr(flag), bit, _stream()),
                "lgcn_check_finite_rows")
        return
    L.check(lib.lgcn_check_finite(_ptr(a), a.numel(), _ptr(b), 0 if b is None else b.numel(), _ptr(flag), bit, _stream()),
            "lgcn_check_finite")


def guarded(run, tensors_of=lambda out: (out,)):
    """run() in the current matrix mode; in f16x2 the result's features are checked on the device (one 4-byte
    device->host read) and a forward that overflowed fp16's range is run again in bf16x3 -- or raises, by policy.
    Non-finite values that survive the re-run were in the inputs: returned as they are, like the reference does."""
    out = run()
    if _guard == "off" or _mma != L.MMA_F16X2:
        return out
    ts = [t for t in tensors_of(out) if t is not None and t.numel() > 0]
    if not ts:
        return out
    flag = torch.zeros(1, dtype=torch.int32, device=ts[0].device)
    for i in range(0, len(ts), 2):
        check_finite(flag, ts[i], ts[i + 1] if i + 1 < len(ts) else None)
    if int(flag.item()) == 0:
        return out
    if _guard == "raise":
        raise L.LgcnError("non-finite features in f16x2 mode: an operand left fp16's range (|x| >= 65520); "
                          "use ops.set_mma('bf16x3') or ops.set_guard('reroute')")
    with mma_scope("bf16x3"):
        return run()


def _stream():
    # the raw hipStream_t of torch's current stream (torch.cuda.current_stream() costs ~9 us of Python per call)
    return C.c_void_p(torch._C._cuda_getCurrentRawStream(torch._C._cuda_getDevice()))


def module_params(module) -> tuple:
    """tuple(module.parameters()), cached on the module (walking the module tree costs more than a launch)."""
    ps = module.__dict__.get("_lgcn_params")
    if ps is None:
        ps = tuple(module.parameters())
        module.__dict__["_lgcn_params"] = ps
    return ps


def _dev(t: torch.Tensor, dtype=None, name="tensor"):
    if not t.is_cuda:
        raise L.LgcnError("%s must be a CUDA tensor (the HIP hot path has no CPU fallback)" % name)
    if dtype is not None and t.dtype != dtype:
        raise L.LgcnError("%s must be %s, got %s" % (name, dtype, t.dtype))
    return t if t.is_contiguous() else t.contiguous()


def _ptr(t: Optional[torch.Tensor]):
    return C.c_void_p(0 if t is None else t.data_ptr())


def wants_grad(*tensors) -> bool:
    """True when autograd must record this call (then the differentiable path of autograd.py runs)."""
    return torch.is_grad_enabled() and any(t is not None and t.requires_grad for t in tensors)


# ------------------------------------------------------------------ integer path
def graph_gather_indices(flat_in: torch.Tensor, seg_off: torch.Tensor, seg_base: torch.Tensor, want32=False):
    """out[e] = in[e] + base[seg(e)] (lanegcn.py:191-208).  Returns (out64, out32|None)."""
    lib = L.load()
    flat_in = _dev(flat_in, torch.int64, "flat_in")
    seg_off = _dev(seg_off, torch.int64, "seg_off")
    seg_base = _dev(seg_base, torch.int64, "seg_base")
    n = flat_in.numel()
    out64 = torch.empty_like(flat_in)
    out32 = torch.empty(n, dtype=torch.int32, device=flat_in.device) if want32 else None
    L.check(lib.lgcn_graph_gather(_ptr(flat_in), n, _ptr(seg_off), _ptr(seg_base), seg_base.numel(),
                                  _ptr(out64), _ptr(out32), _stream()), "lgcn_graph_gather")
    return out64, out32


@dataclass
class LanePlan:
    """Tile-major CSR-by-destination of the lane relations (see include/lgcn.h)."""
    rowptr: torch.Tensor
    col: torch.Tensor
    n_rel: int
    n_nodes: int
    n_edges: List[int]


def csr_build(u_list: Sequence[torch.Tensor], v_list: Sequence[torch.Tensor], n_nodes: int) -> LanePlan:
    lib = L.load()
    n_rel = len(u_list)
    if n_rel < 1 or n_rel > L.MAX_REL or len(v_list) != n_rel:
        raise L.LgcnError("csr_build: need 1..%d relations" % L.MAX_REL)
    us = [_dev(u, torch.int64, "u") for u in u_list]
    vs = [_dev(v, torch.int64, "v") for v in v_list]
    ne = [int(u.numel()) for u in us]
    for u, v in zip(us, vs):
        if u.numel() != v.numel():
            raise L.LgcnError("csr_build: u and v differ in length")
    dev = us[0].device
    nk1 = lib.lgcn_csr_rowptr_elems(n_nodes, n_rel)
    rowptr = torch.empty(nk1, dtype=torch.int32, device=dev)
    col = torch.empty(max(sum(ne), 1), dtype=torch.int32, device=dev)
    ws = torch.empty(lib.lgcn_csr_ws_elems(n_nodes, n_rel), dtype=torch.int32, device=dev)
    up = (C.c_void_p * n_rel)(*[u.data_ptr() if u.numel() else 0 for u in us])
    vp = (C.c_void_p * n_rel)(*[v.data_ptr() if v.numel() else 0 for v in vs])
    nn = (C.c_int64 * n_rel)(*ne)
    L.check(lib.lgcn_csr_build(up, vp, nn, n_rel, n_nodes, _ptr(rowptr), _ptr(col), _ptr(ws), _stream()),
            "lgcn_csr_build")
    return LanePlan(rowptr, col, n_rel, n_nodes, ne)


@dataclass
class PairSet:
    """Result of the Att pair search (lanegcn.py:672-689) kept on device."""
    hi: torch.Tensor          # [cap] int32, first P valid
    wi: torch.Tensor          # [cap] int32
    n_pairs: torch.Tensor     # [1] int32 (device)
    rowptr: torch.Tensor      # [T+1] int32: segments of index_add_(0, hi, .)
    cap: int
    n_agt: int
    agt_ctrs: torch.Tensor    # [T,2] concatenated centres
    ctx_ctrs: torch.Tensor    # [S,2]
    _p_host: Optional[int] = None

    def count(self) -> int:
        """P on the host (one device->host read, cached)."""
        if self._p_host is None:
            self._p_host = int(self.n_pairs.item())
            if self._p_host < 0:
                raise L.LgcnError("pair capacity %d exceeded (P = %d)" % (self.cap, -self._p_host))
        return self._p_host

    def csr_by_wi(self, n_ctx: int):
        """Plain CSR of the pairs by context row (rowptr [S+1], col = pair ids, int32): the transpose of the
        gather V[wi] needed by the backward.  Index plumbing on ATen integer ops, cached."""
        if getattr(self, "_wcsr", None) is None:
            P = self.count()
            wi = self.wi[:P].long()
            order = torch.argsort(wi, stable=True)
            # counts without torch.bincount (it reads the maximum back to the host: ~0.7 ms of sync per call)
            counts = torch.zeros(n_ctx, dtype=torch.int64, device=wi.device).index_add_(0, wi, torch.ones_like(wi))
            rowptr = torch.zeros(n_ctx + 1, dtype=torch.int32, device=wi.device)
            rowptr[1:] = torch.cumsum(counts, 0).to(torch.int32)
            self._wcsr = (rowptr, order.to(torch.int32).contiguous())
        return self._wcsr

    def hi_wi_long(self):
        """(hi, wi) as the reference's LongTensors [P] (test/debug accessor; syncs once)."""
        lib = L.load()
        P = self.count()
        h = torch.empty(self.cap, dtype=torch.int64, device=self.hi.device)
        w = torch.empty_like(h)
        L.check(lib.lgcn_widen_i32(_ptr(self.hi), _ptr(self.n_pairs), self.cap, _ptr(h), _stream()), "lgcn_widen_i32")
        L.check(lib.lgcn_widen_i32(_ptr(self.wi), _ptr(self.n_pairs), self.cap, _ptr(w), _stream()), "lgcn_widen_i32")
        return h[:P], w[:P]


def pairs_alloc(n_agt: int, n_scenes: int, cap: int, device):
    """Output / workspace buffers of pairs_build (allocate them on the stream that will consume the pairs when
    the search itself is enqueued on another stream)."""
    lib = L.load()
    i32 = dict(dtype=torch.int32, device=device)
    return (torch.empty(max(cap, 1), **i32), torch.empty(max(cap, 1), **i32), torch.empty(1, **i32),
            torch.empty(n_agt + 1, **i32), torch.empty(lib.lgcn_pairs_ws_elems(n_agt, n_scenes), **i32))


def pairs_build(agt_ctrs: torch.Tensor, agt_off: torch.Tensor, ctx_ctrs: torch.Tensor, ctx_off: torch.Tensor,
                dist_th: float, cap: int, legacy_offsets: bool = True, bufs=None) -> PairSet:
    lib = L.load()
    agt_ctrs = _dev(agt_ctrs, torch.float32, "agt_ctrs")
    ctx_ctrs = _dev(ctx_ctrs, torch.float32, "ctx_ctrs")
    agt_off = _dev(agt_off, torch.int32, "agt_off")
    ctx_off = _dev(ctx_off, torch.int32, "ctx_off")
    B = agt_off.numel() - 1
    if ctx_off.numel() != B + 1 or B < 1:
        raise L.LgcnError("pairs_build: offset tables must both have B+1 entries")
    T, S = agt_ctrs.shape[0], ctx_ctrs.shape[0]
    hi, wi, n_pairs, rowptr, ws = bufs if bufs is not None else pairs_alloc(T, B, cap, agt_ctrs.device)
    L.check(lib.lgcn_pairs_build(_ptr(agt_ctrs), _ptr(agt_off), _ptr(ctx_ctrs), _ptr(ctx_off), B, T, S,
                                 float(dist_th), int(bool(legacy_offsets)), _ptr(hi), _ptr(wi), cap,
                                 _ptr(n_pairs), _ptr(rowptr), _ptr(ws), _stream()), "lgcn_pairs_build")
    return PairSet(hi, wi, n_pairs, rowptr, cap, T, agt_ctrs, ctx_ctrs)


def pairs_build_multi(searches, legacy_offsets: bool = True, bufs=None) -> List["PairSet"]:
    """Up to four pair searches in the same three launches (the forward's A2M, M2A and A2A sets).  `searches`:
    tuples (agt_ctrs, agt_off, ctx_ctrs, ctx_off, dist_th, cap) as for pairs_build; `bufs`: pairs_alloc() per search."""
    lib = L.load()
    n = len(searches)
    if n < 1 or n > 4:
        raise L.LgcnError("pairs_build_multi: 1..4 searches")
    jobs, out, keep = _pairs_jobs(searches, legacy_offsets, bufs)
    L.check(lib.lgcn_pairs_build_multi(jobs, n, _stream()), "lgcn_pairs_build_multi")
    return out


def _pairs_jobs(searches, legacy_offsets, bufs):
    """ctypes job array + PairSets + tensors to keep alive for lgcn_pairs_build_multi / lgcn_index_build."""
    n = len(searches)
    jobs = (L.PairsJob * max(n, 1))()
    out, keep = [], []
    for k, (agt_ctrs, agt_off, ctx_ctrs, ctx_off, dist_th, cap) in enumerate(searches):
        agt_ctrs = _dev(agt_ctrs, torch.float32, "agt_ctrs")
        ctx_ctrs = _dev(ctx_ctrs, torch.float32, "ctx_ctrs")
        agt_off = _dev(agt_off, torch.int32, "agt_off")
        ctx_off = _dev(ctx_off, torch.int32, "ctx_off")
        B = agt_off.numel() - 1
        if ctx_off.numel() != B + 1 or B < 1:
            raise L.LgcnError("pair search: offset tables must both have B+1 entries")
        T, S = agt_ctrs.shape[0], ctx_ctrs.shape[0]
        hi, wi, n_pairs, rowptr, ws = bufs[k] if bufs is not None else pairs_alloc(T, B, cap, agt_ctrs.device)
        j = jobs[k]
        j.agt_ctrs, j.agt_off, j.ctx_ctrs, j.ctx_off = agt_ctrs.data_ptr(), agt_off.data_ptr(), ctx_ctrs.data_ptr(), ctx_off.data_ptr()
        j.n_scenes, j.legacy_offsets, j.n_agt, j.n_ctx, j.dist_th = B, int(bool(legacy_offsets)), T, S, float(dist_th)
        j.hi, j.wi, j.cap = hi.data_ptr(), wi.data_ptr(), cap
        j.n_pairs, j.rowptr, j.ws = n_pairs.data_ptr(), rowptr.data_ptr(), ws.data_ptr()
        keep += [agt_ctrs, ctx_ctrs, agt_off, ctx_off, ws]    # ws must outlive the launch (nothing else holds it)
        out.append(PairSet(hi, wi, n_pairs, rowptr, cap, T, agt_ctrs, ctx_ctrs))
    return jobs, out, keep


def index_counters(n_nodes: int, n_rel: int, device) -> torch.Tensor:
    """A zeroed counter buffer for index_build (lgcn_index_build needs it all zero and leaves it all zero): keep ONE
    per forward that can be in flight -- two launches sharing a buffer concurrently corrupt each other's counts."""
    lib = L.load()
    return torch.zeros(lib.lgcn_index_cnt_words(n_nodes, n_rel), dtype=torch.int64, device=device)


def index_fused_ok(n_nodes: int, n_rel: int, n_edges_total: int) -> bool:
    """Whether lgcn_index_build takes this size (else: graph_gather_indices + csr_build + pairs_build_multi)."""
    lib = L.load()
    return n_edges_total < (1 << 31) and lib.lgcn_csr_rowptr_elems(n_nodes, n_rel) <= (1 << 22)


def index_build(idx_local: torch.Tensor, seg_off: torch.Tensor, seg_base: torch.Tensor, rel_slices, n_nodes: int,
                searches=(), legacy_offsets: bool = True, bufs=None, cnt: Optional[torch.Tensor] = None,
                clear_word: Optional[torch.Tensor] = None):
    """graph_gather + CSR plan + the pair searches in four launches (lgcn_index_build).  rel_slices: per relation
    ((u_begin, u_end), (v_begin, v_end)) element ranges of idx_local.  cnt: index_counters() buffer owned by the caller
    (all zero; comes back all zero); None: a fresh one per call (one extra fill launch).  clear_word: an int32 device
    word that the first launch sets to 0 (the forward's range-guard flag).
    Returns (LanePlan, [PairSet])."""
    lib = L.load()
    idx_local = _dev(idx_local, torch.int64, "idx_local")
    seg_off = _dev(seg_off, torch.int64, "seg_off")
    seg_base = _dev(seg_base, torch.int64, "seg_base")
    n_rel = len(rel_slices)
    if n_rel < 1 or n_rel > L.MAX_REL or len(searches) > 4:
        raise L.LgcnError("index_build: 1..%d relations, <= 4 pair searches" % L.MAX_REL)
    dev = idx_local.device
    ne = [int(ub - ua) for (ua, ub), _ in rel_slices]
    nk1 = lib.lgcn_csr_rowptr_elems(n_nodes, n_rel)
    rowptr = torch.empty(nk1, dtype=torch.int32, device=dev)
    col = torch.empty(max(sum(ne), 1), dtype=torch.int32, device=dev)
    uv = torch.empty(max(2 * sum(ne), 2), dtype=torch.int32, device=dev)
    if cnt is None:
        cnt = index_counters(n_nodes, n_rel, dev)
    elif cnt.numel() < lib.lgcn_index_cnt_words(n_nodes, n_rel) or cnt.dtype != torch.int64 or cnt.device != dev:
        raise L.LgcnError("index_build: counter buffer of the wrong size / type / device")
    jobs, pairs, keep = _pairs_jobs(searches, legacy_offsets, bufs)
    p = L.Index()
    p.idx_local, p.n_elem = idx_local.data_ptr(), idx_local.numel()
    p.seg_off, p.seg_base, p.n_seg, p.n_rel = seg_off.data_ptr(), seg_base.data_ptr(), seg_base.numel(), n_rel
    for r, ((ua, ub), (va, vb)) in enumerate(rel_slices):
        if vb - va != ub - ua:
            raise L.LgcnError("index_build: u and v runs differ in length")
        p.u_off[r], p.v_off[r], p.n_edges[r] = ua, va, ub - ua
    p.n_nodes = n_nodes
    p.rowptr, p.col, p.cnt, p.uv = rowptr.data_ptr(), col.data_ptr(), cnt.data_ptr(), uv.data_ptr()
    p.jobs, p.n_jobs = C.cast(jobs, C.c_void_p).value if len(searches) else 0, len(searches)
    p.clear_word = 0 if clear_word is None else _dev(clear_word, torch.int32, "clear_word").data_ptr()
    L.check(lib.lgcn_index_build(C.byref(p), _stream()), "lgcn_index_build")
    plan = LanePlan(rowptr, col, n_rel, n_nodes, ne)
    plan.__dict__["_idx_keep"] = (cnt, uv, keep)       # alive until the plan is dropped (the launches are asynchronous)
    return plan, pairs


# ------------------------------------------------------------------ ActorNet's convolution block (row f1)
def conv_packed(weight: torch.Tensor) -> torch.Tensor:
    """Packed image of a Conv1d weight [cout, cin, ks] for lgcn_conv1d_gn, cached on the parameter."""
    def make():
        lib = L.load()
        cout, cin, ks = weight.shape
        nbytes = lib.lgcn_conv_packed_bytes(cin, cout, ks)
        if nbytes < 0:
            raise L.LgcnError("conv_packed: unsupported Conv1d weight shape %s" % (tuple(weight.shape),))
        out = torch.empty(nbytes // 4, dtype=torch.int32, device=weight.device)
        w = _dev(weight.detach(), torch.float32, "weight")
        L.check(lib.lgcn_conv_pack_weight(_ptr(w), cin, cout, ks, _ptr(out), _stream()), "lgcn_conv_pack_weight")
        return out
    return _cached(weight, ("conv",), make)


def conv_packed_f32(weight: torch.Tensor) -> torch.Tensor:
    """fp32 fragment image of a Conv1d weight [cout, cin, ks] for lgcn_conv1d_gn_f32 (the exact units), cached on the
    parameter under its own key like conv_packed (rebuilt once the parameter changes)."""
    def make():
        lib = L.load()
        cout, cin, ks = weight.shape
        nbytes = lib.lgcn_conv_packed_f32_bytes(cin, cout, ks)
        if nbytes < 0:
            raise L.LgcnError("conv_packed_f32: unsupported Conv1d weight shape %s" % (tuple(weight.shape),))
        out = torch.empty(nbytes // 4, dtype=torch.float32, device=weight.device)
        w = _dev(weight.detach(), torch.float32, "weight")
        L.check(lib.lgcn_conv_pack_weight_f32(_ptr(w), cin, cout, ks, _ptr(out), _stream()), "lgcn_conv_pack_weight_f32")
        return out
    return _cached(weight, ("convF32",), make)


def conv1d_gn(x: torch.Tensor, weight: torch.Tensor, stride: int, gamma, beta, eps: float, res: Optional[torch.Tensor] = None,
              res_up2: bool = False, relu: bool = False, exact: bool = False) -> torch.Tensor:
    """Conv1d (k = 1 / 3, padding (k - 1) / 2, no bias) + GroupNorm(1, C) + residual + ReLU on channels-last tensors in one
    launch (lgcn_conv1d_gn): x [A, L, Cin] -> [A, Lout, Cout]; res [A, Lout, Cout], or [A, Lout / 2, Cout] with res_up2.
    exact: fp32 operands on the fp32-input MFMA (lgcn_conv1d_gn_f32) instead of two fp16 planes."""
    lib = L.load()
    x = _dev(x, torch.float32, "x")
    A_, lin, cin = x.shape
    cout, cin_w, ks = weight.shape
    if cin_w != cin:
        raise L.LgcnError("conv1d_gn: weight does not match the input's channels")
    lout = (lin + 2 * ((ks - 1) // 2) - ks) // stride + 1
    out = torch.empty((A_, lout, cout), dtype=torch.float32, device=x.device)
    mode = 0
    if res is not None:
        res = _dev(res, torch.float32, "res")
        mode = 2 if res_up2 else 1
        if tuple(res.shape) != ((A_, lout // 2, cout) if res_up2 else (A_, lout, cout)):
            raise L.LgcnError("conv1d_gn: residual of the wrong shape")
    if exact:
        L.check(lib.lgcn_conv1d_gn_f32(_ptr(x), A_, lin, cin, _ptr(conv_packed_f32(weight)), cout, ks, stride,
                                       _ptr(_dev(gamma.detach(), torch.float32, "gamma")),
                                       _ptr(_dev(beta.detach(), torch.float32, "beta")), float(eps), _ptr(res), mode,
                                       int(bool(relu)), _ptr(out), None, _stream()), "lgcn_conv1d_gn_f32")
        return out
    L.check(lib.lgcn_conv1d_gn(_ptr(x), A_, lin, cin, _ptr(conv_packed(weight)), cout, ks, stride,
                               _ptr(_dev(gamma.detach(), torch.float32, "gamma")), _ptr(_dev(beta.detach(), torch.float32, "beta")),
                               float(eps), _ptr(res), mode, int(bool(relu)), _ptr(out), _stream()), "lgcn_conv1d_gn")
    return out


def conv_packed_t(weight: torch.Tensor) -> torch.Tensor:
    """fp32 image wt[t][ci][co] of a Conv1d weight [cout, cin, ks] (ci padded to 16) for the data backward of
    lgcn_conv1d_gn_bwd, cached on the parameter like conv_packed (rebuilt once the parameter changes)."""
    def make():
        lib = L.load()
        cout, cin, ks = weight.shape
        nbytes = lib.lgcn_conv_packed_t_bytes(cin, cout, ks)
        if nbytes < 0:
            raise L.LgcnError("conv_packed_t: unsupported Conv1d weight shape %s" % (tuple(weight.shape),))
        out = torch.empty(nbytes // 4, dtype=torch.float32, device=weight.device)
        w = _dev(weight.detach(), torch.float32, "weight")
        L.check(lib.lgcn_conv_pack_weight_t(_ptr(w), cin, cout, ks, _ptr(out), _stream()), "lgcn_conv_pack_weight_t")
        return out
    return _cached(weight, ("convT",), make)


def conv1d_gn_train(x: torch.Tensor, weight: torch.Tensor, stride: int, gamma, beta, eps: float,
                    res: Optional[torch.Tensor] = None, res_up2: bool = False, relu: bool = False, exact: bool = False):
    """conv1d_gn that also returns the pre-norm convolution output: (out, y), both [A, Lout, Cout] (lgcn_conv1d_gn_train;
    out is bit-identical to conv1d_gn's).  exact: lgcn_conv1d_gn_f32 with y, as conv1d_gn(exact=True)."""
    lib = L.load()
    x = _dev(x, torch.float32, "x")
    A_, lin, cin = x.shape
    cout, cin_w, ks = weight.shape
    if cin_w != cin:
        raise L.LgcnError("conv1d_gn_train: weight does not match the input's channels")
    lout = (lin + 2 * ((ks - 1) // 2) - ks) // stride + 1
    out = torch.empty((A_, lout, cout), dtype=torch.float32, device=x.device)
    y = torch.empty_like(out)
    mode = 0
    if res is not None:
        res = _dev(res, torch.float32, "res")
        mode = 2 if res_up2 else 1
        if tuple(res.shape) != ((A_, lout // 2, cout) if res_up2 else (A_, lout, cout)):
            raise L.LgcnError("conv1d_gn_train: residual of the wrong shape")
    if exact:
        L.check(lib.lgcn_conv1d_gn_f32(_ptr(x), A_, lin, cin, _ptr(conv_packed_f32(weight)), cout, ks, stride,
                                       _ptr(_dev(gamma.detach(), torch.float32, "gamma")),
                                       _ptr(_dev(beta.detach(), torch.float32, "beta")), float(eps), _ptr(res), mode,
                                       int(bool(relu)), _ptr(out), _ptr(y), _stream()), "lgcn_conv1d_gn_f32")
        return out, y
    L.check(lib.lgcn_conv1d_gn_train(_ptr(x), A_, lin, cin, _ptr(conv_packed(weight)), cout, ks, stride,
                                     _ptr(_dev(gamma.detach(), torch.float32, "gamma")),
                                     _ptr(_dev(beta.detach(), torch.float32, "beta")), float(eps), _ptr(res), mode,
                                     int(bool(relu)), _ptr(out), _ptr(y), _stream()), "lgcn_conv1d_gn_train")
    return out, y


def conv1d_gn_bwd(g: torch.Tensor, x: torch.Tensor, y: torch.Tensor, out: Optional[torch.Tensor], weight: torch.Tensor,
                  stride: int, gamma, eps: float, res_mode: int = 0, relu: bool = False, want_dx: bool = True,
                  want_dres: bool = True):
    """Backward of conv1d_gn_train (lgcn_conv1d_gn_bwd): (dx | None, dW, dgamma, dbeta, dres | None).  out: the forward's
    output (its ReLU mask; needed when relu); res_mode 0 none, 1 same-shape residual, 2 x2-upsampled residual."""
    lib = L.load()
    g, x, y = _dev(g, torch.float32, "g"), _dev(x, torch.float32, "x"), _dev(y, torch.float32, "y")
    A_, lin, cin = x.shape
    cout, _, ks = weight.shape
    lout = y.shape[1]
    if tuple(g.shape) != tuple(y.shape):
        raise L.LgcnError("conv1d_gn_bwd: gradient of the wrong shape")
    out = _dev(out, torch.float32, "out") if relu else None
    dev = x.device
    dx = torch.empty_like(x) if want_dx else None
    dw = torch.empty((cout, cin, ks), dtype=torch.float32, device=dev)
    dgamma = torch.empty(cout, dtype=torch.float32, device=dev)
    dbeta = torch.empty_like(dgamma)
    dres = None
    if res_mode and want_dres:
        dres = torch.empty((A_, lout // 2 if res_mode == 2 else lout, cout), dtype=torch.float32, device=dev)
    nbytes = lib.lgcn_conv1d_gn_bwd_ws_bytes(A_, lin, cin, cout, ks, stride)
    if nbytes < 0:
        raise L.LgcnError("conv1d_gn_bwd: unsupported shape")
    ws = torch.empty(max(nbytes // 4, 1), dtype=torch.float32, device=dev)
    L.check(lib.lgcn_conv1d_gn_bwd(_ptr(g), _ptr(x), _ptr(y), _ptr(out), A_, lin, cin, _ptr(conv_packed_t(weight)), cout, ks,
                                   stride, _ptr(_dev(gamma.detach(), torch.float32, "gamma")), float(eps), int(res_mode),
                                   int(bool(relu)), _ptr(dx), _ptr(dw), _ptr(dgamma), _ptr(dbeta), _ptr(dres), _ptr(ws),
                                   _stream()), "lgcn_conv1d_gn_bwd")
    return dx, dw, dgamma, dbeta, dres


def res1d_gn(x: torch.Tensor, block, second=None) -> torch.Tensor:
    """A whole layers.Res1d block (conv1 k3 + GN + ReLU + conv2 k3 + GN + shortcut [identity | conv k1 + GN] + ReLU) on a
    channels-last tensor x [A, L, Cin] in one launch (lgcn_res1d_gn) -> [A, Lout, C]; with `second` (a Res1d with the
    identity shortcut, C -> C) the two blocks run in the same launch (lgcn_res1d_pair_gn)."""
    lib = L.load()
    x = _dev(x, torch.float32, "x")
    A_, lin, cin = x.shape
    c1, c2, ds = block.conv1, block.conv2, block.downsample
    c, stride = c1.out_channels, c1.stride[0]
    if c1.in_channels != cin or c2.in_channels != c or c2.out_channels != c:
        raise L.LgcnError("res1d_gn: block does not match the input's channels")
    lout = (lin + 2 - 3) // stride + 1
    out = torch.empty((A_, lout, c), dtype=torch.float32, device=x.device)
    f32 = lambda t, n: _dev(t.detach(), torch.float32, n)
    wd = gd = bd = None
    if ds is not None:
        wd, gd, bd = conv_packed(ds[0].weight), f32(ds[1].weight, "gd"), f32(ds[1].bias, "bd")
    first = (_ptr(x), A_, lin, cin, c, stride, _ptr(conv_packed(c1.weight)), _ptr(f32(block.bn1.weight, "g1")),
             _ptr(f32(block.bn1.bias, "b1")), _ptr(conv_packed(c2.weight)), _ptr(f32(block.bn2.weight, "g2")),
             _ptr(f32(block.bn2.bias, "b2")), _ptr(wd), _ptr(gd), _ptr(bd))
    if second is None:
        L.check(lib.lgcn_res1d_gn(*first, float(block.bn1.eps), _ptr(out), _stream()), "lgcn_res1d_gn")
        return out
    q1, q2 = second.conv1, second.conv2
    if second.downsample is not None or q1.in_channels != c or q1.out_channels != c or q2.in_channels != c or q2.out_channels != c:
        raise L.LgcnError("res1d_gn: the chained block must be C -> C with the identity shortcut")
    L.check(lib.lgcn_res1d_pair_gn(*first, _ptr(conv_packed(q1.weight)), _ptr(f32(second.bn1.weight, "g1q")),
                                   _ptr(f32(second.bn1.bias, "b1q")), _ptr(conv_packed(q2.weight)),
                                   _ptr(f32(second.bn2.weight, "g2q")), _ptr(f32(second.bn2.bias, "b2q")),
                                   float(block.bn1.eps), _ptr(out), _stream()), "lgcn_res1d_pair_gn")
    return out


# ------------------------------------------------------------------ PredNet's tail (row f1)
def pred_reg(h: Sequence[torch.Tensor], w: Sequence[torch.Tensor], b: Sequence[torch.Tensor], ctrs: torch.Tensor,
             wd: torch.Tensor, bd: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
    """lgcn_pred_reg: reg [A, M, np2 / 2, 2] = w[m] h[m] + b[m] + ctr for the M heads, and AttDest's first layer
    hd [A M, 128] = relu(wd (ctr - reg[:, :, -1]) + bd), in one launch."""
    lib = L.load()
    M, A_ = len(h), h[0].shape[0]
    np2 = w[0].shape[0]
    q = L.PredReg()
    keep = []
    for m in range(M):
        hm, wm, bm = _dev(h[m], torch.float32, "h"), _dev(w[m].detach(), torch.float32, "w"), _dev(b[m].detach(), torch.float32, "b")
        if tuple(hm.shape) != (A_, C_FEAT) or tuple(wm.shape) != (np2, C_FEAT) or tuple(bm.shape) != (np2,):
            raise L.LgcnError("pred_reg: head %d has the wrong shape" % m)
        keep += [hm, wm, bm]
        q.h[m], q.w[m], q.b[m] = hm.data_ptr(), wm.data_ptr(), bm.data_ptr()
    ctrs, wd, bd = _dev(ctrs, torch.float32, "ctrs"), _dev(wd.detach(), torch.float32, "wd"), _dev(bd.detach(), torch.float32, "bd")
    if tuple(ctrs.shape) != (A_, 2) or tuple(wd.shape) != (C_FEAT, 2) or tuple(bd.shape) != (C_FEAT,):
        raise L.LgcnError("pred_reg: ctrs / dist weight of the wrong shape")
    reg = torch.empty((A_, M, np2 // 2, 2), dtype=torch.float32, device=ctrs.device)
    hd = torch.empty((A_ * M, C_FEAT), dtype=torch.float32, device=ctrs.device)
    keep += [ctrs, wd, bd]
    q.ctrs, q.wd, q.bd, q.reg, q.hd = (t.data_ptr() for t in (ctrs, wd, bd, reg, hd))
    q.n_act, q.n_mod, q.np2 = A_, M, np2
    L.check(lib.lgcn_pred_reg(C.byref(q), _stream()), "lgcn_pred_reg")
    return reg, hd


def pred_final(f: torch.Tensor, wc: torch.Tensor, bc: torch.Tensor, reg: torch.Tensor, rot: Optional[torch.Tensor] = None,
               orig: Optional[torch.Tensor] = None) -> Tuple[torch.Tensor, torch.Tensor]:
    """lgcn_pred_final: cls [A, M] (descending) = wc . f + bc and reg's modes in that order, taken to world coordinates
    when rot [A, 2, 2] / orig [A, 2] are given."""
    lib = L.load()
    A_, M, npred, _ = reg.shape
    f, reg = _dev(f, torch.float32, "f"), _dev(reg, torch.float32, "reg")
    wc, bc = _dev(wc.detach().reshape(-1), torch.float32, "wc"), _dev(bc.detach(), torch.float32, "bc")
    if tuple(f.shape) != (A_ * M, C_FEAT) or wc.numel() != C_FEAT or bc.numel() != 1:
        raise L.LgcnError("pred_final: score head of the wrong shape")
    if rot is not None:
        rot, orig = _dev(rot, torch.float32, "rot"), _dev(orig, torch.float32, "orig")
        if tuple(rot.shape) != (A_, 2, 2) or tuple(orig.shape) != (A_, 2):
            raise L.LgcnError("pred_final: rot / orig of the wrong shape")
    cls = torch.empty((A_, M), dtype=torch.float32, device=reg.device)
    out = torch.empty_like(reg)
    L.check(lib.lgcn_pred_final(_ptr(f), _ptr(wc), _ptr(bc), _ptr(reg), _ptr(rot), _ptr(orig), A_, M, npred,
                                _ptr(cls), _ptr(out), _stream()), "lgcn_pred_final")
    return cls, out


def pred_final_train(f: torch.Tensor, wc: torch.Tensor, bc: torch.Tensor, reg: torch.Tensor):
    """lgcn_pred_final_train: pred_final without rot / orig that also returns order [A, M] int32 (the mode that took each
    rank), which pred_final_bwd scatters back through.  cls / out are bit-identical to pred_final's."""
    lib = L.load()
    A_, M, npred, _ = reg.shape
    f, reg = _dev(f, torch.float32, "f"), _dev(reg, torch.float32, "reg")
    wc, bc = _dev(wc.detach().reshape(-1), torch.float32, "wc"), _dev(bc.detach(), torch.float32, "bc")
    if tuple(f.shape) != (A_ * M, C_FEAT) or wc.numel() != C_FEAT or bc.numel() != 1:
        raise L.LgcnError("pred_final_train: score head of the wrong shape")
    cls = torch.empty((A_, M), dtype=torch.float32, device=reg.device)
    out = torch.empty_like(reg)
    order = torch.empty((A_, M), dtype=torch.int32, device=reg.device)
    L.check(lib.lgcn_pred_final_train(_ptr(f), _ptr(wc), _ptr(bc), _ptr(reg), A_, M, 2 * npred, _ptr(cls), _ptr(out),
                                      _ptr(order), _stream()), "lgcn_pred_final_train")
    return cls, out, order


def pred_final_bwd(g_cls: Optional[torch.Tensor], g_out: Optional[torch.Tensor], order: torch.Tensor, f: torch.Tensor,
                   wc: torch.Tensor, n_pred: int, want_reg: bool = True, want_f: bool = True):
    """lgcn_pred_final_bwd: (g_reg [A, M, T, 2] | None, d_f [A M, 128] | None, d_wc [128], d_bc [1]) from the gradients of
    pred_final_train's cls [A, M] and out [A, M, T, 2], T = n_pred; either may be None (zeros)."""
    lib = L.load()
    order, f = _dev(order, torch.int32, "order"), _dev(f, torch.float32, "f")
    A_, M = order.shape
    wc = _dev(wc.detach().reshape(-1), torch.float32, "wc")
    if f.shape[0] != A_ * M or f.shape[1] != C_FEAT or wc.numel() != C_FEAT:
        raise L.LgcnError("pred_final_bwd: score head of the wrong shape")
    if g_cls is not None:
        g_cls = _dev(g_cls, torch.float32, "g_cls")
        if tuple(g_cls.shape) != (A_, M):
            raise L.LgcnError("pred_final_bwd: g_cls of the wrong shape")
    if g_out is not None:
        g_out = _dev(g_out, torch.float32, "g_out")
        if tuple(g_out.shape) != (A_, M, n_pred, 2):
            raise L.LgcnError("pred_final_bwd: g_out of the wrong shape")
    dev = f.device
    g_reg = torch.empty((A_, M, n_pred, 2), dtype=torch.float32, device=dev) if want_reg else None
    d_f = torch.empty_like(f) if want_f else None
    d_wc = torch.empty(C_FEAT, dtype=torch.float32, device=dev)
    d_bc = torch.empty(1, dtype=torch.float32, device=dev)
    n = lib.lgcn_pred_final_bwd_ws_elems(A_)
    if n < 0:
        raise L.LgcnError("pred_final_bwd: unsupported shape")
    part = torch.empty(max(n, 1), dtype=torch.float32, device=dev)
    L.check(lib.lgcn_pred_final_bwd(_ptr(g_cls), _ptr(g_out), _ptr(order), _ptr(f), _ptr(wc), A_, M, 2 * n_pred, _ptr(g_reg),
                                    _ptr(d_f), _ptr(d_wc), _ptr(d_bc), _ptr(part), _stream()), "lgcn_pred_final_bwd")
    return g_reg, d_f, d_wc, d_bc


def pred_reg_bwd(g_reg: torch.Tensor, g_hd: Optional[torch.Tensor], h: Sequence[torch.Tensor], w: Sequence[torch.Tensor],
                 hd: torch.Tensor, reg: torch.Tensor, ctrs: torch.Tensor, want_h: Sequence[bool], want_w: bool = True,
                 want_d: bool = True):
    """lgcn_pred_reg_bwd: (d_h list (None where want_h is False), d_w list, d_b list, d_wd [128, 2], d_bd [128]) from the
    gradients of pred_reg's reg [A, M, T, 2] and hd [A M, 128] (g_hd may be None: zeros).  want_w False: d_w / d_b are
    None; want_d False: d_wd / d_bd are None."""
    lib = L.load()
    M, A_ = len(h), h[0].shape[0]
    np2 = w[0].shape[0]
    g_reg, hd = _dev(g_reg, torch.float32, "g_reg"), _dev(hd, torch.float32, "hd")
    reg, ctrs = _dev(reg, torch.float32, "reg"), _dev(ctrs, torch.float32, "ctrs")
    if g_reg.numel() != A_ * M * np2 or reg.numel() != A_ * M * np2 or tuple(hd.shape) != (A_ * M, C_FEAT) \
            or tuple(ctrs.shape) != (A_, 2):
        raise L.LgcnError("pred_reg_bwd: gradient / saved tensors of the wrong shape")
    if g_hd is not None:
        g_hd = _dev(g_hd, torch.float32, "g_hd")
        if tuple(g_hd.shape) != (A_ * M, C_FEAT):
            raise L.LgcnError("pred_reg_bwd: g_hd of the wrong shape")
    dev = ctrs.device
    new = lambda *shape: torch.empty(shape, dtype=torch.float32, device=dev)
    q = L.PredRegBwd()
    keep, d_h, d_w, d_b = [], [], [], []
    for m in range(M):
        hm, wm = _dev(h[m], torch.float32, "h"), _dev(w[m].detach(), torch.float32, "w")
        if tuple(hm.shape) != (A_, C_FEAT) or tuple(wm.shape) != (np2, C_FEAT):
            raise L.LgcnError("pred_reg_bwd: head %d has the wrong shape" % m)
        keep += [hm, wm]
        d_h.append(new(A_, C_FEAT) if want_h[m] else None)
        d_w.append(new(np2, C_FEAT) if want_w else None)
        d_b.append(new(np2) if want_w else None)
        q.h[m], q.w[m] = hm.data_ptr(), wm.data_ptr()
        q.d_h[m], q.d_w[m], q.d_b[m] = (None if t is None else t.data_ptr() for t in (d_h[m], d_w[m], d_b[m]))
    d_wd, d_bd = (new(C_FEAT, 2), new(C_FEAT)) if want_d else (None, None)
    n = lib.lgcn_pred_reg_bwd_ws_elems(A_, M, np2)
    if n < 0:
        raise L.LgcnError("pred_reg_bwd: unsupported shape")
    part = new(max(n, 4))
    q.g_reg, q.hd, q.reg, q.ctrs, q.part = (t.data_ptr() for t in (g_reg, hd, reg, ctrs, part))
    q.g_hd = None if g_hd is None else g_hd.data_ptr()
    q.d_wd, q.d_bd = (None, None) if not want_d else (d_wd.data_ptr(), d_bd.data_ptr())
    q.n_act, q.n_mod, q.np2 = A_, M, np2
    L.check(lib.lgcn_pred_reg_bwd(C.byref(q), _stream()), "lgcn_pred_reg_bwd")
    return d_h, d_w, d_b, d_wd, d_bd


# ------------------------------------------------------------------ graph construction (row f3)
def dilated_nbrs(u: torch.Tensor, v: torch.Tensor, num_nodes: int, num_scales: int):
    """Scales 1 .. num_scales - 1 of a relation on the device (reference data.dilated_nbrs, data.py:520-534): the
    boolean powers A^(2^i) of the scale-0 adjacency by repeated squaring.  u, v: int64 device tensors (edge u <- v,
    i.e. row u, column v).  Returns a list of {"u", "v"} int64 device tensors, rows ascending, columns ascending
    within a row, every edge once.  Two host reads per scale (the sizes of the candidate and result arrays)."""
    lib = L.load()
    plan = csr_build([u], [v], num_nodes)              # one relation: key(n, 0) = n, a plain CSR by row
    n = plan.rowptr.numel() - 1                        # rows padded to a multiple of 16 (the padding rows are empty)
    dev = plan.rowptr.device
    rowptr, col = plan.rowptr, plan.col
    i32 = dict(dtype=torch.int32, device=dev)
    ws = torch.empty(max(lib.lgcn_scan_ws_elems(n + 1), 1), **i32)
    out = []
    for _ in range(1, num_scales):
        cand_ptr = torch.empty(n + 1, **i32)
        L.check(lib.lgcn_bool_square_bound(_ptr(rowptr), _ptr(col), n, _ptr(cand_ptr), _ptr(ws), _stream()),
                "lgcn_bool_square_bound")
        cand = torch.empty(max(int(cand_ptr[n].item()), 1), **i32)
        out_rowptr = torch.empty(n + 1, **i32)
        L.check(lib.lgcn_bool_square(_ptr(rowptr), _ptr(col), n, _ptr(cand_ptr), _ptr(cand), _ptr(out_rowptr), _ptr(ws),
                                     _stream()), "lgcn_bool_square")
        nnz = int(out_rowptr[n].item())
        out_col, out_row = torch.empty(max(nnz, 1), **i32), torch.empty(max(nnz, 1), **i32)
        L.check(lib.lgcn_bool_square_compact(_ptr(cand_ptr), _ptr(cand), _ptr(out_rowptr), n, _ptr(out_col), _ptr(out_row),
                                             _stream()), "lgcn_bool_square_compact")
        out.append({"u": out_row[:nnz].long(), "v": out_col[:nnz].long()})
        rowptr, col = out_rowptr, out_col
    return out


def cross_edges(ctrs: torch.Tensor, feats: torch.Tensor, lane_idcs: torch.Tensor, num_lanes: int,
                side_pairs: torch.Tensor, pre_pairs: torch.Tensor, suc_pairs: torch.Tensor, cross_dist: float):
    """Left (or right) node adjacency of one scene (lgcn_cross_edges; reference preprocess_data.py:287-392 without
    cross_angle): returns (u, v) int64 device tensors, u ascending."""
    lib = L.load()
    ctrs = _dev(ctrs, torch.float32, "ctrs")
    feats = _dev(feats, torch.float32, "feats")
    lane_idcs = _dev(lane_idcs, torch.int64, "lane_idcs")
    n = ctrs.shape[0]
    pairs = [_dev(t.reshape(-1, 2), torch.int64, "pairs") for t in (side_pairs, pre_pairs, suc_pairs)]
    dev = ctrs.device
    partner = torch.empty(max(n, 1), dtype=torch.int32, device=dev)
    mat = torch.empty(max(num_lanes * num_lanes, 1), dtype=torch.uint8, device=dev)
    L.check(lib.lgcn_cross_edges(_ptr(ctrs), _ptr(feats), _ptr(lane_idcs), n, num_lanes,
                                 _ptr(pairs[0]), pairs[0].shape[0], _ptr(pairs[1]), pairs[1].shape[0],
                                 _ptr(pairs[2]), pairs[2].shape[0], float(cross_dist), _ptr(mat), _ptr(partner),
                                 _stream()), "lgcn_cross_edges")
    partner = partner[:n]
    u = torch.nonzero(partner >= 0).reshape(-1)
    return u, partner[u].long()


# ------------------------------------------------------------------ graph construction, a batch of scenes (lgcn_graphbatch.hip)
def read_back(t: torch.Tensor):
    """The one place where the batched graph ops copy a device tensor to the host (numpy), so that the copies can be
    counted: each is a synchronisation."""
    return t.cpu().numpy()


def _off_tables(tables, what):
    """Offset tables [S + 1] as one contiguous int32 host array (rows) after the checks the library repeats."""
    import numpy as np
    rows = [np.asarray(t, np.int64).reshape(-1) for t in tables]
    if any(len(r) != len(rows[0]) or len(r) < 1 for r in rows):
        raise L.LgcnError("%s: every offset table must hold S + 1 entries" % what)
    return _i32_table(np.stack(rows), what)


def dilate_batch(pre_u, pre_v, suc_u, suc_v, node_off, pre_off, suc_off, num_scales: int):
    """Scales 1 .. num_scales - 1 of pre and suc for a whole batch of scenes (lgcn_dilate_batch_*): what dilated_nbrs
    gives per scene and relation, from flat arrays.  pre_u / pre_v, suc_u / suc_v: int64 device tensors, the scenes'
    scale-0 edges back to back with scene-local node indices; node_off, pre_off, suc_off: host offset tables [S + 1].
    Returns one dict per scale: pre_u, pre_v, suc_u, suc_v (flat int64 device tensors, scene-local, (u, v)-sorted inside
    a scene) and pre_off, suc_off (numpy int64 [S + 1]).  Each scale squares both relations of all scenes at once: three
    launches and ONE read-back (the scene boundaries of the new row pointer, whose ends are the sizes to allocate)."""
    import numpy as np
    lib = L.load()
    off = _off_tables([node_off, pre_off, suc_off], "dilate_batch")
    S = off.shape[1] - 1
    n_nodes, n_pre, n_suc = (int(x) for x in off[:, -1])
    if [int(t.numel()) for t in (pre_u, pre_v, suc_u, suc_v)] != [n_pre, n_pre, n_suc, n_suc]:
        raise L.LgcnError("dilate_batch: the edge offset tables do not end at the edge counts")
    e = [_dev(t.reshape(-1), torch.int64, "dilate_batch edges") for t in (pre_u, pre_v, suc_u, suc_v)]
    dev = e[0].device
    i32, i64 = dict(dtype=torch.int32, device=dev), dict(dtype=torch.int64, device=dev)
    empty = lambda: {"pre_u": torch.empty(0, **i64), "pre_v": torch.empty(0, **i64), "suc_u": torch.empty(0, **i64),
                     "suc_v": torch.empty(0, **i64), "pre_off": np.zeros(S + 1, np.int64), "suc_off": np.zeros(S + 1, np.int64)}
    if S == 0 or n_nodes == 0 or num_scales <= 1:
        return [empty() for _ in range(1, num_scales)]
    n_ws = int(lib.lgcn_dilate_batch_ws_elems(n_nodes, n_pre + n_suc))
    if n_ws < 0:
        L.check(n_ws, "lgcn_dilate_batch_ws_elems")
    n_rp = int(lib.lgcn_csr_rowptr_elems(2 * n_nodes, 1))
    ws, off_dev = torch.empty(n_ws, **i32), torch.from_numpy(off).to(dev)
    p = L.DilateBatch()
    p.n_scenes, p.n_nodes, p.n_pre, p.n_suc = S, n_nodes, n_pre, n_suc
    p.off_host, p.off_dev, p.ws = off.ctypes.data, off_dev.data_ptr(), ws.data_ptr()
    p.pre_u, p.pre_v, p.suc_u, p.suc_v = (t.data_ptr() if t.numel() else None for t in e)
    rowptr, col = torch.empty(n_rp, **i32), torch.empty(max(n_pre + n_suc, 1), **i32)
    p.rowptr, p.col = rowptr.data_ptr(), col.data_ptr()
    L.check(lib.lgcn_dilate_batch_csr(C.byref(p), _stream()), "lgcn_dilate_batch_csr")
    out = []
    for _ in range(1, num_scales):
        out_rowptr, bounds = torch.empty(n_rp, **i32), torch.empty((2, S + 1), **i32)
        p.out_rowptr, p.bounds = out_rowptr.data_ptr(), bounds.data_ptr()
        L.check(lib.lgcn_dilate_batch_count(C.byref(p), _stream()), "lgcn_dilate_batch_count")
        b = read_back(bounds).astype(np.int64)
        nnz = int(b[1, S])
        out_col = torch.empty(max(nnz, 1), **i32)
        out_u, out_v = torch.empty(max(nnz, 1), **i64), torch.empty(max(nnz, 1), **i64)
        p.nnz, p.out_col, p.out_u, p.out_v = nnz, out_col.data_ptr(), out_u.data_ptr(), out_v.data_ptr()
        L.check(lib.lgcn_dilate_batch_fill(C.byref(p), _stream()), "lgcn_dilate_batch_fill")
        cut = int(b[0, S])
        out.append({"pre_u": out_u[:cut], "pre_v": out_v[:cut], "suc_u": out_u[cut:nnz], "suc_v": out_v[cut:nnz],
                    "pre_off": b[0] - b[0, 0], "suc_off": b[1] - b[1, 0]})
        rowptr, col = out_rowptr, out_col
        p.rowptr, p.col = rowptr.data_ptr(), col.data_ptr()
    return out


def cross_edges_batch(ctrs, feats, lane_idcs, pre_pairs, suc_pairs, left_pairs, right_pairs, node_off, lane_off, pre_off,
                      suc_off, left_off, right_off, cross_dist: float):
    """Left and right node adjacency of a whole batch of scenes (lgcn_cross_edges_batch): what cross_edges gives per scene
    and side, from flat arrays.  ctrs, feats [N,2] fp32, lane_idcs [N] int64 (scene-local lanes), the pair lists [k,2]
    int64 (scene-local lanes), all on the device, the scenes back to back; the offset tables are host arrays [S + 1].
    Returns {"left_u", "left_v", "right_u", "right_v"} (flat int16 device tensors, scene-local, u ascending inside a
    scene) and {"left_off", "right_off"} (numpy int64 [S + 1]).  One memset and four launches; ONE read-back (the counts)."""
    import numpy as np
    lib = L.load()
    six = _off_tables([node_off, lane_off, pre_off, suc_off, left_off, right_off], "cross_edges_batch").astype(np.int64)
    S = six.shape[1] - 1
    n_lane, per = np.diff(six[1]), np.diff(six[2]) + np.diff(six[3]) + 1
    csum = lambda x: np.concatenate([[0], np.cumsum(x, dtype=np.int64)])
    off = _i32_table(np.concatenate([six, np.stack([csum(n_lane * n_lane), csum(np.diff(six[4]) * per),
                                                    csum(np.diff(six[5]) * per)])]), "cross_edges_batch")
    ctrs, feats = _dev(ctrs, torch.float32, "ctrs"), _dev(feats, torch.float32, "feats")
    lane_idcs = _dev(lane_idcs, torch.int64, "lane_idcs")
    pairs = [_dev(t.reshape(-1, 2), torch.int64, "pairs") for t in (pre_pairs, suc_pairs, left_pairs, right_pairs)]
    n_nodes = int(six[0, -1])
    if ctrs.numel() != 2 * n_nodes or feats.numel() != 2 * n_nodes or lane_idcs.numel() != n_nodes or \
            [t.shape[0] for t in pairs] != [int(x) for x in six[2:, -1]]:
        raise L.LgcnError("cross_edges_batch: the offset tables do not end at the array sizes")
    dev = ctrs.device
    i16 = dict(dtype=torch.int16, device=dev)
    if S == 0:
        z = torch.empty(0, **i16)
        return {"left_u": z, "left_v": z, "right_u": z, "right_v": z}, {"left_off": np.zeros(1, np.int64),
                                                                         "right_off": np.zeros(1, np.int64)}
    n_ws = int(lib.lgcn_cross_edges_batch_ws_elems(n_nodes))
    if n_ws < 0:
        L.check(n_ws, "lgcn_cross_edges_batch_ws_elems")
    ws, off_dev = torch.empty(max(n_ws, 1), dtype=torch.int32, device=dev), torch.from_numpy(off).to(dev)
    mat = torch.empty(max(2 * int(off[6, -1]), 1), dtype=torch.uint8, device=dev)
    counts = torch.empty((2, S + 1), dtype=torch.int32, device=dev)
    out_u, out_v = torch.empty(max(2 * n_nodes, 1), **i16), torch.empty(max(2 * n_nodes, 1), **i16)
    p = L.CrossBatch()
    p.n_scenes, p.cross_dist = S, float(cross_dist)
    p.n_nodes, p.n_lanes, p.n_pre, p.n_suc, p.n_left, p.n_right = (int(x) for x in six[:, -1])
    p.off_host, p.off_dev = off.ctypes.data, off_dev.data_ptr()
    p.ctrs, p.feats, p.lane_idcs = (t.data_ptr() if n_nodes else None for t in (ctrs, feats, lane_idcs))
    p.pre_pairs, p.suc_pairs, p.left_pairs, p.right_pairs = (t.data_ptr() if t.numel() else None for t in pairs)
    p.mat, p.ws, p.counts, p.out_u, p.out_v = mat.data_ptr(), ws.data_ptr(), counts.data_ptr(), out_u.data_ptr(), out_v.data_ptr()
    L.check(lib.lgcn_cross_edges_batch(C.byref(p), _stream()), "lgcn_cross_edges_batch")
    c = read_back(counts).astype(np.int64)
    (l0, l1), (r0, r1) = (int(c[0, 0]), int(c[0, S])), (int(c[1, 0]), int(c[1, S]))
    return ({"left_u": out_u[l0:l1], "left_v": out_v[l0:l1], "right_u": out_u[r0:r1], "right_v": out_v[r0:r1]},
            {"left_off": c[0] - c[0, 0], "right_off": c[1] - c[1, 0]})


# ------------------------------------------------------------------ weight packing
def _cached(weight: torch.Tensor, key, make):
    """Per-tensor-object cache, valid while (data_ptr, _version) are unchanged.  Living on the
    Parameter object itself, an entry can never be hit through a recycled device address of some
    other tensor.  (Writes through ``param.data`` do not bump ``_version``: call
    ``invalidate_packed(param)`` after such an edit.)"""
    cache = weight.__dict__.setdefault("_lgcn_cache", {})
    stamp = (weight.data_ptr(), weight._version, weight.device)
    hit = cache.get(key)
    if hit is not None and hit[0] == stamp:
        return hit[1]
    out = make()
    cache[key] = (stamp, out)
    return out


def invalidate_packed(weight: torch.Tensor):
    weight.__dict__.pop("_lgcn_cache", None)


# Every cached [128,128] image is also listed here, so that a training loop can rebuild all of them after an
# optimizer step with ONE launch (lgcn_pack_weight_batch) instead of ~400 single ones on first use.
_pack_jobs = []        # [weakref(weight), cache key, out, col0, transpose, mma]
_pack_tables = {}      # mma -> (job ids, device table [n,3] int64) of the last full refresh


def _register_pack(weight, key, out, col0, transpose, mma):
    import weakref
    _pack_jobs.append([weakref.ref(weight), key, out, col0, transpose, mma])


def refresh_packed(force: bool = False) -> int:
    """Re-pack, in place, every registered image whose parameter changed since it was packed (optimizer step:
    reference train.py:190).  One launch per matrix-core mode in use.  Returns the number of images rebuilt.
    force: every live registered image of a CUDA weight is rebuilt and restamped without looking at its stamp -- for a
    writer that goes through raw pointers (optim_hip.FusedOptim), after which (data_ptr, _version) says nothing; the
    device table of the last such call is reused while the job list is unchanged."""
    if not _pack_jobs:
        return 0
    lib = L.load()
    stale = {}
    alive = []
    for job in _pack_jobs:
        w = job[0]()
        if w is None:
            continue
        entry = w.__dict__.get("_lgcn_cache", {}).get(job[1])
        if entry is None or entry[1] is not job[2] or not w.is_cuda:
            continue                     # cache entry dropped or replaced: nothing to refresh
        alive.append(job)
        if force or entry[0] != (w.data_ptr(), w._version, w.device):
            stale.setdefault(job[5], []).append((job, w))
    _pack_jobs[:] = alive
    n = 0
    for mma, items in stale.items():
        ids = tuple(id(j) for j, _ in items)
        hit = _pack_tables.get(mma)
        if hit is not None and hit[0] == ids and all(h == w.data_ptr() for h, (_, w) in zip(hit[2], items)):
            table = hit[1]
        else:
            rows = [[w.data_ptr() + 4 * j[3], j[2].data_ptr(), w.stride(0) | (int(j[4]) << 32)] for j, w in items]
            table = torch.tensor(rows, dtype=torch.int64).to(items[0][1].device)
            _pack_tables[mma] = (ids, table, [w.data_ptr() for _, w in items])
        L.check(lib.lgcn_pack_weight_batch(_ptr(table), len(items), mma, _stream()), "lgcn_pack_weight_batch")
        for j, w in items:
            w.__dict__["_lgcn_cache"][j[1]] = ((w.data_ptr(), w._version, w.device), j[2])
        n += len(items)
    return n


def packed(weight: torch.Tensor, col0: int = 0, k: Optional[int] = None) -> torch.Tensor:
    """MFMA-packed image of weight[:, col0:col0+k] ([128, k] slice of an nn.Linear weight); cached
    on the parameter and rebuilt only after the parameter changes."""
    lib = L.load()
    if weight.dim() != 2 or weight.shape[0] != C_FEAT:
        raise L.LgcnError("packed(): weight must be [128, K]")
    k = weight.shape[1] - col0 if k is None else k

    mma = _mma

    def make():
        w = _dev(weight.detach(), torch.float32, "weight")
        k_pad = (k + 7) // 8 * 8
        nbytes = lib.lgcn_packed_bytes(k_pad, mma)
        if nbytes < 0:
            raise L.LgcnError("packed(): K = %d is not supported in mma mode %d" % (k, mma))
        out = torch.empty(nbytes // 4, dtype=torch.float32, device=w.device)
        src = w[:, col0:]
        L.check(lib.lgcn_pack_weight(C.c_void_p(src.data_ptr()), w.stride(0), k, k_pad, mma, _ptr(out), _stream()),
                "lgcn_pack_weight")
        if k == C_FEAT:
            _register_pack(weight, ("pack", col0, k, mma), out, col0, 0, mma)
        return out

    return _cached(weight, ("pack", col0, k, mma), make)


def packed_t(weight: torch.Tensor, col0: int = 0) -> torch.Tensor:
    """MFMA image of the TRANSPOSE of the square block weight[:, col0:col0+128]: the backward of
    y = x W^T is dx = dy W, a Linear whose weight is W^T.  Cached like packed()."""
    lib = L.load()
    if weight.dim() != 2 or weight.shape[0] != C_FEAT or weight.shape[1] < col0 + C_FEAT:
        raise L.LgcnError("packed_t(): need a [128, >= col0+128] weight")
    mma = _mma

    def make():
        w = _dev(weight.detach(), torch.float32, "weight")
        out = torch.empty(lib.lgcn_packed_bytes(C_FEAT, mma) // 4, dtype=torch.float32, device=w.device)
        L.check(lib.lgcn_pack_weight_t(C.c_void_p(w[:, col0:].data_ptr()), w.stride(0), mma, _ptr(out), _stream()),
                "lgcn_pack_weight_t")
        _register_pack(weight, ("packT", col0, mma), out, col0, 1, mma)
        return out

    return _cached(weight, ("packT", col0, mma), make)


def cols4(weight: torch.Tensor, col0: int) -> torch.Tensor:
    """Contiguous [128, 4] copy of weight[:, col0:col0+4] (the 4 meta columns of A2M.meta), cached."""
    return _cached(weight, ("c4", col0), lambda: _dev(weight.detach(), torch.float32, "weight")[:, col0:col0 + 4].contiguous())


# ------------------------------------------------------------------ per-kernel timing hook
_timer = None


class kernel_timer:
    """``with ops.kernel_timer() as t:`` brackets every tagged launch with HIP events recorded on the
    stream the kernel is launched on (torch's current stream); ``t.summary()`` -> {tag: [ms, ...]}.
    Used by bench.py for the roofline of the dominant kernel; off (zero overhead) otherwise."""

    def __enter__(self):
        global _timer
        self.recs = []
        _timer = self
        return self

    def __exit__(self, *a):
        global _timer
        _timer = None

    def summary(self):
        torch.cuda.synchronize()
        out = {}
        for tag, e0, e1 in self.recs:
            out.setdefault(tag, []).append(e0.elapsed_time(e1))
        return out


class _Timed:
    def __init__(self, tag):
        self.on = _timer is not None and tag is not None
        self.tag = tag

    def __enter__(self):
        if self.on:
            self.e0 = torch.cuda.Event(enable_timing=True)
            self.e1 = torch.cuda.Event(enable_timing=True)
            self.e0.record()

    def __exit__(self, *a):
        if self.on:
            self.e1.record()
            _timer.recs.append((self.tag, self.e0, self.e1))


# ------------------------------------------------------------------ fp path
@dataclass
class RelSpec:
    src: torch.Tensor
    wp: Optional[torch.Tensor]      # packed weight (None for lgcn_wgrad)
    mode: int = L.REL_IDENT
    ridx: int = 0


def _agg_params(n_rows: int, rels: Sequence[RelSpec], flags: int, *, rowptr=None, col=None, n_rel_csr=0,
                gn1=None, wp2=None, gn2=None, res=None, x4=None, w4=None, out=None, out_pre=None, out_mid=None,
                out_pre2=None, eps=EPS, tile_rb=0, chain_u=None, chain_v=None):
    """Fill one lgcn_agg_mlp_t.  Returns (struct, tensors to keep alive until the launch is enqueued, out).
    chain_u = (wq packed, (gamma, beta), wu packed): also ReLU(GN_q(out wq^T)) wu^T -> out becomes (out, U[, V]);
    chain_v = wv packed: also out wv^T (lgcn.h: the chained outputs of a row block)."""
    if not rels or len(rels) > L.MAX_REL:
        raise L.LgcnError("agg_mlp: 1..%d relations" % L.MAX_REL)
    dev = rels[0].src.device
    p = L.AggMlp()
    p.n_rows, p.n_rel, p.n_rel_csr, p.flags, p.eps = n_rows, len(rels), n_rel_csr, flags, eps
    p.mma, p.tile_rb = _mma, tile_rb
    keep = []
    for i, r in enumerate(rels):
        s = _dev(r.src, torch.float32, "rel.src")
        keep += [s, r.wp]
        p.rel[i].src, p.rel[i].wp, p.rel[i].mode, p.rel[i].ridx = s.data_ptr(), r.wp.data_ptr(), r.mode, r.ridx
    p.rowptr = 0 if rowptr is None else rowptr.data_ptr()
    p.col = 0 if col is None else col.data_ptr()
    if w4 is not None:
        xa, xb, xc = (_dev(t, torch.float32, "x4") for t in x4)
        w4 = _dev(w4, torch.float32, "w4")
        keep += [xa, xb, xc, w4]
        p.x4_a, p.x4_b, p.x4_c, p.w4 = xa.data_ptr(), xb.data_ptr(), xc.data_ptr(), w4.data_ptr()
    if gn1 is not None:
        p.gn1_g, p.gn1_b = gn1[0].data_ptr(), gn1[1].data_ptr()
    if wp2 is not None:
        p.wp2 = wp2.data_ptr()
    if gn2 is not None:
        p.gn2_g, p.gn2_b = gn2[0].data_ptr(), gn2[1].data_ptr()
    if res is not None:
        res = _dev(res, torch.float32, "res")
        keep.append(res)
        p.res = res.data_ptr()
    if out is None:
        out = torch.empty((n_rows, C_FEAT), dtype=torch.float32, device=dev)
    p.out = out.data_ptr()
    p.out_pre = 0 if out_pre is None else out_pre.data_ptr()
    p.out_mid = 0 if out_mid is None else out_mid.data_ptr()
    p.out_pre2 = 0 if out_pre2 is None else out_pre2.data_ptr()
    if chain_u is not None or chain_v is not None:
        outs = [out]
        if chain_u is not None:
            wq, gq, wu = chain_u
            u = torch.empty((n_rows, C_FEAT), dtype=torch.float32, device=dev)
            keep += [wq, gq[0], gq[1], wu]
            p.ch_wq, p.ch_gq_g, p.ch_gq_b, p.ch_wu, p.ch_u_out = wq.data_ptr(), gq[0].data_ptr(), gq[1].data_ptr(), wu.data_ptr(), u.data_ptr()
            outs.append(u)
        if chain_v is not None:
            v = torch.empty((n_rows, C_FEAT), dtype=torch.float32, device=dev)
            keep.append(chain_v)
            p.ch_wv, p.ch_v_out = chain_v.data_ptr(), v.data_ptr()
            outs.append(v)
        out = tuple(outs)
    return p, keep, out


def agg_mlp(n_rows: int, rels: Sequence[RelSpec], flags: int, *, tag=None, **kw):
    """Fused aggregate -> GEMM -> GN -> ReLU -> GEMM -> GN -> +res -> ReLU row block (lgcn_agg_mlp).
    Keywords: rowptr, col, n_rel_csr, gn1, wp2, gn2, res, x4, w4, out, out_pre, out_mid, out_pre2, eps, tile_rb."""
    lib = L.load()
    p, keep, out = _agg_params(n_rows, rels, flags, **kw)
    with _Timed(tag):
        L.check(lib.lgcn_agg_mlp(C.byref(p), _stream()), "lgcn_agg_mlp")
    return out


def agg_mlp_pair(a: dict, b: dict, tag=None):
    """Two independent row blocks in one launch (lgcn_agg_mlp_pair).  a, b: keyword dicts of agg_mlp
    (n_rows, rels, flags, ...).  Returns (out_a, out_b)."""
    lib = L.load()
    pa, ka, oa = _agg_params(**a)
    pb, kb, ob = _agg_params(**b)
    with _Timed(tag):
        L.check(lib.lgcn_agg_mlp_pair(C.byref(pa), C.byref(pb), _stream()), "lgcn_agg_mlp_pair")
    return oa, ob


def agg_mlp_multi(problems: Sequence[dict], tag=None):
    """Up to 4 independent row blocks in one launch (lgcn_agg_mlp_multi).  problems: keyword dicts of agg_mlp.
    Returns their outputs in order (a tuple per problem with chained outputs)."""
    lib = L.load()
    built = [_agg_params(**kw) for kw in problems]
    arr = (C.POINTER(L.AggMlp) * len(built))(*[C.pointer(b[0]) for b in built])
    with _Timed(tag):
        L.check(lib.lgcn_agg_mlp_multi(arr, len(built), _stream()), "lgcn_agg_mlp_multi")
    return [b[2] for b in built]


def ctx_heads_ok() -> bool:
    """lgcn_ctx_heads implements the current matrix-core mode (f16x2, bf16); the others take agg_mlp."""
    return _mma in (L.MMA_F16X2, L.MMA_BF16)


def ctx_heads(x: torch.Tensor, wps: Sequence[torch.Tensor], outs: Optional[Sequence[torch.Tensor]] = None, tag="ctx_heads"):
    """[x W_j^T for j] for one or two packed [128,128] weights over the same rows, one weight-stationary launch
    (lgcn_ctx_heads): bit for bit what agg_mlp gives with one IDENT relation and flags = 0.  f16x2 / bf16 only
    (ctx_heads_ok(); the library refuses the other modes)."""
    lib = L.load()
    x = _dev(x, torch.float32, "x")
    if x.dim() != 2 or x.shape[1] != C_FEAT or not 1 <= len(wps) <= 2:
        raise L.LgcnError("ctx_heads: x must be [N,128], with one or two weights")
    n = x.shape[0]
    if outs is None:
        outs = [torch.empty((n, C_FEAT), dtype=torch.float32, device=x.device) for _ in wps]
    if len(outs) != len(wps) or any(o.shape != (n, C_FEAT) or o.dtype != torch.float32 or not o.is_contiguous()
                                    or o.device != x.device for o in outs):
        raise L.LgcnError("ctx_heads: every output must be a contiguous fp32 [N,128] tensor on x's device")
    w = (C.c_void_p * len(wps))(*[t.data_ptr() for t in wps])
    o = (C.c_void_p * len(wps))(*[t.data_ptr() for t in outs])
    with _Timed(tag):
        L.check(lib.lgcn_ctx_heads(_ptr(x), n, w, len(wps), _mma, o, _stream()), "lgcn_ctx_heads")
    return list(outs)


def node_tail_ok() -> bool:
    """lgcn_node_tail is in the library and implements the current matrix-core mode (f16x2, bf16); the others take agg_mlp."""
    return _mma in (L.MMA_F16X2, L.MMA_BF16) and hasattr(L.load(), "lgcn_node_tail")


def node_tail(n_rows: int, rels: Sequence[RelSpec], flags: int, *, tag="node_tail", **kw):
    """An Att tail over many target rows -- rels = [IDENT(agts, W_agt), RANGE(m, W_c1)], every flag, gn1, wp2, gn2, res,
    optionally chain_u -- in one weight-stationary launch (lgcn_node_tail): bit for bit what agg_mlp gives with the same
    arguments.  The library refuses every other shape and the f32 / bf16x3 modes (node_tail_ok())."""
    lib = L.load()
    p, keep, out = _agg_params(n_rows, rels, flags, **kw)
    with _Timed(tag):
        L.check(lib.lgcn_node_tail(C.byref(p), _stream()), "lgcn_node_tail")
    return out


def node_head_ok() -> bool:
    """lgcn_node_head is in the library and implements the current matrix-core mode (f16x2, bf16); the others take
    agg_mlp_multi."""
    return _mma in (L.MMA_F16X2, L.MMA_BF16) and hasattr(L.load(), "lgcn_node_head")


def node_head_form(kw: dict) -> Optional[str]:
    """The form lgcn_node_head runs an agg_mlp problem (keyword dict) as -- "head", "u-chain" or "plain" -- or None."""
    rels, flags = kw.get("rels", ()), kw.get("flags")
    if len(rels) != 1 or rels[0].mode != L.REL_IDENT or kw.get("chain_v") is not None or kw.get("tile_rb", 0) != 0:
        return None
    if any(kw.get(k) is not None for k in ("out_pre", "out_mid", "out_pre2")):
        return None
    if flags == L.F_GN1 | L.F_RELU1:
        return "head"
    if kw.get("w4") is not None or kw.get("chain_u") is not None:
        return None
    return {L.F_GN1 | L.F_RELU1 | L.F_GEMM2: "u-chain", 0: "plain"}.get(flags)


def node_head(problems: Sequence[dict], tag="att_head"):
    """Up to 4 row-chain problems over one IDENT relation each -- a head (GN1 | RELU1, optionally w4 / x4 and chain_u), a
    u-chain (GN1 | RELU1 | GEMM2) or a plain GEMM (flags 0) -- in one weight-stationary launch (lgcn_node_head): bit for bit
    what agg_mlp_multi gives on the same list, outputs returned alike.  The library refuses every other shape and the
    f32 / bf16x3 modes (node_head_ok(), node_head_form())."""
    lib = L.load()
    built = [_agg_params(**kw) for kw in problems]
    arr = (C.POINTER(L.AggMlp) * len(built))(*[C.pointer(b[0]) for b in built])
    with _Timed(tag):
        L.check(lib.lgcn_node_head(arr, len(built), _stream()), "lgcn_node_head")
    return [b[2] for b in built]


# ------------------------------------------------------------------ LaneConv (gather-free, weight-stationary)
@dataclass
class LcPlan:
    """Work-item plan of lgcn_laneconv_fwd for one lane graph and one row-block geometry (include/lgcn.h)."""
    plan: torch.Tensor            # int32 words (lgcn_lc_plan_build)
    lane: LanePlan
    rows_per_block: int
    cap: int
    n_units: int
    gstart: List[int]             # unit groups: one workgroup per (row block, group)


def lc_config(mma: Optional[int] = None, variant: int = 0):
    """(rows_per_block, LDS source-row capacity) of a matrix mode (variant 0: shared, 1: tall, 2: short);
    None for LGCN_MMA_F32 and LGCN_MMA_BF16X3: those modes run the one-launch lgcn_agg_mlp LaneConv (the three-plane
    shapes of the weight-stationary kernel needed scratch and were slower: removed in round 3)."""
    lib = L.load()
    mma = _mma if mma is None else mma
    if mma in (L.MMA_F32, L.MMA_BF16X3):
        return None
    m, c = C.c_int32(), C.c_int32()
    L.check(lib.lgcn_lc_config(mma, variant, C.byref(m), C.byref(c)), "lgcn_lc_config")
    return m.value, c.value


def lc_groups(n_units: int, n_groups: int) -> List[int]:
    """Consecutive, near-equal unit groups: [0, ..., n_units]."""
    n_groups = max(1, min(n_groups, n_units))
    return [(g * n_units + n_groups - 1) // n_groups for g in range(n_groups)] + [n_units]


_cu_cache = {}


def cu_count(device) -> int:
    idx = torch.device(device).index
    idx = torch.cuda.current_device() if idx is None else idx
    if idx not in _cu_cache:
        _cu_cache[idx] = torch.cuda.get_device_properties(idx).multi_processor_count
    return _cu_cache[idx]


_lc_groups_forced = 0
_lc_impl = "tiled"


def set_laneconv_impl(name: str):
    """"tiled" (lgcn_laneconv_fwd) or "fused" (one lgcn_agg_mlp launch per layer) for inference LaneConv layers."""
    global _lc_impl
    if name not in ("tiled", "fused"):
        raise L.LgcnError("laneconv impl must be 'tiled' or 'fused'")
    _lc_impl = name


def laneconv_impl() -> str:
    return _lc_impl


def set_lc_groups(n: int):
    """Force the number of unit groups of subsequently built LaneConv plans (0 = pick by CU count)."""
    global _lc_groups_forced
    _lc_groups_forced = int(n)


def lc_plan(lane: LanePlan, n_groups: Optional[int] = None, cap: Optional[int] = None,
            variant: Optional[int] = None) -> Optional[LcPlan]:
    """LaneConv work-item plan for the current matrix mode, built once per lane graph and cached on it.
    variant: 0 = shared (96-row blocks, two workgroups per CU), 1 = tall (192 rows, the whole CU), 2 = short (48 rows,
    one launch per layer, within the shared budget); default: short while its row blocks fit the CUs once, tall from
    two tall blocks per CU.
    n_groups: unit groups per row block (default 1: one launch per layer, no partial sums; more groups buy
    parallelism for a single small forward at the price of a second launch)."""
    if lc_config() is None:
        return None
    lib = L.load()
    if variant is None:
        cus = cu_count(lane.rowptr.device)
        m_tall, _ = lc_config(variant=1)
        m_short, _ = lc_config(variant=2)
        if (lane.n_nodes + m_short - 1) // m_short <= cus:
            # a small batch: one short row block per CU finishes the layer in one launch; the shape stays within
            # 128 VGPRs / 79 KB of LDS, so the layers of forwards in flight overlap two per CU
            variant = 2
        else:
            variant = 1 if (lane.n_nodes + m_tall - 1) // m_tall >= 2 * cus else 0
    M, cap_max = lc_config(variant=variant)
    cap = cap_max if cap is None else cap
    n_units = lane.n_rel + 1
    if n_groups is None:
        # one group (one launch per layer, no partial sums) once the row blocks alone fill the chip; small batches
        # buy parallelism with unit groups (S2, 108 short row blocks on 256 CUs: two groups)
        n_blocks = (lane.n_nodes + M - 1) // M
        n_groups = _lc_groups_forced if _lc_groups_forced > 0 else 1 if variant == 2 else max(1, min(4, round(cu_count(lane.rowptr.device) / max(n_blocks, 1))))
    gstart = lc_groups(n_units, n_groups)
    cache = lane.__dict__.setdefault("_lc", {})
    key = (M, cap, tuple(gstart))
    hit = cache.get(key)
    if hit is not None:
        return hit
    n_words = lib.lgcn_lc_plan_elems(lane.n_nodes, M, cap)
    if n_words < 0:
        raise L.LgcnError("lc_plan: bad geometry (n_nodes=%d, M=%d, cap=%d)" % (lane.n_nodes, M, cap))
    plan = torch.empty(max(n_words, 4), dtype=torch.int32, device=lane.rowptr.device)
    gs = (C.c_int32 * len(gstart))(*gstart)
    L.check(lib.lgcn_lc_plan_build(_ptr(lane.rowptr), _ptr(lane.col), lane.n_nodes, lane.n_rel, M, cap,
                                   len(gstart) - 1, gs, _ptr(plan), _stream()), "lgcn_lc_plan_build")
    out = LcPlan(plan, lane, M, cap, n_units, gstart)
    cache[key] = out
    return out


def lc_part(lcp: LcPlan) -> Optional[torch.Tensor]:
    """Partial-sum workspace of lgcn_laneconv_fwd (may be shared by consecutive layers on one stream); None for
    single-group plans, which need none."""
    lib = L.load()
    n = lib.lgcn_lc_part_elems(lcp.lane.n_nodes, lcp.rows_per_block, len(lcp.gstart) - 1)
    if n <= 0:
        return None
    return torch.empty(n, dtype=torch.float32, device=lcp.plan.device)


def laneconv_fwd(x: torch.Tensor, lcp: LcPlan, wps: Sequence[Optional[torch.Tensor]], gn1, wp2, gn2, eps=EPS,
                 part: Optional[torch.Tensor] = None, out: Optional[torch.Tensor] = None, tag="laneconv"):
    """One LaneConv layer (lgcn_laneconv_fwd): wps[u] = packed weight of unit u (ctr, then the plan's relations;
    None for a relation without edges)."""
    lib = L.load()
    x = _dev(x, torch.float32, "x")
    if x.shape[0] != lcp.lane.n_nodes or len(wps) != lcp.n_units:
        raise L.LgcnError("laneconv_fwd: x / weights do not match the plan")
    p = L.LaneConv()
    p.n_rows, p.x = x.shape[0], x.data_ptr()
    for u, w in enumerate(wps):
        p.wp[u] = 0 if w is None else w.data_ptr()
    p.col, p.plan = lcp.lane.col.data_ptr(), lcp.plan.data_ptr()
    p.rows_per_block, p.cap, p.n_units, p.n_groups = lcp.rows_per_block, lcp.cap, lcp.n_units, len(lcp.gstart) - 1
    for g, v in enumerate(lcp.gstart):
        p.gstart[g] = v
    p.gn1_g, p.gn1_b, p.wp2, p.gn2_g, p.gn2_b = gn1[0].data_ptr(), gn1[1].data_ptr(), wp2.data_ptr(), gn2[0].data_ptr(), gn2[1].data_ptr()
    p.eps, p.mma = eps, _mma
    if part is None:
        part = lc_part(lcp)
    if out is None:
        out = torch.empty_like(x)
    p.part, p.out = (0 if part is None else part.data_ptr()), out.data_ptr()
    with _Timed(tag):
        L.check(lib.lgcn_laneconv_fwd(C.byref(p), _stream()), "lgcn_laneconv_fwd")
    return out


def mapnet_input(ctrs, feats, wa1, ba1, wpa2, gn_a, ws1, bs1, wps2, gn_s, eps=EPS):
    lib = L.load()
    ctrs = _dev(ctrs, torch.float32, "ctrs")
    feats = _dev(feats, torch.float32, "feats")
    n = ctrs.shape[0]
    out = torch.empty((n, C_FEAT), dtype=torch.float32, device=ctrs.device)
    L.check(lib.lgcn_mapnet_input(_ptr(ctrs), _ptr(feats), n, _ptr(wa1), _ptr(ba1), _ptr(wpa2), _ptr(gn_a[0]),
                                  _ptr(gn_a[1]), _ptr(ws1), _ptr(bs1), _ptr(wps2), _ptr(gn_s[0]), _ptr(gn_s[1]),
                                  eps, _mma, _ptr(out), _stream()), "lgcn_mapnet_input")
    return out


# Per-pair MLP of Att in the 16-bit-plane modes: "wi" (default) = lgcn_att_pairs_wi, wave-independent 16-pair blocks
# with the weights in LDS one at a time (f16x2 / bf16); "ws" = lgcn_att_pairs_ws, both weights in registers (bf16x3,
# which "wi" does not implement).  f32 runs "stream" = lgcn_att_pairs, weight fragments streamed per 32-pair tile.
_att_pairs_impl = "wi"


def set_att_pairs_impl(name: str):
    """"wi" (default) or "ws" where the mode has both (f16x2 / bf16)."""
    global _att_pairs_impl
    if name not in ("wi", "ws"):
        raise L.LgcnError("att pairs impl must be 'wi' or 'ws'")
    _att_pairs_impl = name


def att_pairs_impl() -> str:
    """The pair-MLP kernel of the current matrix mode: f32 has only "stream"; "wi" runs on two or one 16-bit weight
    plane (f16x2 / bf16), bf16x3 falls back to "ws"."""
    if _mma == L.MMA_F32:
        return "stream"
    if _att_pairs_impl == "wi" and _mma not in (L.MMA_F16X2, L.MMA_BF16):
        return "ws"
    return _att_pairs_impl


def packed_kperm(weight: torch.Tensor, col0: int = 0) -> torch.Tensor:
    """K-permuted MFMA image of weight[:, col0:col0+128] for lgcn_att_pairs_wi (lgcn_pack_weight_kperm); cached on the
    parameter like packed() (rebuilt on first use after the parameter changed)."""
    lib = L.load()
    mma = _mma

    def make():
        w = _dev(weight.detach(), torch.float32, "weight")
        out = torch.empty(lib.lgcn_packed_bytes(C_FEAT, mma) // 4, dtype=torch.float32, device=w.device)
        L.check(lib.lgcn_pack_weight_kperm(C.c_void_p(w[:, col0:].data_ptr()), w.stride(0), mma, _ptr(out), _stream()),
                "lgcn_pack_weight_kperm")
        return out

    return _cached(weight, ("packK", col0, mma), make)


def att_pairs(ps: PairSet, wd0, bd0, wpd2, gn_d, wpc0e, U, V, gn_c, m=None, eps=EPS, seg=0, tag="att_pairs"):
    """m [cap,128] of lgcn_att_pairs / lgcn_att_pairs_ws / lgcn_att_pairs_wi.  seg = 16 (ws / wi): per-target sums of
    16-aligned pieces at each piece's first row; hand m to agg_mlp as a REL_RANGE16 relation.
    wpd2 / wpc0e: (weight parameter, first column) -- packed here in the layout of the kernel in use -- or, for the ws /
    stream kernels, an image already made by packed()."""
    lib = L.load()
    impl = att_pairs_impl()
    if isinstance(wpd2, tuple) != isinstance(wpc0e, tuple):
        raise L.LgcnError("att_pairs: both weights as (parameter, column) or both packed")
    if isinstance(wpd2, tuple):
        pk = packed_kperm if impl == "wi" else (lambda w, c: packed(w, c, C_FEAT))
        wpd2, wpc0e = pk(*wpd2), pk(*wpc0e)
    elif impl == "wi":
        impl = "ws"          # images made by packed(): the kernels that read that layout
    if m is None:
        m = torch.empty((max(ps.cap, 1), C_FEAT), dtype=torch.float32, device=U.device)
    args = (_ptr(ps.agt_ctrs), _ptr(ps.ctx_ctrs), _ptr(ps.hi), _ptr(ps.wi), _ptr(ps.n_pairs),
            ps.cap, _ptr(wd0), _ptr(bd0), _ptr(wpd2), _ptr(gn_d[0]), _ptr(gn_d[1]), _ptr(wpc0e),
            _ptr(U), _ptr(V), _ptr(gn_c[0]), _ptr(gn_c[1]), eps, _mma)
    with _Timed(tag):
        if impl == "wi":
            rc = lib.lgcn_att_pairs_wi(*args, seg, _ptr(m), _stream())
        elif impl == "ws":
            rc = lib.lgcn_att_pairs_ws(*args, seg, _ptr(m), _stream())
        elif seg != 0:
            raise L.LgcnError("att_pairs: seg needs the weight-stationary kernel (16-bit-plane modes)")
        else:
            rc = lib.lgcn_att_pairs(*args, _ptr(m), _stream())
    L.check(rc, "lgcn_att_pairs")
    return m


# ------------------------------------------------------------------ Att's pair stage, training (exact fp32)
PAIR_MASK_WORDS = 12       # per pair: 3 masks x 4 words of 32 channels


def att_pairs_train(ps: PairSet, wd0, bd0, w_d2, gn_d, w_c0, U, V, gn_c, m=None, masks=None, eps=EPS, tag="att_pairs_train"):
    """(m [cap,128], masks [cap,12] int32) of lgcn_att_pairs_train: the pair MLP of lgcn_att_pairs in exact fp32 plus its
    three ReLU masks as bits (att_pair_masks decodes them).  w_d2 [128,128] and w_c0 [128,384] are the parameters; their
    F32 images are made here.  Rows >= *n_pairs of m / masks are not written."""
    lib = L.load()
    U, V = _dev(U, torch.float32, "U"), _dev(V, torch.float32, "V")
    with exact_mma():
        wpd2, wpc0e = packed(w_d2, 0, C_FEAT), packed(w_c0, 0, C_FEAT)
    rows = max(ps.cap, 1)
    if m is None:
        m = torch.empty((rows, C_FEAT), dtype=torch.float32, device=U.device)
    if masks is None:
        masks = torch.empty((rows, PAIR_MASK_WORDS), dtype=torch.int32, device=U.device)
    with _Timed(tag):
        rc = lib.lgcn_att_pairs_train(_ptr(ps.agt_ctrs), _ptr(ps.ctx_ctrs), _ptr(ps.hi), _ptr(ps.wi), _ptr(ps.n_pairs), ps.cap,
                                      _ptr(wd0), _ptr(bd0), _ptr(wpd2), _ptr(gn_d[0]), _ptr(gn_d[1]), _ptr(wpc0e), _ptr(U),
                                      _ptr(V), _ptr(gn_c[0]), _ptr(gn_c[1]), eps, _ptr(m), _ptr(masks), _stream())
    L.check(rc, "lgcn_att_pairs_train")
    return m, masks


def _pool_args(what, ps, ctx_pose, tgt_pose, wp, bp, w_c0, U):
    ctx_pose, tgt_pose = _dev(ctx_pose, torch.float32, "ctx_pose"), _dev(tgt_pose, torch.float32, "tgt_pose")
    U = _dev(U, torch.float32, "U")
    if ctx_pose.dim() != 2 or ctx_pose.shape[1] != 4 or tgt_pose.dim() != 2 or tgt_pose.shape[1] != 4:
        raise L.LgcnError(what + ": poses must be [rows, 4]")
    if U.shape != (ctx_pose.shape[0], C_FEAT):
        raise L.LgcnError(what + ": U must be [context rows, 128]")
    if tuple(w_c0.shape) != (C_FEAT, 2 * C_FEAT) or tuple(wp.shape) != (C_FEAT, 4):
        raise L.LgcnError(what + ": need relpose.0 [128,4] and ctx.0 [128,256] weights")
    return ctx_pose, tgt_pose, _dev(wp.detach(), torch.float32, "wp"), _dev(bp.detach(), torch.float32, "bp"), U


def _row_buf(buf, rows, cols, dtype, device, err, min_rows=0):
    """A caller's output buffer of at least `rows` rows, checked (err: the message of a misfit), or a new one."""
    if buf is None:
        return torch.empty((max(rows, min_rows), cols), dtype=dtype, device=device)
    if buf.shape[0] < rows or not buf.is_contiguous() or buf.dtype != dtype or not buf.is_cuda:
        raise L.LgcnError(err)
    return buf


def _bwd_chunks(n_chunks, rows, cap, dev):
    """Workgroups of a fused backward launch.  Default: one per CU, never more than a quarter of the 32-row tiles of `rows`
    (a workgroup then walks at least four); always within what `cap` rows and the library allow."""
    if n_chunks is None:
        n_chunks = min(cu_count(dev), (rows + 127) // 128)
    return max(1, min(int(n_chunks), (cap + 31) // 32, 1024))


def _bwd_ws(fn, what, *args, dev):
    """The workspace of a fused backward's chunk records.  fn: the library's *_ws_elems, called with args = (rows,
    n_chunks, ...); what: "<op>: <name of the row count>", for the error."""
    n_ws = fn(*args)
    if n_ws < 0:
        raise L.LgcnError("%s = %d / n_chunks = %d not supported" % (what, args[0], args[1]))
    return torch.empty(max(n_ws, 1), dtype=torch.float32, device=dev)


def _pair_masks(masks, P, k):
    """bool [P,k,128] of the first P rows of a pair kernel's k masks of 4 words each (att_pair_masks, pool_pair_masks)."""
    w = masks[:P].reshape(P, k, 4, 1).to(torch.int64) & 0xFFFFFFFF
    bits = (w >> torch.arange(32, device=masks.device)) & 1
    return bits.reshape(P, k, C_FEAT).bool()


def pool_pairs(ps: PairSet, ctx_pose, tgt_pose, wp, bp, w_c0, U, gn, m=None, cap=None, eps=EPS, tag="pool_pairs"):
    """m [cap,128] of lgcn_pool_pairs: the pair stage of the fork's LanePooling (reference lanercnn.py:492-499) in one
    launch, exact fp32 in every matrix mode.  ps: pairs with hi = target row, wi = context row; ctx_pose [C,4], tgt_pose
    [T,4]; wp [128,4] / bp [128]: relpose.0; w_c0 [128,256]: ctx.0's Linear weight (the F32 image of its columns 128:256
    is made here); U [C,128] = context_feat w_c0[:, 0:128]^T; gn = (weight, bias) of ctx.0's norm.  cap: rows of m the
    launch may write (default: the pair search's capacity; a caller that knows P passes it and gets a [P,128] m).  Rows
    >= *n_pairs of m are not written."""
    lib = L.load()
    ctx_pose, tgt_pose, wp, bp, U = _pool_args("pool_pairs", ps, ctx_pose, tgt_pose, wp, bp, w_c0, U)
    with exact_mma():
        wpc0h = packed(w_c0, C_FEAT, C_FEAT)
    cap = ps.cap if cap is None else min(int(cap), ps.cap)
    if m is None:
        m = torch.empty((max(cap, 1), C_FEAT), dtype=torch.float32, device=U.device)
    elif m.shape[0] < cap or not m.is_contiguous():
        raise L.LgcnError("pool_pairs: m must be a contiguous [>= cap, 128] tensor")
    with _Timed(tag):
        rc = lib.lgcn_pool_pairs(_ptr(ctx_pose), _ptr(tgt_pose), _ptr(ps.hi), _ptr(ps.wi), _ptr(ps.n_pairs), cap,
                                 _ptr(wp), _ptr(bp), _ptr(wpc0h), _ptr(U), _ptr(gn[0]), _ptr(gn[1]), eps, _ptr(m),
                                 _stream())
    L.check(rc, "lgcn_pool_pairs")
    return m


# ------------------------------------------------------------------ LanePooling's pair stage, training (exact fp32)
POOL_MASK_WORDS = 8        # per pair: 2 masks x 4 words of 32 channels


def pool_pairs_train(ps: PairSet, ctx_pose, tgt_pose, wp, bp, w_c0, U, gn, m=None, masks=None, cap=None, eps=EPS,
                     tag="pool_pairs_train"):
    """(m [cap,128], masks [cap,8] int32) of lgcn_pool_pairs_train: pool_pairs (same arguments, same bits of m) plus the
    two ReLU masks as bits (pool_pair_masks decodes them).  Rows >= *n_pairs of m / masks are not written."""
    lib = L.load()
    ctx_pose, tgt_pose, wp, bp, U = _pool_args("pool_pairs_train", ps, ctx_pose, tgt_pose, wp, bp, w_c0, U)
    with exact_mma():
        wpc0h = packed(w_c0, C_FEAT, C_FEAT)
    cap = ps.cap if cap is None else min(int(cap), ps.cap)
    err = "pool_pairs_train: %s must be a contiguous [>= cap, %d] tensor"
    m = _row_buf(m, cap, C_FEAT, torch.float32, U.device, err % ("m", C_FEAT), 1)
    masks = _row_buf(masks, cap, POOL_MASK_WORDS, torch.int32, U.device, err % ("masks", POOL_MASK_WORDS), 1)
    with _Timed(tag):
        rc = lib.lgcn_pool_pairs_train(_ptr(ctx_pose), _ptr(tgt_pose), _ptr(ps.hi), _ptr(ps.wi), _ptr(ps.n_pairs), cap,
                                       _ptr(wp), _ptr(bp), _ptr(wpc0h), _ptr(U), _ptr(gn[0]), _ptr(gn[1]), eps, _ptr(m),
                                       _ptr(masks), _stream())
    L.check(rc, "lgcn_pool_pairs_train")
    return m, masks


def pool_pair_masks(masks: torch.Tensor, P: int) -> torch.Tensor:
    """bool [P,2,128] of the first P rows of pool_pairs_train's masks: [p, k, c] = mask k of channel c of pair p, k = 0:
    W_p d + b_p > 0, 1: m > 0.  Layout: word 4 k + j of a row holds channels 32 j .. 32 j + 31, bit b = channel 32 j + b."""
    return _pair_masks(masks, P, 2)


POOL_BWD_OUTS = ("d_w0h", "d_wp", "d_bp", "d_g", "d_bt")


def pool_pairs_bwd(ps: PairSet, dS, masks, ctx_pose, tgt_pose, wp, bp, w_c0, U, gn, want=POOL_BWD_OUTS, want_dz=True, dz=None,
                   cap=None, eps=EPS, n_chunks: Optional[int] = None, tag="pool_pairs_bwd"):
    """lgcn_pool_pairs_bwd for dS [T,128]: dict with "dz" ([cap,128], rows < P written; None unless want_dz) and the
    gradients named in `want` -- d_w0h [128,128] (the columns 128:256 of ctx.0's weight), d_wp [128,4], d_bp (relpose.0),
    d_g, d_bt (ctx.0's norm) [128].  cap: as in pool_pairs.  n_chunks: workgroups, each with one partial record of 69,120 B
    that the reduction launch reads back (default: the rule of att_pairs_bwd -- one per CU, never more than a quarter of
    the 32-pair tiles of the pair count when the host already knows it, else of the capacity)."""
    lib = L.load()
    dS = _dev(dS, torch.float32, "dS")
    ctx_pose, tgt_pose, wp, bp, U = _pool_args("pool_pairs_bwd", ps, ctx_pose, tgt_pose, wp, bp, w_c0, U)
    if dS.dim() != 2 or dS.shape != (tgt_pose.shape[0], C_FEAT):
        raise L.LgcnError("pool_pairs_bwd: dS must be [target rows, 128]")
    dev, want = dS.device, tuple(want)
    with exact_mma():
        wpc0h, wptc0h = packed(w_c0, C_FEAT, C_FEAT), packed_t(w_c0, C_FEAT)
    cap = ps.cap if cap is None else min(int(cap), ps.cap)
    if masks.shape[0] < cap or not masks.is_contiguous() or masks.dtype != torch.int32:
        raise L.LgcnError("pool_pairs_bwd: masks must be a contiguous int32 [>= cap, 8] tensor")
    n_chunks = _bwd_chunks(n_chunks, cap if ps._p_host is None else min(ps._p_host, cap), cap, dev)
    out = {"dz": None}
    q = L.PoolPairsBwd()
    q.ctx_pose, q.tgt_pose, q.ti, q.ci, q.n_pairs = (t.data_ptr() for t in (ctx_pose, tgt_pose, ps.hi, ps.wi, ps.n_pairs))
    q.cap = cap
    q.wp, q.bp, q.wpc0h, q.U, q.g, q.bt = (t.data_ptr() for t in (wp, bp, wpc0h, U, gn[0], gn[1]))
    q.wptc0h, q.masks, q.dS = wptc0h.data_ptr(), masks.data_ptr(), dS.data_ptr()
    if want_dz:
        out["dz"] = _row_buf(dz, cap, C_FEAT, torch.float32, dev, "pool_pairs_bwd: dz must be a contiguous [>= cap, 128] tensor", 1)
        q.dz = out["dz"].data_ptr()
    shapes = {"d_w0h": (C_FEAT, C_FEAT), "d_wp": (C_FEAT, 4)}
    for name in want:
        if name not in POOL_BWD_OUTS:
            raise L.LgcnError("pool_pairs_bwd: unknown output %r" % (name,))
        out[name] = torch.empty(shapes.get(name, (C_FEAT,)), dtype=torch.float32, device=dev)
        setattr(q, name, out[name].data_ptr())
    if want:
        ws = _bwd_ws(lib.lgcn_pool_pairs_bwd_ws_elems, "pool_pairs_bwd: cap", cap, n_chunks, dev=dev)
        q.ws = ws.data_ptr()
    q.eps, q.n_chunks = eps, n_chunks
    with _Timed(tag):
        rc = lib.lgcn_pool_pairs_bwd(C.byref(q), _stream())
    L.check(rc, "lgcn_pool_pairs_bwd")
    return out


def att_pair_masks(masks: torch.Tensor, P: int) -> torch.Tensor:
    """bool [P,3,128] of the first P rows of att_pairs_train's masks: [p, k, c] = mask k of channel c of pair p, k = 0:
    W_d0 d + b_d0 > 0, 1: e > 0, 2: m > 0.  Layout: word 4 k + j of a row holds channels 32 j .. 32 j + 31, bit b =
    channel 32 j + b."""
    return _pair_masks(masks, P, 3)


PAIR_BWD_OUTS = ("d_wd2", "d_wc0e", "d_wd0", "d_bd0", "d_gd", "d_btd", "d_gc", "d_btc")


def att_pairs_bwd(ps: PairSet, dS, masks, wd0, bd0, w_d2, gn_d, w_c0, U, V, gn_c, want=PAIR_BWD_OUTS, want_dc=True, dc=None,
                  eps=EPS, n_chunks: Optional[int] = None, tag="att_pairs_bwd"):
    """lgcn_att_pairs_bwd for dS [T,128]: dict with "dc" ([cap,128], rows < P written; None unless want_dc) and the
    gradients named in `want` -- d_wd2 [128,128], d_wc0e [128,128] (the columns 0:128 of ctx.0's weight), d_wd0 [128,2],
    d_bd0, d_gd, d_btd (dist.2's norm), d_gc, d_btc (ctx.0's norm) [128].  n_chunks: workgroups, each with one partial
    record of 134,656 B that the reduction launch reads back (default: one per CU, never more than a quarter of the
    32-pair tiles of the pair count when the host already knows it -- a workgroup then walks at least four tiles --
    else of the capacity)."""
    lib = L.load()
    dS, U, V = _dev(dS, torch.float32, "dS"), _dev(U, torch.float32, "U"), _dev(V, torch.float32, "V")
    dev, want = dS.device, tuple(want)
    with exact_mma():
        wpd2, wpc0e = packed(w_d2, 0, C_FEAT), packed(w_c0, 0, C_FEAT)
        wptd2, wptc0e = packed_t(w_d2, 0), packed_t(w_c0, 0)
    n_chunks = _bwd_chunks(n_chunks, ps.cap if ps._p_host is None else ps._p_host, ps.cap, dev)
    out = {"dc": None}
    q = L.AttPairsBwd()
    q.agt_ctrs, q.ctx_ctrs, q.hi, q.wi, q.n_pairs = (t.data_ptr() for t in (ps.agt_ctrs, ps.ctx_ctrs, ps.hi, ps.wi, ps.n_pairs))
    q.cap = ps.cap
    q.wd0, q.bd0, q.wpd2, q.gd, q.btd = (t.data_ptr() for t in (wd0, bd0, wpd2, gn_d[0], gn_d[1]))
    q.wpc0e, q.U, q.V, q.gc, q.btc = (t.data_ptr() for t in (wpc0e, U, V, gn_c[0], gn_c[1]))
    q.wptd2, q.wptc0e, q.masks, q.dS = wptd2.data_ptr(), wptc0e.data_ptr(), masks.data_ptr(), dS.data_ptr()
    if want_dc:
        out["dc"] = dc if dc is not None else torch.empty((max(ps.cap, 1), C_FEAT), dtype=torch.float32, device=dev)
        q.dc = out["dc"].data_ptr()
    shapes = {"d_wd2": (C_FEAT, C_FEAT), "d_wc0e": (C_FEAT, C_FEAT), "d_wd0": (C_FEAT, 2)}
    for name in want:
        out[name] = torch.empty(shapes.get(name, (C_FEAT,)), dtype=torch.float32, device=dev)
        setattr(q, name, out[name].data_ptr())
    if want:
        ws = _bwd_ws(lib.lgcn_att_pairs_bwd_ws_elems, "att_pairs_bwd: cap", ps.cap, n_chunks, dev=dev)
        q.ws = ws.data_ptr()
    q.eps, q.n_chunks = eps, n_chunks
    with _Timed(tag):
        rc = lib.lgcn_att_pairs_bwd(C.byref(q), _stream())
    L.check(rc, "lgcn_att_pairs_bwd")
    return out


def pred_loss_fwd(cls, reg, gt, has, cfg):
    """lgcn_pred_loss_fwd: (sums [2] fp32 = cls_loss, reg_loss; counts [2] int32 = num_cls, num_reg; sel [A] int32)."""
    lib = L.load()
    A, M = cls.shape
    T = reg.shape[2]
    dev = cls.device
    sums = torch.empty(2, dtype=torch.float32, device=dev)
    counts = torch.empty(2, dtype=torch.int32, device=dev)
    sel = torch.empty(max(A, 1), dtype=torch.int32, device=dev)
    L.check(lib.lgcn_pred_loss_fwd(_ptr(cls), _ptr(reg), _ptr(gt), _ptr(has), A, M, T, cfg["cls_th"], cfg["cls_ignore"], cfg["mgn"],
                                   cfg["cls_coef"], cfg["reg_coef"], _ptr(sums), _ptr(counts), _ptr(sel), _stream()), "lgcn_pred_loss_fwd")
    return sums, counts, sel


def pred_loss_bwd(cls, reg, gt, has, cfg, sel, g_cls, g_reg):
    lib = L.load()
    A, M = cls.shape
    T = reg.shape[2]
    dcls, dreg = torch.empty_like(cls), torch.empty_like(reg)
    L.check(lib.lgcn_pred_loss_bwd(_ptr(cls), _ptr(reg), _ptr(gt), _ptr(has), A, M, T, cfg["cls_coef"], cfg["reg_coef"], _ptr(sel),
                                   _ptr(g_cls), _ptr(g_reg), _ptr(dcls), _ptr(dreg), _stream()), "lgcn_pred_loss_bwd")
    return dcls, dreg


# ------------------------------------------------------------------ backward building blocks
def gn_fwd(x, gn=None, res=None, relu=False, eps=EPS):
    """out = [ReLU](GroupNorm(1,128)(x) [+ res]) as a stand-alone row kernel."""
    lib = L.load()
    x = _dev(x, torch.float32, "x")
    out = torch.empty_like(x)
    g, b = (gn[0], gn[1]) if gn is not None else (None, None)
    res = None if res is None else _dev(res, torch.float32, "res")
    L.check(lib.lgcn_gn_fwd(_ptr(x), _ptr(g), _ptr(b), _ptr(res), x.shape[0], eps, int(bool(relu)), _ptr(out), _stream()),
            "lgcn_gn_fwd")
    return out


def gn_cl(x, gamma, beta, eps=EPS, res=None, relu=False, res_up2=False):
    """out = [ReLU](GroupNorm(1 group over (C, L))(x) [+ res]) in one launch: ActorNet's conv norms.
    x: [n, C, L] contiguous, or [n, C, 1, L] in torch.channels_last (memory [n, L, C]: the layout MIOpen's
    convolutions take without transposes); out has x's shape and layout.  res_up2: res is at half length and is
    upsampled x2 (linear, align_corners=False) on the fly (FPN top-down step)."""
    lib = L.load()
    if not x.is_cuda or x.dtype != torch.float32:
        raise L.LgcnError("gn_cl: x must be a float32 CUDA tensor")
    cl = x.dim() == 4
    if cl:
        if x.shape[2] != 1 or not x.is_contiguous(memory_format=torch.channels_last):
            raise L.LgcnError("gn_cl: 4-D input must be [n, C, 1, L] in channels_last")
        n, C_, L_ = x.shape[0], x.shape[1], x.shape[3]
    elif x.dim() == 3:
        x = x.contiguous()
        n, C_, L_ = x.shape
    else:
        raise L.LgcnError("gn_cl: x must be [n, C, L] or [n, C, 1, L]")
    if res is not None:
        want = list(x.shape)
        if res_up2:
            want[-1] //= 2
        if list(res.shape) != want or (res_up2 and L_ % 2) or not res.is_cuda or res.dtype != torch.float32:
            raise L.LgcnError("gn_cl: res has shape %s, expected %s" % (tuple(res.shape), tuple(want)))
        if cl and not res.is_contiguous(memory_format=torch.channels_last):
            raise L.LgcnError("gn_cl: res must be channels_last like x")
        if not cl:
            res = res.contiguous()
    out = torch.empty_like(x)
    gamma, beta = _dev(gamma.detach(), torch.float32, "gamma"), _dev(beta.detach(), torch.float32, "beta")
    L.check(lib.lgcn_gn_cl(_ptr(x), n, C_, L_, _ptr(gamma), _ptr(beta), float(eps), _ptr(res),
                           int(bool(res_up2 and res is not None)), int(bool(relu)), int(cl), _ptr(out), _stream()),
            "lgcn_gn_cl")
    return out


def gn_cl_bwd(dy, x, post, gamma, eps=EPS, want_g=False):
    """Backward of gn_cl on [n, C, L]: (dx, g | None, dgamma, dbeta); post = forward output when it applied a ReLU."""
    lib = L.load()
    dy, x = _dev(dy, torch.float32, "dy").contiguous(), _dev(x, torch.float32, "x").contiguous()
    n, C_, L_ = x.shape
    post = None if post is None else _dev(post, torch.float32, "post").contiguous()
    gamma = _dev(gamma.detach(), torch.float32, "gamma")
    dx = torch.empty_like(x)
    g = torch.empty_like(x) if want_g else None
    part = torch.empty((n, 2, C_), dtype=torch.float32, device=x.device)
    L.check(lib.lgcn_gn_cl_bwd(_ptr(dy), _ptr(x), _ptr(post), _ptr(gamma), n, C_, L_, float(eps), _ptr(dx), _ptr(g),
                               _ptr(part), _stream()), "lgcn_gn_cl_bwd")
    sums = part.sum(0)
    return dx, g, sums[0], sums[1]


def gn_bwd(dy, x, post, gamma, eps=EPS, want_g=False):
    """Backward of out = [ReLU](GN(x) [+res]): returns (dx, g, dgamma, dbeta); g = dy masked by post > 0
    (the gradient into `res`), None unless want_g.  gamma None: mask only."""
    lib = L.load()
    dy = _dev(dy, torch.float32, "dy")
    n = dy.shape[0]
    dx = torch.empty_like(dy)
    g = torch.empty_like(dy) if want_g else None
    if gamma is None:
        L.check(lib.lgcn_gn_bwd(_ptr(dy), None, _ptr(post), None, n, eps, _ptr(dx), _ptr(g), None, None, None, _stream()),
                "lgcn_gn_bwd")
        return dx, g, None, None
    x = _dev(x, torch.float32, "x")
    dgamma = torch.empty(C_FEAT, dtype=torch.float32, device=dy.device)
    dbeta = torch.empty_like(dgamma)
    part = torch.empty(2 * ((n + 31) // 32) * C_FEAT, dtype=torch.float32, device=dy.device)
    L.check(lib.lgcn_gn_bwd(_ptr(dy), _ptr(x), _ptr(post), _ptr(gamma), n, eps, _ptr(dx), _ptr(g), _ptr(dgamma),
                            _ptr(dbeta), _ptr(part), _stream()), "lgcn_gn_bwd")
    return dx, g, dgamma, dbeta


def wgrad(n_rows: int, rels: Sequence[RelSpec], dT: torch.Tensor, *, rowptr=None, col=None, n_rel_csr=0,
          n_chunks: Optional[int] = None) -> torch.Tensor:
    """dW[r] = dT^T (G_r src_r) for every relation: [n_rel,128,128] fp32.  The rows are cut into n_chunks
    partial sums per relation (default: ~512 workgroups in all, two per CU; a single-relation launch over the
    67 k pairs of A2A took 557 us on 16 workgroups)."""
    lib = L.load()
    dT = _dev(dT, torch.float32, "dT")
    p = L.AggMlp()
    p.n_rows, p.n_rel, p.n_rel_csr = n_rows, len(rels), n_rel_csr
    keep = []
    for i, r in enumerate(rels):
        s = _dev(r.src, torch.float32, "rel.src")
        keep.append(s)
        p.rel[i].src, p.rel[i].mode, p.rel[i].ridx = s.data_ptr(), r.mode, r.ridx
    p.rowptr = 0 if rowptr is None else rowptr.data_ptr()
    p.col = 0 if col is None else col.data_ptr()
    if n_chunks is None:
        n_chunks = max(1, 512 // len(rels))
    n_chunks = max(1, min(n_chunks, (n_rows + 31) // 32, 1024))
    dW = torch.empty((len(rels), C_FEAT, C_FEAT), dtype=torch.float32, device=dT.device)
    part = torch.empty(len(rels) * n_chunks * C_FEAT * C_FEAT, dtype=torch.float32, device=dT.device)
    L.check(lib.lgcn_wgrad(C.byref(p), _ptr(dT), _ptr(dW), _ptr(part), n_chunks, _stream()), "lgcn_wgrad")
    return dW


LC_BWD_OUTS = ("d_w2", "d_g2", "d_b2", "d_g1", "d_b1")      # with x / w1 (one IDENT relation) also "d_w1"


def laneconv_bwd(d_out, out, Z, Y, T, gn1_w, w2, gn2_w, *, x=None, w1=None, want=None, want_dx=True, dT=None, g2=None,
                 n_chunks: Optional[int] = None, eps=EPS, tag="laneconv_bwd"):
    """lgcn_laneconv_bwd for d_out [N,128] and the tensors LaneConvFn's forward saved (exact fp32 in every matrix mode):
    dict with the gradients named in `want` -- d_w2 [128,128], d_g2, d_b2 (the second norm), d_g1, d_b1 (the first) [128]
    -- and
      without x / w1: "dT" [N,128] and "g2" [N,128] (None unless want_dx), the inputs of the relation stage's backward;
      with x and w1 (T = x w1^T, a LinearRes): "dX" [N,128] (None unless want_dx) and, when wanted, d_w1 [128,128].
    w2 / w1 are the parameters; their transposed F32 images are made here.  dT / g2: preallocated outputs, at least N rows.
    n_chunks: workgroups, each with one partial record that the reduction launch reads back (default: one per CU, never
    more than a quarter of the 32-row tiles -- a workgroup then walks at least four)."""
    lib = L.load()
    ident1 = x is not None
    if ident1 != (w1 is not None):
        raise L.LgcnError("laneconv_bwd: x and w1 come together")
    d_out = _dev(d_out, torch.float32, "d_out")
    out, Z, Y, T = (_dev(t, torch.float32, n) for t, n in ((out, "out"), (Z, "Z"), (Y, "Y"), (T, "T")))
    N, dev = d_out.shape[0], d_out.device
    want = (LC_BWD_OUTS + (("d_w1",) if ident1 else ())) if want is None else tuple(want)
    if not ident1 and "d_w1" in want:
        raise L.LgcnError("laneconv_bwd: d_w1 needs x and w1")
    q = L.LaneConvBwd()
    q.d_out, q.out, q.Z, q.Y, q.T = (t.data_ptr() for t in (d_out, out, Z, Y, T))
    q.gamma1, q.gamma2 = gn1_w.data_ptr(), gn2_w.data_ptr()
    with exact_mma():
        wpt2 = packed_t(w2)
        wpt1 = packed_t(w1) if ident1 else None
    q.wpt2 = wpt2.data_ptr()
    res = {}
    if ident1:
        x = _dev(x, torch.float32, "x")
        q.X, q.wpt1 = x.data_ptr(), wpt1.data_ptr()
        res["dX"] = torch.empty((N, C_FEAT), dtype=torch.float32, device=dev) if want_dx else None
        q.dX = 0 if res["dX"] is None else res["dX"].data_ptr()
    else:
        for name, buf, on in (("dT", dT, True), ("g2", g2, want_dx)):
            err = "laneconv_bwd: %s must be a contiguous float32 [>= %d, 128]" % (name, N)
            res[name] = _row_buf(buf, N, C_FEAT, torch.float32, dev, err) if on else None
            setattr(q, name, 0 if res[name] is None else res[name].data_ptr())
    for name in want:
        res[name] = torch.empty((C_FEAT, C_FEAT) if name in ("d_w2", "d_w1") else (C_FEAT,), dtype=torch.float32, device=dev)
        setattr(q, name, res[name].data_ptr())
    n_chunks = _bwd_chunks(n_chunks, N, N, dev)
    if want:
        ws = _bwd_ws(lib.lgcn_laneconv_bwd_ws_elems, "laneconv_bwd: n_rows", N, n_chunks, int(ident1), dev=dev)
        q.ws = ws.data_ptr()
    q.n_rows, q.eps, q.n_chunks, q.ident1 = N, eps, n_chunks, int(ident1)
    with _Timed(tag):
        rc = lib.lgcn_laneconv_bwd(C.byref(q), _stream())
    L.check(rc, "lgcn_laneconv_bwd")
    return res


def rowblock_bwd(d_out, out, pre, gn_w, rels, *, want_src=None, want_w=None, want_gn=True, want_res=False, d_src=None,
                 d_res=None, n_chunks: Optional[int] = None, eps=EPS, tag="rowblock_bwd"):
    """lgcn_rowblock_bwd: the whole backward of out = [ReLU]([GN](sum_r src_r W_r[:, col0_r:col0_r+128]^T) [+ res]) with
    one or two IDENT relations, for d_out [N,128], in one launch pair (exact fp32 in every matrix mode).
      out:  the block's output when it had a ReLU, else None;  pre / gn_w: the saved pre-normalisation tensor and the
            GroupNorm weight when it had a norm, else both None
      rels: [(src [N,128], weight [128,K], col0)], K and col0 multiples of 4; the weights are the parameters, their
            transposed F32 images are made here
      want_src / want_w: one flag per relation (default: all); want_gn: dgamma / dbeta (ignored without a norm);
      want_res: g = d_out * (out > 0) as the gradient of the residual
      d_src / d_res: preallocated outputs (a list with None for the absent ones / a tensor), at least N rows
    Returns a dict: "d_src" (list per relation, None where not wanted), "d_w" (list per distinct weight, in order of first
    appearance in rels: a tensor shaped like the weight, zero outside the relations' column blocks, or None when none of
    its relations wants it), "w_index" (per relation: its weight's place in "d_w"), "d_gamma", "d_beta", "d_res".
    n_chunks: workgroups, each with one partial record that the reduction launch reads back (default as laneconv_bwd)."""
    lib = L.load()
    n_rel = len(rels)
    if n_rel < 1 or n_rel > 2:
        raise L.LgcnError("rowblock_bwd: one or two relations, got %d" % n_rel)
    if (pre is None) != (gn_w is None):
        raise L.LgcnError("rowblock_bwd: pre and gn_w come together")
    d_out = _dev(d_out, torch.float32, "d_out")
    N, dev = d_out.shape[0], d_out.device
    want_src = [True] * n_rel if want_src is None else [bool(f) for f in want_src]
    want_w = [True] * n_rel if want_w is None else [bool(f) for f in want_w]
    want_gn = bool(want_gn) and pre is not None
    q = L.RowBlockBwd()
    q.d_out = d_out.data_ptr()
    keep = [d_out]
    if out is not None:
        out = _dev(out, torch.float32, "out")
        q.out = out.data_ptr()
    if pre is not None:
        pre = _dev(pre, torch.float32, "pre")
        q.pre, q.gamma = pre.data_ptr(), gn_w.data_ptr()
    ws_of, w_index = [], []           # distinct weights, by identity
    for r, (src, w, col0) in enumerate(rels):
        if w.dim() != 2 or w.shape[0] != C_FEAT or col0 < 0 or col0 + C_FEAT > w.shape[1] or w.shape[1] % 4 or col0 % 4:
            raise L.LgcnError("rowblock_bwd: relation %d needs a [128, K] weight with col0 + 128 <= K, K and col0 multiples of 4" % r)
        src = _dev(src, torch.float32, "src")
        keep.append(src)
        with exact_mma():
            wpt = packed_t(w, col0)
        keep.append(wpt)
        q.src[r], q.wpt[r] = src.data_ptr(), wpt.data_ptr()
        k = next((i for i, t in enumerate(ws_of) if t is w), None)
        if k is None:
            k = len(ws_of)
            ws_of.append(w)
        w_index.append(k)
    res = {"d_src": [None] * n_rel, "d_w": [None] * len(ws_of), "w_index": w_index, "d_gamma": None, "d_beta": None,
           "d_res": None}
    rows = lambda buf, name: _row_buf(buf, N, C_FEAT, torch.float32, dev,
                                      "rowblock_bwd: %s must be a contiguous float32 [>= %d, 128]" % (name, N))
    for r in range(n_rel):
        if want_src[r]:
            res["d_src"][r] = rows(None if d_src is None else d_src[r], "d_src[%d]" % r)
            q.d_src[r] = res["d_src"][r].data_ptr()
    if want_res:
        res["d_res"] = rows(d_res, "d_res")
        q.d_res = res["d_res"].data_ptr()
    for k, w in enumerate(ws_of):
        cols = sorted(rels[r][2] for r in range(n_rel) if w_index[r] == k and want_w[r])
        if not cols:
            continue
        if len(cols) == 2 and cols[1] - cols[0] < C_FEAT:
            raise L.LgcnError("rowblock_bwd: two relations on overlapping column blocks of one weight")
        K = w.shape[1]
        full = cols[0] == 0 and all(b - a == C_FEAT for a, b in zip(cols, cols[1:])) and cols[-1] + C_FEAT == K
        res["d_w"][k] = (torch.empty if full else torch.zeros)((C_FEAT, K), dtype=torch.float32, device=dev)
    for r in range(n_rel):
        if want_w[r]:
            g = res["d_w"][w_index[r]]
            q.d_w[r], q.ld_w[r] = g.data_ptr() + 4 * rels[r][2], g.shape[1]
    if want_gn:
        res["d_gamma"] = torch.empty(C_FEAT, dtype=torch.float32, device=dev)
        res["d_beta"] = torch.empty(C_FEAT, dtype=torch.float32, device=dev)
        q.d_gamma, q.d_beta = res["d_gamma"].data_ptr(), res["d_beta"].data_ptr()
    n_chunks = _bwd_chunks(n_chunks, N, N, dev)
    if want_gn or any(want_w):
        ws = _bwd_ws(lib.lgcn_rowblock_bwd_ws_elems, "rowblock_bwd: n_rows", N, n_chunks, n_rel, dev=dev)
        keep.append(ws)
        q.ws = ws.data_ptr()
    q.n_rows, q.eps, q.n_rel, q.n_chunks = N, eps, n_rel, n_chunks
    with _Timed(tag):
        rc = lib.lgcn_rowblock_bwd(C.byref(q), _stream())
    L.check(rc, "lgcn_rowblock_bwd")
    return res


def gather_rows(src, idx, n_dev, cap):
    lib = L.load()
    src = _dev(src, torch.float32, "src")
    out = torch.empty((max(cap, 1), C_FEAT), dtype=torch.float32, device=src.device)
    L.check(lib.lgcn_gather_rows(_ptr(src), _ptr(idx), _ptr(n_dev), cap, _ptr(out), _stream()), "lgcn_gather_rows")
    return out[:cap]


def gather_sum(src, rowptr, col, n_rows):
    lib = L.load()
    src = _dev(src, torch.float32, "src")
    out = torch.empty((n_rows, C_FEAT), dtype=torch.float32, device=src.device)
    L.check(lib.lgcn_gather_sum(_ptr(src), _ptr(rowptr), _ptr(col), n_rows, _ptr(out), _stream()), "lgcn_gather_sum")
    return out


def pair_add(c, U, hi, V, wi, n_dev, cap):
    lib = L.load()
    c = _dev(c, torch.float32, "c")
    out = torch.empty_like(c)
    L.check(lib.lgcn_pair_add(_ptr(c), _ptr(U), _ptr(hi), _ptr(V), _ptr(wi), _ptr(n_dev), cap, _ptr(out), _stream()),
            "lgcn_pair_add")
    return out


# ------------------------------------------------------------------ goal decoder of the fork model (lanercnn.py:683-924)
GOAL_MAX_MODS, GOAL_STEPS = 8, 30


def _offsets(spans, name):
    """Host span table [0, n_0, n_0 + n_1, ...] as (CPU int32 tensor, plain ints)."""
    off = [int(v) for v in spans]
    if len(off) < 1 or off[0] != 0 or any(b < a for a, b in zip(off, off[1:])):
        raise L.LgcnError("%s must start at 0 and ascend, got %s" % (name, off[:8]))
    return torch.tensor(off, dtype=torch.int32), off


def nms_select_segments(xys: torch.Tensor, logits: torch.Tensor, seg_off, threshold: float = 2.0, min_len: int = 6,
                        max_keep: int = 0):
    """Segmented greedy NMS (lgcn_nms_select): seg_off = host span table of the segments (RoIs) or an int32 CUDA tensor.
    Returns (idx [n] int32 segment-local, -1 past the count, count [n_seg] int32), both on the device."""
    lib = L.load()
    xys = _dev(xys, torch.float32, "xys")
    logits = _dev(logits, torch.float32, "logits")
    n = logits.shape[0]
    if xys.dim() != 2 or xys.shape[1] != 2 or xys.shape[0] != n or logits.dim() != 1:
        raise L.LgcnError("nms_select_segments: xys [n, 2] and logits [n] expected, got %s and %s"
                          % (tuple(xys.shape), tuple(logits.shape)))
    if torch.is_tensor(seg_off) and seg_off.is_cuda:
        seg_dev = _dev(seg_off, torch.int32, "seg_off")
    else:
        host, off = _offsets(seg_off, "seg_off")
        if off[-1] > n:
            raise L.LgcnError("nms_select_segments: seg_off ends at %d, past the %d rows" % (off[-1], n))
        seg_dev = host.to(xys.device, non_blocking=True)
    n_seg = seg_dev.shape[0] - 1
    if n_seg < 0:
        raise L.LgcnError("nms_select_segments: seg_off needs at least one entry")
    idx = torch.full((n,), -1, dtype=torch.int32, device=xys.device)
    count = torch.zeros((n_seg,), dtype=torch.int32, device=xys.device)
    L.check(lib.lgcn_nms_select(_ptr(xys), _ptr(logits), _ptr(seg_dev), n, n_seg, float(threshold), int(min_len),
                                int(max_keep), _ptr(idx), _ptr(count), _stream()), "lgcn_nms_select")
    return idx, count


def goal_decode(pred: torch.Tensor, pred_spans, anc_ctrs: torch.Tensor, anc_dirs: torch.Tensor, anc_first,
                agt_ctrs: torch.Tensor, agt_dir_last: torch.Tensor, agt_vel: torch.Tensor, k: int = 6, threshold: float = 2.0):
    """lgcn_goal_decode: pred [n, 5] with the host span table pred_spans [n_agt + 1]; anc_first = host list of the first
    anchor row of each interest RoI.  Returns (top_idx [A, k] int32, goals [A, k, 2], logits [A, k], coef [A, k, 6],
    s_samples [A, k, 30])."""
    lib = L.load()
    pred = _dev(pred, torch.float32, "pred")
    anc_ctrs = _dev(anc_ctrs, torch.float32, "anc_ctrs")
    anc_dirs = _dev(anc_dirs, torch.float32, "anc_dirs")
    agt_ctrs = _dev(agt_ctrs, torch.float32, "agt_ctrs")
    agt_dir_last = _dev(agt_dir_last, torch.float32, "agt_dir_last")
    agt_vel = _dev(agt_vel, torch.float32, "agt_vel")
    off_host, off = _offsets(pred_spans, "pred_spans")
    A_ = len(off) - 1
    if pred.dim() != 2 or pred.shape[1] != 5 or off[-1] != pred.shape[0]:
        raise L.LgcnError("goal_decode: pred [n, 5] covered by pred_spans expected, got %s and a table ending at %d"
                          % (tuple(pred.shape), off[-1]))
    if anc_ctrs.dim() != 2 or anc_ctrs.shape[1] != 2 or anc_dirs.shape != anc_ctrs.shape:
        raise L.LgcnError("goal_decode: anc_ctrs / anc_dirs [N, 2] expected")
    if tuple(agt_ctrs.shape) != (A_, 2) or tuple(agt_dir_last.shape) != (A_, 2) or tuple(agt_vel.shape) != (A_,):
        raise L.LgcnError("goal_decode: agt_ctrs [A, 2], agt_dir_last [A, 2], agt_vel [A] expected for A = %d" % A_)
    first_host = torch.tensor([int(v) for v in anc_first], dtype=torch.int32)
    if first_host.shape[0] != A_:
        raise L.LgcnError("goal_decode: %d anchor offsets for %d agents" % (first_host.shape[0], A_))
    dev = pred.device
    off_dev, first_dev = off_host.to(dev, non_blocking=True), first_host.to(dev, non_blocking=True)
    top = torch.empty((A_, k), dtype=torch.int32, device=dev)
    goals = torch.empty((A_, k, 2), dtype=torch.float32, device=dev)
    logits = torch.empty((A_, k), dtype=torch.float32, device=dev)
    coef = torch.empty((A_, k, 6), dtype=torch.float32, device=dev)
    ss = torch.empty((A_, k, GOAL_STEPS), dtype=torch.float32, device=dev)
    L.check(lib.lgcn_goal_decode(_ptr(pred), _ptr(off_dev), C.c_void_p(off_host.data_ptr()), pred.shape[0],
                                 _ptr(anc_ctrs), _ptr(anc_dirs), anc_ctrs.shape[0], _ptr(first_dev),
                                 C.c_void_p(first_host.data_ptr()), _ptr(agt_ctrs), _ptr(agt_dir_last), _ptr(agt_vel),
                                 A_, int(k), float(threshold), _ptr(top), _ptr(goals), _ptr(logits), _ptr(coef), _ptr(ss),
                                 _stream()), "lgcn_goal_decode")
    return top, goals, logits, coef, ss


def goal_refine(s_samples: torch.Tensor, coef: torch.Tensor, traj_delta: torch.Tensor) -> torch.Tensor:
    """lgcn_goal_refine: s_samples [A, k, 30], coef [A, k, 6], traj_delta [A, k, 30, 2] -> pred_trajs [A, k, 30, 2]."""
    lib = L.load()
    s_samples = _dev(s_samples, torch.float32, "s_samples")
    coef = _dev(coef, torch.float32, "coef")
    traj_delta = _dev(traj_delta, torch.float32, "traj_delta")
    if s_samples.dim() != 3 or s_samples.shape[2] != GOAL_STEPS:
        raise L.LgcnError("goal_refine: s_samples [A, k, 30] expected, got %s" % (tuple(s_samples.shape),))
    A_, k = s_samples.shape[:2]
    if tuple(coef.shape) != (A_, k, 6) or tuple(traj_delta.shape) != (A_, k, GOAL_STEPS, 2):
        raise L.LgcnError("goal_refine: coef [A, k, 6] and traj_delta [A, k, 30, 2] expected, got %s and %s"
                          % (tuple(coef.shape), tuple(traj_delta.shape)))
    out = torch.empty_like(traj_delta)
    L.check(lib.lgcn_goal_refine(_ptr(s_samples), _ptr(coef), _ptr(traj_delta), A_ * k, _ptr(out), _stream()),
            "lgcn_goal_refine")
    return out


def goal_refine_bwd(s_samples: torch.Tensor, coef: torch.Tensor, traj_delta: torch.Tensor, d_pred_trajs: torch.Tensor):
    """lgcn_goal_refine_bwd: (d_s_samples [A, k, 30], d_coef [A, k, 6], d_traj_delta [A, k, 30, 2]) of goal_refine."""
    lib = L.load()
    s_samples = _dev(s_samples, torch.float32, "s_samples")
    coef = _dev(coef, torch.float32, "coef")
    traj_delta = _dev(traj_delta, torch.float32, "traj_delta")
    d_pred_trajs = _dev(d_pred_trajs, torch.float32, "d_pred_trajs")
    if s_samples.dim() != 3 or s_samples.shape[2] != GOAL_STEPS:
        raise L.LgcnError("goal_refine_bwd: s_samples [A, k, 30] expected, got %s" % (tuple(s_samples.shape),))
    A_, k = s_samples.shape[:2]
    if (tuple(coef.shape) != (A_, k, 6) or tuple(traj_delta.shape) != (A_, k, GOAL_STEPS, 2)
            or d_pred_trajs.shape != traj_delta.shape):
        raise L.LgcnError("goal_refine_bwd: coef [A, k, 6], traj_delta and d_pred_trajs [A, k, 30, 2] expected, got %s, %s, %s"
                          % (tuple(coef.shape), tuple(traj_delta.shape), tuple(d_pred_trajs.shape)))
    d_ss, d_coef, d_delta = torch.empty_like(s_samples), torch.empty_like(coef), torch.empty_like(traj_delta)
    L.check(lib.lgcn_goal_refine_bwd(_ptr(s_samples), _ptr(coef), _ptr(traj_delta), _ptr(d_pred_trajs), A_ * k, _ptr(d_ss),
                                     _ptr(d_coef), _ptr(d_delta), _stream()), "lgcn_goal_refine_bwd")
    return d_ss, d_coef, d_delta


def goal_decode_bwd(pred: torch.Tensor, pred_spans, anc_ctrs: torch.Tensor, anc_dirs: torch.Tensor, anc_first,
                    agt_ctrs: torch.Tensor, agt_dir_last: torch.Tensor, agt_vel: torch.Tensor, top_idx: torch.Tensor,
                    d_goals=None, d_logits=None, d_coef=None, d_s_samples=None) -> torch.Tensor:
    """lgcn_goal_decode_bwd: d_pred [n, 5] of goal_decode for its inputs, its top_idx [A, k] and the upstream gradients
    of goals [A, k, 2], logits [A, k], coef [A, k, 6] and s_samples [A, k, 30] (None = zero)."""
    lib = L.load()
    pred = _dev(pred, torch.float32, "pred")
    anc_ctrs = _dev(anc_ctrs, torch.float32, "anc_ctrs")
    anc_dirs = _dev(anc_dirs, torch.float32, "anc_dirs")
    agt_ctrs = _dev(agt_ctrs, torch.float32, "agt_ctrs")
    agt_dir_last = _dev(agt_dir_last, torch.float32, "agt_dir_last")
    agt_vel = _dev(agt_vel, torch.float32, "agt_vel")
    top_idx = _dev(top_idx, torch.int32, "top_idx")
    off_host, off = _offsets(pred_spans, "pred_spans")
    A_ = len(off) - 1
    if pred.dim() != 2 or pred.shape[1] != 5 or off[-1] != pred.shape[0]:
        raise L.LgcnError("goal_decode_bwd: pred [n, 5] covered by pred_spans expected, got %s and a table ending at %d"
                          % (tuple(pred.shape), off[-1]))
    if anc_ctrs.dim() != 2 or anc_ctrs.shape[1] != 2 or anc_dirs.shape != anc_ctrs.shape:
        raise L.LgcnError("goal_decode_bwd: anc_ctrs / anc_dirs [N, 2] expected")
    if tuple(agt_ctrs.shape) != (A_, 2) or tuple(agt_dir_last.shape) != (A_, 2) or tuple(agt_vel.shape) != (A_,):
        raise L.LgcnError("goal_decode_bwd: agt_ctrs [A, 2], agt_dir_last [A, 2], agt_vel [A] expected for A = %d" % A_)
    if top_idx.dim() != 2 or top_idx.shape[0] != A_ or not 1 <= top_idx.shape[1] <= GOAL_MAX_MODS:
        raise L.LgcnError("goal_decode_bwd: top_idx [A, k] with k in 1..8 expected, got %s" % (tuple(top_idx.shape),))
    k = top_idx.shape[1]
    first_host = torch.tensor([int(v) for v in anc_first], dtype=torch.int32)
    if first_host.shape[0] != A_:
        raise L.LgcnError("goal_decode_bwd: %d anchor offsets for %d agents" % (first_host.shape[0], A_))
    dev = pred.device
    ups = []
    for g, shape, name in ((d_goals, (A_, k, 2), "d_goals"), (d_logits, (A_, k), "d_logits"), (d_coef, (A_, k, 6), "d_coef"),
                           (d_s_samples, (A_, k, GOAL_STEPS), "d_s_samples")):
        if g is None:
            g = torch.zeros(shape, dtype=torch.float32, device=dev)
        g = _dev(g, torch.float32, name)
        if tuple(g.shape) != shape:
            raise L.LgcnError("goal_decode_bwd: %s %s expected, got %s" % (name, shape, tuple(g.shape)))
        ups.append(g)
    off_dev, first_dev = off_host.to(dev, non_blocking=True), first_host.to(dev, non_blocking=True)
    d_pred = torch.empty_like(pred)
    L.check(lib.lgcn_goal_decode_bwd(_ptr(pred), _ptr(off_dev), C.c_void_p(off_host.data_ptr()), pred.shape[0],
                                     _ptr(anc_ctrs), _ptr(anc_dirs), anc_ctrs.shape[0], _ptr(first_dev),
                                     C.c_void_p(first_host.data_ptr()), _ptr(agt_ctrs), _ptr(agt_dir_last), _ptr(agt_vel),
                                     A_, k, _ptr(top_idx), _ptr(ups[0]), _ptr(ups[1]), _ptr(ups[2]), _ptr(ups[3]),
                                     _ptr(d_pred), _stream()), "lgcn_goal_decode_bwd")
    return d_pred


def _roi_loss_args(logits, goals, trajs, gt, has, who):
    logits = _dev(logits, torch.float32, "logits")
    goals = _dev(goals, torch.float32, "goals")
    trajs = _dev(trajs, torch.float32, "trajs")
    gt = _dev(gt, torch.float32, "gt")
    has = _dev(has, torch.uint8 if has.dtype == torch.uint8 else torch.bool, "has")
    if logits.dim() != 2 or trajs.dim() != 4:
        raise L.LgcnError("%s: logits [A, M] and trajs [A, M, T, 2] expected, got %s and %s"
                          % (who, tuple(logits.shape), tuple(trajs.shape)))
    A_, M = logits.shape
    T = trajs.shape[2]
    if (tuple(goals.shape) != (A_, M, 2) or tuple(trajs.shape) != (A_, M, T, 2) or tuple(gt.shape) != (A_, T, 2)
            or tuple(has.shape) != (A_, T)):
        raise L.LgcnError("%s: goals [A, M, 2], trajs [A, M, T, 2], gt [A, T, 2], has [A, T] expected for A = %d, M = %d, "
                          "T = %d; got %s, %s, %s, %s" % (who, A_, M, T, tuple(goals.shape), tuple(trajs.shape),
                                                          tuple(gt.shape), tuple(has.shape)))
    return logits, goals, trajs, gt, has, A_, M, T


def roi_loss_fwd(logits, goals, trajs, gt, has, reg_coef: float = 1.0):
    """lgcn_roi_loss_fwd: (sums [3] fp32 = cls, reg_goal, reg_traj; counts [3] int32 = num_cls, num_reg_goal,
    num_reg_traj; sel [A] int32 = min_idx | has_goal << 8; pred_goals [A, 2])."""
    lib = L.load()
    logits, goals, trajs, gt, has, A_, M, T = _roi_loss_args(logits, goals, trajs, gt, has, "roi_loss_fwd")
    dev = logits.device
    new = torch.zeros if A_ == 0 else torch.empty          # an empty problem launches nothing: its sums are these zeros
    sums = new(3, dtype=torch.float32, device=dev)
    counts = new(3, dtype=torch.int32, device=dev)
    sel = torch.empty(A_, dtype=torch.int32, device=dev)
    pred_goals = torch.empty((A_, 2), dtype=torch.float32, device=dev)
    L.check(lib.lgcn_roi_loss_fwd(_ptr(logits), _ptr(goals), _ptr(trajs), _ptr(gt), _ptr(has), A_, M, T, float(reg_coef),
                                  _ptr(sums), _ptr(counts), _ptr(sel), _ptr(pred_goals), _stream()), "lgcn_roi_loss_fwd")
    return sums, counts, sel, pred_goals


def roi_loss_bwd(logits, goals, trajs, gt, has, reg_coef, sel, g_cls, g_goal, g_traj):
    """lgcn_roi_loss_bwd: (dlogits, dgoals, dtrajs), every element written; g_*: device scalars [1]."""
    lib = L.load()
    logits, goals, trajs, gt, has, A_, M, T = _roi_loss_args(logits, goals, trajs, gt, has, "roi_loss_bwd")
    sel = _dev(sel, torch.int32, "sel")
    gs = [_dev(g, torch.float32, "upstream gradient") for g in (g_cls, g_goal, g_traj)]
    if sel.numel() != A_ or any(g.numel() != 1 for g in gs):
        raise L.LgcnError("roi_loss_bwd: sel [A] and three one-element gradients expected")
    dlogits, dgoals, dtrajs = torch.empty_like(logits), torch.empty_like(goals), torch.empty_like(trajs)
    L.check(lib.lgcn_roi_loss_bwd(_ptr(logits), _ptr(goals), _ptr(trajs), _ptr(gt), _ptr(has), A_, M, T, float(reg_coef),
                                  _ptr(sel), _ptr(gs[0]), _ptr(gs[1]), _ptr(gs[2]), _ptr(dlogits), _ptr(dgoals), _ptr(dtrajs),
                                  _stream()), "lgcn_roi_loss_bwd")
    return dlogits, dgoals, dtrajs


# ------------------------------------------------------------------ lane-RoI extraction (data_lrcnn.generate_lane_roi)
ROI_REL = 14
ROI_STATUS_RANGE, ROI_STATUS_LEVELS = 1, 2


def roi_max_lanes() -> int:
    """Largest lane count of one scene the lane-RoI kernels take (LGCN_ESHAPE above it)."""
    return int(L.load().lgcn_roi_max_lanes())


class RoiJob:
    """One batch's lgcn_roi_t with the tensors it points to.  ``t``: the concatenated inputs on the device -- ctrs, feats,
    turn [N,2] fp32, control, intersect [N] fp32, lane_idcs [N] int32, a_ctrs [A,2], a_feats, a_obs [A,20,2] fp32,
    suc_pairs, pre_pairs [P,2] int32, edge_u, edge_v [E] int32 (scene-local) -- and ``off``: the host int32 offset table
    of include/lgcn.h.  roi_search / roi_nodes / roi_edge_count / roi_edge_fill fill it stage by stage."""

    def __init__(self, t: dict, off, horizon_buffer: float):
        import numpy as np
        self.off = np.ascontiguousarray(off, np.int32)
        S = (len(self.off) - 7) // (ROI_REL + 6)
        if S < 0 or len(self.off) != 6 * (S + 1) + ROI_REL * S + 1:
            raise L.LgcnError("roi: the offset table must hold 6 (S + 1) + 14 S + 1 entries, got %d" % len(self.off))
        kinds = dict(ctrs=torch.float32, feats=torch.float32, turn=torch.float32, control=torch.float32,
                     intersect=torch.float32, lane_idcs=torch.int32, a_ctrs=torch.float32, a_feats=torch.float32,
                     a_obs=torch.float32, suc_pairs=torch.int32, pre_pairs=torch.int32, edge_u=torch.int32, edge_v=torch.int32)
        self.t = {k: _dev(t[k], dt, "roi " + k) for k, dt in kinds.items()}
        N, A_ = self.t["lane_idcs"].numel(), self.t["a_ctrs"].shape[0]
        shapes = dict(ctrs=(N, 2), feats=(N, 2), turn=(N, 2), control=(N,), intersect=(N,), a_feats=(A_, 20, 2), a_obs=(A_, 20, 2),
                      edge_v=tuple(self.t["edge_u"].shape))
        for k, shp in shapes.items():
            if tuple(self.t[k].shape) != shp:
                raise L.LgcnError("roi: %s must be %s, got %s" % (k, shp, tuple(self.t[k].shape)))
        self.S, self.N, self.A = S, N, A_
        dev = self.t["ctrs"].device
        p = self.p = L.Roi()
        p.n_scenes, p.n_agents, p.n_nodes = S, A_, N
        p.n_lanes, p.n_slots = (int(self.off[2 * S + 1]), int(self.off[4 * S + 3])) if S else (0, 0)
        p.n_edges, p.n_suc, p.n_pre = self.t["edge_u"].numel(), self.t["suc_pairs"].shape[0], self.t["pre_pairs"].shape[0]
        p.horizon_buffer = float(horizon_buffer)
        p.off_host = self.off.ctypes.data
        self.off_dev = torch.from_numpy(self.off).to(dev)
        p.off_dev = self.off_dev.data_ptr()
        for k, v in self.t.items():
            setattr(p, k, v.data_ptr() if v.numel() else None)
        n_ws = L.load().lgcn_roi_ws_elems(N, p.n_lanes, p.n_edges, p.n_slots, A_)
        if n_ws < 0:
            L.check(int(n_ws), "lgcn_roi_ws_elems")
        self.ws = torch.empty(int(n_ws), dtype=torch.int32, device=dev)
        # one buffer, one read-back: node counts [A], the status word, then the speeds [A] (fp32 bits)
        self.agent_out = torch.zeros(2 * A_ + 1, dtype=torch.int32, device=dev)
        self.agent_nodes, self.agent_vel = self.agent_out[:A_ + 1], self.agent_out[A_ + 1:].view(torch.float32)
        p.ws, p.agent_nodes, p.agent_vel = self.ws.data_ptr(), self.agent_nodes.data_ptr(), self.agent_vel.data_ptr()


def roi_search(job: RoiJob):
    """lgcn_roi_search: fills job.agent_nodes [A + 1] (node count of every agent's RoI, 0 = dropped; last word = status)
    and job.agent_vel [A]."""
    L.check(L.load().lgcn_roi_search(C.byref(job.p), _stream()), "lgcn_roi_search")
    return job.agent_nodes, job.agent_vel


def roi_nodes(job: RoiJob, roi_agent: torch.Tensor, roi_base: torch.Tensor, n_out_nodes: int):
    """lgcn_roi_nodes: (node_mask [T] int64, feats [T,8], agent_feat [R,80]) of the kept RoIs roi_agent [R] int32 whose
    nodes start at roi_base [R + 1] int32."""
    p, dev = job.p, job.ws.device
    job.roi_agent, job.roi_base = _dev(roi_agent, torch.int32, "roi_agent"), _dev(roi_base, torch.int32, "roi_base")
    R, T = job.roi_agent.numel(), int(n_out_nodes)
    if job.roi_base.numel() != R + 1:
        raise L.LgcnError("roi_nodes: roi_base must hold R + 1 entries")
    job.node_mask = torch.empty(T, dtype=torch.int64, device=dev)
    job.out_feats = torch.empty((T, 8), dtype=torch.float32, device=dev)
    job.agent_feat = torch.empty((R, 80), dtype=torch.float32, device=dev)
    job.near = torch.empty(T, dtype=torch.int32, device=dev)
    p.n_rois, p.n_out_nodes = R, T
    p.roi_agent, p.roi_base = job.roi_agent.data_ptr(), job.roi_base.data_ptr()
    p.node_mask, p.out_feats, p.agent_feat, p.near = (job.node_mask.data_ptr(), job.out_feats.data_ptr(),
                                                      job.agent_feat.data_ptr(), job.near.data_ptr())
    L.check(L.load().lgcn_roi_nodes(C.byref(p), _stream()), "lgcn_roi_nodes")
    return job.node_mask, job.out_feats, job.agent_feat


def roi_edge_count(job: RoiJob) -> torch.Tensor:
    """lgcn_roi_edge_count: [R, 15] int32 -- per RoI the edge counts of the 14 induced relations, then |a2m|."""
    job.edge_cnt = torch.empty((job.p.n_rois, ROI_REL + 1), dtype=torch.int32, device=job.ws.device)
    job.p.edge_cnt = job.edge_cnt.data_ptr()
    L.check(L.load().lgcn_roi_edge_count(C.byref(job.p), _stream()), "lgcn_roi_edge_count")
    return job.edge_cnt


def roi_edge_fill(job: RoiJob, edge_base: torch.Tensor, n_out_edges: int, n_out_a2m: int):
    """lgcn_roi_edge_fill: (u, v [n_out_edges] int64, a2m_v [n_out_a2m] int32) at the offsets edge_base [R, 15] int32."""
    p, dev = job.p, job.ws.device
    job.edge_base = _dev(edge_base, torch.int32, "edge_base")
    if job.edge_base.numel() != p.n_rois * (ROI_REL + 1):
        raise L.LgcnError("roi_edge_fill: edge_base must be [R, 15]")
    job.out_u = torch.empty(int(n_out_edges), dtype=torch.int64, device=dev)
    job.out_v = torch.empty(int(n_out_edges), dtype=torch.int64, device=dev)
    job.a2m_v = torch.empty(int(n_out_a2m), dtype=torch.int32, device=dev)
    p.n_out_edges, p.n_out_a2m = int(n_out_edges), int(n_out_a2m)
    p.edge_base, p.out_u, p.out_v, p.a2m_v = (job.edge_base.data_ptr(), job.out_u.data_ptr(), job.out_v.data_ptr(),
                                              job.a2m_v.data_ptr())
    L.check(L.load().lgcn_roi_edge_fill(C.byref(p), _stream()), "lgcn_roi_edge_fill")
    return job.out_u, job.out_v, job.a2m_v


def roi_edge_fill_graph(job: RoiJob, edge_base: torch.Tensor, n_out_edges: int, n_out_a2m: int):
    """lgcn_roi_edge_fill_graph: (u, v [n_out_edges], a2m_u, a2m_v [n_out_a2m], all int64) -- the indices of the batch's
    merged block-diagonal graph (node index + the RoI's node offset; a2m_u = the RoI's number) at the offsets edge_base
    [R, 15] int32.  With a relation-major edge_base every relation of the batch graph is one run of u / v."""
    p, dev = job.p, job.ws.device
    job.edge_base = _dev(edge_base, torch.int32, "edge_base")
    if job.edge_base.numel() != p.n_rois * (ROI_REL + 1):
        raise L.LgcnError("roi_edge_fill_graph: edge_base must be [R, 15]")
    job.out_u = torch.empty(int(n_out_edges), dtype=torch.int64, device=dev)
    job.out_v = torch.empty(int(n_out_edges), dtype=torch.int64, device=dev)
    job.a2m_u64 = torch.empty(int(n_out_a2m), dtype=torch.int64, device=dev)
    job.a2m_v64 = torch.empty(int(n_out_a2m), dtype=torch.int64, device=dev)
    p.n_out_edges, p.n_out_a2m = int(n_out_edges), int(n_out_a2m)
    p.edge_base, p.out_u, p.out_v = job.edge_base.data_ptr(), job.out_u.data_ptr(), job.out_v.data_ptr()
    L.check(L.load().lgcn_roi_edge_fill_graph(C.byref(p), job.a2m_u64.data_ptr(), job.a2m_v64.data_ptr(), _stream()),
            "lgcn_roi_edge_fill_graph")
    return job.out_u, job.out_v, job.a2m_u64, job.a2m_v64


# ------------------------------------------------------------------ device-resident scene store (flatfile.DeviceSceneStore)
STORE_FLOATS = ("node_ctrs", "node_feats", "turn", "control", "intersect", "actor_ctrs", "actor_feats", "rot", "orig")


def store_table_elems(n_scenes: int, n_rel: int) -> int:
    """int64 entries of the per-batch table of lgcn_store_gather for n_scenes picked scenes and n_rel relations."""
    n = int(L.load().lgcn_store_table_elems(int(n_scenes), int(n_rel)))
    if n < 0:
        L.check(n, "lgcn_store_table_elems")
    return n


class StoreJob:
    """A flat store's lgcn_store_t with the device tensors it points to.  ``t``: node_ctrs, node_feats, turn [N,2],
    control, intersect [N], actor_ctrs [A,2], actor_feats [A,20,3], rot [S,2,2], orig [S,2] fp32, edge_u, edge_v [E] int32
    and, both or neither, gt_preds [A,30,2] fp32 and has_preds [A,30] uint8."""

    def __init__(self, t: dict):
        kinds = {k: torch.float32 for k in STORE_FLOATS}
        kinds.update(edge_u=torch.int32, edge_v=torch.int32)
        if ("gt_preds" in t) != ("has_preds" in t):
            raise L.LgcnError("store: gt_preds and has_preds come together")
        if "gt_preds" in t:
            kinds.update(gt_preds=torch.float32, has_preds=torch.uint8)
        self.t = {k: _dev(t[k], dt, "store " + k) for k, dt in kinds.items()}
        N, A_, S = self.t["control"].numel(), self.t["actor_ctrs"].shape[0], self.t["rot"].shape[0]
        shapes = dict(node_ctrs=(N, 2), node_feats=(N, 2), turn=(N, 2), control=(N,), intersect=(N,), actor_ctrs=(A_, 2),
                      actor_feats=(A_, 20, 3), rot=(S, 2, 2), orig=(S, 2), edge_v=tuple(self.t["edge_u"].shape),
                      gt_preds=(A_, 30, 2), has_preds=(A_, 30))
        for k, v in self.t.items():
            if k in shapes and tuple(v.shape) != shapes[k]:
                raise L.LgcnError("store: %s must be %s, got %s" % (k, shapes[k], tuple(v.shape)))
        p = self.p = L.Store()
        p.n_scenes, p.n_nodes, p.n_actors, p.n_edges = S, N, A_, self.t["edge_u"].numel()
        for k, v in self.t.items():
            setattr(p, k, v.data_ptr() if v.numel() else None)
        self.has_gt = "gt_preds" in self.t
        self.device = self.t["rot"].device
        self.nbytes = sum(v.numel() * v.element_size() for v in self.t.values())


def store_gather(job: StoreJob, tab_host: torch.Tensor, tab_dev: torch.Tensor, n_scenes: int, n_rel: int, n_nodes: int,
                 n_actors: int, n_elem: int, out: dict, aug_host: torch.Tensor = None, aug_dev: torch.Tensor = None) -> None:
    """lgcn_store_gather: one launch on the current stream fills ``out`` (name -> device tensor, the output fields of
    lgcn_store_batch_t) with the batch that the table describes.  ``tab_host``: the int64 table on the host, validated by
    the library before the launch; ``tab_dev``: the same words on the device (the caller has queued the copy on the
    current stream).  ``aug_host`` / ``aug_dev``: both or neither; the [n_scenes, 8] fp32 rotation table of
    lgcn_store_gather_aug on the host and on the device -- the same launch, with the scenes turned on the way through."""
    if tab_host.is_cuda or tab_host.dtype != torch.int64 or not tab_host.is_contiguous():
        raise L.LgcnError("store_gather: tab_host must be a contiguous int64 host tensor")
    if (aug_host is None) != (aug_dev is None):
        raise L.LgcnError("store_gather: aug_host and aug_dev come together")
    if aug_host is not None:
        if aug_host.is_cuda or aug_host.dtype != torch.float32 or not aug_host.is_contiguous():
            raise L.LgcnError("store_gather: aug_host must be a contiguous float32 host tensor")
        aug_dev = _dev(aug_dev, torch.float32, "store aug_dev")
        if aug_dev.device != job.device or aug_host.numel() != 8 * n_scenes or aug_dev.numel() != 8 * n_scenes:
            raise L.LgcnError("store_gather: the rotation table must hold [n_scenes, 8] floats on the host and on the "
                              "store's device")
    tab_dev = _dev(tab_dev, torch.int64, "store tab_dev")
    if tab_dev.device != job.device or tab_dev.device.index != torch.cuda.current_device():
        raise L.LgcnError("store_gather: the store lives on %s, which is not the current device" % (job.device,))
    if tab_host.numel() != tab_dev.numel() or tab_host.numel() != store_table_elems(n_scenes, n_rel):
        raise L.LgcnError("store_gather: the table must hold lgcn_store_table_elems(n_scenes, n_rel) entries")
    b = _store_batch(job, tab_dev, n_scenes, n_rel, n_nodes, n_actors, n_elem, out)
    b.tab_host = tab_host.data_ptr()
    if aug_host is None:
        L.check(L.load().lgcn_store_gather(C.byref(job.p), C.byref(b), _stream()), "lgcn_store_gather")
    else:
        L.check(L.load().lgcn_store_gather_aug(C.byref(job.p), C.byref(b), aug_host.data_ptr(), aug_dev.data_ptr(), _stream()),
                "lgcn_store_gather_aug")


def _store_batch(job: StoreJob, tab_dev: torch.Tensor, n_scenes: int, n_rel: int, n_nodes: int, n_actors: int, n_elem: int,
                 out: dict) -> "L.StoreBatch":
    """The lgcn_store_batch_t of a gather into ``out`` (tab_host is left to the caller), its outputs checked."""
    b = L.StoreBatch()
    b.n_scenes, b.n_rel, b.n_nodes, b.n_actors, b.n_elem = n_scenes, n_rel, n_nodes, n_actors, n_elem
    b.tab_dev = tab_dev.data_ptr()
    n_seg = 2 * n_rel * n_scenes
    f32, i32, i64 = torch.float32, torch.int32, torch.int64
    want = dict(node_ctrs=(f32, 2 * n_nodes), node_feats=(f32, 2 * n_nodes), turn=(f32, 2 * n_nodes), control=(f32, n_nodes),
                intersect=(f32, n_nodes), actor_ctrs=(f32, 2 * n_actors), node_off=(i32, n_scenes + 1),
                actor_off=(i32, n_scenes + 1), idx_local=(i64, n_elem), seg_off=(i64, n_seg + 1), seg_base=(i64, n_seg),
                actor_feats=(f32, 60 * n_actors), rot=(f32, 4 * n_actors), orig=(f32, 2 * n_actors))
    if job.has_gt:
        want.update(gt_preds=(f32, 60 * n_actors), has_preds=(None, 30 * n_actors))
    if set(out) != set(want):
        raise L.LgcnError("store_gather: outputs must be %s, got %s" % (sorted(want), sorted(out)))
    for k, v in out.items():
        dt, n = want[k]
        if not v.is_cuda or not v.is_contiguous() or v.device != job.device:
            raise L.LgcnError("store_gather: %s must be a contiguous CUDA tensor on the store's device (the HIP hot path "
                              "has no CPU fallback)" % k)
        if v.numel() != n or (v.dtype != dt if dt is not None else v.element_size() != 1):
            raise L.LgcnError("store_gather: %s must hold %d elements of %s, got %d of %s" % (k, n, dt or "one byte", v.numel(), v.dtype))
        setattr(b, k, v.data_ptr() if n else None)
    return b


class StorePadJob:
    """The lgcn_store_batch_t of a PADDED batch (lgcn_store_gather_pad: n_scenes = picked scenes + the filler, the totals
    are the capacities), built once per slot: ``check(tab_host)`` is lgcn_store_pad_check on a host table (no launch, no
    GPU work), ``launch()`` the gather on the current stream from the words that are in ``tab_dev`` by then.  Arguments as
    store_gather's."""

    def __init__(self, job: StoreJob, tab_dev: torch.Tensor, n_scenes: int, n_rel: int, n_nodes: int, n_actors: int,
                 n_elem: int, out: dict):
        tab_dev = _dev(tab_dev, torch.int64, "store tab_dev")
        if tab_dev.device != job.device or tab_dev.numel() != store_table_elems(n_scenes, n_rel):
            raise L.LgcnError("store_gather_pad: tab_dev must hold lgcn_store_table_elems(n_scenes, n_rel) entries on the "
                              "store's device")
        self.job, self.tab_dev, self.out = job, tab_dev, dict(out)      # (the struct holds their addresses)
        self.b = _store_batch(job, tab_dev, n_scenes, n_rel, n_nodes, n_actors, n_elem, out)

    def check(self, tab_host: torch.Tensor) -> None:
        if tab_host.is_cuda or tab_host.dtype != torch.int64 or not tab_host.is_contiguous() \
                or tab_host.numel() != self.tab_dev.numel():
            raise L.LgcnError("store_gather_pad: tab_host must be a contiguous int64 host tensor of tab_dev's size")
        L.check(L.load().lgcn_store_pad_check(C.byref(self.job.p), C.byref(self.b), tab_host.data_ptr()), "lgcn_store_pad_check")

    def launch(self) -> None:
        if self.job.device.index != torch.cuda.current_device():
            raise L.LgcnError("store_gather_pad: the store lives on %s, which is not the current device" % (self.job.device,))
        L.check(L.load().lgcn_store_gather_pad(C.byref(self.job.p), C.byref(self.b), _stream()), "lgcn_store_gather_pad")


def store_pack_table_elems(n_seg: int, n_src: int) -> int:
    """int64 entries of the table of lgcn_store_pack for n_seg runs out of n_src sources."""
    n = int(L.load().lgcn_store_pack_table_elems(int(n_seg), int(n_src)))
    if n < 0:
        L.check(n, "lgcn_store_pack_table_elems")
    return n


_PACK_KINDS = {torch.int16: 2, torch.int32: 4, torch.int64: 8}


class StorePackJob:
    """One lgcn_store_pack_t with its table (host and device copy) and the tensors it points to; store_pack's arguments.
    Building it validates what the wrapper can see and uploads the table; nothing is launched."""

    def __init__(self, sources, seg_src, seg_at, seg_len, dst: torch.Tensor, frame: torch.Tensor = None,
                 rot: torch.Tensor = None, orig: torch.Tensor = None):
        import numpy as np
        seg_src, seg_at, seg_len = (np.asarray(x).reshape(-1) for x in (seg_src, seg_at, seg_len))
        G, K = len(seg_len), len(sources)
        if len(seg_src) != G or len(seg_at) != G or any(x.size and x.dtype.kind not in "iu" for x in (seg_src, seg_at, seg_len)):
            raise L.LgcnError("store_pack: seg_src, seg_at and seg_len must be integer sequences of one length")
        if not dst.is_contiguous():
            raise L.LgcnError("store_pack: dst must be contiguous")
        dst = _dev(dst, torch.int32, "store_pack dst")
        dev = dst.device
        if dev.index != torch.cuda.current_device():
            raise L.LgcnError("store_pack: dst lives on %s, which is not the current device" % (dev,))
        tab = np.empty(store_pack_table_elems(G, K), np.int64)
        tab[0] = 0
        np.cumsum(seg_len, dtype=np.int64, out=tab[1:G + 1])
        tab[G + 1:2 * G + 1], tab[2 * G + 1:3 * G + 1] = seg_src, seg_at
        at = 3 * G + 1
        for i, t in enumerate(sources):
            if not torch.is_tensor(t) or t.dtype not in _PACK_KINDS or not t.is_cuda or t.device != dev or not t.is_contiguous():
                raise L.LgcnError("store_pack: source %d must be a contiguous int16 / int32 / int64 tensor on %s (the HIP hot "
                                  "path has no CPU fallback)" % (i, dev))
            n = t.numel()
            tab[at + i], tab[at + K + i], tab[at + 2 * K + i] = (t.data_ptr() if n else 0), _PACK_KINDS[t.dtype], n
        n_dst = int(tab[G])
        if G and (int(np.min(seg_len)) < 0 or n_dst > dst.numel()):
            raise L.LgcnError("store_pack: the runs hold %d words, dst %d" % (n_dst, dst.numel()))
        p = L.StorePack()
        p.n_seg, p.n_src, p.n_dst = G, K, n_dst
        if (frame is None) != (rot is None) or (frame is None) != (orig is None):
            raise L.LgcnError("store_pack: frame, rot and orig come together")
        if frame is not None:
            if not (rot.is_contiguous() and orig.is_contiguous()):
                raise L.LgcnError("store_pack: rot and orig must be contiguous")
            frame, rot, orig = (_dev(t, torch.float32, "store_pack " + k) for t, k in ((frame, "frame"), (rot, "rot"), (orig, "orig")))
            S = frame.shape[0] if frame.dim() == 2 else -1
            if tuple(frame.shape) != (S, 6) or rot.numel() != 4 * S or orig.numel() != 2 * S or {frame.device, rot.device, orig.device} != {dev}:
                raise L.LgcnError("store_pack: frame [S,6], rot [S,2,2] and orig [S,2] on dst's device")
            p.n_scenes = S
            p.frame, p.rot, p.orig = (t.data_ptr() if S else None for t in (frame, rot, orig))
        if G == 0 and p.n_scenes:
            raise L.LgcnError("store_pack: frame rows need at least one run")
        tab_dev = torch.from_numpy(tab).to(dev) if G else None
        p.tab_host, p.tab_dev, p.dst = tab.ctypes.data, (tab_dev.data_ptr() if G else None), (dst.data_ptr() if n_dst else None)
        self.p, self.n_dst, self.keep = p, n_dst, (tab, tab_dev, dst, list(sources), frame, rot, orig)


def store_pack_launch(job: StorePackJob) -> int:
    """The launch of a StorePackJob on the current stream (n_seg == 0: none); returns the words written."""
    L.check(L.load().lgcn_store_pack(C.byref(job.p), _stream()), "lgcn_store_pack")
    return job.n_dst


def store_pack(sources, seg_src, seg_at, seg_len, dst: torch.Tensor, frame: torch.Tensor = None, rot: torch.Tensor = None,
               orig: torch.Tensor = None) -> int:
    """lgcn_store_pack: one launch on the current stream writes dst[:n] (int32 device tensor, n = sum(seg_len)) with the
    runs sources[seg_src[k]][seg_at[k] : seg_at[k] + seg_len[k]] back to back, converted as numpy's astype(int32)
    converts them, and leaves the rest of dst alone.  sources: flat contiguous int16 / int32 / int64 device tensors (views
    of one array are fine); seg_src, seg_at, seg_len: host integer sequences of one length.  frame [S,6] fp32 with rot
    [S,2,2] and orig [S,2] (all three or none): the same launch cuts the frame rows (orig, rot) into them.  Returns n.
    The table is validated by the library on the host before the launch; a table that does not fit raises LgcnError."""
    return store_pack_launch(StorePackJob(sources, seg_src, seg_at, seg_len, dst, frame, rot, orig))


# ------------------------------------------------------------------ resident lane-RoI store (data_lrcnn.RoiStore)
ROI_STORE_SEGS = 2 * ROI_REL + 2        # index runs per picked scene: u and v of the 14 relations, a2m_u, a2m_v


def roi_store_table_elems(n_scenes: int) -> int:
    """int64 entries of the per-batch table of lgcn_roi_store_gather for n_scenes picked scenes."""
    n = int(L.load().lgcn_roi_store_table_elems(int(n_scenes)))
    if n < 0:
        L.check(n, "lgcn_roi_store_table_elems")
    return n


class RoiStoreJob:
    """A resident RoI store's lgcn_roi_store_t with the device tensors it points to.  ``t``: feats [T,8] fp32, node_mask
    [T] int32, agent_feat [R,80], ctrs [R,2], actor_feats, obs [R,20,3] fp32, edge_u, edge_v [E], a2m_u, a2m_v [M] int32
    (scene-local) and, both or neither, gt_preds [R,30,2] fp32 and has_preds [R,30] uint8."""
    FLOATS = ("feats", "agent_feat", "ctrs", "actor_feats", "obs")
    INTS = ("node_mask", "edge_u", "edge_v", "a2m_u", "a2m_v")

    def __init__(self, t: dict, n_scenes: int):
        kinds = {k: torch.float32 for k in self.FLOATS}
        kinds.update({k: torch.int32 for k in self.INTS})
        if ("gt_preds" in t) != ("has_preds" in t):
            raise L.LgcnError("roi store: gt_preds and has_preds come together")
        if "gt_preds" in t:
            kinds.update(gt_preds=torch.float32, has_preds=torch.uint8)
        self.t = {k: _dev(t[k], dt, "roi store " + k) for k, dt in kinds.items()}
        T, R = self.t["node_mask"].numel(), self.t["agent_feat"].shape[0]
        shapes = dict(feats=(T, 8), agent_feat=(R, 80), ctrs=(R, 2), actor_feats=(R, 20, 3), obs=(R, 20, 3),
                      edge_v=tuple(self.t["edge_u"].shape), a2m_v=tuple(self.t["a2m_u"].shape), gt_preds=(R, 30, 2),
                      has_preds=(R, 30))
        for k, v in self.t.items():
            if k in shapes and tuple(v.shape) != shapes[k]:
                raise L.LgcnError("roi store: %s must be %s, got %s" % (k, shapes[k], tuple(v.shape)))
        p = self.p = L.RoiStore()
        p.n_scenes, p.n_nodes, p.n_rois = int(n_scenes), T, R
        p.n_edges, p.n_a2m = self.t["edge_u"].numel(), self.t["a2m_u"].numel()
        for k, v in self.t.items():
            setattr(p, k, v.data_ptr() if v.numel() else None)
        self.has_gt = "gt_preds" in self.t
        self.device = self.t["feats"].device
        self.nbytes = sum(v.numel() * v.element_size() for v in self.t.values())


def roi_store_gather(job: RoiStoreJob, tab_host: torch.Tensor, tab_dev: torch.Tensor, n_scenes: int, n_nodes: int,
                     n_rois: int, n_elem: int, out: dict) -> None:
    """lgcn_roi_store_gather: one launch on the current stream fills ``out`` (name -> device tensor, the output fields
    of lgcn_roi_store_batch_t) with the pick that the table describes.  ``tab_host``: the int64 table on the host,
    validated by the library before the launch; ``tab_dev``: the same words on the device (the caller has queued the
    copy on the current stream)."""
    if tab_host.is_cuda or tab_host.dtype != torch.int64 or not tab_host.is_contiguous():
        raise L.LgcnError("roi_store_gather: tab_host must be a contiguous int64 host tensor")
    tab_dev = _dev(tab_dev, torch.int64, "roi store tab_dev")
    if tab_dev.device != job.device or tab_dev.device.index != torch.cuda.current_device():
        raise L.LgcnError("roi_store_gather: the store lives on %s, which is not the current device" % (job.device,))
    if tab_host.numel() != tab_dev.numel() or tab_host.numel() != roi_store_table_elems(n_scenes):
        raise L.LgcnError("roi_store_gather: the table must hold lgcn_roi_store_table_elems(n_scenes) entries")
    b = L.RoiStoreBatch()
    b.n_scenes, b.n_nodes, b.n_rois, b.n_elem = n_scenes, n_nodes, n_rois, n_elem
    b.tab_host, b.tab_dev = tab_host.data_ptr(), tab_dev.data_ptr()
    f32, i64 = torch.float32, torch.int64
    want = dict(feats=(f32, 8 * n_nodes), node_mask=(i64, n_nodes), agent_feat=(f32, 80 * n_rois), idx=(i64, n_elem),
                ctrs=(f32, 2 * n_rois), actor_feats=(f32, 60 * n_rois), obs=(f32, 60 * n_rois))
    if job.has_gt:
        want.update(gt_preds=(f32, 60 * n_rois), has_preds=(None, 30 * n_rois))
    if set(out) != set(want):
        raise L.LgcnError("roi_store_gather: outputs must be %s, got %s" % (sorted(want), sorted(out)))
    for k, v in out.items():
        dt, n = want[k]
        if not v.is_cuda or not v.is_contiguous() or v.device != job.device:
            raise L.LgcnError("roi_store_gather: %s must be a contiguous CUDA tensor on the store's device (the HIP hot "
                              "path has no CPU fallback)" % k)
        if v.numel() != n or (v.dtype != dt if dt is not None else v.element_size() != 1):
            raise L.LgcnError("roi_store_gather: %s must hold %d elements of %s, got %d of %s"
                              % (k, n, dt or "one byte", v.numel(), v.dtype))
        setattr(b, k, v.data_ptr() if n else None)
    L.check(L.load().lgcn_roi_store_gather(C.byref(job.p), C.byref(b), _stream()), "lgcn_roi_store_gather")


# ------------------------------------------------------------------ scene construction (data_raw: get_obj_feats / get_lane_graph)
def _i32_table(off, what):
    import numpy as np
    off = np.asarray(off)
    if off.size and (off.min() < 0 or off.max() > 0x7fffffff):
        raise L.LgcnError("%s: the batch is too large for 32-bit offsets" % what)
    return np.ascontiguousarray(off, np.int32)


class SceneTracksJob:
    """One batch's lgcn_scene_tracks_t (reference data.py:148-217) with the tensors it points to.  xy [R,2] float64, step
    [R] int32, frame [S,6] fp32 (orig, rot) on the device; off: host int32 trk_off [S + 1] then row_off [T + 1]; head: a
    ZEROED int32 device tensor [S + 2].  The outputs hold T rows; head[S] of them are written."""

    def __init__(self, xy, step, frame, off, pred_range, head):
        self.xy, self.step = _dev(xy, torch.float64, "scene xy"), _dev(step, torch.int32, "scene step")
        self.frame, self.head = _dev(frame, torch.float32, "scene frame"), _dev(head, torch.int32, "scene head")
        S, R = self.frame.shape[0], self.step.numel()
        self.off = _i32_table(off, "scene_tracks")
        T = len(self.off) - (S + 1) - 1
        if T < 0 or tuple(self.xy.shape) != (R, 2) or tuple(self.frame.shape) != (S, 6) or self.head.numel() != S + 2:
            raise L.LgcnError("scene_tracks: xy [R,2], step [R], frame [S,6], off [S + T + 2], head [S + 2]")
        dev = self.frame.device
        self.S, self.T = S, T
        n_ws = L.load().lgcn_scene_tracks_ws_elems(T)
        if n_ws < 0:
            L.check(int(n_ws), "lgcn_scene_tracks_ws_elems")
        self.ws = torch.empty(int(n_ws), dtype=torch.int32, device=dev)
        self.off_dev = torch.from_numpy(self.off).to(dev)
        f32 = dict(dtype=torch.float32, device=dev)
        self.feats, self.obs = torch.empty((T, 20, 3), **f32), torch.empty((T, 20, 3), **f32)
        self.ctrs, self.gt = torch.empty((T, 2), **f32), torch.empty((T, 30, 2), **f32)
        self.has = torch.empty((T, 30), dtype=torch.bool, device=dev)
        p = self.p = L.SceneTracks()
        p.n_scenes, p.n_tracks, p.n_rows = S, T, R
        p.pred_range[:] = [float(x) for x in pred_range]
        p.off_host, p.off_dev = self.off.ctypes.data, self.off_dev.data_ptr()
        p.xy, p.step = (self.xy.data_ptr(), self.step.data_ptr()) if R else (None, None)
        p.frame, p.ws, p.head = self.frame.data_ptr(), self.ws.data_ptr(), self.head.data_ptr()
        p.feats, p.obs, p.ctrs, p.gt, p.has = (self.feats.data_ptr(), self.obs.data_ptr(), self.ctrs.data_ptr(),
                                               self.gt.data_ptr(), self.has.data_ptr())


def scene_tracks(job: SceneTracksJob):
    """lgcn_scene_tracks: two launches fill job.feats, obs, ctrs, gt, has (compacted) and job.head."""
    L.check(L.load().lgcn_scene_tracks(C.byref(job.p), _stream()), "lgcn_scene_tracks")


def scene_topo_elems(n_lanes: int, n_pred: int, n_succ: int) -> int:
    n = int(L.load().lgcn_scene_topo_elems(int(n_lanes), int(n_pred), int(n_succ)))
    if n < 0:
        L.check(n, "lgcn_scene_topo_elems")
    return n


class SceneLanesJob:
    """One batch's lgcn_scene_lanes_t (reference data.py:220-353).  tables: the batch's lane tables, each with n_lanes,
    n_pts, n_pred, n_succ, topo_host (numpy int32), topo_dev, pts_dev (device tensors); off: host int32 scene_tab [S],
    cand_off [S + 1], rank_off [S + 1] and, with explicit=True, cand [n_cand]; frame [S,6] fp32 on the device; head: an
    int32 device tensor [4 (S + 1)]."""

    def __init__(self, tables, off, explicit, frame, pred_range, head):
        self.frame, self.head = _dev(frame, torch.float32, "scene frame"), _dev(head, torch.int32, "scene head")
        S = self.frame.shape[0]
        self.off = _i32_table(off, "scene_lanes")
        if len(self.off) < 3 * S + 2 or tuple(self.frame.shape) != (S, 6) or self.head.numel() != 4 * (S + 1):
            raise L.LgcnError("scene_lanes: frame [S,6], off [3 S + 2 (+ n_cand)], head [4 (S + 1)]")
        dev = self.frame.device
        self.S, self.tables = S, list(tables)
        self.tabs = (L.LaneTableC * max(len(self.tables), 1))()
        for i, tb in enumerate(self.tables):
            c = self.tabs[i]
            c.n_lanes, c.n_pts, c.n_pred, c.n_succ = tb.n_lanes, tb.n_pts, tb.n_pred, tb.n_succ
            _dev(tb.topo_dev, torch.int32, "lane table topo")
            _dev(tb.pts_dev, torch.float64, "lane table pts")
            if tb.topo_dev.device != dev or tb.topo_host.size != tb.topo_dev.numel() or tb.pts_dev.numel() != 2 * tb.n_pts \
                    or tb.topo_host.size != scene_topo_elems(tb.n_lanes, tb.n_pred, tb.n_succ):
                raise L.LgcnError("scene_lanes: a lane table does not match its sizes or lives on another device")
            c.topo_host, c.topo_dev = tb.topo_host.ctypes.data, tb.topo_dev.data_ptr()
            c.pts = tb.pts_dev.data_ptr() if tb.n_pts else None
        self.tabs_dev = torch.frombuffer(bytearray(bytes(self.tabs)), dtype=torch.uint8).to(dev)
        self.off_dev = torch.from_numpy(self.off).to(dev)
        p = self.p = L.SceneLanes()
        p.n_scenes, p.n_tables, p.explicit_ids = S, len(self.tables), int(bool(explicit))
        p.n_cand, p.n_rank = (int(self.off[2 * S]), int(self.off[3 * S + 1])) if S else (0, 0)
        if len(self.off) != 3 * S + 2 + (p.n_cand if explicit else 0):
            raise L.LgcnError("scene_lanes: the offset table does not match its candidate count")
        p.pred_range[:] = [float(x) for x in pred_range]
        p.tabs_host, p.tabs_dev = C.addressof(self.tabs), self.tabs_dev.data_ptr()
        p.off_host, p.off_dev = self.off.ctypes.data, self.off_dev.data_ptr()
        n_ws = L.load().lgcn_scene_lanes_ws_elems(p.n_cand, p.n_rank)
        if n_ws < 0:
            L.check(int(n_ws), "lgcn_scene_lanes_ws_elems")
        self.ws = torch.empty(int(n_ws), dtype=torch.int32, device=dev)
        p.frame, p.ws, p.head = self.frame.data_ptr(), self.ws.data_ptr(), self.head.data_ptr()


def scene_lanes_rank(job: SceneLanesJob):
    """lgcn_scene_lanes_rank: one memset and two launches fill job.head (per scene, then in total: kept lanes, nodes,
    pred entries, succ entries, as exclusive sums)."""
    L.check(L.load().lgcn_scene_lanes_rank(C.byref(job.p), _stream()), "lgcn_scene_lanes_rank")


def scene_lanes_fill(job: SceneLanesJob, totals, head2: torch.Tensor) -> dict:
    """lgcn_scene_lanes_fill: two launches write the nodes, pre[0] / suc[0] and the four pair lists of the whole batch.
    totals = (kept lanes, nodes, pred entries, succ entries) as read from job.head; head2: int32 device [4 (S + 1)].
    Returns the output tensors, sized by their upper bounds (head2 tells how much of the edge and pair arrays is used)."""
    p, dev = job.p, job.frame.device
    n_l, n_n, n_p, n_s = (int(x) for x in totals)
    job.head2 = _dev(head2, torch.int32, "scene head2")
    if job.head2.numel() != 4 * (job.S + 1):
        raise L.LgcnError("scene_lanes_fill: head2 must hold 4 (S + 1) entries")
    f32, i64 = dict(dtype=torch.float32, device=dev), dict(dtype=torch.int64, device=dev)
    o = job.out = dict(
        ctrs=torch.empty((n_n, 2), **f32), feats=torch.empty((n_n, 2), **f32), turn=torch.empty((n_n, 2), **f32),
        control=torch.empty(n_n, **f32), intersect=torch.empty(n_n, **f32), lane_idcs=torch.empty(n_n, **i64),
        pre_u=torch.empty(n_n - n_l + n_p, **i64), pre_v=torch.empty(n_n - n_l + n_p, **i64),
        suc_u=torch.empty(n_n - n_l + n_s, **i64), suc_v=torch.empty(n_n - n_l + n_s, **i64),
        pre_pairs=torch.empty((n_p, 2), **i64), suc_pairs=torch.empty((n_s, 2), **i64),
        left_pairs=torch.empty((n_l, 2), **i64), right_pairs=torch.empty((n_l, 2), **i64))
    p.n_nodes, p.cap_pre, p.cap_suc = n_n, n_n - n_l + n_p, n_n - n_l + n_s
    p.cap_pre_pairs, p.cap_suc_pairs, p.cap_left_pairs, p.cap_right_pairs = n_p, n_s, n_l, n_l
    p.head2 = job.head2.data_ptr()
    for k, v in o.items():
        setattr(p, k, v.data_ptr() if v.numel() else None)
    L.check(L.load().lgcn_scene_lanes_fill(C.byref(p), _stream()), "lgcn_scene_lanes_fill")
    return o


# ------------------------------------------------------------------ forecasting metrics of a split (lanegcn_amd.evaluate)
EVAL_REC = 32          # floats of one scene's record (include/lgcn.h, lgcn_eval_scenes)
EVAL_MAX_MOD = 8
EVAL_MAX_T = 64


def _eval_arg(t, dtype, shape, name):
    """A contiguous device tensor of `dtype` and `shape` whose first byte is 16-byte aligned (a copy where a view is not)."""
    t = _dev(t, dtype, name)
    if tuple(t.shape) != tuple(shape):
        raise L.LgcnError("%s must be %s, got %s" % (name, tuple(shape), tuple(t.shape)))
    return t if t.data_ptr() % 16 == 0 else t.clone()


def _eval_out(t, dtype, shape, name):
    if t is None:
        return None
    if not t.is_cuda or not t.is_contiguous() or t.dtype != dtype or tuple(t.shape) != tuple(shape) or t.data_ptr() % 16:
        raise L.LgcnError("%s must be a contiguous, 16-byte aligned CUDA tensor of %s %s" % (name, dtype, tuple(shape)))
    return t


def _eval_batch_args(name, reg, cls, gt, has, actor_off, slot, rec, traj, score, err):
    """The checks eval_scenes and eval_actors share -> (the tensors in that order, A, B, M, T, n_slots)."""
    if reg.dim() != 4 or reg.shape[3] != 2:
        raise L.LgcnError("%s: reg must be [A, M, T, 2], got %s" % (name, tuple(reg.shape)))
    A, M, T, _ = reg.shape
    B = slot.numel()
    reg = _eval_arg(reg, torch.float32, (A, M, T, 2), name + " reg")
    cls = _eval_arg(cls, torch.float32, (A, M), name + " cls")
    gt = _eval_arg(gt, torch.float32, (A, T, 2), name + " gt")
    if has.dtype not in (torch.bool, torch.uint8):
        raise L.LgcnError("%s: has must be bool or uint8, got %s" % (name, has.dtype))
    has = _eval_arg(has, has.dtype, (A, T), name + " has")
    actor_off = _eval_arg(actor_off, torch.int32, (B + 1,), name + " actor_off")
    slot = _eval_arg(slot, torch.int64, (B,), name + " slot")
    if rec.dim() != 2:
        raise L.LgcnError("%s: rec must be [n_slots, %d]" % (name, EVAL_REC))
    n_slots = rec.shape[0]
    rec = _eval_out(rec, torch.float32, (n_slots, EVAL_REC), name + " rec")
    traj = _eval_out(traj, torch.float32, (n_slots, M, T, 2), name + " traj")
    score = _eval_out(score, torch.float32, (n_slots, M), name + " score")
    err = _eval_out(err, torch.int32, (1,), name + " err")
    if err is None:
        raise L.LgcnError("%s: err (int32 [1] on the device) is required" % name)
    if any(t is not None and t.device != reg.device for t in (cls, gt, has, actor_off, slot, rec, traj, score, err)):
        raise L.LgcnError("%s: every tensor must live on %s" % (name, reg.device))
    return (reg, cls, gt, has, actor_off, slot, rec, traj, score, err), A, B, M, T, n_slots


def eval_scenes(reg, cls, gt, has, actor_off, slot, horizon: int, rec, traj=None, score=None, err=None) -> None:
    """lgcn_eval_scenes: one launch on the current stream, no host read.  reg [A, M, T, 2], cls [A, M], gt [A, T, 2] fp32,
    has [A, T] bool / uint8, actor_off [B+1] int32, slot [B] int64; writes rec [n_slots, 32] (and traj [n_slots, M, T, 2],
    score [n_slots, M], both or neither) at the rows `slot` names.  err: int32 [1], set to 1 by a slot outside the table."""
    (reg, cls, gt, has, actor_off, slot, rec, traj, score, err), A, B, M, T, n_slots = _eval_batch_args(
        "eval_scenes", reg, cls, gt, has, actor_off, slot, rec, traj, score, err)
    if A == 0 and B > 0:          # no row to point at: every scene of the batch is empty; the kernel reads no row
        reg, cls, gt, has = rec, rec, rec, rec
    L.check(L.load().lgcn_eval_scenes(_ptr(reg), _ptr(cls), _ptr(gt), _ptr(has), _ptr(actor_off), _ptr(slot), B, M, T, int(horizon),
                                      n_slots, _ptr(rec), _ptr(traj), _ptr(score), _ptr(err), _stream()), "lgcn_eval_scenes")


def eval_reduce(rec, miss_thr: float, out, cnt, err) -> None:
    """lgcn_eval_reduce: one launch on the current stream: out [8, 6] float64 (row k - 1: the six sums at K = k), cnt [3]
    int64 (slots of flag 0, 1, 2), err int32 [1] (set to 1 when evaluated records disagree on M or the horizon)."""
    if rec.dim() != 2:
        raise L.LgcnError("eval_reduce: rec must be [n_slots, %d]" % EVAL_REC)
    n_slots = rec.shape[0]
    rec = _eval_out(rec, torch.float32, (n_slots, EVAL_REC), "eval_reduce rec")
    out = _eval_out(out, torch.float64, (EVAL_MAX_MOD, 6), "eval_reduce out")
    cnt = _eval_out(cnt, torch.int64, (3,), "eval_reduce cnt")
    err = _eval_out(err, torch.int32, (1,), "eval_reduce err")
    if out is None or cnt is None or err is None:
        raise L.LgcnError("eval_reduce: out, cnt and err are required")
    if n_slots == 0:
        out.zero_()
        cnt.zero_()
        return
    L.check(L.load().lgcn_eval_reduce(_ptr(rec), n_slots, float(miss_thr), _ptr(out), _ptr(cnt), _ptr(err), _stream()),
            "lgcn_eval_reduce")


def eval_actors(reg, cls, gt, has, actor_off, slot_base, horizon: int, rec, traj=None, score=None, err=None) -> None:
    """lgcn_eval_actors: one launch on the current stream, no host read: the record of EVERY actor row of the batch, partial
    futures included.  Tensors as eval_scenes; slot_base [B] int64 is the table row of each scene's first actor, the tables
    hold one row per actor of the split (row slot_base[b] + i for the i-th actor of scene b).  err is also set by a row that
    actor_off does not cover."""
    (reg, cls, gt, has, actor_off, slot_base, rec, traj, score, err), A, B, M, T, n_slots = _eval_batch_args(
        "eval_actors", reg, cls, gt, has, actor_off, slot_base, rec, traj, score, err)
    L.check(L.load().lgcn_eval_actors(_ptr(reg), _ptr(cls), _ptr(gt), _ptr(has), _ptr(actor_off), _ptr(slot_base), A, B, M, T,
                                      int(horizon), n_slots, _ptr(rec), _ptr(traj), _ptr(score), _ptr(err), _stream()),
            "lgcn_eval_actors")


EVAL_WHO = {"all": 0, "agent": 1, "others": 2}      # lgcn_eval_reduce_sel's `who`: every actor, local index 0, local index > 0


def eval_reduce_sel(rec, miss_thr: float, who: int, max_missing: int, out, cnt, err) -> None:
    """lgcn_eval_reduce_sel: eval_reduce over the records a selection keeps (who: 0 all, 1 the first actor of a scene, 2 the
    others; a flag-1 record counts only with at most max_missing unobserved steps).  cnt [4] int64: kept slots of flag
    0, 1, 2 and the excluded ones."""
    if rec.dim() != 2:
        raise L.LgcnError("eval_reduce_sel: rec must be [n_slots, %d]" % EVAL_REC)
    n_slots = rec.shape[0]
    rec = _eval_out(rec, torch.float32, (n_slots, EVAL_REC), "eval_reduce_sel rec")
    out = _eval_out(out, torch.float64, (EVAL_MAX_MOD, 6), "eval_reduce_sel out")
    cnt = _eval_out(cnt, torch.int64, (4,), "eval_reduce_sel cnt")
    err = _eval_out(err, torch.int32, (1,), "eval_reduce_sel err")
    if out is None or cnt is None or err is None:
        raise L.LgcnError("eval_reduce_sel: out, cnt and err are required")
    if int(who) not in (0, 1, 2) or int(max_missing) < 0:
        raise L.LgcnError("eval_reduce_sel: who must be 0, 1 or 2 and max_missing >= 0, got %s" % ((who, max_missing),))
    if n_slots == 0:
        out.zero_()
        cnt.zero_()
        return
    L.check(L.load().lgcn_eval_reduce_sel(_ptr(rec), n_slots, float(miss_thr), int(who), int(max_missing), _ptr(out), _ptr(cnt),
                                          _ptr(err), _stream()), "lgcn_eval_reduce_sel")


# ------------------------------------------------------------------ drivable-area compliance (lgcn_eval_*_da)
EVAL_DAC_OUT = 9       # lgcn_eval_dac_reduce's int64 words: the counts at K = 1..8, then n_dac


def _eval_drivable(name, da, scene_city, B, device):
    """The lgcn_drivable_t of `da` (an evaluate.DrivableArea moved to the device) and the batch's scene_city int32 [B]."""
    if getattr(da, "raster_dev", None) is None or da.raster_dev.device != device:
        raise L.LgcnError("%s: the DrivableArea must be moved to %s first (DrivableArea.to)" % (name, device))
    scene_city = _eval_arg(scene_city, torch.int32, (B,), name + " scene_city")
    if scene_city.device != device:
        raise L.LgcnError("%s: scene_city must live on %s" % (name, device))
    d = L.Drivable(da.raster_dev.data_ptr(), da.raster_dev.numel(), da.table_dev.data_ptr(), C.addressof(da.table),
                   len(da.table), scene_city.data_ptr())
    return d, scene_city


def eval_scenes_da(reg, cls, gt, has, actor_off, slot, horizon: int, rec, traj=None, score=None, err=None, da=None,
                   scene_city=None) -> None:
    """lgcn_eval_scenes_da: eval_scenes plus the record floats [30] (the bitmask of the modes that stay on the drivable area
    of the scene's city) and [31] (the city has a raster).  da: an evaluate.DrivableArea on the device; scene_city [B] int32 on
    the device, -1 for a scene without a map.  err is also set by a city id that `da` does not hold."""
    (reg, cls, gt, has, actor_off, slot, rec, traj, score, err), A, B, M, T, n_slots = _eval_batch_args(
        "eval_scenes_da", reg, cls, gt, has, actor_off, slot, rec, traj, score, err)
    d, scene_city = _eval_drivable("eval_scenes_da", da, scene_city, B, reg.device)
    if A == 0 and B > 0:
        reg, cls, gt, has = rec, rec, rec, rec
    L.check(L.load().lgcn_eval_scenes_da(_ptr(reg), _ptr(cls), _ptr(gt), _ptr(has), _ptr(actor_off), _ptr(slot), B, M, T,
                                         int(horizon), n_slots, _ptr(rec), _ptr(traj), _ptr(score), _ptr(err), C.byref(d),
                                         _stream()), "lgcn_eval_scenes_da")


def eval_actors_da(reg, cls, gt, has, actor_off, slot_base, horizon: int, rec, traj=None, score=None, err=None, da=None,
                   scene_city=None) -> None:
    """lgcn_eval_actors_da: eval_actors plus the record floats [30], [31] of eval_scenes_da, for every actor row."""
    (reg, cls, gt, has, actor_off, slot_base, rec, traj, score, err), A, B, M, T, n_slots = _eval_batch_args(
        "eval_actors_da", reg, cls, gt, has, actor_off, slot_base, rec, traj, score, err)
    d, scene_city = _eval_drivable("eval_actors_da", da, scene_city, B, reg.device)
    L.check(L.load().lgcn_eval_actors_da(_ptr(reg), _ptr(cls), _ptr(gt), _ptr(has), _ptr(actor_off), _ptr(slot_base), A, B, M, T,
                                         int(horizon), n_slots, _ptr(rec), _ptr(traj), _ptr(score), _ptr(err), C.byref(d),
                                         _stream()), "lgcn_eval_actors_da")


def eval_dac_reduce(rec, who: int, max_missing: int, dac) -> None:
    """lgcn_eval_dac_reduce: one launch on the current stream: dac [9] int64: dac[k - 1] = the compliant modes among the first
    k over the counted records (flag 1, a raster, kept by the selection), dac[8] = the counted records."""
    if rec.dim() != 2:
        raise L.LgcnError("eval_dac_reduce: rec must be [n_slots, %d]" % EVAL_REC)
    n_slots = rec.shape[0]
    rec = _eval_out(rec, torch.float32, (n_slots, EVAL_REC), "eval_dac_reduce rec")
    dac = _eval_out(dac, torch.int64, (EVAL_DAC_OUT,), "eval_dac_reduce dac")
    if dac is None:
        raise L.LgcnError("eval_dac_reduce: dac is required")
    if int(who) not in (0, 1, 2) or int(max_missing) < 0:
        raise L.LgcnError("eval_dac_reduce: who must be 0, 1 or 2 and max_missing >= 0, got %s" % ((who, max_missing),))
    if n_slots == 0:
        dac.zero_()
        return
    L.check(L.load().lgcn_eval_dac_reduce(_ptr(rec), n_slots, int(who), int(max_missing), _ptr(dac), _stream()),
            "lgcn_eval_dac_reduce")
