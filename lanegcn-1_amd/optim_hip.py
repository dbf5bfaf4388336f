"""The optimizer step on HIP (include/lgcn.h: lgcn_opt_step): gradient clamp + Adam / AdamW / SGD over every parameter
in one launch per (parameter group, step count), in place.  utils.Optimizer builds a FusedOptim instead of a torch.optim
optimizer when its class switch train_hip is set (reference utils.py:98-162).

Parameters stay where they are (engine graphs and the packed weight images depend on their addresses); exp_avg /
exp_avg_sq (SGD: the momentum buffer) live in two flat buffers owned by the optimizer, each tensor's slice starting on a
16-byte boundary; the step count of every tensor is a host integer.  The kernel writes through raw pointers, so after a step
the version counters of the updated parameters are advanced by hand (every image that ops._cached keeps per parameter goes
stale, as after a stock step) and utils.Optimizer.step rebuilds the registered MFMA images with ops.refresh_packed(force=True)."""
import ctypes as C

import torch
from torch import optim

from . import _lib as L

_STOCK = {"adam": optim.Adam, "adamw": optim.AdamW, "sgd": optim.SGD}


def chunk_elems() -> int:
    return L.load().lgcn_opt_chunk_elems()


def chunk_rows(sizes, chunk):
    """The chunk table of tensors with `sizes` elements: [(tensor id, first element)], every element of every tensor in
    exactly one chunk of at most `chunk` elements, in order; an empty tensor has no chunk."""
    return [(t, first) for t, n in enumerate(sizes) for first in range(0, n, chunk)]


def eligible(params) -> bool:
    """What FusedOptim takes: CUDA fp32 contiguous parameters on one device."""
    params = list(params)
    return bool(params) and all(p.is_cuda and p.dtype == torch.float32 and p.is_contiguous() and p.device == params[0].device
                                for p in params)


class _Segment:
    """The tensors of one parameter group that share a step count: one launch."""
    __slots__ = ("group", "ids", "step", "table", "chunks", "n_chunks")


class FusedOptim:
    """The surface of a torch.optim optimizer that utils.Optimizer and train_dp.py use -- param_groups, step(), zero_grad(),
    state_dict(), load_state_dict() -- with state_dict() in torch.optim's own format, so that a checkpoint written on either
    path resumes on the other.  kind: "adam" | "adamw" | "sgd"; groups and hyper as for the torch.optim constructor.
    amsgrad, maximize, Nesterov and dampening are not implemented: a group that asks for one is an error in step()."""

    def __init__(self, groups, kind, **hyper):
        if kind not in _STOCK:
            raise L.LgcnError("FusedOptim: kind must be 'adam', 'adamw' or 'sgd'")
        self.kind = kind
        self.param_groups = _STOCK[kind](groups, **hyper).param_groups      # the stock keys and defaults; "params": tensors
        self.params = [p for g in self.param_groups for p in g["params"]]
        self._group_of = [gi for gi, g in enumerate(self.param_groups) for _ in g["params"]]
        if not eligible(self.params):
            raise L.LgcnError("FusedOptim: every parameter must be a contiguous CUDA fp32 tensor on one device")
        self.chunk = chunk_elems()
        self._off, total = [], 0
        for p in self.params:
            self._off.append(total)
            total += (p.numel() + 3) // 4 * 4                               # every slice starts on a 16-byte boundary
        dev = self.params[0].device
        self.m = torch.zeros(total, dtype=torch.float32, device=dev)        # exp_avg | momentum_buffer
        self.v = torch.zeros(total if kind != "sgd" else 0, dtype=torch.float32, device=dev)      # exp_avg_sq
        self.steps = [0] * len(self.params)                                 # SGD: 0 until the tensor has a momentum buffer
        self._key, self._segments = None, []

    # ------------------------------------------------------------------ state slices
    def _slice(self, buf, i):
        p = self.params[i]
        return buf[self._off[i]:self._off[i] + p.numel()].view_as(p)

    # ------------------------------------------------------------------ tables
    def _build(self, key):
        """Device tables of the tensors that have a gradient, one segment per (group, step count)."""
        sgd = self.kind == "sgd"
        by_seg = {}
        for i, k in enumerate(key):
            if k is None:
                continue                                                    # no gradient: left out of this step, like torch.optim
            p, g = self.params[i], self.params[i].grad
            if not (g.is_cuda and g.dtype == torch.float32 and g.is_contiguous() and g.numel() == p.numel() and g.device == p.device):
                raise L.LgcnError("FusedOptim: the gradient of parameter %d is not a contiguous CUDA fp32 tensor of its shape" % i)
            by_seg.setdefault((self._group_of[i], min(self.steps[i], 1) if sgd else self.steps[i]), []).append(i)
        self._segments = []
        m0, v0 = self.m.data_ptr(), self.v.data_ptr() if not sgd else 0
        for (gi, _), ids in sorted(by_seg.items()):
            s = _Segment()
            s.group, s.ids, s.step = gi, ids, self.steps[ids[0]]
            rows = [[key[i][0], key[i][1], m0 + 4 * self._off[i], v0 + 4 * self._off[i] if not sgd else 0, self.params[i].numel()]
                    for i in ids]
            chunks = chunk_rows([r[4] for r in rows], self.chunk)
            s.n_chunks = len(chunks)
            dev = self.m.device
            s.table = torch.tensor(rows, dtype=torch.int64).to(dev)
            s.chunks = torch.tensor(chunks, dtype=torch.int32).reshape(-1, 2).to(dev)
            self._segments.append(s)
        self._key = key

    # ------------------------------------------------------------------ the torch.optim surface
    def step(self, clip=None):
        """One update of every parameter that has a gradient.  clip: (low, high) clamps the gradients first, in place, in
        the same launch.  Enqueued on the current stream; no synchronisation, no host read of device memory and, while
        the set of (parameter, gradient) addresses stays what it was, no host-to-device copy."""
        key = [None if g is None else (p.data_ptr(), g.data_ptr()) for p, g in ((p, p.grad) for p in self.params)]
        if key != self._key:
            self._build(key)
        lib = L.load()
        stream = C.c_void_p(torch._C._cuda_getCurrentRawStream(torch._C._cuda_getDevice()))
        kind = L.OPT_KINDS[self.kind]
        clip_on, lo, hi = (0, 0.0, 0.0) if clip is None else (1, float(clip[0]), float(clip[1]))
        stepped = []
        for s in self._segments:
            g = self.param_groups[s.group]
            if g.get("amsgrad") or g.get("maximize") or g.get("nesterov") or g.get("dampening"):
                raise L.LgcnError("FusedOptim: amsgrad, maximize, nesterov and dampening are not implemented")
            t = float(s.step + 1)
            if self.kind == "sgd":
                b1 = b2 = eps = 0.0
                bc1 = bc2 = 1.0
                mom = float(g["momentum"])
            else:
                b1, b2 = g["betas"]
                eps, mom = float(g["eps"]), 0.0
                bc1, bc2 = 1 - b1 ** t, 1 - b2 ** t                          # as torch.optim: Python floats
            if s.n_chunks:
                L.check(lib.lgcn_opt_step(s.table.data_ptr(), len(s.ids), s.chunks.data_ptr(), s.n_chunks, kind, float(g["lr"]),
                                          float(b1), float(b2), eps, float(g["weight_decay"]), mom, int(s.step == 0), bc1, bc2,
                                          clip_on, lo, hi, stream), "lgcn_opt_step")
            s.step += 1
            for i in s.ids:
                self.steps[i] = s.step
            stepped += [self.params[i] for i in s.ids]
        if stepped:
            torch.autograd.graph.increment_version(stepped)                 # written through raw pointers: say so

    def zero_grad(self, set_to_none: bool = True):
        for p in self.params:
            if p.grad is not None:
                if set_to_none:
                    p.grad = None
                else:
                    p.grad.detach_().requires_grad_(False).zero_()

    def state_dict(self):
        """torch.optim's format: state[i] = {"step", "exp_avg", "exp_avg_sq"} | {"momentum_buffer"} of every tensor that
        has been stepped (copies), and param_groups with the stock keys and "params" as indices."""
        groups, start = [], 0
        for g in self.param_groups:
            d = {k: v for k, v in g.items() if k != "params"}
            d["params"] = list(range(start, start + len(g["params"])))
            start += len(g["params"])
            groups.append(d)
        state = {}
        for i, t in enumerate(self.steps):
            if t == 0:
                continue
            if self.kind == "sgd":
                if self.param_groups[self._group_of[i]]["momentum"] != 0:
                    state[i] = {"momentum_buffer": self._slice(self.m, i).clone()}
            else:
                state[i] = {"step": torch.tensor(float(t), dtype=torch.float32), "exp_avg": self._slice(self.m, i).clone(),
                            "exp_avg_sq": self._slice(self.v, i).clone()}
        return {"state": state, "param_groups": groups}

    def load_state_dict(self, sd):
        """A state_dict of this class or of the torch.optim optimizer of the same kind over the same parameters."""
        saved = sd["param_groups"]
        if len(saved) != len(self.param_groups) or any(len(a["params"]) != len(b["params"]) for a, b in zip(saved, self.param_groups)):
            raise ValueError("loaded state dict has different parameter groups")
        index = {}
        for a, b in zip(saved, self.param_groups):
            for old, new in zip(a["params"], range(len(index), len(index) + len(a["params"]))):
                index[old] = new
            b.update({k: v for k, v in a.items() if k != "params"})
        self.m.zero_()
        self.v.zero_()
        self.steps = [0] * len(self.params)
        for old, st in sd["state"].items():
            i = index[old]
            if self.kind == "sgd":
                buf = st.get("momentum_buffer")
                if buf is not None:
                    self._slice(self.m, i).copy_(buf)
                    self.steps[i] = 1
            else:
                self._slice(self.m, i).copy_(st["exp_avg"])
                self._slice(self.v, i).copy_(st["exp_avg_sq"])
                self.steps[i] = int(round(float(st["step"])))
        self._key = None                                                    # the grouping by step count may have changed
