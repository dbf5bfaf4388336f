"""CPU: the training entry points of LanePooling's pair stage (lgcn_pool_pairs_train, lgcn_pool_pairs_bwd and its
workspace helper) are exported, bound and declared in the header, the ctypes struct mirrors the header's, and null and
misaligned pointers, a negative or oversized capacity, an out-of-range chunk count and a missing workspace are refused
before anything is launched (no GPU needed).  LanePooling.train_hip exists and is off by default, and the float64 model
of the training (tests/pool_train_model.py) with the pre-activations' own signs as masks is pool_pairs_model.pair_stage."""
import ctypes as C
import os
import re

import pytest
import torch

import pool_pairs_model as PM
import pool_train_model as TM

EINVAL, ESHAPE, EALIGN = -1, -2, -3
NEW = ("lgcn_pool_pairs_train", "lgcn_pool_pairs_bwd_ws_elems", "lgcn_pool_pairs_bwd")
REC = 128 * 128 + 7 * 128              # floats of one chunk record: dW_0h and seven [128] vectors; the design adds nothing
HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "lgcn.h")


@pytest.fixture(scope="module")
def lib():
    import lanegcn_amd  # noqa: F401
    from lanegcn_amd import _lib
    return _lib.load(), _lib


def test_training_symbols_are_exported_bound_and_declared(lib):
    l, mod = lib
    text = open(HEADER).read()
    for n in NEW:
        assert hasattr(l, n), "liblgcn.so does not export " + n
        assert n in mod.SIGNATURES
        assert re.search(r"\b%s\(" % n, text), "include/lgcn.h does not declare " + n
    assert l.lgcn_version() == 100


def test_train_hip_is_opt_in():
    import lanegcn_amd  # noqa: F401
    from lanegcn_amd import lanercnn as R
    assert R.LanePooling.train_hip is False


def header_fields():
    """(type, name) of every member of lgcn_pool_pairs_bwd_t, in the header's order."""
    text = open(HEADER).read()
    body = re.search(r"typedef struct \{([^}]*)\} lgcn_pool_pairs_bwd_t;", text).group(1)
    fields = []
    for decl in body.split(";"):
        decl = decl.strip()
        if not decl:
            continue
        base = re.match(r"(const\s+)?(\w+)", decl).group(2)
        for part in decl[re.match(r"(const\s+)?\w+", decl).end():].split(","):
            part = part.strip()
            fields.append(("ptr" if part.startswith("*") else base, part.lstrip("*").strip()))
    return fields


def test_struct_layout_matches_header(lib):
    _, mod = lib
    fields = header_fields()
    size = {"ptr": 8, "int64_t": 8, "float": 4, "int32_t": 4}
    assert [n for n, _ in mod.PoolPairsBwd._fields_] == [n for _, n in fields]
    off = 0
    for kind, name in fields:
        off = (off + size[kind] - 1) // size[kind] * size[kind]
        f = getattr(mod.PoolPairsBwd, name)
        assert (f.offset, f.size) == (off, size[kind]), name
        off += size[kind]
    # 5 pointers, cap, 16 pointers, eps, n_chunks
    assert mod.PoolPairsBwd.cap.offset == 5 * 8 and mod.PoolPairsBwd.eps.offset == 22 * 8
    assert C.sizeof(mod.PoolPairsBwd) == (off + 7) // 8 * 8 == 23 * 8


def test_workspace_helper(lib):
    l, _ = lib
    ws = l.lgcn_pool_pairs_bwd_ws_elems
    assert ws(0, 1) == 0 and ws(0, 1024) == 0
    # one record per workgroup, never more workgroups than 32-pair tiles
    assert ws(1, 1) == REC and ws(32, 8) == REC and ws(33, 8) == 2 * REC and ws(130, 3) == 3 * REC and ws(130, 8) == 5 * REC
    assert ws(100000, 256) == 256 * REC and ws(0x7ffffff0, 1024) == 1024 * REC
    assert ws(-1, 4) < 0 and ws(1 << 40, 4) < 0 and ws(0x7ffffff1, 4) < 0
    assert ws(64, 0) < 0 and ws(64, -1) < 0 and ws(64, 1025) < 0


def test_pairs_train_validates_before_launching(lib):
    l, _ = lib
    names = ("ctx_pose", "tgt_pose", "ti", "ci", "n_pairs", "wp", "bp", "wpc0h", "U", "g", "bt", "m", "masks")

    def call(cap=64, **kw):
        a = {n: 256 for n in names}
        a.update(kw)
        return l.lgcn_pool_pairs_train(a["ctx_pose"], a["tgt_pose"], a["ti"], a["ci"], a["n_pairs"], cap,
                                       *(a[n] for n in names[5:11]), 1e-5, a["m"], a["masks"], None)

    assert call(cap=0) == 0                                              # nothing to do: no launch
    assert call(cap=-1) == EINVAL and call(cap=1 << 40) == ESHAPE and call(cap=0x7ffffff1) == ESHAPE
    for n in names:
        assert call(**{n: None}) == EINVAL, n
    for n in names[:2] + names[5:]:
        assert call(**{n: 260}) == EALIGN, n


def test_pairs_bwd_validates_before_launching(lib):
    l, mod = lib
    required = ("ctx_pose", "tgt_pose", "ti", "ci", "n_pairs", "wp", "bp", "wpc0h", "U", "g", "bt", "masks", "dS")
    outs = ("d_w0h", "d_wp", "d_bp", "d_g", "d_bt")

    def call(cap=64, n_chunks=2, **kw):
        q = mod.PoolPairsBwd()
        for n in required + outs + ("wptc0h", "dz", "ws"):
            setattr(q, n, 256)
        q.cap, q.n_chunks, q.eps = cap, n_chunks, 1e-5
        for k, v in kw.items():
            setattr(q, k, v)
        return l.lgcn_pool_pairs_bwd(C.byref(q), None)

    assert l.lgcn_pool_pairs_bwd(None, None) == EINVAL
    assert call(cap=0) == 0                                              # nothing to do: no launch
    assert call(cap=-1) == EINVAL and call(cap=1 << 40) == ESHAPE and call(cap=0x7ffffff1) == ESHAPE
    assert call(n_chunks=0) == EINVAL and call(n_chunks=-3) == EINVAL and call(n_chunks=1025) == EINVAL
    for n in required:
        assert call(**{n: None}) == EINVAL, n
    # the transposed image and the workspace are required by the outputs that need them
    assert call(wptc0h=None) == EINVAL and call(ws=None) == EINVAL
    for only in outs:
        assert call(ws=None, **{n: None for n in outs if n != only}) == EINVAL, only
    for n in required[:2] + required[5:] + outs + ("wptc0h", "dz", "ws"):
        assert call(**{n: 260}) == EALIGN, n
    # every output absent: nothing to compute, no launch
    assert call(dz=None, ws=None, wptc0h=None, **{n: None for n in outs}) == 0


@pytest.mark.parametrize("scale", [0.1, 1.0, 8.0])
def test_model_with_true_masks_is_the_inference_model(scale):
    T, S, P = 9, 11, 130
    g = torch.Generator().manual_seed(7)
    ti, ci = torch.sort(torch.randint(T, (P,), generator=g))[0], torch.randint(S, (P,), generator=g)
    grid = lambda n: torch.randint(256, (n, 4), generator=g).float() / 64
    tgt_pose, ctx_pose = grid(T), grid(S)
    rn = lambda *shape, fan: torch.randn(*shape, generator=g) * (scale * 1.5 / fan ** 0.5)
    inp = dict(wp=rn(128, 4, fan=4), bp=rn(128, fan=4), w0h=rn(128, 128, fan=256), U=torch.randn(S, 128, generator=g) * scale,
               g=1 + 0.1 * (2 * torch.rand(128, generator=g) - 1), bt=0.1 * torch.randn(128, generator=g))
    masks = TM.true_masks(ctx_pose, tgt_pose, ti, ci, inp)
    m, Sx = TM.forward(ctx_pose, tgt_pose, ti, ci, inp, masks, T)
    want = PM.pair_stage(ctx_pose, tgt_pose, ti, ci, inp["wp"], inp["bp"], inp["w0h"], inp["U"], inp["g"], inp["bt"])
    assert torch.equal(m, want)
    assert torch.equal(Sx, torch.zeros(T, 128, dtype=torch.float64).index_add(0, ti, want))
    # and its autograd step returns every gradient, finite
    dS = torch.randn(T, 128, generator=g)
    S2, grads, _ = TM.train_step(ctx_pose, tgt_pose, ti, ci, inp, masks, dS)
    assert torch.equal(S2, Sx)
    assert set(grads) == set(TM.NAMES) | {"dz"} and all(bool(torch.isfinite(v).all()) for v in grads.values())
    assert grads["wp"].shape == (128, 4) and grads["dz"].shape == (P, 128) and grads["U"].shape == (S, 128)
