"""CPU: the float64 model of LanePooling's pair stage (tests/pool_pairs_model.py) reproduces the reference's own capture
pool/out of lanercnn_b3.npz, which pins the formula of lgcn_pool_pairs before any kernel is compared with it; the entry
point is exported and bound and refuses bad arguments before launching anything; ops.pool_pairs has no CPU path;
LanePooling.fused exists and is off by default."""
import json
import os

import numpy as np
import pytest
import torch

import pool_pairs_model as PM
from conftest import GOLDEN_DIR
from oracle import lanercnn_oracle as OR
from test_lanercnn import inputs

EINVAL, ESHAPE, EALIGN = -1, -2, -3
NAMES = ("ctx_pose", "tgt_pose", "ti", "ci", "n_pairs", "wp", "bp", "wpc0h", "U", "g", "bt", "m")


@pytest.fixture(scope="module")
def lib():
    import lanegcn_amd  # noqa: F401
    from lanegcn_amd import _lib
    return _lib.load(), _lib


def test_model_reproduces_reference_capture():
    with np.load(os.path.join(GOLDEN_DIR, "lanercnn_b3.npz")) as z:
        g = {k: z[k] for k in z.files}
    names = json.load(open(os.path.join(GOLDEN_DIR, "lanercnn_state_names.json")))
    sd = OR.seeded_state([(k, tuple(s)) for k, s in names["pool"]], int(g["seed"]) + 2)
    sd = {"pool." + k: v for k, v in sd.items()}
    _, _, ctx_g, tgt_g, _ = inputs(g)
    out, ci, ti = PM.lane_pooling(torch.from_numpy(g["pool/cfeat"]), ctx_g, torch.from_numpy(g["pool/tfeat"]), tgt_g, sd)
    assert np.array_equal(ti.numpy(), g["pool/wi"])                # the index the reference's index_add_ received
    # rel_err of test_gpu_training.py: max |got - ref| / max |ref|.  The capture is the reference's own fp32 result with
    # values up to 6.3, where one fp32 ulp is 4.8e-7: the bar of 1e-6 is read in that measure (the absolute difference,
    # printed too, is 1.4e-6 = 3 ulp of the capture).
    want = torch.from_numpy(g["pool/out"]).double()
    e_abs = float((out - want).abs().max())
    e = e_abs / float(want.abs().max())
    print("float64 model against pool/out: rel_err %.3e (max |delta| %.3e) over %d pairs" % (e, e_abs, len(ti)))
    assert out.dtype == torch.float64 and e <= 1e-6


def test_pair_stage_is_the_reference_lines():
    """pair_stage against the reference's own composition (cat, one Linear over 256 columns) in float64."""
    r = torch.Generator().manual_seed(3)
    n_c, n_t, P = 9, 5, 40
    cp, tp = torch.randn(n_c, 4, generator=r), torch.randn(n_t, 4, generator=r)
    ci, ti = torch.randint(n_c, (P,), generator=r), torch.randint(n_t, (P,), generator=r)
    wp, bp = torch.randn(128, 4, generator=r).double(), torch.randn(128, generator=r).double()
    w0 = torch.randn(128, 256, generator=r).double() / 16
    g, bt = 1 + 0.1 * torch.randn(128, generator=r).double(), 0.1 * torch.randn(128, generator=r).double()
    cf = torch.randn(n_c, 128, generator=r).double()
    got = PM.pair_stage(cp, tp, ti, ci, wp, bp, w0[:, 128:], cf @ w0[:, :128].t(), g, bt)
    d = torch.relu(torch.nn.functional.linear((cp[ci] - tp[ti]).double(), wp, bp))
    want = torch.relu(torch.nn.functional.group_norm(torch.nn.functional.linear(torch.cat([cf[ci], d], -1), w0), 1, g, bt, 1e-5))
    assert float((got - want).abs().max()) <= 1e-12


def test_symbol_is_exported_and_bound(lib):
    l, mod = lib
    assert hasattr(l, "lgcn_pool_pairs"), "liblgcn.so does not export lgcn_pool_pairs"
    assert "lgcn_pool_pairs" in mod.SIGNATURES
    header = open(os.path.join(os.path.dirname(GOLDEN_DIR), os.pardir, "include", "lgcn.h")).read()
    assert "int lgcn_pool_pairs(" in header and "lanercnn.py:492-499" in header


def test_validates_before_launching(lib):
    l, _ = lib

    def call(cap=64, **kw):
        a = {n: 256 for n in NAMES}
        a.update(kw)
        return l.lgcn_pool_pairs(a["ctx_pose"], a["tgt_pose"], a["ti"], a["ci"], a["n_pairs"], cap,
                                 *(a[n] for n in NAMES[5:11]), 1e-5, a["m"], None)

    assert call(cap=0) == 0                                          # nothing to do: no launch
    assert call(cap=0, m=None) == 0
    assert call(cap=-1) == EINVAL
    assert call(cap=1 << 40) == ESHAPE and call(cap=0x7ffffff1) == ESHAPE
    for n in NAMES:
        assert call(**{n: None}) == EINVAL, n
    for n in ("ctx_pose", "tgt_pose") + NAMES[5:]:                    # pose rows are read as one 16-byte load
        assert call(**{n: 260}) == EALIGN, n


def test_ops_has_no_cpu_path(lib):
    _, mod = lib
    from lanegcn_amd import ops
    i32 = lambda *v: torch.tensor(v, dtype=torch.int32)
    ps = ops.PairSet(i32(0, 1), i32(1, 0), i32(2), i32(0, 1, 2), 2, 2, torch.zeros(2, 2), torch.zeros(2, 2))
    z = torch.zeros
    with pytest.raises(mod.LgcnError):
        ops.pool_pairs(ps, z(2, 4), z(2, 4), z(128, 4), z(128), z(128, 256), z(2, 128), (torch.ones(128), z(128)))


def test_fused_is_opt_in():
    import lanegcn_amd  # noqa: F401
    from lanegcn_amd import lanercnn as R
    assert R.LanePooling.fused is False
