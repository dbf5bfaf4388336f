"""lgcn_att_pairs_wi (8-wave workgroups, one weight in LDS per phase) against the exact-f32 pair kernel lgcn_att_pairs
on synthetic pair sets: empty sets, counts just below and above multiples of 16 and of a workgroup's 8 blocks,
overflowed (negative) and too-large counts, seg = 0 and seg = 16 (per-target sums of the 16-aligned pieces)."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

C = 128
N_AGT, N_CTX = 61, 47


@pytest.fixture(scope="module")
def ops():
    import lanegcn_amd  # noqa: F401
    from lanegcn_amd import ops as o
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return o


@pytest.fixture(scope="module")
def weights():
    g = torch.Generator().manual_seed(7)

    def rn(*s, scale=1.0):
        return (torch.randn(*s, generator=g) * scale).cuda()

    gn = lambda: (1.0 + rn(C, scale=0.1), rn(C, scale=0.1))      # noqa: E731
    return dict(wd0=rn(C, 2, scale=0.7), bd0=rn(C, scale=0.1), wd2=rn(C, C, scale=C ** -0.5), gn_d=gn(),
                wc0=rn(C, 3 * C, scale=C ** -0.5), U=rn(N_AGT, C), V=rn(N_CTX, C), gn_c=gn())


def pair_set(ops, cap, stored, seed):
    """cap sorted targets (runs of 1-40 pairs per target, like the pair search's output) and random contexts; n_pairs
    holds `stored` (negative / above cap = overflowed: the kernels then take all cap rows)."""
    rng = np.random.default_rng(seed)
    runs = []
    while sum(runs) < cap:
        runs.append(int(rng.integers(1, 41)))
    hi = np.repeat(np.arange(len(runs)) % N_AGT, runs)[:cap]
    hi.sort(kind="stable")
    wi = rng.integers(0, N_CTX, cap)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.int32)).cuda()      # noqa: E731
    return ops.PairSet(hi=t(hi), wi=t(wi), n_pairs=t([stored]), rowptr=t([0]), cap=cap, n_agt=N_AGT,
                       agt_ctrs=torch.from_numpy(rng.normal(0, 20, (N_AGT, 2)).astype(np.float32)).cuda(),
                       ctx_ctrs=torch.from_numpy(rng.normal(0, 20, (N_CTX, 2)).astype(np.float32)).cuda())


def run(ops, ps, w, mma, seg=0, m=None):
    with ops.mma_scope(mma):
        return ops.att_pairs(ps, w["wd0"], w["bd0"], (w["wd2"], 0), w["gn_d"], (w["wc0"], 0), w["U"], w["V"],
                             w["gn_c"], m=m, seg=seg)


# (pairs stored in n_pairs, cap); stored < 0 or > cap: overflowed; 70,001 pairs: several rounds per workgroup
CASES = [(0, 64), (15, 40), (17, 40), (127, 160), (129, 160), (255, 300), (257, 300), (2047, 2100), (2049, 2100),
         (-5, 300), (-1, 129), (500, 333), (70001, 70100)]


@pytest.mark.parametrize("mma,bar", [("f16x2", 1e-4), ("bf16", 2e-2)])
@pytest.mark.parametrize("stored,cap", CASES)
def test_att_pairs_wi_matches_f32_kernel(ops, weights, mma, bar, stored, cap):
    ps = pair_set(ops, cap, stored, seed=cap * 31 + stored % 97)
    P = cap if stored < 0 or stored > cap else stored
    fill = 7777.0
    ref = run(ops, ps, weights, "f32", m=torch.full((cap, C), fill, device="cuda")).cpu().numpy().astype(np.float64)
    got = run(ops, ps, weights, mma, m=torch.full((cap, C), fill, device="cuda")).cpu().numpy()
    assert (got[P:] == fill).all() and (ref[P:] == fill).all()
    if P:
        scale = max(1.0, float(np.abs(ref[:P]).max()))
        assert float(np.abs(got[:P] - ref[:P]).max()) <= bar * scale
    # seg = 16: every piece (a run of one target inside a 16-aligned block) summed at its first row, nothing else written
    seg = run(ops, ps, weights, mma, seg=16, m=torch.full((cap, C), fill, device="cuda")).cpu().numpy()
    hi = ps.hi[:P].cpu().numpy()
    first = np.ones(P, bool)
    first[1:] = (hi[1:] != hi[:-1]) | (np.arange(1, P) % 16 == 0)
    starts = np.flatnonzero(first)
    untouched = np.ones(cap, bool)
    untouched[starts] = False
    assert (seg[untouched] == fill).all()
    if P:
        want = np.add.reduceat(ref[:P], starts, axis=0)
        assert float(np.abs(seg[starts] - want).max()) <= bar * max(1.0, float(np.abs(want).max()))


def test_att_pairs_wi_empty_capacity(ops, weights):
    """cap = 0: nothing is launched and nothing is written."""
    ps = pair_set(ops, 0, 0, seed=1)
    for seg in (0, 16):
        m = torch.full((1, C), 5.0, device="cuda")
        run(ops, ps, weights, "f16x2", seg=seg, m=m)
        assert (m.cpu() == 5.0).all()
