"""GPU: the fused optimizer step (lgcn_opt_step; optim_hip.FusedOptim; utils.Optimizer.train_hip) -- the update of every kind
against the float64 rule at a bar taken from torch.optim on the device, parameter groups, a parameter without a gradient,
non-finite gradients, repeatability and untouched neighbours, checkpoints interchangeable with torch.optim in both directions,
fresh weight images after a step, and one step of the whole Net with and without a flat gradient bucket.

Every comparison runs three sides on the SAME supplied gradients: the float64 numpy rule (ref_step of
tests/test_host_opt_cabi.py, checked there against torch.optim in float64), torch.optim on the device ("stock") and
FusedOptim.  No test compares two free-running training loops: Adam's g / (|g| + eps) amplifies rounding-level differences
of near-zero gradients, which makes such a comparison ill-conditioned even for the stock path against itself.
Errors are rel_err = max |got - ref| / max |ref| per tensor of p, exp_avg / momentum buffer (m), exp_avg_sq (v) and of the
update p_after - p_before (relative to its own maximum: an error of the update is otherwise hidden by |p| >> lr); the bar is
bar(e_stock) = min(max(2 e_stock, 1e-6), 1e-4), e_stock the stock side's error against the same reference (the rule of
tests/test_gpu_rowblock_train.py).  All are printed before anything is asserted (by check_rows of the LaneConv test: its
column "composed" is the stock side here).

Sizes (c = lgcn_opt_chunk_elems()): 5, c + 1, 2 c + 5, 3, 127, 128, c, 0 and 1 elements -- one 16-byte access and a tail
(the only tensor whose four pointers are all aligned), one element into the second chunk, three chunks with a tail of 5, below
one 16-byte access, a ragged and a whole number of accesses, a full chunk, nothing, and a single element.  Gradients are views
of one flat buffer laid out back to back (0, 4, 8, 12, 8, 4, 4, -, 4 bytes off a 16-byte boundary), parameters views of
allocations of their own with guard elements on both sides, the 128-element one 4 bytes off.

Conditioning of the update's error: p_after - p_before carries half a unit in the last place of p whatever computes it, and
with one- and three-element tensors "its own maximum" is a single entry, so no entry's update may be a cancellation residue.
Parameters are N(0, 0.005) (half a unit: at most 2e-9 once they have moved), every gradient entry keeps its sign from step to
step and has magnitude 2e-3 (0.25 + |N(0, 1)|) >= 5e-4 (the clamp to (-1e-3, 1e-3) binds on both sides and leaves a fifth of
the entries alone), lr is 1e-2 (Adam kinds) or 1.0 (SGD), 0.3 of that from step 3, 0.1 of that in a second group: the
smallest update is 1.5e-5 (SGD, second group: 0.03 x 5e-4), half a unit below 1e-4 of it and far below the others."""
import numpy as np
import pytest
import torch

import test_gpu_training as TG
from golden_io import load_scenes
from test_gpu_laneconv_train import check_rows, randomize, same_bits
from test_host_opt_cabi import HYPER, KIND_OF, ref_kwargs, ref_state, ref_step, stock_optimizer

pytestmark = pytest.mark.gpu

GUARD = -7.5
CLIP = (-1e-3, 1e-3)
STEPS = 5


class Mods:
    pass


@pytest.fixture(scope="module")
def mods():
    import lanegcn_amd  # noqa: F401
    from lanegcn_amd import _lib, autograd, dist, lanegcn, layers, ops, optim_hip, utils
    m = Mods()
    m.L, m.A, m.dist, m.M, m.layers, m.ops, m.OH, m.utils = _lib, autograd, dist, lanegcn, layers, ops, optim_hip, utils
    return m


@pytest.fixture
def launches(mods, monkeypatch):
    """A list that grows by one with every lgcn_opt_step call through the ctypes binding: its n_chunks."""
    lib = mods.L.load()
    calls, real = [], lib.lgcn_opt_step

    def counted(*a):
        calls.append(a[3])
        return real(*a)

    monkeypatch.setattr(lib, "lgcn_opt_step", counted)
    return calls


def sizes_of(mods):
    c = mods.OH.chunk_elems()
    return [5, c + 1, 2 * c + 5, 3, 127, 128, c, 0, 1]


def lr_of(name, step):
    """lr changes at step 3 (step counts from 0 here)."""
    a = 1.0 if KIND_OF[name] == "sgd" else 1e-2
    return a if step < 2 else 0.3 * a


def inputs(sizes, seed, steps=STEPS):
    rng = np.random.default_rng(seed)
    p0 = [(rng.normal(0, 1, n) * 0.005).astype(np.float32) for n in sizes]
    sign = [np.where(rng.random(n) < 0.5, -1.0, 1.0) for n in sizes]
    grads = [[(s * (0.25 + np.abs(rng.normal(0, 1, n))) * 2e-3).astype(np.float32) for s, n in zip(sign, sizes)] for _ in range(steps)]
    return p0, grads


def rel(got, ref):
    """max |got - ref| / max |ref| over the entries where ref is finite; 0 for an empty tensor."""
    got, ref = np.asarray(got, dtype=np.float64).ravel(), np.asarray(ref, dtype=np.float64).ravel()
    ok = np.isfinite(ref)
    if not ok.any():
        return 0.0
    d, s = np.abs(got[ok] - ref[ok]).max(), np.abs(ref[ok]).max()
    if not np.isfinite(d):
        return float("inf")
    return float(d / s) if s > 0 else (0.0 if d == 0 else float("inf"))


class Side:
    """One device side, "stock" (torch.optim) or "fused" (FusedOptim), over parameters with guard elements around each and
    gradients that are back-to-back views of one flat buffer (guards at its ends)."""

    def __init__(self, mods, side, name, p0, split=None):
        self.side, self.name, self.ps, self.bufs = side, name, [], []
        for i, x in enumerate(p0):
            lead = 9 if i == 5 else 8                                   # one parameter 4 bytes off a 16-byte boundary
            b = torch.full((lead + x.size + 8,), GUARD, device="cuda")
            b[lead:lead + x.size] = torch.from_numpy(x).cuda()
            self.ps.append(torch.nn.Parameter(b[lead:lead + x.size]))
            self.bufs.append((b, lead, x.size))
        total = sum(x.size for x in p0)
        self.gflat = torch.full((8 + total + 8,), GUARD, device="cuda")
        self.gviews, off = [], 8
        for x in p0:
            self.gviews.append(self.gflat[off:off + x.size])
            off += x.size
        split = len(p0) if split is None else split
        groups = [{"params": g, "lr": 0} for g in (self.ps[:split], self.ps[split:]) if g]
        h = HYPER[name]
        if side == "stock":
            self.opt = stock_optimizer(name, groups)
        else:
            kw = dict(momentum=h["momentum"], weight_decay=h["wd"]) if KIND_OF[name] == "sgd" else dict(weight_decay=h["wd"])
            self.opt = mods.OH.FusedOptim(groups, KIND_OF[name], **kw)

    def step(self, grads, lrs, clip=None):
        for p, v, g in zip(self.ps, self.gviews, grads):
            if g is None:
                p.grad = None
            else:
                v.copy_(torch.from_numpy(g))
                p.grad = v
        for g, a in zip(self.opt.param_groups, lrs):
            g["lr"] = a
        if self.side == "fused":
            self.opt.step(clip=clip)
            return
        if clip is not None:
            for p in self.ps:
                if p.grad is not None:
                    p.grad.data.clamp_(*clip)
        self.opt.step()

    def state(self, i):
        """(m, v) of parameter i, None where the optimizer keeps none."""
        if self.side == "stock":
            st = self.opt.state.get(self.ps[i], {})
            return st.get("exp_avg", st.get("momentum_buffer")), st.get("exp_avg_sq")
        o = self.opt
        if o.steps[i] == 0 or (o.kind == "sgd" and not HYPER[self.name]["momentum"]):
            return None, None
        return o._slice(o.m, i), (o._slice(o.v, i) if o.kind != "sgd" else None)

    def snap(self):
        f = lambda t: None if t is None else t.detach().cpu().double().numpy().copy()
        mv = [self.state(i) for i in range(len(self.ps))]
        return dict(p=[f(p) for p in self.ps], m=[f(m) for m, _ in mv], v=[f(v) for _, v in mv],
                    g=[f(p.grad) for p in self.ps])

    def guards_ok(self):
        ok = all(bool((b[:lead] == GUARD).all()) and bool((b[lead + n:] == GUARD).all()) for b, lead, n in self.bufs)
        return ok and bool((self.gflat[:8] == GUARD).all()) and bool((self.gflat[-8:] == GUARD).all())


def rows_of(label, before, fused, stock, ref, ref_before):
    """(name, e_fused, e_stock) of p, m, v and the update of every tensor; a state that the reference rule does not have
    (SGD without momentum) must be absent on both sides."""
    rows = []
    for i in range(len(ref["p"])):
        if ref["p"][i].size == 0:
            continue
        rows.append(("%s p[%d]" % (label, i), rel(fused["p"][i], ref["p"][i]), rel(stock["p"][i], ref["p"][i])))
        rows.append(("%s upd[%d]" % (label, i), rel(fused["p"][i] - before["fused"][i], ref["p"][i] - ref_before[i]),
                     rel(stock["p"][i] - before["stock"][i], ref["p"][i] - ref_before[i])))
        for k in ("m", "v"):
            assert (fused[k][i] is None) == (stock[k][i] is None), (label, k, i)
            if fused[k][i] is not None:
                rows.append(("%s %s[%d]" % (label, k, i), rel(fused[k][i], ref[k][i]), rel(stock[k][i], ref[k][i])))
    return rows


def run_three(mods, name, clip, seed, split=None, coef=(1.0, 1.0), missing=None, steps=STEPS):
    """`steps` steps of all three sides on the same gradients: (rows, fused Side, stock Side, reference state).
    missing: (tensor, n): that tensor has no gradient in the first n steps."""
    sizes = sizes_of(mods)
    p0, grads = inputs(sizes, seed, steps)
    fused, stock = Side(mods, "fused", name, p0, split), Side(mods, "stock", name, p0, split)
    st = ref_state(KIND_OF[name], [x.astype(np.float64) for x in p0])
    n_split = len(sizes) if split is None else split
    rows = []
    for s in range(steps):
        gs = [None if missing is not None and i == missing[0] and s < missing[1] else g for i, g in enumerate(grads[s])]
        lr = lr_of(name, s)
        before = dict(fused=fused.snap()["p"], stock=stock.snap()["p"])
        ref_before = [p.copy() for p in st["p"]]
        for side in (fused, stock):
            side.step(gs, [lr * c for c in coef], clip)
        left = ref_step(st, [None if g is None else g.astype(np.float64) for g in gs],
                        [lr * (coef[0] if i < n_split else coef[1]) for i in range(len(sizes))], clip=clip, **ref_kwargs(name))
        f, k = fused.snap(), stock.snap()
        rows += rows_of("%s step %d" % (name, s + 1), before, f, k, st, ref_before)
        for i, g in enumerate(left):                                    # the gradient as the step leaves it: clamped in place
            if g is not None:
                assert np.array_equal(f["g"][i], g.astype(np.float32).astype(np.float64)), (name, s, i)
                assert np.array_equal(k["g"][i], f["g"][i])
            else:
                assert f["g"][i] is None
    return rows, fused, stock, st


# ------------------------------------------------------------------ 1. the entry against fp64
@pytest.mark.parametrize("clip", [None, CLIP], ids=["noclip", "clip"])
@pytest.mark.parametrize("name", sorted(HYPER))
def test_entry_against_fp64(mods, launches, name, clip):
    sizes = sizes_of(mods)
    c = mods.OH.chunk_elems()
    rows, fused, stock, _ = run_three(mods, name, clip, seed=11)
    assert launches == [sum((n + c - 1) // c for n in sizes)] * STEPS    # one launch per step, every chunk in it
    offs = [v.data_ptr() % 16 for v, n in zip(fused.gviews, sizes) if n]
    assert offs == [0, 4, 8, 12, 8, 4, 4, 4] and [p.data_ptr() % 16 for p, n in zip(fused.ps, sizes) if n] == [0, 0, 0, 0, 0, 4, 0, 0]
    if clip is not None:
        g = np.concatenate(inputs(sizes, 11)[1][0])
        assert (g < clip[0]).any() and (g > clip[1]).any() and ((g > clip[0]) & (g < clip[1])).any()      # both bounds bind
    assert fused.guards_ok() and stock.guards_ok()
    check_rows(rows, "clip=%s" % (clip is not None))


# ------------------------------------------------------------------ 2. parameter groups
@pytest.mark.parametrize("name", ["adam", "sgd"])
def test_two_groups_follow_their_own_lr(mods, launches, name):
    rows, fused, _, _ = run_three(mods, name, None, seed=12, split=3, coef=(1.0, 0.1))
    assert len(launches) == 2 * STEPS and all(n > 0 for n in launches)   # one launch per group and step
    assert [g["lr"] for g in fused.opt.param_groups] == [lr_of(name, STEPS - 1), lr_of(name, STEPS - 1) * 0.1]
    check_rows(rows, "groups")


def test_optimizer_wrapper_builds_the_fused_step(mods, launches):
    """utils.Optimizer with the switch on: FusedOptim, lr = lr_func(epoch) * coef, the clamp inside the launch; with the switch
    off, and by default, torch.optim as before."""
    U = mods.utils
    cfg = dict(opt="adam", lr_func=lambda e: 1e-3 if e < 1 else 1e-4, clip_grads=True, clip_low=CLIP[0], clip_high=CLIP[1])
    mk = lambda: [torch.nn.Parameter(torch.full((5,), 0.01, device="cuda")), torch.nn.Parameter(torch.full((3,), 0.02, device="cuda"))]
    assert isinstance(U.Optimizer(mk(), cfg).opt, torch.optim.Adam)
    sides = []
    for flag in (True, False):
        U.Optimizer.train_hip = flag
        try:
            ps = mk()
            opt = U.Optimizer([[ps[0]], [ps[1]]], cfg, coef=[1.0, 0.1])
        finally:
            U.Optimizer.train_hip = False
        assert isinstance(opt.opt, mods.OH.FusedOptim) == flag and opt.fused == flag
        for e in (0.0, 1.0):
            for p in ps:
                p.grad = torch.linspace(-3e-3, 3e-3, p.numel(), device="cuda")
            assert opt.step(e) == cfg["lr_func"](e)
            assert [g["lr"] for g in opt.opt.param_groups] == [cfg["lr_func"](e), cfg["lr_func"](e) * 0.1]
            assert all(float(p.grad.max()) == np.float32(1e-3) and float(p.grad.min()) == np.float32(-1e-3) for p in ps)
        sides.append(ps)
    assert len(launches) == 4
    for a, b in zip(*sides):
        assert rel(a.detach().cpu().numpy(), b.detach().cpu().numpy()) <= 1e-6


# ------------------------------------------------------------------ 3. a parameter without a gradient
@pytest.mark.parametrize("name", ["adam", "sgd"])
def test_missing_gradient(mods, launches, name):
    """Tensor 6 (one full chunk) has grad = None in steps 1-2: bitwise untouched and not counted; from step 3 it runs two
    steps behind the others -- two segments, two launches -- and matches the reference, as do the others throughout."""
    c = mods.OH.chunk_elems()
    sizes = sizes_of(mods)
    p0 = inputs(sizes, 13)[0]
    rows2, fused2, _, _ = run_three(mods, name, None, seed=13, missing=(6, 2), steps=2)
    assert torch.equal(fused2.ps[6].detach().cpu(), torch.from_numpy(p0[6])) and fused2.opt.steps[6] == 0
    assert fused2.opt.steps == [2, 2, 2, 2, 2, 2, 0, 2, 2] and fused2.state(6) == (None, None)
    assert 6 not in fused2.opt.state_dict()["state"]
    all_chunks = sum((n + c - 1) // c for n in sizes)
    assert launches == [all_chunks - 1] * 2
    del launches[:]
    rows, fused, _, _ = run_three(mods, name, None, seed=13, missing=(6, 2))
    assert fused.opt.steps == [5, 5, 5, 5, 5, 5, 3, 5, 5]
    assert launches[:2] == [all_chunks - 1] * 2 and sorted(launches[2:4]) == [1, all_chunks - 1] and len(launches) == 2 + 2 * 3
    check_rows(rows2 + rows, "missing")


# ------------------------------------------------------------------ 4. non-finite gradients
@pytest.mark.parametrize("clip", [None, CLIP], ids=["noclip", "clip"])
@pytest.mark.parametrize("name", ["adam", "adamw", "sgd"])
def test_non_finite_gradients(mods, name, clip):
    """One NaN, one +inf and one -inf gradient element (tensors 1, 4 and 0, the last in the tail behind a 16-byte access): the NaN /
    inf patterns of p, m, v and of the written-back gradient are the stock path's, every other element is within the bar."""
    sizes = sizes_of(mods)
    p0, grads = inputs(sizes, 14, 2)
    grads[0][1][100], grads[0][4][5], grads[0][0][4] = np.nan, np.inf, -np.inf
    fused, stock = Side(mods, "fused", name, p0), Side(mods, "stock", name, p0)
    st = ref_state(KIND_OF[name], [x.astype(np.float64) for x in p0])
    rows = []
    for s in range(2):
        lr = lr_of(name, s)
        with np.errstate(all="ignore"):
            ref_step(st, [g.astype(np.float64) for g in grads[s]], lr, clip=clip, **ref_kwargs(name))
        for side in (fused, stock):
            side.step(grads[s], [lr], clip)
        f, k = fused.snap(), stock.snap()
        for key in ("p", "m", "v", "g"):
            for i in range(len(sizes)):
                a, b = f[key][i], k[key][i]
                assert (a is None) == (b is None), (key, i)
                if a is None:
                    continue
                assert np.array_equal(np.isnan(a), np.isnan(b)), (name, s, key, i)
                assert np.array_equal(np.isposinf(a), np.isposinf(b)) and np.array_equal(np.isneginf(a), np.isneginf(b)), (name, s, key, i)
                if key != "g" and a.size:
                    rows.append(("%s step %d %s[%d]" % (name, s + 1, key, i), rel(a, st[key][i]), rel(b, st[key][i])))
        if s == 0:
            bad = sum(int((~np.isfinite(x)).sum()) for x in f["p"])
            assert bad == (1 if clip is not None else 3), bad           # the clamp turns the infinities into its bounds, not the NaN
            assert np.isnan(f["g"][1][100]) and np.isnan(f["p"][1][100])
    check_rows(rows, "non-finite clip=%s" % (clip is not None))


# ------------------------------------------------------------------ 5. repeatable, neighbours untouched
@pytest.mark.parametrize("name", ["adam", "sgd"])
def test_repeatable_and_neighbours_untouched(mods, name):
    sizes = sizes_of(mods)
    p0, grads = inputs(sizes, 15)
    runs = []
    for _ in range(2):
        side = Side(mods, "fused", name, p0)
        for s in range(STEPS):
            side.step(grads[s], [lr_of(name, s)], CLIP)
        torch.cuda.synchronize()
        assert side.guards_ok()
        o = side.opt
        pad = torch.ones_like(o.m, dtype=torch.bool)                    # the padding between the state slices stays zero
        for i, p in enumerate(side.ps):
            pad[o._off[i]:o._off[i] + p.numel()] = False
        assert bool((o.m[pad] == 0).all()) and (o.kind == "sgd" or bool((o.v[pad] == 0).all()))
        runs.append([p.detach().clone() for p in side.ps] + [o.m.clone(), o.v.clone(), side.gflat.clone()])
    assert all(torch.equal(a, b) for a, b in zip(*runs))


# ------------------------------------------------------------------ 6. checkpoints
@pytest.mark.parametrize("name", ["adam", "adamw", "sgd"])
def test_state_interchange_with_torch_optim(mods, name):
    """Three steps on one side, state_dict(), load_state_dict() on the other, two more steps: both directions against the
    float64 rule over all five steps, at the bar of a stock run that never changed sides."""
    sizes = sizes_of(mods)
    p0, grads = inputs(sizes, 16)
    st = ref_state(KIND_OF[name], [x.astype(np.float64) for x in p0])
    pure = Side(mods, "stock", name, p0)
    for s in range(STEPS):
        ref_step(st, [g.astype(np.float64) for g in grads[s]], lr_of(name, s), **ref_kwargs(name))
        pure.step(grads[s], [lr_of(name, s)])
    want = pure.snap()
    for first, second in (("stock", "fused"), ("fused", "stock")):
        a = Side(mods, first, name, p0)
        for s in range(3):
            a.step(grads[s], [lr_of(name, s)])
        sd = a.opt.state_dict()
        if first == "fused":
            assert sorted(sd["state"]) == [i for i in range(len(sizes))]
            assert set(sd["param_groups"][0]) == set(pure.opt.state_dict()["param_groups"][0])
            assert sd["param_groups"][0]["params"] == list(range(len(sizes)))
        b = Side(mods, second, name, [x.detach().cpu().numpy() for x in a.ps])
        b.opt.load_state_dict(sd)                                        # torch.optim accepts FusedOptim's, and the reverse
        for s in range(3, STEPS):
            b.step(grads[s], [lr_of(name, s)])
        got = b.snap()
        rows = []
        for i, n in enumerate(sizes):
            if n:
                rows.append(("%s->%s p[%d]" % (first, second, i), rel(got["p"][i], st["p"][i]), rel(want["p"][i], st["p"][i])))
                for k in ("m", "v"):
                    assert (got[k][i] is None) == (want[k][i] is None)
                    if got[k][i] is not None:
                        rows.append(("%s->%s %s[%d]" % (first, second, k, i), rel(got[k][i], st[k][i]), rel(want[k][i], st[k][i])))
        check_rows(rows, name)
        if second == "fused" and name != "sgd":
            assert b.opt.steps == [STEPS] * len(sizes)
            assert float(b.opt.state_dict()["state"][0]["step"]) == STEPS


# ------------------------------------------------------------------ 7. fresh images
def module_step(mods, mod, x0, d_out, mode):
    mod.zero_grad(set_to_none=True)
    x = x0.clone().requires_grad_(True)
    with mods.ops.mma_scope(mode):
        out = mod(x)
        out.backward(d_out)
    return [out.detach(), x.grad] + [p.grad.clone() for p in mod.parameters()]


@pytest.fixture
def block_switches(mods):
    owners = [mods.layers.LinearRes, mods.A.RowBlockFn, mods.utils.Optimizer]
    prev = [o.train_hip for o in owners]
    for o in owners:
        o.train_hip = True
    yield
    for o, p in zip(owners, prev):
        o.train_hip = p


@pytest.mark.parametrize("mode", ["f32", "bf16x3", "f16x2"])
@pytest.mark.parametrize("block", ["Linear", "LinearRes"])
def test_fresh_images_after_fused_step(mods, block_switches, launches, block, mode):
    """The kernel writes the weights through raw pointers: after Optimizer.step the module's forward, and its fused backward
    (which reads the exact-F32 transposed images whatever the mode), are bit for bit those of a fresh module loaded with its
    state_dict(), which packs every image anew."""
    M, layers = mods.M, mods.layers
    g = torch.Generator().manual_seed(31)
    make = lambda: getattr(layers, block)(128, 128, norm="GN", ng=1)
    mod = randomize(make(), 24).cuda().train()
    x0, d_out = torch.randn(130, 128, generator=g).cuda(), torch.randn(130, 128, generator=g).cuda()
    first = module_step(mods, mod, x0, d_out, mode)                      # packs every image the block uses
    before = {k: v.clone() for k, v in mod.state_dict().items()}
    opt = M.Optimizer(mod.parameters(), M.config)
    assert opt.fused
    opt.step(0.0)
    c = mods.OH.chunk_elems()
    assert launches == [sum((p.numel() + c - 1) // c for p in mod.parameters())]      # one launch for every tensor
    assert all(not torch.equal(before[k], v) for k, v in mod.state_dict().items())
    got = module_step(mods, mod, x0, d_out, mode)
    fresh = make()
    fresh.load_state_dict({k: v.cpu() for k, v in mod.state_dict().items()})
    want = module_step(mods, fresh.cuda().train(), x0, d_out, mode)
    assert not torch.equal(got[0], first[0])
    assert all(same_bits(a, b) for a, b in zip(got, want)), [i for i, (a, b) in enumerate(zip(got, want)) if not same_bits(a, b)]


# ------------------------------------------------------------------ 8. the whole Net
@pytest.fixture
def all_on(mods):
    """Every train_hip switch of the package but the optimizer's."""
    M = mods.M
    owners = [M.ActorNet, M.PredNet, M.Att, M.MapNet, M.M2M, mods.layers.LinearRes, mods.A.RowBlockFn]
    prev = [o.train_hip for o in owners]
    for o in owners:
        o.train_hip = True
    yield
    for o, p in zip(owners, prev):
        o.train_hip = p


def flat_out(out):
    return [t for k in ("cls", "reg") for t in out[k]]


@pytest.mark.parametrize("bucket", [False, True], ids=["grads", "bucket"])
def test_whole_net_step(mods, all_on, launches, golden, ref_state_names, bucket):
    """One backward of Net on the batch-4 golden scenes with every train_hip switch on; its 405 gradients go to two
    identically initialised nets, one stepped by torch.optim, one by the fused step (with `bucket`: gradients as views of
    dist.GradBucket's flat buffer, most of them off 16-byte alignment).  All parameters and updates against the float64 rule
    on the same gradients; then two more fused training steps, and the forward of a fresh net loaded from the state_dict."""
    M, ops, U = mods.M, mods.ops, mods.utils
    from lanegcn_amd import data as gen
    from oracle import lanegcn_oracle as O
    with np.load(TG.GOLDEN_DIR + "/train_b4.npz") as z:
        seed = int(z["seed"])
    prev = ops.get_mma()
    ops.set_mma("f16x2")
    try:
        def new_net():
            net = M.Net(M.config)
            net.load_state_dict(O.seeded_state(ref_state_names, seed), strict=True)
            return net.cuda().train()

        batch = gen.collate_fn(load_scenes(golden))
        loss_fn = M.Loss(M.config).cuda()
        stock_net, fused_net = new_net(), new_net()
        loss_fn(stock_net(batch), batch)["loss"].backward()
        names = [n for n, _ in stock_net.named_parameters()]
        grads = [p.grad.clone() for p in stock_net.parameters()]
        assert len(grads) == 405 and all(g is not None for g in grads)
        # Net's only parameter whose size is no multiple of 4 is its last (pred_net.cls.1.bias, one element): in parameter order
        # every view of the bucket is 16-byte aligned, so the bucket is built in reverse order, which puts the other 404 views
        # 4 bytes off
        bk = mods.dist.GradBucket(list(fused_net.parameters())[::-1]) if bucket else None
        for p, g in zip(fused_net.parameters(), grads):
            if bucket:
                p.grad.copy_(g)
            else:
                p.grad = g.clone()
        if bucket:
            assert sum(1 for p in fused_net.parameters() if p.grad.data_ptr() % 16 == 4) == 404
        before = [p.detach().cpu().double().numpy().copy() for p in stock_net.parameters()]
        stock_opt = M.Optimizer(stock_net.parameters(), M.config)
        U.Optimizer.train_hip = True
        try:
            fused_opt = M.Optimizer(fused_net.parameters(), M.config)
        finally:
            U.Optimizer.train_hip = False
        assert fused_opt.fused and not stock_opt.fused and not launches
        lr = stock_opt.step(0.0)
        assert fused_opt.step(0.0) == lr and len(launches) == 1          # one lgcn_opt_step for the 405 tensors
        st = ref_state("adam", before)
        ref_step(st, [g.cpu().double().numpy() for g in grads], lr)
        rows = []
        for i, (n, ps, pf) in enumerate(zip(names, stock_net.parameters(), fused_net.parameters())):
            s, f = ps.detach().cpu().double().numpy(), pf.detach().cpu().double().numpy()
            rows.append(("p " + n, rel(f, st["p"][i]), rel(s, st["p"][i])))
            rows.append(("upd " + n, rel(f - before[i], st["p"][i] - before[i]), rel(s - before[i], st["p"][i] - before[i])))
        check_rows(rows, "Net bucket=%s" % bucket)
        # two more training steps on the fused side
        for k in range(2):
            if bucket:
                bk.zero()
            else:
                fused_opt.zero_grad()
            lo = loss_fn(fused_net(batch), batch)["loss"]
            lo.backward()
            fused_opt.step(0.0)
            assert np.isfinite(float(lo.detach()))
        assert len(launches) == 3
        with torch.no_grad():
            got = flat_out(fused_net(batch))
            fresh = M.Net(M.config)
            fresh.load_state_dict({k: v.cpu() for k, v in fused_net.state_dict().items()}, strict=True)
            want = flat_out(fresh.cuda().train()(batch))
        assert len(got) == len(want) and all(torch.equal(a, b) for a, b in zip(got, want))
    finally:
        ops.set_mma(prev)
