"""ActorNet's two-plane conv path over operand scale and statistics: the states, the inputs, and the CPU evaluations every
check of them shares -- the float64 truth (the stock modules run in double), the fp32 run of the stock modules, and the
operand-format model (split_model.conv1d_unit / res1d_block / actor_net) -- computed once per case and cached.

Test infrastructure for tests/test_actornet_model_host.py and tests/test_gpu_actornet_scale.py, in the style of
hot_path_cases.py.  Everything is regenerated from a fixed seed; nothing is stored and nothing comes from the kernels.

States (oracle.seeded_state over ActorNet's parameter shapes at seed 3):
    ("uniform", e)   every conv weight times 2^e (exact), GroupNorm parameters as seeded;  e = 0, -4, -8, -12, -16
    ("input", e)     the weights as seeded, the module's input times 2^e (exact);          e = 12, -8, -14
    ("wide",)        per-tensor weight scales 2^U[-8, 2], GroupNorm scales log-uniform in [0.05, 8] with 10 % negative,
                     shifts x 5: oracle.wide_state's statistics (which it applies to matrices of K >= 128 only; the
                     narrower conv weights get their own draw of the same distribution)
Every conv feeds a GroupNorm, so the float64 function moves with a weight scale only through eps, while the f16x2 operands
run out of bits below fp16's normal range.
Inputs [A, 3, 20]:
    "randn"   3 x N(0, 1)
    "track"   track-like: displacement steps around a per-actor velocity, third channel 1 where the step is observed; the
              first three actors are observed at the last 1, 2 and 7 steps only (zero rows in front), the fourth stands
              still (constant rows)
Actor counts: 1 and 17 -- one past a full workgroup at every level (4, 8, 16 actors at lout = 20, 10, 5): the ragged last
workgroup and the per-actor statistics beside a neighbour's.
Range: |x| 2^12 stays under 65520 (fp16's overflow threshold) for both draws, asserted in inputs()."""
import functools
import zlib

import numpy as np
import torch

import split_model as S
from oracle import lanegcn_oracle as O

SEED = 3
WIDE = ("wide",)
UNIFORM = [("uniform", e) for e in (0, -4, -8, -12, -16)]
INPUT = [("input", e) for e in (12, -8, -14)]
STATES = UNIFORM + INPUT + [WIDE]
DRAWS = ("randn", "track")
COUNTS = (1, 17)
L_IN = 20
# ActorNet's Res1d blocks (module path, lin) and its groups
BLOCKS = [("groups.0.0", 20), ("groups.0.1", 20), ("groups.1.0", 20), ("groups.1.1", 10), ("groups.2.0", 10), ("groups.2.1", 5),
          ("output", 20)]
GROUPS = [("groups.0", 20), ("groups.1", 20), ("groups.2", 10)]


def case_id(state):
    return "wide" if state == WIDE else ("w2^%d" if state[0] == "uniform" else "x2^%d") % state[1]


def p2(t, e):
    """t * 2^e in fp32, exactly (no underflow, no overflow)."""
    out = torch.ldexp(t, torch.tensor(e))
    assert out.dtype == torch.float32 and torch.equal(out.double(), torch.ldexp(t.double(), torch.tensor(e)))
    return out


def modules():
    import lanegcn_amd  # noqa: F401
    from lanegcn_amd import lanegcn as M
    return M


@functools.lru_cache(maxsize=None)
def shapes():
    return [(k, tuple(v.shape)) for k, v in modules().ActorNet(modules().config).state_dict().items()]


def input_exp(state):
    return state[1] if state[0] == "input" else 0


def state_dict(state):
    """A fresh state dict of ActorNet (fp32 CPU tensors) for `state`."""
    sd = O.seeded_state(shapes(), SEED)
    if state[0] == "uniform":
        return {k: p2(v, state[1]) if v.dim() == 3 else v for k, v in sd.items()}
    if state == WIDE:
        wide = O.wide_state(shapes(), SEED, -8, 2)
        for name, shape in shapes():
            if len(shape) == 3 and int(np.prod(shape[1:])) < 128:          # wide_state left it as seeded
                rs = np.random.RandomState((zlib.crc32(name.encode()) + 1000003 * SEED + 700000001) % (2 ** 32))
                wide[name] = wide[name] * np.float32(2.0 ** rs.uniform(-8, 2))
        return wide
    return sd


def make_net(sd, double=False):
    """A fresh stock ActorNet on the CPU holding sd (fresh: no packed image is reused between cases)."""
    M = modules()
    net = M.ActorNet(M.config).eval()
    net.load_state_dict({k: v.clone() for k, v in sd.items()})
    return net.double() if double else net


def submodule(net, path):
    for part in path.split("."):
        net = net[int(part)] if part.isdigit() else getattr(net, part)
    return net


@functools.lru_cache(maxsize=None)
def inputs(draw, n_act):
    """x [n_act, 3, 20] fp32 (unscaled: a state's input exponent is applied by scaled_input)."""
    g = torch.Generator().manual_seed(1000 * DRAWS.index(draw) + n_act)
    if draw == "randn":
        x = 3.0 * torch.randn(n_act, 3, L_IN, generator=g)
    else:
        vel = 1.5 * torch.randn(n_act, 2, 1, generator=g)
        x = torch.cat([vel + 0.2 * torch.randn(n_act, 2, L_IN, generator=g), torch.ones(n_act, 1, L_IN)], 1)
        for a, seen in zip(range(n_act), (1, 2, 7)):               # observed at the last `seen` steps only
            x[a, :, :L_IN - seen] = 0.0
        if n_act > 3:
            x[3, :2] = 0.0                                          # stands still: constant rows (0, 0, 1)
    assert float(x.abs().max()) * 2.0 ** 12 < 65520.0
    return x


def scaled_input(draw, n_act, state):
    return p2(inputs(draw, n_act), input_exp(state))


def rel_err(got, ref):
    return S.rel_err(got, ref)


def finite(*arrays):
    return all(np.isfinite(S.arr(a, np.float64)).all() for a in arrays)


# ------------------------------------------------------------------ the whole module
@functools.lru_cache(maxsize=None)
def net_cpu(draw, n_act, state):
    """dict(truth [A, 128] float64, ref32, e_ref32, e_model) of the whole module in f16x2."""
    sd, x = state_dict(state), scaled_input(draw, n_act, state)
    with torch.no_grad():
        truth = make_net(sd, double=True)(x.double()).numpy()
        ref32 = make_net(sd)(x).numpy()
    model = S.actor_net(x, sd, "f16x2")
    assert finite(truth, model), "the case itself left the format's range"
    return dict(truth=truth, ref32=ref32, e_ref32=rel_err(ref32, truth), e_model=rel_err(model, truth))


# ------------------------------------------------------------------ blocks and groups
def block_input(path, lin, n_act, state):
    """Channels-last x [n_act, lin, cin] of a block: the module's randn draw for the first block, 3 N(0, 1) behind a
    ReLU for the others (what a block hands on), times the state's input scale."""
    blk = submodule(make_net(state_dict(("uniform", 0))), path)
    cin = (blk[0] if isinstance(blk, torch.nn.Sequential) else blk).conv1.in_channels
    if cin == 3:
        x = inputs("randn", n_act).transpose(1, 2).contiguous()
    else:
        g = torch.Generator().manual_seed(7 * cin + lin + n_act)
        x = torch.randn(n_act, lin, cin, generator=g).relu()
    return p2(x, input_exp(state))


def block_dicts(sd, path):
    """split_model.res1d_block's dicts of a block (one) or a group (two)."""
    groups, _, output = S.actor_blocks(sd)
    if path == "output":
        return [output]
    parts = path.split(".")
    return groups[int(parts[1])] if len(parts) == 2 else [groups[int(parts[1])][int(parts[2])]]


@functools.lru_cache(maxsize=None)
def block_cpu(path, lin, n_act, state):
    """dict(truth [A, lout, c] float64, e_ref32, e_model) of a Res1d block or a group of two in f16x2; the stock modules
    take [A, cin, lin]."""
    sd, x = state_dict(state), block_input(path, lin, n_act, state)
    with torch.no_grad():
        truth = submodule(make_net(sd, double=True), path)(x.transpose(1, 2).double()).transpose(1, 2).numpy()
        ref32 = submodule(make_net(sd), path)(x.transpose(1, 2)).transpose(1, 2).numpy()
    d = block_dicts(sd, path)
    model = S.res1d_block(x, d[0], "f16x2", second=d[1] if len(d) == 2 else None)
    assert finite(truth, model), "the case itself left the format's range"
    return dict(truth=truth, e_ref32=rel_err(ref32, truth), e_model=rel_err(model, truth))


# ------------------------------------------------------------------ single units
@functools.lru_cache(maxsize=None)
def unit_draw(shape, n_act):
    """(x [A, lin, cin], w [cout, cin, ks], gamma, beta, res [A, lout, cout], res_half [A, lout / 2, cout] | None) of one
    unit shape (cin, cout, ks, stride, lin): weights as oracle.seeded_state draws them."""
    cin, cout, ks, stride, lin = shape
    lout = (lin + 2 * ((ks - 1) // 2) - ks) // stride + 1
    g = torch.Generator().manual_seed(7 * cin + cout + 13 * ks + stride + lin + 1000 * n_act)
    rn = lambda *s: torch.randn(*s, generator=g)
    return (rn(n_act, lin, cin), rn(cout, cin, ks) * (1.5 / (cin * ks) ** 0.5), 1 + 0.1 * rn(cout), 0.1 * rn(cout),
            rn(n_act, lout, cout), rn(n_act, lout // 2, cout) if lout % 2 == 0 else None)


def unit_case(shape, n_act, state, res_mode):
    """(x, w, stride, gamma, beta, res | None) of a unit at `state` (uniform: w scaled; input: x scaled)."""
    x, w, gamma, beta, res, res_half = unit_draw(shape, n_act)
    x, w = p2(x, input_exp(state)), p2(w, state[1] if state[0] == "uniform" else 0)
    return x, w, shape[3], gamma, beta, (None, res, res_half)[res_mode]


def bar(e_model, e_ref32):
    """Blocks, groups and the whole module: hot_path_cases.bar (several fp32 GroupNorms deep)."""
    import hot_path_cases as H
    return H.bar(e_model, e_ref32)
