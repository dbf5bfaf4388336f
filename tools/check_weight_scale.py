#!/usr/bin/env python
"""List the weight blocks of a checkpoint (or a module) that lie below the f16x2 window (DESIGN.md "Operand scale").

The default matrix mode rounds every operand of a 128-wide contraction to two fp16 planes.  With O(1) activations the
result stays within 1e-4 of fp32 while max |W| of the block is at least 2^-9 (2.0e-3): measured <= 7e-5 there, 5e-4 .. 1e-3
at 2^-13, 1e-2 at 2^-17; the whole hot path with EVERY block at 2^-9 measures 8.3e-5, so the threshold holds for
the 14-layer stack too, by a factor 1.2 ("Whole hot path").  A trained network with a small layer (weight decay, a near-dead head) can sit below that and
nothing else says so: the range guard only looks for NaN.  Such a network should run in bf16x3 (ops.set_mma("bf16x3")),
which has fp32's exponent range.

Blocks are taken as the kernels consume them: every [128, K >= 128] matrix in 128-column blocks (ctx.0's [128, 384] as
three; a tail of fewer than 128 columns -- A2M.meta's four -- and the [128, 2] input layers run in plain fp32 and are not
listed), every Conv1d weight [cout, cin, k] as a whole.  All-zero blocks are exact and not listed.  CPU only.

    python tools/check_weight_scale.py results/lanegcn/36.000.ckpt
"""
import sys

W_LOW = 2.0 ** -9          # lower edge of the f16x2 window for max |W| of a block
C = 128


def weight_blocks(state):
    """(name, first column | None, block) of a state dict's matrix-core operands."""
    for name, w in state.items():
        if not hasattr(w, "dim") or not w.is_floating_point():
            continue
        if w.dim() == 2 and w.shape[0] == C and w.shape[1] >= C:
            for col0 in range(0, w.shape[1] - C + 1, C):
                yield name, col0, w[:, col0:col0 + C]
        elif w.dim() == 3:
            yield name, None, w


def small_blocks(model, lower=W_LOW):
    """[(name, first column | None, max |W|)] of the blocks with 0 < max |W| < lower; model: a state dict, a checkpoint
    dict with a "state_dict" entry, or an nn.Module."""
    state = model.state_dict() if hasattr(model, "state_dict") else model.get("state_dict", model)
    out = []
    for name, col0, block in weight_blocks(state):
        m = float(block.detach().abs().max()) if block.numel() else 0.0
        if 0.0 < m < lower:
            out.append((name, col0, m))
    return out


def describe(found, lower=W_LOW):
    lines = ["%d weight block(s) below the f16x2 window (max |W| < %.2e): fp16 planes lose precision there; "
             "use ops.set_mma('bf16x3')" % (len(found), lower)]
    for name, col0, m in found:
        lines.append("  %s%s  max |W| = %.3e" % (name, "" if col0 is None else "[:, %d:%d]" % (col0, col0 + C), m))
    return "\n".join(lines)


def warn_small_blocks(model, lower=W_LOW):
    """warnings.warn once when the model has blocks below the window; returns them."""
    found = small_blocks(model, lower)
    if found:
        import warnings
        warnings.warn(describe(found, lower), RuntimeWarning, stacklevel=2)
    return found


def main(argv=None):
    import torch
    argv = sys.argv[1:] if argv is None else argv
    if len(argv) != 1:
        print(__doc__)
        return 2
    found = small_blocks(torch.load(argv[0], map_location="cpu", weights_only=True))
    print(describe(found) if found else "every weight block is inside the f16x2 window (max |W| >= %.2e)" % W_LOW)
    return 1 if found else 0


if __name__ == "__main__":
    sys.exit(main())
