"""CPU: tools/check_weight_scale.py on a synthetic state dict -- the blocks are the ones the kernels consume."""
import warnings

import torch

from tools import check_weight_scale as W


def state():
    g = torch.Generator().manual_seed(1)
    rn = lambda *s: torch.randn(*s, generator=g) * 0.13
    ctx0 = rn(128, 384)
    ctx0[:, 128:256] *= 2.0 ** -12                 # one column block of ctx.0 far below the window
    meta = rn(128, 132)
    meta[:, 128:] *= 2.0 ** -20                    # the four meta columns run in fp32: not a block
    dead = rn(128, 256)
    dead[:, :128] = 0.0                            # an all-zero block is exact
    return {"a2m.att.0.ctx.0.weight": ctx0, "a2m.meta.linear.weight": meta, "m2m.fuse.ctr.0.weight": rn(128, 128),
            "map_net.input.0.weight": rn(128, 2) * 2.0 ** -20, "actor_net.groups.0.0.conv1.weight": rn(32, 3, 3) * 2.0 ** -10,
            "pred_net.att_dest.agt.linear.weight": dead, "m2m.fuse.norm.0.weight": torch.full((128,), 1e-6),
            "edge.weight": torch.full((128, 128), W.W_LOW), "steps": torch.tensor(3)}


def test_small_blocks_are_the_kernels_blocks():
    found = W.small_blocks(state())
    assert [(n, c) for n, c, _ in found] == [("a2m.att.0.ctx.0.weight", 128), ("actor_net.groups.0.0.conv1.weight", None)]
    assert all(0 < m < W.W_LOW for _, _, m in found)
    assert W.small_blocks({"state_dict": state(), "epoch": 1.0}) == found          # a checkpoint dict
    text = W.describe(found)
    assert "a2m.att.0.ctx.0.weight[:, 128:256]" in text and "bf16x3" in text


def test_module_and_warning(tmp_path):
    lin = torch.nn.Linear(128, 128, bias=False)
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        assert W.warn_small_blocks(lin) == []                                        # default init: max |W| ~ 0.088
    with torch.no_grad():
        lin.weight.mul_(2.0 ** -10)
    with warnings.catch_warnings(record=True) as seen:
        warnings.simplefilter("always")
        assert [n for n, _, _ in W.warn_small_blocks(lin)] == ["weight"]
    assert len(seen) == 1 and "f16x2 window" in str(seen[0].message)
    path = tmp_path / "w.ckpt"
    torch.save({"state_dict": lin.state_dict()}, path)
    assert W.main([str(path)]) == 1
    torch.save({"state_dict": torch.nn.Linear(128, 128).state_dict()}, path)
    assert W.main([str(path)]) == 0
