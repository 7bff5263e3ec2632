"""CPU proof that the criteria of tests/taming_blocks_reference.py have teeth, before anyone trusts a green run of tests/test_hip_taming_blocks.py:
for every stage the float64 reference WITH the design's documented fp16 roundings, fed in as "got", passes -- and each wrong wiring a launch
could have (a mutant of the same reference) is rejected.  No device, nothing of the product."""
import pytest
import torch

import taming_blocks_reference as R


def rejected(stage, check, *args):
    """the check fails, and at the launch named `stage` -- not at an earlier one, not on a shape"""
    with pytest.raises(AssertionError) as e:
        check(*args)
    assert stage in str(e.value) and "shape" not in str(e.value), str(e.value)


# ------------------------------------------------------------------------------------------------ ResBlock
# one case per form at the smaller size, with bias: the wiring is what is mutated, not the shape
BLOCKS = {0: (0, 128, 128), 1: (1, 128, 256), 2: (2, 64, 128)}
_BLOCKS = {}


def block(form):
    if form not in _BLOCKS:
        f, cin, cout = BLOCKS[form]
        case = R.make_block(f, cin, cout, 16, 32, True, seed=40 + form)
        _BLOCKS[form] = (case, R.ref_block(case))
    return _BLOCKS[form]


@pytest.mark.parametrize("form", [0, 1, 2])
def test_block_rounded_reference_passes(form):
    case, good = block(form)
    res = R.check_block(case, good)
    assert all(abs(res[k][1] - 1.0) < 1e-6 for k in res if k != "ss")          # "got" IS the model: its rms error is E_model


def test_block_form1_run_as_form2_and_the_reverse_are_rejected():
    case1, _ = block(1)
    rejected(" mid", R.check_block, case1, R.ref_block(case1, form=2))
    case2, _ = block(2)
    rejected(" mid", R.check_block, case2, R.ref_block(case2, form=1))


def test_block_residual_taken_from_h1_is_rejected():
    case, good = block(0)
    bad = R.ref_block(case, residual="h1")
    assert torch.equal(bad["h1"], good["h1"])                                   # only the last launch is wrong
    rejected(" out", R.check_block, case, bad)


def test_block_norm2_statistics_of_the_shortcut_output_are_rejected():
    """what a stats = false launch that clobbered gn.ss would give: conv2's prologue normalises h1 with the shortcut output's statistics"""
    case, good = block(1)
    bad = R.ref_block(case, stats_from="mid")
    assert torch.equal(bad["h1"], good["h1"]) and torch.equal(bad["mid"], good["mid"])
    rejected(" out", R.check_block, case, bad)


def test_block_output_statistics_of_another_tensor_are_rejected():
    """the further launch_gn picking the wrong source: (scale, shift) of h1 handed out as those of the block's output"""
    case, good = block(0)
    B, cout = case["B"], case["cout"]
    bad = dict(good, ss=R.ref_scale_shift(good["h1"].reshape(B, -1, cout), case["og"], case["ob"]))
    rejected("output GroupNorm", R.check_block, case, bad)


# ------------------------------------------------------------------------------------------------ AttnBlock
@pytest.mark.parametrize("case", R.ATTN_CASES, ids=lambda c: "block{}_{}x{}_b{}_latent{}".format(*c))
def test_attention_inputs_are_not_degenerate(case):
    block_, H, W, B, _ = case
    mp = R.make_attn(block_, H, W, B, seed=R.attn_seed(case))["mp"]
    print(f"attention case {case}: mean maximum probability {mp:.3f}")
    assert 0.3 < mp < 0.7


def attn():
    c = R.ATTN_CASES[1]                                                         # 8 x 16, B 2
    case = R.make_attn(c[0], c[1], c[2], c[3], seed=R.attn_seed(c))
    return case, R.ref_attn_block(case)


def test_attn_rounded_reference_passes():
    case, good = attn()
    res = R.check_attn_block(case, good)
    assert abs(res["qkv"][1] - 1.0) < 1e-6 and abs(res["out"][1] - 1.0) < 1e-6 and res["attn"] < 1.0


@pytest.mark.parametrize("stage,mutant", [(" qkv", dict(silu=True)), (" qkv", dict(rotate=1)), (" qkv", dict(rotate=2)), (" attention", dict(scale=1.0)),
                                          (" proj_out", dict(residual=None)), (" proj_out", dict(residual="attn"))],
                         ids=["silu_in_qkv_prologue", "qkv_blocks_rotated_1", "qkv_blocks_rotated_2", "scale_dropped", "proj_without_residual",
                              "proj_residual_attn_out"])
def test_attn_mutants_are_rejected(stage, mutant):
    case, _ = attn()
    rejected(stage, R.check_attn_block, case, R.ref_attn_block(case, **mutant))


# ------------------------------------------------------------------------------------------------ folded final layer, packer
def test_final_rounded_reference_passes_and_fold_mutants_are_rejected():
    case = R.make_final(32, 48, 2, seed=70)
    worst, ratio = R.check_final(case, R.ref_final(case))
    assert worst <= 1.0 and abs(ratio - 1.0) < 1e-3                             # (the fp32 image rounds the float64 model once more)
    rejected("final", R.check_final, case, R.ref_final(case, fold=None), "final")
    rejected("final", R.check_final, case, R.ref_final(case, fold="weight"), "final")
    w2, b2 = R.prefolded(case)                                                  # the pre-folded operands are the same layer
    pre, _ = R.ref_conv(case["x16"], w2, b2, case["gamma"], case["beta"], None, 3, False, True, True)
    assert float((pre.float() - R.ref_final(case)).abs().max()) <= 2.0 ** -22


@pytest.mark.parametrize("H,W", R.PACK_SHAPES)
@pytest.mark.parametrize("B", [1, 3])
def test_packer_reference_passes_and_unscaled_mutant_is_rejected(B, H, W):
    img = R.make_pack(B, H, W, seed=B * 100 + H)
    R.check_pack(R.ref_pack(img), img)
    rejected("packed image", R.check_pack, R.ref_pack(img, scaled=False), img)
    out = R.ref_pack(img)
    assert bool((out[:, 3:] == 0).all()) and float(out.float().abs().max()) <= 65504.0
