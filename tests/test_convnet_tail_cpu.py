"""CPU checks of the references and the inputs that tests/test_hip_convnet_tail.py holds the feature networks' tail kernels to (the BatchNorm
fold, the spatial mean, the head): the fp32 restatements stay within their derived distance of float64, the two networks' epsilons give
different folds in every layer (so a handle with the other network's epsilon cannot pass the bit-equality), and the "integer" inputs are exact
in fp32.  No GPU.

Bounds, each from the operations' roundings (u = 2^-24):
* scale = g / sqrt(v + eps): the add, the root (which halves the add's error) and the division: 2.5 u, asserted as 3 u relative.
* shift = b - m scale: 2.5 u from the scale and one rounding of the product on |m scale|, one rounding of the difference on |shift| <=
  |b| + |m scale|: 4.5 u (|b| + |m scale|), asserted as 5 u.
* mean: (ceil(HW / 256) + 9) u mean|x|; head: (D / 64 + 7) u (sum |p w| + |bias|) -- convnet_reference.mean_bound / head_bound.
"""
import numpy as np
import pytest
import torch

import convnet_reference as CR
import inception_reference as RI
import resnet_reference as RR
from maskbit_amd.synth import inception_convs, resnet50_convs

U32 = CR.U32


def bn_layers():
    """-> [(tag, state dict, BatchNorm prefix, the network's own eps)]: 94 + 94 + 53"""
    out = []
    for style in ("he", "tf"):
        out += [(f"inception {style}", RI.weights(style), name + ".bn", CR.INCEPTION_EPS) for name, *_ in inception_convs()]
    out += [("resnet", RR.weights(), bn, CR.RESNET_EPS) for _conv, bn, *_ in resnet50_convs()]
    return out


def test_the_epsilons_are_the_networks_own():
    assert CR.INCEPTION_EPS == RI.BN_EPS and CR.RESNET_EPS == RR.BN_EPS
    assert len(bn_layers()) == 94 + 94 + 53


def test_fold32_is_within_three_roundings_of_float64():
    worst_scale = worst_shift = 0.0
    layers = bn_layers() + [(f"case {c}", None, None, eps) for c in CR.FOLD_COUTS for eps in (CR.INCEPTION_EPS, CR.RESNET_EPS)]
    for tag, sd, prefix, eps in layers:
        parts = CR.bn_parts(sd, prefix) if sd is not None else tuple(CR.fold_case(int(tag.split()[1])))
        s32, t32 = CR.bn_fold32(*parts, eps)
        s64, t64, mag = CR.bn_fold64(*parts, eps)
        assert s32.dtype == torch.float32 and t32.dtype == torch.float32 and bool(torch.isfinite(s32).all()) and bool(torch.isfinite(t32).all())
        es, et = (s32.double() - s64).abs(), (t32.double() - t64).abs()
        assert bool((es <= 3 * U32 * s64.abs()).all()), (tag, prefix)
        assert bool((et <= 5 * U32 * mag).all()), (tag, prefix)
        nz = s64 != 0
        if bool(nz.any()):
            worst_scale = max(worst_scale, float((es[nz] / s64[nz].abs()).max()) / U32)
        worst_shift = max(worst_shift, float((et / mag.clamp(min=1e-300)).max()) / U32)
    print(f"bn_fold32 against float64: scale at most {worst_scale:.3f} u relative, shift at most {worst_shift:.3f} u of |b| + |m scale|")


def test_fold32_agrees_with_float64_rounded_after_every_operation():
    """the second way to state the five operations: float64 arithmetic, rounded to fp32 after each (exact for +, -, *, / and sqrt of fp32 operands:
    float64 carries more than twice fp32's precision plus two bits)"""
    r = lambda a: a.astype(np.float32).astype(np.float64)
    for tag, sd, prefix, eps in bn_layers():
        g, b, m, v = (t.float().double().numpy() for t in CR.bn_parts(sd, prefix))
        a = r(v + np.float64(np.float32(eps)))
        s = r(g / r(np.sqrt(a)))
        shift = r(b - r(m * s))
        s32, t32 = CR.bn_fold32(*CR.bn_parts(sd, prefix), eps)
        assert np.array_equal(s32.numpy().view(np.int32), s.astype(np.float32).view(np.int32)), (tag, prefix)
        assert np.array_equal(t32.numpy().view(np.int32), shift.astype(np.float32).view(np.int32)), (tag, prefix)


def test_the_other_networks_epsilon_changes_every_layer():
    same_channels = total = 0
    for tag, sd, prefix, eps in bn_layers():
        other = CR.RESNET_EPS if eps == CR.INCEPTION_EPS else CR.INCEPTION_EPS
        parts = CR.bn_parts(sd, prefix)
        s_own, t_own = CR.bn_fold32(*parts, eps)
        s_other, t_other = CR.bn_fold32(*parts, other)
        live = parts[0] != 0                                           # a zero gamma folds to a zero scale under any epsilon
        assert bool(live.any()) and not torch.equal(s_own, s_other), (tag, prefix)
        assert bool((s_own[live] != s_other[live]).all()), (tag, prefix)
        same_channels += int((s_own == s_other).sum())
        total += s_own.numel()
    print(f"scales unchanged under the other epsilon: {same_channels} of {total}")


def test_fold_cases_hold_what_they_are_for():
    for cout in CR.FOLD_COUTS:
        gamma, _beta, _mean, var = CR.fold_case(cout)
        assert float(var.min()) >= 0.0 and float(var.max()) <= 10.0
        if cout >= 32:
            assert bool((gamma == 0).any()) and bool((gamma < 0).any()) and bool((var == 0).any())
            assert float(var[var > 0].min()) < 1e-2 and float(var.max()) > 1.0


@pytest.mark.parametrize("HW", CR.MEAN_HW)
def test_mean32_is_within_its_bound_of_float64(HW):
    for C_ in CR.MEAN_C:
        for B in CR.MEAN_B:
            for kind in ("seeded", "integer"):
                x16 = CR.mean_case(kind, B, HW, C_)
                got = CR.spatial_mean32(x16)
                exact, mag = CR.spatial_mean64(x16)
                assert got.dtype == torch.float32 and tuple(got.shape) == (B, C_)
                assert bool(((got.double() - exact).abs() <= CR.mean_bound(HW, mag)).all()), (kind, B, HW, C_)
                if kind == "seeded":
                    assert bool((x16[..., 1] < 0).all()) and float(x16.max()) == 65504.0 and float(x16.min()) == -65504.0
                    assert bool((got[:, 1] < 0).all())
                else:                                                  # every partial sum is an integer below 2^24: any order gives S, then one division
                    assert float(x16.min()) >= 0 and float(x16.max()) <= 64 and 64 * HW < 2 ** 24
                    S = x16.double().sum(1)
                    want = (S.float().numpy() / np.float32(HW))
                    assert bool((S == S.float().double()).all()) and np.array_equal(got.numpy().view(np.int32), want.view(np.int32))


def test_mean32_is_not_the_plain_pixel_order():
    """the reference pins the kernel's order: on the seeded 1225- and 5329-pixel inputs a sum in plain pixel order gives other bits somewhere"""
    differs = 0
    for HW in (1225, 5329):
        x16 = CR.mean_case("seeded", 3, HW, 72)
        plain = np.zeros((3, 72), dtype=np.float32)
        for p in range(HW):
            plain = plain + x16[:, p].float().numpy()
        differs += int((torch.from_numpy(plain / np.float32(HW)) != CR.spatial_mean32(x16)).sum())
    assert differs > 0


def test_head_cases_cover_every_pair_and_the_integer_ones_are_exact():
    cases = set(CR.HEAD_CASES)
    assert (2048, 1008, 17) in cases and (2048, 1000, 9) in cases and len(cases) == 25
    assert {(d, n) for d, n, _ in cases} == {(d, n) for d in CR.HEAD_D for n in CR.HEAD_N}
    assert {(d, b) for d, _, b in cases} == {(d, b) for d in CR.HEAD_D for b in CR.HEAD_B}
    assert {(n, b) for _, n, b in cases} == {(n, b) for n in CR.HEAD_N for b in CR.HEAD_B}
    for D, N, B in CR.HEAD_CASES:
        pool, w, bias = CR.head_case("integer", B, D, N)
        assert float(pool.min()) >= 0 and float(pool.max()) < 8 and float(w.abs().max()) <= 4 and bool((bias * 2 == (bias * 2).round()).all())
        unbiased, biased, S = CR.fc_head64(pool, w, bias)
        assert float(S.max()) < 2 ** 23                                # every partial sum of |p w|, and the bias on top, stays exact in fp32
        assert torch.equal(unbiased.float().double(), unbiased) and torch.equal(biased.float().double(), biased)
        pool, w, bias = CR.head_case("seeded", B, D, N)
        assert float(pool.min()) >= 0 and float(pool.max()) > 0
