"""CPU-only tests of LPIPS: the float64 restatement (tests/lpips_reference.py) against the recorded runs of the reference's own ``LPIPS``
(tests/golden/lpips.npz, tools/make_golden_lpips.py), the seeded VGG16 weights, the fp16 error model that is the unit of the GPU bounds, and the
host side -- state-dict keys, key layouts, loud failure without a GPU, the evaluator's attachment point, the C entries."""
import inspect
import os
import re

import numpy as np
import pytest
import torch

import lpips_reference as R
from conftest import ROOT
from maskbit_amd.synth import VGG16_CONVS, make_vgg16_weights


@pytest.mark.parametrize("name", list(R.CASES))
def test_restatement_reproduces_the_reference(name):
    """`exact` against the reference on .double() inputs (1e-12 relative) and against the reference as it runs (within 4 x its own fp32 error)"""
    z = R.golden()
    assert [str(c) for c in z["cases"]] == list(R.CASES) and int(z["vgg_seed"]) == R.VGG_SEED
    fam, sig, B, H, W, seed, style = R.CASES[name]
    assert str(z[name + ".family"]) == fam and str(z[name + ".style"]) == style
    assert z[name + ".params"].tolist() == [sig, B, H, W, seed]
    real, fake = R.case_images(name)
    with torch.no_grad():
        exact = R.lpips64(real, fake, R.vgg_weights(style), R.lin_vectors(z)).numpy()
    ref64, ref32 = z[name + ".ref64"], z[name + ".ref32"]
    assert exact.shape == ref64.shape == (B,)
    rel = np.abs(exact - ref64) / ref64
    e_ref = np.abs(ref32 - ref64).max()
    print(f"{name}: exact vs ref64 {rel.max():.2e} relative; |ref32 - ref64| {e_ref:.2e}, |exact - ref32| {np.abs(exact - ref32).max():.2e}")
    assert rel.max() <= 1e-12
    assert e_ref > 0 and np.abs(exact - ref32).max() <= 4 * e_ref


def test_fixture_lin_vectors():
    z = R.golden()
    lins = R.lin_vectors(z)
    assert [int(v.numel()) for v in lins] == list(R.TAP_CHANNELS) == [64, 128, 256, 512, 512]
    assert sum(int(v.numel()) for v in lins) == 1472
    assert all(bool((v >= 0).all()) and float(v.sum()) > 0 for v in lins)
    assert len(z["state_dict_keys"]) == 33
    assert os.path.getsize(R.GOLDEN) < 64 * 1024


def test_weight_styles_reach_their_activation_ranges():
    """He-normal keeps the taps O(1); "grown" climbs to the order of 100 at relu5_3 and stays a factor 4 inside the fp16 range"""
    with torch.no_grad():
        for name in R.RESTATEMENT_CASES:
            style = R.CASES[name][6]
            real, fake = R.case_images(name)
            _, taps = R.lpips64(real, fake, R.vgg_weights(style), R.lin_vectors(), return_taps=True)
            rms = [float(t.pow(2).mean().sqrt()) for t in taps]
            mx = [float(t.max()) for t in taps]
            print(f"{name} ({style}): tap rms {['%.3g' % v for v in rms]} max {['%.3g' % v for v in mx]}")
            if style == "he":
                assert all(0.3 <= v <= 3.0 for v in rms), rms
            else:
                assert rms[-1] >= 30.0 and max(mx) < 65504 / 4, (rms, mx)
                assert all(a < b for a, b in zip(rms, rms[1:]))


def test_weight_styles_are_reproducible_by_seed():
    for style in ("he", "grown"):
        a, b, c = make_vgg16_weights(7, style), make_vgg16_weights(7, style), make_vgg16_weights(8, style)
        assert list(a) == [f"{i}.{p}" for i, _, _ in VGG16_CONVS for p in ("weight", "bias")]
        assert all(torch.equal(a[k], b[k]) for k in a) and not torch.equal(a["0.weight"], c["0.weight"])
        assert all(tuple(a[f"{i}.weight"].shape) == (co, ci, 3, 3) and tuple(a[f"{i}.bias"].shape) == (co,) for i, ci, co in VGG16_CONVS)
    with pytest.raises(ValueError):
        make_vgg16_weights(0, "kaiming")


@pytest.mark.parametrize("name", list(R.ENGINE_CASES))
def test_error_model_is_positive_on_engine_cases(name):
    """E_model = |model - exact| per image: what fp16 weights and fp16 stored activations cost; the unit of the GPU bounds (profiles/lpips.md)"""
    o = R.case_oracle(name)
    e = (o["model"] - o["exact"]).abs()
    print(f"{name}: exact {o['exact'].tolist()} E_model {e.tolist()} relative {(e / o['exact']).tolist()}")
    assert bool((e > 0).all()) and bool((e < 0.05 * o["exact"]).all())
    for k, (m, x) in enumerate(zip(o["model_taps"], o["exact_taps"])):
        rel = float((m - x).pow(2).mean().sqrt() / x.pow(2).mean().sqrt())
        assert 1e-4 < rel < 2e-3, (k, rel)                    # a few fp16 roundings deep: between one tenth of and 4 x the unit roundoff 2^-11


def _same_device_free_tensors(a, b):
    return list(a) == list(b) and all(torch.equal(a[k], b[k]) for k in a)


def test_state_dict_keys_and_key_layouts():
    from maskbit_amd import LPIPS
    z = R.golden()
    m = LPIPS()
    assert list(m.state_dict()) == [str(k) for k in z["state_dict_keys"]] and len(m.state_dict()) == 33      # the reference's, in its order
    assert not any(p.requires_grad for p in m.parameters())
    nd = LPIPS(use_dropout=False)
    assert [k for k in nd.state_dict() if k.startswith("lin")] == [f"lin{k}.model.0.weight" for k in range(5)]
    assert [k for k in m.state_dict() if k.startswith("lin")] == [f"lin{k}.model.1.weight" for k in range(5)]
    # nothing is loaded at construction
    assert all(float(v.abs().sum()) == 0 for k, v in m.state_dict().items() if not k.startswith("scaling_layer"))
    assert not m._vgg_loaded and not m._lin_loaded

    vgg = R.vgg_weights("he")
    ref_sd = R.reference_state_dict(vgg, R.lin_vectors(z))
    assert list(ref_sd) == list(m.state_dict())
    layouts = {
        "bare": vgg,
        "torchvision": {**{"features." + k: v for k, v in vgg.items()}, "classifier.0.weight": torch.zeros(2, 2)},
        "reference": {k: v for k, v in ref_sd.items() if k.startswith("net.")},
    }
    loaded = []
    for name, sd in layouts.items():
        mm = LPIPS()
        mm.load_vgg16(sd)
        assert mm._vgg_loaded and not mm._lin_loaded
        mm.load_linear(ref_sd)
        assert mm._lin_loaded
        loaded.append(mm.state_dict())
    assert all(_same_device_free_tensors(loaded[0], other) for other in loaded[1:])
    assert all(torch.equal(loaded[0][k], ref_sd[k]) for k in ref_sd)
    # the lin index of the file need not be the model's; a full state dict loads strictly
    nd.load_linear(ref_sd)
    assert torch.equal(nd.state_dict()["lin3.model.0.weight"], ref_sd["lin3.model.1.weight"])
    full = LPIPS()
    full.load_state_dict(ref_sd, strict=True)
    assert full._vgg_loaded and full._lin_loaded
    with pytest.raises(KeyError):
        LPIPS().load_vgg16({k: v for k, v in vgg.items() if k != "28.bias"})
    with pytest.raises(KeyError):
        LPIPS().load_linear({"lin0.model.1.weight": torch.zeros(1, 64, 1, 1)})


def test_load_from_files(tmp_path):
    from maskbit_amd import LPIPS
    vgg = R.vgg_weights("grown")
    ref_sd = R.reference_state_dict(vgg, R.lin_vectors())
    torch.save({"features." + k: v for k, v in vgg.items()}, tmp_path / "vgg16.pth")
    torch.save({k: v for k, v in ref_sd.items() if not k.startswith("net.")}, tmp_path / "vgg_lpips.pth")       # 7 entries, as the reference's file
    m = LPIPS()
    m.load_vgg16(tmp_path / "vgg16.pth")
    m.load_linear(str(tmp_path / "vgg_lpips.pth"))
    assert all(torch.equal(m.state_dict()[k], ref_sd[k]) for k in ref_sd)


def test_no_cpu_path_and_size_checks():
    from maskbit_amd import LPIPS
    import modeling.modules
    assert modeling.modules.LPIPS is LPIPS                     # the reference's import path
    m = LPIPS()
    m.load_state_dict(R.reference_state_dict(R.vgg_weights("he"), R.lin_vectors()))
    x = torch.zeros(1, 3, 256, 256)
    with pytest.raises(RuntimeError, match="no CPU path"):
        m(x, x)
    with pytest.raises(RuntimeError, match="no CPU path"):
        m.per_image(x, x)
    for shape in ((1, 3, 64, 64), (3, 3, 37, 50), (1, 3, 256, 128), (1, 3, 192, 256), (1, 1, 256, 256), (1, 4, 256, 256), (0, 3, 256, 256)):
        with pytest.raises(ValueError):
            LPIPS.check_images(shape, shape)
    with pytest.raises(ValueError):
        LPIPS.check_images((1, 3, 256, 256), (2, 3, 256, 256))
    for shape in ((1, 3, 256, 256), (2, 3, 128, 256), (1, 3, 512, 512), (7, 3, 384, 768)):
        LPIPS.check_images(shape, shape)
    assert list(inspect.signature(LPIPS.__init__).parameters) == ["self", "use_dropout"]
    assert list(inspect.signature(LPIPS.per_image).parameters) == ["self", "input", "target", "clamp"]


def test_evaluator_attachment_point():
    from maskbit_amd import TokenizerEvaluator
    assert list(inspect.signature(TokenizerEvaluator.use_lpips).parameters) == ["self", "model"]
    with pytest.raises(NotImplementedError, match="reference's own evaluator") as e:
        TokenizerEvaluator("cuda:0", enable_lpips_score=True)
    assert "use_lpips" in str(e.value)


def test_c_entries_are_declared_and_bound():
    from maskbit_amd import _lib, build
    abi = open(os.path.join(ROOT, "include", "maskbit_hip.h")).read()
    diag = open(os.path.join(ROOT, "include", "maskbit_hip_diag.h")).read()
    for name in ("mb_lpips_create", "mb_lpips_destroy", "mb_lpips_load", "mb_lpips_forward", "mb_lpips_saturation_count"):
        assert name in _lib.SIGNATURES and re.search(r"\b%s\s*\(" % name, abi)
    for name in ("mb_conv_relu_layer", "mb_maxpool2", "mb_lpips_input", "mb_lpips_distance", "mb_lpips_features"):
        assert name in _lib.SIGNATURES and re.search(r"\b%s\s*\(" % name, diag) and not re.search(r"\b%s\s*\(" % name, abi)
    assert "#define MB_ABI_VERSION 8" in abi and _lib.ABI_VERSION == 8          # additions only
    assert "lpips.hip" in build.SOURCES
    lib = _lib.load()
    assert all(hasattr(lib, n) for n in _lib.SIGNATURES) and lib.mb_abi_version() == 8
