"""CPU-only tests of the ResNet-50 perceptual loss: the resize of tests/resnet_reference.py against torch's own antialiased ``F.interpolate``, the
written-out network's parameter count and key list, both loader layouts, loud failure without weights or a GPU, and the C entries (declared, bound,
refusing bad arguments before any device work).  torchvision and the ImageNet checkpoint are not available: nothing is held against the real network."""
import ctypes as C
import inspect
import os
import re

import pytest
import torch
import torch.nn.functional as F

import resnet_reference as R
from conftest import ROOT
from maskbit_amd.synth import make_resnet50_weights, resnet50_convs


# ------------------------------------------------------------------------------------------------ the restatement's pieces
@pytest.mark.parametrize("H,W", R.RESIZE_SIZES)
def test_resize_matrices_against_torch(H, W):
    x = torch.rand(2, 3, H, W, generator=torch.Generator().manual_seed(H + W), dtype=torch.float64)
    want = F.interpolate(x, size=R.SIDE, mode="bilinear", antialias=True, align_corners=False)
    got = R.resize64(x)
    err = float((got - want).abs().max())
    print(f"resize {H}x{W}: max |matrix form - F.interpolate| {err:.2e}")
    assert got.shape == want.shape and err <= 1e-12


def test_resize_of_the_network_size_is_the_identity_and_taps_fit_the_kernel():
    assert torch.equal(R.resize_matrix(224), torch.eye(224, dtype=torch.float64))
    for n in (32, 33, 224, 225, 447, 448, 1000, 1023, 1024):
        taps = R.resize_taps(n)
        assert max(len(w) for _lo, w in taps) <= 12                # RN_MAXT of csrc/mb_resnet.h
        assert all(abs(sum(w) - 1.0) < 1e-15 and lo >= 0 and lo + len(w) <= n for lo, w in taps)


def test_stem_cols_are_the_convolution():
    """the fold: conv1 on the image == a 1x1 convolution with the weight read as [64, 147] on the patches"""
    g = torch.Generator().manual_seed(1)
    img = torch.randn(2, 3, 18, 18, generator=g, dtype=torch.float64)
    w = torch.randn(64, 3, 7, 7, generator=g, dtype=torch.float64)
    cols = R.stem_cols64(img)
    assert tuple(cols.shape) == (2, 9, 9, 147)
    got = (cols @ w.reshape(64, 147).T).permute(0, 3, 1, 2)
    assert float((got - F.conv2d(img, w, None, 2, 3)).abs().max()) < 1e-12


def test_model_rounding_is_a_small_positive_error():
    sd = R.weights()
    img = torch.randn(1, 3, 32, 32, generator=torch.Generator().manual_seed(2)).to(torch.float16).double()
    with torch.no_grad():
        exact, model = R.trunk64(img, sd, False), R.trunk64(img, sd, True)
    assert [tuple(m.shape[1:]) for m in exact["maps"]] == [(256, 8, 8), (512, 4, 4), (1024, 2, 2), (2048, 1, 1)]
    for ex, mo in zip(exact["maps"], model["maps"]):
        e = float((ex - mo).abs().max())
        rms = float(ex.pow(2).mean().sqrt())
        zeros = float((ex == 0).double().mean())
        assert 0 < e < 0.05 * rms and 0.1 < rms < 10 and 0.1 < zeros < 0.9, (e, rms, zeros)     # no layer dead, grown or saturated
    E = float((exact["logits"] - model["logits"]).abs().max())
    assert 0 < E < 0.05 and float(exact["logits"].abs().max()) > 0.5


# ------------------------------------------------------------------------------------------------ keys and loaders
def test_parameter_count_and_keys():
    from maskbit_amd import PerceptualLoss
    from maskbit_amd.perceptual import perceptual_keys, resnet50_keys
    m = PerceptualLoss()
    written = R.written_out_keys()
    sd = m.state_dict()
    assert sorted(sd) == sorted(k for k, _ in written) and list(sd) == perceptual_keys()
    assert all(tuple(sd[k].shape) == tuple(s) for k, s in written)
    assert m.num_parameters() == R.PARAMETERS == 25_557_032
    assert sum(v.numel() for k, v in make_resnet50_weights(0).items() if not k.endswith(("running_mean", "running_var", "num_batches_tracked"))) == R.PARAMETERS
    assert len(resnet50_convs()) == 53 and len(resnet50_keys()) == 320 and len(resnet50_keys(counters=False)) == 267
    assert torch.equal(sd["mean"].flatten(), torch.tensor(R.MEAN)) and torch.equal(sd["std"].flatten(), torch.tensor(R.STD))
    assert all(not p.requires_grad for p in m.parameters()) and not m.training
    assert list(inspect.signature(PerceptualLoss.__init__).parameters) == ["self", "model_name", "compute_perceptual_loss_on_logits"]


def test_both_loader_layouts_map_onto_the_keys(tmp_path):
    from maskbit_amd import PerceptualLoss
    tv = R.weights()
    ref = R.reference_layout(tv)
    a, b, c = PerceptualLoss(), PerceptualLoss(), PerceptualLoss()
    a.load_resnet50(tv)
    b.load_resnet50(ref)
    c.load_state_dict(ref, strict=True)                           # a reference VQGANLoss checkpoint's perceptual_loss.* entries
    path = tmp_path / "resnet50.pth"
    torch.save(tv, path)
    d = PerceptualLoss()
    d.load_resnet50(str(path))
    for m in (a, b, c, d):
        assert m._loaded
        sd = m.state_dict()
        assert all(torch.equal(sd["model." + k], v) for k, v in tv.items())
    short = {k: v for k, v in tv.items() if k != "layer3.4.bn2.running_var"}
    with pytest.raises(KeyError, match="layer3.4.bn2.running_var"):
        PerceptualLoss().load_resnet50(short)
    no_counters = {k: v for k, v in tv.items() if not k.endswith("num_batches_tracked")}
    e = PerceptualLoss()
    e.load_resnet50(no_counters)
    assert e._loaded


def test_convnext_raises_and_the_factory_dispatches():
    from maskbit_amd import LPIPS, PerceptualLoss, create_perception_loss
    import modeling.modules as MM
    with pytest.raises(NotImplementedError, match="ConvNeXt"):
        PerceptualLoss("convnext_s")
    with pytest.raises(NotImplementedError):
        create_perception_loss("convnext_s")
    with pytest.raises(ValueError):
        PerceptualLoss("vgg")
    with pytest.raises(ValueError):
        create_perception_loss("nothing")
    assert isinstance(create_perception_loss("lpips"), LPIPS)
    p = create_perception_loss("resnet50", compute_on_logits=False)
    assert isinstance(p, PerceptualLoss) and p.compute_perceptual_loss_on_logits is False and not p.training
    assert create_perception_loss("resnet50").compute_perceptual_loss_on_logits is True
    assert MM.PerceptualLoss is PerceptualLoss and MM.create_perception_loss is create_perception_loss


def test_forward_without_weights_or_gpu_raises():
    from maskbit_amd import PerceptualLoss
    x = torch.zeros(1, 3, 64, 64)
    with pytest.raises(RuntimeError, match="load_resnet50"):
        PerceptualLoss()(x, x)
    m = PerceptualLoss()
    m.load_resnet50(R.weights())
    with pytest.raises(RuntimeError, match="no CPU path"):
        m(x, x)
    for bad in (torch.zeros(1, 3, 31, 64), torch.zeros(1, 3, 64, 1025), torch.zeros(1, 1, 64, 64), torch.zeros(3, 64, 64), torch.zeros(0, 3, 64, 64)):
        with pytest.raises(ValueError):
            m(bad, bad)
    with pytest.raises(ValueError):
        m(x, torch.zeros(2, 3, 64, 64))
    src = open(os.path.join(ROOT, "maskbit_amd", "perceptual.py")).read()
    assert not re.search(r"^\s*(import|from)\s+(urllib|requests|http|socket|torch\.hub|torchvision)", src, re.M)


def test_evaluator_surface():
    from maskbit_amd import TokenizerEvaluator
    assert list(inspect.signature(TokenizerEvaluator.use_perceptual).parameters) == ["self", "model"]


# ------------------------------------------------------------------------------------------------ the C side
def test_c_entries_are_declared_and_bound():
    from maskbit_amd import _lib, build
    abi = open(os.path.join(ROOT, "include", "maskbit_hip.h")).read()
    diag = open(os.path.join(ROOT, "include", "maskbit_hip_diag.h")).read()
    for name in ("mb_resnet_create", "mb_resnet_destroy", "mb_resnet_load", "mb_resnet_forward", "mb_resnet_saturation_count"):
        assert name in _lib.SIGNATURES and re.search(r"\b%s\s*\(" % name, abi)
    for name in ("mb_convbn_layer_ex", "mb_pool3_ex", "mb_resnet_input", "mb_resnet_stem_cols", "mb_resnet_distance", "mb_resnet_taps",
                 "mb_resnet_folded_bn"):
        assert name in _lib.SIGNATURES and re.search(r"\b%s\s*\(" % name, diag) and not re.search(r"\b%s\s*\(" % name, abi)
    assert "#define MB_ABI_VERSION 8" in abi and _lib.ABI_VERSION == 8          # additions only
    assert "resnet.hip" in build.SOURCES
    lib = _lib.load()
    assert all(hasattr(lib, n) for n in _lib.SIGNATURES) and lib.mb_abi_version() == 8


def test_argument_refusals_need_no_device():
    """every refusal below returns before the first HIP call: non-zero, with a message, on a machine without a GPU"""
    from maskbit_amd import _lib
    lib = _lib.load()
    buf = (C.c_float * 64)()
    p = C.addressof(buf)
    sat = C.c_uint(0)
    h = C.c_void_p()
    assert lib.mb_resnet_create(0, C.byref(h)) != 0 and lib.mb_resnet_create(1, None) != 0
    assert lib.mb_resnet_forward(None, p, p, 1, 64, 64, 0, 1, p, None, None) != 0
    assert lib.mb_resnet_taps(None, p, 1, 64, None, None, None, None, None, None, None) != 0
    assert lib.mb_resnet_load(None, b"conv1.weight", p, None, 0, None) != 0
    assert lib.mb_resnet_saturation_count(None, C.byref(sat), 0, None) != 0

    def conv(**kw):
        a = dict(B=1, H=9, W=9, cin=32, cout=32, kh=1, kw=1, stride=1, ph=0, pw=0, in_off=0, in_cs=32, out_off=0, out_cs=32, variant=0, epilogue=2)
        a.update(kw)
        idn = a.pop("idn", p)
        tail = (a.pop("idn_off", 0), a.pop("idn_cs", 32))
        return lib.mb_convbn_layer_ex(p, p, p, p, p, C.byref(sat), *a.values(), idn, *tail, None)

    for bad in (dict(epilogue=3), dict(epilogue=-1), dict(idn=None), dict(idn_off=2), dict(idn_cs=30), dict(idn_off=4), dict(stride=3), dict(variant=3)):
        assert conv(**bad) != 0, bad
        assert lib.mb_last_error()
    pool = dict(B=1, H=9, W=9, C=64, mode=3, in_off=0, in_cs=64, out_off=0, out_cs=64)
    for bad in (dict(mode=4), dict(mode=-1), dict(C=60), dict(in_cs=60), dict(out_off=4), dict(B=0)):
        assert lib.mb_pool3_ex(p, p, *{**pool, **bad}.values(), None) != 0, bad
    assert lib.mb_pool3(p, p, *pool.values(), None) != 0           # mb_pool3 keeps its three modes
    for H, W in ((31, 64), (64, 1025), (0, 0)):
        assert lib.mb_resnet_input(p, p, p, p, None, 1, H, W, 0, None) != 0
    assert lib.mb_resnet_input(None, p, p, p, None, 1, 64, 64, 0, None) != 0
    assert lib.mb_resnet_stem_cols(p, p, 1, 6, None) != 0 and lib.mb_resnet_stem_cols(None, p, 1, 32, None) != 0
    assert lib.mb_resnet_distance(p, None, 0, 1000, 0, p, None, None) != 0
    assert lib.mb_resnet_distance(p, p, 1, 1000, 12, p, None, None) != 0
    assert lib.mb_resnet_distance(None, None, 1, 1000, 0, p, None, None) != 0
    # the tail both networks share (include/maskbit_hip_diag.h): each -1
    assert lib.mb_bn_fold(p, p, p, 0, 1e-5, None) == -1 and lib.mb_bn_fold(p, p, p, 8, -1.0, None) == -1 and lib.mb_bn_fold(None, p, p, 8, 1e-5, None) == -1
    for B, HW, C_ in ((1, 4, 12), (1, 0, 8), (0, 4, 8), (1, 4, 0)):
        assert lib.mb_spatial_mean(p, p, B, HW, C_, None) == -1
    for B, D, N in ((1, 2047, 4), (1, 2304, 4), (1, 0, 4), (0, 256, 4), (1, 256, 0)):
        assert lib.mb_fc_head(p, p, p, p, p, B, D, N, None) == -1, (B, D, N)
    assert lib.mb_fc_head(p, p, p, None, None, 1, 256, 4, None) == -1 and lib.mb_fc_head(None, p, p, p, None, 1, 256, 4, None) == -1
    for B, HW, C_, off, cs in ((1, 4, 8, 17, 24), (1, 4, 8, -8, 24), (1, 4, 0, 0, 24), (0, 4, 8, 0, 24), (1, 0, 8, 0, 24)):
        assert lib.mb_channel_tap(p, p, B, HW, C_, off, cs, None) == -1
    assert lib.mb_resnet_folded_bn(None, b"bn1", p, p, 64, None) == -1 and lib.mb_inception_folded_bn(None, b"Conv2d_1a_3x3.bn", p, p, 32, None) == -1
    assert b"mb_inception_folded_bn" in lib.mb_last_error()
