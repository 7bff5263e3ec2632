"""CPU-only tests of the Inception-v3 feature extractor: the float64 restatement (tests/inception_reference.py) against independent statements of
its pieces -- the resize as a direct loop, the average pool's divisor, the max pool of the last block --, the seeded weights and the error model
that is the unit of the GPU bounds, and the host side: state-dict keys and shapes, the channel bookkeeping of every concatenation, loud failure
without weights or a GPU, the C entries.  ``torch_fidelity`` and the real checkpoint are not available: nothing is held against the real network."""
import inspect
import os
import re
import socket

import pytest
import torch

import inception_reference as R
from conftest import ROOT
from maskbit_amd.synth import INCEPTION_CONCAT, INCEPTION_FC, inception_convs, make_inception_weights


# ------------------------------------------------------------------------------------------------ the restatement's pieces
def resize_loop(img, out):
    """one channel [H, W] of integers -> [out, out] float64, element by element as the specification states it"""
    H, W = img.shape
    res = torch.zeros(out, out, dtype=torch.float64)
    for y in range(out):
        sy = y * H / out
        y0 = int(sy // 1)
        y1, ty = min(y0 + 1, H - 1), sy - y0
        for x in range(out):
            sx = x * W / out
            x0 = int(sx // 1)
            x1, tx = min(x0 + 1, W - 1), sx - x0
            top = float(img[y0, x0]) + (float(img[y0, x1]) - float(img[y0, x0])) * tx
            bot = float(img[y1, x0]) + (float(img[y1, x1]) - float(img[y1, x0])) * tx
            res[y, x] = top + (bot - top) * ty
    return res


@pytest.mark.parametrize("n,out", [(4, 7), (256, 299)])
def test_resize_against_a_direct_loop(n, out):
    u8 = torch.randint(0, 256, (1, 1, n, n), generator=torch.Generator().manual_seed(n), dtype=torch.uint8)
    got, want = R.resize64(u8, out)[0, 0], resize_loop(u8[0, 0], out)
    assert got.shape == want.shape and float((got - want).abs().max()) <= 1e-10          # (sy - y0 in floating point against the integer remainder)
    assert float(got.min()) >= float(u8.min()) and float(got.max()) <= float(u8.max())
    # the first row / column are the source's: coordinate 0 maps to 0, no half-pixel offset
    assert torch.equal(got[0, 0], u8[0, 0, 0, 0].double())


def test_resize_of_the_network_size_is_the_identity():
    u8 = torch.randint(0, 256, (2, 3, 299, 299), generator=torch.Generator().manual_seed(3), dtype=torch.uint8)
    assert torch.equal(R.resize64(u8), u8.double())
    assert torch.equal(R.input64(u8), (u8.double() - 128.0) / 128.0)
    assert torch.equal(R.h16r(R.input64(u8)), R.input64(u8))                              # k / 128 with |k| <= 128 is an fp16 number


def test_average_pool_divides_by_the_taps_inside_the_image():
    net = R.Net({}, model=False)
    y = net.avg(torch.ones(1, 1, 5, 5, dtype=torch.float64))
    assert torch.equal(y, torch.ones_like(y))                                             # with the padding counted the border would drop to 4/9, 6/9
    x = torch.arange(25, dtype=torch.float64).view(1, 1, 5, 5)
    y = net.avg(x)
    assert float(y[0, 0, 0, 0]) == (0 + 1 + 5 + 6) / 4 and float(y[0, 0, 0, 2]) == (1 + 2 + 3 + 6 + 7 + 8) / 6
    assert float(y[0, 0, 2, 2]) == float(x[0, 0, 1:4, 1:4].sum()) / 9


def test_last_block_pools_with_the_maximum():
    """Mixed_7c's pool branch reads max_pool2d(3, 1, 1), Mixed_7b's the average: on a map with one hot pixel the two differ by the factor 9"""
    sd = {k: v for k, v in R.weights("he").items() if k.startswith("Mixed_7b.") or k.startswith("fc.")}
    sd = {**sd, **{k.replace("Mixed_7b.", "E."): v for k, v in sd.items()}}
    name = "E.branch_pool"
    sd[name + ".conv.weight"] = torch.ones_like(sd[name + ".conv.weight"])
    for p, v in (("weight", 1.0), ("bias", 0.0), ("running_mean", 0.0), ("running_var", 1.0 - R.BN_EPS)):
        sd[f"{name}.bn.{p}"] = torch.full_like(sd[f"{name}.bn.{p}"], v)
    x = torch.zeros(1, 1280, 8, 8, dtype=torch.float64)
    x[0, 0, 4, 4] = 9.0
    with torch.no_grad():
        avg = R.Net(sd, False).e(x, "E", use_max=False)[:, 1856:]
        mx = R.Net(sd, False).e(x, "E", use_max=True)[:, 1856:]
    assert avg.shape == (1, 192, 8, 8)
    assert torch.allclose(avg[0, 0, 3:6, 3:6], torch.ones(3, 3, dtype=torch.float64), rtol=1e-6) and float(avg[0, 0, 0, 0]) == 0
    assert torch.allclose(mx[0, 0, 3:6, 3:6], torch.full((3, 3), 9.0, dtype=torch.float64), rtol=1e-6)


# ------------------------------------------------------------------------------------------------ keys, shapes, bookkeeping
def test_state_dict_keys_and_shapes():
    from maskbit_amd import InceptionV3
    from maskbit_amd.inception import inception_keys
    convs = inception_convs()
    assert len(convs) == 94 and len({c[0] for c in convs}) == 94
    m = InceptionV3()
    sd = m.state_dict()
    assert len(sd) == 94 * 5 + 2 and set(sd) == set(inception_keys())
    for name, cin, cout, (kh, kw), stride, (ph, pw) in convs:
        assert tuple(sd[name + ".conv.weight"].shape) == (cout, cin, kh, kw)
        for p in ("weight", "bias", "running_mean", "running_var"):
            assert tuple(sd[f"{name}.bn.{p}"].shape) == (cout,)
        assert stride in (1, 2) and ph < kh and pw < kw and (cin == 3 or cin % 16 == 0) and cout % 16 == 0
    assert tuple(sd["fc.weight"].shape) == INCEPTION_FC == (1008, 2048) and tuple(sd["fc.bias"].shape) == (1008,)
    assert not any(p.requires_grad for p in m.parameters())
    # nothing is loaded at construction
    assert all(float(v.abs().sum()) == 0 for v in sd.values()) and not m._loaded
    w = R.weights("he")
    assert set(w) == set(sd) and all(w[k].shape == sd[k].shape for k in sd)
    # num_batches_tracked and entries the network does not read are accepted and ignored
    extra = {**w, "Conv2d_1a_3x3.bn.num_batches_tracked": torch.tensor(7), "AuxLogits.fc.bias": torch.zeros(3)}
    m.load_weights(extra)
    assert m._loaded and all(torch.equal(m.state_dict()[k], w[k]) for k in w)
    m2 = InceptionV3()
    m2.load_state_dict({**w, "Mixed_7c.branch_pool.bn.num_batches_tracked": torch.tensor(1)}, strict=True)
    assert m2._loaded
    with pytest.raises(KeyError):
        InceptionV3().load_weights({k: v for k, v in w.items() if k != "Mixed_6c.branch7x7dbl_4.bn.running_var"})


def test_load_from_a_file_and_the_environment(tmp_path, monkeypatch):
    from maskbit_amd import InceptionV3, get_inception_model
    from maskbit_amd.inception import WEIGHTS_ENV
    w = R.weights("tf")
    path = tmp_path / "pt_inception.pth"
    torch.save(w, path)
    m = get_inception_model(str(path))
    assert isinstance(m, InceptionV3) and m.features_list == ["2048", "logits_unbiased"] and m._loaded
    assert all(torch.equal(m.state_dict()[k], w[k]) for k in w)
    monkeypatch.setenv(WEIGHTS_ENV, str(path))
    assert get_inception_model()._loaded


def test_every_concatenation_has_its_channels():
    u8 = R.images_u8(1, 16, 16, 1)
    with torch.no_grad():
        o = R.inception64(u8, R.weights("he"))
    assert o["concat"] == INCEPTION_CONCAT
    assert [o["concat"][k] for k in ("Mixed_5b", "Mixed_5c", "Mixed_5d", "Mixed_6a", "Mixed_7a", "Mixed_7c")] == [256, 288, 288, 768, 1280, 2048]
    assert o["used"] == [c[0] for c in inception_convs()]                                    # every layer once, in the table's order
    assert [tuple(m.shape[1:]) for m in o["maps"]] == [(c, s, s) for s, c in R.MAP_SHAPES]
    assert [tuple(o[k].shape) for k in ("64", "192", "768", "2048", "logits_unbiased", "logits")] == [(1, 64), (1, 192), (1, 768), (1, 2048), (1, 1008), (1, 1008)]
    assert torch.equal(o["logits"] - o["logits_unbiased"], (o["logits_unbiased"] + R.weights("he")["fc.bias"].double()) - o["logits_unbiased"])


# ------------------------------------------------------------------------------------------------ the seeded weights
@pytest.mark.parametrize("style", ["he", "tf"])
def test_weight_styles_keep_every_tap_alive(style):
    """a condition on the inputs of the GPU tests: no tap dead or saturated, exact zeros after ReLU between 20 % and 80 %"""
    name = style + "_64"
    exact, _ = R.case_oracle(name)
    names = ("Conv2d_2b", "Conv2d_4a") + R.MAP_NAMES[1:]
    for what, t in zip(names, exact["relu"]):
        rms, mx, zeros = float(t.pow(2).mean().sqrt()), float(t.max()), float((t == 0).double().mean())
        print(f"{style} {what}: rms {rms:.3g} max {mx:.3g} zeros {zeros:.3f}")
        assert 0.1 <= rms <= 10.0 and mx < 65504 / 4 and 0.2 <= zeros <= 0.8, (what, rms, mx, zeros)
    for k in ("64", "192", "768", "2048"):
        rms = float(exact[k].pow(2).mean().sqrt())
        print(f"{style} tap {k}: rms {rms:.3g} max {float(exact[k].max()):.3g}")
        assert 0.1 <= rms <= 10.0 and float(exact[k].min()) >= 0
    assert 0.1 <= float(exact["logits_unbiased"].std()) <= 10.0
    sd = R.weights(style)
    var = torch.cat([v for k, v in sd.items() if k.endswith("running_var")])
    if style == "tf":
        assert all(bool((v == 1).all()) for k, v in sd.items() if k.endswith(".bn.weight"))
        assert float(var.max() / var.min()) > 1e3                                            # decades: the epilogue scale matters
    else:
        assert float(var.max() / var.min()) < 2


def test_weights_are_reproducible_by_seed():
    a, b, c = make_inception_weights(7, "tf"), make_inception_weights(7, "tf"), make_inception_weights(8, "tf")
    assert list(a) == list(b) and all(torch.equal(a[k], b[k]) for k in a) and not torch.equal(a["fc.weight"], c["fc.weight"])
    with pytest.raises(ValueError):
        make_inception_weights(0, "kaiming")


@pytest.mark.parametrize("name", list(R.CASES))
def test_error_model_is_positive(name):
    """E_model = |model - exact|: what fp16 weights and fp16 stored activations cost; the unit of the GPU bounds"""
    exact, model = R.case_oracle(name)
    for k, (m, x) in enumerate(zip(model["maps"], exact["maps"])):
        rel = float((m - x).pow(2).mean().sqrt() / x.pow(2).mean().sqrt())
        print(f"{name} {R.MAP_NAMES[k]}: model error {rel:.2e} of the rms")
        assert 1e-4 < rel < 5e-3, (k, rel)                      # between a fifth of and ten times the unit roundoff 2^-11 after up to 40 layers
    for k in ("64", "192", "768", "2048", "logits_unbiased", "logits"):
        e = float((model[k] - exact[k]).abs().max())
        print(f"{name} {k}: E {e:.3e}, values of rms {float(exact[k].pow(2).mean().sqrt()):.3g}")
        assert 0 < e < 0.02


# ------------------------------------------------------------------------------------------------ the host side
def test_forward_without_weights_or_gpu_raises():
    from maskbit_amd import InceptionV3
    x = torch.zeros(1, 3, 32, 32, dtype=torch.uint8)
    with pytest.raises(RuntimeError, match="load_weights"):
        InceptionV3()(x)
    m = InceptionV3()
    m.load_weights(R.weights("he"))
    with pytest.raises(RuntimeError, match="no CPU path"):
        m(x)
    with pytest.raises(ValueError):
        InceptionV3(["2048", "fc"])
    assert InceptionV3(["64", "logits"]).features_list == ["64", "logits"]
    assert list(inspect.signature(InceptionV3.__init__).parameters) == ["self", "features_list"]


def test_get_inception_model_without_a_path_raises_and_opens_no_socket(monkeypatch):
    from maskbit_amd import get_inception_model
    from maskbit_amd.inception import WEIGHTS_ENV, WEIGHTS_FILE

    def no_socket(*a, **k):
        raise AssertionError("get_inception_model tried to open a socket")

    monkeypatch.setattr(socket, "socket", no_socket)
    monkeypatch.setattr(socket, "create_connection", no_socket)
    monkeypatch.delenv(WEIGHTS_ENV, raising=False)
    with pytest.raises(RuntimeError, match=re.escape(WEIGHTS_FILE)):
        get_inception_model()
    # by construction: the module imports nothing that could fetch
    src = open(os.path.join(ROOT, "maskbit_amd", "inception.py")).read()
    assert not re.search(r"^\s*(import|from)\s+(urllib|requests|http|socket|torch\.hub|torch_fidelity)", src, re.M)
    assert "load_state_dict_from_url" not in src and "http" not in src


def test_check_images_rejects_without_device_work():
    from maskbit_amd import InceptionV3
    ok = torch.zeros(2, 3, 37, 50, dtype=torch.uint8)
    InceptionV3.check_images(ok)
    InceptionV3.check_images(torch.zeros(1, 3, 2, 2, dtype=torch.uint8))
    for bad in (ok.float(), ok.to(torch.int64), torch.zeros(2, 1, 37, 50, dtype=torch.uint8), torch.zeros(2, 4, 37, 50, dtype=torch.uint8),
                torch.zeros(3, 37, 50, dtype=torch.uint8), torch.zeros(0, 3, 37, 50, dtype=torch.uint8), torch.zeros(1, 3, 1, 50, dtype=torch.uint8)):
        with pytest.raises(ValueError):
            InceptionV3.check_images(bad)
    with pytest.raises(TypeError):
        InceptionV3.check_images([[0]])
    m = InceptionV3()
    m.load_weights(R.weights("he"))
    with pytest.raises(ValueError):                             # the shape check comes before the device check
        m(ok.float())


def test_evaluators_take_it_unchanged():
    from maskbit_amd import GeneratorEvaluator, InceptionV3, TokenizerEvaluator
    assert list(inspect.signature(GeneratorEvaluator.use_inception).parameters) == ["self", "extractor", "real_statistics"]
    assert list(inspect.signature(TokenizerEvaluator.use_inception).parameters) == ["self", "extractor", "rfid", "inception_score"]
    assert callable(InceptionV3())


def test_c_entries_are_declared_and_bound():
    from maskbit_amd import _lib, build
    abi = open(os.path.join(ROOT, "include", "maskbit_hip.h")).read()
    diag = open(os.path.join(ROOT, "include", "maskbit_hip_diag.h")).read()
    for name in ("mb_inception_create", "mb_inception_destroy", "mb_inception_load", "mb_inception_forward", "mb_inception_saturation_count"):
        assert name in _lib.SIGNATURES and re.search(r"\b%s\s*\(" % name, abi)
    for name in ("mb_convbn_layer", "mb_pool3", "mb_inception_input", "mb_inception_taps", "mb_bn_fold", "mb_spatial_mean", "mb_fc_head",
                 "mb_channel_tap", "mb_inception_folded_bn"):
        assert name in _lib.SIGNATURES and re.search(r"\b%s\s*\(" % name, diag) and not re.search(r"\b%s\s*\(" % name, abi)
    assert "#define MB_ABI_VERSION 8" in abi and _lib.ABI_VERSION == 8          # additions only
    assert "inception.hip" in build.SOURCES
    lib = _lib.load()
    assert all(hasattr(lib, n) for n in _lib.SIGNATURES) and lib.mb_abi_version() == 8
