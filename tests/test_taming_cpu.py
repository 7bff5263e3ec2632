"""CPU checks of the Taming VQGAN tokenizer (maskbit_amd.OriginalVQModel): the float64 restatement of tests/taming_reference.py pinned to the
reference's fixture (tests/golden/tok_taming_full.npz, tools/make_golden_taming.py), the state dict against the reference's recorded names and
shapes, load_pretrained, the import shims and the argument checks that need no device."""
import hashlib
import os
import re

import pytest
import torch

import taming_reference as TR
from conftest import ROOT, load_golden
from maskbit_amd.synth import make_taming_weights, make_vq_codebook

_CACHE = {}


def fixture():
    """-> (fixture dict, state dict with the codebook, the two images)"""
    if not _CACHE:
        z = load_golden("tok_taming_full.npz")
        seed = int(z["seed"])
        sd = make_taming_weights(seed, float(z["qk_gain"]))
        sd["quantize.embedding.weight"] = make_vq_codebook(1024, 256, seed + 2, torch.from_numpy(z["cb_mean"]), torch.from_numpy(z["cb_std"]))
        x = torch.rand(2, 3, 256, 256, generator=torch.Generator().manual_seed(seed + 1))
        _CACHE["f"] = (z, sd, x)
    return _CACHE["f"]


def forward64():
    """The restatement's whole forward on the fixture's images, once per session."""
    if "fw" not in _CACHE:
        z, sd, x = fixture()
        taps = {}
        with torch.no_grad():
            lat = TR.latent(sd, x, taps)
            zq, idx, d, losses = TR.quantize(sd, lat)
            rec = TR.decode_tokens(sd, torch.from_numpy(z["indices"]), taps)
        _CACHE["fw"] = (lat, zq, idx, d, losses, rec, taps)
    return _CACHE["fw"]


def sha(t):
    return hashlib.sha256(t.detach().contiguous().numpy().tobytes()).hexdigest()


def test_seeded_weights_match_the_fixture_sentinels():
    z, sd, x = fixture()
    assert sha(sd["encoder.conv_in.weight"]) == str(z["w_sha_conv_in"])
    assert sha(sd["quantize.embedding.weight"]) == str(z["cb_sha"])
    assert len(sd) == 343
    plain = make_taming_weights(int(z["seed"]), 1.0)
    g = float(z["qk_gain"])
    for k in sd:
        if k == "quantize.embedding.weight":
            continue
        scaled = k.split(".")[-2] in ("q", "k")
        assert torch.equal(sd[k], plain[k] * g if scaled else plain[k]), k


def test_fixture_attention_is_not_uniform():
    z, _, _ = fixture()
    mp = z["max_prob"]
    assert mp.shape == (7,) and bool(((mp >= 0.2) & (mp <= 0.9)).all())


def test_restatement_latent_and_indices_match_reference():
    z, sd, x = fixture()
    lat, zq, idx, d, losses, rec, taps = forward64()
    zref = torch.from_numpy(z["z"]).double()
    err = float((lat - zref).abs().max())
    print(f"restatement latent: max abs difference to the reference's fp32 latent {err:.3g}")
    assert err < 1e-4                                                   # fp32 against fp64 of the same network
    # indices: equal wherever the recorded best-to-second gap is not within fp32 noise of zero (the reference's distances are fp32 sums of
    # magnitude `scale`: 1e-5 of it is ~100 ulp)
    gap, scale = torch.from_numpy(z["gap"]), torch.from_numpy(z["scale"])
    clear = gap > 1e-5 * scale
    assert float(clear.float().mean()) > 0.99
    ref = torch.from_numpy(z["indices"]).flatten()
    assert torch.equal(idx.flatten()[clear], ref[clear])
    # the recorded gap is the fp64 gap of the reference's own latent
    top2 = d.topk(2, dim=1, largest=False).values
    assert float(((top2[:, 1] - top2[:, 0]) - gap.double()).abs().max()) < 1e-2
    for k in ("codebook_loss", "commitment_loss", "quantizer_loss"):
        assert abs(float(losses[k]) - float(z[k])) <= 1e-4 * float(z[k])
    assert torch.equal(zq, sd["quantize.embedding.weight"].double()[idx].permute(0, 3, 1, 2))


def test_restatement_reconstruction_matches_reference():
    z, sd, x = fixture()
    rec = forward64()[5]
    for (y, xx) in ((0, 0), (120, 120), (240, 240), (37, 201)):
        err = float((rec[:, :, y:y + 16, xx:xx + 16] - torch.from_numpy(z[f"crop_{y}_{xx}"]).double()).abs().max())
        assert err < 1e-4, (y, xx, err)
    half = torch.from_numpy(z["recon_half"]).double()
    assert float((rec[:, :, ::2, ::2] - half).abs().max()) < 1e-4 + 2e-3       # (the fixture stores this array as fp16)


def test_restatement_attention_rows_match_reference():
    z, sd, x = fixture()
    taps = forward64()[6]
    rows = [int(r) for r in z["hook_rows"]]
    for name, key in ((TR.ATTN[0], "attn_enc_first"), (TR.ATTN[-1], "attn_dec_last")):
        ours = taps[name].permute(0, 2, 3, 1).reshape(2, 256, 512)[:, rows]
        ref = torch.from_numpy(z[key]).double()
        assert float((ours - ref).abs().max()) < 1e-4 * max(1.0, float(ref.abs().max())), name
    assert set(taps) == set(TR.ATTN)


def test_downsample_is_the_space_to_depth_conv():
    """Downsample (zero column right / row below, 3x3 stride 2, no padding) on an even size = the 2x2 convolution on the space-to-depth input
    with the 3x3 kernel's taps regrouped, which is what the engine executes (shape_down_conv / launch_s2d)."""
    g = torch.Generator().manual_seed(3)
    x = torch.randn(1, 4, 8, 8, generator=g, dtype=torch.float64)
    w = torch.randn(5, 4, 3, 3, generator=g, dtype=torch.float64)
    b = torch.randn(5, generator=g, dtype=torch.float64)
    ref = TR.downsample({"d.conv.weight": w, "d.conv.bias": b}, "d", x)
    s2d = torch.cat([x[:, :, py::2, px::2] for py in (0, 1) for px in (0, 1)], dim=1)            # channel (py * 2 + px) * C + c
    w2 = torch.zeros(5, 16, 2, 2, dtype=torch.float64)
    for by in (0, 1):
        for bx in (0, 1):
            for py in (0, 1):
                for px in (0, 1):
                    dy, dx = 2 * by + py, 2 * bx + px
                    if dy < 3 and dx < 3:
                        w2[:, (py * 2 + px) * 4:(py * 2 + px + 1) * 4, by, bx] = w[:, :, dy, dx]
    out = torch.nn.functional.conv2d(torch.nn.functional.pad(s2d, (0, 1, 0, 1)), w2, b)
    assert float((out - ref).abs().max()) < 1e-12


def test_state_dict_matches_reference():
    from maskbit_amd import OriginalVQModel
    z = load_golden("tok_taming_statedict.npz")
    m = OriginalVQModel(None)
    ours = [(k, tuple(v.shape)) for k, v in m.state_dict().items()]
    ref = [(str(k), tuple(int(v) for v in s if v >= 0)) for k, s in zip(z["names"], z["shapes"])]
    assert ours == ref                                                 # names, shapes and order
    assert len(ours) == 343 and m.num_parameters() == int(z["num_parameters"]) == 72_141_699
    assert float(m.quantize.embedding.weight.detach().abs().max()) <= 1.0 / 1024
    m.load_state_dict(make_taming_weights(1), strict=True)


def test_shim_and_package_exports():
    import maskbit_amd
    from modeling.taming_vqgan import OriginalVQModel
    assert OriginalVQModel is maskbit_amd.OriginalVQModel and "OriginalVQModel" in maskbit_amd.__all__
    assert issubclass(OriginalVQModel, maskbit_amd.BaseModel)
    OriginalVQModel(object())                                          # the argument is ignored
    for meth in ("encode", "decode", "decode_tokens", "decode_tokens_uint8", "forward", "load_pretrained", "saturation_count"):
        assert callable(getattr(OriginalVQModel, meth))


def test_load_pretrained(tmp_path):
    from maskbit_amd import OriginalVQModel
    sd = make_taming_weights(5)
    wrapped = {"state_dict": {**sd, "loss.discriminator.main.0.weight": torch.zeros(3), "loss.logvar": torch.zeros(())}}
    f = tmp_path / "taming.ckpt"
    torch.save(wrapped, f)
    m = OriginalVQModel(None).train()
    m.load_pretrained(str(f))
    assert not m.training
    assert all(torch.equal(v, sd[k]) for k, v in m.state_dict().items())
    d = tmp_path / "dir"
    d.mkdir()
    torch.save(sd, d / "pytorch_model.bin")                            # a flat state dict, directory form
    m2 = OriginalVQModel(None)
    m2.load_pretrained(d)
    assert torch.equal(m2.state_dict()["decoder.up.4.attn.2.q.weight"], sd["decoder.up.4.attn.2.q.weight"])
    short = dict(sd)
    del short["encoder.mid.attn_1.k.bias"]
    torch.save(short, f)
    with pytest.raises(RuntimeError, match="encoder.mid.attn_1.k.bias"):
        OriginalVQModel(None).load_pretrained(str(f))
    OriginalVQModel(None).load_pretrained(str(f), strict_loading=False)
    with pytest.raises(ValueError):
        OriginalVQModel(None).load_pretrained(str(tmp_path / "missing"))
    with pytest.raises(ValueError):
        OriginalVQModel(None).load_pretrained(str(tmp_path))            # a directory without pytorch_model.bin


def test_argument_checks_need_no_device():
    from maskbit_amd import OriginalVQModel
    m = OriginalVQModel(None)                                            # on the CPU: anything that reached the engine would raise RuntimeError
    for shape in ((1, 3, 128, 128), (1, 3, 256, 512), (1, 3, 384, 384), (1, 1, 256, 256), (3, 256, 256)):
        with pytest.raises(ValueError):
            m.encode(torch.zeros(shape))
        with pytest.raises(ValueError):
            m(torch.zeros(shape))
    with pytest.raises(ValueError):
        m.decode_tokens(torch.zeros(1, 64, dtype=torch.long))
    with pytest.raises(ValueError):
        m.decode(torch.zeros(1, 256, 8, 8))
    with pytest.raises(ValueError):
        m.decode(torch.zeros(1, 64, 16, 16))
    with pytest.raises(IndexError):
        m.decode_tokens(torch.full((1, 256), 1024))
    with pytest.raises(IndexError):
        m.decode_tokens_uint8(torch.full((1, 1024), -1))
    with pytest.raises(RuntimeError, match="no CPU path"):
        m.decode_tokens(torch.zeros(1, 256, dtype=torch.long))
    assert m.saturation_count() == 0


def test_sampler_refuses_the_taming_tokenizer():
    from maskbit_amd import LFQBert, OriginalVQModel, inpaint, sample, sample_from_tokens, sample_seeded
    gen = LFQBert(img_size=256, hidden_dim=128, codebook_size=1024, codebook_splits=2, depth=1, heads=4, mlp_dim=256, dropout=0.0, nclass=10,
                  input_stride=16)
    tok = OriginalVQModel(None)
    with pytest.raises(TypeError, match="OriginalVQModel"):
        sample(gen, tok, num_samples=1, labels=torch.tensor([1]), mask_token=32, codebook_size=1024, codebook_splits=2, num_steps=2)
    with pytest.raises(TypeError, match="OriginalVQModel"):
        sample_seeded(gen, tok, torch.tensor([1]), torch.tensor([1]), num_steps=2)
    with pytest.raises(TypeError, match="OriginalVQModel"):
        sample_from_tokens(gen, tok, torch.full((1, 256, 2), 32, dtype=torch.long), torch.tensor([1]), num_steps=2)
    with pytest.raises(TypeError, match="OriginalVQModel"):
        inpaint(gen, tok, torch.zeros(1, 3, 256, 256), torch.ones(1, 256, 256, dtype=torch.bool), torch.tensor([1]), num_steps=2)


def test_abi_additions():
    from maskbit_amd import _lib
    abi = open(os.path.join(ROOT, "include", "maskbit_hip.h")).read()
    diag = open(os.path.join(ROOT, "include", "maskbit_hip_diag.h")).read()
    assert re.search(r"#define MB_ABI_VERSION 8\b", abi) and _lib.ABI_VERSION == 8              # additions only
    lib = _lib.load()
    for name in ("mb_taming_create", "mb_taming_destroy", "mb_taming_load", "mb_taming_encode", "mb_taming_decode", "mb_taming_decode_latent",
                 "mb_taming_saturation_count"):
        assert re.search(rf"\b{name}\(", abi) and name in _lib.SIGNATURES and hasattr(lib, name)
    for name in ("mb_spatial_attention", "mb_taming_set_tap"):
        assert re.search(rf"\b{name}\(", diag) and name in _lib.SIGNATURES and hasattr(lib, name)
    # refusals that need no device
    import ctypes as C
    h = C.c_void_p()
    assert lib.mb_taming_create(1, 24, C.byref(h)) == -1 and b"latent_size" in lib.mb_last_error()
    assert lib.mb_spatial_attention(None, None, None, None, None, 1, 16, 512, 512, None) == -1
