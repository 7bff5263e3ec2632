"""CPU checks of the lookup (VQ) tokenizer surface: the shipped configs' state dicts against the reference's recorded names and shapes, the
legacy (MaskGIT) layout, an fp64 restatement of SimpleVectorizer against the reference's indices, and the sampler's codebook check."""
import pytest
import torch

from conftest import load_golden
from hip_helpers import Cfg
from maskbit_amd.synth import TokCfg, make_tokenizer_weights, make_vq_codebook

SHIPPED = {
    "vqgan_plus_10bit": (dict(codebook_size=1024, token_size=256, sample_with_conv=True), False),
    "vqgan_plus_12bit": (dict(codebook_size=4096, token_size=64, sample_with_conv=True), False),
    "maskgit": (dict(codebook_size=1024, token_size=256, sample_with_conv=False, entropy_loss_weight=0.02), True),
}


def vq_cfg(**over):
    c = Cfg(quantizer_type="lookup", codebook_size=1024, token_size=256, commitment_cost=0.25, entropy_loss_weight=0.0,
            entropy_loss_temperature=0.01, entropy_gamma=1.0, num_channels=3, hidden_channels=128, channel_mult=[1, 1, 2, 2, 4],
            num_resolutions=5, num_res_blocks=2, sample_with_conv=True)
    c.update(over)
    return c


@pytest.mark.parametrize("name", list(SHIPPED))
def test_shipped_config_state_dict_matches_reference(name):
    from maskbit_amd import ConvVQModel
    over, legacy = SHIPPED[name]
    m = ConvVQModel(vq_cfg(**over), legacy=legacy)
    z = load_golden("tok_vq_statedicts.npz")
    ref = {str(k): tuple(int(v) for v in s if v >= 0) for k, s in zip(z[name + "_names"], z[name + "_shapes"])}
    ours = {k: tuple(v.shape) for k, v in m.state_dict().items()}
    assert ours == ref
    assert m.codebook_size == over["codebook_size"]
    w = m.quantize.embedding.weight
    assert float(w.detach().abs().max()) <= 1.0 / over["codebook_size"]            # uniform(+-1/C), quantizer.py:37


def test_legacy_layout_loads_strict_and_remaps():
    from maskbit_amd import ConvVQModel
    from maskbit_amd.conv_vqgan import legacy_to_canonical
    over, _ = SHIPPED["maskgit"]
    cfg = vq_cfg(**over, num_res_blocks_decoder=3)                           # the legacy decoder ignores num_res_blocks_decoder
    leg = ConvVQModel(cfg, legacy=True)
    sd = {k: torch.randn(v.shape) for k, v in leg.state_dict().items()}
    leg.load_state_dict(sd, strict=True)
    assert "decoder.up.0.upsample_conv.weight" not in sd and "decoder.up.4.upsample_conv.weight" in sd   # up.0 = finest level
    assert sd["decoder.up.0.res_blocks.0.conv1.weight"].shape == (128, 128, 3, 3)
    can = ConvVQModel(vq_cfg(**over), legacy=False)
    remapped = legacy_to_canonical(sd, 5)
    can.load_state_dict(remapped, strict=True)
    for k, v in can.state_dict().items():
        assert torch.equal(v, remapped[k])
    assert torch.equal(remapped["decoder.up.0.upsample_conv.weight"], sd["decoder.up.4.upsample_conv.weight"])


def test_quantizer_types():
    from maskbit_amd import ConvVQModel
    with pytest.raises(NotImplementedError):
        ConvVQModel(vq_cfg(quantizer_type="vae"))
    with pytest.raises(NotImplementedError):
        ConvVQModel(vq_cfg(quantizer_type="nearest"))
    with pytest.raises(ValueError):
        ConvVQModel(vq_cfg(token_size=320))
    lfq = ConvVQModel(vq_cfg(quantizer_type="lookup-free", token_size=12, codebook_size=4096))
    assert "quantize.codebook" in lfq.state_dict() and "quantize.embedding.weight" not in lfq.state_dict()


def _simple_vectorizer_fp64(z, emb, l2):
    zf = z.permute(0, 2, 3, 1).reshape(-1, z.shape[1]).double()
    e = emb.double()
    if l2:
        zf = torch.nn.functional.normalize(zf, dim=-1)
        e = torch.nn.functional.normalize(e, dim=-1)
    d = zf.pow(2).sum(1, keepdim=True) + e.pow(2).sum(1) - 2 * zf @ e.T
    idx = d.argmin(1)
    zq = e[idx]
    return idx, float((zq - zf).pow(2).mean())


def _fixture_codebook(z, name):
    if "codebook" in z:
        return torch.from_numpy(z["codebook"])
    K = z["z"].shape[1]
    C = {64: 4096, 256: 1024}[K]
    return make_vq_codebook(C, K, int(z["seed"]) + 2, torch.from_numpy(z["cb_mean"]), torch.from_numpy(z["cb_std"]))


@pytest.mark.parametrize("name,tag", [("tok_vq_tiny.npz", ""), ("tok_vq_tiny.npz", "l2_"), ("tok_vq_legacy256_tiny.npz", ""),
                                      ("tok_vq_full12.npz", ""), ("tok_vq_full10.npz", "")])
def test_fp64_restatement_reproduces_reference_indices(name, tag):
    z = load_golden(name)
    emb = _fixture_codebook(z, name)
    if "cb_sha" in z:
        import hashlib
        assert hashlib.sha256(emb.contiguous().numpy().tobytes()).hexdigest() == str(z["cb_sha"])
    idx, loss = _simple_vectorizer_fp64(torch.from_numpy(z[tag + "z"]), emb, bool(tag))
    ref = torch.from_numpy(z[tag + "indices"]).flatten()
    clear = torch.from_numpy(z[tag + "gap"]) > 1e-6 * torch.from_numpy(z[tag + "scale"])
    assert bool(clear.float().mean() > 0.9)
    assert torch.equal(idx[clear], ref[clear])
    assert abs(loss - float(z[tag + "codebook_loss"])) <= 1e-4 * max(1.0, loss)
    assert int(z[tag + "codes_used"]) > 16                                  # the codebook makes the argmin non-trivial


def test_sample_rejects_too_small_lookup_codebook():
    from maskbit_amd import ConvVQModel, sample
    from maskbit_amd.bert import Bert
    gen = Bert(img_size=256, hidden_dim=128, codebook_size=4096, codebook_splits=2, depth=1, heads=4, mlp_dim=256, dropout=0.1, nclass=10,
               input_stride=16)
    tok = ConvVQModel(vq_cfg(codebook_size=1024, token_size=64, hidden_channels=64, channel_mult=[1, 1, 2], num_resolutions=3,
                             num_res_blocks=1))
    with pytest.raises(ValueError, match="codebook"):
        sample(gen, tok, num_samples=2, labels=torch.tensor([1, 2]), mask_token=64, codebook_size=4096, codebook_splits=2, num_steps=2)
    from maskbit_amd.harness import generate_uint8
    with pytest.raises(ValueError, match="codebook"):
        next(generate_uint8(gen, tok, torch.tensor([1, 2]), 2))


def test_vq_codebook_helper_and_weights_without_lfq_buffers():
    sd = make_tokenizer_weights(TokCfg(token_size=256, hidden_channels=64, channel_mult=(1, 1, 2), num_resolutions=3, num_res_blocks=1),
                                seed=1, with_encoder=True, lfq_buffers=False)
    assert not any(k.startswith("quantize.") for k in sd)
    cb = make_vq_codebook(16, 4, 0, torch.zeros(4), torch.ones(4))
    assert cb.shape == (16, 4) and torch.equal(cb, make_vq_codebook(16, 4, 0, torch.zeros(4), torch.ones(4)))
