"""GPU checks of the lookup (VQ) tokenizer: the fused nearest-codeword search (mb_vq_argmin) against an fp64 argmin, encode / decode of
ConvVQModel(quantizer_type="lookup") against the reference's fixtures (tests/golden/tok_vq_*.npz, tools/make_golden_vq.py), the legacy
layout, determinism, and sample() / generate_uint8() with the embedding-table Bert generator on a lookup tokenizer."""
import pytest
import torch

import quantizer_reference as QR
from conftest import load_golden
from hip_helpers import Cfg
from oracle import maskbit_oracle as O
from maskbit_amd.synth import make_vq_codebook

pytestmark = pytest.mark.gpu
DEV = "cuda"


def vq_argmin(z, cb, l2, splits=0):
    from maskbit_amd import _lib
    N, K = z.shape
    idx = torch.empty(N, dtype=torch.int64, device=DEV)
    dist = torch.empty(N, dtype=torch.float32, device=DEV)
    _lib.check(_lib.load().mb_vq_argmin(z.data_ptr(), cb.data_ptr(), N, cb.shape[0], K, int(l2), splits, idx.data_ptr(), dist.data_ptr(),
                                        torch.cuda.current_stream().cuda_stream), "mb_vq_argmin")
    return idx, dist


def fp64_dist(z, cb, l2):
    zd, e = z.double(), cb.double()
    if l2:
        zd, e = torch.nn.functional.normalize(zd, dim=-1), torch.nn.functional.normalize(e, dim=-1)
    return torch.cdist(zd, e).pow(2), zd, e


@pytest.mark.parametrize("CK", [(4096, 64), (1024, 256), (1000, 48), *QR.ARGMIN_L2_ADDED])
@pytest.mark.parametrize("l2", [False, True])
def test_argmin_exact_vs_fp64(CK, l2):
    Cn, K = CK
    g = torch.Generator(device=DEV).manual_seed(Cn + K + int(l2))
    if CK in QR.ARGMIN_L2_ADDED:      # 64 < K <= 128, the Kp = 128 search; CPU-seeded: tests/test_quantizer_cpu.py computes the clear-row share of these
        cb, rows = QR.argmin_inputs(Cn, K, l2)
        cb = cb.to(DEV)
    else:
        cb, rows = torch.randn(Cn, K, device=DEV, generator=g), None
    for N in (1, 255, 16401):
        z = rows[N].to(DEV) if rows else torch.randn(N, K, device=DEV, generator=g) * 1.1 + 0.05
        idx, dist = vq_argmin(z, cb, l2)
        d, zd, e = fp64_dist(z, cb, l2)
        top2 = d.topk(2, dim=1, largest=False)
        gap = top2.values[:, 1] - top2.values[:, 0]
        scale = zd.pow(2).sum(1) + e.pow(2).sum(1).max()
        clear = gap > 1e-5 * scale
        assert bool(clear.float().mean() > 0.9)
        assert torch.equal(idx[clear], top2.indices[clear, 0])
        # the reported distance is the chosen entry's fp32 squared distance
        dsel = d.gather(1, idx[:, None])[:, 0]
        assert float(((dist.double() - dsel).abs() / (dsel + 1e-6)).max()) < 1e-4
        if N == 16401:
            for sp in (1, 64):
                i2, d2 = vq_argmin(z, cb, l2, splits=sp)
                assert torch.equal(i2, idx) and torch.equal(d2, dist)
            # batch composition: a subset of the rows gets the same answers
            i3, d3 = vq_argmin(z[100:357].contiguous(), cb, l2)
            assert torch.equal(i3, idx[100:357]) and torch.equal(d3, dist[100:357])


def test_argmin_ties_pick_lowest_index():
    g = torch.Generator(device=DEV).manual_seed(5)
    base = torch.randn(300, 64, device=DEV, generator=g)
    cb = torch.cat([base, base, base[:100]])                     # entries j, j + 300 (and j + 600) identical
    z = base[torch.arange(0, 300, 3, device=DEV)] + 0.01 * torch.randn(100, 64, device=DEV, generator=g)
    for sp in (1, 0, 64):
        idx, dist = vq_argmin(z.contiguous(), cb.contiguous(), False, sp)
        assert bool((idx < 300).all())
        assert torch.equal(idx, torch.arange(0, 300, 3, device=DEV))


# ------------------------------------------------------------------ tokenizer fixtures
def vq_cfg(tc: O.TokCfg, C, l2=False):
    return Cfg(quantizer_type="lookup", codebook_size=C, token_size=tc.token_size, commitment_cost=0.25, entropy_loss_weight=0.0,
               entropy_loss_temperature=0.01, entropy_gamma=1.0, num_channels=3, hidden_channels=tc.hidden_channels,
               channel_mult=list(tc.channel_mult), num_resolutions=tc.num_resolutions, num_res_blocks=tc.num_res_blocks,
               sample_with_conv=tc.sample_with_conv, use_l2_normalisation=l2)


FIXTURES = {
    "tiny": ("tok_vq_tiny.npz", "", O.TokCfg(token_size=64, hidden_channels=64, channel_mult=(1, 1, 2), num_resolutions=3, num_res_blocks=1), 512),
    "tiny_l2": ("tok_vq_tiny.npz", "l2_", O.TokCfg(token_size=64, hidden_channels=64, channel_mult=(1, 1, 2), num_resolutions=3, num_res_blocks=1), 512),
    "legacy256": ("tok_vq_legacy256_tiny.npz", "", O.TokCfg(token_size=256, hidden_channels=64, channel_mult=(1, 1, 2), num_resolutions=3,
                                                             num_res_blocks=1, sample_with_conv=False), 128),
    "full12": ("tok_vq_full12.npz", "", O.TokCfg(token_size=64), 4096),
    "full10": ("tok_vq_full10.npz", "", O.TokCfg(token_size=256), 1024),
}
_CACHE = {}


def fixture(name):
    """-> (fixture dict, tag, TokCfg, oracle state dict (canonical names, with codebook), HIP model, input image)"""
    if name in _CACHE:
        return _CACHE[name]
    from maskbit_amd import ConvVQModel
    from maskbit_amd.conv_vqgan import legacy_to_canonical
    fname, tag, tc, Cn = FIXTURES[name]
    z = load_golden(fname)
    sd = O.make_tokenizer_weights(tc, seed=int(z["seed"]), with_encoder=True, lfq_buffers=False)
    if "codebook" in z:
        cb = torch.from_numpy(z["codebook"])
        x = torch.from_numpy(z["image"])
    else:
        cb = make_vq_codebook(Cn, tc.token_size, int(z["seed"]) + 2, torch.from_numpy(z["cb_mean"]), torch.from_numpy(z["cb_std"]))
        x = torch.rand(1, 3, 256, 256, generator=torch.Generator().manual_seed(int(z["seed"]) + 1))
    sd["quantize.embedding.weight"] = cb
    legacy = name == "legacy256"
    m = ConvVQModel(vq_cfg(tc, Cn, bool(tag)), legacy=legacy)
    m.load_state_dict(legacy_to_canonical(sd, tc.num_resolutions) if legacy else sd, strict=True)
    m = m.eval().requires_grad_(False).to(DEV)
    _CACHE[name] = (z, tag, tc, sd, m, x)
    return _CACHE[name]


def prepared_codebook(cb, l2):
    return torch.nn.functional.normalize(cb, dim=-1) if l2 else cb


@pytest.mark.parametrize("name", list(FIXTURES))
def test_encode_vs_reference(name):
    z, tag, tc, sd, m, x = fixture(name)
    zq, idx, zraw, dist = m._encode(x.to(DEV), want_raw=True, want_dist=True)
    zref = torch.from_numpy(z[tag + "z"])
    lat_err = float((zraw.cpu() - zref).abs().mean() / zref.abs().mean())
    ref = torch.from_numpy(z[tag + "indices"]).flatten()
    ours = idx.cpu().flatten()
    # bound on the distance change the latent error can cause: 2 |dz| (|z| + |e|) per row, generous
    dz = (zraw.cpu() - zref).permute(0, 2, 3, 1).reshape(-1, tc.token_size)
    zr = zref.permute(0, 2, 3, 1).reshape(-1, tc.token_size)
    cb = sd["quantize.embedding.weight"]
    bound = 4 * dz.norm(dim=1) * (zr.norm(dim=1) + cb.norm(dim=1).max())
    if tag:
        bound = bound / zr.norm(dim=1).clamp_min(1e-12) + 1e-4
    clear = torch.from_numpy(z[tag + "gap"]) > bound
    differ = float((ours != ref).float().mean())
    print(f"{name}: latent error {lat_err:.4f} of mean |z|, indices differing {differ:.4f}, clear rows {float(clear.float().mean()):.3f}")
    assert lat_err < 0.03
    assert torch.equal(ours[clear], ref[clear])
    assert differ <= 0.02
    pc = prepared_codebook(cb, bool(tag)).to(DEV)
    sel = pc[idx.flatten()].reshape(x.shape[0], *idx.shape[1:], tc.token_size).permute(0, 3, 1, 2)
    if tag:
        assert float((zq - sel).abs().max()) < 1e-6
    else:
        assert torch.equal(zq, sel)
    # losses: the engine's row distances against an fp64 recompute on its own latent, and against the reference
    zr64 = zraw.double().permute(0, 2, 3, 1).reshape(-1, tc.token_size)
    if tag:
        zr64 = torch.nn.functional.normalize(zr64, dim=-1)
    cl64 = float((zq.double().permute(0, 2, 3, 1).reshape(-1, tc.token_size) - zr64).pow(2).mean())
    zq_, res = m.encode(x.to(DEV))
    assert torch.equal(zq_, zq) and torch.equal(res["min_encoding_indices"], idx)
    cl = float(res["codebook_loss"])
    assert abs(cl - cl64) <= 1e-4 * max(1.0, cl64)
    assert abs(float(res["commitment_loss"]) - 0.25 * cl) <= 1e-6 * max(1.0, cl)
    assert abs(float(res["quantizer_loss"]) - 1.25 * cl) <= 1e-6 * max(1.0, cl)
    assert abs(cl - float(z[tag + "codebook_loss"])) <= 0.1 * float(z[tag + "codebook_loss"])
    assert all(float(res[k]) == 0.0 for k in ("entropy_loss", "per_sample_entropy", "avg_entropy"))
    assert float(dist.sum()) > 0
    assert m.saturation_count() == 0


@pytest.mark.parametrize("name", list(FIXTURES))
def test_decode_vs_reference(name):
    z, tag, tc, sd, m, x = fixture(name)
    ref_idx = torch.from_numpy(z[tag + "indices"]).reshape(x.shape[0], -1)
    img = m.decode_tokens(ref_idx.to(DEV))
    if tag + "recon" in z:
        ref = torch.from_numpy(z[tag + "recon"])
        err = float((img.cpu() - ref).abs().max())
    else:
        errs = [float((img.cpu()[:, :, y:y + 16, xx:xx + 16] - torch.from_numpy(z[f"crop_{y}_{xx}"])).abs().max())
                for (y, xx) in ((0, 0), (120, 120), (240, 240), (37, 201))]
        errs.append(float((img.cpu()[:, :, ::2, ::2] - torch.from_numpy(z["recon_half"]).float()).abs().max()) - 2e-3)
        err = max(errs)
    print(f"{name}: decode_tokens(reference indices) max abs error vs the reference reconstruction {err:.4f}")
    assert err < 0.02
    # decode of the codebook rows == decode_tokens of the indices, bitwise: the rows as encode() returns them (the engine's prepared codebook;
    # with L2 normalisation its rows may differ from F.normalize's in the last bit), and without normalisation the checkpoint's rows themselves
    zq, idx, _ = m._encode(x.to(DEV))
    assert torch.equal(m.decode(zq), m.decode_tokens(idx.reshape(x.shape[0], -1)))
    if not tag:
        side = int(round(ref_idx.shape[1] ** 0.5))
        lat = sd["quantize.embedding.weight"].to(DEV)[ref_idx.to(DEV)].reshape(x.shape[0], side, side, -1).permute(0, 3, 1, 2).contiguous()
        assert torch.equal(m.decode(lat), img)
    img2, u8 = m.decode_tokens_uint8(ref_idx.to(DEV))
    assert torch.equal(img2, img) and u8.shape == (x.shape[0], img.shape[2], img.shape[3], 3)
    assert m.saturation_count() == 0


def test_decode_float_latent_and_range_policy():
    z, tag, tc, sd, m, x = fixture("tiny")
    lat = torch.randn(2, 64, 16, 16, generator=torch.Generator().manual_seed(3)) * 0.7
    img = m.decode(lat.to(DEV))
    ref = O.decode_latents(sd, tc, lat)
    err = float((img.cpu() - ref).abs().max())
    print(f"decode(float latent) max abs error vs oracle.decode_latents {err:.4f}")
    assert err < 0.02
    with pytest.raises(IndexError):
        m.decode_tokens(torch.full((1, 256), 512))
    with pytest.raises(IndexError):
        m.decode_tokens(torch.full((1, 256), -1))
    # device-resident codes are clamped in the kernel
    hi = m.decode_tokens(torch.full((1, 256), 10_000, device=DEV))
    assert torch.equal(hi, m.decode_tokens(torch.full((1, 256), 511, device=DEV)))


def test_legacy_equals_remapped_canonical():
    from maskbit_amd import ConvVQModel
    z, tag, tc, sd, leg, x = fixture("legacy256")
    can = ConvVQModel(vq_cfg(tc, 128)).to(DEV)
    can.load_state_dict(sd, strict=True)
    can.eval()
    idx = torch.from_numpy(z["indices"]).reshape(1, -1).to(DEV)
    assert torch.equal(leg.decode_tokens(idx), can.decode_tokens(idx))
    a, ra = leg(x.to(DEV))
    b, rb = can(x.to(DEV))
    assert torch.equal(a, b) and torch.equal(ra["min_encoding_indices"], rb["min_encoding_indices"])


def test_batch_invariance_and_determinism():
    z, tag, tc, sd, m, x = fixture("tiny")
    g = torch.Generator().manual_seed(8)
    xs = torch.rand(3, 3, 64, 64, generator=g).to(DEV)
    zq3, idx3, _ = m._encode(xs)
    zq1, idx1, _ = m._encode(xs[1:2].contiguous())
    assert torch.equal(idx3[1:2], idx1) and torch.equal(zq3[1:2], zq1)
    again = m._encode(xs)
    assert torch.equal(again[1], idx3) and torch.equal(again[0], zq3)
    codes = torch.randint(0, 512, (3, 256), generator=g).to(DEV)
    i3 = m.decode_tokens(codes)
    assert torch.equal(m.decode_tokens(codes[2:3]), i3[2:3])
    assert torch.equal(m.decode_tokens(codes), i3)
    rec, res = m(xs)
    assert torch.equal(rec, m.decode_tokens(res["min_encoding_indices"].reshape(3, -1)))
    assert m.saturation_count() == 0


def test_sample_bert_with_lookup_tokenizer():
    from maskbit_amd import ConvVQModel, sample
    from maskbit_amd.bert import Bert
    from maskbit_amd.harness import generate_uint8
    from oracle.make_golden_variants import VARIANTS
    gcfg, gseed = VARIANTS["bert_postnorm"]
    assert 2 ** gcfg.bits == 4096
    gsd = O.make_generator_weights(gcfg, seed=gseed, head_gain=20.0)
    gen = Bert(img_size=256, hidden_dim=gcfg.hidden, codebook_size=4096, codebook_splits=gcfg.splits, depth=gcfg.depth, heads=gcfg.heads,
               mlp_dim=gcfg.mlp, dropout=0.1, nclass=gcfg.nclass, input_stride=16)
    gen.load_state_dict(gsd, strict=True)
    gen = gen.eval().requires_grad_(False).to(DEV)
    tc = O.TokCfg(token_size=64, hidden_channels=64, channel_mult=(1, 1, 2), num_resolutions=3, num_res_blocks=1)
    tsd = O.make_tokenizer_weights(tc, seed=51, with_encoder=True, lfq_buffers=False)
    tsd["quantize.embedding.weight"] = make_vq_codebook(4096, 64, 52, torch.zeros(64), torch.ones(64) * 0.5)
    tok = ConvVQModel(vq_cfg(tc, 4096))
    tok.load_state_dict(tsd, strict=True)
    tok = tok.eval().requires_grad_(False).to(DEV)
    torch.manual_seed(0)
    labels = torch.tensor([1, 5])
    img, steps = sample(gen, tok, num_samples=2, labels=labels, mask_token=64, codebook_size=4096, codebook_splits=2, num_steps=4,
                        guidance_scale=2.0, guidance_annealing="cosine", mask_schedule_strategy="arccos")
    torch.cuda.synchronize()
    codes = O.combine_groups(steps[-1].cpu(), gcfg.bits, gcfg.splits).long()
    assert img.shape == (2, 3, 64, 64) and len(steps) == 4
    assert int(codes.max()) < 4096
    assert torch.equal(img, tok.decode_tokens(codes.to(DEV)))
    ref = O.decode_latents(tsd, tc, tsd["quantize.embedding.weight"][codes].reshape(2, 16, 16, 64).permute(0, 3, 1, 2))
    err = float((img.cpu() - ref).abs().max())
    print(f"sample(Bert, lookup tokenizer): image vs oracle decode of the codebook rows, max abs error {err:.4f}")
    assert err < 0.02
    out = list(generate_uint8(gen, tok, torch.tensor([2, 3, 4, 6]), 2, num_steps=4, return_codes=True))
    assert len(out) == 2
    u8, c = out[0]
    assert u8.shape == (2, 64, 64, 3) and c.shape == (2, 256) and int(c.max()) < 4096
    assert tok.saturation_count() == 0
