"""GPU checks of the Taming VQGAN tokenizer (maskbit_amd.OriginalVQModel, csrc/taming.hip): encode and decode against the reference's fixture
(tests/golden/tok_taming_full.npz, tools/make_golden_taming.py) with the bounds of test_hip_vq.py -- the arithmetic is the same fp16 storage
with fp32 accumulation --, the outputs of two AttnBlocks against the reference's hooked rows, bitwise consistency between the decode entries,
batch invariance, a 512 x 512 decode (N = 1024 in the attention) against the float64 restatement of tests/taming_reference.py, the evaluators
and the sampler's refusal.  The model is built once per module from the fixture's seeds."""
import pytest
import torch

import taming_reference as TR
from conftest import load_golden
from maskbit_amd.synth import make_taming_weights, make_vq_codebook

pytestmark = pytest.mark.gpu
DEV = "cuda"
CROPS = ((0, 0), (120, 120), (240, 240), (37, 201))
_CACHE = {}


def fixture():
    """-> (fixture dict, state dict with the codebook, HIP model, the two images)"""
    if not _CACHE:
        from maskbit_amd import OriginalVQModel
        z = load_golden("tok_taming_full.npz")
        seed = int(z["seed"])
        sd = make_taming_weights(seed, float(z["qk_gain"]))
        sd["quantize.embedding.weight"] = make_vq_codebook(1024, 256, seed + 2, torch.from_numpy(z["cb_mean"]), torch.from_numpy(z["cb_std"]))
        m = OriginalVQModel(None)
        m.load_state_dict(sd, strict=True)
        m = m.eval().requires_grad_(False).to(DEV)
        x = torch.rand(2, 3, 256, 256, generator=torch.Generator().manual_seed(seed + 1))
        _CACHE["f"] = (z, sd, m, x)
    return _CACHE["f"]


@pytest.fixture(autouse=True)
def no_saturation():
    yield
    if _CACHE:
        assert _CACHE["f"][2].saturation_count() == 0


def test_encode_vs_reference():
    z, sd, m, x = fixture()
    zq, idx, zraw, dist = m._encode(x.to(DEV), want_raw=True, want_dist=True)
    zref = torch.from_numpy(z["z"])
    lat_err = float((zraw.cpu() - zref).abs().mean() / zref.abs().mean())
    ref = torch.from_numpy(z["indices"]).flatten()
    ours = idx.cpu().flatten()
    # bound on the distance change the latent error can cause: 2 |dz| (|z| + |e|) per row, generous (as test_hip_vq.test_encode_vs_reference)
    dz = (zraw.cpu() - zref).permute(0, 2, 3, 1).reshape(-1, 256)
    zr = zref.permute(0, 2, 3, 1).reshape(-1, 256)
    cb = sd["quantize.embedding.weight"]
    bound = 4 * dz.norm(dim=1) * (zr.norm(dim=1) + cb.norm(dim=1).max())
    clear = torch.from_numpy(z["gap"]) > bound
    differ = float((ours != ref).float().mean())
    print(f"taming: latent error {lat_err:.4f} of mean |z|, indices differing {differ:.4f}, clear rows {float(clear.float().mean()):.3f}")
    assert lat_err < 0.03
    assert torch.equal(ours[clear], ref[clear])                         # every differing row is a near-tie
    assert differ <= 0.02
    sel = cb.to(DEV)[idx.flatten()].reshape(2, 16, 16, 256).permute(0, 3, 1, 2)
    assert torch.equal(zq, sel)
    # losses: the engine's row distances against an fp64 recompute on its own latent, and against the reference
    zr64 = zraw.double().permute(0, 2, 3, 1).reshape(-1, 256)
    cl64 = float((zq.double().permute(0, 2, 3, 1).reshape(-1, 256) - zr64).pow(2).mean())
    zq_, res = m.encode(x.to(DEV))
    assert torch.equal(zq_, zq) and torch.equal(res["min_encoding_indices"], idx) and res["min_encoding_indices"].shape == (2, 16, 16)
    cl = float(res["codebook_loss"])
    print(f"taming: codebook loss {cl:.6f}, fp64 recompute {cl64:.6f}, reference {float(z['codebook_loss']):.6f}")
    assert abs(cl - cl64) <= 1e-4 * max(1.0, cl64)
    assert abs(float(res["commitment_loss"]) - 0.25 * cl) <= 1e-6 * max(1.0, cl)
    assert abs(float(res["quantizer_loss"]) - 1.25 * cl) <= 1e-6 * max(1.0, cl)
    for k in ("codebook_loss", "commitment_loss", "quantizer_loss"):
        assert abs(float(res[k]) - float(z[k])) <= 0.1 * float(z[k])
    assert all(float(res[k]) == 0.0 for k in ("entropy_loss", "per_sample_entropy", "avg_entropy"))


def test_decode_vs_reference():
    z, sd, m, x = fixture()
    ref_idx = torch.from_numpy(z["indices"]).reshape(2, -1)
    img = m.decode_tokens(ref_idx.to(DEV))
    errs = [float((img.cpu()[:, :, y:y + 16, xx:xx + 16] - torch.from_numpy(z[f"crop_{y}_{xx}"])).abs().max()) for (y, xx) in CROPS]
    half = float((img.cpu()[:, :, ::2, ::2] - torch.from_numpy(z["recon_half"]).float()).abs().max())
    print(f"taming: decode_tokens(reference indices) max abs error vs the reference: crops {max(errs):.4f}, half-resolution {half:.4f}")
    assert max(errs) < 0.02 and half - 2e-3 < 0.02
    # consistency between the decode entries, bitwise
    zq, idx, _, _ = m._encode(x.to(DEV))
    assert torch.equal(m.decode(zq), m.decode_tokens(idx.reshape(2, -1)))
    lat = sd["quantize.embedding.weight"].to(DEV)[ref_idx.to(DEV)].reshape(2, 16, 16, 256).permute(0, 3, 1, 2).contiguous()
    assert torch.equal(m.decode(lat), img)
    img2, u8 = m.decode_tokens_uint8(ref_idx.to(DEV))
    assert torch.equal(img2, img) and u8.shape == (2, 256, 256, 3) and u8.dtype == torch.uint8
    assert torch.equal(u8, (img.clamp(0, 1) * 255.0).to(torch.uint8).permute(0, 2, 3, 1))       # the truncation of its own fp32 image
    for (y, xx) in CROPS:                                               # 0.02 * 255 = 5.1, + 1 for the truncation
        want = (torch.from_numpy(z[f"crop_{y}_{xx}"]).clamp(0, 1) * 255.0).to(torch.uint8).permute(0, 2, 3, 1).int()
        assert int((u8.cpu()[:, y:y + 16, xx:xx + 16].int() - want).abs().max()) <= 6
    rec, res = m(x.to(DEV))
    assert torch.equal(rec, m.decode_tokens(res["min_encoding_indices"].reshape(2, -1)))


def test_hooked_attention_rows():
    """The outputs of encoder.down.4.attn.0 and decoder.up.4.attn.2 (mb_taming_set_tap) against the rows the reference's forward hooks recorded:
    the same relative bound as the latent."""
    from maskbit_amd import _lib
    z, sd, m, x = fixture()
    rows = [int(r) for r in z["hook_rows"]]
    h = m.engine(2, 16)
    lib = _lib.load()
    buf = torch.zeros(2, 256, 512, dtype=torch.float16, device=DEV)
    for block, key, go in ((0, "attn_enc_first", lambda: m._encode(x.to(DEV))),
                           (6, "attn_dec_last", lambda: m.decode_tokens(torch.from_numpy(z["indices"]).reshape(2, -1).to(DEV)))):
        _lib.check(lib.mb_taming_set_tap(h, block, buf.data_ptr()), "mb_taming_set_tap")
        try:
            go()
            torch.cuda.synchronize()
        finally:
            _lib.check(lib.mb_taming_set_tap(h, block, None), "mb_taming_set_tap")
        ref = torch.from_numpy(z[key])
        ours = buf[:, rows].float().cpu()
        err = float((ours - ref).abs().mean() / ref.abs().mean())
        print(f"taming: {key}: mean abs error {err:.4f} of mean |ref| (max abs {float((ours - ref).abs().max()):.4f}, max |ref| {float(ref.abs().max()):.2f})")
        assert err < 0.03
    assert lib.mb_taming_set_tap(h, 7, None) == -1


def test_batch_invariance_and_determinism():
    z, sd, m, x = fixture()
    g = torch.Generator().manual_seed(8)
    xs = torch.rand(3, 3, 256, 256, generator=g).to(DEV)
    zq3, idx3, _, _ = m._encode(xs)
    zq1, idx1, _, _ = m._encode(xs[1:2].contiguous())
    assert torch.equal(idx3[1:2], idx1) and torch.equal(zq3[1:2], zq1)
    again = m._encode(xs)
    assert torch.equal(again[1], idx3) and torch.equal(again[0], zq3)
    codes = torch.randint(0, 1024, (3, 256), generator=g).to(DEV)
    i3 = m.decode_tokens(codes)
    assert torch.equal(m.decode_tokens(codes[1:2]), i3[1:2])
    assert torch.equal(m.decode_tokens(codes), i3)
    # device-resident codes are clamped in the kernel; host-resident ones raise
    assert torch.equal(m.decode_tokens(torch.full((1, 256), 10_000, device=DEV)), m.decode_tokens(torch.full((1, 256), 1023, device=DEV)))
    with pytest.raises(IndexError):
        m.decode_tokens(torch.full((1, 256), 1024))


def test_512_decode_vs_fp64_restatement():
    """One 512 x 512 image: latent side 32, N = 1024 keys in the four decoder AttnBlocks.  The float64 forward of a whole 512 x 512 image takes
    longer than a few seconds on the CPU, so (as for the other tokenizers' large shapes) the 256 x 256 encode is what test_encode_vs_reference
    compares, and here the 512 x 512 decode of given tokens is compared with the restatement on 16 x 16 crops; the 512 x 512 encode runs for
    its own consistency (N = 1024 in the three encoder AttnBlocks: deterministic, batch-invariant, no saturation, decodable)."""
    z, sd, m, x = fixture()
    g = torch.Generator().manual_seed(21)
    codes = torch.from_numpy(z["indices"]).reshape(-1)[torch.randint(0, 512, (1, 1024), generator=g)]       # codes the fixture's images use
    img = m.decode_tokens(codes.to(DEV))
    assert img.shape == (1, 3, 512, 512)
    with torch.no_grad():
        ref = TR.decode_tokens(sd, codes)
    errs = [float((img.cpu().double()[:, :, y:y + 16, xx:xx + 16] - ref[:, :, y:y + 16, xx:xx + 16]).abs().max())
            for (y, xx) in ((0, 0), (248, 248), (496, 496), (75, 403))]
    print(f"taming 512: decode_tokens max abs error vs the float64 restatement on 16 x 16 crops {max(errs):.4f}")
    assert max(errs) < 0.02
    xs = torch.rand(2, 3, 512, 512, generator=g).to(DEV)
    zq, idx, _, _ = m._encode(xs)
    assert idx.shape == (2, 32, 32) and int(idx.min()) >= 0 and int(idx.max()) < 1024 and bool(torch.isfinite(zq).all())
    zq1, idx1, _, _ = m._encode(xs[1:2].contiguous())
    assert torch.equal(idx[1:2], idx1) and torch.equal(zq[1:2], zq1)
    assert torch.equal(m.decode(zq1), m.decode_tokens(idx1.reshape(1, -1)))
    assert m.saturation_count() == 0
    m.engine(2, 16)                                                      # back to the 256 x 256 engine for the tests that follow


def test_evaluators_accept_the_model():
    from maskbit_amd import TokenizerEvaluator, eval_reconstruction
    z, sd, m, x = fixture()
    ev = TokenizerEvaluator(device=DEV, enable_psnr_score=True, enable_ssim_score=True, enable_mse_error=True, enable_codebook_usage_measure=True,
                            enable_codebook_entropy_measure=True, num_codebook_entries=1024)
    rec, res = m(x.to(DEV))
    ev.update(x.to(DEV).clamp(0, 1), rec.clamp(0, 1), res["min_encoding_indices"])
    r1 = ev.result()
    r2 = eval_reconstruction(m, [{"image": x[:1]}, {"image": x[1:]}], ev)
    for r in (r1, r2):
        vals = {k: float(v) for k, v in r.items()}
        print("taming evaluator:", vals)
        assert all(torch.isfinite(torch.tensor(v)) for v in vals.values())
        assert any("psnr" in k.lower() for k in vals) and any("ssim" in k.lower() for k in vals)


def test_sampler_refuses_the_taming_tokenizer():
    from maskbit_amd import LFQBert, sample
    z, sd, m, x = fixture()
    gen = LFQBert(img_size=256, hidden_dim=128, codebook_size=1024, codebook_splits=2, depth=1, heads=4, mlp_dim=256, dropout=0.0, nclass=10,
                  input_stride=16).to(DEV)
    with pytest.raises(TypeError, match="OriginalVQModel"):
        sample(gen, m, num_samples=1, labels=torch.tensor([1]), mask_token=32, codebook_size=1024, codebook_splits=2, num_steps=2)
