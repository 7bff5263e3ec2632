"""GPU checks of maskbit_amd.TokenizerEvaluator (csrc/evaluator.hip) against the reference's recorded results (tests/golden/evaluator.npz) and,
for shapes without a golden, against the float64 restatement of tests/test_evaluator_cpu.py.

Bounds (none of them comes from the code under test):
  MAE, MSE  relative 1e-10: fp32 differences are exact in fp64, and an fp64 sum of N <= 786 432 terms is off by at most N * 2^-53 ~ 9e-11.
  PSNR      1e-9 dB: 10 log10 moves by 4.34 dB per unit of relative error of the MSE.
  SSIM      per image |hip - ref64| <= 4 x E_ref, E_ref = the reference's own fp32 evaluation error on that case (max over its images of
            |ref32 - ref64|, recorded in the golden).  The kernel's separable filter replaces the reference's fp32-rounded 2-D weights
            outer(g, g) by g[i] * g[j]: a perturbation of 2^-24 per tap, of the same order as and independent of the reference's rounding,
            hence a small multiple of E_ref rather than 1 x.  For shapes without a golden, E_ref is computed here the same way: the
            reference's formulation in fp32 torch operations on the CPU against the float64 restatement.
  Codebook  usage and histogram exact (integer counts), entropy 1e-12 (fp64 sum of K terms of magnitude <= 0.53).
Measured SSIM ratios per golden case: profiles/tokenizer_evaluator.md.
"""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from hip_helpers import Cfg, hip_tokenizer
from oracle import maskbit_oracle as O
from maskbit_amd.synth import make_eval_images
from test_evaluator_cpu import KEYS, codebook_metrics64, evaluator_golden, image_case, index_case, per_image_metrics64

pytestmark = pytest.mark.gpu
DEV = "cuda"
REL_ERR, PSNR_DB, SSIM_MULT, ENTROPY_ABS = 1e-10, 1e-9, 4.0, 1e-12


def evaluator(**kw):
    from maskbit_amd import TokenizerEvaluator
    if not kw:
        kw = dict(enable_psnr_score=True, enable_ssim_score=True, enable_mse_error=True, enable_mae_error=True)
    return TokenizerEvaluator(DEV, **kw)


def ssim_reference_formulation(real, fake):
    """evaluator.py:296-334 restated with torch operations in the inputs' dtype and on their device (reflect pad, the five fields through one
    depthwise 11 x 11 convolution with the 2-D window, the SSIM formula) -> float64 [B] per-image means.  In fp32 on the CPU this is what
    the reference computes, so its distance to the float64 restatement is the reference's own error."""
    g = torch.from_numpy(evaluator_golden()["window_1d"]).to(fake.device)
    w = torch.outer(g, g).to(fake.dtype).expand(3, 1, 11, 11)
    x, y = F.pad(fake, [5, 5, 5, 5], mode="reflect"), F.pad(real, [5, 5, 5, 5], mode="reflect")
    mx, my, xx, yy, xy = F.conv2d(torch.cat([x, y, x * x, y * y, x * y]), w, groups=3).chunk(5)
    c1, c2 = 0.01 ** 2, 0.03 ** 2
    mxx, myy, mxy = mx * mx, my * my, mx * my
    idx = ((2 * mxy + c1) * (2 * (xy - mxy) + c2)) / ((mxx + myy + c1) * ((xx - mxx) + (yy - myy) + c2))
    return idx.mean((1, 2, 3), dtype=torch.float64)


def hip_per_image(ev, real, fake, **kw):
    """float64 [B, 4] MAE, MSE, PSNR, SSIM of every image through B = 1 updates (reset in between): what result() reports for one image."""
    rows = []
    for b in range(fake.shape[0]):
        ev.reset_metrics()
        ev.update(real[b:b + 1], fake[b:b + 1], **kw)
        r = ev.result()
        rows.append([r.get(k, float("nan")) for k in KEYS])
    return np.array(rows, dtype=np.float64)


def check_images(ours, ref, e_ref, what, ssim=True):
    ours, ref = np.atleast_2d(ours), np.atleast_2d(ref)
    ratio = np.abs(ours[:, 3] - ref[:, 3]).max() / e_ref if ssim else 0.0
    print(f"{what}: MAE rel {np.abs(ours[:, 0] / ref[:, 0] - 1).max():.2e} MSE rel {np.abs(ours[:, 1] / ref[:, 1] - 1).max():.2e} "
          f"PSNR {np.abs(ours[:, 2] - ref[:, 2]).max():.2e} dB SSIM {ratio:.3f} x E_ref ({e_ref:.3g})")
    assert np.all(np.abs(ours[:, 0] - ref[:, 0]) <= REL_ERR * ref[:, 0]), what
    assert np.all(np.abs(ours[:, 1] - ref[:, 1]) <= REL_ERR * ref[:, 1]), what
    assert np.all(np.abs(ours[:, 2] - ref[:, 2]) <= PSNR_DB), what
    if ssim:
        assert np.all(np.abs(ours[:, 3] - ref[:, 3]) <= SSIM_MULT * e_ref), (what, ratio)
    return ratio


# ---- goldens ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", [str(n) for n in evaluator_golden()["image_cases"]])
def test_image_metrics_vs_reference(name):
    z = evaluator_golden()
    real, fake = (t.to(DEV) for t in image_case(name))
    ev = evaluator()
    e_ref = float(z[name + ".E_ref"])
    check_images(hip_per_image(ev, real, fake), z[name + ".ref64_img"], e_ref, name + " per image")
    ev.reset_metrics()
    ev.update(real, fake)
    r = ev.result()
    assert tuple(r) == KEYS and all(type(v) is float for v in r.values())
    check_images([r[k] for k in KEYS], z[name + ".ref64"], e_ref, name + " whole case")
    # the per-image sums the update left behind are those values before the division
    n = float(fake[0].numel())
    per = ev.last_per_image.cpu().numpy() / n
    assert np.all(np.abs(per[:, 0] - z[name + ".ref64_img"][:, 0]) <= REL_ERR * per[:, 0])
    assert np.all(np.abs(per[:, 2] - z[name + ".ref64_img"][:, 3]) <= SSIM_MULT * e_ref)


@pytest.mark.parametrize("name", [str(n) for n in evaluator_golden()["index_cases"]])
def test_codebook_metrics_vs_reference(name):
    z = evaluator_golden()
    K, ups = index_case(name)
    ev = evaluator(enable_codebook_usage_measure=True, enable_codebook_entropy_measure=True, num_codebook_entries=K)
    dummy = torch.zeros(1, 3, 8, 8, device=DEV)
    for i, idx in enumerate(ups):
        ev.update(dummy, dummy, idx.to(DEV) if i % 2 == 0 else idx.to(DEV).int())      # int64 and int32 indices alike
    r = ev.result()
    assert tuple(r) == ("CodebookUsage", "CodebookEntropy")
    assert type(r["CodebookUsage"]) is float and r["CodebookUsage"] == float(z[name + ".usage"])
    ent = r["CodebookEntropy"]
    assert torch.is_tensor(ent) and ent.dim() == 0 and ent.dtype == torch.float64 and ent.device.type == "cuda"
    assert abs(float(ent) - float(z[name + ".entropy"])) <= ENTROPY_ABS
    assert torch.equal(ev._hist.cpu(), codebook_metrics64(K, ups)[2])
    assert ev._num_updates == len(ups) and ev._num_examples == len(ups)


def test_usage_alone_and_large_index_tensor():
    K = 4096
    idx = torch.randint(0, K, (3_000_001,), device=DEV, generator=torch.Generator(device=DEV).manual_seed(3))     # more than one grid pass
    ev = evaluator(enable_codebook_usage_measure=True, num_codebook_entries=K)
    ev.update(torch.zeros(2, 1, 6, 6, device=DEV), torch.zeros(2, 1, 6, 6, device=DEV), idx)
    assert torch.equal(ev._hist, torch.bincount(idx, minlength=K))
    assert ev.result() == {"CodebookUsage": 1.0}


# ---- bit-exact properties -------------------------------------------------------------------------------------------------------------
def state(ev):
    return ev._sums.clone(), ev._hist.clone(), ev._out_of_range.clone(), ev.last_per_image.clone()


def same(a, b):
    return all(torch.equal(x, y) for x, y in zip(a, b))


def test_same_update_twice_and_reset():
    real, fake = (t.to(DEV) for t in make_eval_images("sin", 0.05, 5, 70, 45, 7))
    idx = torch.randint(0, 1024, (5, 16, 16), device=DEV)
    kw = dict(enable_psnr_score=True, enable_ssim_score=True, enable_mse_error=True, enable_mae_error=True, enable_codebook_usage_measure=True,
              enable_codebook_entropy_measure=True)
    a, b = evaluator(**kw), evaluator(**kw)
    a.update(real, fake, idx)
    b.update(real, fake, idx)
    first = state(a)
    assert same(first, state(b))
    assert float(first[0].abs().min()) > 0 and int(first[1].sum()) == idx.numel()
    a.reset_metrics()
    assert a._num_examples == 0 and a._num_updates == 0 and a.last_per_image is None
    assert not bool(a._sums.any()) and not bool(a._hist.any()) and not bool(a._out_of_range.any())
    with pytest.raises(ValueError, match="No examples to evaluate."):
        a.result()
    a.update(real, fake, idx)
    assert same(first, state(a))


def test_per_image_values_do_not_depend_on_the_batch():
    g = torch.Generator(device=DEV).manual_seed(11)
    real = torch.rand(64, 3, 40, 72, device=DEV, generator=g)
    fake = real + 0.05 * torch.randn(64, 3, 40, 72, device=DEV, generator=g)
    ev = evaluator()
    ev.update(real, fake)
    batch = ev.last_per_image.clone()
    assert batch.shape == (64, 3) and bool((batch > 0).all())
    for b in (0, 1, 37, 63):
        ev.update(real[b:b + 1], fake[b:b + 1])
        assert torch.equal(ev.last_per_image[0], batch[b]), b


def test_split_batch_leaves_the_same_state():
    real, fake = (t.to(DEV) for t in make_eval_images("bright", 0.05, 8, 50, 33, 9))
    idx = torch.randint(0, 1024, (8, 64), device=DEV)
    kw = dict(enable_psnr_score=True, enable_ssim_score=True, enable_mse_error=True, enable_mae_error=True, enable_codebook_entropy_measure=True)
    whole, parts = evaluator(**kw), evaluator(**kw)
    whole.update(real, fake, idx)
    parts.update(real[:3], fake[:3], idx[:3])
    parts.update(real[3:], fake[3:], idx[3:])
    assert torch.equal(whole._sums, parts._sums) and torch.equal(whole._hist, parts._hist)
    assert torch.equal(whole.last_per_image[3:], parts.last_per_image)
    rw, rp = whole.result(), parts.result()
    assert parts._num_updates == 2 and parts._num_examples == 8
    assert all(rw[k] == rp[k] for k in KEYS) and torch.equal(rw["CodebookEntropy"], rp["CodebookEntropy"])


# ---- shapes without goldens -----------------------------------------------------------------------------------------------------------
def check_against_restatement(real, fake, what, clamp=False):
    """real / fake: CPU fp32 [B, 3, H, W]; the evaluator is fed their device copies per image and as a batch."""
    rc, fc = (real.clamp(0, 1), fake.clamp(0, 1)) if clamp else (real, fake)
    ref = per_image_metrics64(real, fake, clamp=clamp).numpy()
    e_ref = float((ssim_reference_formulation(rc, fc) - torch.from_numpy(ref[:, 3])).abs().max())
    ev = evaluator()
    check_images(hip_per_image(ev, real.to(DEV), fake.to(DEV), clamp=clamp), ref, e_ref, what + " per image")
    ev.reset_metrics()
    ev.update(real.to(DEV), fake.to(DEV), clamp=clamp)
    r = ev.result()
    check_images([r[k] for k in KEYS], ref.mean(0), e_ref, what + " batch")


@pytest.mark.parametrize("shape", [(16, 6, 6), (16, 11, 7), (4, 33, 65), (1, 512, 512)])
def test_odd_shapes_vs_restatement(shape):
    B, H, W = shape
    check_against_restatement(*make_eval_images("noise" if H > 100 else "bright", 0.05, B, H, W, 100 + H), f"{B}x3x{H}x{W}")


def test_clamp_on_inputs_outside_the_unit_range():
    g = torch.Generator().manual_seed(21)
    real = torch.randn(4, 3, 48, 40, generator=g) * 0.5 + 0.5
    fake = real + 0.1 * torch.randn(4, 3, 48, 40, generator=g)
    assert float(real.min()) < -0.2 and float(fake.max()) > 1.2
    check_against_restatement(real, fake, "clamp", clamp=True)
    # and without the flag nothing is clamped
    ev = evaluator(enable_mse_error=True)
    ev.update(real.to(DEV), fake.to(DEV))
    mse = per_image_metrics64(real, fake, ssim=False)[:, 1].mean().item()
    assert abs(ev.result()["MSE"] - mse) <= REL_ERR * mse


@pytest.mark.parametrize("C", [1, 4])
def test_other_channel_counts_without_ssim(C):
    real, fake = make_eval_images("noise", 0.05, 3, 19, 45, 30 + C, C=C)
    ev = evaluator(enable_psnr_score=True, enable_mse_error=True, enable_mae_error=True)
    ev.update(real.to(DEV), fake.to(DEV))
    r = ev.result()
    assert tuple(r) == ("MAE", "MSE", "PSNR")
    ref = per_image_metrics64(real, fake, ssim=False).numpy().mean(0)
    check_images([r["MAE"], r["MSE"], r["PSNR"], float("nan")], ref, 1.0, f"C={C}", ssim=False)
    with pytest.raises(ValueError, match="3 channels"):
        evaluator().update(real.to(DEV), fake.to(DEV))


def test_non_contiguous_and_fp16_inputs():
    real, fake = make_eval_images("sin", 0.05, 3, 40, 52, 41)
    ref = per_image_metrics64(real, fake).numpy()
    e_ref = float((ssim_reference_formulation(real, fake) - torch.from_numpy(ref[:, 3])).abs().max())
    big_r, big_f = torch.zeros(3, 3, 45, 60, device=DEV), torch.zeros(3, 3, 45, 60, device=DEV)
    big_r[:, :, 2:42, 3:55], big_f[:, :, 2:42, 3:55] = real.to(DEV), fake.to(DEV)
    views = big_r[:, :, 2:42, 3:55], big_f[:, :, 2:42, 3:55].to(memory_format=torch.channels_last)
    assert not views[0].is_contiguous() and not views[1].is_contiguous()
    ev = evaluator()
    ev.update(*views)
    r = ev.result()
    check_images([r[k] for k in KEYS], ref.mean(0), e_ref, "non-contiguous")
    # fp16 inputs are evaluated as the values they hold; real may come in any shape of the same size (view_as, evaluator.py:283)
    r16, f16 = real.half(), fake.half()
    ref = per_image_metrics64(r16.float(), f16.float()).numpy()
    e_ref = float((ssim_reference_formulation(r16.float(), f16.float()) - torch.from_numpy(ref[:, 3])).abs().max())
    ev.reset_metrics()
    ev.update(r16.to(DEV), f16.to(DEV))
    r = ev.result()
    check_images([r[k] for k in KEYS], ref.mean(0), e_ref, "fp16")
    ev2 = evaluator(enable_mae_error=True)
    ev2.update(real.to(DEV).reshape(9, 1, 40, 52), fake.to(DEV))
    mae = per_image_metrics64(real, fake, ssim=False)[:, 0].mean().item()
    assert abs(ev2.result()["MAE"] - mae) <= REL_ERR * mae


# ---- errors ---------------------------------------------------------------------------------------------------------------------------
def test_out_of_range_indices_raise_at_result():
    img = torch.zeros(1, 3, 8, 8, device=DEV)
    for bad in (1024, -1, 2 ** 40):
        ev = evaluator(enable_codebook_usage_measure=True, num_codebook_entries=1024)
        ev.update(img, img, torch.tensor([[0, 5, bad, 7]], device=DEV))          # update itself does not look at the values
        with pytest.raises(IndexError, match="outside"):
            ev.result()
        assert int(ev._hist.sum()) == 3                                          # the valid ones were counted, nothing was written elsewhere


def test_value_errors_before_any_device_work():
    ev = evaluator(enable_ssim_score=True, enable_mae_error=True, enable_codebook_usage_measure=True)
    ok = torch.zeros(2, 3, 8, 8, device=DEV)
    idx = torch.zeros(2, 4, dtype=torch.int64, device=DEV)
    with pytest.raises(ValueError, match="No examples"):
        ev.result()
    for real, fake, ind in ((ok[0], ok[0], idx),                                              # not 4-D
                            (ok, torch.zeros(2, 3, 8, 9, device=DEV), idx),                  # element counts differ
                            (torch.zeros(2, 3, 5, 8, device=DEV), torch.zeros(2, 3, 5, 8, device=DEV), idx),      # H < 6
                            (torch.zeros(2, 3, 8, 4, device=DEV), torch.zeros(2, 3, 8, 4, device=DEV), idx),      # W < 6
                            (torch.zeros(2, 1, 8, 8, device=DEV), torch.zeros(2, 1, 8, 8, device=DEV), idx),      # SSIM with C != 3
                            (ok, ok, None),                                                    # codebook metric without indices
                            (ok, ok, idx.float())):
        with pytest.raises(ValueError):
            ev.update(real, fake, ind)
    assert ev._num_examples == 0 and ev._num_updates == 0 and not bool(ev._sums.any()) and not bool(ev._hist.any())
    ev.update(ok, ok, idx)
    r = ev.result()
    assert r["MAE"] == 0.0 and r["SSIM"] == 1.0 and r["CodebookUsage"] == 1.0 / 1024


# ---- end to end -----------------------------------------------------------------------------------------------------------------------
def tiny_tokenizers():
    tc = O.TokCfg(token_size=12, hidden_channels=64, channel_mult=(1, 1, 2), num_resolutions=3, num_res_blocks=1)
    yield "lfq", hip_tokenizer(tc, O.make_tokenizer_weights(tc, seed=21, with_encoder=True), DEV), 4096
    from maskbit_amd import ConvVQModel
    from conftest import load_golden
    tc = O.TokCfg(token_size=64, hidden_channels=64, channel_mult=(1, 1, 2), num_resolutions=3, num_res_blocks=1)
    z = load_golden("tok_vq_tiny.npz")
    sd = O.make_tokenizer_weights(tc, seed=int(z["seed"]), with_encoder=True, lfq_buffers=False)
    sd["quantize.embedding.weight"] = torch.from_numpy(z["codebook"])
    m = ConvVQModel(Cfg(quantizer_type="lookup", codebook_size=512, token_size=64, commitment_cost=0.25, entropy_loss_weight=0.0,
                        entropy_loss_temperature=0.01, entropy_gamma=1.0, num_channels=3, hidden_channels=64, channel_mult=[1, 1, 2],
                        num_resolutions=3, num_res_blocks=1, sample_with_conv=tc.sample_with_conv, use_l2_normalisation=False))
    m.load_state_dict(sd, strict=True)
    yield "vq", m.eval().requires_grad_(False).to(DEV), 512


class Recording:
    """A tokenizer that keeps what it was given and what it returned."""

    def __init__(self, model):
        self.model, self.seen = model, []

    def eval(self):
        self.model.eval()
        return self

    def _require_cuda(self, what):
        return self.model._require_cuda(what)

    def __call__(self, images):
        rec, d = self.model(images)
        self.seen.append((images.cpu(), rec.cpu(), d["min_encoding_indices"].cpu()))
        return rec, d


def test_eval_reconstruction_end_to_end():
    from maskbit_amd import eval_reconstruction
    g = torch.Generator().manual_seed(77)
    loader = [{"image": torch.rand(2, 3, 64, 64, generator=g) * 1.2 - 0.1, "__key__": ["a", "b"]} for _ in range(2)]
    for name, model, K in tiny_tokenizers():
        ev = evaluator(enable_psnr_score=True, enable_ssim_score=True, enable_mse_error=True, enable_mae_error=True,
                       enable_codebook_usage_measure=True, enable_codebook_entropy_measure=True, num_codebook_entries=K)
        ev.update(torch.ones(1, 3, 8, 8, device=DEV), torch.zeros(1, 3, 8, 8, device=DEV), torch.zeros(1, dtype=torch.int64, device=DEV))
        model = Recording(model)
        r = eval_reconstruction(model, loader, ev)                                # resets what was there before
        assert tuple(r) == KEYS + ("CodebookUsage", "CodebookEntropy") and ev._num_examples == 4 and ev._num_updates == 2
        real, fake = torch.cat([s[0] for s in model.seen]), torch.cat([s[1] for s in model.seen])
        idxs = [s[2] for s in model.seen]
        assert torch.equal(real, torch.cat([b["image"] for b in loader])) and fake.shape == real.shape
        assert float(fake.min()) < 0.0 or float(fake.max()) > 1.0 or float(real.min()) < 0.0                  # the clamp matters
        ref = per_image_metrics64(real, fake, clamp=True).numpy()
        e_ref = float((ssim_reference_formulation(real.clamp(0, 1), fake.clamp(0, 1)) - torch.from_numpy(ref[:, 3])).abs().max())
        check_images([r[k] for k in KEYS], ref.mean(0), e_ref, "eval_reconstruction " + name)
        usage, entropy, _ = codebook_metrics64(K, idxs)
        assert r["CodebookUsage"] == usage and abs(float(r["CodebookEntropy"]) - entropy) <= ENTROPY_ABS
