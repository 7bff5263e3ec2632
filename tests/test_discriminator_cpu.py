"""CPU-only tests of the VQGAN+ discriminator's Python surface and of the float64 restatement the GPU tests compare against: the restatement
against the reference's own logits (tests/golden/discriminator.npz, written by tools/make_golden_discriminator.py), the loss functions against the
values the reference's gan_utils gave, the module's key list, VQGANLoss's two dicts against the formulas, the adaptive-pool windows and the blur's
padding rule against torch, and the refusals.  Not held against the reference's VQGANLoss class (its constructor needs torchvision) or a trained
checkpoint."""
import ctypes as C
import functools

import pytest
import torch
import torch.nn.functional as F

import discriminator_reference as R
from conftest import load_golden
from maskbit_amd import discriminator as D
from maskbit_amd.synth import make_discriminator_weights

CASES = ("blur4_128", "blur4_32x48", "blur4_192x128", "avg_64", "blur3_64", "blur5_64")


@functools.lru_cache(maxsize=None)
def golden():
    return load_golden("discriminator.npz")


def case_images(name):
    z = golden()
    return torch.rand(*[int(v) for v in z[name + ".shape"]], generator=torch.Generator().manual_seed(int(z[name + ".image_seed"])))


def case_weights(name):
    z = golden()
    return make_discriminator_weights(int(z["seed"]), int(z["hidden"]), int(z["stages"]), int(z[name + ".blur"]))


class Cfg(dict):
    __getattr__ = dict.__getitem__


def loss_config(**kw):
    c = Cfg(discriminator_loss="hinge", reconstruction_loss="l2", discriminator_gradient_penalty="none", quantizer_weight=0.7, perceptual_loss="resnet50",
            perceptual_weight=0.1, lecam_regularization_weight=0.001, discriminator_start=20, discriminator_factor=1.0, discriminator_weight=0.1,
            discriminator_penalty_cost=10.0)
    c.update(kw)
    return c


DISC_CFG = Cfg(name="VQGAN+Discriminator", num_channels=3, num_stages=3, hidden_channels=32, blur_resample=True, blur_kernel_size=4)


# ------------------------------------------------------------------------------------------------ the restatement against the reference
@pytest.mark.parametrize("name", CASES)
def test_restatement_against_the_reference_logits(name):
    z = golden()
    got = R.forward64(case_weights(name), case_images(name), int(z[name + ".blur"]))
    e32 = float((got - torch.from_numpy(z[name + ".logits"]).double()).abs().max())
    e64 = float((got - torch.from_numpy(z[name + ".logits64"])).abs().max())
    print(f"{name}: max |restatement - reference| fp32 {e32:.2e}, float64 {e64:.2e}; max |logit| {float(got.abs().max()):.2f}")
    assert tuple(got.shape) == tuple(z[name + ".logits"].shape)
    assert e32 <= 1e-5 and e64 <= 1e-10


def test_emulation_differs_by_a_small_positive_error():
    z = golden()
    sd, x = case_weights("blur4_32x48"), case_images("blur4_32x48")
    e = float((R.forward64(sd, x, 4, emulate=True) - R.forward64(sd, x, 4)).abs().max())
    assert 0 < e < 0.05, e
    assert float(torch.from_numpy(z["blur4_128.logits"]).abs().max()) > 1.0 and float(torch.from_numpy(z["blur4_128.logits"]).min()) < -1.0


def test_recorded_hidden128_logits_are_the_current_restatements():
    """tests/golden/discriminator_h128.npz holds this restatement's own results for the GPU test's full-width cases; its small case is recomputed
    here, so an edit of discriminator_reference.py that the file does not follow fails (then: tools/make_golden_discriminator.py h128)"""
    z = load_golden("discriminator_h128.npz")
    sd = make_discriminator_weights(int(z["seed"]), 128, 3, 4)
    x = torch.rand(*[int(v) for v in z["h128_64.shape"]], generator=torch.Generator().manual_seed(int(z["h128_64.image_seed"])))
    with torch.no_grad():
        ref, emu = R.forward64(sd, x, 4), R.forward64(sd, x, 4, emulate=True)
    assert float((ref - torch.from_numpy(z["h128_64.ref64"])).abs().max()) <= 1e-12
    assert float((emu - torch.from_numpy(z["h128_64.emu64"])).abs().max()) <= 1e-12
    for name in ("h128_256", "h128_512x256"):
        E = float((torch.from_numpy(z[name + ".emu64"]) - torch.from_numpy(z[name + ".ref64"])).abs().max())
        assert tuple(z[name + ".ref64"].shape) == (1, 1, 16, 16) and 1e-4 < E < 1e-2, (name, E)


def test_losses_against_the_recorded_values():
    z = golden()
    both = torch.from_numpy(z["blur4_128.logits"])
    real, fake = D.stats_from_logits(both[0:1]), D.stats_from_logits(both[1:2])
    got = dict(hinge_d=D.hinge_d_loss(real, fake), vanilla_d=D.vanilla_d_loss(real, fake), non_saturating_d=D.non_saturating_d_loss(real, fake),
               hinge_g=D.hinge_g_loss(fake), non_saturating_g=D.non_saturating_g_loss(fake))
    by_hand = R.losses64(both[0:1], both[1:2])
    for k, v in got.items():
        assert v.dtype == torch.float64
        assert abs(float(v) - float(z["loss." + k])) <= 2e-6 * max(1.0, abs(float(v))), k     # the reference's value is an fp32 mean
        assert abs(float(v) - by_hand[k]) <= 1e-13, k
    ema_r, ema_f = (torch.tensor([v]) for v in z["ema"])
    lecam = D.compute_lecam_loss(D.logits_mean(real), D.logits_mean(fake), ema_r, ema_f)
    assert abs(float(lecam) - float(z["loss.lecam"])) <= 1e-6
    assert abs(float(lecam) - R.lecam64(float(both[0].double().mean()), float(both[1].double().mean()), *[float(v) for v in z["ema"]])) <= 1e-7
    assert torch.equal(D.stats_from_logits(both), R.stats64(both))
    assert D.adopt_weight(0.5, 9, threshold=10) == 0.0 and D.adopt_weight(0.5, 10, threshold=10) == 0.5 and D.adopt_weight(0.5, 0, 5, 2.0) == 2.0


def test_softplus_sums_do_not_overflow():
    l = torch.tensor([[-1000.0, 1000.0, 0.0, 1.0] * 64])
    s = D.stats_from_logits(l)
    assert torch.isfinite(s).all() and abs(float(s[0, 3]) - 64 * (1000.0 + 0.6931471805599453 + 0.3132616875182228)) < 1e-9


def test_module_keys_are_the_reference_modules():
    z = golden()
    blur = D.NLayerDiscriminatorv2(hidden_channels=32, blur_resample=True, blur_kernel_size=4)
    avg = D.NLayerDiscriminatorv2(hidden_channels=32, blur_resample=False)
    assert sorted(blur.state_dict().keys()) == list(z["keys.blur"]) and sorted(avg.state_dict().keys()) == list(z["keys.avg"])
    assert list(blur.state_dict().keys()) == D.discriminator_keys(3, True) and list(avg.state_dict().keys()) == D.discriminator_keys(3, False)
    blur.load_state_dict(case_weights("blur4_128"), strict=True)                  # the seeded weights carry the reference's keys and shapes
    avg.load_state_dict(case_weights("avg_64"), strict=True)
    assert tuple(blur.state_dict()["blocks.1.1.kernel"].shape) == (1, 1, 4, 4) and blur._engine is None
    assert torch.equal(blur.state_dict()["blocks.0.1.kernel"], D.blur_kernel(4)) and float(D.blur_kernel(5).sum()) == 1.0
    sd = case_weights("blur4_128")
    assert not torch.equal(sd["blocks.0.2.weight"], torch.ones(32)) and float(sd["blocks.0.2.bias"].abs().min()) > 0 and float(sd["to_logits.0.bias"].abs().max()) > 0
    import maskbit_amd
    import modeling.modules as MM
    assert MM.NLayerDiscriminatorv2 is D.NLayerDiscriminatorv2 is maskbit_amd.NLayerDiscriminatorv2 and MM.VQGANLoss is maskbit_amd.VQGANLoss
    assert isinstance(D.create_discriminator(DISC_CFG), D.NLayerDiscriminatorv2)


# ------------------------------------------------------------------------------------------------ VQGANLoss against the formulas
class StubDisc(torch.nn.Module):
    """logits are a fixed function of the images: their mean over channels at 16 x 16, times 4 minus 2"""
    @staticmethod
    def logits(x):
        return F.adaptive_avg_pool2d(x.double().mean(1, keepdim=True), 16) * 4 - 2

    def logit_stats(self, x, clamp=False, running_sum=None):
        return R.stats64(self.logits(x))


class StubPerceptual(torch.nn.Module):
    def forward(self, a, b):
        return (a - b).abs().mean() * 3.0


def stubbed(**kw):
    loss = D.VQGANLoss(DISC_CFG, loss_config(**kw))
    loss.discriminator, loss.perceptual_loss = StubDisc(), StubPerceptual()
    return loss


def pair(seed=3):
    g = torch.Generator().manual_seed(seed)
    x = torch.rand(2, 3, 32, 32, generator=g)
    return x, (x + 0.2 * torch.randn(2, 3, 32, 32, generator=g)).clamp(0, 1)


EXTRA = dict(quantizer_loss=torch.tensor(0.25), commitment_loss=torch.tensor(0.05), entropy_loss=torch.tensor(0.4), per_sample_entropy=torch.tensor(0.3),
             avg_entropy=torch.tensor(0.9), codebook_loss=torch.tensor(0.2))


@pytest.mark.parametrize("kind", ("hinge", "vanilla", "non-saturating"))
@pytest.mark.parametrize("step", (5, 50))
def test_vqganloss_generator_dict_against_the_formulas(kind, step):
    loss = stubbed(discriminator_loss=kind, reconstruction_loss="l1", reconstruction_weight=2.0, entropy_annealing_factor=0.5, entropy_annealing_steps=100)
    x, y = pair()
    total, d = loss(x, y, dict(EXTRA), step, None, mode="gen")
    lf = StubDisc.logits(y)
    factor = 1.0 if step >= 20 else 0.0
    gan = 0.0 if factor == 0 else (float(R.softplus64(-lf).mean()) if kind == "non-saturating" else -float(lf.mean()))
    rec = 2.0 * float((x.double() - y.double()).abs().mean())
    perc = 3.0 * float((x.double() - y.double()).abs().mean())
    quant = 0.25 + max(0.0, 1 - step / 100) * 0.5 * 0.4
    want = rec + 0.1 * perc + 0.7 * quant + 0.1 * factor * gan
    assert set(d) == {"total_loss", "reconstruction_loss", "perceptual_loss", "quantizer_loss", "weighted_gan_loss", "discriminator_factor", "commitment_loss",
                      "entropy_loss", "per_sample_entropy", "avg_entropy", "d_weight", "gan_loss", "codebook_loss"}
    for k, v in (("total_loss", want), ("reconstruction_loss", rec), ("perceptual_loss", 0.1 * perc), ("quantizer_loss", 0.7 * quant),
                 ("weighted_gan_loss", 0.1 * factor * gan), ("gan_loss", gan), ("discriminator_factor", factor), ("d_weight", 0.1)):
        assert abs(float(d[k]) - v) <= 2e-6 * max(1.0, abs(v)), (k, float(d[k]), v)
    assert abs(float(total) - want) <= 2e-6 * max(1.0, abs(want)) and total.dtype == torch.float32
    assert float(EXTRA["quantizer_loss"]) == 0.25                                # the caller's tensor is not added to in place


@pytest.mark.parametrize("kind", ("hinge", "vanilla", "non-saturating"))
def test_vqganloss_discriminator_dict_and_ema(kind):
    loss = stubbed(discriminator_loss=kind, lecam_regularization_weight=0.5, ema_decay=0.9)
    x, y = pair(4)
    lr, lf = StubDisc.logits(x), StubDisc.logits(y)
    mr, mf = float(lr.mean()), float(lf.mean())
    key = {"hinge": "hinge_d", "vanilla": "vanilla_d", "non-saturating": "non_saturating_d"}[kind]
    ema_r = ema_f = 0.0
    for rep, update in enumerate((False, True, True)):
        total, d = loss(x, y, {}, 30, mode="disc", update_ema=update)
        want = R.losses64(lr, lf)[key] + 0.5 * R.lecam64(mr, mf, ema_r, ema_f)
        assert set(d) == {"discriminator_loss", "logits_real", "logits_fake", "lecam_loss"}
        assert abs(float(total) - want) <= 2e-6 * max(1.0, abs(want)) and abs(float(d["discriminator_loss"]) - want) <= 2e-6 * max(1.0, abs(want)), rep
        assert abs(float(d["logits_real"]) - mr) <= 1e-6 and abs(float(d["logits_fake"]) - mf) <= 1e-6
        assert abs(float(d["lecam_loss"]) - 0.5 * R.lecam64(mr, mf, ema_r, ema_f)) <= 1e-6
        if update:
            ema_r, ema_f = ema_r * 0.9 + mr * 0.1, ema_f * 0.9 + mf * 0.1
        assert abs(float(loss.ema_real_logits_mean) - ema_r) <= 1e-6 and abs(float(loss.ema_fake_logits_mean) - ema_f) <= 1e-6, rep
    assert tuple(loss.ema_real_logits_mean.shape) == (1,) and "ema_fake_logits_mean" in loss.state_dict()
    total, d = loss(x, y, {}, 10, mode="disc")                                   # before discriminator_start the factor is 0
    assert abs(float(total) - float(d["lecam_loss"])) <= 1e-7
    assert loss.should_discriminator_be_trained(20) and not loss.should_discriminator_be_trained(19)


@pytest.mark.parametrize("name", ("resnet50", "lpips"))
def test_vqganloss_checkpoint_load_counts_the_perceptual_network_as_loaded(name):
    """a strict load of a whole loss-module checkpoint leaves nothing to load by hand, for either perceptual loss"""
    src = D.VQGANLoss(DISC_CFG, loss_config(perceptual_loss=name))
    ckpt = {k: v.clone() for k, v in src.state_dict().items()}
    loss = D.VQGANLoss(DISC_CFG, loss_config(perceptual_loss=name))
    assert loss.perceptual_loss._no_weights() is not None
    part = {k: v for k, v in ckpt.items() if not k.startswith("perceptual_loss.")}
    loss.load_state_dict(part, strict=False)
    assert loss.perceptual_loss._no_weights() is not None                     # a checkpoint without the network loads none
    loss.load_state_dict(ckpt, strict=True)
    assert loss.perceptual_loss._no_weights() is None


def test_vqganloss_keys_defaults_and_refusals():
    loss = D.VQGANLoss(DISC_CFG, loss_config())
    keys = set(loss.state_dict())
    assert {"ema_real_logits_mean", "ema_fake_logits_mean", "discriminator.block_in.0.weight", "discriminator.blocks.2.1.kernel", "perceptual_loss.mean",
            "perceptual_loss.model.conv1.weight"} <= keys
    assert (loss.reconstruction_weight, loss.ema_decay, loss.entropy_annealing_steps, loss.entropy_annealing_factor) == (1.0, 0.999, 2000, 0.0)
    assert "ema_real_logits_mean" not in D.VQGANLoss(DISC_CFG, loss_config(lecam_regularization_weight=0.0)).state_dict()
    with pytest.raises(NotImplementedError, match="adopt_weight"):
        D.VQGANLoss(DISC_CFG, loss_config(discriminator_gradient_penalty="adopt_weight"))
    for bad in (dict(discriminator_loss="wgan"), dict(reconstruction_loss="huber"), dict(discriminator_gradient_penalty="r1")):
        with pytest.raises(AssertionError):
            D.VQGANLoss(DISC_CFG, loss_config(**bad))
    with pytest.raises(NotImplementedError, match="Original"):
        D.create_discriminator(Cfg(DISC_CFG, name="Original"))
    with pytest.raises(ValueError, match="not implemented"):
        D.create_discriminator(Cfg(DISC_CFG, name="StyleGAN"))
    with pytest.raises(AssertionError):
        stubbed()(torch.zeros(1, 3, 32, 32), torch.zeros(1, 3, 32, 32), {}, 0, mode="both")


# ------------------------------------------------------------------------------------------------ the pieces against torch
def test_pool_windows_are_torchs():
    for n in range(1, 41):
        x = torch.randn(1, 1, n, 1, generator=torch.Generator().manual_seed(n), dtype=torch.float64)
        want = torch.nn.AdaptiveMaxPool2d((16, 1))(x).flatten()
        got = torch.stack([x[0, 0, a:b, 0].max() for a, b in R.pool_windows(n)])
        assert all(0 <= a < b <= n for a, b in R.pool_windows(n)) and torch.equal(got, want), n
    assert R.pool_windows(16) == [(i, i + 1) for i in range(16)] and R.pool_windows(32)[3] == (6, 8) and R.pool_windows(24)[:2] == [(0, 2), (1, 3)]
    x = torch.randn(2, 3, 24, 40, generator=torch.Generator().manual_seed(1), dtype=torch.float64) - 5.0
    assert torch.equal(R.adaptive_maxpool64(x), torch.nn.AdaptiveMaxPool2d((16, 16))(x))


@pytest.mark.parametrize("k", (3, 4, 5))
def test_blur_padding_rule_against_conv2d(k):
    w = R.blur_kernel64(k)
    for H, W in ((8, 16), (6, 10), (7, 9), (5, 5), (2, 3)):
        x = torch.randn(2, 3, H, W, generator=torch.Generator().manual_seed(H * 100 + W), dtype=torch.float64)
        (t, b), (l, r) = R.blur_pad(H, k), R.blur_pad(W, k)
        want = F.conv2d(F.pad(x, [l, r, t, b]), w[None, None].expand(3, -1, -1, -1), stride=2, groups=3)
        got = R.downsample64(x, k)
        assert tuple(got.shape) == (2, 3, (H + 1) // 2, (W + 1) // 2) == tuple(want.shape), (H, W)
        assert float((got - want).abs().max()) <= 1e-14
    assert R.blur_pad(8, 4) == (1, 1) and R.blur_pad(7, 4) == (1, 2) and R.blur_pad(7, 3) == (1, 1) and R.blur_pad(8, 3) == (0, 1) and R.blur_pad(8, 5) == (1, 2)
    x = torch.randn(1, 2, 7, 9, dtype=torch.float64)
    assert float((R.downsample64(x, 0) - F.avg_pool2d(x, 2)).abs().max()) <= 1e-15


# ------------------------------------------------------------------------------------------------ refusals without a device
def test_constructor_refusals_say_what_is_taken():
    with pytest.raises(NotImplementedError, match="leaky_relu"):
        D.NLayerDiscriminatorv2(activation_fn="silu")
    with pytest.raises(ValueError, match="takes 3"):
        D.NLayerDiscriminatorv2(num_channels=1)
    for h in (48, 16, 0):
        with pytest.raises(ValueError, match="multiples of 32"):
            D.NLayerDiscriminatorv2(hidden_channels=h)
    with pytest.raises(AssertionError):
        D.NLayerDiscriminatorv2(num_stages=0)
    with pytest.raises(AssertionError):
        D.NLayerDiscriminatorv2(blur_resample=True, blur_kernel_size=6)
    with pytest.raises(ValueError, match="stages"):
        D.NLayerDiscriminatorv2(num_stages=5)
    m = D.NLayerDiscriminatorv2(hidden_channels=32)
    for shape in ((1, 3, 40, 64), (1, 3, 16, 64), (1, 3, 528, 64), (1, 1, 64, 64), (0, 3, 64, 64), (3, 64, 64)):
        with pytest.raises(ValueError):
            m.check_images(shape)
    with pytest.raises(RuntimeError, match="no CPU path"):
        m(torch.zeros(1, 3, 64, 64))


def test_c_entries_refuse_bad_arguments_before_any_device_work():
    from maskbit_amd import _lib
    lib = _lib.load()
    buf = (C.c_float * 64)()
    p = C.addressof(buf)
    h = C.c_void_p()
    for args in ((0, 32, 3, 4), (1, 48, 3, 4), (1, 32, 0, 4), (1, 32, 5, 4), (1, 32, 3, 2), (1, 32, 3, 6), (1, 1024, 3, 4), (257, 32, 3, 4)):
        assert lib.mb_disc_create(*args, C.byref(h)) == -1 and lib.mb_last_error(), args
    assert lib.mb_disc_create(1, 32, 3, 4, None) == -1
    assert lib.mb_disc_forward(None, p, 1, 64, 64, 0, p, None, None, None) == -1
    assert lib.mb_disc_load(None, b"block_in.0.weight", p, None, 0, None) == -1
    assert lib.mb_disc_saturation_count(None, None, 0, None) == -1
    for K in (1, 2, 6, -1):
        assert lib.mb_disc_downsample(p, p, None, 1, 8, 8, 32, K, None) == -1
    assert lib.mb_disc_downsample(p, p, p, 1, 8, 8, 40, 4, None) == -1            # partials need whole groups
    assert lib.mb_disc_downsample(p, p, None, 1, 8, 8, 36, 4, None) == -1 and lib.mb_disc_downsample(p, p, None, 1, 1, 8, 32, 4, None) == -1
    assert lib.mb_disc_downsample(None, p, None, 1, 8, 8, 32, 4, None) == -1
    assert lib.mb_disc_groupnorm(p, p, 1, p, p, None, 1, 4, 48, 0.1, None) == -1 and lib.mb_disc_groupnorm(p, p, 0, p, p, None, 1, 4, 32, 0.1, None) == -1
    assert lib.mb_disc_groupnorm(p, p, 1, p, p, None, 1, 4, 32, 1.5, None) == -1 and lib.mb_disc_groupnorm(p, None, 1, p, p, None, 1, 4, 32, 0.1, None) == -1
    assert lib.mb_disc_pool(p, p, 1, 0, 8, 32, None) == -1 and lib.mb_disc_pool(p, p, 1, 8, 8, 12, None) == -1 and lib.mb_disc_pool(p, None, 1, 8, 8, 32, None) == -1
    assert lib.mb_disc_logits(p, p, p, p, None, p, 1, 32, None) == -1 and lib.mb_disc_logits(p, p, p, p, None, None, 1, 12, None) == -1
    assert lib.mb_disc_logits(p, None, p, p, None, None, 1, 32, None) == -1
    assert lib.mb_disc_cols(p, p, 0, 8, 8, 0, None) == -1 and lib.mb_disc_cols(None, p, 1, 8, 8, 0, None) == -1
    assert lib.mb_disc_down_chunks(8, 8, 12) == -1 and lib.mb_disc_down_chunks(8, 8, 32) == 1 and lib.mb_disc_down_chunks(128, 128, 128) == 128
    sat = C.c_uint(0)
    conv = [1, 9, 9, 32, 32, 1, 1, 1, 0, 0, 0, 32, 0, 32, 0]
    assert lib.mb_convbn_layer_leaky(p, p, p, p, p, C.byref(sat), *conv, 3, 1.5, None, 0, 0, None) == -1     # slope outside [0, 1]
    assert lib.mb_convbn_layer_leaky(p, p, p, p, p, C.byref(sat), *conv, 4, 0.1, None, 0, 0, None) == -1
    assert lib.mb_convbn_layer_ex(p, p, p, p, p, C.byref(sat), *conv, 3, None, 0, 0, None) == -1            # the older entry keeps its three epilogues
