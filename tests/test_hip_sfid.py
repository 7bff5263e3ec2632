"""GPU checks of the sFID path: the ``"spatial"`` features of InceptionV3 (mb_inception_forward_spatial) and GeneratorEvaluator.use_spatial_statistics.

``spatial`` [B, 2023] = the first 7 channels of Mixed_6d.branch1x1 (BatchNorm, ReLU) on the 17 x 17 map in (h, w, c) order.  Yardsticks, none from
the code under test:
* against tests/inception_reference.py's ``Net`` run up to that layer, in float64 (``exact``) and with the engine's fp16 storage (``model``): the
  criterion of test_hip_inception.py for maps -- error rms <= 1.5 x and max <= 2 x the model's own error against float64.
* the order: a weight set whose channel c of that layer is the constant c + 1 (zero convolution, BatchNorm shift c + 1) gives rows 1, 2, .. 7 repeated.
* bit identity: rows against batch and chunking, the other outputs with and without ``spatial``: torch.equal.
* sFID: |hip - float64| <= S 2^-52 (tr S_r + tr S_f), the bound test_hip_fid.py states for FID (its other term, the golden reference's own error,
  has no counterpart here), against tests/fid_reference.py's float64 evaluation of the same features; full-rank statistics (more rows than columns),
  as there.
"""
import functools

import numpy as np
import pytest
import torch

import fid_reference as FR
import inception_reference as R
from maskbit_amd.synth import make_eval_features, make_eval_statistics

pytestmark = pytest.mark.gpu
DEV = "cuda"
KEYS = ["2048", "logits_unbiased", "spatial"]


def spatial64(u8, sd, model):
    """R.Net up to Mixed_6d.branch1x1 -> float64 [B, 2023] in (h, w, c) order"""
    net = R.Net(sd, model)
    x = net.store(R.input64(u8))
    x = net.conv(x, "Conv2d_1a_3x3", stride=2)
    x = net.conv(x, "Conv2d_2a_3x3")
    x = net.conv(x, "Conv2d_2b_3x3", padding=1)
    x = torch.nn.functional.max_pool2d(x, 3, 2)
    x = net.conv(x, "Conv2d_3b_1x1")
    x = net.conv(x, "Conv2d_4a_3x3")
    x = torch.nn.functional.max_pool2d(x, 3, 2)
    for n in ("Mixed_5b", "Mixed_5c", "Mixed_5d"):
        x = net.a(x, n)
    x = net.b(x, "Mixed_6a")
    for n in ("Mixed_6b", "Mixed_6c"):
        x = net.c(x, n)
    y = net.conv(x, "Mixed_6d.branch1x1")
    assert tuple(y.shape[1:]) == (192, 17, 17)
    return y[:, :7].permute(0, 2, 3, 1).reshape(y.shape[0], -1)


@functools.lru_cache(maxsize=None)
def hip_model(style):
    from maskbit_amd import InceptionV3
    m = InceptionV3(KEYS)
    m.load_weights(R.weights(style))
    return m.to(DEV)


def images(n, seed=9, side=64):
    return R.images_u8(n, side, side, seed).to(DEV)


@pytest.mark.parametrize("name", list(R.CASES))
def test_spatial_against_the_restatement(name):
    sd = R.weights(R.CASES[name][4])
    u8 = R.case_images(name)
    with torch.no_grad():
        exact, model = spatial64(u8, sd, False), spatial64(u8, sd, True)
    got = hip_model(R.CASES[name][4])(u8.to(DEV))["spatial"]
    assert tuple(got.shape) == (u8.shape[0], 2023) and got.dtype == torch.float32
    got = got.cpu().double()
    e_hip, e_mod = got - exact, model - exact
    r_rms = (e_hip.pow(2).mean().sqrt() / e_mod.pow(2).mean().sqrt()).item()
    r_max = (e_hip.abs().max() / e_mod.abs().max()).item()
    print(f"{name} spatial: rms error / model's {r_rms:.3f}, max error / model's {r_max:.3f}; nonzero share {(exact > 0).double().mean():.2f}")
    assert 0.05 < (exact > 0).double().mean() < 1.0 and float(e_mod.abs().max()) > 0      # (the inputs: the ReLU neither cuts everything nor nothing)
    assert bool(torch.isfinite(got).all()) and r_rms <= 1.5 and r_max <= 2.0


def test_spatial_order_is_h_w_c():
    from maskbit_amd import InceptionV3
    sd = dict(R.weights("he"))
    n = "Mixed_6d.branch1x1"
    sd[n + ".conv.weight"] = torch.zeros_like(sd[n + ".conv.weight"])
    sd[n + ".bn.running_mean"] = torch.zeros_like(sd[n + ".bn.running_mean"])
    sd[n + ".bn.bias"] = torch.arange(1, 193, dtype=torch.float32)                 # scale * 0 + (bias - 0 * scale) = c + 1
    m = InceptionV3(KEYS)
    m.load_weights(sd)
    got = m.to(DEV)(images(3))["spatial"]
    want = torch.arange(1, 8, dtype=torch.float32, device=DEV).repeat(17 * 17).expand(3, -1)
    assert tuple(got.shape) == (3, 2023) and torch.equal(got, want)


def test_rows_and_the_other_outputs_keep_their_bits():
    from maskbit_amd import InceptionV3
    x = images(5, seed=10)
    m = hip_model("he")
    whole = m(x)
    assert list(whole) == KEYS
    again = m(x)
    assert all(torch.equal(whole[k], again[k]) for k in whole)
    small = InceptionV3(KEYS)
    small.load_weights(R.weights("he"))
    small = small.to(DEV)
    small.max_images_per_call = 2                                                  # 5 = 2 + 2 + 1
    chunked = small(x)
    assert all(torch.equal(whole[k], chunked[k]) for k in whole)
    for b in (0, 3, 4):
        one = m(x[b:b + 1])
        assert all(torch.equal(one[k], whole[k][b:b + 1]) for k in whole), b
    # without "spatial" (mb_inception_forward), and next to the pooled taps (mb_inception_taps + a pass for spatial): the same bits
    plain = InceptionV3()
    plain.load_weights(R.weights("he"))
    out = plain.to(DEV)(x)
    assert list(out) == ["2048", "logits_unbiased"]
    assert torch.equal(out["2048"], whole["2048"]) and torch.equal(out["logits_unbiased"], whole["logits_unbiased"])
    every = InceptionV3(["64", "768", "spatial", "2048", "logits"])
    every.load_weights(R.weights("he"))
    out = every.to(DEV)(x)
    assert list(out) == ["64", "768", "spatial", "2048", "logits"]
    assert torch.equal(out["spatial"], whole["spatial"]) and torch.equal(out["2048"], whole["2048"])
    assert m.saturation_count() == 0


# ---- the evaluator ------------------------------------------------------------------------------------------------------------------------
S, N_REAL, N_FAKE = 40, 96, 67


def spatial_case():
    mu_s, sigma_s = make_eval_statistics(S, N_REAL, seed=21)
    fake, logits = make_eval_features(S, 10, N_FAKE, seed=22, kind="fake")
    pool, _ = make_eval_features(16, 10, N_FAKE, seed=23, kind="fake")
    return mu_s, sigma_s, fake, logits, pool, make_eval_statistics(16, 40, seed=24)


def test_sfid_against_float64(tmp_path):
    from maskbit_amd import GeneratorEvaluator
    mu_s, sigma_s, fake, logits, pool, stats = spatial_case()
    total, sigma = torch.zeros(S, dtype=torch.float64), torch.zeros(S, S, dtype=torch.float64)
    total, sigma, _, _ = FR.fid_update64(total, sigma, fake)
    cov = FR.covariance64(sigma, total, N_FAKE)
    want = FR.frechet64(mu_s, sigma_s, total / N_FAKE, cov)
    bound = S * 2.0 ** -52 * float(torch.trace(sigma_s) + torch.trace(cov))

    def run(statistics_s, dtype):
        ev = GeneratorEvaluator(DEV, enable_fid=True, enable_inception_score=True)
        ev.use_inception(None, stats)
        ev.use_spatial_statistics(statistics_s)
        at = 0
        for n in (1, 3, 32, N_FAKE - 36):
            ev.update_features_spatial(pool[at:at + n].to(DEV), logits[at:at + n].to(DEV), fake[at:at + n].to(DEV, dtype))
            at += n
        return ev

    ev = run((mu_s, sigma_s), torch.float64)
    r = ev.result()
    assert list(r) == ["InceptionScore", "FID", "sFID"] and isinstance(r["sFID"], float)
    print(f"sFID {r['sFID']:.12g}, float64 {want:.12g}, |diff| {abs(r['sFID'] - want):.3g}, bound {bound:.3g}")
    assert want > 1.0 and abs(r["sFID"] - want) <= bound
    n, t, s = ev.spatial_statistics()
    assert n == N_FAKE and t.shape == (S,) and s.shape == (S, S) and torch.equal(s, s.T)
    # the ADM file format: an .npz with mu_s / sigma_s
    path = tmp_path / "ref_batch.npz"
    np.savez(path, mu=np.zeros(3), sigma=np.eye(3), mu_s=mu_s.numpy(), sigma_s=sigma_s.numpy())
    assert run(str(path), torch.float64).result() == r
    # the pre-existing keys keep their bits; without the call the result is what it was
    base = GeneratorEvaluator(DEV, enable_fid=True, enable_inception_score=True)
    base.use_inception(None, stats)
    at = 0
    for n in (1, 3, 32, N_FAKE - 36):
        base.update_features(pool[at:at + n].to(DEV), logits[at:at + n].to(DEV))
        at += n
    rb = base.result()
    assert list(rb) == ["InceptionScore", "FID"] and all(rb[k] == r[k] for k in rb)
    ev.reset_metrics()
    with pytest.raises(ValueError, match="No examples"):
        ev.result()
    ev.use_spatial_statistics(None)
    ev.update_features(pool.to(DEV), logits.to(DEV))
    assert list(ev.result()) == ["InceptionScore", "FID"]


def test_sfid_refusals(tmp_path):
    from maskbit_amd import GeneratorEvaluator
    mu_s, sigma_s, fake, logits, pool, stats = spatial_case()
    ev = GeneratorEvaluator(DEV, enable_fid=True, enable_inception_score=True)
    ev.use_inception(lambda u8: {"2048": pool[:u8.shape[0]].to(DEV), "logits_unbiased": logits[:u8.shape[0]].to(DEV)}, stats)
    with pytest.raises(ValueError, match="no spatial statistics"):
        ev.update_features_spatial(pool[:4].to(DEV), logits[:4].to(DEV), fake[:4].to(DEV))
    path = tmp_path / "no_spatial.npz"
    np.savez(path, mu=np.zeros(3), sigma=np.eye(3))
    with pytest.raises(ValueError, match="mu_s"):
        ev.use_spatial_statistics(str(path))
    with pytest.raises(ValueError, match="does not exist"):
        ev.use_spatial_statistics(str(tmp_path / "missing.npz"))
    with pytest.raises(ValueError, match="sigma of that size"):
        ev.use_spatial_statistics((mu_s, sigma_s[:, :5]))
    ev.use_spatial_statistics((mu_s, sigma_s))
    with pytest.raises(ValueError, match="'spatial'"):                                  # the attached extractor does not return the key
        ev.update_uint8(torch.zeros(4, 3, 8, 8, dtype=torch.uint8, device=DEV))
    with pytest.raises(ValueError, match="spatial features"):
        ev.update_features(pool[:4].to(DEV), logits[:4].to(DEV))
    with pytest.raises(ValueError, match="columns"):
        ev.update_features_spatial(pool[:4].to(DEV), logits[:4].to(DEV), fake[:4, :7].to(DEV))
    with pytest.raises(ValueError, match="for a batch of"):
        ev.update_features_spatial(pool[:4].to(DEV), logits[:4].to(DEV), fake[:5].to(DEV))
    with pytest.raises(ValueError, match="No examples"):
        ev.result()                                                                    # nothing was accumulated by the refused updates
    ev.update_features_spatial(pool[:4].to(DEV), logits[:4].to(DEV), fake[:4].to(DEV))
    with pytest.raises(ValueError, match="in progress"):
        ev.use_spatial_statistics((mu_s, sigma_s))


def test_evaluator_takes_the_spatial_features_of_the_network():
    from maskbit_amd import GeneratorEvaluator
    net = hip_model("tf")
    x = images(6, seed=11)
    stats = (torch.zeros(2048, dtype=torch.float64), torch.eye(2048, dtype=torch.float64))
    stats_s = (torch.zeros(2023, dtype=torch.float64), torch.eye(2023, dtype=torch.float64))
    a = GeneratorEvaluator(DEV, enable_fid=True, enable_inception_score=True)
    a.use_inception(net, stats)
    a.use_spatial_statistics(stats_s)
    a.update_uint8(x[:4])
    a.update_uint8(x[4:])
    feats = net(x)
    b = GeneratorEvaluator(DEV, enable_fid=True, enable_inception_score=True)
    b.use_inception(None, stats)
    b.use_spatial_statistics(stats_s)
    b.update_features_spatial(feats["2048"][:4], feats["logits_unbiased"][:4], feats["spatial"][:4])
    b.update_features_spatial(feats["2048"][4:], feats["logits_unbiased"][4:], feats["spatial"][4:])
    (na, ta, sa), (nb, tb, sb) = a.spatial_statistics(), b.spatial_statistics()
    assert na == nb == 6 and torch.equal(ta, tb) and torch.equal(sa, sb) and float(ta.sum()) > 0
    assert torch.allclose(ta, feats["spatial"].double().sum(0), rtol=1e-12, atol=0)
