"""CPU checks of the tokenizer evaluator: the C ABI additions, the constructor's refusals, the kernel's window constants, and a float64
restatement of the six metrics (MAE, MSE, PSNR, SSIM, CodebookUsage, CodebookEntropy) against the reference's recorded results
(tests/golden/evaluator.npz, tools/make_golden_evaluator.py).  The restatement is the yardstick tests/test_hip_evaluator.py uses for shapes
that have no golden."""
import ctypes
import functools
import math
import os
import re

import numpy as np
import pytest
import torch

from conftest import ROOT, load_golden
from maskbit_amd.synth import make_eval_images, make_eval_indices

KEYS = ("MAE", "MSE", "PSNR", "SSIM")


@functools.lru_cache(maxsize=None)
def evaluator_golden():
    return load_golden("evaluator.npz")


def image_case(name):
    """-> (real, fake) fp32 [B, 3, H, W] of a golden image case, regenerated from its recorded seed."""
    z = evaluator_golden()
    sig, B, H, W, seed = z[name + ".params"]
    return make_eval_images(str(z[name + ".family"]), float(sig), int(B), int(H), int(W), int(seed))


def index_case(name):
    """-> (K, [indices of every update]) of a golden index case."""
    z = evaluator_golden()
    K = int(z[name + ".K"])
    ups = [make_eval_indices(str(kind), K, [int(v) for v in shape if v >= 0], int(seed))
           for kind, shape, seed in zip(z[name + ".kinds"], z[name + ".shapes"], z[name + ".seeds"])]
    return K, ups


# ---- the float64 restatement ------------------------------------------------------------------------------------------------------------
def window_2d() -> torch.Tensor:
    """The reference's SSIM window, outer(g, g) of the fp32 gaussian(11, 1.5) ROUNDED IN FP32 (evaluator.py:83), as float64."""
    g = torch.from_numpy(evaluator_golden()["window_1d"])
    return torch.outer(g, g).double()


def per_image_metrics64(real: torch.Tensor, fake: torch.Tensor, ssim: bool = True, clamp: bool = False) -> torch.Tensor:
    """float64 [B, 4]: MAE, MSE, PSNR, SSIM of every image (evaluator.py:282-334 on exact inputs); SSIM column NaN when not asked for."""
    x, y = fake.double(), real.double().reshape(fake.shape)
    if clamp:
        x, y = x.clamp(0.0, 1.0), y.clamp(0.0, 1.0)
    B, _, H, W = x.shape
    d = x - y
    mse = d.pow(2).mean(dim=(1, 2, 3))
    out = torch.full((B, 4), float("nan"), dtype=torch.float64)
    out[:, 0] = d.abs().mean(dim=(1, 2, 3))
    out[:, 1] = mse
    out[:, 2] = 10.0 * torch.log10(1.0 / (mse + 1e-10))
    if ssim:
        w = window_2d()
        xp = torch.nn.functional.pad(x, [5, 5, 5, 5], mode="reflect")
        yp = torch.nn.functional.pad(y, [5, 5, 5, 5], mode="reflect")
        f = [torch.zeros_like(x) for _ in range(5)]
        for i in range(11):
            for j in range(11):
                a, b = xp[:, :, i:i + H, j:j + W], yp[:, :, i:i + H, j:j + W]
                for acc, v in zip(f, (a, b, a * a, b * b, a * b)):
                    acc += w[i, j] * v
        c1, c2 = 0.01 ** 2, 0.03 ** 2
        mu_xx, mu_yy, mu_xy = f[0] * f[0], f[1] * f[1], f[0] * f[1]
        s_xx, s_yy, s_xy = f[2] - mu_xx, f[3] - mu_yy, f[4] - mu_xy
        idx = ((2 * mu_xy + c1) * (2 * s_xy + c2)) / ((mu_xx + mu_yy + c1) * (s_xx + s_yy + c2))
        out[:, 3] = idx.mean(dim=(1, 2, 3))
    return out


def codebook_metrics64(K: int, updates):
    """-> (usage, entropy, counts int64 [K]) of evaluator.py:370-375,457-464 from a bincount."""
    counts = torch.zeros(K, dtype=torch.int64)
    for idx in updates:
        counts += torch.bincount(idx.flatten().cpu(), minlength=K)
    p = counts.double() / counts.double().sum()
    return float((counts > 0).sum()) / K, float((-torch.log2(p + 1e-8) * p).sum()), counts


# ---- tests ----------------------------------------------------------------------------------------------------------------------------
def test_abi_exports_evaluator_entries():
    from maskbit_amd import _lib
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name in ("mb_eval_workspace_bytes", "mb_eval_images", "mb_eval_codebook"):
        assert name in _lib.SIGNATURES
        getattr(lib, name)
    assert _lib.load().mb_abi_version() == 8 == _lib.ABI_VERSION
    ws = _lib.load().mb_eval_workspace_bytes
    assert ws(64, 3, 256, 256) == 64 * 3 * 64 * 3 * 8
    assert ws(1, 1, 6, 6) == 24 and ws(2, 3, 37, 50) == 2 * 3 * 4 * 3 * 8
    assert ws(1, 3, 5, 64) == 0 and ws(0, 3, 64, 64) == 0            # H < 6, empty batch: not taken


def test_kernel_window_is_the_references_gaussian_bit_for_bit():
    src = open(os.path.join(ROOT, "maskbit_amd", "csrc", "evaluator.hip")).read()
    body = re.search(r"#define EV_GAUSS_1D(.*?)\}", src, re.S).group(1)
    taps = np.array([float.fromhex(t[:-1]) for t in re.findall(r"0x[0-9a-f.]+p[-+]?\d+f", body)], dtype=np.float64)
    ref = evaluator_golden()["window_1d"]
    assert ref.dtype == np.float32 and taps.shape == (11,)
    assert np.array_equal(taps.astype(np.float32).astype(np.float64), taps)          # every literal is an fp32 value
    assert np.array_equal(taps.astype(np.float32), ref)
    k = torch.linspace(-5.0, 5.0, steps=11)
    g = torch.exp(-0.5 * (k / 1.5).pow(2))
    assert np.allclose((g / g.sum()).numpy(), ref, rtol=1e-6, atol=0)                 # and it is gaussian(11, 1.5) (evaluator.py:44-56)


def test_constructor_refuses_network_metrics_and_cpu():
    from maskbit_amd import TokenizerEvaluator
    for kw in ("enable_rfid", "enable_inception_score", "enable_lpips_score"):
        with pytest.raises(NotImplementedError, match="reference's own evaluator"):
            TokenizerEvaluator("cuda:0", **{kw: True})
    with pytest.raises(RuntimeError, match="no CPU path"):
        TokenizerEvaluator("cpu", enable_psnr_score=True)
    with pytest.raises(RuntimeError, match="no CPU path"):
        TokenizerEvaluator(torch.device("cpu"))
    with pytest.raises(ValueError):
        TokenizerEvaluator("cuda:0", enable_codebook_usage_measure=True, num_codebook_entries=0)


def test_constructor_keywords_are_the_references():
    import inspect
    from maskbit_amd import TokenizerEvaluator, eval_reconstruction
    p = inspect.signature(TokenizerEvaluator.__init__).parameters
    assert list(p) == ["self", "device", "enable_rfid", "enable_inception_score", "enable_psnr_score", "enable_ssim_score", "enable_lpips_score",
                       "enable_mse_error", "enable_mae_error", "enable_codebook_usage_measure", "enable_codebook_entropy_measure",
                       "num_codebook_entries"]                                                                     # evaluator.py:146-158
    assert all(p[k].default is False for k in list(p)[2:-1]) and p["num_codebook_entries"].default == 1024
    u = inspect.signature(TokenizerEvaluator.update).parameters
    assert list(u) == ["self", "real_images", "fake_images", "codebook_indices", "clamp"] and u["clamp"].default is False
    assert list(inspect.signature(eval_reconstruction).parameters) == ["model", "loader", "evaluator"]


@pytest.mark.parametrize("name", [str(n) for n in evaluator_golden()["image_cases"]])
def test_fp64_restatement_reproduces_ref64_images(name):
    z = evaluator_golden()
    real, fake = image_case(name)
    ours = per_image_metrics64(real, fake).numpy()
    ref = z[name + ".ref64_img"]
    assert ours.shape == ref.shape
    for k in range(4):
        scale = np.maximum(1.0, np.abs(ref[:, k]))
        assert np.all(np.abs(ours[:, k] - ref[:, k]) <= 1e-12 * scale), (KEYS[k], ours[:, k] - ref[:, k])
    assert np.all(np.abs(ours.mean(0) - z[name + ".ref64"]) <= 1e-12 * np.maximum(1.0, np.abs(z[name + ".ref64"])))
    # the recorded unit of the SSIM bound is the reference's own fp32 error, and it is small next to SSIM itself
    e_ref = float(z[name + ".E_ref"])
    assert e_ref == np.abs(z[name + ".ref32_img"][:, 3] - ref[:, 3]).max() and 0.0 < e_ref < 1e-4


@pytest.mark.parametrize("name", [str(n) for n in evaluator_golden()["index_cases"]])
def test_fp64_restatement_reproduces_codebook_metrics(name):
    z = evaluator_golden()
    K, ups = index_case(name)
    usage, entropy, counts = codebook_metrics64(K, ups)
    assert usage == float(z[name + ".usage"])
    assert abs(entropy - float(z[name + ".entropy"])) <= 1e-12
    assert usage < 1.0 and int(counts.max()) > 1                      # not every entry used, some repeated


def test_golden_covers_the_issue_cases():
    z = evaluator_golden()
    names = [str(n) for n in z["image_cases"]]
    for fam in ("noise", "sin", "flat", "bright"):
        for tag in ("lo", "hi"):
            assert tuple(z[f"{fam}_{tag}.params"][1:4]) == (6.0, 128.0, 128.0)
    sizes = {tuple(int(v) for v in z[n + ".params"][2:4]) for n in names}
    assert {(256, 256), (64, 64), (37, 50)} <= sizes
    assert {int(z[str(n) + ".K"]) for n in z["index_cases"]} == {1024, 4096, 65536}
    assert any(len(z[str(n) + ".seeds"]) > 1 for n in z["index_cases"])
    assert math.isclose(float(z["window_1d"].astype(np.float64).sum()), 1.0, abs_tol=1e-6)
