"""Golden fixture of the tokenizer evaluator: the reference's ``TokenizerEvaluator`` (evaluator/evaluator.py:145-466) run on the CPU on
seeded procedural inputs.  Needs the reference checkout (MASKBIT_REFERENCE, as oracle/make_golden.py); writes results only (a few KB) to
tests/golden/evaluator.npz -- the tests regenerate the inputs from the recorded seeds (maskbit_amd.synth.make_eval_images / make_eval_indices).

Per image case, for every image alone and for the whole batch, [MAE, MSE, PSNR, SSIM] of
  ref32  the reference as it runs (fp32 inputs, fp32 window),
  ref64  the same code on ``.double()`` inputs with its window cast to double (the fp32-rounded 2-D weights, evaluated exactly),
and E_ref = max over the case's images of |ref32 - ref64| of SSIM: the reference's own fp32 evaluation error, the unit of the SSIM bound.
Per index case the reference's CodebookUsage and CodebookEntropy.  ``window_1d`` is ``gaussian(11, 1.5)`` as the reference builds it.

The reference imports torchvision and torch_fidelity for its network metrics (absent here, out of scope): they get empty stand-ins.

    python tools/make_golden_evaluator.py
"""
from __future__ import annotations

import os
import sys
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from oracle import make_golden as MG  # noqa: E402
from maskbit_amd.synth import make_eval_images, make_eval_indices  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "evaluator.npz")

# name -> (family, err_sigma, B, H, W, seed)
IMAGE_CASES = {}
for _i, _fam in enumerate(("noise", "sin", "flat", "bright")):
    for _j, _sig in enumerate((0.003, 0.05)):
        IMAGE_CASES[f"{_fam}_{'lo' if _j == 0 else 'hi'}"] = (_fam, _sig, 6, 128, 128, 1000 + 10 * _i + _j)
IMAGE_CASES["noise_256"] = ("noise", 0.05, 2, 256, 256, 1100)
IMAGE_CASES["sin_64"] = ("sin", 0.003, 3, 64, 64, 1101)
IMAGE_CASES["bright_37x50"] = ("bright", 0.05, 3, 37, 50, 1102)

# name -> (K, [(kind, shape, seed) per update])
INDEX_CASES = {
    "cb1024_partial": (1024, [("uniform", (4, 16, 16), 2000)]),                 # 1024 draws: about 63 % of the entries used
    "cb1024_skew": (1024, [("skew", (8, 16, 16), 2001)]),
    "cb4096_repeated": (4096, [("uniform", (8, 16, 16), 2010), ("skew", (8, 16, 16), 2011), ("uniform", (3, 256), 2012)]),
    "cb65536_sparse": (65536, [("uniform", (6, 256), 2020), ("skew", (6, 256), 2021)]),
}

KEYS = ("MAE", "MSE", "PSNR", "SSIM")


def import_reference_evaluator():
    MG._import_reference()                              # torchvision stand-ins, reference root first on sys.path
    names = ("torch_fidelity", "torch_fidelity.feature_extractor_base", "torch_fidelity.helpers", "torch_fidelity.feature_extractor_inceptionv3",
             "torch_fidelity.interpolate_compat_tensorflow")
    for name in names:
        sys.modules.setdefault(name, types.ModuleType(name))
    sys.modules["torch_fidelity.feature_extractor_base"].FeatureExtractorBase = object
    sys.modules["torch_fidelity.helpers"].vassert = None
    for cls in ("BasicConv2d", "InceptionA", "InceptionB", "InceptionC", "InceptionD", "InceptionE_1", "InceptionE_2"):
        setattr(sys.modules["torch_fidelity.feature_extractor_inceptionv3"], cls, object)
    sys.modules["torch_fidelity.interpolate_compat_tensorflow"].interpolate_bilinear_2d_like_tensorflow1x = None
    from evaluator import evaluator as E
    assert os.path.realpath(E.__file__).startswith(os.path.realpath(MG.REF))
    return E


def image_metrics(E, real, fake, double):
    ev = E.TokenizerEvaluator("cpu", enable_psnr_score=True, enable_ssim_score=True, enable_mse_error=True, enable_mae_error=True)
    if double:
        ev._ssim_kernel = ev._ssim_kernel.double()
        real, fake = real.double(), fake.double()
    ev.update(real, fake)
    r = ev.result()
    assert tuple(r) == KEYS
    return np.array([r[k] for k in KEYS], dtype=np.float64)


def main():
    E = import_reference_evaluator()
    torch.set_grad_enabled(False)
    out = dict(window_1d=E.gaussian(11, 1.5).numpy(), image_cases=np.array(list(IMAGE_CASES)), index_cases=np.array(list(INDEX_CASES)))
    for name, (fam, sig, B, H, W, seed) in IMAGE_CASES.items():
        real, fake = make_eval_images(fam, sig, B, H, W, seed)
        out[name + ".family"] = np.array(fam)
        out[name + ".params"] = np.array([sig, B, H, W, seed], dtype=np.float64)
        for tag, dbl in (("ref32", False), ("ref64", True)):
            out[f"{name}.{tag}"] = image_metrics(E, real, fake, dbl)
            out[f"{name}.{tag}_img"] = np.stack([image_metrics(E, real[b:b + 1], fake[b:b + 1], dbl) for b in range(B)])
        e_ref = np.abs(out[name + ".ref32_img"][:, 3] - out[name + ".ref64_img"][:, 3]).max()
        out[name + ".E_ref"] = np.float64(e_ref)
        print(f"{name:14s} SSIM {out[name + '.ref64'][3]:.6f} PSNR {out[name + '.ref64'][2]:.3f} E_ref {e_ref:.3g}")
    for name, (K, updates) in INDEX_CASES.items():
        ev = E.TokenizerEvaluator("cpu", enable_codebook_usage_measure=True, enable_codebook_entropy_measure=True, num_codebook_entries=K)
        dummy = torch.zeros(1, 3, 8, 8)
        for kind, shape, seed in updates:
            ev.update(dummy, dummy, make_eval_indices(kind, K, shape, seed))
        r = ev.result()
        out[name + ".K"] = np.int64(K)
        out[name + ".kinds"] = np.array([u[0] for u in updates])
        out[name + ".shapes"] = np.array([list(u[1]) + [-1] * (3 - len(u[1])) for u in updates], dtype=np.int64)
        out[name + ".seeds"] = np.array([u[2] for u in updates], dtype=np.int64)
        out[name + ".usage"] = np.float64(r["CodebookUsage"])
        out[name + ".entropy"] = np.float64(r["CodebookEntropy"].item())
        print(f"{name:16s} usage {r['CodebookUsage']:.6f} entropy {r['CodebookEntropy'].item():.9f}")
    np.savez_compressed(OUT, **out)
    print(OUT, os.path.getsize(OUT))


if __name__ == "__main__":
    main()
