"""Golden fixture of the VQGAN+ discriminator: the reference's NLayerDiscriminatorv2 (modeling/modules/discriminator.py) and the loss functions
of modeling/modules/gan_utils.py run on the CPU in fp32 on seeded weights.  Needs the reference checkout (MASKBIT_REFERENCE, as
oracle/make_golden.py); writes the tensor-only tests/golden/discriminator.npz.

Weights come from maskbit_amd.synth.make_discriminator_weights and the images from torch.rand on seeded generators, so the fixture keeps the
seeds, the reference's logits, the loss values on them and the module's state-dict keys -- no weights and no images.

    python tools/make_golden_discriminator.py
    python tools/make_golden_discriminator.py h128      # + tests/golden/discriminator_h128.npz (minutes of float64 convolutions on the CPU)

The second file holds, for the two full-width cases of the GPU test (hidden 128 on 1 x 3 x 256 x 256 and 1 x 3 x 512 x 256), the logits of the
float64 restatement tests/discriminator_reference.py and of its fp16-storage emulation: recorded results of this project's own reference, kept so
that the test does not spend minutes on them.  A third, small case (1 x 3 x 64 x 64) is recomputed by a CPU test: the file must be written
again whenever the restatement changes, and that test says so.
"""
from __future__ import annotations

import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from oracle import make_golden as MG  # noqa: E402
from maskbit_amd.synth import make_discriminator_weights  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "discriminator.npz")
SEED = 900
HIDDEN, STAGES = 32, 3
# name -> (blur kernel size, 0 = average pool; image seed; image shape)
CASES = {"blur4_128": (4, 901, (2, 3, 128, 128)), "blur4_32x48": (4, 902, (1, 3, 32, 48)), "blur4_192x128": (4, 903, (1, 3, 192, 128)),
         "avg_64": (0, 904, (1, 3, 64, 64)), "blur3_64": (3, 905, (1, 3, 64, 64)), "blur5_64": (5, 906, (1, 3, 64, 64))}
# hidden 128, 3 stages, blur 4, weights of seed SEED; h128_64 is the guard: small enough for a CPU test to recompute, so that an edit of the
# restatement which this file does not follow is noticed (tests/test_discriminator_cpu.py)
H128 = {"h128_256": (911, (1, 3, 256, 256)), "h128_512x256": (912, (1, 3, 512, 256)), "h128_64": (913, (1, 3, 64, 64))}
EMA = (0.3, -0.2)                                # ema_real_logits_mean, ema_fake_logits_mean of the LeCam value


def images(seed: int, shape) -> torch.Tensor:
    return torch.rand(*shape, generator=torch.Generator().manual_seed(seed))


def h128():
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import discriminator_reference as R
    sd = make_discriminator_weights(SEED, 128, 3, 4)
    out = dict(seed=np.int64(SEED))
    for name, (iseed, shape) in H128.items():
        x = images(iseed, shape)
        ref, emu = R.forward64(sd, x, 4), R.forward64(sd, x, 4, emulate=True)
        out[f"{name}.image_seed"], out[f"{name}.shape"] = np.int64(iseed), np.array(shape, dtype=np.int64)
        out[f"{name}.ref64"], out[f"{name}.emu64"] = ref.numpy(), emu.numpy()
        print(name, f"logits in [{float(ref.min()):.3f}, {float(ref.max()):.3f}], max |emulation - float64| {float((emu - ref).abs().max()):.3e}")
    path = OUT.replace(".npz", "_h128.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path))


def main():
    torch.set_grad_enabled(False)
    if "h128" in sys.argv[1:]:
        return h128()
    MG._import_reference()
    from modeling.modules import gan_utils
    from modeling.modules.discriminator import NLayerDiscriminatorv2
    assert os.path.realpath(sys.modules["modeling.modules.discriminator"].__file__).startswith(os.path.realpath(MG.REF))
    torch.set_grad_enabled(False)
    out = dict(seed=np.int64(SEED), hidden=np.int64(HIDDEN), stages=np.int64(STAGES), ema=np.array(EMA, dtype=np.float64))
    for name, (blur, iseed, shape) in CASES.items():
        model = NLayerDiscriminatorv2(num_channels=3, hidden_channels=HIDDEN, num_stages=STAGES, blur_resample=blur != 0, blur_kernel_size=blur or 4)
        model.load_state_dict(make_discriminator_weights(SEED, HIDDEN, STAGES, blur), strict=True)
        model.eval()
        logits = model(images(iseed, shape))
        out[f"{name}.blur"], out[f"{name}.image_seed"], out[f"{name}.shape"] = np.int64(blur), np.int64(iseed), np.array(shape, dtype=np.int64)
        out[f"{name}.logits"] = logits.numpy()
        out[f"{name}.logits64"] = model.double()(images(iseed, shape).double()).numpy()    # the reference's own graph in float64: its fp32 error
        print(name, tuple(logits.shape), f"logits in [{float(logits.min()):.3f}, {float(logits.max()):.3f}], std {float(logits.std()):.3f}, "
              f"fp32 vs float64 {float((logits.double() - torch.from_numpy(out[name + '.logits64'])).abs().max()):.3g}")
        out[f"keys.{'blur' if blur else 'avg'}"] = np.array(sorted(model.state_dict().keys()))
    both = torch.from_numpy(out["blur4_128.logits"])
    real, fake = both[0:1], both[1:2]
    out["loss.hinge_d"] = np.float32(gan_utils.hinge_d_loss(real, fake))
    out["loss.vanilla_d"] = np.float32(gan_utils.vanilla_d_loss(real, fake))
    out["loss.non_saturating_d"] = np.float32(gan_utils.non_saturating_d_loss(real, fake))
    out["loss.hinge_g"] = np.float32(gan_utils.hinge_g_loss(fake))
    out["loss.non_saturating_g"] = np.float32(gan_utils.non_saturating_g_loss(fake))
    out["loss.lecam"] = np.float32(gan_utils.compute_lecam_loss(real.mean(), fake.mean(), torch.tensor([EMA[0]]), torch.tensor([EMA[1]])))
    np.savez_compressed(OUT, **out)
    print({k: float(v) for k, v in out.items() if k.startswith("loss.")})
    print(OUT, os.path.getsize(OUT))


if __name__ == "__main__":
    main()
