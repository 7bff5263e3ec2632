"""Golden fixture of LPIPS: the reference's ``LPIPS`` (modeling/modules/lpips.py) run on the CPU with seeded VGG16 weights
(maskbit_amd.synth.make_vgg16_weights: ImageNet VGG16 is not available) and the reference's own ``pretrained/vgg_lpips.pth``.  Needs the reference
checkout (MASKBIT_REFERENCE, as oracle/make_golden.py).  Writes results, seeds and the five lin vectors only (a few KB) to tests/golden/lpips.npz;
the tests regenerate images and VGG16 weights from the recorded seeds.

The reference builds its VGG16 through ``torchvision.models.vgg16(weights=...)`` (absent here): it gets a stand-in that returns an object whose
``.features`` is an ``nn.Sequential`` in torchvision's VGG16-D layout holding the seeded weights.

Per case and image:  ref32 = the reference as it runs (fp32),  ref64 = the same module and inputs after ``.double()``.

    python tools/make_golden_lpips.py
"""
from __future__ import annotations

import os
import sys
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from oracle import make_golden as MG  # noqa: E402
import lpips_reference as R  # noqa: E402

VGG16_D = (64, 64, "M", 128, 128, "M", 256, 256, 256, "M", 512, 512, 512, "M", 512, 512, 512, "M")


def vgg16_features(state_dict):
    layers, cin = [], 3
    for v in VGG16_D:
        if v == "M":
            layers.append(torch.nn.MaxPool2d(kernel_size=2, stride=2))
        else:
            layers += [torch.nn.Conv2d(cin, v, kernel_size=3, padding=1), torch.nn.ReLU(inplace=True)]
            cin = v
    seq = torch.nn.Sequential(*layers)
    seq.load_state_dict(state_dict, strict=True)
    return seq


def import_reference_lpips(current):
    """``current`` = {"sd": bare VGG16 state dict}: what the stand-in's vgg16() hands out at construction"""
    MG._import_reference()
    tv = sys.modules["torchvision.models"]
    tv.VGG16_Weights = types.SimpleNamespace(IMAGENET1K_V1=None)
    tv.vgg16 = lambda weights=None: types.SimpleNamespace(features=vgg16_features(current["sd"]))
    from modeling.modules import lpips as L
    assert os.path.realpath(L.__file__).startswith(os.path.realpath(MG.REF))
    return L


def main():
    torch.set_grad_enabled(False)
    current = {}
    L = import_reference_lpips(current)
    nets = {}
    for style in ("he", "grown"):
        current["sd"] = R.vgg_weights(style)
        nets[style] = L.LPIPS().eval()
    sd = nets["he"].state_dict()
    assert len(sd) == 33
    out = dict(cases=np.array(list(R.CASES)), vgg_seed=np.int64(R.VGG_SEED), state_dict_keys=np.array(list(sd)))
    for k in range(5):
        out[f"lin{k}"] = sd[f"lin{k}.model.1.weight"].reshape(-1).numpy()
    for name, (fam, sig, B, H, W, seed, style) in R.CASES.items():
        real, fake = R.case_images(name)
        net = nets[style]
        ref32 = net(real, fake).reshape(-1).double().numpy()
        ref64 = net.double()(real.double(), fake.double()).reshape(-1).numpy()
        net.float()
        out[name + ".family"], out[name + ".style"] = np.array(fam), np.array(style)
        out[name + ".params"] = np.array([sig, B, H, W, seed], dtype=np.float64)
        out[name + ".ref32"], out[name + ".ref64"] = ref32, ref64
        print(f"{name:22s} ref64 {ref64}  |ref32 - ref64| {np.abs(ref32 - ref64).max():.3g}")
    np.savez_compressed(R.GOLDEN, **out)
    print(R.GOLDEN, os.path.getsize(R.GOLDEN))


if __name__ == "__main__":
    main()
