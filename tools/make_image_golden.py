"""Records tests/golden/image_transform.npz from Pillow: the inputs of tests/image_reference.py's size list and what ``PIL.Image.resize`` gives
for them with BOX / BILINEAR / BICUBIC, and the two loader recipes written out with Pillow calls on the ragged batch at R = 16 and 32.  The
fixture keeps the numpy restatement pinned on a machine without Pillow.

    python tools/make_image_golden.py            # needs Pillow; prints its version and the file size
"""
import os
import sys

import numpy as np
from PIL import Image

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import image_reference as IR  # noqa: E402

PIL_FILTER = {IR.BOX: Image.BOX, IR.BILINEAR: Image.BILINEAR, IR.BICUBIC: Image.BICUBIC}


def pil_reference(img, R, filt):
    """torchvision Resize(R) + CenterCrop(R) on a PIL image, written out."""
    pil = Image.fromarray(img)
    w, h = pil.size
    if w <= h:
        ow, oh = R, int(R * h / w)
    else:
        oh, ow = R, int(R * w / h)
    if (w, h) != (ow, oh):
        pil = pil.resize((ow, oh), PIL_FILTER[filt])
    top, left = int(round((oh - R) / 2.0)), int(round((ow - R) / 2.0))
    return np.asarray(pil.crop((left, top, left + R, top + R)))


def pil_adm(img, R):
    """guided-diffusion's center_crop_arr."""
    pil = Image.fromarray(img)
    while min(*pil.size) >= 2 * R:
        pil = pil.resize(tuple(x // 2 for x in pil.size), resample=Image.BOX)
    scale = R / min(*pil.size)
    pil = pil.resize(tuple(round(x * scale) for x in pil.size), resample=Image.BICUBIC)
    arr = np.array(pil)
    cy, cx = (arr.shape[0] - R) // 2, (arr.shape[1] - R) // 2
    return arr[cy:cy + R, cx:cx + R]


def main():
    import PIL
    out = {"pillow_version": np.array(PIL.__version__)}
    for (H, W), (h, w) in IR.SIZE_CASES:
        for content in IR.CONTENTS:
            img = IR.make_image(H, W, content)
            out[f"in/{H}x{W}/{content}"] = img
            for filt, name in IR.FILTER_NAMES.items():
                out[f"out/{H}x{W}/{h}x{w}/{content}/{name}"] = np.asarray(Image.fromarray(img).resize((w, h), PIL_FILTER[filt]))
    for R in (16, 32):
        for i, img in enumerate(IR.ragged_batch()):
            out[f"recipe/adm/{R}/{i}"] = pil_adm(img, R)
            for filt in (IR.BILINEAR, IR.BICUBIC):
                out[f"recipe/reference-{IR.FILTER_NAMES[filt]}/{R}/{i}"] = pil_reference(img, R, filt)
    path = os.path.join(ROOT, "tests", "golden", "image_transform.npz")
    np.savez_compressed(path, **out)
    print(f"Pillow {PIL.__version__}: {len(out)} arrays, {os.path.getsize(path)} bytes -> {path}")


if __name__ == "__main__":
    main()
