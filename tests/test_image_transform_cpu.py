"""CPU-side checks of the image transform: the numpy restatement of tests/image_reference.py against Pillow (where it is installed) and against
the recorded fixture tests/golden/image_transform.npz (everywhere) -- every byte --, the two recipes against the Pillow chain written out here,
the ToTensor() table, the ABI surface, and the refusals that need no device."""
import ctypes as C
import inspect
import os
import re

import numpy as np
import pytest
import torch

import image_reference as IR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("mb_image_workspace_bytes", "mb_image_resample")
_GOLDEN = None


def golden():
    global _GOLDEN
    if _GOLDEN is None:
        z = np.load(os.path.join(ROOT, "tests", "golden", "image_transform.npz"), allow_pickle=False)
        _GOLDEN = {k: z[k] for k in z.files}
    return _GOLDEN


CASES = [(src, dst, content, filt) for src, dst in IR.SIZE_CASES for content in IR.CONTENTS for filt in (IR.BOX, IR.BILINEAR, IR.BICUBIC)]
case_id = lambda c: f"{c[0][0]}x{c[0][1]}-{c[1][0]}x{c[1][1]}-{c[2]}-{IR.FILTER_NAMES[c[3]]}"


# ---- the restatement ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_restatement_equals_the_fixture(case):
    (H, W), (h, w), content, filt = case
    z = golden()
    img = IR.make_image(H, W, content)
    assert np.array_equal(img, z[f"in/{H}x{W}/{content}"])                                      # the case builders give the recorded inputs
    assert np.array_equal(IR.resize(img, h, w, filt), z[f"out/{H}x{W}/{h}x{w}/{content}/{IR.FILTER_NAMES[filt]}"])


@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_restatement_equals_pillow(case):
    Image = pytest.importorskip("PIL.Image")
    (H, W), (h, w), content, filt = case
    img = IR.make_image(H, W, content)
    pil = np.asarray(Image.fromarray(img).resize((w, h), {IR.BOX: Image.BOX, IR.BILINEAR: Image.BILINEAR, IR.BICUBIC: Image.BICUBIC}[filt]))
    assert np.array_equal(IR.resize(img, h, w, filt), pil)


def test_checkerboard_drives_the_sum_outside_the_byte_range():
    """Upscaled with bicubic, the 0 / 255 checkerboard overshoots: the clip is exercised, and dropping it changes bytes."""
    seen = []
    out = IR.resize(IR.make_image(9, 7, "checker"), 32, 25, IR.BICUBIC, clip_seen=seen)
    assert seen and np.array_equal(out, golden()["out/9x7/32x25/checker/bicubic"]) and out.min() == 0 and out.max() == 255
    seen = []
    IR.resize(IR.make_image(5, 5, "checker"), 16, 16, IR.BICUBIC, clip_seen=seen)
    assert seen
    seen = []
    IR.resize(IR.make_image(9, 7, "checker"), 32, 25, IR.BILINEAR, clip_seen=seen)               # a convex combination never overshoots
    assert not seen


def test_order_and_intermediate_matter():
    """Vertical first gives other bytes than Pillow's horizontal first on at least one case of the list: the GPU tests tell the orders apart."""
    z = golden()
    differing = 0
    for (H, W), (h, w) in IR.SIZE_CASES:
        img = IR.make_image(H, W, "random")
        wrong = IR.resize(img, h, w, IR.BICUBIC, vertical_first=True)
        differing += not np.array_equal(wrong, z[f"out/{H}x{W}/{h}x{w}/random/bicubic"])
    assert differing >= 3


def test_coefficient_tables_closed_forms():
    xmin, n, k = IR.coeffs(32, 16, IR.BOX)                         # scale 2: two taps of one half
    assert IR.ksize_for(32, 16, IR.BOX) == 3 and n.tolist() == [2] * 16 and xmin.tolist() == list(range(0, 32, 2))
    assert (k[:, :2] == 1 << 21).all() and (k[:, 2] == 0).all()
    xmin, n, k = IR.coeffs(16, 32, IR.BILINEAR)                    # upscaling by 2: weights 0.75 / 0.25 inside, one tap at the edges
    assert k[1, :2].tolist() == [3 << 20, 1 << 20] and n[0] == 1 and k[0, 0] == 1 << 22
    assert IR.ksize_for(300, 16, IR.BICUBIC) == 77 and IR.ksize_for(100, 16, IR.BICUBIC) == 27 and IR.ksize_for(1, 16, IR.BICUBIC) == 5
    for filt in (IR.BOX, IR.BILINEAR, IR.BICUBIC):
        for a, b in ((300, 16), (17, 16), (1, 16), (7, 25)):
            xmin, n, k = IR.coeffs(a, b, filt)
            assert (n >= 1).all() and (xmin + n <= a).all() and (np.abs(k).sum(1) < 1.3 * 2 ** 22).all() and (np.diff(xmin) >= 0).all()
            assert (np.abs(k.sum(1) - (1 << 22)) <= k.shape[1]).all()                            # normalised, up to the taps' rounding
    ident = IR.identity_coeffs(5)
    assert np.array_equal(IR._pass(IR.make_image(5, 4, "random"), *ident, 0), IR.make_image(5, 4, "random"))


# ---- the recipes --------------------------------------------------------------------------------------------------------------------------
def test_recipe_sizes():
    assert IR.reference_sizes(375, 500, 256) == ((256, 341), (0, 42))
    assert IR.reference_sizes(500, 375, 256) == ((341, 256), (42, 0))
    # crop-origin halves round to even: (res - R) / 2 = 0.5 -> 0, 1.5 -> 2
    assert IR.reference_sizes(16, 17, 16) == ((16, 17), (0, 0)) and IR.reference_sizes(16, 19, 16) == ((16, 19), (0, 2))
    assert IR.reference_sizes(16, 40, 16) == ((16, 40), (0, 12)) and IR.reference_sizes(32, 16, 16) == ((32, 16), (8, 0))       # a side equal to R
    assert IR.adm_sizes(375, 500, 256) == ([], (256, 341), (0, 42))
    assert IR.adm_sizes(131, 64, 16) == ([(65, 32), (32, 16)], (32, 16), (8, 0))                 # halved twice
    assert IR.adm_sizes(70, 45, 16) == ([(35, 22)], (25, 16), (4, 0))
    assert IR.adm_sizes(16, 19, 16) == ([], (16, 19), (0, 1))                                     # "adm" floors where "reference" rounds to even


def test_python_plan_matches_the_restatement():
    from maskbit_amd import ImageTransform
    sizes = [im.shape[:2] for im in IR.ragged_batch()] + [(375, 500), (16, 17), (16, 19), (1, 7), (300, 30), (1, 1)]
    for R in (16, 32, 256):
        for interp in ("bilinear", "bicubic"):
            (p,) = ImageTransform(R, interp).plan(sizes)
            assert p["filter"] == interp and p["final"] and [j["image"] for j in p["jobs"]] == list(range(len(sizes)))
            for (H, W), j in zip(sizes, p["jobs"]):
                res, (top, left) = IR.reference_sizes(H, W, R)
                assert j["src_size"] == (H, W) and j["res_size"] == res and j["window"] == (top, left, R, R)
        passes = ImageTransform(R, recipe="adm").plan(sizes)
        assert [p["filter"] for p in passes[:-1]] == ["box"] * (len(passes) - 1) and passes[-1]["filter"] == "bicubic" and passes[-1]["final"]
        for i, (H, W) in enumerate(sizes):
            halvings, res, (top, left) = IR.adm_sizes(H, W, R)
            mine = [j for p in passes[:-1] for j in p["jobs"] if j["image"] == i]
            assert [j["res_size"] for j in mine] == halvings and all(j["window"] == (0, 0) + j["res_size"] for j in mine)
            assert [i in [j["image"] for j in p["jobs"]] for p in passes[:-1]] == [lvl < len(halvings) for lvl in range(len(passes) - 1)]
            last = passes[-1]["jobs"][i]
            assert last["src_size"] == (halvings[-1] if halvings else (H, W)) and last["res_size"] == res and last["window"] == (top, left, R, R)
    assert len(ImageTransform(16, recipe="adm").plan([(131, 64), (70, 45), (20, 33)])) == 3       # 2, 1 and 0 halvings
    with pytest.raises(ValueError, match="beyond 16384"):
        ImageTransform(256).plan([(300, 3)])                                                     # the long side would become 25 600


@pytest.mark.parametrize("R", [16, 32])
def test_recipes_equal_the_fixture(R):
    z = golden()
    for i, img in enumerate(IR.ragged_batch()):
        assert np.array_equal(IR.adm_transform(img, R), z[f"recipe/adm/{R}/{i}"])
        for filt in (IR.BILINEAR, IR.BICUBIC):
            assert np.array_equal(IR.reference_transform(img, R, filt), z[f"recipe/reference-{IR.FILTER_NAMES[filt]}/{R}/{i}"])


def test_recipes_equal_the_pillow_chain():
    Image = pytest.importorskip("PIL.Image")

    def pil_reference(img, R, resample):
        pil = Image.fromarray(img)
        w, h = pil.size
        ow, oh = (R, int(R * h / w)) if w <= h else (int(R * w / h), R)                          # torchvision Resize(int)
        if (w, h) != (ow, oh):
            pil = pil.resize((ow, oh), resample)
        top, left = int(round((oh - R) / 2.0)), int(round((ow - R) / 2.0))                       # torchvision CenterCrop
        return np.asarray(pil.crop((left, top, left + R, top + R)))

    def pil_adm(img, R):                                                                         # guided-diffusion center_crop_arr
        pil = Image.fromarray(img)
        while min(*pil.size) >= 2 * R:
            pil = pil.resize(tuple(x // 2 for x in pil.size), resample=Image.BOX)
        scale = R / min(*pil.size)
        pil = pil.resize(tuple(round(x * scale) for x in pil.size), resample=Image.BICUBIC)
        arr = np.array(pil)
        cy, cx = (arr.shape[0] - R) // 2, (arr.shape[1] - R) // 2
        return arr[cy:cy + R, cx:cx + R]

    cases = [(375, 500, 256), (16, 17, 16), (16, 19, 16), (19, 16, 16), (131, 64, 16), (64, 200, 16), (16, 40, 16), (40, 16, 16), (70, 45, 16)]
    for H, W, R in cases:
        img = IR.make_image(H, W, "random")
        for filt, resample in ((IR.BILINEAR, Image.BILINEAR), (IR.BICUBIC, Image.BICUBIC)):
            out = IR.reference_transform(img, R, filt)
            assert out.shape == (R, R, 3) and np.array_equal(out, pil_reference(img, R, resample)), (H, W, R, filt)
        assert np.array_equal(IR.adm_transform(img, R), pil_adm(img, R)), (H, W, R)
    assert len(IR.adm_sizes(131, 64, 16)[0]) == 2 and len(IR.adm_sizes(64, 200, 16)[0]) == 2    # sources "adm" halves twice


# ---- ToTensor() ---------------------------------------------------------------------------------------------------------------------------
def test_float_table():
    v = np.arange(256, dtype=np.float32)
    table = torch.arange(256, dtype=torch.uint8).to(torch.float32).div(255).numpy()            # what ToTensor() does
    assert table.dtype == np.float32 and np.array_equal(IR.FLOAT_TABLE.view(np.uint32), table.view(np.uint32))
    assert int((v * np.float32(1.0 / 255.0) != IR.FLOAT_TABLE).sum()) == 126                     # a reciprocal multiply is another function
    # the kernel's table entry: the double quotient rounded to float is the correctly rounded float quotient for every byte value
    assert np.array_equal((v.astype(np.float64) / 255.0).astype(np.float32).view(np.uint32), IR.FLOAT_TABLE.view(np.uint32))
    img = IR.make_image(5, 4, "random")
    assert np.array_equal(IR.to_float_nchw(img), torch.from_numpy(img).permute(2, 0, 1).float().div(255).numpy())


# ---- surface ------------------------------------------------------------------------------------------------------------------------------
def test_header_exports_abi_sources_and_all():
    import maskbit_amd
    from maskbit_amd import _lib, build, image_transform
    abi = open(os.path.join(ROOT, "include", "maskbit_hip.h")).read()
    diag = open(os.path.join(ROOT, "include", "maskbit_hip_diag.h")).read()
    lib = C.CDLL(_lib.LIB_PATH)
    for name in ENTRIES:
        assert re.search(r"\b%s\s*\(" % name, abi) and name in _lib.SIGNATURES and hasattr(lib, name)
    assert re.search(r"\bmb_image_coeffs\s*\(", diag) and not re.search(r"\bmb_image_coeffs\s*\(", abi) and "mb_image_coeffs" in _lib.SIGNATURES
    assert hasattr(lib, "mb_image_coeffs")
    assert re.search(r"#define MB_ABI_VERSION 8\b", abi) and _lib.ABI_VERSION == 8 and _lib.load().mb_abi_version() == 8         # additions only
    assert "typedef struct {" in abi and "} mb_image_job;" in abi and C.sizeof(_lib.ImageJob) == 72
    assert len(_lib.SIGNATURES["mb_image_resample"][1]) == 12 and len(_lib.SIGNATURES["mb_image_coeffs"][1]) == 10
    assert "image.hip" in build.SOURCES and os.path.exists(os.path.join(build.CSRC, "image.hip"))
    src = open(os.path.join(build.CSRC, "image.hip")).read()
    assert "#pragma clang fp contract(off)" in src                                               # the coefficients must not be contracted
    for name in ("ImageTransform", "transformed"):
        assert name in maskbit_amd.__all__ and getattr(maskbit_amd, name) is getattr(image_transform, name)
    p = inspect.signature(maskbit_amd.ImageTransform.__init__).parameters
    assert list(p) == ["self", "resolution", "interpolation", "recipe", "device"]
    assert (p["resolution"].default, p["interpolation"].default, p["recipe"].default, p["device"].default) == (256, "bilinear", "reference", None)
    q = inspect.signature(maskbit_amd.transformed).parameters
    assert list(q) == ["loader", "transform", "key"] and q["key"].default == "image"
    # the consumers keep their signatures
    assert list(inspect.signature(maskbit_amd.eval_reconstruction).parameters) == ["model", "loader", "evaluator"]
    assert list(inspect.signature(maskbit_amd.eval_masked_prediction).parameters)[:4] == ["model", "vqgan_model", "loader", "evaluator"]


def job(**kw):
    from maskbit_amd import _lib
    j = dict(src_offset=0, dst_offset=0, src_h=37, src_w=53, src_stride=159, res_h=16, res_w=23, win_y=0, win_x=3, win_h=16, win_w=16)
    j.update(kw)
    arr = (_lib.ImageJob * 1)()
    for k, v in j.items():
        setattr(arr[0], k, v)
    return arr


def test_workspace_layout():
    from maskbit_amd import _lib
    lib = _lib.load()
    jobs = (_lib.ImageJob * 2)()
    for j, (H, W, rh, rw, wy, wx) in zip(jobs, ((37, 53, 16, 23, 0, 3), (16, 40, 16, 40, 0, 12))):
        j.src_h, j.src_w, j.src_stride, j.res_h, j.res_w, j.win_y, j.win_x, j.win_h, j.win_w = H, W, 3 * W, rh, rw, wy, wx, 16, 16
    total = lib.mb_image_workspace_bytes(jobs, 2, IR.BICUBIC)
    assert (jobs[0].kx, jobs[0].ky) == (IR.ksize_for(53, 23, IR.BICUBIC), IR.ksize_for(37, 16, IR.BICUBIC))
    assert (jobs[1].kx, jobs[1].ky) == (1, 1)                                                   # both axes keep their size: identity tables
    slot = lambda j: (4 * (16 * (2 + j.kx) + 16 * (2 + j.ky)) + 15) // 16 * 16 + (48 * j.src_h + 15) // 16 * 16
    assert jobs[0].work_offset == 0 and jobs[1].work_offset == slot(jobs[0]) and total == slot(jobs[0]) + slot(jobs[1])
    assert lib.mb_image_workspace_bytes(jobs, 2, 3) == 0 and lib.mb_image_workspace_bytes(jobs, 0, 1) == 0 and lib.mb_image_workspace_bytes(None, 2, 1) == 0
    assert lib.mb_image_workspace_bytes(job(src_w=16385, src_stride=3 * 16385), 1, 1) == 0 and lib.mb_image_workspace_bytes(job(win_h=0), 1, 1) == 0


def test_library_refuses_without_a_device():
    """Every refusal is decided on the host before a launch and names its entry."""
    from maskbit_amd import _lib
    lib = _lib.load()
    p = 4096                                                   # never dereferenced: each call below is refused first
    good = job()
    need = lib.mb_image_workspace_bytes(good, 1, IR.BILINEAR)
    assert need > 0
    nbytes = 37 * 159

    def call(jobs=good, dev=p, B=1, filt=IR.BILINEAR, src=p, src_bytes=nbytes, u8=p, f32=p, cap=256, work=p, work_bytes=need, lay=True, lay_filt=None):
        if lay and jobs is not None:
            lib.mb_image_workspace_bytes(jobs, 1, IR.BILINEAR if lay_filt is None else lay_filt)
        return lib.mb_image_resample(jobs, dev, B, filt, src, src_bytes, u8, f32, cap, work, work_bytes, None)

    refused = [
        lambda: call(jobs=None), lambda: call(dev=None), lambda: call(src=None), lambda: call(work=None),            # null pointers
        lambda: call(u8=None, f32=None),
        lambda: call(filt=3), lambda: call(filt=-1),                                                                 # nearest / lanczos have no code
        lambda: call(B=0), lambda: call(B=4097),
        lambda: call(jobs=job(src_h=0), lay=False), lambda: call(jobs=job(src_w=16385, src_stride=3 * 16385), lay=False),
        lambda: call(jobs=job(src_h=16385), lay=False), lambda: call(jobs=job(src_w=0), lay=False),
        lambda: call(jobs=job(win_h=0), lay=False), lambda: call(jobs=job(win_w=-1), lay=False),                      # R < 1
        lambda: call(jobs=job(win_x=8)), lambda: call(jobs=job(win_y=1)),                                             # window outside the resized image
        lambda: call(jobs=job(src_stride=158)),
        lambda: call(src_bytes=nbytes - 1), lambda: call(jobs=job(src_offset=1)),                                     # reads beyond the source
        lambda: call(cap=255), lambda: call(jobs=job(dst_offset=1)),                                                  # writes beyond the output
        lambda: call(work_bytes=need - 1),
        lambda: call(lay_filt=IR.BICUBIC),                                                                            # the layout of another filter
        lambda: call(dev=p + 4), lambda: call(work=p + 8), lambda: call(f32=p + 2),
    ]
    for i, c in enumerate(refused):
        assert c() == -1, i
        assert lib.mb_last_error().decode().startswith("mb_image_resample:"), i
    coeffs = [
        lambda: lib.mb_image_coeffs(37, 16, 2, 0, 16, 11, None, p, p, None), lambda: lib.mb_image_coeffs(37, 16, 3, 0, 16, 11, p, p, p, None),
        lambda: lib.mb_image_coeffs(0, 16, 2, 0, 16, 11, p, p, p, None), lambda: lib.mb_image_coeffs(37, 16385, 2, 0, 16, 11, p, p, p, None),
        lambda: lib.mb_image_coeffs(37, 16, 2, 1, 16, 11, p, p, p, None), lambda: lib.mb_image_coeffs(37, 16, 2, 0, 0, 11, p, p, p, None),
        lambda: lib.mb_image_coeffs(37, 16, 2, 0, 16, 13, p, p, p, None), lambda: lib.mb_image_coeffs(16, 16, 2, 0, 16, 5, p, p, p, None),
    ]
    assert IR.ksize_for(37, 16, IR.BICUBIC) == 11
    for i, c in enumerate(coeffs):
        assert c() == -1, i
        assert lib.mb_last_error().decode().startswith("mb_image_coeffs:"), i


def test_python_refusals_without_a_device():
    from maskbit_amd import ImageTransform, transformed
    for bad in ("nearest", "lanczos"):
        with pytest.raises(ValueError, match=bad):
            ImageTransform(256, bad)
    with pytest.raises(ValueError, match="box"):
        ImageTransform(256, "box")
    with pytest.raises(ValueError, match="recipe"):
        ImageTransform(256, recipe="tf")
    with pytest.raises(ValueError, match="resolution"):
        ImageTransform(0)
    t = ImageTransform(16, device="cpu")
    ok = np.zeros((5, 7, 3), np.uint8)
    for images in ([], ok, torch.zeros(2, 5, 7, 3, dtype=torch.uint8), [ok.astype(np.float32)], [ok[:, :, :2]], [ok[:, :, 0]], [np.zeros((0, 7, 3), np.uint8)],
                   [np.zeros((5, 7, 4), np.uint8)], [ok, "x"], [torch.zeros(5, 7, 3)], None):
        with pytest.raises(ValueError):
            t(images)
        with pytest.raises(ValueError):
            t.uint8(images)
    with pytest.raises(ValueError, match="16384"):
        t.plan([(16385, 4)])
    with pytest.raises(RuntimeError, match="no CPU path"):
        t([ok, torch.zeros(9, 3, 3, dtype=torch.uint8)])
    with pytest.raises(RuntimeError, match="no CPU path"):
        next(transformed([{"image": [ok], "class_id": torch.zeros(1)}], t))
    assert ImageTransform(16, "bilinear", "adm").interpolation == "bicubic"                      # "adm" fixes its own filters
