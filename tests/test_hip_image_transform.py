"""GPU checks of csrc/image.hip (mb_image_coeffs, mb_image_resample) and maskbit_amd.ImageTransform against the numpy restatement of Pillow's
resize in tests/image_reference.py (itself pinned to Pillow and to tests/golden/image_transform.npz by tests/test_image_transform_cpu.py).

Everything is EQUALITY: every coefficient, every output byte, every bit of every float.  There is no tolerance anywhere in this file.  Each case
is milliseconds of device work; the restatement's outputs are computed once per case and shared.
"""
import ctypes as C
import functools
import os

import numpy as np
import pytest
import torch

import image_reference as IR

pytestmark = pytest.mark.gpu
DEV = "cuda"
FILTERS = (IR.BOX, IR.BILINEAR, IR.BICUBIC)
U8_SENTINEL, F32_SENTINEL, GUARD = 0xA5, -7.0, 64
# beyond the CPU list: a horizontal segment too long for the LDS tile (the global-byte path, 751 taps), and more than one tile of outputs along x
EXTRA_CASES = [((3, 1500), (3, 8)), ((6, 700), (5, 600))]


@functools.lru_cache(maxsize=None)
def expected(H, W, h, w, content, filt):
    out = IR.resize(IR.make_image(H, W, content), h, w, filt)
    out.setflags(write=False)
    return out


def stream():
    return torch.cuda.current_stream().cuda_stream


class Pass:
    """One mb_image_resample call on caller buffers: sources packed into one device buffer at the given (odd) offsets and padded strides between
    random bytes, sentinel-filled outputs with guard bytes before and after."""

    def __init__(self, images, geometry, filt, pad=(1, 5), want_u8=True, want_f32=True, seed=0):
        from maskbit_amd import _lib
        self.lib = _lib.load()
        self.filt, self.n = filt, len(images)
        rng = np.random.default_rng(seed)
        self.jobs = (_lib.ImageJob * self.n)()
        at, pix, chunks = 0, 0, []
        for j, img, (res, win) in zip(self.jobs, images, geometry):
            H, W = img.shape[:2]
            stride = 3 * W + pad[1]
            at += pad[0]
            if pad[0]:
                at += 1 - at % 2                              # an odd offset
            j.src_offset, j.src_h, j.src_w, j.src_stride = at, H, W, stride
            j.res_h, j.res_w = res
            j.win_y, j.win_x, j.win_h, j.win_w = win
            j.dst_offset = pix
            pix += win[2] * win[3]
            rows = rng.integers(0, 256, (H, stride), dtype=np.uint8)
            rows[:, :3 * W] = img.reshape(H, 3 * W)
            chunks.append((at, rows.reshape(-1)[:(H - 1) * stride + 3 * W]))
            at += (H - 1) * stride + 3 * W
        host = rng.integers(0, 256, at, dtype=np.uint8)
        for off, data in chunks:
            host[off:off + len(data)] = data
        self.src = torch.from_numpy(host).to(DEV)
        self.pixels = pix
        self.work_bytes = int(self.lib.mb_image_workspace_bytes(self.jobs, self.n, filt))
        assert self.work_bytes > 0
        self.work = torch.empty(self.work_bytes, dtype=torch.uint8, device=DEV)
        self.jobs_dev = torch.from_numpy(np.frombuffer(self.jobs, dtype=np.uint8).copy()).to(DEV)
        self.u8 = torch.full((GUARD + 3 * pix + GUARD,), U8_SENTINEL, dtype=torch.uint8, device=DEV) if want_u8 else None
        self.f32 = torch.full((GUARD + 3 * pix + GUARD,), F32_SENTINEL, dtype=torch.float32, device=DEV) if want_f32 else None

    def run(self, **override):
        a = dict(jobs=self.jobs, dev=self.jobs_dev.data_ptr(), B=self.n, filt=self.filt, src=self.src.data_ptr(), src_bytes=self.src.numel(),
                 u8=self.u8.data_ptr() + GUARD if self.u8 is not None else None, f32=self.f32.data_ptr() + 4 * GUARD if self.f32 is not None else None,
                 cap=self.pixels, work=self.work.data_ptr(), work_bytes=self.work_bytes)
        a.update(override)
        return self.lib.mb_image_resample(a["jobs"], a["dev"], a["B"], a["filt"], a["src"], a["src_bytes"], a["u8"], a["f32"], a["cap"], a["work"],
                                          a["work_bytes"], stream())

    def outputs(self):
        """-> per job (uint8 [h, w, 3] or None, float32 [3, h, w] or None) after checking the guards."""
        u8 = self.u8.cpu().numpy() if self.u8 is not None else None
        f32 = self.f32.cpu().numpy() if self.f32 is not None else None
        if u8 is not None:
            assert (u8[:GUARD] == U8_SENTINEL).all() and (u8[GUARD + 3 * self.pixels:] == U8_SENTINEL).all()
        if f32 is not None:
            assert (f32[:GUARD] == F32_SENTINEL).all() and (f32[GUARD + 3 * self.pixels:] == F32_SENTINEL).all()
        outs = []
        for j in self.jobs:
            lo, n = GUARD + 3 * j.dst_offset, 3 * j.win_h * j.win_w
            outs.append((u8[lo:lo + n].reshape(j.win_h, j.win_w, 3) if u8 is not None else None,
                         f32[lo:lo + n].reshape(3, j.win_h, j.win_w) if f32 is not None else None))
        return outs

    def untouched(self):
        return all(bool((t == s).all()) for t, s in ((self.u8, U8_SENTINEL), (self.f32, F32_SENTINEL)) if t is not None)


def same_bits(f32, u8_expected):
    return np.array_equal(f32.view(np.uint32), IR.to_float_nchw(u8_expected).view(np.uint32))


# ---- coefficient tables ----------------------------------------------------------------------------------------------------------------
PAIRS = [(7, 25), (16, 32), (16, 16), (17, 16), (32, 16), (53, 23), (100, 16), (300, 16), (1, 16), (1, 1), (1500, 8)]


@pytest.mark.parametrize("pair", PAIRS, ids=lambda p: f"{p[0]}-{p[1]}")
def test_coefficient_tables(pair):
    """scale < 1, = 1, just above 1, 2, 6.25, 18.75 (27 and 77 taps: far beyond a register-resident list), 187.5, and in = 1."""
    from maskbit_amd import _lib
    lib = _lib.load()
    n_in, n_out = pair
    for filt in FILTERS:
        xmin_r, n_r, k_r = IR.identity_coeffs(n_in) if n_in == n_out else IR.coeffs(n_in, n_out, filt)
        K = k_r.shape[1]
        assert K == (1 if n_in == n_out else IR.ksize_for(n_in, n_out, filt))
        for first, count in {(0, n_out), (n_out // 2, n_out - n_out // 2), (n_out - 1, 1)}:
            xmin = torch.full((count,), -99, dtype=torch.int32, device=DEV)
            n = torch.full((count,), -99, dtype=torch.int32, device=DEV)
            k = torch.full((count + 1, K), -99, dtype=torch.int32, device=DEV)                  # one row of guard
            _lib.check(lib.mb_image_coeffs(n_in, n_out, filt, first, count, K, xmin.data_ptr(), n.data_ptr(), k.data_ptr(), stream()), "mb_image_coeffs")
            assert np.array_equal(xmin.cpu().numpy(), xmin_r[first:first + count]), (pair, filt, first)
            assert np.array_equal(n.cpu().numpy(), n_r[first:first + count]), (pair, filt, first)
            kk = k.cpu().numpy()
            bad = np.argwhere(kk[:count] != k_r[first:first + count])
            assert len(bad) == 0, (pair, IR.FILTER_NAMES[filt], first, bad[:4], kk[:count][tuple(bad[0])], k_r[first:first + count][tuple(bad[0])])
            assert (kk[count] == -99).all()


# ---- one pass, every byte and every float bit ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", IR.SIZE_CASES + EXTRA_CASES, ids=lambda c: f"{c[0][0]}x{c[0][1]}-{c[1][0]}x{c[1][1]}")
def test_single_jobs(case):
    (H, W), (h, w) = case
    for filt in FILTERS:
        for content in IR.CONTENTS:
            p = Pass([IR.make_image(H, W, content)], [((h, w), (0, 0, h, w))], filt)
            assert p.run() == 0, p.lib.mb_last_error()
            ((u8, f32),) = p.outputs()
            want = expected(H, W, h, w, content, filt)
            assert np.array_equal(u8, want), (case, IR.FILTER_NAMES[filt], content, np.argwhere(u8 != want)[:4])
            assert same_bits(f32, want), (case, IR.FILTER_NAMES[filt], content)


@pytest.mark.parametrize("filt", FILTERS, ids=lambda f: IR.FILTER_NAMES[f])
def test_ragged_batch_in_one_call(filt):
    """All sizes of the list as ONE call: odd source offsets, row strides with padding, guard bytes around sentinel-filled outputs."""
    cases = [(c, content) for c in IR.SIZE_CASES + EXTRA_CASES for content in IR.CONTENTS]
    p = Pass([IR.make_image(H, W, content) for ((H, W), _), content in cases], [((h, w), (0, 0, h, w)) for (_, (h, w)), _ in cases], filt, pad=(1, 7))
    assert all(j.src_offset % 2 == 1 for j in p.jobs) and any(j.src_stride % 4 for j in p.jobs)
    assert p.run() == 0, p.lib.mb_last_error()
    for (((H, W), (h, w)), content), (u8, f32) in zip(cases, p.outputs()):
        want = expected(H, W, h, w, content, filt)
        assert np.array_equal(u8, want), (H, W, h, w, content)
        assert same_bits(f32, want), (H, W, h, w, content)


def test_every_byte_value_becomes_torchs_float():
    """An unresized image holding all 256 values: the float output is arange(256) / 255 in float32 bit for bit (never a reciprocal multiply)."""
    img = ((np.arange(256).reshape(16, 16, 1) + np.array([0, 85, 170])) % 256).astype(np.uint8)
    p = Pass([img], [((16, 16), (0, 0, 16, 16))], IR.BILINEAR)
    assert p.run() == 0, p.lib.mb_last_error()
    ((u8, f32),) = p.outputs()
    assert np.array_equal(u8, img)
    want = torch.from_numpy(img).permute(2, 0, 1).to(torch.float32).div(255).numpy()
    assert np.array_equal(f32.view(np.uint32), want.view(np.uint32)) and len(np.unique(u8)) == 256
    assert not np.array_equal(f32, (img.transpose(2, 0, 1).astype(np.float32) * np.float32(1.0 / 255.0)))


# ---- windows ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", [((37, 53), (16, 23)), ((9, 7), (32, 25)), ((100, 67), (16, 11)), ((6, 700), (5, 600))], ids=lambda c: f"{c[0][0]}x{c[0][1]}")
def test_windows_equal_the_crop_of_the_full_result(case):
    (H, W), (h, w) = case
    img = IR.make_image(H, W, "random")
    wh, ww = max(1, h - 4), max(1, w - 5)
    origins = [(0, 0), (1, 0), (0, 1), (1, 1), (2, 3), (h - wh, w - ww), (0, w - ww), (h - wh, 0)]          # every parity; right and bottom edge
    wins = [(y, x, wh, ww) for y, x in origins] + [(h - 1, w - 1, 1, 1), (0, 0, h, 1), (0, 0, 1, w)]
    for filt in (IR.BILINEAR, IR.BICUBIC):
        full = expected(H, W, h, w, "random", filt)
        p = Pass([img] * len(wins), [((h, w), win) for win in wins], filt)
        assert p.run() == 0, p.lib.mb_last_error()
        for (y, x, a, b), (u8, f32) in zip(wins, p.outputs()):
            assert np.array_equal(u8, full[y:y + a, x:x + b]), (case, filt, (y, x, a, b))
            assert same_bits(f32, full[y:y + a, x:x + b]), (case, filt, (y, x, a, b))


# ---- the recipes end to end ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("R", [16, 32])
def test_recipes_end_to_end(R):
    from maskbit_amd import ImageTransform
    images = IR.ragged_batch()
    assert len(images) == 8
    z = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "image_transform.npz"))
    for recipe, interp in (("reference", "bilinear"), ("reference", "bicubic"), ("adm", "bicubic")):
        t = ImageTransform(R, interp, recipe)
        if recipe == "adm":
            want = [IR.adm_transform(im, R) for im in images]
            key = "recipe/adm/%d/%d"
            if R == 16:
                assert sorted({len(IR.adm_sizes(*im.shape[:2], R)[0]) for im in images}) == [0, 1, 2]      # 0, 1 and 2 halvings in one batch
        else:
            want = [IR.reference_transform(im, R, IR.FILTERS_BY_NAME[interp]) for im in images]
            key = f"recipe/reference-{interp}/%d/%d"
        for i, w in enumerate(want):
            assert np.array_equal(w, z[key % (R, i)])                                            # ... which is what Pillow gave
        mixed = [torch.from_numpy(im) if i % 2 else im for i, im in enumerate(images)]             # numpy arrays and CPU tensors
        u8, f32 = t.uint8(mixed), t(mixed)
        assert u8.shape == (8, R, R, 3) and u8.dtype == torch.uint8 and u8.is_cuda and f32.shape == (8, 3, R, R) and f32.dtype == torch.float32
        u8, f32 = u8.cpu().numpy(), f32.cpu().numpy()
        for i, w in enumerate(want):
            assert np.array_equal(u8[i], w), (recipe, interp, R, i, images[i].shape)
            assert same_bits(f32[i], w), (recipe, interp, R, i)


@pytest.mark.parametrize("interp", ["bilinear", "bicubic"])
def test_common_imagenet_shape(interp):
    """(375, 500) -> 256: resized to (256, 341), crop origin 42; several output tiles along both axes."""
    from maskbit_amd import ImageTransform
    img = IR.make_image(375, 500, "random")
    want = IR.reference_transform(img, 256, IR.FILTERS_BY_NAME[interp])
    t = ImageTransform(256, interp)
    u8, f32 = t.uint8([img]), t([img])
    assert np.array_equal(u8[0].cpu().numpy(), want) and same_bits(f32[0].cpu().numpy(), want)
    if interp == "bicubic":
        adm = ImageTransform(256, recipe="adm").uint8([img])[0].cpu().numpy()                    # no halving; floor instead of round-half-even
        assert np.array_equal(adm, IR.adm_transform(img, 256))


# ---- consumers ----------------------------------------------------------------------------------------------------------------------------
def test_transformed_feeds_eval_reconstruction():
    from maskbit_amd import ImageTransform, TokenizerEvaluator, eval_reconstruction, to_evaluator_uint8, transformed
    from test_hip_evaluator import tiny_tokenizers
    name, model, K = next(tiny_tokenizers())
    raw = [[IR.make_image(70 + 9 * i, 90 - 7 * i, "random", seed=b) for i in range(2)] for b in range(2)]
    loader = [{"image": imgs, "__key__": ["a", "b"]} for imgs in raw]
    t = ImageTransform(64, "bilinear")
    ev = TokenizerEvaluator(DEV, enable_psnr_score=True, enable_ssim_score=True, enable_mse_error=True, enable_mae_error=True,
                            enable_codebook_usage_measure=True, enable_codebook_entropy_measure=True, num_codebook_entries=K)
    through = eval_reconstruction(model, transformed(loader, t), ev)
    tensors = [t(imgs) for imgs in raw]
    for x, imgs in zip(tensors, raw):
        for b, im in enumerate(imgs):
            assert same_bits(x[b].cpu().numpy(), IR.reference_transform(im, 64, IR.BILINEAR))
    direct = eval_reconstruction(model, [{"image": x} for x in tensors], ev)
    assert list(through) == list(direct) and all(float(through[k]) == float(direct[k]) for k in through), (through, direct)
    batch = next(transformed(loader, t))
    assert batch["__key__"] == ["a", "b"] and batch["image"].shape == (2, 3, 64, 64) and isinstance(loader[0]["image"], list)      # the loader's dict is not changed
    assert to_evaluator_uint8(t.uint8(raw[0])).shape == (2, 3, 64, 64)


def test_single_outputs_and_staging_reuse():
    from maskbit_amd import ImageTransform
    img = IR.make_image(37, 53, "random")
    want = expected(37, 53, 16, 23, "random", IR.BICUBIC)
    for want_u8, want_f32 in ((True, False), (False, True)):                                     # pointer-only outputs
        p = Pass([img], [((16, 23), (0, 0, 16, 23))], IR.BICUBIC, want_u8=want_u8, want_f32=want_f32)
        assert p.run() == 0, p.lib.mb_last_error()
        ((u8, f32),) = p.outputs()
        assert (u8 is None) == (not want_u8) and (f32 is None) == (not want_f32)
        assert np.array_equal(u8, want) if want_u8 else same_bits(f32, want)
    t = ImageTransform(16, "bicubic")
    small = IR.ragged_batch()[:2]
    first = t.uint8(small).cpu().numpy()
    big = IR.ragged_batch() + [IR.make_image(300, 420, "random"), IR.make_image(1200, 900, "random")]  # the staging buffers grow
    second = t.uint8(big).cpu().numpy()
    third = t.uint8(small).cpu().numpy()
    fourth = t.uint8(big).cpu().numpy()
    assert np.array_equal(first, third) and np.array_equal(second, fourth) and np.array_equal(second[:2], first)
    for i, im in enumerate(big):
        assert np.array_equal(second[i], IR.reference_transform(im, 16, IR.BICUBIC)), i


# ---- refusals -----------------------------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_outputs_untouched():
    from maskbit_amd import _lib
    img = IR.make_image(37, 53, "random")
    p = Pass([img], [((16, 23), (0, 3, 16, 16))], IR.BILINEAR)

    def with_job(**kw):
        jobs = (_lib.ImageJob * 1)()
        C.memmove(jobs, p.jobs, C.sizeof(jobs))
        for k, v in kw.items():
            setattr(jobs[0], k, v)
        return jobs

    refused = [dict(jobs=None), dict(dev=None), dict(src=None), dict(work=None), dict(u8=None, f32=None), dict(filt=3), dict(filt=-1), dict(B=0),
               dict(jobs=with_job(src_h=0)), dict(jobs=with_job(src_w=16385)), dict(jobs=with_job(src_h=16385)), dict(jobs=with_job(win_h=0)),
               dict(jobs=with_job(win_w=0)), dict(jobs=with_job(win_x=8)), dict(jobs=with_job(src_stride=158)), dict(src_bytes=p.src.numel() - 1),
               dict(cap=p.pixels - 1), dict(work_bytes=p.work_bytes - 1), dict(jobs=with_job(kx=p.jobs[0].kx + 2)), dict(jobs=with_job(work_offset=16))]
    for i, r in enumerate(refused):
        assert p.run(**r) == -1, i
        assert p.lib.mb_last_error().decode().startswith("mb_image_resample:"), i
    torch.cuda.synchronize()
    assert p.untouched()
    assert p.run() == 0                                                                         # and the same buffers then serve a good call
    ((u8, f32),) = p.outputs()
    want = expected(37, 53, 16, 23, "random", IR.BILINEAR)[:, 3:19]
    assert np.array_equal(u8, want) and same_bits(f32, want)
