"""CPU tests of per-sample seeded sampling: the numpy restatement of the noise definition (tests/seeded_reference.py) against Random123's known
answers and for its distribution, and the host-side plumbing (header, ctypes signatures, ABI version, argument checks that need no device).

Bounds: chi-square at the 0.999 quantile of 63 degrees of freedom (103.44); Kolmogorov-Smirnov at 1.95 / sqrt(n) (the 0.001 critical value of the
one-sample statistic); correlations at 4 / sqrt(n) (four standard deviations of Pearson's r of independent samples).  The seeds are fixed, so
nothing here is flaky."""
import ctypes
import inspect
import os
import re

import numpy as np
import pytest
import torch

import seeded_reference as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHI2_999_63 = 103.44                  # chi2.ppf(0.999, 63)
SEEDS = (1, 2, 3, 12345)


def race_probabilities(C=64):
    """A fixed softmax row whose smallest expected count over 16 384 draws is >= 2 (3.8): logits spread over [-3, 3] in a fixed shuffled order."""
    logits = np.linspace(-3.0, 3.0, C)[np.random.RandomState(0).permutation(C)]
    p = np.exp(logits - logits.max())
    return p / p.sum()


def chi_square(picks, p, R):
    counts = np.bincount(picks.reshape(-1), minlength=len(p)).astype(np.float64)
    return float(((counts - R * p) ** 2 / (R * p)).sum())


# ---- the generator ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ctr,key,want", [
    ((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
    ((0xffffffff,) * 4, (0xffffffff,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
    ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1)),
])
def test_philox_known_answers(ctr, key, want):
    """Random123's kat_vectors for philox4x32 with ten rounds."""
    got = S.philox4x32_10(ctr, key)
    assert tuple(int(x) for x in got) == want


def test_uniform_is_exact_and_never_zero_or_one():
    x = np.array([0, 1, 255, 256, 0x7fffffff, 0x80000000, 0xffffff00, 0xffffffff], dtype=np.uint32)
    u = S.uniform(x)
    assert u.dtype == np.float32
    assert u.min() == np.float32(2.0 ** -24) and u.max() == np.float32(1.0 - 2.0 ** -24)
    assert np.array_equal(u.astype(np.float64) * 2.0 ** 24, ((x >> 8) | 1).astype(np.float64))     # exact: odd 24-bit integers
    assert np.all(-np.log(u.astype(np.float64)) > 0)                                                # q is never 0


def test_key_and_counter_layout():
    """Key = (low, high) dword of the seed; class c takes word c & 3 of block c >> 2; the two streams differ in the counter's last word."""
    seed = 0xfedcba9876543210
    u = S.exp_uniforms([seed], 5, 3, 10)
    blk = S.philox4x32_10((2, 1, 5, 0), (0x76543210, 0xfedcba98))
    assert u[0, 1, 9] == S.uniform(blk[1]) and u[0, 1, 8] == S.uniform(blk[0])
    cu = S.conf_uniforms([seed], 5, 3)
    assert cu[0, 2] == S.uniform(S.philox4x32_10((0, 2, 5, 1), (0x76543210, 0xfedcba98))[0])
    assert np.array_equal(S.exp_uniforms([2 ** 64 - 1, 0, 2 ** 63], 0, 2, 8)[1], S.exp_uniforms([0], 0, 2, 8)[0])   # a sample's noise: its own seed alone


# ---- the distribution ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", SEEDS)
def test_race_picks_follow_the_softmax(seed):
    """argmax p / q over R = 16 384 slots, C = 64: chi-square of the pick counts against R p below the 0.999 quantile."""
    R, p = 16384, race_probabilities()
    assert R * p.min() >= 2.0
    chi2 = chi_square(S.race_picks([seed], 0, R, p), p, R)
    print(f"seed {seed}: chi-square {chi2:.2f}")
    assert chi2 < CHI2_999_63


@pytest.mark.parametrize("seed", SEEDS)
def test_gumbel_values_follow_the_gumbel_cdf(seed):
    n = 65536
    g = np.sort(S.gumbel64(S.conf_uniforms([seed], 3, n)).reshape(-1))
    cdf = np.exp(-np.exp(-g))
    i = np.arange(1, n + 1, dtype=np.float64)
    ks = float(max((i / n - cdf).max(), (cdf - (i - 1) / n).max()))
    print(f"seed {seed}: KS {ks:.5f} (bound {1.95 / np.sqrt(n):.5f})")
    assert ks < 1.95 / np.sqrt(n)


def pearson(a, b):
    return float(np.corrcoef(a.reshape(-1).astype(np.float64), b.reshape(-1).astype(np.float64))[0, 1])


@pytest.mark.parametrize("seed", SEEDS)
def test_neighbouring_steps_seeds_and_streams_are_uncorrelated(seed):
    P, C = 1024, 64
    n = P * C
    bound = 4.0 / np.sqrt(n)
    a = S.exp_uniforms([seed], 4, P, C)
    r_step = pearson(a, S.exp_uniforms([seed], 5, P, C))
    r_seed = pearson(a, S.exp_uniforms([seed + 1], 4, P, C))
    c0 = S.conf_uniforms([seed], 4, n)
    r_stream = pearson(S.exp_uniforms([seed], 4, n, 1), c0)                     # class 0 of every slot against the slot's confidence uniform
    r_cstep = pearson(c0, S.conf_uniforms([seed], 5, n))
    print(f"seed {seed}: r step {r_step:.5f} seed {r_seed:.5f} stream {r_stream:.5f} conf step {r_cstep:.5f} (bound {bound:.5f})")
    assert max(abs(r_step), abs(r_seed), abs(r_stream), abs(r_cstep)) < bound


# ---- plumbing --------------------------------------------------------------------------------------------------------------------------------
ENTRIES = ("mb_sample_step_seeded", "mb_sample_seeded")


def test_abi_declares_and_binds_the_seeded_entries():
    from maskbit_amd import _lib
    abi = open(os.path.join(ROOT, "include", "maskbit_hip.h")).read()
    diag = open(os.path.join(ROOT, "include", "maskbit_hip_diag.h")).read()
    assert re.search(r"#define MB_ABI_VERSION 8\b", abi) and _lib.ABI_VERSION == 8               # additions only
    raw = ctypes.CDLL(_lib.LIB_PATH)
    for name in ENTRIES:
        assert re.search(r"\b%s\s*\(" % name, abi) and name in _lib.SIGNATURES
        getattr(raw, name)
    assert re.search(r"\bmb_seeded_noise\s*\(", diag) and not re.search(r"\bmb_seeded_noise\s*\(", abi) and "mb_seeded_noise" in _lib.SIGNATURES
    getattr(raw, "mb_seeded_noise")
    assert _lib.load().mb_abi_version() == 8
    assert len(_lib.SIGNATURES["mb_sample_step_seeded"][1]) == 18 and len(_lib.SIGNATURES["mb_sample_seeded"][1]) == 14
    assert len(_lib.SIGNATURES["mb_seeded_noise"][1]) == 12
    # the header states the definition the restatement was written from
    flat = re.sub(r"\s*\n \*\s*", " ", abi)                                                        # (comment lines joined)
    for text in ("0xD2511F53", "0xCD9E8D57", "0x9E3779B9", "0xBB67AE85", "(c >> 2, slot, step, 0)", "(0, slot, step, 1)", "(x >> 8) | 1", "exact confidence ties"):
        assert text in flat, text


def test_public_surface():
    import maskbit_amd
    from maskbit_amd import generate_uint8, inpaint, sample, sample_from_tokens, sample_seeded
    from maskbit_amd.parallel import sample_sharded
    assert "sample_seeded" in maskbit_amd.__all__
    p = inspect.signature(sample_seeded).parameters
    assert list(p) == ["model", "vqgan_model", "seeds", "labels", "softmax_temperature", "randomize_temperature", "mask_schedule_strategy", "num_steps",
                       "guidance_scale", "guidance_annealing", "use_sampling_annealing", "scale_pow"]
    assert all(p[k].kind is inspect.Parameter.KEYWORD_ONLY for k in list(p)[4:])
    s = inspect.signature(sample).parameters
    assert all(p[k].default == s[k].default for k in list(p)[4:])                                  # the sampling keywords of sample(), its defaults
    assert "seeds" not in s and "seed" not in s                                                    # sample() itself is untouched
    for fn, name in ((sample_from_tokens, "seeds"), (inpaint, "seeds"), (generate_uint8, "seed"), (sample_sharded, "seeds")):
        q = inspect.signature(fn).parameters[name]
        assert q.default is None and q.kind is inspect.Parameter.KEYWORD_ONLY


def test_seeds_validation_needs_no_device():
    from maskbit_amd.sampling import check_seeds
    out = check_seeds([0, 1, 2 ** 63 - 1, 2 ** 63, 2 ** 64 - 1], 5)
    assert out.dtype == torch.int64 and out.tolist() == [0, 1, 2 ** 63 - 1, -2 ** 63, -1]         # the bit patterns
    assert np.array_equal(S.seed_key(out.tolist())[0], S.seed_key([0, 1, 2 ** 63 - 1, 2 ** 63, 2 ** 64 - 1])[0])
    t = torch.tensor([5, -1], dtype=torch.int64)
    assert torch.equal(check_seeds(t, 2), t)
    assert check_seeds(range(3), 3).tolist() == [0, 1, 2] and check_seeds((7,), 1).tolist() == [7]
    for bad, n in (([1, 2], 3), ([-1], 1), ([2 ** 64], 1), ([1.0], 1), ([True], 1), (["1"], 1), (5, 1), (torch.tensor([1, 2], dtype=torch.int32), 2),
                   (torch.tensor([1.0, 2.0]), 2), (torch.tensor([[1, 2]]), 2), (torch.tensor([1, 2, 3]), 2), (None, 1)):
        with pytest.raises(ValueError):
            check_seeds(bad, n)


def test_public_entries_refuse_bad_seeds_before_any_device_work():
    """On CPU-resident models: the seeds are checked before the device is asked for (which would raise RuntimeError)."""
    from maskbit_amd import ConvVQModel, LFQBert, sample_seeded, sample_from_tokens
    from hip_helpers import tok_config
    from test_edit_cpu import TINY_GEN, TINY_TOK
    gm = LFQBert(img_size=256, hidden_dim=TINY_GEN.hidden, codebook_size=2 ** TINY_GEN.bits, codebook_splits=TINY_GEN.splits, depth=TINY_GEN.depth,
                 heads=TINY_GEN.heads, mlp_dim=TINY_GEN.mlp, dropout=0.1, nclass=TINY_GEN.nclass, input_stride=16)
    tm = ConvVQModel(tok_config(TINY_TOK))
    y = torch.tensor([1, 2, 3])
    for bad in ([1, 2], [1, 2, -3], [1, 2, 2 ** 64], torch.tensor([1, 2, 3], dtype=torch.int32), [1, 2, 3.5]):
        with pytest.raises(ValueError):
            sample_seeded(gm, tm, bad, y)
        with pytest.raises(ValueError):
            sample_from_tokens(gm, tm, torch.full((3, 256, 2), 64, dtype=torch.int64), y, seeds=bad)
    with pytest.raises(TypeError):
        sample_seeded(gm, tm, [1, 2, 3], [1, 2, 3])
    from maskbit_amd.parallel import sample_sharded
    with pytest.raises(ValueError, match="go together"):
        sample_sharded(gm, tm, y, noise="seeded")
    with pytest.raises(ValueError, match="go together"):
        sample_sharded(gm, tm, y, noise="rank", seeds=[1, 2, 3])
    with pytest.raises(ValueError):
        sample_sharded(gm, tm, y, noise="seeded", seeds=[1, 2])


def test_c_entries_refuse_bad_arguments_without_a_gpu():
    """The checks in front of every launch: null pointers, aliasing, sizes (no device is touched before they pass)."""
    from maskbit_amd import _lib
    lib = _lib.load()
    buf = (ctypes.c_int64 * 64)()
    a = ctypes.addressof(buf)
    b = a + 128

    def refused(rc, text):
        assert rc < 0 and text in lib.mb_last_error().decode(), (rc, lib.mb_last_error())

    step = lambda **kw: lib.mb_sample_step_seeded(*[kw.get(k, d) for k, d in (
        ("lc", a), ("lu", None), ("scale", 0.0), ("temp", 1.0), ("seeds", a), ("step", 0), ("rt", 1.0), ("w", 1.0), ("ratio", 0.5), ("num_regen", a),
        ("tin", a), ("tout", b), ("pred", None), ("B", 1), ("n", 2), ("m", 1), ("C", 4), ("stream", None))])
    refused(step(seeds=None), "null argument")
    refused(step(num_regen=None), "null argument")
    refused(step(lc=None), "null argument")
    refused(step(tin=None), "null argument")
    refused(step(tout=a), "must not alias")
    refused(step(pred=b), "pred_out must not alias")
    refused(step(step=-1), "negative")
    refused(step(B=0), "bad sizes")
    refused(step(C=8192), "too large")
    refused(step(n=8193), "too large")
    noise = lambda **kw: lib.mb_seeded_noise(*[kw.get(k, d) for k, d in (
        ("seeds", a), ("step", 0), ("rt", 1.0), ("w", 1.0), ("eu", None), ("e", a), ("cu", None), ("c", b), ("B", 1), ("P", 2), ("C", 4), ("stream", None))])
    refused(noise(seeds=None), "null argument")
    refused(noise(e=None), "null argument")
    refused(noise(c=None), "null argument")
    refused(noise(eu=a), "must not alias")
    refused(noise(step=-1), "bad sizes")
    refused(noise(B=0), "bad sizes")
    refused(noise(C=4097), "too large")
    refused(noise(P=8193), "too large")
    plan = _lib.EditPlan(2, 0, (ctypes.c_float * 2)(), (ctypes.c_float * 2)(1, 1), (ctypes.c_float * 2)(0.5, 0.0), 0, 0)
    w = (ctypes.c_float * 2)(0.5, 0.0)
    run = lambda **kw: lib.mb_sample_seeded(*[kw.get(k, d) for k, d in (
        ("g", None), ("d", None), ("plan", ctypes.byref(plan)), ("labels", a), ("B", 1), ("init", None), ("seeds", a), ("rt", 1.0), ("w", w),
        ("steps", None), ("codes", None), ("img", None), ("u8", None), ("stream", None))])
    refused(run(), "null argument")                                                                # no generator handle
    refused(run(plan=None), "null argument")
    refused(run(seeds=None), "null argument")
    refused(run(w=None), "null argument")
    plan.mask_ratio = None
    refused(run(), "incomplete plan")
