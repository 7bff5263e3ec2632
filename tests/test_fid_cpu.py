"""CPU checks of the generator evaluator: the C ABI additions, the constructor and its refusals, the checks that raise before any device work,
and the closed forms -- ``frechet_distance`` / ``inception_score`` / ``get_covariance`` and the float64 restatement of tests/fid_reference.py --
against the reference's recorded results (tests/golden/generator_evaluator.npz, tools/make_golden_generator_evaluator.py).

Bounds: |FID - FID_hp| <= max(2 E_ref, D 2^-52 (tr S_r + tr S_f)) and |IS - IS_hp| <= max(2 E_ref, C 2^-50 IS_hp), where *_hp is the 40-digit
evaluation of the reference's own statistics and E_ref = |ref - hp| the reference's own evaluation error, both recorded in the golden."""
import ctypes
import inspect
import os

import numpy as np
import pytest
import torch

import fid_reference as R
from conftest import ROOT


def accumulate64(feats, logits, splits):
    D, C = feats.shape[1], logits.shape[1]
    total, sigma = torch.zeros(D, dtype=torch.float64), torch.zeros(D, D, dtype=torch.float64)
    pt, kl = torch.zeros(C, dtype=torch.float64), torch.zeros(C, dtype=torch.float64)
    for a, b in splits:
        total, sigma, _, _ = R.fid_update64(total, sigma, feats[a:b])
        pt, kl, _, _ = R.is_update64(pt, kl, logits[a:b])
    return total, sigma, pt, kl


# ---- ABI ------------------------------------------------------------------------------------------------------------------------------------
def test_abi_exports_fid_entries():
    from maskbit_amd import _lib, build
    import maskbit_amd
    lib = ctypes.CDLL(_lib.LIB_PATH)
    header = open(os.path.join(ROOT, "include", "maskbit_hip.h")).read()
    for name in ("mb_fid_accumulate", "mb_is_workspace_bytes", "mb_is_accumulate"):
        assert name in _lib.SIGNATURES and name + "(" in header
        getattr(lib, name)
    assert "#define MB_ABI_VERSION 8" in header
    assert _lib.load().mb_abi_version() == 8 == _lib.ABI_VERSION
    assert "fid.hip" in build.SOURCES and os.path.exists(os.path.join(build.CSRC, "fid.hip"))
    for name in ("GeneratorEvaluator", "eval_generation", "frechet_distance", "inception_score", "get_covariance"):
        assert name in maskbit_amd.__all__ and hasattr(maskbit_amd, name)
    from maskbit_amd.evaluator import GeneratorEvaluator
    assert GeneratorEvaluator is maskbit_amd.GeneratorEvaluator
    ws = _lib.load().mb_is_workspace_bytes
    assert ws(64, 1008) == 64 * 2 * 8 and ws(1, 1) == 16
    assert ws(0, 1008) == 0 and ws(64, 0) == 0 and ws(-1, 5) == 0


def test_entries_refuse_bad_arguments_without_a_device():
    """Every refusal is decided on the host before a launch: null pointers, dtype codes, shapes, strides, alignment -> an error code and a
    message through mb_last_error."""
    from maskbit_amd import _lib
    lib = _lib.load()
    p = 4096                                                  # never dereferenced: each call below is refused first
    bad = [
        lambda: lib.mb_fid_accumulate(None, 1, 4, 4, 4, p, p, None),
        lambda: lib.mb_fid_accumulate(p, 2, 4, 4, 4, p, p, None),
        lambda: lib.mb_fid_accumulate(p, 1, 0, 4, 4, p, p, None),
        lambda: lib.mb_fid_accumulate(p, 1, 4, 0, 4, p, p, None),
        lambda: lib.mb_fid_accumulate(p, 1, 4, 8, 7, p, p, None),
        lambda: lib.mb_fid_accumulate(p, 1, 4, (1 << 20) + 1, 1 << 21, p, p, None),
        lambda: lib.mb_fid_accumulate(p + 4, 1, 4, 4, 4, p, p, None),
        lambda: lib.mb_is_accumulate(p, 0, 4, 4, 4, p, p, None, None),
        lambda: lib.mb_is_accumulate(p, 0, 4, 4, 3, p, p, p, None),
        lambda: lib.mb_is_accumulate(p, -1, 4, 4, 4, p, p, p, None),
        lambda: lib.mb_is_accumulate(p, 0, -4, 4, 4, p, p, p, None),
        lambda: lib.mb_is_accumulate(p, 0, 4, 4, 4, p, p + 2, p, None),
    ]
    for call in bad:
        assert call() == -1
        assert lib.mb_last_error().decode().startswith(("mb_fid_accumulate:", "mb_is_accumulate:"))


# ---- the class surface ---------------------------------------------------------------------------------------------------------------------
def test_constructor_keywords_are_the_references():
    from maskbit_amd import GeneratorEvaluator, eval_generation, generate_uint8
    p = inspect.signature(GeneratorEvaluator.__init__).parameters
    assert list(p) == ["self", "device", "enable_fid", "enable_inception_score", "enable_codebook_usage_measure",
                       "enable_codebook_entropy_measure", "test_resolution", "num_codebook_entries"]                   # evaluator.py:470-478
    assert all(p[k].default is False for k in list(p)[2:6]) and p["test_resolution"].default == 256 and p["num_codebook_entries"].default == 1024
    assert list(inspect.signature(GeneratorEvaluator.update).parameters) == ["self", "generated_images", "codebook_indices"]
    assert list(inspect.signature(GeneratorEvaluator.update_uint8).parameters) == ["self", "u8_nchw", "codebook_indices"]
    assert list(inspect.signature(GeneratorEvaluator.update_features).parameters) == ["self", "pool", "logits", "codebook_indices"]
    assert list(inspect.signature(GeneratorEvaluator.use_inception).parameters) == ["self", "extractor", "real_statistics"]
    e = inspect.signature(eval_generation).parameters
    assert list(e)[:6] == ["model", "vqgan_model", "evaluator", "num_samples", "batchsize", "labels"] and e["labels"].default is None
    g = inspect.signature(generate_uint8).parameters
    sampling = [k for k in g if k not in ("model", "vqgan_model", "labels", "batchsize", "total_samples", "return_codes")]
    assert list(e)[6:] == sampling and all(e[k].default == g[k].default for k in sampling)


def test_constructor_refusals():
    from maskbit_amd import GeneratorEvaluator, TokenizerEvaluator
    with pytest.raises(RuntimeError, match="no CPU path"):
        GeneratorEvaluator("cpu", enable_fid=True)
    with pytest.raises(RuntimeError, match="no CPU path"):
        GeneratorEvaluator(torch.device("cpu"))
    with pytest.raises(ValueError, match="256 or 512"):
        GeneratorEvaluator("cuda:0", test_resolution=128)
    with pytest.raises(ValueError):
        GeneratorEvaluator("cuda:0", enable_codebook_usage_measure=True, num_codebook_entries=0)
    for kw in ("enable_rfid", "enable_inception_score"):                       # the tokenizer's flags keep meaning "fetch the network"
        with pytest.raises(NotImplementedError, match="reference's own evaluator"):
            TokenizerEvaluator("cuda:0", **{kw: True})
    assert callable(TokenizerEvaluator.use_inception)


def test_checks_raise_before_any_device_work(tmp_path):
    """A CUDA device that is never touched: construction allocates nothing, and every refusal comes before the first kernel or allocation (this
    test runs on a machine without a GPU)."""
    from maskbit_amd import GeneratorEvaluator
    ev = GeneratorEvaluator("cuda:0", enable_fid=True, enable_inception_score=True, enable_codebook_usage_measure=True)
    ev.reset_metrics()
    with pytest.raises(ValueError, match="No examples"):
        ev.result()
    images, u8 = torch.rand(2, 3, 8, 8), torch.zeros(2, 3, 8, 8, dtype=torch.uint8)
    with pytest.raises(RuntimeError, match="use_inception"):
        ev.update(images, torch.zeros(2, 4, dtype=torch.int64))
    with pytest.raises(RuntimeError, match="use_inception"):
        ev.update_uint8(u8, torch.zeros(2, 4, dtype=torch.int64))
    with pytest.raises(TypeError):
        ev.use_inception("inception")
    with pytest.raises(ValueError, match="does not exist"):
        ev.use_inception(None, str(tmp_path / "missing.npz"))
    np.savez(tmp_path / "nomu.npz", sigma=np.eye(4))
    with pytest.raises(ValueError, match='"mu"'):
        ev.use_inception(None, str(tmp_path / "nomu.npz"))
    with pytest.raises(ValueError, match="sigma"):
        ev.use_inception(None, (torch.zeros(4), torch.zeros(3, 3)))
    np.savez(tmp_path / "stats.npz", mu=np.arange(4.0), sigma=np.eye(4))
    called = []
    ev.use_inception(lambda x: called.append(x) or {"2048": torch.rand(2, 4)}, str(tmp_path / "stats.npz"))
    assert torch.equal(ev._fid_real_mu, torch.arange(4.0, dtype=torch.float64)) and ev._fid_real_sigma.dtype == torch.float64
    with pytest.raises(ValueError, match="codebook_indices is required"):
        ev.update_uint8(u8)
    with pytest.raises(ValueError, match="integer"):
        ev.update_uint8(u8, torch.zeros(2, 4))
    assert not called
    with pytest.raises(ValueError, match="logits_unbiased"):                  # the extractor's contract
        ev.update_uint8(u8, torch.zeros(2, 4, dtype=torch.int64))
    with pytest.raises(ValueError, match="uint8"):
        ev.update_uint8(images)
    idx = torch.zeros(2, 4, dtype=torch.int64)
    pool, logits = torch.rand(2, 4, dtype=torch.float64), torch.rand(2, 6)
    for args, msg in (((None, logits, idx), "pool"), ((pool, None, idx), "logits"), ((pool, logits[:1], idx), "batch of 2"),
                      ((pool.reshape(-1), logits, idx), "needs pool"), ((pool.long(), logits, idx), "floating-point"),
                      ((torch.rand(2, 5), logits, idx), "real statistics"), ((pool, logits, None), "codebook_indices is required"),
                      ((pool[:0], logits[:0], idx), "empty")):
        with pytest.raises(ValueError, match=msg):
            ev.update_features(*args)
    assert ev._num_examples == 0 and ev._fid is None and ev._hist is None      # nothing was counted, bound or allocated
    with pytest.raises(ValueError, match="no FID statistics"):
        ev.fid_statistics()
    # FID without real statistics: result() says so (checked on a state that needs no device: the counter alone)
    ev2 = GeneratorEvaluator("cuda:0", enable_fid=True)
    ev2._num_examples = 3
    with pytest.raises(RuntimeError, match="real statistics"):
        ev2.result()


def test_tokenizer_use_inception_argument_checks():
    from maskbit_amd import TokenizerEvaluator
    assert list(inspect.signature(TokenizerEvaluator.use_inception).parameters) == ["self", "extractor", "rfid", "inception_score"]
    ev = object.__new__(TokenizerEvaluator)                                    # the constructor allocates on the device; the checks do not need it
    ev._is_stats = ev._rfid_real = ev._rfid_fake = object()
    with pytest.raises(TypeError):
        TokenizerEvaluator.use_inception(ev, 3)
    with pytest.raises(ValueError, match="rfid or inception_score"):
        TokenizerEvaluator.use_inception(ev, len, rfid=False, inception_score=False)
    TokenizerEvaluator.use_inception(ev, len, rfid=False)
    assert ev._inception is len and not ev._rfid and ev._inception_score
    TokenizerEvaluator.use_inception(ev, None)
    assert ev._inception is None and not ev._inception_score


# ---- the closed forms against the reference -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", R.feature_cases())
def test_closed_forms_reproduce_the_reference(name):
    from maskbit_amd import frechet_distance, get_covariance, inception_score
    z, c = R.golden(), R.feature_case(name)
    N = c["N"]
    total, sigma, pt, kl = accumulate64(c["fake"], c["logits"], c["splits"])
    cov = get_covariance(sigma, total, N)
    assert torch.equal(cov, R.covariance64(sigma, total, N))
    fid_hp, is_hp = float(z[name + ".FID_hp"]), float(z[name + ".IS_hp"])
    fid, fid64 = frechet_distance(c["mu"], c["sigma"], total / N, cov), R.frechet64(c["mu"], c["sigma"], total / N, cov)
    score, score64 = inception_score(pt, kl, N), R.score64(pt, kl, N)
    print(f"{name}: FID {fid:.12g} |FID - hp| {abs(fid - fid_hp):.3g} (restatement {abs(fid64 - fid_hp):.3g}), E_ref "
          f"{abs(float(z[name + '.FID_ref']) - fid_hp):.3g}, bound {R.fid_bound(name):.3g}; IS {score:.12g} |IS - hp| {abs(score - is_hp):.3g}, "
          f"bound {R.is_bound(name):.3g}")
    assert isinstance(fid, float) and isinstance(score, float)
    assert abs(fid - fid_hp) <= R.fid_bound(name) and abs(fid64 - fid_hp) <= R.fid_bound(name)
    assert abs(score - is_hp) <= R.is_bound(name) and abs(score64 - is_hp) <= R.is_bound(name)
    # the reference itself sits inside the bound it defines, and the distance is not trivial
    assert abs(float(z[name + ".FID_ref"]) - fid_hp) <= R.fid_bound(name) and fid_hp > 0.1
    assert 1.5 < is_hp < 0.9 * c["C"]


@pytest.mark.parametrize("name", [n for n in R.feature_cases() if n + ".rFID_hp" in R.golden()])
def test_rfid_closed_form_reproduces_the_reference(name):
    from maskbit_amd import frechet_distance, get_covariance, inception_score
    z, c = R.golden(), R.feature_case(name)
    N = c["N"]
    t_f, s_f, pt, kl = accumulate64(c["fake"], c["logits"], c["splits"])
    t_r, s_r, _, _ = accumulate64(c["real"], c["logits"], c["splits"])
    rfid = frechet_distance(t_r / N, get_covariance(s_r, t_r, N), t_f / N, get_covariance(s_f, t_f, N))
    hp = float(z[name + ".rFID_hp"])
    print(f"{name}: rFID {rfid:.12g} |rFID - hp| {abs(rfid - hp):.3g}, E_ref {abs(float(z[name + '.rFID_ref']) - hp):.3g}, "
          f"bound {R.fid_bound(name, 'rFID'):.3g}")
    assert abs(rfid - hp) <= R.fid_bound(name, "rFID")
    assert abs(inception_score(pt, kl, N) - float(z[name + ".IS_hp"])) <= R.is_bound(name, "tIS_ref")


@pytest.mark.parametrize("name", R.index_cases())
def test_codebook_restatement_reproduces_the_reference(name):
    z = R.golden()
    usage, entropy = R.codebook64(*R.index_case(name))
    assert usage == float(z[name + ".usage"]) and abs(entropy - float(z[name + ".entropy"])) <= 1e-12


def test_frechet_distance_properties():
    from maskbit_amd import frechet_distance, get_covariance
    c = R.feature_case("full32")
    mu, s = c["mu"], c["sigma"]
    assert abs(frechet_distance(mu, s, mu, s)) <= 32 * 2.0 ** -52 * 2 * float(torch.trace(s)) * 4            # d(P, P) = 0 up to the eigensolver
    x = torch.arange(4.0, dtype=torch.float64)
    d, e = torch.diag(x + 1), torch.diag(2 * x + 3)                                                           # commuting: closed form
    want = float((torch.ones(4) * 0.5).double().pow(2).sum() + ((x + 1).sqrt() - (2 * x + 3).sqrt()).pow(2).sum())
    assert abs(frechet_distance(x, d, x + 0.5, e) - want) <= 1e-13
    assert abs(frechet_distance(x.numpy(), d.numpy(), (x + 0.5).float(), e) - want) <= 1e-13                  # arrays and fp32 are widened
    with pytest.raises(ValueError):
        frechet_distance(x, d, x[:3], e)
    assert torch.equal(get_covariance(d, x, 0), torch.zeros_like(d))                                          # evaluator.py:95-96


def test_golden_covers_the_issue_cases():
    z = R.golden()
    shape = {n: tuple(int(v) for v in z[n + ".params"][:3]) for n in R.feature_cases()}
    full = {d for d, _, n in shape.values() if n >= 3 * d}
    singular = {d for d, _, n in shape.values() if n < d}
    assert {32, 64} <= full and {32, 64} <= singular
    assert any(d == 256 and c == 1008 for d, c, _ in shape.values())
    assert {int(z[n + ".K"]) for n in R.index_cases()} == {1024, 4096, 65536}
    for n, (d, _, _) in shape.items():
        assert (n + ".mu" in z) == (d <= 64)
    assert os.path.getsize(os.path.join(ROOT, "tests", "golden", "generator_evaluator.npz")) < 512 * 1024
