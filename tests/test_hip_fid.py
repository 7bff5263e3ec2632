"""GPU checks of csrc/fid.hip (mb_fid_accumulate, mb_is_accumulate), maskbit_amd.GeneratorEvaluator, TokenizerEvaluator.use_inception and
harness.eval_generation, against the float64 restatement of tests/fid_reference.py and the reference's recorded results
(tests/golden/generator_evaluator.npz).

Bounds (none of them comes from the code under test):
  sigma, total   per element |hip - fp64| <= 2 N 2^-53 sum_n |f_ni f_nj| (sum_n |f_ni| for total), N = all rows accumulated so far: a chain of N
                 fp64 multiply-adds is off by at most N 2^-53 times the sum of the magnitudes, and so is the restatement's own matmul.
  prob / kl      per column |hip - fp64| <= 4 (C + 16) 2^-53 sum_n |term|: a row sum of C exponentials may carry C 2^-53 into every p; exp, log,
                 the division and the product a few units each (both sides round the row sum once, see test_is_accumulate).
  FID, rFID      |hip - hp| <= max(2 E_ref, D 2^-52 (tr S_r + tr S_f)); InceptionScore |hip - hp| <= max(2 E_ref, C 2^-50 IS_hp): hp is the
                 40-digit evaluation of the reference's own statistics, E_ref = |ref - hp| the reference's own error (tests/test_fid_cpu.py).
  Codebook       usage exact, entropy 1e-12, as for the tokenizer evaluator.
  Bit identity   repeated runs, batch splits at multiples of 4 rows, the three update entries, eval_generation against generate_uint8: torch.equal.
Measured distances per golden case: profiles/generator_evaluator.md.
"""
import numpy as np
import pytest
import torch

import fid_reference as R
from maskbit_amd.synth import make_eval_features, make_eval_statistics

pytestmark = pytest.mark.gpu
DEV = "cuda"
B_LIST = (1, 3, 4, 5, 64, 67)
EPS = R.EPS64


def stream():
    return torch.cuda.current_stream().cuda_stream


def fid_accumulate(feats, total, sigma):
    """mb_fid_accumulate on device tensors: feats [B, D] fp32 / fp64 with unit column stride and any row stride."""
    from maskbit_amd import _lib
    B, D = feats.shape
    assert feats.stride(1) == 1 or D == 1
    _lib.check(_lib.load().mb_fid_accumulate(feats.data_ptr(), 1 if feats.dtype == torch.float64 else 0, B, D, feats.stride(0) if B > 1 else D,
                                             total.data_ptr(), sigma.data_ptr(), stream()), "mb_fid_accumulate")


def is_accumulate(logits, sums):
    from maskbit_amd import _lib
    lib = _lib.load()
    B, C = logits.shape
    ws = torch.empty(lib.mb_is_workspace_bytes(B, C) // 8, dtype=torch.float64, device=DEV)
    _lib.check(lib.mb_is_accumulate(logits.data_ptr(), 1 if logits.dtype == torch.float64 else 0, B, C, logits.stride(0) if B > 1 else C,
                                    sums[0].data_ptr(), sums[1].data_ptr(), ws.data_ptr(), stream()), "mb_is_accumulate")


def zeros_state(D):
    return torch.zeros(D, dtype=torch.float64, device=DEV), torch.zeros(D, D, dtype=torch.float64, device=DEV)


def mirrored(sigma):
    return torch.triu(sigma) + torch.triu(sigma, 1).T


def check_fid_state(total, sigma, batches, what):
    """The device state after ``batches`` (CPU tensors, in order, from a zero state) against the restatement, inside the derived bound."""
    D = batches[0].shape[1]
    t64, s64 = torch.zeros(D, dtype=torch.float64), torch.zeros(D, D, dtype=torch.float64)
    at, as_ = torch.zeros_like(t64), torch.zeros_like(s64)
    for f in batches:
        t64, s64, a, b = R.fid_update64(t64, s64, f)
        at, as_ = at + a, as_ + b
    N = sum(f.shape[0] for f in batches)
    dt, ds = (total.cpu() - t64).abs(), (mirrored(sigma).cpu() - s64).abs()
    bt, bs = 2 * N * EPS * at, 2 * N * EPS * as_
    print(f"{what}: total worst {float((dt / bt.clamp_min(1e-300)).max()):.3f} x bound, sigma worst {float((ds / bs.clamp_min(1e-300)).max()):.3f} x bound")
    assert bool((dt <= bt).all()) and bool((ds <= bs).all()), what


def features(D, B, seed, dtype=torch.float64):
    return make_eval_features(D, 1, B, seed)[0].to(dtype)


# ---- mb_fid_accumulate ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("D", [1, 15, 16, 17, 64, 100])
def test_fid_accumulate_shapes(D):
    for B in B_LIST:
        for dtype in (torch.float64, torch.float32):
            f = features(D, B, 100 * D + B, dtype)
            total, sigma = zeros_state(D)
            fid_accumulate(f.to(DEV), total, sigma)
            check_fid_state(total, sigma, [f], f"D {D} B {B} {dtype}")


def test_fid_accumulate_production_shape():
    D, B = 2048, 5
    f = features(D, B, 77)
    total, sigma = zeros_state(D)
    fid_accumulate(f.to(DEV), total, sigma)
    check_fid_state(total, sigma, [f], "D 2048 B 5")
    i = torch.arange(D, device=DEV)
    below = (i[:, None] // 64) > (i[None, :] // 64)
    assert bool((sigma[below] == 0).all())                                     # the blocks below the diagonal are never written


def test_fid_accumulate_strided_rows_and_carried_state():
    D = 100
    parts = [features(D, B, 500 + B, dt) for B, dt in ((67, torch.float64), (5, torch.float32), (64, torch.float64))]
    total, sigma = zeros_state(D)
    for k, f in enumerate(parts):
        wide = torch.full((f.shape[0], D + 2 * k + 3), float("nan"), dtype=f.dtype, device=DEV)     # rows with a gap the kernel must not read
        wide[:, :D] = f.to(DEV)
        view = wide[:, :D]
        assert not view.is_contiguous()
        fid_accumulate(view, total, sigma)
        check_fid_state(total, sigma, parts[:k + 1], f"after update {k + 1}")


def test_fid_accumulate_is_bitwise_reproducible_and_split_invariant():
    D = 100
    f = features(D, 64, 901).to(DEV)
    start_t, start_s = features(1, D, 902).reshape(D).to(DEV), mirrored(features(D, D, 903).to(DEV))   # a state that is not zero
    runs = []
    for cuts in ((0, 64), (0, 64), (0, 32, 64), (0, 16, 32, 48, 64), (0, 4, 64), (0, 60, 64)):
        total, sigma = start_t.clone(), start_s.clone()
        for a, b in zip(cuts[:-1], cuts[1:]):
            fid_accumulate(f[a:b], total, sigma)
        runs.append((total, sigma))
    for total, sigma in runs[1:]:
        assert torch.equal(total, runs[0][0]) and torch.equal(sigma, runs[0][1])
    f32 = f.float()                                                            # fp32 input is widened exactly: the same bits as its fp64 copy
    a, b = zeros_state(D), zeros_state(D)
    fid_accumulate(f32, *a)
    fid_accumulate(f32.double(), *b)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])


def test_entries_refuse_bad_shapes_on_the_device():
    from maskbit_amd import _lib
    lib = _lib.load()
    total, sigma = zeros_state(8)
    f = torch.zeros(4, 8, dtype=torch.float64, device=DEV)
    for args in ((1, 0, 8, 8), (1, 4, 0, 8), (1, 4, 8, 7), (3, 4, 8, 8)):
        assert lib.mb_fid_accumulate(f.data_ptr(), *args, total.data_ptr(), sigma.data_ptr(), stream()) == -1
        assert lib.mb_last_error().decode().startswith("mb_fid_accumulate:")
    assert lib.mb_is_accumulate(f.data_ptr(), 1, 4, 8, 8, total.data_ptr(), total.data_ptr(), None, stream()) == -1
    torch.cuda.synchronize()
    assert float(sigma.abs().sum()) == 0.0


# ---- mb_is_accumulate -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("scale", [1.0, 50.0])
@pytest.mark.parametrize("C", [1, 47, 48, 1008])
def test_is_accumulate(C, scale):
    """C x scale x every B of B_LIST x fp64 / fp32 logits (``make_eval_features``'s, times ``scale``) against the restatement, per column inside
    4 (C + 16) 2^-53 sum_n |term|.  Times 50 the rows are nearly one-hot: most probabilities lie below 1e-16 and the largest just below 1, where
    log(u) = -(1 - u) hands one unit in the last place of the row sum on to the term as 2^-52 ABSOLUTE.  Kernel and restatement therefore both
    round the row sum once (a (hi, lo) pair through the reduction; ``math.fsum``).  Measured on the MI355X: at most 0.016 x the bound at every C
    and scale.  With plain sums on both sides -- a shuffle tree in the kernel, ``torch.softmax`` in the restatement -- 6 of the 12 672 kl columns
    at scale 50 differed by 2.2e-16 where the whole column was one such term of 2e-3 down to 3e-12 (profiles/generator_evaluator.md)."""
    worst, outside = 0.0, []
    for B in B_LIST:
        for dtype in (torch.float64, torch.float32):
            x = (scale * make_eval_features(1, C, B, 7000 + C + B)[1]).to(dtype)
            sums = torch.zeros(2, C, dtype=torch.float64, device=DEV)
            is_accumulate(x.to(DEV), sums)
            again = torch.zeros_like(sums)
            is_accumulate(x.to(DEV), again)
            assert torch.equal(sums, again)
            zero = torch.zeros(C, dtype=torch.float64)
            pt, kl, ap, akl = R.is_update64(zero, zero, x)
            for got, want, mag, what in ((sums[0].cpu(), pt, ap, "prob"), (sums[1].cpu(), kl, akl, "kl")):
                bound = 4 * (C + 16) * EPS * mag
                ratio = (got - want).abs() / bound.clamp_min(1e-300)
                worst = max(worst, float(ratio.max()))
                if not bool(((got - want).abs() <= bound).all()):
                    col = int(ratio.argmax())
                    outside.append(f"{what} B {B} {dtype} column {col}: |delta| {float((got - want).abs()[col]):.3g} = {float(ratio[col]):.2f} x bound, "
                                   f"column sum {float(want[col]):.6g}, largest p of the column {float(R.softmax64(x)[:, col].max()):.12g}")
            if scale > 1 and C > 1:
                assert float(R.softmax64(x).min()) < 1e-16     # the + 1e-16 decides these terms
    print(f"C {C} scale {scale}: worst {worst:.3f} x bound")
    for line in outside:
        print("OUTSIDE", line)
    assert not outside, outside


def test_is_accumulate_strided_rows_and_carried_state():
    C = 47
    parts = [make_eval_features(1, C, B, 7100 + B)[1] for B in (5, 64, 3)]
    sums = torch.zeros(2, C, dtype=torch.float64, device=DEV)
    pt, kl = torch.zeros(C, dtype=torch.float64), torch.zeros(C, dtype=torch.float64)
    ap, akl = torch.zeros_like(pt), torch.zeros_like(pt)
    for x in parts:
        wide = torch.full((x.shape[0], C + 9), float("nan"), dtype=torch.float64, device=DEV)
        wide[:, :C] = x.to(DEV)
        is_accumulate(wide[:, :C], sums)
        pt, kl, a, b = R.is_update64(pt, kl, x)
        ap, akl = ap + a, akl + b
    assert bool(((sums[0].cpu() - pt).abs() <= 4 * (C + 16) * EPS * ap).all())
    assert bool(((sums[1].cpu() - kl).abs() <= 4 * (C + 16) * EPS * akl).all())


# ---- GeneratorEvaluator -----------------------------------------------------------------------------------------------------------------------
def generator_evaluator(K=1024, **kw):
    from maskbit_amd import GeneratorEvaluator
    if not kw:
        kw = dict(enable_fid=True, enable_inception_score=True)
    return GeneratorEvaluator(DEV, num_codebook_entries=K, **kw)


@pytest.mark.parametrize("name", R.feature_cases())
def test_generator_evaluator_vs_reference(name):
    z, c = R.golden(), R.feature_case(name)
    ev = generator_evaluator()
    ev.use_inception(R.Handout(((c["fake"][a:b], c["logits"][a:b]) for a, b in c["splits"]), DEV), (c["mu"], c["sigma"]))
    for a, b in c["splits"]:
        ev.update(R.tiny_images(b - a, a).to(DEV))
    r = ev.result()
    assert list(r) == ["InceptionScore", "FID"] and all(isinstance(v, float) for v in r.values())
    d_fid, d_is = abs(r["FID"] - float(z[name + ".FID_hp"])), abs(r["InceptionScore"] - float(z[name + ".IS_hp"]))
    print(f"{name}: FID {r['FID']:.12g} |hip - hp| {d_fid:.3g} bound {R.fid_bound(name):.3g} (E_ref {abs(float(z[name + '.FID_ref']) - float(z[name + '.FID_hp'])):.3g}); "
          f"IS {r['InceptionScore']:.12g} |hip - hp| {d_is:.3g} bound {R.is_bound(name):.3g}")
    assert d_fid <= R.fid_bound(name)
    assert d_is <= R.is_bound(name)
    n, total, sigma = ev.fid_statistics()
    assert n == c["N"] and total.dtype == sigma.dtype == torch.float64 and sigma.is_cuda
    assert torch.equal(sigma, sigma.T)                                         # exactly symmetric
    check_fid_state(total, sigma, [c["fake"][a:b] for a, b in c["splits"]], name)


@pytest.mark.parametrize("name", R.index_cases())
def test_generator_evaluator_codebook_vs_reference(name):
    z = R.golden()
    K, ups = R.index_case(name)
    ev = generator_evaluator(K, enable_codebook_usage_measure=True, enable_codebook_entropy_measure=True)
    for idx in ups:
        ev.update(R.tiny_images(1, 0).to(DEV), idx.to(DEV))                    # no network metric: no extractor needed
    r = ev.result()
    assert list(r) == ["CodebookUsage", "CodebookEntropy"]
    assert isinstance(r["CodebookUsage"], float) and r["CodebookUsage"] == float(z[name + ".usage"])
    ent = r["CodebookEntropy"]
    assert isinstance(ent, torch.Tensor) and ent.dim() == 0 and ent.dtype == torch.float64 and ent.is_cuda
    assert abs(float(ent) - float(z[name + ".entropy"])) <= 1e-12


@pytest.mark.parametrize("name", [n for n in R.feature_cases() if n + ".rFID_hp" in R.golden()])
def test_tokenizer_evaluator_rfid_vs_reference(name):
    from maskbit_amd import TokenizerEvaluator
    z, c = R.golden(), R.feature_case(name)
    ev = TokenizerEvaluator(DEV, enable_mae_error=True)
    ev.use_inception(R.Handout((x for a, b in c["splits"] for x in ((c["fake"][a:b], c["logits"][a:b]), (c["real"][a:b], c["logits"][a:b]))), DEV))
    for a, b in c["splits"]:
        img = R.tiny_images(b - a, a).to(DEV)
        ev.update(img, img)
    r = ev.result()
    assert list(r) == ["MAE", "InceptionScore", "rFID"] and r["MAE"] == 0.0
    d_fid, d_is = abs(r["rFID"] - float(z[name + ".rFID_hp"])), abs(r["InceptionScore"] - float(z[name + ".IS_hp"]))
    print(f"{name}: rFID {r['rFID']:.12g} |hip - hp| {d_fid:.3g} bound {R.fid_bound(name, 'rFID'):.3g}; IS |hip - hp| {d_is:.3g}")
    assert d_fid <= R.fid_bound(name, "rFID")
    assert d_is <= R.is_bound(name, "tIS_ref")
    ev.reset_metrics()
    with pytest.raises(ValueError, match="No examples"):
        ev.result()


def test_update_entries_agree_and_reset():
    D, C, K = 24, 16, 4096
    ext = R.hashed_extractor(D, C)
    images = R.tiny_images(6, 11, size=16).to(DEV)
    idx = torch.randint(0, K, (6, 5), generator=torch.Generator().manual_seed(3)).to(DEV)
    stats = make_eval_statistics(D, 96, 12)
    kw = dict(enable_fid=True, enable_inception_score=True, enable_codebook_usage_measure=True, enable_codebook_entropy_measure=True)
    u8 = (images * 255).to(torch.uint8)
    feats = ext(u8)
    assert float(feats["2048"].std()) > 0 and float(feats["logits_unbiased"].std()) > 0
    states, results = [], []
    for how in ("update", "update_uint8", "update_features"):
        ev = generator_evaluator(K, **kw)
        ev.use_inception(ext, stats)
        for a, b in ((0, 4), (4, 6)):
            if how == "update":
                ev.update(images[a:b], idx[a:b])
            elif how == "update_uint8":
                ev.update_uint8(u8[a:b], idx[a:b])
            else:
                ev.update_features(feats["2048"][a:b], feats["logits_unbiased"][a:b], idx[a:b])
        states.append(ev.fid_statistics() + ev.is_statistics() + (ev._hist.clone(),))
        results.append(ev.result())
    assert list(results[0]) == ["InceptionScore", "FID", "CodebookUsage", "CodebookEntropy"]
    for st, r in zip(states[1:], results[1:]):
        assert all(torch.equal(a, b) if isinstance(a, torch.Tensor) else a == b for a, b in zip(st, states[0]))
        assert all(float(r[k]) == float(results[0][k]) for k in r)
    # reset: a second pass leaves the bits of the first, and a new feature width is accepted only after it
    with pytest.raises(ValueError, match="reset_metrics"):
        ev.update_features(torch.rand(2, D + 1, device=DEV), feats["logits_unbiased"][:2], idx[:2])
    with pytest.raises(ValueError, match="reset_metrics"):
        ev.update_features(feats["2048"][:2], torch.rand(2, C + 1, device=DEV), idx[:2])
    ev.reset_metrics()
    with pytest.raises(ValueError, match="No examples"):
        ev.result()
    ev.update_features(feats["2048"][:4], feats["logits_unbiased"][:4], idx[:4])
    ev.update_features(feats["2048"][4:], feats["logits_unbiased"][4:], idx[4:])
    assert all(torch.equal(a, b) if isinstance(a, torch.Tensor) else a == b
               for a, b in zip(ev.fid_statistics() + ev.is_statistics() + (ev._hist,), states[0]))
    # without statistics FID is refused and the rest is still reported; out-of-range indices surface at result()
    ev = generator_evaluator(K, **kw)
    ev.use_inception(ext)
    ev.update_uint8(u8, idx)
    with pytest.raises(RuntimeError, match="real statistics"):
        ev.result()
    n, total, sigma = ev.fid_statistics()
    assert n == 6 and torch.equal(sigma, sigma.T)
    ev = generator_evaluator(K, enable_inception_score=True, enable_codebook_usage_measure=True)
    ev.use_inception(ext)
    ev.update_uint8(u8, idx)
    assert list(ev.result()) == ["InceptionScore", "CodebookUsage"]
    bad = idx.clone()
    bad[0, 0], bad[1, 1] = K, -1
    ev.update_uint8(u8, bad)
    with pytest.raises(IndexError, match="2 codebook indices"):
        ev.result()


def test_eval_generation_matches_generate_uint8_bit_for_bit():
    from maskbit_amd import eval_generation, generate_uint8, to_evaluator_uint8
    from test_hip_edit import tiny_models
    gm, tm = tiny_models()
    D, C, K = 24, 16, 4096
    ext, stats = R.hashed_extractor(D, C), make_eval_statistics(D, 96, 12)
    kw = dict(enable_fid=True, enable_inception_score=True, enable_codebook_usage_measure=True, enable_codebook_entropy_measure=True)
    sampling = dict(softmax_temperature=1.0, randomize_temperature=8.2, mask_schedule_strategy="arccos", num_steps=4, guidance_scale=7.1,
                    guidance_annealing="cosine", use_sampling_annealing=False, scale_pow=3.0)
    labels = torch.tensor([1, 4, 8, 0])
    ev = generator_evaluator(K, **kw)
    ev.use_inception(ext, stats)
    ev.update_features(torch.rand(3, D, device=DEV), torch.rand(3, C, device=DEV), torch.zeros(3, 2, dtype=torch.int64, device=DEV))   # reset by the run
    r = eval_generation(gm, tm, ev, 4, 2, labels, seed=7, **sampling)
    other = generator_evaluator(K, **kw)
    other.use_inception(ext, stats)
    batches = list(generate_uint8(gm, tm, labels, 2, seed=7, return_codes=True, **sampling))
    assert len(batches) == 2
    for imgs, codes in batches:
        other.update_uint8(to_evaluator_uint8(torch.from_numpy(imgs).to(DEV)), torch.from_numpy(codes).to(DEV))
    for a, b in zip(ev.fid_statistics() + ev.is_statistics() + (ev._hist,), other.fid_statistics() + other.is_statistics() + (other._hist,)):
        assert torch.equal(a, b) if isinstance(a, torch.Tensor) else a == b
    want = other.result()
    assert list(r) == list(want) == ["InceptionScore", "FID", "CodebookUsage", "CodebookEntropy"]
    assert all(float(r[k]) == float(want[k]) for k in r) and np.isfinite(r["FID"]) and r["InceptionScore"] >= 1.0
    assert int(ev._hist.sum()) == 4 * batches[0][1].shape[1]
    # default labels cover the run; an unseeded run goes through the same loop
    r2 = eval_generation(gm, tm, ev, 4, 2, **sampling)
    assert list(r2) == list(r) and ev._num_examples == 4
