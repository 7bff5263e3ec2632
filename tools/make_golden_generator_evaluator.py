"""Golden fixture of the generator evaluator: the reference's ``GeneratorEvaluator`` (evaluator/evaluator.py:469-641) and the rFID / Inception
score half of its ``TokenizerEvaluator`` (:336-364, :406-451) run on the CPU on seeded synthetic features.  Needs the reference checkout
(MASKBIT_REFERENCE, as oracle/make_golden.py) and mpmath; writes results only to tests/golden/generator_evaluator.npz -- the tests regenerate the
inputs from the recorded seeds (maskbit_amd.synth.make_eval_features / make_eval_statistics / make_eval_indices).

The Inception network is out of scope (its weights are a download), so the evaluators are constructed with every flag off, then given the flags,
the feature widths, the real statistics and a stand-in ``_inception_model`` that hands out the synthetic features batch by batch, and reset.

Per feature case:
  FID_ref, IS_ref      the reference's ``GeneratorEvaluator.result()`` (scipy ``sqrtm`` of the non-symmetric product, fp64),
  rFID_ref, tIS_ref    the reference's ``TokenizerEvaluator.result()`` on paired real / fake features (D <= 64),
  FID_hp, IS_hp, rFID_hp   the same quantities from the REFERENCE'S OWN accumulated statistics, taken as exact numbers and evaluated with mpmath
                       at 40 digits (covariance, matrix square root through the symmetric eigenproblem, trace; softmax sums -> score),
  tr                   tr S_real + tr S_fake (the unit of the FID bound's floor); rtr for rFID,
  mu, sigma            the real statistics, for D <= 64.
E_ref = |ref - hp| is the reference's own evaluation error: the unit of the bounds in tests/test_hip_fid.py.  The tool also evaluates this
project's ``frechet_distance`` / ``inception_score`` on the same statistics and says so loudly if either -- or the reference -- falls outside
max(2 E_ref, floor): such a case is to be replaced, not the bound.

Per index case the reference's CodebookUsage and CodebookEntropy from ``GeneratorEvaluator``.

    python tools/make_golden_generator_evaluator.py
"""
from __future__ import annotations

import os
import sys
import time

import mpmath as mp
import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from make_golden_evaluator import INDEX_CASES, import_reference_evaluator  # noqa: E402
from maskbit_amd.generator_evaluator import frechet_distance, get_covariance, inception_score  # noqa: E402
from maskbit_amd.synth import make_eval_features, make_eval_indices, make_eval_statistics  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "generator_evaluator.npz")

# name -> (D, C, N, batch, seed of the fake features, seed of the paired real features, seed and N of the real statistics)
FEATURE_CASES = {
    "full32": (32, 48, 96, 32, 3000, 3001, 3002, 128),
    "full64": (64, 100, 192, 64, 3010, 3011, 3012, 256),
    "sing32": (32, 48, 24, 8, 3020, 3021, 3022, 128),        # N < D: a singular covariance
    "sing64": (64, 100, 40, 16, 3030, 3031, 3032, 256),      # batches of 16, 16, 8
    "wide256": (256, 1008, 768, 64, 3040, 3041, 3042, 1024),
}
RFID_MAX_D = 64

mp.mp.dps = 40


def to_mp(t: torch.Tensor):
    a = t.double().numpy()
    return mp.matrix([[mp.mpf(float(v)) for v in row] for row in a]) if a.ndim == 2 else [mp.mpf(float(v)) for v in a]


def covariance_hp(sigma, total, n):
    D = len(total)
    return mp.matrix([[(sigma[i, j] - total[i] * total[j] / n) / (n - 1) for j in range(D)] for i in range(D)])


def frechet_hp(mu1, s1, mu2, s2):
    """40-digit Frechet distance; tr sqrt(S1 S2) = sum sqrt eig(L^T S2 L) with S1 = L L^T (Cholesky, or the symmetric square root when S1 is
    singular)."""
    D = len(mu1)
    s1, s2 = (s1 + s1.T) / 2, (s2 + s2.T) / 2
    try:
        left = mp.cholesky(s1)
    except (ValueError, ZeroDivisionError):
        w, v = mp.eigsy(s1)
        left = v * mp.diag([mp.sqrt(max(x, mp.mpf(0))) for x in w])         # S1 = left left^T with the negative dust clamped
    m = left.T * s2 * left
    ev = mp.eigsy((m + m.T) / 2, eigvals_only=True)
    tr_covmean = mp.fsum(mp.sqrt(max(x, mp.mpf(0))) for x in ev)
    diff2 = mp.fsum((a - b) ** 2 for a, b in zip(mu1, mu2))
    tr = mp.fsum(s1[i, i] + s2[i, i] for i in range(D))
    return diff2 + tr - 2 * tr_covmean, tr


def score_hp(prob_total, kl_total, n):
    p, k = to_mp(prob_total), to_mp(kl_total)
    eps = mp.mpf(float(1e-16))
    return mp.exp(mp.fsum(kk - pp * mp.log(pp / n + eps) for pp, kk in zip(p, k)) / n)


class Handout:
    """Stand-in for the Inception network: returns the next prepared batch whatever the images are."""

    def __init__(self, batches):
        self.batches = list(batches)

    def __call__(self, images):
        pool, logits = self.batches.pop(0)
        assert pool.shape[0] == images.shape[0]
        return {"2048": pool, "logits_unbiased": logits}


def splits(N, batch):
    return [(a, min(a + batch, N)) for a in range(0, N, batch)]


def verdict(name, what, ref, ours, hp, floor):
    e_ref, e_ours = abs(ref - hp), abs(ours - hp)
    bound = max(2 * e_ref, floor)
    flag = "" if e_ours <= bound and e_ref <= bound else "   <-- OUTSIDE THE BOUND: replace this case"
    print(f"{name:8s} {what:5s} hp {hp:.15g}  E_ref {e_ref:.3g}  eigh form {e_ours:.3g}  floor {floor:.3g}{flag}")


def main():
    E = import_reference_evaluator()
    torch.set_grad_enabled(False)
    out = dict(feature_cases=np.array(list(FEATURE_CASES)), index_cases=np.array(list(INDEX_CASES)))
    for name, (D, C, N, batch, seed_fake, seed_real, seed_stats, n_stats) in FEATURE_CASES.items():
        t0 = time.time()
        fake, logits = make_eval_features(D, C, N, seed_fake, "fake")
        mu, sigma = make_eval_statistics(D, n_stats, seed_stats)
        ev = E.GeneratorEvaluator("cpu")
        ev._enable_fid = ev._enable_inception_score = True
        ev._fid_num_features, ev._is_num_features = D, C
        ev._fid_real_mu, ev._fid_real_sigma = mu, sigma
        ev._inception_model = Handout((fake[a:b], logits[a:b]) for a, b in splits(N, batch))
        ev.reset_metrics()
        for a, b in splits(N, batch):
            ev.update(torch.zeros(b - a, 3, 8, 8))
        r = ev.result()
        assert tuple(r) == ("InceptionScore", "FID")
        fid_hp, tr = frechet_hp(to_mp(mu), to_mp(sigma), [t / N for t in to_mp(ev._fid_fake_total)],
                                covariance_hp(to_mp(ev._fid_fake_sigma), to_mp(ev._fid_fake_total), N))
        is_hp = score_hp(ev._is_prob_total, ev._is_total_kl_d, N)
        out[name + ".params"] = np.array([D, C, N, batch, seed_fake, seed_real, seed_stats, n_stats], dtype=np.int64)
        out[name + ".FID_ref"], out[name + ".FID_hp"] = np.float64(r["FID"]), np.float64(float(fid_hp))
        out[name + ".IS_ref"], out[name + ".IS_hp"] = np.float64(r["InceptionScore"]), np.float64(float(is_hp))
        out[name + ".tr"] = np.float64(float(tr))
        if D <= 64:
            out[name + ".mu"], out[name + ".sigma"] = mu.numpy(), sigma.numpy()
        ours = frechet_distance(mu, sigma, ev._fid_fake_total / N, get_covariance(ev._fid_fake_sigma, ev._fid_fake_total, N))
        verdict(name, "FID", r["FID"], ours, float(fid_hp), D * 2.0 ** -52 * float(tr))
        verdict(name, "IS", r["InceptionScore"], inception_score(ev._is_prob_total, ev._is_total_kl_d, N), float(is_hp), C * 2.0 ** -50 * float(is_hp))

        if D <= RFID_MAX_D:
            real, _ = make_eval_features(D, C, N, seed_real, "real")
            tv = E.TokenizerEvaluator("cpu")
            tv._enable_rfid = tv._enable_inception_score = True
            tv._rfid_num_features, tv._is_num_features = D, C
            tv._inception_model = Handout(x for a, b in splits(N, batch) for x in ((fake[a:b], logits[a:b]), (real[a:b], logits[a:b])))
            tv.reset_metrics()
            for a, b in splits(N, batch):
                z = torch.zeros(b - a, 3, 8, 8)
                tv.update(z, z)
            r = tv.result()
            assert tuple(r) == ("InceptionScore", "rFID")
            stats = [(to_mp(t), to_mp(s)) for t, s in ((tv._rfid_real_total, tv._rfid_real_sigma), (tv._rfid_fake_total, tv._rfid_fake_sigma))]
            (mu_r, s_r), (mu_f, s_f) = (([v / N for v in t], covariance_hp(s, t, N)) for t, s in stats)
            rfid_hp, rtr = frechet_hp(mu_r, s_r, mu_f, s_f)
            out[name + ".rFID_ref"], out[name + ".rFID_hp"] = np.float64(r["rFID"]), np.float64(float(rfid_hp))
            out[name + ".tIS_ref"], out[name + ".rtr"] = np.float64(r["InceptionScore"]), np.float64(float(rtr))
            ours = frechet_distance(tv._rfid_real_total / N, get_covariance(tv._rfid_real_sigma, tv._rfid_real_total, N),
                                    tv._rfid_fake_total / N, get_covariance(tv._rfid_fake_sigma, tv._rfid_fake_total, N))
            verdict(name, "rFID", r["rFID"], ours, float(rfid_hp), D * 2.0 ** -52 * float(rtr))
        print(f"{name:8s} {time.time() - t0:.0f} s")

    for name, (K, updates) in INDEX_CASES.items():
        ev = E.GeneratorEvaluator("cpu", enable_codebook_usage_measure=True, enable_codebook_entropy_measure=True, num_codebook_entries=K)
        for kind, shape, seed in updates:
            ev.update(torch.zeros(1, 3, 8, 8), make_eval_indices(kind, K, shape, seed))
        r = ev.result()
        assert tuple(r) == ("CodebookUsage", "CodebookEntropy")
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
