"""A plain float64 torch restatement of the FID / Inception-score state update (evaluator/evaluator.py:549-569) and of both result formulas
(:586-626), with the terms the derived bounds of tests/test_hip_fid.py are stated in.  Test-side code: the yardstick for shapes that have no
golden, checked against the reference's recorded values in tests/test_fid_cpu.py."""
import functools
import math

import torch

from conftest import load_golden
from maskbit_amd.synth import make_eval_features, make_eval_indices, make_eval_statistics

EPS64 = 2.0 ** -53
IS_EPS = 1e-16


@functools.lru_cache(maxsize=None)
def golden():
    return load_golden("generator_evaluator.npz")


def feature_cases():
    return [str(n) for n in golden()["feature_cases"]]


def index_cases():
    return [str(n) for n in golden()["index_cases"]]


@functools.lru_cache(maxsize=None)
def feature_case(name):
    """-> dict of a golden feature case: its inputs regenerated from the recorded seeds, shared by every test that needs them (read only)."""
    z = golden()
    D, C, N, batch, seed_fake, seed_real, seed_stats, n_stats = (int(v) for v in z[name + ".params"])
    fake, logits = make_eval_features(D, C, N, seed_fake, "fake")
    real, _ = make_eval_features(D, C, N, seed_real, "real")
    if name + ".mu" in z:
        mu, sigma = torch.from_numpy(z[name + ".mu"]), torch.from_numpy(z[name + ".sigma"])
    else:
        mu, sigma = make_eval_statistics(D, n_stats, seed_stats)
    return dict(D=D, C=C, N=N, batch=batch, fake=fake, real=real, logits=logits, mu=mu, sigma=sigma,
                splits=[(a, min(a + batch, N)) for a in range(0, N, batch)])


def index_case(name):
    """-> (K, [indices of every update]) of a golden index case."""
    z = golden()
    K = int(z[name + ".K"])
    return K, [make_eval_indices(str(kind), K, [int(v) for v in shape if v >= 0], int(seed))
               for kind, shape, seed in zip(z[name + ".kinds"], z[name + ".shapes"], z[name + ".seeds"])]


# ---- the state update -----------------------------------------------------------------------------------------------------------------------
def fid_update64(total, sigma, feats):
    """total += sum_n f_n, sigma += F^T F in float64 -> (total, sigma, |.| terms): the last two are sum_n |f_n| and |F|^T |F| of THIS batch,
    what the rounding bound of the update is stated in."""
    f = feats.double()
    return total + f.sum(0), sigma + f.T @ f, f.abs().sum(0), f.abs().T @ f.abs()


def softmax64(logits):
    """softmax in float64 with the row maximum subtracted, the row sum of the exponentials rounded ONCE (``math.fsum``: the exactly rounded sum).
    ``torch.softmax`` adds the exponentials lane by lane; next to a dominant 1 every such addition rounds to the grid of the 1, the sum ends up a
    unit or two of its last place off, and log(p + 1e-16) close to p = 1 -- where log(u) = -(1 - u) -- hands that on to the term as an ABSOLUTE
    2^-52, whatever the size of the term.  A yardstick that is compared per column, relative to the terms, must not carry that itself."""
    x = logits.double()
    e = torch.exp(x - x.max(-1, keepdim=True).values)
    s = torch.tensor([math.fsum(row) for row in e.tolist()], dtype=torch.float64).unsqueeze(1)
    return e / s


def is_update64(prob_total, kl_total, logits):
    """evaluator.py:553-564 in float64 -> (prob_total, kl_total, sum_n |p|, sum_n |p log(p + eps)|)."""
    p = softmax64(logits)
    kl = p * torch.log(p + IS_EPS)
    return prob_total + p.sum(0), kl_total + kl.sum(0), p.sum(0), kl.abs().sum(0)


# ---- the results ------------------------------------------------------------------------------------------------------------------------------
def covariance64(sigma, total, n):
    return (sigma - torch.outer(total, total) / n) / (n - 1)


def frechet64(mu1, s1, mu2, s2):
    """The Frechet distance through the symmetric form: eigenvalues of S1^(1/2) S2 S1^(1/2), clamped at 0."""
    w, v = torch.linalg.eigh((s1 + s1.T) / 2)
    root = (v * w.clamp_min(0).sqrt()) @ v.T
    m = root @ ((s2 + s2.T) / 2) @ root
    ev = torch.linalg.eigvalsh((m + m.T) / 2).clamp_min(0)
    d = mu1 - mu2
    return float(d.dot(d) + torch.trace(s1) + torch.trace(s2) - 2 * ev.sqrt().sum())


def score64(prob_total, kl_total, n):
    mean = prob_total / n
    return float(torch.exp(torch.sum(kl_total - prob_total * torch.log(mean + IS_EPS)) / n))


def fid_bound(name, key="FID"):
    """max(2 E_ref, D 2^-52 (tr S_r + tr S_f)) of a golden case, E_ref = |ref - hp|."""
    z = golden()
    D = int(z[name + ".params"][0])
    e_ref = abs(float(z[f"{name}.{key}_ref"]) - float(z[f"{name}.{key}_hp"]))
    return max(2 * e_ref, D * 2.0 ** -52 * float(z[name + (".tr" if key == "FID" else ".rtr")]))


def is_bound(name, key="IS_ref"):
    z = golden()
    C = int(z[name + ".params"][1])
    hp = float(z[name + ".IS_hp"])
    return max(2 * abs(float(z[f"{name}.{key}"]) - hp), C * 2.0 ** -50 * hp)


def codebook64(K, updates):
    counts = torch.zeros(K, dtype=torch.int64)
    for idx in updates:
        counts += torch.bincount(idx.flatten(), minlength=K)
    p = counts.double() / counts.double().sum()
    return float((counts > 0).sum()) / K, float((-torch.log2(p + 1e-8) * p).sum())


class Handout:
    """Stand-in feature extractor with the contract of the reference's get_inception_model(): hands out prepared (pool, logits) batches in
    order, whatever the uint8 images are, and keeps the images it was called with."""

    def __init__(self, batches, device=None):
        self.batches = [(p.to(device) if device else p, l.to(device) if device else l) for p, l in batches]
        self.seen = []

    def __call__(self, u8):
        assert u8.dtype == torch.uint8 and u8.dim() == 4
        self.seen.append(u8)
        pool, logits = self.batches.pop(0)
        assert pool.shape[0] == u8.shape[0]
        return {"2048": pool, "logits_unbiased": logits}


def hashed_extractor(D, C):
    """A deterministic extractor that DOES depend on the image bytes: pooled means of image strips -> (pool [B, D], logits [B, C]) in float64."""
    def run(u8):
        x = u8.double().flatten(1)
        n = x.shape[1]
        pool = torch.stack([x[:, (i * 37) % n::D + 3].mean(1) / 255.0 for i in range(D)], 1)
        logits = torch.stack([x[:, (i * 53) % n::C + 5].mean(1) / 16.0 for i in range(C)], 1)
        return {"2048": pool, "logits_unbiased": logits}
    return run


def tiny_images(B, seed, size=8):
    g = torch.Generator().manual_seed(seed)
    return torch.rand(B, 3, size, size, generator=g)

