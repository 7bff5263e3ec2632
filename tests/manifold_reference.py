"""A float64 restatement of the k-NN manifolds behind precision / recall (ADM's manifold_radii / evaluate_pr / compute_prec_recall) BY DIFFERENCES,
independent of the GEMM form |a|^2 + |b|^2 - 2 a.b the kernels of csrc/manifold.hip use, and the derived error bound of that form.

    d2(a, b)  = sum_d (a_d - b_d)^2 in float64, the diagonal of a set against itself exactly 0
    radii2[i] = the (k+1)-th smallest of row i of d2(X, X) (sort, with multiplicity)
    inside[q] = any_j d2(q, b_j) <= radii2[j]

Bound of the kernels' form against this restatement, per pair, derived and not measured (u = 2^-53, fp32 inputs widened, so every product is exact):

    E(a, b) = 2 (D + 4) u (|a|^2 + |b|^2)

  |a|^2, |b|^2 and a.b are each a chain of at most D fp64 multiply-adds: off by at most D u times the sum of the magnitudes of the terms, that is
  D u |a|^2, D u |b|^2 and D u sum_d |a_d b_d| <= D u (|a|^2 + |b|^2) / 2.  The cross term enters twice, so the three sums contribute at most
  2 D u (|a|^2 + |b|^2); the rounding of |a|^2 + |b|^2 and of the final fma add at most 3 u (|a|^2 + |b|^2) (|d2| <= 2 (|a|^2 + |b|^2)):
  (2 D + 3) u (|a|^2 + |b|^2) < E.  That is the worst case of chains of the full length with every rounding in the same direction; the kernel's
  norm chains are D / 64 + 6 long, and roundings of mixed sign grow like the square root of the length, so the restatement's own error -- below
  (D + 2) u d2 for a sum of D squares of once-rounded differences -- sits inside the same E.
"""
import numpy as np

U = 2.0 ** -53


def pair_d2(a, b, same=False, block=64):
    """float64 [Na, Nb] of sum_d (a_d - b_d)^2; ``same``: a is b, the diagonal is exactly 0"""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    out = np.empty((a.shape[0], b.shape[0]), dtype=np.float64)
    for i0 in range(0, a.shape[0], block):
        diff = a[i0:i0 + block, None, :] - b[None, :, :]
        out[i0:i0 + block] = (diff * diff).sum(axis=2)
    if same:
        np.fill_diagonal(out, 0.0)
    return out


def pair_bound(a, b):
    """E(a, b) [Na, Nb]"""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    D = a.shape[1]
    return 2.0 * (D + 4) * U * ((a * a).sum(axis=1)[:, None] + (b * b).sum(axis=1)[None, :])


def knn_radii(x, k):
    return np.sort(pair_d2(x, x, same=True), axis=1)[:, k]


def cover(q, b, radii2, d2=None):
    d2 = pair_d2(q, b) if d2 is None else d2
    return (d2 <= np.asarray(radii2)[None, :]).any(axis=1)


def precision_recall(ref, samples, k):
    in_ref = cover(samples, ref, knn_radii(ref, k))
    in_samples = cover(ref, samples, knn_radii(samples, k))
    return int(in_ref.sum()) / samples.shape[0], int(in_samples.sum()) / ref.shape[0]


def seeded_sets(Nr, Ns, D, shift, scale, seed):
    """the seeded case of the tests: standard-normal reference rows, sample rows scaled and shifted; fp32"""
    rng = np.random.default_rng(seed)
    ref = rng.standard_normal((Nr, D)).astype(np.float32)
    samples = (rng.standard_normal((Ns, D)) * scale + shift).astype(np.float32)
    return ref, samples


def cover_margin(d2, radii2):
    """per query min_j (d2 - radii2_j): <= 0 inside, > 0 outside; its magnitude is how far the decision is from flipping, its argmin the pair"""
    g = d2 - np.asarray(radii2)[None, :]
    return g.min(axis=1), g.argmin(axis=1)
