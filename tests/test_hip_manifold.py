"""GPU checks of csrc/manifold.hip (mb_knn_radii, mb_manifold_cover), maskbit_amd.manifold and GeneratorEvaluator.use_precision_recall against the
float64 restatement by differences of tests/manifold_reference.py.

Bounds (none of them comes from the code under test):
  radii2        per row |hip - restatement| <= max_j E(x_i, x_j), E(a, b) = 2 (D + 4) 2^-53 (|a|^2 + |b|^2) (derived in manifold_reference.py): an
                order statistic moves by at most the largest change of the values it is taken over.
  inside, P, R  EQUAL to the restatement's.  A query is decidable when a pair puts it inside by more than E(q, b_j) + max_j' E(b_j, b_j') (the
                pair's own error plus that of the radius it is compared with), or every pair keeps it outside by more than that; the seeded cases
                have no undecidable row, which is asserted on the restatement alone before anything is compared.
  exact cases   integer-valued features, |v| <= 64: every sum is an integer far below 2^53, so the kernels must equal integer arithmetic.
  bit identity  repeated runs, row permutations, query chunks: torch.equal.
"""
import functools

import numpy as np
import pytest
import torch

import manifold_reference as M

pytestmark = pytest.mark.gpu
DEV = "cuda"
SEEDED = ((257, 301, 64, 3, 0.15, 0.9), (130, 75, 24, 3, 0.2, 0.85), (67, 193, 2048, 3, 0.0, 0.98), (257, 301, 16, 5, 0.3, 0.8))
SEEDS = (0, 1, 2)


def dev(x, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(x))
    return t.to(DEV, dtype) if dtype is not None else t.to(DEV)


def strided(x, pad, dtype=None):
    """the rows of x inside a wider matrix whose other columns hold large values: a row stride above D, and a kernel that reads past D shows"""
    wide = torch.full((x.shape[0], x.shape[1] + pad), 1.0e3, dtype=dtype or torch.from_numpy(x[:1]).dtype, device=DEV)
    view = wide[:, :x.shape[1]]
    view.copy_(dev(x))
    return view


@functools.lru_cache(maxsize=None)
def seeded(case, seed):
    """the restatement of one seeded case, computed once: sets, radii, flags, and the decidability of every row"""
    Nr, Ns, D, k, shift, scale = case
    ref, smp = M.seeded_sets(Nr, Ns, D, shift, scale, seed)
    out = {"ref": ref, "smp": smp, "k": k}
    for name, base, query in (("ref", ref, smp), ("smp", smp, ref)):
        self_bound = M.pair_bound(base, base).max(axis=1)              # max_j E(x_i, x_j): the bound of radii2[i]
        radii2 = M.knn_radii(base, k)
        d2 = M.pair_d2(query, base)
        gap = d2 - radii2[None, :]
        tol = M.pair_bound(query, base) + self_bound[None, :]
        decidable = (gap <= -tol).any(axis=1) | (gap > tol).all(axis=1)
        out[name + "_radii2"], out[name + "_bound"] = radii2, self_bound
        out[name + "_inside"], out[name + "_undecidable"] = (gap <= 0).any(axis=1), int((~decidable).sum())
    return out


def check_radii(got, want, bound, what):
    err = np.abs(got.cpu().numpy() - want)
    print(f"{what}: radii2 max err {err.max():.3e}, bound min {bound.min():.3e}, worst ratio {(err / bound).max():.3e}")
    assert (err <= bound).all(), f"{what}: {int((err > bound).sum())} radii outside the bound, worst ratio {(err / bound).max()}"


@pytest.mark.parametrize("seed", SEEDS)
@pytest.mark.parametrize("case", SEEDED, ids=lambda c: f"{c[0]}x{c[1]}x{c[2]}k{c[3]}")
def test_seeded_against_restatement(case, seed):
    from maskbit_amd import knn_radii, manifold_coverage, precision_recall
    z = seeded(case, seed)
    k = z["k"]
    want_p, want_r = z["ref_inside"].mean(), z["smp_inside"].mean()
    # the inputs, on the restatement alone: neither figure degenerate, every row decidable
    assert 0.885 <= want_p <= 0.995 and 0.155 <= want_r <= 0.485, (want_p, want_r)
    assert z["ref_undecidable"] == 0 and z["smp_undecidable"] == 0
    ref32, smp32 = dev(z["ref"]), dev(z["smp"])
    ref64, smp64 = ref32.double(), smp32.double()
    ref_wide, smp_wide = strided(z["ref"], 3), strided(z["smp"].astype(np.float64), 5, torch.float64)
    for what, ref, smp in (("fp32", ref32, smp32), ("fp64", ref64, smp64), ("mixed", ref32, smp64), ("mixed2", ref64, smp32),
                           ("strided", ref_wide, smp_wide)):
        r_ref, r_smp = knn_radii(ref, k), knn_radii(smp, k)
        check_radii(r_ref, z["ref_radii2"], z["ref_bound"], f"{what} reference")
        check_radii(r_smp, z["smp_radii2"], z["smp_bound"], f"{what} samples")
        in_ref, in_smp = manifold_coverage(smp, ref, r_ref), manifold_coverage(ref, smp, r_smp)
        assert in_ref.dtype == torch.bool and in_smp.dtype == torch.bool
        assert np.array_equal(in_ref.cpu().numpy(), z["ref_inside"]), what
        assert np.array_equal(in_smp.cpu().numpy(), z["smp_inside"]), what
        p, r = precision_recall(ref, smp, k)
        assert (p, r) == (int(z["ref_inside"].sum()) / len(z["smp"]), int(z["smp_inside"].sum()) / len(z["ref"])), what


# ---- exact cases --------------------------------------------------------------------------------------------------------------------------
def int_d2(a, b):
    a, b = a.astype(np.int64), b.astype(np.int64)
    return ((a[:, None, :] - b[None, :, :]) ** 2).sum(axis=2)


def int_radii(x, k):
    d2 = int_d2(x, x)
    return np.sort(d2, axis=1)[:, k]


@pytest.mark.parametrize("dtype", (torch.float32, torch.float64), ids=("fp32", "fp64"))
@pytest.mark.parametrize("D", (1, 3, 5, 2048))
def test_integer_features_are_exact(D, dtype):
    from maskbit_amd import knn_radii, manifold_coverage
    rng = np.random.default_rng(100 + D)
    x = rng.integers(-64, 65, size=(83, D)).astype(np.float64)
    q = rng.integers(-64, 65, size=(41, D)).astype(np.float64)
    x[7] = x[3]; x[20] = x[3]; x[21] = x[3]                             # duplicate rows: the zeros count
    for k in (1, 3, 8):
        want = int_radii(x, k)
        got = knn_radii(dev(x, dtype), k)
        assert np.array_equal(got.cpu().numpy(), want.astype(np.float64)), (D, k)
        inside = manifold_coverage(dev(q, dtype), dev(x, dtype), got)
        assert np.array_equal(inside.cpu().numpy(), (int_d2(q, x) <= want[None, :]).any(axis=1)), (D, k)
    assert knn_radii(dev(x, dtype), 3)[3].item() == 0.0                 # three other copies of row 3


@pytest.mark.parametrize("dtype", (torch.float32, torch.float64), ids=("fp32", "fp64"))
def test_constructed_ties(dtype):
    from maskbit_amd import knn_radii, manifold_coverage
    # base on a line: 0, 3, 4 (the point), 5, 12 along the first axis, D = 3.  k = 1: the point at 4 has both neighbours at distance 1.
    base = np.zeros((5, 3)); base[:, 0] = (0, 3, 4, 5, 12)
    r1 = knn_radii(dev(base, dtype), 1).cpu().numpy()
    assert r1.tolist() == [9.0, 1.0, 1.0, 1.0, 49.0]
    r2 = knn_radii(dev(base, dtype), 2).cpu().numpy()                   # equal distances among the neighbours: with multiplicity
    assert r2.tolist() == [16.0, 4.0, 1.0, 4.0, 64.0]
    # one far base row of radius^2 = 25 (k = 1: its only neighbour is at (3, 4, 0) from it)
    far = np.array([[60.0, 0, 0], [63.0, 4, 0]])
    rf = knn_radii(dev(far, dtype), 1)
    assert rf.cpu().numpy().tolist() == [25.0, 25.0]                    # N = k + 1
    queries = np.array([[60.0, 0, 5],       # d2 = 25 to row 0: exactly the radius -> inside (<=)
                        [60.0, 1, 5],       # d2 = 26 to row 0, 9 + 9 + 25 = 43 to row 1 -> outside
                        [55.0, 0, 0],       # 25 again, along another axis
                        [54.0, 0, 0],       # 36 -> outside
                        [63.0, 4, 0]])     # a base row itself
    inside = manifold_coverage(dev(queries, dtype), dev(far, dtype), rf).cpu().numpy()
    assert inside.tolist() == [True, False, True, False, True]
    # duplicates: four copies of one row and another row; k = 3 -> radius 0 for the copies, and a copy of them is inside (0 <= 0)
    dup = np.array([[2.0, -1, 7]] * 4 + [[10.0, 0, 0]])
    rd = knn_radii(dev(dup, dtype), 3).cpu().numpy()
    assert rd[:4].tolist() == [0.0] * 4 and rd[4] == 64.0 + 1 + 49
    assert manifold_coverage(dev(dup[:1], dtype), dev(dup, dtype), dev(rd)).cpu().numpy().tolist() == [True]
    assert manifold_coverage(dev(np.array([[2.0, -1, 8]]), dtype), dev(dup[:4], dtype), dev(rd[:4])).cpu().numpy().tolist() == [False]


# ---- edges and the walk -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("D", (1, 3, 4, 5))
def test_edges_of_the_tiles(D):
    """N around the 16-row strip and the 64-column tile.  Standard-normal rows: a phantom all-zero row past the edge would be at |a|^2, about D,
    nearer than the real neighbours at about 2 D -- as a neighbour it shrinks radii, as a base row it covers queries it must not."""
    from maskbit_amd import knn_radii, manifold_coverage
    k = 3
    rng = np.random.default_rng(7 + D)
    for N in (k + 1, 15, 16, 17, 63, 64, 65, 67, 130):
        x = rng.standard_normal((N, D)).astype(np.float32)
        q = (rng.standard_normal((N + 2, D)) * 3).astype(np.float32)
        want = M.knn_radii(x, k)
        got = knn_radii(dev(x), k)
        check_radii(got, want, M.pair_bound(x, x).max(axis=1), f"N {N} D {D}")
        gap = M.pair_d2(q, x) - want[None, :]
        tol = M.pair_bound(q, x) + M.pair_bound(x, x).max(axis=1)[None, :]
        ok = (gap <= -tol).any(axis=1) | (gap > tol).all(axis=1)
        inside = manifold_coverage(dev(q), dev(x), got).cpu().numpy()
        assert ok.all()                                                 # (the inputs, on the restatement alone)
        assert 0 < (gap <= 0).any(axis=1).sum() < len(q)
        assert np.array_equal(inside, (gap <= 0).any(axis=1)), (N, D)


def test_long_walk():
    from maskbit_amd import knn_radii, manifold_coverage
    rng = np.random.default_rng(11)
    x = rng.standard_normal((1030, 8)).astype(np.float32)
    q = (rng.standard_normal((1030, 8)) * 2.5).astype(np.float32)
    want = M.knn_radii(x, 3)
    got = knn_radii(dev(x), 3)
    check_radii(got, want, M.pair_bound(x, x).max(axis=1), "N 1030")
    gap = M.pair_d2(q, x) - want[None, :]
    tol = M.pair_bound(q, x) + M.pair_bound(x, x).max(axis=1)[None, :]
    assert ((gap <= -tol).any(axis=1) | (gap > tol).all(axis=1)).all()
    want_in = (gap <= 0).any(axis=1)
    assert 0.05 < want_in.mean() < 0.95
    assert np.array_equal(manifold_coverage(dev(q), dev(x), got).cpu().numpy(), want_in)


# ---- bit identity -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N,D", ((130, 24), (67, 2048), (1030, 5)))
def test_bit_identity(N, D):
    from maskbit_amd import knn_radii, manifold_coverage
    rng = np.random.default_rng(N + D)
    x = dev(rng.standard_normal((N, D)).astype(np.float32))
    q = dev((rng.standard_normal((N + 9, D)) * 0.9).astype(np.float32))
    r = knn_radii(x, 3)
    assert torch.equal(r, knn_radii(x, 3))
    perm = torch.from_numpy(rng.permutation(N)).to(DEV)
    assert torch.equal(knn_radii(x[perm].contiguous(), 3), r[perm])     # the multiset of values a row sees does not depend on tile placement
    inside = manifold_coverage(q, x, r)
    assert torch.equal(inside, manifold_coverage(q, x, r))
    parts, at = [], 0
    for n in (1, 3, 64, q.shape[0] - 68):
        parts.append(manifold_coverage(q[at:at + n], x, r))
        at += n
    assert at == q.shape[0] and torch.equal(torch.cat(parts), inside)
    assert torch.equal(manifold_coverage(q, x[perm].contiguous(), r[perm]), inside)


# ---- refusals of the Python layer ---------------------------------------------------------------------------------------------------------
def test_function_refusals():
    from maskbit_amd import knn_radii, manifold_coverage
    x = torch.zeros(5, 4, device=DEV)
    with pytest.raises(RuntimeError, match="no CPU path"):
        knn_radii(torch.zeros(5, 4))
    with pytest.raises(ValueError, match="k \\+ 1 <= N"):
        knn_radii(x, 5)
    with pytest.raises(ValueError, match="1 <= k"):
        knn_radii(x, 0)
    with pytest.raises(ValueError, match="1 <= k"):
        knn_radii(torch.zeros(20, 4, device=DEV), 9)
    with pytest.raises(ValueError, match="floating-point"):
        knn_radii(torch.zeros(5, 4, device=DEV, dtype=torch.int32))
    with pytest.raises(ValueError, match="columns"):
        manifold_coverage(torch.zeros(3, 5, device=DEV), x, torch.zeros(5, device=DEV, dtype=torch.float64))
    with pytest.raises(ValueError, match="radii2"):
        manifold_coverage(x, x, torch.zeros(4, device=DEV, dtype=torch.float64))


# ---- the evaluator --------------------------------------------------------------------------------------------------------------------------
CASE = SEEDED[1]


def make_evaluator(**kw):
    from maskbit_amd import GeneratorEvaluator
    from maskbit_amd.synth import make_eval_statistics
    ev = GeneratorEvaluator(DEV, enable_fid=True, enable_inception_score=True, **kw)
    ev.use_inception(None, make_eval_statistics(CASE[2], 64, seed=5))
    return ev


def feed(ev, pool, logits, sizes=(1, 3, 64)):
    at = 0
    for n in list(sizes) + [pool.shape[0] - sum(sizes)]:
        ev.update_features(pool[at:at + n], logits[at:at + n])
        at += n
    assert at == pool.shape[0]


def pr(result):
    return result["Precision"], result["Recall"]


def test_evaluator_precision_recall():
    from maskbit_amd import precision_recall
    z = seeded(CASE, 0)
    ref, smp = dev(z["ref"]), dev(z["smp"])
    logits = dev(np.random.default_rng(3).standard_normal((smp.shape[0], 10)).astype(np.float32))
    plain = make_evaluator()
    feed(plain, smp, logits)
    base = plain.result()
    assert list(base) == ["InceptionScore", "FID"]
    ev = make_evaluator()
    ev.use_precision_recall(ref.cpu(), k=z["k"])                        # the reference set may live on any device
    feed(ev, smp, logits)
    got = ev.result()
    assert list(got) == ["InceptionScore", "FID", "Precision", "Recall"]
    assert got["InceptionScore"] == base["InceptionScore"] and got["FID"] == base["FID"]       # the same bits with and without
    want = (int(z["ref_inside"].sum()) / len(z["smp"]), int(z["smp_inside"].sum()) / len(z["ref"]))
    assert (got["Precision"], got["Recall"]) == precision_recall(ref, smp, z["k"]) == want
    assert isinstance(got["Precision"], float) and isinstance(got["Recall"], float)
    assert ev.result() == got
    # a preallocated buffer that is too small grows; one that is large enough is used as it is
    for cap in (8, 4096):
        ev2 = make_evaluator()
        ev2.use_precision_recall(ref, k=z["k"], max_samples=cap)
        feed(ev2, smp, logits, sizes=(5, 2, 30))                        # (other batches: the running sums of FID / IS round differently)
        assert pr(ev2.result()) == pr(got)
    # reset_metrics empties the buffer; the next pass stands alone
    ev.reset_metrics()
    with pytest.raises(ValueError, match="No examples"):
        ev.result()
    ev.update_features(smp[:3], logits[:3])
    with pytest.raises(ValueError, match="at least 4 samples"):
        ev.result()
    ev.reset_metrics()
    feed(ev, smp, logits)
    assert ev.result() == got
    # detached: result() is what it is without the call
    ev.use_precision_recall(None)
    assert ev.result() == base


def test_evaluator_refusals():
    from maskbit_amd import GeneratorEvaluator
    ref = torch.zeros(10, CASE[2])
    with pytest.raises(ValueError, match="enable_fid"):
        GeneratorEvaluator(DEV, enable_inception_score=True).use_precision_recall(ref)
    ev = make_evaluator()
    for bad_k in (0, 9):
        with pytest.raises(ValueError, match="1 <= k"):
            ev.use_precision_recall(ref, k=bad_k)
    with pytest.raises(ValueError, match="k \\+ 1"):
        ev.use_precision_recall(ref[:3], k=3)
    with pytest.raises(ValueError, match="floating-point"):
        ev.use_precision_recall(ref.long())
    with pytest.raises(ValueError, match="floating-point"):
        ev.use_precision_recall(ref[0])
    with pytest.raises(ValueError, match="max_samples"):
        ev.use_precision_recall(ref, max_samples=0)
    ev.use_precision_recall(torch.zeros(10, CASE[2] + 1))
    with pytest.raises(ValueError, match="use_precision_recall"):
        ev.update_features(torch.zeros(4, CASE[2], device=DEV), torch.zeros(4, 10, device=DEV))
