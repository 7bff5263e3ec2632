"""CPU-side checks of the precision / recall surface: the ABI (header == SIGNATURES == library), the host-side refusals of csrc/manifold.hip, the
pinned signatures of the classes the feature adds methods to, and the restatement of tests/manifold_reference.py on its own closed-form cases."""
import ctypes
import inspect
import os

import numpy as np
import pytest
import torch

import manifold_reference as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("mb_manifold_workspace_bytes", "mb_knn_radii", "mb_manifold_cover")


def test_symbols_in_header_signatures_and_library():
    from maskbit_amd import _lib
    lib = ctypes.CDLL(_lib.LIB_PATH)
    header = open(os.path.join(ROOT, "include", "maskbit_hip.h")).read()
    for name in ENTRIES:
        assert name in _lib.SIGNATURES and name + "(" in header
        getattr(lib, name)
    assert "#define MB_ABI_VERSION 8" in header and _lib.ABI_VERSION == 8 and _lib.load().mb_abi_version() == 8


def test_workspace_bytes():
    from maskbit_amd import _lib
    lib = _lib.load()
    per_row = 8 * (1 + 16 * 9)                                 # the norm, and 16 parts of the column walk with a list of 9 doubles each
    assert lib.mb_manifold_workspace_bytes(1, 1) == per_row
    assert lib.mb_manifold_workspace_bytes(50000, 2048) == 50000 * per_row
    assert lib.mb_manifold_workspace_bytes(60000, 2048) == 60000 * per_row         # mb_manifold_cover: queries + base
    assert lib.mb_manifold_workspace_bytes(1 << 24, 1 << 20) == (1 << 24) * per_row
    for N, D in ((0, 4), (-1, 4), (4, 0), ((1 << 24) + 1, 4), (4, (1 << 20) + 1)):
        assert lib.mb_manifold_workspace_bytes(N, D) == 0


def test_entries_refuse_bad_arguments_without_a_device():
    """Every refusal is decided on the host before a launch and names its entry."""
    from maskbit_amd import _lib
    lib = _lib.load()
    p = 4096                                                  # never dereferenced: each call below is refused first
    knn = [
        lambda: lib.mb_knn_radii(None, 0, 8, 4, 4, 3, p, p, None),
        lambda: lib.mb_knn_radii(p, 0, 8, 4, 4, 3, None, p, None),
        lambda: lib.mb_knn_radii(p, 0, 8, 4, 4, 3, p, None, None),
        lambda: lib.mb_knn_radii(p, 2, 8, 4, 4, 3, p, p, None),
        lambda: lib.mb_knn_radii(p, -1, 8, 4, 4, 3, p, p, None),
        lambda: lib.mb_knn_radii(p, 0, 0, 4, 4, 3, p, p, None),
        lambda: lib.mb_knn_radii(p, 0, (1 << 24) + 1, 4, 4, 3, p, p, None),
        lambda: lib.mb_knn_radii(p, 0, 8, 0, 4, 3, p, p, None),
        lambda: lib.mb_knn_radii(p, 0, 8, (1 << 20) + 1, 1 << 21, 3, p, p, None),
        lambda: lib.mb_knn_radii(p, 0, 8, 4, 3, 3, p, p, None),               # stride < D
        lambda: lib.mb_knn_radii(p, 0, 8, 4, 4, 0, p, p, None),
        lambda: lib.mb_knn_radii(p, 0, 20, 4, 4, 9, p, p, None),
        lambda: lib.mb_knn_radii(p, 0, 3, 4, 4, 3, p, p, None),               # k + 1 > N
        lambda: lib.mb_knn_radii(p + 2, 0, 8, 4, 4, 3, p, p, None),
        lambda: lib.mb_knn_radii(p + 4, 1, 8, 4, 4, 3, p, p, None),           # fp64 rows need 8 bytes
        lambda: lib.mb_knn_radii(p, 0, 8, 4, 4, 3, p + 4, p, None),
        lambda: lib.mb_knn_radii(p, 0, 8, 4, 4, 3, p, p + 4, None),
    ]
    cover = [
        lambda: lib.mb_manifold_cover(None, 0, 8, 4, p, 0, 8, 4, 4, p, p, p, None),
        lambda: lib.mb_manifold_cover(p, 0, 8, 4, None, 0, 8, 4, 4, p, p, p, None),
        lambda: lib.mb_manifold_cover(p, 0, 8, 4, p, 0, 8, 4, 4, None, p, p, None),
        lambda: lib.mb_manifold_cover(p, 0, 8, 4, p, 0, 8, 4, 4, p, None, p, None),
        lambda: lib.mb_manifold_cover(p, 0, 8, 4, p, 0, 8, 4, 4, p, p, None, None),
        lambda: lib.mb_manifold_cover(p, 2, 8, 4, p, 0, 8, 4, 4, p, p, p, None),
        lambda: lib.mb_manifold_cover(p, 0, 8, 4, p, -1, 8, 4, 4, p, p, p, None),
        lambda: lib.mb_manifold_cover(p, 0, 0, 4, p, 0, 8, 4, 4, p, p, p, None),
        lambda: lib.mb_manifold_cover(p, 0, 8, 4, p, 0, 0, 4, 4, p, p, p, None),
        lambda: lib.mb_manifold_cover(p, 0, 1 << 23, 4, p, 0, (1 << 23) + 1, 4, 4, p, p, p, None),
        lambda: lib.mb_manifold_cover(p, 0, 8, 4, p, 0, 8, 4, 0, p, p, p, None),
        lambda: lib.mb_manifold_cover(p, 0, 8, 3, p, 0, 8, 4, 4, p, p, p, None),     # a stride < D
        lambda: lib.mb_manifold_cover(p, 0, 8, 4, p, 0, 8, 3, 4, p, p, p, None),
        lambda: lib.mb_manifold_cover(p + 2, 0, 8, 4, p, 0, 8, 4, 4, p, p, p, None),
        lambda: lib.mb_manifold_cover(p, 0, 8, 4, p + 4, 1, 8, 4, 4, p, p, p, None),
        lambda: lib.mb_manifold_cover(p, 0, 8, 4, p, 0, 8, 4, 4, p + 4, p, p, None),
        lambda: lib.mb_manifold_cover(p, 0, 8, 4, p, 0, 8, 4, 4, p, p, p + 4, None),
    ]
    for calls, prefix in ((knn, "mb_knn_radii:"), (cover, "mb_manifold_cover:")):
        for i, call in enumerate(calls):
            assert call() == -1, (prefix, i)
            assert lib.mb_last_error().decode().startswith(prefix), (prefix, i)


def test_surface():
    import maskbit_amd
    from maskbit_amd import GeneratorEvaluator, InceptionV3, manifold
    for name in ("knn_radii", "manifold_coverage", "precision_recall"):
        assert name in maskbit_amd.__all__ and getattr(maskbit_amd, name) is getattr(manifold, name)
    assert list(inspect.signature(manifold.knn_radii).parameters) == ["features", "k"]
    assert list(inspect.signature(manifold.manifold_coverage).parameters) == ["queries", "base", "radii2"]
    assert list(inspect.signature(manifold.precision_recall).parameters) == ["reference_features", "sample_features", "k"]
    assert inspect.signature(manifold.knn_radii).parameters["k"].default == 3
    # the classes the feature adds to keep what they had
    p = inspect.signature(GeneratorEvaluator.__init__).parameters
    assert list(p) == ["self", "device", "enable_fid", "enable_inception_score", "enable_codebook_usage_measure", "enable_codebook_entropy_measure",
                       "test_resolution", "num_codebook_entries"]
    assert list(inspect.signature(GeneratorEvaluator.update_features).parameters)[:4] == ["self", "pool", "logits", "codebook_indices"]
    assert list(inspect.signature(GeneratorEvaluator.use_inception).parameters) == ["self", "extractor", "real_statistics"]
    assert list(inspect.signature(InceptionV3.__init__).parameters) == ["self", "features_list"]
    q = inspect.signature(GeneratorEvaluator.use_precision_recall).parameters
    assert list(q) == ["self", "reference_features", "k", "max_samples"] and q["k"].default == 3 and q["max_samples"].default is None


def test_no_cpu_path():
    from maskbit_amd import knn_radii, manifold_coverage, precision_recall
    x = torch.zeros(8, 4)
    for call in (lambda: knn_radii(x), lambda: manifold_coverage(x, x, torch.zeros(8, dtype=torch.float64)), lambda: precision_recall(x, x)):
        with pytest.raises(RuntimeError, match="no CPU path"):
            call()


def test_restatement_closed_forms():
    rng = np.random.default_rng(0)
    a = rng.standard_normal((40, 6)).astype(np.float32)
    assert M.precision_recall(a, a.copy(), 3) == (1.0, 1.0)             # identical sets: every row is at distance 0 from a row of the other
    b = a + np.float32(1000.0)
    assert M.precision_recall(a, b, 3) == (0.0, 0.0)                     # disjoint far sets
    # radii by hand: points 0, 3, 4, 5, 12 on a line
    x = np.zeros((5, 2)); x[:, 0] = (0, 3, 4, 5, 12)
    assert M.knn_radii(x, 1).tolist() == [9.0, 1.0, 1.0, 1.0, 49.0] and M.knn_radii(x, 2).tolist() == [16.0, 4.0, 1.0, 4.0, 64.0]
    assert M.cover(np.array([[-3.0, 0], [-4.0, 0]]), x, M.knn_radii(x, 1)).tolist() == [True, False]     # `<=`: 9 <= 9 of the point at 0; 16 > 9
    e = M.pair_bound(a, a)
    assert e.shape == (40, 40) and np.allclose(e, e.T) and e[0, 1] == 2.0 * 10 * 2.0 ** -53 * ((a[0].astype(np.float64) ** 2).sum() + (a[1].astype(np.float64) ** 2).sum())
