"""CPU checks of masked-token validation: the float64 restatement of tests/mlm_reference.py against the reference's recorded results
(tests/golden/mlm.npz, tools/make_golden_mlm.py), the host-side mask schedule bit for bit, the C ABI additions and the reference's import path.
The restatement is the yardstick tests/test_hip_mlm.py uses for inputs that have no golden."""
import ctypes
import inspect
import os
import re

import numpy as np
import pytest
import torch

from conftest import ROOT
from mlm_reference import CONFIGS, KEYS, loss_bound, loss_case, mask_case, mask_tokens_ref, mlm_golden, mlm_loss64, unpack_mask

LOSS_CASES = [str(n) for n in mlm_golden()["loss_cases"]]
MASK_CASES = [str(n) for n in mlm_golden()["mask_cases"]]
ENTRIES = ("mb_mlm_workspace_bytes", "mb_mlm_state_bytes", "mb_mlm_mask", "mb_mlm_loss")


def test_golden_covers_the_issue_cases():
    z = mlm_golden()
    shapes = [tuple(int(v) for v in z[n + ".params"][:4]) for n in LOSS_CASES]
    assert shapes == [(3, 16, 2, 64), (2, 256, 2, 128), (2, 16, 1, 1024), (3, 7, 3, 16), (2, 16, 2, 512), (3, 16, 1, 10), (2, 8, 1, 4100)]
    assert [tuple(c) for c in z["configs"]] == [(ls, float(ss)) for ls, ss in CONFIGS] == [(0.1, 0.0), (0.0, 1.0), (0.1, 1.0)]
    seen = {(tuple(int(v) for v in z[n + ".params"][:3]), str(z[n + ".mode"]), float(z[n + ".min_masking_ratio"])) for n in MASK_CASES}
    for shape in ((5, 16, 2), (3, 256, 3)):
        for mode, lo in (("linear", 0.0), ("square", 0.0), ("cosine", 0.0), ("arccos", 0.0), ("arccos", 0.5)):
            assert (shape, mode, lo) in seen
    for n in LOSS_CASES:                                             # a masked and an unmasked row in every case; accuracies not degenerate
        rows, masked, correct, masked_correct = (int(v) for v in z[n + ".counts"])
        assert 0 < masked < rows and 0 < correct < rows and 0 < masked_correct < masked
        e = z[n + ".E_rel"]
        assert e.shape == (3, 2) and np.array_equal(e, np.abs(z[n + ".ref32"][:, [0, 2]] - z[n + ".ref64"][:, [0, 2]]) / np.abs(z[n + ".ref64"][:, [0, 2]]))
    assert 1e-8 < loss_bound() / 4.0 < 1e-6                          # the reference's own fp32 error: a few ulps of a float32 mean


@pytest.mark.parametrize("name", LOSS_CASES)
def test_fp64_restatement_reproduces_ref64(name):
    z = mlm_golden()
    logits, targets, mask = loss_case(name)
    top2 = logits.topk(2, dim=-1).values
    assert bool((top2[..., 0] > top2[..., 1]).all())                 # the condition on the inputs: no row with two equal largest logits
    for i, (ls, ss) in enumerate(CONFIGS):
        r = mlm_loss64(logits, targets, mask, ls, ss)
        ref = z[name + ".ref64"][i]
        for k, key in enumerate(KEYS):
            # the two losses are float64 in ref64; the two accuracies are not -- the reference forms ``.float().mean() ** m`` in float32 whatever
            # the logits' dtype (losses.py:322,326) -- so they are held to 4 float32 ulps here and pinned exactly by the counts below
            tol = 1e-12 if key.endswith("loss") else 4 * 2.0 ** -24
            assert abs(r[key] - ref[k]) <= tol * abs(ref[k]), (key, r[key], ref[k])
        assert [r["rows"], r["masked"], r["correct"], r["masked_correct"]] == [int(v) for v in z[name + ".counts"]]


@pytest.mark.parametrize("name", MASK_CASES)
def test_host_mask_schedule_is_the_references_bit_for_bit(name):
    from maskbit_amd.validation import mask_thresholds
    z = mlm_golden()
    tokens, mask_token, mode, lo, seed = mask_case(name)
    gold = z[name + ".val_to_mask"]
    assert gold.dtype == np.float32
    torch.manual_seed(seed)                                          # the global CPU generator, as a reference script seeds it
    val = mask_thresholds(tokens.shape[0], mode, lo)
    assert val.dtype == torch.float32 and np.array_equal(val.numpy(), gold)
    val = mask_thresholds(tokens.shape[0], mode, lo, generator=torch.Generator().manual_seed(seed))      # or an explicit one
    assert np.array_equal(val.numpy(), gold)
    # and the restatement, continuing the same stream, masks the slots the reference masked
    masked, mask, val = mask_tokens_ref(tokens, mask_token, mode, lo, generator=torch.Generator().manual_seed(seed))
    assert np.array_equal(val.numpy(), gold) and torch.equal(mask, unpack_mask(z[name + ".mask"], tokens.shape))
    assert torch.equal(masked, torch.where(mask, torch.full_like(tokens, mask_token), tokens))


def test_invalid_mode_raises_and_cpu_tokens_raise():
    from maskbit_amd import get_mask_tokens
    from maskbit_amd.validation import mask_thresholds
    tokens = torch.zeros(2, 4, 2, dtype=torch.int64)
    for bad in ("root", "cubic", ""):
        with pytest.raises(ValueError, match="Invalid mode. Choose between 'linear','square', 'cosine', 'arccos'."):
            get_mask_tokens(tokens, 64, mode=bad)
        with pytest.raises(ValueError, match="Invalid mode"):
            mask_thresholds(2, bad)
    with pytest.raises(RuntimeError, match="no CPU path"):
        get_mask_tokens(tokens, 64)
    from maskbit_amd import MLMLoss, MaskedTokenEvaluator
    with pytest.raises(RuntimeError, match="no CPU path"):
        MLMLoss()(torch.zeros(2, 4, 2, 8), tokens, tokens.bool())
    with pytest.raises(RuntimeError, match="no CPU path"):
        MaskedTokenEvaluator().update(torch.zeros(2, 4, 2, 8), tokens, tokens.bool())
    with pytest.raises(ValueError, match="No examples"):
        MaskedTokenEvaluator().result()
    for shape_err in ((torch.zeros(2, 4, 8), tokens, tokens.bool()), (torch.zeros(2, 4, 2, 8), tokens[:1], tokens.bool()),
                      (torch.zeros(2, 4, 2, 8), tokens.float(), tokens.bool()), (torch.zeros(2, 4, 2, 1), tokens, tokens.bool())):
        with pytest.raises(ValueError):
            MLMLoss()(*shape_err)
    with pytest.raises(ValueError):
        MLMLoss(label_smoothing=1.5)


def test_reference_import_path_and_signatures():
    from modeling.modules import get_mask_tokens, MLMLoss
    import maskbit_amd
    assert get_mask_tokens is maskbit_amd.get_mask_tokens and MLMLoss is maskbit_amd.MLMLoss
    for name in ("get_mask_tokens", "MLMLoss", "MaskedTokenEvaluator", "eval_masked_prediction"):
        assert name in maskbit_amd.__all__
    p = inspect.signature(get_mask_tokens).parameters
    assert list(p) == ["tokens", "mask_token", "mode", "min_masking_ratio", "generator"]                    # masking.py:7-12 + generator
    assert p["mode"].default == "arccos" and p["min_masking_ratio"].default == 0.0 and p["generator"].kind is inspect.Parameter.KEYWORD_ONLY
    for cls in (MLMLoss, maskbit_amd.MaskedTokenEvaluator):
        q = inspect.signature(cls.__init__).parameters
        assert list(q) == ["self", "label_smoothing", "sum_splits"] and q["label_smoothing"].default == 0.1 and q["sum_splits"].default is False
    assert list(inspect.signature(MLMLoss.forward).parameters) == ["self", "inputs", "targets", "masks"]      # losses.py:302-307
    loss = MLMLoss(0.05, True)
    assert isinstance(loss, torch.nn.Module) and loss.label_smoothing == 0.05 and loss.sum_splits is True
    assert "inference only" in MLMLoss.__doc__.lower()
    e = inspect.signature(maskbit_amd.eval_masked_prediction).parameters
    assert list(e) == ["model", "vqgan_model", "loader", "evaluator", "mask_schedule_strategy", "min_masking_ratio", "class_label_dropout", "generator"]
    assert all(e[k].kind is inspect.Parameter.KEYWORD_ONLY for k in list(e)[4:])


def test_abi_declares_and_binds_the_mlm_entries():
    from maskbit_amd import _lib
    header = open(os.path.join(ROOT, "include", "maskbit_hip.h")).read()
    assert re.search(r"#define MB_ABI_VERSION 8\b", header)
    raw = ctypes.CDLL(_lib.LIB_PATH)
    for name in ENTRIES:
        assert re.search(r"\b" + name + r"\(", header), name
        assert name in _lib.SIGNATURES
        getattr(raw, name)
    lib = _lib.load()
    assert lib.mb_abi_version() == 8 == _lib.ABI_VERSION
    assert lib.mb_mlm_state_bytes() == 37 * 8
    ws = lib.mb_mlm_workspace_bytes
    # one 48-byte slot per workgroup and per sample; the split of a sample's rows depends on (n * m, C) alone
    assert ws(1, 256, 2, 64) > 0 and (ws(64, 256, 2, 64) - 64 * 48) == 64 * (ws(1, 256, 2, 64) - 48)
    assert ws(3, 7, 3, 16) == 3 * 2 * 48                                        # 21 rows: one workgroup per sample
    assert ws(2, 8, 1, 4100) == 2 * 48 * (2 + 1)                                # 4 rows per workgroup at C >= 1024
    assert ws(0, 16, 2, 64) == 0 and ws(1, 16, 2, 1) == 0 and ws(70000, 16, 2, 64) == 0
    assert "mlm.hip" in __import__("maskbit_amd.build", fromlist=["SOURCES"]).SOURCES


def test_host_side_error_paths_of_the_entries():
    from maskbit_amd import _lib
    lib = _lib.load()
    assert lib.mb_mlm_mask(None, None, None, 64, None, None, 1, 16, 2, None) != 0 and b"null" in lib.mb_last_error()
    assert lib.mb_mlm_loss(None, None, None, 0.1, 1, 16, 2, 64, None, None, None, None, None) != 0 and b"null" in lib.mb_last_error()
    assert lib.mb_mlm_loss(16, 16, 16, 0.1, 1, 16, 2, 1, 16, None, None, None, None) != 0 and b"C >= 2" in lib.mb_last_error()
    assert lib.mb_mlm_loss(16, 16, 16, 1.5, 1, 16, 2, 64, 16, None, None, None, None) != 0 and b"label_smoothing" in lib.mb_last_error()
    assert lib.mb_mlm_mask(16, 16, 16, 64, 16, 16, 1, 16, 2, None) != 0 and b"alias" in lib.mb_last_error()
