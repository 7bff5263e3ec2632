"""CPU-only tests of the fp32 reference mode's host side (MB_PREC_F32 = 5) and of the checkpoint self-check's arithmetic: the header and the library's
exports, the precision knob's resolution, the Poisson limit and the report's logic on hand-made counts, and the recorded-run layout."""
import ctypes
import math
import os
import re

import pytest
import torch

from conftest import ROOT


def test_header_declares_the_mode_and_keeps_the_abi_version():
    from maskbit_amd import _lib
    abi = open(os.path.join(ROOT, "include", "maskbit_hip.h")).read()
    assert re.search(r"\bMB_PREC_F32 = 5\b", abi)
    assert re.search(r"#define MB_ABI_VERSION 8\b", abi) and _lib.ABI_VERSION == 8               # additions only
    diag = open(os.path.join(ROOT, "include", "maskbit_hip_diag.h")).read()
    assert re.search(r"\bint mb_gemm_f32\(", diag) and re.search(r"\bint mb_attention_f32\(", diag)


def test_library_exports_the_two_diag_entries():
    from maskbit_amd import _lib
    raw = ctypes.CDLL(_lib.LIB_PATH)
    for name in ("mb_gemm_f32", "mb_attention_f32"):
        assert hasattr(raw, name) and name in _lib.SIGNATURES
    assert len(_lib.SIGNATURES["mb_gemm_f32"][1]) == 12 and len(_lib.SIGNATURES["mb_attention_f32"][1]) == 7


def test_resolved_precision_is_5_for_any_shape_and_never_automatic(monkeypatch):
    from maskbit_amd import LFQBert
    from maskbit_amd import bert
    assert bert.PREC_F32 == 5
    tiny = LFQBert(hidden_dim=128, codebook_size=4096, codebook_splits=2, depth=2, heads=4, mlp_dim=256, nclass=10)
    full = LFQBert(img_size=256, hidden_dim=1024, codebook_size=4096, codebook_splits=2, depth=24, heads=16, mlp_dim=4096)
    for m in (tiny, full):
        m.precision = 5
        assert m.resolved_precision() == 5                          # the "shape not capable -> PREC_DIFF" fallback does not touch it
        m.precision = -1
        assert m.resolved_precision() in (1, 2, 3, 4)               # the auto rule never selects the reference mode
    monkeypatch.setenv("MASKBIT_AMD_PRECISION", "5")
    env = LFQBert(hidden_dim=128, codebook_size=4096, codebook_splits=2, depth=2, heads=4, mlp_dim=256, nclass=10)
    assert env.precision == 5 and env.resolved_precision() == 5


def test_poisson_upper_limit():
    from maskbit_amd.checkpoint_check import poisson_upper_limit
    assert poisson_upper_limit(0) == pytest.approx(2.996, rel=1e-3)                 # -ln(0.05)
    assert poisson_upper_limit(0) == pytest.approx(-math.log(0.05), rel=1e-9)
    # known one-sided 95 % limits (chi-square quantiles / 2)
    assert poisson_upper_limit(1) == pytest.approx(4.744, rel=1e-3)
    assert poisson_upper_limit(10) == pytest.approx(16.962, rel=1e-3)
    lim = [poisson_upper_limit(k) for k in (0, 1, 2, 3, 5, 8, 13, 50, 200, 1000)]
    assert all(b > a for a, b in zip(lim, lim[1:]))                                  # monotone in k
    assert all(l > k for l, k in zip(lim, (0, 1, 2, 3, 5, 8, 13, 50, 200, 1000)))
    assert poisson_upper_limit(1000) == pytest.approx(1000 + 1.645 * math.sqrt(1000), rel=5e-3)   # the normal limit


def test_report_logic_on_hand_made_counts():
    from maskbit_amd.checkpoint_check import CheckpointReport
    n = 100_000
    rep = CheckpointReport.from_counts({2: (120, n), 3: (80, n), 4: (30, n)}, auto_precision=2, bound=1e-3)
    # 120 / 1e5 = 1.2e-3 is over the bound; 80: the upper limit 95.9 / 1e5 holds; 30 holds
    assert rep.holds == {2: False, 3: True, 4: True}
    assert rep.recommended == 3 and rep.default_ok is False
    assert rep.results[3].rate == pytest.approx(8e-4) and rep.results[3].upper_limit == pytest.approx(95.9e-5, rel=5e-3)
    # a rate under the bound whose upper limit is not: 90 -> 106.6
    rep = CheckpointReport.from_counts({2: (90, n), 4: (0, n)}, auto_precision=4, bound=1e-3)
    assert rep.results[2].rate < 1e-3 and rep.holds == {2: False, 4: True}
    assert rep.recommended == 4 and rep.default_ok is True
    assert rep.results[4].upper_limit == pytest.approx(2.996 / n, rel=1e-3)
    rep = CheckpointReport.from_counts({0: (500, n), 1: (400, n)}, auto_precision=1, bound=1e-3)
    assert rep.recommended is None and rep.default_ok is False
    rep = CheckpointReport.from_counts({0: (1, n)}, auto_precision=2)
    assert rep.default_ok is None and rep.recommended == 0                            # the auto precision was not among those checked
    text = str(rep)
    assert "recommended precision: 0" in text and "95% upper" in text


def test_recorded_run_round_trips_through_tokens_in():
    """The record layout is parity_replay.load_run's: tokens_in(g, i) rebuilds step i's input from the previous step's predictions and step i's mask."""
    from maskbit_amd import parity_replay
    from maskbit_amd.checkpoint_check import record_dict
    S, B, n, m, C_ = 4, 2, 9, 3, 8
    gen = torch.Generator().manual_seed(5)
    inputs, steps, masks = [], [], []
    tin = torch.full((B, n, m), C_, dtype=torch.int64)
    for i in range(S):
        inputs.append(tin)
        msk = tin == C_
        pred = torch.where(msk, torch.randint(0, C_, tin.shape, generator=gen), tin)       # known tokens are kept, masked ones predicted
        steps.append(pred); masks.append(msk)
        remask = (torch.rand(tin.shape, generator=gen) < 0.5 * (1 - (i + 1) / S)) & msk     # the next input re-masks some of this step's positions
        tin = torch.where(remask, torch.full_like(pred, C_), pred)
    kw = dict(num_steps=S, guidance_scale=0.0, guidance_annealing="none", scale_pow=4.0, randomize_temperature=4.5, mask_schedule_strategy="arccos")
    g = record_dict(torch.stack(steps), torch.stack(masks), torch.arange(B), kw, seed=3, bits=9, C=C_)
    assert set(("steps", "masks", "labels", "kw", "seed", "bits", "C", "n")) <= set(g)
    assert g["n"] == n and g["C"] == C_ and g["kw"]["num_steps"] == "4" and all(isinstance(v, str) for v in g["kw"].values())
    for i in range(S):
        assert torch.equal(parity_replay.tokens_in(g, i), inputs[i]), i
    # the noise and the plan follow the record's own group count and codebook
    q, c = parity_replay.reference_noise(g, "cpu")
    assert q.shape == (S, B * n * m, C_) and c.shape == (S, B, n, m)
    scale, temp, mask_len = parity_replay.plan_of(g)
    assert len(mask_len) == S and max(mask_len) <= n * m and all(s == 0.0 for s in scale)


def test_teacher_forced_noise_of_the_recorded_runs_is_unchanged():
    """reference_noise generalised over the group count draws what it drew: the reference's order and shapes for the two-group fixtures."""
    from maskbit_amd import parity_replay
    g = {"steps": torch.zeros((2, 3, 4, 2), dtype=torch.int64), "kw": {"randomize_temperature": "2.0"}, "seed": 11, "C": 8}
    q, c = parity_replay.reference_noise(g, "cpu")
    torch.manual_seed(11)
    gum = torch.distributions.Gumbel(0.0, 1.0)
    for i in range(2):
        assert torch.equal(q[i], torch.empty(3 * 4 * 2, 8).exponential_(1))
        assert torch.equal(c[i], gum.sample((3, 4, 2)) * 2.0 * (1 - (i + 1) / 2))
