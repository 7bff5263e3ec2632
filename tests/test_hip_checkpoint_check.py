"""maskbit_amd.check_checkpoint on the GPU: the self-recorded fp32 run in the place of the reference's recorded one."""
import math

import pytest
import torch

from conftest import load_golden, golden_weights
from hip_helpers import hip_generator
from oracle import maskbit_oracle as O

pytestmark = pytest.mark.gpu
DEV = "cuda"
TINY_GEN = O.GenCfg(bits=12, splits=2, hidden=128, depth=2, heads=4, mlp=256, seq=256, nclass=10)


def test_self_check_agrees_with_the_replay_of_the_reference_run():
    """The weights, labels, seed and sampler settings of the reference's recorded run sample_full10_16_nocfg: the noise is then the fixture's, and the
    record differs from the fixture only where the engine's fp32 and the reference's fp32 fall on different sides of a near-tie.  The precision-2
    count against the self-recorded run must agree with the count against the fixture within 3 sqrt(c) + 3 -- and be equal if the record reproduces
    the fixture bit for bit (which of the two happened: profiles/f32_reference.md)."""
    from maskbit_amd import check_checkpoint, parity_replay
    run = parity_replay.RUN_CFG1
    gen, _ = parity_replay.build_models(DEV, with_tokenizer=False, name=run)
    g = parity_replay.load_run(run)
    kw = {k: (v if k in ("guidance_annealing", "mask_schedule_strategy") else (int(v) if k == "num_steps" else float(v))) for k, v in g["kw"].items()}
    gen.precision = 3                                                       # a setting of the caller's own: must survive the check
    rep = check_checkpoint(gen, num_samples=g["labels"].numel(), labels=g["labels"], seed=g["seed"], precisions=(0, 2), **kw)
    assert gen.precision == 3
    print(rep)
    gen.precision = 2
    c_fix, total, _, _ = parity_replay.teacher_forced(gen, g=g)
    rec = rep.record
    same = torch.equal(rec["steps"], g["steps"]) and torch.equal(rec["masks"], g["masks"])
    c_self = rep.results[2].mismatches
    print(f"precision 2: {c_self} mismatches against the self-recorded run, {c_fix} against the fixture, over {total} positions; "
          f"record == fixture bit for bit: {same} ({int((rec['steps'] != g['steps']).sum())} tokens differ)")
    assert rep.results[2].positions == total or not same
    assert abs(c_self - c_fix) <= 3 * math.sqrt(c_fix) + 3
    if same:
        assert c_self == c_fix
    assert rep.results[0].rate >= rep.results[2].rate
    assert rep.auto_precision == 2 and rep.default_ok == rep.holds[2] and rep.weight_statistics["heavy_tailed"] is False
    assert rep.results[2].saturation == 0 and rep.results[2].seconds > 0 and len(rep.results[2].per_step) == 16
    text = str(rep)
    assert "recommended precision" in text and "auto" in text


def test_tiny_model_runs_the_check_the_mode_is_shape_generic():
    """hidden 128, heads of 32, no pair or mini tiles: the fp32 mode and the check serve it like any other shape."""
    from maskbit_amd import check_checkpoint
    m = hip_generator(TINY_GEN, golden_weights(load_golden("gen_tiny.npz")))
    m.precision = -1
    rep = check_checkpoint(m, num_samples=3, precisions=(0, 1), num_steps=8)
    print(rep)
    assert set(rep.results) == {0, 1} and rep.auto_precision == 1
    assert all(r.positions > 0 and 0 <= r.mismatches <= r.positions for r in rep.results.values())
    assert rep.default_ok == rep.holds[1] and rep.record["steps"].shape == (8, 3, 256, 2)
    assert m.precision == -1
