"""CPU tests of per-sample sampling arguments (include/maskbit_hip.h "per-sample sampling arguments"): the host-side plan of a requests run against
``seeded_plan`` and the conf-weight expression of the seeded run, bit for bit; the refusals of the Python entries and of the library's entries, none
of which needs a device; the header and the public surface."""
import ctypes
import dataclasses
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("mb_sample_step_requests", "mb_sample_requests")


def f32_bits(values):
    """The float32 bit patterns of Python floats, rounded once as ctypes' c_float does."""
    return [ctypes.c_uint32.from_buffer(ctypes.c_float(v)).value for v in values]


def five_requests():
    """N = (8, 3, 5, 8, 1): all three annealings, sampling annealing on and off, two schedules; one scale 0."""
    from maskbit_amd import SampleRequest
    return [SampleRequest(seed=11, label=1, num_steps=8, guidance_scale=7.1, guidance_annealing="cosine", scale_pow=3.0, randomize_temperature=8.2,
                          mask_schedule_strategy="arccos"),
            SampleRequest(seed=2 ** 64 - 3, label=4, num_steps=3, guidance_scale=0.0, softmax_temperature=0.7, randomize_temperature=2.5),
            SampleRequest(seed=2 ** 63, label=8, num_steps=5, guidance_scale=2.5, guidance_annealing="linear", use_sampling_annealing=True,
                          mask_schedule_strategy="arccos"),
            SampleRequest(seed=0, label=0, num_steps=8, guidance_scale=4.0, guidance_annealing="none", softmax_temperature=1.3, randomize_temperature=6.0),
            SampleRequest(seed=999, label=9, num_steps=1, guidance_scale=1.5, guidance_annealing="cosine", use_sampling_annealing=True)]


def test_plan_table_equals_the_seeded_plan_of_every_request():
    from maskbit_amd.sampling import REQUEST_COLUMNS, build_request_plan, seeded_plan
    reqs = five_requests()
    order, active, table = build_request_plan(reqs)
    assert order == [0, 3, 2, 1, 4]                                                                 # N descending; the two 8s keep request order
    assert active == [2, 2, 2, 3, 3, 4, 4, 5]
    S, B = 8, 5
    assert table.dtype == torch.int32 and tuple(table.shape) == (S, B, 6) and table.device.type == "cpu" and table.is_contiguous()
    assert REQUEST_COLUMNS == ("scale", "temperature", "mask_ratio", "randomize_temperature", "conf_weight", "step")
    seen_active = 0
    for p, b in enumerate(order):
        r = reqs[b]
        N = r.num_steps
        scale, temp, ratio = seeded_plan(N, r.guidance_scale, r.guidance_annealing, r.scale_pow, r.softmax_temperature, r.use_sampling_annealing,
                                         r.mask_schedule_strategy)
        for t in range(S):
            rec = [v & 0xFFFFFFFF for v in table[t, p].tolist()]
            i = t - (S - N)
            assert (p < active[t]) == (i >= 0)
            if i < 0:
                assert rec == [0, 0, 0, 0, 0, 0xFFFFFFFF], (t, p)                                   # inactive: step = -1
                continue
            want = f32_bits([scale[i], temp[i], ratio[i], r.randomize_temperature, 1 - (i + 1) / N]) + [i]
            assert rec == want, (t, p, rec, want)
            seen_active += 1
    assert seen_active == sum(r.num_steps for r in reqs) == sum(active)
    # the cosine request's first step has scale 0 (and the last step's conf weight is 0 for everyone)
    f = table.view(torch.float32)
    assert float(f[0, 0, 0]) == 0.0 and float(f[1, 0, 0]) != 0.0 and f[S - 1, :, 4].tolist() == [0.0] * B


def test_ties_in_num_steps_keep_request_order():
    from maskbit_amd import SampleRequest
    from maskbit_amd.sampling import build_request_plan
    reqs = [SampleRequest(seed=b, label=0, num_steps=N) for b, N in enumerate((2, 4, 2, 4, 4, 1, 2))]
    order, active, table = build_request_plan(reqs)
    assert order == [1, 3, 4, 0, 2, 6, 5]
    assert active == [3, 3, 6, 7]
    assert table[:, :, 5].tolist() == [[0, 0, 0, -1, -1, -1, -1], [1, 1, 1, -1, -1, -1, -1], [2, 2, 2, 0, 0, 0, -1], [3, 3, 3, 1, 1, 1, 0]]
    order1, active1, table1 = build_request_plan(reqs[:1])
    assert order1 == [0] and active1 == [1, 1] and tuple(table1.shape) == (2, 1, 6)


def test_python_entries_refuse_bad_fields_before_any_device_work():
    """On CPU-resident models: a request's fields are checked before the device is asked for (which would raise RuntimeError)."""
    from maskbit_amd import ConvVQModel, LFQBert, SampleRequest, sample_requests
    from maskbit_amd.sampling import build_request_plan
    from hip_helpers import tok_config
    from test_edit_cpu import TINY_GEN, TINY_TOK
    gm = LFQBert(img_size=256, hidden_dim=TINY_GEN.hidden, codebook_size=2 ** TINY_GEN.bits, codebook_splits=TINY_GEN.splits, depth=TINY_GEN.depth,
                 heads=TINY_GEN.heads, mlp_dim=TINY_GEN.mlp, dropout=0.1, nclass=TINY_GEN.nclass, input_stride=16)
    tm = ConvVQModel(tok_config(TINY_TOK))
    good = SampleRequest(seed=1, label=2)
    with pytest.raises(dataclasses.FrozenInstanceError):
        good.seed = 2
    for field, value in (("num_steps", 0), ("num_steps", -3), ("num_steps", 2.0), ("guidance_annealing", "quadratic"), ("mask_schedule_strategy", "zigzag"),
                         ("seed", -1), ("seed", 2 ** 64), ("seed", 1.5)):
        bad = dataclasses.replace(good, **{field: value})
        with pytest.raises(ValueError):
            build_request_plan([good, bad])
        with pytest.raises(ValueError):
            sample_requests(gm, tm, [good, bad])
    with pytest.raises(ValueError):
        build_request_plan([])
    with pytest.raises(ValueError, match="guided=False"):
        sample_requests(gm, tm, [good, dataclasses.replace(good, guidance_scale=0.0)], guided=False)
    with pytest.raises(ValueError, match="init_tokens"):
        sample_requests(gm, tm, [good], init_tokens=torch.full((2, 256, 2), 64, dtype=torch.int64))
    with pytest.raises(RuntimeError, match="runs only on an AMD GPU"):                              # a good call gets as far as the device
        sample_requests(gm, tm, [good])


def test_library_entries_refuse_bad_arguments_without_a_gpu():
    """The checks in front of every launch, each with its own message.  (2 B or B beyond the engine needs a handle: tests/test_hip_requests.py.)"""
    from maskbit_amd import _lib
    lib = _lib.load()
    buf = (ctypes.c_int64 * 64)()
    a = ctypes.addressof(buf)
    b = a + 128

    def refused(rc, text):
        assert rc < 0 and text in lib.mb_last_error().decode(), (rc, lib.mb_last_error())

    step = lambda **kw: lib.mb_sample_step_requests(*[kw.get(k, d) for k, d in (
        ("lc", a), ("lu", None), ("row", a), ("seeds", a), ("num_regen", a), ("tin", a), ("tout", b), ("pred", None), ("B", 1), ("n", 2), ("m", 1),
        ("C", 4), ("stream", None))])
    for name in ("row", "seeds", "num_regen", "lc", "tin", "tout"):
        refused(step(**{name: None}), "null argument")
    refused(step(tout=a), "must not alias")
    refused(step(pred=b), "pred_out must not alias")
    refused(step(B=0), "bad sizes")
    refused(step(C=8192), "too large")
    refused(step(n=8193), "too large")

    def run(active=(1, 2, 2), B=2, **kw):
        arr = (ctypes.c_int * len(active))(*active)
        plan = _lib.RequestPlan(len(active), kw.pop("guided", 0), None if kw.pop("no_active", False) else arr, kw.pop("table", a))
        return lib.mb_sample_requests(*[kw.get(k, d) for k, d in (
            ("g", None), ("d", None), ("plan", ctypes.byref(plan)), ("labels", a), ("B", B), ("init", None), ("seeds", a), ("steps", None),
            ("codes", None), ("img", None), ("u8", None), ("stream", None))])
    _lib.prof_enable(True)                                                                          # (a launch, or a forward, would leave a record)
    try:
        refused(run(plan=None), "null argument")
        refused(run(no_active=True), "null argument")
        refused(run(table=None), "null argument")
        refused(run(labels=None), "null argument")
        refused(run(seeds=None), "null argument")
        refused(run(), "null argument")                                                             # everything else in order: no generator handle
        refused(run(active=(2, 1, 2)), "not non-decreasing")
        refused(run(active=(0, 2, 2)), "outside [1, 2]")
        refused(run(active=(1, 2, 3)), "outside [1, 2]")
        refused(run(active=(1, 1, 1)), "all 2 requests run the last step")
        refused(run(img=a), "image requested without a decoder")
        refused(run(u8=a), "image requested without a decoder")
        assert _lib.prof_read() == {}
    finally:
        _lib.prof_enable(False)


def test_header_declares_and_exports():
    import maskbit_amd
    from maskbit_amd import SampleRequest, _lib, sample_requests, sample_seeded
    import inspect
    abi = open(os.path.join(ROOT, "include", "maskbit_hip.h")).read()
    assert re.search(r"#define MB_ABI_VERSION 8\b", abi) and _lib.ABI_VERSION == 8 and _lib.load().mb_abi_version() == 8   # additions only
    raw = ctypes.CDLL(_lib.LIB_PATH)
    for name in ENTRIES:
        assert re.search(r"\b%s\s*\(" % name, abi) and name in _lib.SIGNATURES
        getattr(raw, name)
    assert len(_lib.SIGNATURES["mb_sample_step_requests"][1]) == 13 and len(_lib.SIGNATURES["mb_sample_requests"][1]) == 12
    assert "} mb_request_step;" in abi and "} mb_request_plan;" in abi
    assert ctypes.sizeof(_lib.RequestStep) == 24 and [f[0] for f in _lib.RequestStep._fields_] == list(maskbit_amd.sampling.REQUEST_COLUMNS)
    flat = re.sub(r"\s*\n \*\s*", " ", abi)
    for text in ("RIGHT-ALIGNED", "i = t - (S - N_b)", "c + 0 * (c - u)", "THIS DIFFERS from mb_sample_seeded", "sum_b N_b sequence-forwards"):
        assert text in flat, text
    assert "SampleRequest" in maskbit_amd.__all__ and "sample_requests" in maskbit_amd.__all__
    fields = {f.name: f.default for f in dataclasses.fields(SampleRequest)}
    assert list(fields)[:2] == ["seed", "label"] and fields["seed"] is dataclasses.MISSING and fields["label"] is dataclasses.MISSING
    p = inspect.signature(sample_seeded).parameters
    assert {k: fields[k] for k in list(fields)[2:]} == {k: p[k].default for k in list(p)[4:]}         # the defaults of sample_seeded
    q = inspect.signature(sample_requests).parameters
    assert list(q) == ["model", "vqgan_model", "requests", "guided", "init_tokens", "return_uint8"]
    assert all(q[k].kind is inspect.Parameter.KEYWORD_ONLY for k in list(q)[3:]) and q["guided"].default is None
