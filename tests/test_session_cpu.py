"""CPU tests of the sampling session (include/maskbit_hip.h "sampling session"): the header and the exports, the refusals of the library's entries and of
``SamplingSession.submit`` (none needs a device), the ticket and queue accounting, and a pure torch restatement of the hole-fill rule -- the yardstick
the GPU tests (tests/test_hip_session.py) hold the kernels to -- on hand-written cases."""
import ctypes
import dataclasses
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("mb_session_create", "mb_session_destroy", "mb_session_admit", "mb_session_due", "mb_session_active", "mb_session_tick")
DIAG_ENTRIES = ("mb_session_row_table", "mb_session_admit_rows", "mb_session_retire")


# ---- the hole-fill rule, restated ----------------------------------------------------------------------------------------------------------------
def hole_fill(done):
    """done: bool [A], row r finished.  -> (finished rows ascending, sources, destinations, A'): A' = A - |F|; the holes are the finished rows below
    A', the movers the unfinished rows at or above A', both ascending; mover j goes to hole j."""
    done = torch.as_tensor(done, dtype=torch.bool)
    A = int(done.numel())
    rows = torch.arange(A)
    fin = rows[done]
    Ap = A - int(fin.numel())
    dst = rows[done & (rows < Ap)]
    src = rows[~done & (rows >= Ap)]
    assert dst.numel() == src.numel()
    return fin.tolist(), src.tolist(), dst.tolist(), Ap


def compact(done, fields):
    """fields: {name: tensor [A, ...]} -> the same fields of the A' surviving rows after the moves (rows [0, A') of the session's arrays)."""
    _, src, dst, Ap = hole_fill(done)
    out = {}
    for name, t in fields.items():
        t = t.clone()
        if src:
            t[torch.tensor(dst)] = t[torch.tensor(src)]                                           # (sources >= A' > destinations: disjoint)
        out[name] = t[:Ap]
    return out


DONE_PATTERNS = ("none", "all", "tail", "head", "alternating", "random")


def done_pattern(name, A, seed=0):
    rows = torch.arange(A)
    if name == "none":
        return torch.zeros(A, dtype=torch.bool)
    if name == "all":
        return torch.ones(A, dtype=torch.bool)
    if name == "tail":
        return rows >= A - (A + 1) // 2
    if name == "head":
        return rows < (A + 1) // 2
    if name == "alternating":
        return rows % 2 == 0
    return torch.rand(A, generator=torch.Generator().manual_seed(1000 + 7 * A + seed)) < 0.4


def test_hole_fill_on_hand_written_cases():
    assert hole_fill([False, False, False]) == ([], [], [], 3)                                    # nothing finished
    assert hole_fill([True, True, True]) == ([0, 1, 2], [], [], 0)                                # everything finished
    assert hole_fill([False, False, True, True]) == ([2, 3], [], [], 2)                           # only the tail: no moves
    assert hole_fill([True, True, False, False, False]) == ([0, 1], [3, 4], [0, 1], 3)            # only the head: the last two rows fill it
    assert hole_fill([True, False, True, False, True]) == ([0, 2, 4], [3], [0], 2)                # alternating: A' = 2, row 1 stays, row 3 -> 0
    assert hole_fill([False, True, False, True, False, False]) == ([1, 3], [4, 5], [1, 3], 4)
    assert hole_fill([True]) == ([0], [], [], 0) and hole_fill([False]) == ([], [], [], 1)
    vals = torch.tensor([10, 11, 12, 13, 14])
    assert compact([True, False, True, False, True], {"v": vals})["v"].tolist() == [13, 11]
    assert compact([True, True, False, False, False], {"v": vals})["v"].tolist() == [13, 14, 12]
    assert compact([False, False, True, True, False], {"v": vals})["v"].tolist() == [10, 11, 14]
    for A in (1, 2, 3, 65, 130):
        for name in DONE_PATTERNS:
            done = done_pattern(name, A)
            fin, src, dst, Ap = hole_fill(done)
            assert Ap == A - len(fin) and all(s >= Ap > d for s, d in zip(src, dst))
            kept = compact(done, {"r": torch.arange(A)})["r"].tolist()
            assert sorted(kept) == [r for r in range(A) if not bool(done[r])]                     # every survivor exactly once


# ---- header, bindings, exports ---------------------------------------------------------------------------------------------------------------------
def test_header_declares_and_exports():
    import maskbit_amd
    from maskbit_amd import _lib
    abi = open(os.path.join(ROOT, "include", "maskbit_hip.h")).read()
    diag = open(os.path.join(ROOT, "include", "maskbit_hip_diag.h")).read()
    assert re.search(r"#define MB_ABI_VERSION 8\b", abi) and _lib.ABI_VERSION == 8 and _lib.load().mb_abi_version() == 8   # additions only
    raw = ctypes.CDLL(_lib.LIB_PATH)
    for name, text in [(e, abi) for e in ENTRIES] + [(e, diag) for e in DIAG_ENTRIES]:
        assert re.search(r"\b%s\s*\(" % name, text) and name in _lib.SIGNATURES, name
        getattr(raw, name)
    assert len(_lib.SIGNATURES["mb_session_tick"][1]) == 11 and len(_lib.SIGNATURES["mb_session_admit"][1]) == 9
    assert ctypes.sizeof(_lib.SessionRows) == 7 * 8 + 2 * 4 and "} mb_session_rows;" in diag
    flat = re.sub(r"\s*\n \*\s*", " ", abi)
    for text in ("runs its local step i at tick t + i and finishes at tick t + N - 1", "IN ASCENDING ROW ORDER", "row M[j] moves to H[j]", "c + 0 * (c - u)",
                 "invalidates the cache whenever membership changed", "ends any chunked run in progress", "owns its token state", "snapshot"):
        assert text in flat, text
    assert "SamplingSession" in maskbit_amd.__all__ and "Finished" in maskbit_amd.__all__
    from maskbit_amd.build import SOURCES
    assert "session.hip" in SOURCES


def test_library_entries_refuse_bad_arguments_without_a_gpu():
    """Every check in front of the first launch (and of the first allocation): a session object is host memory until an admit passes its checks."""
    from maskbit_amd import _lib
    lib = _lib.load()
    buf = (ctypes.c_int64 * 64)()
    a = ctypes.addressof(buf)

    def refused(rc, text):
        assert rc < 0 and text in lib.mb_last_error().decode(), (rc, lib.mb_last_error())

    h = ctypes.c_void_p()
    create = lambda seq=256, splits=2, bits=12, cap=4, steps=8, out=ctypes.byref(h): lib.mb_session_create(seq, splits, bits, cap, steps, 1, out)
    _lib.prof_enable(True)                                                                         # (a launch would leave a record)
    try:
        refused(create(out=None), "null argument")
        refused(create(cap=0), "bad sizes")
        refused(create(cap=-2), "bad sizes")
        refused(create(steps=0), "bad sizes")
        refused(create(bits=13), "no generator configuration")
        refused(create(seq=8192), "no generator configuration")
        assert h.value is None
        assert create() == 0 and h.value
        try:
            assert lib.mb_session_active(h) == 0 and lib.mb_session_due(h) == 0
            assert lib.mb_session_active(None) == -1 and lib.mb_session_due(None) == -1
            tickets = (ctypes.c_uint64 * 8)()

            def admit(K=1, steps=(3,), s=h, **kw):
                arr = (ctypes.c_int * max(len(steps), 1))(*steps)
                args = dict(labels=a, seeds=a, num_steps=arr, schedule=a, init=None, tickets=tickets)
                args.update(kw)
                return lib.mb_session_admit(s, K, args["labels"], args["seeds"], args["num_steps"], args["schedule"], args["init"], args["tickets"], None)
            refused(admit(K=0), "bad sizes")
            refused(admit(K=-1), "bad sizes")
            refused(admit(K=0, s=None), "bad sizes")                                              # the same way without a session
            for name in ("labels", "seeds", "num_steps", "schedule", "tickets"):
                refused(admit(**{name: None}), "null argument")
            refused(admit(s=None), "null argument")
            refused(admit(steps=(0,)), "num_steps[0] = 0 outside [1, 8]")
            refused(admit(steps=(9,)), "num_steps[0] = 9 outside [1, 8]")
            refused(admit(K=3, steps=(8, 1, -4)), "num_steps[2] = -4 outside [1, 8]")
            refused(admit(K=5, steps=(1,) * 5), "0 active + 5 new requests exceed max_active = 4")
            assert lib.mb_session_active(h) == 0
            k = ctypes.c_int(-1)
            fin = (ctypes.c_uint64 * 4)()
            refused(lib.mb_session_tick(None, None, None, None, None, None, None, fin, None, ctypes.byref(k), None), "null argument")
            refused(lib.mb_session_tick(h, None, None, None, None, None, None, fin, None, None, None), "null argument")
            assert lib.mb_session_tick(h, None, None, None, None, None, None, fin, None, ctypes.byref(k), None) == 0 and k.value == 0   # A = 0: nothing to do
            assert _lib.prof_read() == {}
        finally:
            lib.mb_session_destroy(h)
        # the single-kernel entries
        rows = _lib.SessionRows(a, a, a, a, a, a, a, 4, 8)
        one = (ctypes.c_int * 1)(3)
        refused(lib.mb_session_row_table(None, a, 1, None), "null argument")
        refused(lib.mb_session_row_table(ctypes.byref(rows), None, 1, None), "null argument")
        refused(lib.mb_session_row_table(ctypes.byref(rows), a, 0, None), "rows outside [1, max_active]")
        refused(lib.mb_session_row_table(ctypes.byref(rows), a, 5, None), "rows outside [1, max_active]")
        refused(lib.mb_session_admit_rows(ctypes.byref(rows), a, 0, 0, a, a, one, a, None, 16, 2, 64, None), "bad sizes")
        refused(lib.mb_session_admit_rows(ctypes.byref(rows), a, 4, 1, a, a, one, a, None, 16, 2, 64, None), "rows outside [1, max_active]")
        refused(lib.mb_session_admit_rows(ctypes.byref(rows), a, 0, 1, a, a, (ctypes.c_int * 1)(9), a, None, 16, 2, 64, None), "outside [1, 8]")
        refused(lib.mb_session_admit_rows(ctypes.byref(rows), a, 0, 1, a, a, one, a, None, 16, 2, 48, None), "power of two")
        refused(lib.mb_session_admit_rows(ctypes.byref(rows), None, 0, 1, a, a, one, a, None, 16, 2, 64, None), "null argument")
        refused(lib.mb_session_retire(ctypes.byref(rows), a, a, a, a, None, 2, 16, 2, 64, None), "null argument")
        refused(lib.mb_session_retire(ctypes.byref(rows), a, a, a, a, a, 5, 16, 2, 64, None), "rows outside [1, max_active]")
        refused(lib.mb_session_retire(ctypes.byref(rows), a, a, a, a, a, 2, 8193, 1, 64, None), "n * m outside [1, 8192]")
        rows.pool = None
        refused(lib.mb_session_retire(ctypes.byref(rows), a, a, a, a, a, 2, 16, 2, 64, None), "null argument")
        assert _lib.prof_read() == {}
    finally:
        _lib.prof_enable(False)


# ---- SamplingSession without a device ------------------------------------------------------------------------------------------------------------
def cpu_models():
    from maskbit_amd import ConvVQModel, LFQBert
    from hip_helpers import tok_config
    from test_edit_cpu import TINY_GEN, TINY_TOK
    gm = LFQBert(img_size=256, hidden_dim=TINY_GEN.hidden, codebook_size=2 ** TINY_GEN.bits, codebook_splits=TINY_GEN.splits, depth=TINY_GEN.depth,
                 heads=TINY_GEN.heads, mlp_dim=TINY_GEN.mlp, dropout=0.1, nclass=TINY_GEN.nclass, input_stride=16)
    return gm, ConvVQModel(tok_config(TINY_TOK))


def test_submit_refuses_bad_requests_and_counts_tickets_without_a_device():
    from maskbit_amd import SampleRequest, SamplingSession
    gm, tm = cpu_models()
    n, m, mask = gm.seq_len, gm.splits, gm.mask_token
    for kw in (dict(max_active=0), dict(max_steps=0), dict(max_active=2.0)):
        with pytest.raises(ValueError):
            SamplingSession(gm, tm, **kw)
    with pytest.raises(TypeError):
        SamplingSession(tm, tm)
    s = SamplingSession(gm, tm, max_active=2, max_steps=6, guided=True)
    good = SampleRequest(seed=1, label=2, num_steps=6)
    assert (s.active, s.queued, s.ticks) == (0, 0, 0)
    assert s.step() == [] and s.step(return_predictions=True) == ([], {})                        # empty: nothing to run, no device asked for
    with pytest.raises(TypeError):
        s.submit((1, 2))
    with pytest.raises(TypeError):
        s.submit(None)
    with pytest.raises(ValueError, match="max_steps"):
        s.submit(dataclasses.replace(good, num_steps=7))
    for field, value in (("num_steps", 0), ("num_steps", 2.0), ("guidance_annealing", "quadratic"), ("mask_schedule_strategy", "zigzag"),
                         ("seed", -1), ("seed", 2 ** 64), ("seed", 1.5)):
        with pytest.raises(ValueError):
            s.submit(dataclasses.replace(good, **{field: value}))
    with pytest.raises(IndexError):
        s.submit(dataclasses.replace(good, label=gm.nclass + 1))
    ok = torch.full((n, m), mask, dtype=torch.int64)
    with pytest.raises(ValueError, match="init_tokens"):
        s.submit(good, init_tokens=torch.full((1, n, m), mask, dtype=torch.int64))               # shape
    with pytest.raises(ValueError, match="init_tokens"):
        s.submit(good, init_tokens=ok[:, :1])
    with pytest.raises(TypeError, match="int64"):
        s.submit(good, init_tokens=ok.to(torch.int32))                                           # dtype
    with pytest.raises(TypeError, match="int64"):
        s.submit(good, init_tokens=ok.tolist())
    for bad in (-1, mask + 1):                                                                    # range
        t = ok.clone()
        t[3, 1] = bad
        with pytest.raises(ValueError, match="token outside"):
            s.submit(good, init_tokens=t)
    assert s.queued == 0                                                                          # a refused request takes no ticket
    assert [s.submit(good), s.submit(dataclasses.replace(good, num_steps=1, guidance_scale=0.0)), s.submit(good, init_tokens=ok)] == [0, 1, 2]
    assert (s.active, s.queued, s.ticks) == (0, 3, 0)
    with pytest.raises(RuntimeError, match="runs only on an AMD GPU"):                            # a good step gets as far as the device
        s.step()
    assert s.queued == 3
    u = SamplingSession(gm, None, guided=False)
    with pytest.raises(ValueError, match="guided=False"):
        u.submit(good)
    assert u.submit(dataclasses.replace(good, guidance_scale=0.0)) == 0 and u.queued == 1
