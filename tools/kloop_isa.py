"""What the K loops of the half-tile GEMM hold, per instantiation with mini-tiles (XP = 6): compiles maskbit_amd/csrc/gemm_ht.hip to gfx950 assembly with
the flags of maskbit_amd/build.py and prints VGPRs, scratch bytes and the instruction mix of every K-loop body, per wave and per K-tile.  A K loop is an
innermost loop (a label with a backward branch to it) that holds both MFMAs and LDS-DMA instructions; plain tiles have two (one per accumulator half).
The counts are STATIC: every instruction between the loop's label and its backward branch, rarely taken branches included (the once-per-tile switch
to the second mini-tile operand set is about 30 scalar instructions of the pair kernels' bodies).  Classes, by mnemonic prefix only: MFMA (v_mfma),
other VALU (v_), of which wide / multiply (64-bit or integer-multiply forms), ds_read, LDS-DMA (global_load_lds), SALU (s_ without waits, barriers,
nops, priorities and branches).  A reporting tool, not a test.
usage: python tools/kloop_isa.py [--asm FILE] [--all] [--markdown]"""
import argparse
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from maskbit_amd import build as B

FLAGS = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-Wno-unused-result"]      # maskbit_amd/build.py
EPI = {0: "h16", 1: "gelu_h16", 2: "res_f32", 3: "gelu_f32"}
S_SKIP = ("s_waitcnt", "s_barrier", "s_nop", "s_setprio", "s_cbranch", "s_branch", "s_endpgm", "s_sleep")
WIDE = ("_u64", "_i64", "v_mul_lo", "v_mul_hi", "v_mad_u32", "v_mad_i32", "v_addc", "v_subb")


def assemble(path):
    cmd = [B.hipcc(), *FLAGS, "-S", "--cuda-device-only", os.path.join(B.CSRC, "gemm_ht.hip"), "-o", path]
    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    if r.returncode != 0:
        raise RuntimeError(r.stdout)


def kernels(text):
    """-> [(symbol, body lines, {NumVgprs, ScratchSize, ...})]"""
    out = []
    for m in re.finditer(r"^(_ZN2mb14gemm_ht_kernel\w+):[^\n]*\n(.*?)^\s*\.end_amdhsa_kernel", text, re.S | re.M):
        tail = text[m.end():m.end() + 4000]
        info = {k: int(v) for k, v in re.findall(r"^; (NumVgprs|NumAgprs|ScratchSize|Occupancy): (\d+)", tail, re.M)}
        out.append((m.group(1), m.group(2).split("\n"), info))
    return out


def template_args(sym):
    """MT, EPI, XP, SEQ, PAIR, NS of gemm_ht_kernel<...> from the mangled name."""
    a = re.match(r"_ZN2mb14gemm_ht_kernelILi(\d+)ELi(\d+)ELi(\d+)ELb([01])ELb([01])ELi(\d+)EEE", sym)
    return tuple(int(x) for x in a.groups()) if a else None


def mnemonic(line):
    s = line.split(";")[0].strip()
    if not s or s.startswith(".") or s.endswith(":"):
        return None
    return s.split()[0]


def loops(lines):
    """Innermost (label line, branch line) ranges that hold MFMAs and LDS-DMA."""
    label_at = {}
    spans = []
    for i, l in enumerate(lines):
        m = re.match(r"^(\.LBB\d+_\d+):", l)
        if m:
            label_at[m.group(1)] = i
            continue
        m = re.match(r"^\s+s_c?branch\w*\s+(\.LBB\d+_\d+)", l)
        if m and m.group(1) in label_at:
            spans.append((label_at[m.group(1)], i))
    def holds(sp):
        ms = [mnemonic(l) or "" for l in lines[sp[0]:sp[1] + 1]]
        return any(x.startswith("v_mfma") for x in ms) and any(x.startswith("global_load_lds") for x in ms)
    spans = [sp for sp in spans if holds(sp)]
    return [sp for sp in spans if not any(o != sp and sp[0] <= o[0] and o[1] <= sp[1] for o in spans)]


def mix(lines):
    c = dict(mfma=0, valu=0, wide=0, ds_read=0, dma=0, salu=0, barrier=0, wide_names={})
    for l in lines:
        m = mnemonic(l)
        if not m:
            continue
        if m.startswith("v_mfma"):
            c["mfma"] += 1
        elif m.startswith("v_"):
            c["valu"] += 1
            if any(w in m for w in WIDE):
                c["wide"] += 1
                c["wide_names"][m] = c["wide_names"].get(m, 0) + 1
        elif m.startswith("ds_read") or m.startswith("ds_load"):
            c["ds_read"] += 1
        elif m.startswith("global_load_lds"):
            c["dma"] += 1
        elif m == "s_barrier":
            c["barrier"] += 1
        elif m.startswith("s_") and not m.startswith(S_SKIP):
            c["salu"] += 1
    return c


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--asm", help="read this assembly file instead of compiling")
    ap.add_argument("--all", action="store_true", help="every instantiation, not only XP = 6")
    ap.add_argument("--markdown", action="store_true")
    args = ap.parse_args()
    if args.asm:
        text = open(args.asm).read()
    else:
        with tempfile.TemporaryDirectory() as d:
            assemble(os.path.join(d, "gemm_ht.s"))
            text = open(os.path.join(d, "gemm_ht.s")).read()
    head = ["kernel", "VGPRs", "scratch B", "loop", "barriers", "MFMA", "other v_", "wide/mul v_", "ds_read", "LDS-DMA", "s_ arith"]
    rows = []
    for sym, lines, info in kernels(text):
        t = template_args(sym)
        if not t or (t[2] != 6 and not args.all):
            continue
        name = f"{'pair' if t[4] else 'seq' if t[3] else 'MT%d' % t[0]} {EPI.get(t[1], t[1])}" + (f" NS{t[5]}" if t[5] > 1 else "") + ("" if t[2] == 6 else " (no mini)")
        for i, (a, b) in enumerate(loops(lines)):
            c = mix(lines[a:b + 1])
            wide = str(c["wide"]) + (" (" + ", ".join(f"{k} x{v}" for k, v in sorted(c["wide_names"].items())) + ")" if c["wide"] else "")
            rows.append([name, info.get("NumVgprs", "?"), info.get("ScratchSize", "?"), i, c["barrier"], c["mfma"], c["valu"], wide, c["ds_read"], c["dma"], c["salu"]])
    if args.markdown:
        print("| " + " | ".join(head) + " |")
        print("|" + "---|" * len(head))
        for r in rows:
            print("| " + " | ".join(str(x) for x in r) + " |")
    else:
        w = [max(len(str(x)) for x in col) for col in zip(head, *rows)]
        for r in [head] + rows:
            print("  ".join(str(x).ljust(n) for x, n in zip(r, w)))


if __name__ == "__main__":
    main()
