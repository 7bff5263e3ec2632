"""numpy restatement of the seeded noise definition, written from the text of include/maskbit_hip.h ("per-sample seeded sampling") alone: Philox4x32-10
keyed by the sample's 64-bit seed, the counter layouts of the two streams, the 24-bit odd uniform, and the float64 values the two noise tensors are
compared against.  Nothing here comes from the kernels; tests/test_seeded_cpu.py checks it against Random123's known answers and for its distribution,
tests/test_hip_seeded.py holds the device to it."""
import numpy as np

M0, M1 = 0xD2511F53, 0xCD9E8D57
W0, W1 = 0x9E3779B9, 0xBB67AE85
MASK32 = np.uint64(0xFFFFFFFF)


def philox4x32_10(ctr, key):
    """ctr: four broadcastable integer arrays, key: two -> four uint32 arrays (the ten-round Philox4x32 of Salmon et al.)."""
    c = [np.asarray(x, dtype=np.uint64) & MASK32 for x in np.broadcast_arrays(*ctr)]
    k0, k1 = [np.asarray(x, dtype=np.uint64) & MASK32 for x in key]
    for _ in range(10):
        p0, p1 = np.uint64(M0) * c[0], np.uint64(M1) * c[2]                    # 32 x 32 -> 64 bits: exact in uint64
        c = [(p1 >> np.uint64(32)) ^ c[1] ^ k0, p1 & MASK32, (p0 >> np.uint64(32)) ^ c[3] ^ k1, p0 & MASK32]
        k0, k1 = (k0 + np.uint64(W0)) & MASK32, (k1 + np.uint64(W1)) & MASK32
    return [x.astype(np.uint32) for x in c]


def seed_key(seeds):
    """(low dword, high dword) of each seed in [0, 2^64)."""
    s = np.array([int(v) & 0xFFFFFFFFFFFFFFFF for v in np.asarray(seeds, dtype=object).reshape(-1)], dtype=np.uint64)
    return s & MASK32, s >> np.uint64(32)


def uniform(x):
    """u = float((x >> 8) | 1) * 2^-24 as float32 (exact)."""
    return (((np.asarray(x, dtype=np.uint32) >> np.uint32(8)) | np.uint32(1)).astype(np.float32) * np.float32(2.0 ** -24)).astype(np.float32)


def exp_uniforms(seeds, step, P, C):
    """The categorical stream's uniforms float32 [B, P, C]: counter (c >> 2, slot, step, 0), class c takes word c & 3."""
    k0, k1 = seed_key(seeds)
    B = len(k0)
    blocks = (C + 3) // 4
    w = philox4x32_10((np.arange(blocks).reshape(1, 1, -1), np.arange(P).reshape(1, -1, 1), step, 0), (k0.reshape(B, 1, 1), k1.reshape(B, 1, 1)))
    words = np.stack(w, axis=-1).reshape(B, P, blocks * 4)[:, :, :C]           # word j of block b is class 4 b + j
    return uniform(words)


def conf_uniforms(seeds, step, P):
    """The confidence stream's uniforms float32 [B, P]: counter (0, slot, step, 1), word 0."""
    k0, k1 = seed_key(seeds)
    B = len(k0)
    w = philox4x32_10((0, np.arange(P).reshape(1, -1), step, 1), (k0.reshape(B, 1), k1.reshape(B, 1)))
    return uniform(w[0])


def exp_noise64(u):
    """q = -log u in float64."""
    return -np.log(u.astype(np.float64))


def gumbel64(u):
    """g = -log(-log u) in float64."""
    return -np.log(-np.log(u.astype(np.float64)))


def race_picks(seeds, step, P, p):
    """argmax_c p[c] / q[c] per (sample, slot) in float64: the categorical draw of a seeded step for one probability row p [C]."""
    q = exp_noise64(exp_uniforms(seeds, step, P, len(p)))
    return np.argmax(np.asarray(p, dtype=np.float64) / q, axis=-1)
