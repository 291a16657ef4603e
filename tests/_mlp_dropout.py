"""Host twins of the MLP's dropout keep law (csrc/hmcx_keep_law.h), shared by test_mlp_dropout_cpu.py and
test_gpu_mlp_dropout.py.  Written from the law's definition with plain per-byte compares — never the kernels'
four-bytes-at-once form — and NumPy only: no device, no library."""
import math

import numpy as np

RATIOS = (0.0, 0.05, 0.1, 0.25, 0.5, 0.75, 0.9)


def threshold(ratio):
    """t = ceil(ratio * 2^24) in double."""
    return int(math.ceil(float(ratio) * 16777216.0))


def philox_host(c0, c1, c2, c3, seed):
    """Philox4x32-10 of counters (c0 vector, c1..c3 scalars) under key `seed`: the four output words."""
    M0, M1, m32 = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57), np.uint64(0xFFFFFFFF)
    c0 = np.asarray(c0, dtype=np.uint64)
    c1, c2, c3 = (np.full(c0.shape, v & 0xFFFFFFFF, dtype=np.uint64) for v in (c1, c2, c3))
    k0, k1 = seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF
    for _ in range(10):
        p0, p1 = M0 * c0, M1 * c2
        c0, c1, c2, c3 = (p1 >> np.uint64(32)) ^ c1 ^ np.uint64(k0), p1 & m32, \
            (p0 >> np.uint64(32)) ^ c3 ^ np.uint64(k1), p0 & m32
        k0, k1 = (k0 + 0x9E3779B9) & 0xFFFFFFFF, (k1 + 0xBB67AE85) & 0xFFFFFFFF
    return c0, c1, c2, c3


def group_bytes(seed, n3, slot, step, chain):
    """The top byte of every element's 24-bit uniform, [groups, 64]: element p of group G takes byte p / 8 % 4 of
    word 8 * (p / 32) + p % 8 of the group's four main blocks."""
    nG = (n3 + 63) // 64
    G = np.arange(nG, dtype=np.uint64)
    words = []                                                     # word kk = 4k + q of the group
    for k in range(4):
        words.extend(philox_host(4 * G + k, slot, step, chain, seed))
    p = np.arange(64)
    widx = 8 * (p // 32) + p % 8
    return np.stack([(words[w] >> np.uint64(8 * ((q // 8) % 4))) & np.uint64(0xFF)
                     for q, w in zip(p, widx)], axis=1).astype(np.int64)


def _resolve_ties(keep, byte, tb, tl, seed, slot, step, chain):
    """The a-th element of a group whose byte equals tb (ascending element order) reads 16-bit half a % 8 (low half
    first) of fallback block a / 8 and keeps iff it is >= tl."""
    for g in np.nonzero((byte == tb).any(axis=1))[0]:
        amb = np.nonzero(byte[g] == tb)[0]
        for a, e in enumerate(amb):
            r = philox_host([0x80000000 | (int(g) << 3) | (a // 8)], slot, step, chain, seed)
            h = a % 8
            x = (int(r[h // 2][0]) >> (16 * (h % 2))) & 0xFFFF
            keep[g, e] = x >= tl


def keep_group_host(ratio, seed, n3, slot, step, chain):
    """The keep flags of elements 0 … n3 − 1 of one forward at `ratio`: kept iff byte > tb, or byte == tb and the
    element's low 16 bits >= tl, for t = ceil(ratio * 2^24), tb = t >> 16, tl = t & 0xFFFF."""
    t = threshold(ratio)
    tb, tl = t >> 16, t & 0xFFFF
    byte = group_bytes(seed, n3, slot, step, chain)
    keep = byte > tb
    _resolve_ties(keep, byte, tb, tl, seed, slot, step, chain)
    return keep.reshape(-1)[:n3]


def keep_group_host_default(seed, n3, slot, step, chain):
    """The constants-only law of ratio 0.1 as the library had it before the ratio became a parameter (the logic of
    tests/test_gpu_mlp.py::_keep_group_host): byte > 0x19, ties by low bits >= 0x999A."""
    byte = group_bytes(seed, n3, slot, step, chain)
    keep = byte > 0x19
    for g in np.nonzero((byte == 0x19).any(axis=1))[0]:
        amb = np.nonzero(byte[g] == 0x19)[0]                       # ascending element order
        for a, e in enumerate(amb):
            r = philox_host([0x80000000 | (int(g) << 3) | (a // 8)], slot, step, chain, seed)
            h = a % 8
            x = (int(r[h // 2][0]) >> (16 * (h % 2))) & 0xFFFF
            keep[g, e] = x >= 0x999A
    return keep.reshape(-1)[:n3]
