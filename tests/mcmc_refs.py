"""References for the MCMC densification kernels (csrc/mcmc.hip, gs4d_train/mcmc.py), in Python integers and numpy
fp64; nothing here imports the code under test.

  philox4x32_10 / blocks   the generator, one block at a time in Python integers
  sample                   the sampler: Python-int weights and prefix sums, (u * total) >> 64
  relocated                o' and s'/s of the correction, with math.comb, term by term in fp64
  normals64 / noise_delta  fp64 Box-Muller of the exact words; the position change in fp64
  regulariser              value and both gradients in fp64
"""
import bisect
import math

import numpy as np

M0, M1, W0, W1 = 0xD2511F53, 0xCD9E8D57, 0x9E3779B9, 0xBB67AE85
MASK32 = 0xFFFFFFFF
NOISE, RELOCATE, GROW = 0, 1, 2
N_MAX = 51
FLT_EPSILON = 2.0 ** -23


def philox4x32_10(counter, key):
    """counter: 4 words, key: 2 words -> 4 words (Salmon et al. 2011; Random123's philox4x32, 10 rounds)"""
    c0, c1, c2, c3 = (int(x) & MASK32 for x in counter)
    k0, k1 = (int(x) & MASK32 for x in key)
    for _ in range(10):
        p0, p1 = M0 * c0, M1 * c2
        c0, c1, c2, c3 = (p1 >> 32) ^ c1 ^ k0, p1 & MASK32, (p0 >> 32) ^ c3 ^ k1, p0 & MASK32
        k0, k1 = (k0 + W0) & MASK32, (k1 + W1) & MASK32
    return c0, c1, c2, c3


def blocks(n, seed, iteration, purpose):
    """(n, 4) uint32: blocks 0 .. n - 1 of key (seed lo, seed hi), counter (j, purpose, iteration, 0)"""
    seed = int(seed) & 0xFFFFFFFFFFFFFFFF
    key = (seed & MASK32, seed >> 32)
    out = np.zeros((n, 4), np.uint32)
    for j in range(n):
        out[j] = philox4x32_10((j, purpose, iteration, 0), key)
    return out


def weight(o, min_opacity):
    """(uint64)(o 2^32) for a float32 opacity above the float32 threshold, else 0 (exact: Python float -> int)"""
    o, m = float(np.float32(o)), float(np.float32(min_opacity))
    return int(min(o, 1.0) * 4294967296.0) if o > m else 0


def sample(opacity, min_opacity, n, seed, iteration, purpose):
    """(draws (n) int32, counts (P) int32, drawn): the first row with S[i] > (u * total) >> 64, all in Python ints"""
    o = np.asarray(opacity, np.float32).reshape(-1)
    P = o.shape[0]
    draws, counts = np.zeros(n, np.int32), np.zeros(P, np.int32)
    if P == 0 or n == 0:
        return draws, counts, 0
    S, acc = [], 0
    for x in o:
        acc += weight(x, min_opacity)
        S.append(acc)
    if acc == 0:
        return draws, counts, 0
    words = blocks(n, seed, iteration, purpose)
    for d in range(n):
        u = int(words[d, 0]) | (int(words[d, 1]) << 32)
        t = (u * acc) >> 64
        i = bisect.bisect_right(S, t)  # the first i with S[i] > t
        draws[d] = i
        counts[i] += 1
    return draws, counts, n


def relocated(o, n):
    """(o', s'/s) of a source of opacity o shared among n copies, before the clamp: fp64, math.comb, term by term"""
    o = float(o)
    o_new = -math.expm1(math.log1p(-o) / n)
    D = 0.0
    for i in range(1, n + 1):
        for k in range(i):
            D += math.comb(i - 1, k) * (-1.0) ** k * o_new ** (k + 1) / math.sqrt(k + 1)
    return o_new, o / D


def relocate_rows(opacity_raw, scaling_raw, counts, min_opacity):
    """the raw opacity (P, 1) and scaling (P, 3) after gs4d_mcmc_relocate, in fp64 (float32 inputs taken exactly)"""
    oraw = np.asarray(opacity_raw, np.float64).reshape(-1).copy()
    sraw = np.asarray(scaling_raw, np.float64).copy()
    lo, hi = float(np.float32(min_opacity)), 1.0 - FLT_EPSILON
    for r in np.nonzero(np.asarray(counts).reshape(-1) > 0)[0]:
        n = min(int(counts[r]) + 1, N_MAX)
        o = 1.0 / (1.0 + math.exp(-oraw[r]))
        o_new, ratio = relocated(o, n)
        o_new = min(max(o_new, lo), hi)
        oraw[r] = math.log(o_new / (1.0 - o_new))
        sraw[r] = np.log(np.exp(sraw[r]) * ratio)
    return oraw.reshape(np.asarray(opacity_raw).shape), sraw


def units64(words):
    return ((np.asarray(words, np.uint32) >> np.uint32(8)).astype(np.float64) + 0.5) * 2.0 ** -24


def normals64(words):
    """(n, 3) fp64 Box-Muller normals of (n, 4) words: the kernel's formula on the exact words"""
    u = units64(words)
    r0, r1 = np.sqrt(-2.0 * np.log(u[:, 0])), np.sqrt(-2.0 * np.log(u[:, 2]))
    return np.stack([r0 * np.cos(2 * np.pi * u[:, 1]), r0 * np.sin(2 * np.pi * u[:, 1]), r1 * np.cos(2 * np.pi * u[:, 3])], 1)


def normals32(words):
    """the same in numpy fp32: the unfused formulation whose error sets the generated normals' bar"""
    u = ((np.asarray(words, np.uint32) >> np.uint32(8)).astype(np.float32) + np.float32(0.5)) * np.float32(2.0 ** -24)
    r0, r1 = np.sqrt(np.float32(-2) * np.log(u[:, 0])), np.sqrt(np.float32(-2) * np.log(u[:, 2]))
    tp = np.float32(2 * np.pi)
    return np.stack([r0 * np.cos(tp * u[:, 1]), r0 * np.sin(tp * u[:, 1]), r1 * np.cos(tp * u[:, 3])], 1).astype(np.float32)


def rotations64(q):
    q = np.asarray(q, np.float64)
    q = q / np.maximum(np.sqrt((q * q).sum(1, keepdims=True)), 1e-12)
    w, x, y, z = q[:, 0], q[:, 1], q[:, 2], q[:, 3]
    R = np.empty((q.shape[0], 3, 3))
    R[:, 0, 0], R[:, 0, 1], R[:, 0, 2] = 1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)
    R[:, 1, 0], R[:, 1, 1], R[:, 1, 2] = 2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)
    R[:, 2, 0], R[:, 2, 1], R[:, 2, 2] = 2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)
    return R


def gate64(opacity_raw):
    o = 1.0 / (1.0 + np.exp(-np.asarray(opacity_raw, np.float64).reshape(-1)))
    return 1.0 / (1.0 + np.exp(-100.0 * ((1.0 - o) - 0.995)))


def noise_delta(scaling_raw, rotation_raw, opacity_raw, step_scale, normals):
    """(P, 3) fp64: R diag(s^2) R^T (z g step_scale)"""
    R = rotations64(rotation_raw)
    s2 = np.exp(np.asarray(scaling_raw, np.float64)) ** 2
    v = np.asarray(normals, np.float64) * gate64(opacity_raw)[:, None] * float(step_scale)
    cov = np.einsum("pab,pb,pcb->pac", R, s2, R)
    return np.einsum("pac,pc->pa", cov, v)


def implied_normals(delta, scaling_raw, rotation_raw, opacity_raw, step_scale):
    """z from a position change: (R diag(s^-2) R^T delta) / (g step_scale), fp64"""
    R = rotations64(rotation_raw)
    s2 = np.exp(np.asarray(scaling_raw, np.float64)) ** 2
    inv = np.einsum("pab,pb,pcb->pac", R, 1.0 / s2, R)
    return np.einsum("pac,pc->pa", inv, np.asarray(delta, np.float64)) / (gate64(opacity_raw)[:, None] * float(step_scale))


def regulariser(opacity_raw, scaling_raw, w_opacity, w_scale):
    """(value, d/d raw opacity (P, 1), d/d raw scaling (P, 3)) in fp64"""
    o = 1.0 / (1.0 + np.exp(-np.asarray(opacity_raw, np.float64)))
    s = np.exp(np.asarray(scaling_raw, np.float64))
    P = o.shape[0]
    value = w_opacity * o.mean() + w_scale * s.mean() if P else 0.0
    return value, w_opacity / max(P, 1) * o * (1 - o), w_scale / max(3 * P, 1) * s
