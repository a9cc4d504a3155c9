"""
NumPy restatement of the direct Monte-Carlo under gate-level faults (DESIGN.md section 5e "Direct Monte-Carlo under gate-level
faults"), for tests/test_gate_mc.py and tests/test_gpu_gate_mc.py.  Written from the definition alone: it shares no code with the
HIP kernel, with gf2_gate_outcomes_host (csrc/gf2_host.cpp) or with the package; only mix64, quantise and the two constants come from
tests/strata_ref.py, itself such a restatement.

    ks = mix64(seed + G (i + 1))
    class 0: the n1 one-operand sites, radix 3,  site base 0,  T = quantise(p1), slot base 4096
    class 1: the n2 CNOT sites,        radix 15, site base n1, T = quantise(p2), slot base 8192
    per class, per segment s of 512 sites (nb = 512, or what is left in the last one):
      d = mix64(ks + M (slot base + s + 1)),  K = #{k < nb : (d >> 32) >= cdf[k]},  cdf = the inverse binomial CDF table of (T, nb)
      k = 0 .. K - 1:  v = mix64(d + G (k + 1)),  j = nb - K + k,  t = ((v >> 32) (j + 1)) >> 32,
                       position = j if an earlier pick of the segment took t else t,  kappa = 1 + (((v & (2^32 - 1)) radix) >> 32),
                       site = site base + 512 s + position
    words = XOR over the picks and the set bits t of kappa of eff[site_loc[site] + (t >> 1)][t & 1]
    (a, b, c) = picks of class 0, picks of class 1, picks of class 1 with (kappa & 3) and (kappa >> 2) both non-zero
"""
import math

import numpy as np

from tests.strata_ref import GOLDEN, STREAM_MULT, mix64, quantise

SEG = 512
SLOT_BASE = (4096, 8192)
RADIX = (3, 15)
TWO32 = float(1 << 32)


def _cdf_direct(t_any, nb):
    """round(2^32 P(Bin(nb, t_any / 2^32) <= k)) for k < nb, in IEEE doubles in the order DESIGN.md "Sampler" fixes."""
    if t_any >= 1 << 32:
        return [0] * nb
    q = t_any / TWO32
    om = 1.0 - q
    pmf = 1.0
    for _ in range(nb):
        pmf *= om
    cum, out = 0.0, []
    for k in range(nb):
        cum += pmf
        out.append(int(min(math.floor(cum * TWO32 + 0.5), TWO32)))
        pmf = pmf * float(nb - k) / float(k + 1) * q / om
    return out


def cdf_table(t_any, nb):
    """The table of a segment of nb sites: above one half the complementary count's table, mirrored."""
    if t_any <= 1 << 31 or t_any >= 1 << 32:
        return np.array(_cdf_direct(t_any, nb), dtype=np.uint64)
    other = _cdf_direct((1 << 32) - t_any, nb)
    return np.array([(1 << 32) - other[nb - k - 1] for k in range(nb)], dtype=np.uint64)


def gate_mc_faults(seed, first, count, n1, n2, p1, p2):
    """(sample, site, kappa) of every fault of samples [first, first + count), in the order of the draw: three int64 arrays, `sample`
    relative to `first`, `site` in the unified numbering (one-operand sites [0, n1), CNOT sites [n1, n1 + n2))."""
    samples, sites, kappas = [], [], []
    with np.errstate(over="ignore"):
        i = np.arange(count, dtype=np.uint64) + np.uint64(first)
        ks = mix64(np.uint64(seed) + np.uint64(GOLDEN) * (i + np.uint64(1)))
        for m, base, radix, slot, p in ((n1, 0, RADIX[0], SLOT_BASE[0], p1), (n2, n1, RADIX[1], SLOT_BASE[1], p2)):
            t_any = int(quantise(p))
            for s in range((m + SEG - 1) // SEG):
                nb = min(SEG, m - SEG * s)
                cdf = cdf_table(t_any, nb)
                d = mix64(ks + np.uint64(STREAM_MULT) * np.uint64(slot + s + 1))
                K = ((d >> np.uint64(32))[:, None] >= cdf[None, :]).sum(axis=1).astype(np.int64)
                taken = np.zeros((count, nb), dtype=bool)
                for k in range(int(K.max()) if count else 0):
                    rows = np.nonzero(K > k)[0]
                    v = mix64(d[rows] + np.uint64(GOLDEN) * np.uint64(k + 1))
                    hi, lo = v >> np.uint64(32), v & np.uint64(0xFFFFFFFF)
                    j = nb - K[rows] + k
                    t = ((hi * (j + 1).astype(np.uint64)) >> np.uint64(32)).astype(np.int64)
                    pos = np.where(taken[rows, t], j, t)
                    assert not taken[rows, pos].any()
                    taken[rows, pos] = True
                    samples.append(rows)
                    sites.append(base + SEG * s + pos)
                    kappas.append((1 + ((lo * np.uint64(radix)) >> np.uint64(32))).astype(np.int64))
    if not samples:
        return (np.zeros(0, dtype=np.int64),) * 3
    sample, site, kappa = np.concatenate(samples), np.concatenate(sites), np.concatenate(kappas)
    order = np.argsort(sample, kind="stable")                                # by sample, the order of the draw kept inside one
    return sample[order], site[order], kappa[order]


def fault_counts(sample, site, kappa, count, n1):
    """(count, 3) int32 (a, b, c) per sample."""
    cnot = site >= n1
    two = cnot & ((kappa & 3) != 0) & ((kappa >> 2) != 0)
    out = np.zeros((count, 3), dtype=np.int32)
    out[:, 0] = np.bincount(sample[~cnot], minlength=count)
    out[:, 1] = np.bincount(sample[cnot], minlength=count)
    out[:, 2] = np.bincount(sample[two], minlength=count)
    return out


def gate_mc_words(eff, site_loc, n1, n2, seed, first, count, p1, p2):
    """(words (count, ldr) uint64, faults (count, 3) int32) of those samples over the effect words eff (L, 2, ldr)."""
    eff = np.asarray(eff, dtype=np.uint64)
    site_loc = np.asarray(site_loc, dtype=np.int64)
    sample, site, kappa = gate_mc_faults(seed, first, count, n1, n2, p1, p2)
    words = np.zeros((count, eff.shape[2]), dtype=np.uint64)
    loc = site_loc[site]
    for bit in range(4):
        has = ((kappa >> bit) & 1).astype(bool)
        np.bitwise_xor.at(words, sample[has], eff[loc[has] + (bit >> 1), bit & 1])
    return words, fault_counts(sample, site, kappa, count, n1)
