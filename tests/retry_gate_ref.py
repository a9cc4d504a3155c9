"""
NumPy restatement of the repeat-until-success sampler under gate-level faults (DESIGN.md section 5d "Repeat-until-success under
gate-level faults"), for tests/test_retry_gate.py and tests/test_gpu_retry_gate.py, and the exact distributions its samples must
follow.  Written from the definition alone: it shares no code with the HIP kernel or with gf2_retry_gate_words_host
(csrc/gf2_host.cpp); of a gadget it reads the block tables only (every type's effects, flag rows, regions and sites, the blocks'
types and kinds).  The keys, the frame masks and the exact helpers come from tests/retry_ref.py, the inverse-CDF table, the slots
and the radices from tests/gate_mc_ref.py, mix64 and quantise from tests/strata_ref.py, themselves such restatements.

    ks, kr (region g), ka (attempt a): tests/retry_ref.py's
    under ka, per class of the region's sites -- class 0: its n1 one-operand sites, radix 3, T = quantise(p1), slot base 4096;
    class 1: its n2 CNOT sites, radix 15, T = quantise(p2), slot base 8192 -- and per segment s of 512 of the class's sites:
      d = mix64(ka + M (slot base + s + 1)),  K = #{k < nb : (d >> 32) >= cdf[k]},  cdf = the inverse binomial CDF table of (T, nb)
      k = 0 .. K - 1:  v = mix64(d + G (k + 1)),  j = nb - K + k,  t = ((v >> 32) (j + 1)) >> 32,
                       position = j if an earlier pick of the segment took t else t,  kappa = 1 + (((v & (2^32 - 1)) radix) >> 32)
    (local, tail, flags) ^= XOR over the picks and the set bits t of kappa of eff[site_loc[site] + (t >> 1)][t & 1]
    retried regions, exhaustion, blocks, words: tests/retry_ref.py's
"""
import numpy as np

from oracle import exact_dist
from tests import retry_ref
from tests.gate_mc_ref import RADIX, SEG, SLOT_BASE, cdf_table
from tests.retry_ref import FINAL, FRAME, NONE, _extract, _u64, frame_mask, key_mask, xor_convolution
from tests.strata_ref import GOLDEN, STREAM_MULT, mix64, quantise


def draw_region(ka, eff, site_loc, n1, n2, t_class, tables):
    """(local, tail, flags) of one attempt per key of `ka` over a type's table eff (L_b, 2, 3) and a region's sites: site_loc holds its
    n1 one-operand sites, then its n2 CNOT sites (type-local first locations)."""
    out = np.zeros((len(ka), 3), dtype=np.uint64)
    for cl, (m, base) in enumerate(((n1, 0), (n2, n1))):
        for s in range((m + SEG - 1) // SEG):
            nb = min(SEG, m - SEG * s)
            if (cl, nb) not in tables:
                tables[cl, nb] = cdf_table(t_class[cl], nb)
            d = mix64(ka + _u64(STREAM_MULT * (SLOT_BASE[cl] + s + 1)))
            K = ((d >> np.uint64(32))[:, None] >= tables[cl, nb][None, :]).sum(axis=1).astype(np.int64)
            taken = np.zeros((len(ka), nb), dtype=bool)
            for k in range(int(K.max()) if len(ka) else 0):
                rows = np.nonzero(K > k)[0]
                v = mix64(d[rows] + _u64(GOLDEN * (k + 1)))
                hi, lo = v >> np.uint64(32), v & np.uint64(0xFFFFFFFF)
                j = nb - K[rows] + k
                t = ((hi * (j + 1).astype(np.uint64)) >> np.uint64(32)).astype(np.int64)
                pos = np.where(taken[rows, t], j, t)
                taken[rows, pos] = True
                kappa = (1 + ((lo * np.uint64(RADIX[cl])) >> np.uint64(32))).astype(np.int64)
                loc = site_loc[base + SEG * s + pos]
                for bit in range(4):
                    has = ((kappa >> bit) & 1).astype(bool)
                    out[rows[has]] ^= eff[loc[has] + (bit >> 1), bit & 1]
    return out


def retry_gate_words(gadget, seed, first, count, p1, p2, max_attempts):
    """(words (count, nsteps + F + 1) uint64, attempts (count, preparations) uint32) of samples [first, first + count)."""
    types = []
    for t in gadget.types:
        site_loc, site_regions = t.gate_regions()
        starts = np.concatenate([[0], np.cumsum(site_regions.sum(axis=1))])
        types.append((np.asarray(t.effects, dtype=np.uint64), np.asarray(t.regions), int(t.num_flags), np.asarray(site_loc, dtype=np.int64),
                      np.asarray(site_regions), starts))
    kinds = [int(k) for k in gadget.block_kind]
    nsteps = sum(k != NONE for k in kinds)
    rows = sum(types[t][2] for t in gadget.block_type if t >= 0)
    flag_words = max(1, (rows + 63) // 64)
    preparations = sum(int(types[t][1][:, 2].sum()) for t in gadget.block_type if t >= 0)
    t_class = (int(quantise(p1)), int(quantise(p2)))
    tables = {}
    words = np.zeros((count, nsteps + flag_words + 1), dtype=np.uint64)
    tries = np.zeros((count, preparations), dtype=np.uint32)
    with np.errstate(over="ignore"):
        i = np.arange(count, dtype=np.uint64) + np.uint64(first)
        ks = mix64(_u64(seed) + np.uint64(GOLDEN) * (i + np.uint64(1)))
        T = np.zeros(count, dtype=np.uint64)
        alive = np.ones(count, dtype=bool)
        g = prep = step = flag_row = 0
        for t, kind in zip(gadget.block_type, kinds):
            local, tail = np.zeros(count, dtype=np.uint64), np.zeros(count, dtype=np.uint64)
            if kind != FINAL:
                eff, regions, num_flags, site_loc, site_regions, starts = types[t]
                for r, (_, _, retried) in enumerate(regions.tolist()):
                    n1, n2 = (int(v) for v in site_regions[r])
                    sites = site_loc[starts[r]:starts[r + 1]]
                    kr = mix64(ks + _u64(STREAM_MULT * (retry_ref.SLOT_BASE + g + 1)))
                    got = np.zeros((count, 3), dtype=np.uint64)
                    used = np.zeros(count, dtype=np.uint32)
                    pending, a = alive.copy(), 0
                    while pending.any() and a < (max_attempts if retried else 1):
                        rows_ = np.nonzero(pending)[0]
                        got[rows_] = draw_region(mix64(kr[rows_] + _u64(GOLDEN * (a + 1))), eff, sites, n1, n2, t_class, tables)
                        used[rows_] = a + 1
                        pending[rows_] = got[rows_, 2] != 0
                        a += 1
                    if retried:
                        tries[alive, prep] = used[alive]
                        prep += 1
                    word, shift = divmod(flag_row, 64)                          # the exhausted: `pending` is what is left of `alive`
                    words[pending, nsteps + word] |= got[pending, 2] << np.uint64(shift)
                    if shift and word + 1 < flag_words:
                        words[pending, nsteps + word + 1] |= got[pending, 2] >> np.uint64(64 - shift)
                    alive &= ~pending
                    local ^= got[:, 0]
                    tail ^= got[:, 1]
                    g += 1
                flag_row += num_flags
            if kind != NONE:
                words[alive, step] = (T[alive] & np.uint64(FRAME[kind])) ^ local[alive]
                step += 1
            T ^= tail
    words[:, -1] = tries.sum(axis=1, dtype=np.uint64)
    return words, tries


# -- exact distributions -----------------------------------------------------------------------------------------------------

def region_joint(block, region, p1, p2, local_mask, tail_mask):
    """The exact joint distribution of one attempt of a region under gate faults: index = local bits | tail bits << nl | flag bits
    << (nl + nt), the bits those of the masks (the flag bits: the region's own) packed from bit 0 -- the XOR-convolution of the
    one-operand sites' product distribution (3 points at p1 / 3) and the CNOT sites' (15 points at p2 / 15, each the XOR of the
    effects its kappa mask names).  Returns (dist, nl, nt, nf)."""
    first, size, _ = (int(v) for v in block.regions[region])
    effects = np.asarray(block.effects, dtype=np.uint64)
    eff = effects[first:first + size]
    flag_mask = int(np.bitwise_or.reduce(eff[:, :, 2].reshape(-1)))
    nl, nt, nf = bin(local_mask).count("1"), bin(tail_mask).count("1"), bin(flag_mask).count("1")
    if local_mask or tail_mask:                                                          # (both zero: the flags alone are asked for)
        assert not int(np.bitwise_or.reduce(eff[:, :, 0].reshape(-1))) & ~local_mask
        assert not int(np.bitwise_or.reduce(eff[:, :, 1].reshape(-1))) & ~tail_mask
    cell = _extract(effects[:, :, 0], local_mask) | _extract(effects[:, :, 1], tail_mask) << nl | _extract(effects[:, :, 2], flag_mask) << (nl + nt)
    site_loc, site_regions = block.gate_regions()
    start = int(site_regions[:region].sum())
    n1, n2 = (int(v) for v in site_regions[region])
    one, two = site_loc[start:start + n1].astype(np.int64), site_loc[start + n1:start + n1 + n2].astype(np.int64)
    assert n1 + 2 * n2 == size and (n1 == 0 or (first <= one.min() and one.max() < first + size))
    assert n2 == 0 or (first <= two.min() and two.max() + 1 < first + size)
    parts = [cell[one][:, [0, 1]], cell[two][:, [0, 1]], cell[two + 1][:, [0, 1]]]       # per site: (X, Z) of its location(s)
    bits = nl + nt + nf
    dists = []
    if n1:
        x, z = parts[0][:, 0], parts[0][:, 1]
        dists.append(exact_dist.product_distribution(bits, np.stack([x, z, x ^ z], axis=1), [p1 / 3.0] * 3))      # kappa = 1, 2, 3
    if n2:
        columns = []
        for kappa in range(1, 16):
            point = np.zeros(n2, dtype=np.int64)
            for bit in range(4):
                if (kappa >> bit) & 1:
                    point ^= parts[1 + (bit >> 1)][:, bit & 1]
            columns.append(point)
        dists.append(exact_dist.product_distribution(bits, np.stack(columns, axis=1), [p2 / 15.0] * 15))
    dist = dists[0] if len(dists) == 1 else xor_convolution(dists)
    return dist, nl, nt, nf


def region_pass_probability(block, region, p1, p2):
    """q = P(the flags of one attempt are zero)."""
    dist, _, _, nf = region_joint(block, region, p1, p2, 0, 0)
    return float(dist[0]) if nf else 1.0


def region_conditional(block, region, p1, p2, local_mask, tail_mask):
    """P(local, tail | flags = 0) of a region over nl + nt bits, and q."""
    dist, nl, nt, _ = region_joint(block, region, p1, p2, local_mask, tail_mask)
    accepted = dist[:1 << (nl + nt)]
    q = float(accepted.sum())
    return accepted / q, q


def attempts_mean_var(gadget, p1, p2):
    """Mean and variance of a sample's attempts with unbounded retries: per preparation geometric, 1 / q and (1 - q) / q^2."""
    mean = var = 0.0
    for t in gadget.block_type:
        if t >= 0:
            for r, (_, _, retried) in enumerate(gadget.types[t].regions.tolist()):
                if retried:
                    q = region_pass_probability(gadget.types[t], r, p1, p2)
                    mean, var = mean + 1.0 / q, var + (1.0 - q) / (q * q)
    return mean, var


def prepare_final_distribution(gadget, p1, p2, r_1, r_2):
    """[prepare, FINAL]: the exact P(T | flags = 0) over T's packed bits."""
    return region_conditional(gadget.types[0], 0, p1, p2, 0, frame_mask(r_1, r_2))[0]


def one_round_distribution(gadget, p1, p2, r_1, r_2):
    """The one-round cycle: the exact joint of (step word, T) -- tests/retry_ref.py's index -- as the XOR-convolution of the regions'
    conditional distributions."""
    block = gadget.types[0]
    return xor_convolution([region_conditional(block, r, p1, p2, key_mask(r_1, r_2), frame_mask(r_1, r_2))[0] for r in range(len(block.regions))])


def sparse_share(exact, samples, least=10.0):
    """The share of the mass in cells that expect fewer than `least` of `samples` samples."""
    exact = np.asarray(exact, dtype=np.float64)
    return float(exact[exact * samples < least].sum())
