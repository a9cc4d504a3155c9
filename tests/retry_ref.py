"""
NumPy restatement of the repeat-until-success sampler (DESIGN.md section 5d "Repeat-until-success"), for tests/test_retry.py and
tests/test_gpu_retry.py, and the exact distributions its samples must follow.  Written from the definition alone: it shares no code
with the HIP kernel or with gf2_retry_words_host (csrc/gf2_host.cpp); of a gadget it reads the block tables only (every type's
effects, flag rows and regions, the blocks' types and kinds).  mix64, quantise and the constants come from tests/strata_ref.py, the
inverse-CDF table from tests/gate_mc_ref.py, themselves such restatements.

    ks = mix64(seed + G (i + 1))
    region g (counted through the whole sequence), attempt a:  kr = mix64(ks + M (2^32 + g + 1)),  ka = mix64(kr + G (a + 1))
    per segment s of 512 of the region's locations (nb = 512, or what is left in the last one):
      d = mix64(ka + M (s + 1)),  K = #{k < nb : (d >> 32) >= cdf[k]},  cdf = the inverse binomial CDF table of (T_any, nb)
      k = 0 .. K - 1:  v = mix64(d + G (k + 1)),  j = nb - K + k,  t = ((v >> 32) (j + 1)) >> 32,
                       position = j if an earlier pick of the segment took t else t,  c = v & (2^32 - 1):  X if c < t_1, Y if c < t_2, else Z
    a region that is not retried: attempt 0; a retried one: the first attempt below max_attempts whose flags are zero, else the
    sample is exhausted -- the walk stops, its later step words stay 0, the flag words hold the last attempt's flags.
    block after block: word = mask_kind(T) ^ local, T ^= tail;  words = [steps] [flag words] [attempts of the sample]
"""
import numpy as np

from oracle import exact_dist
from tests.gate_mc_ref import cdf_table
from tests.strata_ref import GOLDEN, STREAM_MULT, mix64, quantise

SEG = 512
SLOT_BASE = 1 << 32
NONE, EC, MEASURE, FINAL = 0, 1, 2, 3
U64 = (1 << 64) - 1
FRAME = {NONE: 0, EC: U64 & ~(1 << 31 | 1 << 63), MEASURE: 0xFFFFFFFF, FINAL: U64}


def _u64(value):
    return np.uint64(value & U64)


def thresholds(p):
    p_x, p_y, p_z = (float(v) for v in p)
    p_t = p_x + p_y + p_z
    return quantise(p_t), (quantise(p_x / p_t), quantise((p_x + p_y) / p_t)) if p_t > 0.0 else (0, 0)


def draw_region(ka, eff, t_any, t_12, tables):
    """(local, tail, flags) of one attempt per key of `ka` over a region's table eff (count, 2, 3)."""
    count, out = len(eff), np.zeros((len(ka), 3), dtype=np.uint64)
    for s in range((count + SEG - 1) // SEG):
        nb = min(SEG, count - SEG * s)
        if nb not in tables:
            tables[nb] = cdf_table(t_any, nb)
        d = mix64(ka + _u64(STREAM_MULT * (s + 1)))
        K = ((d >> np.uint64(32))[:, None] >= tables[nb][None, :]).sum(axis=1).astype(np.int64)
        taken = np.zeros((len(ka), nb), dtype=bool)
        for k in range(int(K.max()) if len(ka) else 0):
            rows = np.nonzero(K > k)[0]
            v = mix64(d[rows] + _u64(GOLDEN * (k + 1)))
            hi, c = v >> np.uint64(32), (v & np.uint64(0xFFFFFFFF)).astype(np.int64)
            j = nb - K[rows] + k
            t = ((hi * (j + 1).astype(np.uint64)) >> np.uint64(32)).astype(np.int64)
            pos = np.where(taken[rows, t], j, t)
            taken[rows, pos] = True
            has_x, has_z = c < t_12[1], c >= t_12[0]
            where = SEG * s + pos
            out[rows[has_x]] ^= eff[where[has_x], 0]
            out[rows[has_z]] ^= eff[where[has_z], 1]
    return out


def retry_words(gadget, seed, first, count, p, max_attempts):
    """(words (count, nsteps + F + 1) uint64, attempts (count, preparations) uint32) of samples [first, first + count)."""
    types = [(np.asarray(t.effects, dtype=np.uint64), np.asarray(t.regions), int(t.num_flags)) for t in gadget.types]
    kinds = [int(k) for k in gadget.block_kind]
    nsteps = sum(k != NONE for k in kinds)
    rows = sum(types[t][2] for t in gadget.block_type if t >= 0)
    flag_words = max(1, (rows + 63) // 64)
    preparations = sum(int(types[t][1][:, 2].sum()) for t in gadget.block_type if t >= 0)
    t_any, t_12 = thresholds(p)
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
                eff, regions, num_flags = types[t]
                for start, size, retried in regions.tolist():
                    kr = mix64(ks + _u64(STREAM_MULT * (SLOT_BASE + g + 1)))
                    got = np.zeros((count, 3), dtype=np.uint64)
                    used = np.zeros(count, dtype=np.uint32)
                    pending, a = alive.copy(), 0
                    while pending.any() and a < (max_attempts if retried else 1):
                        rows_ = np.nonzero(pending)[0]
                        got[rows_] = draw_region(mix64(kr[rows_] + _u64(GOLDEN * (a + 1))), eff[start:start + size], t_any, t_12, tables)
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

def _extract(values, mask):
    """The bits of `values` (uint64 array) at the set bits of `mask`, packed from bit 0 (int64)."""
    values = np.asarray(values, dtype=np.uint64)
    out, at, bit = np.zeros(values.shape, dtype=np.int64), 0, 0
    while mask >> bit:                                                          # run by run of set bits
        if (mask >> bit) & 1:
            run = 1
            while (mask >> (bit + run)) & 1:
                run += 1
            out |= ((values >> np.uint64(bit)) & np.uint64((1 << run) - 1)).astype(np.int64) << at
            at, bit = at + run, bit + run
        else:
            bit += 1
    return out


def frame_mask(r_1, r_2):
    """The bits a data frame T can have: key_x, bit 31, key_z from bit 32, bit 63; a step word's key bits are those below 31 / 63."""
    return ((1 << r_2) - 1) | 1 << 31 | ((1 << r_1) - 1) << 32 | 1 << 63


def key_mask(r_1, r_2):
    return ((1 << r_2) - 1) | ((1 << r_1) - 1) << 32


def region_joint(block, region, p, local_mask, tail_mask):
    """The exact joint distribution of one attempt of a region: index = local bits | tail bits << nl | flag bits << (nl + nt), the
    bits those of the masks (the flag bits: the region's own) packed from bit 0.  Returns (dist, nl, nt, nf)."""
    first, size, _ = (int(v) for v in block.regions[region])
    eff = np.asarray(block.effects, dtype=np.uint64)[first:first + size]
    flag_mask = int(np.bitwise_or.reduce(eff[:, :, 2].reshape(-1)))
    nl, nt, nf = bin(local_mask).count("1"), bin(tail_mask).count("1"), bin(flag_mask).count("1")
    if local_mask or tail_mask:                                                          # (both zero: the flags alone are asked for)
        assert not int(np.bitwise_or.reduce(eff[:, :, 0].reshape(-1))) & ~local_mask
        assert not int(np.bitwise_or.reduce(eff[:, :, 1].reshape(-1))) & ~tail_mask
    cell = _extract(eff[:, :, 0], local_mask) | _extract(eff[:, :, 1], tail_mask) << nl | _extract(eff[:, :, 2], flag_mask) << (nl + nt)
    points = np.stack([cell[:, 0], cell[:, 0] ^ cell[:, 1], cell[:, 1]], axis=1)          # X, Y, Z
    return exact_dist.product_distribution(nl + nt + nf, points, [float(v) for v in p]), nl, nt, nf


def region_pass_probability(block, region, p):
    """q = P(the flags of one attempt are zero)."""
    dist, _, _, nf = region_joint(block, region, p, 0, 0)
    return float(dist[0]) if nf else 1.0


def region_conditional(block, region, p, local_mask, tail_mask):
    """P(local, tail | flags = 0) of a region over nl + nt bits, and q."""
    dist, nl, nt, _ = region_joint(block, region, p, local_mask, tail_mask)
    accepted = dist[:1 << (nl + nt)]
    q = float(accepted.sum())
    return accepted / q, q


def xor_convolution(dists):
    """The distribution of the XOR of independent variables with the given distributions over [0, 2^m)."""
    spectrum = np.ones(len(dists[0]), dtype=np.float64)
    for dist in dists:
        spectrum *= exact_dist.fwht(np.array(dist, dtype=np.float64))
    out = exact_dist.fwht(spectrum) / float(len(spectrum))
    return np.clip(out, 0.0, 1.0)


def attempts_mean_var(gadget, p):
    """Mean and variance of a sample's attempts with unbounded retries: per preparation geometric, 1 / q and (1 - q) / q^2."""
    mean = var = 0.0
    for t in gadget.block_type:
        if t >= 0:
            for r, (_, _, retried) in enumerate(gadget.types[t].regions.tolist()):
                if retried:
                    q = region_pass_probability(gadget.types[t], r, p)
                    mean, var = mean + 1.0 / q, var + (1.0 - q) / (q * q)
    return mean, var


def prepare_final_distribution(gadget, p, r_1, r_2):
    """[prepare, FINAL]: the exact P(T | flags = 0) over T's packed bits."""
    dist, _ = region_conditional(gadget.types[0], 0, p, 0, frame_mask(r_1, r_2))
    return dist


def prepare_final_cells(words, r_1, r_2):
    return _extract(words[:, 0], frame_mask(r_1, r_2))


def one_round_distribution(gadget, p, r_1, r_2):
    """The one-round cycle: the exact joint of (step word, T) -- index = key bits of the round's word | T's bits << (r_1 + r_2) -- as
    the XOR-convolution of the regions' conditional distributions."""
    block = gadget.types[0]
    return xor_convolution([region_conditional(block, r, p, key_mask(r_1, r_2), frame_mask(r_1, r_2))[0] for r in range(len(block.regions))])


def one_round_cells(words, r_1, r_2):
    return _extract(words[:, 0], key_mask(r_1, r_2)) | _extract(words[:, 1], frame_mask(r_1, r_2)) << (r_1 + r_2)
