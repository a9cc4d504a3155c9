"""
NumPy restatement of the repeat-until-success sampler with waiting faults (DESIGN.md section 5d "Repeat-until-success with waiting
faults"), for tests/test_retry_wait.py and tests/test_gpu_retry_wait.py, and the exact distributions its samples must follow.  Written
from the definition alone: it shares no code with the HIP kernel or with gf2_host.cpp; of a sequence it reads the block tables (every
type's effects, regions and flag rows, the blocks' types and kinds) and the wait tables (every type's wait rows and wait counts).  A
region's own draw is tests/retry_ref.py's draw_region, unchanged; the walk is restated here because the wait draws live inside it.

    everything of tests/retry_ref.py's definition, and for region g with W_g > 0 wait rows and every attempt a actually made:
      kw = mix64(ks + M (2^33 + g + 1)),  kwa = mix64(kw + G (a + 1)),  d = mix64(kwa + M)
      K = #{k < W_g : (d >> 32) >= cdf[k]},  cdf = the inverse binomial CDF table of (T_any(q), W_g)
      picks, Floyd's rule and kinds as for a region's segment, with q's thresholds
      the picked rows' (local, tail) are XORed into the block's local and tail, for every attempt made
    words = [steps] [flag words] [attempts of the sample] [wait faults drawn over all attempts of the sample]
"""
import numpy as np

from oracle import exact_dist
from tests import retry_ref
from tests.gate_mc_ref import cdf_table
from tests.retry_ref import FINAL, FRAME, NONE, _extract, _u64, frame_mask, key_mask, thresholds
from tests.strata_ref import GOLDEN, STREAM_MULT, mix64

WAIT_SLOT_BASE = 1 << 33


def tables_of(gadget, wait_steps=1):
    """(types, block_type, block_kind, waits) of a StreamedGadget: what retry_wait_words reads."""
    types = [(np.asarray(t.effects, dtype=np.uint64), np.asarray(t.regions), int(t.num_flags)) for t in gadget.types]
    waits = [t.waits(wait_steps) for t in gadget.types]
    return types, [int(t) for t in gadget.block_type], [int(k) for k in gadget.block_kind], waits


def draw_wait(kwa, rows, w_any, w_12, tables):
    """((local, tail) per key, K per key) of one attempt's wait draw over a region's wait rows (W, 2, 2)."""
    count = len(rows)
    if count not in tables:
        tables[count] = cdf_table(w_any, count)
    d = mix64(kwa + _u64(STREAM_MULT))
    K = ((d >> np.uint64(32))[:, None] >= tables[count][None, :]).sum(axis=1).astype(np.int64)
    padded = np.zeros((count, 2, 3), dtype=np.uint64)
    padded[:, :, :2] = rows
    return retry_ref.draw_region(kwa, padded, w_any, w_12, {count: tables[count]})[:, :2], K


def retry_wait_words(types, block_type, block_kind, waits, seed, first, count, p, q, max_attempts):
    """(words (count, nsteps + F + 2) uint64, attempts (count, preparations) uint32) of samples [first, first + count)."""
    nsteps = sum(k != NONE for k in block_kind)
    rows = sum(types[t][2] for t in block_type if t >= 0)
    flag_words = max(1, (rows + 63) // 64)
    preparations = sum(int(types[t][1][:, 2].sum()) for t in block_type if t >= 0)
    t_any, t_12 = thresholds(p)
    w_any, w_12 = thresholds(q)
    tables, wait_tables = {}, {}
    words = np.zeros((count, nsteps + flag_words + 2), dtype=np.uint64)
    tries = np.zeros((count, preparations), dtype=np.uint32)
    faults = np.zeros(count, dtype=np.uint64)
    with np.errstate(over="ignore"):
        i = np.arange(count, dtype=np.uint64) + np.uint64(first)
        ks = mix64(_u64(seed) + np.uint64(GOLDEN) * (i + np.uint64(1)))
        T = np.zeros(count, dtype=np.uint64)
        alive = np.ones(count, dtype=bool)
        g = prep = step = flag_row = 0
        for t, kind in zip(block_type, block_kind):
            local, tail = np.zeros(count, dtype=np.uint64), np.zeros(count, dtype=np.uint64)
            if kind != FINAL:
                eff, regions, num_flags = types[t]
                wait_eff, wait_count = waits[t]
                wait_first = np.concatenate([[0], np.cumsum(wait_count)])
                for r, (start, size, retried) in enumerate(regions.tolist()):
                    kr = mix64(ks + _u64(STREAM_MULT * (retry_ref.SLOT_BASE + g + 1)))
                    kw = mix64(ks + _u64(STREAM_MULT * (WAIT_SLOT_BASE + g + 1)))
                    wait_rows = np.asarray(wait_eff, dtype=np.uint64).reshape(-1, 2, 2)[int(wait_first[r]):int(wait_first[r + 1])]
                    got = np.zeros((count, 3), dtype=np.uint64)
                    waited = np.zeros((count, 2), dtype=np.uint64)              # never cleared between attempts
                    used = np.zeros(count, dtype=np.uint32)
                    pending, a = alive.copy(), 0
                    while pending.any() and a < (max_attempts if retried else 1):
                        rows_ = np.nonzero(pending)[0]
                        got[rows_] = retry_ref.draw_region(mix64(kr[rows_] + _u64(GOLDEN * (a + 1))), eff[start:start + size], t_any, t_12, tables)
                        if len(wait_rows):
                            hit, K = draw_wait(mix64(kw[rows_] + _u64(GOLDEN * (a + 1))), wait_rows, w_any, w_12, wait_tables)
                            waited[rows_] ^= hit
                            faults[rows_] += K.astype(np.uint64)
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
                    local ^= got[:, 0] ^ waited[:, 0]
                    tail ^= got[:, 1] ^ waited[:, 1]
                    g += 1
                flag_row += num_flags
            if kind != NONE:
                words[alive, step] = (T[alive] & np.uint64(FRAME[kind])) ^ local[alive]
                step += 1
            T ^= tail
    words[:, -2] = tries.sum(axis=1, dtype=np.uint64)
    words[:, -1] = faults
    return words, tries


# -- exact distributions (consequence 4) -------------------------------------------------------------------------------------------

def quantised_total(rates):
    """The total rate the sampler really uses: T_any / 2^32."""
    return thresholds(rates)[0] / 4294967296.0


def attempts_law(block, region, p, max_attempts):
    """P(A = a | not exhausted), a = 1 .. max_attempts, of a retried region: the geometric law of tests/retry_ref.py's
    attempts_mean_var, truncated."""
    s = retry_ref.region_pass_probability(block, region, p)
    law = s * (1.0 - s) ** np.arange(max_attempts, dtype=np.float64)
    return law / law.sum()


def wait_noise(rows, q, local_mask, tail_mask):
    """One attempt's wait noise of a region over (local bits | tail bits << nl): the product distribution of its wait rows."""
    rows = np.asarray(rows, dtype=np.uint64).reshape(-1, 2, 2)
    nl, nt = bin(local_mask).count("1"), bin(tail_mask).count("1")
    cell = _extract(rows[:, :, 0], local_mask) | _extract(rows[:, :, 1], tail_mask) << nl
    points = np.stack([cell[:, 0], cell[:, 0] ^ cell[:, 1], cell[:, 1]], axis=1)          # X, Y, Z
    return exact_dist.product_distribution(nl + nt, points, [float(v) for v in q])


def region_distribution(block, region, wait_rows, p, q, local_mask, tail_mask, max_attempts=256):
    """The exact distribution of a region over (local, tail): its conditional distribution given flags = 0 XOR-convolved with
    sum_a P(A = a | not exhausted) W^{*a}, W one attempt's wait noise -- the attempts are independent of the accepted attempt's
    content and of the wait draws."""
    accepted, _ = retry_ref.region_conditional(block, region, p, local_mask, tail_mask)
    if not int(block.regions[region][2]) or not len(wait_rows):
        return accepted
    spectrum = exact_dist.fwht(np.array(wait_noise(wait_rows, q, local_mask, tail_mask), dtype=np.float64))   # of W; W^{*a} has spectrum^a
    mixed = np.zeros_like(spectrum)
    power = np.ones_like(spectrum)
    for weight in attempts_law(block, region, p, max_attempts):
        power = power * spectrum
        mixed += weight * power
    out = exact_dist.fwht(exact_dist.fwht(np.array(accepted, dtype=np.float64)) * mixed) / float(len(mixed))
    return np.clip(out, 0.0, 1.0)


def one_round_distribution(gadget, p, q, r_1, r_2, wait_steps=1, max_attempts=256):
    """The one-round cycle with waiting faults: the exact joint of (step word, T), tests/retry_ref.py's one_round_distribution with
    every retried region's distribution convolved with its wait noise."""
    block = gadget.types[0]
    wait_eff, wait_count = block.waits(wait_steps)
    first = np.concatenate([[0], np.cumsum(wait_count)])
    return retry_ref.xor_convolution([region_distribution(block, r, wait_eff[int(first[r]):int(first[r + 1])], p, q, key_mask(r_1, r_2),
                                                          frame_mask(r_1, r_2), max_attempts) for r in range(len(block.regions))])


def wait_faults_mean_var(gadget, p, q, wait_steps=1):
    """(mean, variance, mean if only the accepted attempt waited, attempts per preparation) of a sample's wait faults with unbounded
    retries: per region a sum of A_g binomials (W_g, q_t), A_g geometric with the region's pass probability."""
    q_t = quantised_total(q)
    mean = var = once = attempts = 0.0
    preparations = 0
    for t in gadget.block_type:
        if t >= 0:
            block = gadget.types[t]
            for r, ((_, _, retried), w) in enumerate(zip(block.regions.tolist(), block.waits(wait_steps)[1].tolist())):
                if retried:
                    s = retry_ref.region_pass_probability(block, r, p)
                    e_a, v_a = 1.0 / s, (1.0 - s) / (s * s)
                    mean += w * q_t * e_a
                    var += e_a * w * q_t * (1.0 - q_t) + v_a * (w * q_t) ** 2
                    once += w * q_t
                    attempts, preparations = attempts + e_a, preparations + 1
    return mean, var, once, attempts / max(1, preparations)
