"""
NumPy restatement of the repeat-until-success sampler under gate-level faults with waiting faults (DESIGN.md section 5d
"Repeat-until-success with waiting faults under gate-level faults"), for tests/test_retry_gate_wait.py and
tests/test_gpu_retry_gate_wait.py, and the exact distributions its samples must follow.  Written from the definition alone: it
shares no code with the HIP kernel or with gf2_host.cpp.  A region's own draw is tests/retry_gate_ref.py's draw_region and its wait
draw tests/retry_wait_ref.py's draw_wait, both unchanged; the walk is restated here because the two live inside it.

    everything of tests/retry_gate_ref.py's definition, and for region g with W_g > 0 wait rows and every attempt a actually made:
      kw = mix64(ks + M (2^33 + g + 1)),  kwa = mix64(kw + G (a + 1)),  d = mix64(kwa + M)
      K, the picks, Floyd's rule and the kinds: tests/retry_wait_ref.py's, with q's thresholds
      the picked rows' (local, tail) are XORed into the block's local and tail, for every attempt made
    words = [steps] [flag words] [attempts of the sample] [wait faults drawn over all attempts of the sample]
"""
import numpy as np

from oracle import exact_dist
from tests import retry_gate_ref, retry_ref, retry_wait_ref
from tests.retry_ref import FINAL, FRAME, NONE, _u64, frame_mask, key_mask, thresholds
from tests.strata_ref import GOLDEN, STREAM_MULT, mix64, quantise


def tables_of(gadget, wait_steps=1):
    """(types, block_type, block_kind, waits) of a StreamedGadget: what retry_gate_wait_words reads.  A type is (effects, regions,
    flag rows, site_loc, site_regions)."""
    types = [(np.asarray(t.effects, dtype=np.uint64), np.asarray(t.regions), int(t.num_flags)) + tuple(t.gate_regions()) for t in gadget.types]
    waits = [t.waits(wait_steps) for t in gadget.types]
    return types, [int(t) for t in gadget.block_type], [int(k) for k in gadget.block_kind], waits


def retry_gate_wait_words(types, block_type, block_kind, waits, seed, first, count, p1, p2, q, max_attempts):
    """(words (count, nsteps + F + 2) uint64, attempts (count, preparations) uint32) of samples [first, first + count)."""
    nsteps = sum(k != NONE for k in block_kind)
    rows = sum(types[t][2] for t in block_type if t >= 0)
    flag_words = max(1, (rows + 63) // 64)
    preparations = sum(int(types[t][1][:, 2].sum()) for t in block_type if t >= 0)
    t_class = (int(quantise(p1)), int(quantise(p2)))
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
                eff, regions, num_flags, site_loc, site_regions = types[t]
                site_loc, site_regions = np.asarray(site_loc, dtype=np.int64), np.asarray(site_regions)
                starts = np.concatenate([[0], np.cumsum(site_regions.sum(axis=1))])
                wait_eff, wait_count = waits[t]
                wait_first = np.concatenate([[0], np.cumsum(wait_count)])
                for r, (_, _, retried) in enumerate(regions.tolist()):
                    n1, n2 = (int(v) for v in site_regions[r])
                    sites = site_loc[starts[r]:starts[r + 1]]
                    kr = mix64(ks + _u64(STREAM_MULT * (retry_ref.SLOT_BASE + g + 1)))
                    kw = mix64(ks + _u64(STREAM_MULT * (retry_wait_ref.WAIT_SLOT_BASE + g + 1)))
                    wait_rows = np.asarray(wait_eff, dtype=np.uint64).reshape(-1, 2, 2)[int(wait_first[r]):int(wait_first[r + 1])]
                    got = np.zeros((count, 3), dtype=np.uint64)
                    waited = np.zeros((count, 2), dtype=np.uint64)              # never cleared between attempts
                    used = np.zeros(count, dtype=np.uint32)
                    pending, a = alive.copy(), 0
                    while pending.any() and a < (max_attempts if retried else 1):
                        rows_ = np.nonzero(pending)[0]
                        got[rows_] = retry_gate_ref.draw_region(mix64(kr[rows_] + _u64(GOLDEN * (a + 1))), eff, sites, n1, n2, t_class, tables)
                        if len(wait_rows):
                            hit, K = retry_wait_ref.draw_wait(mix64(kw[rows_] + _u64(GOLDEN * (a + 1))), wait_rows, w_any, w_12, wait_tables)
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

def attempts_law(block, region, p1, p2, max_attempts):
    """P(A = a | not exhausted), a = 1 .. max_attempts, of a retried region: geometric with the gate model's pass probability,
    truncated."""
    s = retry_gate_ref.region_pass_probability(block, region, p1, p2)
    law = s * (1.0 - s) ** np.arange(max_attempts, dtype=np.float64)
    return law / law.sum()


def region_distribution(block, region, wait_rows, p1, p2, q, local_mask, tail_mask, max_attempts=256):
    """The exact distribution of a region over (local, tail): tests/retry_gate_ref.py's region_conditional XOR-convolved with
    sum_a P(A = a | not exhausted) W^{*a}, W one attempt's wait noise (tests/retry_wait_ref.py's wait_noise) -- the attempts are
    independent of the accepted attempt's content and of the wait draws."""
    accepted, _ = retry_gate_ref.region_conditional(block, region, p1, p2, local_mask, tail_mask)
    if not int(block.regions[region][2]) or not len(wait_rows):
        return accepted
    spectrum = exact_dist.fwht(np.array(retry_wait_ref.wait_noise(wait_rows, q, local_mask, tail_mask), dtype=np.float64))   # W^{*a} has spectrum^a
    mixed = np.zeros_like(spectrum)
    power = np.ones_like(spectrum)
    for weight in attempts_law(block, region, p1, p2, max_attempts):
        power = power * spectrum
        mixed += weight * power
    out = exact_dist.fwht(exact_dist.fwht(np.array(accepted, dtype=np.float64)) * mixed) / float(len(mixed))
    return np.clip(out, 0.0, 1.0)


def one_round_distribution(gadget, p1, p2, q, r_1, r_2, wait_steps=1, max_attempts=256):
    """The one-round cycle with waiting faults under gate-level faults: the exact joint of (step word, T), tests/retry_ref.py's index."""
    block = gadget.types[0]
    wait_eff, wait_count = block.waits(wait_steps)
    first = np.concatenate([[0], np.cumsum(wait_count)])
    return retry_ref.xor_convolution([region_distribution(block, r, wait_eff[int(first[r]):int(first[r + 1])], p1, p2, q, key_mask(r_1, r_2),
                                                          frame_mask(r_1, r_2), max_attempts) for r in range(len(block.regions))])


def wait_faults_mean_var(gadget, p1, p2, q, wait_steps=1):
    """(mean, variance, mean if only the accepted attempt waited, attempts per preparation) of a sample's wait faults with unbounded
    retries: tests/retry_wait_ref.py's form -- per region a sum of A_g binomials (W_g, q_t), A_g geometric -- with the gate model's
    pass probabilities."""
    q_t = retry_wait_ref.quantised_total(q)
    mean = var = once = attempts = 0.0
    preparations = 0
    passes = {}                                                                  # per (type, region): a long sequence repeats its types
    for t in gadget.block_type:
        if t >= 0:
            block = gadget.types[t]
            for r, ((_, _, retried), w) in enumerate(zip(block.regions.tolist(), block.waits(wait_steps)[1].tolist())):
                if retried:
                    if (t, r) not in passes:
                        passes[t, r] = retry_gate_ref.region_pass_probability(block, r, p1, p2)
                    s = passes[t, r]
                    e_a, v_a = 1.0 / s, (1.0 - s) / (s * s)
                    mean += w * q_t * e_a
                    var += e_a * w * q_t * (1.0 - q_t) + v_a * (w * q_t) ** 2
                    once += w * q_t
                    attempts, preparations = attempts + e_a, preparations + 1
    return mean, var, once, attempts / max(1, preparations)
