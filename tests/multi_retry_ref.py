"""
NumPy restatement of the repeat-until-success sampler of multi-block programs (DESIGN.md section 5d "Repeat-until-success of
multi-block programs"), for tests/test_multi_retry.py and tests/test_gpu_multi_retry.py.  Written from the definition alone: it
shares no code with the HIP kernel or with gf2_mretry_words_host (csrc/gf2_host.cpp); of a program it reads the block tables only
(every type's effects, flag rows and regions, the blocks' types, kinds and frames).  mix64, quantise and the constants come from
tests/strata_ref.py, the inverse-CDF table from tests/gate_mc_ref.py, as tests/retry_ref.py takes them.

    ks = mix64(seed + G (i + 1))
    region g (counted through the whole sequence, blocks in order), attempt a:
      kr = mix64(ks + M (2^32 + g + 1)),  ka = mix64(kr + G (a + 1))
    per segment s of 512 of the region's locations (nb = 512, or what is left in the last one):
      d = mix64(ka + M (s + 1)),  K = #{k < nb : (d >> 32) >= cdf[k]},  cdf = the inverse binomial CDF table of (T_any, nb)
      k = 0 .. K - 1:  v = mix64(d + G (k + 1)),  j = nb - K + k,  t = ((v >> 32) (j + 1)) >> 32,
                       position = j if an earlier pick of the segment took t else t,  c = v & (2^32 - 1):  X if c < t_1, Y if c < t_2, else Z
    a region that is not retried: attempt 0; a retried one: the first attempt below max_attempts whose flags are zero, else the
    sample is exhausted -- the walk stops, its later step words stay 0, the flag words hold the last attempt's flags.
    closing a block: CNOT a -> b: T_b ^= T_a & LOW, T_a ^= T_b & HIGH, then T_a ^= first words, T_b ^= second words;
                     any other: word = mask_kind(T_a) ^ local, T_a ^= tail
    words = [EC and MEASURE steps] [flag words] [attempts of the sample]
"""
import numpy as np

from tests.gate_mc_ref import cdf_table
from tests.strata_ref import GOLDEN, STREAM_MULT, mix64, quantise

SEG = 512
SLOT_BASE = 1 << 32
NONE, EC, MEASURE, CNOT = 0, 1, 2, 4
U64 = (1 << 64) - 1
LOW, HIGH = np.uint64(0x00000000FFFFFFFF), np.uint64(0xFFFFFFFF00000000)
FRAME = {NONE: 0, EC: U64 & ~(1 << 31 | 1 << 63), MEASURE: 0xFFFFFFFF}


def _u64(value):
    return np.uint64(value & U64)


def _thresholds(p):
    p_x, p_y, p_z = (float(v) for v in p)
    p_t = p_x + p_y + p_z
    return quantise(p_t), (quantise(p_x / p_t), quantise((p_x + p_y) / p_t)) if p_t > 0.0 else (0, 0)


def _attempt(ka, eff, t_any, t_12, tables):
    """One attempt per key of `ka` over a region's table eff (count, 2, 3): its (local, tail, flags) words (len(ka), 3) and its
    faults as arrays (row of ka, location inside the region, kind 1 X / 2 Z / 3 Y)."""
    count, out = len(eff), np.zeros((len(ka), 3), dtype=np.uint64)
    who, where, what = [np.zeros(0, dtype=np.int64)], [np.zeros(0, dtype=np.int64)], [np.zeros(0, dtype=np.int64)]
    for s in range((count + SEG - 1) // SEG):
        nb = min(SEG, count - SEG * s)
        if nb not in tables:
            tables[nb] = cdf_table(t_any, nb)
        d = mix64(ka + _u64(STREAM_MULT * (s + 1)))
        errors = ((d >> np.uint64(32))[:, None] >= tables[nb][None, :]).sum(axis=1).astype(np.int64)
        taken = np.zeros((len(ka), nb), dtype=bool)
        for k in range(int(errors.max()) if len(ka) else 0):
            rows = np.nonzero(errors > k)[0]
            v = mix64(d[rows] + _u64(GOLDEN * (k + 1)))
            high, c = v >> np.uint64(32), (v & np.uint64(0xFFFFFFFF)).astype(np.int64)
            j = nb - errors[rows] + k
            t = ((high * (j + 1).astype(np.uint64)) >> np.uint64(32)).astype(np.int64)
            pos = np.where(taken[rows, t], j, t)
            taken[rows, pos] = True
            has_x, has_z = c < t_12[1], c >= t_12[0]
            at = SEG * s + pos
            out[rows[has_x]] ^= eff[at[has_x], 0]
            out[rows[has_z]] ^= eff[at[has_z], 1]
            who.append(rows)
            where.append(at)
            what.append(has_x.astype(np.int64) | has_z.astype(np.int64) << 1)
    return out, np.concatenate(who), np.concatenate(where), np.concatenate(what)


def retry_words(program, seed, first, count, p, max_attempts):
    """(words (count, nsteps + F + 1) uint64, attempts (count, preparations) uint32, faults) of samples [first, first + count);
    faults = (fault_first (count + 1,) int64, fault_location int32, fault_kind uint8): per sample, the global location and the kind
    of every fault of the attempts that entered the blocks (a passed attempt of a retried region, the one attempt of another)."""
    types = [(np.asarray(t.effects, dtype=np.uint64), np.asarray(t.regions), int(t.num_flags)) for t in program.types]
    kinds = [int(k) for k in program.block_kind]
    nsteps = sum(k in (EC, MEASURE) for k in kinds)
    flag_rows = sum(types[t][2] for t in program.block_type)
    flag_words = max(1, (flag_rows + 63) // 64)
    preparations = sum(int(types[t][1][:, 2].sum()) for t in program.block_type)
    t_any, t_12 = _thresholds(p)
    tables = {}
    words = np.zeros((count, nsteps + flag_words + 1), dtype=np.uint64)
    tries = np.zeros((count, preparations), dtype=np.uint32)
    f_sample, f_where, f_kind = [np.zeros(0, dtype=np.int64)], [np.zeros(0, dtype=np.int64)], [np.zeros(0, dtype=np.int64)]
    with np.errstate(over="ignore"):
        i = np.arange(count, dtype=np.uint64) + np.uint64(first)
        ks = mix64(_u64(seed) + np.uint64(GOLDEN) * (i + np.uint64(1)))
        T = [np.zeros(count, dtype=np.uint64) for _ in range(int(program.nframes))]
        alive = np.ones(count, dtype=bool)
        g = prep = step = flag_row = block_first = 0
        for t, kind, fa, fb in zip(program.block_type, kinds, program.block_a, program.block_b):
            one, two = np.zeros(count, dtype=np.uint64), np.zeros(count, dtype=np.uint64)
            eff, regions, num_flags = types[t]
            for start, size, retried in regions.tolist():
                kr = mix64(ks + _u64(STREAM_MULT * (SLOT_BASE + g + 1)))
                got = np.zeros((count, 3), dtype=np.uint64)
                used = np.zeros(count, dtype=np.uint32)
                pending, a = alive.copy(), 0
                while pending.any() and a < (max_attempts if retried else 1):
                    rows = np.nonzero(pending)[0]
                    got[rows], who, where, what = _attempt(mix64(kr[rows] + _u64(GOLDEN * (a + 1))), eff[start:start + size], t_any, t_12, tables)
                    used[rows] = a + 1
                    pending[rows] = got[rows, 2] != 0
                    entered = ~pending[rows[who]]                               # the faults of an attempt that passed
                    f_sample.append(rows[who][entered])
                    f_where.append(block_first + start + where[entered])
                    f_kind.append(what[entered])
                    a += 1
                if retried:
                    tries[alive, prep] = used[alive]
                    prep += 1
                word, shift = divmod(flag_row, 64)                              # the exhausted: `pending` is what is left of `alive`
                words[pending, nsteps + word] |= got[pending, 2] << np.uint64(shift)
                if shift and word + 1 < flag_words:
                    words[pending, nsteps + word + 1] |= got[pending, 2] >> np.uint64(64 - shift)
                alive &= ~pending
                one ^= got[:, 0]
                two ^= got[:, 1]
                g += 1
            flag_row += num_flags
            block_first += len(eff)
            if kind == CNOT:
                T[fb] ^= T[fa] & LOW
                T[fa] ^= T[fb] & HIGH
                T[fa] ^= one
                T[fb] ^= two
            else:
                if kind != NONE:
                    words[alive, step] = (T[fa][alive] & np.uint64(FRAME[kind])) ^ one[alive]
                    step += 1
                T[fa] ^= two
    words[:, -1] = tries.sum(axis=1, dtype=np.uint64)
    sample, where, what = np.concatenate(f_sample), np.concatenate(f_where), np.concatenate(f_kind)
    order = np.argsort(sample, kind="stable")
    fault_first = np.concatenate([[0], np.cumsum(np.bincount(sample, minlength=count))]).astype(np.int64)
    return words, tries, (fault_first, where[order].astype(np.int32), what[order].astype(np.uint8))
