"""
NumPy restatement of the repeat-until-success sampler of multi-block programs under gate-level faults (DESIGN.md section 5d
"Repeat-until-success of multi-block programs under gate-level faults"), for tests/test_multi_retry_gate.py and
tests/test_gpu_multi_retry_gate.py, and the exact laws its samples must follow.  Written from the definition alone: it shares no code
with the HIP kernel or with gf2_mretry_gate_words_host (csrc/gf2_host.cpp); of a program it reads the block tables only (every type's
effects, flag rows, regions and sites, the blocks' types, kinds and frames).  mix64, quantise and the constants come from
tests/strata_ref.py, the inverse-CDF table, the slots and the radices from tests/gate_mc_ref.py, themselves such restatements.

    ks = mix64(seed + G (i + 1))
    region g (counted through the whole sequence, blocks in order, the CNOT blocks' regions included), attempt a:
      kr = mix64(ks + M (2^32 + g + 1)),  ka = mix64(kr + G (a + 1))
    under ka, per class of the region's sites -- class 0: its n1 one-operand sites, radix 3, T = quantise(p1), slot base 4096;
    class 1: its n2 CNOT sites, radix 15, T = quantise(p2), slot base 8192 -- and per segment s of 512 of the class's sites:
      d = mix64(ka + M (slot base + s + 1)),  K = #{k < nb : (d >> 32) >= cdf[k]},  cdf = the inverse binomial CDF table of (T, nb)
      k = 0 .. K - 1:  v = mix64(d + G (k + 1)),  j = nb - K + k,  t = ((v >> 32) (j + 1)) >> 32,
                       position = j if an earlier pick of the segment took t else t,  kappa = 1 + (((v & (2^32 - 1)) radix) >> 32)
    an event is the location faults (site_loc[site], kappa & 3) and, for a CNOT, (site_loc[site] + 1, kappa >> 2), kind 1 X, 2 Z, 3 Y,
    kind 0 none; (first, second, flags) ^= the X row of a fault with kind & 1, the Z row of one with kind & 2
    a region that is not retried: attempt 0; a retried one: the first attempt below max_attempts whose flags are zero, else the
    sample is exhausted -- the walk stops, its later step words stay 0, the flag words hold the last attempt's flags.
    closing a block: CNOT a -> b: T_b ^= T_a & LOW, T_a ^= T_b & HIGH, then T_a ^= first words, T_b ^= second words;
                     any other: word = mask_kind(T_a) ^ first (local), T_a ^= second (tail)
    words = [EC and MEASURE steps] [flag words] [attempts of the sample]
"""
import numpy as np

from tests import retry_gate_ref
from tests.gate_mc_ref import RADIX, SEG, SLOT_BASE, cdf_table
from tests.retry_ref import _extract, frame_mask, key_mask, xor_convolution
from tests.strata_ref import GOLDEN, STREAM_MULT, mix64, quantise

REGION_SLOT_BASE = 1 << 32
NONE, EC, MEASURE, CNOT = 0, 1, 2, 4
U64 = (1 << 64) - 1
LOW, HIGH = np.uint64(0x00000000FFFFFFFF), np.uint64(0xFFFFFFFF00000000)
FRAME = {NONE: 0, EC: U64 & ~(1 << 31 | 1 << 63), MEASURE: 0xFFFFFFFF}


def _u64(value):
    return np.uint64(value & U64)


def _attempt(ka, eff, sites, n1, n2, t_class, tables):
    """One attempt per key of `ka` over a type's table eff (L_b, 2, 3) and a region's sites (its n1 one-operand sites, then its n2
    CNOT sites, type-local first locations): its three words (len(ka), 3) and its location faults as arrays (row of ka, type-local
    location, kind), a CNOT event expanded into its one or two location faults."""
    out = np.zeros((len(ka), 3), dtype=np.uint64)
    who, where, what = [np.zeros(0, dtype=np.int64)], [np.zeros(0, dtype=np.int64)], [np.zeros(0, dtype=np.int64)]
    for cl, (m, base) in enumerate(((n1, 0), (n2, n1))):
        for s in range((m + SEG - 1) // SEG):
            nb = min(SEG, m - SEG * s)
            if (cl, nb) not in tables:
                tables[cl, nb] = cdf_table(t_class[cl], nb)
            d = mix64(ka + _u64(STREAM_MULT * (SLOT_BASE[cl] + s + 1)))
            errors = ((d >> np.uint64(32))[:, None] >= tables[cl, nb][None, :]).sum(axis=1).astype(np.int64)
            taken = np.zeros((len(ka), nb), dtype=bool)
            for k in range(int(errors.max()) if len(ka) else 0):
                rows = np.nonzero(errors > k)[0]
                v = mix64(d[rows] + _u64(GOLDEN * (k + 1)))
                high, low = v >> np.uint64(32), v & np.uint64(0xFFFFFFFF)
                j = nb - errors[rows] + k
                t = ((high * (j + 1).astype(np.uint64)) >> np.uint64(32)).astype(np.int64)
                pos = np.where(taken[rows, t], j, t)
                taken[rows, pos] = True
                kappa = (1 + ((low * np.uint64(RADIX[cl])) >> np.uint64(32))).astype(np.int64)
                loc = sites[base + SEG * s + pos]
                for operand in range(cl + 1):
                    kind = (kappa >> (2 * operand)) & 3
                    hit = kind != 0
                    has_x, has_z = (kind & 1) != 0, (kind & 2) != 0
                    out[rows[has_x]] ^= eff[loc[has_x] + operand, 0]
                    out[rows[has_z]] ^= eff[loc[has_z] + operand, 1]
                    who.append(rows[hit])
                    where.append(loc[hit] + operand)
                    what.append(kind[hit])
    return out, np.concatenate(who), np.concatenate(where), np.concatenate(what)


def retry_gate_words(program, seed, first, count, p1, p2, max_attempts):
    """(words (count, nsteps + F + 1) uint64, attempts (count, preparations) uint32, faults) of samples [first, first + count);
    faults = (fault_first (count + 1,) int64, fault_location int32, fault_kind uint8): per sample, the global location and the kind
    of every location fault of the attempts that entered the blocks (a passed attempt of a retried region, the one attempt of
    another)."""
    types = []
    for t in program.types:
        site_loc, site_regions = t.gate_regions()
        starts = np.concatenate([[0], np.cumsum(np.asarray(site_regions).sum(axis=1))])
        types.append((np.asarray(t.effects, dtype=np.uint64), np.asarray(t.regions), int(t.num_flags), np.asarray(site_loc, dtype=np.int64),
                      np.asarray(site_regions), starts))
    kinds = [int(k) for k in program.block_kind]
    nsteps = sum(k in (EC, MEASURE) for k in kinds)
    flag_rows = sum(types[t][2] for t in program.block_type)
    flag_words = max(1, (flag_rows + 63) // 64)
    preparations = sum(int(types[t][1][:, 2].sum()) for t in program.block_type)
    t_class = (int(quantise(p1)), int(quantise(p2)))
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
            eff, regions, num_flags, site_loc, site_regions, starts = types[t]
            for r, (_, _, retried) in enumerate(regions.tolist()):
                n1, n2 = (int(v) for v in site_regions[r])
                sites = site_loc[starts[r]:starts[r + 1]]
                kr = mix64(ks + _u64(STREAM_MULT * (REGION_SLOT_BASE + g + 1)))
                got = np.zeros((count, 3), dtype=np.uint64)
                used = np.zeros(count, dtype=np.uint32)
                pending, a = alive.copy(), 0
                while pending.any() and a < (max_attempts if retried else 1):
                    rows = np.nonzero(pending)[0]
                    got[rows], who, where, what = _attempt(mix64(kr[rows] + _u64(GOLDEN * (a + 1))), eff, sites, n1, n2, t_class, tables)
                    used[rows] = a + 1
                    pending[rows] = got[rows, 2] != 0
                    entered = ~pending[rows[who]]                               # the faults of an attempt that passed
                    f_sample.append(rows[who][entered])
                    f_where.append(block_first + where[entered])
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


# -- exact laws ----------------------------------------------------------------------------------------------------------------

def retried_pass_probabilities(program, p1, p2):
    """q of every preparation of the sequence in order (retry_gate_ref.region_pass_probability per retried region)."""
    cache, out = {}, []
    for t in program.block_type:
        for r, (_, _, retried) in enumerate(program.types[t].regions.tolist()):
            if retried:
                if (t, r) not in cache:
                    cache[t, r] = retry_gate_ref.region_pass_probability(program.types[t], r, p1, p2)
                out.append(cache[t, r])
    return out


def attempts_mean_var(program, p1, p2):
    """Mean and variance of a sample's attempts with unbounded retries: per preparation geometric, 1 / q and (1 - q) / q^2."""
    qs = np.array(retried_pass_probabilities(program, p1, p2))
    return float((1.0 / qs).sum()), float(((1.0 - qs) / (qs * qs)).sum())


def _block_conditional(block, p1, p2, local_mask, tail_mask):
    """P(local, tail | every flag of the block zero): the XOR-convolution of its regions' conditionals."""
    return xor_convolution([retry_gate_ref.region_conditional(block, r, p1, p2, local_mask, tail_mask)[0] for r in range(len(block.regions))])


def cnot_pair_cells(words, r_1, r_2):
    """The cell of a sample in cnot_pair_law's index: the key bits of its first two step words, word 0's from bit 0."""
    keys = key_mask(r_1, r_2)
    return _extract(words[:, 0], keys) | _extract(words[:, 1], keys) << (r_1 + r_2)


def cnot_pair_law(program, p1, p2):
    """The exact law of the key bits of the first two step words of `CNOT a b; ...` on two data blocks [prepare D_0, prepare D_1, CNOT,
    EC on D_0, EC on D_1, ...] given that the sample is accepted, over 2 (r_1 + r_2) bits in cnot_pair_cells' index: the product of the
    two preparations' conditional tails, pushed through the frame map, XOR-convolved with the CNOT block's joint of (tail for a, tail
    for b), projected to the key bits and XOR-convolved with the two rounds' conditional local words."""
    code = program.code
    r_1, r_2 = int(code.r_1), int(code.r_2)
    kinds = [int(k) for k in program.block_kind[:5]]
    assert kinds == [NONE, NONE, CNOT, EC, EC] and [int(f) for f in program.block_a[:5]] == [0, 1, int(program.block_a[2]), 0, 1]
    assert {int(program.block_a[2]), int(program.block_b[2])} == {0, 1}
    prepare, cnot, rounds = program.types[program.block_type[0]], program.types[program.block_type[2]], [program.types[t] for t in program.block_type[3:5]]
    frame, keys = frame_mask(r_1, r_2), key_mask(r_1, r_2)
    nt, nk = bin(frame).count("1"), r_1 + r_2
    tail = _block_conditional(prepare, p1, p2, 0, frame)                         # over a frame's nt packed bits
    assert len(tail) == 1 << nt
    # the packed frame bits: key_x (r_2), bit 31, key_z (r_1), bit 63 -- the X half below, the Z half above
    half_x = (1 << (r_2 + 1)) - 1
    half_z = ((1 << (r_1 + 1)) - 1) << (r_2 + 1)
    fa, fb = int(program.block_a[2]), int(program.block_b[2])
    cells = np.arange(1 << (2 * nt), dtype=np.int64)
    T = [cells & ((1 << nt) - 1), cells >> nt]                                   # frame 0 in the low bits, frame 1 above
    product = tail[T[0]] * tail[T[1]]
    T[fb] = T[fb] ^ (T[fa] & half_x)
    T[fa] = T[fa] ^ (T[fb] & half_z)
    moved = np.bincount(T[0] | T[1] << nt, weights=product, minlength=1 << (2 * nt))
    joint, nl, nt_2, nf = retry_gate_ref.region_joint(cnot, 0, p1, p2, frame, frame)   # (tail for a, tail for b): a's bits below
    assert (nl, nt_2, nf) == (nt, nt, 0)
    if fa == 1:                                                                  # put frame 0's bits below
        joint = joint.reshape(1 << nt, 1 << nt).T.reshape(-1)
    after = xor_convolution([moved, joint])
    # project a frame's packed bits to its key bits: drop the packed bits r_2 (bit 31) and r_2 + 1 + r_1 (bit 63)
    key_of = lambda v: (v & ((1 << r_2) - 1)) | ((v >> (r_2 + 1)) & ((1 << r_1) - 1)) << r_2
    index = key_of(cells & ((1 << nt) - 1)) | key_of(cells >> nt) << nk
    projected = np.bincount(index, weights=after, minlength=1 << (2 * nk))
    local = []
    for block in rounds:                                                         # a round's local word, its tail summed out
        both = _block_conditional(block, p1, p2, keys, frame)
        local.append(both.reshape(1 << nt, 1 << nk).sum(axis=0))
    pair = (local[0][None, :] * local[1][:, None]).reshape(-1)                   # word 0's bits below
    law = xor_convolution([projected, pair])
    return law / law.sum()
