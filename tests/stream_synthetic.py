"""
Synthetic block sequences for the streamed and retried routes (DESIGN.md section 5h "Synthetic block sequences"): the smallest sequences
that reach the paths of stream_kernel, mstream_kernel and the four retried kernels which no sequence of a real code reaches.  NumPy only,
no GPU and nothing of quantum_css_codes_amd; everything is seeded from SEED0, made once (functools.lru_cache) and frozen.

A Sequence holds plain arrays in the order the _native entry points take them (stream_args, mstream_args, retry_args, sites, waits) and
is at the same time the duck-typed gadget tests/retry_ref.py and its three siblings read: .types[*].effects / .regions / .num_flags
(.gate_regions(), .waits()), .block_type, .block_kind.

The rules of the plans in csrc/gf2_host.cpp hold by construction: local words stay within the layout of (r_1, r_2) -- a NONE block has
no local bit, an EC block key bits, a MEASURE block key_x bits and bit 31 -- tails may also set bits 31 and 63, flag bits lie below the
type's flag count, a region that is not retried sets no flag, the flag masks of a type's regions are disjoint, the sites of a region
partition it as n_1 + 2 n_2 locations with each class ascending and a CNOT site on rows l and l + 1, wait rows sit on retried regions only
and are at most 512.

Keys come from a pool of 24 values per side and (r_1, r_2); a decoder table holds every second one (at least one with bit 30 set where
r = 31), so about half of the keys single rows produce are matched.  A row's tail usually carries the key its local word shows, as a
real data error does: a matched key then leaves T ^ K = 0 for the steps after it, an unmatched one is missed by every later step.  The
share of rows with a key or a parity bit is set from the sequence's mean faults per sample: one sample in two has a key on a side, one
in three a parity bit; 95 % of the keys drawn are ones the tables hold (none on a side of one bit, which has the key 1 alone), so the
unmatched keys stay below the accepted samples.

  overlap8        stream, mstream   eight blocks in one 512-location segment (closed in it: 8 x 64; open at its end: 449 1 2 3 1 2 3 60),
                                    blocks that start and end on multiples of 512, a last segment of one location
  flags64         all six           flag counts 64, 1, 63, 64, 5, 64: first flag rows 0, 64, 65, 128, 192, 197, the last across words 3 and 4
  long_regions    the retried four  regions of 513, 7, 1024, 1100, 1 and 511, 2, 600 locations
  sixteen_sizes   the retried four  sixteen distinct last-segment sizes (per class at gate level); a part of them that is staged; the sixteen
                                    largest sizes, whose tables nearly fill the LDS
  attempts        the retried four  one region that fails 98 % of its attempts
  decoder         all six           tables for (r_1, r_2) in R_SETS and the three ways of key 0
"""
import functools
import math

import numpy as np

SEED0 = 20261020
SEG = 512
NONE, EC, MEASURE, FINAL, CNOT = 0, 1, 2, 3, 4
R_SETS = ((31, 31), (1, 31), (31, 1))
KEY0 = ("zero", "absent", "one")                                          # key 0 -> flip 0, no key 0, key 0 -> flip 1
POOL = 24
SPLIT = (0.4, 0.2, 0.4)                                                    # p_x : p_y : p_z
KEYED, PARITY, HELD = 0.5, 0.3, 0.95                                       # faults with a key (per side) and with a parity bit (per bit) per sample; keys the tables hold
SIZES16 = (1, 2, 3, 31, 32, 33, 63, 64, 65, 255, 256, 257, 509, 510, 511, 512)
SIZES_FULL = tuple(range(497, 513))
PASS_TARGET = 0.47                                                         # flagged faults per attempt of a retried region: it passes 5 times in 8


def frozen(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays


@functools.lru_cache(maxsize=None)
def key_pool(r, side):
    """POOL distinct non-zero keys below 2^r (fewer when r is small), every second one with its top bit set."""
    r = int(r)
    if r <= 4:
        return frozen(np.arange(1, 1 << r, dtype=np.uint64))[0]
    rng = np.random.default_rng([SEED0, 10, r, side])
    keys = set()
    while len(keys) < POOL:
        key = int(rng.integers(1, 1 << (r - 1)))
        keys.add(key | (1 << (r - 1)) if len(keys) % 2 else key)
    return frozen(np.array(sorted(keys, key=lambda k: (k * 0x9E3779B97F4A7C15) % (1 << 64)), dtype=np.uint64))[0]


@functools.lru_cache(maxsize=None)
def decoder(r1, r2, key0="zero"):
    """(r1, keys1, flips1, r2, keys2, flips2): per side every second key of the pool (key 1 alone is left out where r = 1), and key 0 as
    `key0` says."""
    out = []
    for side, r in ((1, r1), (0, r2)):
        rng = np.random.default_rng([SEED0, 11, r, side])
        pool = key_pool(r, side)
        keys = pool[::2] if len(pool) > 1 else pool[:0]
        flips = rng.integers(0, 2, len(keys)).astype(np.uint8)
        if key0 != "absent":
            keys, flips = np.concatenate([[np.uint64(0)], keys]), np.concatenate([[np.uint8(key0 == "one")], flips])
        if len(keys) == 0:                                                 # (r = 1 without key 0: a table must hold something)
            keys, flips = pool[:1].copy(), np.ones(1, dtype=np.uint8)
        out.append(frozen(keys.astype(np.uint64), flips.astype(np.uint8)))
    return (r1, out[0][0], out[0][1], r2, out[1][0], out[1][1])


def rates(total):
    return tuple(f * total for f in SPLIT)


class BlockType(object):
    """A block type: effects (L_t, 2, 3); regions (n, 3) of (first, count, retried); its sites and wait rows, region by region."""

    def __init__(self, kind, effects, num_flags, regions, site_loc, site_regions, wait_eff, wait_count):
        self.kind, self.num_flags = int(kind), int(num_flags)
        self.effects, self.regions, self.site_loc, self.site_regions, self.wait_eff, self.wait_count = frozen(
            effects, np.asarray(regions, dtype=np.int64).reshape(-1, 3), np.asarray(site_loc, dtype=np.int32),
            np.asarray(site_regions, dtype=np.int64).reshape(-1, 2), np.asarray(wait_eff, dtype=np.uint64).reshape(-1, 2, 2),
            np.asarray(wait_count, dtype=np.int64))

    def gate_regions(self):
        return self.site_loc, self.site_regions

    def waits(self, wait_steps=1):
        return self.wait_eff, self.wait_count


def _rows(rng, count, kind, r, key_density, parity_density):
    """(count, 2, 2) uint64: the (local, tail) words of an X and of a Z fault on `count` rows of a block of `kind`; for a CNOT block the
    tails left on frame a and on frame b."""
    r1, r2 = r
    shape = (count, 2)
    bit = lambda p, at: (rng.random(shape) < p).astype(np.uint64) << np.uint64(at)
    pick = lambda pool: pool[rng.integers(0, len(pool), shape)]
    def side_keys(width, side):                                               # 95 % of the keys are ones the decoder tables hold
        pool = key_pool(width, side)
        held, other = (pool[::2], pool[1::2]) if len(pool) > 1 else (pool[:0], pool)
        want_held = rng.random(shape) < HELD
        drawn = np.where(want_held, pick(held) if len(held) else np.uint64(0), pick(other))
        return np.where(rng.random(shape) < key_density, drawn, np.uint64(0))
    kx, kz = side_keys(r2, 0), side_keys(r1, 1)
    keys = kx | kz << np.uint64(32)
    out = np.zeros((count, 2, 2), dtype=np.uint64)
    if kind == CNOT:
        other = np.where(rng.random(shape) < 0.5, keys, np.uint64(0))
        out[:, :, 0] = keys | bit(parity_density, 31) | bit(parity_density, 63)
        out[:, :, 1] = other | bit(parity_density, 31) | bit(parity_density, 63)
        return out
    stays = rng.random(shape) < (1.0 if kind == NONE else 0.75)            # the error stays on the data: the tail carries the key
    out[:, :, 0] = {NONE: np.zeros(shape, dtype=np.uint64), EC: keys, MEASURE: kx | bit(parity_density, 31)}[kind]
    out[:, :, 1] = np.where(stays, keys, np.uint64(0)) | bit(parity_density, 31) | bit(parity_density, 63)
    return out


def _flags(rng, count, bits, density):
    """(count, 2) uint64: with probability `density` a row has one of `bits` (an eighth of them the highest), a quarter of those a second."""
    out = np.zeros((count, 2), dtype=np.uint64)
    if len(bits) == 0 or density <= 0.0:
        return out
    bits = np.asarray(bits, dtype=np.uint64)
    one = lambda: np.uint64(1) << np.where(rng.random(out.shape) < 0.125, bits[-1], bits[rng.integers(0, len(bits), out.shape)])
    hit = rng.random(out.shape) < density
    return np.where(hit, one() | np.where(rng.random(out.shape) < 0.25, one(), np.uint64(0)), np.uint64(0))


def _sites(rng, first, n1, n2):
    """The type-local first locations of a region's n1 one-operand sites, then of its n2 CNOT sites, in a random arrangement."""
    width = np.concatenate([np.ones(n1, dtype=np.int64), np.full(n2, 2, dtype=np.int64)])[rng.permutation(n1 + n2)]
    start = first + np.cumsum(width) - width
    return np.concatenate([start[width == 1], start[width == 2]]).astype(np.int32)


def make_type(rng, kind, r, num_flags, regions, p_total, key_density, parity_density, flag_density=None, q_total=0.0):
    """regions: [(locations, retried, (n1, n2) or None, wait rows)].  A retried region's flag density makes PASS_TARGET flagged faults per
    attempt at p_total (all its rows where that is not enough), or is flag_density where given; the type's flag rows are dealt to its
    flagged regions in order, the last region taking the highest."""
    size = sum(reg[0] for reg in regions)
    eff = np.zeros((size, 2, 3), dtype=np.uint64)
    eff[:, :, :2] = _rows(rng, size, kind, r, key_density, parity_density)
    flagged = [k for k, reg in enumerate(regions) if reg[1]] if num_flags else []
    cuts = [num_flags * k // max(1, len(flagged)) for k in range(len(flagged) + 1)]
    table, site_loc, site_regions, wait_eff, wait_count = [], [], [], [], []
    first = 0
    for k, (count, retried, split, wait) in enumerate(regions):
        if k in flagged:
            at = flagged.index(k)
            density = min(1.0, PASS_TARGET / (p_total * count)) if flag_density is None else flag_density
            eff[first:first + count, :, 2] = _flags(rng, count, list(range(cuts[at], cuts[at + 1])), density)
        n1, n2 = split if split is not None else (count - 2 * (count // 3), count // 3)
        assert n1 + 2 * n2 == count and (wait == 0 or retried) and 0 <= wait <= SEG
        table.append((first, count, int(bool(retried))))
        site_loc.append(_sites(rng, first, n1, n2))
        site_regions.append((n1, n2))
        wait_count.append(wait)
        wait_density = min(0.5, KEYED / 4.0 / max(q_total * wait, 1e-9)) if wait else 0.0
        wait_eff.append(_rows(rng, wait, EC if kind == CNOT else kind, r, wait_density, wait_density))
        first += count
    return BlockType(kind, eff, num_flags, table, np.concatenate(site_loc), site_regions, np.concatenate(wait_eff), wait_count)


class Sequence(object):
    """types: [BlockType]; blocks: [(type or -1, kind, frame a, frame b)]; r = (r_1, r_2)."""

    def __init__(self, name, types, blocks, r, p_total, nframes=1, q_total=0.0):
        self.name, self.types, self.r, self.nframes = name, list(types), tuple(r), int(nframes)
        self.p, self.p_gate, self.q = rates(p_total), (p_total, p_total), rates(q_total)
        cols = np.array(blocks, dtype=np.int32).reshape(-1, 4)
        self.block_type, self.block_kind, self.block_a, self.block_b = frozen(*(np.ascontiguousarray(cols[:, k]) for k in range(4)))
        self.type_eff, self.type_regions, self.site_loc, self.site_regions, self.wait_eff, self.wait_count = frozen(
            np.concatenate([t.effects for t in types]), np.concatenate([t.regions for t in types]), np.concatenate([t.site_loc for t in types]),
            np.concatenate([t.site_regions for t in types]), np.concatenate([t.wait_eff for t in types]), np.concatenate([t.wait_count for t in types]))
        self.type_locations = [len(t.effects) for t in types]
        self.type_flags = [t.num_flags for t in types]
        self.type_nregions = [len(t.regions) for t in types]
        real = [int(t) for t in self.block_type if t >= 0]
        sizes = [self.type_locations[t] for t in self.block_type if t >= 0]
        self.start = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)     # of every block with locations, then L
        self.locations = int(self.start[-1])
        self.nsteps = int(np.count_nonzero((self.block_kind != NONE) & (self.block_kind != CNOT)))
        self.flag_rows = sum(self.type_flags[t] for t in real)
        self.flag_words = max(1, (self.flag_rows + 63) // 64)
        self.ldw = self.nsteps + self.flag_words
        self.preparations = sum(int(types[t].regions[:, 2].sum()) for t in real)

    def stream_args(self):
        return self.type_eff, self.type_locations, self.type_flags, self.block_type, self.block_kind

    def mstream_args(self):
        return self.stream_args() + (self.block_a, self.block_b, self.nframes)

    def retry_args(self):
        return self.stream_args() + (self.type_regions, self.type_nregions)

    def sites(self):
        return self.site_loc, self.site_regions

    def waits(self):
        return self.wait_eff, self.wait_count

    def flag_row_of(self, block):
        return sum(self.type_flags[t] for t in self.block_type[:block] if t >= 0)


class _Builder(object):
    """Types are made as the blocks ask for them: one type per (locations, kind, flag rows, tag)."""

    def __init__(self, name, r, locations, mean_faults=None, p_total=None, q_total=0.0):
        self.rng = np.random.default_rng([SEED0, 1 + R_SETS.index(tuple(r))] + [ord(c) for c in name])
        self.name, self.r, self.q_total = name, tuple(r), q_total
        self.p_total = p_total if p_total is not None else mean_faults / locations
        self.density = min(0.5, KEYED / (self.p_total * locations))
        self.parity = min(0.5, PARITY / (self.p_total * locations))
        self.types, self.index, self.blocks = [], {}, []

    def add(self, size, kind, a=0, b=-1, num_flags=8, flag_density=None, regions=None, tag=None):
        key = (size, kind, num_flags, tag)
        if key not in self.index:
            regions = regions if regions is not None else [(size, 1, None, 0)]
            self.index[key] = len(self.types)
            self.types.append(make_type(self.rng, kind, self.r, num_flags, regions, self.p_total, self.density, self.parity, flag_density, self.q_total))
        self.blocks.append((self.index[key], kind, a, b))
        return self

    def final(self):
        self.blocks.append((-1, FINAL, 0, -1))
        return self

    def done(self, nframes=1):
        return Sequence(self.name, self.types, self.blocks, self.r, self.p_total, nframes, self.q_total)


# ---- overlap8 ----------------------------------------------------------------------------------------------------------------------------

STREAM_FLAG_DENSITY = 0.12                                                  # of the post-selected routes: a fault in eight fires a verification
OVERLAP_TRIALS = {1: 5, 2: 1, 3: 3, 4: 3}                                   # trials per measurement by frame count


def _eight_closed(b, kinds, frames):
    for kind, a in zip(kinds, frames):                                     # 8 x 64: all eight end in the segment, the next block starts at 512 k
        b.add(64, kind, a)


@functools.lru_cache(maxsize=None)
def overlap8_stream(variant, r):
    """variant "last1": 3585 locations, a last segment of one location (block 64 of the FINAL step's segment crosses into it);
    "final8": 1485 locations, the last segment overlaps seven blocks and the FINAL step."""
    b = _Builder("overlap8 " + variant, r, 3585 if variant == "last1" else 1485, mean_faults=1.5)
    f = dict(flag_density=STREAM_FLAG_DENSITY)
    for kind in (NONE, EC, MEASURE, EC, EC, MEASURE, EC, EC):
        b.add(64, kind, **f)
    b.add(512, EC, **f)                                                    # [512, 1024)
    for size, kind in ((449, EC), (1, EC), (2, MEASURE), (3, EC), (1, NONE), (2, MEASURE), (3, EC)):
        b.add(size, kind, **f)                                             # [1024, 1485): seven blocks
    if variant == "last1":
        b.add(60, EC, **f)                                                 # the eighth, open at the segment's end: [1485, 1545)
        for size, kind in ((449, EC), (449, MEASURE), (449, EC), (60, EC), (60, MEASURE), (60, EC)):
            b.add(size, kind, **f)                                         # ... back on a multiple of 512: 3072
        b.add(449, EC, **f).add(64, EC, **f)                               # [3072, 3521), [3521, 3585): one location in segment 7
    seq = b.final().done()
    assert seq.locations == (3585 if variant == "last1" else 1485)
    return seq


@functools.lru_cache(maxsize=None)
def overlap8_mstream(frames, r):
    """The same with `frames` data frames and no FINAL step: four CNOT blocks of 1 and 2 locations among the eight; every ordered pair of
    frames has a CNOT block, the pairs the eight do not take in groups of five blocks (449 60 1 1 1) that fill a segment; one
    measurement per frame with OVERLAP_TRIALS[frames] trials; a last segment of one location."""
    trials = OVERLAP_TRIALS[frames]
    pairs = [(a, c) for a in range(frames) for c in range(frames) if a != c]
    groups = max(0, -(-(len(pairs) - 4) // 3))                             # aligned groups 449 60 1 1 1 for the pairs the eight do not take
    measures = -(-frames * (trials + 1) // 8)
    b = _Builder("overlap8 mstream %d" % frames, r, 512 * (7 + groups + measures) + 1, mean_faults=1.5)
    f = dict(flag_density=STREAM_FLAG_DENSITY)
    for k in range(8):
        b.add(64, NONE if k < frames else EC, k % frames, **f)
    b.add(512, EC, 0, **f)
    pair = iter(pairs + pairs[:4])
    b.add(449, EC, frames - 1, **f)
    for size in (1, 2, 3, 1, 2, 3):
        if size < 3 and frames > 1:
            b.add(size, CNOT, *next(pair), num_flags=0)
        else:
            b.add(size, EC, size % frames, **f)
    b.add(60, EC, 0, **f)
    for k, size in enumerate((449, 449, 449, 60, 60, 60)):
        b.add(size, EC, k % frames, **f)
    for g in range(groups):
        b.add(449, EC, g % frames, **f).add(60, EC, (g + 1) % frames, **f)
        for _ in range(3):
            b.add(1, CNOT, *next(pair), num_flags=0)
    at = 0
    for frame in range(frames):                                            # the measurements: trials x MEASURE and one EC step, 64 locations each
        for k in range(trials):
            b.add(64, MEASURE, frame, **f)
            at += 1
            if k == 0:
                b.add(64, EC, (frame + 1) % frames, **f)
                at += 1
    for k in range(at, 8 * measures):
        b.add(64, EC, k % frames, **f)
    b.add(449, EC, 0, **f).add(64, EC, frames - 1, **f)
    seq = b.done(frames)
    assert seq.locations == 512 * (7 + groups + measures) + 1
    return seq


# ---- flags64 -----------------------------------------------------------------------------------------------------------------------------

FLAGS64 = (64, 1, 63, 64, 5, 64)
FLAGS64_SIZES = (100, 40, 90, 130, 30, 150)
FLAGS64_KINDS = (NONE, EC, MEASURE, EC, EC, EC)


@functools.lru_cache(maxsize=None)
def flags64(route, r):
    """route "stream" (FINAL step last), "mstream" (one frame, no FINAL step) or "retry" (FINAL step last; a retried region with the
    flags and ten locations that are not retried per type; wait rows on two regions)."""
    retried = route == "retry"
    b = _Builder("flags64 " + route, r, sum(FLAGS64_SIZES), p_total=0.008 if retried else None, mean_faults=1.5, q_total=0.004)
    for k, (size, kind, nflags) in enumerate(zip(FLAGS64_SIZES, FLAGS64_KINDS, FLAGS64)):
        regions = [(size - 10, 1, None, (5, 0, 9, 0, 0, 5)[k]), (10, 0, None, 0)] if retried else None
        b.add(size, kind, num_flags=nflags, regions=regions, tag=k, flag_density=None if retried else STREAM_FLAG_DENSITY * (4 if nflags == 1 else 1))
    if route != "mstream":
        b.final()
    seq = b.done()
    assert [seq.flag_row_of(k) for k in range(6)] == [0, 64, 65, 128, 192, 197] and seq.flag_words == 5
    return seq


# ---- long_regions, sixteen_sizes, attempts -----------------------------------------------------------------------------------------------

P_RETRY = 0.01
Q_WAIT = 0.001


@functools.lru_cache(maxsize=None)
def long_regions(r):
    """Blocks A, B, A, FINAL of kinds EC, MEASURE, EC, FINAL; 64 and 63 flag rows."""
    b = _Builder("long_regions", r, 2 * 2645 + 1113, p_total=P_RETRY, q_total=Q_WAIT)
    type_a = [(513, 1, (1, 256), 512), (7, 0, (3, 2), 0), (1024, 1, (600, 212), 300), (1100, 1, (40, 530), 0), (1, 0, (1, 0), 0)]
    type_b = [(511, 1, (511, 0), 0), (2, 1, (0, 1), 1), (600, 1, (88, 256), 0)]
    b.add(2645, EC, num_flags=64, regions=type_a).add(1113, MEASURE, num_flags=63, regions=type_b).add(2645, EC, num_flags=64, regions=type_a)
    return b.final().done()


@functools.lru_cache(maxsize=None)
def sixteen_sizes(variant, r):
    """One EC block of one type, then the FINAL step.
    "location"        16 retried regions whose last segments have the SIZES16 (the 512: a region of 1024); 16 distinct wait sizes
    "location-staged" 14 of them (all but 510 and 511), which leave room for the block table in LDS: with one more region of 510 the
                      tables of retry_wait no longer fit; wait sizes 3, 31, 64
    "gate"            16 regions with the SIZES16 as n_1 and, rotated, as n_2 (the 512: 1024 sites); wait sizes 510, 511, 512
    "gate-staged"     8 regions, a class of 513 sites in two of them (the 512 and a last segment of 1), small enough to be staged
    "location-full"   the SIZES_FULL, 497 .. 512, as last-segment sizes and as wait sizes: sixteen distinct sizes cannot make longer tables
    "gate-full"       the SIZES_FULL as n_1 and, rotated, as n_2; wait sizes 510, 511, 512: 35 packed tables of 141 696 bytes, which with
                      the taken maps and the bins come within 5 KiB of the 160 KiB of LDS and leave no room for a wait row"""
    if variant.startswith("location"):
        sizes = {"location": SIZES16, "location-staged": SIZES16[:13] + (512,), "location-full": SIZES_FULL}[variant]
        waits = [3, 0, 31, 0, 64] + [0] * 9 if variant == "location-staged" else list(sizes)
        regions = [(1024 if s == 512 else s, 1, None, w) for s, w in zip(sizes, waits)]
    else:
        ones = {"gate": SIZES16, "gate-staged": (513, 1, 2, 33, 64, 255, 3, 31), "gate-full": SIZES_FULL}[variant]
        twos = (3, 513, 31, 1, 2, 33, 64, 0) if variant == "gate-staged" else ones[5:] + ones[:5]
        if variant == "gate-full":                                             # (the regions' location counts n_1 + 2 n_2 have their own sixteen sizes at
            twos = twos[1::-1] + twos[2:]                                      # most, the 512 among them: the first two regions share one)
        full = lambda s: 1024 if s == 512 else s
        waits = {3: 64, 4: 255} if variant == "gate-staged" else {0: 510, 1: 511, 2: 512}
        regions = [(full(a) + 2 * full(c), 1, (full(a), full(c)), waits.get(k, 0)) for k, (a, c) in enumerate(zip(ones, twos))]
    locations = sum(reg[0] for reg in regions)
    b = _Builder("sixteen_sizes " + variant, r, locations, p_total=P_RETRY, q_total=Q_WAIT)
    return b.add(locations, EC, num_flags=64, regions=regions).final().done()


@functools.lru_cache(maxsize=None)
def attempts(r):
    """[one retried region of 600 locations (n_1 = 200, n_2 = 200), FINAL]: an attempt has 3.9 flagged faults, so it passes once in 50."""
    b = _Builder("attempts", r, 600, p_total=P_RETRY)
    seq = b.add(600, NONE, num_flags=64, regions=[(600, 1, (200, 200), 0)], flag_density=-math.log(0.02) / (P_RETRY * 600)).final().done()
    seq.p_gate = (1.3 * P_RETRY, 1.3 * P_RETRY)                                # 400 sites for 600 locations: the gates fail more often to flag as often
    return seq
