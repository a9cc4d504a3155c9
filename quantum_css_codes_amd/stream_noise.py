"""
Streamed gadgets: error-correction cycles and rewritten programs of any length, block by block [build-defined; DESIGN.md "Streamed
gadgets"].

ec_noise.py and ft_noise.py keep one dense effect table for a whole gadget and one sample's outcome words in registers, which stops
the cycle at 6 rounds and a program at 7 logical gates.  This module is a third route beside them, for the questions those sizes
cannot ask: the logical error per round over tens to thousands of rounds, the cost of a long program.  Nothing of the two resident
routes changes.

Both ancilla blocks are RESET at the start of every preparation, so only the data block survives from one BLOCK of a gadget -- the
first preparation, a round of error_correct (with the physical Paulis of a logical gate or the idle locations before it), a trial of
the logical measurement -- to the next.  A fault inside a block acts through three words, BlockType.effects[l, c]:
    local   what it flips of its own block's measured word (an EC step: key_x in bits 0 .. r_2 - 1, key_z in bits 32 ..; a MEASURE
            step: key_x and, in bit 31, the measured z_operator parity)
    tail    what it leaves on the data frame at the block's end (key_x, z_operator . e_x in bit 31, key_z from bit 32,
            x_operator . e_z in bit 63: the final-frame word of ec_noise's layout)
    flags   what it flips of its own block's verifications, in measurement order (at most 64 rows)
and they come from gf2_circuit_effects_timed on the block's own gate list at ldr = 3.  With T = 0 at the start, block after block:
its step word is mask_kind(T) ^ (XOR of its faults' local words), then T ^= (XOR of their tail words).  A cycle ends with a FINAL step,
a pseudo-block of no locations whose word is T itself.  At most seven block types occur, whatever the length.

Stream layout of a sample's words: [step 0 .. nsteps - 1] [flag words: the flag rows of all blocks in order, 64 per word, at least
one word]; to_cycle_layout / to_program_layout permute them into ec_noise's and ft_noise's layouts.  The sampler, the fault location
numbering (the blocks' locations one after the other: that of error_correct_gates / program_gates) and the tally rules are the
resident routes', so sample i is the same sample on all of them.

Acceptance falls like exp(-c p rounds): every preparation is post-selected, roughly 200 locations per Steane round reject the
sample when they fail, so a run of `rounds` rounds keeps about exp(-200 p_kind rounds) of its samples.  Long runs are for p <~ 1e-4.

Repeat-until-success (the retry_* methods; DESIGN.md section 5d "Repeat-until-success") lifts that limit: a block type is cut into
BlockType.regions, every `prep ...` part of the builder a retried region, and a retried region is redrawn on its own until its
verifications pass.  Locations fail independently and a flag row depends on one region only, so the accepted samples have exactly
the distribution post-selection gives, essentially every sample is accepted, and the cost is linear in the number of blocks.  The
samples are other samples than the post-selected routes draw: the rates agree, the counts of a seed do not.

The retry_gate_* methods run the same walk under gate-level faults (DESIGN.md section 5d "Repeat-until-success under gate-level
faults"): BlockType.gate_regions gives every region its sites, a one-operand gate fails with probability p1 and one of 3 kinds, a
CNOT as one event with probability p2 and one of 15.  Regions are cut at gate boundaries, so the argument above holds for sites.

The retry_wait_* methods make the data block pay for the retries (DESIGN.md section 5d "Repeat-until-success with waiting faults"):
BlockType.waits gives every retried region its wait rows, one per qubit of the data block that no gate of the region touches, and
every attempt made of the region, the failed ones included, draws them with memory error rates (q_x, q_y, q_z) of their own.
The retry_gate_wait_* methods do the same under gate-level faults (DESIGN.md section 5d "Repeat-until-success with waiting faults
under gate-level faults"): retry_gate_*'s walk and draw plus retry_wait_*'s wait draw.

MultiProgram is the same walk for rewritten programs on up to four logical qubits with the transversal CNOT (DESIGN.md section 5d
"Multi-block programs"): one data frame T per logical qubit, the existing block types serving frame a, and one new block type and
kind, CNOT, whose closing applies T_b ^= T_a & 0x00000000FFFFFFFF, T_a ^= T_b & 0xFFFFFFFF00000000 to the two carried words and then
XORs its faults' two tails.  Its retry_* methods are the repeat-until-success sampler of such programs (DESIGN.md section 5d
"Repeat-until-success of multi-block programs"): the regions of the block types as above, a CNOT block one region that is not
retried.  Its retry_gate_* methods run that walk under gate-level faults (DESIGN.md section 5d "Repeat-until-success of multi-block
programs under gate-level faults"): a physical CNOT of a CNOT block fails as one event that puts a correlated Pauli on both data
frames.  The waiting variants are those of one qubit.
"""
import numpy as np

from . import _native
from . import circuit_noise
from . import ec_noise
from . import ft_noise
from .ec_noise import GATE_CNOT, GATE_IDLE, ROW_FINAL, ROW_ROUND

NONE, EC, MEASURE, FINAL = _native.STREAM_NONE, _native.STREAM_EC, _native.STREAM_MEASURE, _native.STREAM_FINAL
STREAM_FIELDS = ('accepted', 'logical_x', 'logical_z', 'logical_any', 'uncorrectable_x', 'uncorrectable_z', 'unmatched_x', 'unmatched_z',
                 'wrong', 'trial_wrong', 'first_trial_wrong', 'split_vote')
RETRY_FIELDS = STREAM_FIELDS + ('exhausted', 'attempts')
MAX_FLAG_ROWS = 64
_BIT31, _BIT63 = np.uint64(1 << 31), np.uint64(1 << 63)
FRAME_MASK = {NONE: np.uint64(0), EC: ~(_BIT31 | _BIT63), MEASURE: np.uint64(0xFFFFFFFF), FINAL: ~np.uint64(0)}   # what a step reads of T
# the fields of the two resident routes, as indices into STREAM_FIELDS
_CYCLE_FIELDS = (0, 1, 2, 3, 4, 5, 6, 7)
_PROGRAM_FIELDS = (0, 8, 9, 10, 11, 6, 7)


class BlockType(object):
    """One type of block: `name`, `kind` (NONE, EC or MEASURE), its gate list `gates` (g, 3) int32 on 3n qubits, `locations` (L_b, 2)
    rows (gate, qubit), `num_flags` flag rows and `effects` (L_b, 2, 3) uint64: (local, tail, flags) of an X and of a Z fault;
    `regions` (R, 3) int64 rows (first location, count, retried) that partition the locations in order -- every `prep ...` part of
    the builder a retried region, the locations between and around them maximal regions that are not.  waits() gives the retried
    regions' wait rows."""

    def __init__(self, code, name, kind, emit):
        build = ec_noise.GadgetBuilder(code)
        emit(build)
        end, data, r_1, r_2 = len(build.gates), build.data, build.r_1, build.r_2
        for i in range(r_2):                                        # word 1: the data frame at the block's end (error_correct_gates' final frame)
            build.rows.append((64 + r_2 - 1 - i, ROW_FINAL, 0, end, data, 0, build.h_2[i]))
        build.rows.append((64 + 31, ROW_FINAL, 0, end, data, 0, build.z_op[0]))
        for i in range(r_1):
            build.rows.append((64 + 32 + r_1 - 1 - i, ROW_FINAL, 0, end, data, 1, build.h_1[i]))
        build.rows.append((64 + 63, ROW_FINAL, 0, end, data, 1, build.x_op[0]))
        self.name, self.kind, self.num_flags = name, kind, build.num_flags
        if self.num_flags > MAX_FLAG_ROWS:
            raise ValueError("a block (%s) has %d flag rows (an EC block 2 (r_1 + r_2) + 2), more than the %d one flag word holds"
                             % (name, self.num_flags, MAX_FLAG_ROWS))
        gates, rows_x, rows_z, row_time, _, _, _ = build.arrays(3, 2)
        self.gates = gates
        self._rows = (3 * build.n, [int(q) for q in build.data], _native.pack_rows(rows_x), _native.pack_rows(rows_z), np.asarray(row_time, dtype=np.int64))
        self.effects, self.locations = _native.circuit_effects_timed(gates, *self._rows[:1], *self._rows[2:], ldr=3)
        gate_of = self.locations[:, 0]                              # non-descending: locations are in gate order
        regions, at = [], 0
        self._region_gates, self._waits = [], {}                    # per region: its gates [first, stop) if retried, else None
        for first, stop, path in sorted(span for span in build.spans if span[2][-1].startswith("prep ")):
            lo, hi = (int(v) for v in np.searchsorted(gate_of, [first, stop]))
            if lo > at:
                regions.append((at, lo - at, 0))
                self._region_gates.append(None)
            if hi > lo:
                regions.append((lo, hi - lo, 1))
                self._region_gates.append((int(first), int(stop)))
            at = max(at, hi)
        if at < len(gate_of):
            regions.append((at, len(gate_of) - at, 0))
            self._region_gates.append(None)
        self.regions = np.array(regions, dtype=np.int64).reshape(-1, 3)

    @property
    def num_locations(self):
        return len(self.locations)

    def region_masks(self):
        """Per region, the OR of the flag words of its locations: the flag rows it sets."""
        return np.array([np.bitwise_or.reduce(self.effects[first:first + count, :, 2].reshape(-1)) for first, count, _ in self.regions],
                        dtype=np.uint64)

    def waits(self, wait_steps=1):
        """The wait rows of the retried regions (DESIGN.md section 5d "Repeat-until-success with waiting faults"): (wait_eff, wait_count).
        A retried region's waiting qubits are the data-block qubits that none of its gates touches; a wait row holds the (local, tail)
        words of an X and of a Z fault of an IDLE on such a qubit placed immediately before the region's first gate.  wait_eff is
        (rows, 2, 2) uint64, region by region, a region's rows in the data block's qubit order and repeated wait_steps times (more
        waiting periods per attempt); wait_count (R,) int64 has a region's rows, 0 for one that is not retried.  Computed on the
        block's own gate list with those IDLEs inserted, where two things are checked: an inserted location sets no flag row, and
        the rows of all other locations are those of `effects`.  More than 512 wait rows in a region is a ValueError."""
        wait_steps = int(wait_steps)
        if wait_steps < 1:
            raise ValueError("wait_steps must be at least 1")
        if wait_steps in self._waits:
            return self._waits[wait_steps]
        qubits, data, rows_x, rows_z, row_time = self._rows
        inserts = []                                                # (gate in front of which they go, the qubits that wait)
        for span in self._region_gates:
            if span is not None:
                part = self.gates[span[0]:span[1]]
                touched = set(part[:, 1].tolist()) | set(part[part[:, 0] == GATE_CNOT, 2].tolist())
                inserts.append((span[0], [q for q in data if q not in touched]))
        points = np.array([at for at, _ in inserts], dtype=np.int64)
        sizes = np.array([len(waiting) for _, waiting in inserts], dtype=np.int64)
        moved = lambda gate: gate + (sizes[None, :] * (points[None, :] <= np.asarray(gate)[:, None])).sum(axis=1)   # an old gate's new number
        pieces, at = [], 0
        for point, waiting in inserts:
            pieces += [self.gates[at:point], np.array([(GATE_IDLE, q, 0) for q in waiting], dtype=np.int32).reshape(-1, 3)]
            at = point
        gates = np.concatenate(pieces + [self.gates[at:]]) if inserts else self.gates
        effects, locations = _native.circuit_effects_timed(gates, qubits, rows_x, rows_z, moved(row_time), ldr=3)
        firsts = moved(points) - sizes                              # the new numbers of every region's first IDLE
        inserted = np.zeros(len(locations), dtype=bool)
        parts = []
        for first, size in zip(firsts, sizes):
            rows = (locations[:, 0] >= first) & (locations[:, 0] < first + size)
            assert int(rows.sum()) == size
            inserted |= rows
            parts.append(effects[rows])
        if any(int(part[:, :, 2].any()) for part in parts):
            raise ValueError("a waiting fault of block type %s sets a flag row: a preparation's flags depend on its own blocks only" % self.name)
        kept = locations[~inserted]
        if not (np.array_equal(effects[~inserted], self.effects) and np.array_equal(kept[:, 1], self.locations[:, 1]) and
                np.array_equal(kept[:, 0], moved(self.locations[:, 0]))):
            raise ValueError("inserting the waiting locations changed the rows of block type %s" % self.name)
        count = np.zeros(len(self.regions), dtype=np.int64)
        count[[r for r, span in enumerate(self._region_gates) if span is not None]] = sizes * wait_steps
        if count.max(initial=0) > _native.RETRY_WAIT_MAX_ROWS:
            raise ValueError("a region of block type %s has %d wait rows, more than the %d of one sampler segment"
                             % (self.name, int(count.max()), _native.RETRY_WAIT_MAX_ROWS))
        rows = [np.tile(part[:, :, :2], (wait_steps, 1, 1)) for part in parts]
        wait_eff = np.ascontiguousarray(np.concatenate(rows + [np.zeros((0, 2, 2), dtype=np.uint64)]), dtype=np.uint64)
        self._waits[wait_steps] = (wait_eff, count)
        return self._waits[wait_steps]

    def gate_regions(self):
        """The sites of the gate-level fault model (circuit_noise.gate_sites) region by region: (site_loc, site_regions).  site_loc
        (int32) is the type-local first location of every site in region-major order -- for each region of `regions` in order its
        one-operand gates in gate order, then its CNOTs in gate order, a CNOT's second location being site_loc + 1 -- and
        site_regions (R, 2) int64 rows (n1, n2) with n1 + 2 n2 the region's locations.  The regions are cut at gate boundaries; a
        gate whose locations fall into two regions is a ValueError."""
        loc, n1, _, _ = circuit_noise.gate_sites(self.gates, self.locations)
        loc = loc.astype(np.int64)
        width = np.where(np.arange(len(loc)) < n1, 1, 2)
        stops = np.cumsum(self.regions[:, 1])
        region = np.searchsorted(stops, loc, side="right")
        if np.any(np.searchsorted(stops, loc + width - 1, side="right") != region):
            raise ValueError("a gate of block type %s has its locations in two regions" % self.name)
        order = np.lexsort((np.arange(len(loc)), width, region))       # by region, one-operand sites first, gate order inside a class
        counts = np.zeros((len(self.regions), 2), dtype=np.int64)
        np.add.at(counts, (region, width - 1), 1)
        return loc[order].astype(np.int32), counts


def _emit_prepare(build):
    build.prep(build.data, 'zero', 0, verifier=build.anc_1)        # ftqc.py:78


def _emit_ec(qubits):
    """A round of error_correct after one IDLE location on each of the data block's `qubits` (a logical gate's physical Paulis, or
    idle_data's locations)."""
    def emit(build):
        build.gates.extend((GATE_IDLE, build.data[q], 0) for q in qubits)
        build.error_correct(1, 0)
    return emit


def _emit_measure(build):
    r_2 = build.r_2
    build.prep(build.anc_1, 'zero', 1)                              # css_code.py:629
    build.gates.extend((GATE_CNOT, d, a) for d, a in zip(build.data, build.anc_1))
    build.measure(build.anc_1, np.concatenate([build.h_2, build.z_op[:1]]), ROW_ROUND, 1, [r_2 - 1 - i for i in range(r_2)] + [31])


class StreamedGadget(object):
    """A sequence of blocks prepared for the Monte-Carlo: `types` (BlockType), `block_type` (index into types, -1 for the FINAL step)
    and `block_kind` per block; `block_start`, `block_step`, `block_flag`: a block's first location, its step (-1: none) and its
    first flag row; `nsteps`, `flag_rows`, `flag_words` and `ldw` = nsteps + flag_words, the words of a sample in the stream layout.
    Made by StreamedGadget.cycle or StreamedGadget.program."""

    def __init__(self, code, what, types, block_type, block_kind):
        self.code, self.what, self.types = code, what, list(types)
        self.block_type = np.array(block_type, dtype=np.int32)
        self.block_kind = np.array(block_kind, dtype=np.int32)
        sizes = np.array([0 if t < 0 else self.types[t].num_locations for t in block_type], dtype=np.int64)
        flags = np.array([0 if t < 0 else self.types[t].num_flags for t in block_type], dtype=np.int64)
        self.block_start = np.concatenate([[0], np.cumsum(sizes)])
        self.block_flag = np.concatenate([[0], np.cumsum(flags)])[:-1]
        has_step = self.block_kind != NONE
        self.block_step = np.where(has_step, np.cumsum(has_step) - 1, -1)
        self.num_locations = int(self.block_start[-1])
        self.nsteps = int(has_step.sum())
        self.flag_rows = int(flags.sum())
        self.flag_words = max(1, (self.flag_rows + 63) // 64)
        self.ldw = self.nsteps + self.flag_words
        self.trials = int((self.block_kind == MEASURE).sum())
        if not 1 <= self.num_locations <= circuit_noise.MAX_LOCATIONS:
            raise ValueError("the Monte-Carlo needs 1 <= L <= %d (2^20) fault locations, the %s has %d"
                             % (circuit_noise.MAX_LOCATIONS, what, self.num_locations))
        self.type_eff = np.ascontiguousarray(np.concatenate([t.effects for t in self.types]))
        self.type_locations = np.array([t.num_locations for t in self.types], dtype=np.int64)
        self.type_flags = np.array([t.num_flags for t in self.types], dtype=np.int64)
        self.type_regions = np.ascontiguousarray(np.concatenate([t.regions for t in self.types]))
        self.type_nregions = np.array([len(t.regions) for t in self.types], dtype=np.int64)
        self.preparations = int(sum(int(self.types[t].regions[:, 2].sum()) for t in self.block_type if t >= 0))
        sites = [t.gate_regions() for t in self.types]
        self.type_site_loc = np.ascontiguousarray(np.concatenate([loc for loc, _ in sites]), dtype=np.int32)
        self.type_site_regions = np.ascontiguousarray(np.concatenate([counts for _, counts in sites]), dtype=np.int64)
        self._device = None
        self._retry_device = None
        self._retry_gate_device = None
        self._retry_wait = {}                                       # per wait_steps: (wait_eff, wait_count, wait rows of a sample's preparations)
        self._retry_wait_device = {}
        self._retry_gate_wait_device = {}

    @classmethod
    def cycle(cls, code, rounds, idle_data=False):
        """`rounds` rounds of CSSCode.error_correct (ec_noise.error_correct_gates' gadget; idle_data: one IDLE per data qubit at the
        start of each round), then the FINAL step.  Any rounds >= 1 with L = rounds L_b <= 2^20."""
        rounds = int(rounds)
        if rounds < 1:
            raise ValueError("the error-correction cycle needs rounds >= 1")
        block = BlockType(code, "EC, idle data" if idle_data else "EC", EC, _emit_ec(range(int(code.n)) if idle_data else ()))
        out = cls(code, "cycle", [block], [0] * rounds + [-1], [EC] * rounds + [FINAL])
        out.rounds = rounds
        return out

    @classmethod
    def program(cls, code, ops):
        """The rewritten program `ops; MEASURE` (ft_noise.program_gates' block sequence: the first preparation, an EC block per logical
        gate, then 2t + 1 times a MEASURE trial and an EC block).  Any number of gates; ft_noise.check_ops' refusals."""
        ops = ft_noise.check_ops(ops)
        types, index = [], {}

        def use(name, kind, emit):
            if name not in index:
                index[name] = len(types)
                types.append(BlockType(code, name, kind, emit))
            return index[name]

        ec = lambda op: use("EC" if op == 'I' else "logical %s, EC" % op, EC, _emit_ec(ft_noise.logical_pauli_qubits(code, op)))
        block_type, block_kind = [use("prepare data", NONE, _emit_prepare)], [NONE]
        for op in ops:                                              # ftqc.py:80-83
            block_type.append(ec(op))
            block_kind.append(EC)
        for _ in range(2 * int(code.t) + 1):                        # ftqc.py:84-89, css_code.py:576-579
            block_type += [use("MEASURE trial", MEASURE, _emit_measure), ec('I')]
            block_kind += [MEASURE, EC]
        out = cls(code, "program", types, block_type, block_kind)
        out.ops = ops
        return out

    # -- the whole gadget, as the resident routes see it ---------------------------------------------------------------------
    def gates(self):
        """The gate list of the whole sequence: error_correct_gates' / program_gates'."""
        return np.concatenate([self.types[t].gates for t in self.block_type if t >= 0])

    def locations(self):
        """(L, 2) rows (gate, qubit) of the whole sequence's fault locations, the blocks' one after the other."""
        parts, first_gate = [], 0
        for t in self.block_type:
            if t >= 0:
                parts.append(self.types[t].locations + np.array([first_gate, 0]))
                first_gate += len(self.types[t].gates)
        return np.concatenate(parts)

    def dense_effects(self):
        """The dense effect table (L, 2, ldw) of the whole sequence in the stream layout, rebuilt from the block tables: a fault's
        local word in its own step, its tail under every later step's mask, its flags among its block's flag rows."""
        out = np.zeros((self.num_locations, 2, self.ldw), dtype=np.uint64)
        steps = self.block_step
        masks = np.array([FRAME_MASK[int(k)] for k in self.block_kind[steps >= 0]], dtype=np.uint64)
        for b, t in enumerate(self.block_type):
            if t < 0:
                continue
            eff = self.types[t].effects
            rows = slice(int(self.block_start[b]), int(self.block_start[b + 1]))
            if steps[b] >= 0:
                out[rows, :, steps[b]] = eff[:, :, 0]
            later = int(steps[b + 1:].max(initial=-1))
            first = int(steps[b]) + 1 if steps[b] >= 0 else int((steps[:b] >= 0).sum())
            if later >= first:
                out[rows, :, first:later + 1] = eff[:, :, 1, None] & masks[first:later + 1]
            word, shift = divmod(int(self.block_flag[b]), 64)
            out[rows, :, self.nsteps + word] |= eff[:, :, 2] << np.uint64(shift)
            if shift and word + 1 < self.flag_words:
                out[rows, :, self.nsteps + word + 1] |= eff[:, :, 2] >> np.uint64(64 - shift)
        return out

    def to_cycle_layout(self, words):
        """Stream-layout words (.., ldw) of a cycle as ec_noise's [final frame] [round 1 .. rounds] [flag words]."""
        if self.what != "cycle":
            raise ValueError("not a cycle")
        words = np.asarray(words)
        order = [self.nsteps - 1] + list(range(self.nsteps - 1)) + list(range(self.nsteps, self.ldw))
        return np.ascontiguousarray(words[..., order])

    def to_program_layout(self, words):
        """Stream-layout words (.., ldw) of a program as ft_noise's [step 0 .. nsteps - 1] [flag words]: the same order."""
        if self.what != "program":
            raise ValueError("not a program")
        return np.ascontiguousarray(np.asarray(words)[..., :self.ldw])

    # -- the Monte-Carlo -----------------------------------------------------------------------------------------------------
    def _sequence(self):
        return self.type_eff, self.type_locations, self.type_flags, self.block_type, self.block_kind

    def device(self):
        if self._device is None:
            self._device = _native.default_context().stream_create(*self._sequence())
        return self._device

    def _tables(self):
        keys1, flips1, keys2, flips2 = circuit_noise.code_tables(self.code)
        return self.code.r_1, keys1, flips1, self.code.r_2, keys2, flips2

    def _dict(self, counts, samples):
        names = ec_noise.EC_FIELDS if self.what == "cycle" else ft_noise.FT_FIELDS
        out = {name: int(counts[k]) for name, k in zip(names, _CYCLE_FIELDS if self.what == "cycle" else _PROGRAM_FIELDS)}
        out['samples'] = int(samples)
        return out

    def outcomes(self, num_samples, p_x, p_y, p_z, seed=0, first_sample=0):
        """The stream-layout words of samples [first_sample, first_sample + num_samples), rejected ones included: a (num_samples,
        ldw) uint64 array (gf2_stream_outcomes_dev)."""
        ctx = _native.default_context()
        return ctx.outcomes(ctx.stream_outcomes_dev, self.device(), seed, first_sample, num_samples, p_x, p_y, p_z, self.ldw)

    def counts(self, num_samples, p_x, p_y, p_z, seed=0, first_sample=0):
        """The twelve STREAM_FIELDS counts of samples [first_sample, first_sample + num_samples) on the device (gf2_mc_stream_decode)."""
        return _native.default_context().mc_stream_decode(self.device(), *self._tables(), int(seed), int(first_sample), int(num_samples),
                                                          float(p_x), float(p_y), float(p_z))

    def error_rates(self, num_samples, p_x, p_y, p_z, seed=0, first_sample=0):
        """The tally of samples [first_sample, first_sample + num_samples) on the device: a dict of ec_noise.EC_FIELDS for a cycle, of
        ft_noise.FT_FIELDS for a program, plus 'samples'; what ECCircuit.logical_error_rates / FTProgram.measurement_error_rates
        give where they accept the size.  The counts of sample ranges add."""
        return self._dict(self.counts(num_samples, p_x, p_y, p_z, seed, first_sample), num_samples)

    def words_of_faults(self, fault_first, fault_location, fault_kind):
        """The stream-layout words of samples given by their faults, on the host (gf2_stream_words_host, no GPU): sample i has faults
        fault_first[i] .. fault_first[i + 1] - 1, each a location and a kind 1 (X), 2 (Z) or 3 (Y)."""
        return _native.stream_words_host(*self._sequence(), fault_first, fault_location, fault_kind, self.ldw)

    def tally_host(self, words, classes=False, fields=False):
        """The tally rule over stream-layout words (samples, ldw) on the host (gf2_stream_tally_host, no GPU): error_rates' dict;
        fields=True gives the twelve STREAM_FIELDS counts instead, classes=True (result, class byte per sample)."""
        words = np.ascontiguousarray(words, dtype=np.uint64).reshape(-1, self.ldw)
        got = _native.stream_tally_host(words, self.block_kind, self.flag_words, *self._tables(), classes=classes)
        counts = got[0] if classes else got
        out = counts if fields else self._dict(counts, len(words))
        return (out, got[1]) if classes else out

    # -- repeat-until-success ----------------------------------------------------------------------------------------------------
    def _retry_sequence(self):
        return self._sequence() + (self.type_regions, self.type_nregions)

    def retry_device(self):
        if self._retry_device is None:
            self._retry_device = _native.default_context().retry_create(*self._retry_sequence())
        return self._retry_device

    def retry_outcomes(self, num_samples, p_x, p_y, p_z, seed=0, first_sample=0, max_attempts=256):
        """The words of samples [first_sample, first_sample + num_samples) of the repeat-until-success sampler, every preparation
        retried until its verifications pass or max_attempts are used up: a (num_samples, ldw + 1) uint64 array [steps] [flag words,
        zero unless the sample is exhausted] [attempts of the sample] (gf2_retry_outcomes_dev).  The rates are those of the
        post-selected routes at every p; the samples are different samples."""
        ctx = _native.default_context()
        return ctx.outcomes(ctx.retry_outcomes_dev, self.retry_device(), seed, first_sample, num_samples, p_x, p_y, p_z, self.ldw + 1,
                            int(max_attempts))

    def retry_counts(self, num_samples, p_x, p_y, p_z, seed=0, first_sample=0, max_attempts=256):
        """The fourteen RETRY_FIELDS counts of samples [first_sample, first_sample + num_samples) on the device (gf2_mc_retry_decode):
        the STREAM_FIELDS with accepted = not exhausted, the exhausted samples, the attempts of all samples.  The rates are those
        of the post-selected routes at every p; the samples are different samples."""
        return _native.default_context().mc_retry_decode(self.retry_device(), *self._tables(), int(seed), int(first_sample), int(num_samples),
                                                         float(p_x), float(p_y), float(p_z), int(max_attempts))

    def retry_error_rates(self, num_samples, p_x, p_y, p_z, seed=0, first_sample=0, max_attempts=256):
        """error_rates' dict from the repeat-until-success sampler, plus 'exhausted', 'attempts' and 'preparations' (the retried
        regions per sample: attempts / (samples * preparations) is the mean number of attempts per preparation).  The rates are
        those of the post-selected routes at every p; the samples are different samples.  The counts of sample ranges add."""
        counts = self.retry_counts(num_samples, p_x, p_y, p_z, seed, first_sample, max_attempts)
        out = self._dict(counts, num_samples)
        out.update(exhausted=int(counts[12]), attempts=int(counts[13]), preparations=self.preparations)
        return out

    def retry_words_host(self, num_samples, p_x, p_y, p_z, seed=0, first_sample=0, max_attempts=256):
        """retry_outcomes' words on the host (gf2_retry_words_host, no GPU) and the (num_samples, preparations) uint32 attempts of
        every preparation in order, 0 for one never reached.  tally_host on words[:, :ldw] completes the statement.  The rates are
        those of the post-selected routes at every p; the samples are different samples."""
        return _native.retry_words_host(*self._retry_sequence(), seed, first_sample, num_samples, p_x, p_y, p_z, max_attempts, self.ldw + 1,
                                        self.preparations)

    # -- repeat-until-success with waiting faults ---------------------------------------------------------------------------------
    def _retry_wait_sequence(self, wait_steps=1):
        wait_steps = int(wait_steps)
        if wait_steps not in self._retry_wait:
            waits = [t.waits(wait_steps) for t in self.types]
            self._retry_wait[wait_steps] = (np.ascontiguousarray(np.concatenate([eff for eff, _ in waits])),
                                            np.concatenate([count for _, count in waits]).astype(np.int64),
                                            int(sum(int(waits[t][1].sum()) for t in self.block_type if t >= 0)))
        return self._retry_sequence() + self._retry_wait[wait_steps][:2]

    def wait_locations(self, wait_steps=1):
        """The wait rows per attempt summed over the sequence's preparations."""
        self._retry_wait_sequence(wait_steps)
        return self._retry_wait[int(wait_steps)][2]

    def retry_wait_device(self, wait_steps=1):
        wait_steps = int(wait_steps)
        if wait_steps not in self._retry_wait_device:
            self._retry_wait_device[wait_steps] = _native.default_context().retry_wait_create(*self._retry_wait_sequence(wait_steps))
        return self._retry_wait_device[wait_steps]

    def retry_wait_outcomes(self, num_samples, p_x, p_y, p_z, q_x, q_y, q_z, seed=0, first_sample=0, wait_steps=1, max_attempts=256):
        """retry_outcomes with waiting faults (DESIGN.md section 5d "Repeat-until-success with waiting faults"): every attempt made of
        a retried region, the failed ones included, also draws the region's wait rows (BlockType.waits) with the memory error rates
        (q_x, q_y, q_z) into the block's words.  A (num_samples, ldw + 2) uint64 array [steps] [flag words] [attempts] [wait faults
        drawn over all attempts of the sample] (gf2_retry_wait_outcomes_dev).  With q = 0 the first ldw + 1 words are retry_outcomes'."""
        ctx = _native.default_context()
        return ctx.outcomes(ctx.retry_wait_outcomes_dev, self.retry_wait_device(wait_steps), seed, first_sample, num_samples, p_x, p_y, p_z,
                            self.ldw + 2, float(q_x), float(q_y), float(q_z), int(max_attempts))

    def retry_wait_counts(self, num_samples, p_x, p_y, p_z, q_x, q_y, q_z, seed=0, first_sample=0, wait_steps=1, max_attempts=256):
        """The fifteen counts -- the RETRY_FIELDS, then the wait faults of all samples -- of samples [first_sample, first_sample +
        num_samples) on the device (gf2_mc_retry_wait_decode)."""
        return _native.default_context().mc_retry_wait_decode(self.retry_wait_device(wait_steps), *self._tables(), int(seed), int(first_sample),
                                                               int(num_samples), float(p_x), float(p_y), float(p_z), float(q_x), float(q_y),
                                                               float(q_z), int(max_attempts))

    def retry_wait_error_rates(self, num_samples, p_x, p_y, p_z, q_x, q_y, q_z, seed=0, first_sample=0, wait_steps=1, max_attempts=256):
        """retry_error_rates' dict with waiting faults, plus 'wait_faults' (those drawn over all attempts of all samples) and
        'wait_locations' (the wait rows per attempt summed over the sequence's preparations).  The counts of sample ranges add."""
        counts = self.retry_wait_counts(num_samples, p_x, p_y, p_z, q_x, q_y, q_z, seed, first_sample, wait_steps, max_attempts)
        out = self._dict(counts, num_samples)
        out.update(exhausted=int(counts[12]), attempts=int(counts[13]), preparations=self.preparations, wait_faults=int(counts[14]),
                   wait_locations=self.wait_locations(wait_steps))
        return out

    def retry_wait_words_host(self, num_samples, p_x, p_y, p_z, q_x, q_y, q_z, seed=0, first_sample=0, wait_steps=1, max_attempts=256):
        """retry_wait_outcomes' words on the host (gf2_retry_wait_words_host, no GPU) and the (num_samples, preparations) uint32
        attempts of every preparation in order, 0 for one never reached.  tally_host on words[:, :ldw] completes the statement."""
        return _native.retry_wait_words_host(*self._retry_wait_sequence(wait_steps), seed, first_sample, num_samples, p_x, p_y, p_z, q_x, q_y, q_z,
                                             max_attempts, self.ldw + 2, self.preparations)

    # -- repeat-until-success under gate-level faults ----------------------------------------------------------------------------
    def _retry_gate_sequence(self):
        return self._retry_sequence() + (self.type_site_loc, self.type_site_regions)

    def retry_gate_device(self):
        if self._retry_gate_device is None:
            self._retry_gate_device = _native.default_context().retry_gate_create(*self._retry_gate_sequence())
        return self._retry_gate_device

    def retry_gate_outcomes(self, num_samples, p1, p2, seed=0, first_sample=0, max_attempts=256):
        """retry_outcomes under gate-level faults (DESIGN.md section 5d "Repeat-until-success under gate-level faults"): every
        one-operand gate fails with probability p1 and one of 3 kinds, every CNOT as one event with probability p2 and one of 15; a
        (num_samples, ldw + 1) uint64 array [steps] [flag words, zero unless the sample is exhausted] [attempts of the sample]
        (gf2_retry_gate_outcomes_dev).  max_attempts = 1 is gate-level post-selection of any length."""
        ctx = _native.default_context()
        count = int(num_samples)
        buf = ctx.alloc(max(1, count) * (self.ldw + 1) * 8)
        try:
            ctx.retry_gate_outcomes_dev(self.retry_gate_device(), int(seed), int(first_sample), count, float(p1), float(p2), int(max_attempts),
                                        buf, self.ldw + 1)
            return buf.download((count, self.ldw + 1), np.uint64)
        finally:
            buf.free()

    def retry_gate_counts(self, num_samples, p1, p2, seed=0, first_sample=0, max_attempts=256):
        """The fourteen RETRY_FIELDS counts of samples [first_sample, first_sample + num_samples) under gate-level faults on the
        device (gf2_mc_retry_gate_decode)."""
        return _native.default_context().mc_retry_gate_decode(self.retry_gate_device(), *self._tables(), int(seed), int(first_sample),
                                                               int(num_samples), float(p1), float(p2), int(max_attempts))

    def retry_gate_error_rates(self, num_samples, p1, p2, seed=0, first_sample=0, max_attempts=256):
        """retry_error_rates' dict under gate-level faults: the rates per accepted sample are those of ECCircuit / FTProgram
        .gate_error_rates at every (p1, p2) where those accept the size; the samples are different samples.  The counts of sample
        ranges add."""
        counts = self.retry_gate_counts(num_samples, p1, p2, seed, first_sample, max_attempts)
        out = self._dict(counts, num_samples)
        out.update(exhausted=int(counts[12]), attempts=int(counts[13]), preparations=self.preparations)
        return out

    def retry_gate_words_host(self, num_samples, p1, p2, seed=0, first_sample=0, max_attempts=256):
        """retry_gate_outcomes' words on the host (gf2_retry_gate_words_host, no GPU) and the (num_samples, preparations) uint32
        attempts of every preparation in order, 0 for one never reached.  tally_host on words[:, :ldw] completes the statement."""
        return _native.retry_gate_words_host(*self._retry_gate_sequence(), seed, first_sample, num_samples, p1, p2, max_attempts, self.ldw + 1,
                                             self.preparations)

    # -- repeat-until-success with waiting faults under gate-level faults ---------------------------------------------------------
    def _retry_gate_wait_sequence(self, wait_steps=1):
        return self._retry_gate_sequence() + self._retry_wait_sequence(wait_steps)[-2:]

    def retry_gate_wait_device(self, wait_steps=1):
        wait_steps = int(wait_steps)
        if wait_steps not in self._retry_gate_wait_device:
            self._retry_gate_wait_device[wait_steps] = _native.default_context().retry_gate_wait_create(*self._retry_gate_wait_sequence(wait_steps))
        return self._retry_gate_wait_device[wait_steps]

    def retry_gate_wait_outcomes(self, num_samples, p1, p2, q_x, q_y, q_z, seed=0, first_sample=0, wait_steps=1, max_attempts=256):
        """retry_gate_outcomes with waiting faults (DESIGN.md section 5d "Repeat-until-success with waiting faults under gate-level
        faults"): every attempt made of a retried region, the failed ones included, also draws the region's wait rows
        (BlockType.waits) with the memory error rates (q_x, q_y, q_z) into the block's words.  A (num_samples, ldw + 2) uint64 array
        [steps] [flag words] [attempts] [wait faults drawn over all attempts of the sample] (gf2_retry_gate_wait_outcomes_dev).  With
        q = 0 the first ldw + 1 words are retry_gate_outcomes'."""
        ctx = _native.default_context()
        count = int(num_samples)
        buf = ctx.alloc(max(1, count) * (self.ldw + 2) * 8)
        try:
            ctx.retry_gate_wait_outcomes_dev(self.retry_gate_wait_device(wait_steps), int(seed), int(first_sample), count, float(p1), float(p2),
                                             float(q_x), float(q_y), float(q_z), int(max_attempts), buf, self.ldw + 2)
            return buf.download((count, self.ldw + 2), np.uint64)
        finally:
            buf.free()

    def retry_gate_wait_counts(self, num_samples, p1, p2, q_x, q_y, q_z, seed=0, first_sample=0, wait_steps=1, max_attempts=256):
        """The fifteen counts -- the RETRY_FIELDS, then the wait faults of all samples -- of samples [first_sample, first_sample +
        num_samples) under gate-level faults on the device (gf2_mc_retry_gate_wait_decode)."""
        return _native.default_context().mc_retry_gate_wait_decode(self.retry_gate_wait_device(wait_steps), *self._tables(), int(seed),
                                                                    int(first_sample), int(num_samples), float(p1), float(p2), float(q_x),
                                                                    float(q_y), float(q_z), int(max_attempts))

    def retry_gate_wait_error_rates(self, num_samples, p1, p2, q_x, q_y, q_z, seed=0, first_sample=0, wait_steps=1, max_attempts=256):
        """retry_gate_error_rates' dict with waiting faults, plus 'wait_faults' (those drawn over all attempts of all samples) and
        'wait_locations' (the wait rows per attempt summed over the sequence's preparations).  The counts of sample ranges add."""
        counts = self.retry_gate_wait_counts(num_samples, p1, p2, q_x, q_y, q_z, seed, first_sample, wait_steps, max_attempts)
        out = self._dict(counts, num_samples)
        out.update(exhausted=int(counts[12]), attempts=int(counts[13]), preparations=self.preparations, wait_faults=int(counts[14]),
                   wait_locations=self.wait_locations(wait_steps))
        return out

    def retry_gate_wait_words_host(self, num_samples, p1, p2, q_x, q_y, q_z, seed=0, first_sample=0, wait_steps=1, max_attempts=256):
        """retry_gate_wait_outcomes' words on the host (gf2_retry_gate_wait_words_host, no GPU) and the (num_samples, preparations)
        uint32 attempts of every preparation in order, 0 for one never reached.  tally_host on words[:, :ldw] completes the statement."""
        return _native.retry_gate_wait_words_host(*self._retry_gate_wait_sequence(wait_steps), seed, first_sample, num_samples, p1, p2, q_x, q_y,
                                                  q_z, max_attempts, self.ldw + 2, self.preparations)


CNOT = _native.MSTREAM_CNOT
MULTI_FIELDS = ('accepted', 'wrong_any', 'unmatched_x', 'unmatched_z')
MEASUREMENT_FIELDS = ('wrong', 'trial_wrong', 'first_trial_wrong', 'split_vote')
RECORDS = {'reference': _native.MSTREAM_REFERENCE, 'propagated': _native.MSTREAM_PROPAGATED}
_LOW, _HIGH = np.uint64(0x00000000FFFFFFFF), np.uint64(0xFFFFFFFF00000000)


def _emit_pauli(qubits):
    """The physical Paulis of a logical gate alone, one IDLE location each (a block of kind NONE)."""
    def emit(build):
        build.gates.extend((GATE_IDLE, build.data[q], 0) for q in qubits)
    return emit


class CnotBlockType(object):
    """The block type of a transversal CNOT: `gates`, n rows (GATE_CNOT, i, n + i) on the 2n qubits of the data blocks a (0 .. n-1)
    and b (n .. 2n-1); `locations` (2n, 2); no flag rows; `effects` (2n, 2, 3) uint64: (the tail the fault leaves on frame a, the
    tail it leaves on frame b, 0) of an X and of a Z fault, from gf2_circuit_effects_timed on this gate list with the final-frame
    rows of block a in word 0 and of block b in word 1; `regions`, the one region (0, 2n, 0): nothing of a CNOT block is retried."""

    def __init__(self, code):
        n, r_1, r_2 = int(code.n), int(code.r_1), int(code.r_2)
        h_1, h_2 = np.asarray(code.parity_check_c1), np.asarray(code.parity_check_c2)
        z_op, x_op = np.asarray(code.z_operator_matrix())[0], np.asarray(code.x_operator_matrix())[0]
        self.name, self.kind, self.num_flags = "CNOT", CNOT, 0
        self.gates = np.array([(GATE_CNOT, i, n + i) for i in range(n)], dtype=np.int32).reshape(-1, 3)
        rows_x = np.zeros((64 * 3, 2 * n), dtype=np.uint8)
        rows_z = np.zeros_like(rows_x)
        for word in range(2):                                       # the tail's layout (BlockType's word 1), once per data block
            block = slice(word * n, (word + 1) * n)
            for i in range(r_2):
                rows_x[64 * word + r_2 - 1 - i, block] = h_2[i] & 1
            rows_x[64 * word + 31, block] = z_op & 1
            for i in range(r_1):
                rows_z[64 * word + 32 + r_1 - 1 - i, block] = h_1[i] & 1
            rows_z[64 * word + 63, block] = x_op & 1
        self._rows = (2 * n, list(range(n)), _native.pack_rows(rows_x), _native.pack_rows(rows_z), np.full(64 * 3, n, dtype=np.int64))
        self.effects, self.locations = _native.circuit_effects_timed(self.gates, 2 * n, *self._rows[2:], ldr=3)
        self.regions = np.array([[0, 2 * n, 0]], dtype=np.int64)

    @property
    def num_locations(self):
        return len(self.locations)

    def gate_regions(self):
        """The sites of the gate-level fault model (BlockType.gate_regions): (site_loc, [[0, n]]) with site_loc = 0, 2, ..., 2 n - 2.
        Site i is the physical CNOT D_a[i] -> D_b[i]: location 2 i is its control on frame a, 2 i + 1 its target on frame b."""
        loc, n1, n2, _ = circuit_noise.gate_sites(self.gates, self.locations)
        return loc.astype(np.int32), np.array([[n1, n2]], dtype=np.int64)


class MultiProgram(object):
    """A rewritten program on 1 <= Q <= 4 logical qubits with the transversal CNOT, prepared for the Monte-Carlo (DESIGN.md section
    5d "Multi-block programs").  `instructions` as ft_noise.check_instructions takes them; `qubits`, the sorted logical qubit
    indices (data frame f serves qubits[f]).  The block sequence mirrors ftqc.rewrite_program step for step:
        prep(D_q, zero) verified by A1 for every block in index order                 -- NONE blocks
        per gate: a Pauli's IDLE locations on its block, or the n physical CNOTs D_a[i] -> D_b[i] (a CNOT block), then one round of
        error_correct on every block in index order                                   -- EC blocks
        per MEASURE, 2t + 1 times: the MEASURE trial on D_q, then a round of error_correct on every block in index order
    The data blocks wait at no cost while another block is served: the project's standing convention (ec_noise's docstring).
    A Pauli on the first block shares StreamedGadget.program's type "logical P, EC" with the round that follows it; on another
    block its IDLE locations are a block of kind NONE of their own, so that the locations keep the emitted program's order.

    `types`, `block_type`, `block_kind`, `block_a`, `block_b` (-1 unless a CNOT block), `block_start`, `block_step`, `block_flag`,
    `nsteps`, `flag_words`, `ldw` as StreamedGadget's; `measured`, the measured qubits in program order; `preparations`, the
    retried regions of the whole sequence."""

    def __init__(self, code, instructions):
        self.code = code
        self.instructions, self.qubits = ft_noise.check_instructions(instructions)
        frame = {q: f for f, q in enumerate(self.qubits)}
        self.nframes = len(self.qubits)
        types, index = [], {}

        def use(name, kind, emit):
            if name not in index:
                index[name] = len(types)
                types.append(CnotBlockType(code) if kind == CNOT else BlockType(code, name, kind, emit))
            return index[name]

        blocks = []                                                 # (type, kind, a, b)

        def correct_all(first="EC", emit=_emit_ec(())):             # ftqc.py:112-114: every block, in index order
            for f in range(self.nframes):
                blocks.append((use(first, EC, emit) if f == 0 else use("EC", EC, _emit_ec(())), EC, f, -1))

        for f in range(self.nframes):                               # ftqc.py:50-51
            blocks.append((use("prepare data", NONE, _emit_prepare), NONE, f, -1))
        self.measured = []
        for inst in self.instructions:                              # ftqc.py:53-61
            name = inst[0]
            if name == 'CNOT':
                blocks.append((use("CNOT", CNOT, None), CNOT, frame[inst[1]], frame[inst[2]]))
                correct_all()
            elif name == 'MEASURE':
                self.measured.append(inst[1])
                for _ in range(2 * int(code.t) + 1):                # css_code.py:576-579
                    blocks.append((use("MEASURE trial", MEASURE, _emit_measure), MEASURE, frame[inst[1]], -1))
                    correct_all()
            else:
                paulis = ft_noise.logical_pauli_qubits(code, name)
                if paulis and frame[inst[1]] == 0:
                    correct_all("logical %s, EC" % name, _emit_ec(paulis))
                else:
                    if paulis:
                        blocks.append((use("logical %s" % name, NONE, _emit_pauli(paulis)), NONE, frame[inst[1]], -1))
                    correct_all()
        self.types = types
        self.block_type, self.block_kind, self.block_a, self.block_b = (np.array(col, dtype=np.int32) for col in zip(*blocks))
        sizes = np.array([types[t].num_locations for t in self.block_type], dtype=np.int64)
        flags = np.array([types[t].num_flags for t in self.block_type], dtype=np.int64)
        self.block_start = np.concatenate([[0], np.cumsum(sizes)])
        self.block_flag = np.concatenate([[0], np.cumsum(flags)])[:-1]
        has_step = (self.block_kind == EC) | (self.block_kind == MEASURE)
        self.block_step = np.where(has_step, np.cumsum(has_step) - 1, -1)
        self.num_locations = int(self.block_start[-1])
        self.nsteps = int(has_step.sum())
        self.flag_rows = int(flags.sum())
        self.flag_words = max(1, (self.flag_rows + 63) // 64)
        self.ldw = self.nsteps + self.flag_words
        self.trials = 2 * int(code.t) + 1
        if not 1 <= self.num_locations <= circuit_noise.MAX_LOCATIONS:
            raise ValueError("the Monte-Carlo needs 1 <= L <= %d (2^20) fault locations, the program has %d"
                             % (circuit_noise.MAX_LOCATIONS, self.num_locations))
        self.type_eff = np.ascontiguousarray(np.concatenate([t.effects for t in types]))
        self.type_locations = np.array([t.num_locations for t in types], dtype=np.int64)
        self.type_flags = np.array([t.num_flags for t in types], dtype=np.int64)
        self.type_regions = np.ascontiguousarray(np.concatenate([t.regions for t in types]))
        self.type_nregions = np.array([len(t.regions) for t in types], dtype=np.int64)
        self.preparations = int(sum(int(types[t].regions[:, 2].sum()) for t in self.block_type))
        sites = [t.gate_regions() for t in types]
        self.type_site_loc = np.ascontiguousarray(np.concatenate([loc for loc, _ in sites]), dtype=np.int32)
        self.type_site_regions = np.ascontiguousarray(np.concatenate([counts for _, counts in sites]), dtype=np.int64)
        self._device = None
        self._retry_device = None
        self._retry_gate_device = None

    @classmethod
    def from_quil(cls, raw_prog, code):
        """The model of ftqc.rewrite_program(raw_prog, code) for a quil.Program of the accepted shape (ft_noise.instructions_of_quil)."""
        return cls(code, ft_noise.instructions_of_quil(raw_prog))

    # -- the whole program ----------------------------------------------------------------------------------------------------
    def _block_qubits(self, b):
        """The program's qubit of every qubit of block b's gate list: D_f = f n .., A1 = Q n .., A2 = (Q + 1) n .. (the order in which
        rewrite_program allocates them)."""
        n, q = int(self.code.n), self.nframes
        bases = [self.block_a[b], self.block_b[b]] if self.block_kind[b] == CNOT else [self.block_a[b], q, q + 1]
        return np.concatenate([np.arange(n) + int(base) * n for base in bases])

    def gates(self):
        """The gate list of the whole program on (Q + 2) n qubits: the quantum instructions ftqc.rewrite_program emits, one pass
        through every loop body."""
        parts = []
        for b, t in enumerate(self.block_type):
            qubit_of = self._block_qubits(b)
            g = self.types[t].gates.copy()
            two = g[:, 0] == GATE_CNOT
            g[:, 1] = qubit_of[g[:, 1]]
            g[two, 2] = qubit_of[g[two, 2]]
            parts.append(g)
        return np.concatenate(parts)

    def locations(self):
        """(L, 2) rows (gate, qubit) of the whole program's fault locations, the blocks' one after the other."""
        parts, first_gate = [], 0
        for b, t in enumerate(self.block_type):
            loc = self.types[t].locations.copy()
            loc[:, 1] = self._block_qubits(b)[loc[:, 1]]
            loc[:, 0] += first_gate
            parts.append(loc)
            first_gate += len(self.types[t].gates)
        return np.concatenate(parts)

    def outcome_rows(self):
        """(rows_x, rows_z, row_time) of the whole program as gf2_circuit_effects_timed takes them, (64 ldw, (Q + 2) n) uint8 each: a
        block's local rows at its step word, its flag rows among the flag words; row r is bit r & 63 of word r >> 6."""
        width = (self.nframes + 2) * int(self.code.n)
        rows = [np.zeros((64 * self.ldw, width), dtype=np.uint8) for _ in range(2)]
        row_time = np.zeros(64 * self.ldw, dtype=np.int64)
        first_gate = 0
        for b, t in enumerate(self.block_type):
            kind = self.types[t]
            if self.block_kind[b] != CNOT:
                qubits, _, packed_x, packed_z, times = kind._rows
                qubit_of = self._block_qubits(b)
                local = slice(0, 64) if self.block_step[b] >= 0 else slice(0, 0)
                moves = [(local, 64 * int(self.block_step[b])), (slice(128, 128 + kind.num_flags), 64 * self.nsteps + int(self.block_flag[b]))]
                for packed, out in zip((packed_x, packed_z), rows):
                    dense = _native.unpack_rows(packed, qubits, dtype=np.uint8)
                    for src, at in moves:
                        out[at:at + (src.stop - src.start)][:, qubit_of] |= dense[src]
                for src, at in moves:
                    row_time[at:at + (src.stop - src.start)] = times[src] + first_gate
            first_gate += len(kind.gates)
        return rows[0], rows[1], row_time

    def dense_effects(self):
        """The dense effect table (L, 2, ldw) of the whole program, rebuilt from the block tables: a fault's local word in its own
        step, its flags among its block's flag rows, and its tails -- pushed through the frame map of every later CNOT block --
        under the mask of every later step of the frame they sit on."""
        out = np.zeros((self.num_locations, 2, self.ldw), dtype=np.uint64)
        for b, t in enumerate(self.block_type):
            eff = self.types[t].effects
            rows = slice(int(self.block_start[b]), int(self.block_start[b + 1]))
            tails = [np.zeros(eff.shape[:2], dtype=np.uint64) for _ in range(self.nframes)]
            if self.block_kind[b] == CNOT:
                tails[self.block_a[b]], tails[self.block_b[b]] = eff[:, :, 0].copy(), eff[:, :, 1].copy()
            else:
                tails[self.block_a[b]] = eff[:, :, 1].copy()
                if self.block_step[b] >= 0:
                    out[rows, :, self.block_step[b]] = eff[:, :, 0]
                word, shift = divmod(int(self.block_flag[b]), 64)
                out[rows, :, self.nsteps + word] |= eff[:, :, 2] << np.uint64(shift)
                if shift and word + 1 < self.flag_words:
                    out[rows, :, self.nsteps + word + 1] |= eff[:, :, 2] >> np.uint64(64 - shift)
            for c in range(b + 1, len(self.block_type)):
                fa, fb = int(self.block_a[c]), int(self.block_b[c])
                if self.block_kind[c] == CNOT:
                    tails[fb] = tails[fb] ^ (tails[fa] & _LOW)
                    tails[fa] = tails[fa] ^ (tails[fb] & _HIGH)
                elif self.block_step[c] >= 0:
                    out[rows, :, self.block_step[c]] = tails[fa] & FRAME_MASK[int(self.block_kind[c])]
        return out

    # -- the Monte-Carlo -----------------------------------------------------------------------------------------------------
    def _sequence(self):
        return (self.type_eff, self.type_locations, self.type_flags, self.block_type, self.block_kind, self.block_a, self.block_b,
                self.nframes)

    def device(self):
        if self._device is None:
            self._device = _native.default_context().mstream_create(*self._sequence())
        return self._device

    def _tables(self):
        keys1, flips1, keys2, flips2 = circuit_noise.code_tables(self.code)
        return self.code.r_1, keys1, flips1, self.code.r_2, keys2, flips2

    @staticmethod
    def _records(records):
        if records not in RECORDS:
            raise ValueError("records must be 'reference' or 'propagated', got %r" % (records,))
        return RECORDS[records]

    def _dict(self, counts, samples):
        out = {name: int(counts[k]) for k, name in enumerate(MULTI_FIELDS)}
        out['measurements'] = [dict({name: int(counts[4 + 4 * m + k]) for k, name in enumerate(MEASUREMENT_FIELDS)}, qubit=q)
                               for m, q in enumerate(self.measured)]
        out['samples'] = int(samples)
        return out

    def outcomes(self, num_samples, p_x, p_y, p_z, seed=0, first_sample=0):
        """The words [steps] [flag words] of samples [first_sample, first_sample + num_samples), rejected ones included: a
        (num_samples, ldw) uint64 array (gf2_mstream_outcomes_dev).  They do not depend on `records`."""
        ctx = _native.default_context()
        return ctx.outcomes(ctx.mstream_outcomes_dev, self.device(), seed, first_sample, num_samples, p_x, p_y, p_z, self.ldw)

    def counts(self, num_samples, p_x, p_y, p_z, seed=0, first_sample=0, records='reference'):
        """The twenty counts of samples [first_sample, first_sample + num_samples) on the device (gf2_mc_mstream_decode): the
        MULTI_FIELDS, then the MEASUREMENT_FIELDS of every MEASURE in program order, zero for the absent ones."""
        return _native.default_context().mc_mstream_decode(self.device(), self._records(records), *self._tables(), int(seed), int(first_sample),
                                                           int(num_samples), float(p_x), float(p_y), float(p_z))

    def error_rates(self, num_samples, p_x, p_y, p_z, seed=0, first_sample=0, records='reference'):
        """The tally of samples [first_sample, first_sample + num_samples) on the device: a dict of the MULTI_FIELDS, 'samples' and
        'measurements', per MEASURE in program order a dict of its qubit and the MEASUREMENT_FIELDS.  records='reference' leaves
        the records of known errors alone at a CNOT, as the rewritten program does; 'propagated' moves them as the CNOT moves the
        errors.  Every field but 'accepted' counts among accepted samples; the counts of sample ranges add."""
        return self._dict(self.counts(num_samples, p_x, p_y, p_z, seed, first_sample, records), num_samples)

    def words_of_faults(self, fault_first, fault_location, fault_kind):
        """The words of samples given by their faults, on the host (gf2_mstream_words_host, no GPU): sample i has faults
        fault_first[i] .. fault_first[i + 1] - 1, each a location and a kind 1 (X), 2 (Z) or 3 (Y)."""
        return _native.mstream_words_host(*self._sequence(), fault_first, fault_location, fault_kind, self.ldw)

    def tally_host(self, words, records='reference', classes=False, fields=False):
        """The tally rule over words (samples, ldw) on the host (gf2_mstream_tally_host, no GPU): error_rates' dict; fields=True gives
        the twenty counts instead, classes=True (result, class byte per sample)."""
        words = np.ascontiguousarray(words, dtype=np.uint64).reshape(-1, self.ldw)
        got = _native.mstream_tally_host(words, self.block_kind, self.block_a, self.block_b, self.nframes, self.flag_words,
                                         self._records(records), *self._tables(), classes=classes)
        counts = got[0] if classes else got
        out = counts if fields else self._dict(counts, len(words))
        return (out, got[1]) if classes else out

    # -- repeat-until-success ----------------------------------------------------------------------------------------------------
    def _retry_sequence(self):
        return self._sequence() + (self.type_regions, self.type_nregions)

    def retry_device(self):
        if self._retry_device is None:
            self._retry_device = _native.default_context().mretry_create(*self._retry_sequence())
        return self._retry_device

    def retry_outcomes(self, num_samples, p_x, p_y, p_z, seed=0, first_sample=0, max_attempts=256):
        """The words of samples [first_sample, first_sample + num_samples) of the repeat-until-success sampler, every preparation
        retried until its verifications pass or max_attempts are used up: a (num_samples, ldw + 1) uint64 array [steps] [flag words,
        zero unless the sample is exhausted] [attempts of the sample] (gf2_mretry_outcomes_dev).  The other data blocks wait at no
        cost while a preparation is repeated.  The rates are those of the post-selected route; the samples are different samples."""
        ctx = _native.default_context()
        return ctx.outcomes(ctx.mretry_outcomes_dev, self.retry_device(), seed, first_sample, num_samples, p_x, p_y, p_z, self.ldw + 1,
                            int(max_attempts))

    def retry_counts(self, num_samples, p_x, p_y, p_z, seed=0, first_sample=0, records='reference', max_attempts=256):
        """The twenty-two counts of samples [first_sample, first_sample + num_samples) on the device (gf2_mc_mretry_decode): counts'
        twenty with accepted = not exhausted, the exhausted samples, the attempts of all samples."""
        records = self._records(records)
        return _native.default_context().mc_mretry_decode(self.retry_device(), records, *self._tables(), int(seed), int(first_sample),
                                                          int(num_samples), float(p_x), float(p_y), float(p_z), int(max_attempts))

    def retry_error_rates(self, num_samples, p_x, p_y, p_z, seed=0, first_sample=0, records='reference', max_attempts=256):
        """error_rates' dict from the repeat-until-success sampler, plus 'exhausted', 'attempts' and 'preparations' (the retried
        regions per sample: attempts / (samples * preparations) is the mean number of attempts per preparation).  The counts of
        sample ranges add."""
        counts = self.retry_counts(num_samples, p_x, p_y, p_z, seed, first_sample, records, max_attempts)
        out = self._dict(counts, num_samples)
        out.update(exhausted=int(counts[20]), attempts=int(counts[21]), preparations=self.preparations)
        return out

    def retry_words_host(self, num_samples, p_x, p_y, p_z, seed=0, first_sample=0, max_attempts=256):
        """retry_outcomes' words on the host (gf2_mretry_words_host, no GPU) and the (num_samples, preparations) uint32 attempts of
        every preparation in order, 0 for one never reached.  tally_host on words[:, :ldw] completes the statement."""
        return _native.mretry_words_host(*self._retry_sequence(), seed, first_sample, num_samples, p_x, p_y, p_z, max_attempts, self.ldw + 1,
                                         self.preparations)

    # -- repeat-until-success under gate-level faults ----------------------------------------------------------------------------
    def _retry_gate_sequence(self):
        return self._retry_sequence() + (self.type_site_loc, self.type_site_regions)

    def retry_gate_device(self):
        if self._retry_gate_device is None:
            self._retry_gate_device = _native.default_context().mretry_gate_create(*self._retry_gate_sequence())
        return self._retry_gate_device

    def retry_gate_outcomes(self, num_samples, p1, p2, seed=0, first_sample=0, max_attempts=256):
        """retry_outcomes under gate-level faults (DESIGN.md section 5d "Repeat-until-success of multi-block programs under gate-level
        faults"): every one-operand gate fails with probability p1 and one of 3 kinds, every CNOT -- those of a CNOT block
        included, where the event acts on both data frames -- as one event with probability p2 and one of 15; a (num_samples, ldw
        + 1) uint64 array [steps] [flag words, zero unless the sample is exhausted] [attempts of the sample]
        (gf2_mretry_gate_outcomes_dev).  max_attempts = 1 is gate-level post-selection."""
        ctx = _native.default_context()
        count = int(num_samples)
        buf = ctx.alloc(max(1, count) * (self.ldw + 1) * 8)
        try:
            ctx.mretry_gate_outcomes_dev(self.retry_gate_device(), int(seed), int(first_sample), count, float(p1), float(p2), int(max_attempts),
                                         buf, self.ldw + 1)
            return buf.download((count, self.ldw + 1), np.uint64)
        finally:
            buf.free()

    def retry_gate_counts(self, num_samples, p1, p2, seed=0, first_sample=0, records='reference', max_attempts=256):
        """retry_counts' twenty-two counts of samples [first_sample, first_sample + num_samples) under gate-level faults on the
        device (gf2_mc_mretry_gate_decode)."""
        records = self._records(records)
        return _native.default_context().mc_mretry_gate_decode(self.retry_gate_device(), records, *self._tables(), int(seed), int(first_sample),
                                                                int(num_samples), float(p1), float(p2), int(max_attempts))

    def retry_gate_error_rates(self, num_samples, p1, p2, seed=0, first_sample=0, records='reference', max_attempts=256):
        """retry_error_rates' dict under gate-level faults.  The counts of sample ranges add."""
        counts = self.retry_gate_counts(num_samples, p1, p2, seed, first_sample, records, max_attempts)
        out = self._dict(counts, num_samples)
        out.update(exhausted=int(counts[20]), attempts=int(counts[21]), preparations=self.preparations)
        return out

    def retry_gate_words_host(self, num_samples, p1, p2, seed=0, first_sample=0, max_attempts=256):
        """retry_gate_outcomes' words on the host (gf2_mretry_gate_words_host, no GPU) and the (num_samples, preparations) uint32
        attempts of every preparation in order, 0 for one never reached.  tally_host on words[:, :ldw] completes the statement."""
        return _native.mretry_gate_words_host(*self._retry_gate_sequence(), seed, first_sample, num_samples, p1, p2, max_attempts, self.ldw + 1,
                                              self.preparations)


def multi_program_for(code, instructions):
    """MultiProgram(code, instructions), cached on the code object."""
    cache = code.__dict__.setdefault("_multi_programs", {})
    key = ft_noise.check_instructions(instructions)[0]
    if key not in cache:
        cache[key] = MultiProgram(code, key)
    return cache[key]


def stream_for(code, what, key):
    """StreamedGadget.cycle(code, *key) or StreamedGadget.program(code, key), cached on the code object."""
    cache = code.__dict__.setdefault("_streamed_gadgets", {})
    if (what, key) not in cache:
        cache[(what, key)] = StreamedGadget.cycle(code, *key) if what == "cycle" else StreamedGadget.program(code, key)
    return cache[(what, key)]
