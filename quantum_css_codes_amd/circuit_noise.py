"""
Circuit-level fault Monte-Carlo [build-defined; DESIGN.md "Circuit faults"].

The reference warns that its encoders are not fault tolerant: "any physical errors that occur during preparation may create
many correlated errors in the code block" (noisy_encode_zero / noisy_encode_plus, css_code.py:203-312).  This module answers
what a fault INSIDE such a circuit does to the block.  A gate list -- rows (kind, a, b): GATE_H on a, GATE_CNOT control a target
b, GATE_IDLE on a (no action) -- has one fault location per gate operand, in gate order (CNOT: control, then target).  Every
location fails independently with a Pauli X, Y or Z (p_x, p_y, p_z): a CNOT has no correlated two-qubit fault, and a qubit no
gate touches has no fault (IDLE gates model input or memory noise).  Sample i draws its faults from the Monte-Carlo sampler of
DESIGN.md "Sampler" run over the L locations instead of n qubits.  The Pauli frame starts at zero, every gate acts on it (H:
swap e_x[a], e_z[a]; CNOT: e_x[b] ^= e_x[a], e_z[a] ^= e_z[b]) and then its locations' faults are XOR-ed in.

Frame propagation is linear over GF(2), so the syndromes and logical parities of the final frame are the XOR of one
precomputed effect per fault (gf2_circuit_effects, host code); the device kernels gather those and never store a frame.

After encode_zero only `logical_x` (a flipped logical Z measurement) is physical -- Z-type operators act trivially on |0_L> --
and after encode_plus only `logical_z`; both are reported as statistics of the frame.
"""
import math

import numpy as np

from . import _native
from . import montecarlo

GATE_H, GATE_CNOT, GATE_IDLE = _native.GATE_H, _native.GATE_CNOT, _native.GATE_IDLE
MAX_LOCATIONS = _native.CIRCUIT_MAX_LOCATIONS
MAX_ROWS = 64 * _native.CIRCUIT_MAX_LDR
# FaultCircuit.enumerate_strata's default budget of configurations: about ten seconds of one MI355X (DESIGN.md "Exact strata")
ENUMERATE_BUDGET = 1 << 32


def _gates(gates):
    gates = np.ascontiguousarray(gates, dtype=np.int32)
    if gates.size == 0:
        return gates.reshape(0, 3)
    if gates.ndim != 2 or gates.shape[1] != 3:
        raise ValueError("gates must be rows (kind, a, b)")
    return gates


def fault_locations(gates):
    """The fault locations of a gate list as an (L, 2) int64 array of (gate index, qubit): H and IDLE give one, (g, a); CNOT
    two, (g, a) then (g, b)."""
    gates = _gates(gates)
    if np.any((gates[:, 0] < GATE_H) | (gates[:, 0] > GATE_IDLE)):
        raise ValueError("unknown gate kind (0 = H, 1 = CNOT, 2 = IDLE)")
    index = np.arange(len(gates), dtype=np.int64)
    two = gates[:, 0] == GATE_CNOT
    order = np.concatenate((2 * index, 2 * index[two] + 1))
    rows = np.concatenate((np.stack((index, gates[:, 1].astype(np.int64)), axis=1),
                           np.stack((index[two], gates[two, 2].astype(np.int64)), axis=1)))
    return rows[np.argsort(order, kind='stable')]


def _key_words(r):
    return 1 if r <= 63 else 2


def _parity_bytes(words, operator):
    """operator . row (mod 2) for every row of packed `words` (entries x w) as uint8."""
    masked = np.ascontiguousarray(words & operator[None, :words.shape[1]])
    return (np.unpackbits(masked.view(np.uint8), axis=1).sum(axis=1) & 1).astype(np.uint8)


def code_tables(code):
    """(keys1, flips1, keys2, flips2) of a code's syndrome tables: keys as gf2_mc_decode_hashed takes them and one flip byte per
    entry (x_operator . correction for C1's table, z_operator . correction for C2's), cached on the code object like decode_local's."""
    cached = getattr(code, "_hashed_table_arrays", None)
    if cached is None or cached[0] is not code._c1_syndromes or cached[1] is not code._c2_syndromes:
        cached = (code._c1_syndromes, code._c2_syndromes, montecarlo.table_entries(code._c1_syndromes, code.r_1, code.n),
                  montecarlo.table_entries(code._c2_syndromes, code.r_2, code.n))
        code._hashed_table_arrays = cached
    flips = getattr(code, "_circuit_flip_arrays", None)
    if flips is None or flips[0] is not cached:
        two = lambda vec: np.pad(_native.pack_rows(np.asarray(vec).reshape(1, -1))[0], (0, 2))[:2]
        flips = (cached, _parity_bytes(cached[2][1], two(code.x_operator_matrix()[0])),
                 _parity_bytes(cached[3][1], two(code.z_operator_matrix()[0])))
        code._circuit_flip_arrays = flips
    return cached[2][0], flips[1], cached[3][0], flips[2]


def gadget_enumerate_request(total, weights, first_rank, count, max_configurations, what):
    """The argument rules of the exact strata over `total` locations (FaultCircuit.enumerate_strata and ec_noise.Gadget's, `what`
    naming the circuit or gadget): (weights, firsts, counts) as lists of ints, ValueError for a weight, a range or a size that is refused."""
    weights = [int(w) for w in np.asarray(weights).reshape(-1)]
    limit = min(total, _native.ENUMERATE_MAX_WEIGHT)
    if any(w < 0 or w > limit for w in weights):
        raise ValueError("an enumerated stratum's weight lies in [0, min(L = %d, %d)]" % (total, _native.ENUMERATE_MAX_WEIGHT))
    if not 1 <= total <= MAX_LOCATIONS:
        raise ValueError("the enumeration needs 1 <= L <= %d (2^20) fault locations, the %s has %d" % (MAX_LOCATIONS, what, total))
    subsets = [math.comb(total, w) for w in weights]
    firsts = [0] * len(weights) if first_rank is None else [int(v) for v in np.broadcast_to(np.asarray(first_rank, dtype=object), (len(weights),))]
    counts = ([c - f for c, f in zip(subsets, firsts)] if count is None
              else [int(v) for v in np.broadcast_to(np.asarray(count, dtype=object), (len(weights),))])
    for w, c, f, n in zip(weights, subsets, firsts, counts):
        if f < 0 or n < 0 or f + n > c:
            raise ValueError("ranks [%d, %d + %d) leave the range [0, C(%d, %d) = %d)" % (f, f, n, total, w, c))
    size = sum(n * 3**w for w, n in zip(weights, counts))
    budget = ENUMERATE_BUDGET if max_configurations is None else int(max_configurations)
    if size > budget:
        raise ValueError("%d fault configurations to enumerate, more than max_configurations = %d" % (size, budget))
    return weights, firsts, counts


def gate_sites(gates, locations):
    """The sites of the gate-level fault model of a gate list whose fault locations are `locations`, (L, 2)
    rows (gate index, qubit) in location order: (site_loc, n1, n2, site_gate).  The n1 one-operand gates come first, then the n2
    CNOTs, each in gate order; site_loc[s] (int32) is the first location of site s -- a CNOT's control, its target being
    site_loc[s] + 1 -- and site_gate[s] its gate index.  The sites partition [0, L): n1 + 2 n2 = L."""
    gates = _gates(gates)
    loc_gate = np.asarray(locations, dtype=np.int64).reshape(-1, 2)[:, 0]
    two = gates[:, 0] == GATE_CNOT
    if len(loc_gate) and (loc_gate.min() < 0 or loc_gate.max() >= len(gates) or np.any(np.diff(loc_gate) < 0)):
        raise ValueError("the locations must be in gate order, each on a gate of the list")
    per_gate = np.bincount(loc_gate, minlength=len(gates))
    if np.any(per_gate != np.where(two, 2, 1)):
        raise ValueError("every gate needs its own fault locations: two for a CNOT, one for any other gate")
    first = np.concatenate(([0], np.cumsum(per_gate)[:-1])).astype(np.int64)
    site_gate = np.concatenate((np.nonzero(~two)[0], np.nonzero(two)[0])).astype(np.int64)
    return first[site_gate].astype(np.int32), int(np.count_nonzero(~two)), int(np.count_nonzero(two)), site_gate


def gate_enumerate_request(n1, n2, weights, max_configurations, what):
    """The argument rules of ECCircuit / FTProgram.enumerate_gate_strata: the weights as a list of ints, ValueError for a weight or a
    size that is refused (the size is named)."""
    weights = [int(w) for w in np.asarray(weights).reshape(-1)]
    if any(w < 0 or w > _native.GATE_ENUMERATE_MAX_WEIGHT for w in weights):
        raise ValueError("a gate-fault stratum's weight lies in [0, %d]" % _native.GATE_ENUMERATE_MAX_WEIGHT)
    if not 1 <= n1 + 2 * n2 <= MAX_LOCATIONS:
        raise ValueError("the enumeration needs 1 <= L <= %d (2^20) fault locations, the %s has %d" % (MAX_LOCATIONS, what, n1 + 2 * n2))
    size = sum(math.comb(n1, w - b) * math.comb(n2, b) * 3**(w - b) * 15**b for w in weights for b in range(w + 1))
    budget = ENUMERATE_BUDGET if max_configurations is None else int(max_configurations)
    if size > budget:
        raise ValueError("%d gate-fault configurations to enumerate, more than max_configurations = %d" % (size, budget))
    return weights


class FaultCircuit(object):
    """
    A gate list on n qubits with outcome rows, prepared for the Monte-Carlo: the effect table (host) and, on first use, its
    device copy.  FaultCircuit(gates, n, rows_x, rows_z) takes any outcome rows (dense 0/1 arrays, at most 512 rows; row r is
    bit r & 63 of word r >> 6 of a sample's outcome words); FaultCircuit.for_code(code, gates) lays out the syndromes and the two
    logical parities of a CSSCode's final frame the way `monte_carlo` and `logical_error_rates` read them:
        [key_x: kw(r_2) words] [key_z: kw(r_1) words] [parity: 1 word],  kw(r) = 1 for r <= 63, else 2 (low word first),
    key_x = vec_to_int(parity_check_c2 . e_x), key_z = vec_to_int(parity_check_c1 . e_z), parity bit 0 = z_operator . e_x,
    bit 1 = x_operator . e_z.
    """

    def __init__(self, gates, n, rows_x, rows_z, code=None):
        self.gates = _gates(gates)
        self.n = int(n)
        rows_x, rows_z = np.asarray(rows_x), np.asarray(rows_z)
        if rows_x.ndim != 2 or rows_x.shape != rows_z.shape or rows_x.shape[1] != self.n:
            raise ValueError("rows_x and rows_z must be (rows, n) arrays of one shape")
        if self.n < 1 or self.n > _native.CIRCUIT_MAX_N:
            raise ValueError("circuit faults need 1 <= n <= %d qubits" % _native.CIRCUIT_MAX_N)
        if not 1 <= rows_x.shape[0] <= MAX_ROWS:
            raise ValueError("circuit faults need 1 to %d outcome rows (ldr <= %d words per sample)" % (MAX_ROWS, _native.CIRCUIT_MAX_LDR))
        self.rows = int(rows_x.shape[0])
        self.code = code
        self.effects, self.locations = _native.circuit_effects(self.gates, self.n, _native.pack_rows(rows_x), _native.pack_rows(rows_z))
        self.ldr = int(self.effects.shape[2])
        self._device = None

    @classmethod
    def for_code(cls, code, gates):
        r_1, r_2, n = code.r_1, code.r_2, code.n
        if min(r_1, r_2) < 1 or max(r_1, r_2) > 127:
            raise ValueError("the Monte-Carlo layout of a circuit's outcomes needs 1 <= r_1, r_2 <= 127")
        kwx, kwz = _key_words(r_2), _key_words(r_1)
        rows_x = np.zeros((64 * (kwx + kwz + 1), n), dtype=np.uint8)
        rows_z = np.zeros_like(rows_x)
        rows_x[r_2 - 1 - np.arange(r_2)] = code.parity_check_c2                 # vec_to_int: row 0 is the most significant bit
        rows_z[64 * kwx + r_1 - 1 - np.arange(r_1)] = code.parity_check_c1
        rows_x[64 * (kwx + kwz)] = code.z_operator_matrix()[0]
        rows_z[64 * (kwx + kwz) + 1] = code.x_operator_matrix()[0]
        return cls(gates, n, rows_x, rows_z, code=code)

    @property
    def num_locations(self):
        return len(self.locations)

    def device(self):
        if self._device is None:
            if not 1 <= self.num_locations <= MAX_LOCATIONS:
                raise ValueError("the Monte-Carlo needs 1 <= L <= %d (2^20) fault locations, the circuit has %d"
                                 % (MAX_LOCATIONS, self.num_locations))
            self._device = _native.default_context().circuit_create(self.effects)
        return self._device

    def outcomes(self, num_samples, p_x, p_y, p_z, seed=0, first_sample=0):
        """The outcome words of samples [first_sample, first_sample + num_samples): a (num_samples, ldr) uint64 array."""
        ctx = _native.default_context()
        return ctx.outcomes(ctx.circuit_outcomes_dev, self.device(), seed, first_sample, num_samples, p_x, p_y, p_z, self.ldr)

    def _need_code(self):
        if self.code is None:
            raise ValueError("histograms and the table decode need a circuit made by FaultCircuit.for_code")
        return self.code

    def monte_carlo(self, num_samples, p_x, p_y, p_z, seed=0, first_sample=0, mode=None):
        """Histograms of the final frame's syndromes, shaped like CSSCode.monte_carlo's."""
        code = self._need_code()
        mode = montecarlo.pick_mode(code.r_1, code.r_2, mode)
        hist_z, hist_x = _native.default_context().mc_circuit_run(
            self.device(), code.r_1, code.r_2, int(seed), int(first_sample), int(num_samples), float(p_x), float(p_y), float(p_z),
            _native.HIST_FULL if mode == 'full' else _native.HIST_WEIGHT)
        return {'hist_z': hist_z, 'hist_x': hist_x, 'mode': mode}

    def _tables(self):
        return code_tables(self.code)

    def logical_error_rates(self, num_samples, p_x, p_y, p_z, seed=0, first_sample=0):
        """Table decode + logical tally of the final frame by CSSCode.logical_error_rates' rule; the same dict of counts."""
        code = self._need_code()
        if code.n > 128:
            raise ValueError("the table decode of a circuit's final frame needs n <= 128 (where the syndrome tables exist)")
        keys1, flips1, keys2, flips2 = self._tables()
        counts = _native.default_context().mc_circuit_decode(
            self.device(), code.r_1, keys1, flips1, code.r_2, keys2, flips2, int(seed), int(first_sample), int(num_samples),
            float(p_x), float(p_y), float(p_z))
        out = {name: int(v) for name, v in zip(montecarlo.DECODE_FIELDS, counts)}
        out['samples'] = int(num_samples)
        return out

    def logical_error_strata(self, weights, samples, kinds=(1, 1, 1), seed=0, first_sample=0):
        """The strata of logical_error_rates (DESIGN.md "Strata"): stratum s draws samples [first_sample, first_sample + samples[s])
        of exactly weights[s] faults among the L locations (at most 16), kinds X : Y : Z = kinds.  Returns a montecarlo.Strata over
        nb = L, whose rate(p_t) is the logical error rate at fault probability p_t per location."""
        code = self._need_code()
        if code.n > 128:
            raise ValueError("the table decode of a circuit's final frame needs n <= 128 (where the syndrome tables exist)")
        weights, samples, firsts, kinds = montecarlo._strata_request(weights, samples, kinds, first_sample)
        limit = min(self.num_locations, _native.CIRCUIT_STRATUM_MAX_WEIGHT)
        if any(w < 0 or w > limit for w in weights):
            raise ValueError("a circuit stratum's weight lies in [0, min(L = %d, %d)]" % (self.num_locations, _native.CIRCUIT_STRATUM_MAX_WEIGHT))
        keys1, flips1, keys2, flips2 = self._tables()
        ctx, circ = _native.default_context(), self.device()
        counts = np.zeros((len(weights), len(montecarlo.DECODE_FIELDS)), dtype=np.uint64)
        for first, rows in montecarlo._strata_calls(firsts):
            counts[rows] = ctx.mc_circuit_decode_strata(circ, code.r_1, keys1, flips1, code.r_2, keys2, flips2, int(seed), int(first),
                                                        [weights[s] for s in rows], samples[rows], *kinds)
        return montecarlo.Strata(self.num_locations, weights, samples, counts, kinds)

    def enumerate_strata(self, weights, first_rank=None, count=None, max_configurations=None, host=False):
        """Exact strata (DESIGN.md "Exact strata"): every configuration of exactly weights[s] <= 8 faults -- each subset of the L
        locations with every assignment of X, Y, Z to its picks -- decoded and tallied by logical_error_rates' rule, counted per
        kind composition.  Nothing is sampled.  `first_rank` and `count` (one number or one per weight; default: everything)
        select the subsets of ranks [first_rank, first_rank + count) in the combinatorial number system; the counts of parts add
        up.  More than `max_configurations` (default ENUMERATE_BUDGET) configurations in all is a ValueError.  host=True runs
        the serial host statement and needs no GPU.  Returns a montecarlo.ExactStrata over nb = L, which is meaningful as whole
        strata (fractions, rate) only when the ranges are whole."""
        code = self._need_code()
        if code.n > 128:
            raise ValueError("the table decode of a circuit's final frame needs n <= 128 (where the syndrome tables exist)")
        total = self.num_locations
        weights, firsts, counts = gadget_enumerate_request(total, weights, first_rank, count, max_configurations, "circuit")
        keys1, flips1, keys2, flips2 = self._tables()
        if host:
            run = lambda w, f, n: _native.circuit_enumerate_host(self.effects, code.r_1, keys1, flips1, code.r_2, keys2, flips2, w, f, n)
        else:
            ctx, circ = _native.default_context(), self.device()
            run = lambda w, f, n: ctx.circuit_enumerate(circ, code.r_1, keys1, flips1, code.r_2, keys2, flips2, w, f, n)
        return montecarlo.ExactStrata(total, weights, [run(w, f, n) for w, f, n in zip(weights, firsts, counts)])

    # The two with montecarlo.run_sharded's / decode_sharded's local_fn signature (the code argument must be this circuit's).
    def run_local(self, code, num_samples, p_x, p_y, p_z, seed=0, first_sample=0, mode=None):
        if code is not self.code:
            raise ValueError("this circuit was made for another code object")
        return self.monte_carlo(num_samples, p_x, p_y, p_z, seed=seed, first_sample=first_sample, mode=mode)

    def decode_local(self, code, num_samples, p_x, p_y, p_z, seed=0, first_sample=0):
        if code is not self.code:
            raise ValueError("this circuit was made for another code object")
        return self.logical_error_rates(num_samples, p_x, p_y, p_z, seed=seed, first_sample=first_sample)

    def strata_local(self, code, weights, samples, kinds=(1, 1, 1), seed=0, first_sample=0):
        """logical_error_strata with montecarlo.strata_sharded's local_fn signature."""
        if code is not self.code:
            raise ValueError("this circuit was made for another code object")
        return self.logical_error_strata(weights, samples, kinds=kinds, seed=seed, first_sample=first_sample)


def circuit_for(code, gates):
    """FaultCircuit.for_code(code, gates), cached on the code object by the gate list's contents."""
    gates = _gates(gates)
    cache = code.__dict__.setdefault("_fault_circuits", {})
    key = gates.tobytes()
    if key not in cache:
        cache[key] = FaultCircuit.for_code(code, gates)
    return cache[key]


def idle_gates(n):
    """One IDLE gate per qubit: the circuit whose fault model is the code-capacity model (one independent error per qubit)."""
    return np.array([(GATE_IDLE, q, 0) for q in range(int(n))], dtype=np.int32).reshape(-1, 3)


def encoder_gates(code, state):
    if state not in ('zero', 'plus'):
        raise ValueError("state must be 'zero' or 'plus'")
    return code.encode_zero_gates() if state == 'zero' else code.encode_plus_gates()
