"""
Circuit-level fault Monte-Carlo on the GPU (quantum_css_codes_amd/circuit_noise.py, csrc/gf2_circuit.hip; DESIGN.md "Circuit
faults").  Every comparison is exact: against the code-capacity paths (a circuit of IDLE gates is one independent error per
qubit) and against a forward restatement written here -- faults from the oracle's sampler run over the L locations, NumPy
Pauli-frame propagation gate by gate, syndromes, vec_to_int keys, the code's own table dicts.
"""
import ctypes
import functools

import numpy as np
import pytest

from oracle import c_oracle
from quantum_css_codes_amd import _native, bin_matrix, circuit_noise, css_code, montecarlo
from quantum_css_codes_amd.circuit_noise import FaultCircuit
from quantum_css_codes_amd.css_code import CSSCode

pytestmark = pytest.mark.gpu

H, CNOT, IDLE = 0, 1, 2
STEANE = np.array([[0, 0, 0, 1, 1, 1, 1], [0, 1, 1, 0, 0, 1, 1], [1, 0, 1, 0, 1, 0, 1]])


def dual_pair(rng, n, r1):
    """H1 (r1 x n, full rank) and all but one row of a basis of its dual: a k = 1 CSS pair."""
    while True:
        h1 = rng.integers(0, 2, (r1, n))
        if bin_matrix.rank(h1) == r1:
            break
    null = bin_matrix.nullspace(h1)
    return h1, null[: null.shape[0] - 1]


@functools.lru_cache(maxsize=None)
def make_code(name):
    if name == "steane":
        return CSSCode(STEANE, STEANE)
    if name == "rm15":
        cols = np.arange(1, 16)
        h1 = np.array([(cols >> b) & 1 for b in range(4)])
        return CSSCode(h1, np.vstack([h1] + [h1[a] & h1[b] for a in range(4) for b in range(a + 1, 4)]))
    n, r1, cap = name
    h1, h2 = dual_pair(np.random.default_rng(n + r1), n, r1)
    return CSSCode(h1, h2, max_table_weight=cap)


# ---- the forward restatement ---------------------------------------------------------------------------------------

def sample_faults(total, seed, first, count, p):
    """(f_x, f_z) as L x count bit arrays: the oracle's sampler with n := L."""
    ex, ez = c_oracle.sample_errors(total, seed, first, count, *p)
    return (np.ascontiguousarray(c_oracle.unpack_rows(ex, total, dtype=np.uint8).T),
            np.ascontiguousarray(c_oracle.unpack_rows(ez, total, dtype=np.uint8).T))


def propagate(gates, n, f_x, f_z):
    """Final frames (n x count each): every gate acts, then its locations' faults are XOR-ed in."""
    count = f_x.shape[1]
    e_x = np.zeros((n, count), dtype=np.uint8)
    e_z = np.zeros((n, count), dtype=np.uint8)
    loc = 0
    for kind, a, b in gates.tolist():
        if kind == H:
            e_x[a], e_z[a] = e_z[a].copy(), e_x[a].copy()
        elif kind == CNOT:
            e_x[b] ^= e_x[a]
            e_z[a] ^= e_z[b]
        for q in ((a, b) if kind == CNOT else (a,)):
            e_x[q] ^= f_x[loc]
            e_z[q] ^= f_z[loc]
            loc += 1
    assert loc == f_x.shape[0]
    return e_x, e_z


def keys_of(synd):
    """vec_to_int of every row of a (count, r) bit array (row 0 of the check = most significant bit), as Python ints."""
    count, r = synd.shape
    padded = np.zeros((count, 8 * ((r + 7) // 8)), dtype=np.uint8)
    padded[:, padded.shape[1] - r:] = synd
    packed = np.packbits(padded, axis=1, bitorder="big")
    return [int.from_bytes(row.tobytes(), "big") for row in packed]


def restate(code, gates, seed, first, count, p, mode, chunk=4096):
    """Outcome words, histograms and the five counts of samples [first, first + count), one chunk at a time."""
    n, r_1, r_2 = code.n, code.r_1, code.r_2
    total = len(circuit_noise.fault_locations(gates))
    kwx, kwz = (1 if r_2 <= 63 else 2), (1 if r_1 <= 63 else 2)
    words = np.zeros((count, kwx + kwz + 1), dtype=np.uint64)
    full = mode == 'full'
    hist_z = np.zeros(1 << r_1 if full else r_1 + 1, dtype=np.uint64)
    hist_x = np.zeros(1 << r_2 if full else r_2 + 1, dtype=np.uint64)
    counts = [0, 0, 0, 0, 0]
    z_op, x_op = code.z_operator_matrix()[0], code.x_operator_matrix()[0]
    sides = ((code.parity_check_c2, code._c2_syndromes, z_op, 0, kwx, hist_x, 3, {}),
             (code.parity_check_c1, code._c1_syndromes, x_op, kwx, kwz, hist_z, 4, {}))
    mask = (1 << 64) - 1
    for start in range(0, count, chunk):
        now = min(chunk, count - start)
        frames = propagate(gates, n, *sample_faults(total, seed, first + start, now, p))
        flips = []
        for err, (check, table, op, word, kw, hist, slot, memo) in zip(frames, sides):
            err = err.T.astype(np.int64)                                   # (now, n)
            synd = ((err @ check.T) & 1).astype(np.uint8)
            parity = (err @ op) & 1
            keys = keys_of(synd)
            np.add.at(hist, np.array(keys, dtype=np.int64) if full else synd.sum(axis=1, dtype=np.int64), np.uint64(1))
            flip = np.zeros(now, dtype=np.int64)
            for i, key in enumerate(keys):
                words[start + i, word] = key & mask
                if kw == 2:
                    words[start + i, word + 1] = key >> 64
                if key not in memo:                                        # operator . correction, or None: not in the table
                    memo[key] = (int(np.dot(op, table[key])) & 1) if key in table else None
                if memo[key] is None:
                    counts[slot] += 1                                      # css_code.py:655-657: no match leaves the error as it is
                    flip[i] = parity[i]
                else:
                    flip[i] = parity[i] ^ memo[key]
            words[start:start + now, kwx + kwz] |= (parity.astype(np.uint64) << np.uint64(0 if slot == 3 else 1))
            flips.append(flip)
        counts[0] += int(flips[0].sum())
        counts[1] += int(flips[1].sum())
        counts[2] += int((flips[0] | flips[1]).sum())
    return words, hist_z, hist_x, counts


def assert_matches_restatement(code, gates, seed, first, count, p, mode=None):
    mode = montecarlo.pick_mode(code.r_1, code.r_2, mode)
    words, hist_z, hist_x, counts = restate(code, gates, seed, first, count, p, mode)
    circ = circuit_noise.circuit_for(code, gates)
    assert np.array_equal(circ.outcomes(count, *p, seed=seed, first_sample=first), words)
    got = code.circuit_monte_carlo(gates, count, *p, seed=seed, first_sample=first, mode=mode)
    assert got['mode'] == mode and np.array_equal(got['hist_z'], hist_z) and np.array_equal(got['hist_x'], hist_x)
    assert int(got['hist_z'].sum()) == count == int(got['hist_x'].sum())
    tally = code.circuit_logical_error_rates(gates, count, *p, seed=seed, first_sample=first)
    assert [tally[f] for f in montecarlo.DECODE_FIELDS] == counts and tally['samples'] == count


# ---- 5: a circuit of IDLE gates is the code-capacity model ----------------------------------------------------------------

@pytest.mark.parametrize("name,count", [("steane", 10**6), ("rm15", 10**6), ((47, 23, None), 3 * 10**5), ((63, 31, None), 3 * 10**5),
                                        ((128, 64, 2), 3 * 10**5)])
def test_idle_circuit_is_code_capacity(name, count):
    code = make_code(name)
    gates = [(IDLE, q, 0) for q in range(code.n)]
    for p, seed, first in (((0.01, 0.005, 0.02), 5, 0), ((0.001, 0.001, 0.001), 77, 123456789)):
        got = code.circuit_monte_carlo(gates, count, *p, seed=seed, first_sample=first)
        want = code.monte_carlo(count, *p, seed=seed, first_sample=first)
        assert got['mode'] == want['mode']
        assert np.array_equal(got['hist_z'], want['hist_z']) and np.array_equal(got['hist_x'], want['hist_x'])
        assert code.circuit_logical_error_rates(gates, count, *p, seed=seed, first_sample=first) == \
            code.logical_error_rates(count, *p, seed=seed, first_sample=first)
    if code.r_1 <= 24 and code.r_2 <= 24:                                  # ... and the weight bins where 'full' is the default
        got = code.circuit_monte_carlo(gates, count, 0.02, 0.01, 0.02, seed=1, mode='weight')
        want = code.monte_carlo(count, 0.02, 0.01, 0.02, seed=1, mode='weight')
        assert np.array_equal(got['hist_z'], want['hist_z']) and np.array_equal(got['hist_x'], want['hist_x'])


# ---- 6: the encoders against the forward restatement ------------------------------------------------------------------------
# Samples per case, sized so that the NumPy side stays under about a minute: 2 x 10^5 for the two small codes (L = 21 .. 85),
# 10^5 at 47 and 63 qubits (L about 600 and 1000), 4 x 10^4 at 100 qubits (L about 2500), 2 x 10^4 at 127 (L about 4000).

@pytest.mark.parametrize("state", ["zero", "plus"])
@pytest.mark.parametrize("name,count,p", [("steane", 2 * 10**5, (0.004, 0.003, 0.005)), ("rm15", 2 * 10**5, (0.002, 0.001, 0.003)),
                                          ((47, 23, None), 10**5, (0.0006, 0.0002, 0.0004)),
                                          ((63, 31, None), 10**5, (0.0003, 0.0003, 0.0002)),
                                          ((100, 49, 3), 4 * 10**4, (0.0002, 0.0001, 0.0002)),
                                          ((127, 63, 2), 2 * 10**4, (0.0001, 0.0001, 0.0001))])
def test_encoders_against_the_forward_restatement(name, count, p, state):
    code = make_code(name)
    gates = circuit_noise.encoder_gates(code, state)
    assert_matches_restatement(code, gates, seed=31, first=1000, count=count, p=p)
    # ... and the methods named after the encoders are the same calls
    got = code.encoder_monte_carlo(state, 5000, *p, seed=2)
    want = code.circuit_monte_carlo(gates, 5000, *p, seed=2)
    assert np.array_equal(got['hist_z'], want['hist_z']) and np.array_equal(got['hist_x'], want['hist_x'])
    assert code.encoder_logical_error_rates(state, 5000, *p, seed=2) == code.circuit_logical_error_rates(gates, 5000, *p, seed=2)


def test_steane_location_counts_and_weight_mode():
    code = make_code("steane")
    assert circuit_noise.circuit_for(code, code.encode_zero_gates()).num_locations == 21
    assert circuit_noise.circuit_for(code, code.encode_plus_gates()).num_locations == 26
    assert_matches_restatement(code, code.encode_plus_gates(), seed=8, first=0, count=50000, p=(0.01, 0.02, 0.01), mode='weight')


# ---- 7: segment boundaries, rates, first_sample beyond 2^32 -----------------------------------------------------------------

def padded_encoder(code, total):
    """encode_zero between IDLE gates (input noise in front, memory noise behind) with `total` fault locations in all."""
    gates = code.encode_zero_gates()
    pad = total - len(circuit_noise.fault_locations(gates))
    idle = np.array([(IDLE, q % code.n, 0) for q in range(pad)], dtype=np.int32).reshape(-1, 3)
    front = pad // 2
    return np.concatenate((idle[:front], gates, idle[front:]))


@pytest.mark.parametrize("total", [511, 512, 513, 1024, 1025])
def test_segment_boundaries_and_rates(total):
    code = make_code("steane")
    gates = padded_encoder(code, total)
    assert len(circuit_noise.fault_locations(gates)) == total
    rates = [(0.5 * t, 0.2 * t, 0.3 * t) for t in (0.0, 1e-4, 1e-2, 0.3, 1.0)]
    rates += [(0.01, 0.0, 0.0), (0.0, 0.01, 0.0), (0.0, 0.0, 0.01)]          # one kind only (p_y alone: both components set)
    for k, p in enumerate(rates):
        first = (1 << 32) + 12345 if k % 2 else 77
        assert_matches_restatement(code, gates, seed=total + k, first=first, count=20000, p=p)
    if total == 513:                                                       # p_y alone: every fault sets both components
        words, _, _, _ = restate(code, gates, 3, 0, 2000, (0.0, 0.05, 0.0), 'full')
        assert words.any()


# ---- 8: shards -----------------------------------------------------------------------------------------------------------------

def test_shard_invariance():
    code = make_code((47, 23, None))
    circ = circuit_noise.circuit_for(code, code.encode_plus_gates())
    p, seed, first, count = (0.001, 0.0005, 0.001), 9, (1 << 33) + 5, 200001
    whole_h = circ.monte_carlo(count, *p, seed=seed, first_sample=first)
    whole_d = circ.logical_error_rates(count, *p, seed=seed, first_sample=first)
    hist_z, hist_x, tally = 0, 0, np.zeros(5, dtype=np.int64)
    start = first
    for part in (1, 65537, count - 65538):
        h = circ.monte_carlo(part, *p, seed=seed, first_sample=start)
        d = circ.logical_error_rates(part, *p, seed=seed, first_sample=start)
        hist_z, hist_x = hist_z + h['hist_z'], hist_x + h['hist_x']
        tally += np.array([d[f] for f in montecarlo.DECODE_FIELDS])
        start += part
    assert np.array_equal(hist_z, whole_h['hist_z']) and np.array_equal(hist_x, whole_h['hist_x'])
    assert [int(v) for v in tally] == [whole_d[f] for f in montecarlo.DECODE_FIELDS]
    # no process group: the sharded drivers return what the local call returns
    assert montecarlo.decode_sharded(code, count, *p, seed=seed, first_sample=first, local_fn=circ.decode_local) == whole_d
    sharded = montecarlo.run_sharded(code, count, *p, seed=seed, first_sample=first, local_fn=circ.run_local)
    assert np.array_equal(sharded['hist_z'], whole_h['hist_z']) and np.array_equal(sharded['hist_x'], whole_h['hist_x'])
    assert sharded['mode'] == whole_h['mode'] and sharded['shard'] == (first, count)


def test_outcomes_of_any_rows_are_the_frames():
    # identity(2n) rows on 130 qubits (ldr = 5) and on 256 (ldr = 8): the stored words are the final frames themselves
    rng = np.random.default_rng(4)
    for n, ngates in ((130, 300), (256, 700), (20, 50)):
        gates = np.zeros((ngates, 3), dtype=np.int32)
        for g in range(ngates):
            a, b = rng.choice(n, 2, replace=False)
            gates[g] = (int(rng.integers(0, 3)), a, b)
        ident = np.identity(2 * n, dtype=np.uint8)
        circ = FaultCircuit(gates, n, ident[:, :n], ident[:, n:])
        p, count = (0.004, 0.002, 0.003), 30000
        got = circ.outcomes(count, *p, seed=6, first_sample=10)
        e_x, e_z = propagate(gates, n, *sample_faults(circ.num_locations, 6, 10, count, p))
        want = _native.pack_rows(np.ascontiguousarray(np.concatenate((e_x, e_z)).T))
        assert got.shape == want.shape and np.array_equal(got, want)
        with pytest.raises(ValueError, match="for_code"):
            circ.monte_carlo(10, *p)


# ---- 9: limits -------------------------------------------------------------------------------------------------------------------

def test_limits_are_refused_with_a_message():
    lib, ctx = _native.lib(), _native.default_context()
    steane = make_code("steane")
    # decode beyond 128 qubits: histograms still run
    big = make_code((130, 65, 1))
    gates = big.encode_zero_gates()
    hist = big.circuit_monte_carlo(gates, 20000, 1e-4, 1e-4, 1e-4, seed=1)
    assert hist['mode'] == 'weight' and int(hist['hist_z'].sum()) == 20000 == int(hist['hist_x'].sum())
    with pytest.raises(ValueError, match="n <= 128"):
        big.circuit_logical_error_rates(gates, 10, 1e-4, 1e-4, 1e-4)
    # full histograms beyond 24 checks
    mid = make_code((63, 31, None))
    with pytest.raises(ValueError, match="<= 24"):
        mid.encoder_monte_carlo('zero', 10, 0.01, 0.01, 0.01, mode='full')
    circ = circuit_noise.circuit_for(mid, mid.encode_zero_gates()).device()
    bins = np.zeros(8, dtype=np.uint64)
    assert lib.gf2_mc_circuit_run(ctx.handle, circ.handle, mid.r_1, mid.r_2, 0, 0, 10, 0.01, 0.01, 0.01, _native.HIST_FULL,
                                  bins.ctypes.data, 8, bins.ctypes.data, 8) == _native.GF2_E_ARG
    assert b"r <= 24" in lib.gf2_last_error()
    with pytest.raises(ValueError, match="zero.*plus"):
        steane.encoder_monte_carlo('minus', 10, 0.01, 0.01, 0.01)
    # L and ldr over the caps
    many = FaultCircuit.for_code(steane, np.array([(IDLE, 0, 0)] * ((1 << 20) + 1), dtype=np.int32))
    with pytest.raises(ValueError, match=r"2\^20"):
        many.device()
    with pytest.raises(ValueError, match="512"):
        FaultCircuit([(IDLE, 0, 0)], 7, np.zeros((513, 7), int), np.zeros((513, 7), int))
    out, dummy = ctypes.c_void_p(), np.zeros(64, dtype="<u8")
    assert lib.gf2_circuit_create(ctx.handle, dummy.ctypes.data, (1 << 20) + 1, 1, ctypes.byref(out)) == _native.GF2_E_ARG
    assert b"2^20" in lib.gf2_last_error() and out.value is None
    assert lib.gf2_circuit_create(ctx.handle, dummy.ctypes.data, 2, 9, ctypes.byref(out)) == _native.GF2_E_ARG
    assert b"ldr <= 8" in lib.gf2_last_error() and out.value is None
    # tables: a null array with entries > 0, a key twice, effects of the wrong width
    small = circuit_noise.circuit_for(steane, steane.encode_zero_gates())
    keys1, flips1, keys2, flips2 = small._tables()
    args = (0, 0, 100, 0.01, 0.01, 0.01)
    with pytest.raises(_native.GF2Error, match="null array with entries > 0"):
        ctx.mc_circuit_decode(small.device(), 3, keys1, None, 3, keys2, flips2, *args)
    twice = np.concatenate((keys2, keys2[:1]))
    with pytest.raises(_native.GF2Error, match="twice"):
        ctx.mc_circuit_decode(small.device(), 3, keys1, flips1, 3, twice, np.concatenate((flips2, flips2[:1])), *args)
    with pytest.raises(_native.GF2Error, match="need effects of 5 words"):
        ctx.mc_circuit_decode(small.device(), 70, keys1, flips1, 70, keys2, flips2, *args)
    with pytest.raises(_native.GF2Error, match="beyond the keys"):
        ctx.mc_circuit_run(small.device(), 2, 3, 0, 0, 100, 0.01, 0.01, 0.01, _native.HIST_WEIGHT)
    # an empty table is a table: every non-trivial syndrome is uncorrectable, and nothing is corrected
    none = np.zeros((0, 1), dtype=np.uint64)
    counts = ctx.mc_circuit_decode(small.device(), 3, none, None, 3, none, None, 0, 0, 5000, 0.01, 0.01, 0.01)
    assert int(counts[3]) == 5000 and int(counts[4]) == 5000
    # the conjugation entry points keep refusing IDLE
    with pytest.raises(ValueError):
        css_code.transform_stabilisers(steane.stabiliser_matrix(), np.array([(H, 0, 0), (IDLE, 1, 0)], dtype=np.int32))
