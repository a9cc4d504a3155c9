"""
Calderbank-Shor-Steane codes: the numeric core of the reference's css_code.py with every GF(2)
product and elimination running on the MI355X (libgf2hip.so).

Drop-in surface (same names, arguments, mutation and exception behaviour):
    CSSCode(parity_check_c1, parity_check_c2)         css_code.py:32-75
      .n .k .t .r_1 .r_2 .parity_check_c1 .parity_check_c2 ._c1_syndromes ._c2_syndromes
      .z_operator_matrix() .x_operator_matrix()       css_code.py:124-136, 149-161
      .stabilisers() .x_operators() .z_operators() .y_operators()   css_code.py:98-172
      .is_transversal(gate_name)                      css_code.py:174-201
    syndrome_table, normalize_parity_check, swap_columns, codes_equal, is_doubly_even,
    pauli_term_for_row                                css_code.py:715-735, 783-850

    CSSCode.noisy_encode_zero / noisy_encode_plus    css_code.py:203-312   (gate arrays, see below)
    transform_stabilisers, conjugate_h_with_check_mat, conjugate_cnot_with_check_mat   css_code.py:737-781

The two encoders are returned as gate arrays -- rows (kind, a, b), GATE_H on qubit a or GATE_CNOT control a target b, in
the reference's instruction order -- which is what transform_stabilisers takes here [SURVEY.md 8f item 3].  The other
emitters (encode_zero / encode_plus, apply_gate, error_correct, measure, noisy_measure, quil_classical_correct /
quil_classical_detect; css_code.py:314-713) build pyQuil-free instruction tuples (quil.py, css_emit.py) [8f item 4].
pyQuil is not required: Pauli operators are returned as text labels ("X0*X3*X4*X5") unless pyQuil is
importable, in which case PauliTerm objects are returned as in the reference.

Build-defined additions (8f item 1): CSSCode(..., max_table_weight=), CSSCode.syndromes,
CSSCode.monte_carlo, CSSCode.logical_error_rates, syndrome_batch.
"""
import itertools

import numpy as np

from . import _native
from . import bin_matrix
from . import css_emit
from .css_emit import apply_transversally, quil_classical_correct, quil_classical_detect  # noqa: F401  (module-level in the reference)
from .errors import InvalidCodeError
from .qecc import QECC

try:                                                # optional, as in SURVEY.md 7.3 item 7
    from pyquil.paulis import ID as _ID, sX as _sX, sY as _sY, sZ as _sZ
    _HAVE_PYQUIL = True
except Exception:                                   # pragma: no cover - pyquil is absent in this image
    _HAVE_PYQUIL = False


GATE_H, GATE_CNOT = 0, 1                            # kinds of a gate-array row (kind, a, b)
GATE_IDLE = 2                                       # no action on qubit a, one fault location: circuit_noise only


class CSSCode(QECC):
    """
    A CSS code defined by two binary linear codes C_1, C_2 with the dual of C_2 inside C_1, given by
    their parity check matrices.  Measured in the X basis a codeword is a codeword of C_1, in the Z
    basis a codeword of C_2 (the reference's convention, css_code.py:22-31).
    """

    def __init__(self, parity_check_c1, parity_check_c2, max_table_weight=None):
        parity_check_c1 = np.asarray(parity_check_c1)
        parity_check_c2 = np.asarray(parity_check_c2)
        r_1, n_1 = parity_check_c1.shape
        r_2, n_2 = parity_check_c2.shape
        if n_1 != n_2:
            raise ValueError("C_1 and C_2 must have the same code word length")

        # css_code.py:39-44: entries must be 0 or 1 (tested while the rows are packed: one pass over each 64 MiB array at n = 4096
        # instead of copy + np.mod + np.array_equal); from here to the end of the normalisations the matrices stay packed
        p_1, binary = _native.pack_rows_binary(parity_check_c1)
        if not binary:
            raise ValueError("C_1 parity check matrix must be binary")
        p_2, binary = _native.pack_rows_binary(parity_check_c2)
        if not binary:
            raise ValueError("C_2 parity check matrix must be binary")

        ctx = _native.default_context()
        # css_code.py:47-49 -- H1 . H2^T must vanish over GF(2)
        product = ctx.matmul_abt(p_1, r_1, p_2, r_2, n_1)
        if np.any(product):
            raise ValueError("C_2 dual code must be a subspace of C_1")

        # css_code.py:51-61 -- standard forms H1 = [I A1 A2], H2 = [D I E]; each normalisation's qubit
        # swaps are applied to the other matrix as well.
        for i, j in _normalize_packed(ctx, p_1, r_1, n_1, 0):
            if r_2 and i != j:
                ctx.swap_columns(p_2, r_2, n_1, i, j)
        for i, j in _normalize_packed(ctx, p_2, r_2, n_1, r_1):
            if r_1 and i != j:
                ctx.swap_columns(p_1, r_1, n_1, i, j)
        h_1 = _native.unpack_rows(p_1[:r_1], n_1, dtype='int')
        h_2 = _native.unpack_rows(p_2[:r_2], n_1, dtype='int')

        self._n = n_1
        self._k = n_1 - r_1 - r_2
        self.r_1 = r_1
        self.r_2 = r_2
        self.parity_check_c1 = h_1
        self.parity_check_c2 = h_2
        t_1, self._c1_syndromes = syndrome_table(h_1, max_weight=max_table_weight, _packed=p_1[:r_1])
        t_2, self._c2_syndromes = syndrome_table(h_2, max_weight=max_table_weight, _packed=p_2[:r_2])
        self._t = min(t_1, t_2)
        self._transversal_gates = self._determine_transversal_gates(h_1, h_2)
        self._checks = None

        if self.k != 1:
            raise InvalidCodeError("currently only supports CSS codes for a single logical qubit")

    @property
    def n(self):
        """Number of physical qubits per code block."""
        return self._n

    @property
    def k(self):
        """Number of logical qubits per code block."""
        return self._k

    @property
    def t(self):
        """Maximum number of errors per code block that can be corrected."""
        return self._t

    # -- operators ----------------------------------------------------------------------------------------
    def stabilisers(self):
        """Generators of the stabiliser group: the rows of H1 as X-type operators, then the rows of H2
        as Z-type operators (css_code.py:98-111)."""
        zeros = np.zeros(self.n, dtype='int')
        x_type = (pauli_term_for_row(self.parity_check_c1[i, :], zeros) for i in range(self.r_1))
        z_type = (pauli_term_for_row(zeros, self.parity_check_c2[i, :]) for i in range(self.r_2))
        return list(itertools.chain(x_type, z_type))

    def stabiliser_matrix(self):
        """[build-defined]  The same generators as a (r_1 + r_2) x 2n check matrix [X part | Z part]."""
        out = np.zeros((self.r_1 + self.r_2, 2 * self.n), dtype='int')
        out[:self.r_1, :self.n] = self.parity_check_c1
        out[self.r_1:, self.n:] = self.parity_check_c2
        return out

    def z_operator_matrix(self):
        """Check matrix of the logical Z operators, the row [A2^T 0 I] (css_code.py:124-136)."""
        n, r_1, r_2, k = self.n, self.r_1, self.r_2, self.k
        check_mat = np.zeros((k, n), dtype='int')
        check_mat[:, 0:r_1] = np.transpose(self.parity_check_c1[:, (r_1 + r_2):n])
        check_mat[:, (r_1 + r_2):n] = np.identity(k)
        return check_mat

    def x_operator_matrix(self):
        """Check matrix of the logical X operators, the row [0 E^T I] (css_code.py:149-161)."""
        n, r_1, r_2, k = self.n, self.r_1, self.r_2, self.k
        check_mat = np.zeros((k, n), dtype='int')
        check_mat[:, r_1:(r_1 + r_2)] = np.transpose(self.parity_check_c2[:, (r_1 + r_2):n])
        check_mat[:, (r_1 + r_2):n] = np.identity(k)
        return check_mat

    def z_operators(self):
        """css_code.py:113-122."""
        z_matrix = self.z_operator_matrix()
        zeros = np.zeros_like(z_matrix, dtype='int')
        return [pauli_term_for_row(zeros[i, :], z_matrix[i, :]) for i in range(self.k)]

    def x_operators(self):
        """css_code.py:138-147."""
        x_matrix = self.x_operator_matrix()
        zeros = np.zeros_like(x_matrix, dtype='int')
        return [pauli_term_for_row(x_matrix[i, :], zeros[i, :]) for i in range(self.k)]

    def y_operators(self):
        """Y = iXZ (css_code.py:163-172): qubits carrying both X and Z carry Y."""
        x_matrix, z_matrix = self.x_operator_matrix(), self.z_operator_matrix()
        return [pauli_term_for_row(x_matrix[i, :], z_matrix[i, :]) for i in range(self.k)]

    def is_transversal(self, gate_name):
        """Whether the gate is known to be fault tolerant when applied transversally (css_code.py:174-180)."""
        return gate_name in self._transversal_gates

    def _determine_transversal_gates(self, parity_check_c1, parity_check_c2):
        # css_code.py:182-201 (Steane 1998, Lemmas 2 and 3)
        names = ['I', 'CNOT']
        if codes_equal(parity_check_c1, parity_check_c2):
            names += ['H', 'CZ']
            if is_doubly_even(parity_check_c1):
                names.append('S')
        return frozenset(names)

    # -- build-defined: batched syndromes and Monte-Carlo ---------------------------------------------------
    def encode_zero_gates(self, qubits=None):
        """
        The instruction sequence of noisy_encode_zero (css_code.py:203-259) as an (g, 3) int32 array: H on the first
        r_1 qubits, then CNOT(i, j) for every 1 of parity_check_c1[i, j] with j >= r_1, rows in order, columns in order.
        """
        n, r_1 = self.n, self.r_1
        qubits = np.arange(n, dtype=np.int32) if qubits is None else np.asarray(list(qubits), dtype=np.int32)
        ctrl, targ = np.nonzero(self.parity_check_c1[:, r_1:] == 1)          # row-major: i ascending, then j
        gates = np.zeros((r_1 + len(ctrl), 3), dtype=np.int32)
        gates[:r_1, 0], gates[:r_1, 1] = GATE_H, qubits[:r_1]
        gates[r_1:, 0], gates[r_1:, 1], gates[r_1:, 2] = GATE_CNOT, qubits[ctrl], qubits[targ + r_1]
        return gates

    def encode_plus_gates(self, qubits=None):
        """
        The instruction sequence of noisy_encode_plus (css_code.py:261-312): H on the first r_1 and on the last
        n - r_1 - r_2 qubits, CNOT(j, i) for every 1 of parity_check_c2[i - r_1, j] with j >= r_1 + r_2, then the CNOTs of
        noisy_encode_zero.
        """
        n, r_1, r_2 = self.n, self.r_1, self.r_2
        qubits = np.arange(n, dtype=np.int32) if qubits is None else np.asarray(list(qubits), dtype=np.int32)
        had = np.concatenate((qubits[:r_1], qubits[r_1 + r_2:]))
        rows, cols = np.nonzero(self.parity_check_c2[:, r_1 + r_2:] == 1)
        ctrl, targ = np.nonzero(self.parity_check_c1[:, r_1:] == 1)
        gates = np.zeros((len(had) + len(rows) + len(ctrl), 3), dtype=np.int32)
        a, b = len(had), len(had) + len(rows)
        gates[:a, 0], gates[:a, 1] = GATE_H, had
        gates[a:b, 0], gates[a:b, 1], gates[a:b, 2] = GATE_CNOT, qubits[cols + r_1 + r_2], qubits[rows + r_1]
        gates[b:, 0], gates[b:, 1], gates[b:, 2] = GATE_CNOT, qubits[ctrl], qubits[targ + r_1]
        return gates

    def noisy_encode_zero(self, qubits):
        """css_code.py:203-259 as a gate array (see encode_zero_gates); qubits must be integers."""
        return self.encode_zero_gates(qubits)

    def noisy_encode_plus(self, qubits):
        """css_code.py:261-312 as a gate array (see encode_plus_gates); qubits must be integers."""
        return self.encode_plus_gates(qubits)

    # -- program emission (css_code.py:314-646), pyQuil-free: quantum_css_codes_amd/css_emit.py ------------------------------
    def noisy_encode_zero_program(self, qubits):
        """noisy_encode_zero (css_code.py:203-259) as instruction tuples on `qubits` (integers or placeholders)."""
        return css_emit.noisy_encode_zero_program(self, qubits)

    def noisy_encode_plus_program(self, qubits):
        """noisy_encode_plus (css_code.py:261-312) as instruction tuples."""
        return css_emit.noisy_encode_plus_program(self, qubits)

    def encode_zero(self, prog, block, ancilla, scratch):
        css_emit.encode_zero(self, prog, block, ancilla, scratch)

    def encode_plus(self, prog, block, ancilla, scratch):
        css_emit.encode_plus(self, prog, block, ancilla, scratch)

    def apply_gate(self, prog, gate_name, *blocks):
        css_emit.apply_gate(self, prog, gate_name, *blocks)

    def error_correct(self, prog, data, ancilla_1, ancilla_2, scratch):
        css_emit.error_correct(self, prog, data, ancilla_1, ancilla_2, scratch)

    def _error_detect_x(self, prog, data, ancilla, outcome, scratch, include_operators):
        css_emit.error_detect_x(self, prog, data, ancilla, outcome, scratch, include_operators)

    def _error_detect_z(self, prog, data, ancilla, outcome, scratch, include_operators):
        css_emit.error_detect_z(self, prog, data, ancilla, outcome, scratch, include_operators)

    def measure(self, prog, data, index, outcome, ancilla_1, ancilla_2, scratch, scratch_int):
        return css_emit.measure(self, prog, data, index, outcome, ancilla_1, ancilla_2, scratch, scratch_int)

    def noisy_measure(self, prog, data, index, outcome, ancilla_1, ancilla_2, scratch):
        css_emit.noisy_measure(self, prog, data, index, outcome, ancilla_1, ancilla_2, scratch)

    @property
    def encode_scratch_size(self):
        return css_emit.encode_scratch_size(self)

    @property
    def error_correct_scratch_size(self):
        return css_emit.error_correct_scratch_size(self)

    @property
    def measure_scratch_size(self):
        return css_emit.measure_scratch_size(self)

    def _device_checks(self):
        if self._checks is None:
            ctx = _native.default_context()
            self._checks = (ctx.check_create(_native.pack_rows(self.parity_check_c1), self.r_1, self.n),
                            ctx.check_create(_native.pack_rows(self.parity_check_c2), self.r_2, self.n))
        return self._checks

    def syndromes(self, x_errors, z_errors):
        """[build-defined, x2]  Syndromes of B errors at once.  x_errors and z_errors are B x n 0/1
        arrays.  X errors are detected by parity_check_c2 and Z errors by parity_check_c1
        (css_code.py:457-470).  Returns (s_x: B x r_2, s_z: B x r_1)."""
        return (syndrome_batch(self.parity_check_c2, x_errors), syndrome_batch(self.parity_check_c1, z_errors))

    def monte_carlo(self, num_samples, p_x, p_y, p_z, seed=0, first_sample=0, mode=None):
        """[build-defined, x3]  Histograms of the syndromes of `num_samples` independent Pauli errors
        (X, Y, Z with probability p_x, p_y, p_z per qubit); sample i of the global stream is a pure
        function of (seed, i).  mode 'full': bins indexed by bin_matrix.vec_to_int(syndrome), needs
        r_1, r_2 <= 24; mode 'weight': bins indexed by syndrome weight.  Default: 'full' when possible.
        Returns {'hist_z': from parity_check_c1 . e_z, 'hist_x': from parity_check_c2 . e_x, 'mode'}."""
        from . import montecarlo
        return montecarlo.run_local(self, num_samples, p_x, p_y, p_z, seed=seed, first_sample=first_sample,
                                    mode=mode)


    def logical_error_rates(self, num_samples, p_x, p_y, p_z, seed=0, first_sample=0):
        """[build-defined, SURVEY.md 8f item 1]  Monte-Carlo of the classical side of error correction followed by
        a logical measurement: for every sampled error the syndrome is looked up in this code's tables
        (quil_classical_correct, css_code.py:649-685: the correction is applied when the syndrome is in the table,
        otherwise the error stays), and the logical Z (X) measurement flips iff z_operator . residual_x
        (x_operator . residual_z) is odd (noisy_measure, css_code.py:640-646).  Codes of at most 128 qubits (dense tables of
        2^r words for n <= 63 and r_1, r_2 <= 20, hash tables on the device beyond).  Returns counts: logical_x, logical_z, logical_any, uncorrectable_x, uncorrectable_z, samples."""
        from . import montecarlo
        return montecarlo.decode_local(self, num_samples, p_x, p_y, p_z, seed=seed, first_sample=first_sample)

    def logical_error_strata(self, weights, samples, kinds=(1, 1, 1), seed=0, first_sample=0):
        """[build-defined, DESIGN.md "Strata"]  `logical_error_rates` stratified by error weight: stratum s draws `samples`
        (one number, or one per stratum) errors of exactly weights[s] qubits -- a uniformly random subset, kinds X : Y : Z =
        kinds -- and tallies the same five counts.  Returns a montecarlo.Strata; its rate(p_t) combines the strata with binomial
        weights in double precision, for every p_t at once and with no floor at 2^-32 (logical_error_rates returns 0 flips for
        the Steane code at p_t = 1e-6; rate(1e-6) gives 1.63e-11)."""
        from . import montecarlo
        return montecarlo.strata_local(self, weights, samples, kinds=kinds, seed=seed, first_sample=first_sample)

    # -- build-defined: faults inside a circuit (circuit_noise.py) ----------------------------------------------
    def circuit_monte_carlo(self, gates, num_samples, p_x, p_y, p_z, seed=0, first_sample=0, mode=None):
        """[build-defined]  `monte_carlo` for the final Pauli frame of a noisy circuit: every operand of every gate of `gates`
        (rows (kind, a, b): GATE_H, GATE_CNOT, GATE_IDLE) suffers X, Y, Z with probability p_x, p_y, p_z, independently; the
        faults propagate through the gates that follow.  Same modes and the same dict as `monte_carlo`."""
        from . import circuit_noise
        return circuit_noise.circuit_for(self, gates).monte_carlo(num_samples, p_x, p_y, p_z, seed=seed,
                                                                  first_sample=first_sample, mode=mode)

    def circuit_logical_error_rates(self, gates, num_samples, p_x, p_y, p_z, seed=0, first_sample=0):
        """[build-defined]  `logical_error_rates` for the final Pauli frame of a noisy circuit (see circuit_monte_carlo):
        the frame's syndromes are looked up in this code's tables and the logical flips tallied by the same rule.  n <= 128."""
        from . import circuit_noise
        return circuit_noise.circuit_for(self, gates).logical_error_rates(num_samples, p_x, p_y, p_z, seed=seed,
                                                                          first_sample=first_sample)

    def encoder_monte_carlo(self, state, num_samples, p_x, p_y, p_z, seed=0, first_sample=0, mode=None):
        """[build-defined]  circuit_monte_carlo of this code's own encoder: noisy_encode_zero (state 'zero',
        css_code.py:203-259) or noisy_encode_plus ('plus', css_code.py:261-312) -- the syndrome statistics of a freshly
        encoded block whose preparation "is not fault tolerant"."""
        from . import circuit_noise
        return self.circuit_monte_carlo(circuit_noise.encoder_gates(self, state), num_samples, p_x, p_y, p_z, seed=seed,
                                        first_sample=first_sample, mode=mode)

    def encoder_logical_error_rates(self, state, num_samples, p_x, p_y, p_z, seed=0, first_sample=0):
        """[build-defined]  circuit_logical_error_rates of this code's own encoder.  After 'zero' only logical_x (a flipped
        logical Z measurement) is physical, after 'plus' only logical_z; both are reported as statistics of the frame."""
        from . import circuit_noise
        return self.circuit_logical_error_rates(circuit_noise.encoder_gates(self, state), num_samples, p_x, p_y, p_z, seed=seed,
                                                first_sample=first_sample)

    def circuit_logical_error_strata(self, gates, weights, samples, kinds=(1, 1, 1), seed=0, first_sample=0):
        """[build-defined]  `logical_error_strata` over the fault locations of a noisy circuit (see circuit_monte_carlo): exactly
        weights[s] <= 16 faults per sample; rate(p_t) of the result is per fault location."""
        from . import circuit_noise
        return circuit_noise.circuit_for(self, gates).logical_error_strata(weights, samples, kinds=kinds, seed=seed,
                                                                           first_sample=first_sample)

    def encoder_logical_error_strata(self, state, weights, samples, kinds=(1, 1, 1), seed=0, first_sample=0):
        """[build-defined]  circuit_logical_error_strata of this code's own encoder ('zero' or 'plus')."""
        from . import circuit_noise
        return self.circuit_logical_error_strata(circuit_noise.encoder_gates(self, state), weights, samples, kinds=kinds, seed=seed,
                                                 first_sample=first_sample)

    # -- build-defined: exact strata (DESIGN.md "Exact strata") ---------------------------------------------------
    def logical_error_strata_exact(self, weights, **options):
        """[build-defined]  The strata of `logical_error_strata` counted instead of sampled: every error of exactly weights[s] <= 8
        qubits with every assignment of X, Y, Z, through the circuit of n IDLE gates (whose strata are this code's).  Returns a
        montecarlo.ExactStrata: exact f_w for every kind ratio, rate(p_t) without statistical error.  Options as
        FaultCircuit.enumerate_strata's."""
        from . import circuit_noise
        return self.circuit_logical_error_strata_exact(circuit_noise.idle_gates(self.n), weights, **options)

    def circuit_logical_error_strata_exact(self, gates, weights, **options):
        """[build-defined]  Every configuration of exactly weights[s] <= 8 faults among the locations of a noisy circuit (see
        circuit_monte_carlo), counted per kind composition: FaultCircuit.enumerate_strata."""
        from . import circuit_noise
        return circuit_noise.circuit_for(self, gates).enumerate_strata(weights, **options)

    def encoder_logical_error_strata_exact(self, state, weights, **options):
        """[build-defined]  circuit_logical_error_strata_exact of this code's own encoder ('zero' or 'plus')."""
        from . import circuit_noise
        return self.circuit_logical_error_strata_exact(circuit_noise.encoder_gates(self, state), weights, **options)

    # -- build-defined: the error-correction cycle under faults (ec_noise.py; DESIGN.md "Error-correction cycle") ---------
    def error_correct_gates(self, rounds=1, idle_data=False):
        """[build-defined]  The gate list (H, CNOT, IDLE, RESET on 3n qubits: data, ancilla_1, ancilla_2) and the timed outcome rows
        of `rounds` rounds of `error_correct` (css_code.py:436-470) with one attempt per ancilla preparation: an ec_noise.ECGates."""
        from . import ec_noise
        return ec_noise.error_correct_gates(self, rounds, idle_data)

    def error_correct_logical_error_rates(self, num_samples, p_x, p_y, p_z, rounds=1, seed=0, first_sample=0, idle_data=False):
        """[build-defined]  The logical error rate per cycle of `rounds` rounds of `error_correct` when every fault location of the
        gadget fails independently: a dict of ec_noise.EC_FIELDS (counts; all but 'accepted' among accepted samples) plus
        'samples'.  Repeat-until-success is post-selection on the verifications (ec_noise's docstring); counts of sample ranges
        add, so sharding by first_sample needs no collective of its own."""
        from . import ec_noise
        return ec_noise.circuit_for(self, rounds, idle_data).logical_error_rates(num_samples, p_x, p_y, p_z, seed=seed,
                                                                                 first_sample=first_sample)

    def error_correct_strata_exact(self, weights, rounds=1, idle_data=False, **options):
        """The exact strata `weights` of the cycle (ec_noise.ECCircuit.enumerate_strata; DESIGN.md "Exact strata of the cycle"): a
        montecarlo.PostSelectedStrata, whose series() gives the Taylor coefficients of the logical error rate per cycle."""
        from . import ec_noise
        return ec_noise.circuit_for(self, rounds, idle_data).enumerate_strata(weights, **options)

    def error_correct_malignant_faults(self, weight, rounds=1, idle_data=False, **options):
        """The fault sets of exactly `weight` faults of the cycle that are accepted and, by default, flip the logical state, listed
        (ec_noise.ECCircuit.malignant_faults; DESIGN.md "Malignant fault sets of the cycle"): a montecarlo.FaultList."""
        from . import ec_noise
        return ec_noise.circuit_for(self, rounds, idle_data).malignant_faults(weight, **options)

    def error_correct_strata(self, weights, samples, rounds=1, idle_data=False, **options):
        """Sampled strata `weights` of the cycle, samples[s] stratified samples each (ec_noise.ECCircuit.strata; DESIGN.md "Sampled
        strata of the cycle"): a montecarlo.SampledPostSelectedStrata.  error_correct_strata_exact(...).merged(it) combines them
        with the exact strata into a rate with a standard error and rigorous bounds."""
        from . import ec_noise
        return ec_noise.circuit_for(self, rounds, idle_data).strata(weights, samples, **options)

    def error_correct_single_faults(self, rounds=1):
        """[build-defined]  The census of every single fault of the cycle, no GPU needed: ECCircuit.single_faults."""
        from . import ec_noise
        return ec_noise.circuit_for(self, rounds).single_faults()

    def error_correct_gate_strata_exact(self, weights, rounds=1, idle_data=False, **options):
        """The exact strata `weights` of the cycle under gate-level faults, a CNOT failing as one event with one of the 15 two-qubit
        Paulis (ec_noise.ECCircuit.enumerate_gate_strata): a montecarlo.GateStrata, whose
        series(('depolarising', 1), 'logical_any') gives the Taylor coefficients of the logical error rate per cycle."""
        from . import ec_noise
        return ec_noise.circuit_for(self, rounds, idle_data).enumerate_gate_strata(weights, **options)

    def error_correct_gate_strata(self, strata, samples, rounds=1, idle_data=False, **options):
        """Sampled strata of the cycle under gate-level faults: strata[s] = (a, b), samples[s] stratified samples of exactly a faulty
        one-operand gates and b faulty CNOTs each (ec_noise.ECCircuit.gate_strata; DESIGN.md section 5e "Sampled strata under
        gate-level faults"): a montecarlo.SampledGateStrata.  error_correct_gate_strata_exact(...).merged(it) combines them with the
        exact strata into a rate with a standard error and rigorous bounds."""
        from . import ec_noise
        return ec_noise.circuit_for(self, rounds, idle_data).gate_strata(strata, samples, **options)

    def error_correct_gate_error_rates(self, num_samples, p1, p2, rounds=1, idle_data=False, **options):
        """The direct Monte-Carlo of the cycle under gate-level faults: every one-operand gate fails with probability p1, every CNOT
        as one event with probability p2, no truncation in the number of faulty gates (ec_noise.ECCircuit.gate_error_rates; DESIGN.md
        section 5e "Direct Monte-Carlo under gate-level faults"): a dict of ec_noise.EC_FIELDS plus 'samples'."""
        from . import ec_noise
        return ec_noise.circuit_for(self, rounds, idle_data).gate_error_rates(num_samples, p1, p2, **options)

    def error_correct_malignant_gate_faults(self, weight, rounds=1, idle_data=False, **options):
        """The sets of exactly `weight` faulty gates of the cycle that are accepted and, by default, flip the logical state, listed
        (ec_noise.ECCircuit.malignant_gate_faults; DESIGN.md section 5e "Malignant fault sets under gate-level faults"): a
        montecarlo.GateFaultList for one CNOT count b, a montecarlo.GateFaultLists over every b by default."""
        from . import ec_noise
        return ec_noise.circuit_for(self, rounds, idle_data).malignant_gate_faults(weight, **options)

    def error_correct_gate_single_faults(self, rounds=1):
        """[build-defined]  The census of every single gate fault of the cycle, no GPU needed: ECCircuit.gate_single_faults."""
        from . import ec_noise
        return ec_noise.circuit_for(self, rounds).gate_single_faults()

    # -- build-defined: the rewritten program's measured bit under faults (ft_noise.py; DESIGN.md "Logical measurement") ---------
    def logical_program_error_rates(self, ops, num_samples, p_x, p_y, p_z, seed=0, first_sample=0):
        """[build-defined]  How often the bit measured by ftqc.rewrite_program of `ops; MEASURE` (ops: logical 'I', 'X', 'Y', 'Z' on
        one qubit) is wrong when every fault location of the rewritten program fails independently: a dict of ft_noise.FT_FIELDS
        (counts; all but 'accepted' among accepted samples) plus 'samples'.  ft_noise.raw_program_error_rate is the bare program's
        side of the comparison."""
        from . import ft_noise
        return ft_noise.program_for(self, ops).measurement_error_rates(num_samples, p_x, p_y, p_z, seed=seed, first_sample=first_sample)

    def logical_program_strata_exact(self, ops, weights, **options):
        """The exact strata `weights` of the rewritten program `ops; MEASURE` (ft_noise.FTProgram.enumerate_strata; DESIGN.md "Exact
        strata of the measurement"): a montecarlo.PostSelectedStrata, whose series((k_x, k_y, k_z), 'wrong') gives the Taylor
        coefficients of the probability that the measured bit is wrong."""
        from . import ft_noise
        return ft_noise.program_for(self, ops).enumerate_strata(weights, **options)

    def logical_program_malignant_faults(self, ops, weight, **options):
        """The fault sets of exactly `weight` faults of the rewritten program `ops; MEASURE` that are accepted and, by default, make
        the measured bit wrong, listed (ft_noise.FTProgram.malignant_faults; DESIGN.md "Malignant fault sets of the measurement"):
        a montecarlo.FaultList."""
        from . import ft_noise
        return ft_noise.program_for(self, ops).malignant_faults(weight, **options)

    def logical_program_strata(self, ops, weights, samples, **options):
        """Sampled strata `weights` of the rewritten program `ops; MEASURE`, samples[s] stratified samples each
        (ft_noise.FTProgram.strata; DESIGN.md "Sampled strata of the measurement"): a montecarlo.SampledPostSelectedStrata, to be
        merged with logical_program_strata_exact's."""
        from . import ft_noise
        return ft_noise.program_for(self, ops).strata(weights, samples, **options)

    def logical_program_single_faults(self, ops):
        """[build-defined]  The census of every single fault of the rewritten program, no GPU needed: FTProgram.single_faults."""
        from . import ft_noise
        return ft_noise.program_for(self, ops).single_faults()

    def logical_program_gate_strata_exact(self, ops, weights, **options):
        """The exact strata `weights` of the rewritten program `ops; MEASURE` under gate-level faults
        (ft_noise.FTProgram.enumerate_gate_strata): a montecarlo.GateStrata, whose
        series(('depolarising', 1), 'wrong') gives the Taylor coefficients of the probability that the measured bit is wrong."""
        from . import ft_noise
        return ft_noise.program_for(self, ops).enumerate_gate_strata(weights, **options)

    def logical_program_gate_strata(self, ops, strata, samples, **options):
        """Sampled strata (a, b) of the rewritten program `ops; MEASURE` under gate-level faults, samples[s] stratified samples each
        (ft_noise.FTProgram.gate_strata; DESIGN.md section 5e "Sampled strata under gate-level faults"): a
        montecarlo.SampledGateStrata, to be merged with logical_program_gate_strata_exact's."""
        from . import ft_noise
        return ft_noise.program_for(self, ops).gate_strata(strata, samples, **options)

    def logical_program_gate_error_rates(self, ops, num_samples, p1, p2, **options):
        """The direct Monte-Carlo of the rewritten program `ops; MEASURE` under gate-level faults, every gate failing on its own
        (ft_noise.FTProgram.gate_error_rates; DESIGN.md section 5e "Direct Monte-Carlo under gate-level faults"): a dict of
        ft_noise.FT_FIELDS plus 'samples'; wrong / accepted estimates the probability that the measured bit is wrong."""
        from . import ft_noise
        return ft_noise.program_for(self, ops).gate_error_rates(num_samples, p1, p2, **options)

    def logical_program_malignant_gate_faults(self, ops, weight, **options):
        """The sets of exactly `weight` faulty gates of the rewritten program `ops; MEASURE` that are accepted and, by default, make
        the measured bit wrong, listed (ft_noise.FTProgram.malignant_gate_faults; DESIGN.md section 5e "Malignant fault sets under
        gate-level faults"): a montecarlo.GateFaultList for one CNOT count b, a montecarlo.GateFaultLists over every b by default."""
        from . import ft_noise
        return ft_noise.program_for(self, ops).malignant_gate_faults(weight, **options)

    def logical_program_gate_single_faults(self, ops):
        """[build-defined]  The census of every single gate fault of the rewritten program, no GPU needed:
        FTProgram.gate_single_faults."""
        from . import ft_noise
        return ft_noise.program_for(self, ops).gate_single_faults()

    # -- build-defined: both gadgets at any length, block by block (stream_noise.py; DESIGN.md "Streamed gadgets") ---------------
    def error_correct_streamed_error_rates(self, num_samples, p_x, p_y, p_z, rounds, seed=0, first_sample=0, idle_data=False):
        """[build-defined]  error_correct_logical_error_rates for any number of rounds (L = rounds L_b <= 2^20 locations): the same
        samples, the same tally and the same dict, computed block by block (stream_noise.StreamedGadget.cycle), so time and memory
        are linear in `rounds`.  Acceptance falls like exp(-c p rounds): long runs are for p <~ 1e-4."""
        from . import stream_noise
        gadget = stream_noise.stream_for(self, "cycle", (int(rounds), bool(idle_data)))
        return gadget.error_rates(num_samples, p_x, p_y, p_z, seed=seed, first_sample=first_sample)

    def logical_program_streamed_error_rates(self, ops, num_samples, p_x, p_y, p_z, seed=0, first_sample=0):
        """[build-defined]  logical_program_error_rates for any number of logical gates and trials, likewise
        (stream_noise.StreamedGadget.program)."""
        from . import ft_noise, stream_noise
        gadget = stream_noise.stream_for(self, "program", ft_noise.check_ops(ops))
        return gadget.error_rates(num_samples, p_x, p_y, p_z, seed=seed, first_sample=first_sample)

    def logical_circuit_error_rates(self, instructions, num_samples, p_x, p_y, p_z, seed=0, first_sample=0, records='reference'):
        """[build-defined]  How often the bits measured by ftqc.rewrite_program of a program on up to four logical qubits --
        `instructions`: ('I' | 'X' | 'Y' | 'Z', q) and ('CNOT', a, b), then ('MEASURE', q) on distinct qubits -- are wrong when every
        fault location of the rewritten program fails independently (stream_noise.MultiProgram.error_rates has the dict).
        records='propagated' moves the records of known errors through a CNOT as the CNOT moves the errors; the rewritten program
        does not ('reference').  ft_noise.raw_circuit_error_rate is the bare program's side of the comparison."""
        from . import stream_noise
        gadget = stream_noise.multi_program_for(self, instructions)
        return gadget.error_rates(num_samples, p_x, p_y, p_z, seed=seed, first_sample=first_sample, records=records)

    def logical_circuit_retried_error_rates(self, instructions, num_samples, p_x, p_y, p_z, seed=0, first_sample=0, records='reference',
                                            max_attempts=256):
        """[build-defined]  logical_circuit_error_rates with every preparation retried on its own until its verifications pass
        (stream_noise.MultiProgram.retry_error_rates), as the reference's while_do loops run them: essentially every sample is
        accepted, whatever p and the program's length.  The rates are those of the post-selected route at every p; the samples are
        different samples.  The dict also has 'exhausted', 'attempts' and 'preparations'.  The other data blocks wait at no cost
        while a preparation is repeated."""
        from . import stream_noise
        gadget = stream_noise.multi_program_for(self, instructions)
        return gadget.retry_error_rates(num_samples, p_x, p_y, p_z, seed=seed, first_sample=first_sample, records=records,
                                        max_attempts=max_attempts)

    def logical_circuit_retried_gate_error_rates(self, instructions, num_samples, p1, p2, seed=0, first_sample=0, records='reference',
                                                 max_attempts=256):
        """[build-defined]  logical_circuit_retried_error_rates under gate-level faults (stream_noise.MultiProgram
        .retry_gate_error_rates): a one-operand gate fails with probability p1 and one of 3 kinds, a CNOT -- a physical CNOT of a
        transversal logical CNOT included -- as one event with probability p2 and one of 15.  retry_error_rates' dict;
        max_attempts=1 is gate-level post-selection.  ft_noise.raw_circuit_gate_error_rate is the bare program under the same
        model."""
        from . import stream_noise
        gadget = stream_noise.multi_program_for(self, instructions)
        return gadget.retry_gate_error_rates(num_samples, p1, p2, seed=seed, first_sample=first_sample, records=records,
                                             max_attempts=max_attempts)

    def error_correct_retried_error_rates(self, num_samples, p_x, p_y, p_z, rounds, seed=0, first_sample=0, idle_data=False, max_attempts=256):
        """[build-defined]  error_correct_streamed_error_rates with every preparation retried on its own until its verifications
        pass (stream_noise.StreamedGadget.retry_error_rates), as the reference's while_do loops run them: essentially every sample is
        accepted, whatever p and `rounds`.  The rates are those of the post-selected routes at every p; the samples are different
        samples.  The dict also has 'exhausted' (samples with a preparation that failed max_attempts times), 'attempts' and
        'preparations': attempts / (samples * preparations) is the mean number of attempts per preparation."""
        from . import stream_noise
        gadget = stream_noise.stream_for(self, "cycle", (int(rounds), bool(idle_data)))
        return gadget.retry_error_rates(num_samples, p_x, p_y, p_z, seed=seed, first_sample=first_sample, max_attempts=max_attempts)

    def logical_program_retried_error_rates(self, ops, num_samples, p_x, p_y, p_z, seed=0, first_sample=0, max_attempts=256):
        """[build-defined]  logical_program_streamed_error_rates with every preparation retried on its own, likewise.  The rates
        are those of the post-selected routes at every p; the samples are different samples."""
        from . import ft_noise, stream_noise
        gadget = stream_noise.stream_for(self, "program", ft_noise.check_ops(ops))
        return gadget.retry_error_rates(num_samples, p_x, p_y, p_z, seed=seed, first_sample=first_sample, max_attempts=max_attempts)

    def error_correct_retried_wait_error_rates(self, num_samples, p_x, p_y, p_z, q_x, q_y, q_z, rounds, seed=0, first_sample=0, idle_data=False,
                                               wait_steps=1, max_attempts=256):
        """[build-defined]  error_correct_retried_error_rates in which the data block pays for the retries (stream_noise
        .StreamedGadget.retry_wait_error_rates): while a preparation is attempted, every qubit of the data block has a fault location
        of its own with the memory error rates (q_x, q_y, q_z), wait_steps of them per attempt, on every attempt made, the failed ones
        included.  The dict also has 'wait_faults' and 'wait_locations'.  With q = 0 the counts are
        error_correct_retried_error_rates' of the same seed."""
        from . import stream_noise
        gadget = stream_noise.stream_for(self, "cycle", (int(rounds), bool(idle_data)))
        return gadget.retry_wait_error_rates(num_samples, p_x, p_y, p_z, q_x, q_y, q_z, seed=seed, first_sample=first_sample, wait_steps=wait_steps,
                                             max_attempts=max_attempts)

    def logical_program_retried_wait_error_rates(self, ops, num_samples, p_x, p_y, p_z, q_x, q_y, q_z, seed=0, first_sample=0, wait_steps=1,
                                                 max_attempts=256):
        """[build-defined]  logical_program_retried_error_rates with waiting faults on the data block, likewise (none while the data
        block itself is prepared)."""
        from . import ft_noise, stream_noise
        gadget = stream_noise.stream_for(self, "program", ft_noise.check_ops(ops))
        return gadget.retry_wait_error_rates(num_samples, p_x, p_y, p_z, q_x, q_y, q_z, seed=seed, first_sample=first_sample, wait_steps=wait_steps,
                                             max_attempts=max_attempts)

    def error_correct_retried_gate_error_rates(self, num_samples, p1, p2, rounds, seed=0, first_sample=0, idle_data=False, max_attempts=256):
        """[build-defined]  error_correct_retried_error_rates under gate-level faults (stream_noise.StreamedGadget
        .retry_gate_error_rates): every one-operand gate fails with probability p1 and one of 3 kinds, every CNOT as one event with
        probability p2 and one of 15 two-qubit Paulis.  Any number of rounds; the rates per accepted sample are those of
        error_correct_gate_error_rates where that accepts the size, the samples are different samples.  max_attempts = 1 is
        gate-level post-selection of any length."""
        from . import stream_noise
        gadget = stream_noise.stream_for(self, "cycle", (int(rounds), bool(idle_data)))
        return gadget.retry_gate_error_rates(num_samples, p1, p2, seed=seed, first_sample=first_sample, max_attempts=max_attempts)

    def logical_program_retried_gate_error_rates(self, ops, num_samples, p1, p2, seed=0, first_sample=0, max_attempts=256):
        """[build-defined]  logical_program_retried_error_rates under gate-level faults, likewise."""
        from . import ft_noise, stream_noise
        gadget = stream_noise.stream_for(self, "program", ft_noise.check_ops(ops))
        return gadget.retry_gate_error_rates(num_samples, p1, p2, seed=seed, first_sample=first_sample, max_attempts=max_attempts)

    def error_correct_retried_gate_wait_error_rates(self, num_samples, p1, p2, q_x, q_y, q_z, rounds, seed=0, first_sample=0, idle_data=False,
                                                    wait_steps=1, max_attempts=256):
        """[build-defined]  error_correct_retried_gate_error_rates in which the data block pays for the retries (stream_noise
        .StreamedGadget.retry_gate_wait_error_rates): while a preparation is attempted, every qubit of the data block has a fault
        location of its own with the memory error rates (q_x, q_y, q_z), wait_steps of them per attempt, on every attempt made, the
        failed ones included.  The dict also has 'wait_faults' and 'wait_locations'.  With q = 0 the counts are
        error_correct_retried_gate_error_rates' of the same seed."""
        from . import stream_noise
        gadget = stream_noise.stream_for(self, "cycle", (int(rounds), bool(idle_data)))
        return gadget.retry_gate_wait_error_rates(num_samples, p1, p2, q_x, q_y, q_z, seed=seed, first_sample=first_sample, wait_steps=wait_steps,
                                                  max_attempts=max_attempts)

    def logical_program_retried_gate_wait_error_rates(self, ops, num_samples, p1, p2, q_x, q_y, q_z, seed=0, first_sample=0, wait_steps=1,
                                                      max_attempts=256):
        """[build-defined]  logical_program_retried_gate_error_rates with waiting faults on the data block, likewise (none while the
        data block itself is prepared)."""
        from . import ft_noise, stream_noise
        gadget = stream_noise.stream_for(self, "program", ft_noise.check_ops(ops))
        return gadget.retry_gate_wait_error_rates(num_samples, p1, p2, q_x, q_y, q_z, seed=seed, first_sample=first_sample, wait_steps=wait_steps,
                                                  max_attempts=max_attempts)


# -- free functions -----------------------------------------------------------------------------------------

def syndrome_batch(parity_check, errors):
    """[build-defined, x2]  np.mod(np.matmul(parity_check, e), 2) (css_code.py:728) for every row e of
    `errors` (B x n).  Returns a B x r array of dtype 'int'."""
    parity_check = np.asarray(parity_check)
    errors = np.asarray(errors)
    r, n = parity_check.shape
    if errors.ndim != 2 or errors.shape[1] != n:
        raise ValueError("errors must be B x n")
    batch = errors.shape[0]
    if batch == 0 or r == 0:
        return np.zeros((batch, r), dtype='int')
    ctx = _native.default_context()
    out = ctx.syndrome_batch(_native.pack_rows(parity_check), r, n, _native.pack_rows(errors), batch)
    return _native.unpack_rows(out, r, dtype='int')


def syndrome_table(parity_check, max_weight=None, _packed=None):
    """
    Given a parity check matrix of a binary linear code, determine the unique decoding threshold t and
    return it along with a lookup table from syndromes (as bin_matrix.vec_to_int keys) to error vectors
    of weight at most t (css_code.py:715-735).

    Codes of at most 8192 bits are searched entirely on the device (gf2_table.hip): up to 24 checks against a dense table of
    2^r slots, up to 127 checks against a hash table sized from the weight classes it holds.  Otherwise (r > 127) each
    weight class is enumerated in bin_matrix.weight_w_vectors order, in chunks, and its syndromes are computed on the GPU; a class containing a syndrome already seen (in an earlier class or earlier in the
    same class) ends the search and is discarded as a whole, exactly as the reference's loop does.  Keys are
    formed and compared as machine words when r <= 63 (the reference's own keys are only meaningful there,
    SURVEY.md 7.3 item 2) and as Python ints beyond.  max_weight [build-defined] caps the search for large
    codes, where the reference cannot finish.
    """
    parity_check = np.asarray(parity_check)
    r, n = parity_check.shape
    ctx = _native.default_context()
    packed_h = _native.pack_rows(parity_check) if _packed is None else np.ascontiguousarray(_packed)     # (the constructor has them)
    if 0 < n <= ctx.TABLE_MAX_N and r <= ctx.TABLE_MAX_R:
        # whole search on the device (gf2_syndrome_table): one kernel per weight class, first collision ends it
        t, dense = ctx.syndrome_table(packed_h, r, n, max_weight)
        keys = np.nonzero(dense != ctx.TABLE_EMPTY)[0]
        words = dense[keys]
        # the reference's insertion order: by weight, then bin_matrix.weight_w_vectors order (supports ascending
        # lexicographically = the word read with qubit 0 as its most significant bit, descending)
        rev = np.unpackbits(words.view(np.uint8).reshape(-1, 8), axis=1, bitorder="little")
        rev = np.packbits(rev, axis=1, bitorder="big").view(">u8").reshape(-1).astype(np.uint64)
        order = np.lexsort((~rev, np.bitwise_count(words)))
        errs = _native.unpack_rows(words[order].reshape(-1, 1), n, dtype=np.uint8).astype('int')
        return t, dict(zip(keys[order].tolist(), errs))
    if ctx.TABLE_MAX_N < n <= ctx.TABLE_COLS_MAX_N and r <= ctx.TABLE_MAX_R:
        # two-word errors (n up to 127) or, beyond 128 bits, errors as position lists: the device table
        # holds (weight, rank in the class)
        if n <= ctx.TABLE_WIDE_MAX_N:
            t, dense = ctx.syndrome_table_wide(packed_h, r, n, max_weight)
        else:
            t, dense = ctx.syndrome_table_cols(packed_h, r, n, max_weight)
        keys = np.nonzero(dense != ctx.TABLE_EMPTY)[0]
        weight = (dense[keys] >> np.uint64(32)).astype(np.int64)
        rank = dense[keys] & np.uint64(0xFFFFFFFF)
        table = {}
        for w in range(int(weight.max()) + 1 if keys.size else 0):
            sel = np.flatnonzero(weight == w)
            supports = _native.unrank_supports(rank[sel], n, w)
            # the reference's insertion order inside a class: supports ascending lexicographically (bin_matrix.py:57-72)
            order = np.lexsort(tuple(supports[:, k] for k in range(w - 1, -1, -1))) if w else np.arange(sel.size)
            errs = np.zeros((sel.size, n), dtype='int')
            if w:
                errs[np.arange(sel.size)[:, None], supports] = 1
            table.update(zip(keys[sel][order].tolist(), errs[order]))
        return t, table
    if ctx.TABLE_MAX_R < r <= ctx.TABLE_HASH_MAX_R and 0 < n <= ctx.TABLE_HASH_MAX_N:
        # more than 24 checks (round 4; every k = 1 CSS code from n = 51 on has such a check): an open-addressing hash table on
        # the device, sized from the weight classes it holds (gf2_syndrome_table_hashed); exact keys of up to 127 bits
        try:
            t, keys, weight, rank = ctx.syndrome_table_hashed(packed_h, r, n, max_weight)
        except _native.GF2Error as err:
            if err.code != _native.GF2_E_NOMEM:
                raise
            # 2^28 errors enumerated and no two with one syndrome yet: where the reference's loop (css_code.py:722-733) would go on
            # for days (the first collision of a random code with r checks is expected after some 2^((r+1)/2) errors: from about
            # r = 56 on without a bound), this says so and names the way out
            raise ValueError("syndrome_table: more than 2^28 errors without two of one syndrome (r = %d checks, n = %d); pass "
                             "max_weight (CSSCode: max_table_weight) to bound the table" % (r, n)) from err
        keys = np.asarray(keys, dtype=object if r > 63 else np.uint64)
        table = {}
        for w in range(int(weight.max()) + 1 if weight.size else 0):
            sel = np.flatnonzero(weight == w)
            supports = _native.unrank_supports(rank[sel], n, w)
            order = np.lexsort(tuple(supports[:, k] for k in range(w - 1, -1, -1))) if w else np.arange(sel.size)
            errs = np.zeros((sel.size, n), dtype='int')
            if w:
                errs[np.arange(sel.size)[:, None], supports] = 1
            table.update(zip(keys[sel][order].tolist(), errs[order]))
        return t, table
    chk = ctx.check_create(packed_h, r, n) if r else None
    table = {}
    seen = np.zeros(0, dtype=np.uint64)                       # keys of `table`, sorted (r <= 63)
    chunk_size = 1 << 18
    weights = (np.uint64(1) << np.arange(r - 1, -1, -1, dtype=np.uint64)) if 0 < r <= 63 else None
    for w in range(n + 1):
        if max_weight is not None and w > max_weight:
            return max_weight, table
        layer_keys, layer_errs = [], []
        layer_seen = np.zeros(0, dtype=np.uint64)             # keys of this weight class so far (r <= 63)
        layer_seen_big = set()                                # the same as Python ints (r > 63)
        combos = itertools.combinations(range(n), w)
        while True:
            batch = list(itertools.islice(combos, chunk_size))
            count = len(batch)
            if count == 0:
                break
            supports = np.array(batch, dtype=np.int64).reshape(count, w)
            # the error vectors as the table hands them out (dtype 'int'; np.zeros maps untouched pages lazily) and, packed
            # straight from the supports, as the syndrome kernel reads them
            errors = np.zeros((count, n), dtype='int')
            packed_e = np.zeros((count, max(1, _native.words_for(n))), dtype=np.uint64)
            if w:
                rows = np.arange(count)[:, None]
                errors[rows, supports] = 1
                np.bitwise_or.at(packed_e, (np.broadcast_to(rows, supports.shape), supports >> 6),
                                 np.uint64(1) << (supports & 63).astype(np.uint64))
            if r:
                syn = _native.unpack_rows(_syndromes_of(ctx, chk, packed_h, r, n, packed_e, count), r, dtype=np.uint8)
            else:
                syn = np.zeros((count, 0), dtype=np.uint8)
            if weights is not None or r == 0:
                keys = (syn.astype(np.uint64) @ weights) if r else np.zeros(count, dtype=np.uint64)
                collide = (np.unique(keys).size != count or np.isin(keys, seen).any() or
                           np.isin(keys, layer_seen).any())
                if collide:
                    return w - 1, table
                layer_seen = np.union1d(layer_seen, keys)
                layer_keys.extend(int(k) for k in keys)
            else:
                # bin_matrix.vec_to_int of every row (bits, row 0 most significant), as exact Python ints
                big = np.packbits(syn, axis=1, bitorder='big')
                shift = (-r) % 8
                keys = [int.from_bytes(row.tobytes(), 'big') >> shift for row in big]
                fresh = set(keys)
                if len(fresh) != count or any(k in table for k in keys) or not fresh.isdisjoint(layer_seen_big):
                    return w - 1, table
                layer_seen_big |= fresh
                layer_keys.extend(keys)
            layer_errs.append(errors)
        errs = (layer_errs[0] if len(layer_errs) == 1 else np.concatenate(layer_errs)) if layer_errs else np.zeros((0, n), dtype='int')
        table.update(zip(layer_keys, errs))
        if weights is not None:
            seen = np.union1d(seen, layer_seen)
    return n, table


def _syndromes_of(ctx, chk, packed_h, r, n, packed_e, count):
    """Packed syndromes (count x words(r)) of packed errors through a prepared check."""
    if chk.handle is None:
        return ctx.syndrome_batch(packed_h, r, n, packed_e, count)
    lde, lds = packed_e.shape[1], max(1, _native.words_for(r))
    e_buf = ctx.alloc(packed_e.nbytes).upload(packed_e)
    s_buf = ctx.alloc(count * lds * 8).zero()
    ctx.syndrome_dev(chk, e_buf, count, lde, s_buf, lds)
    out = s_buf.download((count, lds), "<u8")
    e_buf.free()
    s_buf.free()
    return out


def _gate_array(prog):
    """Gate array of a program: an (g, 3) array as is; a pyQuil Program (when pyQuil is importable) or any sequence
    of (name, qubits...) tuples is converted, with the reference's checks (css_code.py:741-755)."""
    if isinstance(prog, np.ndarray):
        return np.ascontiguousarray(prog, dtype=np.int32).reshape(-1, 3)
    gates = []
    for inst in getattr(prog, "instructions", prog):
        if isinstance(inst, (tuple, list)):
            name, qubits = inst[0], [int(q) for q in inst[1:]]
        else:
            if not hasattr(inst, "qubits") or not hasattr(inst, "name"):
                raise ValueError("program must only contain gates")
            if any(not hasattr(qubit, "index") for qubit in inst.qubits):
                raise ValueError("gate cannot have placeholders")
            name, qubits = inst.name, [qubit.index for qubit in inst.qubits]
        if name in ('H', GATE_H) and len(qubits) == 1:
            gates.append((GATE_H, qubits[0], 0))
        elif name in ('CNOT', GATE_CNOT) and len(qubits) == 2:
            gates.append((GATE_CNOT, qubits[0], qubits[1]))
        else:
            gates.append((-1, qubits[0] if qubits else 0, 0))        # refused when the walk reaches it
    return np.array(gates, dtype=np.int32).reshape(-1, 3)


def transform_stabilisers(mat, prog):
    """
    Conjugate the k x 2n stabiliser matrix [X | Z] through a Clifford program of H and CNOT gates, in place
    (css_code.py:737-755).  prog is a gate array as returned by CSSCode.noisy_encode_zero / noisy_encode_plus (or a
    pyQuil Program, or tuples ('H', q) / ('CNOT', c, t)).  Gates apply in order on the GPU (gf2_conjugate_gates).
    As in the reference, a gate is checked when it is reached: ValueError for a qubit outside [0, n) or a gate other
    than H / CNOT, NotImplementedError("only handles CSS codes") for an H on a qubit where a row has both X and Z; mat
    then holds what the reference leaves behind (all earlier gates, and the rows before the offending one swapped).
    """
    k, cols = mat.shape
    n = cols // 2
    gates = _gate_array(prog)
    packed = _native.pack_rows(mat)
    rc, stop = _native.default_context().conjugate_gates(packed, k, n, gates)
    _native.unpack_rows_into(packed, mat)
    if rc == _native.GF2_E_NOTCSS:
        q = int(gates[stop, 1])
        bad = int(np.flatnonzero((mat[:, q] == 1) & (mat[:, n + q] == 1))[0])
        upper = mat[:bad, [q, n + q]].copy()                       # css_code.py:761-767: rows above were swapped already
        mat[:bad, q], mat[:bad, n + q] = upper[:, 1], upper[:, 0]
        raise NotImplementedError("only handles CSS codes")
    if rc == _native.GF2_E_ARG:
        kind, a, b = (int(v) for v in gates[stop])
        if kind in (GATE_H, GATE_CNOT):
            raise ValueError("qubit index must be within [0, n)")
        raise ValueError("cannot conjugate gate {}".format(kind))


def conjugate_h_with_check_mat(mat, qubit):
    """css_code.py:757-767."""
    transform_stabilisers(mat, np.array([[GATE_H, qubit, 0]], dtype=np.int32))


def conjugate_cnot_with_check_mat(mat, control, target):
    """css_code.py:769-781."""
    transform_stabilisers(mat, np.array([[GATE_CNOT, control, target]], dtype=np.int32))


def swap_columns(mat, indices):
    """In-place swap of two columns (css_code.py:783-785).  The two columns travel to the GPU as packed
    bits (gf2_swap_columns), so their entries come back reduced modulo 2; the reference's callers
    (css_code.py:56-61) only pass binary matrices."""
    i, j = indices
    m, n = mat.shape
    if m == 0 or i == j:
        return
    packed = _native.pack_rows(mat[:, [i, j]])
    _native.default_context().swap_columns(packed, m, 2, 0, 1)
    mat[:, [i, j]] = _native.unpack_rows(packed, 2, dtype=mat.dtype)


def pauli_term_for_row(x_check, z_check):
    """
    The Pauli operator of a check-matrix row (css_code.py:787-807; Nielsen & Chuang 10.5.1): Y where
    both checks are set, else X or Z.  A pyQuil PauliTerm when pyQuil is importable, otherwise the text
    label with factors in qubit order ("X0*X3*X4*X5"; "I" for the identity).
    """
    x_check = np.asarray(x_check)
    z_check = np.asarray(z_check)
    n = x_check.size
    if not x_check.shape == (n,):
        raise ValueError("x_check has the wrong dimensions")
    if not z_check.shape == (n,):
        raise ValueError("z_check has the wrong dimensions")
    if _HAVE_PYQUIL:                                # pragma: no cover
        result = _ID()
        for i in range(n):
            if x_check[i] and z_check[i]:
                result *= _sY(i)
            elif x_check[i]:
                result *= _sX(i)
            elif z_check[i]:
                result *= _sZ(i)
        return result
    factors = []
    for i in range(n):
        if x_check[i] and z_check[i]:
            factors.append("Y%d" % i)
        elif x_check[i]:
            factors.append("X%d" % i)
        elif z_check[i]:
            factors.append("Z%d" % i)
    return "*".join(factors) if factors else "I"


def _normalize_packed(ctx, packed, r, n, offset):
    """gf2_normalize on packed rows, in place; returns the swaps; the reference's two exceptions (css_code.py:811-812, 825-826)."""
    if n < offset + r:
        raise ValueError("not enough columns")
    if r == 0:
        return []
    try:
        return ctx.normalize(packed, r, n, offset)
    except _native.GF2Error as err:
        if err.code == _native.GF2_E_DEPENDENT:
            raise InvalidCodeError("rows are not independent") from None
        if err.code == _native.GF2_E_COLUMNS:
            raise ValueError("not enough columns") from None
        raise


def normalize_parity_check(h, offset):
    """
    Put h into the form with an identity block in columns offset..offset+r-1 (css_code.py:809-836),
    swapping qubits (columns) where a pivot is missing.  Like the reference it works in place AND returns
    (h mod 2, list of (column, column) swaps).  The swaps and the result are bit-identical to the
    reference's: the GPU kernel performs the same operations in the same order.
    After the call `h` holds the reduced matrix (the reference leaves un-reduced integers congruent to
    it modulo 2).
    """
    r, n = h.shape
    if n < offset + r:
        raise ValueError("not enough columns")
    if r == 0:
        return np.mod(h, 2), []
    packed = _native.pack_rows(h)
    swaps = _normalize_packed(_native.default_context(), packed, r, n, offset)
    _native.unpack_rows_into(packed, h)                       # h is reduced from here on: np.mod(h, 2) is the same matrix again,
    # unpacked a second time (on several host threads: a 64 MiB h.copy() on one takes three times as long)
    if isinstance(h, np.ndarray) and h.dtype in (np.int64, np.uint8):
        return _native.unpack_rows(packed, n, dtype=h.dtype), swaps
    return h.copy(), swaps


def codes_equal(parity_check_1, parity_check_2):
    """Two parity checks define the same code iff their RREFs agree (css_code.py:838-844)."""
    parity_check_1 = np.asarray(parity_check_1)
    parity_check_2 = np.asarray(parity_check_2)
    if parity_check_1.shape != parity_check_2.shape:
        return False
    return np.array_equal(bin_matrix.reduced_row_echelon_form(parity_check_1),
                          bin_matrix.reduced_row_echelon_form(parity_check_2))


def is_doubly_even(mat):
    """Whether every row weight is a multiple of 4 (css_code.py:846-850).  Row weights by popcount on
    the GPU; for 0/1 matrices this is np.sum(mat, axis=1)."""
    mat = np.asarray(mat)
    m, n = mat.shape
    if m == 0:
        return True
    if np.issubdtype(mat.dtype, np.integer) and mat.size and (mat.min() < 0 or mat.max() > 1):
        # the reference sums the raw entries; outside {0,1} that is not a popcount
        return not np.any(np.mod(np.sum(mat, axis=1), 4))
    weights = _native.default_context().row_weights(_native.pack_rows(mat), m, n)
    return not np.any(weights % 4)
