"""
ctypes binding of libgf2hip.so (include/gf2hip.h) and the packed-word helpers the host side uses.

There is no CPU fallback.  If the shared library is missing, or no gfx950 device is usable, the
first compute call raises GF2Error -- the product never routes through oracle/ or NumPy arithmetic.
"""
import collections
import contextlib
import ctypes
import math
import os
import threading

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libgf2hip.so")

GF2_OK, GF2_E_ARG, GF2_E_COLUMNS, GF2_E_DEPENDENT, GF2_E_HIP, GF2_E_NOMEM, GF2_E_NOTCSS, GF2_E_RCCL = 0, -1, -2, -3, -4, -5, -6, -7
COMM_ID_BYTES = 128
LAYOUT_SAMPLE_MAJOR, LAYOUT_BIT_SLICED, LAYOUT_TILED = 0, 1, 2
HIST_FULL, HIST_WEIGHT = 0, 1
GATE_H, GATE_CNOT, GATE_IDLE = 0, 1, 2
GATE_RESET = 3                                      # circuit_effects_timed only
EC_FIELDS_COUNT, EC_MAX_ROUNDS = 8, 6
FT_FIELDS_COUNT, FT_MAX_LDR = 7, 16
STREAM_FIELDS_COUNT, STREAM_MAX_TYPES, STREAM_MAX_OVERLAP = 12, 64, 8
STREAM_NONE, STREAM_EC, STREAM_MEASURE, STREAM_FINAL = 0, 1, 2, 3
MSTREAM_FIELDS_COUNT, MSTREAM_MAX_FRAMES, MSTREAM_MAX_TRIALS, MSTREAM_CNOT = 20, 4, 255, 4
MSTREAM_REFERENCE, MSTREAM_PROPAGATED = 0, 1
RETRY_FIELDS_COUNT, RETRY_MAX_ATTEMPTS, RETRY_MAX_SIZES = 14, 65536, 16
RETRY_WAIT_FIELDS_COUNT, RETRY_WAIT_MAX_ROWS = 15, 512
RETRY_GATE_WAIT_MAX_SIZES = 3
MRETRY_FIELDS_COUNT = 22                            # GF2_MRETRY_FIELDS
CIRCUIT_MAX_N, CIRCUIT_MAX_ROWS, CIRCUIT_MAX_LOCATIONS, CIRCUIT_MAX_LDR = 8192, 16384, 1 << 20, 8
STRATA_MAX, STRATUM_MAX_POSITIONS, CIRCUIT_STRATUM_MAX_WEIGHT = 256, 1 << 20, 16
ENUMERATE_MAX_WEIGHT = 8
GATE_ENUMERATE_MAX_WEIGHT = 4                       # GF2_GATE_ENUMERATE_MAX_WEIGHT
GATE_STRATUM_MAX_WEIGHT = 16                        # GF2_GATE_STRATUM_MAX_WEIGHT
FAULT_RECORD_WORDS, FAULT_LIST_MAX_CAPACITY = 2, 1 << 28       # GF2_FAULT_RECORD_WORDS, GF2_FAULT_LIST_MAX_CAPACITY
K_SYNDROME, K_HIST, K_SAMPLER, K_ELIM = 0, 1, 2, 3
# routing flags of a context and its tunables: the few a caller needs are in include/gf2hip.h (F_MC_DENSE, F_RREF_SEQUENTIAL,
# F_NORMALIZE_SEQUENTIAL, OPT_SLAB_PASS_LOG2, OPT_MC_CHUNK_LOG2), the rest -- routes for the parity tests and the A/B scripts -- in
# csrc/gf2_tuning.h
(F_SPARSE_GATHER, F_SPARSE_SLABS, F_NO_REDO, F_GATHER_GENERIC, F_MC_UNFUSED, F_MC_DENSE, F_MC_FUSED, F_MC_PIPELINE,
 F_RREF_SEQUENTIAL, F_RREF_NO_SMALL, F_NORMALIZE_SEQUENTIAL, F_SAMPLER_GENERIC, F_DIAG_CLOCKS,
 F_DIAG_MC_TIMES, F_MC_ROWS, F_COMBINE_FOLDED, F_RREF_NO_LOOKAHEAD, F_RREF_LOOKAHEAD, F_COMBINE_SEPARATE) = (1 << k for k in range(19))
(OPT_SLAB_PASS_LOG2, OPT_COMBINE_BLOCKS, OPT_GATHER_REVERSE, OPT_REDO_BLOCKS_PER_CU, OPT_MC_CHUNK_LOG2, OPT_COMBINE_THREADS,
 OPT_GATHER_CROSS, OPT_GATHER_OVER, OPT_RREF_SMALL_BCAST, OPT_MC_SAMPLER_WAVES,
 OPT_MC_TAIL_CAP, OPT_RREF_STREAM_VARIANT, OPT_RREF_ROWS_WG, OPT_RREF_SWEEP_K) = range(14)


class GF2Error(RuntimeError):
    """A libgf2hip.so call failed (code and message from gf2_last_error)."""

    def __init__(self, code, message):
        super().__init__("libgf2hip error %d: %s" % (code, message))
        self.code = code
        self.message = message


_c_i64 = ctypes.c_int64
_c_u64 = ctypes.c_uint64
_p = ctypes.c_void_p
_pp = ctypes.POINTER(ctypes.c_void_p)

# name -> argument types; every function returns int unless listed in _RESTYPES.  This table is the
# Python statement of include/gf2hip.h; tests/test_abi.py checks the two against each other.
SIGNATURES = {
    "gf2_version": [],
    "gf2_last_error": [],
    "gf2_device_count": [ctypes.POINTER(ctypes.c_int)],
    "gf2_ctx_create": [ctypes.c_int, _pp],
    "gf2_ctx_destroy": [_p],
    "gf2_ctx_sync": [_p],
    "gf2_ctx_set_flags": [_p, ctypes.c_uint32],
    "gf2_ctx_get_flags": [_p, ctypes.POINTER(ctypes.c_uint32)],
    "gf2_ctx_set_option": [_p, ctypes.c_int, _c_i64],
    "gf2_ctx_fill_workspace": [_p, ctypes.c_int, _p],
    "gf2_dev_alloc": [_p, ctypes.c_size_t, _pp],
    "gf2_dev_free": [_p, _p],
    "gf2_dev_zero": [_p, _p, ctypes.c_size_t],
    "gf2_h2d": [_p, _p, _p, ctypes.c_size_t],
    "gf2_d2h": [_p, _p, _p, ctypes.c_size_t],
    "gf2_timer_start": [_p],
    "gf2_timer_stop": [_p, ctypes.POINTER(ctypes.c_float)],
    "gf2_profile_enable": [_p, ctypes.c_int],
    "gf2_profile_reset": [_p],
    "gf2_profile_get": [_p, ctypes.c_int, ctypes.POINTER(ctypes.c_double), ctypes.POINTER(_c_i64)],
    "gf2_membw_probe_dev": [_p, _p, _p, ctypes.c_size_t, _p],
    "gf2_pack_rows_u8": [_p, _c_i64, _c_i64, _c_i64, _p, _c_i64],
    "gf2_pack_rows_i64": [_p, _c_i64, _c_i64, _c_i64, _p, _c_i64],
    "gf2_pack_rows_binary_u8": [_p, _c_i64, _c_i64, _c_i64, _p, _c_i64, ctypes.POINTER(ctypes.c_int)],
    "gf2_pack_rows_binary_i64": [_p, _c_i64, _c_i64, _c_i64, _p, _c_i64, ctypes.POINTER(ctypes.c_int)],
    "gf2_unpack_rows_u8": [_p, _c_i64, _c_i64, _c_i64, _p, _c_i64],
    "gf2_unpack_rows_i64": [_p, _c_i64, _c_i64, _c_i64, _p, _c_i64],
    "gf2_rref": [_p, _p, _c_i64, _c_i64, _c_i64, _p, _p],
    "gf2_rref_batch": [_p, _p, _c_i64, _c_i64, _c_i64, _c_i64, _p, _p],
    "gf2_rref_batch_dev": [_p, _p, _c_i64, _c_i64, _c_i64, _c_i64, _p, _p],
    "gf2_normalize_dev": [_p, _p, _c_i64, _c_i64, _c_i64, _c_i64, _p, _p, _p],
    "gf2_nullspace": [_p, _p, _c_i64, _c_i64, _c_i64, _p, _c_i64, _p],
    "gf2_normalize": [_p, _p, _c_i64, _c_i64, _c_i64, _c_i64, _p, _p],
    "gf2_swap_columns": [_p, _p, _c_i64, _c_i64, _c_i64, _c_i64, _c_i64],
    "gf2_matmul_abt": [_p, _p, _c_i64, _c_i64, _p, _c_i64, _c_i64, _c_i64, _p, _c_i64],
    "gf2_row_weights": [_p, _p, _c_i64, _c_i64, _c_i64, _p],
    "gf2_conjugate_gates": [_p, _p, _c_i64, _c_i64, _c_i64, _p, _c_i64, ctypes.POINTER(_c_i64)],
    "gf2_syndrome_table": [_p, _p, _c_i64, _c_i64, _c_i64, _p, ctypes.POINTER(_c_i64), ctypes.POINTER(_c_i64)],
    "gf2_syndrome_table_wide": [_p, _p, _c_i64, _c_i64, _c_i64, _p, ctypes.POINTER(_c_i64), ctypes.POINTER(_c_i64)],
    "gf2_syndrome_table_cols": [_p, _p, _c_i64, _c_i64, _c_i64, _c_i64, _p, ctypes.POINTER(_c_i64), ctypes.POINTER(_c_i64)],
    "gf2_syndrome_table_hashed": [_p, _p, _c_i64, _c_i64, _c_i64, _c_i64, _p, _p, _c_i64, ctypes.POINTER(_c_i64), ctypes.POINTER(_c_i64)],
    "gf2_check_create": [_p, _p, _c_i64, _c_i64, _c_i64, _pp],
    "gf2_check_destroy": [_p, _p],
    "gf2_syndrome_batch": [_p, _p, _c_i64, _c_i64, _c_i64, _p, _c_i64, _c_i64, ctypes.c_int, _p, _c_i64],
    "gf2_syndrome_dev": [_p, _p, _p, _c_i64, _c_i64, ctypes.c_int, _p, _c_i64],
    "gf2_syndrome_sparse_dev": [_p, _p, _p, _c_i64, _c_i64, _p, _c_i64, _p, _c_i64],
    "gf2_histogram_dev": [_p, _p, _c_i64, _c_i64, ctypes.c_int, _c_i64, ctypes.c_int, _p, _c_i64],
    "gf2_sample_errors_dev": [_p, _c_i64, _c_u64, _c_i64, _c_i64, ctypes.c_double, ctypes.c_double,
                              ctypes.c_double, _p, _p, _c_i64, ctypes.c_int],
    "gf2_tiled_ld": [_c_i64],
    "gf2_tiled_words": [_c_i64, _c_i64],
    "gf2_retile_dev": [_p, _p, _c_i64, _c_i64, _c_i64, _p],
    "gf2_mc_decode": [_p, _p, _p, _p, _p, _c_u64, _c_u64, _c_u64, _c_i64, _c_i64, ctypes.c_double, ctypes.c_double,
                      ctypes.c_double, _p],
    "gf2_mc_decode_hashed": [_p, _c_i64, _c_i64, _p, _c_i64, _p, _p, _c_i64, _p, _c_i64, _p, _p, _c_i64, _p, _p, _c_u64, _c_i64, _c_i64,
                             ctypes.c_double, ctypes.c_double, ctypes.c_double, _p],
    "gf2_stratum_errors": [_c_i64, _c_i64, _c_u64, _c_i64, _c_i64, ctypes.c_double, ctypes.c_double, ctypes.c_double, _p, _p, _c_i64],
    "gf2_mc_decode_strata": [_p, _c_i64, _c_i64, _p, _c_i64, _p, _p, _c_i64, _p, _c_i64, _p, _p, _c_i64, _p, _p, _c_u64, _c_i64, _c_i64,
                             _p, _p, ctypes.c_double, ctypes.c_double, ctypes.c_double, _p],
    "gf2_mc_run": [_p, _p, _p, _c_u64, _c_i64, _c_i64, ctypes.c_double, ctypes.c_double, ctypes.c_double,
                   ctypes.c_int, _p, _c_i64, _p, _c_i64],
    "gf2_circuit_effects": [_p, _c_i64, _c_i64, _p, _p, _c_i64, _c_i64, _p, _c_i64, _c_i64, _p, ctypes.POINTER(_c_i64)],
    "gf2_circuit_effects_timed": [_p, _c_i64, _c_i64, _p, _p, _c_i64, _c_i64, _p, _c_i64, _c_i64, _p, ctypes.POINTER(_c_i64), _p],
    "gf2_ec_tally_host": [_p, _c_i64, _c_i64, _c_i64, _c_i64, _c_i64, _p, _p, _c_i64, _c_i64, _p, _p, _c_i64, _p, _p],
    "gf2_mc_ec_decode": [_p, _p, _c_i64, _c_i64, _p, _p, _c_i64, _c_i64, _p, _p, _c_i64, _c_u64, _c_i64, _c_i64, ctypes.c_double,
                         ctypes.c_double, ctypes.c_double, _p],
    "gf2_ft_tally_host": [_p, _c_i64, _c_i64, _c_i64, _c_i64, _c_u64, _c_i64, _p, _p, _c_i64, _c_i64, _p, _p, _c_i64, _p, _p],
    "gf2_ft_circuit_create": [_p, _p, _c_i64, _c_i64, _pp],
    "gf2_ft_outcomes_dev": [_p, _p, _c_u64, _c_i64, _c_i64, ctypes.c_double, ctypes.c_double, ctypes.c_double, _p, _c_i64],
    "gf2_mc_ft_decode": [_p, _p, _c_i64, _c_u64, _c_i64, _p, _p, _c_i64, _c_i64, _p, _p, _c_i64, _c_u64, _c_i64, _c_i64, ctypes.c_double,
                         ctypes.c_double, ctypes.c_double, _p],
    "gf2_circuit_create": [_p, _p, _c_i64, _c_i64, _pp],
    "gf2_circuit_destroy": [_p, _p],
    "gf2_circuit_outcomes_dev": [_p, _p, _c_u64, _c_i64, _c_i64, ctypes.c_double, ctypes.c_double, ctypes.c_double, _p, _c_i64],
    "gf2_mc_circuit_run": [_p, _p, _c_i64, _c_i64, _c_u64, _c_i64, _c_i64, ctypes.c_double, ctypes.c_double, ctypes.c_double,
                           ctypes.c_int, _p, _c_i64, _p, _c_i64],
    "gf2_mc_circuit_decode": [_p, _p, _c_i64, _p, _p, _c_i64, _c_i64, _p, _p, _c_i64, _c_u64, _c_i64, _c_i64, ctypes.c_double,
                              ctypes.c_double, ctypes.c_double, _p],
    "gf2_mc_circuit_decode_strata": [_p, _p, _c_i64, _p, _p, _c_i64, _c_i64, _p, _p, _c_i64, _c_u64, _c_i64, _c_i64, _p, _p,
                                     ctypes.c_double, ctypes.c_double, ctypes.c_double, _p],
    "gf2_subset_unrank": [_c_i64, _c_i64, _c_i64, _p],
    "gf2_circuit_enumerate_host": [_p, _c_i64, _c_i64, _c_i64, _p, _p, _c_i64, _c_i64, _p, _p, _c_i64, _c_i64, _c_i64, _c_i64, _p],
    "gf2_circuit_enumerate": [_p, _p, _c_i64, _p, _p, _c_i64, _c_i64, _p, _p, _c_i64, _c_i64, _c_i64, _c_i64, _p],
    "gf2_ec_enumerate_host": [_p, _c_i64, _c_i64, _c_i64, _c_i64, _p, _p, _c_i64, _c_i64, _p, _p, _c_i64, _c_i64, _c_i64, _c_i64, _p],
    "gf2_ft_enumerate_host": [_p, _c_i64, _c_i64, _c_i64, _c_u64, _c_i64, _p, _p, _c_i64, _c_i64, _p, _p, _c_i64, _c_i64, _c_i64, _c_i64, _p],
    "gf2_ec_enumerate": [_p, _p, _c_i64, _c_i64, _p, _p, _c_i64, _c_i64, _p, _p, _c_i64, _c_i64, _c_i64, _c_i64, _p],
    "gf2_ft_enumerate": [_p, _p, _c_i64, _c_u64, _c_i64, _p, _p, _c_i64, _c_i64, _p, _p, _c_i64, _c_i64, _c_i64, _c_i64, _p],
    "gf2_ec_gate_enumerate_host": [_p, _c_i64, _c_i64, _c_i64, _c_i64, _p, _p, _c_i64, _c_i64, _p, _p, _c_i64, _p, _c_i64, _c_i64, _c_i64, _c_i64, _c_i64,
                                   _c_i64, _p],
    "gf2_ft_gate_enumerate_host": [_p, _c_i64, _c_i64, _c_i64, _c_u64, _c_i64, _p, _p, _c_i64, _c_i64, _p, _p, _c_i64, _p, _c_i64, _c_i64, _c_i64, _c_i64,
                                   _c_i64, _c_i64, _p],
    "gf2_ec_gate_enumerate": [_p, _p, _c_i64, _c_i64, _p, _p, _c_i64, _c_i64, _p, _p, _c_i64, _p, _c_i64, _c_i64, _c_i64, _c_i64, _c_i64, _c_i64, _p],
    "gf2_ft_gate_enumerate": [_p, _p, _c_i64, _c_u64, _c_i64, _p, _p, _c_i64, _c_i64, _p, _p, _c_i64, _p, _c_i64, _c_i64, _c_i64, _c_i64, _c_i64, _c_i64,
                              _p],
    "gf2_ec_enumerate_list_host": [_p, _c_i64, _c_i64, _c_i64, _c_i64, _p, _p, _c_i64, _c_i64, _p, _p, _c_i64, _c_i64, _c_i64, _c_i64, _c_u64, _c_i64,
                                   _p, ctypes.POINTER(_c_i64)],
    "gf2_ft_enumerate_list_host": [_p, _c_i64, _c_i64, _c_i64, _c_u64, _c_i64, _p, _p, _c_i64, _c_i64, _p, _p, _c_i64, _c_i64, _c_i64, _c_i64, _c_u64,
                                   _c_i64, _p, ctypes.POINTER(_c_i64)],
    "gf2_ec_enumerate_list": [_p, _p, _c_i64, _c_i64, _p, _p, _c_i64, _c_i64, _p, _p, _c_i64, _c_i64, _c_i64, _c_i64, _c_u64, _c_i64, _p,
                              ctypes.POINTER(_c_i64)],
    "gf2_ft_enumerate_list": [_p, _p, _c_i64, _c_u64, _c_i64, _p, _p, _c_i64, _c_i64, _p, _p, _c_i64, _c_i64, _c_i64, _c_i64, _c_u64, _c_i64, _p,
                              ctypes.POINTER(_c_i64)],
    "gf2_ec_gate_enumerate_list_host": [_p, _c_i64, _c_i64, _c_i64, _c_i64, _p, _p, _c_i64, _c_i64, _p, _p, _c_i64, _p, _c_i64, _c_i64, _c_i64, _c_i64,
                                        _c_i64, _c_i64, _c_u64, _c_i64, _p, ctypes.POINTER(_c_i64)],
    "gf2_ft_gate_enumerate_list_host": [_p, _c_i64, _c_i64, _c_i64, _c_u64, _c_i64, _p, _p, _c_i64, _c_i64, _p, _p, _c_i64, _p, _c_i64, _c_i64, _c_i64,
                                        _c_i64, _c_i64, _c_i64, _c_u64, _c_i64, _p, ctypes.POINTER(_c_i64)],
    "gf2_ec_gate_enumerate_list": [_p, _p, _c_i64, _c_i64, _p, _p, _c_i64, _c_i64, _p, _p, _c_i64, _p, _c_i64, _c_i64, _c_i64, _c_i64, _c_i64, _c_i64,
                                   _c_u64, _c_i64, _p, ctypes.POINTER(_c_i64)],
    "gf2_ft_gate_enumerate_list": [_p, _p, _c_i64, _c_u64, _c_i64, _p, _p, _c_i64, _c_i64, _p, _p, _c_i64, _p, _c_i64, _c_i64, _c_i64, _c_i64, _c_i64,
                                   _c_i64, _c_u64, _c_i64, _p, ctypes.POINTER(_c_i64)],
    "gf2_stratum_outcomes_host": [_p, _c_i64, _c_i64, _c_i64, _c_u64, _c_i64, _c_i64, ctypes.c_double, ctypes.c_double, ctypes.c_double, _p,
                                  _c_i64],
    "gf2_mc_ec_decode_strata": [_p, _p, _c_i64, _c_i64, _p, _p, _c_i64, _c_i64, _p, _p, _c_i64, _c_u64, _c_i64, _c_i64, _p, _p,
                                ctypes.c_double, ctypes.c_double, ctypes.c_double, _p],
    "gf2_mc_ft_decode_strata": [_p, _p, _c_i64, _c_u64, _c_i64, _p, _p, _c_i64, _c_i64, _p, _p, _c_i64, _c_u64, _c_i64, _c_i64, _p, _p,
                                ctypes.c_double, ctypes.c_double, ctypes.c_double, _p],
    "gf2_gate_stratum_outcomes_host": [_p, _c_i64, _c_i64, _p, _c_i64, _c_i64, _c_i64, _c_i64, _c_u64, _c_i64, _c_i64, _p, _c_i64, _p],
    "gf2_mc_ec_decode_gate_strata": [_p, _p, _c_i64, _c_i64, _p, _p, _c_i64, _c_i64, _p, _p, _c_i64, _p, _c_i64, _c_i64, _c_u64, _c_i64,
                                     _c_i64, _p, _p, _p, _p],
    "gf2_mc_ft_decode_gate_strata": [_p, _p, _c_i64, _c_u64, _c_i64, _p, _p, _c_i64, _c_i64, _p, _p, _c_i64, _p, _c_i64, _c_i64, _c_u64,
                                     _c_i64, _c_i64, _p, _p, _p, _p],
    "gf2_gate_outcomes_host": [_p, _c_i64, _c_i64, _p, _c_i64, _c_i64, _c_u64, _c_i64, _c_i64, ctypes.c_double, ctypes.c_double, _p, _c_i64,
                               _p],
    "gf2_mc_ec_decode_gate": [_p, _p, _c_i64, _c_i64, _p, _p, _c_i64, _c_i64, _p, _p, _c_i64, _p, _c_i64, _c_i64, _c_u64, _c_i64, _c_i64,
                              ctypes.c_double, ctypes.c_double, _p],
    "gf2_mc_ft_decode_gate": [_p, _p, _c_i64, _c_u64, _c_i64, _p, _p, _c_i64, _c_i64, _p, _p, _c_i64, _p, _c_i64, _c_i64, _c_u64, _c_i64,
                              _c_i64, ctypes.c_double, ctypes.c_double, _p],
    "gf2_stream_words_host": [_p, _p, _p, _c_i64, _p, _p, _c_i64, _p, _p, _p, _c_i64, _p, _c_i64],
    "gf2_stream_tally_host": [_p, _c_i64, _c_i64, _p, _c_i64, _c_i64, _c_i64, _p, _p, _c_i64, _c_i64, _p, _p, _c_i64, _p, _p],
    "gf2_stream_create": [_p, _p, _p, _p, _c_i64, _p, _p, _c_i64, _pp],
    "gf2_stream_destroy": [_p, _p],
    "gf2_stream_outcomes_dev": [_p, _p, _c_u64, _c_i64, _c_i64, ctypes.c_double, ctypes.c_double, ctypes.c_double, _p, _c_i64],
    "gf2_mc_stream_decode": [_p, _p, _c_i64, _p, _p, _c_i64, _c_i64, _p, _p, _c_i64, _c_u64, _c_i64, _c_i64, ctypes.c_double, ctypes.c_double,
                             ctypes.c_double, _p],
    "gf2_mstream_words_host": [_p, _p, _p, _c_i64, _p, _p, _p, _p, _c_i64, _c_i64, _p, _p, _p, _c_i64, _p, _c_i64],
    "gf2_mstream_tally_host": [_p, _c_i64, _c_i64, _p, _p, _p, _c_i64, _c_i64, _c_i64, _c_i64, _c_i64, _p, _p, _c_i64, _c_i64, _p, _p, _c_i64, _p, _p],
    "gf2_mstream_create": [_p, _p, _p, _p, _c_i64, _p, _p, _p, _p, _c_i64, _c_i64, _pp],
    "gf2_mstream_destroy": [_p, _p],
    "gf2_mstream_outcomes_dev": [_p, _p, _c_u64, _c_i64, _c_i64, ctypes.c_double, ctypes.c_double, ctypes.c_double, _p, _c_i64],
    "gf2_mc_mstream_decode": [_p, _p, _c_i64, _c_i64, _p, _p, _c_i64, _c_i64, _p, _p, _c_i64, _c_u64, _c_i64, _c_i64, ctypes.c_double, ctypes.c_double,
                              ctypes.c_double, _p],
    "gf2_mretry_words_host": [_p, _p, _p, _c_i64, _p, _p, _p, _p, _c_i64, _c_i64, _p, _p, _c_u64, _c_i64, _c_i64, ctypes.c_double, ctypes.c_double,
                              ctypes.c_double, _c_i64, _p, _c_i64, _p],
    "gf2_mretry_create": [_p, _p, _p, _p, _c_i64, _p, _p, _p, _p, _c_i64, _c_i64, _p, _p, _pp],
    "gf2_mretry_destroy": [_p, _p],
    "gf2_mretry_outcomes_dev": [_p, _p, _c_u64, _c_i64, _c_i64, ctypes.c_double, ctypes.c_double, ctypes.c_double, _c_i64, _p, _c_i64],
    "gf2_mc_mretry_decode": [_p, _p, _c_i64, _c_i64, _p, _p, _c_i64, _c_i64, _p, _p, _c_i64, _c_u64, _c_i64, _c_i64, ctypes.c_double, ctypes.c_double,
                             ctypes.c_double, _c_i64, _p],
    "gf2_mretry_gate_words_host": [_p, _p, _p, _c_i64, _p, _p, _p, _p, _c_i64, _c_i64, _p, _p, _p, _p, _c_u64, _c_i64, _c_i64, ctypes.c_double,
                                   ctypes.c_double, _c_i64, _p, _c_i64, _p],
    "gf2_mretry_gate_create": [_p, _p, _p, _p, _c_i64, _p, _p, _p, _p, _c_i64, _c_i64, _p, _p, _p, _p, _pp],
    "gf2_mretry_gate_destroy": [_p, _p],
    "gf2_mretry_gate_outcomes_dev": [_p, _p, _c_u64, _c_i64, _c_i64, ctypes.c_double, ctypes.c_double, _c_i64, _p, _c_i64],
    "gf2_mc_mretry_gate_decode": [_p, _p, _c_i64, _c_i64, _p, _p, _c_i64, _c_i64, _p, _p, _c_i64, _c_u64, _c_i64, _c_i64, ctypes.c_double,
                                  ctypes.c_double, _c_i64, _p],
    "gf2_retry_words_host": [_p, _p, _p, _c_i64, _p, _p, _c_i64, _p, _p, _c_u64, _c_i64, _c_i64, ctypes.c_double, ctypes.c_double, ctypes.c_double,
                             _c_i64, _p, _c_i64, _p],
    "gf2_retry_create": [_p, _p, _p, _p, _c_i64, _p, _p, _c_i64, _p, _p, _pp],
    "gf2_retry_destroy": [_p, _p],
    "gf2_retry_outcomes_dev": [_p, _p, _c_u64, _c_i64, _c_i64, ctypes.c_double, ctypes.c_double, ctypes.c_double, _c_i64, _p, _c_i64],
    "gf2_mc_retry_decode": [_p, _p, _c_i64, _p, _p, _c_i64, _c_i64, _p, _p, _c_i64, _c_u64, _c_i64, _c_i64, ctypes.c_double, ctypes.c_double,
                            ctypes.c_double, _c_i64, _p],
    "gf2_retry_wait_words_host": [_p, _p, _p, _c_i64, _p, _p, _c_i64, _p, _p, _p, _p, _c_u64, _c_i64, _c_i64] + [ctypes.c_double] * 6 +
                                 [_c_i64, _p, _c_i64, _p],
    "gf2_retry_wait_create": [_p, _p, _p, _p, _c_i64, _p, _p, _c_i64, _p, _p, _p, _p, _pp],
    "gf2_retry_wait_destroy": [_p, _p],
    "gf2_retry_wait_outcomes_dev": [_p, _p, _c_u64, _c_i64, _c_i64] + [ctypes.c_double] * 6 + [_c_i64, _p, _c_i64],
    "gf2_mc_retry_wait_decode": [_p, _p, _c_i64, _p, _p, _c_i64, _c_i64, _p, _p, _c_i64, _c_u64, _c_i64, _c_i64] + [ctypes.c_double] * 6 +
                                [_c_i64, _p],
    "gf2_retry_gate_words_host": [_p, _p, _p, _c_i64, _p, _p, _c_i64, _p, _p, _p, _p, _c_u64, _c_i64, _c_i64, ctypes.c_double, ctypes.c_double,
                                  _c_i64, _p, _c_i64, _p],
    "gf2_retry_gate_create": [_p, _p, _p, _p, _c_i64, _p, _p, _c_i64, _p, _p, _p, _p, _pp],
    "gf2_retry_gate_destroy": [_p, _p],
    "gf2_retry_gate_outcomes_dev": [_p, _p, _c_u64, _c_i64, _c_i64, ctypes.c_double, ctypes.c_double, _c_i64, _p, _c_i64],
    "gf2_mc_retry_gate_decode": [_p, _p, _c_i64, _p, _p, _c_i64, _c_i64, _p, _p, _c_i64, _c_u64, _c_i64, _c_i64, ctypes.c_double, ctypes.c_double,
                                 _c_i64, _p],
    "gf2_retry_gate_wait_words_host": [_p, _p, _p, _c_i64, _p, _p, _c_i64, _p, _p, _p, _p, _p, _p, _c_u64, _c_i64, _c_i64] + [ctypes.c_double] * 5 +
                                      [_c_i64, _p, _c_i64, _p],
    "gf2_retry_gate_wait_create": [_p, _p, _p, _p, _c_i64, _p, _p, _c_i64, _p, _p, _p, _p, _p, _p, _pp],
    "gf2_retry_gate_wait_destroy": [_p, _p],
    "gf2_retry_gate_wait_outcomes_dev": [_p, _p, _c_u64, _c_i64, _c_i64] + [ctypes.c_double] * 5 + [_c_i64, _p, _c_i64],
    "gf2_mc_retry_gate_wait_decode": [_p, _p, _c_i64, _p, _p, _c_i64, _c_i64, _p, _p, _c_i64, _c_u64, _c_i64, _c_i64] + [ctypes.c_double] * 5 +
                                     [_c_i64, _p],
    "gf2_comm_unique_id": [_p, ctypes.c_size_t],
    "gf2_comm_create": [_p, _p, ctypes.c_int, ctypes.c_int, _pp],
    "gf2_comm_create_all": [_pp, ctypes.c_int, _pp],
    "gf2_comm_size": [_p, ctypes.POINTER(ctypes.c_int), ctypes.POINTER(ctypes.c_int)],
    "gf2_comm_destroy": [_p],
    "gf2_hist_allreduce": [_p, _pp, _c_i64],
    "gf2_rccl_version": [ctypes.POINTER(ctypes.c_int)],
}
_RESTYPES = {"gf2_last_error": ctypes.c_char_p, "gf2_tiled_ld": _c_i64, "gf2_tiled_words": _c_i64}

_lib = None
_lib_lock = threading.Lock()


def lib():
    """The loaded library.  Raises GF2Error when it has not been built."""
    global _lib
    if _lib is None:
        with _lib_lock:
            if _lib is None:
                if not os.path.exists(LIB_PATH):
                    raise GF2Error(GF2_E_HIP, "%s not found: build it with `python -c 'import "
                                   "__graft_entry__ as g; g.build()'` (there is no CPU fallback)" % LIB_PATH)
                handle = ctypes.CDLL(LIB_PATH)
                for name, argtypes in SIGNATURES.items():
                    fn = getattr(handle, name)
                    fn.argtypes = argtypes
                    fn.restype = _RESTYPES.get(name, ctypes.c_int)
                _lib = handle
    return _lib


def check(code):
    if code != GF2_OK:
        raise GF2Error(code, lib().gf2_last_error().decode("utf-8", "replace"))


def device_count():
    count = ctypes.c_int(0)
    rc = lib().gf2_device_count(ctypes.byref(count))
    return count.value if rc == GF2_OK else 0


# ---- packed words ---------------------------------------------------------------------------------------

def words_for(bits):
    return (int(bits) + 63) >> 6


def pack_rows(mat, ld=None):
    """Dense 2-D integer array -> packed uint64 rows (column j at word j>>6, bit j&63).  Entries are
    reduced with `& 1`, which is what the reference's lazy np.mod(., 2) amounts to for integers."""
    mat = np.asarray(mat)
    if mat.ndim != 2:
        raise ValueError("expected a 2-D array")
    m, n = mat.shape
    width = max(1, words_for(n)) if ld is None else int(ld)
    if m and n and mat.flags.c_contiguous and mat.dtype in (np.int64, np.uint8):
        # one pass in C (gf2_pack_rows_*): 2.5x faster than the NumPy route below on a 2048 x 4096 int64 array
        out = np.zeros((m, width), dtype="<u8")
        fn = lib().gf2_pack_rows_i64 if mat.dtype == np.int64 else lib().gf2_pack_rows_u8
        check(fn(_ptr(mat), m, n, n, _ptr(out), width))
        return out
    if mat.dtype == np.bool_:
        bits = mat.astype(np.uint8)
    elif np.issubdtype(mat.dtype, np.integer):
        bits = (mat & 1).astype(np.uint8)
    else:
        bits = np.mod(mat, 2).astype(np.uint8)
    padded = np.zeros((m, width * 64), dtype=np.uint8)
    padded[:, :n] = bits
    return np.ascontiguousarray(np.packbits(padded, axis=1, bitorder="little").view("<u8").reshape(m, width))


def pack_rows_binary(mat):
    """(packed rows, every entry is 0 or 1) -- the test of css_code.py:39-44 made while packing: for C-contiguous int64 / uint8
    arrays one threaded pass in C; otherwise the reference's own expression."""
    mat = np.asarray(mat)
    if mat.ndim != 2:
        raise ValueError("expected a 2-D array")
    m, n = mat.shape
    if m and n and mat.flags.c_contiguous and mat.dtype in (np.int64, np.uint8):
        out = np.zeros((m, max(1, words_for(n))), dtype="<u8")
        other = ctypes.c_int(0)
        fn = lib().gf2_pack_rows_binary_i64 if mat.dtype == np.int64 else lib().gf2_pack_rows_binary_u8
        check(fn(_ptr(mat), m, n, n, _ptr(out), out.shape[1], ctypes.byref(other)))
        return out, other.value == 0
    reduced = np.mod(np.array(mat, dtype='int'), 2)
    return pack_rows(reduced), bool(np.array_equal(reduced, mat))


def unpack_rows(words, n, dtype="int"):
    """Packed uint64 rows -> dense m x n array of `dtype`."""
    words = np.ascontiguousarray(words, dtype="<u8")
    m = words.shape[0]
    if m == 0 or n == 0:
        return np.zeros((m, n), dtype=dtype)
    if np.dtype(dtype) in (np.dtype(np.int64), np.dtype(np.uint8)):
        out = np.empty((m, n), dtype=dtype)
        fn = lib().gf2_unpack_rows_i64 if np.dtype(dtype) == np.dtype(np.int64) else lib().gf2_unpack_rows_u8
        check(fn(_ptr(words), m, n, words.shape[1], _ptr(out), n))
        return out
    bits = np.unpackbits(words.view(np.uint8).reshape(m, -1), axis=1, bitorder="little")
    return bits[:, :n].astype(dtype)


def unpack_rows_into(words, out):
    """Packed uint64 rows -> the existing dense array `out` (m x n), in place; one pass in C when `out` is a C-contiguous
    int64 or uint8 array."""
    m, n = out.shape
    words = np.ascontiguousarray(words, dtype="<u8")
    if m and n and out.flags.c_contiguous and out.dtype in (np.int64, np.uint8):
        fn = lib().gf2_unpack_rows_i64 if out.dtype == np.int64 else lib().gf2_unpack_rows_u8
        check(fn(_ptr(words), m, n, words.shape[1], _ptr(out), n))
    else:
        out[...] = unpack_rows(words, n, dtype=out.dtype)
    return out


def unrank_supports(ranks, n, w):
    """Supports (count x w, ascending positions) of the weight-w errors with the given ranks in the combinatorial number system:
    positions c_1 < ... < c_w have rank C(c_1, 1) + ... + C(c_w, w) (the order gf2_syndrome_table_wide enumerates in)."""
    import math
    ranks = np.array(ranks, dtype=np.uint64)
    out = np.zeros((ranks.size, w), dtype=np.int64)
    for k in range(w, 0, -1):
        column = np.array([min(math.comb(c, k), 1 << 63) for c in range(n + 1)], dtype=np.uint64)   # C(c, k), ascending in c
        c = np.searchsorted(column, ranks, side='right').astype(np.int64) - 1                        # largest c with C(c, k) <= rank
        out[:, k - 1] = c
        ranks = ranks - column[c]
    return out


def tiled_ld(n):
    return int(lib().gf2_tiled_ld(int(n)))


def tiled_words(n, batch):
    return int(lib().gf2_tiled_words(int(n), int(batch)))


def tile_rows(packed, n):
    """Host model of GF2_LAYOUT_TILED: sample-major packed rows (B x ld) -> flat tiled words."""
    packed = np.ascontiguousarray(packed, dtype="<u8")
    batch, ld = packed.shape
    ldt = tiled_ld(n)
    tiles = max(1, (batch + 63) // 64)
    full = np.zeros((tiles * 64, ldt), dtype="<u8")
    full[:batch, :min(ld, ldt)] = packed[:, :min(ld, ldt)]
    # (tile, lane, pair, half) -> (tile, pair, lane, half)
    return np.ascontiguousarray(full.reshape(tiles, 64, ldt // 2, 2).transpose(0, 2, 1, 3)).reshape(-1)


def untile_rows(flat, n, batch):
    flat = np.ascontiguousarray(flat, dtype="<u8")
    ldt = tiled_ld(n)
    tiles = flat.size // (64 * ldt)
    rows = flat.reshape(tiles, ldt // 2, 64, 2).transpose(0, 2, 1, 3).reshape(tiles * 64, ldt)
    return np.ascontiguousarray(rows[:batch])


def _ptr(arr):
    return arr.ctypes.data_as(ctypes.c_void_p)


def circuit_effects(gates, n, rows_x, rows_z, ldr=None):
    """gf2_circuit_effects (host code, no GPU): gates (g, 3) int32 rows (kind, a, b) with kind GATE_H / GATE_CNOT / GATE_IDLE;
    rows_x / rows_z: packed outcome rows (nrows x words(n)).  Returns (eff, locations): eff[l, c] = the ldr packed words of the
    outcomes an X (c = 0) / Z (c = 1) fault at location l flips; locations (L, 2) int64 rows (gate, qubit)."""
    gates = np.ascontiguousarray(gates, dtype=np.int32).reshape(-1, 3)
    rows_x = np.ascontiguousarray(rows_x, dtype="<u8")
    rows_z = np.ascontiguousarray(rows_z, dtype="<u8")
    if rows_x.ndim != 2 or rows_x.shape != rows_z.shape:
        raise ValueError("rows_x and rows_z must be packed 2-D arrays of one shape")
    nrows = rows_x.shape[0]
    ldr = max(1, words_for(nrows)) if ldr is None else int(ldr)
    count = _c_i64(0)
    args = (_ptr(gates) if len(gates) else None, len(gates), int(n), _ptr(rows_x) if nrows else None,
            _ptr(rows_z) if nrows else None, nrows, rows_x.shape[1])
    check(lib().gf2_circuit_effects(*args, None, ldr, 0, None, ctypes.byref(count)))
    total = int(count.value)
    eff = np.zeros((max(1, total), 2, ldr), dtype="<u8")
    locations = np.zeros((max(1, total), 2), dtype=np.int64)
    check(lib().gf2_circuit_effects(*args, _ptr(eff), ldr, total, _ptr(locations), ctypes.byref(count)))
    return eff[:total], locations[:total]


def circuit_effects_timed(gates, n, rows_x, rows_z, row_time, ldr=None):
    """gf2_circuit_effects_timed (host code, no GPU): circuit_effects with GATE_RESET among the kinds and one time per outcome row
    in [0, len(gates)] -- row r is read on the frame just before gate row_time[r] (DESIGN.md "Error-correction cycle")."""
    gates = np.ascontiguousarray(gates, dtype=np.int32).reshape(-1, 3)
    rows_x = np.ascontiguousarray(rows_x, dtype="<u8")
    rows_z = np.ascontiguousarray(rows_z, dtype="<u8")
    row_time = np.ascontiguousarray(row_time, dtype=np.int64).reshape(-1)
    if rows_x.ndim != 2 or rows_x.shape != rows_z.shape or len(row_time) != rows_x.shape[0]:
        raise ValueError("rows_x and rows_z must be packed 2-D arrays of one shape, with one time per row")
    nrows = rows_x.shape[0]
    ldr = max(1, words_for(nrows)) if ldr is None else int(ldr)
    count = _c_i64(0)
    args = (_ptr(gates) if len(gates) else None, len(gates), int(n), _ptr(rows_x) if nrows else None,
            _ptr(rows_z) if nrows else None, nrows, rows_x.shape[1])
    times = _ptr(row_time) if nrows else None
    check(lib().gf2_circuit_effects_timed(*args, None, ldr, 0, None, ctypes.byref(count), times))
    total = int(count.value)
    eff = np.zeros((max(1, total), 2, ldr), dtype="<u8")
    locations = np.zeros((max(1, total), 2), dtype=np.int64)
    check(lib().gf2_circuit_effects_timed(*args, _ptr(eff), ldr, total, _ptr(locations), ctypes.byref(count), times))
    return eff[:total], locations[:total]


# ---- the tally rules of the gadgets ---------------------------------------------------------------------------------------------
# A rule: the prefix of its entry points' and wrappers' names, its number of count fields, and `head`, which converts the arguments its
# entry points take in front of the two syndrome tables.  Every family of entry points below is marshalled once, for all rules.
Rule = collections.namedtuple("Rule", "name fields head")
EC_RULE = Rule("ec", EC_FIELDS_COUNT, lambda rounds: (int(rounds),))
FT_RULE = Rule("ft", FT_FIELDS_COUNT, lambda nsteps, measure_mask: (int(nsteps), int(measure_mask) & 0xFFFFFFFFFFFFFFFF))
CIRCUIT_RULE, STREAM_RULE, RETRY_RULE, RETRY_WAIT_RULE = (Rule(name, fields, lambda: ()) for name, fields in
                                                          (("circuit", 5), ("stream", STREAM_FIELDS_COUNT), ("retry", RETRY_FIELDS_COUNT),
                                                           ("retry_wait", RETRY_WAIT_FIELDS_COUNT)))
MSTREAM_RULE = Rule("mstream", MSTREAM_FIELDS_COUNT, lambda: ())
MRETRY_RULE = Rule("mretry", MRETRY_FIELDS_COUNT, lambda: ())


def _enumerate_tables(keys1, flips1, keys2, flips2, null_flips=False):
    """The two syndrome tables as the entry points take them: (the arrays, to keep alive; ((keys, flips, entries) of C1's, of C2's)).
    An empty table is a null one; null_flips: flips may be None, a null pointer beside the keys (gf2_mc_circuit_decode takes it)."""
    keep, tables = [], []
    for keys, flips in ((keys1, flips1), (keys2, flips2)):
        keys = np.ascontiguousarray(keys, dtype="<u8")
        flips = None if flips is None and null_flips else np.ascontiguousarray(flips, dtype=np.uint8)
        keep += [keys, flips]
        tables.append((_ptr(keys) if len(keys) else None, _ptr(flips) if len(keys) and flips is not None else None, len(keys)))
    return tuple(keep), tuple(tables)


def _rule_arguments(rule, head, tables, null_flips=False):
    """(arrays to keep alive, the arguments every entry point of a rule takes after its effect table or its handles): the rule's own,
    then r and the (keys, flips, entries) of either table.  tables: (r1, keys1, flips1, r2, keys2, flips2)."""
    r1, keys1, flips1, r2, keys2, flips2 = tables
    keep, (t1, t2) = _enumerate_tables(keys1, flips1, keys2, flips2, null_flips)
    return keep, rule.head(*head) + (int(r1),) + t1 + (int(r2),) + t2


def _effects(eff):
    """An effect table (L, 2, ldr) as the host statements take it: (the array, to keep alive; (eff, locations, ldr))."""
    eff = np.ascontiguousarray(eff, dtype="<u8")
    if eff.ndim != 3 or eff.shape[1] != 2:
        raise ValueError("eff must be (locations, 2, ldr)")
    return eff, (_ptr(eff), eff.shape[0], eff.shape[2])


def _tally_words(words):
    words = np.ascontiguousarray(words, dtype="<u8")
    if words.ndim != 2:
        raise ValueError("words must be (samples, ldw)")
    return words


def _tally_host(fn, rule, words, middle, head, tables, classes):
    """A gf2_*_tally_host entry point over `words` (_tally_words'); middle: its arguments between ldw and the rule's."""
    keep, rest = _rule_arguments(rule, head, tables)
    counts = np.zeros(rule.fields, dtype=np.uint64)
    cls = np.zeros(max(1, len(words)), dtype=np.uint8)
    check(fn(_ptr(words) if len(words) else None, len(words), words.shape[1], *middle, *rest, _ptr(counts), _ptr(cls) if classes else None))
    return (counts, cls[:len(words)]) if classes else counts


def ec_tally_host(words, rounds, r1, keys1, flips1, r2, keys2, flips2, ldr=None, classes=False):
    """gf2_ec_tally_host (host code, no GPU): the eight counts of the error-correction cycle's tally rule over outcome words
    (count, ldw); ldr (default ldw) is the cycle's 1 + rounds + F.  classes=True also returns the class byte of every sample."""
    words = _tally_words(words)
    return _tally_host(lib().gf2_ec_tally_host, EC_RULE, words, (words.shape[1] if ldr is None else int(ldr),), (rounds,),
                       (r1, keys1, flips1, r2, keys2, flips2), classes)


def ft_tally_host(words, nsteps, measure_mask, r1, keys1, flips1, r2, keys2, flips2, ldr=None, classes=False):
    """gf2_ft_tally_host (host code, no GPU): the seven counts of the logical measurement's tally rule over outcome words
    (count, ldw); ldr (default ldw) is the program's nsteps + F.  classes=True also returns the class byte of every sample."""
    words = _tally_words(words)
    return _tally_host(lib().gf2_ft_tally_host, FT_RULE, words, (words.shape[1] if ldr is None else int(ldr),), (nsteps, measure_mask),
                       (r1, keys1, flips1, r2, keys2, flips2), classes)


def _stream_sequence(type_eff, type_locations, type_flags, block_type, block_kind):
    """The arrays of a block sequence as the gf2_stream_* entry points take them, and their pointer arguments."""
    eff = np.ascontiguousarray(type_eff, dtype="<u8")
    if eff.ndim != 3 or eff.shape[1:] != (2, 3):
        raise ValueError("type_eff must be (locations of all types, 2, 3)")
    locs = np.ascontiguousarray(type_locations, dtype=np.int64).reshape(-1)
    flags = np.ascontiguousarray(type_flags, dtype=np.int64).reshape(-1)
    types = np.ascontiguousarray(block_type, dtype=np.int32).reshape(-1)
    kinds = np.ascontiguousarray(block_kind, dtype=np.int32).reshape(-1)
    if len(locs) != len(flags) or len(types) != len(kinds) or int(locs.sum()) != len(eff):
        raise ValueError("one location count and one flag count per type, one type and one kind per block, type_eff as long as the types")
    keep = (eff, locs, flags, types, kinds)
    return keep, (_ptr(eff), _ptr(locs), _ptr(flags), len(locs), _ptr(types), _ptr(kinds), len(kinds))


def stream_words_host(type_eff, type_locations, type_flags, block_type, block_kind, fault_first, fault_location, fault_kind, ldw):
    """gf2_stream_words_host (host code, no GPU): the (samples, ldw) stream-layout words of samples given by their faults -- sample i
    has faults fault_first[i] .. fault_first[i + 1] - 1, each a location and a kind 1 (X), 2 (Z) or 3 (Y)."""
    keep, seq = _stream_sequence(type_eff, type_locations, type_flags, block_type, block_kind)
    first = np.ascontiguousarray(fault_first, dtype=np.int64).reshape(-1)
    where = np.ascontiguousarray(fault_location, dtype=np.int32).reshape(-1)
    kind = np.ascontiguousarray(fault_kind, dtype=np.uint8).reshape(-1)
    count = len(first) - 1
    if count < 0 or len(where) != len(kind) or (count >= 0 and len(first) and int(first[-1]) != len(where)):
        raise ValueError("fault_first has one entry per sample and one more, the last the number of faults")
    out = np.zeros((max(1, count), max(1, int(ldw))), dtype="<u8")
    check(lib().gf2_stream_words_host(*seq, _ptr(first), _ptr(where) if len(where) else None, _ptr(kind) if len(where) else None, count,
                                      _ptr(out), int(ldw)))
    return out[:count]


def stream_tally_host(words, block_kind, flag_words, r1, keys1, flips1, r2, keys2, flips2, classes=False):
    """gf2_stream_tally_host (host code, no GPU): the twelve counts of the streamed tally rule over stream-layout words (count, ldw).
    classes=True also returns the class byte of every sample."""
    words = _tally_words(words)
    kinds = np.ascontiguousarray(block_kind, dtype=np.int32).reshape(-1)
    return _tally_host(lib().gf2_stream_tally_host, STREAM_RULE, words, (_ptr(kinds), len(kinds), int(flag_words)), (),
                       (r1, keys1, flips1, r2, keys2, flips2), classes)


def _mstream_sequence(type_eff, type_locations, type_flags, block_type, block_kind, block_a, block_b, nframes):
    """The arrays of a multi-block sequence as the gf2_mstream_* entry points take them, and their pointer arguments."""
    keep, seq = _stream_sequence(type_eff, type_locations, type_flags, block_type, block_kind)
    frames_a = np.ascontiguousarray(block_a, dtype=np.int32).reshape(-1)
    frames_b = np.ascontiguousarray(block_b, dtype=np.int32).reshape(-1)
    if len(frames_a) != len(keep[3]) or len(frames_b) != len(keep[3]):
        raise ValueError("one frame a and one frame b per block")
    return keep + (frames_a, frames_b), seq[:6] + (_ptr(frames_a), _ptr(frames_b), seq[6], int(nframes))


def mstream_words_host(type_eff, type_locations, type_flags, block_type, block_kind, block_a, block_b, nframes, fault_first, fault_location,
                       fault_kind, ldw):
    """gf2_mstream_words_host (host code, no GPU): the (samples, ldw) words of samples of a multi-block program given by their faults
    -- sample i has faults fault_first[i] .. fault_first[i + 1] - 1, each a location and a kind 1 (X), 2 (Z) or 3 (Y)."""
    keep, seq = _mstream_sequence(type_eff, type_locations, type_flags, block_type, block_kind, block_a, block_b, nframes)
    first = np.ascontiguousarray(fault_first, dtype=np.int64).reshape(-1)
    where = np.ascontiguousarray(fault_location, dtype=np.int32).reshape(-1)
    kind = np.ascontiguousarray(fault_kind, dtype=np.uint8).reshape(-1)
    count = len(first) - 1
    if count < 0 or len(where) != len(kind) or (count >= 0 and len(first) and int(first[-1]) != len(where)):
        raise ValueError("fault_first has one entry per sample and one more, the last the number of faults")
    out = np.zeros((max(1, count), max(1, int(ldw))), dtype="<u8")
    check(lib().gf2_mstream_words_host(*seq, _ptr(first), _ptr(where) if len(where) else None, _ptr(kind) if len(where) else None, count,
                                       _ptr(out), int(ldw)))
    return out[:count]


def mstream_tally_host(words, block_kind, block_a, block_b, nframes, flag_words, records, r1, keys1, flips1, r2, keys2, flips2, classes=False):
    """gf2_mstream_tally_host (host code, no GPU): the twenty counts of the multi-block tally rule over words (count, ldw).
    classes=True also returns the class byte of every sample."""
    words = _tally_words(words)
    kinds = np.ascontiguousarray(block_kind, dtype=np.int32).reshape(-1)
    frames_a = np.ascontiguousarray(block_a, dtype=np.int32).reshape(-1)
    frames_b = np.ascontiguousarray(block_b, dtype=np.int32).reshape(-1)
    if len(frames_a) != len(kinds) or len(frames_b) != len(kinds):
        raise ValueError("one frame a and one frame b per block")
    return _tally_host(lib().gf2_mstream_tally_host, MSTREAM_RULE, words,
                       (_ptr(kinds), _ptr(frames_a), _ptr(frames_b), len(kinds), int(nframes), int(flag_words), int(records)), (),
                       (r1, keys1, flips1, r2, keys2, flips2), classes)


def _retry_regions(type_regions, type_nregions, ntypes):
    """The regions of a sequence's block types as the gf2_retry_* entry points take them, and their pointer arguments."""
    regions = np.ascontiguousarray(type_regions, dtype=np.int64).reshape(-1, 3)
    counts = np.ascontiguousarray(type_nregions, dtype=np.int64).reshape(-1)
    if len(counts) != ntypes or int(counts.clip(0).sum()) != len(regions):
        raise ValueError("one region count per type, type_regions as long as their sum")
    return (regions, counts), (_ptr(regions) if len(regions) else None, _ptr(counts))


def retry_words_host(type_eff, type_locations, type_flags, block_type, block_kind, type_regions, type_nregions, seed, first, count, p_x, p_y, p_z,
                     max_attempts, ldw, preparations):
    """gf2_retry_words_host (host code, no GPU): the (count, ldw) words [steps] [flag words] [attempts] of samples [first, first +
    count) of the repeat-until-success sampler and the (count, preparations) uint32 attempts of every retried region."""
    keep, seq = _stream_sequence(type_eff, type_locations, type_flags, block_type, block_kind)
    keep_regions, regions = _retry_regions(type_regions, type_nregions, len(keep[1]))
    count = int(count)
    out = np.zeros((max(1, count), max(1, int(ldw))), dtype="<u8")
    attempts = np.zeros((max(1, count), max(1, int(preparations))), dtype=np.uint32)
    check(lib().gf2_retry_words_host(*seq, *regions, int(seed) & 0xFFFFFFFFFFFFFFFF, int(first), count, float(p_x), float(p_y), float(p_z),
                                     int(max_attempts), _ptr(out), int(ldw), _ptr(attempts)))
    return out[:max(0, count)], attempts[:max(0, count), :int(preparations)]


def mretry_words_host(type_eff, type_locations, type_flags, block_type, block_kind, block_a, block_b, nframes, type_regions, type_nregions, seed,
                      first, count, p_x, p_y, p_z, max_attempts, ldw, preparations):
    """gf2_mretry_words_host (host code, no GPU): the (count, ldw) words [steps] [flag words] [attempts] of samples [first, first +
    count) of the repeat-until-success sampler of a multi-block program and the (count, preparations) uint32 attempts of every
    retried region."""
    keep, seq = _mstream_sequence(type_eff, type_locations, type_flags, block_type, block_kind, block_a, block_b, nframes)
    keep_regions, regions = _retry_regions(type_regions, type_nregions, len(keep[1]))
    count = int(count)
    out = np.zeros((max(1, count), max(1, int(ldw))), dtype="<u8")
    attempts = np.zeros((max(1, count), max(1, int(preparations))), dtype=np.uint32)
    check(lib().gf2_mretry_words_host(*seq, *regions, int(seed) & 0xFFFFFFFFFFFFFFFF, int(first), count, float(p_x), float(p_y), float(p_z),
                                      int(max_attempts), _ptr(out), int(ldw), _ptr(attempts)))
    return out[:max(0, count)], attempts[:max(0, count), :int(preparations)]


def _retry_waits(wait_eff, wait_count, regions):
    """The wait rows of a sequence's regions as the gf2_retry_wait_* entry points take them, and their pointer arguments."""
    counts = np.ascontiguousarray(wait_count, dtype=np.int64).reshape(-1)
    eff = np.ascontiguousarray(wait_eff, dtype="<u8").reshape(-1, 2, 2)
    if len(counts) != regions or int(counts.clip(0).sum()) != len(eff):
        raise ValueError("one wait count per region, wait_eff (rows, 2, 2) as long as their sum")
    return (eff, counts), (_ptr(eff) if len(eff) else None, _ptr(counts) if len(counts) else None)


def retry_wait_words_host(type_eff, type_locations, type_flags, block_type, block_kind, type_regions, type_nregions, wait_eff, wait_count, seed,
                          first, count, p_x, p_y, p_z, q_x, q_y, q_z, max_attempts, ldw, preparations):
    """gf2_retry_wait_words_host (host code, no GPU): the (count, ldw) words [steps] [flag words] [attempts] [wait faults] of samples
    [first, first + count) of the repeat-until-success sampler with waiting faults and the (count, preparations) uint32 attempts
    of every retried region."""
    keep, seq = _stream_sequence(type_eff, type_locations, type_flags, block_type, block_kind)
    keep_regions, regions = _retry_regions(type_regions, type_nregions, len(keep[1]))
    keep_waits, waits = _retry_waits(wait_eff, wait_count, len(keep_regions[0]))
    count = int(count)
    out = np.zeros((max(1, count), max(1, int(ldw))), dtype="<u8")
    attempts = np.zeros((max(1, count), max(1, int(preparations))), dtype=np.uint32)
    check(lib().gf2_retry_wait_words_host(*seq, *regions, *waits, int(seed) & 0xFFFFFFFFFFFFFFFF, int(first), count, float(p_x), float(p_y),
                                          float(p_z), float(q_x), float(q_y), float(q_z), int(max_attempts), _ptr(out), int(ldw), _ptr(attempts)))
    return out[:max(0, count)], attempts[:max(0, count), :int(preparations)]


def _retry_sites(site_loc, site_regions, regions):
    """The site table of a sequence's regions as the gf2_retry_gate_* entry points take it, and its pointer arguments."""
    counts = np.ascontiguousarray(site_regions, dtype=np.int64).reshape(-1, 2)
    loc = np.ascontiguousarray(site_loc, dtype=np.int32).reshape(-1)
    if len(counts) != regions or int(counts.clip(0).sum()) != len(loc):
        raise ValueError("one (n_1, n_2) per region, site_loc as long as their sum")
    keep = (np.concatenate([loc, np.zeros(1, dtype=np.int32)]), counts)             # (never empty: a pointer to pass)
    return keep, (_ptr(keep[0]), _ptr(counts) if len(counts) else None)


def retry_gate_words_host(type_eff, type_locations, type_flags, block_type, block_kind, type_regions, type_nregions, site_loc, site_regions, seed,
                          first, count, p1, p2, max_attempts, ldw, preparations):
    """gf2_retry_gate_words_host (host code, no GPU): the (count, ldw) words [steps] [flag words] [attempts] of samples [first, first +
    count) of the repeat-until-success sampler under gate-level faults and the (count, preparations) uint32 attempts of every
    retried region."""
    keep, seq = _stream_sequence(type_eff, type_locations, type_flags, block_type, block_kind)
    keep_regions, regions = _retry_regions(type_regions, type_nregions, len(keep[1]))
    keep_sites, sites = _retry_sites(site_loc, site_regions, len(keep_regions[0]))
    count = int(count)
    out = np.zeros((max(1, count), max(1, int(ldw))), dtype="<u8")
    attempts = np.zeros((max(1, count), max(1, int(preparations))), dtype=np.uint32)
    check(lib().gf2_retry_gate_words_host(*seq, *regions, *sites, int(seed) & 0xFFFFFFFFFFFFFFFF, int(first), count, float(p1), float(p2),
                                          int(max_attempts), _ptr(out), int(ldw), _ptr(attempts)))
    return out[:max(0, count)], attempts[:max(0, count), :int(preparations)]


def mretry_gate_words_host(type_eff, type_locations, type_flags, block_type, block_kind, block_a, block_b, nframes, type_regions, type_nregions,
                           site_loc, site_regions, seed, first, count, p1, p2, max_attempts, ldw, preparations):
    """gf2_mretry_gate_words_host (host code, no GPU): the (count, ldw) words [steps] [flag words] [attempts] of samples [first, first
    + count) of the repeat-until-success sampler of a multi-block program under gate-level faults and the (count, preparations)
    uint32 attempts of every retried region."""
    keep, seq = _mstream_sequence(type_eff, type_locations, type_flags, block_type, block_kind, block_a, block_b, nframes)
    keep_regions, regions = _retry_regions(type_regions, type_nregions, len(keep[1]))
    keep_sites, sites = _retry_sites(site_loc, site_regions, len(keep_regions[0]))
    count = int(count)
    out = np.zeros((max(1, count), max(1, int(ldw))), dtype="<u8")
    attempts = np.zeros((max(1, count), max(1, int(preparations))), dtype=np.uint32)
    check(lib().gf2_mretry_gate_words_host(*seq, *regions, *sites, int(seed) & 0xFFFFFFFFFFFFFFFF, int(first), count, float(p1), float(p2),
                                           int(max_attempts), _ptr(out), int(ldw), _ptr(attempts)))
    return out[:max(0, count)], attempts[:max(0, count), :int(preparations)]


def retry_gate_wait_words_host(type_eff, type_locations, type_flags, block_type, block_kind, type_regions, type_nregions, site_loc, site_regions,
                               wait_eff, wait_count, seed, first, count, p1, p2, q_x, q_y, q_z, max_attempts, ldw, preparations):
    """gf2_retry_gate_wait_words_host (host code, no GPU): the (count, ldw) words [steps] [flag words] [attempts] [wait faults] of
    samples [first, first + count) of the repeat-until-success sampler under gate-level faults with waiting faults and the (count,
    preparations) uint32 attempts of every retried region."""
    keep, seq = _stream_sequence(type_eff, type_locations, type_flags, block_type, block_kind)
    keep_regions, regions = _retry_regions(type_regions, type_nregions, len(keep[1]))
    keep_sites, sites = _retry_sites(site_loc, site_regions, len(keep_regions[0]))
    keep_waits, waits = _retry_waits(wait_eff, wait_count, len(keep_regions[0]))
    count = int(count)
    out = np.zeros((max(1, count), max(1, int(ldw))), dtype="<u8")
    attempts = np.zeros((max(1, count), max(1, int(preparations))), dtype=np.uint32)
    check(lib().gf2_retry_gate_wait_words_host(*seq, *regions, *sites, *waits, int(seed) & 0xFFFFFFFFFFFFFFFF, int(first), count, float(p1),
                                               float(p2), float(q_x), float(q_y), float(q_z), int(max_attempts), _ptr(out), int(ldw),
                                               _ptr(attempts)))
    return out[:max(0, count)], attempts[:max(0, count), :int(preparations)]


def stratum_errors(nb, w, count, kinds=(1, 1, 1), seed=0, first=0):
    """gf2_stratum_errors (host code, no GPU): the packed (e_x, e_z) rows, count x words(nb) each, of samples [first, first + count)
    of the stratum of weight w over nb positions (DESIGN.md "Strata")."""
    count = int(count)
    ld = max(1, words_for(nb))
    ex = np.zeros((max(1, count), ld), dtype="<u8")
    ez = np.zeros_like(ex)
    k_x, k_y, k_z = (float(k) for k in kinds)
    check(lib().gf2_stratum_errors(int(nb), int(w), int(seed) & 0xFFFFFFFFFFFFFFFF, int(first), count, k_x, k_y, k_z, _ptr(ex), _ptr(ez), ld))
    return ex[:count], ez[:count]


def stratum_outcomes_host(eff, w, count, kinds=(1, 1, 1), seed=0, first=0, ldw=None):
    """gf2_stratum_outcomes_host (host code, no GPU): the (count, ldw) outcome words of samples [first, first + count) of the stratum
    of weight w over the L locations of an effect table eff, (L, 2, ldr) as circuit_effects_timed returns it; ldw (default ldr) words
    per sample, those past ldr zero here."""
    eff, table = _effects(eff)
    count = int(count)
    ldw = eff.shape[2] if ldw is None else int(ldw)
    out = np.zeros((max(1, count), max(1, ldw)), dtype="<u8")
    k_x, k_y, k_z = (float(k) for k in kinds)
    check(lib().gf2_stratum_outcomes_host(*table, int(w), int(seed) & 0xFFFFFFFFFFFFFFFF, int(first), count, k_x, k_y, k_z, _ptr(out), ldw))
    return out[:max(0, count)]


def _strata_arrays(weights, counts, fields=5):
    weights = np.ascontiguousarray(weights, dtype=np.int32).reshape(-1)
    counts = np.ascontiguousarray(counts, dtype=np.int64).reshape(-1)
    if weights.shape != counts.shape:
        raise ValueError("one sample count per stratum")
    return weights, counts, np.zeros((len(weights), fields), dtype=np.uint64)


def subset_unrank(nb, w, rank):
    """gf2_subset_unrank (host code): the w positions, ascending, of the subset of [0, nb) whose rank in the combinatorial number
    system, sum_k C(s_k, k + 1), is `rank` (DESIGN.md "Exact strata")."""
    if not -(1 << 63) <= int(rank) < (1 << 63):
        raise GF2Error(GF2_E_ARG, "gf2_subset_unrank: the rank does not fit 63 bits")
    out = np.zeros(max(1, int(w)), dtype=np.int32)
    check(lib().gf2_subset_unrank(int(nb), int(w), int(rank), _ptr(out)))
    return out[:max(0, int(w))]


def _enumerate(fn, rule, front, head, tables, w, first_rank, count):
    """A gf2_*_enumerate(_host) entry point; front: (context, circuit) handles, or _effects' arguments for a host statement."""
    keep, rest = _rule_arguments(rule, head, tables)
    side = max(0, min(int(w), ENUMERATE_MAX_WEIGHT)) + 1
    out = np.zeros((side, side, rule.fields), dtype=np.uint64)
    check(fn(*front, *rest, int(w), int(first_rank), int(count), _ptr(out)))
    return out


def circuit_enumerate_host(eff, r1, keys1, flips1, r2, keys2, flips2, w, first_rank, count):
    """gf2_circuit_enumerate_host (host code, no GPU): the (w + 1, w + 1, 5) uint64 counts [n_x][n_y][field] over the subsets of
    ranks [first_rank, first_rank + count), each with all 3^w kind assignments.  eff: (L, 2, ldr) as circuit_effects returns it."""
    eff, table = _effects(eff)
    return _enumerate(lib().gf2_circuit_enumerate_host, CIRCUIT_RULE, table, (), (r1, keys1, flips1, r2, keys2, flips2), w, first_rank, count)


def ec_enumerate_host(eff, rounds, r1, keys1, flips1, r2, keys2, flips2, w, first_rank, count):
    """gf2_ec_enumerate_host (host code, no GPU): the (w + 1, w + 1, 8) uint64 counts [n_x][n_y][field] of the error-correction
    cycle's tally rule over the subsets of ranks [first_rank, first_rank + count), each with all 3^w kind assignments."""
    eff, table = _effects(eff)
    return _enumerate(lib().gf2_ec_enumerate_host, EC_RULE, table, (rounds,), (r1, keys1, flips1, r2, keys2, flips2), w, first_rank, count)


def ft_enumerate_host(eff, nsteps, measure_mask, r1, keys1, flips1, r2, keys2, flips2, w, first_rank, count):
    """gf2_ft_enumerate_host (host code, no GPU): the (w + 1, w + 1, 7) counts of the logical measurement's tally rule, likewise."""
    eff, table = _effects(eff)
    return _enumerate(lib().gf2_ft_enumerate_host, FT_RULE, table, (nsteps, measure_mask), (r1, keys1, flips1, r2, keys2, flips2), w,
                      first_rank, count)


def _gate_sites(site_loc, n1, n2):
    sites = np.ascontiguousarray(site_loc, dtype=np.int32).reshape(-1)
    if len(sites) != int(n1) + int(n2):
        raise ValueError("site_loc must have n1 + n2 entries")
    return sites


def _gate_arguments(rule, head, tables, sites):
    """_rule_arguments followed by the site table (site_loc, n1, n2) of the gate-level fault model."""
    keep, rest = _rule_arguments(rule, head, tables)
    site_loc, n1, n2 = sites
    site_loc = _gate_sites(site_loc, n1, n2)
    return (keep, site_loc), rest + (_ptr(site_loc), int(n1), int(n2))


def _gate_enumerate(fn, rule, front, head, tables, sites, w, b, first_rank, count):
    """A gf2_*_gate_enumerate(_host) entry point; front as _enumerate's."""
    keep, rest = _gate_arguments(rule, head, tables, sites)
    out = np.zeros((max(0, min(int(b), GATE_ENUMERATE_MAX_WEIGHT)) + 1, rule.fields), dtype=np.uint64)
    check(fn(*front, *rest, int(w), int(b), int(first_rank), int(count), _ptr(out)))
    return out


def ec_gate_enumerate_host(eff, rounds, r1, keys1, flips1, r2, keys2, flips2, site_loc, n1, n2, w, b, first_rank, count):
    """gf2_ec_gate_enumerate_host (host code, no GPU): the (b + 1, 8) uint64 counts [c][field] of the error-correction cycle's tally
    rule over the site subsets of ranks [first_rank, first_rank + count) of (w, b), each with all 3^(w - b) 15^b kind assignments."""
    eff, table = _effects(eff)
    return _gate_enumerate(lib().gf2_ec_gate_enumerate_host, EC_RULE, table, (rounds,), (r1, keys1, flips1, r2, keys2, flips2),
                           (site_loc, n1, n2), w, b, first_rank, count)


def ft_gate_enumerate_host(eff, nsteps, measure_mask, r1, keys1, flips1, r2, keys2, flips2, site_loc, n1, n2, w, b, first_rank, count):
    """gf2_ft_gate_enumerate_host (host code, no GPU): the (b + 1, 7) counts of the logical measurement's tally rule, likewise."""
    eff, table = _effects(eff)
    return _gate_enumerate(lib().gf2_ft_gate_enumerate_host, FT_RULE, table, (nsteps, measure_mask), (r1, keys1, flips1, r2, keys2, flips2),
                           (site_loc, n1, n2), w, b, first_rank, count)


def gate_stratum_outcomes_host(eff, site_loc, n1, n2, a, b, count, seed=0, first=0, ldw=None):
    """gf2_gate_stratum_outcomes_host (host code, no GPU): (words, c) of samples [first, first + count) of the stratum of a faulty
    one-operand gates and b faulty CNOTs among the sites of an effect table eff, (L, 2, ldr): the (count, ldw) outcome words (ldw
    defaults to ldr; the words past ldr zero here) and the (count,) uint8 number of two-operand kinds per sample."""
    eff, table = _effects(eff)
    site_loc = _gate_sites(site_loc, n1, n2)
    count = int(count)
    ldw = eff.shape[2] if ldw is None else int(ldw)
    out = np.zeros((max(1, count), max(1, ldw)), dtype="<u8")
    two = np.zeros(max(1, count), dtype=np.uint8)
    check(lib().gf2_gate_stratum_outcomes_host(*table, _ptr(site_loc), int(n1), int(n2), int(a), int(b), int(seed) & 0xFFFFFFFFFFFFFFFF,
                                               int(first), count, _ptr(out), ldw, _ptr(two)))
    return out[:max(0, count)], two[:max(0, count)]


def gate_outcomes_host(eff, site_loc, n1, n2, count, p1, p2, seed=0, first=0, ldw=None, faults=True):
    """gf2_gate_outcomes_host (host code, no GPU): (words, faults) of samples [first, first + count) of the direct Monte-Carlo under
    gate-level faults -- every one-operand site of an effect table eff, (L, 2, ldr), fails with probability p1, every CNOT site with
    p2: the (count, ldw) outcome words (ldw defaults to ldr; the words past ldr zero here) and the (count, 3) int32 numbers (a, b, c)
    of faulty one-operand gates, faulty CNOTs and two-operand kinds per sample (None with faults=False)."""
    eff, table = _effects(eff)
    site_loc = _gate_sites(site_loc, n1, n2)
    count = int(count)
    ldw = eff.shape[2] if ldw is None else int(ldw)
    out = np.zeros((max(1, count), max(1, ldw)), dtype="<u8")
    abc = np.zeros((max(1, count), 3), dtype=np.int32) if faults else None
    check(lib().gf2_gate_outcomes_host(*table, _ptr(site_loc), int(n1), int(n2), int(seed) & 0xFFFFFFFFFFFFFFFF, int(first), count,
                                       float(p1), float(p2), _ptr(out), ldw, _ptr(abc) if faults else None))
    return out[:max(0, count)], (abc[:max(0, count)] if faults else None)


def _gate_strata_arrays(strata, counts, fields):
    strata = np.ascontiguousarray(strata, dtype=np.int32).reshape(-1, 2)
    counts = np.ascontiguousarray(counts, dtype=np.int64).reshape(-1)
    if len(strata) != len(counts):
        raise ValueError("one sample count per stratum")
    return (np.ascontiguousarray(strata[:, 0]), np.ascontiguousarray(strata[:, 1]), counts,
            np.zeros((len(counts), GATE_STRATUM_MAX_WEIGHT + 1, fields), dtype=np.uint64))


def _enumerate_list(fn, rule, front, head, tables, w, first_rank, count, select, capacity, limit=None):
    """A gf2_*_enumerate_list(_host) entry point, front as _enumerate's: (found, records) -- records the (found, 2) uint64 words, or
    None when `capacity` records (0: just count) do not hold them.  limit: the capacity above which the entry point refuses the call."""
    keep, rest = _rule_arguments(rule, head, tables)
    capacity = int(capacity)
    records = np.zeros((max(1, capacity if limit is None else min(capacity, limit)), FAULT_RECORD_WORDS), dtype="<u8")
    found = _c_i64(0)
    check(fn(*front, *rest, int(w), int(first_rank), int(count), int(select) & 0xFFFFFFFFFFFFFFFF, capacity,
             _ptr(records) if capacity > 0 else None, ctypes.byref(found)))
    found = int(found.value)
    return found, (records[:found].copy() if found <= capacity else None)


def ec_enumerate_list_host(eff, rounds, r1, keys1, flips1, r2, keys2, flips2, w, first_rank, count, select, capacity):
    """gf2_ec_enumerate_list_host (host code, no GPU): (found, records) of the error-correction cycle over the subsets of ranks
    [first_rank, first_rank + count) -- found, the number of accepted configurations whose class byte has a bit of `select`;
    records, their (found, 2) uint64 words sorted by (rank, kinds code), or None when `capacity` records do not hold them."""
    eff, table = _effects(eff)
    return _enumerate_list(lib().gf2_ec_enumerate_list_host, EC_RULE, table, (rounds,), (r1, keys1, flips1, r2, keys2, flips2), w, first_rank,
                           count, select, capacity)


def ft_enumerate_list_host(eff, nsteps, measure_mask, r1, keys1, flips1, r2, keys2, flips2, w, first_rank, count, select, capacity):
    """gf2_ft_enumerate_list_host (host code, no GPU): (found, records) of the logical measurement, likewise."""
    eff, table = _effects(eff)
    return _enumerate_list(lib().gf2_ft_enumerate_list_host, FT_RULE, table, (nsteps, measure_mask), (r1, keys1, flips1, r2, keys2, flips2),
                           w, first_rank, count, select, capacity)


def _gate_enumerate_list(fn, rule, front, head, tables, sites, w, b, first_rank, count, select, capacity, limit=None, into=None):
    """A gf2_*_gate_enumerate_list(_host) entry point, front as _enumerate's: (found, records) as _enumerate_list gives them, the
    records' word 1 holding a kind mask per pick.  into: a C-contiguous uint64 array of at least `capacity` records that the entry
    point writes in place of a fresh one (the records returned are then a view of it)."""
    keep, rest = _gate_arguments(rule, head, tables, sites)
    capacity = int(capacity)
    if into is None:
        records = np.zeros((max(1, capacity if limit is None else min(capacity, limit)), FAULT_RECORD_WORDS), dtype="<u8")
    else:
        records = into
        if records.dtype != np.dtype("<u8") or not records.flags.c_contiguous or records.size < FAULT_RECORD_WORDS * max(0, capacity):
            raise ValueError("into must be a C-contiguous uint64 array of at least capacity records")
        records = records.reshape(-1)[:records.size // FAULT_RECORD_WORDS * FAULT_RECORD_WORDS].reshape(-1, FAULT_RECORD_WORDS)
    found = _c_i64(0)
    check(fn(*front, *rest, int(w), int(b), int(first_rank), int(count), int(select) & 0xFFFFFFFFFFFFFFFF, capacity,
             _ptr(records) if capacity > 0 else None, ctypes.byref(found)))
    found = int(found.value)
    if found > capacity:
        return found, None
    return found, (records[:found].copy() if into is None else records[:found])


def ec_gate_enumerate_list_host(eff, rounds, r1, keys1, flips1, r2, keys2, flips2, site_loc, n1, n2, w, b, first_rank, count, select, capacity,
                                into=None):
    """gf2_ec_gate_enumerate_list_host (host code, no GPU): (found, records) of the error-correction cycle over the site subsets of
    ranks [first_rank, first_rank + count) of (w, b) -- found, the number of accepted configurations whose class byte has a bit of
    `select`; records, their (found, 2) uint64 words sorted by (rank, kind masks), or None when `capacity` records do not hold them."""
    eff, table = _effects(eff)
    return _gate_enumerate_list(lib().gf2_ec_gate_enumerate_list_host, EC_RULE, table, (rounds,), (r1, keys1, flips1, r2, keys2, flips2),
                                (site_loc, n1, n2), w, b, first_rank, count, select, capacity, into=into)


def ft_gate_enumerate_list_host(eff, nsteps, measure_mask, r1, keys1, flips1, r2, keys2, flips2, site_loc, n1, n2, w, b, first_rank, count,
                                select, capacity, into=None):
    """gf2_ft_gate_enumerate_list_host (host code, no GPU): (found, records) of the logical measurement, likewise."""
    eff, table = _effects(eff)
    return _gate_enumerate_list(lib().gf2_ft_gate_enumerate_list_host, FT_RULE, table, (nsteps, measure_mask),
                                (r1, keys1, flips1, r2, keys2, flips2), (site_loc, n1, n2), w, b, first_rank, count, select, capacity, into=into)


def _decode(fn, rule, front, head, tables, seed, first, count, p_x, p_y, p_z, *more, null_flips=False):
    """A gf2_mc_*_decode entry point: the rule's counts over samples [first, first + count); more: its arguments after p_z."""
    keep, rest = _rule_arguments(rule, head, tables, null_flips)
    counts = np.zeros(rule.fields, dtype=np.uint64)
    check(fn(*front, *rest, seed & 0xFFFFFFFFFFFFFFFF, first, count, p_x, p_y, p_z, *more, _ptr(counts)))
    return counts


def _decode_strata(fn, rule, front, head, tables, seed, first, weights, counts, k_x, k_y, k_z):
    """A gf2_mc_*_decode_strata entry point: the (nstrata, fields) counts."""
    keep, rest = _rule_arguments(rule, head, tables)
    weights, counts, out = _strata_arrays(weights, counts, rule.fields)
    check(fn(*front, *rest, seed & 0xFFFFFFFFFFFFFFFF, first, len(weights), _ptr(weights), _ptr(counts), k_x, k_y, k_z, _ptr(out)))
    return out


def _decode_gate_strata(fn, rule, front, head, tables, sites, seed, first, strata, counts):
    """A gf2_mc_*_decode_gate_strata entry point: the (nstrata, 17, fields) counts [stratum][c][field]."""
    keep, rest = _gate_arguments(rule, head, tables, sites)
    wa, wb, counts, out = _gate_strata_arrays(strata, counts, rule.fields)
    check(fn(*front, *rest, int(seed) & 0xFFFFFFFFFFFFFFFF, int(first), len(counts), _ptr(wa), _ptr(wb), _ptr(counts), _ptr(out)))
    return out


def _decode_gate(fn, rule, front, head, tables, sites, seed, first, count, p1, p2):
    """A gf2_mc_*_decode_gate entry point: the rule's counts over samples [first, first + count)."""
    keep, rest = _gate_arguments(rule, head, tables, sites)
    counts = np.zeros(rule.fields, dtype=np.uint64)
    check(fn(*front, *rest, int(seed) & 0xFFFFFFFFFFFFFFFF, int(first), int(count), float(p1), float(p2), _ptr(counts)))
    return counts


# ---- context ----------------------------------------------------------------------------------------------

class DeviceBuffer(object):
    """Device memory owned by a Context."""

    def __init__(self, ctx, nbytes):
        self.ctx = ctx
        self.nbytes = int(nbytes)
        out = ctypes.c_void_p()
        check(lib().gf2_dev_alloc(ctx.handle, self.nbytes, ctypes.byref(out)))
        self.ptr = out.value

    def upload(self, arr):
        arr = np.ascontiguousarray(arr)
        if arr.nbytes > self.nbytes:
            raise ValueError("upload larger than the buffer")
        check(lib().gf2_h2d(self.ctx.handle, self.ptr, _ptr(arr), arr.nbytes))
        return self

    def download(self, shape, dtype):
        out = np.empty(shape, dtype=dtype)
        if out.nbytes > self.nbytes:
            raise ValueError("download larger than the buffer")
        check(lib().gf2_d2h(self.ctx.handle, _ptr(out), self.ptr, out.nbytes))
        return out

    def zero(self):
        check(lib().gf2_dev_zero(self.ctx.handle, self.ptr, self.nbytes))
        return self

    def view(self, offset, nbytes):
        """A window of this buffer (same upload / download / zero interface; the parent keeps the memory)."""
        if offset < 0 or nbytes < 0 or offset + nbytes > self.nbytes:
            raise ValueError("view outside the buffer")
        return DeviceView(self, int(offset), int(nbytes))

    def free(self):
        if self.ptr:
            check(lib().gf2_dev_free(self.ctx.handle, self.ptr))
            self.ptr = None

    def __del__(self):
        try:
            if self.ptr and self.ctx.handle:
                lib().gf2_dev_free(self.ctx.handle, self.ptr)
        except Exception:
            pass


class DeviceView(DeviceBuffer):
    """Part of a DeviceBuffer: owns nothing."""

    def __init__(self, parent, offset, nbytes):
        self.ctx, self.parent, self.nbytes = parent.ctx, parent, nbytes
        self.ptr = parent.ptr + offset

    def free(self):
        self.ptr = None

    def __del__(self):
        pass


class _Handle(object):
    """An object on the device, owned by a Context: `ctx`, `handle`, and the name of the entry point that destroys it."""
    _destroy = None

    def free(self):
        if self.handle:
            check(getattr(lib(), self._destroy)(self.ctx.handle, self.handle))
            self.handle = None

    def __del__(self):
        try:
            if self.handle and self.ctx.handle:
                getattr(lib(), self._destroy)(self.ctx.handle, self.handle)
        except Exception:
            pass


class Check(_Handle):
    """A parity-check matrix prepared on the device (gf2_check_create)."""
    _destroy = "gf2_check_destroy"

    def __init__(self, ctx, packed, r, n):
        self.ctx = ctx
        self.r, self.n = int(r), int(n)
        packed = np.ascontiguousarray(packed, dtype="<u8")
        out = ctypes.c_void_p()
        ld = packed.shape[1] if packed.ndim == 2 and packed.shape[0] else max(1, words_for(n))
        check(lib().gf2_check_create(ctx.handle, _ptr(packed), self.r, self.n, ld, ctypes.byref(out)))
        self.handle = out.value

    @property
    def slabs(self):
        return max(1, words_for(self.r))



class Circuit(_Handle):
    """The effect table of a circuit's fault locations on the device (gf2_circuit_create).  eff: (L, 2, ldr) packed words."""
    _destroy = "gf2_circuit_destroy"

    def __init__(self, ctx, eff, ft=False):
        self.ctx = ctx
        eff = np.ascontiguousarray(eff, dtype="<u8")
        if eff.ndim != 3 or eff.shape[1] != 2:
            raise ValueError("effects must be an (L, 2, ldr) array")
        self.locations, self.ldr = int(eff.shape[0]), int(eff.shape[2])
        out = ctypes.c_void_p()
        create = lib().gf2_ft_circuit_create if ft else lib().gf2_circuit_create             # (ft: up to FT_MAX_LDR words)
        check(create(ctx.handle, _ptr(eff), self.locations, self.ldr, ctypes.byref(out)))
        self.handle = out.value



class Stream(_Handle):
    """A block sequence on the device (gf2_stream_create): the block types' tables (locations of all types, 2, 3) and the blocks."""
    _destroy = "gf2_stream_destroy"

    def __init__(self, ctx, type_eff, type_locations, type_flags, block_type, block_kind):
        self.ctx = ctx
        keep, seq = _stream_sequence(type_eff, type_locations, type_flags, block_type, block_kind)
        out = ctypes.c_void_p()
        check(lib().gf2_stream_create(ctx.handle, *seq, ctypes.byref(out)))
        self.handle = out.value



class MStream(_Handle):
    """A multi-block sequence on the device (gf2_mstream_create): the block types' tables and the blocks (type, kind, a, b)."""
    _destroy = "gf2_mstream_destroy"

    def __init__(self, ctx, type_eff, type_locations, type_flags, block_type, block_kind, block_a, block_b, nframes):
        self.ctx = ctx
        keep, seq = _mstream_sequence(type_eff, type_locations, type_flags, block_type, block_kind, block_a, block_b, nframes)
        out = ctypes.c_void_p()
        check(lib().gf2_mstream_create(ctx.handle, *seq, ctypes.byref(out)))
        self.handle = out.value



class Retry(_Handle):
    """A block sequence and its regions on the device (gf2_retry_create)."""
    _destroy = "gf2_retry_destroy"

    def __init__(self, ctx, type_eff, type_locations, type_flags, block_type, block_kind, type_regions, type_nregions):
        self.ctx = ctx
        keep, seq = _stream_sequence(type_eff, type_locations, type_flags, block_type, block_kind)
        keep_regions, regions = _retry_regions(type_regions, type_nregions, len(keep[1]))
        out = ctypes.c_void_p()
        check(lib().gf2_retry_create(ctx.handle, *seq, *regions, ctypes.byref(out)))
        self.handle = out.value



class MRetry(_Handle):
    """A multi-block sequence and its regions on the device (gf2_mretry_create)."""
    _destroy = "gf2_mretry_destroy"

    def __init__(self, ctx, type_eff, type_locations, type_flags, block_type, block_kind, block_a, block_b, nframes, type_regions, type_nregions):
        self.ctx = ctx
        keep, seq = _mstream_sequence(type_eff, type_locations, type_flags, block_type, block_kind, block_a, block_b, nframes)
        keep_regions, regions = _retry_regions(type_regions, type_nregions, len(keep[1]))
        out = ctypes.c_void_p()
        check(lib().gf2_mretry_create(ctx.handle, *seq, *regions, ctypes.byref(out)))
        self.handle = out.value



class MRetryGate(_Handle):
    """A multi-block sequence, its regions and their sites on the device (gf2_mretry_gate_create)."""
    _destroy = "gf2_mretry_gate_destroy"

    def __init__(self, ctx, type_eff, type_locations, type_flags, block_type, block_kind, block_a, block_b, nframes, type_regions, type_nregions,
                 site_loc, site_regions):
        self.ctx = ctx
        keep, seq = _mstream_sequence(type_eff, type_locations, type_flags, block_type, block_kind, block_a, block_b, nframes)
        keep_regions, regions = _retry_regions(type_regions, type_nregions, len(keep[1]))
        keep_sites, sites = _retry_sites(site_loc, site_regions, len(keep_regions[0]))
        out = ctypes.c_void_p()
        check(lib().gf2_mretry_gate_create(ctx.handle, *seq, *regions, *sites, ctypes.byref(out)))
        self.handle = out.value



class RetryWait(_Handle):
    """A block sequence, its regions and their wait rows on the device (gf2_retry_wait_create)."""
    _destroy = "gf2_retry_wait_destroy"

    def __init__(self, ctx, type_eff, type_locations, type_flags, block_type, block_kind, type_regions, type_nregions, wait_eff, wait_count):
        self.ctx = ctx
        keep, seq = _stream_sequence(type_eff, type_locations, type_flags, block_type, block_kind)
        keep_regions, regions = _retry_regions(type_regions, type_nregions, len(keep[1]))
        keep_waits, waits = _retry_waits(wait_eff, wait_count, len(keep_regions[0]))
        out = ctypes.c_void_p()
        check(lib().gf2_retry_wait_create(ctx.handle, *seq, *regions, *waits, ctypes.byref(out)))
        self.handle = out.value



class RetryGate(_Handle):
    """A block sequence, its regions and their sites on the device (gf2_retry_gate_create)."""
    _destroy = "gf2_retry_gate_destroy"

    def __init__(self, ctx, type_eff, type_locations, type_flags, block_type, block_kind, type_regions, type_nregions, site_loc, site_regions):
        self.ctx = ctx
        keep, seq = _stream_sequence(type_eff, type_locations, type_flags, block_type, block_kind)
        keep_regions, regions = _retry_regions(type_regions, type_nregions, len(keep[1]))
        keep_sites, sites = _retry_sites(site_loc, site_regions, len(keep_regions[0]))
        out = ctypes.c_void_p()
        check(lib().gf2_retry_gate_create(ctx.handle, *seq, *regions, *sites, ctypes.byref(out)))
        self.handle = out.value



class RetryGateWait(_Handle):
    """A block sequence, its regions, their sites and their wait rows on the device (gf2_retry_gate_wait_create)."""
    _destroy = "gf2_retry_gate_wait_destroy"

    def __init__(self, ctx, type_eff, type_locations, type_flags, block_type, block_kind, type_regions, type_nregions, site_loc, site_regions,
                 wait_eff, wait_count):
        self.ctx = ctx
        keep, seq = _stream_sequence(type_eff, type_locations, type_flags, block_type, block_kind)
        keep_regions, regions = _retry_regions(type_regions, type_nregions, len(keep[1]))
        keep_sites, sites = _retry_sites(site_loc, site_regions, len(keep_regions[0]))
        keep_waits, waits = _retry_waits(wait_eff, wait_count, len(keep_regions[0]))
        out = ctypes.c_void_p()
        check(lib().gf2_retry_gate_wait_create(ctx.handle, *seq, *regions, *sites, *waits, ctypes.byref(out)))
        self.handle = out.value



class Context(object):
    """One HIP stream on one MI355X (gf2_ctx)."""

    def __init__(self, device=0):
        out = ctypes.c_void_p()
        check(lib().gf2_ctx_create(int(device), ctypes.byref(out)))
        self.handle = out.value
        self.device = int(device)

    def close(self):
        if self.handle:
            lib().gf2_ctx_destroy(self.handle)
            self.handle = None

    def sync(self):
        check(lib().gf2_ctx_sync(self.handle))

    def alloc(self, nbytes):
        return DeviceBuffer(self, nbytes)

    def outcomes(self, fill, obj, seed, first, count, p_x, p_y, p_z, ldo, *more):
        """The (count, ldo) uint64 words of samples [first, first + count) that `fill` -- this context's circuit_outcomes_dev,
        ft_outcomes_dev, stream_outcomes_dev, retry_outcomes_dev (more: its max_attempts) or retry_wait_outcomes_dev (more: the q rates
        and max_attempts) -- writes for `obj`, through a device buffer that is freed whether the call succeeds or raises."""
        count = int(count)
        buf = self.alloc(max(1, count) * ldo * 8)
        try:
            fill(obj, int(seed), int(first), count, float(p_x), float(p_y), float(p_z), *more, buf, ldo)
            return buf.download((count, ldo), np.uint64)
        finally:
            buf.free()

    def fill_workspace(self, byte):
        """Testing: every byte of the four workspace slots set to `byte`; returns the slots' sizes in bytes."""
        sizes = np.zeros(4, dtype=np.int64)
        check(lib().gf2_ctx_fill_workspace(self.handle, int(byte), _ptr(sizes)))
        return [int(v) for v in sizes]

    # -- routing ----------------------------------------------------------------------------------------
    def get_flags(self):
        out = ctypes.c_uint32(0)
        check(lib().gf2_ctx_get_flags(self.handle, ctypes.byref(out)))
        return int(out.value)

    def set_flags(self, flags):
        check(lib().gf2_ctx_set_flags(self.handle, int(flags)))

    @contextlib.contextmanager
    def flags(self, extra):
        """`with ctx.flags(F_SPARSE_SLABS): ...` forces a route (GF2_F_*) for the calls inside."""
        before = self.get_flags()
        self.set_flags(before | int(extra))
        try:
            yield self
        finally:
            self.set_flags(before)

    def set_option(self, option, value):
        check(lib().gf2_ctx_set_option(self.handle, int(option), -1 if value is None else int(value)))

    # -- timing ---------------------------------------------------------------------------------------
    def timer_start(self):
        check(lib().gf2_timer_start(self.handle))

    def timer_stop(self):
        ms = ctypes.c_float(0)
        check(lib().gf2_timer_stop(self.handle, ctypes.byref(ms)))
        return float(ms.value)

    def profile(self, on):
        check(lib().gf2_profile_enable(self.handle, 1 if on else 0))

    def profile_reset(self):
        check(lib().gf2_profile_reset(self.handle))

    def profile_get(self, family):
        ms, count = ctypes.c_double(0), _c_i64(0)
        check(lib().gf2_profile_get(self.handle, int(family), ctypes.byref(ms), ctypes.byref(count)))
        return float(ms.value), int(count.value)

    def membw_probe(self, src_buf, nbytes, dst_buf=None, reps=5):
        """GB/s of a plain streaming read (or copy) of `nbytes` of src_buf: the measured ceiling beside the 8 TB/s spec."""
        sink = self.alloc(8).zero()
        call = lambda: check(lib().gf2_membw_probe_dev(self.handle, src_buf.ptr, dst_buf.ptr if dst_buf is not None else None,
                                                       int(nbytes), sink.ptr))
        call()
        self.sync()
        self.timer_start()
        for _ in range(reps):
            call()
        ms = self.timer_stop() / reps
        sink.free()
        return (2 if dst_buf is not None else 1) * nbytes / ms / 1e6

    # -- linear algebra on packed host arrays ------------------------------------------------------------
    def rref(self, packed, m, n):
        """In place.  Returns (pivot columns, rank)."""
        cap = max(1, min(m, n))
        pivots = np.zeros(cap, dtype=np.int64)
        rank = _c_i64(0)
        check(lib().gf2_rref(self.handle, _ptr(packed), m, n, packed.shape[1] if m else max(1, words_for(n)),
                             _ptr(pivots), ctypes.byref(rank)))
        return pivots[:rank.value], int(rank.value)

    def rref_batch(self, packed, batch, m, n):
        cap = max(1, min(m, n))
        pivots = np.zeros((batch, cap), dtype=np.int64)
        ranks = np.zeros(max(1, batch), dtype=np.int64)
        check(lib().gf2_rref_batch(self.handle, _ptr(packed), batch, m, n, packed.shape[-1], _ptr(pivots),
                                   _ptr(ranks)))
        return pivots, ranks[:batch]

    def nullspace(self, packed, m, n):
        ld = packed.shape[1] if m else max(1, words_for(n))
        out = np.zeros((max(1, n), max(1, words_for(n))), dtype="<u8")
        rows = _c_i64(0)
        check(lib().gf2_nullspace(self.handle, _ptr(packed), m, n, ld, _ptr(out), out.shape[1], ctypes.byref(rows)))
        return out[:rows.value]

    def normalize(self, packed, r, n, offset):
        """In place.  Returns the list of (column, column) swaps."""
        swaps = np.zeros((max(1, r), 2), dtype=np.int64)
        count = _c_i64(0)
        ld = packed.shape[1] if r else max(1, words_for(n))
        check(lib().gf2_normalize(self.handle, _ptr(packed), r, n, ld, offset, _ptr(swaps), ctypes.byref(count)))
        return [(int(a), int(b)) for a, b in swaps[:count.value]]

    def swap_columns(self, packed, m, n, i, j):
        ld = packed.shape[1] if m else max(1, words_for(n))
        check(lib().gf2_swap_columns(self.handle, _ptr(packed), m, n, ld, int(i), int(j)))

    def matmul_abt(self, a, ra, b, rb, n):
        out = np.zeros((max(1, ra), max(1, words_for(rb))), dtype="<u8")
        if ra and rb:
            check(lib().gf2_matmul_abt(self.handle, _ptr(a), ra, a.shape[1], _ptr(b), rb, b.shape[1], n, _ptr(out),
                                       out.shape[1]))
        return out[:ra]

    def row_weights(self, packed, m, n):
        out = np.zeros(max(1, m), dtype=np.uint32)
        ld = packed.shape[1] if m else max(1, words_for(n))
        check(lib().gf2_row_weights(self.handle, _ptr(packed), m, n, ld, _ptr(out)))
        return out[:m]

    def conjugate_gates(self, packed, k, n, gates):
        """css_code.transform_stabilisers on a packed k x 2n matrix, in place.  gates: (g, 3) int32 rows (kind, a, b).
        Returns (code, stop): (GF2_OK, -1), or (GF2_E_NOTCSS | GF2_E_ARG, index of the gate that stopped the walk) with
        `packed` holding the result of the gates before it."""
        gates = np.ascontiguousarray(gates, dtype=np.int32).reshape(-1, 3)
        stop = _c_i64(-1)
        ld = packed.shape[1] if k else max(1, words_for(2 * n))
        rc = lib().gf2_conjugate_gates(self.handle, _ptr(packed) if k else None, k, n, ld,
                                       _ptr(gates) if len(gates) else None, len(gates), ctypes.byref(stop))
        if rc not in (GF2_OK, GF2_E_NOTCSS, GF2_E_ARG) or (rc == GF2_E_ARG and stop.value < 0):
            check(rc)
        return rc, int(stop.value)

    TABLE_MAX_N, TABLE_MAX_R = 64, 24
    TABLE_EMPTY = np.uint64(0xFFFFFFFFFFFFFFFF)

    def syndrome_table(self, packed, r, n, max_weight=None):
        """css_code.syndrome_table on the device (n <= 64, r <= 24): returns (t, dense) where dense[key] is the packed
        error with syndrome key = vec_to_int(syndrome), or TABLE_EMPTY."""
        rows = np.ascontiguousarray(packed[:, 0] if r else np.zeros(0, dtype="<u8"), dtype="<u8")
        dense = np.empty(1 << r, dtype="<u8")
        t, entries = _c_i64(), _c_i64()
        check(lib().gf2_syndrome_table(self.handle, _ptr(rows) if r else None, r, n,
                                       -1 if max_weight is None else max_weight, _ptr(dense), ctypes.byref(t),
                                       ctypes.byref(entries)))
        return int(t.value), dense

    TABLE_WIDE_MAX_N = 128

    def syndrome_table_wide(self, packed, r, n, max_weight=None):
        """The same for 64 < n <= 128: dense[key] = (weight << 32) | rank of the error inside its weight class (combinatorial
        number system), or TABLE_EMPTY; unrank with unrank_supports."""
        rows = np.zeros((max(1, r), 2), dtype="<u8")
        rows[:r, :packed.shape[1]] = packed[:r, :2]
        dense = np.empty(1 << r, dtype="<u8")
        t, entries = _c_i64(), _c_i64()
        check(lib().gf2_syndrome_table_wide(self.handle, _ptr(rows) if r else None, r, n,
                                            -1 if max_weight is None else max_weight, _ptr(dense), ctypes.byref(t),
                                            ctypes.byref(entries)))
        return int(t.value), dense

    TABLE_COLS_MAX_N = 8192

    def syndrome_table_cols(self, packed, r, n, max_weight=None):
        """The same for 128 < n <= 8192 (errors as position lists on the device): dense[key] = (weight << 32) | rank, or
        TABLE_EMPTY; unrank with unrank_supports."""
        rows = np.ascontiguousarray(packed, dtype="<u8") if r else np.zeros((1, max(1, words_for(n))), dtype="<u8")
        dense = np.empty(1 << r, dtype="<u8")
        t, entries = _c_i64(), _c_i64()
        check(lib().gf2_syndrome_table_cols(self.handle, _ptr(rows) if r else None, r, n, rows.shape[1],
                                            -1 if max_weight is None else max_weight, _ptr(dense), ctypes.byref(t),
                                            ctypes.byref(entries)))
        return int(t.value), dense

    TABLE_HASH_MAX_R, TABLE_HASH_MAX_N = 127, 8192

    def syndrome_table_hashed(self, packed, r, n, max_weight=None):
        """css_code.syndrome_table beyond 24 checks (1 <= r <= 127, n <= 8192): a hash table on the device.  Returns
        (t, keys, weights, ranks): keys as a uint64 array (r <= 63) or a list of Python ints (two-word keys), the entries'
        weights and their ranks inside their weight class (unrank with unrank_supports), in no particular order."""
        rows = np.ascontiguousarray(packed, dtype="<u8")
        kw = 1 if r <= 63 else 2
        # The C call writes the entries only into a buffer that holds them all (it counts the classes, it does not keep them), so
        # a buffer that is too small costs a second search.  With a weight bound the table cannot exceed the classes up to it; without
        # one, 2^22 entries (100 MB on the host) cover every table met so far -- the first collision of a code with r checks comes
        # after some 2^((r+1)/2) errors -- and only larger tables are searched twice.
        cap = 1 << 22
        if max_weight is not None:
            total, w = 0, 0
            while w <= min(max_weight, n) and total <= (1 << 28):
                total += math.comb(n, w)
                w += 1
            cap = max(1, min(total, 1 << 28))
        t, entries = _c_i64(), _c_i64()
        while True:
            keys = np.empty((cap, kw), dtype="<u8")
            vals = np.empty(cap, dtype="<u8")
            check(lib().gf2_syndrome_table_hashed(self.handle, _ptr(rows), r, n, rows.shape[1], -1 if max_weight is None else max_weight,
                                                  _ptr(keys), _ptr(vals), cap, ctypes.byref(t), ctypes.byref(entries)))
            if entries.value <= cap:
                break
            cap = int(entries.value)                    # (the search runs once more: the classes were counted, not kept)
        count = int(entries.value)
        keys, vals = keys[:count], vals[:count]
        weights = (vals >> np.uint64(32)).astype(np.int64)
        ranks = vals & np.uint64(0xFFFFFFFF)
        if kw == 1:
            return int(t.value), keys[:, 0].copy(), weights, ranks
        return int(t.value), [int(lo) | (int(hi) << 64) for lo, hi in keys.tolist()], weights, ranks

    def mc_decode_hashed(self, n, h1, r1, keys1, corr1, h2, r2, keys2, corr2, x_operator, z_operator, seed, first, count,
                         p_x, p_y, p_z):
        """gf2_mc_decode_hashed: h1 / h2 packed rows (ld words), keys (entries x 1 or 2 words), corr (entries x 2 words),
        operators (2 words).  Returns the five counts."""
        h1, h2 = np.ascontiguousarray(h1, dtype="<u8"), np.ascontiguousarray(h2, dtype="<u8")
        arrays = [np.ascontiguousarray(a, dtype="<u8") for a in (keys1, corr1, keys2, corr2, x_operator, z_operator)]
        counts = np.zeros(5, dtype=np.uint64)
        check(lib().gf2_mc_decode_hashed(self.handle, n, h1.shape[1], _ptr(h1), r1, _ptr(arrays[0]), _ptr(arrays[1]), len(arrays[1]),
                                         _ptr(h2), r2, _ptr(arrays[2]), _ptr(arrays[3]), len(arrays[3]), _ptr(arrays[4]),
                                         _ptr(arrays[5]), seed & 0xFFFFFFFFFFFFFFFF, first, count, p_x, p_y, p_z, _ptr(counts)))
        return counts

    def mc_decode_strata(self, n, h1, r1, keys1, corr1, h2, r2, keys2, corr2, x_operator, z_operator, seed, first, weights, counts,
                         k_x, k_y, k_z):
        """gf2_mc_decode_strata: mc_decode_hashed's arrays; weights and counts per stratum.  Returns the (nstrata, 5) counts."""
        h1, h2 = np.ascontiguousarray(h1, dtype="<u8"), np.ascontiguousarray(h2, dtype="<u8")
        arrays = [np.ascontiguousarray(a, dtype="<u8") for a in (keys1, corr1, keys2, corr2, x_operator, z_operator)]
        weights, counts, out = _strata_arrays(weights, counts)
        check(lib().gf2_mc_decode_strata(self.handle, n, h1.shape[1], _ptr(h1), r1, _ptr(arrays[0]), _ptr(arrays[1]), len(arrays[1]),
                                         _ptr(h2), r2, _ptr(arrays[2]), _ptr(arrays[3]), len(arrays[3]), _ptr(arrays[4]),
                                         _ptr(arrays[5]), seed & 0xFFFFFFFFFFFFFFFF, first, len(weights), _ptr(weights), _ptr(counts),
                                         k_x, k_y, k_z, _ptr(out)))
        return out

    # -- circuit-level faults -----------------------------------------------------------------------------
    def circuit_create(self, eff):
        return Circuit(self, eff)

    def circuit_outcomes_dev(self, circ, seed, first, count, p_x, p_y, p_z, out_buf, ldo):
        check(lib().gf2_circuit_outcomes_dev(self.handle, circ.handle, seed & 0xFFFFFFFFFFFFFFFF, first, count, p_x, p_y, p_z,
                                             out_buf.ptr, ldo))

    def mc_circuit_run(self, circ, r1, r2, seed, first, count, p_x, p_y, p_z, mode):
        """gf2_mc_circuit_run: returns (hist_z, hist_x) as uint64 arrays."""
        if mode == HIST_FULL:
            if r1 > 24 or r2 > 24:
                raise ValueError("full histograms need r_1, r_2 <= 24")
            nz, nx = 1 << r1, 1 << r2
        else:
            nz, nx = r1 + 1, r2 + 1
        hist_z = np.zeros(nz, dtype=np.uint64)
        hist_x = np.zeros(nx, dtype=np.uint64)
        check(lib().gf2_mc_circuit_run(self.handle, circ.handle, r1, r2, seed & 0xFFFFFFFFFFFFFFFF, first, count, p_x, p_y, p_z,
                                       mode, _ptr(hist_z), nz, _ptr(hist_x), nx))
        return hist_z, hist_x

    def mc_circuit_decode(self, circ, r1, keys1, flips1, r2, keys2, flips2, seed, first, count, p_x, p_y, p_z):
        """gf2_mc_circuit_decode: keys (entries x 1 or 2 words), flips (entries bytes; None with keys = a null table).  Returns
        the five counts."""
        return _decode(lib().gf2_mc_circuit_decode, CIRCUIT_RULE, (self.handle, circ.handle), (), (r1, keys1, flips1, r2, keys2, flips2),
                       seed, first, count, p_x, p_y, p_z, null_flips=True)

    def mc_ec_decode(self, circ, rounds, r1, keys1, flips1, r2, keys2, flips2, seed, first, count, p_x, p_y, p_z):
        """gf2_mc_ec_decode: the eight counts of the error-correction cycle's tally over samples [first, first + count)."""
        return _decode(lib().gf2_mc_ec_decode, EC_RULE, (self.handle, circ.handle), (rounds,), (r1, keys1, flips1, r2, keys2, flips2),
                       seed, first, count, p_x, p_y, p_z)

    def ft_circuit_create(self, eff):
        """gf2_ft_circuit_create: an effect table of up to FT_MAX_LDR words, for ft_outcomes_dev and mc_ft_decode only."""
        return Circuit(self, eff, ft=True)

    def ft_outcomes_dev(self, circ, seed, first, count, p_x, p_y, p_z, out_buf, ldo):
        check(lib().gf2_ft_outcomes_dev(self.handle, circ.handle, seed & 0xFFFFFFFFFFFFFFFF, first, count, p_x, p_y, p_z, out_buf.ptr, ldo))

    def mc_ft_decode(self, circ, nsteps, measure_mask, r1, keys1, flips1, r2, keys2, flips2, seed, first, count, p_x, p_y, p_z):
        """gf2_mc_ft_decode: the seven counts of the logical measurement's tally over samples [first, first + count)."""
        return _decode(lib().gf2_mc_ft_decode, FT_RULE, (self.handle, circ.handle), (nsteps, measure_mask),
                       (r1, keys1, flips1, r2, keys2, flips2), seed, first, count, p_x, p_y, p_z)

    def stream_create(self, type_eff, type_locations, type_flags, block_type, block_kind):
        return Stream(self, type_eff, type_locations, type_flags, block_type, block_kind)

    def stream_outcomes_dev(self, stream, seed, first, count, p_x, p_y, p_z, out_buf, ldo):
        check(lib().gf2_stream_outcomes_dev(self.handle, stream.handle, seed & 0xFFFFFFFFFFFFFFFF, first, count, p_x, p_y, p_z, out_buf.ptr, ldo))

    def mc_stream_decode(self, stream, r1, keys1, flips1, r2, keys2, flips2, seed, first, count, p_x, p_y, p_z):
        """gf2_mc_stream_decode: the twelve counts of the streamed tally over samples [first, first + count)."""
        return _decode(lib().gf2_mc_stream_decode, STREAM_RULE, (self.handle, stream.handle), (), (r1, keys1, flips1, r2, keys2, flips2),
                       seed, first, count, p_x, p_y, p_z)

    def mstream_create(self, type_eff, type_locations, type_flags, block_type, block_kind, block_a, block_b, nframes):
        return MStream(self, type_eff, type_locations, type_flags, block_type, block_kind, block_a, block_b, nframes)

    def mstream_outcomes_dev(self, mstream, seed, first, count, p_x, p_y, p_z, out_buf, ldo):
        check(lib().gf2_mstream_outcomes_dev(self.handle, mstream.handle, seed & 0xFFFFFFFFFFFFFFFF, first, count, p_x, p_y, p_z, out_buf.ptr, ldo))

    def mc_mstream_decode(self, mstream, records, r1, keys1, flips1, r2, keys2, flips2, seed, first, count, p_x, p_y, p_z):
        """gf2_mc_mstream_decode: the twenty counts of the multi-block tally over samples [first, first + count)."""
        return _decode(lib().gf2_mc_mstream_decode, MSTREAM_RULE, (self.handle, mstream.handle, int(records)), (),
                       (r1, keys1, flips1, r2, keys2, flips2), seed, first, count, p_x, p_y, p_z)

    def retry_create(self, type_eff, type_locations, type_flags, block_type, block_kind, type_regions, type_nregions):
        return Retry(self, type_eff, type_locations, type_flags, block_type, block_kind, type_regions, type_nregions)

    def retry_outcomes_dev(self, retry, seed, first, count, p_x, p_y, p_z, max_attempts, out_buf, ldo):
        check(lib().gf2_retry_outcomes_dev(self.handle, retry.handle, seed & 0xFFFFFFFFFFFFFFFF, first, count, p_x, p_y, p_z, int(max_attempts),
                                           out_buf.ptr, ldo))

    def mc_retry_decode(self, retry, r1, keys1, flips1, r2, keys2, flips2, seed, first, count, p_x, p_y, p_z, max_attempts):
        """gf2_mc_retry_decode: the fourteen counts of the repeat-until-success tally over samples [first, first + count)."""
        return _decode(lib().gf2_mc_retry_decode, RETRY_RULE, (self.handle, retry.handle), (), (r1, keys1, flips1, r2, keys2, flips2),
                       seed, first, count, p_x, p_y, p_z, int(max_attempts))

    def mretry_create(self, type_eff, type_locations, type_flags, block_type, block_kind, block_a, block_b, nframes, type_regions, type_nregions):
        return MRetry(self, type_eff, type_locations, type_flags, block_type, block_kind, block_a, block_b, nframes, type_regions, type_nregions)

    def mretry_outcomes_dev(self, mretry, seed, first, count, p_x, p_y, p_z, max_attempts, out_buf, ldo):
        check(lib().gf2_mretry_outcomes_dev(self.handle, mretry.handle, seed & 0xFFFFFFFFFFFFFFFF, first, count, p_x, p_y, p_z, int(max_attempts),
                                            out_buf.ptr, ldo))

    def mc_mretry_decode(self, mretry, records, r1, keys1, flips1, r2, keys2, flips2, seed, first, count, p_x, p_y, p_z, max_attempts):
        """gf2_mc_mretry_decode: the twenty-two counts of the repeat-until-success tally of a multi-block program."""
        return _decode(lib().gf2_mc_mretry_decode, MRETRY_RULE, (self.handle, mretry.handle, int(records)), (),
                       (r1, keys1, flips1, r2, keys2, flips2), seed, first, count, p_x, p_y, p_z, int(max_attempts))

    def mretry_gate_create(self, type_eff, type_locations, type_flags, block_type, block_kind, block_a, block_b, nframes, type_regions,
                           type_nregions, site_loc, site_regions):
        return MRetryGate(self, type_eff, type_locations, type_flags, block_type, block_kind, block_a, block_b, nframes, type_regions,
                          type_nregions, site_loc, site_regions)

    def mretry_gate_outcomes_dev(self, mretry, seed, first, count, p1, p2, max_attempts, out_buf, ldo):
        check(lib().gf2_mretry_gate_outcomes_dev(self.handle, mretry.handle, seed & 0xFFFFFFFFFFFFFFFF, first, count, p1, p2, int(max_attempts),
                                                 out_buf.ptr, ldo))

    def mc_mretry_gate_decode(self, mretry, records, r1, keys1, flips1, r2, keys2, flips2, seed, first, count, p1, p2, max_attempts):
        """gf2_mc_mretry_gate_decode: the twenty-two counts of the repeat-until-success tally of a multi-block program under
        gate-level faults."""
        keep, rest = _rule_arguments(MRETRY_RULE, (), (r1, keys1, flips1, r2, keys2, flips2))
        counts = np.zeros(MRETRY_RULE.fields, dtype=np.uint64)
        check(lib().gf2_mc_mretry_gate_decode(self.handle, mretry.handle, int(records), *rest, seed & 0xFFFFFFFFFFFFFFFF, first, count, p1, p2,
                                              int(max_attempts), _ptr(counts)))
        return counts

    def retry_wait_create(self, type_eff, type_locations, type_flags, block_type, block_kind, type_regions, type_nregions, wait_eff, wait_count):
        return RetryWait(self, type_eff, type_locations, type_flags, block_type, block_kind, type_regions, type_nregions, wait_eff, wait_count)

    def retry_wait_outcomes_dev(self, retry, seed, first, count, p_x, p_y, p_z, q_x, q_y, q_z, max_attempts, out_buf, ldo):
        check(lib().gf2_retry_wait_outcomes_dev(self.handle, retry.handle, seed & 0xFFFFFFFFFFFFFFFF, first, count, p_x, p_y, p_z, float(q_x),
                                                float(q_y), float(q_z), int(max_attempts), out_buf.ptr, ldo))

    def mc_retry_wait_decode(self, retry, r1, keys1, flips1, r2, keys2, flips2, seed, first, count, p_x, p_y, p_z, q_x, q_y, q_z, max_attempts):
        """gf2_mc_retry_wait_decode: the fifteen counts of the repeat-until-success tally with waiting faults."""
        return _decode(lib().gf2_mc_retry_wait_decode, RETRY_WAIT_RULE, (self.handle, retry.handle), (), (r1, keys1, flips1, r2, keys2, flips2),
                       seed, first, count, p_x, p_y, p_z, float(q_x), float(q_y), float(q_z), int(max_attempts))

    def retry_gate_create(self, type_eff, type_locations, type_flags, block_type, block_kind, type_regions, type_nregions, site_loc, site_regions):
        return RetryGate(self, type_eff, type_locations, type_flags, block_type, block_kind, type_regions, type_nregions, site_loc, site_regions)

    def retry_gate_outcomes_dev(self, retry, seed, first, count, p1, p2, max_attempts, out_buf, ldo):
        check(lib().gf2_retry_gate_outcomes_dev(self.handle, retry.handle, seed & 0xFFFFFFFFFFFFFFFF, first, count, p1, p2, int(max_attempts),
                                                out_buf.ptr, ldo))

    def mc_retry_gate_decode(self, retry, r1, keys1, flips1, r2, keys2, flips2, seed, first, count, p1, p2, max_attempts):
        """gf2_mc_retry_gate_decode: the fourteen counts of the repeat-until-success tally under gate-level faults."""
        keep, rest = _rule_arguments(RETRY_RULE, (), (r1, keys1, flips1, r2, keys2, flips2))
        counts = np.zeros(RETRY_RULE.fields, dtype=np.uint64)
        check(lib().gf2_mc_retry_gate_decode(self.handle, retry.handle, *rest, seed & 0xFFFFFFFFFFFFFFFF, first, count, p1, p2, int(max_attempts),
                                             _ptr(counts)))
        return counts

    def retry_gate_wait_create(self, type_eff, type_locations, type_flags, block_type, block_kind, type_regions, type_nregions, site_loc,
                               site_regions, wait_eff, wait_count):
        return RetryGateWait(self, type_eff, type_locations, type_flags, block_type, block_kind, type_regions, type_nregions, site_loc,
                             site_regions, wait_eff, wait_count)

    def retry_gate_wait_outcomes_dev(self, retry, seed, first, count, p1, p2, q_x, q_y, q_z, max_attempts, out_buf, ldo):
        check(lib().gf2_retry_gate_wait_outcomes_dev(self.handle, retry.handle, seed & 0xFFFFFFFFFFFFFFFF, first, count, p1, p2, float(q_x),
                                                     float(q_y), float(q_z), int(max_attempts), out_buf.ptr, ldo))

    def mc_retry_gate_wait_decode(self, retry, r1, keys1, flips1, r2, keys2, flips2, seed, first, count, p1, p2, q_x, q_y, q_z, max_attempts):
        """gf2_mc_retry_gate_wait_decode: the fifteen counts of the repeat-until-success tally under gate-level faults with waiting
        faults."""
        keep, rest = _rule_arguments(RETRY_WAIT_RULE, (), (r1, keys1, flips1, r2, keys2, flips2))
        counts = np.zeros(RETRY_WAIT_RULE.fields, dtype=np.uint64)
        check(lib().gf2_mc_retry_gate_wait_decode(self.handle, retry.handle, *rest, seed & 0xFFFFFFFFFFFFFFFF, first, count, p1, p2, float(q_x),
                                                  float(q_y), float(q_z), int(max_attempts), _ptr(counts)))
        return counts

    def mc_circuit_decode_strata(self, circ, r1, keys1, flips1, r2, keys2, flips2, seed, first, weights, counts, k_x, k_y, k_z):
        """gf2_mc_circuit_decode_strata: mc_circuit_decode's tables; weights and counts per stratum.  Returns the (nstrata, 5) counts."""
        return _decode_strata(lib().gf2_mc_circuit_decode_strata, CIRCUIT_RULE, (self.handle, circ.handle), (),
                              (r1, keys1, flips1, r2, keys2, flips2), seed, first, weights, counts, k_x, k_y, k_z)

    def mc_ec_decode_strata(self, circ, rounds, r1, keys1, flips1, r2, keys2, flips2, seed, first, weights, counts, k_x, k_y, k_z):
        """gf2_mc_ec_decode_strata: mc_ec_decode's tables; weights and counts per stratum.  Returns the (nstrata, 8) counts."""
        return _decode_strata(lib().gf2_mc_ec_decode_strata, EC_RULE, (self.handle, circ.handle), (rounds,),
                              (r1, keys1, flips1, r2, keys2, flips2), seed, first, weights, counts, k_x, k_y, k_z)

    def mc_ft_decode_strata(self, circ, nsteps, measure_mask, r1, keys1, flips1, r2, keys2, flips2, seed, first, weights, counts, k_x,
                            k_y, k_z):
        """gf2_mc_ft_decode_strata: mc_ft_decode's tables; weights and counts per stratum.  Returns the (nstrata, 7) counts."""
        return _decode_strata(lib().gf2_mc_ft_decode_strata, FT_RULE, (self.handle, circ.handle), (nsteps, measure_mask),
                              (r1, keys1, flips1, r2, keys2, flips2), seed, first, weights, counts, k_x, k_y, k_z)

    def circuit_enumerate(self, circ, r1, keys1, flips1, r2, keys2, flips2, w, first_rank, count):
        """gf2_circuit_enumerate: circuit_enumerate_host's counts from the device."""
        return _enumerate(lib().gf2_circuit_enumerate, CIRCUIT_RULE, (self.handle, circ.handle), (),
                          (r1, keys1, flips1, r2, keys2, flips2), w, first_rank, count)

    # -- syndromes ----------------------------------------------------------------------------------------
    def ec_enumerate(self, circ, rounds, r1, keys1, flips1, r2, keys2, flips2, w, first_rank, count):
        """gf2_ec_enumerate: ec_enumerate_host's counts from the device."""
        return _enumerate(lib().gf2_ec_enumerate, EC_RULE, (self.handle, circ.handle), (rounds,), (r1, keys1, flips1, r2, keys2, flips2),
                          w, first_rank, count)

    def ft_enumerate(self, circ, nsteps, measure_mask, r1, keys1, flips1, r2, keys2, flips2, w, first_rank, count):
        """gf2_ft_enumerate: ft_enumerate_host's counts from the device."""
        return _enumerate(lib().gf2_ft_enumerate, FT_RULE, (self.handle, circ.handle), (nsteps, measure_mask),
                          (r1, keys1, flips1, r2, keys2, flips2), w, first_rank, count)

    def ec_gate_enumerate(self, circ, rounds, r1, keys1, flips1, r2, keys2, flips2, site_loc, n1, n2, w, b, first_rank, count):
        """gf2_ec_gate_enumerate: ec_gate_enumerate_host's counts from the device."""
        return _gate_enumerate(lib().gf2_ec_gate_enumerate, EC_RULE, (self.handle, circ.handle), (rounds,),
                               (r1, keys1, flips1, r2, keys2, flips2), (site_loc, n1, n2), w, b, first_rank, count)

    def ft_gate_enumerate(self, circ, nsteps, measure_mask, r1, keys1, flips1, r2, keys2, flips2, site_loc, n1, n2, w, b, first_rank, count):
        """gf2_ft_gate_enumerate: ft_gate_enumerate_host's counts from the device."""
        return _gate_enumerate(lib().gf2_ft_gate_enumerate, FT_RULE, (self.handle, circ.handle), (nsteps, measure_mask),
                               (r1, keys1, flips1, r2, keys2, flips2), (site_loc, n1, n2), w, b, first_rank, count)

    def mc_ec_decode_gate_strata(self, circ, rounds, r1, keys1, flips1, r2, keys2, flips2, site_loc, n1, n2, seed, first, strata, counts):
        """gf2_mc_ec_decode_gate_strata: mc_ec_decode's tables, gate_sites' site table; strata (nstrata, 2) rows (a, b) and counts per
        stratum.  Returns the (nstrata, 17, 8) counts [stratum][c][field]."""
        return _decode_gate_strata(lib().gf2_mc_ec_decode_gate_strata, EC_RULE, (self.handle, circ.handle), (rounds,),
                                   (r1, keys1, flips1, r2, keys2, flips2), (site_loc, n1, n2), seed, first, strata, counts)

    def mc_ft_decode_gate_strata(self, circ, nsteps, measure_mask, r1, keys1, flips1, r2, keys2, flips2, site_loc, n1, n2, seed, first,
                                 strata, counts):
        """gf2_mc_ft_decode_gate_strata: mc_ft_decode's tables, likewise.  Returns the (nstrata, 17, 7) counts."""
        return _decode_gate_strata(lib().gf2_mc_ft_decode_gate_strata, FT_RULE, (self.handle, circ.handle), (nsteps, measure_mask),
                                   (r1, keys1, flips1, r2, keys2, flips2), (site_loc, n1, n2), seed, first, strata, counts)

    def mc_ec_decode_gate(self, circ, rounds, r1, keys1, flips1, r2, keys2, flips2, site_loc, n1, n2, seed, first, count, p1, p2):
        """gf2_mc_ec_decode_gate: mc_ec_decode's eight counts over samples [first, first + count) when every gate fails on its own,
        a one-operand site of gate_sites' table with probability p1, a CNOT site with p2."""
        return _decode_gate(lib().gf2_mc_ec_decode_gate, EC_RULE, (self.handle, circ.handle), (rounds,),
                            (r1, keys1, flips1, r2, keys2, flips2), (site_loc, n1, n2), seed, first, count, p1, p2)

    def mc_ft_decode_gate(self, circ, nsteps, measure_mask, r1, keys1, flips1, r2, keys2, flips2, site_loc, n1, n2, seed, first, count,
                          p1, p2):
        """gf2_mc_ft_decode_gate: mc_ft_decode's seven counts, likewise."""
        return _decode_gate(lib().gf2_mc_ft_decode_gate, FT_RULE, (self.handle, circ.handle), (nsteps, measure_mask),
                            (r1, keys1, flips1, r2, keys2, flips2), (site_loc, n1, n2), seed, first, count, p1, p2)

    def ec_enumerate_list(self, circ, rounds, r1, keys1, flips1, r2, keys2, flips2, w, first_rank, count, select, capacity):
        """gf2_ec_enumerate_list: ec_enumerate_list_host's (found, records) from the device, byte for byte."""
        return _enumerate_list(lib().gf2_ec_enumerate_list, EC_RULE, (self.handle, circ.handle), (rounds,),
                               (r1, keys1, flips1, r2, keys2, flips2), w, first_rank, count, select, capacity, FAULT_LIST_MAX_CAPACITY)

    def ft_enumerate_list(self, circ, nsteps, measure_mask, r1, keys1, flips1, r2, keys2, flips2, w, first_rank, count, select, capacity):
        """gf2_ft_enumerate_list: ft_enumerate_list_host's (found, records) from the device, byte for byte."""
        return _enumerate_list(lib().gf2_ft_enumerate_list, FT_RULE, (self.handle, circ.handle), (nsteps, measure_mask),
                               (r1, keys1, flips1, r2, keys2, flips2), w, first_rank, count, select, capacity, FAULT_LIST_MAX_CAPACITY)

    def ec_gate_enumerate_list(self, circ, rounds, r1, keys1, flips1, r2, keys2, flips2, site_loc, n1, n2, w, b, first_rank, count, select,
                               capacity, into=None):
        """gf2_ec_gate_enumerate_list: ec_gate_enumerate_list_host's (found, records) from the device, byte for byte."""
        return _gate_enumerate_list(lib().gf2_ec_gate_enumerate_list, EC_RULE, (self.handle, circ.handle), (rounds,),
                                    (r1, keys1, flips1, r2, keys2, flips2), (site_loc, n1, n2), w, b, first_rank, count, select, capacity,
                                    FAULT_LIST_MAX_CAPACITY, into)

    def ft_gate_enumerate_list(self, circ, nsteps, measure_mask, r1, keys1, flips1, r2, keys2, flips2, site_loc, n1, n2, w, b, first_rank,
                               count, select, capacity, into=None):
        """gf2_ft_gate_enumerate_list: ft_gate_enumerate_list_host's (found, records) from the device, byte for byte."""
        return _gate_enumerate_list(lib().gf2_ft_gate_enumerate_list, FT_RULE, (self.handle, circ.handle), (nsteps, measure_mask),
                                    (r1, keys1, flips1, r2, keys2, flips2), (site_loc, n1, n2), w, b, first_rank, count, select, capacity,
                                    FAULT_LIST_MAX_CAPACITY, into)

    def check_create(self, packed, r, n):
        return Check(self, packed, r, n)

    def syndrome_batch(self, h, r, n, e, batch):
        """Sample-major host arrays: e is batch x words(n); returns batch x words(r)."""
        out = np.zeros((max(1, batch), max(1, words_for(r))), dtype="<u8")
        if batch and r:
            check(lib().gf2_syndrome_batch(self.handle, _ptr(h), r, n, h.shape[1], _ptr(e), batch, e.shape[1],
                                           LAYOUT_SAMPLE_MAJOR, _ptr(out), out.shape[1]))
        return out[:batch]

    def syndrome_batch_sliced(self, h, r, n, e, batch):
        """Bit-sliced host arrays: e is n x words(batch); returns r x words(batch)."""
        width = max(1, words_for(batch))
        out = np.zeros((max(1, r), width), dtype="<u8")
        if batch and r:
            check(lib().gf2_syndrome_batch(self.handle, _ptr(h), r, n, h.shape[1], _ptr(e), batch, e.shape[1],
                                           LAYOUT_BIT_SLICED, _ptr(out), width))
        return out[:r]

    def syndrome_dev(self, chk, e_buf, batch, lde, s_buf, lds, layout=LAYOUT_SAMPLE_MAJOR):
        check(lib().gf2_syndrome_dev(self.handle, chk.handle, e_buf.ptr, batch, lde, layout, s_buf.ptr, lds))

    def syndrome_sparse_dev(self, chk, e_buf, batch, lde, s_buf=None, lds=0, hist_buf=None, nbins=0):
        """Sparse-error kernel: sample-major errors; writes syndromes and/or accumulates the weight histogram."""
        check(lib().gf2_syndrome_sparse_dev(self.handle, chk.handle, e_buf.ptr, batch, lde,
                                            s_buf.ptr if s_buf is not None else None, lds,
                                            hist_buf.ptr if hist_buf is not None else None, nbins))

    def histogram_dev(self, s_buf, batch, lds, r, mode, hist_buf, nbins, layout=LAYOUT_SAMPLE_MAJOR):
        check(lib().gf2_histogram_dev(self.handle, s_buf.ptr, batch, lds, layout, r, mode, hist_buf.ptr, nbins))

    def sample_errors_dev(self, n, seed, first, count, p_x, p_y, p_z, ex_buf, ez_buf, lde,
                          layout=LAYOUT_SAMPLE_MAJOR):
        check(lib().gf2_sample_errors_dev(self.handle, n, seed & 0xFFFFFFFFFFFFFFFF, first, count, p_x, p_y, p_z,
                                          ex_buf.ptr, ez_buf.ptr, lde, layout))

    def retile_dev(self, e_buf, batch, lde, n, tiled_buf):
        check(lib().gf2_retile_dev(self.handle, e_buf.ptr, batch, lde, n, tiled_buf.ptr))

    def mc_run(self, chk1, chk2, seed, first, count, p_x, p_y, p_z, mode):
        """Returns (hist_z, hist_x) as uint64 arrays."""
        if mode == HIST_FULL:
            nz, nx = 1 << chk1.r, 1 << chk2.r
        else:
            nz, nx = chk1.r + 1, chk2.r + 1
        hist_z = np.zeros(nz, dtype=np.uint64)
        hist_x = np.zeros(nx, dtype=np.uint64)
        check(lib().gf2_mc_run(self.handle, chk1.handle, chk2.handle, seed & 0xFFFFFFFFFFFFFFFF, first, count,
                               p_x, p_y, p_z, mode, _ptr(hist_z), nz, _ptr(hist_x), nx))
        return hist_z, hist_x


    def mc_decode(self, chk1, chk2, table_c1, table_c2, x_operator, z_operator, seed, first, count, p_x, p_y, p_z):
        """Returns the five counts of gf2_mc_decode as a uint64 array."""
        t1 = np.ascontiguousarray(table_c1, dtype=np.uint64)
        t2 = np.ascontiguousarray(table_c2, dtype=np.uint64)
        counts = np.zeros(5, dtype=np.uint64)
        check(lib().gf2_mc_decode(self.handle, chk1.handle, chk2.handle, _ptr(t1), _ptr(t2), int(x_operator),
                                  int(z_operator), seed & 0xFFFFFFFFFFFFFFFF, first, count, p_x, p_y, p_z, _ptr(counts)))
        return counts


class Comm(object):
    """An RCCL communicator for the histogram all-reduce (gf2_comm_*).

    Comm.unique_id()                     bytes to hand to every rank out of band (rank 0 makes them)
    Comm(ctx, id, nranks, rank)          one process per GPU
    Comm.all_local([ctx0, ctx1, ...])    one process, one context per device
    """

    def __init__(self, ctx, unique_id, nranks, rank):
        if len(unique_id) != COMM_ID_BYTES:
            raise ValueError("the communicator id has %d bytes" % COMM_ID_BYTES)
        out = ctypes.c_void_p()
        ident = ctypes.create_string_buffer(bytes(unique_id), COMM_ID_BYTES)
        check(lib().gf2_comm_create(ctx.handle, ident, int(nranks), int(rank), ctypes.byref(out)))
        self.handle, self.contexts, self.nranks = out.value, [ctx], int(nranks)

    @staticmethod
    def unique_id():
        ident = ctypes.create_string_buffer(COMM_ID_BYTES)
        check(lib().gf2_comm_unique_id(ident, COMM_ID_BYTES))
        return ident.raw

    @classmethod
    def all_local(cls, contexts):
        self = cls.__new__(cls)
        handles = (ctypes.c_void_p * len(contexts))(*[c.handle for c in contexts])
        out = ctypes.c_void_p()
        check(lib().gf2_comm_create_all(handles, len(contexts), ctypes.byref(out)))
        self.handle, self.contexts, self.nranks = out.value, list(contexts), len(contexts)
        return self

    def allreduce(self, bufs, nbins):
        """In-place sum of `nbins` uint64 bins over all ranks; bufs: one DeviceBuffer per context of this communicator."""
        bufs = list(bufs) if isinstance(bufs, (list, tuple)) else [bufs]
        if len(bufs) != len(self.contexts):
            raise ValueError("one buffer per context")
        if any(b.nbytes < 8 * nbins for b in bufs):
            raise ValueError("buffer smaller than nbins words")
        ptrs = (ctypes.c_void_p * len(bufs))(*[b.ptr for b in bufs])
        check(lib().gf2_hist_allreduce(self.handle, ptrs, int(nbins)))

    def allreduce_host(self, hists):
        """Sums a list of host uint64 arrays over the ranks (one all-reduce of the concatenation, through device memory of
        this process's context)."""
        if len(self.contexts) != 1:
            raise ValueError("allreduce_host is for one context per process")
        sizes = [int(np.asarray(h).size) for h in hists]
        flat = np.ascontiguousarray(np.concatenate([np.asarray(h, dtype=np.uint64).ravel() for h in hists]))
        buf = self.contexts[0].alloc(flat.nbytes).upload(flat)
        self.allreduce(buf, flat.size)
        total = buf.download((flat.size,), np.uint64)
        buf.free()
        out, pos = [], 0
        for size in sizes:
            out.append(total[pos:pos + size].copy())
            pos += size
        return out

    def close(self):
        if self.handle:
            handle, self.handle = self.handle, None
            check(lib().gf2_comm_destroy(handle))


def rccl_version():
    out = ctypes.c_int(0)
    check(lib().gf2_rccl_version(ctypes.byref(out)))
    return int(out.value)


_default = None
_default_lock = threading.Lock()


def default_context():
    """Process-wide context on GF2_DEVICE, else LOCAL_RANK, else device 0."""
    global _default
    if _default is None:
        with _default_lock:
            if _default is None:
                device = int(os.environ.get("GF2_DEVICE", os.environ.get("LOCAL_RANK", "0")))
                _default = Context(device)
    return _default
