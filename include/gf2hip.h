/*
 * gf2hip.h -- C ABI of libgf2hip.so, the MI355X (gfx950) GF(2) engine behind the bin_matrix /
 * CSSCode hot path of jimpo/quantum-css-codes.
 *
 * The reference has no FFI layer: its boundary is the Python module surface (bin_matrix.py,
 * css_code.py).  The Python package quantum_css_codes_amd keeps that surface and binds these entry
 * points with ctypes (quantum_css_codes_amd/_native.py; INTEGRATION.md shows the stub a reference
 * maintainer would add).  Each entry point names the reference lines it replaces; paths are
 * relative to the reference repository.
 *
 * Conventions
 *   - Every function returns an int: GF2_OK or a negative GF2_E_* code.  gf2_last_error() returns
 *     a thread-local human-readable message for the last failure on the calling thread.
 *   - Packed layout: row-major uint64_t words, column j in word j>>6 at bit j&63, `ld` words per
 *     row (ld >= ceil(n/64)).  Pad bits (columns >= n) must be zero on input and are zero on output.
 *   - Device buffers (tests/test_gpu_state.py holds the library to each of these):
 *       outputs need no initialisation: every word an entry point promises is stored, whatever it is (an all-zero syndrome
 *       too), and nothing is written outside the buffer;
 *       pitch padding (words of a row past the ones promised, when a pitch is larger than needed) is either left as it was
 *       or zeroed, and exactly left as it was where an entry point says so (the outcome stores); it is never read;
 *       histograms (hist_dev) are ACCUMULATED into: the caller zeroes the bins before the first call, and calls add up;
 *       alignment: every device pointer must be 8-byte aligned (4-byte for status_dev); "any 8-byte-aligned address" at an
 *       argument below means that nothing more is asked -- a kernel that has a 16-byte path picks it by looking at the
 *       pointer and the pitch -- and "16-byte aligned" that the entry point refuses anything else with GF2_E_ARG (the
 *       tiled layout and the blocked eliminations are read and written as 16-byte pieces).  gf2_dev_alloc, hipMalloc and
 *       torch allocations are aligned to 256 bytes or more.  DESIGN.md "State between calls" lists the wide accesses.
 *       No result depends on what the context's workspaces, or any device buffer of the library, held before a call.
 *   - "host" pointers are caller-owned host memory; the library never keeps them past return.
 *     "dev" pointers are device memory from gf2_dev_alloc (or any hipMalloc'ed / torch-allocated
 *     buffer on the context's device).
 *   - A gf2_ctx owns one HIP stream.  Host-buffer entry points are synchronous.  `_dev` entry points
 *     enqueue on the context's stream and return; gf2_ctx_sync() waits.  A context is not
 *     thread-safe; distinct contexts are independent.
 *   - There is no CPU fallback: without a usable GPU, compute entry points fail with GF2_E_HIP.
 */
#ifndef GF2HIP_H
#define GF2HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define GF2_OK            0
#define GF2_E_ARG        (-1)  /* bad argument                                                   */
#define GF2_E_COLUMNS    (-2)  /* ValueError("not enough columns"), css_code.py:811-812          */
#define GF2_E_DEPENDENT  (-3)  /* InvalidCodeError("rows are not independent"), css_code.py:825  */
#define GF2_E_HIP        (-4)  /* HIP runtime error / no device                                  */
#define GF2_E_NOMEM      (-5)  /* allocation failure                                             */
#define GF2_E_NOTCSS     (-6)  /* NotImplementedError("only handles CSS codes"), css_code.py:762-763 */
#define GF2_E_RCCL       (-7)  /* RCCL error (gf2_comm_*, gf2_hist_allreduce)                    */

#define GF2_LAYOUT_SAMPLE_MAJOR 0  /* E: B rows of lde words (one error per row); S: B rows of lds words */
#define GF2_LAYOUT_BIT_SLICED   1  /* E: n rows of ceil(B/64) words (word b of row q = qubit q of samples
                                      64b..64b+63); S: r rows likewise.  Requires n <= 64 and r <= 64. */
#define GF2_LAYOUT_TILED        2  /* Device-native error layout of the large-n syndrome kernel.  Samples are
                                      grouped in tiles of 64; with ldt = gf2_tiled_ld(n) (even) words per sample,
                                      word w of sample b sits at word offset
                                          (b>>6)*64*ldt + (w>>1)*128 + (b&63)*2 + (w&1)
                                      so the 64 lanes of a wavefront read one 16-byte piece each from 1 KiB of
                                      contiguous memory.  The buffer holds ceil(B/64) whole tiles
                                      (gf2_tiled_words).  Syndromes of tiled errors are SLAB-MAJOR: word s
                                      (rows 64s..64s+63) of sample b at s*lds + b with lds >= B, so a wavefront
                                      stores 512 contiguous bytes. */

#define GF2_HIST_FULL    0     /* bins indexed by vec_to_int(syndrome) (bin_matrix.py:36-43), 2^r bins  */
#define GF2_HIST_WEIGHT  1     /* bins indexed by the syndrome's Hamming weight, r+1 bins               */

typedef struct gf2_ctx gf2_ctx;
typedef struct gf2_check gf2_check;   /* a parity-check matrix prepared on the device */

/* ---- library / context ------------------------------------------------------------------------ */
int gf2_version(void);
const char* gf2_last_error(void);
int gf2_device_count(int* count_out);
int gf2_ctx_create(int device, gf2_ctx** ctx_out);
int gf2_ctx_destroy(gf2_ctx* ctx);
int gf2_ctx_sync(gf2_ctx* ctx);

/* Routing flags of a context.  Several entry points have more than one implementation behind them, all bit-identical; 0 (the
 * default) leaves the choice to the library.  The routes a caller of the bin_matrix / CSSCode surface may want to force: */
#define GF2_F_MC_DENSE             (1u << 5)   /* gf2_mc_run: dense table kernel whatever the error rate                */
#define GF2_F_RREF_SEQUENTIAL      (1u << 8)   /* gf2_rref*: one pivot per step                                         */
#define GF2_F_NORMALIZE_SEQUENTIAL (1u << 10)  /* gf2_normalize*: one pivot per step                                    */
/* (The other bits name routes that exist for the parity tests and the A/B scripts under profiles/ -- quantum_css_codes_amd/csrc/
 * gf2_tuning.h lists them; gf2_ctx_set_flags refuses bits no route is defined for.  The library never reads the environment per
 * call; gf2_ctx_create reads GF2_FLAGS once as the initial value.) */
int gf2_ctx_set_flags(gf2_ctx* ctx, uint32_t flags);
int gf2_ctx_get_flags(gf2_ctx* ctx, uint32_t* flags_out);
/* Tunables of a context (value < 0 restores the default).  The two that size device memory: */
#define GF2_OPT_SLAB_PASS_LOG2  0   /* slab pipeline: 2^k samples per pass through the workspace, 12 <= k <= 24 (default 22) */
#define GF2_OPT_MC_CHUNK_LOG2   4   /* gf2_mc_run at n <= 4096, sparse rates: 2^k samples per chunk, 16 <= k <= 22 (default 22; 21 with GF2_F_MC_ROWS) */
/* (Further option numbers, used by the A/B scripts: quantum_css_codes_amd/csrc/gf2_tuning.h.) */
int gf2_ctx_set_option(gf2_ctx* ctx, int option, int64_t value);

/* ---- testing ----
 * Sets every byte of the context's workspaces (four slots that only grow and are never cleared between calls) to `byte`
 * (0..255), after waiting for all of the context's streams, and waits for the fills.  slot_bytes_out (four int64, may be null)
 * receives the slots' sizes.  No result of this library depends on what the workspaces hold between calls; the test suite
 * shows it by calling this between two identical calls.  GF2_E_ARG for a null context or a byte outside 0..255. */
int gf2_ctx_fill_workspace(gf2_ctx* ctx, int byte, int64_t* slot_bytes_out /* 4, may be null */);

/* Device memory and stream-ordered copies on the context's stream (copies are synchronous). */
int gf2_dev_alloc(gf2_ctx* ctx, size_t bytes, void** dev_out);
int gf2_dev_free(gf2_ctx* ctx, void* dev);
int gf2_dev_zero(gf2_ctx* ctx, void* dev, size_t bytes);
int gf2_h2d(gf2_ctx* ctx, void* dev_dst, const void* host_src, size_t bytes);
int gf2_d2h(gf2_ctx* ctx, void* host_dst, const void* dev_src, size_t bytes);

/* HIP-event timing on the context's stream: bracket any sequence of _dev calls. */
int gf2_timer_start(gf2_ctx* ctx);
int gf2_timer_stop(gf2_ctx* ctx, float* elapsed_ms_out);   /* synchronises on the stop event */
/* Accumulated HIP-event time of one kernel family since the last reset (see GF2_K_*); each launch of
 * that family is bracketed by its own pair of events when profiling is enabled. */
#define GF2_K_SYNDROME 0
#define GF2_K_HIST     1
#define GF2_K_SAMPLER  2
#define GF2_K_ELIM     3
#define GF2_K_COUNT    4
int gf2_profile_enable(gf2_ctx* ctx, int on);
int gf2_profile_reset(gf2_ctx* ctx);
int gf2_profile_get(gf2_ctx* ctx, int kernel_family, double* total_ms_out, int64_t* launches_out);

/* Memory-bandwidth probe: streams `bytes` (a multiple of 16) from src_dev with 16-byte loads; dst_dev null = read only,
 * else the bytes are also stored there (copy).  Asynchronous on the context's stream; bracket it with gf2_timer_*.  It is
 * what bench.py quotes roofline fractions against next to the 8 TB/s specification.  sink_dev: one device word. */
int gf2_membw_probe_dev(gf2_ctx* ctx, const void* src_dev, void* dst_dev, size_t bytes, uint64_t* sink_dev);

/* ---- host-side packing (pure host code, no GPU needed) -------------------------------------------
 * Dense integer arrays <-> packed words.  Packing applies `& 1` (the reference reduces lazily with
 * np.mod(.,2), bin_matrix.py:34, css_code.py:39-40).  Strides are in elements. */
int gf2_pack_rows_u8(const uint8_t* src, int64_t m, int64_t n, int64_t src_stride, uint64_t* dst, int64_t ld);
int gf2_pack_rows_i64(const int64_t* src, int64_t m, int64_t n, int64_t src_stride, uint64_t* dst, int64_t ld);
/* The same with CSSCode's input test (css_code.py:39-44, "parity check matrix must be binary") made on the way: *other_out = 1
 * when some entry is neither 0 nor 1 (the packed rows are still entries & 1). */
int gf2_pack_rows_binary_u8(const uint8_t* src, int64_t m, int64_t n, int64_t src_stride, uint64_t* dst, int64_t ld, int* other_out);
int gf2_pack_rows_binary_i64(const int64_t* src, int64_t m, int64_t n, int64_t src_stride, uint64_t* dst, int64_t ld, int* other_out);
int gf2_unpack_rows_u8(const uint64_t* src, int64_t m, int64_t n, int64_t ld, uint8_t* dst, int64_t dst_stride);
int gf2_unpack_rows_i64(const uint64_t* src, int64_t m, int64_t n, int64_t ld, int64_t* dst, int64_t dst_stride);

/* ---- GF(2) linear algebra on host buffers -------------------------------------------------------- */

/* bin_matrix.reduced_row_echelon_form (bin_matrix.py:8-34).  In place on the packed matrix.
 * pivots_out (capacity min(m,n)) receives the pivot column of each of the first *rank_out rows. */
int gf2_rref(gf2_ctx* ctx, uint64_t* a, int64_t m, int64_t n, int64_t ld,
             int64_t* pivots_out, int64_t* rank_out);

/* Batched form: `batch` independent m x n matrices, matrix b at a + b*m*ld.  One workgroup per
 * matrix.  pivots_out: batch x min(m,n); rank_out: batch. */
int gf2_rref_batch(gf2_ctx* ctx, uint64_t* a, int64_t batch, int64_t m, int64_t n, int64_t ld,
                   int64_t* pivots_out, int64_t* rank_out);

/* Device-resident forms (asynchronous on the context's stream).  pivots_dev: batch x min(m,n) int64
 * (may be null); the first rank entries of a row are written, the others are left as they were or zeroed; rank_dev: batch
 * int64.  gf2_normalize_dev: swaps_dev capacity 2*r int64 (the first 2 * *nswaps_dev are written), nswaps_dev one
 * int64, status_dev one int (0 = ok, 1 = rows are not independent).
 * Alignment.  a_dev: any 8-byte-aligned address for matrices of at most 256 rows with ld <= 16 and ceil(m/64) * ld <= 32 (one
 * wavefront per matrix; contiguous rows at a 16-byte-aligned address are moved as 16-byte pieces), 16-byte aligned otherwise
 * (the blocked routes).  h_dev: 16-byte aligned.  pivots_dev, rank_dev, swaps_dev, nswaps_dev: any 8-byte-aligned address;
 * status_dev: any 4-byte-aligned address. */
int gf2_rref_batch_dev(gf2_ctx* ctx, uint64_t* a_dev, int64_t batch, int64_t m, int64_t n, int64_t ld,
                       int64_t* pivots_dev, int64_t* rank_dev);
int gf2_normalize_dev(gf2_ctx* ctx, uint64_t* h_dev, int64_t r, int64_t n, int64_t ld, int64_t offset,
                      int64_t* swaps_dev, int64_t* nswaps_dev, int* status_dev);

/* [build-defined; anchored on bin_matrix.py:8-34 + css_code.py:124-161]  Canonical
 * nullspace basis read off the RREF: row t has a 1 at free column F[t] and R[i,F[t]] at pivot column
 * P[i].  n_out needs capacity n rows of ldn words (at most n - rank are written); *rows_out = n-rank. */
int gf2_nullspace(gf2_ctx* ctx, const uint64_t* a, int64_t m, int64_t n, int64_t ld,
                  uint64_t* n_out, int64_t ldn, int64_t* rows_out);

/* css_code.normalize_parity_check (css_code.py:809-836).  In place; identity block lands in columns
 * offset..offset+r-1; swaps_out (capacity 2*r) receives (column, column) pairs in order.
 * Returns GF2_E_COLUMNS / GF2_E_DEPENDENT for the two reference exceptions. */
int gf2_normalize(gf2_ctx* ctx, uint64_t* h, int64_t r, int64_t n, int64_t ld, int64_t offset,
                  int64_t* swaps_out, int64_t* nswaps_out);

/* css_code.swap_columns (css_code.py:783-785).  In place. */
int gf2_swap_columns(gf2_ctx* ctx, uint64_t* a, int64_t m, int64_t n, int64_t ld, int64_t i, int64_t j);

/* np.mod(np.matmul(A, B.T), 2): the commutation check of css_code.py:47.  C is ra x rb packed
 * (ldc >= ceil(rb/64)). */
int gf2_matmul_abt(gf2_ctx* ctx, const uint64_t* a, int64_t ra, int64_t lda,
                   const uint64_t* b, int64_t rb, int64_t ldb, int64_t n,
                   uint64_t* c, int64_t ldc);

/* css_code.syndrome_table (css_code.py:715-735) for n <= 64, r <= 24 [SURVEY.md 8f item 2].  h_rows: r words, qubit j =
 * bit j.  table_out: 2^r words indexed by bin_matrix.vec_to_int(syndrome) (row 0 = most significant bit,
 * bin_matrix.py:36-43); an entry is the packed error of weight <= t with that syndrome, or all ones.  *t_out is the
 * decoding threshold the reference returns: the classes 0..t have pairwise distinct syndromes and class t + 1 does not
 * (or t = n, or t = max_weight when max_weight >= 0 [build-defined cap] is reached first).  *entries_out (may be null)
 * = number of filled entries. */
int gf2_syndrome_table(gf2_ctx* ctx, const uint64_t* h_rows, int64_t r, int64_t n, int64_t max_weight,
                       uint64_t* table_out, int64_t* t_out, int64_t* entries_out);

/* The same search for 64 < n <= 128 (SURVEY.md 8f item 2 names n = 23..127).  h_rows: r rows of two words.  A slot of table_out
 * (2^r words) holds (weight << 32) | rank -- the error's rank inside its weight class in the combinatorial number system
 * (positions c_1 < ... < c_w have rank C(c_1, 1) + ... + C(c_w, w)) -- or all ones; the caller unranks.  t_out, entries_out and
 * max_weight as above. */
int gf2_syndrome_table_wide(gf2_ctx* ctx, const uint64_t* h_rows, int64_t r, int64_t n, int64_t max_weight,
                            uint64_t* table_out, int64_t* t_out, int64_t* entries_out);

/* The same search for 128 < n <= 8192 (still r <= 24: the table has 2^r slots; beyond that the Python host enumerates the classes
 * and only the syndromes come from the device).  h_rows: r packed rows of ld words.  Errors are enumerated as position lists
 * and keyed by the XOR of their columns' keys; a class is enumerated only if it can fit the table (C(n, w) <= 2^r), which
 * keeps w <= 8 for every n > 128.  Table slots, t_out, entries_out and max_weight as in gf2_syndrome_table_wide. */
int gf2_syndrome_table_cols(gf2_ctx* ctx, const uint64_t* h_rows, int64_t r, int64_t n, int64_t ld, int64_t max_weight,
                            uint64_t* table_out, int64_t* t_out, int64_t* entries_out);

/* The same search beyond 24 checks [SURVEY.md 8f item 2: a k = 1 CSS code has r_1 + r_2 = n - 1, so from n = 51 on one of its
 * checks has more than 24 rows]: an open-addressing hash table on the device, sized from the weight classes it holds instead
 * of 2^r.  1 <= r <= 127, 1 <= n <= 8192, h_rows: r packed rows of ld words.  Keys are vec_to_int(syndrome) exactly (row 0 =
 * most significant bit): one word per entry for r <= 63, two (low word first) for 64 <= r <= 127 -- the reference's own keys
 * wrap beyond 63 bits (bin_matrix.py:40-43).  Output: *entries_out entries (the classes 0 .. t), in no particular order --
 * keys_out (1 or 2 words each) and vals_out = (weight << 32) | rank in the class (combinatorial number system, as above); they
 * are written only if capacity >= *entries_out (call again with larger buffers otherwise; capacity 0 just counts).  At most
 * 2^28 errors are enumerated in all: GF2_E_NOMEM if no collision has shown by then and max_weight (>= 0) does not stop the
 * search earlier. */
int gf2_syndrome_table_hashed(gf2_ctx* ctx, const uint64_t* h_rows, int64_t r, int64_t n, int64_t ld, int64_t max_weight,
                              uint64_t* keys_out, uint64_t* vals_out, int64_t capacity, int64_t* t_out, int64_t* entries_out);

/* css_code.transform_stabilisers (css_code.py:737-781) [SURVEY.md 8f item 3].  mat: k rows of ld words holding the k x 2n
 * stabiliser matrix [X | Z] (column j = bit j), rewritten in place.  gates: ngates rows of three int32 (kind, a, b):
 * kind 0 = H on qubit a (conjugate_h_with_check_mat, :757-767), kind 1 = CNOT control a target b
 * (conjugate_cnot_with_check_mat, :769-781).  Gates apply in order.  *stop_out = -1 and GF2_OK when all applied.
 * Otherwise mat holds the result of gates[0 : *stop_out] and the call returns GF2_E_NOTCSS (that gate is an H on a
 * qubit where some row has X and Z) or GF2_E_ARG (unknown kind / qubit outside [0, n): the reference's ValueErrors,
 * :747-755).  2n <= 20480. */
int gf2_conjugate_gates(gf2_ctx* ctx, uint64_t* mat, int64_t k, int64_t n, int64_t ld, const int32_t* gates,
                        int64_t ngates, int64_t* stop_out);

/* Row Hamming weights: np.sum(mat, axis=1) of css_code.is_doubly_even (css_code.py:846-850). */
int gf2_row_weights(gf2_ctx* ctx, const uint64_t* a, int64_t m, int64_t n, int64_t ld, uint32_t* weights_out);

/* ---- syndrome extraction -------------------------------------------------------------------------
 * np.mod(np.matmul(parity_check, e), 2) of css_code.py:728 for B errors at once
 * [build-defined batching, SURVEY.md 8a x2]. */

/* Uploads H and builds its device-side lookup tables.  The handle belongs to ctx. */
int gf2_check_create(gf2_ctx* ctx, const uint64_t* h, int64_t r, int64_t n, int64_t ld, gf2_check** check_out);
int gf2_check_destroy(gf2_ctx* ctx, gf2_check* check);

/* Tiled layout helpers: words per sample (even, >= ceil(n/64)) and words of a buffer for `batch` samples. */
int64_t gf2_tiled_ld(int64_t n);
int64_t gf2_tiled_words(int64_t n, int64_t batch);
/* Sample-major (batch x lde) -> tiled, both on the device; asynchronous.  Every word of the gf2_tiled_words(n, batch) is written
 * (pad samples and the pad word are zero).  e_dev: any 8-byte-aligned address; tiled_dev: 16-byte aligned. */
int gf2_retile_dev(gf2_ctx* ctx, const uint64_t* e_dev, int64_t batch, int64_t lde, int64_t n, uint64_t* tiled_dev);

/* Host buffers, synchronous. */
int gf2_syndrome_batch(gf2_ctx* ctx, const uint64_t* h, int64_t r, int64_t n, int64_t ldh,
                       const uint64_t* e, int64_t batch, int64_t lde, int layout,
                       uint64_t* s_out, int64_t lds);

/* Device buffers, asynchronous on the context's stream.
 * Sample-major: e_dev is batch x lde, s_dev is batch x lds (lds >= ceil(r/64)).  For n > 64 the errors are
 *               first re-tiled into context workspace (one extra streaming pass); keep resident data in
 *               GF2_LAYOUT_TILED to avoid it.
 * Tiled:        e_dev as described at GF2_LAYOUT_TILED (lde ignored); s_dev is slab-major: ceil(r/64) rows
 *               of lds >= batch words.
 * Bit-sliced:   e_dev is n x lde with lde >= ceil(batch/64); s_dev is r x lds, lds >= ceil(batch/64).
 * Words of a row of s_dev past the ones named are left as they were.  e_dev: 16-byte aligned in the tiled layout, else any
 * 8-byte-aligned address; s_dev: any 8-byte-aligned address (n, r <= 64: one word per sample, or even bit-sliced pitches,
 * at 16-byte-aligned addresses take 16-byte accesses). */
int gf2_syndrome_dev(gf2_ctx* ctx, const gf2_check* check, const uint64_t* e_dev, int64_t batch, int64_t lde,
                     int layout, uint64_t* s_dev, int64_t lds);

/* Sparse-error path: work proportional to the weight of each error.  Sample-major errors (batch x lde).  Produces the
 * sample-major syndromes (s_dev, batch x lds; may be null) and/or accumulates the syndrome-weight histogram (hist_dev
 * with r+1 uint64 bins; may be null) without materialising the syndromes.  Identical results to gf2_syndrome_dev;
 * faster when errors are sparse (DESIGN.md gives the crossover).  Fails for small checks (n, r <= 64) and r > 8192.
 * Three implementations behind it: batches of at least 32768 samples on a check with r <= 2048 and
 * n - r <= 2400 take the LDS row-slab pipeline (compact -> gather -> combine, plus a redo pass for columns left out of the
 * records), with or without syndromes stored (since round 4 every gather workgroup stores its slab's 64-byte piece); checks
 * with n <= 512 and r <= 256 the lane-per-sample kernel; everything else one wavefront per sample gathering columns of the
 * transposed check from L2.  Words of a syndrome row past ceil(r/64) (lds larger than needed) are either left as they were
 * or zeroed.  e_dev, s_dev, hist_dev: any 8-byte-aligned address (the slab pipeline runs its hand-scheduled gather kernel when
 * e_dev -- and s_dev, if given -- are 16-byte aligned with even pitches, its compiler-scheduled one otherwise). */
int gf2_syndrome_sparse_dev(gf2_ctx* ctx, const gf2_check* check, const uint64_t* e_dev, int64_t batch, int64_t lde,
                            uint64_t* s_dev, int64_t lds, uint64_t* hist_dev, int64_t nbins);

/* Histogram of packed syndromes (device), accumulated into hist_dev (uint64 bins).  layout
 * GF2_LAYOUT_SAMPLE_MAJOR: s_dev is batch x lds; GF2_LAYOUT_TILED: slab-major as written by gf2_syndrome_dev for
 * tiled errors (lds >= batch).  mode GF2_HIST_FULL needs r <= 24 and nbins == 2^r; GF2_HIST_WEIGHT needs
 * nbins == r+1.  s_dev, hist_dev: any 8-byte-aligned address. */
int gf2_histogram_dev(gf2_ctx* ctx, const uint64_t* s_dev, int64_t batch, int64_t lds, int layout, int64_t r,
                      int mode, uint64_t* hist_dev, int64_t nbins);

/* ---- Monte-Carlo --------------------------------------------------------------------------------
 * [build-defined, SURVEY.md 8a x3]  Sample `i` (global index) is a pure function of (seed, i); the
 * generator is specified in DESIGN.md ("Sampler") and restated in oracle/.  X errors are caught by
 * parity_check_c2, Z errors by parity_check_c1 (css_code.py:457-470). */

/* Writes packed errors for samples first_sample .. first_sample+count-1.  layout GF2_LAYOUT_SAMPLE_MAJOR:
 * count x lde; GF2_LAYOUT_TILED: gf2_tiled_words(n, count) words (lde ignored; pad samples are zero).  Sample-major: words of a
 * row past ceil(n/64) are zeroed or left as they were; ex_dev, ez_dev: any 8-byte-aligned address.  Tiled: 16-byte aligned. */
int gf2_sample_errors_dev(gf2_ctx* ctx, int64_t n, uint64_t seed, int64_t first_sample, int64_t count,
                          double p_x, double p_y, double p_z,
                          uint64_t* ex_dev, uint64_t* ez_dev, int64_t lde, int layout);

/* Full pipeline: sample -> syndromes -> histograms, chunked through device workspace owned by ctx.
 * hist_z (from H1 . e_z) and hist_x (from H2 . e_x) are host uint64 arrays, overwritten.  The same histograms whatever the
 * route: n <= 64: one fused kernel; mid-size checks: sampler + lane-per-sample kernel; n <= 4096 at sparse
 * rates with both checks in standard form: the record sampler (no packed rows) + gather / combine kernels of the LDS row-slab
 * pipeline; otherwise packed rows from the sampler through the sparse or the dense syndrome kernels.  The first call of a size
 * allocates the workspaces. */
int gf2_mc_run(gf2_ctx* ctx, const gf2_check* check_c1, const gf2_check* check_c2,
               uint64_t seed, int64_t first_sample, int64_t count,
               double p_x, double p_y, double p_z, int mode,
               uint64_t* hist_z, int64_t nbins_z, uint64_t* hist_x, int64_t nbins_x);

/* Table decode + logical-error tally [build-defined, SURVEY.md 8f item 1]: the classical content of
 * quil_classical_correct (css_code.py:649-685) and noisy_measure (css_code.py:599-646) applied to sampled errors.
 * Per sample: s_x = H2.e_x; if vec_to_int(s_x) is in the C2 syndrome table the correction is XOR-ed in, otherwise the
 * error is left unchanged (css_code.py:655-657); the logical Z measurement flips iff z_operator . residual_x is odd
 * (css_code.py:640-646).  Likewise for Z errors with H1, the C1 table and x_operator.  Small codes only (n <= 63,
 * r_1, r_2 <= 20).  table_c1 / table_c2: 2^r_1 / 2^r_2 host words indexed by vec_to_int(syndrome): the packed
 * correction, or ~0 where the table has no entry.  counts_out[5] = { logical X flips, logical Z flips, samples with
 * either flip, samples whose X syndrome has no table entry, samples whose Z syndrome has no table entry }. */
int gf2_mc_decode(gf2_ctx* ctx, const gf2_check* check_c1, const gf2_check* check_c2,
                  const uint64_t* table_c1, const uint64_t* table_c2, uint64_t x_operator, uint64_t z_operator,
                  uint64_t seed, int64_t first_sample, int64_t count, double p_x, double p_y, double p_z,
                  uint64_t* counts_out);

/* The same tally for codes of up to 128 qubits through hashed tables [SURVEY.md 8f item 1 for the mid-size codes of item 2]:
 * checks of up to 127 rows, tables given by their entries instead of 2^r dense words.  h1 / h2: packed rows (ld words each) of
 * parity_check_c1 / parity_check_c2; keys: vec_to_int(syndrome) of every table entry, one word each for r <= 63 and two (low
 * word first) beyond; corr: the entry's packed error, two words; x_operator / z_operator: two words each.  counts_out[5] as
 * above.  GF2_E_ARG if a key occurs twice. */
int gf2_mc_decode_hashed(gf2_ctx* ctx, int64_t n, int64_t ld, const uint64_t* h1, int64_t r1, const uint64_t* keys1,
                         const uint64_t* corr1, int64_t entries1, const uint64_t* h2, int64_t r2, const uint64_t* keys2,
                         const uint64_t* corr2, int64_t entries2, const uint64_t* x_operator, const uint64_t* z_operator,
                         uint64_t seed, int64_t first_sample, int64_t count, double p_x, double p_y, double p_z,
                         uint64_t* counts_out);

/* ---- weight-stratified Monte-Carlo ------------------------------------------------------------------
 * [build-defined, DESIGN.md "Strata"]  The sampler above draws the number of errors from a 32-bit table, so an event rarer than
 * 2^-32 per segment never occurs.  A stratum fixes the number of errors instead: stratified sample i of weight w over nb positions
 * (the n qubits of a code, the L fault locations of a circuit; always ONE segment) is a pure function of (seed, i, w) --
 * d = segment_draw(sample_key(seed, i), w), then for k = 0 .. w - 1 the sampler's error_draw(d, k, K := w, nb, t_1, t_2) with Floyd's
 * rule: a uniformly random w-subset with i.i.d. kinds, X : Y : Z = k_x : k_y : k_z (t_1 = quantise(k_x / s), t_2 =
 * quantise((k_x + k_y) / s), s = k_x + k_y + k_z > 0; a negative weight or s = 0 is GF2_E_ARG).  The tallies f_w of the strata
 * combine on the host, in double precision, to P_L(p) = sum_w C(nb, w) p^w (1 - p)^(nb - w) f_w for every p at once. */
#define GF2_STRATA_MAX                  256     /* strata per call                                                 */
#define GF2_STRATUM_MAX_POSITIONS  (1 << 20)    /* gf2_stratum_errors: nb                                          */

/* The definition on the host (no GPU needed): packed e_x, e_z rows (lde >= ceil(nb / 64) words each, pad bits zero) of the samples
 * first_sample .. first_sample + count - 1 of stratum w, 0 <= w <= nb, 1 <= nb <= GF2_STRATUM_MAX_POSITIONS. */
int gf2_stratum_errors(int64_t nb, int64_t w, uint64_t seed, int64_t first_sample, int64_t count, double k_x, double k_y, double k_z,
                       uint64_t* ex_out, uint64_t* ez_out, int64_t lde);

/* gf2_mc_decode_hashed over strata: stratum s has weights[s] errors (0 <= w <= n) and samples first_sample .. first_sample +
 * counts[s] - 1; counts_out is nstrata x 5 words in gf2_mc_decode's field order.  Column keys and hash tables are made once per
 * call.  Any code of at most 128 qubits with 1 <= r_1, r_2 <= 127 (small ones too); nstrata <= GF2_STRATA_MAX. */
int gf2_mc_decode_strata(gf2_ctx* ctx, int64_t n, int64_t ld, const uint64_t* h1, int64_t r1, const uint64_t* keys1,
                         const uint64_t* corr1, int64_t entries1, const uint64_t* h2, int64_t r2, const uint64_t* keys2,
                         const uint64_t* corr2, int64_t entries2, const uint64_t* x_operator, const uint64_t* z_operator,
                         uint64_t seed, int64_t first_sample, int64_t nstrata, const int32_t* weights, const int64_t* counts,
                         double k_x, double k_y, double k_z, uint64_t* counts_out);

/* ---- circuit-level faults of a Clifford circuit -------------------------------------------------------
 * [build-defined; the question the docstrings of noisy_encode_zero / noisy_encode_plus raise, css_code.py:203-312: "any
 * physical errors that occur during preparation may create many correlated errors in the code block"]  A Pauli-frame
 * Monte-Carlo over the fault locations of a gate list (DESIGN.md "Circuit faults").  Gates are rows (kind, a, b) as
 * gf2_conjugate_gates takes them, plus GF2_GATE_IDLE (no action on qubit a, one fault location; b ignored), which only these
 * entry points accept.  Locations in gate order: H and IDLE give one, (g, a); CNOT two, (g, a) then (g, b); L = their number.
 * Sample i draws its faults from the Monte-Carlo sampler with n := L -- every operand of a gate fails independently, a CNOT has
 * no correlated two-qubit fault, a qubit no gate touches has none.  The frame starts at zero; each gate acts (H: swap e_x[a],
 * e_z[a]; CNOT: e_x[b] ^= e_x[a], e_z[a] ^= e_z[b]), then its locations' faults are XOR-ed in.  An outcome row (row_x, row_z)
 * has the value row_x . e_x ^ row_z . e_z on the final frame. */
#define GF2_GATE_H     0
#define GF2_GATE_CNOT  1
#define GF2_GATE_IDLE  2
#define GF2_CIRCUIT_MAX_N          8192         /* gf2_circuit_effects: qubits                                    */
#define GF2_CIRCUIT_MAX_ROWS       16384        /* gf2_circuit_effects: outcome rows (identity(2n) up to n = 8192) */
#define GF2_CIRCUIT_MAX_LOCATIONS  (1 << 20)    /* gf2_circuit_create: fault locations                            */
#define GF2_CIRCUIT_MAX_LDR        8            /* gf2_circuit_create: words per effect (512 outcome rows)        */
typedef struct gf2_circuit gf2_circuit;         /* an effect table on the device */

/* Effect table (pure host code, no GPU needed).  rows_x / rows_z: nrows packed rows of ld words (n bits each).  *nloc_out = L.
 * eff_out[(2 l + c) * ldr + w]: bit r of the ldr-word vector = outcome r flips under an X (c = 0) or Z (c = 1) fault at
 * location l (a Y fault flips the XOR of both); pad bits zero.  locations_out (may be null): L pairs (gate, qubit).  Both are
 * written only if capacity >= L (capacity 0 just counts).  GF2_E_ARG: unknown kind, qubit outside [0, n), CNOT with a == b. */
int gf2_circuit_effects(const int32_t* gates, int64_t ngates, int64_t n, const uint64_t* rows_x, const uint64_t* rows_z,
                        int64_t nrows, int64_t ld, uint64_t* eff_out, int64_t ldr, int64_t capacity, int64_t* locations_out,
                        int64_t* nloc_out);

/* Uploads an effect table (host, 2 L ldr words).  1 <= L <= GF2_CIRCUIT_MAX_LOCATIONS, 1 <= ldr <= GF2_CIRCUIT_MAX_LDR. */
int gf2_circuit_create(gf2_ctx* ctx, const uint64_t* eff, int64_t locations, int64_t ldr, gf2_circuit** circuit_out);
int gf2_circuit_destroy(gf2_ctx* ctx, gf2_circuit* circuit);

/* Outcome words of samples first_sample .. first_sample + count - 1: out_dev is count x ldo (ldo >= ldr), sample-major; words
 * past ldr are left as they were.  Asynchronous on the context's stream.  out_dev: any 8-byte-aligned address. */
int gf2_circuit_outcomes_dev(gf2_ctx* ctx, const gf2_circuit* circuit, uint64_t seed, int64_t first_sample, int64_t count,
                             double p_x, double p_y, double p_z, uint64_t* out_dev, int64_t ldo);

/* Syndrome histograms of the final frame, as gf2_mc_run's (same modes, bins and host outputs).  The circuit's outcome words
 * must be laid out [key_x: kw(r_2)] [key_z: kw(r_1)] [parity: 1] with kw(r) = 1 word for r <= 63, else 2 (low word first):
 * key_x = vec_to_int(parity_check_c2 . e_x), key_z = vec_to_int(parity_check_c1 . e_z) (row 0 = most significant bit), parity
 * bit 0 = z_operator . e_x, bit 1 = x_operator . e_z; ldr = kw(r_2) + kw(r_1) + 1.  GF2_HIST_FULL needs r_1, r_2 <= 24; a
 * weight is the population count of the key.  1 <= r_1, r_2 <= 127. */
int gf2_mc_circuit_run(gf2_ctx* ctx, const gf2_circuit* circuit, int64_t r1, int64_t r2, uint64_t seed, int64_t first_sample,
                       int64_t count, double p_x, double p_y, double p_z, int mode, uint64_t* hist_z, int64_t nbins_z,
                       uint64_t* hist_x, int64_t nbins_x);

/* Table decode + logical tally of the final frame by gf2_mc_decode_hashed's rule (css_code.py:649-685, :640-646), same outcome
 * layout.  keys: vec_to_int(syndrome) of every table entry as gf2_mc_decode_hashed takes them; flips: one byte per entry,
 * z_operator . correction for C2's table (keys2, X errors), x_operator . correction for C1's.  A key found: the logical flip is
 * the parity bit XOR the entry's byte; not found: the parity bit, and the sample counts as uncorrectable.  counts_out[5] as
 * gf2_mc_decode's.  GF2_E_ARG if a key occurs twice. */
int gf2_mc_circuit_decode(gf2_ctx* ctx, const gf2_circuit* circuit, int64_t r1, const uint64_t* keys1, const uint8_t* flips1,
                          int64_t entries1, int64_t r2, const uint64_t* keys2, const uint8_t* flips2, int64_t entries2,
                          uint64_t seed, int64_t first_sample, int64_t count, double p_x, double p_y, double p_z,
                          uint64_t* counts_out);

/* gf2_mc_circuit_decode over strata (see "weight-stratified Monte-Carlo"): exactly weights[s] faults among the circuit's L
 * locations, 0 <= weights[s] <= min(L, GF2_CIRCUIT_STRATUM_MAX_WEIGHT); counts_out is nstrata x 5 words. */
#define GF2_CIRCUIT_STRATUM_MAX_WEIGHT 16
int gf2_mc_circuit_decode_strata(gf2_ctx* ctx, const gf2_circuit* circuit, int64_t r1, const uint64_t* keys1, const uint8_t* flips1,
                                 int64_t entries1, int64_t r2, const uint64_t* keys2, const uint8_t* flips2, int64_t entries2,
                                 uint64_t seed, int64_t first_sample, int64_t nstrata, const int32_t* weights, const int64_t* counts,
                                 double k_x, double k_y, double k_z, uint64_t* counts_out);

/* ---- exact strata: the low-weight fault configurations counted, not sampled --------------------------
 * [build-defined, DESIGN.md "Exact strata"]  A configuration of weight w of a circuit with L locations and effect table eff is a
 * pair (S, kappa): S = {s_0 < ... < s_{w-1}} a subset of [0, L), kappa in {1, 2, 3}^w with the sampler's kind bits (1 = X, 2 = Z,
 * 3 = Y).  Its outcome words are the XOR over k of eff[s_k][0] if kappa_k & 1 and of eff[s_k][1] if kappa_k & 2; it is decoded and
 * tallied exactly by gf2_mc_circuit_decode's rule (same outcome layout, same tables and flip bytes, the same five fields).
 * rank(S) = sum_k C(s_k, k + 1) (the combinatorial number system: a bijection onto [0, C(L, w)), colexicographic order; w = 0
 * has the single rank 0).  A call covers the subsets of ranks [first_rank, first_rank + count), each with all 3^w kind
 * assignments.  counts_out[(w + 1)][(w + 1)][5]: entry [n_x][n_y][field] is the tally of `field` over the configurations of the
 * range with n_x X faults, n_y Y faults and w - n_x - n_y Z faults (entries with n_x + n_y > w are zero).  For kind weights
 * (k_x, k_y, k_z) of sum s the host then has f_w = sum counts[n_x][n_y] k_x^n_x k_y^n_y k_z^n_z / (s^w C(L, w)), exactly.
 * 0 <= w <= min(L, GF2_ENUMERATE_MAX_WEIGHT).  GF2_E_ARG if C(L, w) >= 2^63, if count * 3^w >= 2^63, or if the range leaves
 * [0, C(L, w)). */
#define GF2_ENUMERATE_MAX_WEIGHT 8

/* The inverse of rank (host code): the w positions, ascending, of the subset of [0, nb) with that rank.  1 <= nb <= 2^20,
 * 0 <= w <= min(nb, GF2_ENUMERATE_MAX_WEIGHT), 0 <= rank < min(C(nb, w), 2^63). */
int gf2_subset_unrank(int64_t nb, int64_t w, int64_t rank, int32_t* positions_out);

/* The definition on the host: serial, no GPU needed.  eff: 2 * locations * ldr words as gf2_circuit_effects writes them. */
int gf2_circuit_enumerate_host(const uint64_t* eff, int64_t locations, int64_t ldr, int64_t r1, const uint64_t* keys1,
                               const uint8_t* flips1, int64_t entries1, int64_t r2, const uint64_t* keys2, const uint8_t* flips2,
                               int64_t entries2, int64_t w, int64_t first_rank, int64_t count, uint64_t* counts_out);

/* The same counts on the device: the hash tables are made once, the range is cut into launches of bounded size, the counts come
 * back once. */
int gf2_circuit_enumerate(gf2_ctx* ctx, const gf2_circuit* circuit, int64_t r1, const uint64_t* keys1, const uint8_t* flips1,
                          int64_t entries1, int64_t r2, const uint64_t* keys2, const uint8_t* flips2, int64_t entries2, int64_t w,
                          int64_t first_rank, int64_t count, uint64_t* counts_out);

/* ---- the error-correction cycle: Steane's gadget under circuit-level faults ---------------------------
 * [build-defined, DESIGN.md "Error-correction cycle"; CSSCode.error_correct, css_code.py:436-470]  Two additions to the frame model,
 * accepted by gf2_circuit_effects_timed only.  GF2_GATE_RESET on a clears the frame of a (e_x[a] = e_z[a] = 0), then its one fault
 * location (g, a) models a preparation fault.  Every outcome row r has a time row_time[r] in [0, ngates]: its value is
 * row_x . e_x ^ row_z . e_z on the frame just before gate row_time[r] acts (ngates: the final frame).  A measurement is a set of
 * timed rows, its error an IDLE gate on every measured qubit immediately before.  With all times = ngates and no RESET the table
 * is gf2_circuit_effects' bit for bit.  Same limits and errors, plus GF2_E_ARG for a time outside [0, ngates]. */
#define GF2_GATE_RESET 3
int gf2_circuit_effects_timed(const int32_t* gates, int64_t ngates, int64_t n, const uint64_t* rows_x, const uint64_t* rows_z,
                              int64_t nrows, int64_t ld, uint64_t* eff_out, int64_t ldr, int64_t capacity, int64_t* locations_out,
                              int64_t* nloc_out, const int64_t* row_time);

/* Outcome words of a cycle of `rounds` rounds, ldr = 1 + rounds + F (F >= 1 words of flag rows), 1 <= r_1, r_2 <= 31:
 *   word 0, the final data frame: bits 0 .. r_2 - 1 key_x = vec_to_int(parity_check_c2 . e_x) (row 0 the most significant of the r_2
 *     bits), bit 31 z_operator . e_x, bits 32 .. 32 + r_1 - 1 key_z, bit 63 x_operator . e_z;
 *   words 1 .. rounds: round t's measured key_x in bits 0 .. r_2 - 1 and key_z in bits 32 .. 32 + r_1 - 1;
 *   words rounds + 1 .. ldr - 1: the flag rows (the verifications of the ancilla preparations), in measurement order.
 * Tally rule per sample: accepted iff every flag word is zero (repeat-until-success as post-selection).  Accepted, on each side
 * independently (x: key_x, parity_check_c2's table, flip bytes z_operator . correction; z: key_z, c1's, x_operator . correction),
 * with K = 0 and P = 0: for t = 1 .. rounds, s = key_t ^ K; found: K ^= s, P ^= the entry's flip byte; not found: nothing is
 * recorded (css_code.py:655-657) and round_unmatched counts once.  Then s = key_final ^ K, flip = parity_final ^ P; found:
 * flip ^= the entry's flip byte; not found: uncorrectable counts.  counts[GF2_EC_FIELDS]: accepted, logical_x, logical_z,
 * logical_any, uncorrectable_x, uncorrectable_z, round_unmatched_x, round_unmatched_z -- all but the first among accepted samples. */
#define GF2_EC_FIELDS 8
#define GF2_EC_MAX_ROUNDS 6

/* The rule on the host, serial, no GPU needed: words is count x ldw (ldw >= ldr); keys are one word per entry, tables as
 * gf2_mc_circuit_decode takes them.  class_out (may be null): one byte per sample, bit 0 accepted, bit 1 flip_x, bit 2 flip_z, bit 3
 * uncorrectable x, bit 4 uncorrectable z (0 for a rejected sample).  GF2_E_ARG, naming the limit: r > 31, rounds outside
 * [1, GF2_EC_MAX_ROUNDS], ldr > GF2_CIRCUIT_MAX_LDR, ldr < rounds + 2, a key twice in a table. */
int gf2_ec_tally_host(const uint64_t* words, int64_t count, int64_t ldw, int64_t ldr, int64_t rounds, int64_t r1, const uint64_t* keys1,
                      const uint8_t* flips1, int64_t entries1, int64_t r2, const uint64_t* keys2, const uint8_t* flips2,
                      int64_t entries2, uint64_t* counts_out, uint8_t* class_out);

/* The same tally of samples first_sample .. first_sample + count - 1 on the device, drawn as gf2_circuit_outcomes_dev draws them;
 * no outcome word is stored.  The circuit's ldr must be 1 + rounds + F, and its effects may set no bit outside the keys, the two
 * parity bits and the flag words.  counts_out[GF2_EC_FIELDS] on the host. */
int gf2_mc_ec_decode(gf2_ctx* ctx, const gf2_circuit* circuit, int64_t rounds, int64_t r1, const uint64_t* keys1, const uint8_t* flips1,
                     int64_t entries1, int64_t r2, const uint64_t* keys2, const uint8_t* flips2, int64_t entries2, uint64_t seed,
                     int64_t first_sample, int64_t count, double p_x, double p_y, double p_z, uint64_t* counts_out);

/* ---- the fault-tolerant logical measurement: a rewritten one-qubit program under circuit-level faults ----
 * [build-defined, DESIGN.md "Logical measurement"; ftqc.rewrite_program, ftqc.py:76-95; CSSCode.measure / noisy_measure,
 * css_code.py:542-646]  The program is a sequence of steps in program order, nsteps of them, and bit s of measure_mask says that
 * step s is a MEASURE step (one trial of the logical measurement) and not an EC step (one round of error_correct on the data).
 * Outcome words, ldr = nsteps + F (F >= 1 words of flag rows), 1 <= r_1, r_2 <= 31, ldr <= GF2_FT_MAX_LDR:
 *   word s of an EC step: the measured key_x in bits 0 .. r_2 - 1 and key_z in bits 32 .. 32 + r_1 - 1 (row 0 the most significant);
 *   word s of a MEASURE step: key_x in bits 0 .. r_2 - 1 and z_operator . e_x of the measured ancilla in bit 31; the high half zero;
 *   words nsteps .. ldr - 1: the flag rows (the verifications of every preparation), in measurement order.
 * There is no final-frame word: the result is classical.  Tally rule per sample (quil_classical_correct, css_code.py:649-685, which
 * corrections and measurements share because both update data.x_errors): accepted iff every flag word is zero.  Accepted, with
 * K_x = P_x = K_z = P_z = 0, for s = 0 .. nsteps - 1: an EC step does, on each side, v = key ^ K; found: K ^= v, P ^= the entry's
 * flip byte; not found: unmatched counts.  A MEASURE step does the same on the x side only, and then its trial is wrong iff
 * bit 31 ^ P_x is 1.  The sample is wrong iff more than half of its trials are.  counts[GF2_FT_FIELDS]: accepted, wrong,
 * trial_wrong (wrong trials summed), first_trial_wrong, split_vote (trials not unanimous), unmatched_x, unmatched_z -- all but the
 * first among accepted samples. */
#define GF2_FT_FIELDS  7
#define GF2_FT_MAX_LDR 16

/* The rule on the host, serial, no GPU needed (replaces running the rewritten program's classical side, css_code.py:542-589 and
 * :649-685, per sample): words is count x ldw (ldw >= ldr), tables as gf2_ec_tally_host takes them.  class_out (may be null): one
 * byte per sample, bit 0 accepted, bit 1 wrong, bit 2 first trial wrong, bit 3 split vote, bit 4 an unmatched x key, bit 5 an
 * unmatched z key (0 for a rejected sample).  GF2_E_ARG, naming the limit: r > 31, ldr > GF2_FT_MAX_LDR, nsteps outside
 * [1, ldr - 1], a measure_mask with bits at or above nsteps or with an even number of bits, a key twice in a table. */
int gf2_ft_tally_host(const uint64_t* words, int64_t count, int64_t ldw, int64_t ldr, int64_t nsteps, uint64_t measure_mask, int64_t r1,
                      const uint64_t* keys1, const uint8_t* flips1, int64_t entries1, int64_t r2, const uint64_t* keys2,
                      const uint8_t* flips2, int64_t entries2, uint64_t* counts_out, uint8_t* class_out);

/* gf2_circuit_create for the effect table of a rewritten program (ftqc.py:76-95): 1 <= ldr <= GF2_FT_MAX_LDR words per effect.
 * The circuit is destroyed by gf2_circuit_destroy.  One with ldr > GF2_CIRCUIT_MAX_LDR is taken by gf2_ft_outcomes_dev and
 * gf2_mc_ft_decode only: every other entry point refuses it with GF2_E_ARG. */
int gf2_ft_circuit_create(gf2_ctx* ctx, const uint64_t* eff, int64_t locations, int64_t ldr, gf2_circuit** circuit_out);

/* gf2_circuit_outcomes_dev for 1 <= ldr <= GF2_FT_MAX_LDR (the rewritten program run once per sample, test_fidelity.py's loop):
 * words past ldr are left as they were; out_dev: any 8-byte-aligned address. */
int gf2_ft_outcomes_dev(gf2_ctx* ctx, const gf2_circuit* circuit, uint64_t seed, int64_t first_sample, int64_t count, double p_x,
                        double p_y, double p_z, uint64_t* out_dev, int64_t ldo);

/* The tally of samples first_sample .. first_sample + count - 1 on the device (test_fidelity.py's trial loop over the rewritten
 * program), drawn as gf2_ft_outcomes_dev draws them; no outcome word is stored.  The circuit's ldr must be nsteps + F with
 * 8 <= ldr <= GF2_FT_MAX_LDR, and its effects may set no bit outside the layout above.  counts_out[GF2_FT_FIELDS] on the host. */
int gf2_mc_ft_decode(gf2_ctx* ctx, const gf2_circuit* circuit, int64_t nsteps, uint64_t measure_mask, int64_t r1, const uint64_t* keys1,
                     const uint8_t* flips1, int64_t entries1, int64_t r2, const uint64_t* keys2, const uint8_t* flips2, int64_t entries2,
                     uint64_t seed, int64_t first_sample, int64_t count, double p_x, double p_y, double p_z, uint64_t* counts_out);

/* ---- exact strata of the two post-selected gadgets ----------------------------------------------------
 * [build-defined, DESIGN.md "Exact strata of the cycle" and "Exact strata of the measurement"]  The notions of "exact strata" above,
 * unchanged: a configuration (S, kappa) of weight w, its outcome words the XOR of its picks' effects, rank(S) in the combinatorial
 * number system, a call covering ranks [first_rank, first_rank + count) with all 3^w kind assignments each, 0 <= w <=
 * min(L, GF2_ENUMERATE_MAX_WEIGHT), the same range errors.  What differs is the judgement: the tally rule per sample of the
 * error-correction cycle (gf2_ec_tally_host) or of the logical measurement (gf2_ft_tally_host), post-selection included.
 * counts_out[(w + 1)][(w + 1)][F], F = GF2_EC_FIELDS or GF2_FT_FIELDS: entry [n_x][n_y][field] over the configurations of the range
 * with that kind composition; field 0 is `accepted`, the others count among accepted configurations.  Counts of disjoint ranges add.
 * With kind weights (k_x, k_y, k_z) of sum s, A_w(field) = sum counts[n_x][n_y][field] k_x^n_x k_y^n_y k_z^n_z / s^w, and
 * P(accepted and field) = sum_w A_w p^w (1 - p)^(L - w) at total fault probability p per location.
 *
 * The definitions on the host, serial, no GPU needed (they stand for running the gadget once per fault configuration:
 * CSSCode.error_correct, css_code.py:436-470, with its classical side :649-685; ftqc.rewrite_program, ftqc.py:76-95, with
 * CSSCode.measure, css_code.py:542-589 -- test_fidelity.py's trial loop, one trial per configuration).  eff: 2 * locations * ldr
 * words as gf2_circuit_effects_timed writes them.  Argument errors as gf2_ec_tally_host's / gf2_ft_tally_host's (r > 31, rounds,
 * nsteps, the mask, ldr, the tables) and gf2_circuit_enumerate_host's (weight, range), plus GF2_E_ARG for effects that set bits
 * outside the layout. */
int gf2_ec_enumerate_host(const uint64_t* eff, int64_t locations, int64_t ldr, int64_t rounds, int64_t r1, const uint64_t* keys1,
                          const uint8_t* flips1, int64_t entries1, int64_t r2, const uint64_t* keys2, const uint8_t* flips2,
                          int64_t entries2, int64_t w, int64_t first_rank, int64_t count, uint64_t* counts_out);
int gf2_ft_enumerate_host(const uint64_t* eff, int64_t locations, int64_t ldr, int64_t nsteps, uint64_t measure_mask, int64_t r1,
                          const uint64_t* keys1, const uint8_t* flips1, int64_t entries1, int64_t r2, const uint64_t* keys2,
                          const uint8_t* flips2, int64_t entries2, int64_t w, int64_t first_rank, int64_t count, uint64_t* counts_out);

/* The same counts on the device (css_code.py:436-470 and ftqc.py:76-95 as above).  The circuit is one of gf2_circuit_create
 * (the cycle: ldr = 1 + rounds + F, 3 <= ldr <= GF2_CIRCUIT_MAX_LDR) or of either constructor (the measurement: ldr = nsteps + F,
 * 8 <= ldr <= GF2_FT_MAX_LDR); its effects may set no bit outside the layout, as gf2_mc_ec_decode / gf2_mc_ft_decode require.
 * The hash tables are made once, the range is cut into launches of bounded size, the counts come back once. */
int gf2_ec_enumerate(gf2_ctx* ctx, const gf2_circuit* circuit, int64_t rounds, int64_t r1, const uint64_t* keys1, const uint8_t* flips1,
                     int64_t entries1, int64_t r2, const uint64_t* keys2, const uint8_t* flips2, int64_t entries2, int64_t w,
                     int64_t first_rank, int64_t count, uint64_t* counts_out);
int gf2_ft_enumerate(gf2_ctx* ctx, const gf2_circuit* circuit, int64_t nsteps, uint64_t measure_mask, int64_t r1, const uint64_t* keys1,
                     const uint8_t* flips1, int64_t entries1, int64_t r2, const uint64_t* keys2, const uint8_t* flips2, int64_t entries2,
                     int64_t w, int64_t first_rank, int64_t count, uint64_t* counts_out);

/* ---- exact strata of the two post-selected gadgets under gate-level faults -----------------------------
 * [build-defined, DESIGN.md section 5e]  The same effect tables, outcome layouts and tally rules, but what fails is a gate, not a
 * location.  A site is one gate of the gadget's gate list: a one-operand gate (H, IDLE, RESET) with its one location l, or a CNOT
 * with its two locations l (control) and l + 1 (target).  Sites are numbered with the n_1 one-operand gates first, then the n_2
 * CNOTs, each in gate order; site_loc[s] is the first location of site s, and the sites partition [0, L): n_1 + 2 n_2 = L.  A kind
 * is a non-zero mask kappa: 2 bits on a one-operand site (1 = X, 2 = Z, 3 = Y), 4 bits on a CNOT site (bits 0, 1: the control's X
 * and Z components; bits 2, 3: the target's).  A pick's outcome words are the XOR over the set bits t of
 * eff[site_loc + (t >> 1)][t & 1].  A CNOT kind is two-operand when both halves of kappa are non-zero (9 of the 15).
 * A configuration of weight w and CNOT count b is a = w - b distinct one-operand sites, b distinct CNOT sites and a kind per pick
 * (3^a 15^b per subset), judged by the gadget's tally rule, post-selection included.  rank = r_s + C(n_1, a) r_c with r_s, r_c the
 * ranks of the one-operand picks among [0, n_1) and of the CNOT picks among [0, n_2) in the combinatorial number system.  A call
 * covers ranks [first_rank, first_rank + count) of one (w, b), 0 <= b <= w <= GF2_GATE_ENUMERATE_MAX_WEIGHT.
 * counts_out[(b + 1)][F], F = GF2_EC_FIELDS or GF2_FT_FIELDS: entry [c][field] is the tally of `field` over the configurations of
 * the range in which exactly c of the b CNOT picks carry a two-operand kind.  Counts of disjoint ranges add.
 * GF2_E_ARG if C(n_1, a) C(n_2, b) >= 2^63, if count 3^a 15^b >= 2^63, if the range leaves the rank space or if the site table is no
 * partition of [0, L); layout, table and effect errors as gf2_ec_enumerate_host's / gf2_ft_enumerate_host's.
 *
 * The definitions on the host, serial, no GPU needed (they stand for running the gadget once per gate-fault configuration,
 * css_code.py:436-470 and ftqc.py:76-95 as above). */
#define GF2_GATE_ENUMERATE_MAX_WEIGHT 4
int gf2_ec_gate_enumerate_host(const uint64_t* eff, int64_t locations, int64_t ldr, int64_t rounds, int64_t r1, const uint64_t* keys1,
                               const uint8_t* flips1, int64_t entries1, int64_t r2, const uint64_t* keys2, const uint8_t* flips2,
                               int64_t entries2, const int32_t* site_loc, int64_t n1, int64_t n2, int64_t w, int64_t b, int64_t first_rank,
                               int64_t count, uint64_t* counts_out);
int gf2_ft_gate_enumerate_host(const uint64_t* eff, int64_t locations, int64_t ldr, int64_t nsteps, uint64_t measure_mask, int64_t r1,
                               const uint64_t* keys1, const uint8_t* flips1, int64_t entries1, int64_t r2, const uint64_t* keys2,
                               const uint8_t* flips2, int64_t entries2, const int32_t* site_loc, int64_t n1, int64_t n2, int64_t w, int64_t b,
                               int64_t first_rank, int64_t count, uint64_t* counts_out);

/* The same counts on the device.  Circuit, layout and tables as gf2_ec_enumerate / gf2_ft_enumerate check them; the hash tables and
 * the device copy of site_loc are made once per call, the range is cut into launches of at most 2^28 configurations, the counts
 * come back once. */
int gf2_ec_gate_enumerate(gf2_ctx* ctx, const gf2_circuit* circuit, int64_t rounds, int64_t r1, const uint64_t* keys1, const uint8_t* flips1,
                          int64_t entries1, int64_t r2, const uint64_t* keys2, const uint8_t* flips2, int64_t entries2,
                          const int32_t* site_loc, int64_t n1, int64_t n2, int64_t w, int64_t b, int64_t first_rank, int64_t count,
                          uint64_t* counts_out);
int gf2_ft_gate_enumerate(gf2_ctx* ctx, const gf2_circuit* circuit, int64_t nsteps, uint64_t measure_mask, int64_t r1, const uint64_t* keys1,
                          const uint8_t* flips1, int64_t entries1, int64_t r2, const uint64_t* keys2, const uint8_t* flips2, int64_t entries2,
                          const int32_t* site_loc, int64_t n1, int64_t n2, int64_t w, int64_t b, int64_t first_rank, int64_t count,
                          uint64_t* counts_out);

/* ---- malignant fault sets of the two post-selected gadgets ---------------------------------------------
 * [build-defined, DESIGN.md "Malignant fault sets of the cycle" and "Malignant fault sets of the measurement"]  The walk of "exact
 * strata of the two post-selected gadgets" above, unchanged -- ranks [first_rank, first_rank + count) of weight w, all 3^w kind
 * assignments each, the same judgement -- but the configurations of a chosen class are listed instead of counted.  A
 * configuration's class byte is the byte gf2_ec_tally_host / gf2_ft_tally_host write to class_out for its outcome words (bit 0
 * accepted; the cycle: bit 1 flip_x, 2 flip_z, 3 uncorrectable x, 4 uncorrectable z; the measurement: bit 1 wrong, 2 first trial
 * wrong, 3 split vote, 4 an unmatched x key, 5 an unmatched z key; 0 for a rejected configuration).  `select` is a non-empty subset of
 * the rule's class bits, and a configuration is listed iff it is accepted and (class & select) != 0: select = 1 lists every
 * accepted configuration.  A record is GF2_FAULT_RECORD_WORDS words:
 *   word 0: rank(S) in the combinatorial number system, absolute (the rank first_rank counts in);
 *   word 1: bits 0 .. 15 the kinds code sum_j kind_j 3^j, kind_j = 0 X, 1 Y, 2 Z the kind of the j-th pick in ascending location
 *           order; bits 32 .. 39 the class byte; every other bit zero.
 * *found_out is the number of listed configurations of the range, whatever the capacity; records_out (capacity records) holds them
 * sorted by (word 0, kinds code) ascending and is written only if capacity >= *found_out (call again with a larger buffer
 * otherwise; capacity 0 just counts, and records_out may then be null).  The lists of disjoint ranges concatenate.
 *
 * The definitions on the host, serial, no GPU needed: gf2_ec_enumerate_host's / gf2_ft_enumerate_host's walk, rule and argument
 * errors, plus GF2_E_ARG for select == 0, for a select bit outside the rule's class bits and for capacity < 0. */
#define GF2_FAULT_RECORD_WORDS 2
#define GF2_EC_CLASS_BITS 0x1full
#define GF2_FT_CLASS_BITS 0x3full
#define GF2_FAULT_LIST_MAX_CAPACITY (1ll << 28)  /* records a device list may hold (4 GiB) */
int gf2_ec_enumerate_list_host(const uint64_t* eff, int64_t locations, int64_t ldr, int64_t rounds, int64_t r1, const uint64_t* keys1,
                               const uint8_t* flips1, int64_t entries1, int64_t r2, const uint64_t* keys2, const uint8_t* flips2,
                               int64_t entries2, int64_t w, int64_t first_rank, int64_t count, uint64_t select, int64_t capacity,
                               uint64_t* records_out, int64_t* found_out);
int gf2_ft_enumerate_list_host(const uint64_t* eff, int64_t locations, int64_t ldr, int64_t nsteps, uint64_t measure_mask, int64_t r1,
                               const uint64_t* keys1, const uint8_t* flips1, int64_t entries1, int64_t r2, const uint64_t* keys2,
                               const uint8_t* flips2, int64_t entries2, int64_t w, int64_t first_rank, int64_t count, uint64_t select,
                               int64_t capacity, uint64_t* records_out, int64_t* found_out);

/* The same lists from the device.  Circuit, layout, tables and range as gf2_ec_enumerate / gf2_ft_enumerate check them, the list's
 * arguments as above, and capacity <= GF2_FAULT_LIST_MAX_CAPACITY.  The range is cut into the same launches; a wavefront that has
 * anything to list takes its slots with one atomic add on a 64-bit counter that is zeroed once per call and runs on across the
 * launches, and a record is stored only if its slot is below capacity.  The call allocates `capacity` records on the device,
 * downloads them only when *found_out <= capacity and sorts them on the host by (word 0, kinds code): the result does not depend
 * on the order the wavefronts arrived in and is byte-identical to the host statement's. */
int gf2_ec_enumerate_list(gf2_ctx* ctx, const gf2_circuit* circuit, int64_t rounds, int64_t r1, const uint64_t* keys1, const uint8_t* flips1,
                          int64_t entries1, int64_t r2, const uint64_t* keys2, const uint8_t* flips2, int64_t entries2, int64_t w,
                          int64_t first_rank, int64_t count, uint64_t select, int64_t capacity, uint64_t* records_out, int64_t* found_out);
int gf2_ft_enumerate_list(gf2_ctx* ctx, const gf2_circuit* circuit, int64_t nsteps, uint64_t measure_mask, int64_t r1, const uint64_t* keys1,
                          const uint8_t* flips1, int64_t entries1, int64_t r2, const uint64_t* keys2, const uint8_t* flips2, int64_t entries2,
                          int64_t w, int64_t first_rank, int64_t count, uint64_t select, int64_t capacity, uint64_t* records_out,
                          int64_t* found_out);

/* ---- malignant fault sets under gate-level faults ------------------------------------------------------
 * [build-defined, DESIGN.md section 5e "Malignant fault sets under gate-level faults"]  The walk of "exact strata of the two
 * post-selected gadgets under gate-level faults" above, unchanged -- site table, ranks [first_rank, first_rank + count) of one
 * (w, b), all 3^a 15^b kind assignments each, the same judgement -- but the configurations of a chosen class are listed instead of
 * counted.  Class byte and `select` as "malignant fault sets" above define them (GF2_EC_CLASS_BITS, GF2_FT_CLASS_BITS): a
 * configuration is listed iff it is accepted and (class & select) != 0.  A record is GF2_FAULT_RECORD_WORDS words:
 *   word 0: the rank r_s + C(n_1, a) r_c within (w, b), absolute (the rank first_rank counts in);
 *   word 1: bits 0 .. 15 the kind masks kappa of the picks, one nibble each: the a one-operand picks first in ascending site order
 *           (kappa in 1 .. 3), then the b CNOT picks in ascending site order (kappa in 1 .. 15, the bit meaning above); bits
 *           32 .. 39 the class byte; every other bit zero.  The number c of two-operand kinds is a function of the record.
 * *found_out is the number of listed configurations of the range, whatever the capacity; records_out (capacity records) holds them
 * sorted by (word 0, word 1 bits 0 .. 15) ascending and is written only if capacity >= *found_out (capacity 0 just counts, and
 * records_out may then be null).  The lists of disjoint ranges concatenate.
 *
 * The definitions on the host, serial, no GPU needed: gf2_ec_gate_enumerate_host's / gf2_ft_gate_enumerate_host's walk, rule and
 * argument errors, plus GF2_E_ARG for select == 0, for a select bit outside the rule's class bits and for capacity < 0. */
int gf2_ec_gate_enumerate_list_host(const uint64_t* eff, int64_t locations, int64_t ldr, int64_t rounds, int64_t r1, const uint64_t* keys1,
                                    const uint8_t* flips1, int64_t entries1, int64_t r2, const uint64_t* keys2, const uint8_t* flips2,
                                    int64_t entries2, const int32_t* site_loc, int64_t n1, int64_t n2, int64_t w, int64_t b,
                                    int64_t first_rank, int64_t count, uint64_t select, int64_t capacity, uint64_t* records_out,
                                    int64_t* found_out);
int gf2_ft_gate_enumerate_list_host(const uint64_t* eff, int64_t locations, int64_t ldr, int64_t nsteps, uint64_t measure_mask, int64_t r1,
                                    const uint64_t* keys1, const uint8_t* flips1, int64_t entries1, int64_t r2, const uint64_t* keys2,
                                    const uint8_t* flips2, int64_t entries2, const int32_t* site_loc, int64_t n1, int64_t n2, int64_t w,
                                    int64_t b, int64_t first_rank, int64_t count, uint64_t select, int64_t capacity, uint64_t* records_out,
                                    int64_t* found_out);

/* The same lists from the device.  Every check of gf2_ec_gate_enumerate / gf2_ft_gate_enumerate, the list's arguments as above, and
 * capacity <= GF2_FAULT_LIST_MAX_CAPACITY.  The hash tables and the device copy of site_loc are made once per call and the range is
 * cut into launches of at most 2^28 configurations; ranks stay absolute across them.  A wavefront that has anything to list takes
 * its slots with one atomic add on a 64-bit counter that is zeroed once per call and runs on across the launches, and a record is
 * stored only if its slot is below capacity.  The call allocates `capacity` records on the device, downloads them only when
 * *found_out <= capacity and sorts them on the host by (word 0, kind masks): the result does not depend on the order the wavefronts
 * arrived in, nor on what an earlier call left in the workspace, and is byte-identical to the host statement's. */
int gf2_ec_gate_enumerate_list(gf2_ctx* ctx, const gf2_circuit* circuit, int64_t rounds, int64_t r1, const uint64_t* keys1, const uint8_t* flips1,
                               int64_t entries1, int64_t r2, const uint64_t* keys2, const uint8_t* flips2, int64_t entries2,
                               const int32_t* site_loc, int64_t n1, int64_t n2, int64_t w, int64_t b, int64_t first_rank, int64_t count,
                               uint64_t select, int64_t capacity, uint64_t* records_out, int64_t* found_out);
int gf2_ft_gate_enumerate_list(gf2_ctx* ctx, const gf2_circuit* circuit, int64_t nsteps, uint64_t measure_mask, int64_t r1, const uint64_t* keys1,
                               const uint8_t* flips1, int64_t entries1, int64_t r2, const uint64_t* keys2, const uint8_t* flips2, int64_t entries2,
                               const int32_t* site_loc, int64_t n1, int64_t n2, int64_t w, int64_t b, int64_t first_rank, int64_t count,
                               uint64_t select, int64_t capacity, uint64_t* records_out, int64_t* found_out);

/* ---- sampled strata of the two post-selected gadgets ----------------------------------------------------
 * [build-defined, DESIGN.md "Sampled strata of the cycle" and "Sampled strata of the measurement"]  The two notions above combined,
 * neither changed: stratified sample i of weight w over the gadget's L locations is the pure function of (seed, i, w) of
 * "weight-stratified Monte-Carlo" (one segment, Floyd's rule, kinds X : Y : Z = k_x : k_y : k_z), its outcome words are the XOR of
 * its picks' effects, and the words are judged by the tally rule per sample of the error-correction cycle (gf2_ec_tally_host) or of
 * the logical measurement (gf2_ft_tally_host), post-selection included.  With a_w = accepted / N_w and n_w = field / N_w of
 * stratum w, P(accepted and field) = sum_w C(L, w) p^w (1 - p)^(L - w) n_w and the conditional rate is the ratio of two such sums.
 *
 * The definition on the host, serial, no GPU needed (it stands for running the gadget once per stratified sample:
 * CSSCode.error_correct, css_code.py:436-470; ftqc.rewrite_program, ftqc.py:76-95, with CSSCode.measure, css_code.py:542-589): the
 * outcome words of samples first_sample .. first_sample + count - 1 of stratum w.  eff: 2 * locations * ldr words as
 * gf2_circuit_effects_timed writes them, 1 <= locations <= GF2_CIRCUIT_MAX_LOCATIONS, 1 <= ldr <= GF2_FT_MAX_LDR,
 * 0 <= w <= min(L, GF2_CIRCUIT_STRATUM_MAX_WEIGHT); words_out is count x ldw (ldw >= ldr), words past ldr are left as they were.
 * gf2_ec_tally_host / gf2_ft_tally_host applied to words_out complete the statement. */
int gf2_stratum_outcomes_host(const uint64_t* eff, int64_t locations, int64_t ldr, int64_t w, uint64_t seed, int64_t first_sample,
                              int64_t count, double k_x, double k_y, double k_z, uint64_t* words_out, int64_t ldw);

/* gf2_mc_ec_decode over strata (css_code.py:436-470 with its classical side :649-685, once per stratified sample): stratum s has
 * exactly weights[s] faults among the circuit's L locations, 0 <= weights[s] <= min(L, GF2_CIRCUIT_STRATUM_MAX_WEIGHT), and samples
 * first_sample .. first_sample + counts[s] - 1; counts_out is nstrata x GF2_EC_FIELDS words.  Circuit, layout and tables as
 * gf2_mc_ec_decode requires them (ldr = 1 + rounds + F, 3 <= ldr <= GF2_CIRCUIT_MAX_LDR, no effect bit outside the layout); strata
 * arguments as gf2_mc_circuit_decode_strata requires them (nstrata <= GF2_STRATA_MAX, non-negative counts and first_sample, the kind
 * weights).  The hash tables are made once per call, the counts come back once. */
int gf2_mc_ec_decode_strata(gf2_ctx* ctx, const gf2_circuit* circuit, int64_t rounds, int64_t r1, const uint64_t* keys1,
                            const uint8_t* flips1, int64_t entries1, int64_t r2, const uint64_t* keys2, const uint8_t* flips2,
                            int64_t entries2, uint64_t seed, int64_t first_sample, int64_t nstrata, const int32_t* weights,
                            const int64_t* counts, double k_x, double k_y, double k_z, uint64_t* counts_out);

/* gf2_mc_ft_decode over strata (ftqc.py:76-95 and css_code.py:542-589, test_fidelity.py's trial loop with one trial per stratified
 * sample), likewise: the circuit's ldr = nsteps + F with 8 <= ldr <= GF2_FT_MAX_LDR; counts_out is nstrata x GF2_FT_FIELDS words. */
int gf2_mc_ft_decode_strata(gf2_ctx* ctx, const gf2_circuit* circuit, int64_t nsteps, uint64_t measure_mask, int64_t r1,
                            const uint64_t* keys1, const uint8_t* flips1, int64_t entries1, int64_t r2, const uint64_t* keys2,
                            const uint8_t* flips2, int64_t entries2, uint64_t seed, int64_t first_sample, int64_t nstrata,
                            const int32_t* weights, const int64_t* counts, double k_x, double k_y, double k_z, uint64_t* counts_out);

/* ---- sampled strata of the two post-selected gadgets under gate-level faults ---------------------------
 * [build-defined, DESIGN.md section 5e "Sampled strata under gate-level faults"]  The sites, kind masks and outcome rule of "exact
 * strata ... under gate-level faults" above and the generator of "weight-stratified Monte-Carlo", combined.  A stratum is a pair
 * (a, b): exactly a faulty one-operand gates and b faulty CNOTs, 0 <= a <= n_1, 0 <= b <= n_2, a + b <= GF2_GATE_STRATUM_MAX_WEIGHT.
 * Sample i of stratum (a, b) is a pure function of (seed, i, a, b): ks = sample_key(seed, i), d = segment_draw(ks, 64 + 17 b + a)
 * (the slot carries the stratum and starts above every location stratum's), and for pick k = 0 .. a + b - 1 with
 * v = mix64(d + G (k + 1)), hi = v >> 32, lo = v & 0xFFFFFFFF:
 *   k < a:   j = n_1 - a + k, t = (hi (j + 1)) >> 32; the site is t unless an earlier pick is t, then j (Floyd's rule);
 *            kappa = 1 + ((lo * 3) >> 32);
 *   k >= a:  m = k - a, j = n_2 - b + m, t = (hi (j + 1)) >> 32; the CNOT index is t unless an earlier CNOT pick is t, then j; the
 *            site is n_1 + that index; kappa = 1 + ((lo * 15) >> 32).
 * The outcome words are the XOR over the picks and the set bits t of each kappa of eff[site_loc[site] + (t >> 1)][t & 1]; c is the
 * number of CNOT picks with a two-operand kind; the sample is judged by the gadget's tally rule, post-selection included, and
 * tallied into row c.  counts[c][field] / N estimates the exact strata's counts[a + b][b][c][field] / (C(n_1, a) C(n_2, b) 3^a 15^b).
 *
 * The definition on the host, serial, no GPU needed: the outcome words (count x ldw, ldw >= ldr, the words past ldr left as they
 * were, 1 <= ldr <= GF2_FT_MAX_LDR) and one byte c per sample of samples first_sample .. first_sample + count - 1.
 * gf2_ec_tally_host / gf2_ft_tally_host applied to the words, grouped by c, complete the statement.  GF2_E_ARG for a stratum outside
 * the limits above, a site table that is no partition of [0, L), a negative count or first_sample. */
#define GF2_GATE_STRATUM_MAX_WEIGHT 16
int gf2_gate_stratum_outcomes_host(const uint64_t* eff, int64_t locations, int64_t ldr, const int32_t* site_loc, int64_t n1, int64_t n2,
                                   int64_t a, int64_t b, uint64_t seed, int64_t first_sample, int64_t count, uint64_t* words_out,
                                   int64_t ldw, uint8_t* two_operand_out);

/* The tallies on the device: stratum s is (a[s], b[s]) with samples first_sample .. first_sample + counts[s] - 1; counts_out is
 * nstrata x (GF2_GATE_STRATUM_MAX_WEIGHT + 1) x F words [stratum][c][field], F = GF2_EC_FIELDS or GF2_FT_FIELDS, the rows c > b zero.
 * Circuit, layout and tables as gf2_mc_ec_decode_strata / gf2_mc_ft_decode_strata check them, the site table as
 * gf2_ec_gate_enumerate checks it, nstrata <= GF2_STRATA_MAX, every (a, b) within the limits above, non-negative counts and
 * first_sample.  The hash tables and the device copy of site_loc are made once per call, a stratum is cut into launches of at most
 * 2^36 samples, the counts come back once. */
int gf2_mc_ec_decode_gate_strata(gf2_ctx* ctx, const gf2_circuit* circuit, int64_t rounds, int64_t r1, const uint64_t* keys1,
                                 const uint8_t* flips1, int64_t entries1, int64_t r2, const uint64_t* keys2, const uint8_t* flips2,
                                 int64_t entries2, const int32_t* site_loc, int64_t n1, int64_t n2, uint64_t seed, int64_t first_sample,
                                 int64_t nstrata, const int32_t* a, const int32_t* b, const int64_t* counts, uint64_t* counts_out);
int gf2_mc_ft_decode_gate_strata(gf2_ctx* ctx, const gf2_circuit* circuit, int64_t nsteps, uint64_t measure_mask, int64_t r1,
                                 const uint64_t* keys1, const uint8_t* flips1, int64_t entries1, int64_t r2, const uint64_t* keys2,
                                 const uint8_t* flips2, int64_t entries2, const int32_t* site_loc, int64_t n1, int64_t n2, uint64_t seed,
                                 int64_t first_sample, int64_t nstrata, const int32_t* a, const int32_t* b, const int64_t* counts,
                                 uint64_t* counts_out);

/* ---- direct Monte-Carlo of the two post-selected gadgets under gate-level faults ---------------------------
 * [build-defined, DESIGN.md section 5e "Direct Monte-Carlo under gate-level faults"]  Every gate fails on its own: a one-operand
 * gate with probability p_1 and one of its 3 kinds, a CNOT as one event with probability p_2 and one of its 15.  The sites, kind
 * masks and outcome rule are those of "exact strata ... under gate-level faults" above, the draw is the sampler's ("Monte-Carlo"
 * above) run once per class of sites, the kind rule that of the sampled gate strata.  Sample i is a pure function of
 * (seed, i, p_1, p_2, n_1, n_2): ks = sample_key(seed, i), and for each of the two classes
 *   one-operand sites:  m = n_1, radix 3,  site base 0,   T = quantise(p_1), slot base GF2_GATE_MC_SLOT_ONE;
 *   CNOT sites:         m = n_2, radix 15, site base n_1, T = quantise(p_2), slot base GF2_GATE_MC_SLOT_CNOT
 * cut into segments s = 0, 1, ... of 512 sites (nb = 512, or m - 512 s in the last; a class with m = 0 has none):
 *   d = segment_draw(ks, slot base + s);  K = #{k < nb : (d >> 32) >= cdf[k]}, cdf = the inverse binomial CDF table of (T, nb);
 *   for k < K: v = mix64(d + G (k + 1)), j = nb - K + k, t = ((v >> 32) (j + 1)) >> 32; the position is t unless an earlier pick
 *   of this segment took t, then j (Floyd's rule); kappa = 1 + (((v & 0xFFFFFFFF) radix) >> 32); site = site base + 512 s + position.
 * L <= 2^20 gives at most 2048 segments per class, so the two classes, the location sampler (slots below 2048) and every stratum
 * (slots below 353) are disjoint streams of one seed.  The outcome words are the XOR over the picks and the set bits t of each kappa
 * of eff[site_loc[site] + (t >> 1)][t & 1]; the sample is judged by the gadget's tally rule, post-selection included.  As for the
 * sampler, an event rarer than 2^-32 per segment never occurs, and the kinds are uniform up to 2^-28 relative.
 *
 * The definition on the host, serial, no GPU needed: the outcome words (count x ldw, ldw >= ldr, the words past ldr left as they
 * were, 1 <= ldr <= GF2_FT_MAX_LDR) of samples first_sample .. first_sample + count - 1 and, unless faults_out is null, int32
 * [count][3] = (a, b, c): faulty one-operand gates, faulty CNOTs, CNOT picks with a two-operand kind.  gf2_ec_tally_host /
 * gf2_ft_tally_host applied to the words complete the statement.  GF2_E_ARG for p_1 or p_2 outside [0, 1] (NaN included), a site
 * table that is no partition of [0, L), a negative count or first_sample, ldw < ldr, ldr outside [1, GF2_FT_MAX_LDR]. */
#define GF2_GATE_MC_SLOT_ONE  4096              /* first segment slot of the one-operand sites                     */
#define GF2_GATE_MC_SLOT_CNOT 8192              /* ... and of the CNOT sites                                       */
int gf2_gate_outcomes_host(const uint64_t* eff, int64_t locations, int64_t ldr, const int32_t* site_loc, int64_t n1, int64_t n2,
                           uint64_t seed, int64_t first_sample, int64_t count, double p1, double p2, uint64_t* words_out, int64_t ldw,
                           int32_t* faults_out);

/* The tallies on the device: counts_out[GF2_EC_FIELDS] / counts_out[GF2_FT_FIELDS] of samples first_sample .. first_sample +
 * count - 1, as gf2_mc_ec_decode / gf2_mc_ft_decode give them.  Circuit, layout, tables and site table as
 * gf2_mc_ec_decode_gate_strata / gf2_mc_ft_decode_gate_strata check them, rates and range as the host statement does.  The four
 * inverse-CDF tables, the hash tables and the device copy of site_loc are made per call and freed with it: the calls keep no state
 * in the context.  A call is cut into launches of at most 2^36 samples. */
int gf2_mc_ec_decode_gate(gf2_ctx* ctx, const gf2_circuit* circuit, int64_t rounds, int64_t r1, const uint64_t* keys1,
                          const uint8_t* flips1, int64_t entries1, int64_t r2, const uint64_t* keys2, const uint8_t* flips2,
                          int64_t entries2, const int32_t* site_loc, int64_t n1, int64_t n2, uint64_t seed, int64_t first_sample,
                          int64_t count, double p1, double p2, uint64_t* counts_out);
int gf2_mc_ft_decode_gate(gf2_ctx* ctx, const gf2_circuit* circuit, int64_t nsteps, uint64_t measure_mask, int64_t r1,
                          const uint64_t* keys1, const uint8_t* flips1, int64_t entries1, int64_t r2, const uint64_t* keys2,
                          const uint8_t* flips2, int64_t entries2, const int32_t* site_loc, int64_t n1, int64_t n2, uint64_t seed,
                          int64_t first_sample, int64_t count, double p1, double p2, uint64_t* counts_out);

/* ---- streamed gadgets: error-correction cycles and programs of any length, block by block ---------------
 * [build-defined, DESIGN.md "Streamed gadgets"]  Both ancilla blocks are RESET at the start of every preparation, so only the data
 * block survives from one block of a gadget -- the first preparation, an EC round, a MEASURE trial -- to the next.  A fault inside a
 * block therefore acts through three words: `local`, what it flips of its own block's measured word (the layout of an EC or a
 * MEASURE step's word above); `tail`, what it leaves on the data frame at the block's end (word 0 of a cycle's layout: key_x in bits
 * 0 .. r_2 - 1, z_operator . e_x in bit 31, key_z in bits 32 .. 32 + r_1 - 1, x_operator . e_z in bit 63); `flags`, what it flips
 * of its own block's flag rows in measurement order (at most 64 rows per block).  A gadget is a sequence of blocks, each of a block
 * TYPE (a table of 2 * locations * 3 words: per location the three words of an X fault, then those of a Z fault -- gf2_circuit_effects_timed's
 * table of the block's gate list at ldr = 3) and a KIND that says what its word is:
 *   GF2_STREAM_NONE     no word (the first preparation); its local words must be zero
 *   GF2_STREAM_EC       a round of error_correct: an EC step
 *   GF2_STREAM_MEASURE  a trial of the logical measurement: a MEASURE step
 *   GF2_STREAM_FINAL    the judgement of the final data frame: a pseudo-block of no locations, block type -1, the last block
 * Fault locations are numbered through the blocks in order, L <= GF2_CIRCUIT_MAX_LOCATIONS in all, and sample i has the faults
 * gf2_circuit_outcomes_dev draws for a circuit of L locations.  With T = 0, the blocks in order: the block's step word is
 * mask_kind(T) ^ (XOR of its faults' local words) -- an EC step reads T's two keys, a MEASURE step key_x and bit 31, the FINAL step all
 * of T -- then T ^= XOR of its faults' tail words.  Stream layout of a sample, nsteps + F words: [step 0 .. nsteps - 1] [F >= 1 flag
 * words: the flag rows of all blocks in order, 64 per word].  A sequence has either one FINAL step as its last step or an odd number
 * of MEASURE steps and no FINAL step.  Tally rule per sample: gf2_ec_tally_host's and gf2_ft_tally_host's, word for word -- accepted
 * iff every flag word is zero; one record (K, P) per side through the steps in order; an EC step updates both sides, a MEASURE
 * step the x side only and reads its trial against the updated record; the FINAL step judges T against the record.
 * counts[GF2_STREAM_FIELDS]: accepted; the FINAL step's logical_x, logical_z, logical_any, uncorrectable_x, uncorrectable_z;
 * unmatched_x, unmatched_z over the EC and MEASURE steps; wrong, trial_wrong, first_trial_wrong, split_vote over the MEASURE steps
 * (zero without any) -- all but the first among accepted samples. */
#define GF2_STREAM_FIELDS 12
#define GF2_STREAM_NONE 0
#define GF2_STREAM_EC 1
#define GF2_STREAM_MEASURE 2
#define GF2_STREAM_FINAL 3
#define GF2_STREAM_MAX_TYPES 64
#define GF2_STREAM_MAX_OVERLAP 8
typedef struct gf2_stream gf2_stream;

/* The words on the host, serial, no GPU needed: sample i has the faults fault_first[i] .. fault_first[i + 1] - 1 (fault_first[0] = 0),
 * each a location in [0, L) and a kind 1 (X), 2 (Z) or 3 (Y); words_out is count x ldw (ldw >= nsteps + F), words past nsteps + F are
 * left as they were.  type_eff holds the types' tables one after the other; type_flags[t] <= 64 is the number of flag rows of type
 * t.  GF2_E_ARG, naming the limit: ntypes outside [1, GF2_STREAM_MAX_TYPES], a type without locations, more than 64 flag rows in a
 * block, flag bits at or above a type's rows, a block type or kind out of range, a FINAL step that is not last or has a type,
 * neither a FINAL step nor an odd number of MEASURE steps, L > 2^20, a fault outside [0, L) or of no kind. */
int gf2_stream_words_host(const uint64_t* type_eff, const int64_t* type_locations, const int64_t* type_flags, int64_t ntypes,
                          const int32_t* block_type, const int32_t* block_kind, int64_t nblocks, const int64_t* fault_first,
                          const int32_t* fault_location, const uint8_t* fault_kind, int64_t count, uint64_t* words_out, int64_t ldw);

/* The tally rule on the host over stream-layout words (count x ldw, ldw >= nsteps + flag_words), serial, no GPU needed and no bound
 * on the steps; the steps are the blocks whose kind is not NONE.  Tables as gf2_ec_tally_host takes them.  class_out (may be
 * null): one byte per sample, bit 0 accepted, bit 1 flip_x, bit 2 flip_z, bit 3 uncorrectable x, bit 4 uncorrectable z, bit 5 wrong,
 * bit 6 first trial wrong, bit 7 split vote (0 for a rejected sample).  GF2_E_ARG, naming the limit: r > 31, the kind rules above,
 * flag_words < 1, a key twice in a table. */
int gf2_stream_tally_host(const uint64_t* words, int64_t count, int64_t ldw, const int32_t* block_kind, int64_t nblocks, int64_t flag_words,
                          int64_t r1, const uint64_t* keys1, const uint8_t* flips1, int64_t entries1, int64_t r2, const uint64_t* keys2,
                          const uint8_t* flips2, int64_t entries2, uint64_t* counts_out, uint8_t* class_out);

/* A sequence on the device: the types' tables and where every block lies.  Argument rules as gf2_stream_words_host's; in addition
 * no 512-location segment of the sampler may overlap more than GF2_STREAM_MAX_OVERLAP blocks (the FINAL step counts with the last
 * segment): GF2_E_ARG, naming it.  Destroyed by gf2_stream_destroy. */
int gf2_stream_create(gf2_ctx* ctx, const uint64_t* type_eff, const int64_t* type_locations, const int64_t* type_flags, int64_t ntypes,
                      const int32_t* block_type, const int32_t* block_kind, int64_t nblocks, gf2_stream** stream_out);
int gf2_stream_destroy(gf2_ctx* ctx, gf2_stream* stream);

/* The stream-layout words of samples first_sample .. first_sample + count - 1, rejected ones included: ldo >= nsteps + F words per
 * sample in device memory; words past nsteps + F are left as they were.  out_dev: any 8-byte-aligned address. */
int gf2_stream_outcomes_dev(gf2_ctx* ctx, const gf2_stream* stream, uint64_t seed, int64_t first_sample, int64_t count, double p_x,
                            double p_y, double p_z, uint64_t* out_dev, int64_t ldo);

/* The tally of those samples on the device, no word stored: time and memory per sample are linear in the number of blocks.
 * GF2_E_ARG when the sequence's effects set a bit outside the layout given r_1 and r_2.  counts_out[GF2_STREAM_FIELDS] on the host. */
int gf2_mc_stream_decode(gf2_ctx* ctx, const gf2_stream* stream, int64_t r1, const uint64_t* keys1, const uint8_t* flips1, int64_t entries1,
                         int64_t r2, const uint64_t* keys2, const uint8_t* flips2, int64_t entries2, uint64_t seed, int64_t first_sample,
                         int64_t count, double p_x, double p_y, double p_z, uint64_t* counts_out);

/* ---- multi-block streamed programs: several logical qubits and the transversal CNOT, block by block ------------
 * [build-defined, DESIGN.md section 5d "Multi-block programs"]  The streamed route above with one data frame per logical qubit,
 * T[0 .. nframes - 1], 1 <= nframes <= GF2_MSTREAM_MAX_FRAMES.  A block is (type, kind, a, b): the blocks of the kinds NONE, EC and
 * MEASURE are the streamed route's, serving data frame a (b = -1), with the same tables -- they do not depend on which data block
 * they serve.  The new kind is
 *   GF2_MSTREAM_CNOT    the n physical CNOTs of a transversal CNOT from data block a to data block b != a: 2 n locations, no step
 *                       word, no flag rows (type_flags = 0, third word zero); a table row's first word is the tail the fault leaves
 *                       on frame a, its second word the tail it leaves on frame b (gf2_circuit_effects_timed on the block's own gate
 *                       list over the two data blocks, final-frame rows of block a in word 0 and of block b in word 1)
 * There is no FINAL step.  Fault locations are numbered through the blocks in order, L <= GF2_CIRCUIT_MAX_LOCATIONS, and sample i has
 * the faults gf2_circuit_outcomes_dev draws for a circuit of L locations.  With every T = 0, the blocks in order: a CNOT block applies
 *   T_b ^= T_a & 0x00000000FFFFFFFF  (key_x and z_operator . e_x: X errors copy control -> target)
 *   T_a ^= T_b & 0xFFFFFFFF00000000  (key_z and x_operator . e_z: Z errors copy target -> control)
 * then T_a ^= XOR of its faults' first words, T_b ^= XOR of their second words.  Any other block: its step word is
 * mask_kind(T_a) ^ (XOR of its faults' local words), then T_a ^= XOR of their tails.  The carried words suffice because T is linear in
 * the frame and both blocks use the same checks and operators.  A sample's words, nsteps + F: [the EC and MEASURE steps in order]
 * [F >= 1 flag words].  The MEASURE steps of one frame follow one another (EC steps between them) and form one measurement; a frame is
 * measured at most once, there is at least one measurement, and all have the same odd number of trials <= GF2_MSTREAM_MAX_TRIALS.
 *
 * Tally rule per sample: accepted iff every flag word is zero; one record (K, P) per side AND per data frame; an EC or MEASURE step
 * updates the record of its own frame by the streamed rule, word for word.  `records` says what a CNOT block does to the records:
 *   GF2_MSTREAM_REFERENCE    nothing (the rewritten program moves no known-error register through a CNOT)
 *   GF2_MSTREAM_PROPAGATED   the map above on (K, P): the x side a -> b, the z side b -> a
 * The words do not depend on `records`.  counts[GF2_MSTREAM_FIELDS]: accepted, wrong_any (some measurement's vote is wrong),
 * unmatched_x, unmatched_z; then per measurement in program order, four of them: wrong, trial_wrong, first_trial_wrong, split_vote
 * (zero for an absent measurement) -- all but the first among accepted samples.  Counts of sample ranges add. */
#define GF2_MSTREAM_FIELDS 20
#define GF2_MSTREAM_MAX_FRAMES 4
#define GF2_MSTREAM_MAX_TRIALS 255
#define GF2_MSTREAM_CNOT 4
#define GF2_MSTREAM_REFERENCE 0
#define GF2_MSTREAM_PROPAGATED 1
typedef struct gf2_mstream gf2_mstream;

/* The words on the host, serial, no GPU needed; faults and words_out as gf2_stream_words_host takes them.  GF2_E_ARG, naming the
 * limit: the type rules of gf2_stream_words_host; nframes outside [1, GF2_MSTREAM_MAX_FRAMES]; a kind that is not NONE, EC, MEASURE or
 * CNOT (a FINAL step is named); a frame outside [0, nframes); a CNOT block whose frames coincide or whose type has flag rows; another
 * block whose second frame is not -1; a frame measured twice; no MEASURE step; measurements of different or even numbers of trials;
 * L > 2^20; a fault outside [0, L) or of no kind. */
int gf2_mstream_words_host(const uint64_t* type_eff, const int64_t* type_locations, const int64_t* type_flags, int64_t ntypes,
                           const int32_t* block_type, const int32_t* block_kind, const int32_t* block_a, const int32_t* block_b, int64_t nblocks,
                           int64_t nframes, const int64_t* fault_first, const int32_t* fault_location, const uint8_t* fault_kind, int64_t count,
                           uint64_t* words_out, int64_t ldw);

/* The tally rule on the host over such words (count x ldw, ldw >= nsteps + flag_words), serial, no GPU needed.  Tables as
 * gf2_ec_tally_host takes them.  class_out (may be null): one byte per sample, bit 0 accepted, bit 1 wrong_any, bits 2 .. 5 wrong of
 * measurement 0 .. 3, bit 6 an unmatched key, bit 7 a split vote (0 for a rejected sample).  GF2_E_ARG, naming the limit: r > 31,
 * the block rules above, records neither REFERENCE nor PROPAGATED, flag_words < 1, a key twice in a table. */
int gf2_mstream_tally_host(const uint64_t* words, int64_t count, int64_t ldw, const int32_t* block_kind, const int32_t* block_a,
                           const int32_t* block_b, int64_t nblocks, int64_t nframes, int64_t flag_words, int64_t records, int64_t r1,
                           const uint64_t* keys1, const uint8_t* flips1, int64_t entries1, int64_t r2, const uint64_t* keys2,
                           const uint8_t* flips2, int64_t entries2, uint64_t* counts_out, uint8_t* class_out);

/* A sequence on the device.  Argument rules as gf2_mstream_words_host's; in addition no 512-location segment of the sampler may
 * overlap more than GF2_STREAM_MAX_OVERLAP blocks: GF2_E_ARG, naming it.  Destroyed by gf2_mstream_destroy. */
int gf2_mstream_create(gf2_ctx* ctx, const uint64_t* type_eff, const int64_t* type_locations, const int64_t* type_flags, int64_t ntypes,
                       const int32_t* block_type, const int32_t* block_kind, const int32_t* block_a, const int32_t* block_b, int64_t nblocks,
                       int64_t nframes, gf2_mstream** mstream_out);
int gf2_mstream_destroy(gf2_ctx* ctx, gf2_mstream* mstream);

/* The words of samples first_sample .. first_sample + count - 1, rejected ones included: ldo >= nsteps + F words per sample in
 * device memory; words past nsteps + F are left as they were.  out_dev: any 8-byte-aligned address. */
int gf2_mstream_outcomes_dev(gf2_ctx* ctx, const gf2_mstream* mstream, uint64_t seed, int64_t first_sample, int64_t count, double p_x,
                             double p_y, double p_z, uint64_t* out_dev, int64_t ldo);

/* The tally of those samples on the device, no word stored.  GF2_E_ARG when the sequence's effects set a bit outside the layout
 * given r_1 and r_2, or records is neither value.  counts_out[GF2_MSTREAM_FIELDS] on the host. */
int gf2_mc_mstream_decode(gf2_ctx* ctx, const gf2_mstream* mstream, int64_t records, int64_t r1, const uint64_t* keys1, const uint8_t* flips1,
                          int64_t entries1, int64_t r2, const uint64_t* keys2, const uint8_t* flips2, int64_t entries2, uint64_t seed,
                          int64_t first_sample, int64_t count, double p_x, double p_y, double p_z, uint64_t* counts_out);

/* ---- repeat-until-success: every preparation of a streamed gadget retried on its own ------------------------
 * [build-defined, DESIGN.md section 5d "Repeat-until-success"]  The streamed route gives every preparation one attempt and rejects a
 * sample when any verification fires.  Here a block type is cut into REGIONS, consecutive (first location, count, retried) that
 * partition its locations in order; a retried region (a preparation with its verifications) is redrawn until its own flag rows are
 * zero.  Locations fail independently and a flag row depends on one region only, so the accepted samples have the distribution
 * post-selection gives, at a cost linear in the number of blocks.  type_regions holds the types' regions one after the other, three
 * int64 each; type_nregions[t] is their number for type t.  Besides the sequence rules of gf2_stream_words_host, GF2_E_ARG naming
 * the rule: regions that do not partition a type's locations in order, a region that is not retried whose locations set a flag
 * bit, two regions of a type whose flag masks (OR of the flag words of a region's locations) intersect, max_attempts outside
 * [1, GF2_RETRY_MAX_ATTEMPTS], more than GF2_RETRY_MAX_SIZES distinct segment sizes (one inverse-CDF table each).
 *
 * Sample i is a pure function of (seed, i, p_x, p_y, p_z, the sequence, its regions, max_attempts).  ks = sample_key(seed, i).
 * Region g -- the g-th region of the whole sequence, counted through the blocks in order -- and attempt a = 0, 1, ... have the keys
 *   kr = segment_draw(ks, 2^32 + g),  ka = mix64(kr + G (a + 1)).
 * The region's locations are cut into segments s = 0, 1, ... of 512 from its first location (nb = 512, or what is left in its last
 * segment): d = segment_draw(ka, s), K = #{k < nb : (d >> 32) >= cdf[k]} with the inverse binomial CDF table of (T_any, nb), and the
 * picks, Floyd's rule and the kinds are the location sampler's (error_draw).  The slots 2^32 + g lie above those of every other
 * stream of a seed.  A region that is not retried uses a = 0.  A retried one takes the first a < max_attempts whose flags are
 * zero, and only that attempt's local and tail words enter the block; the key of (g, a) never depends on how many attempts earlier
 * regions took.  With none the sample is EXHAUSTED: the walk stops, the step words from that block on stay 0 and the flag words
 * hold the last attempt's flags at that block's flag rows.  Blocks, steps and tally as "streamed gadgets" above.
 * Layout of a sample, nsteps + F + 1 words: [step 0 .. nsteps - 1] [F flag words, zero for an accepted sample] [attempts: the
 * sample's attempts over all its retried regions]. */
#define GF2_RETRY_FIELDS 14                     /* the GF2_STREAM_FIELDS (accepted: not exhausted), exhausted, attempts */
#define GF2_RETRY_MAX_ATTEMPTS 65536
#define GF2_RETRY_MAX_SIZES 16                  /* distinct segment sizes of a sequence's regions: the kernel's inverse-CDF tables */
typedef struct gf2_retry gf2_retry;

/* The words on the host, serial, no GPU needed: words_out is count x ldw (ldw >= nsteps + F + 1), the words past those left as
 * they were.  attempts_out (may be null): uint32 [count][retried regions of the sequence], the attempts of every preparation in
 * order, 0 for one never reached.  gf2_stream_tally_host on the first nsteps + F words completes the statement: an exhausted sample
 * has a non-zero flag word and is rejected there.  GF2_E_ARG also for a negative count or first_sample and for bad rates. */
int gf2_retry_words_host(const uint64_t* type_eff, const int64_t* type_locations, const int64_t* type_flags, int64_t ntypes,
                         const int32_t* block_type, const int32_t* block_kind, int64_t nblocks, const int64_t* type_regions,
                         const int64_t* type_nregions, uint64_t seed, int64_t first_sample, int64_t count, double p_x, double p_y, double p_z,
                         int64_t max_attempts, uint64_t* words_out, int64_t ldw, uint32_t* attempts_out);

/* A sequence and its regions on the device.  Argument rules as gf2_retry_words_host's (max_attempts belongs to the calls).
 * Destroyed by gf2_retry_destroy. */
int gf2_retry_create(gf2_ctx* ctx, const uint64_t* type_eff, const int64_t* type_locations, const int64_t* type_flags, int64_t ntypes,
                     const int32_t* block_type, const int32_t* block_kind, int64_t nblocks, const int64_t* type_regions,
                     const int64_t* type_nregions, gf2_retry** retry_out);
int gf2_retry_destroy(gf2_ctx* ctx, gf2_retry* retry);

/* The words of samples first_sample .. first_sample + count - 1 in device memory, ldo >= nsteps + F + 1 words per sample; words past
 * those are left as they were.  out_dev: any 8-byte-aligned address. */
int gf2_retry_outcomes_dev(gf2_ctx* ctx, const gf2_retry* retry, uint64_t seed, int64_t first_sample, int64_t count, double p_x, double p_y,
                           double p_z, int64_t max_attempts, uint64_t* out_dev, int64_t ldo);

/* The tally of those samples on the device, no word stored.  counts_out[GF2_RETRY_FIELDS] on the host: the twelve streamed fields
 * with accepted = not exhausted, then exhausted, then the attempts of all samples of the call.  Counts of sample ranges add.  The
 * inverse-CDF tables are made per call and freed with it: the calls keep no state beyond the handle. */
int gf2_mc_retry_decode(gf2_ctx* ctx, const gf2_retry* retry, int64_t r1, const uint64_t* keys1, const uint8_t* flips1, int64_t entries1,
                        int64_t r2, const uint64_t* keys2, const uint8_t* flips2, int64_t entries2, uint64_t seed, int64_t first_sample,
                        int64_t count, double p_x, double p_y, double p_z, int64_t max_attempts, uint64_t* counts_out);

/* ---- repeat-until-success with waiting faults on the data block ------------------------------------------
 * [build-defined, DESIGN.md section 5d "Repeat-until-success with waiting faults"]  The retried walk above, in which the data block
 * also pays for the retries: a retried region g has W_g WAIT ROWS, the (local, tail) words of an X and of a Z fault on a qubit that
 * waits while the region is prepared, and every attempt actually made of the region, the failed ones included, draws each of them
 * with the memory error rates (q_x, q_y, q_z).  wait_count holds W per region of every type, in type_regions' order; wait_eff holds
 * the rows region by region, four uint64 each: X local, X tail, Z local, Z tail.  Besides the rules above, GF2_E_ARG naming the rule:
 * a wait count outside [0, 512], a wait count above 0 on a region that is not retried, more than GF2_RETRY_MAX_SIZES distinct
 * non-zero wait counts, bad q rates.
 *
 * Everything of the definition above stands.  In addition, for region g with W_g > 0 and every attempt a = 0, 1, ... made of it:
 *   kw = segment_draw(ks, 2^33 + g),  kwa = mix64(kw + G (a + 1)),  d = segment_draw(kwa, 0),
 * K from the inverse binomial CDF table of (T_any(q), W_g), the picks, Floyd's rule and the kinds error_draw's with q's thresholds.
 * The picked rows' words are XORed into the block's local and tail words for every attempt made: the data is never reset.  Neither
 * the region's own draw nor its key changes, so the attempts of every preparation are those of the walk above.
 * Layout of a sample, nsteps + F + 2 words: [steps] [F flag words] [attempts] [wait faults: those drawn over all attempts of the
 * sample, up to where an exhausted sample stopped]. */
#define GF2_RETRY_WAIT_FIELDS 15                /* the GF2_RETRY_FIELDS, then the wait faults of all samples of the call */
typedef struct gf2_retry_wait gf2_retry_wait;

/* The words on the host, serial, no GPU needed; words_out (ldw >= nsteps + F + 2) and attempts_out as gf2_retry_words_host's.
 * gf2_stream_tally_host on the first nsteps + F words completes the statement. */
int gf2_retry_wait_words_host(const uint64_t* type_eff, const int64_t* type_locations, const int64_t* type_flags, int64_t ntypes,
                              const int32_t* block_type, const int32_t* block_kind, int64_t nblocks, const int64_t* type_regions,
                              const int64_t* type_nregions, const uint64_t* wait_eff, const int64_t* wait_count, uint64_t seed,
                              int64_t first_sample, int64_t count, double p_x, double p_y, double p_z, double q_x, double q_y, double q_z,
                              int64_t max_attempts, uint64_t* words_out, int64_t ldw, uint32_t* attempts_out);

/* A sequence, its regions and their wait rows on the device.  Argument rules as gf2_retry_wait_words_host's (max_attempts, the
 * rates and the range belong to the calls).  Destroyed by gf2_retry_wait_destroy. */
int gf2_retry_wait_create(gf2_ctx* ctx, const uint64_t* type_eff, const int64_t* type_locations, const int64_t* type_flags, int64_t ntypes,
                          const int32_t* block_type, const int32_t* block_kind, int64_t nblocks, const int64_t* type_regions,
                          const int64_t* type_nregions, const uint64_t* wait_eff, const int64_t* wait_count, gf2_retry_wait** retry_out);
int gf2_retry_wait_destroy(gf2_ctx* ctx, gf2_retry_wait* retry);

/* The words of samples first_sample .. first_sample + count - 1 in device memory, ldo >= nsteps + F + 2 words per sample; words past
 * those are left as they were.  out_dev: any 8-byte-aligned address. */
int gf2_retry_wait_outcomes_dev(gf2_ctx* ctx, const gf2_retry_wait* retry, uint64_t seed, int64_t first_sample, int64_t count, double p_x,
                                double p_y, double p_z, double q_x, double q_y, double q_z, int64_t max_attempts, uint64_t* out_dev,
                                int64_t ldo);

/* The tally of those samples on the device, no word stored: counts_out[GF2_RETRY_WAIT_FIELDS] on the host, gf2_mc_retry_decode's
 * fourteen and the wait faults of all samples of the call.  Counts of sample ranges add. */
int gf2_mc_retry_wait_decode(gf2_ctx* ctx, const gf2_retry_wait* retry, int64_t r1, const uint64_t* keys1, const uint8_t* flips1,
                             int64_t entries1, int64_t r2, const uint64_t* keys2, const uint8_t* flips2, int64_t entries2, uint64_t seed,
                             int64_t first_sample, int64_t count, double p_x, double p_y, double p_z, double q_x, double q_y, double q_z,
                             int64_t max_attempts, uint64_t* counts_out);

/* ---- repeat-until-success under gate-level faults ------------------------------------------------------
 * [build-defined, DESIGN.md section 5d "Repeat-until-success under gate-level faults"]  The retried walk above with the fault model
 * of "direct Monte-Carlo ... under gate-level faults": every one-operand gate of a region fails with probability p_1 and one of 3
 * kinds, every CNOT as one event with probability p_2 and one of 15.  Regions are cut at gate boundaries, so a region's locations are
 * partitioned by its SITES: site_regions holds (n_1, n_2) per region of every type, in type_regions' order, with n_1 + 2 n_2 the
 * region's locations; site_loc holds the type-local first location of every site, region by region, a region's n_1 one-operand sites
 * before its n_2 CNOT sites, each class ascending; a CNOT's second location is site_loc + 1.  Besides the rules of
 * gf2_retry_words_host, GF2_E_ARG naming the rule: a region whose n_1 + 2 n_2 is not its location count, sites that do not
 * partition their region's locations or are not ascending within a class, more than GF2_RETRY_MAX_SIZES distinct segment sizes per
 * class, p_1 or p_2 outside [0, 1].
 *
 * Sample i is a pure function of (seed, i, p_1, p_2, the sequence, its regions and sites, max_attempts).  ks, the region number g,
 * kr = segment_draw(ks, 2^32 + g) and ka = mix64(kr + G (a + 1)) are those above.  Under ka the region's two classes are drawn as the
 * direct gate sampler draws a sample's under ks: the one-operand sites (m = n_1, radix 3, T = quantise(p_1), slots
 * GF2_GATE_MC_SLOT_ONE + s), then the CNOT sites (m = n_2, radix 15, T = quantise(p_2), slots GF2_GATE_MC_SLOT_CNOT + s), segments
 * of 512 sites from the class's first site in the region, K from the inverse binomial CDF table of (T, nb), picks and Floyd's rule
 * as there, kappa = 1 + ((lo radix) >> 32); a class without sites draws nothing.  Bits 0-1 of kappa select the X / Z effect of
 * location site_loc[site], bits 2-3 (a CNOT) those of site_loc[site] + 1.  The inner slots (>= 4096) are disjoint from the location
 * version's (s < 2048): the two retried samplers of a seed are independent streams.  Attempts, exhaustion, blocks, steps, the tally
 * and the layout of a sample [steps] [F flag words] [attempts] are those above, word for word. */
typedef struct gf2_retry_gate gf2_retry_gate;

/* The words on the host, serial, no GPU needed; words_out, ldw and attempts_out as gf2_retry_words_host's.  gf2_stream_tally_host on
 * the first nsteps + F words completes the statement. */
int gf2_retry_gate_words_host(const uint64_t* type_eff, const int64_t* type_locations, const int64_t* type_flags, int64_t ntypes,
                              const int32_t* block_type, const int32_t* block_kind, int64_t nblocks, const int64_t* type_regions,
                              const int64_t* type_nregions, const int32_t* site_loc, const int64_t* site_regions, uint64_t seed,
                              int64_t first_sample, int64_t count, double p1, double p2, int64_t max_attempts, uint64_t* words_out, int64_t ldw,
                              uint32_t* attempts_out);

/* A sequence, its regions and their sites on the device.  Argument rules as gf2_retry_gate_words_host's (max_attempts, the rates
 * and the range belong to the calls).  Destroyed by gf2_retry_gate_destroy. */
int gf2_retry_gate_create(gf2_ctx* ctx, const uint64_t* type_eff, const int64_t* type_locations, const int64_t* type_flags, int64_t ntypes,
                          const int32_t* block_type, const int32_t* block_kind, int64_t nblocks, const int64_t* type_regions,
                          const int64_t* type_nregions, const int32_t* site_loc, const int64_t* site_regions, gf2_retry_gate** retry_out);
int gf2_retry_gate_destroy(gf2_ctx* ctx, gf2_retry_gate* retry);

/* The words of samples first_sample .. first_sample + count - 1 in device memory, ldo >= nsteps + F + 1 words per sample; words past
 * those are left as they were.  out_dev: any 8-byte-aligned address. */
int gf2_retry_gate_outcomes_dev(gf2_ctx* ctx, const gf2_retry_gate* retry, uint64_t seed, int64_t first_sample, int64_t count, double p1,
                                double p2, int64_t max_attempts, uint64_t* out_dev, int64_t ldo);

/* The tally of those samples on the device, no word stored: counts_out[GF2_RETRY_FIELDS] on the host, as gf2_mc_retry_decode's.
 * Counts of sample ranges add.  The inverse-CDF tables are made per call and freed with it: no state beyond the handle. */
int gf2_mc_retry_gate_decode(gf2_ctx* ctx, const gf2_retry_gate* retry, int64_t r1, const uint64_t* keys1, const uint8_t* flips1,
                             int64_t entries1, int64_t r2, const uint64_t* keys2, const uint8_t* flips2, int64_t entries2, uint64_t seed,
                             int64_t first_sample, int64_t count, double p1, double p2, int64_t max_attempts, uint64_t* counts_out);

/* ---- repeat-until-success with waiting faults under gate-level faults ------------------------------------
 * [build-defined, DESIGN.md section 5d "Repeat-until-success with waiting faults under gate-level faults"]  The gate-level retried
 * walk above, in which the data block pays for the retries as in "repeat-until-success with waiting faults".  Everything of
 * "repeat-until-success under gate-level faults" stands: ks, g, kr = segment_draw(ks, 2^32 + g), ka = mix64(kr + G (a + 1)), the two
 * classes of sites under ka with radix 3 and 15 and the slots GF2_GATE_MC_SLOT_ONE / GF2_GATE_MC_SLOT_CNOT, exhaustion, blocks, steps
 * and the tally.  In addition, for a retried region g with W_g > 0 wait rows and every attempt a = 0, 1, ... actually made of it, the
 * wait draw is that of "repeat-until-success with waiting faults", word for word:
 *   kw = segment_draw(ks, GF2_RETRY_WAIT_SLOT_BASE + g) = segment_draw(ks, 2^33 + g),  kwa = mix64(kw + G (a + 1)),
 *   d = segment_draw(kwa, 0),
 * K from the inverse binomial CDF table of (T_any(q), W_g), the picks, Floyd's rule and the kinds error_draw's with q's thresholds.
 * The picked rows' (local, tail) words are XORed into the block's words for every attempt made and are never cleared.  The memory
 * rates stay (q_x, q_y, q_z): a memory's noise may be biased where the gates' noise is uniform over kinds.  Neither the region's own
 * draw nor its key changes, so the attempts of every preparation are gf2_retry_gate_words_host's.
 * Arguments: gf2_retry_gate_*'s with wait_eff, wait_count (as gf2_retry_wait_*'s) and the q rates added.  Besides the rules of
 * gf2_retry_gate_words_host, GF2_E_ARG naming the rule: a wait count outside [0, 512], a wait count above 0 on a region that is not
 * retried, more than GF2_RETRY_GATE_WAIT_MAX_SIZES distinct non-zero wait counts (the kernel keeps their inverse-CDF tables in LDS
 * beside those of the two gate classes), bad q rates.
 * Layout of a sample, nsteps + F + 2 words: [steps] [F flag words] [attempts] [wait faults].  The tally has the fifteen counts of
 * GF2_RETRY_WAIT_FIELDS: the fourteen GF2_RETRY_FIELDS, then the wait faults, in 64 bits at every level. */
#define GF2_RETRY_GATE_WAIT_MAX_SIZES 3
typedef struct gf2_retry_gate_wait gf2_retry_gate_wait;

/* The words on the host, serial, no GPU needed; words_out (ldw >= nsteps + F + 2) and attempts_out as gf2_retry_words_host's.
 * gf2_stream_tally_host on the first nsteps + F words completes the statement. */
int gf2_retry_gate_wait_words_host(const uint64_t* type_eff, const int64_t* type_locations, const int64_t* type_flags, int64_t ntypes,
                                   const int32_t* block_type, const int32_t* block_kind, int64_t nblocks, const int64_t* type_regions,
                                   const int64_t* type_nregions, const int32_t* site_loc, const int64_t* site_regions, const uint64_t* wait_eff,
                                   const int64_t* wait_count, uint64_t seed, int64_t first_sample, int64_t count, double p1, double p2, double q_x,
                                   double q_y, double q_z, int64_t max_attempts, uint64_t* words_out, int64_t ldw, uint32_t* attempts_out);

/* A sequence, its regions, their sites and their wait rows on the device.  Argument rules as gf2_retry_gate_wait_words_host's
 * (max_attempts, the rates and the range belong to the calls).  Destroyed by gf2_retry_gate_wait_destroy. */
int gf2_retry_gate_wait_create(gf2_ctx* ctx, const uint64_t* type_eff, const int64_t* type_locations, const int64_t* type_flags, int64_t ntypes,
                               const int32_t* block_type, const int32_t* block_kind, int64_t nblocks, const int64_t* type_regions,
                               const int64_t* type_nregions, const int32_t* site_loc, const int64_t* site_regions, const uint64_t* wait_eff,
                               const int64_t* wait_count, gf2_retry_gate_wait** retry_out);
int gf2_retry_gate_wait_destroy(gf2_ctx* ctx, gf2_retry_gate_wait* retry);

/* The words of samples first_sample .. first_sample + count - 1 in device memory, ldo >= nsteps + F + 2 words per sample; words past
 * those are left as they were.  out_dev: any 8-byte-aligned address. */
int gf2_retry_gate_wait_outcomes_dev(gf2_ctx* ctx, const gf2_retry_gate_wait* retry, uint64_t seed, int64_t first_sample, int64_t count,
                                     double p1, double p2, double q_x, double q_y, double q_z, int64_t max_attempts, uint64_t* out_dev,
                                     int64_t ldo);

/* The tally of those samples on the device, no word stored: counts_out[GF2_RETRY_WAIT_FIELDS] on the host.  Counts of sample ranges
 * add.  The inverse-CDF tables are made per call and freed with it: no state beyond the handle. */
int gf2_mc_retry_gate_wait_decode(gf2_ctx* ctx, const gf2_retry_gate_wait* retry, int64_t r1, const uint64_t* keys1, const uint8_t* flips1,
                                  int64_t entries1, int64_t r2, const uint64_t* keys2, const uint8_t* flips2, int64_t entries2, uint64_t seed,
                                  int64_t first_sample, int64_t count, double p1, double p2, double q_x, double q_y, double q_z,
                                  int64_t max_attempts, uint64_t* counts_out);

/* ---- repeat-until-success of multi-block programs -----------------------------------------------------
 * [build-defined, DESIGN.md section 5d "Repeat-until-success of multi-block programs"]  "repeat-until-success" and "multi-block
 * streamed programs" above, composed; no new randomness.  Blocks are (type, kind, a, b) as gf2_mstream_words_host takes them, the
 * block types are cut into regions (first, count, retried) as gf2_retry_words_host takes them.  The type of a CNOT block is one
 * region (0, 2 n, 0): it has no flag rows, so nothing of it is retried.  Region g is counted through the whole sequence, the blocks
 * in order, and its keys, segments, draws and attempts are gf2_retry_words_host's:
 *   kr = segment_draw(sample_key(seed, i), 2^32 + g),  ka = mix64(kr + G (a + 1)),
 * a region that is not retried uses a = 0, a retried one the first a < max_attempts whose flags are zero.  A block is closed by
 * gf2_mstream_words_host's rule on the XOR of its regions' words: a CNOT block applies the frame map to (T_a, T_b), then XORs its two
 * tails; any other block gives word = mask_kind(T_a) ^ local, then T_a ^= tail.  An exhausted sample stops its walk: later step words
 * stay 0 and the flag words hold the last attempt's flags at that block's flag rows.  A flag row depends on one region only and a
 * CNOT block has none, so the accepted samples have the distribution post-selection gives.  The other data blocks wait at no cost
 * while a preparation is repeated (the standing convention).  The overlap rule of gf2_mstream_create does not apply: regions end at
 * block boundaries.  Layout of a sample, nsteps + F + 1 words: [step words] [F flag words] [attempts].
 * Argument rules, GF2_E_ARG naming the rule: those of gf2_mstream_words_host, then the region rules and the max_attempts rule of
 * gf2_retry_words_host (at most GF2_RETRY_MAX_SIZES distinct segment sizes), then a CNOT block whose type is not one region that is
 * not retried.
 * counts[GF2_MRETRY_FIELDS]: the twenty GF2_MSTREAM_FIELDS with accepted = not exhausted, then exhausted, then the attempts of all
 * samples of the call, summed in 64 bits at every level.  Counts of sample ranges add. */
#define GF2_MRETRY_FIELDS 22
typedef struct gf2_mretry gf2_mretry;

/* The words on the host, serial, no GPU needed: words_out is count x ldw (ldw >= nsteps + F + 1), the words past those left as
 * they were.  attempts_out (may be null): uint32 [count][retried regions of the sequence], the attempts of every preparation in
 * order, 0 for one never reached.  gf2_mstream_tally_host on the first nsteps + F words completes the statement under either setting
 * of `records`: an exhausted sample has a non-zero flag word and is rejected there. */
int gf2_mretry_words_host(const uint64_t* type_eff, const int64_t* type_locations, const int64_t* type_flags, int64_t ntypes,
                          const int32_t* block_type, const int32_t* block_kind, const int32_t* block_a, const int32_t* block_b, int64_t nblocks,
                          int64_t nframes, const int64_t* type_regions, const int64_t* type_nregions, uint64_t seed, int64_t first_sample,
                          int64_t count, double p_x, double p_y, double p_z, int64_t max_attempts, uint64_t* words_out, int64_t ldw,
                          uint32_t* attempts_out);

/* A sequence and its regions on the device.  Argument rules as gf2_mretry_words_host's (max_attempts belongs to the calls).
 * Destroyed by gf2_mretry_destroy. */
int gf2_mretry_create(gf2_ctx* ctx, const uint64_t* type_eff, const int64_t* type_locations, const int64_t* type_flags, int64_t ntypes,
                      const int32_t* block_type, const int32_t* block_kind, const int32_t* block_a, const int32_t* block_b, int64_t nblocks,
                      int64_t nframes, const int64_t* type_regions, const int64_t* type_nregions, gf2_mretry** mretry_out);
int gf2_mretry_destroy(gf2_ctx* ctx, gf2_mretry* mretry);

/* The words of samples first_sample .. first_sample + count - 1 in device memory, ldo >= nsteps + F + 1 words per sample; words past
 * those are left as they were.  out_dev: any 8-byte-aligned address. */
int gf2_mretry_outcomes_dev(gf2_ctx* ctx, const gf2_mretry* mretry, uint64_t seed, int64_t first_sample, int64_t count, double p_x,
                            double p_y, double p_z, int64_t max_attempts, uint64_t* out_dev, int64_t ldo);

/* The tally of those samples on the device, no word stored; `records` and the bit rules as gf2_mc_mstream_decode's.
 * counts_out[GF2_MRETRY_FIELDS] on the host.  The inverse-CDF tables are made per call and freed with it: the calls keep no state
 * beyond the handle. */
int gf2_mc_mretry_decode(gf2_ctx* ctx, const gf2_mretry* mretry, int64_t records, int64_t r1, const uint64_t* keys1, const uint8_t* flips1,
                         int64_t entries1, int64_t r2, const uint64_t* keys2, const uint8_t* flips2, int64_t entries2, uint64_t seed,
                         int64_t first_sample, int64_t count, double p_x, double p_y, double p_z, int64_t max_attempts, uint64_t* counts_out);

/* ---- repeat-until-success of multi-block programs under gate-level faults ------------------------------
 * [build-defined, DESIGN.md section 5d "Repeat-until-success of multi-block programs under gate-level faults"]  "repeat-until-success
 * of multi-block programs" and "repeat-until-success under gate-level faults" above, composed; no new randomness.  The blocks, frames,
 * records, frame map, closing of a block, exhaustion, layout of a sample and the counts are those of the former; the keys and the
 * draw those of the latter: ks, the region number g counted through the whole sequence with the CNOT blocks' regions included,
 * kr = segment_draw(ks, GF2_RETRY_SLOT_BASE + g), ka = mix64(kr + G (a + 1)), and under ka the region's one-operand sites (radix 3,
 * T = quantise(p_1), slots GF2_GATE_MC_SLOT_ONE + s) and then its CNOT sites (radix 15, T = quantise(p_2), slots GF2_GATE_MC_SLOT_CNOT
 * + s) in segments of 512 sites, Floyd's rule, kappa = 1 + ((lo radix) >> 32).  site_loc and site_regions as
 * gf2_retry_gate_words_host takes them, over the regions of all types.
 * A CNOT block is one region that is never retried, with (n_1, n_2) = (0, n): site i is location 2 i, the control of the physical
 * CNOT D_a[i] -> D_b[i] on frame a, and location 2 i + 1 its target on frame b.  Bits 0-1 of kappa pick the control's X / Z rows,
 * bits 2-3 the target's; the rows hold (tail for a, tail for b, 0), so the XOR over the picked rows is the one event's correlated
 * effect on both frames.
 * Sites fail independently, no site straddles two regions and a CNOT block has no flag row, so the accepted samples have the
 * distribution post-selection gives; max_attempts = 1 is gate-level post-selection of a multi-block program.  A program on one
 * logical qubit gives gf2_retry_gate_outcomes_dev's words and gf2_mc_retry_gate_decode's counts bit for bit; the inner slots are
 * disjoint from the location route's, so a seed's samples are other samples than gf2_mretry_*'s.
 * Argument rules, GF2_E_ARG naming the rule: those of gf2_mretry_words_host, then the site rules of gf2_retry_gate_words_host, then a
 * CNOT block whose type has a one-operand site; p_1 or p_2 outside [0, 1].
 * counts[GF2_MRETRY_FIELDS] as gf2_mc_mretry_decode's.  Counts of sample ranges add. */
typedef struct gf2_mretry_gate gf2_mretry_gate;

/* Replaces gf2_mretry_words_host under gate-level faults.  The words on the host, serial, no GPU needed; words_out, ldw and
 * attempts_out as gf2_mretry_words_host's.  gf2_mstream_tally_host on the first nsteps + F words completes the statement under either
 * setting of `records`. */
int gf2_mretry_gate_words_host(const uint64_t* type_eff, const int64_t* type_locations, const int64_t* type_flags, int64_t ntypes,
                               const int32_t* block_type, const int32_t* block_kind, const int32_t* block_a, const int32_t* block_b,
                               int64_t nblocks, int64_t nframes, const int64_t* type_regions, const int64_t* type_nregions,
                               const int32_t* site_loc, const int64_t* site_regions, uint64_t seed, int64_t first_sample, int64_t count, double p1,
                               double p2, int64_t max_attempts, uint64_t* words_out, int64_t ldw, uint32_t* attempts_out);

/* Replaces gf2_mretry_create / gf2_mretry_destroy: a sequence, its regions and their sites on the device.  Argument rules as
 * gf2_mretry_gate_words_host's (max_attempts, the rates and the range belong to the calls). */
int gf2_mretry_gate_create(gf2_ctx* ctx, const uint64_t* type_eff, const int64_t* type_locations, const int64_t* type_flags, int64_t ntypes,
                           const int32_t* block_type, const int32_t* block_kind, const int32_t* block_a, const int32_t* block_b, int64_t nblocks,
                           int64_t nframes, const int64_t* type_regions, const int64_t* type_nregions, const int32_t* site_loc,
                           const int64_t* site_regions, gf2_mretry_gate** mretry_out);
int gf2_mretry_gate_destroy(gf2_ctx* ctx, gf2_mretry_gate* mretry);

/* Replaces gf2_mretry_outcomes_dev (and, on one logical qubit, equals gf2_retry_gate_outcomes_dev): the words of samples first_sample
 * .. first_sample + count - 1 in device memory, ldo >= nsteps + F + 1 words per sample; words past those are left as they were.
 * out_dev: any 8-byte-aligned address. */
int gf2_mretry_gate_outcomes_dev(gf2_ctx* ctx, const gf2_mretry_gate* mretry, uint64_t seed, int64_t first_sample, int64_t count, double p1,
                                 double p2, int64_t max_attempts, uint64_t* out_dev, int64_t ldo);

/* Replaces gf2_mc_mretry_decode: the tally of those samples on the device, no word stored; `records` and the bit rules as
 * gf2_mc_mstream_decode's.  counts_out[GF2_MRETRY_FIELDS] on the host.  The inverse-CDF tables are made per call and freed with it: the
 * calls keep no state beyond the handle. */
int gf2_mc_mretry_gate_decode(gf2_ctx* ctx, const gf2_mretry_gate* mretry, int64_t records, int64_t r1, const uint64_t* keys1,
                              const uint8_t* flips1, int64_t entries1, int64_t r2, const uint64_t* keys2, const uint8_t* flips2, int64_t entries2,
                              uint64_t seed, int64_t first_sample, int64_t count, double p1, double p2, int64_t max_attempts,
                              uint64_t* counts_out);

/* ---- multi-GPU: the histogram all-reduce -------------------------------------------------------------
 * [build-defined, SURVEY.md 8e]  The Monte-Carlo run shards by sample range (sample i = f(seed, i)); ranks never exchange
 * anything on the data path.  The one collective is the sum of the histograms -- keys as css_code.py:729, X errors against
 * parity_check_c2 and Z errors against parity_check_c1 (css_code.py:457-470) -- over RCCL (xGMI inside a node).  librccl is
 * loaded on first use; without it these calls fail with GF2_E_RCCL and nothing else is affected. */
typedef struct gf2_comm gf2_comm;
#define GF2_COMM_ID_BYTES 128
/* One process per GPU: one rank makes an id, every rank receives it out of band (the launcher's store) and joins with the
 * context whose device and stream the collective runs on.  Collective: returns when all `nranks` ranks have called it. */
int gf2_comm_unique_id(void* id_out, size_t bytes);
int gf2_comm_create(gf2_ctx* ctx, const void* id, int nranks, int rank, gf2_comm** comm_out);
/* One process, `count` contexts on `count` different devices (ncclCommInitAll). */
int gf2_comm_create_all(gf2_ctx* const* ctxs, int count, gf2_comm** comm_out);
int gf2_comm_size(const gf2_comm* comm, int* nranks_out, int* nlocal_out);
int gf2_comm_destroy(gf2_comm* comm);
/* In-place sum over all ranks of `nbins` uint64 bins in device memory; hist_dev[i] lives on the device of the i-th context the
 * communicator was created with (one entry for gf2_comm_create).  Enqueued on each context's stream behind whatever produced
 * the bins; synchronous at return. */
int gf2_hist_allreduce(gf2_comm* comm, uint64_t* const* hist_dev, int64_t nbins);
int gf2_rccl_version(int* version_out);

#ifdef __cplusplus
}
#endif
#endif /* GF2HIP_H */
