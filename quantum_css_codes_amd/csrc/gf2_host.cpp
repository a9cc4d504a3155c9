// Host-only part of libgf2hip.so: the thread-local error message and the packing of NumPy-style arrays (uint8 / int64, one entry
// per bit) into packed uint64 rows and back (gf2_pack_rows_*, gf2_unpack_rows_* of include/gf2hip.h: what css_code.py:39-44 and
// every np.mod(..., 2) of the reference do on dense arrays).  Plain C++, no HIP: `make tsan` / `make asan` build this translation
// unit alone for the CPU box (build/libgf2host_{tsan,asan}.so) and tests/test_host_sanitizers.py runs the packing round trips
// of tests/test_abi.py through them.
#include <stdarg.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

#include <algorithm>
#include <atomic>
#include <new>
#include <system_error>
#include <thread>
#include <utility>
#include <vector>

#include "gf2hip.h"
#include "gf2_gadget_rule.h"

static thread_local char g_error[512] = "";

void gf2_set_error(const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_error, sizeof(g_error), fmt, ap);
    va_end(ap);
}

extern "C" const char* gf2_last_error(void) { return g_error; }

#define GF2_FAIL(code, ...)          \
    do {                             \
        gf2_set_error(__VA_ARGS__);  \
        return (code);               \
    } while (0)

static inline int64_t gf2_words(int64_t bits) { return (bits + 63) >> 6; }

// Rows are independent: large arrays are cut into row ranges, one host thread each (a 2048 x 4096 int64 array is 64 MiB, more
// than one core streams in the time the elimination itself takes; gf2_rref on it spent 6 of its 7 ms here on one thread).
// At most GF2_HOST_THREADS threads (default 16), no more than the host's cores divided among the ranks that share it
// (LOCAL_WORLD_SIZE, as torch.distributed.run and bench.py's own launcher set it).  std::thread's constructor throws when the
// process or container is out of threads: nothing may leave an extern "C" entry point, so whatever could not be started runs
// on the calling thread, after the ranges that did start have been handed out, and everything started is joined.
static int64_t host_thread_cap() {
    static const int64_t cap = []() {                                   // read once
        const char* env = getenv("GF2_HOST_THREADS");
        const long v = env ? strtol(env, nullptr, 10) : 0;
        int64_t threads = v >= 1 && v <= 256 ? v : 16;
        const unsigned int hw = std::thread::hardware_concurrency();
        const char* lws = getenv("LOCAL_WORLD_SIZE");
        const long ranks = lws ? strtol(lws, nullptr, 10) : 1;
        int64_t share = hw ? (int64_t)hw / (ranks >= 1 && ranks <= 1024 ? ranks : 1) : 1;
        if (share < 1) share = 1;
        return threads < share ? threads : share;
    }();
    return cap;
}

#ifdef GF2_HOST_TEST_HOOKS
// sanitizer builds only (never in libgf2hip.so): makes the t-th thread creation of a call fail like an exhausted thread limit
static std::atomic<int> g_fail_after(-1);
extern "C" void gf2_host_test_fail_after(int started) { g_fail_after.store(started); }
#endif

template <typename F>
static void host_rows_parallel(int64_t rows, int64_t bytes_per_row, F body) {
    const int64_t total = rows * bytes_per_row;
    int64_t threads = host_thread_cap();
    if (threads > total >> 20) threads = total >> 20;                   // at least 1 MiB per thread
    if (threads > rows) threads = rows;
    if (threads <= 1) {
        body((int64_t)0, rows);
        return;
    }
    std::vector<std::thread> pool;
    const int64_t per = (rows + threads - 1) / threads;
    int64_t started_to = per < rows ? per : rows;                       // rows [0, per) are the caller's; [per, started_to) have a thread
    try {
        pool.reserve((size_t)threads);
        for (int64_t t = 1; t < threads; ++t) {
            const int64_t lo = t * per, hi = lo + per < rows ? lo + per : rows;
            if (lo >= hi) break;
#ifdef GF2_HOST_TEST_HOOKS
            if (g_fail_after >= 0 && t > g_fail_after) throw std::system_error(std::make_error_code(std::errc::resource_unavailable_try_again));
#endif
            pool.emplace_back([=]() { body(lo, hi); });
            started_to = hi;
        }
    } catch (const std::system_error&) {                                // out of threads: the rest is done here
    } catch (const std::bad_alloc&) {
    }
    body((int64_t)0, per < rows ? per : rows);
    if (started_to < rows) body(started_to, rows);
    for (auto& th : pool) th.join();
}

// `other_out` (may be null): set to 1 when some entry is not 0 or 1 -- css_code.py:39-44's "must be binary" test, made on the way
// through the array instead of in three further passes over it.
template <typename T>
static int pack_rows_host(const T* src, int64_t m, int64_t n, int64_t src_stride, uint64_t* dst, int64_t ld, int* other_out = nullptr) {
    if ((!src || !dst) && m > 0 && n > 0) GF2_FAIL(GF2_E_ARG, "pack: null buffer");
    if (m < 0 || n < 0 || ld < gf2_words(n) || src_stride < n) GF2_FAIL(GF2_E_ARG, "pack: bad shape");
    std::atomic<int> other(0);
    std::atomic<int>* const other_p = &other;
    host_rows_parallel(m, n * (int64_t)sizeof(T), [=](int64_t lo, int64_t hi) {
        T seen = 0;
        for (int64_t i = lo; i < hi; ++i) {
            const T* row = src + i * src_stride;
            uint64_t* out = dst + i * ld;
            for (int64_t w = 0; w < ld; ++w) {
                uint64_t acc = 0;
                const int64_t base = w * 64;
                const int64_t lim = n - base < 64 ? n - base : 64;
                for (int64_t b = 0; b < lim; ++b) {
                    acc |= (uint64_t)(row[base + b] & 1) << b;
                    seen |= row[base + b];
                }
                out[w] = acc;
            }
        }
        if (seen & ~(T)1) other_p->store(1, std::memory_order_relaxed);
    });
    if (other_out) *other_out = other.load();
    return GF2_OK;
}

template <typename T>
static int unpack_rows_host(const uint64_t* src, int64_t m, int64_t n, int64_t ld, T* dst, int64_t dst_stride) {
    if ((!src || !dst) && m > 0 && n > 0) GF2_FAIL(GF2_E_ARG, "unpack: null buffer");
    if (m < 0 || n < 0 || ld < gf2_words(n) || dst_stride < n) GF2_FAIL(GF2_E_ARG, "unpack: bad shape");
    host_rows_parallel(m, n * (int64_t)sizeof(T), [=](int64_t lo, int64_t hi) {
        for (int64_t i = lo; i < hi; ++i) {
            const uint64_t* row = src + i * ld;
            T* out = dst + i * dst_stride;
            const int64_t full = n >> 6;
            for (int64_t w = 0; w < full; ++w) {                  /* whole words: a fixed-length loop the compiler vectorises */
                const uint64_t v = row[w];
                T* o = out + w * 64;
                for (int b = 0; b < 64; ++b) o[b] = (T)((v >> b) & 1);
            }
            for (int64_t j = full * 64; j < n; ++j) out[j] = (T)((row[j >> 6] >> (j & 63)) & 1);
        }
    });
    return GF2_OK;
}

extern "C" {

int gf2_pack_rows_u8(const uint8_t* src, int64_t m, int64_t n, int64_t src_stride, uint64_t* dst, int64_t ld) {
    return pack_rows_host<uint8_t>(src, m, n, src_stride, dst, ld);
}

int gf2_pack_rows_i64(const int64_t* src, int64_t m, int64_t n, int64_t src_stride, uint64_t* dst, int64_t ld) {
    return pack_rows_host<int64_t>(src, m, n, src_stride, dst, ld);
}

int gf2_pack_rows_binary_u8(const uint8_t* src, int64_t m, int64_t n, int64_t src_stride, uint64_t* dst, int64_t ld, int* other_out) {
    if (!other_out) GF2_FAIL(GF2_E_ARG, "pack: null output");
    return pack_rows_host<uint8_t>(src, m, n, src_stride, dst, ld, other_out);
}

int gf2_pack_rows_binary_i64(const int64_t* src, int64_t m, int64_t n, int64_t src_stride, uint64_t* dst, int64_t ld, int* other_out) {
    if (!other_out) GF2_FAIL(GF2_E_ARG, "pack: null output");
    return pack_rows_host<int64_t>(src, m, n, src_stride, dst, ld, other_out);
}

int gf2_unpack_rows_u8(const uint64_t* src, int64_t m, int64_t n, int64_t ld, uint8_t* dst, int64_t dst_stride) {
    return unpack_rows_host<uint8_t>(src, m, n, ld, dst, dst_stride);
}

int gf2_unpack_rows_i64(const uint64_t* src, int64_t m, int64_t n, int64_t ld, int64_t* dst, int64_t dst_stride) {
    return unpack_rows_host<int64_t>(src, m, n, ld, dst, dst_stride);
}

}  // extern "C"

// Effect table of a circuit's fault locations (DESIGN.md "Circuit faults"): a serial chain of ngates column operations on two
// nrows x n bit matrices kept by COLUMN (cx[q], cz[q]: rw words each), walked backwards from the outcome rows.  Pauli-frame
// propagation is linear over GF(2), so the column of qubit q at the moment just after gate g says which outcomes an X (cx) or
// a Z (cz) fault on q at that moment flips.
// row_time (null: every row on the final frame) and RESET are gf2_circuit_effects_timed's (DESIGN.md "Error-correction cycle"): a row
// of time T joins the columns when the walk passes from gate T to gate T - 1, and a RESET on a emits its location (the preparation
// fault) and then clears a's columns -- nothing before the reset reaches a later outcome through a.
static int circuit_effects_walk(const char* who, bool timed, const int32_t* gates, int64_t ngates, int64_t n, const uint64_t* rows_x,
                                const uint64_t* rows_z, int64_t nrows, int64_t ld, uint64_t* eff_out, int64_t ldr, int64_t capacity,
                                int64_t* locations_out, int64_t* nloc_out, const int64_t* row_time) {
    if (!nloc_out || (ngates > 0 && !gates)) GF2_FAIL(GF2_E_ARG, "%s: null argument", who);
    if (ngates < 0 || n < 1 || n > GF2_CIRCUIT_MAX_N || nrows < 0 || nrows > GF2_CIRCUIT_MAX_ROWS || capacity < 0)
        GF2_FAIL(GF2_E_ARG, "%s: needs 1 <= n <= %d, nrows <= %d and non-negative counts", who, GF2_CIRCUIT_MAX_N, GF2_CIRCUIT_MAX_ROWS);
    int64_t total = 0;
    for (int64_t g = 0; g < ngates; ++g) {
        const int32_t kind = gates[3 * g], a = gates[3 * g + 1], b = gates[3 * g + 2];
        if (kind != GF2_GATE_H && kind != GF2_GATE_CNOT && kind != GF2_GATE_IDLE && !(timed && kind == GF2_GATE_RESET))
            GF2_FAIL(GF2_E_ARG, "%s: gate %lld has unknown kind %d", who, (long long)g, (int)kind);
        if (a < 0 || a >= n || (kind == GF2_GATE_CNOT && (b < 0 || b >= n)))
            GF2_FAIL(GF2_E_ARG, "%s: gate %lld acts on a qubit outside [0, %lld)", who, (long long)g, (long long)n);
        if (kind == GF2_GATE_CNOT && a == b) GF2_FAIL(GF2_E_ARG, "%s: gate %lld is a CNOT of qubit %d with itself", who, (long long)g, (int)a);
        total += kind == GF2_GATE_CNOT ? 2 : 1;
    }
    if (timed && nrows > 0 && !row_time) GF2_FAIL(GF2_E_ARG, "%s: null row_time", who);
    for (int64_t r = 0; timed && r < nrows; ++r)
        if (row_time[r] < 0 || row_time[r] > ngates)
            GF2_FAIL(GF2_E_ARG, "%s: row %lld has time %lld outside [0, ngates = %lld]", who, (long long)r, (long long)row_time[r], (long long)ngates);
    *nloc_out = total;
    if (capacity < total) return GF2_OK;                                // (capacity 0 just counts)
    const int64_t rw = gf2_words(nrows);
    if (total > 0 && (!eff_out || ldr < rw || ldr < 1)) GF2_FAIL(GF2_E_ARG, "%s: eff_out needs ldr >= ceil(nrows / 64) words", who);
    if (nrows > 0 && (!rows_x || !rows_z || ld < gf2_words(n))) GF2_FAIL(GF2_E_ARG, "%s: rows need ld >= ceil(n / 64) words", who);
    std::vector<uint64_t> cx, cz;
    std::vector<int64_t> order;                                         // timed: the rows by falling time
    try {
        cx.assign((size_t)(n * rw), 0);
        cz.assign((size_t)(n * rw), 0);
        if (timed) {
            order.resize((size_t)nrows);
            for (int64_t r = 0; r < nrows; ++r) order[(size_t)r] = r;
            std::stable_sort(order.begin(), order.end(), [&](int64_t x, int64_t y) { return row_time[x] > row_time[y]; });
        }
    } catch (const std::bad_alloc&) {
        GF2_FAIL(GF2_E_NOMEM, "%s: out of host memory", who);
    }
    auto join = [&](int64_t r) {
        for (int64_t q = 0; q < n; ++q) {
            cx[q * rw + (r >> 6)] |= ((rows_x[r * ld + (q >> 6)] >> (q & 63)) & 1ull) << (r & 63);
            cz[q * rw + (r >> 6)] |= ((rows_z[r * ld + (q >> 6)] >> (q & 63)) & 1ull) << (r & 63);
        }
    };
    for (int64_t r = 0; !timed && r < nrows; ++r) join(r);
    int64_t l = total;
    auto emit = [&](int64_t g, int64_t q) {
        l -= 1;
        for (int64_t w = 0; w < ldr; ++w) {
            eff_out[(2 * l) * ldr + w] = w < rw ? cx[q * rw + w] : 0ull;
            eff_out[(2 * l + 1) * ldr + w] = w < rw ? cz[q * rw + w] : 0ull;
        }
        if (locations_out) locations_out[2 * l] = g, locations_out[2 * l + 1] = q;
    };
    size_t next = 0;
    for (int64_t g = ngates - 1; g >= 0; --g) {
        for (; timed && next < order.size() && row_time[order[next]] > g; ++next) join(order[next]);
        const int32_t kind = gates[3 * g], a = gates[3 * g + 1], b = gates[3 * g + 2];
        if (kind == GF2_GATE_CNOT) emit(g, b);
        emit(g, a);
        if (kind == GF2_GATE_H)
            for (int64_t w = 0; w < rw; ++w) std::swap(cx[a * rw + w], cz[a * rw + w]);
        else if (kind == GF2_GATE_CNOT)
            for (int64_t w = 0; w < rw; ++w) cx[a * rw + w] ^= cx[b * rw + w], cz[b * rw + w] ^= cz[a * rw + w];
        else if (kind == GF2_GATE_RESET)
            for (int64_t w = 0; w < rw; ++w) cx[a * rw + w] = 0, cz[a * rw + w] = 0;
    }
    return GF2_OK;
}

extern "C" {

int gf2_circuit_effects(const int32_t* gates, int64_t ngates, int64_t n, const uint64_t* rows_x, const uint64_t* rows_z,
                        int64_t nrows, int64_t ld, uint64_t* eff_out, int64_t ldr, int64_t capacity, int64_t* locations_out,
                        int64_t* nloc_out) {
    return circuit_effects_walk("gf2_circuit_effects", false, gates, ngates, n, rows_x, rows_z, nrows, ld, eff_out, ldr, capacity,
                                locations_out, nloc_out, nullptr);
}

int gf2_circuit_effects_timed(const int32_t* gates, int64_t ngates, int64_t n, const uint64_t* rows_x, const uint64_t* rows_z,
                              int64_t nrows, int64_t ld, uint64_t* eff_out, int64_t ldr, int64_t capacity, int64_t* locations_out,
                              int64_t* nloc_out, const int64_t* row_time) {
    return circuit_effects_walk("gf2_circuit_effects_timed", true, gates, ngates, n, rows_x, rows_z, nrows, ld, eff_out, ldr, capacity,
                                locations_out, nloc_out, row_time);
}

// A stratum's errors (DESIGN.md "Strata"), the host statement of what decode_strata_kernel and circuit_kernel's stratum mode draw:
// the generator of gf2_sampler.h written out once more in plain C++ (that header is device code).
static inline uint64_t host_mix64(uint64_t z) {
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

static inline uint64_t host_quantise(double x) {                          // threshold in [0, 2^32]
    const double t = __builtin_floor(x * 4294967296.0 + 0.5);
    if (!(t > 0.0)) return 0;
    if (t >= 4294967296.0) return 4294967296ull;
    return (uint64_t)t;
}

int gf2_stratum_errors(int64_t nb, int64_t w, uint64_t seed, int64_t first_sample, int64_t count, double k_x, double k_y, double k_z,
                       uint64_t* ex_out, uint64_t* ez_out, int64_t lde) {
    if (nb < 1 || nb > GF2_STRATUM_MAX_POSITIONS)
        GF2_FAIL(GF2_E_ARG, "gf2_stratum_errors: needs 1 <= nb <= %d (2^20) positions, got %lld", GF2_STRATUM_MAX_POSITIONS, (long long)nb);
    if (w < 0 || w > nb) GF2_FAIL(GF2_E_ARG, "gf2_stratum_errors: weight %lld outside [0, nb = %lld]", (long long)w, (long long)nb);
    if (count < 0 || first_sample < 0) GF2_FAIL(GF2_E_ARG, "gf2_stratum_errors: negative range");
    if (lde < gf2_words(nb)) GF2_FAIL(GF2_E_ARG, "gf2_stratum_errors: lde must be at least ceil(nb / 64) words");
    const double s = k_x + k_y + k_z;
    if (!(k_x >= 0.0) || !(k_y >= 0.0) || !(k_z >= 0.0) || !(s > 0.0) || !(s < __builtin_inf()))
        GF2_FAIL(GF2_E_ARG, "gf2_stratum_errors: the kind weights must be non-negative and finite with a positive sum");
    if (count > 0 && (!ex_out || !ez_out)) GF2_FAIL(GF2_E_ARG, "gf2_stratum_errors: null buffer");
    const uint64_t t_1 = host_quantise(k_x / s), t_2 = host_quantise((k_x + k_y) / s);
    const uint64_t golden = 0x9E3779B97F4A7C15ull, stream = 0xD1B54A32D192ED03ull;
    for (int64_t i = 0; i < count; ++i) {
        uint64_t* const ex = ex_out + i * lde;
        uint64_t* const ez = ez_out + i * lde;
        for (int64_t q = 0; q < lde; ++q) ex[q] = 0, ez[q] = 0;
        const uint64_t ks = host_mix64(seed + golden * ((uint64_t)(first_sample + i) + 1));
        const uint64_t d = host_mix64(ks + stream * ((uint64_t)w + 1));          // the segment slot carries the weight
        for (int64_t k = 0; k < w; ++k) {
            const uint64_t v = host_mix64(d + golden * (uint64_t)(k + 1));
            const uint64_t j = (uint64_t)(nb - w + k);
            const uint64_t t = ((v >> 32) * (j + 1)) >> 32;                       // Floyd: a candidate in [0, j]
            const bool taken = ((ex[t >> 6] | ez[t >> 6]) >> (t & 63)) & 1ull;    // (every kind sets e_x or e_z)
            const uint64_t pos = taken ? j : t;
            const uint64_t c = v & 0xFFFFFFFFull;
            if (c < t_2) ex[pos >> 6] |= 1ull << (pos & 63);
            if (c >= t_1) ez[pos >> 6] |= 1ull << (pos & 63);
        }
    }
    return GF2_OK;
}

// The outcome words of a gadget's stratified samples (DESIGN.md "Sampled strata of the cycle"), the host statement of what
// gadget_strata_kernel draws: the same draw as above over the L locations of an effect table, every pick's X / Z effect XOR-ed into
// the sample's ldr words.  gf2_ec_tally_host / gf2_ft_tally_host judge the words; no tally rule is repeated here.
int gf2_stratum_outcomes_host(const uint64_t* eff, int64_t locations, int64_t ldr, int64_t w, uint64_t seed, int64_t first_sample,
                              int64_t count, double k_x, double k_y, double k_z, uint64_t* words_out, int64_t ldw) {
    const char* who = "gf2_stratum_outcomes_host";
    if (!eff) GF2_FAIL(GF2_E_ARG, "%s: null argument", who);
    if (locations < 1 || locations > GF2_CIRCUIT_MAX_LOCATIONS)
        GF2_FAIL(GF2_E_ARG, "%s: needs 1 <= locations <= %d (2^20), got %lld", who, GF2_CIRCUIT_MAX_LOCATIONS, (long long)locations);
    if (ldr < 1 || ldr > GF2_FT_MAX_LDR) GF2_FAIL(GF2_E_ARG, "%s: needs 1 <= ldr <= %d words per effect, got %lld", who, GF2_FT_MAX_LDR, (long long)ldr);
    if (w < 0 || w > GF2_CIRCUIT_STRATUM_MAX_WEIGHT || w > locations)
        GF2_FAIL(GF2_E_ARG, "%s: weight %lld outside [0, min(L = %lld, %d)]", who, (long long)w, (long long)locations, GF2_CIRCUIT_STRATUM_MAX_WEIGHT);
    if (count < 0 || first_sample < 0) GF2_FAIL(GF2_E_ARG, "%s: negative range", who);
    if (ldw < ldr) GF2_FAIL(GF2_E_ARG, "%s: ldw must be at least the table's %lld words", who, (long long)ldr);
    const double s = k_x + k_y + k_z;
    if (!(k_x >= 0.0) || !(k_y >= 0.0) || !(k_z >= 0.0) || !(s > 0.0) || !(s < __builtin_inf()))
        GF2_FAIL(GF2_E_ARG, "%s: the kind weights must be non-negative and finite with a positive sum", who);
    if (count > 0 && !words_out) GF2_FAIL(GF2_E_ARG, "%s: null buffer", who);
    const uint64_t t_1 = host_quantise(k_x / s), t_2 = host_quantise((k_x + k_y) / s);
    const uint64_t golden = 0x9E3779B97F4A7C15ull, stream = 0xD1B54A32D192ED03ull;
    for (int64_t i = 0; i < count; ++i) {
        uint64_t* const out = words_out + i * ldw;
        for (int64_t q = 0; q < ldr; ++q) out[q] = 0;
        const uint64_t ks = host_mix64(seed + golden * ((uint64_t)(first_sample + i) + 1));
        const uint64_t d = host_mix64(ks + stream * ((uint64_t)w + 1));          // the segment slot carries the weight
        uint64_t picks[GF2_CIRCUIT_STRATUM_MAX_WEIGHT];
        for (int64_t k = 0; k < w; ++k) {
            const uint64_t v = host_mix64(d + golden * (uint64_t)(k + 1));
            const uint64_t j = (uint64_t)(locations - w + k);
            const uint64_t t = ((v >> 32) * (j + 1)) >> 32;                       // Floyd: a candidate in [0, j]
            bool taken = false;
            for (int64_t q = 0; q < k; ++q) taken |= picks[q] == t;
            picks[k] = taken ? j : t;
            const uint64_t c = v & 0xFFFFFFFFull;
            const uint64_t* e = eff + (size_t)(2 * picks[k]) * ldr;
            if (c < t_2)
                for (int64_t q = 0; q < ldr; ++q) out[q] ^= e[q];
            if (c >= t_1)
                for (int64_t q = 0; q < ldr; ++q) out[q] ^= e[ldr + q];
        }
    }
    return GF2_OK;
}

}  // extern "C"

// ---- exact strata (DESIGN.md "Exact strata") ---------------------------------------------------------------------------------
// C(s, k) for k <= 8, saturated at 2^63: c_i = C(s - k + i, i) grows with i, so a partial product at or above 2^63 settles it.
static uint64_t binom_sat(int64_t s, int k) {
    if (s < k) return 0;
    unsigned __int128 c = 1;
    for (int i = 0; i < k; ++i) {
        c = c * (unsigned __int128)(s - k + 1 + i) / (unsigned)(i + 1);
        if (c >> 63) return 1ull << 63;
    }
    return (uint64_t)c;
}

// The subset of rank `rank` in the combinatorial number system: from the top pick down, the largest s below the pick above with
// C(s, k) <= what is left of the rank.
static void subset_unrank(int64_t nb, int w, uint64_t rank, int32_t* pos) {
    int64_t hi = nb;
    for (int k = w; k >= 1; --k) {
        int64_t lo = k - 1;                                                 // C(k - 1, k) = 0 <= rank
        while (hi - lo > 1) {
            const int64_t mid = lo + (hi - lo) / 2;
            if (binom_sat(mid, k) <= rank) lo = mid; else hi = mid;
        }
        pos[k - 1] = (int32_t)lo;
        rank -= binom_sat(lo, k);
        hi = lo;
    }
}

int gf2_enum_check_range(const char* who, int64_t nb, int64_t w, int64_t first_rank, int64_t count) {
    if (nb < 1 || nb > GF2_CIRCUIT_MAX_LOCATIONS) GF2_FAIL(GF2_E_ARG, "%s: needs 1 <= L <= %d (2^20) locations, got %lld", who, GF2_CIRCUIT_MAX_LOCATIONS, (long long)nb);
    if (w < 0 || w > GF2_ENUMERATE_MAX_WEIGHT || w > nb)
        GF2_FAIL(GF2_E_ARG, "%s: weight %lld outside [0, min(L = %lld, %d)]", who, (long long)w, (long long)nb, GF2_ENUMERATE_MAX_WEIGHT);
    const uint64_t total = binom_sat(nb, (int)w);
    if (total >> 63) GF2_FAIL(GF2_E_ARG, "%s: C(%lld, %lld) subsets do not fit 63 bits", who, (long long)nb, (long long)w);
    if (first_rank < 0 || count < 0 || (uint64_t)first_rank > total || (uint64_t)count > total - (uint64_t)first_rank)
        GF2_FAIL(GF2_E_ARG, "%s: ranks [%lld, %lld + %lld) leave the range [0, C(%lld, %lld) = %llu)", who, (long long)first_rank,
                 (long long)first_rank, (long long)count, (long long)nb, (long long)w, (unsigned long long)total);
    int64_t pow3 = 1;
    for (int64_t k = 0; k < w; ++k) pow3 *= 3;
    if (count > INT64_MAX / pow3) GF2_FAIL(GF2_E_ARG, "%s: %lld subsets of 3^%lld kind assignments do not fit 63 bits", who, (long long)count, (long long)w);
    return GF2_OK;
}

namespace {
struct HostTable {                                                          // sorted (high word, low word) -> flip byte
    struct Entry { uint64_t hi, lo; uint8_t flip; };
    std::vector<Entry> entries;
    static bool less(const Entry& a, const Entry& b) { return a.hi != b.hi ? a.hi < b.hi : a.lo < b.lo; }
    bool make(const uint64_t* keys, const uint8_t* flips, int64_t count, int kw) {   // false: a key occurs twice
        entries.resize((size_t)count);
        for (int64_t i = 0; i < count; ++i) entries[(size_t)i] = Entry{kw == 2 ? keys[2 * i + 1] : 0ull, keys[kw * i], flips[i]};
        std::sort(entries.begin(), entries.end(), less);
        for (size_t i = 1; i < entries.size(); ++i)
            if (!less(entries[i - 1], entries[i])) return false;
        return true;
    }
    int find(uint64_t hi, uint64_t lo) const {                               // the flip byte's low bit, or -1
        const Entry key{hi, lo, 0};
        auto it = std::lower_bound(entries.begin(), entries.end(), key, less);
        return it != entries.end() && it->hi == hi && it->lo == lo ? (it->flip & 1) : -1;
    }
};

// One sample of the error-correction cycle's tally rule (DESIGN.md "Error-correction cycle"): the class byte (0: rejected), the
// sample's eight fields added to counts.  gf2_ec_tally_host and gf2_ec_enumerate_host judge with it.
uint8_t ec_tally_sample(const uint64_t* w, int64_t ldr, int64_t rounds, const uint64_t* mask, const HostTable* tab, uint64_t* counts) {
    uint64_t flags = 0;
    for (int64_t q = rounds + 1; q < ldr; ++q) flags |= w[q];
    if (flags) return 0;
    bool flip[2], miss[2];
    uint64_t unmatched[2] = {0, 0};
    for (int c = 0; c < 2; ++c) {
        uint64_t K = 0, P = 0;
        for (int64_t t = 1; t <= rounds; ++t) {
            const uint64_t s = ((w[t] >> (32 * c)) & mask[c]) ^ K;
            const int found = tab[c].find(0, s);
            if (found < 0)
                unmatched[c] += 1;                                       // css_code.py:655-657: no match, nothing recorded
            else
                K ^= s, P ^= (uint64_t)found;
        }
        const uint64_t s = ((w[0] >> (32 * c)) & mask[c]) ^ K;
        const int found = tab[c].find(0, s);
        miss[c] = found < 0;
        flip[c] = (((w[0] >> (32 * c + 31)) & 1ull) ^ P ^ (uint64_t)(found > 0)) != 0;
    }
    counts[0] += 1;
    counts[1] += flip[0];
    counts[2] += flip[1];
    counts[3] += flip[0] | flip[1];
    counts[4] += miss[0];
    counts[5] += miss[1];
    counts[6] += unmatched[0];
    counts[7] += unmatched[1];
    return (uint8_t)(1 | flip[0] << 1 | flip[1] << 2 | miss[0] << 3 | miss[1] << 4);
}

// One sample of the logical measurement's tally rule (DESIGN.md "Logical measurement"), likewise: gf2_ft_tally_host and
// gf2_ft_enumerate_host judge with it.
uint8_t ft_tally_sample(const uint64_t* w, int64_t ldr, int64_t nsteps, uint64_t measure_mask, int trials, const uint64_t* mask,
                        const HostTable* tab, uint64_t* counts) {
    uint64_t flags = 0;
    for (int64_t q = nsteps; q < ldr; ++q) flags |= w[q];
    if (flags) return 0;
    uint64_t K[2] = {0, 0}, P[2] = {0, 0}, unmatched[2] = {0, 0};
    int wrong_trials = 0, seen_trials = 0;
    bool first_wrong = false;
    for (int64_t s = 0; s < nsteps; ++s) {
        const bool measure = (measure_mask >> s) & 1ull;
        for (int c = 0; c < (measure ? 1 : 2); ++c) {
            const uint64_t v = ((w[s] >> (32 * c)) & mask[c]) ^ K[c];
            const int found = tab[c].find(0, v);
            if (found < 0)
                unmatched[c] += 1;                                       // css_code.py:655-657: no match, nothing recorded
            else
                K[c] ^= v, P[c] ^= (uint64_t)found;
        }
        if (measure) {
            const bool bad = (((w[s] >> 31) & 1ull) ^ P[0]) != 0;
            if (seen_trials == 0) first_wrong = bad;
            wrong_trials += bad;
            seen_trials += 1;
        }
    }
    const bool wrong = 2 * wrong_trials > trials, split = wrong_trials != 0 && wrong_trials != trials;
    counts[0] += 1;
    counts[1] += wrong;
    counts[2] += (uint64_t)wrong_trials;
    counts[3] += first_wrong;
    counts[4] += split;
    counts[5] += unmatched[0];
    counts[6] += unmatched[1];
    return (uint8_t)(1 | wrong << 1 | first_wrong << 2 | split << 3 | (unmatched[0] != 0) << 4 | (unmatched[1] != 0) << 5);
}

// The walk of an enumerated rank range (DESIGN.md "Exact strata"), serial: every subset of ranks [first_rank, first_rank + count)
// (the first unranked, the others by the colexicographic successor), every kind assignment by an odometer over {1, 2, 3}^w (1 X,
// 2 Z, 3 Y: the sampler's kind bits), the outcome words XOR-ed from scratch and handed to visit(i, kind, n_x, n_y, out), i the
// subset's place in the range and kind[k] the kind of pick k in ascending location order.
template <class Visit>
void gadget_walk(const uint64_t* eff, int64_t locations, int64_t ldr, int64_t w, int64_t first_rank, int64_t count, Visit visit) {
    int32_t pos[GF2_ENUMERATE_MAX_WEIGHT] = {0};
    int kind[GF2_ENUMERATE_MAX_WEIGHT];
    subset_unrank(locations, (int)w, (uint64_t)first_rank, pos);
    for (int64_t i = 0; i < count; ++i) {
        if (i > 0) {                                                        // successor: the lowest pick that can move up does
            int64_t j = 0;
            while (j < w - 1 && pos[j] + 1 == pos[j + 1]) pos[j] = (int32_t)j, ++j;
            pos[j] += 1;
        }
        for (int64_t k = 0; k < w; ++k) kind[k] = 1;
        for (;;) {
            uint64_t out[GF2_FT_MAX_LDR] = {0};
            int64_t n_x = 0, n_y = 0;
            for (int64_t k = 0; k < w; ++k) {
                const uint64_t* e = eff + (size_t)(2 * pos[k]) * ldr;
                for (int64_t q = 0; q < ldr; ++q) out[q] ^= (kind[k] & 1 ? e[q] : 0ull) ^ (kind[k] & 2 ? e[ldr + q] : 0ull);
                n_x += kind[k] == 1;
                n_y += kind[k] == 3;
            }
            visit(i, kind, n_x, n_y, out);
            int64_t k = 0;                                                   // odometer over 1, 2, 3
            while (k < w && kind[k] == 3) kind[k++] = 1;
            if (k == w) break;
            kind[k] += 1;
        }
    }
}

// ... every configuration handed to judge(out, bin) with the bin [n_x][n_y] of `fields` counts.
template <class Judge>
void gadget_enumerate_walk(const uint64_t* eff, int64_t locations, int64_t ldr, int64_t w, int64_t first_rank, int64_t count, int fields,
                           uint64_t* counts_out, Judge judge) {
    const int64_t side = w + 1;
    gadget_walk(eff, locations, ldr, w, first_rank, count, [&](int64_t, const int*, int64_t n_x, int64_t n_y, const uint64_t* out) {
        judge(out, counts_out + (n_x * side + n_y) * fields);
    });
}

// ... or listed (include/gf2hip.h "malignant fault sets"): classify(out) is the configuration's class byte; the records of the
// listed ones, sorted by (rank, kinds code), go to records_out if they fit `capacity`, their number to *found_out either way.
template <class Classify>
int gadget_list_walk(const char* who, const uint64_t* eff, int64_t locations, int64_t ldr, int64_t w, int64_t first_rank, int64_t count,
                     uint64_t select, int64_t capacity, uint64_t* records_out, int64_t* found_out, Classify classify) {
    struct Record { uint64_t rank, tail; };
    std::vector<Record> records;
    int64_t found = 0;
    try {
        gadget_walk(eff, locations, ldr, w, first_rank, count, [&](int64_t i, const int* kind, int64_t, int64_t, const uint64_t* out) {
            const uint8_t cls = classify(out);
            if (!(cls & 1) || !(cls & select)) return;
            if (found++ >= capacity) return;                                 // (counted; the list is dropped once it cannot fit)
            uint64_t code = 0, place = 1;
            for (int64_t k = 0; k < w; ++k, place *= 3) code += (kind[k] == 1 ? 0u : kind[k] == 3 ? 1u : 2u) * place;   // 0 X, 1 Y, 2 Z
            records.push_back(Record{(uint64_t)first_rank + (uint64_t)i, code | (uint64_t)cls << 32});
        });
    } catch (const std::bad_alloc&) {
        GF2_FAIL(GF2_E_NOMEM, "%s: out of host memory", who);
    }
    *found_out = found;
    if (found > capacity) return GF2_OK;
    std::sort(records.begin(), records.end(), [](const Record& a, const Record& b) {
        return a.rank != b.rank ? a.rank < b.rank : (a.tail & 0xFFFFull) < (b.tail & 0xFFFFull);
    });
    for (size_t k = 0; k < records.size(); ++k) {
        records_out[GF2_FAULT_RECORD_WORDS * k] = records[k].rank;
        records_out[GF2_FAULT_RECORD_WORDS * k + 1] = records[k].tail;
    }
    return GF2_OK;
}

// The argument rules of a list on top of the enumeration's (include/gf2hip.h "malignant fault sets"); class_bits: the rule's.
int list_check_args(const char* who, uint64_t select, uint64_t class_bits, int64_t capacity, const uint64_t* records_out, const int64_t* found_out) {
    if (!found_out) GF2_FAIL(GF2_E_ARG, "%s: null argument", who);
    if (select == 0) GF2_FAIL(GF2_E_ARG, "%s: select names no class bit", who);
    if (select & ~class_bits)
        GF2_FAIL(GF2_E_ARG, "%s: select 0x%llx has bits outside the rule's class bits 0x%llx", who, (unsigned long long)select, (unsigned long long)class_bits);
    if (capacity < 0) GF2_FAIL(GF2_E_ARG, "%s: negative capacity", who);
    if (capacity > 0 && !records_out) GF2_FAIL(GF2_E_ARG, "%s: null buffer for %lld records", who, (long long)capacity);
    return GF2_OK;
}

// The layout rule of the cycle's host statements (gf2_gadget_rule.h: the device entry points' own) ...
int ec_check_layout(const char* who, int64_t ldr, int64_t rounds, int64_t r1, int64_t r2) {
    GadgetRule rule;
    return ec_rule_layout(who, ldr, rounds, r1, r2, &rule);
}

// ... and of the measurement's, which take tables of any number of words up to GF2_FT_MAX_LDR.
int ft_check_layout(const char* who, int64_t ldr, int64_t nsteps, uint64_t measure_mask, int64_t r1, int64_t r2) {
    GadgetRule rule;
    return ft_rule_layout(who, ldr, 0, nsteps, measure_mask, r1, r2, &rule);
}

int check_table_args(const char* who, const uint64_t* keys1, const uint8_t* flips1, int64_t entries1, const uint64_t* keys2,
                     const uint8_t* flips2, int64_t entries2) {
    if (entries1 < 0 || entries2 < 0 || (entries1 && (!keys1 || !flips1)) || (entries2 && (!keys2 || !flips2)))
        GF2_FAIL(GF2_E_ARG, "%s: bad table (a null array with entries > 0, or a negative count)", who);
    return GF2_OK;
}

// [0]: x side, parity_check_c2's table; [1]: z side, c1's (keys of one word)
int make_host_tables(const char* who, HostTable* tab, const uint64_t* keys1, const uint8_t* flips1, int64_t entries1, const uint64_t* keys2,
                     const uint8_t* flips2, int64_t entries2) {
    try {
        if (!tab[0].make(keys2, flips2, entries2, 1) || !tab[1].make(keys1, flips1, entries1, 1))
            GF2_FAIL(GF2_E_ARG, "%s: a syndrome key occurs twice in a table", who);
    } catch (const std::bad_alloc&) {
        GF2_FAIL(GF2_E_NOMEM, "%s: out of host memory", who);
    }
    return GF2_OK;
}

// No effect of the cycle's table may set a bit outside the layout (the layout already checked) ...
int ec_check_effects(const char* who, const uint64_t* eff, int64_t locations, int64_t ldr, int64_t rounds, int64_t r1, int64_t r2) {
    GadgetRule rule;
    if (int rc = gadget_rule_keys(who, r1, r2, &rule)) return rc;
    uint64_t any[GF2_CIRCUIT_MAX_LDR] = {0};
    for (int64_t i = 0; i < 2 * locations; ++i)
        for (int64_t q = 0; q < ldr; ++q) any[q] |= eff[i * ldr + q];
    return ec_rule_effects(who, any, rounds, rule);
}

// ... nor one of the measurement's.
int ft_check_effects(const char* who, const uint64_t* eff, int64_t locations, int64_t ldr, int64_t nsteps, uint64_t measure_mask, int64_t r1,
                     int64_t r2) {
    GadgetRule rule;
    if (int rc = gadget_rule_keys(who, r1, r2, &rule)) return rc;
    uint64_t any[GF2_FT_MAX_LDR] = {0};
    for (int64_t i = 0; i < 2 * locations; ++i)
        for (int64_t q = 0; q < ldr; ++q) any[q] |= eff[i * ldr + q];
    return ft_rule_effects(who, any, nsteps, measure_mask, rule);
}

// The argument rules gf2_ec_enumerate_host and gf2_ec_enumerate_list_host share (eff not null) ...
int ec_enumerate_check(const char* who, const uint64_t* eff, int64_t locations, int64_t ldr, int64_t rounds, int64_t r1, const uint64_t* keys1,
                       const uint8_t* flips1, int64_t entries1, int64_t r2, const uint64_t* keys2, const uint8_t* flips2, int64_t entries2,
                       int64_t w, int64_t first_rank, int64_t count) {
    if (ldr < 1) GF2_FAIL(GF2_E_ARG, "%s: needs ldr >= 1 words per effect", who);
    if (int rc = ec_check_layout(who, ldr, rounds, r1, r2)) return rc;
    if (int rc = check_table_args(who, keys1, flips1, entries1, keys2, flips2, entries2)) return rc;
    if (int rc = gf2_enum_check_range(who, locations, w, first_rank, count)) return rc;
    return ec_check_effects(who, eff, locations, ldr, rounds, r1, r2);
}

// ... and those of gf2_ft_enumerate_host and gf2_ft_enumerate_list_host.
int ft_enumerate_check(const char* who, const uint64_t* eff, int64_t locations, int64_t ldr, int64_t nsteps, uint64_t measure_mask, int64_t r1,
                       const uint64_t* keys1, const uint8_t* flips1, int64_t entries1, int64_t r2, const uint64_t* keys2, const uint8_t* flips2,
                       int64_t entries2, int64_t w, int64_t first_rank, int64_t count) {
    if (ldr < 1) GF2_FAIL(GF2_E_ARG, "%s: needs ldr >= 1 words per effect", who);
    if (int rc = ft_check_layout(who, ldr, nsteps, measure_mask, r1, r2)) return rc;
    if (int rc = check_table_args(who, keys1, flips1, entries1, keys2, flips2, entries2)) return rc;
    if (int rc = gf2_enum_check_range(who, locations, w, first_rank, count)) return rc;
    return ft_check_effects(who, eff, locations, ldr, nsteps, measure_mask, r1, r2);
}
}  // namespace

extern "C" {

int gf2_subset_unrank(int64_t nb, int64_t w, int64_t rank, int32_t* positions_out) {
    if (nb < 1 || nb > GF2_STRATUM_MAX_POSITIONS)
        GF2_FAIL(GF2_E_ARG, "gf2_subset_unrank: needs 1 <= nb <= %d (2^20) positions, got %lld", GF2_STRATUM_MAX_POSITIONS, (long long)nb);
    if (w < 0 || w > GF2_ENUMERATE_MAX_WEIGHT || w > nb)
        GF2_FAIL(GF2_E_ARG, "gf2_subset_unrank: weight %lld outside [0, min(nb = %lld, %d)]", (long long)w, (long long)nb, GF2_ENUMERATE_MAX_WEIGHT);
    if (rank < 0 || (uint64_t)rank >= binom_sat(nb, (int)w))
        GF2_FAIL(GF2_E_ARG, "gf2_subset_unrank: rank %lld outside [0, C(%lld, %lld))", (long long)rank, (long long)nb, (long long)w);
    if (w > 0 && !positions_out) GF2_FAIL(GF2_E_ARG, "gf2_subset_unrank: null buffer");
    subset_unrank(nb, (int)w, (uint64_t)rank, positions_out);
    return GF2_OK;
}

// The definition of gf2_circuit_enumerate, serial: every subset of the rank range (the first unranked, the others by the colexicographic
// successor), every kind assignment by an odometer over {1, 2, 3}^w, the outcome XOR-ed from scratch, the tables as sorted arrays.
int gf2_circuit_enumerate_host(const uint64_t* eff, int64_t locations, int64_t ldr, int64_t r1, const uint64_t* keys1, const uint8_t* flips1,
                               int64_t entries1, int64_t r2, const uint64_t* keys2, const uint8_t* flips2, int64_t entries2, int64_t w,
                               int64_t first_rank, int64_t count, uint64_t* counts_out) {
    const char* who = "gf2_circuit_enumerate_host";
    if (!eff || !counts_out) GF2_FAIL(GF2_E_ARG, "%s: null argument", who);
    if (ldr < 1 || ldr > GF2_CIRCUIT_MAX_LDR) GF2_FAIL(GF2_E_ARG, "%s: needs 1 <= ldr <= %d words per effect", who, GF2_CIRCUIT_MAX_LDR);
    if (r1 < 1 || r2 < 1 || r1 > 127 || r2 > 127) GF2_FAIL(GF2_E_ARG, "%s: needs 1 <= r_1, r_2 <= 127", who);
    const int kwx = r2 <= 63 ? 1 : 2, kwz = r1 <= 63 ? 1 : 2;
    if (ldr != kwx + kwz + 1)
        GF2_FAIL(GF2_E_ARG, "%s: r_1 = %lld and r_2 = %lld need effects of %d words (key_x, key_z, parity), the table has %lld", who,
                 (long long)r1, (long long)r2, kwx + kwz + 1, (long long)ldr);
    if (entries1 < 0 || entries2 < 0 || (entries1 && (!keys1 || !flips1)) || (entries2 && (!keys2 || !flips2)))
        GF2_FAIL(GF2_E_ARG, "%s: bad table (a null array with entries > 0, or a negative count)", who);
    if (int rc = gf2_enum_check_range(who, locations, w, first_rank, count)) return rc;
    uint64_t any[GF2_CIRCUIT_MAX_LDR] = {0};
    for (int64_t i = 0; i < 2 * locations; ++i)
        for (int64_t q = 0; q < ldr; ++q) any[q] |= eff[i * ldr + q];
    auto beyond = [](const uint64_t* words, int kw, int64_t r) { return (words[kw - 1] >> (r - 64 * (kw - 1))) != 0; };
    if (beyond(any, kwx, r2) || beyond(any + kwx, kwz, r1) || (any[ldr - 1] >> 2) != 0)
        GF2_FAIL(GF2_E_ARG, "%s: the effects set bits beyond the keys' r_2 / r_1 bits or the two parity bits", who);
    const int64_t side = w + 1;
    for (int64_t k = 0; k < side * side * 5; ++k) counts_out[k] = 0;
    if (count == 0) return GF2_OK;
    HostTable tab[2];                                                        // [0]: key_x in parity_check_c2's table, [1]: key_z in c1's
    try {
        if (!tab[0].make(keys2, flips2, entries2, kwx) || !tab[1].make(keys1, flips1, entries1, kwz))
            GF2_FAIL(GF2_E_ARG, "%s: a syndrome key occurs twice in a table", who);
    } catch (const std::bad_alloc&) {
        GF2_FAIL(GF2_E_NOMEM, "%s: out of host memory", who);
    }
    int32_t pos[GF2_ENUMERATE_MAX_WEIGHT] = {0};
    int kind[GF2_ENUMERATE_MAX_WEIGHT];
    subset_unrank(locations, (int)w, (uint64_t)first_rank, pos);
    for (int64_t i = 0; i < count; ++i) {
        if (i > 0) {                                                        // successor: the lowest pick that can move up does
            int64_t j = 0;
            while (j < w - 1 && pos[j] + 1 == pos[j + 1]) pos[j] = (int32_t)j, ++j;
            pos[j] += 1;
        }
        for (int64_t k = 0; k < w; ++k) kind[k] = 1;
        for (;;) {
            uint64_t out[GF2_CIRCUIT_MAX_LDR] = {0};
            int64_t n_x = 0, n_y = 0;
            for (int64_t k = 0; k < w; ++k) {
                const uint64_t* e = eff + (size_t)(2 * pos[k]) * ldr;
                for (int64_t q = 0; q < ldr; ++q) out[q] ^= (kind[k] & 1 ? e[q] : 0ull) ^ (kind[k] & 2 ? e[ldr + q] : 0ull);
                n_x += kind[k] == 1;
                n_y += kind[k] == 3;
            }
            const uint64_t key[2][2] = {{out[0], kwx == 2 ? out[1] : 0ull}, {out[kwx], kwz == 2 ? out[kwx + 1] : 0ull}};   // (low, high)
            bool flip[2], miss[2];
            for (int c = 0; c < 2; ++c) {
                const int found = tab[c].find(key[c][1], key[c][0]);
                miss[c] = found < 0;
                flip[c] = ((out[ldr - 1] >> c) & 1ull) != (uint64_t)(found > 0);
            }
            uint64_t* bin = counts_out + (n_x * side + n_y) * 5;
            bin[0] += flip[0];
            bin[1] += flip[1];
            bin[2] += flip[0] | flip[1];
            bin[3] += miss[0];
            bin[4] += miss[1];
            int64_t k = 0;                                                   // odometer over 1, 2, 3
            while (k < w && kind[k] == 3) kind[k++] = 1;
            if (k == w) break;
            kind[k] += 1;
        }
    }
    return GF2_OK;
}

// The tally rule of the error-correction cycle (DESIGN.md "Error-correction cycle"), serial: quil_classical_correct's record of known
// errors (css_code.py:649-685) round by round as (syndrome K, operator parity P) per side, then gf2_mc_circuit_decode's judgement of
// the final data frame relative to that record.
int gf2_ec_tally_host(const uint64_t* words, int64_t count, int64_t ldw, int64_t ldr, int64_t rounds, int64_t r1, const uint64_t* keys1,
                      const uint8_t* flips1, int64_t entries1, int64_t r2, const uint64_t* keys2, const uint8_t* flips2, int64_t entries2,
                      uint64_t* counts_out, uint8_t* class_out) {
    const char* who = "gf2_ec_tally_host";
    if (!counts_out) GF2_FAIL(GF2_E_ARG, "%s: null argument", who);
    if (int rc = ec_check_layout(who, ldr, rounds, r1, r2)) return rc;
    if (count < 0 || ldw < ldr || (count > 0 && !words)) GF2_FAIL(GF2_E_ARG, "%s: needs count >= 0 samples of ldw >= ldr words", who);
    if (int rc = check_table_args(who, keys1, flips1, entries1, keys2, flips2, entries2)) return rc;
    for (int k = 0; k < GF2_EC_FIELDS; ++k) counts_out[k] = 0;
    if (count == 0) return GF2_OK;
    HostTable tab[2];
    if (int rc = make_host_tables(who, tab, keys1, flips1, entries1, keys2, flips2, entries2)) return rc;
    const uint64_t mask[2] = {(1ull << r2) - 1, (1ull << r1) - 1};
    for (int64_t i = 0; i < count; ++i) {
        const uint8_t cls = ec_tally_sample(words + i * ldw, ldr, rounds, mask, tab, counts_out);
        if (class_out) class_out[i] = cls;
    }
    return GF2_OK;
}

// The tally rule of the fault-tolerant logical measurement (DESIGN.md "Logical measurement"), serial: the record of known errors
// (syndrome K, operator parity P per side) runs through the steps in program order; an EC step updates both sides, a MEASURE step
// the x side only (noisy_measure corrects data.x_errors, css_code.py:636-639) and reads its trial's bit against the updated record;
// the majority of the trials is the result (css_code.py:580-583).
int gf2_ft_tally_host(const uint64_t* words, int64_t count, int64_t ldw, int64_t ldr, int64_t nsteps, uint64_t measure_mask, int64_t r1,
                      const uint64_t* keys1, const uint8_t* flips1, int64_t entries1, int64_t r2, const uint64_t* keys2,
                      const uint8_t* flips2, int64_t entries2, uint64_t* counts_out, uint8_t* class_out) {
    const char* who = "gf2_ft_tally_host";
    if (!counts_out) GF2_FAIL(GF2_E_ARG, "%s: null argument", who);
    if (int rc = ft_check_layout(who, ldr, nsteps, measure_mask, r1, r2)) return rc;
    const int trials = __builtin_popcountll(measure_mask);
    if (count < 0 || ldw < ldr || (count > 0 && !words)) GF2_FAIL(GF2_E_ARG, "%s: needs count >= 0 samples of ldw >= ldr words", who);
    if (int rc = check_table_args(who, keys1, flips1, entries1, keys2, flips2, entries2)) return rc;
    for (int k = 0; k < GF2_FT_FIELDS; ++k) counts_out[k] = 0;
    if (count == 0) return GF2_OK;
    HostTable tab[2];
    if (int rc = make_host_tables(who, tab, keys1, flips1, entries1, keys2, flips2, entries2)) return rc;
    const uint64_t mask[2] = {(1ull << r2) - 1, (1ull << r1) - 1};
    for (int64_t i = 0; i < count; ++i) {
        const uint8_t cls = ft_tally_sample(words + i * ldw, ldr, nsteps, measure_mask, trials, mask, tab, counts_out);
        if (class_out) class_out[i] = cls;
    }
    return GF2_OK;
}

// The definition of gf2_ec_enumerate (DESIGN.md "Exact strata of the cycle"), serial: gf2_circuit_enumerate_host's walk, every
// configuration's outcome words judged by gf2_ec_tally_host's per-sample rule.
int gf2_ec_enumerate_host(const uint64_t* eff, int64_t locations, int64_t ldr, int64_t rounds, int64_t r1, const uint64_t* keys1,
                          const uint8_t* flips1, int64_t entries1, int64_t r2, const uint64_t* keys2, const uint8_t* flips2, int64_t entries2,
                          int64_t w, int64_t first_rank, int64_t count, uint64_t* counts_out) {
    const char* who = "gf2_ec_enumerate_host";
    if (!eff || !counts_out) GF2_FAIL(GF2_E_ARG, "%s: null argument", who);
    if (int rc = ec_enumerate_check(who, eff, locations, ldr, rounds, r1, keys1, flips1, entries1, r2, keys2, flips2, entries2, w, first_rank, count)) return rc;
    const uint64_t mask[2] = {(1ull << r2) - 1, (1ull << r1) - 1};
    for (int64_t k = 0; k < (w + 1) * (w + 1) * GF2_EC_FIELDS; ++k) counts_out[k] = 0;
    if (count == 0) return GF2_OK;
    HostTable tab[2];
    if (int rc = make_host_tables(who, tab, keys1, flips1, entries1, keys2, flips2, entries2)) return rc;
    gadget_enumerate_walk(eff, locations, ldr, w, first_rank, count, GF2_EC_FIELDS, counts_out,
                          [&](const uint64_t* out, uint64_t* bin) { (void)ec_tally_sample(out, ldr, rounds, mask, tab, bin); });
    return GF2_OK;
}

// The definition of gf2_ft_enumerate (DESIGN.md "Exact strata of the measurement"), likewise with gf2_ft_tally_host's rule.
int gf2_ft_enumerate_host(const uint64_t* eff, int64_t locations, int64_t ldr, int64_t nsteps, uint64_t measure_mask, int64_t r1,
                          const uint64_t* keys1, const uint8_t* flips1, int64_t entries1, int64_t r2, const uint64_t* keys2,
                          const uint8_t* flips2, int64_t entries2, int64_t w, int64_t first_rank, int64_t count, uint64_t* counts_out) {
    const char* who = "gf2_ft_enumerate_host";
    if (!eff || !counts_out) GF2_FAIL(GF2_E_ARG, "%s: null argument", who);
    if (int rc = ft_enumerate_check(who, eff, locations, ldr, nsteps, measure_mask, r1, keys1, flips1, entries1, r2, keys2, flips2, entries2, w, first_rank, count))
        return rc;
    const int trials = __builtin_popcountll(measure_mask);
    const uint64_t mask[2] = {(1ull << r2) - 1, (1ull << r1) - 1};
    for (int64_t k = 0; k < (w + 1) * (w + 1) * GF2_FT_FIELDS; ++k) counts_out[k] = 0;
    if (count == 0) return GF2_OK;
    HostTable tab[2];
    if (int rc = make_host_tables(who, tab, keys1, flips1, entries1, keys2, flips2, entries2)) return rc;
    gadget_enumerate_walk(eff, locations, ldr, w, first_rank, count, GF2_FT_FIELDS, counts_out, [&](const uint64_t* out, uint64_t* bin) {
        (void)ft_tally_sample(out, ldr, nsteps, measure_mask, trials, mask, tab, bin);
    });
    return GF2_OK;
}

// The definition of gf2_ec_enumerate_list (DESIGN.md "Malignant fault sets of the cycle"), serial: gf2_ec_enumerate_host's walk and
// rule, the class byte of every configuration kept instead of its counts.
int gf2_ec_enumerate_list_host(const uint64_t* eff, int64_t locations, int64_t ldr, int64_t rounds, int64_t r1, const uint64_t* keys1,
                               const uint8_t* flips1, int64_t entries1, int64_t r2, const uint64_t* keys2, const uint8_t* flips2,
                               int64_t entries2, int64_t w, int64_t first_rank, int64_t count, uint64_t select, int64_t capacity,
                               uint64_t* records_out, int64_t* found_out) {
    const char* who = "gf2_ec_enumerate_list_host";
    if (!eff) GF2_FAIL(GF2_E_ARG, "%s: null argument", who);
    if (int rc = list_check_args(who, select, GF2_EC_CLASS_BITS, capacity, records_out, found_out)) return rc;
    if (int rc = ec_enumerate_check(who, eff, locations, ldr, rounds, r1, keys1, flips1, entries1, r2, keys2, flips2, entries2, w, first_rank, count)) return rc;
    const uint64_t mask[2] = {(1ull << r2) - 1, (1ull << r1) - 1};
    *found_out = 0;
    if (count == 0) return GF2_OK;
    HostTable tab[2];
    if (int rc = make_host_tables(who, tab, keys1, flips1, entries1, keys2, flips2, entries2)) return rc;
    return gadget_list_walk(who, eff, locations, ldr, w, first_rank, count, select, capacity, records_out, found_out, [&](const uint64_t* out) {
        uint64_t unused[GF2_EC_FIELDS] = {0};
        return ec_tally_sample(out, ldr, rounds, mask, tab, unused);
    });
}

// The definition of gf2_ft_enumerate_list (DESIGN.md "Malignant fault sets of the measurement"), likewise.
int gf2_ft_enumerate_list_host(const uint64_t* eff, int64_t locations, int64_t ldr, int64_t nsteps, uint64_t measure_mask, int64_t r1,
                               const uint64_t* keys1, const uint8_t* flips1, int64_t entries1, int64_t r2, const uint64_t* keys2,
                               const uint8_t* flips2, int64_t entries2, int64_t w, int64_t first_rank, int64_t count, uint64_t select,
                               int64_t capacity, uint64_t* records_out, int64_t* found_out) {
    const char* who = "gf2_ft_enumerate_list_host";
    if (!eff) GF2_FAIL(GF2_E_ARG, "%s: null argument", who);
    if (int rc = list_check_args(who, select, GF2_FT_CLASS_BITS, capacity, records_out, found_out)) return rc;
    if (int rc = ft_enumerate_check(who, eff, locations, ldr, nsteps, measure_mask, r1, keys1, flips1, entries1, r2, keys2, flips2, entries2, w, first_rank, count))
        return rc;
    const int trials = __builtin_popcountll(measure_mask);
    const uint64_t mask[2] = {(1ull << r2) - 1, (1ull << r1) - 1};
    *found_out = 0;
    if (count == 0) return GF2_OK;
    HostTable tab[2];
    if (int rc = make_host_tables(who, tab, keys1, flips1, entries1, keys2, flips2, entries2)) return rc;
    return gadget_list_walk(who, eff, locations, ldr, w, first_rank, count, select, capacity, records_out, found_out, [&](const uint64_t* out) {
        uint64_t unused[GF2_FT_FIELDS] = {0};
        return ft_tally_sample(out, ldr, nsteps, measure_mask, trials, mask, tab, unused);
    });
}

}  // extern "C"

// ---- exact strata under gate-level faults (include/gf2hip.h "gate-level faults") ------------------------
// The argument rules of the site table alone (the sampled strata of gf2_gate_strata.hip and their host statement check it through
// this too) ...
int gf2_gate_check_sites(const char* who, int64_t locations, const int32_t* site_loc, int64_t n1, int64_t n2) {
    if (locations < 1 || locations > GF2_CIRCUIT_MAX_LOCATIONS)
        GF2_FAIL(GF2_E_ARG, "%s: needs 1 <= L <= %d (2^20) locations, got %lld", who, GF2_CIRCUIT_MAX_LOCATIONS, (long long)locations);
    if (!site_loc || n1 < 0 || n2 < 0 || n1 + 2 * n2 != locations)
        GF2_FAIL(GF2_E_ARG, "%s: the site table is no partition of [0, L): n_1 + 2 n_2 = %lld + 2 * %lld, L = %lld", who, (long long)n1, (long long)n2,
                 (long long)locations);
    try {
        std::vector<uint8_t> seen((size_t)locations, 0);
        for (int64_t s = 0; s < n1 + n2; ++s) {
            const int64_t l = site_loc[s], width = s < n1 ? 1 : 2;
            if (l < 0 || l + width > locations || seen[(size_t)l] || seen[(size_t)(l + width - 1)])
                GF2_FAIL(GF2_E_ARG, "%s: the site table is no partition of [0, L): site %lld at location %lld", who, (long long)s, (long long)l);
            seen[(size_t)l] = seen[(size_t)(l + width - 1)] = 1;
        }
    } catch (const std::bad_alloc&) {
        GF2_FAIL(GF2_E_NOMEM, "%s: out of host memory", who);
    }
    return GF2_OK;
}

// ... and of a rank range of sites, shared by the host statements below and the device entry points (gf2_gate_enumerate.hip).
int gf2_gate_check_range(const char* who, int64_t locations, const int32_t* site_loc, int64_t n1, int64_t n2, int64_t w, int64_t b,
                         int64_t first_rank, int64_t count) {
    if (locations < 1 || locations > GF2_CIRCUIT_MAX_LOCATIONS)                // (gf2_gate_check_sites' test, here to keep the order of the messages)
        GF2_FAIL(GF2_E_ARG, "%s: needs 1 <= L <= %d (2^20) locations, got %lld", who, GF2_CIRCUIT_MAX_LOCATIONS, (long long)locations);
    if (w < 0 || w > GF2_GATE_ENUMERATE_MAX_WEIGHT) GF2_FAIL(GF2_E_ARG, "%s: weight %lld outside [0, %d]", who, (long long)w, GF2_GATE_ENUMERATE_MAX_WEIGHT);
    if (b < 0 || b > w) GF2_FAIL(GF2_E_ARG, "%s: %lld CNOT picks outside [0, w = %lld]", who, (long long)b, (long long)w);
    if (int rc = gf2_gate_check_sites(who, locations, site_loc, n1, n2)) return rc;
    const int64_t a = w - b;
    const unsigned __int128 total = (unsigned __int128)binom_sat(n1, (int)a) * binom_sat(n2, (int)b);
    if (total >> 63) GF2_FAIL(GF2_E_ARG, "%s: C(%lld, %lld) C(%lld, %lld) subsets do not fit 63 bits", who, (long long)n1, (long long)a, (long long)n2, (long long)b);
    if (first_rank < 0 || count < 0 || (uint64_t)first_rank > (uint64_t)total || (uint64_t)count > (uint64_t)total - (uint64_t)first_rank)
        GF2_FAIL(GF2_E_ARG, "%s: ranks [%lld, %lld + %lld) leave the range [0, C(%lld, %lld) C(%lld, %lld) = %llu)", who, (long long)first_rank,
                 (long long)first_rank, (long long)count, (long long)n1, (long long)a, (long long)n2, (long long)b, (unsigned long long)total);
    int64_t kinds = 1;
    for (int64_t k = 0; k < w; ++k) kinds *= k < a ? 3 : 15;
    if (count > INT64_MAX / kinds)
        GF2_FAIL(GF2_E_ARG, "%s: %lld subsets of 3^%lld 15^%lld kind assignments do not fit 63 bits", who, (long long)count, (long long)a, (long long)b);
    return GF2_OK;
}

namespace {
// One step of the colexicographic successor of k ascending picks (gadget_walk's).
void subset_successor(int64_t k, int32_t* pos) {
    int64_t j = 0;
    while (j < k - 1 && pos[j] + 1 == pos[j + 1]) pos[j] = (int32_t)j, ++j;
    pos[j] += 1;
}

// The walk of a rank range of sites, serial: the first subset unranked part by part (rank = r_s + C(n_1, a) r_c), the others by
// the successor of the product order (the one-operand part steps; when it wraps, the CNOT part does), every kind assignment by an
// odometer over [1, 3]^a x [1, 15]^b, the outcome words XOR-ed from scratch and handed to visit(i, site, kappa, c, out): i the
// subset's place in the range, site[k] and kappa[k] the site and kind mask of pick k (the a one-operand picks first, each part in
// ascending site order), c the number of two-operand kinds.  The counting and the listing statements below share it.
template <class Visit>
void gate_walk(const uint64_t* eff, int64_t ldr, const int32_t* site_loc, int64_t n1, int64_t n2, int64_t w, int64_t b, int64_t first_rank,
               int64_t count, Visit visit) {
    const int64_t a = w - b;
    const uint64_t c1 = binom_sat(n1, (int)a);
    int32_t ps[GF2_GATE_ENUMERATE_MAX_WEIGHT] = {0}, pc[GF2_GATE_ENUMERATE_MAX_WEIGHT] = {0}, site[GF2_GATE_ENUMERATE_MAX_WEIGHT] = {0};
    int kappa[GF2_GATE_ENUMERATE_MAX_WEIGHT];
    subset_unrank(n1, (int)a, (uint64_t)first_rank % c1, ps);
    subset_unrank(n2, (int)b, (uint64_t)first_rank / c1, pc);
    for (int64_t i = 0; i < count; ++i) {
        if (i > 0) {
            if (a == 0 || ps[0] == n1 - a) {                                // the one-operand part is at its last subset: it wraps
                for (int64_t k = 0; k < a; ++k) ps[k] = (int32_t)k;
                subset_successor(b, pc);
            } else {
                subset_successor(a, ps);
            }
        }
        for (int64_t k = 0; k < w; ++k) site[k] = k < a ? ps[k] : (int32_t)n1 + pc[k - a], kappa[k] = 1;
        for (;;) {
            uint64_t out[GF2_FT_MAX_LDR] = {0};
            int64_t c = 0;
            for (int64_t k = 0; k < w; ++k) {
                for (int bit = 0; bit < 4; ++bit) {
                    if (!((kappa[k] >> bit) & 1)) continue;
                    const uint64_t* e = eff + (size_t)(2 * (site_loc[site[k]] + (bit >> 1)) + (bit & 1)) * ldr;
                    for (int64_t q = 0; q < ldr; ++q) out[q] ^= e[q];
                }
                c += (kappa[k] & 3) != 0 && (kappa[k] >> 2) != 0;
            }
            visit(i, site, kappa, c, out);
            int64_t k = 0;                                                   // odometer over 1 .. 3 or 1 .. 15
            while (k < w && kappa[k] == (k < a ? 3 : 15)) kappa[k++] = 1;
            if (k == w) break;
            kappa[k] += 1;
        }
    }
}

// ... every configuration of which is either counted (the statements below call gate_walk themselves) or listed (include/gf2hip.h
// "malignant fault sets under gate-level faults"): classify(out) is the configuration's class byte; the records of the listed ones,
// sorted by (rank, kind masks), go to records_out if they fit `capacity`, their number to *found_out either way.
template <class Classify>
int gate_list_walk(const char* who, const uint64_t* eff, int64_t ldr, const int32_t* site_loc, int64_t n1, int64_t n2, int64_t w, int64_t b,
                   int64_t first_rank, int64_t count, uint64_t select, int64_t capacity, uint64_t* records_out, int64_t* found_out,
                   Classify classify) {
    struct Record { uint64_t rank, tail; };
    std::vector<Record> records;
    int64_t found = 0;
    try {
        gate_walk(eff, ldr, site_loc, n1, n2, w, b, first_rank, count, [&](int64_t i, const int32_t*, const int* kappa, int64_t, const uint64_t* out) {
            const uint8_t cls = classify(out);
            if (!(cls & 1) || !(cls & select)) return;
            if (found++ >= capacity) return;                                 // (counted; the list is dropped once it cannot fit)
            uint64_t kinds = 0;
            for (int64_t k = 0; k < w; ++k) kinds |= (uint64_t)kappa[k] << (4 * k);
            records.push_back(Record{(uint64_t)first_rank + (uint64_t)i, kinds | (uint64_t)cls << 32});
        });
    } catch (const std::bad_alloc&) {
        GF2_FAIL(GF2_E_NOMEM, "%s: out of host memory", who);
    }
    *found_out = found;
    if (found > capacity) return GF2_OK;
    std::sort(records.begin(), records.end(), [](const Record& a, const Record& b) {
        return a.rank != b.rank ? a.rank < b.rank : (a.tail & 0xFFFFull) < (b.tail & 0xFFFFull);
    });
    for (size_t k = 0; k < records.size(); ++k) {
        records_out[GF2_FAULT_RECORD_WORDS * k] = records[k].rank;
        records_out[GF2_FAULT_RECORD_WORDS * k + 1] = records[k].tail;
    }
    return GF2_OK;
}

// The argument rules gf2_ec_gate_enumerate_host and gf2_ec_gate_enumerate_list_host share (eff not null) ...
int ec_gate_enumerate_check(const char* who, const uint64_t* eff, int64_t locations, int64_t ldr, int64_t rounds, int64_t r1, const uint64_t* keys1,
                            const uint8_t* flips1, int64_t entries1, int64_t r2, const uint64_t* keys2, const uint8_t* flips2, int64_t entries2,
                            const int32_t* site_loc, int64_t n1, int64_t n2, int64_t w, int64_t b, int64_t first_rank, int64_t count) {
    if (ldr < 1) GF2_FAIL(GF2_E_ARG, "%s: needs ldr >= 1 words per effect", who);
    if (int rc = ec_check_layout(who, ldr, rounds, r1, r2)) return rc;
    if (int rc = check_table_args(who, keys1, flips1, entries1, keys2, flips2, entries2)) return rc;
    if (int rc = gf2_gate_check_range(who, locations, site_loc, n1, n2, w, b, first_rank, count)) return rc;
    return ec_check_effects(who, eff, locations, ldr, rounds, r1, r2);
}

// ... and those of gf2_ft_gate_enumerate_host and gf2_ft_gate_enumerate_list_host.
int ft_gate_enumerate_check(const char* who, const uint64_t* eff, int64_t locations, int64_t ldr, int64_t nsteps, uint64_t measure_mask, int64_t r1,
                            const uint64_t* keys1, const uint8_t* flips1, int64_t entries1, int64_t r2, const uint64_t* keys2, const uint8_t* flips2,
                            int64_t entries2, const int32_t* site_loc, int64_t n1, int64_t n2, int64_t w, int64_t b, int64_t first_rank,
                            int64_t count) {
    if (ldr < 1) GF2_FAIL(GF2_E_ARG, "%s: needs ldr >= 1 words per effect", who);
    if (int rc = ft_check_layout(who, ldr, nsteps, measure_mask, r1, r2)) return rc;
    if (int rc = check_table_args(who, keys1, flips1, entries1, keys2, flips2, entries2)) return rc;
    if (int rc = gf2_gate_check_range(who, locations, site_loc, n1, n2, w, b, first_rank, count)) return rc;
    return ft_check_effects(who, eff, locations, ldr, nsteps, measure_mask, r1, r2);
}
}  // namespace

extern "C" {

// The definition of gf2_ec_gate_enumerate, serial: gate_walk, every configuration's outcome words judged by
// gf2_ec_tally_host's per-sample rule.
int gf2_ec_gate_enumerate_host(const uint64_t* eff, int64_t locations, int64_t ldr, int64_t rounds, int64_t r1, const uint64_t* keys1,
                               const uint8_t* flips1, int64_t entries1, int64_t r2, const uint64_t* keys2, const uint8_t* flips2,
                               int64_t entries2, const int32_t* site_loc, int64_t n1, int64_t n2, int64_t w, int64_t b, int64_t first_rank,
                               int64_t count, uint64_t* counts_out) {
    const char* who = "gf2_ec_gate_enumerate_host";
    if (!eff || !counts_out) GF2_FAIL(GF2_E_ARG, "%s: null argument", who);
    if (int rc = ec_gate_enumerate_check(who, eff, locations, ldr, rounds, r1, keys1, flips1, entries1, r2, keys2, flips2, entries2, site_loc, n1, n2, w, b,
                                         first_rank, count))
        return rc;
    const uint64_t mask[2] = {(1ull << r2) - 1, (1ull << r1) - 1};
    for (int64_t k = 0; k < (b + 1) * GF2_EC_FIELDS; ++k) counts_out[k] = 0;
    if (count == 0) return GF2_OK;
    HostTable tab[2];
    if (int rc = make_host_tables(who, tab, keys1, flips1, entries1, keys2, flips2, entries2)) return rc;
    gate_walk(eff, ldr, site_loc, n1, n2, w, b, first_rank, count, [&](int64_t, const int32_t*, const int*, int64_t c, const uint64_t* out) {
        (void)ec_tally_sample(out, ldr, rounds, mask, tab, counts_out + c * GF2_EC_FIELDS);
    });
    return GF2_OK;
}

// The definition of gf2_ft_gate_enumerate, likewise with gf2_ft_tally_host's rule.
int gf2_ft_gate_enumerate_host(const uint64_t* eff, int64_t locations, int64_t ldr, int64_t nsteps, uint64_t measure_mask, int64_t r1,
                               const uint64_t* keys1, const uint8_t* flips1, int64_t entries1, int64_t r2, const uint64_t* keys2,
                               const uint8_t* flips2, int64_t entries2, const int32_t* site_loc, int64_t n1, int64_t n2, int64_t w, int64_t b,
                               int64_t first_rank, int64_t count, uint64_t* counts_out) {
    const char* who = "gf2_ft_gate_enumerate_host";
    if (!eff || !counts_out) GF2_FAIL(GF2_E_ARG, "%s: null argument", who);
    if (int rc = ft_gate_enumerate_check(who, eff, locations, ldr, nsteps, measure_mask, r1, keys1, flips1, entries1, r2, keys2, flips2, entries2, site_loc,
                                         n1, n2, w, b, first_rank, count))
        return rc;
    const int trials = __builtin_popcountll(measure_mask);
    const uint64_t mask[2] = {(1ull << r2) - 1, (1ull << r1) - 1};
    for (int64_t k = 0; k < (b + 1) * GF2_FT_FIELDS; ++k) counts_out[k] = 0;
    if (count == 0) return GF2_OK;
    HostTable tab[2];
    if (int rc = make_host_tables(who, tab, keys1, flips1, entries1, keys2, flips2, entries2)) return rc;
    gate_walk(eff, ldr, site_loc, n1, n2, w, b, first_rank, count, [&](int64_t, const int32_t*, const int*, int64_t c, const uint64_t* out) {
        (void)ft_tally_sample(out, ldr, nsteps, measure_mask, trials, mask, tab, counts_out + c * GF2_FT_FIELDS);
    });
    return GF2_OK;
}

// The definition of gf2_ec_gate_enumerate_list (DESIGN.md section 5e "Malignant fault sets under gate-level faults"), serial:
// gf2_ec_gate_enumerate_host's walk and rule, the class byte of every configuration kept instead of its counts.
int gf2_ec_gate_enumerate_list_host(const uint64_t* eff, int64_t locations, int64_t ldr, int64_t rounds, int64_t r1, const uint64_t* keys1,
                                    const uint8_t* flips1, int64_t entries1, int64_t r2, const uint64_t* keys2, const uint8_t* flips2,
                                    int64_t entries2, const int32_t* site_loc, int64_t n1, int64_t n2, int64_t w, int64_t b,
                                    int64_t first_rank, int64_t count, uint64_t select, int64_t capacity, uint64_t* records_out,
                                    int64_t* found_out) {
    const char* who = "gf2_ec_gate_enumerate_list_host";
    if (!eff) GF2_FAIL(GF2_E_ARG, "%s: null argument", who);
    if (int rc = list_check_args(who, select, GF2_EC_CLASS_BITS, capacity, records_out, found_out)) return rc;
    if (int rc = ec_gate_enumerate_check(who, eff, locations, ldr, rounds, r1, keys1, flips1, entries1, r2, keys2, flips2, entries2, site_loc, n1, n2, w, b,
                                         first_rank, count))
        return rc;
    const uint64_t mask[2] = {(1ull << r2) - 1, (1ull << r1) - 1};
    *found_out = 0;
    if (count == 0) return GF2_OK;
    HostTable tab[2];
    if (int rc = make_host_tables(who, tab, keys1, flips1, entries1, keys2, flips2, entries2)) return rc;
    return gate_list_walk(who, eff, ldr, site_loc, n1, n2, w, b, first_rank, count, select, capacity, records_out, found_out, [&](const uint64_t* out) {
        uint64_t unused[GF2_EC_FIELDS] = {0};
        return ec_tally_sample(out, ldr, rounds, mask, tab, unused);
    });
}

// The definition of gf2_ft_gate_enumerate_list, likewise.
int gf2_ft_gate_enumerate_list_host(const uint64_t* eff, int64_t locations, int64_t ldr, int64_t nsteps, uint64_t measure_mask, int64_t r1,
                                    const uint64_t* keys1, const uint8_t* flips1, int64_t entries1, int64_t r2, const uint64_t* keys2,
                                    const uint8_t* flips2, int64_t entries2, const int32_t* site_loc, int64_t n1, int64_t n2, int64_t w,
                                    int64_t b, int64_t first_rank, int64_t count, uint64_t select, int64_t capacity, uint64_t* records_out,
                                    int64_t* found_out) {
    const char* who = "gf2_ft_gate_enumerate_list_host";
    if (!eff) GF2_FAIL(GF2_E_ARG, "%s: null argument", who);
    if (int rc = list_check_args(who, select, GF2_FT_CLASS_BITS, capacity, records_out, found_out)) return rc;
    if (int rc = ft_gate_enumerate_check(who, eff, locations, ldr, nsteps, measure_mask, r1, keys1, flips1, entries1, r2, keys2, flips2, entries2, site_loc,
                                         n1, n2, w, b, first_rank, count))
        return rc;
    const int trials = __builtin_popcountll(measure_mask);
    const uint64_t mask[2] = {(1ull << r2) - 1, (1ull << r1) - 1};
    *found_out = 0;
    if (count == 0) return GF2_OK;
    HostTable tab[2];
    if (int rc = make_host_tables(who, tab, keys1, flips1, entries1, keys2, flips2, entries2)) return rc;
    return gate_list_walk(who, eff, ldr, site_loc, n1, n2, w, b, first_rank, count, select, capacity, records_out, found_out, [&](const uint64_t* out) {
        uint64_t unused[GF2_FT_FIELDS] = {0};
        return ft_tally_sample(out, ldr, nsteps, measure_mask, trials, mask, tab, unused);
    });
}

}  // extern "C"

// ---- sampled strata under gate-level faults (include/gf2hip.h "sampled strata ... under gate-level faults") --
// The limits of one stratum (a, b), shared by the host statement below and the device entry points (gf2_gate_strata.hip); `at`
// names the stratum in the message ("" when the call has one).
int gf2_gate_check_stratum(const char* who, const char* at, int64_t n1, int64_t n2, int64_t a, int64_t b) {
    if (a < 0 || b < 0 || a + b > GF2_GATE_STRATUM_MAX_WEIGHT)
        GF2_FAIL(GF2_E_ARG, "%s: %sneeds a, b >= 0 and a + b <= %d faulty gates, got a = %lld and b = %lld", who, at,
                 GF2_GATE_STRATUM_MAX_WEIGHT, (long long)a, (long long)b);
    if (a > n1 || b > n2)
        GF2_FAIL(GF2_E_ARG, "%s: %sneeds a <= n_1 = %lld and b <= n_2 = %lld, got a = %lld and b = %lld", who, at, (long long)n1,
                 (long long)n2, (long long)a, (long long)b);
    return GF2_OK;
}

extern "C" {

// The outcome words and two-operand counts of a gadget's stratified samples under gate-level faults, the host statement of what
// gate_strata_kernel draws: the generator of gf2_stratum_outcomes_host over sites, one array of picks in the unified site numbering
// for Floyd's comparison (the two ranges are disjoint).  gf2_ec_tally_host / gf2_ft_tally_host judge the words; no tally rule is
// repeated here.
int gf2_gate_stratum_outcomes_host(const uint64_t* eff, int64_t locations, int64_t ldr, const int32_t* site_loc, int64_t n1, int64_t n2,
                                   int64_t a, int64_t b, uint64_t seed, int64_t first_sample, int64_t count, uint64_t* words_out,
                                   int64_t ldw, uint8_t* two_operand_out) {
    const char* who = "gf2_gate_stratum_outcomes_host";
    if (!eff) GF2_FAIL(GF2_E_ARG, "%s: null argument", who);
    if (ldr < 1 || ldr > GF2_FT_MAX_LDR) GF2_FAIL(GF2_E_ARG, "%s: needs 1 <= ldr <= %d words per effect, got %lld", who, GF2_FT_MAX_LDR, (long long)ldr);
    if (int rc = gf2_gate_check_sites(who, locations, site_loc, n1, n2)) return rc;
    if (int rc = gf2_gate_check_stratum(who, "", n1, n2, a, b)) return rc;
    if (count < 0 || first_sample < 0) GF2_FAIL(GF2_E_ARG, "%s: negative range (needs count >= 0 and first_sample >= 0)", who);
    if (ldw < ldr) GF2_FAIL(GF2_E_ARG, "%s: ldw must be at least the table's %lld words", who, (long long)ldr);
    if (count > 0 && (!words_out || !two_operand_out)) GF2_FAIL(GF2_E_ARG, "%s: null buffer", who);
    const uint64_t golden = 0x9E3779B97F4A7C15ull, stream = 0xD1B54A32D192ED03ull;
    for (int64_t i = 0; i < count; ++i) {
        uint64_t* const out = words_out + i * ldw;
        for (int64_t q = 0; q < ldr; ++q) out[q] = 0;
        const uint64_t ks = host_mix64(seed + golden * ((uint64_t)(first_sample + i) + 1));
        const uint64_t d = host_mix64(ks + stream * ((uint64_t)(64 + 17 * b + a) + 1));   // the segment slot carries the stratum
        uint64_t picks[GF2_GATE_STRATUM_MAX_WEIGHT];
        unsigned c = 0;
        for (int64_t k = 0; k < a + b; ++k) {
            const uint64_t v = host_mix64(d + golden * (uint64_t)(k + 1));
            const uint64_t hi = v >> 32, lo = v & 0xFFFFFFFFull;
            const bool one = k < a;
            const uint64_t base = one ? 0 : (uint64_t)n1;
            const uint64_t j = one ? (uint64_t)(n1 - a + k) : (uint64_t)(n2 - b + (k - a));
            const uint64_t t = base + ((hi * (j + 1)) >> 32);                    // Floyd: a candidate in [0, j] of its class
            bool taken = false;
            for (int64_t q = 0; q < k; ++q) taken |= picks[q] == t;
            picks[k] = taken ? base + j : t;
            const uint64_t kappa = 1 + ((lo * (one ? 3u : 15u)) >> 32);
            const uint64_t* e = eff + (size_t)(2 * site_loc[picks[k]]) * ldr;     // effect t of the site: (2 l + t) ldr
            for (int bit = 0; bit < 4; ++bit)
                if ((kappa >> bit) & 1)
                    for (int64_t q = 0; q < ldr; ++q) out[q] ^= e[bit * ldr + q];
            c += (kappa & 3) != 0 && (kappa >> 2) != 0;
        }
        two_operand_out[i] = (uint8_t)c;
    }
    return GF2_OK;
}

}  // extern "C"

// ---- direct Monte-Carlo under gate-level faults (include/gf2hip.h "direct Monte-Carlo ... under gate-level faults") --
// The argument rules of the two rates and of the sample range, shared by the host statement below and the device entry points
// (gf2_gate_mc.hip).
int gf2_gate_check_mc(const char* who, double p1, double p2, int64_t first_sample, int64_t count) {
    if (!(p1 >= 0.0) || !(p1 <= 1.0) || !(p2 >= 0.0) || !(p2 <= 1.0))
        GF2_FAIL(GF2_E_ARG, "%s: needs 0 <= p_1, p_2 <= 1, got p_1 = %g and p_2 = %g", who, p1, p2);
    if (count < 0 || first_sample < 0) GF2_FAIL(GF2_E_ARG, "%s: negative range (needs count >= 0 and first_sample >= 0)", who);
    return GF2_OK;
}

// binomial_cdf_direct and binomial_cdf_table of gf2_sampler.h (that header is device code) in the same IEEE operations, in this order.
static void host_binomial_cdf_direct(uint64_t t_any, int nb, uint64_t* cdf, int cap) {
    for (int k = 0; k < cap; ++k) cdf[k] = 4294967296ull;
    if (nb <= 0) return;
    if (t_any >= 4294967296ull) {
        for (int k = 0; k < nb; ++k) cdf[k] = 0;
        return;
    }
    const double q = (double)t_any / 4294967296.0, om = 1.0 - q;
    double pmf = 1.0;
    for (int i = 0; i < nb; ++i) pmf *= om;
    double cum = 0.0;
    for (int k = 0; k < nb; ++k) {
        cum += pmf;
        double c = __builtin_floor(cum * 4294967296.0 + 0.5);
        if (c > 4294967296.0) c = 4294967296.0;
        cdf[k] = (uint64_t)c;
        pmf = pmf * (double)(nb - k) / (double)(k + 1) * q / om;
    }
}

static void host_binomial_cdf_table(uint64_t t_any, int nb, uint64_t* cdf) {     // cdf[513]: a segment's 512 sites and one
    const int cap = 513;
    if (t_any <= 2147483648ull || t_any >= 4294967296ull) {
        host_binomial_cdf_direct(t_any, nb, cdf, cap);
        return;
    }
    uint64_t other[513];
    host_binomial_cdf_direct(4294967296ull - t_any, nb, other, cap);
    for (int k = 0; k < cap; ++k) cdf[k] = 4294967296ull;
    for (int k = 0; k < nb; ++k) cdf[k] = 4294967296ull - other[nb - k - 1];
}

extern "C" {

// The outcome words and fault counts of a gadget's samples when every gate fails on its own, the host statement of what
// gate_mc_kernel draws: the segment sampler of gf2_sampler.h run over the one-operand sites and then over the CNOT sites, each class
// with its own slots, rate and radix of kinds, a pick's effects XOR-ed as gf2_gate_stratum_outcomes_host does.  gf2_ec_tally_host /
// gf2_ft_tally_host judge the words; no tally rule is repeated here.
int gf2_gate_outcomes_host(const uint64_t* eff, int64_t locations, int64_t ldr, const int32_t* site_loc, int64_t n1, int64_t n2,
                           uint64_t seed, int64_t first_sample, int64_t count, double p1, double p2, uint64_t* words_out, int64_t ldw,
                           int32_t* faults_out) {
    const char* who = "gf2_gate_outcomes_host";
    if (!eff) GF2_FAIL(GF2_E_ARG, "%s: null argument", who);
    if (ldr < 1 || ldr > GF2_FT_MAX_LDR) GF2_FAIL(GF2_E_ARG, "%s: needs 1 <= ldr <= %d words per effect, got %lld", who, GF2_FT_MAX_LDR, (long long)ldr);
    if (int rc = gf2_gate_check_sites(who, locations, site_loc, n1, n2)) return rc;
    if (int rc = gf2_gate_check_mc(who, p1, p2, first_sample, count)) return rc;
    if (ldw < ldr) GF2_FAIL(GF2_E_ARG, "%s: ldw must be at least the table's %lld words", who, (long long)ldr);
    if (count > 0 && !words_out) GF2_FAIL(GF2_E_ARG, "%s: null buffer", who);
    const uint64_t golden = 0x9E3779B97F4A7C15ull, stream = 0xD1B54A32D192ED03ull;
    const int SEG = 512;
    const int64_t m[2] = {n1, n2}, site_base[2] = {0, n1};
    const uint64_t radix[2] = {3, 15}, slot_base[2] = {GF2_GATE_MC_SLOT_ONE, GF2_GATE_MC_SLOT_CNOT};
    const uint64_t T[2] = {host_quantise(p1), host_quantise(p2)};
    std::vector<uint64_t> cdf;                                                   // [class][whole, last][SEG + 1]
    try {
        cdf.resize(4 * (SEG + 1));
    } catch (const std::bad_alloc&) {
        GF2_FAIL(GF2_E_NOMEM, "%s: out of host memory", who);
    }
    for (int cl = 0; cl < 2; ++cl) {
        host_binomial_cdf_table(T[cl], SEG, &cdf[(2 * cl) * (SEG + 1)]);
        host_binomial_cdf_table(T[cl], m[cl] > 0 ? (int)(m[cl] - ((m[cl] - 1) / SEG) * SEG) : 0, &cdf[(2 * cl + 1) * (SEG + 1)]);
    }
    for (int64_t i = 0; i < count; ++i) {
        uint64_t* const out = words_out + i * ldw;
        for (int64_t q = 0; q < ldr; ++q) out[q] = 0;
        const uint64_t ks = host_mix64(seed + golden * ((uint64_t)(first_sample + i) + 1));
        int32_t faults[3] = {0, 0, 0};
        for (int cl = 0; cl < 2; ++cl) {
            const int64_t nseg = (m[cl] + SEG - 1) / SEG;                        // (none for an empty class)
            for (int64_t s = 0; s < nseg; ++s) {
                const bool last = s == nseg - 1;
                const int nb = last ? (int)(m[cl] - SEG * s) : SEG;
                const uint64_t* table = &cdf[(2 * cl + (last ? 1 : 0)) * (SEG + 1)];
                const uint64_t d = host_mix64(ks + stream * (slot_base[cl] + (uint64_t)s + 1));
                const uint64_t u = d >> 32;
                int K = 0;
                while (K < nb && u >= table[K]) K += 1;
                uint64_t taken[SEG / 64] = {0, 0, 0, 0, 0, 0, 0, 0};
                for (int k = 0; k < K; ++k) {
                    const uint64_t v = host_mix64(d + golden * (uint64_t)(k + 1));
                    const uint64_t hi = v >> 32, lo = v & 0xFFFFFFFFull;
                    const uint64_t j = (uint64_t)(nb - K + k);
                    const uint64_t t = (hi * (j + 1)) >> 32;                      // Floyd: a candidate in [0, j]
                    const uint64_t pos = ((taken[t >> 6] >> (t & 63)) & 1ull) ? j : t;
                    taken[pos >> 6] |= 1ull << (pos & 63);
                    const uint64_t kappa = 1 + ((lo * radix[cl]) >> 32);
                    const int64_t site = site_base[cl] + SEG * s + (int64_t)pos;
                    const uint64_t* e = eff + (size_t)(2 * site_loc[site]) * ldr;  // effect t of the site: (2 l + t) ldr
                    for (int bit = 0; bit < 4; ++bit)
                        if ((kappa >> bit) & 1)
                            for (int64_t q = 0; q < ldr; ++q) out[q] ^= e[bit * ldr + q];
                    faults[cl] += 1;
                    if (cl == 1) faults[2] += (kappa & 3) != 0 && (kappa >> 2) != 0;
                }
            }
        }
        if (faults_out)
            for (int q = 0; q < 3; ++q) faults_out[3 * i + q] = faults[q];
    }
    return GF2_OK;
}

}  // extern "C"

// ---- streamed gadgets (include/gf2hip.h "streamed gadgets") -------------------------------------------
#include "gf2_stream_plan.h"

int gf2_stream_plan(const char* who, const uint64_t* type_eff, const int64_t* type_locations, const int64_t* type_flags, int64_t ntypes,
                    const int32_t* block_type, const int32_t* block_kind, int64_t nblocks, StreamPlan* plan) {
    if (!type_eff || !type_locations || !type_flags || !block_type || !block_kind || !plan) GF2_FAIL(GF2_E_ARG, "%s: null argument", who);
    if (ntypes < 1 || ntypes > GF2_STREAM_MAX_TYPES)
        GF2_FAIL(GF2_E_ARG, "%s: needs 1 <= ntypes <= %d block types, got %lld", who, GF2_STREAM_MAX_TYPES, (long long)ntypes);
    if (nblocks < 1 || nblocks > GF2_CIRCUIT_MAX_LOCATIONS + 1)
        GF2_FAIL(GF2_E_ARG, "%s: needs 1 <= nblocks <= %d blocks, got %lld", who, GF2_CIRCUIT_MAX_LOCATIONS + 1, (long long)nblocks);
    try {
        plan->type_offset.assign((size_t)ntypes, 0);
        plan->start.assign((size_t)nblocks + 1, 0);
        plan->step.assign((size_t)nblocks, -1);
        plan->flag.assign((size_t)nblocks, 0);
    } catch (const std::bad_alloc&) {
        GF2_FAIL(GF2_E_NOMEM, "%s: out of host memory", who);
    }
    int64_t table = 0;
    for (int64_t t = 0; t < ntypes; ++t) {
        if (type_locations[t] < 1 || type_locations[t] > GF2_CIRCUIT_MAX_LOCATIONS)
            GF2_FAIL(GF2_E_ARG, "%s: block type %lld needs 1 <= locations <= %d (2^20), got %lld", who, (long long)t, GF2_CIRCUIT_MAX_LOCATIONS,
                     (long long)type_locations[t]);
        if (type_flags[t] < 0 || type_flags[t] > 64)
            GF2_FAIL(GF2_E_ARG, "%s: block type %lld has %lld flag rows, a block holds at most 64 (one flag word)", who, (long long)t,
                     (long long)type_flags[t]);
        plan->type_offset[(size_t)t] = table;
        table += type_locations[t];
        if (table > GF2_CIRCUIT_MAX_LOCATIONS)
            GF2_FAIL(GF2_E_ARG, "%s: the block types have more than %d (2^20) locations in all", who, GF2_CIRCUIT_MAX_LOCATIONS);
    }
    // OR of every type's three words
    std::vector<uint64_t> any;
    try {
        any.assign((size_t)ntypes * 3, 0);
    } catch (const std::bad_alloc&) {
        GF2_FAIL(GF2_E_NOMEM, "%s: out of host memory", who);
    }
    for (int64_t t = 0; t < ntypes; ++t)
        for (int64_t i = 0; i < 2 * type_locations[t]; ++i)
            for (int q = 0; q < 3; ++q) any[(size_t)(3 * t + q)] |= type_eff[(2 * plan->type_offset[(size_t)t] + i) * 3 + q];
    plan->any_tail = 0;
    for (int k = 0; k < 4; ++k) plan->any_local[k] = 0;
    int64_t at = 0, steps = 0, rows = 0, trials = 0, finals = 0;
    for (int64_t b = 0; b < nblocks; ++b) {
        const int kind = block_kind[b];
        if (kind < GF2_STREAM_NONE || kind > GF2_STREAM_FINAL)
            GF2_FAIL(GF2_E_ARG, "%s: block %lld has kind %d, not NONE (0), EC (1), MEASURE (2) or FINAL (3)", who, (long long)b, kind);
        plan->start[(size_t)b] = (int32_t)at;
        plan->flag[(size_t)b] = (int32_t)rows;
        if (kind != GF2_STREAM_NONE) plan->step[(size_t)b] = (int32_t)steps++;
        if (kind == GF2_STREAM_FINAL) {
            if (b != nblocks - 1) GF2_FAIL(GF2_E_ARG, "%s: the FINAL step must be the last step, block %lld of %lld is one", who, (long long)b, (long long)nblocks);
            if (block_type[b] != -1) GF2_FAIL(GF2_E_ARG, "%s: the FINAL step has no locations, its block type must be -1", who);
            finals += 1;
            continue;
        }
        const int64_t t = block_type[b];
        if (t < 0 || t >= ntypes) GF2_FAIL(GF2_E_ARG, "%s: block %lld has type %lld outside [0, %lld)", who, (long long)b, (long long)t, (long long)ntypes);
        trials += kind == GF2_STREAM_MEASURE;
        at += type_locations[t];
        rows += type_flags[t];
        if (at > GF2_CIRCUIT_MAX_LOCATIONS)
            GF2_FAIL(GF2_E_ARG, "%s: the sequence has more than L = %d (2^20) fault locations", who, GF2_CIRCUIT_MAX_LOCATIONS);
        plan->any_local[kind] |= any[(size_t)(3 * t)];
        plan->any_tail |= any[(size_t)(3 * t + 1)];
        if (type_flags[t] < 64 && (any[(size_t)(3 * t + 2)] >> type_flags[t]) != 0)
            GF2_FAIL(GF2_E_ARG, "%s: the effects of block type %lld set flag bits at or above its %lld flag rows", who, (long long)t, (long long)type_flags[t]);
    }
    plan->start[(size_t)nblocks] = (int32_t)at;
    if (at < 1) GF2_FAIL(GF2_E_ARG, "%s: the sequence has no fault location", who);
    if (!finals && trials % 2 == 0)
        GF2_FAIL(GF2_E_ARG, "%s: a sequence needs one FINAL step as its last step, or an odd number of MEASURE steps (a majority vote) and no FINAL step; "
                 "it has no FINAL step and %lld MEASURE steps", who, (long long)trials);
    plan->locations = at;
    plan->nsteps = steps;
    plan->flag_rows = rows;
    plan->flag_words = rows > 64 ? (rows + 63) / 64 : 1;
    plan->trials = trials;
    plan->has_final = finals != 0;
    return GF2_OK;
}

int gf2_stream_check_bits(const char* who, const StreamPlan& plan, int64_t r1, int64_t r2) {
    GadgetRule rule;
    if (int rc = gadget_rule_keys(who, r1, r2, &rule)) return rc;
    const uint64_t key_x = rule.mask[0], keys = key_x | rule.mask[1] << 32;
    if (plan.any_local[GF2_STREAM_NONE] || (plan.any_local[GF2_STREAM_EC] & ~keys) || (plan.any_local[GF2_STREAM_MEASURE] & ~(key_x | 1ull << 31)) ||
        (plan.any_tail & ~(keys | 1ull << 31 | 1ull << 63)))
        GF2_FAIL(GF2_E_ARG, "%s: the effects set bits beyond the layout (a NONE block no local bit, an EC step's r_2 / r_1 key bits, a MEASURE step's r_2 key "
                 "bits and bit 31, a tail's key bits and the two parity bits)", who);
    return GF2_OK;
}

namespace {
// One sample of the streamed tally rule: gf2_ec_tally_host's and gf2_ft_tally_host's per-sample rules, the steps' kinds read from a
// list and no bound on their number.  w: the sample's stream-layout words.
uint8_t stream_tally_sample(const uint64_t* w, const std::vector<int>& kinds, int64_t flag_words, int64_t trials, const uint64_t* mask,
                            const HostTable* tab, uint64_t* counts) {
    const int64_t nsteps = (int64_t)kinds.size();
    uint64_t flags = 0;
    for (int64_t q = 0; q < flag_words; ++q) flags |= w[nsteps + q];
    if (flags) return 0;
    uint64_t K[2] = {0, 0}, P[2] = {0, 0}, unmatched[2] = {0, 0};
    int64_t wrong_trials = 0, seen_trials = 0;
    bool first_wrong = false, flip[2] = {false, false}, miss[2] = {false, false};
    for (int64_t s = 0; s < nsteps; ++s) {
        const int kind = kinds[(size_t)s];
        if (kind == GF2_STREAM_FINAL) {
            for (int c = 0; c < 2; ++c) {
                const uint64_t v = ((w[s] >> (32 * c)) & mask[c]) ^ K[c];
                const int found = tab[c].find(0, v);
                miss[c] = found < 0;
                flip[c] = (((w[s] >> (32 * c + 31)) & 1ull) ^ P[c] ^ (uint64_t)(found > 0)) != 0;
            }
            continue;
        }
        const bool measure = kind == GF2_STREAM_MEASURE;
        for (int c = 0; c < (measure ? 1 : 2); ++c) {
            const uint64_t v = ((w[s] >> (32 * c)) & mask[c]) ^ K[c];
            const int found = tab[c].find(0, v);
            if (found < 0)
                unmatched[c] += 1;                                       // css_code.py:655-657: no match, nothing recorded
            else
                K[c] ^= v, P[c] ^= (uint64_t)found;
        }
        if (measure) {
            const bool bad = (((w[s] >> 31) & 1ull) ^ P[0]) != 0;
            if (seen_trials == 0) first_wrong = bad;
            wrong_trials += bad;
            seen_trials += 1;
        }
    }
    const bool wrong = 2 * wrong_trials > trials, split = wrong_trials != 0 && wrong_trials != trials;
    counts[0] += 1;
    counts[1] += flip[0];
    counts[2] += flip[1];
    counts[3] += flip[0] | flip[1];
    counts[4] += miss[0];
    counts[5] += miss[1];
    counts[6] += unmatched[0];
    counts[7] += unmatched[1];
    counts[8] += wrong;
    counts[9] += (uint64_t)wrong_trials;
    counts[10] += first_wrong;
    counts[11] += split;
    return (uint8_t)(1 | flip[0] << 1 | flip[1] << 2 | miss[0] << 3 | miss[1] << 4 | wrong << 5 | first_wrong << 6 | split << 7);
}
}  // namespace

extern "C" {

// The definition of gf2_stream_outcomes_dev's words given a sample's faults, serial: the faults are XOR-ed
// into (local, tail, flags) of their blocks, then the blocks are closed in order -- word = mask_kind(T) ^ local, T ^= tail.
int gf2_stream_words_host(const uint64_t* type_eff, const int64_t* type_locations, const int64_t* type_flags, int64_t ntypes,
                          const int32_t* block_type, const int32_t* block_kind, int64_t nblocks, const int64_t* fault_first,
                          const int32_t* fault_location, const uint8_t* fault_kind, int64_t count, uint64_t* words_out, int64_t ldw) {
    const char* who = "gf2_stream_words_host";
    StreamPlan plan;
    if (int rc = gf2_stream_plan(who, type_eff, type_locations, type_flags, ntypes, block_type, block_kind, nblocks, &plan)) return rc;
    const int64_t ldr = plan.nsteps + plan.flag_words;
    if (count < 0 || ldw < ldr) GF2_FAIL(GF2_E_ARG, "%s: needs count >= 0 samples of ldw >= nsteps + F = %lld words", who, (long long)ldr);
    if (count == 0) return GF2_OK;
    if (!fault_first || !words_out) GF2_FAIL(GF2_E_ARG, "%s: null argument", who);
    if (fault_first[0] != 0) GF2_FAIL(GF2_E_ARG, "%s: fault_first[0] must be 0", who);
    for (int64_t i = 0; i < count; ++i)
        if (fault_first[i + 1] < fault_first[i]) GF2_FAIL(GF2_E_ARG, "%s: fault_first must not descend (sample %lld)", who, (long long)i);
    const int64_t nfaults = fault_first[count];
    if (nfaults > 0 && (!fault_location || !fault_kind)) GF2_FAIL(GF2_E_ARG, "%s: null fault list", who);
    for (int64_t f = 0; f < nfaults; ++f) {
        if (fault_location[f] < 0 || fault_location[f] >= plan.locations)
            GF2_FAIL(GF2_E_ARG, "%s: fault %lld is at location %lld outside [0, L = %lld)", who, (long long)f, (long long)fault_location[f], (long long)plan.locations);
        if (fault_kind[f] < 1 || fault_kind[f] > 3) GF2_FAIL(GF2_E_ARG, "%s: fault %lld has kind %d, not 1 (X), 2 (Z) or 3 (Y)", who, (long long)f, (int)fault_kind[f]);
    }
    std::vector<uint64_t> acc;
    try {
        acc.assign((size_t)nblocks * 3, 0);
    } catch (const std::bad_alloc&) {
        GF2_FAIL(GF2_E_NOMEM, "%s: out of host memory", who);
    }
    for (int64_t i = 0; i < count; ++i) {
        uint64_t* out = words_out + i * ldw;
        for (int64_t q = 0; q < ldr; ++q) out[q] = 0;
        for (int64_t f = fault_first[i]; f < fault_first[i + 1]; ++f) {
            const int32_t g = fault_location[f];
            const int64_t b = (std::upper_bound(plan.start.begin(), plan.start.end(), g) - plan.start.begin()) - 1;   // start[b] <= g < start[b + 1]
            const uint64_t* e = type_eff + (size_t)(plan.type_offset[(size_t)block_type[b]] + (g - plan.start[(size_t)b])) * 6;
            for (int comp = 0; comp < 2; ++comp)
                if (fault_kind[f] >> comp & 1)
                    for (int q = 0; q < 3; ++q) acc[(size_t)(3 * b + q)] ^= e[3 * comp + q];
        }
        uint64_t T = 0;
        for (int64_t b = 0; b < nblocks; ++b) {
            uint64_t* a = &acc[(size_t)(3 * b)];
            if (plan.step[(size_t)b] >= 0) out[plan.step[(size_t)b]] = (T & gf2_stream_frame_mask(block_kind[b])) ^ a[0];
            if (a[2]) {
                const int64_t row = plan.flag[(size_t)b];
                out[plan.nsteps + (row >> 6)] |= a[2] << (row & 63);
                if (row & 63) {
                    const uint64_t over = a[2] >> (64 - (row & 63));
                    if (over) out[plan.nsteps + (row >> 6) + 1] |= over;
                }
            }
            T ^= a[1];
            a[0] = a[1] = a[2] = 0;
        }
    }
    return GF2_OK;
}

// The tally rule of a streamed gadget over stream-layout words, serial: gf2_ec_tally_host's and
// gf2_ft_tally_host's rules step by step, the kinds of the steps taken from the block kinds.
int gf2_stream_tally_host(const uint64_t* words, int64_t count, int64_t ldw, const int32_t* block_kind, int64_t nblocks, int64_t flag_words,
                          int64_t r1, const uint64_t* keys1, const uint8_t* flips1, int64_t entries1, int64_t r2, const uint64_t* keys2,
                          const uint8_t* flips2, int64_t entries2, uint64_t* counts_out, uint8_t* class_out) {
    const char* who = "gf2_stream_tally_host";
    if (!counts_out || !block_kind) GF2_FAIL(GF2_E_ARG, "%s: null argument", who);
    GadgetRule rule;
    if (int rc = gadget_rule_keys(who, r1, r2, &rule)) return rc;
    if (nblocks < 1 || nblocks > GF2_CIRCUIT_MAX_LOCATIONS + 1)
        GF2_FAIL(GF2_E_ARG, "%s: needs 1 <= nblocks <= %d blocks, got %lld", who, GF2_CIRCUIT_MAX_LOCATIONS + 1, (long long)nblocks);
    std::vector<int> kinds;
    int64_t trials = 0, finals = 0;
    try {
        for (int64_t b = 0; b < nblocks; ++b) {
            const int kind = block_kind[b];
            if (kind < GF2_STREAM_NONE || kind > GF2_STREAM_FINAL)
                GF2_FAIL(GF2_E_ARG, "%s: block %lld has kind %d, not NONE (0), EC (1), MEASURE (2) or FINAL (3)", who, (long long)b, kind);
            if (kind == GF2_STREAM_FINAL && b != nblocks - 1)
                GF2_FAIL(GF2_E_ARG, "%s: the FINAL step must be the last step, block %lld of %lld is one", who, (long long)b, (long long)nblocks);
            trials += kind == GF2_STREAM_MEASURE;
            finals += kind == GF2_STREAM_FINAL;
            if (kind != GF2_STREAM_NONE) kinds.push_back(kind);
        }
    } catch (const std::bad_alloc&) {
        GF2_FAIL(GF2_E_NOMEM, "%s: out of host memory", who);
    }
    if (!finals && trials % 2 == 0)
        GF2_FAIL(GF2_E_ARG, "%s: a sequence needs one FINAL step as its last step, or an odd number of MEASURE steps (a majority vote) and no FINAL step; "
                 "it has no FINAL step and %lld MEASURE steps", who, (long long)trials);
    const int64_t ldr = (int64_t)kinds.size() + flag_words;
    if (flag_words < 1) GF2_FAIL(GF2_E_ARG, "%s: needs F >= 1 flag words, got %lld", who, (long long)flag_words);
    if (count < 0 || ldw < ldr || (count > 0 && !words)) GF2_FAIL(GF2_E_ARG, "%s: needs count >= 0 samples of ldw >= nsteps + F = %lld words", who, (long long)ldr);
    if (int rc = check_table_args(who, keys1, flips1, entries1, keys2, flips2, entries2)) return rc;
    for (int k = 0; k < GF2_STREAM_FIELDS; ++k) counts_out[k] = 0;
    if (count == 0) return GF2_OK;
    HostTable tab[2];
    if (int rc = make_host_tables(who, tab, keys1, flips1, entries1, keys2, flips2, entries2)) return rc;
    for (int64_t i = 0; i < count; ++i) {
        const uint8_t cls = stream_tally_sample(words + i * ldw, kinds, flag_words, trials, rule.mask, tab, counts_out);
        if (class_out) class_out[i] = cls;
    }
    return GF2_OK;
}

}  // extern "C"

// ---- multi-block streamed programs (include/gf2hip.h "multi-block streamed programs") ---------------------
#include "gf2_mstream_plan.h"

int gf2_mstream_check_records(const char* who, int64_t records) {
    if (records != GF2_MSTREAM_REFERENCE && records != GF2_MSTREAM_PROPAGATED)
        GF2_FAIL(GF2_E_ARG, "%s: records must be GF2_MSTREAM_REFERENCE (0) or GF2_MSTREAM_PROPAGATED (1), got %lld", who, (long long)records);
    return GF2_OK;
}

int gf2_mstream_block_rules(const char* who, const int32_t* block_kind, const int32_t* block_a, const int32_t* block_b, int64_t nblocks,
                            int64_t nframes, MStreamPlan* plan) {
    if (!block_kind || !block_a || !block_b || !plan) GF2_FAIL(GF2_E_ARG, "%s: null argument", who);
    if (nframes < 1 || nframes > GF2_MSTREAM_MAX_FRAMES)
        GF2_FAIL(GF2_E_ARG, "%s: needs 1 <= nframes <= %d data frames (logical qubits), got %lld", who, GF2_MSTREAM_MAX_FRAMES, (long long)nframes);
    if (nblocks < 1 || nblocks > GF2_CIRCUIT_MAX_LOCATIONS)
        GF2_FAIL(GF2_E_ARG, "%s: needs 1 <= nblocks <= %d blocks, got %lld", who, GF2_CIRCUIT_MAX_LOCATIONS, (long long)nblocks);
    try {
        plan->measure.assign((size_t)nblocks, -1);
        plan->first_trial.assign((size_t)nblocks, 0);
    } catch (const std::bad_alloc&) {
        GF2_FAIL(GF2_E_NOMEM, "%s: out of host memory", who);
    }
    int64_t trials_of[GF2_MSTREAM_MAX_FRAMES] = {0, 0, 0, 0};        // per frame: its MEASURE steps
    int64_t frame_of[GF2_MSTREAM_MAX_FRAMES] = {-1, -1, -1, -1};     // per measurement: its frame
    int64_t measurements = 0, steps = 0;
    for (int64_t b = 0; b < nblocks; ++b) {
        const int kind = block_kind[b];
        if (kind == GF2_STREAM_FINAL) GF2_FAIL(GF2_E_ARG, "%s: block %lld is a FINAL step, this route has none (a program ends with its MEASURE steps)", who, (long long)b);
        if (kind != GF2_STREAM_NONE && kind != GF2_STREAM_EC && kind != GF2_STREAM_MEASURE && kind != GF2_MSTREAM_CNOT)
            GF2_FAIL(GF2_E_ARG, "%s: block %lld has kind %d, not NONE (0), EC (1), MEASURE (2) or CNOT (4)", who, (long long)b, kind);
        if (block_a[b] < 0 || block_a[b] >= nframes)
            GF2_FAIL(GF2_E_ARG, "%s: block %lld has frame %lld outside [0, nframes = %lld)", who, (long long)b, (long long)block_a[b], (long long)nframes);
        if (kind == GF2_MSTREAM_CNOT) {
            if (block_b[b] < 0 || block_b[b] >= nframes)
                GF2_FAIL(GF2_E_ARG, "%s: CNOT block %lld has target frame %lld outside [0, nframes = %lld)", who, (long long)b, (long long)block_b[b], (long long)nframes);
            if (block_b[b] == block_a[b]) GF2_FAIL(GF2_E_ARG, "%s: CNOT block %lld has frame %lld as control and as target", who, (long long)b, (long long)block_a[b]);
        } else if (block_b[b] != -1) {
            GF2_FAIL(GF2_E_ARG, "%s: block %lld is no CNOT block, its second frame must be -1, got %lld", who, (long long)b, (long long)block_b[b]);
        }
        steps += kind == GF2_STREAM_EC || kind == GF2_STREAM_MEASURE;
        if (kind != GF2_STREAM_MEASURE) continue;
        const int64_t f = block_a[b];
        if (measurements == 0 || frame_of[measurements - 1] != f) {
            if (trials_of[f] != 0)
                GF2_FAIL(GF2_E_ARG, "%s: frame %lld is measured twice (MEASURE block %lld; the MEASURE steps of a frame follow one another)", who, (long long)f, (long long)b);
            frame_of[measurements++] = f;                             // (at most nframes <= 4 of them: every frame once)
            plan->first_trial[(size_t)b] = 1;
        }
        plan->measure[(size_t)b] = (int32_t)(measurements - 1);
        trials_of[f] += 1;
    }
    if (measurements < 1) GF2_FAIL(GF2_E_ARG, "%s: a sequence needs at least one MEASURE step", who);
    const int64_t trials = trials_of[frame_of[0]];
    for (int64_t m = 0; m < measurements; ++m)
        if (trials_of[frame_of[m]] != trials || trials % 2 == 0 || trials > GF2_MSTREAM_MAX_TRIALS)
            GF2_FAIL(GF2_E_ARG, "%s: every measurement needs the same odd number of MEASURE steps (a majority vote), at most %d; measurement %lld has %lld, "
                     "measurement 0 has %lld", who, GF2_MSTREAM_MAX_TRIALS, (long long)m, (long long)trials_of[frame_of[m]], (long long)trials);
    plan->nframes = nframes;
    plan->measurements = measurements;
    plan->seq.trials = trials;
    plan->seq.nsteps = steps;
    plan->seq.has_final = false;
    return GF2_OK;
}

// The type-table rules, the OR of every type's words, the start / step / flag fill and the flag-bit check below restate
// gf2_stream_plan's on purpose: that function and its messages keep their text, and this route differs in what a block may be (no FINAL
// step, CNOT blocks without a step word or flag rows, any_cnot beside any_local / any_tail).  A rule changed in one is changed in the
// other; tests/test_multi_stream.py pins every message of this copy, tests/test_stream.py those of the original.
int gf2_mstream_plan(const char* who, const uint64_t* type_eff, const int64_t* type_locations, const int64_t* type_flags, int64_t ntypes,
                     const int32_t* block_type, const int32_t* block_kind, const int32_t* block_a, const int32_t* block_b, int64_t nblocks,
                     int64_t nframes, MStreamPlan* plan) {
    if (!type_eff || !type_locations || !type_flags || !block_type || !block_kind || !block_a || !block_b || !plan) GF2_FAIL(GF2_E_ARG, "%s: null argument", who);
    if (ntypes < 1 || ntypes > GF2_STREAM_MAX_TYPES)
        GF2_FAIL(GF2_E_ARG, "%s: needs 1 <= ntypes <= %d block types, got %lld", who, GF2_STREAM_MAX_TYPES, (long long)ntypes);
    if (int rc = gf2_mstream_block_rules(who, block_kind, block_a, block_b, nblocks, nframes, plan)) return rc;
    StreamPlan& seq = plan->seq;
    std::vector<uint64_t> any;
    try {
        seq.type_offset.assign((size_t)ntypes, 0);
        seq.start.assign((size_t)nblocks + 1, 0);
        seq.step.assign((size_t)nblocks, -1);
        seq.flag.assign((size_t)nblocks, 0);
        any.assign((size_t)ntypes * 3, 0);
    } catch (const std::bad_alloc&) {
        GF2_FAIL(GF2_E_NOMEM, "%s: out of host memory", who);
    }
    int64_t table = 0;
    for (int64_t t = 0; t < ntypes; ++t) {
        if (type_locations[t] < 1 || type_locations[t] > GF2_CIRCUIT_MAX_LOCATIONS)
            GF2_FAIL(GF2_E_ARG, "%s: block type %lld needs 1 <= locations <= %d (2^20), got %lld", who, (long long)t, GF2_CIRCUIT_MAX_LOCATIONS,
                     (long long)type_locations[t]);
        if (type_flags[t] < 0 || type_flags[t] > 64)
            GF2_FAIL(GF2_E_ARG, "%s: block type %lld has %lld flag rows, a block holds at most 64 (one flag word)", who, (long long)t,
                     (long long)type_flags[t]);
        seq.type_offset[(size_t)t] = table;
        table += type_locations[t];
        if (table > GF2_CIRCUIT_MAX_LOCATIONS)
            GF2_FAIL(GF2_E_ARG, "%s: the block types have more than %d (2^20) locations in all", who, GF2_CIRCUIT_MAX_LOCATIONS);
    }
    for (int64_t t = 0; t < ntypes; ++t)                                 // OR of every type's three words
        for (int64_t i = 0; i < 2 * type_locations[t]; ++i)
            for (int q = 0; q < 3; ++q) any[(size_t)(3 * t + q)] |= type_eff[(2 * seq.type_offset[(size_t)t] + i) * 3 + q];
    seq.any_tail = 0;
    for (int k = 0; k < 4; ++k) seq.any_local[k] = 0;
    plan->any_cnot[0] = plan->any_cnot[1] = 0;
    int64_t at = 0, steps = 0, rows = 0;
    for (int64_t b = 0; b < nblocks; ++b) {
        const int kind = block_kind[b];
        const int64_t t = block_type[b];
        if (t < 0 || t >= ntypes) GF2_FAIL(GF2_E_ARG, "%s: block %lld has type %lld outside [0, %lld)", who, (long long)b, (long long)t, (long long)ntypes);
        seq.start[(size_t)b] = (int32_t)at;
        seq.flag[(size_t)b] = (int32_t)rows;
        if (kind == GF2_STREAM_EC || kind == GF2_STREAM_MEASURE) seq.step[(size_t)b] = (int32_t)steps++;
        if (kind == GF2_MSTREAM_CNOT && type_flags[t] != 0)
            GF2_FAIL(GF2_E_ARG, "%s: CNOT block %lld has a type with %lld flag rows, a CNOT block has none", who, (long long)b, (long long)type_flags[t]);
        at += type_locations[t];
        rows += type_flags[t];
        if (at > GF2_CIRCUIT_MAX_LOCATIONS)
            GF2_FAIL(GF2_E_ARG, "%s: the sequence has more than L = %d (2^20) fault locations", who, GF2_CIRCUIT_MAX_LOCATIONS);
        if (kind == GF2_MSTREAM_CNOT) {
            plan->any_cnot[0] |= any[(size_t)(3 * t)];
            plan->any_cnot[1] |= any[(size_t)(3 * t + 1)];
        } else {
            seq.any_local[kind] |= any[(size_t)(3 * t)];
            seq.any_tail |= any[(size_t)(3 * t + 1)];
        }
        if (type_flags[t] < 64 && (any[(size_t)(3 * t + 2)] >> type_flags[t]) != 0)
            GF2_FAIL(GF2_E_ARG, "%s: the effects of block type %lld set flag bits at or above its %lld flag rows", who, (long long)t, (long long)type_flags[t]);
    }
    seq.start[(size_t)nblocks] = (int32_t)at;
    seq.locations = at;
    seq.flag_rows = rows;
    seq.flag_words = rows > 64 ? (rows + 63) / 64 : 1;
    return GF2_OK;
}

int gf2_mstream_check_bits(const char* who, const MStreamPlan& plan, int64_t r1, int64_t r2) {
    GadgetRule rule;
    if (int rc = gadget_rule_keys(who, r1, r2, &rule)) return rc;
    const StreamPlan& seq = plan.seq;
    const uint64_t key_x = rule.mask[0], keys = key_x | rule.mask[1] << 32, frame = keys | 1ull << 31 | 1ull << 63;
    if (seq.any_local[GF2_STREAM_NONE] || (seq.any_local[GF2_STREAM_EC] & ~keys) || (seq.any_local[GF2_STREAM_MEASURE] & ~(key_x | 1ull << 31)) ||
        (seq.any_tail & ~frame) || (plan.any_cnot[0] & ~frame) || (plan.any_cnot[1] & ~frame))
        GF2_FAIL(GF2_E_ARG, "%s: the effects set bits beyond the layout (a NONE block no local bit, an EC step's r_2 / r_1 key bits, a MEASURE step's r_2 key "
                 "bits and bit 31, a tail's key bits and the two parity bits)", who);
    return GF2_OK;
}

int gf2_mstream_check_overlap(const char* who, const MStreamPlan& plan, int64_t nblocks) {
    const StreamPlan& seq = plan.seq;
    for (int64_t seg = 0, lo = 0; seg * 512 < seq.locations; ++seg) {
        const int64_t seg_start = seg * 512, seg_end = seg_start + 512 < seq.locations ? seg_start + 512 : seq.locations;
        while (seq.start[(size_t)lo + 1] <= seg_start) lo += 1;
        int64_t hi = lo;
        while (hi + 1 < nblocks && seq.start[(size_t)hi + 1] < seg_end) hi += 1;
        if (hi - lo + 1 > GF2_STREAM_MAX_OVERLAP)
            GF2_FAIL(GF2_E_ARG, "%s: locations %lld .. %lld (one 512-location segment of the sampler) overlap %lld blocks, more than %d (GF2_STREAM_MAX_OVERLAP)",
                     who, (long long)seg_start, (long long)seg_end - 1, (long long)(hi - lo + 1), GF2_STREAM_MAX_OVERLAP);
    }
    return GF2_OK;
}

namespace {
// One sample of the multi-block tally rule: stream_tally_sample's record (K, P) per side, kept per data frame; the blocks in order,
// because a CNOT block moves the records when `records` says so.  w: the sample's words, [steps] [flag words].
uint8_t mstream_tally_sample(const uint64_t* w, const int32_t* block_kind, const int32_t* block_a, const int32_t* block_b, int64_t nblocks,
                             const MStreamPlan& plan, int64_t flag_words, int64_t records, const uint64_t* mask, const HostTable* tab, uint64_t* counts) {
    const int64_t nsteps = plan.seq.nsteps, trials = plan.seq.trials;
    uint64_t flags = 0;
    for (int64_t q = 0; q < flag_words; ++q) flags |= w[nsteps + q];
    if (flags) return 0;
    uint64_t K[GF2_MSTREAM_MAX_FRAMES][2] = {}, P[GF2_MSTREAM_MAX_FRAMES][2] = {}, unmatched[2] = {0, 0};
    int64_t wrong_trials[GF2_MSTREAM_MAX_FRAMES] = {0, 0, 0, 0};
    bool first_wrong[GF2_MSTREAM_MAX_FRAMES] = {false, false, false, false};
    int64_t s = 0;
    for (int64_t b = 0; b < nblocks; ++b) {
        const int kind = block_kind[b], fa = block_a[b];
        if (kind == GF2_MSTREAM_CNOT) {
            if (records == GF2_MSTREAM_PROPAGATED) {
                const int fb = block_b[b];
                K[fb][0] ^= K[fa][0], P[fb][0] ^= P[fa][0];              // the x side goes a -> b
                K[fa][1] ^= K[fb][1], P[fa][1] ^= P[fb][1];              // the z side goes b -> a
            }
            continue;
        }
        if (kind == GF2_STREAM_NONE) continue;
        const bool measure = kind == GF2_STREAM_MEASURE;
        for (int c = 0; c < (measure ? 1 : 2); ++c) {
            const uint64_t v = ((w[s] >> (32 * c)) & mask[c]) ^ K[fa][c];
            const int found = tab[c].find(0, v);
            if (found < 0)
                unmatched[c] += 1;                                       // css_code.py:655-657: no match, nothing recorded
            else
                K[fa][c] ^= v, P[fa][c] ^= (uint64_t)found;
        }
        if (measure) {
            const int m = plan.measure[(size_t)b];
            const bool bad = (((w[s] >> 31) & 1ull) ^ P[fa][0]) != 0;
            if (plan.first_trial[(size_t)b]) first_wrong[m] = bad;
            wrong_trials[m] += bad;
        }
        s += 1;
    }
    bool any = false, any_split = false;
    counts[0] += 1;
    for (int64_t m = 0; m < plan.measurements; ++m) {
        const bool wrong = 2 * wrong_trials[m] > trials, split = wrong_trials[m] != 0 && wrong_trials[m] != trials;
        counts[4 + 4 * m] += wrong;
        counts[5 + 4 * m] += (uint64_t)wrong_trials[m];
        counts[6 + 4 * m] += first_wrong[m];
        counts[7 + 4 * m] += split;
        any |= wrong, any_split |= split;
    }
    counts[1] += any;
    counts[2] += unmatched[0];
    counts[3] += unmatched[1];
    uint8_t cls = (uint8_t)(1 | any << 1 | (unmatched[0] || unmatched[1]) << 6 | any_split << 7);
    for (int64_t m = 0; m < plan.measurements; ++m) cls |= (uint8_t)((2 * wrong_trials[m] > trials) << (2 + m));
    return cls;
}
}  // namespace

extern "C" {

// The definition of gf2_mstream_outcomes_dev's words given a sample's faults, serial: the faults are XOR-ed
// into the three words of their blocks, then the blocks are closed in order -- a CNOT block applies the frame map to (T_a, T_b) and
// XORs its two tails, any other block is gf2_stream_words_host's rule on T_a.
int gf2_mstream_words_host(const uint64_t* type_eff, const int64_t* type_locations, const int64_t* type_flags, int64_t ntypes,
                           const int32_t* block_type, const int32_t* block_kind, const int32_t* block_a, const int32_t* block_b, int64_t nblocks,
                           int64_t nframes, const int64_t* fault_first, const int32_t* fault_location, const uint8_t* fault_kind, int64_t count,
                           uint64_t* words_out, int64_t ldw) {
    const char* who = "gf2_mstream_words_host";
    MStreamPlan mplan;
    if (int rc = gf2_mstream_plan(who, type_eff, type_locations, type_flags, ntypes, block_type, block_kind, block_a, block_b, nblocks, nframes, &mplan)) return rc;
    const StreamPlan& plan = mplan.seq;
    const int64_t ldr = plan.nsteps + plan.flag_words;
    if (count < 0 || ldw < ldr) GF2_FAIL(GF2_E_ARG, "%s: needs count >= 0 samples of ldw >= nsteps + F = %lld words", who, (long long)ldr);
    if (count == 0) return GF2_OK;
    if (!fault_first || !words_out) GF2_FAIL(GF2_E_ARG, "%s: null argument", who);
    if (fault_first[0] != 0) GF2_FAIL(GF2_E_ARG, "%s: fault_first[0] must be 0", who);
    for (int64_t i = 0; i < count; ++i)
        if (fault_first[i + 1] < fault_first[i]) GF2_FAIL(GF2_E_ARG, "%s: fault_first must not descend (sample %lld)", who, (long long)i);
    const int64_t nfaults = fault_first[count];
    if (nfaults > 0 && (!fault_location || !fault_kind)) GF2_FAIL(GF2_E_ARG, "%s: null fault list", who);
    for (int64_t f = 0; f < nfaults; ++f) {
        if (fault_location[f] < 0 || fault_location[f] >= plan.locations)
            GF2_FAIL(GF2_E_ARG, "%s: fault %lld is at location %lld outside [0, L = %lld)", who, (long long)f, (long long)fault_location[f], (long long)plan.locations);
        if (fault_kind[f] < 1 || fault_kind[f] > 3) GF2_FAIL(GF2_E_ARG, "%s: fault %lld has kind %d, not 1 (X), 2 (Z) or 3 (Y)", who, (long long)f, (int)fault_kind[f]);
    }
    std::vector<uint64_t> acc;
    try {
        acc.assign((size_t)nblocks * 3, 0);
    } catch (const std::bad_alloc&) {
        GF2_FAIL(GF2_E_NOMEM, "%s: out of host memory", who);
    }
    for (int64_t i = 0; i < count; ++i) {
        uint64_t* out = words_out + i * ldw;
        for (int64_t q = 0; q < ldr; ++q) out[q] = 0;
        for (int64_t f = fault_first[i]; f < fault_first[i + 1]; ++f) {
            const int32_t g = fault_location[f];
            const int64_t b = (std::upper_bound(plan.start.begin(), plan.start.end(), g) - plan.start.begin()) - 1;   // start[b] <= g < start[b + 1]
            const uint64_t* e = type_eff + (size_t)(plan.type_offset[(size_t)block_type[b]] + (g - plan.start[(size_t)b])) * 6;
            for (int comp = 0; comp < 2; ++comp)
                if (fault_kind[f] >> comp & 1)
                    for (int q = 0; q < 3; ++q) acc[(size_t)(3 * b + q)] ^= e[3 * comp + q];
        }
        uint64_t T[GF2_MSTREAM_MAX_FRAMES] = {0, 0, 0, 0};
        for (int64_t b = 0; b < nblocks; ++b) {
            uint64_t* a = &acc[(size_t)(3 * b)];
            uint64_t& Ta = T[block_a[b]];
            if (block_kind[b] == GF2_MSTREAM_CNOT) {
                uint64_t& Tb = T[block_b[b]];
                gf2_mstream_cnot_map(&Ta, &Tb);
                Ta ^= a[0], Tb ^= a[1];                                  // a CNOT block's words: the tail for frame a, the tail for frame b
            } else {
                if (plan.step[(size_t)b] >= 0) out[plan.step[(size_t)b]] = (Ta & gf2_stream_frame_mask(block_kind[b])) ^ a[0];
                if (a[2]) {
                    const int64_t row = plan.flag[(size_t)b];
                    out[plan.nsteps + (row >> 6)] |= a[2] << (row & 63);
                    if (row & 63) {
                        const uint64_t over = a[2] >> (64 - (row & 63));
                        if (over) out[plan.nsteps + (row >> 6) + 1] |= over;
                    }
                }
                Ta ^= a[1];
            }
            a[0] = a[1] = a[2] = 0;
        }
    }
    return GF2_OK;
}

// The tally rule of a multi-block program over its words, serial.
int gf2_mstream_tally_host(const uint64_t* words, int64_t count, int64_t ldw, const int32_t* block_kind, const int32_t* block_a,
                           const int32_t* block_b, int64_t nblocks, int64_t nframes, int64_t flag_words, int64_t records, int64_t r1,
                           const uint64_t* keys1, const uint8_t* flips1, int64_t entries1, int64_t r2, const uint64_t* keys2,
                           const uint8_t* flips2, int64_t entries2, uint64_t* counts_out, uint8_t* class_out) {
    const char* who = "gf2_mstream_tally_host";
    if (!counts_out) GF2_FAIL(GF2_E_ARG, "%s: null argument", who);
    GadgetRule rule;
    if (int rc = gadget_rule_keys(who, r1, r2, &rule)) return rc;
    if (int rc = gf2_mstream_check_records(who, records)) return rc;
    MStreamPlan plan;
    if (int rc = gf2_mstream_block_rules(who, block_kind, block_a, block_b, nblocks, nframes, &plan)) return rc;
    const int64_t ldr = plan.seq.nsteps + flag_words;
    if (flag_words < 1) GF2_FAIL(GF2_E_ARG, "%s: needs F >= 1 flag words, got %lld", who, (long long)flag_words);
    if (count < 0 || ldw < ldr || (count > 0 && !words)) GF2_FAIL(GF2_E_ARG, "%s: needs count >= 0 samples of ldw >= nsteps + F = %lld words", who, (long long)ldr);
    if (int rc = check_table_args(who, keys1, flips1, entries1, keys2, flips2, entries2)) return rc;
    for (int k = 0; k < GF2_MSTREAM_FIELDS; ++k) counts_out[k] = 0;
    if (count == 0) return GF2_OK;
    HostTable tab[2];
    if (int rc = make_host_tables(who, tab, keys1, flips1, entries1, keys2, flips2, entries2)) return rc;
    for (int64_t i = 0; i < count; ++i) {
        const uint8_t cls = mstream_tally_sample(words + i * ldw, block_kind, block_a, block_b, nblocks, plan, flag_words, records, rule.mask, tab, counts_out);
        if (class_out) class_out[i] = cls;
    }
    return GF2_OK;
}

}  // extern "C"

// ---- repeat-until-success (include/gf2hip.h "repeat-until-success") -----------------------------------
#include "gf2_retry_plan.h"

int gf2_retry_plan(const char* who, const uint64_t* type_eff, const int64_t* type_locations, const int64_t* type_flags, int64_t ntypes,
                   const int32_t* block_type, const int32_t* block_kind, int64_t nblocks, const int64_t* type_regions,
                   const int64_t* type_nregions, int64_t max_attempts, StreamPlan* plan, RetryPlan* retry) {
    if (int rc = gf2_stream_plan(who, type_eff, type_locations, type_flags, ntypes, block_type, block_kind, nblocks, plan)) return rc;
    return gf2_retry_region_rules(who, type_eff, type_locations, ntypes, block_type, block_kind, nblocks, type_regions, type_nregions, max_attempts,
                                  *plan, retry);
}

int gf2_retry_region_rules(const char* who, const uint64_t* type_eff, const int64_t* type_locations, int64_t ntypes, const int32_t* block_type,
                           const int32_t* block_kind, int64_t nblocks, const int64_t* type_regions, const int64_t* type_nregions,
                           int64_t max_attempts, const StreamPlan& checked, RetryPlan* retry) {
    const StreamPlan* const plan = &checked;
    if (!type_regions || !type_nregions || !retry) GF2_FAIL(GF2_E_ARG, "%s: null argument", who);
    int64_t total = 0;
    for (int64_t t = 0; t < ntypes; ++t) {
        if (type_nregions[t] < 1 || type_nregions[t] > type_locations[t])
            GF2_FAIL(GF2_E_ARG, "%s: the regions of block type %lld do not partition its %lld locations in order: it has %lld regions", who,
                     (long long)t, (long long)type_locations[t], (long long)type_nregions[t]);
        total += type_nregions[t];
    }
    std::vector<uint64_t> masks;
    try {
        retry->type_first.assign((size_t)ntypes + 1, 0);
        retry->first.assign((size_t)total, 0);
        retry->count.assign((size_t)total, 0);
        retry->retried.assign((size_t)total, 0);
        retry->last_size.assign((size_t)total, 0);
        retry->sizes.clear();
        masks.assign((size_t)total, 0);
    } catch (const std::bad_alloc&) {
        GF2_FAIL(GF2_E_NOMEM, "%s: out of host memory", who);
    }
    std::vector<int32_t> sizes;                                                  // a set of at most GF2_RETRY_MAX_SIZES + 1 values
    auto note_size = [&](int32_t nb) {
        if (std::find(sizes.begin(), sizes.end(), nb) == sizes.end() && sizes.size() <= (size_t)GF2_RETRY_MAX_SIZES) sizes.push_back(nb);
    };
    int64_t at = 0;
    try {
        sizes.reserve(GF2_RETRY_MAX_SIZES + 1);
    } catch (const std::bad_alloc&) {
        GF2_FAIL(GF2_E_NOMEM, "%s: out of host memory", who);
    }
    for (int64_t t = 0; t < ntypes; ++t) {
        retry->type_first[(size_t)t] = at;
        int64_t next = 0;
        for (int64_t r = 0; r < type_nregions[t]; ++r, ++at) {
            const int64_t first = type_regions[3 * at], count = type_regions[3 * at + 1], retried = type_regions[3 * at + 2];
            if (first != next || count < 1 || count > type_locations[t] - first || (retried != 0 && retried != 1))
                GF2_FAIL(GF2_E_ARG, "%s: the regions of block type %lld do not partition its %lld locations in order: region %lld is "
                         "(first %lld, count %lld, retried %lld) where location %lld is next", who, (long long)t, (long long)type_locations[t],
                         (long long)r, (long long)first, (long long)count, (long long)retried, (long long)next);
            next = first + count;
            uint64_t mask = 0;
            const uint64_t* e = type_eff + (size_t)(plan->type_offset[(size_t)t] + first) * 6;
            for (int64_t l = 0; l < count; ++l) mask |= e[6 * l + 2] | e[6 * l + 5];
            if (!retried && mask)
                GF2_FAIL(GF2_E_ARG, "%s: region %lld of block type %lld (locations %lld .. %lld) is not retried but its locations set a flag bit", who,
                         (long long)r, (long long)t, (long long)first, (long long)next - 1);
            for (int64_t q = retry->type_first[(size_t)t]; q < at; ++q)
                if (masks[(size_t)q] & mask)
                    GF2_FAIL(GF2_E_ARG, "%s: the flag masks of regions %lld and %lld of block type %lld intersect: a flag row must depend on one "
                             "region only", who, (long long)(q - retry->type_first[(size_t)t]), (long long)r, (long long)t);
            masks[(size_t)at] = mask;
            retry->first[(size_t)at] = (int32_t)first;
            retry->count[(size_t)at] = (int32_t)count;
            retry->retried[(size_t)at] = (int32_t)retried;
            if (count > 512) note_size(512);
            note_size((int32_t)(count - (count - 1) / 512 * 512));
        }
        if (next != type_locations[t])
            GF2_FAIL(GF2_E_ARG, "%s: the regions of block type %lld do not partition its %lld locations in order: they end at location %lld", who,
                     (long long)t, (long long)type_locations[t], (long long)next);
    }
    retry->type_first[(size_t)ntypes] = at;
    if (max_attempts < 1 || max_attempts > GF2_RETRY_MAX_ATTEMPTS)
        GF2_FAIL(GF2_E_ARG, "%s: needs 1 <= max_attempts <= %d, got %lld", who, GF2_RETRY_MAX_ATTEMPTS, (long long)max_attempts);
    if (sizes.size() > (size_t)GF2_RETRY_MAX_SIZES)
        GF2_FAIL(GF2_E_ARG, "%s: the regions have more than GF2_RETRY_MAX_SIZES = %d distinct segment sizes, one inverse-CDF table each", who,
                 GF2_RETRY_MAX_SIZES);
    std::sort(sizes.begin(), sizes.end());
    retry->sizes = sizes;
    retry->full_size = !sizes.empty() && sizes.back() == 512 ? (int32_t)sizes.size() - 1 : -1;
    for (int64_t q = 0; q < total; ++q) {
        const int32_t nb = retry->count[(size_t)q] - (retry->count[(size_t)q] - 1) / 512 * 512;
        retry->last_size[(size_t)q] = (int32_t)(std::find(sizes.begin(), sizes.end(), nb) - sizes.begin());
    }
    retry->regions = retry->preparations = 0;
    for (int64_t b = 0; b < nblocks; ++b) {
        if (block_kind[b] == GF2_STREAM_FINAL) continue;
        const int64_t t = block_type[b];
        retry->regions += type_nregions[t];
        for (int64_t q = retry->type_first[(size_t)t]; q < retry->type_first[(size_t)t + 1]; ++q) retry->preparations += retry->retried[(size_t)q];
    }
    return GF2_OK;
}

int gf2_retry_check_range(const char* who, double p_x, double p_y, double p_z, int64_t first_sample, int64_t count) {
    if (count < 0 || first_sample < 0) GF2_FAIL(GF2_E_ARG, "%s: negative range", who);
    if (!(p_x >= 0.0) || !(p_y >= 0.0) || !(p_z >= 0.0) || p_x + p_y + p_z > 1.0 + 1e-12)
        GF2_FAIL(GF2_E_ARG, "probabilities must be non-negative and sum to at most 1");
    return GF2_OK;
}

// ---- ... with waiting faults on the data block (include/gf2hip.h, DESIGN.md section 5d "Repeat-until-success with waiting faults") ----
#include "gf2_retry_wait_plan.h"

int gf2_retry_wait_plan(const char* who, const uint64_t* type_eff, const int64_t* type_locations, const int64_t* type_flags, int64_t ntypes,
                        const int32_t* block_type, const int32_t* block_kind, int64_t nblocks, const int64_t* type_regions,
                        const int64_t* type_nregions, const uint64_t* wait_eff, const int64_t* wait_count, int64_t max_attempts,
                        StreamPlan* plan, RetryPlan* retry, RetryWaitPlan* wait) {
    if (int rc = gf2_retry_plan(who, type_eff, type_locations, type_flags, ntypes, block_type, block_kind, nblocks, type_regions, type_nregions,
                                max_attempts, plan, retry))
        return rc;
    return gf2_retry_wait_rules(who, ntypes, block_type, block_kind, nblocks, wait_eff, wait_count, GF2_RETRY_MAX_SIZES, "GF2_RETRY_MAX_SIZES", plan,
                                *retry, wait);
}

int gf2_retry_wait_rules(const char* who, int64_t ntypes, const int32_t* block_type, const int32_t* block_kind, int64_t nblocks,
                         const uint64_t* wait_eff, const int64_t* wait_count, int max_sizes, const char* max_sizes_name, StreamPlan* plan,
                         const RetryPlan& retried, RetryWaitPlan* wait) {
    const RetryPlan* const retry = &retried;
    if (!wait_count || !wait) GF2_FAIL(GF2_E_ARG, "%s: null argument", who);
    const int64_t total = retry->type_first[(size_t)ntypes];
    std::vector<int32_t> sizes;                                                  // a set of at most max_sizes + 1 values
    try {
        wait->first.assign((size_t)total, 0);
        wait->count.assign((size_t)total, 0);
        wait->size.assign((size_t)total, -1);
        sizes.reserve((size_t)max_sizes + 1);
    } catch (const std::bad_alloc&) {
        GF2_FAIL(GF2_E_NOMEM, "%s: out of host memory", who);
    }
    int64_t rows = 0;
    for (int64_t t = 0; t < ntypes; ++t)
        for (int64_t q = retry->type_first[(size_t)t]; q < retry->type_first[(size_t)t + 1]; ++q) {
            const int64_t r = q - retry->type_first[(size_t)t], w = wait_count[q];
            if (w < 0 || w > GF2_RETRY_WAIT_MAX_ROWS)
                GF2_FAIL(GF2_E_ARG, "%s: region %lld of block type %lld has %lld wait rows, a region holds 0 <= wait rows <= %d (one segment)", who,
                         (long long)r, (long long)t, (long long)w, GF2_RETRY_WAIT_MAX_ROWS);
            if (w > 0 && !retry->retried[(size_t)q])
                GF2_FAIL(GF2_E_ARG, "%s: region %lld of block type %lld is not retried but has %lld wait rows", who, (long long)r, (long long)t,
                         (long long)w);
            wait->first[(size_t)q] = rows;
            wait->count[(size_t)q] = (int32_t)w;
            rows += w;
            if (w > 0 && std::find(sizes.begin(), sizes.end(), (int32_t)w) == sizes.end() && sizes.size() <= (size_t)max_sizes)
                sizes.push_back((int32_t)w);
        }
    if (sizes.size() > (size_t)max_sizes)
        GF2_FAIL(GF2_E_ARG, "%s: the regions have more than %s = %d distinct wait sizes, one inverse-CDF table each", who, max_sizes_name,
                 max_sizes);
    if (rows > 0 && !wait_eff) GF2_FAIL(GF2_E_ARG, "%s: null argument", who);
    std::sort(sizes.begin(), sizes.end());
    wait->sizes = sizes;
    wait->rows = rows;
    for (int64_t q = 0; q < total; ++q)
        if (wait->count[(size_t)q] > 0)
            wait->size[(size_t)q] = (int32_t)(std::find(sizes.begin(), sizes.end(), wait->count[(size_t)q]) - sizes.begin());
    wait->locations = 0;
    for (int64_t b = 0; b < nblocks; ++b) {                                      // the wait rows act on their block's local and tail words
        if (block_kind[b] == GF2_STREAM_FINAL) continue;
        const int64_t t = block_type[b];
        for (int64_t q = retry->type_first[(size_t)t]; q < retry->type_first[(size_t)t + 1]; ++q) {
            wait->locations += wait->count[(size_t)q];
            const uint64_t* e = wait_eff + (size_t)wait->first[(size_t)q] * 4;
            for (int64_t l = 0; l < wait->count[(size_t)q]; ++l) {
                plan->any_local[block_kind[b]] |= e[4 * l] | e[4 * l + 2];
                plan->any_tail |= e[4 * l + 1] | e[4 * l + 3];
            }
        }
    }
    return GF2_OK;
}

int gf2_retry_wait_check_rates(const char* who, double q_x, double q_y, double q_z) {
    if (!(q_x >= 0.0) || !(q_y >= 0.0) || !(q_z >= 0.0) || q_x + q_y + q_z > 1.0 + 1e-12)
        GF2_FAIL(GF2_E_ARG, "%s: the waiting probabilities must be non-negative and sum to at most 1", who);
    return GF2_OK;
}

namespace {
// One sampler segment of nb rows under the draw d: K from the inverse-CDF table, the picks by Floyd's rule, their kinds by (t_1, t_2);
// every pick XORs its row's X and / or Z component, `width` words each, into acc.  Returns K.
int retry_segment_host(uint64_t d, int nb, const uint64_t* table, uint64_t t_1, uint64_t t_2, const uint64_t* rows, int width, uint64_t* acc) {
    const uint64_t golden = 0x9E3779B97F4A7C15ull;
    const uint64_t u = d >> 32;
    int K = 0;
    while (K < nb && u >= table[K]) K += 1;
    uint64_t taken[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    for (int k = 0; k < K; ++k) {
        const uint64_t v = host_mix64(d + golden * (uint64_t)(k + 1));
        const uint64_t j = (uint64_t)(nb - K + k);
        const uint64_t pick = ((v >> 32) * (j + 1)) >> 32;                       // Floyd: a candidate in [0, j]
        const uint64_t pos = ((taken[pick >> 6] >> (pick & 63)) & 1ull) ? j : pick;
        taken[pos >> 6] |= 1ull << (pos & 63);
        const uint64_t c = v & 0xFFFFFFFFull;
        const int kind = (c < t_2 ? 1 : 0) | (c >= t_1 ? 2 : 0);
        const uint64_t* e = rows + (size_t)pos * 2 * width;
        for (int comp = 0; comp < 2; ++comp)
            if (kind >> comp & 1)
                for (int q = 0; q < width; ++q) acc[q] ^= e[width * comp + q];
    }
    return K;
}

struct RetryWaitDraw {                                                           // the waiting faults of a call
    const RetryWaitPlan* plan;
    const uint64_t* eff;
    double q_x, q_y, q_z;
};

// The definition of gf2_retry_outcomes_dev's words (DESIGN.md section 5d "Repeat-until-success"), serial: the blocks in order, the
// regions of a block in order, a retried region redrawn under the key of (region, attempt) until its flags are zero.  The draw of a
// segment is gf2_gate_outcomes_host's with the location sampler's kinds; the block rule is gf2_stream_words_host's.  With `waits`
// (gf2_retry_wait_outcomes_dev's words, "Repeat-until-success with waiting faults") every attempt made of a region with wait rows
// also draws that region's waiting faults, under a key of its own, into the block's local and tail words, which no retry clears;
// a sample then has one word more, the waiting faults it drew.
int retry_walk_host(const char* who, const StreamPlan& plan, const RetryPlan& retry, const RetryWaitDraw* waits, const uint64_t* type_eff,
                    const int32_t* block_type, const int32_t* block_kind, int64_t nblocks, uint64_t seed, int64_t first_sample, int64_t count,
                    double p_x, double p_y, double p_z, int64_t max_attempts, uint64_t* words_out, int64_t ldw, uint32_t* attempts_out) {
    const int64_t ldr = plan.nsteps + plan.flag_words + (waits ? 2 : 1);
    if (ldw < ldr)
        GF2_FAIL(GF2_E_ARG, "%s: ldw must be at least the sequence's nsteps + F + %d = %lld words", who, waits ? 2 : 1, (long long)ldr);
    if (count == 0) return GF2_OK;
    if (!words_out) GF2_FAIL(GF2_E_ARG, "%s: null buffer", who);
    const uint64_t golden = 0x9E3779B97F4A7C15ull, stream = 0xD1B54A32D192ED03ull;
    const int SEG = 512;
    const double p_t = p_x + p_y + p_z, p_xy = p_x + p_y;
    const uint64_t t_any = host_quantise(p_t), t_1 = p_t > 0.0 ? host_quantise(p_x / p_t) : 0, t_2 = p_t > 0.0 ? host_quantise(p_xy / p_t) : 0;
    const double q_t = waits ? waits->q_x + waits->q_y + waits->q_z : 0.0;
    const uint64_t w_any = host_quantise(q_t), w_1 = q_t > 0.0 ? host_quantise(waits->q_x / q_t) : 0,
                   w_2 = q_t > 0.0 ? host_quantise((waits->q_x + waits->q_y) / q_t) : 0;
    const size_t wait_sizes = waits ? waits->plan->sizes.size() : 0;
    std::vector<uint64_t> cdf, wait_cdf;                                         // [size][SEG + 1]
    try {
        cdf.resize(retry.sizes.size() * (SEG + 1));
        wait_cdf.resize(wait_sizes * (SEG + 1));
    } catch (const std::bad_alloc&) {
        GF2_FAIL(GF2_E_NOMEM, "%s: out of host memory", who);
    }
    for (size_t k = 0; k < retry.sizes.size(); ++k) host_binomial_cdf_table(t_any, retry.sizes[k], &cdf[k * (SEG + 1)]);
    for (size_t k = 0; k < wait_sizes; ++k) host_binomial_cdf_table(w_any, waits->plan->sizes[k], &wait_cdf[k * (SEG + 1)]);
    for (int64_t i = 0; i < count; ++i) {
        uint64_t* const out = words_out + i * ldw;
        for (int64_t q = 0; q < ldr; ++q) out[q] = 0;
        uint32_t* const tries = attempts_out ? attempts_out + i * retry.preparations : nullptr;
        for (int64_t q = 0; tries && q < retry.preparations; ++q) tries[q] = 0;
        const uint64_t ks = host_mix64(seed + golden * ((uint64_t)(first_sample + i) + 1));
        uint64_t T = 0, attempts = 0, wait_faults = 0;
        int64_t g = 0, prep = 0;
        bool exhausted = false;
        for (int64_t b = 0; b < nblocks && !exhausted; ++b) {
            uint64_t local = 0, tail = 0;
            if (block_kind[b] != GF2_STREAM_FINAL) {
                const int64_t t = block_type[b];
                for (int64_t r = retry.type_first[(size_t)t]; r < retry.type_first[(size_t)t + 1] && !exhausted; ++r, ++g) {
                    const int64_t rows = plan.type_offset[(size_t)t] + retry.first[(size_t)r], m = retry.count[(size_t)r];
                    const int64_t nseg = (m + SEG - 1) / SEG, limit = retry.retried[(size_t)r] ? max_attempts : 1;
                    const uint64_t kr = host_mix64(ks + stream * (GF2_RETRY_SLOT_BASE + (uint64_t)g + 1));
                    const int nw = waits ? waits->plan->count[(size_t)r] : 0;
                    const uint64_t kw = host_mix64(ks + stream * (GF2_RETRY_WAIT_SLOT_BASE + (uint64_t)g + 1));
                    uint64_t acc[3] = {0, 0, 0}, waited[2] = {0, 0};
                    int64_t a = 0;
                    do {
                        const uint64_t ka = host_mix64(kr + golden * ((uint64_t)a + 1));
                        acc[0] = acc[1] = acc[2] = 0;
                        for (int64_t s = 0; s < nseg; ++s) {
                            const bool last = s == nseg - 1;
                            const int nb = last ? (int)(m - SEG * s) : SEG;
                            const uint64_t* table = &cdf[(size_t)(last ? retry.last_size[(size_t)r] : retry.full_size) * (SEG + 1)];
                            (void)retry_segment_host(host_mix64(ka + stream * ((uint64_t)s + 1)), nb, table, t_1, t_2, type_eff + (size_t)(rows + SEG * s) * 6,
                                                     3, acc);
                        }
                        if (nw > 0) {                                            // the data waits through this attempt, passed or not
                            const uint64_t kwa = host_mix64(kw + golden * ((uint64_t)a + 1));
                            wait_faults += (uint64_t)retry_segment_host(host_mix64(kwa + stream), nw,
                                                                        &wait_cdf[(size_t)waits->plan->size[(size_t)r] * (SEG + 1)], w_1, w_2,
                                                                        waits->eff + (size_t)waits->plan->first[(size_t)r] * 4, 2, waited);
                        }
                        a += 1;
                    } while (acc[2] != 0 && a < limit);
                    if (retry.retried[(size_t)r]) {
                        attempts += (uint64_t)a;
                        if (tries) tries[prep] = (uint32_t)a;
                        prep += 1;
                    }
                    if (acc[2] != 0) {                                           // no attempt passed: the walk stops here
                        exhausted = true;
                        const int64_t row = plan.flag[(size_t)b];
                        out[plan.nsteps + (row >> 6)] |= acc[2] << (row & 63);
                        if ((row & 63) && (acc[2] >> (64 - (row & 63)))) out[plan.nsteps + (row >> 6) + 1] |= acc[2] >> (64 - (row & 63));
                    }
                    local ^= acc[0] ^ waited[0], tail ^= acc[1] ^ waited[1];
                }
            }
            if (exhausted) break;
            if (plan.step[(size_t)b] >= 0) out[plan.step[(size_t)b]] = (T & gf2_stream_frame_mask(block_kind[b])) ^ local;
            T ^= tail;
        }
        out[plan.nsteps + plan.flag_words] = attempts;
        if (waits) out[plan.nsteps + plan.flag_words + 1] = wait_faults;
    }
    return GF2_OK;
}
}  // namespace

extern "C" {

int gf2_retry_words_host(const uint64_t* type_eff, const int64_t* type_locations, const int64_t* type_flags, int64_t ntypes,
                         const int32_t* block_type, const int32_t* block_kind, int64_t nblocks, const int64_t* type_regions,
                         const int64_t* type_nregions, uint64_t seed, int64_t first_sample, int64_t count, double p_x, double p_y, double p_z,
                         int64_t max_attempts, uint64_t* words_out, int64_t ldw, uint32_t* attempts_out) {
    const char* who = "gf2_retry_words_host";
    StreamPlan plan;
    RetryPlan retry;
    if (int rc = gf2_retry_plan(who, type_eff, type_locations, type_flags, ntypes, block_type, block_kind, nblocks, type_regions, type_nregions,
                                max_attempts, &plan, &retry))
        return rc;
    if (int rc = gf2_retry_check_range(who, p_x, p_y, p_z, first_sample, count)) return rc;
    return retry_walk_host(who, plan, retry, nullptr, type_eff, block_type, block_kind, nblocks, seed, first_sample, count, p_x, p_y, p_z, max_attempts,
                           words_out, ldw, attempts_out);
}

int gf2_retry_wait_words_host(const uint64_t* type_eff, const int64_t* type_locations, const int64_t* type_flags, int64_t ntypes,
                              const int32_t* block_type, const int32_t* block_kind, int64_t nblocks, const int64_t* type_regions,
                              const int64_t* type_nregions, const uint64_t* wait_eff, const int64_t* wait_count, uint64_t seed,
                              int64_t first_sample, int64_t count, double p_x, double p_y, double p_z, double q_x, double q_y, double q_z,
                              int64_t max_attempts, uint64_t* words_out, int64_t ldw, uint32_t* attempts_out) {
    const char* who = "gf2_retry_wait_words_host";
    StreamPlan plan;
    RetryPlan retry;
    RetryWaitPlan wait;
    if (int rc = gf2_retry_wait_plan(who, type_eff, type_locations, type_flags, ntypes, block_type, block_kind, nblocks, type_regions, type_nregions,
                                     wait_eff, wait_count, max_attempts, &plan, &retry, &wait))
        return rc;
    if (int rc = gf2_retry_check_range(who, p_x, p_y, p_z, first_sample, count)) return rc;
    if (int rc = gf2_retry_wait_check_rates(who, q_x, q_y, q_z)) return rc;
    const RetryWaitDraw waits = {&wait, wait_eff, q_x, q_y, q_z};
    return retry_walk_host(who, plan, retry, &waits, type_eff, block_type, block_kind, nblocks, seed, first_sample, count, p_x, p_y, p_z, max_attempts,
                           words_out, ldw, attempts_out);
}

}  // extern "C"

// ---- repeat-until-success of multi-block programs (include/gf2hip.h) --------------------------------------
#include "gf2_mretry_plan.h"

int gf2_mretry_plan(const char* who, const uint64_t* type_eff, const int64_t* type_locations, const int64_t* type_flags, int64_t ntypes,
                    const int32_t* block_type, const int32_t* block_kind, const int32_t* block_a, const int32_t* block_b, int64_t nblocks,
                    int64_t nframes, const int64_t* type_regions, const int64_t* type_nregions, int64_t max_attempts, MStreamPlan* plan,
                    RetryPlan* retry) {
    if (int rc = gf2_mstream_plan(who, type_eff, type_locations, type_flags, ntypes, block_type, block_kind, block_a, block_b, nblocks, nframes, plan))
        return rc;
    if (int rc = gf2_retry_region_rules(who, type_eff, type_locations, ntypes, block_type, block_kind, nblocks, type_regions, type_nregions,
                                        max_attempts, plan->seq, retry))
        return rc;
    for (int64_t b = 0; b < nblocks; ++b) {
        if (block_kind[b] != GF2_MSTREAM_CNOT) continue;
        const int64_t t = block_type[b], q = retry->type_first[(size_t)t];
        if (type_nregions[t] != 1 || retry->retried[(size_t)q])
            GF2_FAIL(GF2_E_ARG, "%s: the type of CNOT block %lld has %lld regions, the first retried %d: a CNOT block has no flag rows, its type is one "
                     "region that is not retried", who, (long long)b, (long long)type_nregions[t], (int)retry->retried[(size_t)q]);
    }
    return GF2_OK;
}

extern "C" {

// The definition of gf2_mretry_outcomes_dev's words (DESIGN.md section 5d "Repeat-until-success of multi-block programs"), serial:
// retry_walk_host's draw per (region, attempt) with gf2_mstream_words_host's closing of a block.
int gf2_mretry_words_host(const uint64_t* type_eff, const int64_t* type_locations, const int64_t* type_flags, int64_t ntypes,
                          const int32_t* block_type, const int32_t* block_kind, const int32_t* block_a, const int32_t* block_b, int64_t nblocks,
                          int64_t nframes, const int64_t* type_regions, const int64_t* type_nregions, uint64_t seed, int64_t first_sample,
                          int64_t count, double p_x, double p_y, double p_z, int64_t max_attempts, uint64_t* words_out, int64_t ldw,
                          uint32_t* attempts_out) {
    const char* who = "gf2_mretry_words_host";
    MStreamPlan mplan;
    RetryPlan retry;
    if (int rc = gf2_mretry_plan(who, type_eff, type_locations, type_flags, ntypes, block_type, block_kind, block_a, block_b, nblocks, nframes,
                                 type_regions, type_nregions, max_attempts, &mplan, &retry))
        return rc;
    if (int rc = gf2_retry_check_range(who, p_x, p_y, p_z, first_sample, count)) return rc;
    const StreamPlan& plan = mplan.seq;
    const int64_t ldr = plan.nsteps + plan.flag_words + 1;
    if (ldw < ldr) GF2_FAIL(GF2_E_ARG, "%s: ldw must be at least the sequence's nsteps + F + 1 = %lld words", who, (long long)ldr);
    if (count == 0) return GF2_OK;
    if (!words_out) GF2_FAIL(GF2_E_ARG, "%s: null buffer", who);
    const uint64_t golden = 0x9E3779B97F4A7C15ull, stream = 0xD1B54A32D192ED03ull;
    const int SEG = 512;
    const double p_t = p_x + p_y + p_z, p_xy = p_x + p_y;
    const uint64_t t_any = host_quantise(p_t), t_1 = p_t > 0.0 ? host_quantise(p_x / p_t) : 0, t_2 = p_t > 0.0 ? host_quantise(p_xy / p_t) : 0;
    std::vector<uint64_t> cdf;                                                   // [size][SEG + 1]
    try {
        cdf.resize(retry.sizes.size() * (SEG + 1));
    } catch (const std::bad_alloc&) {
        GF2_FAIL(GF2_E_NOMEM, "%s: out of host memory", who);
    }
    for (size_t k = 0; k < retry.sizes.size(); ++k) host_binomial_cdf_table(t_any, retry.sizes[k], &cdf[k * (SEG + 1)]);
    for (int64_t i = 0; i < count; ++i) {
        uint64_t* const out = words_out + i * ldw;
        for (int64_t q = 0; q < ldr; ++q) out[q] = 0;
        uint32_t* const tries = attempts_out ? attempts_out + i * retry.preparations : nullptr;
        for (int64_t q = 0; tries && q < retry.preparations; ++q) tries[q] = 0;
        const uint64_t ks = host_mix64(seed + golden * ((uint64_t)(first_sample + i) + 1));
        uint64_t T[GF2_MSTREAM_MAX_FRAMES] = {0, 0, 0, 0}, attempts = 0;
        int64_t g = 0, prep = 0;
        bool exhausted = false;
        for (int64_t b = 0; b < nblocks && !exhausted; ++b) {
            const int64_t t = block_type[b];
            uint64_t first = 0, second = 0;                                      // local and tail; a CNOT block's: tail for a, tail for b
            for (int64_t r = retry.type_first[(size_t)t]; r < retry.type_first[(size_t)t + 1] && !exhausted; ++r, ++g) {
                const int64_t rows = plan.type_offset[(size_t)t] + retry.first[(size_t)r], m = retry.count[(size_t)r];
                const int64_t nseg = (m + SEG - 1) / SEG, limit = retry.retried[(size_t)r] ? max_attempts : 1;
                const uint64_t kr = host_mix64(ks + stream * (GF2_RETRY_SLOT_BASE + (uint64_t)g + 1));
                uint64_t acc[3] = {0, 0, 0};
                int64_t a = 0;
                do {
                    const uint64_t ka = host_mix64(kr + golden * ((uint64_t)a + 1));
                    acc[0] = acc[1] = acc[2] = 0;
                    for (int64_t s = 0; s < nseg; ++s) {
                        const bool last = s == nseg - 1;
                        const int nb = last ? (int)(m - SEG * s) : SEG;
                        const uint64_t* table = &cdf[(size_t)(last ? retry.last_size[(size_t)r] : retry.full_size) * (SEG + 1)];
                        (void)retry_segment_host(host_mix64(ka + stream * ((uint64_t)s + 1)), nb, table, t_1, t_2, type_eff + (size_t)(rows + SEG * s) * 6, 3,
                                                 acc);
                    }
                    a += 1;
                } while (acc[2] != 0 && a < limit);
                if (retry.retried[(size_t)r]) {
                    attempts += (uint64_t)a;
                    if (tries) tries[prep] = (uint32_t)a;
                    prep += 1;
                }
                if (acc[2] != 0) {                                               // no attempt passed: the walk stops here
                    exhausted = true;
                    const int64_t row = plan.flag[(size_t)b];
                    out[plan.nsteps + (row >> 6)] |= acc[2] << (row & 63);
                    if ((row & 63) && (acc[2] >> (64 - (row & 63)))) out[plan.nsteps + (row >> 6) + 1] |= acc[2] >> (64 - (row & 63));
                }
                first ^= acc[0], second ^= acc[1];
            }
            if (exhausted) break;
            uint64_t& Ta = T[block_a[b]];
            if (block_kind[b] == GF2_MSTREAM_CNOT) {
                uint64_t& Tb = T[block_b[b]];
                gf2_mstream_cnot_map(&Ta, &Tb);
                Ta ^= first, Tb ^= second;
            } else {
                if (plan.step[(size_t)b] >= 0) out[plan.step[(size_t)b]] = (Ta & gf2_stream_frame_mask(block_kind[b])) ^ first;
                Ta ^= second;
            }
        }
        out[plan.nsteps + plan.flag_words] = attempts;
    }
    return GF2_OK;
}

}  // extern "C"

// ---- repeat-until-success under gate-level faults (include/gf2hip.h) -------------------------------------
#include "gf2_retry_gate_plan.h"

int gf2_retry_gate_plan(const char* who, const uint64_t* type_eff, const int64_t* type_locations, const int64_t* type_flags, int64_t ntypes,
                        const int32_t* block_type, const int32_t* block_kind, int64_t nblocks, const int64_t* type_regions,
                        const int64_t* type_nregions, const int32_t* site_loc, const int64_t* site_regions, int64_t max_attempts,
                        StreamPlan* plan, RetryPlan* retry, RetryGatePlan* gate) {
    if (int rc = gf2_retry_plan(who, type_eff, type_locations, type_flags, ntypes, block_type, block_kind, nblocks, type_regions, type_nregions,
                                max_attempts, plan, retry))
        return rc;
    return gf2_retry_gate_site_rules(who, type_locations, ntypes, site_loc, site_regions, *retry, gate);
}

int gf2_retry_gate_site_rules(const char* who, const int64_t* type_locations, int64_t ntypes, const int32_t* site_loc, const int64_t* site_regions,
                              const RetryPlan& checked, RetryGatePlan* gate) {
    const RetryPlan* const retry = &checked;
    if (!site_loc || !site_regions || !gate) GF2_FAIL(GF2_E_ARG, "%s: null argument", who);
    const int64_t total = retry->type_first[(size_t)ntypes];
    std::vector<uint8_t> seen;
    std::vector<int32_t> sizes[2];                                               // sets of at most GF2_RETRY_MAX_SIZES + 1 values
    try {
        gate->site_first.assign((size_t)total, 0);
        for (int c = 0; c < 2; ++c) {
            gate->n[c].assign((size_t)total, 0);
            gate->last_size[c].assign((size_t)total, -1);
            sizes[c].reserve(GF2_RETRY_MAX_SIZES + 1);
        }
        int64_t most = 0;
        for (int64_t t = 0; t < ntypes; ++t) most = type_locations[t] > most ? type_locations[t] : most;
        seen.assign((size_t)most, 0);
    } catch (const std::bad_alloc&) {
        GF2_FAIL(GF2_E_NOMEM, "%s: out of host memory", who);
    }
    auto note_size = [&](int c, int32_t nb) {
        if (std::find(sizes[c].begin(), sizes[c].end(), nb) == sizes[c].end() && sizes[c].size() <= (size_t)GF2_RETRY_MAX_SIZES) sizes[c].push_back(nb);
    };
    int64_t at = 0;                                                              // the next site of site_loc
    for (int64_t t = 0; t < ntypes; ++t) {
        for (int64_t q = retry->type_first[(size_t)t]; q < retry->type_first[(size_t)t + 1]; ++q) {
            const int64_t r = q - retry->type_first[(size_t)t], first = retry->first[(size_t)q], count = retry->count[(size_t)q];
            const int64_t n1 = site_regions[2 * q], n2 = site_regions[2 * q + 1];
            if (n1 < 0 || n2 < 0 || n2 > count || n1 + 2 * n2 != count)
                GF2_FAIL(GF2_E_ARG, "%s: region %lld of block type %lld has n_1 + 2 n_2 = %lld + 2 * %lld sites' locations, not its %lld locations", who,
                         (long long)r, (long long)t, (long long)n1, (long long)n2, (long long)count);
            gate->site_first[(size_t)q] = at;
            gate->n[0][(size_t)q] = (int32_t)n1;
            gate->n[1][(size_t)q] = (int32_t)n2;
            for (int64_t l = 0; l < count; ++l) seen[(size_t)(first + l)] = 0;
            for (int c = 0; c < 2; ++c) {
                const int64_t m = c ? n2 : n1, width = c + 1;
                for (int64_t s = 0; s < m; ++s, ++at) {
                    const int64_t l = site_loc[at];
                    if (l < first || l + width > first + count || seen[(size_t)l] || seen[(size_t)(l + width - 1)])
                        GF2_FAIL(GF2_E_ARG, "%s: the sites of region %lld of block type %lld do not partition its locations %lld .. %lld: %s site %lld at "
                                 "location %lld", who, (long long)r, (long long)t, (long long)first, (long long)(first + count - 1),
                                 c ? "CNOT" : "one-operand", (long long)s, (long long)l);
                    if (s > 0 && l <= site_loc[at - 1])
                        GF2_FAIL(GF2_E_ARG, "%s: the %s sites of region %lld of block type %lld are not ascending: site %lld at location %lld follows "
                                 "location %lld", who, c ? "CNOT" : "one-operand", (long long)r, (long long)t, (long long)s, (long long)l,
                                 (long long)site_loc[at - 1]);
                    seen[(size_t)l] = seen[(size_t)(l + width - 1)] = 1;
                }
                if (m > 512) note_size(c, 512);
                if (m > 0) note_size(c, (int32_t)(m - (m - 1) / 512 * 512));
            }                                                                     // (n_1 + 2 n_2 = count disjoint locations inside the region: a partition)
        }
    }
    gate->sites = at;
    for (int c = 0; c < 2; ++c) {
        if (sizes[c].size() > (size_t)GF2_RETRY_MAX_SIZES)
            GF2_FAIL(GF2_E_ARG, "%s: the %s sites of the regions have more than GF2_RETRY_MAX_SIZES = %d distinct segment sizes, one inverse-CDF table "
                     "each", who, c ? "CNOT" : "one-operand", GF2_RETRY_MAX_SIZES);
        std::sort(sizes[c].begin(), sizes[c].end());
        gate->sizes[c] = sizes[c];
        gate->full_size[c] = !sizes[c].empty() && sizes[c].back() == 512 ? (int32_t)sizes[c].size() - 1 : -1;
        for (int64_t q = 0; q < total; ++q) {
            const int32_t m = gate->n[c][(size_t)q];
            if (m > 0) gate->last_size[c][(size_t)q] = (int32_t)(std::find(sizes[c].begin(), sizes[c].end(), m - (m - 1) / 512 * 512) - sizes[c].begin());
        }
    }
    return GF2_OK;
}

// ... and with waiting faults on the data block ("Repeat-until-success with waiting faults under gate-level faults")
#include "gf2_retry_gate_wait_plan.h"

int gf2_retry_gate_wait_plan(const char* who, const uint64_t* type_eff, const int64_t* type_locations, const int64_t* type_flags, int64_t ntypes,
                             const int32_t* block_type, const int32_t* block_kind, int64_t nblocks, const int64_t* type_regions,
                             const int64_t* type_nregions, const int32_t* site_loc, const int64_t* site_regions, const uint64_t* wait_eff,
                             const int64_t* wait_count, int64_t max_attempts, StreamPlan* plan, RetryPlan* retry, RetryGatePlan* gate,
                             RetryWaitPlan* wait) {
    if (int rc = gf2_retry_gate_plan(who, type_eff, type_locations, type_flags, ntypes, block_type, block_kind, nblocks, type_regions, type_nregions,
                                     site_loc, site_regions, max_attempts, plan, retry, gate))
        return rc;
    return gf2_retry_wait_rules(who, ntypes, block_type, block_kind, nblocks, wait_eff, wait_count, GF2_RETRY_GATE_WAIT_MAX_SIZES,
                                "GF2_RETRY_GATE_WAIT_MAX_SIZES", plan, *retry, wait);
}

namespace {
// The inverse-CDF tables of a call's two classes, [size][512 + 1] per class ...
struct RetryGateTables {
    std::vector<uint64_t> cdf[2];
    int make(const char* who, const RetryGatePlan& gate, double p1, double p2) {
        const uint64_t T[2] = {host_quantise(p1), host_quantise(p2)};
        try {
            for (int cl = 0; cl < 2; ++cl) cdf[cl].resize(gate.sizes[cl].size() * (512 + 1));
        } catch (const std::bad_alloc&) {
            GF2_FAIL(GF2_E_NOMEM, "%s: out of host memory", who);
        }
        for (int cl = 0; cl < 2; ++cl)
            for (size_t k = 0; k < gate.sizes[cl].size(); ++k) host_binomial_cdf_table(T[cl], gate.sizes[cl][k], &cdf[cl][k * (512 + 1)]);
        return GF2_OK;
    }
};

// ... and the draw of one attempt of region r (RetryPlan's numbering) under its key ka, XOR-ed into acc = (local, tail, flags): the
// region's one-operand sites, then its CNOT sites, as gf2_gate_outcomes_host draws a sample's.  `rows` is the table of the region's
// type: sites are type-local.  Shared by the one-qubit walk below and gf2_mretry_gate_words_host.
void retry_gate_attempt_host(const RetryGatePlan& gate, const RetryGateTables& tables, const uint64_t* rows, const int32_t* site_loc, int64_t r,
                             uint64_t ka, uint64_t* acc) {
    const uint64_t golden = 0x9E3779B97F4A7C15ull, stream = 0xD1B54A32D192ED03ull;
    const int SEG = 512;
    const uint64_t radix[2] = {3, 15}, slot_base[2] = {GF2_GATE_MC_SLOT_ONE, GF2_GATE_MC_SLOT_CNOT};
    int64_t site_base = gate.site_first[(size_t)r];
    for (int cl = 0; cl < 2; site_base += gate.n[cl][(size_t)r], ++cl) {
        const int64_t m = gate.n[cl][(size_t)r], nseg = (m + SEG - 1) / SEG;      // (none for an empty class)
        for (int64_t s = 0; s < nseg; ++s) {
            const bool last = s == nseg - 1;
            const int nb = last ? (int)(m - SEG * s) : SEG;
            const uint64_t* table = &tables.cdf[cl][(size_t)(last ? gate.last_size[cl][(size_t)r] : gate.full_size[cl]) * (SEG + 1)];
            const uint64_t d = host_mix64(ka + stream * (slot_base[cl] + (uint64_t)s + 1));
            const uint64_t u = d >> 32;
            int K = 0;
            while (K < nb && u >= table[K]) K += 1;
            uint64_t taken[SEG / 64] = {0, 0, 0, 0, 0, 0, 0, 0};
            for (int k = 0; k < K; ++k) {
                const uint64_t v = host_mix64(d + golden * (uint64_t)(k + 1));
                const uint64_t hi = v >> 32, lo = v & 0xFFFFFFFFull;
                const uint64_t j = (uint64_t)(nb - K + k);
                const uint64_t pick = (hi * (j + 1)) >> 32;          // Floyd: a candidate in [0, j]
                const uint64_t pos = ((taken[pick >> 6] >> (pick & 63)) & 1ull) ? j : pick;
                taken[pos >> 6] |= 1ull << (pos & 63);
                const uint64_t kappa = 1 + ((lo * radix[cl]) >> 32);
                const uint64_t* e = rows + (size_t)site_loc[site_base + SEG * s + (int64_t)pos] * 6;
                for (int bit = 0; bit < 4; ++bit)                     // bits 2, 3: the CNOT's second location
                    if ((kappa >> bit) & 1)
                        for (int q = 0; q < 3; ++q) acc[q] ^= e[3 * bit + q];
            }
        }
    }
}

// The definition of gf2_retry_gate_outcomes_dev's words (DESIGN.md section 5d "Repeat-until-success under gate-level faults"),
// serial: gf2_retry_words_host's walk, an attempt drawn as gf2_gate_outcomes_host draws a sample -- the region's one-operand sites,
// then its CNOT sites, each class with its own slots, rate and radix of kinds -- under the attempt's key.
// With `waits` (gf2_retry_gate_wait_outcomes_dev's words, "Repeat-until-success with waiting faults under gate-level faults") every
// attempt made of a region with wait rows also draws that region's waiting faults as retry_walk_host does, and a sample has one word
// more, the waiting faults it drew.
int retry_gate_walk_host(const char* who, const StreamPlan& plan, const RetryPlan& retry, const RetryGatePlan& gate, const RetryWaitDraw* waits,
                         const uint64_t* type_eff, const int32_t* block_type, const int32_t* block_kind, int64_t nblocks, const int32_t* site_loc,
                         uint64_t seed, int64_t first_sample, int64_t count, double p1, double p2, int64_t max_attempts, uint64_t* words_out,
                         int64_t ldw, uint32_t* attempts_out) {
    const int64_t ldr = plan.nsteps + plan.flag_words + (waits ? 2 : 1);
    if (ldw < ldr)
        GF2_FAIL(GF2_E_ARG, "%s: ldw must be at least the sequence's nsteps + F + %d = %lld words", who, waits ? 2 : 1, (long long)ldr);
    if (count == 0) return GF2_OK;
    if (!words_out) GF2_FAIL(GF2_E_ARG, "%s: null buffer", who);
    const uint64_t golden = 0x9E3779B97F4A7C15ull, stream = 0xD1B54A32D192ED03ull;
    const int SEG = 512;
    const double q_t = waits ? waits->q_x + waits->q_y + waits->q_z : 0.0;
    const uint64_t w_any = host_quantise(q_t), w_1 = q_t > 0.0 ? host_quantise(waits->q_x / q_t) : 0,
                   w_2 = q_t > 0.0 ? host_quantise((waits->q_x + waits->q_y) / q_t) : 0;
    const size_t wait_sizes = waits ? waits->plan->sizes.size() : 0;
    RetryGateTables tables;
    if (int rc = tables.make(who, gate, p1, p2)) return rc;
    std::vector<uint64_t> wait_cdf;                                              // of the wait sizes: [size][SEG + 1]
    try {
        wait_cdf.resize(wait_sizes * (SEG + 1));
    } catch (const std::bad_alloc&) {
        GF2_FAIL(GF2_E_NOMEM, "%s: out of host memory", who);
    }
    for (size_t k = 0; k < wait_sizes; ++k) host_binomial_cdf_table(w_any, waits->plan->sizes[k], &wait_cdf[k * (SEG + 1)]);
    for (int64_t i = 0; i < count; ++i) {
        uint64_t* const out = words_out + i * ldw;
        for (int64_t q = 0; q < ldr; ++q) out[q] = 0;
        uint32_t* const tries = attempts_out ? attempts_out + i * retry.preparations : nullptr;
        for (int64_t q = 0; tries && q < retry.preparations; ++q) tries[q] = 0;
        const uint64_t ks = host_mix64(seed + golden * ((uint64_t)(first_sample + i) + 1));
        uint64_t frame = 0, attempts = 0, wait_faults = 0;
        int64_t g = 0, prep = 0;
        bool exhausted = false;
        for (int64_t b = 0; b < nblocks && !exhausted; ++b) {
            uint64_t local = 0, tail = 0;
            if (block_kind[b] != GF2_STREAM_FINAL) {
                const int64_t t = block_type[b];
                for (int64_t r = retry.type_first[(size_t)t]; r < retry.type_first[(size_t)t + 1] && !exhausted; ++r, ++g) {
                    const int64_t limit = retry.retried[(size_t)r] ? max_attempts : 1;
                    const uint64_t* const rows = type_eff + (size_t)plan.type_offset[(size_t)t] * 6;   // the type's table: sites are type-local
                    const uint64_t kr = host_mix64(ks + stream * (GF2_RETRY_SLOT_BASE + (uint64_t)g + 1));
                    const int nw = waits ? waits->plan->count[(size_t)r] : 0;
                    const uint64_t kw = host_mix64(ks + stream * (GF2_RETRY_WAIT_SLOT_BASE + (uint64_t)g + 1));
                    uint64_t acc[3] = {0, 0, 0}, waited[2] = {0, 0};
                    int64_t a = 0;
                    do {
                        const uint64_t ka = host_mix64(kr + golden * ((uint64_t)a + 1));
                        acc[0] = acc[1] = acc[2] = 0;
                        retry_gate_attempt_host(gate, tables, rows, site_loc, r, ka, acc);
                        if (nw > 0) {                                            // the data waits through this attempt, passed or not
                            const uint64_t kwa = host_mix64(kw + golden * ((uint64_t)a + 1));
                            wait_faults += (uint64_t)retry_segment_host(host_mix64(kwa + stream), nw,
                                                                        &wait_cdf[(size_t)waits->plan->size[(size_t)r] * (SEG + 1)], w_1, w_2,
                                                                        waits->eff + (size_t)waits->plan->first[(size_t)r] * 4, 2, waited);
                        }
                        a += 1;
                    } while (acc[2] != 0 && a < limit);
                    if (retry.retried[(size_t)r]) {
                        attempts += (uint64_t)a;
                        if (tries) tries[prep] = (uint32_t)a;
                        prep += 1;
                    }
                    if (acc[2] != 0) {                                           // no attempt passed: the walk stops here
                        exhausted = true;
                        const int64_t row = plan.flag[(size_t)b];
                        out[plan.nsteps + (row >> 6)] |= acc[2] << (row & 63);
                        if ((row & 63) && (acc[2] >> (64 - (row & 63)))) out[plan.nsteps + (row >> 6) + 1] |= acc[2] >> (64 - (row & 63));
                    }
                    local ^= acc[0] ^ waited[0], tail ^= acc[1] ^ waited[1];
                }
            }
            if (exhausted) break;
            if (plan.step[(size_t)b] >= 0) out[plan.step[(size_t)b]] = (frame & gf2_stream_frame_mask(block_kind[b])) ^ local;
            frame ^= tail;
        }
        out[plan.nsteps + plan.flag_words] = attempts;
        if (waits) out[plan.nsteps + plan.flag_words + 1] = wait_faults;
    }
    return GF2_OK;
}
}  // namespace

extern "C" {

int gf2_retry_gate_words_host(const uint64_t* type_eff, const int64_t* type_locations, const int64_t* type_flags, int64_t ntypes,
                              const int32_t* block_type, const int32_t* block_kind, int64_t nblocks, const int64_t* type_regions,
                              const int64_t* type_nregions, const int32_t* site_loc, const int64_t* site_regions, uint64_t seed,
                              int64_t first_sample, int64_t count, double p1, double p2, int64_t max_attempts, uint64_t* words_out, int64_t ldw,
                              uint32_t* attempts_out) {
    const char* who = "gf2_retry_gate_words_host";
    StreamPlan plan;
    RetryPlan retry;
    RetryGatePlan gate;
    if (int rc = gf2_retry_gate_plan(who, type_eff, type_locations, type_flags, ntypes, block_type, block_kind, nblocks, type_regions, type_nregions,
                                     site_loc, site_regions, max_attempts, &plan, &retry, &gate))
        return rc;
    if (int rc = gf2_gate_check_mc(who, p1, p2, first_sample, count)) return rc;
    return retry_gate_walk_host(who, plan, retry, gate, nullptr, type_eff, block_type, block_kind, nblocks, site_loc, seed, first_sample, count, p1,
                                p2, max_attempts, words_out, ldw, attempts_out);
}

int gf2_retry_gate_wait_words_host(const uint64_t* type_eff, const int64_t* type_locations, const int64_t* type_flags, int64_t ntypes,
                                   const int32_t* block_type, const int32_t* block_kind, int64_t nblocks, const int64_t* type_regions,
                                   const int64_t* type_nregions, const int32_t* site_loc, const int64_t* site_regions, const uint64_t* wait_eff,
                                   const int64_t* wait_count, uint64_t seed, int64_t first_sample, int64_t count, double p1, double p2, double q_x,
                                   double q_y, double q_z, int64_t max_attempts, uint64_t* words_out, int64_t ldw, uint32_t* attempts_out) {
    const char* who = "gf2_retry_gate_wait_words_host";
    StreamPlan plan;
    RetryPlan retry;
    RetryGatePlan gate;
    RetryWaitPlan wait;
    if (int rc = gf2_retry_gate_wait_plan(who, type_eff, type_locations, type_flags, ntypes, block_type, block_kind, nblocks, type_regions,
                                          type_nregions, site_loc, site_regions, wait_eff, wait_count, max_attempts, &plan, &retry, &gate, &wait))
        return rc;
    if (int rc = gf2_gate_check_mc(who, p1, p2, first_sample, count)) return rc;
    if (int rc = gf2_retry_wait_check_rates(who, q_x, q_y, q_z)) return rc;
    const RetryWaitDraw waits = {&wait, wait_eff, q_x, q_y, q_z};
    return retry_gate_walk_host(who, plan, retry, gate, &waits, type_eff, block_type, block_kind, nblocks, site_loc, seed, first_sample, count, p1,
                                p2, max_attempts, words_out, ldw, attempts_out);
}

}  // extern "C"

// ---- repeat-until-success of multi-block programs under gate-level faults (include/gf2hip.h) ---------------
#include "gf2_mretry_gate_plan.h"

int gf2_mretry_gate_plan(const char* who, const uint64_t* type_eff, const int64_t* type_locations, const int64_t* type_flags, int64_t ntypes,
                         const int32_t* block_type, const int32_t* block_kind, const int32_t* block_a, const int32_t* block_b, int64_t nblocks,
                         int64_t nframes, const int64_t* type_regions, const int64_t* type_nregions, const int32_t* site_loc,
                         const int64_t* site_regions, int64_t max_attempts, MStreamPlan* plan, RetryPlan* retry, RetryGatePlan* gate) {
    if (int rc = gf2_mretry_plan(who, type_eff, type_locations, type_flags, ntypes, block_type, block_kind, block_a, block_b, nblocks, nframes,
                                 type_regions, type_nregions, max_attempts, plan, retry))
        return rc;
    if (int rc = gf2_retry_gate_site_rules(who, type_locations, ntypes, site_loc, site_regions, *retry, gate)) return rc;
    for (int64_t b = 0; b < nblocks; ++b) {
        if (block_kind[b] != GF2_MSTREAM_CNOT) continue;
        const int64_t q = retry->type_first[(size_t)block_type[b]];
        if (gate->n[0][(size_t)q] != 0)
            GF2_FAIL(GF2_E_ARG, "%s: the type of CNOT block %lld has %d one-operand sites: every site of a CNOT block is a physical CNOT, its "
                     "control on frame a and its target on frame b", who, (long long)b, (int)gate->n[0][(size_t)q]);
    }
    return GF2_OK;
}

extern "C" {

// The definition of gf2_mretry_gate_outcomes_dev's words (DESIGN.md section 5d "Repeat-until-success of multi-block programs under
// gate-level faults"), serial: gf2_mretry_words_host's walk and closing of a block, an attempt drawn by retry_gate_attempt_host.
int gf2_mretry_gate_words_host(const uint64_t* type_eff, const int64_t* type_locations, const int64_t* type_flags, int64_t ntypes,
                               const int32_t* block_type, const int32_t* block_kind, const int32_t* block_a, const int32_t* block_b,
                               int64_t nblocks, int64_t nframes, const int64_t* type_regions, const int64_t* type_nregions,
                               const int32_t* site_loc, const int64_t* site_regions, uint64_t seed, int64_t first_sample, int64_t count, double p1,
                               double p2, int64_t max_attempts, uint64_t* words_out, int64_t ldw, uint32_t* attempts_out) {
    const char* who = "gf2_mretry_gate_words_host";
    MStreamPlan mplan;
    RetryPlan retry;
    RetryGatePlan gate;
    if (int rc = gf2_mretry_gate_plan(who, type_eff, type_locations, type_flags, ntypes, block_type, block_kind, block_a, block_b, nblocks, nframes,
                                      type_regions, type_nregions, site_loc, site_regions, max_attempts, &mplan, &retry, &gate))
        return rc;
    if (int rc = gf2_gate_check_mc(who, p1, p2, first_sample, count)) return rc;
    const StreamPlan& plan = mplan.seq;
    const int64_t ldr = plan.nsteps + plan.flag_words + 1;
    if (ldw < ldr) GF2_FAIL(GF2_E_ARG, "%s: ldw must be at least the sequence's nsteps + F + 1 = %lld words", who, (long long)ldr);
    if (count == 0) return GF2_OK;
    if (!words_out) GF2_FAIL(GF2_E_ARG, "%s: null buffer", who);
    const uint64_t golden = 0x9E3779B97F4A7C15ull, stream = 0xD1B54A32D192ED03ull;
    RetryGateTables tables;
    if (int rc = tables.make(who, gate, p1, p2)) return rc;
    for (int64_t i = 0; i < count; ++i) {
        uint64_t* const out = words_out + i * ldw;
        for (int64_t q = 0; q < ldr; ++q) out[q] = 0;
        uint32_t* const tries = attempts_out ? attempts_out + i * retry.preparations : nullptr;
        for (int64_t q = 0; tries && q < retry.preparations; ++q) tries[q] = 0;
        const uint64_t ks = host_mix64(seed + golden * ((uint64_t)(first_sample + i) + 1));
        uint64_t T[GF2_MSTREAM_MAX_FRAMES] = {0, 0, 0, 0}, attempts = 0;
        int64_t g = 0, prep = 0;
        bool exhausted = false;
        for (int64_t b = 0; b < nblocks && !exhausted; ++b) {
            const int64_t t = block_type[b];
            const uint64_t* const rows = type_eff + (size_t)plan.type_offset[(size_t)t] * 6;   // the type's table: sites are type-local
            uint64_t first = 0, second = 0;                                      // local and tail; a CNOT block's: tail for a, tail for b
            for (int64_t r = retry.type_first[(size_t)t]; r < retry.type_first[(size_t)t + 1] && !exhausted; ++r, ++g) {
                const int64_t limit = retry.retried[(size_t)r] ? max_attempts : 1;
                const uint64_t kr = host_mix64(ks + stream * (GF2_RETRY_SLOT_BASE + (uint64_t)g + 1));
                uint64_t acc[3] = {0, 0, 0};
                int64_t a = 0;
                do {
                    const uint64_t ka = host_mix64(kr + golden * ((uint64_t)a + 1));
                    acc[0] = acc[1] = acc[2] = 0;
                    retry_gate_attempt_host(gate, tables, rows, site_loc, r, ka, acc);
                    a += 1;
                } while (acc[2] != 0 && a < limit);
                if (retry.retried[(size_t)r]) {
                    attempts += (uint64_t)a;
                    if (tries) tries[prep] = (uint32_t)a;
                    prep += 1;
                }
                if (acc[2] != 0) {                                               // no attempt passed: the walk stops here
                    exhausted = true;
                    const int64_t row = plan.flag[(size_t)b];
                    out[plan.nsteps + (row >> 6)] |= acc[2] << (row & 63);
                    if ((row & 63) && (acc[2] >> (64 - (row & 63)))) out[plan.nsteps + (row >> 6) + 1] |= acc[2] >> (64 - (row & 63));
                }
                first ^= acc[0], second ^= acc[1];
            }
            if (exhausted) break;
            uint64_t& Ta = T[block_a[b]];
            if (block_kind[b] == GF2_MSTREAM_CNOT) {
                uint64_t& Tb = T[block_b[b]];
                gf2_mstream_cnot_map(&Ta, &Tb);
                Ta ^= first, Tb ^= second;
            } else {
                if (plan.step[(size_t)b] >= 0) out[plan.step[(size_t)b]] = (Ta & gf2_stream_frame_mask(block_kind[b])) ^ first;
                Ta ^= second;
            }
        }
        out[plan.nsteps + plan.flag_words] = attempts;
    }
    return GF2_OK;
}

}  // extern "C"
