// Stand-alone driver of gf2_gate_outcomes_host followed by gf2_ec_tally_host / gf2_ft_tally_host (csrc/gf2_host.cpp) for
// tests/test_gate_mc_sanitizers.py, which compiles it together with that translation unit under -fsanitize=address,undefined or
// -fsanitize=thread and runs it as it is.  It reads cases (inputs, and the words, fault counts and tally tests/gate_mc_ref.py expects)
// from the file named on the command line, a stream of little-endian int64 words, copies every array into a heap block of exactly
// the size the entry point may touch, so that any access past an end is the sanitizer's, and compares the results exactly.  The
// cases run once on the main thread and then on two threads at once (the error message is thread-local).
//
//   case      := 1 cycle | 2 program | 0 (end)
//   cycle     := locations ldr rounds        r1 entries1 r2 entries2 n1 n2 p1 p2 seed first_sample count ldw with_faults
//                eff[2 locations ldr] site_loc[n1 + n2] keys1 flips1 keys2 flips2 message
//   program   := locations ldr nsteps mask   ... the same
//                (p1, p2: the bits of the doubles.  message empty: words[count ldr], faults[3 count] and the gadget's counts[F] follow;
//                else the call must be refused with that text)
//   message   := length, then one word per character
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <thread>
#include <vector>

#include "gf2hip.h"

namespace {

struct Reader {
    const std::vector<int64_t>& file;
    size_t at = 0;
    int64_t next() {
        if (at >= file.size()) {
            std::fprintf(stderr, "gate_mc_host_check: the case file ends inside a case\n");
            std::exit(2);
        }
        return file[at++];
    }
    double real() {
        const int64_t bits = next();
        double out;
        std::memcpy(&out, &bits, sizeof out);
        return out;
    }
    // count words as a heap block of exactly count elements of T (null for none)
    template <typename T>
    T* block(int64_t count) {
        T* out = count > 0 ? static_cast<T*>(std::malloc(sizeof(T) * (size_t)count)) : nullptr;
        for (int64_t i = 0; i < count; ++i) out[i] = (T)next();
        return out;
    }
    std::string message() {
        std::string out;
        for (int64_t i = 0, len = next(); i < len; ++i) out.push_back((char)next());
        return out;
    }
};

bool refused(int status, const std::string& message) { return status == -1 && std::strstr(gf2_last_error(), message.c_str()); }

const uint64_t UNTOUCHED = 0xA5A5A5A5A5A5A5A5ull;
const int32_t UNTOUCHED32 = (int32_t)0xA5A5A5A5;

bool mc_case(Reader& in, bool program) {
    const int64_t locations = in.next(), ldr = in.next();
    const int64_t rounds_or_nsteps = in.next();
    const uint64_t measure_mask = program ? (uint64_t)in.next() : 0;
    const int64_t r1 = in.next(), entries1 = in.next(), r2 = in.next(), entries2 = in.next();
    const int64_t n1 = in.next(), n2 = in.next();
    const double p1 = in.real(), p2 = in.real();
    const uint64_t seed = (uint64_t)in.next();
    const int64_t first_sample = in.next(), count = in.next(), ldw = in.next(), with_faults = in.next();
    uint64_t* eff = in.block<uint64_t>(2 * locations * ldr);
    int32_t* site_loc = in.block<int32_t>(n1 + n2);
    uint64_t* keys1 = in.block<uint64_t>(entries1);
    uint8_t* flips1 = in.block<uint8_t>(entries1);
    uint64_t* keys2 = in.block<uint64_t>(entries2);
    uint8_t* flips2 = in.block<uint8_t>(entries2);
    const std::string message = in.message();
    const int fields = program ? GF2_FT_FIELDS : GF2_EC_FIELDS;
    // a refused call may not touch the words or the fault counts at all
    const int64_t nwords = count > 0 && ldw > 0 ? count * ldw : 0, nfaults = count > 0 ? 3 * count : 0;
    uint64_t* words = static_cast<uint64_t*>(std::malloc(sizeof(uint64_t) * (size_t)(nwords > 0 ? nwords : 1)));
    int32_t* faults = static_cast<int32_t*>(std::malloc(sizeof(int32_t) * (size_t)(nfaults > 0 ? nfaults : 1)));
    for (int64_t i = 0; i < (nwords > 0 ? nwords : 1); ++i) words[i] = UNTOUCHED;
    for (int64_t i = 0; i < (nfaults > 0 ? nfaults : 1); ++i) faults[i] = UNTOUCHED32;
    const int status = gf2_gate_outcomes_host(eff, locations, ldr, site_loc, n1, n2, seed, first_sample, count, p1, p2, words, ldw,
                                              with_faults ? faults : nullptr);
    bool ok = true;
    if (!message.empty()) {
        ok = refused(status, message);
        for (int64_t i = 0; i < nwords; ++i) ok = ok && words[i] == UNTOUCHED;
        for (int64_t i = 0; i < nfaults; ++i) ok = ok && faults[i] == UNTOUCHED32;
    } else {
        uint64_t* want = in.block<uint64_t>(count * ldr);
        int32_t* want_faults = in.block<int32_t>(3 * count);
        uint64_t* want_counts = in.block<uint64_t>(fields);
        ok = status == 0;
        for (int64_t i = 0; ok && i < count; ++i) {
            for (int q = 0; q < 3; ++q) ok = ok && faults[3 * i + q] == (with_faults ? want_faults[3 * i + q] : UNTOUCHED32);
            for (int64_t q = 0; q < ldw; ++q) ok = ok && words[i * ldw + q] == (q < ldr ? want[i * ldr + q] : UNTOUCHED);
        }
        if (ok) {                                                                  // the gadget's rule on the words, pitch ldw
            uint64_t* counts = static_cast<uint64_t*>(std::malloc(sizeof(uint64_t) * (size_t)fields));
            std::memset(counts, 0xff, sizeof(uint64_t) * (size_t)fields);
            const int tallied = program ? gf2_ft_tally_host(count > 0 ? words : nullptr, count, ldw, ldr, rounds_or_nsteps, measure_mask, r1, keys1,
                                                            flips1, entries1, r2, keys2, flips2, entries2, counts, nullptr)
                                        : gf2_ec_tally_host(count > 0 ? words : nullptr, count, ldw, ldr, rounds_or_nsteps, r1, keys1, flips1, entries1,
                                                            r2, keys2, flips2, entries2, counts, nullptr);
            ok = tallied == 0 && std::memcmp(counts, want_counts, sizeof(uint64_t) * (size_t)fields) == 0;
            std::free(counts);
        }
        std::free(want), std::free(want_faults), std::free(want_counts);
    }
    std::free(eff), std::free(site_loc), std::free(keys1), std::free(flips1), std::free(keys2), std::free(flips2), std::free(words), std::free(faults);
    return ok;
}

// every case of the file; the number of cases that failed
int run(const std::vector<int64_t>& file, int* cases_out) {
    Reader in{file};
    int failed = 0, cases = 0;
    for (int64_t tag = in.next(); tag != 0; tag = in.next(), ++cases) {
        if (tag != 1 && tag != 2) {
            std::fprintf(stderr, "gate_mc_host_check: unknown case tag %lld\n", (long long)tag);
            std::exit(2);
        }
        if (!mc_case(in, tag == 2)) {
            std::fprintf(stderr, "gate_mc_host_check: case %d differs; last message: %s\n", cases, gf2_last_error());
            failed += 1;
        }
    }
    *cases_out = cases;
    return failed;
}

}  // namespace

int main(int argc, char** argv) {
    if (argc != 2) {
        std::fprintf(stderr, "usage: gate_mc_host_check CASES\n");
        return 2;
    }
    std::FILE* f = std::fopen(argv[1], "rb");
    if (!f) {
        std::fprintf(stderr, "gate_mc_host_check: cannot open %s\n", argv[1]);
        return 2;
    }
    std::vector<int64_t> file;
    int64_t word;
    while (std::fread(&word, sizeof word, 1, f) == 1) file.push_back(word);
    std::fclose(f);
    int cases = 0, twice[2] = {0, 0}, failed_twice[2] = {0, 0};
    int failed = run(file, &cases);
    std::thread workers[2];
    for (int t = 0; t < 2; ++t) workers[t] = std::thread([&, t] { failed_twice[t] = run(file, &twice[t]); });
    for (int t = 0; t < 2; ++t) workers[t].join();
    failed += failed_twice[0] + failed_twice[1];
    if (failed || twice[0] != cases || twice[1] != cases) return 1;
    std::printf("gate mc host ok: %d cases\n", cases);
    return 0;
}
