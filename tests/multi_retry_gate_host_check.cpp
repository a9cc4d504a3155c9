// Stand-alone driver of gf2_mretry_gate_words_host (csrc/gf2_host.cpp) for tests/test_multi_retry_gate_sanitizers.py, which compiles
// it together with that translation unit under -fsanitize=address,undefined or -fsanitize=thread and runs it as it is.  It reads cases
// (inputs and the results tests/multi_retry_gate_ref.py expects) from the file named on the command line, a stream of little-endian int64
// words, copies every array into a heap block of exactly the size the entry point may touch, so that any access past an end is the
// sanitizer's, and compares the results exactly.  The cases run once on the main thread and then on two threads at once (the error
// message is thread-local).
//
//   case      := 1 ntypes nblocks rows nframes nregions nsites type_locations[ntypes] type_flags[ntypes] block_type[nblocks]
//                block_kind[nblocks] block_a[nblocks] block_b[nblocks] type_eff[6 rows] type_regions[3 nregions] type_nregions[ntypes]
//                site_loc[nsites] site_regions[2 nregions]
//                seed first_sample count p_1 p_2 (the bits of the doubles) max_attempts ldw preparations message | 0 (end)
//                message not empty: the call must be refused with that text, nothing follows; else words[count ldw] follow (the
//                buffer starts out as a copy of them with the first nsteps + F + 1 words of every row inverted, so the padding must
//                come back untouched), then attempts[count preparations]; the call is made with and without the attempts array
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
            std::fprintf(stderr, "multi_retry_gate_host_check: the case file ends inside a case\n");
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

bool same(const void* got, const void* want, size_t bytes) { return bytes == 0 || std::memcmp(got, want, bytes) == 0; }

bool refused(int status, const std::string& message) { return status == -1 && std::strstr(gf2_last_error(), message.c_str()); }

bool mretry_gate_case(Reader& in) {
    const int64_t ntypes = in.next(), nblocks = in.next(), rows = in.next(), nframes = in.next(), nregions = in.next(), nsites = in.next();
    int64_t* type_locations = in.block<int64_t>(ntypes);
    int64_t* type_flags = in.block<int64_t>(ntypes);
    int32_t* block_type = in.block<int32_t>(nblocks);
    int32_t* block_kind = in.block<int32_t>(nblocks);
    int32_t* block_a = in.block<int32_t>(nblocks);
    int32_t* block_b = in.block<int32_t>(nblocks);
    uint64_t* type_eff = in.block<uint64_t>(6 * rows);
    int64_t* type_regions = in.block<int64_t>(3 * nregions);
    int64_t* type_nregions = in.block<int64_t>(ntypes);
    int32_t* site_loc = in.block<int32_t>(nsites);
    int64_t* site_regions = in.block<int64_t>(2 * nregions);
    const uint64_t seed = (uint64_t)in.next();
    const int64_t first_sample = in.next(), count = in.next();
    const double p1 = in.real(), p2 = in.real();
    const int64_t max_attempts = in.next(), ldw = in.next(), preparations = in.next();
    const std::string message = in.message();
    const int64_t cells = count > 0 && ldw > 0 ? count * ldw : 0, tries = count > 0 ? count * preparations : 0;
    bool ok = true;
    auto call = [&](uint64_t* words, uint32_t* attempts) {
        return gf2_mretry_gate_words_host(type_eff, type_locations, type_flags, ntypes, block_type, block_kind, block_a, block_b, nblocks, nframes,
                                          type_regions, type_nregions, site_loc, site_regions, seed, first_sample, count, p1, p2, max_attempts, words,
                                          ldw, attempts);
    };
    if (!message.empty()) {
        uint64_t* words = cells ? static_cast<uint64_t*>(std::calloc((size_t)cells, 8)) : nullptr;
        uint32_t* attempts = tries ? static_cast<uint32_t*>(std::calloc((size_t)tries, 4)) : nullptr;
        ok = refused(call(words, attempts), message);
        std::free(words), std::free(attempts);
    } else {
        int64_t nsteps = 0, flag_rows = 0;
        for (int64_t b = 0; b < nblocks; ++b) {
            nsteps += block_kind[b] == GF2_STREAM_EC || block_kind[b] == GF2_STREAM_MEASURE;
            flag_rows += type_flags[block_type[b]];
        }
        const int64_t ldr = nsteps + (flag_rows > 64 ? (flag_rows + 63) / 64 : 1) + 1;
        uint64_t* want_words = in.block<uint64_t>(cells);
        uint32_t* want_attempts = in.block<uint32_t>(tries);
        for (int pass = 0; pass < 2; ++pass) {                                     // with the attempts array, then without
            uint64_t* words = cells ? static_cast<uint64_t*>(std::malloc((size_t)cells * 8)) : nullptr;
            uint32_t* attempts = tries && pass == 0 ? static_cast<uint32_t*>(std::malloc((size_t)tries * 4)) : nullptr;
            for (int64_t i = 0; i < count; ++i)
                for (int64_t q = 0; q < ldw; ++q) words[i * ldw + q] = q < ldr ? ~want_words[i * ldw + q] : want_words[i * ldw + q];
            if (attempts) std::memset(attempts, 0xff, (size_t)tries * 4);
            ok = ok && call(words, attempts) == 0;
            ok = ok && same(words, want_words, (size_t)cells * 8);
            if (attempts) ok = ok && same(attempts, want_attempts, (size_t)tries * 4);
            std::free(words), std::free(attempts);
        }
        std::free(want_words), std::free(want_attempts);
    }
    std::free(type_locations), std::free(type_flags), std::free(block_type), std::free(block_kind), std::free(block_a), std::free(block_b);
    std::free(type_eff), std::free(type_regions), std::free(type_nregions), std::free(site_loc), std::free(site_regions);
    return ok;
}

// every case of the file; the number of cases that failed
int run(const std::vector<int64_t>& file, int* cases_out) {
    Reader in{file};
    int failed = 0, cases = 0;
    for (int64_t tag = in.next(); tag != 0; tag = in.next(), ++cases) {
        if (tag != 1) {
            std::fprintf(stderr, "multi_retry_gate_host_check: unknown case tag %lld\n", (long long)tag);
            std::exit(2);
        }
        if (!mretry_gate_case(in)) {
            std::fprintf(stderr, "multi_retry_gate_host_check: case %d differs; last message: %s\n", cases, gf2_last_error());
            failed += 1;
        }
    }
    *cases_out = cases;
    return failed;
}

}  // namespace

int main(int argc, char** argv) {
    if (argc != 2) {
        std::fprintf(stderr, "usage: multi_retry_gate_host_check CASES\n");
        return 2;
    }
    std::FILE* f = std::fopen(argv[1], "rb");
    if (!f) {
        std::fprintf(stderr, "multi_retry_gate_host_check: cannot open %s\n", argv[1]);
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
    std::printf("multi retry gate host ok: %d cases\n", cases);
    return 0;
}
