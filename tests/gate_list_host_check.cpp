// Stand-alone driver of gf2_ec_gate_enumerate_list_host and gf2_ft_gate_enumerate_list_host (csrc/gf2_host.cpp) for
// tests/test_gate_list_sanitizers.py, which compiles it together with that translation unit under -fsanitize=address,undefined or
// -fsanitize=thread and runs it as it is.  It reads cases (inputs and the records tests/gate_list_ref.py expects) from the file named
// on the command line, a stream of little-endian int64 words, copies every array into a heap block of exactly the size the entry point
// may touch -- the site table is n1 + n2 entries, the record buffer exactly `capacity` records, none at all for capacity 0 -- so that
// any access past an end is the sanitizer's, and compares the results exactly.  The cases run once on the main thread and then on two
// threads at once.
//
//   case      := 1 cycle | 2 program | 0 (end)
//   cycle     := locations ldr rounds      r1 entries1 r2 entries2 n1 n2 w b first_rank count select capacity eff[2 locations ldr]
//                site_loc[n1 + n2] keys1 flips1 keys2 flips2 message
//   program   := locations ldr nsteps mask r1 entries1 r2 entries2 n1 n2 w b first_rank count select capacity eff[2 locations ldr]
//                site_loc[n1 + n2] keys1 flips1 keys2 flips2 message
//                (message empty: found follows, and found records of two words if found <= capacity; else the call must be refused
//                with that text, found and the buffer left as they were)
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
            std::fprintf(stderr, "gate_list_host_check: the case file ends inside a case\n");
            std::exit(2);
        }
        return file[at++];
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

const uint64_t kUntouched = 0xffffffffffffffffull;

bool untouched(const uint64_t* words, int64_t from, int64_t to) {
    for (int64_t i = from; i < to; ++i)
        if (words[i] != kUntouched) return false;
    return true;
}

bool refused(int status, const std::string& message) { return status == -1 && std::strstr(gf2_last_error(), message.c_str()); }

bool list_case(Reader& in, bool program) {
    const int64_t locations = in.next(), ldr = in.next();
    const int64_t rounds_or_nsteps = in.next();
    const uint64_t measure_mask = program ? (uint64_t)in.next() : 0;
    const int64_t r1 = in.next(), entries1 = in.next(), r2 = in.next(), entries2 = in.next();
    const int64_t n1 = in.next(), n2 = in.next(), w = in.next(), b = in.next(), first_rank = in.next(), count = in.next();
    const uint64_t select = (uint64_t)in.next();
    const int64_t capacity = in.next();
    uint64_t* eff = in.block<uint64_t>(2 * locations * ldr);
    int32_t* site_loc = in.block<int32_t>(n1 + n2);
    uint64_t* keys1 = in.block<uint64_t>(entries1);
    uint8_t* flips1 = in.block<uint8_t>(entries1);
    uint64_t* keys2 = in.block<uint64_t>(entries2);
    uint8_t* flips2 = in.block<uint8_t>(entries2);
    const std::string message = in.message();
    const int64_t words = capacity > 0 ? GF2_FAULT_RECORD_WORDS * capacity : 0;
    uint64_t* records = words ? static_cast<uint64_t*>(std::malloc(sizeof(uint64_t) * (size_t)words)) : nullptr;
    for (int64_t i = 0; i < words; ++i) records[i] = kUntouched;
    int64_t found = -7;
    const int status =
        program ? gf2_ft_gate_enumerate_list_host(eff, locations, ldr, rounds_or_nsteps, measure_mask, r1, keys1, flips1, entries1, r2, keys2, flips2,
                                                  entries2, site_loc, n1, n2, w, b, first_rank, count, select, capacity, records, &found)
                : gf2_ec_gate_enumerate_list_host(eff, locations, ldr, rounds_or_nsteps, r1, keys1, flips1, entries1, r2, keys2, flips2, entries2,
                                                  site_loc, n1, n2, w, b, first_rank, count, select, capacity, records, &found);
    bool ok;
    if (!message.empty()) {
        ok = refused(status, message) && found == -7 && untouched(records, 0, words);
    } else {
        const int64_t want_found = in.next();
        ok = status == 0 && found == want_found;
        if (want_found <= capacity) {
            uint64_t* want = in.block<uint64_t>(GF2_FAULT_RECORD_WORDS * want_found);
            ok = ok && (want_found == 0 || std::memcmp(records, want, sizeof(uint64_t) * (size_t)(GF2_FAULT_RECORD_WORDS * want_found)) == 0) &&
                 untouched(records, GF2_FAULT_RECORD_WORDS * want_found, words);
            std::free(want);
        } else {
            ok = ok && untouched(records, 0, words);
        }
    }
    std::free(eff), std::free(site_loc), std::free(keys1), std::free(flips1), std::free(keys2), std::free(flips2), std::free(records);
    return ok;
}

// every case of the file; the number of cases that failed
int run(const std::vector<int64_t>& file, int* cases_out) {
    Reader in{file};
    int failed = 0, cases = 0;
    for (int64_t tag = in.next(); tag != 0; tag = in.next(), ++cases) {
        if (tag != 1 && tag != 2) {
            std::fprintf(stderr, "gate_list_host_check: unknown case tag %lld\n", (long long)tag);
            std::exit(2);
        }
        if (!list_case(in, tag == 2)) {
            std::fprintf(stderr, "gate_list_host_check: case %d differs; last message: %s\n", cases, gf2_last_error());
            failed += 1;
        }
    }
    *cases_out = cases;
    return failed;
}

}  // namespace

int main(int argc, char** argv) {
    if (argc != 2) {
        std::fprintf(stderr, "usage: gate_list_host_check CASES\n");
        return 2;
    }
    std::FILE* f = std::fopen(argv[1], "rb");
    if (!f) {
        std::fprintf(stderr, "gate_list_host_check: cannot open %s\n", argv[1]);
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
    std::printf("gate list host ok: %d cases\n", cases);
    return 0;
}
