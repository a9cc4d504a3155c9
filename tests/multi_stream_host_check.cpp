// Stand-alone driver of gf2_mstream_words_host and gf2_mstream_tally_host (csrc/gf2_host.cpp) for tests/test_multi_stream_sanitizers.py,
// which compiles it together with that translation unit under -fsanitize=address,undefined or -fsanitize=thread and runs it as it
// is.  It reads cases (inputs and the results tests/multi_stream_ref.py expects) from the file named on the command line, a stream of
// little-endian int64 words, copies every array into a heap block of exactly the size the entry point may touch, so that any access
// past an end is the sanitizer's, and compares the results exactly.  The cases run once on the main thread and then on two threads
// at once (the error message is thread-local).
//
//   case      := 1 ntypes nblocks rows nframes type_locations[ntypes] type_flags[ntypes] block_type[nblocks] block_kind[nblocks]
//                block_a[nblocks] block_b[nblocks] type_eff[6 rows] count nfaults fault_first[count + 1] fault_location[nfaults]
//                fault_kind[nfaults] ldw flag_words r1 entries1 r2 entries2 keys1 flips1 keys2 flips2 message_words message_tally
//                | 0 (end)
//                message_words not empty: gf2_mstream_words_host must be refused with that text, nothing follows; else
//                words[count ldw] follow (the buffer starts out as a copy of them with the first nsteps + flag_words words of every
//                row inverted, so the padding must come back untouched) and are tallied under both settings of `records`:
//                message_tally not empty: gf2_mstream_tally_host must be refused with that text; else counts[20] of REFERENCE and
//                counts[20] of PROPAGATED follow
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
            std::fprintf(stderr, "multi_stream_host_check: the case file ends inside a case\n");
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

template <typename T>
T* fresh(int64_t count) {
    return count > 0 ? static_cast<T*>(std::calloc((size_t)count, sizeof(T))) : nullptr;
}

bool same(const void* got, const void* want, size_t bytes) { return bytes == 0 || std::memcmp(got, want, bytes) == 0; }

bool refused(int status, const std::string& message) { return status == -1 && std::strstr(gf2_last_error(), message.c_str()); }

bool mstream_case(Reader& in) {
    const int64_t ntypes = in.next(), nblocks = in.next(), rows = in.next(), nframes = in.next();
    int64_t* type_locations = in.block<int64_t>(ntypes);
    int64_t* type_flags = in.block<int64_t>(ntypes);
    int32_t* block_type = in.block<int32_t>(nblocks);
    int32_t* block_kind = in.block<int32_t>(nblocks);
    int32_t* block_a = in.block<int32_t>(nblocks);
    int32_t* block_b = in.block<int32_t>(nblocks);
    uint64_t* type_eff = in.block<uint64_t>(6 * rows);
    const int64_t count = in.next(), nfaults = in.next();
    int64_t* fault_first = in.block<int64_t>(count + 1);
    int32_t* fault_location = in.block<int32_t>(nfaults);
    uint8_t* fault_kind = in.block<uint8_t>(nfaults);
    const int64_t ldw = in.next(), flag_words = in.next();
    const int64_t r1 = in.next(), entries1 = in.next(), r2 = in.next(), entries2 = in.next();
    uint64_t* keys1 = in.block<uint64_t>(entries1);
    uint8_t* flips1 = in.block<uint8_t>(entries1);
    uint64_t* keys2 = in.block<uint64_t>(entries2);
    uint8_t* flips2 = in.block<uint8_t>(entries2);
    const std::string message_words = in.message(), message_tally = in.message();
    uint64_t* counts = fresh<uint64_t>(GF2_MSTREAM_FIELDS);
    bool ok = true;
    if (!message_words.empty()) {
        uint64_t* words = fresh<uint64_t>(count * ldw);
        ok = refused(gf2_mstream_words_host(type_eff, type_locations, type_flags, ntypes, block_type, block_kind, block_a, block_b, nblocks, nframes,
                                            fault_first, fault_location, fault_kind, count, words, ldw), message_words);
        std::free(words);
    } else {
        int64_t nsteps = 0;
        for (int64_t b = 0; b < nblocks; ++b) nsteps += block_kind[b] == GF2_STREAM_EC || block_kind[b] == GF2_STREAM_MEASURE;
        uint64_t* want_words = in.block<uint64_t>(count * ldw);
        uint64_t* words = count * ldw > 0 ? static_cast<uint64_t*>(std::malloc((size_t)(count * ldw) * 8)) : nullptr;
        for (int64_t i = 0; i < count; ++i)
            for (int64_t q = 0; q < ldw; ++q) words[i * ldw + q] = q < nsteps + flag_words ? ~want_words[i * ldw + q] : want_words[i * ldw + q];
        ok = gf2_mstream_words_host(type_eff, type_locations, type_flags, ntypes, block_type, block_kind, block_a, block_b, nblocks, nframes, fault_first,
                                    fault_location, fault_kind, count, words, ldw) == 0;
        ok = ok && same(words, want_words, sizeof(uint64_t) * (size_t)(count * ldw));
        if (!message_tally.empty()) {
            ok = ok && refused(gf2_mstream_tally_host(words, count, ldw, block_kind, block_a, block_b, nblocks, nframes, flag_words, GF2_MSTREAM_REFERENCE, r1,
                                                      keys1, flips1, entries1, r2, keys2, flips2, entries2, counts, nullptr), message_tally);
        } else {
            for (int64_t records = GF2_MSTREAM_REFERENCE; records <= GF2_MSTREAM_PROPAGATED; ++records) {
                uint64_t* want_counts = in.block<uint64_t>(GF2_MSTREAM_FIELDS);
                uint8_t* classes = fresh<uint8_t>(count);
                std::memset(counts, 0xff, sizeof(uint64_t) * GF2_MSTREAM_FIELDS);
                ok = ok && gf2_mstream_tally_host(words, count, ldw, block_kind, block_a, block_b, nblocks, nframes, flag_words, records, r1, keys1, flips1,
                                                  entries1, r2, keys2, flips2, entries2, counts, classes) == 0;
                ok = ok && same(counts, want_counts, sizeof(uint64_t) * GF2_MSTREAM_FIELDS);
                uint64_t accepted = 0;
                for (int64_t i = 0; i < count; ++i) accepted += classes[i] & 1u;
                ok = ok && accepted == want_counts[0];
                std::memset(counts, 0xff, sizeof(uint64_t) * GF2_MSTREAM_FIELDS);        // ... and without class bytes
                ok = ok && gf2_mstream_tally_host(words, count, ldw, block_kind, block_a, block_b, nblocks, nframes, flag_words, records, r1, keys1, flips1,
                                                  entries1, r2, keys2, flips2, entries2, counts, nullptr) == 0;
                ok = ok && same(counts, want_counts, sizeof(uint64_t) * GF2_MSTREAM_FIELDS);
                std::free(want_counts), std::free(classes);
            }
        }
        std::free(want_words), std::free(words);
    }
    std::free(type_locations), std::free(type_flags), std::free(block_type), std::free(block_kind), std::free(block_a), std::free(block_b);
    std::free(type_eff), std::free(fault_first), std::free(fault_location), std::free(fault_kind);
    std::free(keys1), std::free(flips1), std::free(keys2), std::free(flips2), std::free(counts);
    return ok;
}

// every case of the file; the number of cases that failed
int run(const std::vector<int64_t>& file, int* cases_out) {
    Reader in{file};
    int failed = 0, cases = 0;
    for (int64_t tag = in.next(); tag != 0; tag = in.next(), ++cases) {
        if (tag != 1) {
            std::fprintf(stderr, "multi_stream_host_check: unknown case tag %lld\n", (long long)tag);
            std::exit(2);
        }
        if (!mstream_case(in)) {
            std::fprintf(stderr, "multi_stream_host_check: case %d differs; last message: %s\n", cases, gf2_last_error());
            failed += 1;
        }
    }
    *cases_out = cases;
    return failed;
}

}  // namespace

int main(int argc, char** argv) {
    if (argc != 2) {
        std::fprintf(stderr, "usage: multi_stream_host_check CASES\n");
        return 2;
    }
    std::FILE* f = std::fopen(argv[1], "rb");
    if (!f) {
        std::fprintf(stderr, "multi_stream_host_check: cannot open %s\n", argv[1]);
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
    std::printf("multi stream host ok: %d cases\n", cases);
    return 0;
}
