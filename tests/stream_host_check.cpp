// Stand-alone driver of gf2_stream_words_host and gf2_stream_tally_host (csrc/gf2_host.cpp) for tests/test_stream_sanitizers.py,
// which compiles it together with that translation unit under -fsanitize=address,undefined or -fsanitize=thread and runs it as it
// is.  It reads cases (inputs and the results tests/stream_ref.py expects) from the file named on the command line, a stream of
// little-endian int64 words, copies every array into a heap block of exactly the size the entry point may touch, so that any access
// past an end is the sanitizer's, and compares the results exactly.  The cases run once on the main thread and then on two threads
// at once (the error message is thread-local).
//
//   case      := 1 ntypes nblocks rows type_locations[ntypes] type_flags[ntypes] block_type[nblocks] block_kind[nblocks]
//                type_eff[6 rows] count nfaults fault_first[count + 1] fault_location[nfaults] fault_kind[nfaults] ldw flag_words
//                r1 entries1 r2 entries2 keys1 flips1 keys2 flips2 message_words message_tally | 0 (end)
//                message_words not empty: gf2_stream_words_host must be refused with that text, nothing follows; else
//                words[count ldw] follow and are tallied: message_tally not empty: gf2_stream_tally_host must be refused with that
//                text; else counts[12] classes[count] follow
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
            std::fprintf(stderr, "stream_host_check: the case file ends inside a case\n");
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

bool stream_case(Reader& in) {
    const int64_t ntypes = in.next(), nblocks = in.next(), rows = in.next();
    int64_t* type_locations = in.block<int64_t>(ntypes);
    int64_t* type_flags = in.block<int64_t>(ntypes);
    int32_t* block_type = in.block<int32_t>(nblocks);
    int32_t* block_kind = in.block<int32_t>(nblocks);
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
    uint64_t* words = fresh<uint64_t>(count * ldw);
    uint64_t* counts = fresh<uint64_t>(GF2_STREAM_FIELDS);
    bool ok = true;
    const int status = gf2_stream_words_host(type_eff, type_locations, type_flags, ntypes, block_type, block_kind, nblocks, fault_first, fault_location,
                                             fault_kind, count, words, ldw);
    if (!message_words.empty()) {
        ok = refused(status, message_words);
    } else {
        uint64_t* want_words = in.block<uint64_t>(count * ldw);
        ok = status == 0 && same(words, want_words, sizeof(uint64_t) * (size_t)(count * ldw));
        if (!message_tally.empty()) {
            ok = ok && refused(gf2_stream_tally_host(words, count, ldw, block_kind, nblocks, flag_words, r1, keys1, flips1, entries1, r2, keys2, flips2,
                                                     entries2, counts, nullptr), message_tally);
        } else {
            uint64_t* want_counts = in.block<uint64_t>(GF2_STREAM_FIELDS);
            uint8_t* want_classes = in.block<uint8_t>(count);
            uint8_t* classes = fresh<uint8_t>(count);
            ok = ok && gf2_stream_tally_host(words, count, ldw, block_kind, nblocks, flag_words, r1, keys1, flips1, entries1, r2, keys2, flips2, entries2,
                                             counts, classes) == 0;
            ok = ok && same(counts, want_counts, sizeof(uint64_t) * GF2_STREAM_FIELDS) && same(classes, want_classes, (size_t)count);
            std::memset(counts, 0xff, sizeof(uint64_t) * GF2_STREAM_FIELDS);            // ... and without class bytes
            ok = ok && gf2_stream_tally_host(words, count, ldw, block_kind, nblocks, flag_words, r1, keys1, flips1, entries1, r2, keys2, flips2, entries2,
                                             counts, nullptr) == 0;
            ok = ok && same(counts, want_counts, sizeof(uint64_t) * GF2_STREAM_FIELDS);
            std::free(want_counts), std::free(want_classes), std::free(classes);
        }
        std::free(want_words);
    }
    std::free(type_locations), std::free(type_flags), std::free(block_type), std::free(block_kind), std::free(type_eff);
    std::free(fault_first), std::free(fault_location), std::free(fault_kind);
    std::free(keys1), std::free(flips1), std::free(keys2), std::free(flips2), std::free(words), std::free(counts);
    return ok;
}

// every case of the file; the number of cases that failed
int run(const std::vector<int64_t>& file, int* cases_out) {
    Reader in{file};
    int failed = 0, cases = 0;
    for (int64_t tag = in.next(); tag != 0; tag = in.next(), ++cases) {
        if (tag != 1) {
            std::fprintf(stderr, "stream_host_check: unknown case tag %lld\n", (long long)tag);
            std::exit(2);
        }
        if (!stream_case(in)) {
            std::fprintf(stderr, "stream_host_check: case %d differs; last message: %s\n", cases, gf2_last_error());
            failed += 1;
        }
    }
    *cases_out = cases;
    return failed;
}

}  // namespace

int main(int argc, char** argv) {
    if (argc != 2) {
        std::fprintf(stderr, "usage: stream_host_check CASES\n");
        return 2;
    }
    std::FILE* f = std::fopen(argv[1], "rb");
    if (!f) {
        std::fprintf(stderr, "stream_host_check: cannot open %s\n", argv[1]);
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
    std::printf("stream host ok: %d cases\n", cases);
    return 0;
}
