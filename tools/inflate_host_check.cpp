// inflate_host_check.cpp -- a stand-alone check of the gunzip code that runs on the host, for a sanitizer build:
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=undefined -Iinclude \
//       tools/inflate_host_check.cpp -o /tmp/inflate_host_check
// It runs the device decoder's host model (csrc/pf_deflate.h: host_inflate_model, the format functions the kernel uses
// too), which inflates every member from a heap buffer of exactly its payload into one of exactly its ISIZE: a step
// past either end is the sanitizer's to report.  This is where the decoder's bounds are proven before anything hostile
// reaches a GPU.  Without an argument it round-trips a few texts through the encoder's host model and refuses a few
// damaged members made here.  The accepted and the rejected inputs of tests/inflate_cases.py come from a file, given as
// the one argument (tests/test_inflate_host_model.py writes it):
// -- records of taken (u32), name length (u32), name, members length (u64), members, text length (u64), text,
// little-endian, for the built chunk size.  Exit status 0: every accepted input gave its text, every rejected one was
// refused.
#include "../panfeed_amd/csrc/pf_deflate.h"

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <string>

namespace {
using Bytes = std::vector<uint8_t>;
int failures = 0, checks = 0;

void check(const std::string& name, const Bytes& members, const Bytes& text, bool taken) {
    // (from a heap copy of exactly the file's bytes: the member listing reads tails and heads near both ends)
    const Bytes file(members);
    Bytes got;
    uint64_t bad = 0;
    uint32_t status = 0;
    checks++;
    const bool ok = pfgz::host_inflate_model(file.data(), file.size(), got, &bad, &status);
    if (ok != taken || (taken && got != text)) {
        failures++;
        fprintf(stderr, "FAIL %s: %s, member %llu: %s\n", name.c_str(), ok ? "taken" : "not taken", (unsigned long long)bad,
                pfgz::inf_status_name(status));
    }
}

bool read_bytes(FILE* f, Bytes& b) {
    uint64_t n;
    if (fread(&n, 8, 1, f) != 1 || n > (1u << 28)) return false;
    b.resize((size_t)n);
    return fread(b.data(), 1, b.size(), f) == b.size();
}

bool check_file(const char* path) {
    FILE* f = fopen(path, "rb");
    if (!f) return false;
    bool ok = true;
    for (;;) {
        uint32_t head[2];
        if (fread(head, 4, 2, f) != 2) { ok = feof(f) != 0; break; }
        std::string name(head[1] <= 256 ? head[1] : 0, '\0');
        Bytes members, text;
        if (head[1] > 256 || fread(&name[0], 1, head[1], f) != head[1] || !read_bytes(f, members) || !read_bytes(f, text)) { ok = false; break; }
        check(name, members, text, head[0] != 0);
    }
    fclose(f);
    return ok;
}

Bytes random_bytes(uint32_t seed, size_t n, uint32_t alphabet) {
    std::mt19937 rng(seed);
    Bytes b(n);
    for (auto& x : b) x = (uint8_t)(rng() % alphabet);
    return b;
}
}  // namespace

int main(int argc, char** argv) {
    const uint32_t C = pfgz::CHUNK, FLAGS[4] = {0, PF_GZ_FIXED_ONLY, PF_GZ_DYNAMIC_ONLY, PF_GZ_DYNAMIC_ONLY | PF_GZ_LITERALS_ONLY};
    std::vector<std::pair<std::string, Bytes>> texts = {
        {"empty", {}}, {"one", Bytes(1, 'q')}, {"run", Bytes(2 * C + 3, 'a')}, {"random", random_bytes(3, C + 17, 256)},
        {"four_letters", random_bytes(4, 3 * C - 1, 4)}, {"short_run", Bytes(259, 'a')}};
    for (const auto& t : texts)
        for (uint32_t flags : FLAGS) {
            Bytes members;
            if (!pfgz::host_model(t.second.data(), t.second.size(), flags, members)) { failures++; continue; }
            check(t.first, members, t.second, true);
            if (members.size() < 40) continue;
            Bytes cut(members.begin(), members.end() - 5), flipped(members), crc(members);
            flipped[members.size() / 2] ^= 0x04; crc[members.size() - 7] ^= 0x80;
            check(t.first + " cut", cut, {}, false);
            check(t.first + " wrong crc", crc, {}, false);
            // (a flipped bit inside a stored block's text only changes the text: the CRC32 refuses it all the same)
            check(t.first + " flipped", flipped, {}, false);
        }
    if (argc > 1 && !check_file(argv[1])) { failures++; fprintf(stderr, "FAIL reading %s\n", argv[1]); }
    printf("%d checks, %d failures\n", checks, failures);
    return failures ? 1 : 0;
}
