// bgzf_host_check.cpp -- a stand-alone check of the BGZF code that runs on the host, for a sanitizer build:
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=undefined -Iinclude \
//       tools/bgzf_host_check.cpp -o /tmp/bgzf_host_check
// It runs the device decoder's host model for BGZF (csrc/pf_deflate.h: list_members_bgzf and host_inflate_model_bgzf over
// the format functions the kernels use too), which inflates every member from a heap buffer of exactly its payload into
// one of exactly its ISIZE -- up to 65 536 bytes here: a step past either end is the sanitizer's to report.  Without an
// argument it frames a few texts by the encoder's host model under PF_GZ_BGZF, appends the end marker, reads them back
// and refuses a few damaged files made here.  The accepted and the refused files of tests/bgzf_cases.py come from a file,
// given as the one argument (tests/test_bgzf_host_model.py writes it):
// -- records of taken (u32), name length (u32), name, file length (u64), file, text length (u64), text, little-endian.
// Exit status 0: every accepted file gave its text, every refused one was refused.
#include "../panfeed_amd/csrc/pf_deflate.h"

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <string>

namespace {
using Bytes = std::vector<uint8_t>;
int failures = 0, checks = 0;

void check(const std::string& name, const Bytes& data, const Bytes& text, bool taken) {
    // (from a heap copy of exactly the file's bytes: the member listing reads heads and tails near both ends)
    const Bytes file(data);
    Bytes got;
    uint64_t bad = 0;
    uint32_t status = 0;
    checks++;
    const bool ok = pfgz::host_inflate_model_bgzf(file.data(), file.size(), got, &bad, &status);
    if (ok != taken || (taken && got != text)) {
        failures++;
        fprintf(stderr, "FAIL %s: %s, member %llu: %s\n", name.c_str(), ok ? "taken" : "not taken", (unsigned long long)bad,
                pfgz::inf_status_name(status));
    }
    // the listing alone, as the feed calls it: every prefix length near a member's end, not the last block of a file
    std::vector<pfgz::MemberRef> ms;
    uint64_t consumed = 0;
    for (size_t cut = file.size() > 40 ? file.size() - 40 : 0; cut <= file.size(); cut++) {
        const Bytes part(file.begin(), file.begin() + (ptrdiff_t)cut);
        if (pfgz::list_members_bgzf(part.data(), part.size(), false, ms, &consumed) && consumed > cut) {
            failures++;
            fprintf(stderr, "FAIL %s: %llu bytes listed of %zu\n", name.c_str(), (unsigned long long)consumed, cut);
        }
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
        Bytes data, text;
        if (head[1] > 256 || fread(&name[0], 1, head[1], f) != head[1] || !read_bytes(f, data) || !read_bytes(f, text)) { ok = false; break; }
        check(name, data, text, head[0] != 0);
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
    const uint32_t C = pfgz::CHUNK, FLAGS[3] = {PF_GZ_BGZF, PF_GZ_BGZF | PF_GZ_FIXED_ONLY, PF_GZ_BGZF | PF_GZ_DYNAMIC_ONLY | PF_GZ_LITERALS_ONLY};
    const Bytes eof(pfgz::bgzf_eof(), pfgz::bgzf_eof() + pfgz::BGZF_EOF_BYTES);
    check("marker only", eof, {}, true);
    std::vector<std::pair<std::string, Bytes>> texts = {
        {"one", Bytes(1, 'q')}, {"run", Bytes(2 * C + 3, 'a')}, {"random", random_bytes(3, C + 17, 256)},
        {"four_letters", random_bytes(4, 3 * C - 1, 4)}, {"short_run", Bytes(259, 'a')}};
    for (const auto& t : texts)
        for (uint32_t flags : FLAGS) {
            Bytes members;
            if (!pfgz::host_model(t.second.data(), t.second.size(), flags, members)) { failures++; continue; }
            Bytes file(members);
            file.insert(file.end(), eof.begin(), eof.end());
            check(t.first, file, t.second, true);
            check(t.first + " without the marker", members, t.second, true);
            Bytes cut(members.begin(), members.end() - 5), flipped(file), crc(file), bsize(file);
            const size_t first = (size_t)(members[16] | members[17] << 8) + 1;       // the first member: its payload's middle byte
            flipped[pfgz::BGZF_HEAD + (first - pfgz::BGZF_HEAD - pfgz::MEMBER_TAIL) / 2] ^= 0x04; crc[members.size() - 7] ^= 0x80; bsize[16] ^= 0x40;
            check(t.first + " cut", cut, {}, false);
            check(t.first + " wrong crc", crc, {}, false);
            check(t.first + " another BSIZE", bsize, {}, false);
            // (a flipped bit inside a stored block's text only changes the text: the CRC32 refuses it all the same; in a run of
            // one letter another distance, or another length of an unused code, is another valid stream of the same text)
            if (t.first.find("run") == std::string::npos) check(t.first + " flipped", flipped, {}, false);
        }
    if (argc > 1 && !check_file(argv[1])) { failures++; fprintf(stderr, "FAIL reading %s\n", argv[1]); }
    printf("%d checks, %d failures\n", checks, failures);
    return failures ? 1 : 0;
}
