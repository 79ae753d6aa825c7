// inflate_large_host_check.cpp -- a stand-alone check of the large-member gunzip route's host code, for a sanitizer build:
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=undefined -Iinclude \
//       tools/inflate_large_host_check.cpp -o /tmp/inflate_large_host_check
// It runs the route's host model (csrc/pf_deflate.h: host_inflate_large -- the find, marker, chain and byte steps the
// kernels run, from the same functions): every pass reads from a heap copy of exactly the bytes a call may look at, every
// ring is a heap buffer of exactly WINDOW entries and every live piece's text one of exactly its size, so a step past any
// of them is the sanitizer's to report.
// Without an argument it feeds the speculative paths hostile bytes: random data, bare and behind a head, and heads cut at
// every byte.  The accepted and the refused inputs of tests/inflate_large_cases.py come from a file, given as the one
// argument (tests/test_inflate_large_host.py writes it); the streams of its first three distinct accepted cases of 1 000 to
// 8 192 bytes, whole and cut short at two thirds, also go to the finder and the marker sink at every bit offset, as the
// random bytes do.  Those paths must never read or write out of bounds and must always
// end.  The file:
// -- records of taken (u32), piece_bytes (u32), name length (u32), name, members length (u64), members, text length (u64),
// text, little-endian.  Every record is also fed to the feed's call sequence in blocks of 4 096 bytes (a member that spans
// calls).  Exit status 0: every accepted input gave its text either way, every refused one was refused.
#include "../panfeed_amd/csrc/pf_deflate.h"

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <string>

namespace {
using Bytes = std::vector<uint8_t>;
int failures = 0, checks = 0;

// the file as a feed gives it: blocks of `block` bytes, what a call does not consume in front of the next block
bool by_blocks(const Bytes& file, uint32_t piece_bytes, size_t block, Bytes& text) {
    pfgz::HostLarge be;
    pfgz::LargeState s;
    pfgz::LargeStats stats;
    Bytes carry;
    size_t at = 0;
    bool eof = false;
    text.clear();
    for (int guard = 0; guard < (1 << 20); guard++) {
        if (!eof) {
            const size_t m = std::min(block, file.size() - at);
            carry.insert(carry.end(), file.begin() + at, file.begin() + at + m);
            at += m; eof = m < block;
        }
        const Bytes call(carry);               // (exactly the call's bytes)
        pfgz::LargeOut o;
        if (pfgz::large_call(be, s, stats, call.data(), call.size(), eof, piece_bytes, o) || !o.taken) return false;
        if (!o.none_yet) text.insert(text.end(), be.text.begin(), be.text.end());
        if (o.none_yet && eof) return false;
        if (o.consumed > carry.size()) return false;
        carry.erase(carry.begin(), carry.begin() + (long)o.consumed);
        if (eof && carry.empty()) return !s.open;
    }
    return false;
}

void check(const std::string& name, const Bytes& members, uint32_t piece_bytes, const Bytes& text, bool taken) {
    const Bytes file(members);
    Bytes got;
    pfgz::LargeStats stats;
    uint64_t bad = 0;
    uint32_t status = 0;
    checks++;
    const bool ok = pfgz::host_inflate_large(file.data(), file.size(), piece_bytes, got, stats, &bad, &status);
    if (ok != taken || (taken && got != text)) {
        failures++;
        fprintf(stderr, "FAIL %s (piece %u): %s, member %llu: %s\n", name.c_str(), piece_bytes, ok ? "taken" : "not taken", (unsigned long long)bad,
                pfgz::inf_status_name(status));
    }
    checks++;
    const bool ok2 = by_blocks(file, piece_bytes, 4096, got);
    if (ok2 != taken || (taken && got != text)) {
        failures++;
        fprintf(stderr, "FAIL %s (piece %u) in blocks of 4096: %s\n", name.c_str(), piece_bytes, ok2 ? "taken" : "not taken");
    }
}

bool read_bytes(FILE* f, Bytes& b) {
    uint64_t n;
    if (fread(&n, 8, 1, f) != 1 || n > (1u << 28)) return false;
    b.resize((size_t)n);
    return fread(b.data(), 1, b.size(), f) == b.size();
}

// the finder and the marker sink at every bit offset of `data`, whatever stands there
void hostile(const std::string& name, const Bytes& data) {
    const Bytes heap(data);
    pfgz::DecodeTables T;
    std::vector<uint64_t> starts;
    for (uint64_t bit = 0; bit < heap.size() * 8; bit++) {
        checks++;
        if (pfgz::block_start_ok(heap.data(), (uint32_t)heap.size(), bit, T)) starts.push_back(bit);
    }
    // every bit offset as a start of its own (most are garbage), and the found ones with the stop rule among them.  (A run
    // writes the ring's entries 0 .. min(produced, WINDOW): those are set back behind it, the rest still hold their markers)
    std::vector<uint16_t> ring(pfgz::WINDOW);
    auto fresh = [&](uint32_t upto) { for (uint32_t j = 0; j < std::min(upto, pfgz::WINDOW); j++) ring[j] = (uint16_t)(pfgz::MARK | j); };
    fresh(pfgz::WINDOW);
    for (uint64_t bit = 0; bit < heap.size() * 8; bit++) {
        pfgz::HostRing<uint16_t> sink{ring.data(), nullptr};
        const uint64_t one[2] = {bit, heap.size() * 8};
        const pfgz::PieceResult R = pfgz::marker_run(heap.data(), (uint32_t)heap.size(), one, 2, 0, T, sink);
        checks++;
        if (R.status == pfgz::INF_OK && R.end_bit > heap.size() * 8) { failures++; fprintf(stderr, "FAIL %s: a run ended past the data\n", name.c_str()); }
        fresh(R.produced);
    }
    for (uint32_t i = 0; i < starts.size(); i++) {
        fresh(pfgz::WINDOW);
        pfgz::HostRing<uint16_t> sink{ring.data(), nullptr};
        (void)pfgz::marker_run(heap.data(), (uint32_t)heap.size(), starts.data(), (uint32_t)starts.size(), i, T, sink);
        checks++;
    }
    // and as a file: whatever it is, the calls end
    Bytes got;
    pfgz::LargeStats stats;
    uint64_t bad = 0;
    uint32_t status = 0;
    for (uint32_t piece : {64u, 200u, 0u}) { (void)pfgz::host_inflate_large(heap.data(), heap.size(), piece, got, stats, &bad, &status); checks++; }
}

bool check_file(const char* path) {
    FILE* f = fopen(path, "rb");
    if (!f) return false;
    bool ok = true;
    std::vector<std::string> fuzzed;           // the cases whose streams went to hostile(): each once, whatever its records
    for (;;) {
        uint32_t head[3];
        if (fread(head, 4, 3, f) != 3) { ok = feof(f) != 0; break; }
        std::string name(head[2] <= 256 ? head[2] : 0, '\0');
        Bytes members, text;
        if (head[2] > 256 || fread(&name[0], 1, head[2], f) != head[2] || !read_bytes(f, members) || !read_bytes(f, text)) { ok = false; break; }
        check(name, members, head[1], text, head[0] != 0);
        // the real streams of a few distinct cases (the small ones: a hand-written chain, zlib's blocks under a full head),
        // whole and cut short: the finder and the marker sink at every bit offset of each
        if (head[0] && members.size() > 1000 && members.size() < 8192 && fuzzed.size() < 3 && std::find(fuzzed.begin(), fuzzed.end(), name) == fuzzed.end()) {
            fuzzed.push_back(name);
            hostile(name, members);
            hostile(name + " cut", Bytes(members.begin(), members.begin() + (long)(members.size() * 2 / 3)));
        }
    }
    fclose(f);
    if (fuzzed.size() < 2) { ok = false; fprintf(stderr, "FAIL: fewer than two cases small enough for every bit offset\n"); }
    printf("every bit offset of:");
    for (const auto& n : fuzzed) printf(" %s", n.c_str());
    printf("\n");
    return ok;
}

Bytes random_bytes(uint32_t seed, size_t n) {
    std::mt19937 rng(seed);
    Bytes b(n);
    for (auto& x : b) x = (uint8_t)rng();
    return b;
}
}  // namespace

int main(int argc, char** argv) {
    // random data, bare and behind a head; heads that run past the data; a dynamic header cut at every byte
    for (uint32_t seed = 1; seed <= 4; seed++) {
        Bytes r = random_bytes(seed, 3000 + 977 * seed);
        hostile("random", r);
        const uint8_t head[10] = {0x1F, 0x8B, 8, 0, 0, 0, 0, 0, 0, 255};
        r.insert(r.begin(), head, head + 10);
        hostile("random behind a head", r);
        check("random behind a head", r, 64, {}, false);
    }
    const uint8_t flagged[] = {0x1F, 0x8B, 8, 0x1E, 0, 0, 0, 0, 0, 3, 4, 0, 'a', 'b', 'c', 'd', 'n', 'a', 'm', 'e', 0, 'c', 0, 0x12, 0x34, 3, 0};
    for (size_t n = 1; n <= sizeof flagged; n++) {
        uint64_t head = 0;
        const Bytes cut(flagged, flagged + n);
        const uint32_t st = pfgz::parse_head(cut.data(), cut.size(), &head);
        checks++;
        if ((st == pfgz::INF_OK) != (n >= 25) || (st == pfgz::INF_OK && head != 25)) { failures++; fprintf(stderr, "FAIL head cut at %zu: status %u, %llu bytes\n", n, st, (unsigned long long)head); }
        check("head cut", cut, 64, {}, false);
    }
    if (argc > 1 && !check_file(argv[1])) { failures++; fprintf(stderr, "FAIL reading %s\n", argv[1]); }
    printf("%d checks, %d failures\n", checks, failures);
    return failures ? 1 : 0;
}
