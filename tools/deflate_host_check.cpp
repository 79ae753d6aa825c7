// deflate_host_check.cpp -- a stand-alone check of the gzip code that runs on the host, for a sanitizer build:
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=undefined -Iinclude \
//       tools/deflate_host_check.cpp panfeed_amd/csrc/pf_gzip.cpp -lz -lpthread -o /tmp/deflate_host_check
// It runs the device encoder's host model (csrc/pf_deflate.h: the format functions the kernel uses too) and the host
// path's pf_gzip_members (csrc/pf_gzip.cpp) over the edge cases of tests/deflate_cases.py (cases 1-9, generated here),
// under every flag set that applies, and inflates every result with zlib: it must be the input.  Exit status 0: all equal.
// Every case also runs under PF_GZ_DEEP (the second candidate and the lazy parse); case 11 is texts of rows for it.
// Case 10 is the segmented container (chunk_plan, host_model_segments) over the segment shapes of tests/deflate_segments.py.
// The cases that are built in Python only (wide_tokens, whose widest tokens put_bits writes into three words, and the
// fibonacci text that reaches the code length limit) come from a file, given as the one argument:
//   python tests/deflate_cases.py /tmp/deflate_cases.bin && /tmp/deflate_host_check /tmp/deflate_cases.bin
// -- records of flags (u32), name length (u32), name, text length (u64), text, little-endian, for the built chunk size.
#include "../panfeed_amd/csrc/pf_deflate.h"
#include "../panfeed_amd/csrc/pf_host.h"

#include <zlib.h>

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <string>

extern "C" void pf_set_error_(const char* msg) { fprintf(stderr, "library error: %s\n", msg); }
unsigned pf_host_threads(unsigned cap) { return cap < 4 ? cap : 4; }

namespace {
using Bytes = std::vector<uint8_t>;
int failures = 0, checks = 0;

// every member of a multi-member gzip stream, inflated and joined
bool gunzip(const uint8_t* p, size_t n, Bytes& out) {
    out.clear();
    size_t at = 0;
    while (at < n) {
        z_stream zs;
        memset(&zs, 0, sizeof zs);
        if (inflateInit2(&zs, 15 + 16) != Z_OK) return false;
        zs.next_in = const_cast<Bytef*>(p + at);
        zs.avail_in = (uInt)(n - at);
        int rc = Z_OK;
        while (rc == Z_OK) {
            uint8_t buf[65536];
            zs.next_out = buf; zs.avail_out = sizeof buf;
            rc = inflate(&zs, Z_NO_FLUSH);
            out.insert(out.end(), buf, buf + (sizeof buf - zs.avail_out));
        }
        at += zs.total_in;
        inflateEnd(&zs);
        if (rc != Z_STREAM_END) return false;
    }
    return true;
}

void check(const std::string& name, const Bytes& data, uint32_t flags) {
    Bytes members, back;
    checks++;
    bool ok = pfgz::host_model(data.data(), data.size(), flags, members) && gunzip(members.data(), members.size(), back) && back == data;
    if (data.empty()) ok = ok && members.empty();
    if (!ok) { failures++; fprintf(stderr, "FAIL host model %s flags %u\n", name.c_str(), flags); }
    if (flags == 0 && !data.empty()) {
        char* out = nullptr;
        uint64_t out_n = 0;
        checks++;
        const int rc = pf_gzip_members(reinterpret_cast<const char*>(data.data()), data.size(), 9, 65536, &out, &out_n);
        if (rc != 0 || !gunzip(reinterpret_cast<const uint8_t*>(out), out_n, back) || back != data) {
            failures++; fprintf(stderr, "FAIL pf_gzip_members %s\n", name.c_str());
        }
        free(out);
    }
}

// the host model over segments: every segment's members are those of its text alone, member_end their running sum, the
// whole inflates to the text; lens: the segments' lengths
void check_segments(const std::string& name, const Bytes& data, const std::vector<uint64_t>& lens, uint32_t flags) {
    std::vector<uint64_t> ends, member_end(lens.size() + 1);
    uint64_t at = 0;
    for (uint64_t l : lens) ends.push_back(at += l);
    Bytes members, want, back;
    checks++;
    bool ok = at == data.size() &&
              pfgz::host_model_segments(data.data(), data.size(), ends.data(), ends.size(), flags, members, member_end.data()) == 0;
    at = 0;
    for (size_t i = 0; ok && i < lens.size(); i++) {
        Bytes one;
        ok = pfgz::host_model(data.data() + at, lens[i], flags, one);
        want.insert(want.end(), one.begin(), one.end());
        ok = ok && member_end[i] == want.size();
        at += lens[i];
    }
    ok = ok && members == want && gunzip(members.data(), members.size(), back) && back == data;
    if (!ok) { failures++; fprintf(stderr, "FAIL host model segments %s flags %u\n", name.c_str(), flags); }
}
// ends that are no plan are refused, nothing is read through them
void check_refusals() {
    const Bytes d(10, 'x');
    Bytes members;
    uint64_t member_end[3];
    const uint64_t decreasing[3] = {5, 3, 10}, short_of_n[2] = {4, 9}, past_n[2] = {4, 11};
    checks++;
    if (pfgz::host_model_segments(d.data(), 10, decreasing, 3, 0, members, member_end) != 1 ||
        pfgz::host_model_segments(d.data(), 10, short_of_n, 2, 0, members, member_end) != 1 ||
        pfgz::host_model_segments(d.data(), 10, past_n, 2, 0, members, member_end) != 1 ||
        pfgz::host_model_segments(d.data(), 10, nullptr, 0, 0, members, member_end) != 1 ||
        pfgz::host_model_segments(d.data(), 0, nullptr, 0, 0, members, member_end) != 0 || !members.empty()) {
        failures++; fprintf(stderr, "FAIL host model segments: refusals\n");
    }
}

Bytes random_bytes(uint32_t seed, size_t n) {
    std::mt19937 rng(seed);
    Bytes b(n);
    for (auto& x : b) x = (uint8_t)rng();
    return b;
}

// the records of a file written by tests/deflate_cases.py's dump_cases; false: the file is cut short or cannot be read
bool check_file(const char* path) {
    FILE* f = fopen(path, "rb");
    if (!f) return false;
    bool ok = true;
    for (;;) {
        uint32_t head[2];
        uint64_t n;
        if (fread(head, 4, 2, f) != 2) { ok = feof(f) != 0; break; }
        std::string name(head[1], '\0');
        if (head[1] > 256 || fread(&name[0], 1, head[1], f) != head[1] || fread(&n, 8, 1, f) != 1 || n > (1u << 28)) { ok = false; break; }
        Bytes data((size_t)n);
        if (fread(data.data(), 1, data.size(), f) != data.size()) { ok = false; break; }
        check(name, data, head[0]);
    }
    fclose(f);
    return ok;
}
}  // namespace

int main(int argc, char** argv) {
    const uint32_t C = pfgz::CHUNK, ALL[6] = {0, PF_GZ_FIXED_ONLY, PF_GZ_DYNAMIC_ONLY, PF_GZ_DEEP, PF_GZ_DEEP | PF_GZ_FIXED_ONLY,
                                              PF_GZ_DEEP | PF_GZ_DYNAMIC_ONLY};
    auto all = [&](const std::string& name, const Bytes& d) { for (uint32_t f : ALL) check(name, d, f); };
    for (size_t n = 0; n <= 4; n++) all("short", Bytes(n, 'q'));                                  // 1
    Bytes every(512);
    for (size_t i = 0; i < 512; i++) every[i] = (uint8_t)i;
    all("all_bytes_twice", every);                                                               // 2
    for (size_t n : {1u, 2u, 3u, 4u, 5u, 257u, 258u, 259u, 260u, 261u, 516u, 517u, C - 1, C, C + 1, 2 * C + 3}) {   // 3
        all("run", Bytes(n, 'a'));
        Bytes p2(n);
        for (size_t i = 0; i < n; i++) p2[i] = i & 1 ? '\t' : '0';
        all("period2", p2);
    }
    for (uint32_t L : {3u, 4u, 10u, 11u, 12u, 13u, 16u, 18u, 19u, 26u, 34u, 35u, 66u, 67u, 130u, 131u, 226u, 257u, 258u}) {   // 4
        Bytes R = random_bytes(1000 + L, 300);
        for (auto& x : R) if (x == 0xEE) x = 0x11;               // 0xEE is the byte absent from R
        Bytes d = R;
        d.push_back(0xEE);
        d.insert(d.end(), R.begin(), R.begin() + L);
        d.push_back((uint8_t)(R[L] + 1) == 0xEE ? (uint8_t)(R[L] + 2) : (uint8_t)(R[L] + 1));
        all("length_edge", d);
    }
    for (uint32_t D : {1u, 2u, 3u, 4u, 5u, 7u, 9u, 13u, 17u, 25u, 33u, 49u, 65u, 97u, 129u, 193u, 257u, 385u, 513u, 769u, 1025u,
                       1537u, 2049u, 3073u, 4097u, 6145u, 8193u, 12289u, 16385u, 24577u, 32768u}) {            // 5
        if (D >= 8193 && D >= C - 16) continue;
        Bytes d = random_bytes(2000 + D, D + 8);
        for (uint32_t i = 0; i < 8; i++) d[D + i] = d[i];
        all("distance_edge", d);
    }
    check("incompressible", random_bytes(3, 3 * C + 17), 0);                                      // 6
    {                                                                                            // 7
        uint64_t F[64] = {0, 1, 1};
        for (int i = 3; i < 64; i++) F[i] = F[i - 1] + F[i - 2];
        int m = 2;                                       // byte i occurs F(i) times from F(2) on: with the end-of-block
        while (F[m + 3] - 2 <= C) m++;                   // symbol's one the weights are F(1), F(2), .. -- a chain
        Bytes d;
        for (int i = 2; i <= m; i++) d.insert(d.end(), (size_t)F[i], (uint8_t)i);
        std::mt19937 rng(7);
        for (size_t i = d.size(); i > 1; i--) std::swap(d[i - 1], d[rng() % i]);
        check("fibonacci", d, PF_GZ_LITERALS_ONLY | PF_GZ_DYNAMIC_ONLY);
        check("fibonacci", d, PF_GZ_DYNAMIC_ONLY);
    }
    {                                                                                            // 8
        Bytes perm(every.begin(), every.begin() + 256);
        std::mt19937 rng(8);
        for (size_t i = 256; i > 1; i--) std::swap(perm[i - 1], perm[rng() % i]);
        check("no_distance_symbol", perm, PF_GZ_DYNAMIC_ONLY);
    }
    check("one_literal_symbol", Bytes(64, 'a'), PF_GZ_LITERALS_ONLY | PF_GZ_DYNAMIC_ONLY);         // 9
    {                                                                                            // 10: segments
        const std::vector<std::vector<uint64_t>> shapes = {{0}, {1}, {C}, {C + 1}, {0, 5, 0, 0, C - 1, 1, C, C + 1, 2 * C + 3, 0},
                                                           std::vector<uint64_t>(2100, 40)};
        for (const auto& lens : shapes) {
            uint64_t n = 0;
            for (uint64_t l : lens) n += l;
            Bytes d((size_t)n);                          // rows of a few repeating fields, then bytes no code shortens
            for (size_t i = 0; i < d.size(); i++) d[i] = "ACGTTGCA\tgroup_12\tq83hdkPZ\n"[(i * 7 + i / 29) % 27];
            const Bytes noise = random_bytes(10, std::min<size_t>(4096, d.size() / 2));
            std::copy(noise.begin(), noise.end(), d.begin() + (d.size() - noise.size()) / 3);
            for (uint32_t f : {0u, PF_GZ_FIXED_ONLY, PF_GZ_DYNAMIC_ONLY, PF_GZ_LITERALS_ONLY}) check_segments("segments", d, lens, f);
        }
        check_refusals();
    }
    {                                                                                            // 11: rows, for PF_GZ_DEEP's
        all("only_newlines", Bytes(C + 5, '\n'));                                                // candidate from the row before
        for (size_t row : {1u, 2u, 3u, 40u, 127u, 255u, 256u, 257u, 300u, 5000u, C - 1, C}) {
            Bytes d;
            std::mt19937 rng((uint32_t)row);
            Bytes cells(row);
            for (auto& x : cells) x = "01\t"[rng() % 3];
            while (d.size() < 2 * C + 77) {                     // every row the one before with a few cells changed,
                for (int k = 0; k < 3; k++) cells[rng() % row] = "01\t"[rng() % 3];
                const size_t len = rng() % 5 ? row : 1 + rng() % row;      // some cut short: a candidate past the row's end
                d.insert(d.end(), cells.begin(), cells.begin() + len);
                d.push_back('\n');
            }
            all("rows", d);
            d.erase(d.begin(), d.begin() + row / 2);             // (a chunk that starts inside a row)
            all("rows_from_inside_a_row", d);
        }
    }
    if (argc > 1 && !check_file(argv[1])) { failures++; fprintf(stderr, "FAIL reading %s\n", argv[1]); }
    printf("%d checks, %d failures\n", checks, failures);
    return failures ? 1 : 0;
}
