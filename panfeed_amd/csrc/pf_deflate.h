// pf_deflate.h -- internal: gzip (RFC 1952) members with deflate (RFC 1951) blocks, written by the GPU.
//
// The format logic is written once, as host+device functions: length / distance symbols and their extra bits, the fixed
// codes, the length-limited code builder, the canonical code assignment, the dynamic block header, the bit writer, CRC32
// and its combination.  pf_deflate.hip runs them in the encoder kernel; host_model() below runs the same functions
// serially, with a plain one-candidate greedy matcher, so that the format can be tested without a GPU.
//
// Container: the text is cut into chunks of CHUNK bytes; every chunk becomes one complete gzip member holding one final
// deflate block -- stored, fixed or dynamic, whichever is smallest by exact bit count.  No match reaches before its chunk.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "../../include/panfeed_hip.h"

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define PF_HD __host__ __device__ inline
#else
#define PF_HD inline
#endif

#include <algorithm>
#include <vector>

namespace pfgz {

#ifndef PF_GZ_CHUNK
#define PF_GZ_CHUNK 32768                    // (experiment builds: PF_CXXFLAGS=-DPF_GZ_CHUNK=16384, a multiple of 256 up to 32768)
#endif
constexpr uint32_t CHUNK = PF_GZ_CHUNK;      // bytes of text per member (pf_gzip_device_chunk_bytes)
constexpr uint32_t MAX_MATCH = 258;
constexpr uint32_t N_LL = 286, N_D = 30, N_CL = 19, MAX_BITS = 15;
constexpr uint32_t HASH_BITS = 12;
constexpr uint32_t CRC_SUB = CHUNK / 256;    // a chunk's CRC is combined from those of CRC_SUB-byte pieces
constexpr uint32_t MEMBER_HEAD = 10, MEMBER_TAIL = 8;
// a chunk's slot: the largest member any mode may produce (fixed codes on bytes of 9 bits each; a mode that would not
// fit is replaced by stored, which always does), a multiple of 16
constexpr uint32_t SLOT_BYTES = (CHUNK + CHUNK / 8 + 256 + 15) & ~15u;
constexpr uint32_t SLOT_WORDS = SLOT_BYTES / 4;
constexpr uint32_t MAX_CODED_BITS = (SLOT_BYTES - MEMBER_HEAD - MEMBER_TAIL - 16) * 8;

enum Mode : uint32_t { STORED = 0, FIXED = 1, DYNAMIC = 2 };

// a token: a literal byte (< 256), or bit 31 | (length - 3) << 16 | (distance - 1)
PF_HD uint32_t match_token(uint32_t len, uint32_t dist) { return 0x80000000u | ((len - 3) << 16) | (dist - 1); }

// length 3..258 -> symbol 257..285, its extra bits and their value
PF_HD uint32_t len_sym(uint32_t len, uint32_t* eb, uint32_t* ev) {
    const uint32_t l = len - 3;
    if (len == 258) { *eb = 0; *ev = 0; return 285; }
    if (l < 8) { *eb = 0; *ev = 0; return 257 + l; }
    const uint32_t n = 31 - (uint32_t)__builtin_clz(l);
    *eb = n - 2; *ev = l & ((1u << *eb) - 1);
    return 257 + (*eb + 1) * 4 + ((l >> *eb) & 3);
}
PF_HD uint32_t len_sym_extra(uint32_t sym) { return sym < 265 || sym == 285 ? 0 : (sym - 261) / 4; }
// distance - 1 (0..32767) -> symbol 0..29
PF_HD uint32_t dist_sym(uint32_t d, uint32_t* eb, uint32_t* ev) {
    if (d < 4) { *eb = 0; *ev = 0; return d; }
    const uint32_t n = 31 - (uint32_t)__builtin_clz(d);
    *eb = n - 1; *ev = d & ((1u << *eb) - 1);
    return 2 * n + ((d >> (n - 1)) & 1);
}
PF_HD uint32_t dist_sym_extra(uint32_t sym) { return sym < 4 ? 0 : sym / 2 - 1; }

PF_HD uint32_t bit_reverse(uint32_t code, uint32_t len) {
    uint32_t r = 0;
    for (uint32_t i = 0; i < len; i++) { r = (r << 1) | (code & 1); code >>= 1; }
    return r;
}

// the codes of one block, as they go into the bit stream (bit-reversed: Huffman codes are packed from their top bit)
struct Codes {
    uint16_t ll_code[288], d_code[32];
    uint8_t ll_len[288], d_len[32];
};

PF_HD uint32_t fixed_ll_len(uint32_t s) { return s < 144 ? 8 : s < 256 ? 9 : s < 280 ? 7 : 8; }
PF_HD uint32_t fixed_ll_code(uint32_t s) {          // RFC 1951 3.2.6
    const uint32_t c = s < 144 ? 0x30 + s : s < 256 ? 0x190 + (s - 144) : s < 280 ? s - 256 : 0xC0 + (s - 280);
    return bit_reverse(c, fixed_ll_len(s));
}

// canonical codes (RFC 1951 3.2.2) of n symbols with the given lengths, bit-reversed
PF_HD void canonical_codes(const uint8_t* len, uint32_t n, uint16_t* code) {
    uint32_t count[MAX_BITS + 2] = {0}, next[MAX_BITS + 2];
    for (uint32_t s = 0; s < n; s++) count[len[s]]++;
    count[0] = 0;
    uint32_t c = 0;
    for (uint32_t b = 1; b <= MAX_BITS; b++) { c = (c + count[b - 1]) << 1; next[b] = c; }
    for (uint32_t s = 0; s < n; s++) code[s] = len[s] ? (uint16_t)bit_reverse(next[len[s]]++, len[s]) : 0;
}

struct SymFreq { uint32_t key, sym; };

// Code lengths of the n symbols of A (frequency > 0, sorted by ascending (frequency, symbol)) into len[] (zeroed by the
// caller, indexed by symbol): Huffman's lengths by Moffat and Katajainen's in-place method, then limited to MAX_BITS by
// the bl_count heuristic of miniz / zlib (the over-long codes are cut to the limit and the Kraft sum is repaired from
// the deepest level up).  A code must be complete for inflate to take it, so with fewer than two symbols a second one is
// declared: both get one bit.
PF_HD void build_lengths(SymFreq* A, int n, uint8_t* len) {
    if (n == 0) { len[0] = 1; len[1] = 1; return; }
    if (n == 1) { len[A[0].sym] = 1; len[A[0].sym == 0 ? 1 : 0] = 1; return; }
    A[0].key += A[1].key;
    int root = 0, leaf = 2, next;
    for (next = 1; next < n - 1; next++) {
        if (leaf >= n || A[root].key < A[leaf].key) { A[next].key = A[root].key; A[root++].key = (uint32_t)next; }
        else A[next].key = A[leaf++].key;
        if (leaf >= n || (root < next && A[root].key < A[leaf].key)) { A[next].key += A[root].key; A[root++].key = (uint32_t)next; }
        else A[next].key += A[leaf++].key;
    }
    A[n - 2].key = 0;
    for (next = n - 3; next >= 0; next--) A[next].key = A[A[next].key].key + 1;
    int avbl = 1, used = 0, dpth = 0;
    root = n - 2; next = n - 1;
    while (avbl > 0) {
        while (root >= 0 && (int)A[root].key == dpth) { used++; root--; }
        while (avbl > used) { A[next--].key = (uint32_t)dpth; avbl--; }
        avbl = 2 * used; dpth++; used = 0;
    }
    // A[i].key is now the depth of the i-th rarest symbol
    uint32_t num[40] = {0};
    for (int i = 0; i < n; i++) num[A[i].key < 39 ? A[i].key : 39]++;
    for (uint32_t i = MAX_BITS + 1; i < 40; i++) num[MAX_BITS] += num[i];
    uint32_t total = 0;
    for (uint32_t i = MAX_BITS; i > 0; i--) total += num[i] << (MAX_BITS - i);
    while (total != (1u << MAX_BITS)) {
        num[MAX_BITS]--;
        for (uint32_t i = MAX_BITS - 1; i > 0; i--)
            if (num[i]) { num[i]--; num[i + 1] += 2; break; }
        total--;
    }
    int j = n;
    for (uint32_t i = 1; i <= MAX_BITS; i++)
        for (uint32_t l = num[i]; l > 0; l--) len[A[--j].sym] = (uint8_t)i;
}

// The code-length alphabet's code is one constant complete code, 13 symbols of 4 bits and 6 of 5 bits, and the lengths
// are written one by one, without the run codes 16 / 17 / 18.
PF_HD uint32_t cl_len(uint32_t s) { return (s == 0 || (s >= 3 && s <= 14)) ? 4 : 5; }
constexpr uint32_t DYN_HEADER_FIXED_BITS = 5 + 5 + 4 + 3 * N_CL;

// ---- the bit writer: values are ORed into a zeroed array of 32-bit words, least significant bit first
PF_HD void or_word(uint32_t* w, uint32_t v) {
#if defined(__HIP_DEVICE_COMPILE__)
    if (v) atomicOr(w, v);
#else
    *w |= v;
#endif
}
PF_HD void put_bits(uint32_t* words, uint32_t bitpos, uint64_t v, uint32_t nb) {      // nb <= 48
    if (!nb) return;
    const uint32_t wi = bitpos >> 5, sh = bitpos & 31;
    const uint64_t lo = v << sh;
    or_word(&words[wi], (uint32_t)lo);
    if (sh + nb > 32) or_word(&words[wi + 1], (uint32_t)(lo >> 32));
    if (sh + nb > 64) or_word(&words[wi + 2], (uint32_t)(v >> (64 - sh)));
}

// the dynamic block's header behind BFINAL / BTYPE: HLIT, HDIST, HCLEN, the code-length code, then all 286 + 30 lengths
PF_HD uint32_t put_dyn_header(uint32_t* words, uint32_t bitpos, const Codes& c) {
    const uint8_t order[N_CL] = {16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15};
    uint8_t cl[N_CL];
    uint16_t cc[N_CL];
    for (uint32_t s = 0; s < N_CL; s++) cl[s] = (uint8_t)cl_len(s);
    canonical_codes(cl, N_CL, cc);
    put_bits(words, bitpos, N_LL - 257, 5); bitpos += 5;
    put_bits(words, bitpos, N_D - 1, 5); bitpos += 5;
    put_bits(words, bitpos, N_CL - 4, 4); bitpos += 4;
    for (uint32_t i = 0; i < N_CL; i++) { put_bits(words, bitpos, cl[order[i]], 3); bitpos += 3; }
    for (uint32_t s = 0; s < N_LL; s++) { put_bits(words, bitpos, cc[c.ll_len[s]], cl[c.ll_len[s]]); bitpos += cl[c.ll_len[s]]; }
    for (uint32_t s = 0; s < N_D; s++) { put_bits(words, bitpos, cc[c.d_len[s]], cl[c.d_len[s]]); bitpos += cl[c.d_len[s]]; }
    return bitpos;
}

// the bits of one token under the block's codes
PF_HD uint32_t token_bits(uint32_t tok, const Codes& c, uint64_t* val) {
    if (!(tok >> 31)) { *val = c.ll_code[tok]; return c.ll_len[tok]; }
    uint32_t leb, lev, deb, dev;
    const uint32_t ls = len_sym(((tok >> 16) & 0xFF) + 3, &leb, &lev), ds = dist_sym(tok & 0x7FFF, &deb, &dev);
    uint64_t v = c.ll_code[ls];
    uint32_t nb = c.ll_len[ls];
    v |= (uint64_t)lev << nb; nb += leb;
    v |= (uint64_t)c.d_code[ds] << nb; nb += c.d_len[ds];
    v |= (uint64_t)dev << nb; nb += deb;
    *val = v;
    return nb;
}

// what a symbol contributes to the three sizes: {fixed, dynamic, header} bits
PF_HD void ll_sym_bits(uint32_t s, uint32_t f, const Codes& dyn, uint32_t out[3]) {
    const uint32_t e = s > 256 ? len_sym_extra(s) : 0;
    out[0] += f * (fixed_ll_len(s) + e); out[1] += f * (dyn.ll_len[s] + e); out[2] += cl_len(dyn.ll_len[s]);
}
PF_HD void d_sym_bits(uint32_t s, uint32_t f, const Codes& dyn, uint32_t out[3]) {
    const uint32_t e = dist_sym_extra(s);
    out[0] += f * (5 + e); out[1] += f * (dyn.d_len[s] + e); out[2] += cl_len(dyn.d_len[s]);
}

// The block type of a chunk of n bytes, by exact size: bits[] as summed above over all symbols.  *coded_bits: the block's
// bits from BFINAL to the end-of-block code.  The test hooks force a type; a forced type that would not fit the slot is
// stored all the same.
PF_HD Mode choose_mode(const uint32_t bits[3], uint32_t n, uint32_t flags, uint32_t* coded_bits) {
    const uint32_t fixed = 3 + bits[0], dyn = 3 + DYN_HEADER_FIXED_BITS + bits[2] + bits[1], stored = 8 * (5 + n);
    Mode m = STORED;
    uint32_t best = stored;
    if (flags & PF_GZ_FIXED_ONLY) { m = FIXED; best = fixed; }
    else if (flags & PF_GZ_DYNAMIC_ONLY) { m = DYNAMIC; best = dyn; }
    else {
        if (fixed < best) { m = FIXED; best = fixed; }
        if (dyn < best) { m = DYNAMIC; best = dyn; }
    }
    if (m != STORED && best > MAX_CODED_BITS) { m = STORED; best = stored; }
    *coded_bits = best;
    return m;
}
PF_HD uint32_t member_bytes(uint32_t coded_bits) { return MEMBER_HEAD + (coded_bits + 7) / 8 + MEMBER_TAIL; }

// ---- CRC32 (the gzip polynomial, reflected), bit by bit, and the combination of the CRCs of two neighbouring pieces
// by multiplication modulo the polynomial (zlib's crc32_combine in its multmodp / x2nmodp form)
constexpr uint32_t CRC_POLY = 0xEDB88320u;
PF_HD uint32_t crc32_bytes(const uint8_t* p, uint32_t n) {
    uint32_t c = 0xFFFFFFFFu;
    for (uint32_t i = 0; i < n; i++) {
        c ^= p[i];
        for (int k = 0; k < 8; k++) c = (c >> 1) ^ (CRC_POLY & (0u - (c & 1)));
    }
    return ~c;
}
PF_HD uint32_t crc_multmodp(uint32_t a, uint32_t b) {
    uint32_t p = 0;
    for (uint32_t m = 1u << 31; m; m >>= 1) {
        if (a & m) p ^= b;
        b = (b >> 1) ^ (CRC_POLY & (0u - (b & 1)));
    }
    return p;
}
PF_HD uint32_t crc_x8nmodp(uint32_t nbytes) {        // x^(8 nbytes) modulo the polynomial
    uint32_t sq = 1u << 30;                          // x^1
    for (int i = 0; i < 3; i++) sq = crc_multmodp(sq, sq);
    uint32_t p = 1u << 31;                           // x^0
    for (; nbytes; nbytes >>= 1) {
        if (nbytes & 1) p = crc_multmodp(sq, p);
        sq = crc_multmodp(sq, sq);
    }
    return p;
}
PF_HD uint32_t crc_combine(uint32_t crc1, uint32_t crc2, uint32_t len2) {
    return len2 ? crc_multmodp(crc_x8nmodp(len2), crc1) ^ crc2 : crc1;
}

// ---- the member's frame
PF_HD void put_member_head(uint32_t* words) {        // ID1 ID2 CM=8 FLG=0 MTIME=0 XFL=0 OS=255 (unknown)
    put_bits(words, 0, 0x00088B1Full, 32);
    put_bits(words, 32, 0, 32);
    put_bits(words, 64, 0xFF00u, 16);
}
PF_HD void put_member_tail(uint32_t* words, uint32_t coded_bits, uint32_t crc, uint32_t n) {
    const uint32_t at = 8 * (MEMBER_HEAD + (coded_bits + 7) / 8);
    put_bits(words, at, crc, 32);
    put_bits(words, at + 32, n, 32);
}

PF_HD uint32_t hash4(uint32_t w) { return (w * 2654435761u) >> (32 - HASH_BITS); }
// a candidate's match is taken from 4 bytes on; 3 bytes only when near (a far 3-byte match costs more than 3 literals).
// As long as a candidate comes from an equal hash4 of four bytes, the 3-byte clause never holds: two words that differ
// only in their top byte differ by d << 24, the odd multiplier keeps that product's top byte non-zero, so their hashes
// differ in their top 8 bits -- a candidate agrees in 0, 1, 2 or at least 4 bytes, and length symbol 257 is never
// emitted (tests/test_deflate_host_model.py checks both).  The clause is what a candidate from any other source would need.
PF_HD bool match_ok(uint32_t len, uint32_t dist) { return len >= 4 || (len == 3 && dist <= 4096); }

// ---- the serial host model: same chunking, same coder, one candidate per position from a hash table of the positions
// seen so far, greedy parse
inline void host_model_chunk(const uint8_t* text, uint32_t n, uint32_t flags, std::vector<uint8_t>& out) {
    std::vector<uint32_t> head(1u << HASH_BITS, 0), tokens;
    uint32_t ll_hist[288] = {0}, d_hist[32] = {0};
    auto insert = [&](uint32_t p) {
        if (p + 3 < n) head[hash4(text[p] | text[p + 1] << 8 | text[p + 2] << 16 | (uint32_t)text[p + 3] << 24)] = p + 1;
    };
    for (uint32_t p = 0; p < n;) {
        uint32_t len = 0, dist = 0;
        if (p + 3 < n && !(flags & PF_GZ_LITERALS_ONLY)) {
            const uint32_t cand = head[hash4(text[p] | text[p + 1] << 8 | text[p + 2] << 16 | (uint32_t)text[p + 3] << 24)];
            if (cand) {
                const uint32_t c = cand - 1, maxl = std::min(MAX_MATCH, n - p);
                uint32_t l = 0;
                while (l < maxl && text[c + l] == text[p + l]) l++;
                if (match_ok(l, p - c)) { len = l; dist = p - c; }
            }
        }
        if (len) {
            uint32_t eb, ev;
            tokens.push_back(match_token(len, dist));
            ll_hist[len_sym(len, &eb, &ev)]++; d_hist[dist_sym(dist - 1, &eb, &ev)]++;
            for (uint32_t i = 0; i < len; i++) insert(p + i);
            p += len;
        } else {
            tokens.push_back(text[p]); ll_hist[text[p]]++;
            insert(p); p++;
        }
    }
    ll_hist[256] = 1;
    // the dynamic codes from the histograms
    Codes dyn{}, use{};
    auto lengths = [](const uint32_t* hist, uint32_t nsym, uint8_t* len) {
        std::vector<SymFreq> A;
        for (uint32_t s = 0; s < nsym; s++) if (hist[s]) A.push_back({hist[s], s});
        std::sort(A.begin(), A.end(), [](const SymFreq& x, const SymFreq& y) { return x.key != y.key ? x.key < y.key : x.sym < y.sym; });
        build_lengths(A.data(), (int)A.size(), len);
    };
    lengths(ll_hist, N_LL, dyn.ll_len);
    lengths(d_hist, N_D, dyn.d_len);
    canonical_codes(dyn.ll_len, N_LL, dyn.ll_code);
    canonical_codes(dyn.d_len, N_D, dyn.d_code);
    uint32_t bits[3] = {0, 0, 0}, coded = 0;
    for (uint32_t s = 0; s < N_LL; s++) ll_sym_bits(s, ll_hist[s], dyn, bits);
    for (uint32_t s = 0; s < N_D; s++) d_sym_bits(s, d_hist[s], dyn, bits);
    const Mode mode = choose_mode(bits, n, flags, &coded);
    // the chunk's CRC as the kernel makes it: pieces of CRC_SUB bytes, combined
    uint32_t crc = 0;
    for (uint32_t at = 0; at < n; at += CRC_SUB) {
        const uint32_t m = std::min(CRC_SUB, n - at);
        crc = at ? crc_combine(crc, crc32_bytes(text + at, m), m) : crc32_bytes(text, m);
    }
    std::vector<uint32_t> words(SLOT_WORDS, 0);
    put_member_head(words.data());
    uint32_t at = 8 * MEMBER_HEAD;
    if (mode == STORED) {
        put_bits(words.data(), at, 1, 8);
        put_bits(words.data(), at + 8, n | (uint64_t)(~n & 0xFFFF) << 16, 32);
        for (uint32_t i = 0; i < n; i++) put_bits(words.data(), at + 40 + 8 * i, text[i], 8);
    } else {
        put_bits(words.data(), at, 1 | (uint32_t)mode << 1, 3); at += 3;
        if (mode == DYNAMIC) { use = dyn; at = put_dyn_header(words.data(), at, use); }
        else {
            for (uint32_t s = 0; s < 288; s++) { use.ll_len[s] = (uint8_t)fixed_ll_len(s); use.ll_code[s] = (uint16_t)fixed_ll_code(s); }
            for (uint32_t s = 0; s < 32; s++) { use.d_len[s] = 5; use.d_code[s] = (uint16_t)bit_reverse(s, 5); }
        }
        for (uint32_t t : tokens) { uint64_t v; const uint32_t nb = token_bits(t, use, &v); put_bits(words.data(), at, v, nb); at += nb; }
        put_bits(words.data(), at, use.ll_code[256], use.ll_len[256]); at += use.ll_len[256];
        if (at != 8 * MEMBER_HEAD + coded) { out.clear(); return; }       // the size that chose the mode must be exact
    }
    put_member_tail(words.data(), coded, crc, n);
    const uint32_t nbytes = member_bytes(coded);
    for (uint32_t i = 0; i < nbytes; i++) out.push_back((uint8_t)(words[i >> 2] >> (8 * (i & 3))));
}

// the members of `data`; false: a chunk's size did not come out as counted (a bug)
inline bool host_model(const uint8_t* data, uint64_t n, uint32_t flags, std::vector<uint8_t>& out) {
    out.clear();
    for (uint64_t at = 0; at < n; at += CHUNK) {
        std::vector<uint8_t> one;
        host_model_chunk(data + at, (uint32_t)std::min<uint64_t>(CHUNK, n - at), flags, one);
        if (one.empty()) return false;
        out.insert(out.end(), one.begin(), one.end());
    }
    return true;
}

}  // namespace pfgz

#if defined(__HIPCC__)
#include "pf_buf.h"
// The device encoder: its buffers (worst-case slots, member sizes and offsets, the token streams of the resident
// workgroups, append cursors and their pinned read-backs) and the launches.  One per context; every call is
// stream-ordered on the stream given.
struct PfGzEncoder {
    static constexpr uint64_t BLOCK = 64ull << 20;       // text bytes per launch: the product's block size
    // one append cursor per text that may be on its way at once: a render's two texts, the stream's two blocks
    enum Cursor { RENDER_KMERS_TO_HASHES, RENDER_HASHES_TO_PATTERNS, STREAM_BLOCK0, STREAM_BLOCK1, N_CURSORS };
    DevBuf slots, sizes, offs, tokens, cursors;
    PinBuf pin; uint64_t caps[N_CURSORS] = {};           // per cursor: its value read back, the bytes its last encode's members may take
    uint32_t grid_cap = 0;                               // resident workgroups the token streams are sized for
    static uint64_t chunks(uint64_t n) { return (n + pfgz::CHUNK - 1) / pfgz::CHUNK; }
    static uint64_t bound(uint64_t n) { return chunks(n) * pfgz::SLOT_BYTES; }       // of the members of n bytes of text
    uint64_t device_bytes() const { return slots.cap + sizes.cap + offs.cap + tokens.cap + cursors.cap; }
    int ensure(int n_cu);
    // On `st`: cursor w back to zero, the members of text[0 .. n) (device memory) written from `members` on, which holds
    // cap bytes, and the cursor -- their size -- on its way into w's pinned word.  t0 / t1, where given, are recorded
    // around the cursor's reset and the launches.
    int encode(hipStream_t st, Cursor w, const char* text, uint64_t n, uint32_t flags, char* members, uint64_t cap,
               hipEvent_t t0 = nullptr, hipEvent_t t1 = nullptr);
    // once the caller has synchronised with that encode: the bytes of its members; PF_ERR_STATE if they exceed its cap
    int member_bytes(Cursor w, uint64_t* z) const;
};
#endif
