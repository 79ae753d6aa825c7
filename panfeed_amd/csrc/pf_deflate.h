// pf_deflate.h -- internal: gzip (RFC 1952) members with deflate (RFC 1951) blocks, written and read by the GPU.
//
// The format logic is written once, as host+device functions: length / distance symbols and their extra bits, the fixed
// codes, the length-limited code builder, the canonical code assignment, the dynamic block header, the bit writer, CRC32
// and its combination.  pf_deflate.hip runs them in the encoder kernel; host_model() below runs the same functions
// serially, with a plain one-candidate greedy matcher, so that the format can be tested without a GPU.
//
// The decoder's side stands behind the encoder's: bit reader, decode tables, the dynamic header with its run codes, stored
// blocks, several blocks per member -- inflate_blocks(), run by the decoder kernel and by host_inflate_model().
//
// Container: the text is cut into chunks of CHUNK bytes; every chunk becomes one complete gzip member holding one final
// deflate block -- stored, fixed or dynamic, whichever is smallest by exact bit count.  No match reaches before its chunk.
// A text made of segments (several files' bodies, one behind the other) is cut segment by segment, each from its own
// start, so that no member holds bytes of two segments: chunk_plan() below.
//
// BGZF (SAM specification 4.1; what bgzip and htslib write) is the second container, read and written: a chain of
// independent gzip members of at most 65 536 bytes, of at most 65 536 bytes of text each, whose 18-byte head carries the
// member's size -- FLG = 4, XLEN = 6, the one extra subfield 'B' 'C' 02 00 BSIZE, BSIZE = the member's size - 1 -- and that
// ends with a 28-byte member of no text.  Only that head is taken as BGZF: any other extra field (XLEN != 6, another or a
// second subfield) is "not taken", and such a file goes the host's way.  A file is one container or the other: a head of the
// other kind inside a chain is refused.  list_members_bgzf() walks the BSIZE chain; the encoder's members become BGZF under
// PF_GZ_BGZF by 8 more bytes of head each (bgzf_frame), applied where the members are sized and gathered -- the end marker
// is the host writer's to append.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "../../include/panfeed_hip.h"

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define PF_HD __host__ __device__ inline
#define PF_HD_M __host__ __device__
#else
#define PF_HD inline
#define PF_HD_M
#endif

#include <string.h>

#include <algorithm>
#include <functional>
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
// BGZF: the head with its BC subfield, what it adds to the plain head, the most a member and its text may be
constexpr uint32_t BGZF_HEAD = 18, BGZF_EXTRA = BGZF_HEAD - MEMBER_HEAD, BGZF_MAX_MEMBER = 65536, BGZF_MAX_TEXT = 65536;
// the largest member the encoder makes is SLOT_BYTES - 16 (MAX_CODED_BITS; a stored one is CHUNK + 23): framed, it still
// fits its slot's share of every bound and BSIZE
static_assert(SLOT_BYTES - 16 + BGZF_EXTRA <= SLOT_BYTES, "a framed member stays within the per-chunk bound");
static_assert(SLOT_BYTES - 16 + BGZF_EXTRA <= BGZF_MAX_MEMBER, "a framed member's size - 1 fits BSIZE");
static_assert(CHUNK + 5 + MEMBER_HEAD + MEMBER_TAIL <= SLOT_BYTES - 16, "a stored member is no larger than a coded one may be");

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

// BGZF: byte i (< BGZF_HEAD) of the head of a member of `framed` bytes whose plain head is plain[0 .. MEMBER_HEAD): the
// plain head with FLG = 4, then XLEN = 6, 'B' 'C', SLEN = 2, BSIZE = framed - 1
PF_HD uint8_t bgzf_head_byte(const uint8_t* plain, uint32_t framed, uint32_t i) {
    const uint64_t extra = 0x0000000243420006ull | (uint64_t)(framed - 1) << 48;      // (bytes 06 00 'B' 'C' 02 00 lo hi, in a register)
    return i == 3 ? 4 : i < MEMBER_HEAD ? plain[i] : (uint8_t)(extra >> (8 * (i - MEMBER_HEAD)));
}
// the end-of-file member (SAM specification 4.1): an empty fixed block under the head as bgzip writes it
constexpr uint32_t BGZF_EOF_BYTES = 28;
inline const uint8_t* bgzf_eof() {
    static const uint8_t eof[BGZF_EOF_BYTES] = {0x1F, 0x8B, 8, 4, 0, 0, 0, 0, 0, 0xFF, 6, 0, 'B', 'C', 2, 0, 0x1B, 0, 3, 0, 0, 0, 0, 0, 0, 0, 0, 0};
    return eof;
}

PF_HD uint32_t hash4(uint32_t w) { return (w * 2654435761u) >> (32 - HASH_BITS); }
// a candidate's match is taken from 4 bytes on; 3 bytes only when near (a far 3-byte match costs more than 3 literals).
// As long as a candidate comes from an equal hash4 of four bytes, the 3-byte clause never holds: two words that differ
// only in their top byte differ by d << 24, the odd multiplier keeps that product's top byte non-zero, so their hashes
// differ in their top 8 bits -- a candidate agrees in 0, 1, 2 or at least 4 bytes, and length symbol 257 is never
// emitted (tests/test_deflate_host_model.py checks both).  The clause is what a candidate from any other source would need.
PF_HD bool match_ok(uint32_t len, uint32_t dist) { return len >= 4 || (len == 3 && dist <= 4096); }

// ---- the deeper search (PF_GZ_DEEP), written once for the kernel and the host model.  It depends on the chunk's text alone.
// A position p has up to two candidates.  A is the hash table's, as without the flag (the kernel's and the host model's
// tables differ, as they do there).  B is the same column of the row before: with s = 1 + the last '\n' before p (0: none,
// and then no B) and r = 1 + the last '\n' before s - 1 (0: none), B = r + (p - s), taken only if it lies before the
// previous row's '\n', B < s - 1.  A chunk that starts inside a row gets a misaligned B for its second row, no more.
// These texts' rows repeat the row before them column by column, and A is usually a "0\t0\t" a few bytes back.
PF_HD uint32_t match_run(const uint8_t* text, uint32_t c, uint32_t p, uint32_t maxl) {      // c < p, p + maxl within the text
    uint32_t l = 0;
    while (l + 4 <= maxl) {
        uint32_t x, y;
        __builtin_memcpy(&x, text + c + l, 4);
        __builtin_memcpy(&y, text + p + l, 4);
        if (x != y) break;
        l += 4;
    }
    while (l < maxl && text[c + l] == text[p + l]) l++;
    return l;
}
PF_HD bool row_candidate(uint32_t p, uint32_t s, uint32_t r, uint32_t* b) {
    if (!s) return false;
    *b = r + (p - s);
    return *b + 1 < s;
}
// L(p), D(p): both candidates extended to MAX_MATCH, the longer taken, on a tie the nearer, accepted through match_ok --
// B agrees in any number of bytes, so the 3-byte clause is reachable here.  cand_a: 1 + A, or 0 for none.  Defined for
// every p < n, covered by a match or not.  *len == 0: no match.
PF_HD void deep_length(const uint8_t* text, uint32_t n, uint32_t p, uint32_t cand_a, uint32_t s, uint32_t r, uint32_t* len, uint32_t* dist) {
    const uint32_t maxl = n - p < MAX_MATCH ? n - p : MAX_MATCH;
    uint32_t l = 0, d = 0, b = 0;
    if (cand_a) { l = match_run(text, cand_a - 1, p, maxl); d = p - (cand_a - 1); }
    if (row_candidate(p, s, r, &b) && b + 1 != cand_a) {
        const uint32_t lb = match_run(text, b, p, maxl), db = p - b;
        if (lb > l || (lb == l && db < d)) { l = lb; d = db; }
    }
    const bool ok = match_ok(l, d);
    *len = ok ? l : 0; *dist = ok ? d : 0;
}
// the parse at a token start q with L(q) > 0: one literal in place of the match when the next position's match is longer
PF_HD bool deep_defers(uint32_t len_q, uint32_t len_next) { return len_next > len_q; }

// ---- the serial host model: same chunking, same coder, one candidate per position from a hash table of the positions
// seen so far, greedy parse; under PF_GZ_DEEP the rule above, with that table's candidate as A
inline void host_model_chunk(const uint8_t* text, uint32_t n, uint32_t flags, std::vector<uint8_t>& out) {
    std::vector<uint32_t> head(1u << HASH_BITS, 0), tokens;
    uint32_t ll_hist[288] = {0}, d_hist[32] = {0};
    auto insert = [&](uint32_t p) {
        if (p + 3 < n) head[hash4(text[p] | text[p + 1] << 8 | text[p + 2] << 16 | (uint32_t)text[p + 3] << 24)] = p + 1;
    };
    const bool deep = (flags & PF_GZ_DEEP) && !(flags & PF_GZ_LITERALS_ONLY);
    if (deep) {
        // candidate A of every position (the last position before it with its hash: every position is inserted, so the
        // table's state does not depend on the parse) and its row starts, then the lazy parse over L(p), D(p)
        std::vector<uint32_t> cand(n, 0), rs(n), rr(n);
        for (uint32_t p = 0, s = 0, r = 0; p < n; p++) {
            if (p + 3 < n) {
                uint32_t& e = head[hash4(text[p] | text[p + 1] << 8 | text[p + 2] << 16 | (uint32_t)text[p + 3] << 24)];
                cand[p] = e; e = p + 1;
            }
            rs[p] = s; rr[p] = r;
            if (text[p] == '\n') { r = s; s = p + 1; }
        }
        for (uint32_t q = 0; q < n;) {
            uint32_t len, dist, len1 = 0, dist1;
            deep_length(text, n, q, cand[q], rs[q], rr[q], &len, &dist);
            if (len && q + 1 < n) deep_length(text, n, q + 1, cand[q + 1], rs[q + 1], rr[q + 1], &len1, &dist1);
            if (len && !deep_defers(len, len1)) {
                uint32_t eb, ev;
                tokens.push_back(match_token(len, dist));
                ll_hist[len_sym(len, &eb, &ev)]++; d_hist[dist_sym(dist - 1, &eb, &ev)]++;
                q += len;
            } else {
                tokens.push_back(text[q]); ll_hist[text[q]]++;
                q++;
            }
        }
    } else for (uint32_t p = 0; p < n;) {         // level 1, or no match at all (PF_GZ_LITERALS_ONLY)
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
    auto byte = [&](uint32_t i) { return (uint8_t)(words[i >> 2] >> (8 * (i & 3))); };
    uint32_t from = 0;
    if (flags & PF_GZ_BGZF) {                // the same member behind the longer head, as gz_gather_kernel frames it
        uint8_t plain[MEMBER_HEAD];
        for (uint32_t i = 0; i < MEMBER_HEAD; i++) plain[i] = byte(i);
        for (uint32_t i = 0; i < BGZF_HEAD; i++) out.push_back(bgzf_head_byte(plain, nbytes + BGZF_EXTRA, i));
        from = MEMBER_HEAD;
    }
    for (uint32_t i = from; i < nbytes; i++) out.push_back(byte(i));
}

// ---- the chunk plan.  A text may be cut into segments (the per-cluster files' bodies, one behind the other): a member
// never holds bytes of two segments.  Every segment is cut into chunks of CHUNK bytes counted from its own start, its
// last one shorter; an empty segment has no chunk.  One segment over the whole text gives the plain container above.
struct ChunkDesc { uint64_t start; uint32_t len, segment; };      // text offset, bytes (1 .. CHUNK), index into seg_end
static_assert(sizeof(ChunkDesc) == 16, "the kernels read the plan as it stands in host memory");
// the chunks of text[0 .. n) under segment ends seg_end[0 .. n_seg): non-decreasing offsets, the last one n (no segment:
// no text).  false: the ends are not such a list.
inline bool chunk_plan(const uint64_t* seg_end, uint64_t n_seg, uint64_t n, std::vector<ChunkDesc>& plan) {
    plan.clear();
    if (n_seg > 0xFFFFFFFFull || (n_seg ? seg_end[n_seg - 1] != n : n != 0)) return false;
    uint64_t at = 0;
    for (uint64_t s = 0; s < n_seg; s++) {
        if (seg_end[s] < at) return false;
        for (; at < seg_end[s]; at += std::min<uint64_t>(CHUNK, seg_end[s] - at))
            plan.push_back(ChunkDesc{at, (uint32_t)std::min<uint64_t>(CHUNK, seg_end[s] - at), (uint32_t)s});
    }
    return true;
}
inline uint64_t plan_chunks(uint64_t n, uint64_t n_seg) { return (n + CHUNK - 1) / CHUNK + n_seg; }     // never fewer than the plan holds

// The members of `data` under a plan, and behind which byte of them every segment's members end (member_end[n_seg],
// may be null).  0: done; 1: the ends are no plan; 2: a chunk's size did not come out as counted (a bug).
inline int host_model_segments(const uint8_t* data, uint64_t n, const uint64_t* seg_end, uint64_t n_seg, uint32_t flags,
                               std::vector<uint8_t>& out, uint64_t* member_end) {
    out.clear();
    std::vector<ChunkDesc> plan;
    if (!chunk_plan(seg_end, n_seg, n, plan)) return 1;
    size_t c = 0;
    for (uint64_t s = 0; s < n_seg; s++) {
        for (; c < plan.size() && plan[c].segment == s; c++) {
            std::vector<uint8_t> one;
            host_model_chunk(data + plan[c].start, plan[c].len, flags, one);
            if (one.empty()) return 2;
            out.insert(out.end(), one.begin(), one.end());
        }
        if (member_end) member_end[s] = out.size();
    }
    return 0;
}

// the members of `data`; false: a chunk's size did not come out as counted (a bug)
inline bool host_model(const uint8_t* data, uint64_t n, uint32_t flags, std::vector<uint8_t>& out) {
    const uint64_t end = n;
    return host_model_segments(data, n, &end, n ? 1 : 0, flags, out, nullptr) == 0;
}

// ---------------------------------------------------------------------------------------------------------------------
// The decoder's side: all of RFC 1951 for a member of at most CHUNK bytes of text and SLOT_BYTES compressed bytes.
// inflate_blocks() below is the one place that reads a deflate stream; it is a template over the sink that takes the
// tokens (Out): pf_deflate.hip's sink spreads a match copy over a wave, host_inflate_model()'s writes byte by byte.
// Every bound is checked here, before the sink is called: no read past the payload's last byte, no write past ISIZE,
// no distance before the member's first byte, no symbol 286 / 287, no distance symbol 30 / 31.  Every loop iteration
// takes at least one input bit or gives at least one output byte, so any stream ends its decode.
// "bad code" against "truncated": decode_sym looks at MAX_BITS bits at once.  A bit pattern that no code has is
// INF_BAD_CODE where at least MAX_BITS bits of payload are left from its first bit on (two or more whole bytes behind the
// byte it starts in always are); within the payload's last MAX_BITS - 1 bits it cannot be told from a longer code cut
// short and is INF_TRUNCATED -- also for a lone distance code's unused bit and for a block without distance codes, where
// no longer code exists.  Either way the member is not taken (tests/inflate_edges.py pins both answers).
enum InfStatus : uint32_t {
    INF_OK = 0,
    INF_NOT_DECODED,        // (another member of the call was refused before this one was looked at)
    INF_BAD_HEAD,           // not ID1 ID2 CM=8 FLG=0 (BGZF: not FLG=4 with the one BC subfield), or a member shorter than its frame
    INF_TOO_LARGE,          // ISIZE over CHUNK or more than SLOT_BYTES compressed (BGZF: ISIZE over 65 536)
    INF_TRUNCATED,          // the payload ended inside a block (BGZF: the file ended inside a member)
    INF_BAD_BLOCK_TYPE,     // BTYPE 3
    INF_BAD_STORED,         // LEN != ~NLEN
    INF_BAD_CODE,           // an over-subscribed or incomplete code, no end-of-block code, a bit pattern without a symbol
    INF_BAD_LENGTHS,        // the dynamic header: HLIT / HDIST out of range, a repeat without a length before it or past the end
    INF_BAD_SYMBOL,         // length symbol 286 / 287, distance symbol 30 / 31
    INF_BAD_DISTANCE,       // a match that starts before the member's first byte
    INF_TOO_MUCH_TEXT,      // the stream gives more than ISIZE bytes
    INF_TOO_LITTLE_TEXT,    // the final block ended before ISIZE bytes
    INF_NOT_AT_TAIL,        // the final block ended before the member's tail
    INF_BAD_CRC,
    INF_N_STATUS
};
inline const char* inf_status_name(uint32_t s) {
    static const char* const names[INF_N_STATUS] = {"ok", "not decoded", "bad header", "too large", "truncated", "block type 3",
        "stored LEN / NLEN", "bad code", "bad code lengths", "bad symbol", "distance before the start", "more text than ISIZE",
        "less text than ISIZE", "ends before its tail", "CRC32 differs"};
    return s < INF_N_STATUS ? names[s] : "?";
}

// bits from p[0 .. n), least significant first; a read past the end gives zeros and sets `over`
struct BitReader {
    const uint8_t* p; uint32_t n, pos; uint64_t buf; uint32_t cnt; bool over;
};
PF_HD BitReader bit_reader(const uint8_t* p, uint32_t n) { return BitReader{p, n, 0, 0, 0, false}; }
PF_HD void refill(BitReader& r) {
    while (r.cnt <= 56 && r.pos < r.n) { r.buf |= (uint64_t)r.p[r.pos++] << r.cnt; r.cnt += 8; }
}
PF_HD uint32_t take_bits(BitReader& r, uint32_t nb) {            // nb <= 32
    if (r.cnt < nb) {
        refill(r);
        if (r.cnt < nb) { r.over = true; r.buf = 0; r.cnt = 0; return 0; }
    }
    const uint32_t v = (uint32_t)(r.buf & ((1ull << nb) - 1));
    r.buf >>= nb; r.cnt -= nb;
    return v;
}
PF_HD uint32_t byte_pos(const BitReader& r) { return r.pos - (r.cnt >> 3); }     // of the first byte no bit was taken from

// symbol -> first length / distance (the extra bits: len_sym_extra, dist_sym_extra)
PF_HD uint32_t len_base(uint32_t sym) {
    if (sym < 265) return sym - 254;
    if (sym == 285) return 258;
    const uint32_t e = (sym - 261) / 4;
    return 3 + ((4 + (sym - 261) % 4) << e);
}
PF_HD uint32_t dist_base(uint32_t sym) { return sym < 4 ? sym + 1 : 1 + ((2 + (sym & 1)) << (sym / 2 - 1)); }

// a canonical code for decoding: count[b] = codes of b bits, sym[] = the coded symbols by (length, symbol)
struct DecodeTables {
    uint16_t ll_count[MAX_BITS + 1], ll_sym[288], d_count[MAX_BITS + 1], d_sym[32];
    uint8_t lens[288 + 32];
};
struct CodeCounts { uint32_t c[MAX_BITS + 1]; };     // a block's counts, kept by the decode loop in registers

// Tables of the code with these lengths.  INF_BAD_CODE for an over-subscribed code and for an incomplete one, except
// the two incomplete codes RFC 1951 allows where `allow_one` says so: one symbol of one bit, and no symbol at all (a
// block without matches; using such a code is an error where it is used).
PF_HD uint32_t build_decode(const uint8_t* len, uint32_t n, uint16_t* count, uint16_t* sym, bool allow_one) {
    uint32_t cnt[MAX_BITS + 1], offs[MAX_BITS + 2];
    for (uint32_t b = 0; b <= MAX_BITS; b++) cnt[b] = 0;
    for (uint32_t s = 0; s < n; s++) cnt[len[s] & 15]++;
    int32_t left = 1;
    for (uint32_t b = 1; b <= MAX_BITS; b++) {
        left = left * 2 - (int32_t)cnt[b];
        if (left < 0) return INF_BAD_CODE;
    }
    const uint32_t coded = n - cnt[0];
    if (left > 0 && !(allow_one && (coded == 0 || (coded == 1 && cnt[1] == 1)))) return INF_BAD_CODE;
    offs[1] = 0;
    for (uint32_t b = 1; b <= MAX_BITS; b++) offs[b + 1] = offs[b] + cnt[b];
    for (uint32_t s = 0; s < n; s++) if (len[s] & 15) sym[offs[len[s] & 15]++] = (uint16_t)s;
    count[0] = 0;
    for (uint32_t b = 1; b <= MAX_BITS; b++) count[b] = (uint16_t)cnt[b];
    return INF_OK;
}
PF_HD CodeCounts load_counts(const uint16_t* count) {
    CodeCounts k;
    for (uint32_t b = 0; b <= MAX_BITS; b++) k.c[b] = count[b];
    return k;
}
// the next symbol, or -1: no code of up to MAX_BITS bits starts this way, or the payload ended (r.over)
PF_HD int32_t decode_sym(BitReader& r, const CodeCounts& k, const uint16_t* sym) {
    if (r.cnt < MAX_BITS) refill(r);
    uint32_t bits = (uint32_t)r.buf, code = 0, first = 0, index = 0;
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
    for (uint32_t b = 1; b <= MAX_BITS; b++) {
        code |= bits & 1; bits >>= 1;
        const uint32_t c = k.c[b];
        if (code < first + c) {
            if (b > r.cnt) { r.over = true; r.buf = 0; r.cnt = 0; return -1; }
            r.buf >>= b; r.cnt -= b;
            return sym[index + (code - first)];
        }
        index += c; first = (first + c) << 1; code <<= 1;
    }
    if (r.cnt < MAX_BITS) r.over = true;
    return -1;
}

PF_HD uint32_t fixed_tables(DecodeTables& T) {
    for (uint32_t s = 0; s < 288; s++) T.lens[s] = (uint8_t)fixed_ll_len(s);
    for (uint32_t s = 0; s < 32; s++) T.lens[288 + s] = 5;
    const uint32_t a = build_decode(T.lens, 288, T.ll_count, T.ll_sym, false);
    return a ? a : build_decode(T.lens + 288, 32, T.d_count, T.d_sym, false);
}

// the dynamic header behind BTYPE: HLIT, HDIST, HCLEN, the code-length code, the lengths with the run codes 16 / 17 / 18
// (every caller reads the header, so that the reader's state stays the same for all; only the leader writes T)
PF_HD uint32_t dynamic_tables(BitReader& r, DecodeTables& T, bool leader) {
    const uint8_t order[N_CL] = {16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15};
    const uint32_t hlit = take_bits(r, 5) + 257, hdist = take_bits(r, 5) + 1, hclen = take_bits(r, 4) + 4;
    if (r.over) return INF_TRUNCATED;
    if (hlit > N_LL || hdist > N_D) return INF_BAD_LENGTHS;
    uint8_t cl[N_CL];
    for (uint32_t i = 0; i < N_CL; i++) cl[i] = 0;
    for (uint32_t i = 0; i < hclen; i++) cl[order[i]] = (uint8_t)take_bits(r, 3);
    if (r.over) return INF_TRUNCATED;
    uint16_t cl_count[MAX_BITS + 1], cl_sym[N_CL];
    if (build_decode(cl, N_CL, cl_count, cl_sym, false)) return INF_BAD_CODE;
    const CodeCounts k = load_counts(cl_count);
    const uint32_t total = hlit + hdist;
    uint32_t prev = 0;
    for (uint32_t i = 0; i < total;) {
        const int32_t s = decode_sym(r, k, cl_sym);
        if (s < 0) return r.over ? INF_TRUNCATED : INF_BAD_CODE;
        if (s < 16) { if (leader) T.lens[i] = (uint8_t)s; i++; prev = (uint32_t)s; continue; }
        uint32_t rep, v = 0;
        if (s == 16) { if (i == 0) return INF_BAD_LENGTHS; v = prev; rep = 3 + take_bits(r, 2); }
        else if (s == 17) rep = 3 + take_bits(r, 3);
        else rep = 11 + take_bits(r, 7);
        if (r.over) return INF_TRUNCATED;
        if (i + rep > total) return INF_BAD_LENGTHS;
        if (leader) for (uint32_t j = 0; j < rep; j++) T.lens[i + j] = (uint8_t)v;
        i += rep; prev = v;
    }
    if (!leader) return INF_OK;
    if (T.lens[256] == 0) return INF_BAD_CODE;                     // a block cannot end without this code
    // (the distance lengths first: they stand behind the literal / length ones, whose table is not lens[])
    const uint32_t a = build_decode(T.lens + hlit, hdist, T.d_count, T.d_sym, true);
    return a ? a : build_decode(T.lens, hlit, T.ll_count, T.ll_sym, true);
}

// The blocks of a deflate stream from the reader's place on, into a sink.  Out has
//   bool leader()                      whether this caller writes the shared tables (the device: one lane of the wave)
//   void sync()                        after the leader's writes, before anyone reads them
//   uint32_t share(v)                  the leader's v
//   void literal(o, byte)              text[o] = byte
//   void copy(o, dist, len)            text[o + i] = text[o - dist + i], i = 0 .. len - 1, as if byte by byte
//   void stored(o, src, len)           text[o + i] = src[i]
// and Stop has  bool at(uint64_t bit): asked behind every block that is not the final one, with the bit the next block
// starts at; true ends the run there.  `hist`: the bytes of text that stand before o = 0 (a match may reach that far back);
// `cap`: the most bytes the run may give.  *produced: the bytes given.  INF_OK: the run ended behind a block, *why says
// which way (RUN_AT_STOP / RUN_FINAL) and the reader stands behind that block's last bit.
enum RunEnd : uint32_t { RUN_NONE = 0, RUN_AT_STOP, RUN_FINAL };
struct NoStop { PF_HD_M bool at(uint64_t) { return false; } };
PF_HD uint64_t bit_pos(const BitReader& r) { return (uint64_t)r.pos * 8 - r.cnt; }     // of the next bit to take
// a reader of p[0 .. n) that stands at bit `bit` (< 8 n)
PF_HD BitReader bit_reader_at(const uint8_t* p, uint32_t n, uint64_t bit) {
    BitReader r{p, n, (uint32_t)(bit >> 3), 0, 0, false};
    (void)take_bits(r, (uint32_t)(bit & 7));
    return r;
}
template <class Out, class Stop>
PF_HD uint32_t inflate_run(BitReader& r, uint32_t hist, uint32_t cap, DecodeTables& T, Out& out, Stop& stop, uint32_t* produced, uint32_t* why) {
    const uint8_t* const p = r.p;
    const uint32_t n = r.n;
    uint32_t o = 0, bfinal = 0;
    *produced = 0; *why = RUN_NONE;
    for (;;) {
        bfinal = take_bits(r, 1);
        const uint32_t btype = take_bits(r, 2);
        if (r.over) return INF_TRUNCATED;
        if (btype == 3) return INF_BAD_BLOCK_TYPE;
        if (btype == 0) {
            (void)take_bits(r, r.cnt & 7);
            const uint32_t len = take_bits(r, 16), nlen = take_bits(r, 16);
            if (r.over) return INF_TRUNCATED;
            if (len != (~nlen & 0xFFFFu)) return INF_BAD_STORED;
            const uint32_t at = byte_pos(r);
            if (len > n - at) return INF_TRUNCATED;
            if (len > cap - o) return INF_TOO_MUCH_TEXT;
            out.stored(o, p + at, len);
            o += len; *produced = o;
            r.pos = at + len; r.buf = 0; r.cnt = 0;
        } else {
            uint32_t st = INF_OK;
            if (btype == 1) { if (out.leader()) st = fixed_tables(T); }
            else st = dynamic_tables(r, T, out.leader());
            out.sync();
            st = out.share(st);                    // (every caller asks: the leader's lane must be there to answer)
            if (st) return st;
            const CodeCounts kl = load_counts(T.ll_count), kd = load_counts(T.d_count);
            for (;;) {
                const int32_t s = decode_sym(r, kl, T.ll_sym);
                if (s < 0) return r.over ? INF_TRUNCATED : INF_BAD_CODE;
                if (s < 256) {
                    if (o >= cap) return INF_TOO_MUCH_TEXT;
                    out.literal(o, (uint8_t)s);
                    o++; *produced = o;
                    continue;
                }
                if (s == 256) break;
                if (s >= (int32_t)N_LL) return INF_BAD_SYMBOL;
                const uint32_t len = len_base((uint32_t)s) + take_bits(r, len_sym_extra((uint32_t)s));
                const int32_t ds = decode_sym(r, kd, T.d_sym);
                if (ds < 0) return r.over ? INF_TRUNCATED : INF_BAD_CODE;
                if (ds >= (int32_t)N_D) return INF_BAD_SYMBOL;
                const uint32_t dist = dist_base((uint32_t)ds) + take_bits(r, dist_sym_extra((uint32_t)ds));
                if (r.over) return INF_TRUNCATED;
                if (dist > o && dist - o > hist) return INF_BAD_DISTANCE;
                if (len > cap - o) return INF_TOO_MUCH_TEXT;
                out.copy(o, dist, len);
                o += len; *produced = o;
            }
            out.sync();                    // (the next block's tables take this one's place)
        }
        if (bfinal) { *why = RUN_FINAL; return INF_OK; }
        if (stop.at(bit_pos(r))) { *why = RUN_AT_STOP; return INF_OK; }
    }
}

// The blocks of one member's payload, p[0 .. n), into a sink that holds at most `isize` bytes: the run from the payload's
// first bit to its final block.  INF_OK: that block ended with exactly isize bytes given and exactly at p + n.
template <class Out>
PF_HD uint32_t inflate_blocks(const uint8_t* p, uint32_t n, uint32_t isize, DecodeTables& T, Out& out, uint32_t* produced) {
    BitReader r = bit_reader(p, n);
    NoStop never;
    uint32_t why = RUN_NONE;
    const uint32_t st = inflate_run(r, 0, isize, T, out, never, produced, &why);
    if (st) return st;
    if (*produced != isize) return INF_TOO_LITTLE_TEXT;
    return byte_pos(r) == n ? INF_OK : INF_NOT_AT_TAIL;
}

// ---- where members start, without decoding: the first member's ID1 ID2 CM FLG MTIME are the signature, every place
// they stand at is a candidate, a member's tail is the 8 bytes before the next candidate (or the end).  XFL and OS are
// left out of the signature: a file of this project's starts with the header line's member, which zlib wrote with its
// own XFL and OS, and goes on with the device's (both write MTIME = 0).  Eight bytes: a false candidate inside compressed
// bytes comes once in 2^64 positions, and is refused by the checks of the member it cuts in two.
constexpr uint32_t MEMBER_SIG = 8;
struct MemberRef {
    uint64_t at;             // of the member's head in the bytes given
    uint32_t size, isize, crc, status;      // whole member's bytes; from its tail; INF_OK or why it is not taken
    uint32_t head = MEMBER_HEAD;            // the bytes in front of its payload: MEMBER_HEAD, or BGZF_HEAD
};
inline bool member_head_ok(const uint8_t* p, uint64_t n) { return n >= MEMBER_HEAD && p[0] == 0x1F && p[1] == 0x8B && p[2] == 8 && p[3] == 0; }
inline uint32_t le32(const uint8_t* p) { return p[0] | p[1] << 8 | p[2] << 16 | (uint32_t)p[3] << 24; }
// the members of p[0 .. n): those that end before another candidate, and with `last` the one that ends at n too.
// *consumed: the bytes of the members listed.  false: p does not start with a head this decoder takes.
inline bool list_members(const uint8_t* p, uint64_t n, bool last, std::vector<MemberRef>& out, uint64_t* consumed) {
    out.clear(); *consumed = 0;
    if (!n) return true;
    if (!member_head_ok(p, n)) return false;
    std::vector<uint64_t> starts(1, 0);
    for (uint64_t at = 1; at + MEMBER_HEAD <= n;) {
        const void* hit = memmem(p + at, (size_t)(n - at), p, MEMBER_SIG);
        if (!hit) break;
        at = (uint64_t)(static_cast<const uint8_t*>(hit) - p);
        starts.push_back(at);
        at++;
    }
    if (last) starts.push_back(n);
    for (size_t i = 0; i + 1 < starts.size(); i++) {
        MemberRef m{starts[i], 0, 0, 0, INF_OK};
        const uint64_t size = starts[i + 1] - starts[i];
        if (size < MEMBER_HEAD + MEMBER_TAIL) m.status = INF_BAD_HEAD;
        else if (size > SLOT_BYTES) m.status = INF_TOO_LARGE;
        else {
            m.size = (uint32_t)size;
            m.crc = le32(p + starts[i + 1] - 8); m.isize = le32(p + starts[i + 1] - 4);
            if (m.isize > CHUNK) m.status = INF_TOO_LARGE;
        }
        out.push_back(m);
    }
    *consumed = starts.back();
    return true;
}
inline int64_t first_refused(const std::vector<MemberRef>& ms) {
    for (size_t i = 0; i < ms.size(); i++) if (ms[i].status != INF_OK) return (int64_t)i;
    return -1;
}

// ---- BGZF: the same list by the BSIZE chain, no signature search.  A head is taken as BGZF only in the shape bgzip and
// htslib write it: FLG = 4, XLEN = 6, the single subfield BC of two bytes (MTIME, XFL and OS are free).
inline bool bgzf_head_ok(const uint8_t* p, uint64_t n) {
    return n >= BGZF_HEAD && p[0] == 0x1F && p[1] == 0x8B && p[2] == 8 && p[3] == 4 && p[10] == 6 && p[11] == 0 && p[12] == 'B' &&
           p[13] == 'C' && p[14] == 2 && p[15] == 0;
}
// The members of p[0 .. n) in the order of the chain.  A member that runs past n ends the list when !last (the caller
// reads on) and is INF_TRUNCATED with `last`; a head in the chain that is no BGZF head, or a BSIZE too small for a frame,
// is INF_BAD_HEAD; an ISIZE over BGZF_MAX_TEXT is INF_TOO_LARGE.  The list ends with the first member refused.  The end
// marker is a member of no text like any other, and a file without it is taken.  *consumed: the bytes of the members
// listed as taken.  false: p does not start with a BGZF head (with !last and fewer bytes than a head: an empty list).
inline bool list_members_bgzf(const uint8_t* p, uint64_t n, bool last, std::vector<MemberRef>& out, uint64_t* consumed) {
    out.clear(); *consumed = 0;
    uint64_t at = 0;
    while (at < n) {
        MemberRef m{at, 0, 0, 0, INF_OK, BGZF_HEAD};
        const uint64_t left = n - at;
        if (left < BGZF_HEAD && !last) break;
        if (!bgzf_head_ok(p + at, left)) {
            if (at == 0) return false;
            m.status = left < BGZF_HEAD ? INF_TRUNCATED : INF_BAD_HEAD;
        } else {
            const uint32_t size = (p[at + 16] | (uint32_t)p[at + 17] << 8) + 1;
            if (size < BGZF_HEAD + MEMBER_TAIL) m.status = INF_BAD_HEAD;
            else if (size > left) {
                if (!last) break;
                m.status = INF_TRUNCATED;
            } else {
                m.size = size;
                m.crc = le32(p + at + size - 8); m.isize = le32(p + at + size - 4);
                if (m.isize > BGZF_MAX_TEXT) m.status = INF_TOO_LARGE;
            }
        }
        out.push_back(m);
        if (m.status != INF_OK) break;
        at += m.size;
    }
    *consumed = at;
    return true;
}

struct HostSink {
    uint8_t* w;
    bool leader() const { return true; }
    void sync() {}
    uint32_t share(uint32_t v) const { return v; }
    void literal(uint32_t o, uint8_t b) { w[o] = b; }
    void copy(uint32_t o, uint32_t dist, uint32_t len) { for (uint32_t i = 0; i < len; i++) w[o + i] = w[o - dist + i]; }
    void stored(uint32_t o, const uint8_t* src, uint32_t len) { if (len) memcpy(w + o, src, len); }
};

// The serial host model of the device decoder: the same functions, one member after the other, each from a buffer of
// exactly its payload into one of exactly ISIZE bytes (a sanitizer build sees any step past either).  false: "not
// taken", *first_bad / *status name the first member refused (a head that is not taken: member 0, INF_BAD_HEAD).
inline bool host_inflate_listed(const uint8_t* p, const std::vector<MemberRef>& ms, std::vector<uint8_t>& text, uint64_t* first_bad,
                                uint32_t* status) {
    const int64_t bad = first_refused(ms);
    if (bad >= 0) { *first_bad = (uint64_t)bad; *status = ms[(size_t)bad].status; return false; }
    DecodeTables T;
    for (size_t i = 0; i < ms.size(); i++) {
        const std::vector<uint8_t> payload(p + ms[i].at + ms[i].head, p + ms[i].at + ms[i].size - MEMBER_TAIL);
        std::vector<uint8_t> window(ms[i].isize);
        HostSink sink{window.data()};
        uint32_t produced = 0;
        uint32_t st = inflate_blocks(payload.data(), (uint32_t)payload.size(), ms[i].isize, T, sink, &produced);
        if (!st && crc32_bytes(window.data(), ms[i].isize) != ms[i].crc) st = INF_BAD_CRC;
        if (st) { *first_bad = i; *status = st; text.clear(); return false; }
        text.insert(text.end(), window.begin(), window.end());
    }
    return true;
}
inline bool host_inflate_model(const uint8_t* p, uint64_t n, std::vector<uint8_t>& text, uint64_t* first_bad, uint32_t* status) {
    text.clear(); *first_bad = 0; *status = INF_OK;
    std::vector<MemberRef> ms;
    uint64_t consumed = 0;
    if (!list_members(p, n, true, ms, &consumed)) { *status = INF_BAD_HEAD; return false; }
    return host_inflate_listed(p, ms, text, first_bad, status);
}
// the same for a BGZF file: the members by their BSIZE chain, a window of up to BGZF_MAX_TEXT bytes
inline bool host_inflate_model_bgzf(const uint8_t* p, uint64_t n, std::vector<uint8_t>& text, uint64_t* first_bad, uint32_t* status) {
    text.clear(); *first_bad = 0; *status = INF_OK;
    std::vector<MemberRef> ms;
    uint64_t consumed = 0;
    if (!list_members_bgzf(p, n, true, ms, &consumed)) { *status = INF_BAD_HEAD; return false; }
    return host_inflate_listed(p, ms, text, first_bad, status);
}

// ---------------------------------------------------------------------------------------------------------------------
// Large members: a decoder that is parallel inside a member, for the files other writers make (one whole-file member
// from gzip / pigz / Python's gzip.open, 4 MiB zlib members).  A deflate stream can be entered at a block boundary without
// what stands before it, and a dynamic block's header is signature enough to find boundaries by trial:
//   find    the payload is cut every piece_bytes; from each cut on, bit offsets are tried until one holds BTYPE = 2 and a
//           header dynamic_tables() takes whole (block_start_ok) -- a found start -- or the next cut comes.  The payload's
//           first bit is a start.  Stored and fixed blocks are not looked for: they are decoded inside the piece they
//           fall in.
//   marker  every found start is decoded without the text before it, into a window of WINDOW 16-bit entries: a byte, or
//           MARK | j, "byte j of the unknown WINDOW bytes before this piece".  The run ends where a block ends exactly at
//           a later found start, behind the final block, with the data, or at PIECE_TEXT_CAP bytes of text.
//   chain   piece 0 is live; the next live piece is the start the live one ended at; found starts a live piece steps
//           over are dropped (false, or redundant).  In that order each live piece's last window becomes bytes by looking
//           its markers up in the window before it.
//   bytes   every live piece is decoded again, as bytes, with the window before it preset, to its place in the text, and
//           its CRC32 taken; the host combines the CRCs and checks them and the length against the member's tail.
// large_call() below is that sequence for one call, written once for the serial host backend (HostLarge: the host model)
// and the device's (PfGzLarge, pf_deflate.hip).  A member may span calls: LargeState carries it.
constexpr uint32_t WINDOW = 32768, WMASK = WINDOW - 1, MARK = 0x8000;
constexpr uint32_t PIECE_DEFAULT = 32768, PIECE_MIN = 64;
constexpr uint32_t PIECE_TEXT_CAP = 256u << 20;       // a piece of more text (a member without a findable block start in it
                                                      // for that long) is INF_TOO_LARGE: the member is not taken
constexpr uint32_t MAX_PIECES = 2048;                 // starts of a call: every one has a ring with the backend
constexpr uint32_t MAX_CUTS = MAX_PIECES / 4 * 3;     // cuts of a call, which reads MAX_CUTS * piece_bytes at most; the other
                                                      // quarter of the starts is room for the payloads of members side by side
constexpr uint64_t LARGE_MAX_TEXT = 256ull << 20;     // text taken per call (PfGzDecoder::MAX_TEXT)

// The RFC 1952 head at p[0 .. n): INF_OK and *head = its bytes; INF_TRUNCATED: it runs past n; INF_BAD_HEAD: not
// ID1 ID2 CM = 8, or a reserved FLG bit.  FEXTRA, FNAME, FCOMMENT and FHCRC are skipped.
inline uint32_t parse_head(const uint8_t* p, uint64_t n, uint64_t* head) {
    *head = 0;
    if (n >= 1 && p[0] != 0x1F) return INF_BAD_HEAD;
    if (n >= 2 && p[1] != 0x8B) return INF_BAD_HEAD;
    if (n >= 3 && p[2] != 8) return INF_BAD_HEAD;
    if (n >= 4 && (p[3] & 0xE0)) return INF_BAD_HEAD;
    if (n < MEMBER_HEAD) return INF_TRUNCATED;
    const uint32_t flg = p[3];
    uint64_t at = MEMBER_HEAD;
    if (flg & 4) {                                   // FEXTRA
        if (at + 2 > n) return INF_TRUNCATED;
        at += 2 + (p[at] | (uint64_t)p[at + 1] << 8);
        if (at > n) return INF_TRUNCATED;
    }
    for (uint32_t bit : {8u, 16u}) {                 // FNAME, FCOMMENT: to their zero byte
        if (!(flg & bit)) continue;
        const void* z = at < n ? memchr(p + at, 0, (size_t)(n - at)) : nullptr;
        if (!z) return INF_TRUNCATED;
        at = (uint64_t)(static_cast<const uint8_t*>(z) - p) + 1;
    }
    if (flg & 2) at += 2;                            // FHCRC
    if (at > n) return INF_TRUNCATED;
    *head = at;
    return INF_OK;
}

// whether a dynamic block may start at bit `bit` of p[0 .. n): BTYPE = 2 (either BFINAL) and a header that passes
// everything dynamic_tables checks.  T is the caller's scratch.  Reads no byte outside p[0 .. n), ends for any input.
PF_HD bool block_start_ok(const uint8_t* p, uint32_t n, uint64_t bit, DecodeTables& T) {
    if ((bit >> 3) >= n) return false;
    BitReader r = bit_reader_at(p, n, bit);
    const uint32_t head = take_bits(r, 3);
    if (r.over || (head >> 1) != 2) return false;
    return dynamic_tables(r, T, true) == INF_OK;
}

// what the marker pass leaves of a piece, and the stop rule it runs under: a block that ends at a found start behind
// the piece's own (starts[] ascending)
struct PieceResult { uint32_t status, produced, why, next; uint64_t end_bit; };
struct StopAtStart {
    const uint64_t* starts; uint32_t n, k;
    PF_HD_M bool at(uint64_t bit) { while (k < n && starts[k] < bit) k++; return k < n && starts[k] == bit; }
};
struct StopAtBit { uint64_t bit; PF_HD_M bool at(uint64_t b) { return b == bit; } };
// a live piece for the byte pass: where it starts and must end, the text before it that exists, its text's place and size
struct LivePiece { uint64_t start_bit, end_bit, dst; uint32_t piece, hist, produced, why; };
struct ByteResult { uint32_t status, produced, crc, pad; };

// A window of WINDOW entries as a ring (entry of text offset o: w[o & WMASK]; the entries of the WINDOW bytes before o = 0
// stand in it when the run starts), and the text itself where `text` is given.  The serial form; the wave's is in
// pf_deflate.hip.
template <class E> struct HostRing {
    E* w; uint8_t* text;
    bool leader() const { return true; }
    void sync() {}
    uint32_t share(uint32_t v) const { return v; }
    void put(uint32_t o, E v) { w[o & WMASK] = v; if (text) text[o] = (uint8_t)v; }
    void literal(uint32_t o, uint8_t b) { put(o, b); }
    void copy(uint32_t o, uint32_t dist, uint32_t len) { for (uint32_t i = 0; i < len; i++) put(o + i, w[(o + i - dist) & WMASK]); }
    void stored(uint32_t o, const uint8_t* src, uint32_t len) { for (uint32_t i = 0; i < len; i++) put(o + i, src[i]); }
};

// the marker pass's run of one piece: ring[WINDOW] of 16-bit entries, left as the run ends
template <class Sink>
PF_HD PieceResult marker_run(const uint8_t* p, uint32_t n, const uint64_t* starts, uint32_t n_starts, uint32_t i, DecodeTables& T, Sink& sink) {
    BitReader r = bit_reader_at(p, n, starts[i]);
    StopAtStart stop{starts, n_starts, i + 1};
    PieceResult R{INF_OK, 0, RUN_NONE, 0, 0};
    R.status = inflate_run(r, WINDOW, PIECE_TEXT_CAP, T, sink, stop, &R.produced, &R.why);
    if (R.status == INF_TOO_MUCH_TEXT) R.status = INF_TOO_LARGE;
    if (R.status == INF_OK) { R.end_bit = bit_pos(r); R.next = stop.k; }
    return R;
}
// the byte pass's run of one live piece: ring[WINDOW] of bytes preset with the window before it, text to text[0 .. produced)
template <class Sink>
PF_HD ByteResult byte_run(const uint8_t* p, uint32_t n, const LivePiece& L, DecodeTables& T, Sink& sink) {
    BitReader r = bit_reader_at(p, n, L.start_bit);
    StopAtBit stop{L.end_bit};
    ByteResult B{INF_OK, 0, 0, 0};
    uint32_t why = RUN_NONE;
    B.status = inflate_run(r, L.hist, L.produced, T, sink, stop, &B.produced, &why);
    // (the same bits under the same rule: anything else than the marker pass's end is a bug, and refuses the member)
    if (B.status == INF_OK && (B.produced != L.produced || why != L.why || bit_pos(r) != L.end_bit)) B.status = INF_NOT_DECODED;
    return B;
}
// entry j of the window a piece leaves (the WINDOW bytes before its end), from its ring and the window before it
// (`before` null: no text stands before the piece -- a member's first -- and what a marker stands for is never looked at)
PF_HD uint8_t chain_byte(const uint16_t* ring, uint32_t produced, const uint8_t* before, uint32_t j) {
    const uint16_t e = ring[(produced + j) & WMASK];
    return e & MARK ? (before ? before[e & WMASK] : (uint8_t)0) : (uint8_t)e;
}
// a chain of live pieces starts with the call's first piece and with every piece that has no text before it: the chains
// of members decoded side by side are independent of one another
PF_HD bool chain_starts(const LivePiece* live, uint32_t i) { return i == 0 || live[i].hist == 0; }

// an open member between calls, and the route's counters
struct LargeState {
    bool open = false;
    uint32_t bit0 = 0, hist = 0, crc = 0;      // the next block's bit in the first carried byte; bytes in the window; running CRC32
    uint64_t len = 0;                          // running text length
    uint8_t sig[MEMBER_SIG] = {0, 0, 0, 0, 0, 0, 0, 0};      // its head's first bytes: the members that follow it are found under them
};
struct LargeStats { uint64_t found = 0, live = 0, dropped = 0, members = 0; };
struct LargeOut {
    bool taken = false, none_yet = false, member_end = false;
    uint32_t status = INF_OK;
    uint64_t consumed = 0, text_n = 0;
};

// One call of the large-member route over bytes[0 .. n), which start at a member's head (!s.open) or with the byte that
// holds an open member's next block (s.open).  The backend B runs the passes:
//   int begin(bytes, limit)                                 the bytes the passes may look at, bytes[0 .. limit)
//   int find(cuts[], n_cuts, piece_bytes, hit[])            hit[k]: the start found from cuts[k] on, or ~0
//   int marker(starts[], n_starts, results[])               (the rings stay with the backend)
//   int bytes_pass(live[], n_live, text_n, results[])       chain and byte pass: the text, the window carried
// Each returns PF_OK or an error of the library's; "not taken" is out.taken = false with out.status.  out.none_yet: nothing
// could be confirmed yet, nothing is consumed, the caller reads on (only with !last).  The state moves only with a call
// that consumes bytes.  A call may take several members, one behind the other, where their heads can be found beforehand.
template <class B>
int large_call(B& be, LargeState& s, LargeStats& stats, const uint8_t* bytes, uint64_t n, bool last, uint32_t piece_bytes, LargeOut& out) {
    out = LargeOut{};
    auto refuse = [&](uint32_t st) { out.taken = false; out.status = st; s = LargeState{}; return 0; };
    auto read_on = [&]() { out.taken = true; out.none_yet = true; return 0; };
    if (piece_bytes == 0) piece_bytes = PIECE_DEFAULT;
    LargeState t = s;
    uint64_t start_bit = t.bit0;
    if (!t.open) {
        uint64_t head = 0;
        const uint32_t st = parse_head(bytes, n, &head);
        if (st == INF_TRUNCATED && !last) return read_on();
        if (st) return refuse(st);
        t = LargeState{};
        t.open = true; start_bit = head * 8;
        memcpy(t.sig, bytes, MEMBER_SIG);
    }
    const uint64_t first = start_bit >> 3;
    const uint64_t limit = std::min<uint64_t>(n, first + (uint64_t)MAX_CUTS * piece_bytes);     // (< 4 GiB: the readers' offsets are 32-bit)
    if (limit >= (1ull << 32) || first >= limit) return first >= limit && !last ? read_on() : refuse(first >= limit ? INF_TRUNCATED : INF_TOO_LARGE);
    const bool cut_short = limit < n, end_here = last && !cut_short;
    { const int rc = be.begin(bytes, limit); if (rc) return rc; }
    // find: the cuts' hits, and -- members side by side -- the payload's first bit of every member whose head stands in these
    // bytes under the signature of the call's first member, open or not (list_members' search; a false candidate is a false
    // start like any other)
    // A call has MAX_PIECES starts at most -- the backend's rings are sized by it: the cuts come first, then as many members'
    // payloads as still fit (the chain ends in front of a member whose payload is no start; the next call begins there)
    std::vector<uint64_t> cuts, hit, starts(1, start_bit), payloads, heads;
    for (uint64_t c = first + piece_bytes; c < limit; c += piece_bytes) cuts.push_back(c);
    const size_t room = MAX_PIECES - 1 - std::min<size_t>(MAX_PIECES - 1, cuts.size());
    if (limit > MEMBER_SIG)
        for (uint64_t c = s.open ? 0 : 1; c + MEMBER_HEAD <= limit;) {
            const void* m = memmem(bytes + c, (size_t)(limit - c), t.sig, MEMBER_SIG);
            if (!m) break;
            c = (uint64_t)(static_cast<const uint8_t*>(m) - bytes);
            uint64_t head = 0;
            if (parse_head(bytes + c, limit - c, &head) == INF_OK && c + head < limit) { heads.push_back(c); if (payloads.size() < room) payloads.push_back((c + head) * 8); }
            c++;
        }
    hit.assign(cuts.size(), ~0ull);
    if (!cuts.empty()) { const int rc = be.find(cuts.data(), (uint32_t)cuts.size(), piece_bytes, hit.data()); if (rc) return rc; }
    for (uint64_t h : hit) if (h != ~0ull) starts.push_back(h);
    starts.insert(starts.end(), payloads.begin(), payloads.end());
    std::sort(starts.begin(), starts.end());
    starts.erase(std::unique(starts.begin(), starts.end()), starts.end());
    if (starts.size() > MAX_PIECES) return refuse(INF_TOO_LARGE);          // (cannot be: 1 + the cuts + the payloads that fit)
    // marker
    std::vector<PieceResult> res(starts.size());
    { const int rc = be.marker(starts.data(), (uint32_t)starts.size(), res.data()); if (rc) return rc; }
    // the live chain: what is confirmed and fits the call.  Behind a member's tail the chain goes on with the member whose
    // payload starts there, if its first bit is a start of this call
    struct Ended { size_t n_live; uint64_t tail; };            // a member that ends in this call: its last live piece, its tail's place
    std::vector<LivePiece> live;
    std::vector<Ended> ended;
    uint64_t text_n = 0, consumed = 0, member_len = t.len;
    uint32_t at = 0, next_bit0 = 0;
    bool member_end = false;
    for (;;) {
        const PieceResult& R = res[at];
        if (R.status == INF_TRUNCATED && !end_here) break;                    // its end is not in these bytes yet
        if (R.status != INF_OK) { if (ended.empty()) return refuse(R.status); break; }      // (a later member: in a call of its own)
        if (!live.empty() && text_n + R.produced > LARGE_MAX_TEXT) break;
        const uint64_t tail = (R.end_bit + 7) >> 3;
        if (R.why == RUN_FINAL && tail + MEMBER_TAIL > n) {
            if (!last || !ended.empty()) break;
            return refuse(INF_TRUNCATED);
        }
        live.push_back(LivePiece{starts[at], R.end_bit, text_n, at, (uint32_t)std::min<uint64_t>(WINDOW, member_len), R.produced, R.why});
        text_n += R.produced; member_len += R.produced;
        member_end = R.why == RUN_FINAL;
        if (member_end) {
            consumed = tail + MEMBER_TAIL; next_bit0 = 0; member_len = 0;
            ended.push_back(Ended{live.size(), tail});
            uint64_t head = 0;
            if (consumed >= limit || parse_head(bytes + consumed, limit - consumed, &head) != INF_OK) break;
            // (a member within the small-member kernels' limits, as list_members sizes it, is theirs: the call ends here)
            const auto after = std::upper_bound(heads.begin(), heads.end(), consumed);
            const uint64_t ends = after != heads.end() ? *after : end_here ? n : 0;        // (0: not known)
            if (ends >= consumed + MEMBER_HEAD + MEMBER_TAIL && bytes[consumed + 3] == 0 && ends - consumed <= SLOT_BYTES && le32(bytes + ends - 4) <= CHUNK) break;
            const auto next = std::lower_bound(starts.begin(), starts.end(), (consumed + head) * 8);
            if (next == starts.end() || *next != (consumed + head) * 8) break;
            at = (uint32_t)(next - starts.begin());
            continue;
        }
        if (R.next >= starts.size()) return refuse(INF_NOT_DECODED);           // (a run that stopped at a start names it)
        consumed = starts[R.next] >> 3; next_bit0 = (uint32_t)(starts[R.next] & 7);
        at = R.next;
    }
    if (live.empty()) {
        // nothing confirmed: with more bytes to come the caller reads on, unless this call already looked as far as one may
        if (cut_short || last) return refuse(cut_short ? INF_TOO_LARGE : INF_TRUNCATED);
        return read_on();
    }
    // chain and byte pass, then every ended member's CRC32 and length against its tail
    std::vector<ByteResult> br(live.size());
    { const int rc = be.bytes_pass(live.data(), (uint32_t)live.size(), text_n, br.data()); if (rc) return rc; }
    size_t e = 0;
    for (size_t i = 0; i < live.size(); i++) {
        if (br[i].status != INF_OK) return refuse(br[i].status);
        t.crc = crc_combine(t.crc, br[i].crc, live[i].produced);
        t.len += live[i].produced;
        if (e < ended.size() && ended[e].n_live == i + 1) {
            const uint8_t* tail = bytes + ended[e].tail;
            if (le32(tail) != t.crc) return refuse(INF_BAD_CRC);
            if (le32(tail + 4) != (uint32_t)t.len) return refuse(t.len > le32(tail + 4) ? INF_TOO_MUCH_TEXT : INF_TOO_LITTLE_TEXT);
            stats.members++; e++;
            const LargeState ended_one = t;
            t = LargeState{};
            if (i + 1 < live.size()) { t.open = true; memcpy(t.sig, ended_one.sig, MEMBER_SIG); }
        }
    }
    if (t.open) { t.bit0 = next_bit0; t.hist = (uint32_t)std::min<uint64_t>(WINDOW, t.len); }
    uint64_t found = 0;                        // the found starts up to where the call's text ends: the rest is found again
    for (uint64_t b : starts) if (b < live.back().end_bit) found++;
    stats.found += found; stats.live += live.size(); stats.dropped += found - live.size();
    s = t;
    out.taken = true; out.member_end = !t.open; out.consumed = consumed; out.text_n = text_n;
    return 0;
}

// The serial backend: the host model.  Every pass reads from a heap copy of exactly the bytes a call may look at, and a
// live piece's text goes to a buffer of exactly its size (a sanitizer build sees any step past either).
struct HostLarge {
    std::vector<uint16_t> rings;               // of the call's found starts, WINDOW entries each
    std::vector<uint8_t> window = std::vector<uint8_t>(WINDOW, 0), text;     // the window carried; the call's text
    std::vector<uint8_t> data;                 // a heap copy of exactly the bytes the call may look at
    uint64_t limit = 0;
    int begin(const uint8_t* bytes, uint64_t n) { data.assign(bytes, bytes + n); limit = n; return 0; }
    int find(const uint64_t* cuts, uint32_t n_cuts, uint32_t piece_bytes, uint64_t* hit) {
        DecodeTables T;
        for (uint32_t k = 0; k < n_cuts; k++) {
            const uint64_t end = std::min<uint64_t>(limit, cuts[k] + piece_bytes) * 8;
            for (uint64_t bit = cuts[k] * 8; bit < end; bit++)
                if (block_start_ok(data.data(), (uint32_t)limit, bit, T)) { hit[k] = bit; break; }
        }
        return 0;
    }
    int marker(const uint64_t* starts, uint32_t n_starts, PieceResult* res) {
        DecodeTables T;
        rings.assign((size_t)n_starts * WINDOW, 0);
        for (uint32_t i = 0; i < n_starts; i++) {
            uint16_t* ring = rings.data() + (size_t)i * WINDOW;
            for (uint32_t j = 0; j < WINDOW; j++) ring[j] = (uint16_t)(MARK | j);
            HostRing<uint16_t> sink{ring, nullptr};
            res[i] = marker_run(data.data(), (uint32_t)limit, starts, n_starts, i, T, sink);
        }
        return 0;
    }
    int bytes_pass(const LivePiece* live, uint32_t n_live, uint64_t text_n, ByteResult* br) {
        DecodeTables T;
        text.assign((size_t)text_n, 0);
        std::vector<uint8_t> before(window), after(WINDOW), ring(WINDOW);
        for (uint32_t i = 0; i < n_live; i++) {
            const uint16_t* marks = rings.data() + (size_t)live[i].piece * WINDOW;
            for (uint32_t j = 0; j < WINDOW; j++) after[j] = chain_byte(marks, live[i].produced, live[i].hist ? before.data() : nullptr, j);
            ring = before;
            std::vector<uint8_t> piece(live[i].produced);
            HostRing<uint8_t> sink{ring.data(), piece.data()};
            br[i] = byte_run(data.data(), (uint32_t)limit, live[i], T, sink);
            br[i].crc = crc32_bytes(piece.data(), live[i].produced);
            // (the chain's window and the byte pass's own must be the same bytes)
            if (br[i].status == INF_OK)
                for (uint32_t j = 0; j < WINDOW; j++) if (ring[(live[i].produced + j) & WMASK] != after[j] && WINDOW - j <= live[i].hist + live[i].produced) br[i].status = INF_NOT_DECODED;
            if (!piece.empty()) memcpy(text.data() + live[i].dst, piece.data(), piece.size());
            before.swap(after);
        }
        window = before;
        return 0;
    }
};

// a whole file of gzip members by the large-member route, each member alone, call after call as a feed would; false: "not
// taken", *member / *status name the member refused
inline bool host_inflate_large(const uint8_t* p, uint64_t n, uint32_t piece_bytes, std::vector<uint8_t>& text, LargeStats& stats,
                               uint64_t* member, uint32_t* status) {
    text.clear(); *member = 0; *status = INF_OK;
    HostLarge be;
    LargeState s;
    for (uint64_t at = 0; at < n;) {
        LargeOut o;
        if (large_call(be, s, stats, p + at, n - at, true, piece_bytes, o) || !o.taken || !o.consumed) {
            *member = stats.members; *status = o.status ? o.status : (uint32_t)INF_NOT_DECODED; text.clear();
            return false;
        }
        text.insert(text.end(), be.text.begin(), be.text.end());
        at += o.consumed;
    }
    if (s.open) { *member = stats.members; *status = INF_TRUNCATED; text.clear(); return false; }
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
    DevBuf slots, sizes, offs, tokens;                   // of one launch: BLOCK / CHUNK chunks
    // per cursor: the chunk plan of its last encode (pinned, and on the device), the cursor with the member offset of
    // every segment's first chunk behind it (on the device, and read back in one copy)
    PinBuf plan_pin[N_CURSORS], seg_pin[N_CURSORS];
    DevBuf plan_dev[N_CURSORS], seg_dev[N_CURSORS];
    uint64_t caps[N_CURSORS] = {}, n_segs[N_CURSORS] = {};      // the bytes the last encode's members may take, its segments
    uint32_t grid_cap = 0;                               // resident workgroups the token streams are sized for
    std::vector<pfgz::ChunkDesc> plan;                   // (scratch of encode_segments)
    static uint64_t chunks(uint64_t n) { return (n + pfgz::CHUNK - 1) / pfgz::CHUNK; }
    static uint64_t bound(uint64_t n) { return chunks(n) * pfgz::SLOT_BYTES; }       // of the members of n bytes of text in one segment
    // of the members of n bytes in n_seg segments: every segment may end in a short chunk of its own
    static uint64_t bound_segments(uint64_t n, uint64_t n_seg) { return pfgz::plan_chunks(n, n_seg) * pfgz::SLOT_BYTES; }
    uint64_t device_bytes() const {
        uint64_t b = slots.cap + sizes.cap + offs.cap + tokens.cap;
        for (int w = 0; w < N_CURSORS; w++) b += plan_dev[w].cap + seg_dev[w].cap;
        return b;
    }
    int ensure(int n_cu);
    // On `st`: cursor w back to zero, the members of text[0 .. n) (device memory) written from `members` on, which holds
    // cap bytes, and the cursor -- their size -- on its way into w's pinned word.  t0 / t1, where given, are recorded
    // around the cursor's reset and the launches.
    int encode(hipStream_t st, Cursor w, const char* text, uint64_t n, uint32_t flags, char* members, uint64_t cap,
               hipEvent_t t0 = nullptr, hipEvent_t t1 = nullptr);
    // The same with members that end wherever a segment does: seg_end[0 .. n_seg) as pfgz::chunk_plan takes them
    // (PF_ERR_ARG otherwise).  A launch takes BLOCK / CHUNK chunks of the plan; cap must hold the plan's worst case
    // (bound_segments), or PF_ERR_ARG.  The offsets of the segments' first members travel back with the cursor.
    int encode_segments(hipStream_t st, Cursor w, const char* text, uint64_t n, const uint64_t* seg_end, uint64_t n_seg, uint32_t flags,
                        char* members, uint64_t cap, hipEvent_t t0 = nullptr, hipEvent_t t1 = nullptr);
    // once the caller has synchronised with that encode: the bytes of its members; PF_ERR_STATE if they exceed its cap
    int member_bytes(Cursor w, uint64_t* z) const;
    // and the offset behind every segment's members, member_end[n_seg of that encode]
    int segment_ends(Cursor w, uint64_t* member_end) const;
};
// The device decoder: members in, text out, one wave per member (gz_inflate_kernel; gz_inflate64_kernel for the BGZF members
// of more than CHUNK bytes of text).  Its buffers hold the members of one call, MAX_MEMBERS at most, and are sized from the
// members given: device_bytes() <= their bytes + 52 per member + slack (members of this project's own: at most
// MAX_MEMBERS * (SLOT_BYTES + 52)); the text buffer is the caller's.  Every call is stream-ordered on the stream given.
namespace pfgz {
struct DecMember { uint64_t src, dst; uint32_t csize, isize, crc, pad; };     // payload offset in the upload, text offset
struct DecResult { uint32_t status, produced, crc, pad; };                   // an InfStatus, the bytes given, the CRC32 found
}
struct PfGzDecoder {
    static constexpr uint64_t MAX_TEXT = 256ull << 20;        // text bytes per call: the row filter's block
    static constexpr uint32_t MAX_MEMBERS = (uint32_t)(MAX_TEXT / pfgz::CHUNK);
    DevBuf members, desc, results;                           // (desc: the descriptors, then the two kernels' member indices)
    PinBuf pin;                                              // the results, read back
    std::vector<pfgz::DecMember> desc_host;
    std::vector<uint32_t> index_host;                        // the members of at most CHUNK bytes of text, then the larger ones
    uint32_t n_last = 0;
    bool large_ready = false;                                // gz_inflate64_kernel's dynamic LDS limit is raised (once, on the decoder's device)
    uint64_t device_bytes() const { return members.cap + desc.cap + results.cap; }
    // On `st`: the n members ms[] (listed over `bytes`, host memory, all with status INF_OK, each with its own head
    // length: MEMBER_HEAD or BGZF_HEAD) uploaded and inflated into text[0 .. sum of their ISIZE), which must fit text_cap;
    // their results on the way into pinned memory.
    int decode(hipStream_t st, const uint8_t* bytes, const pfgz::MemberRef* ms, uint32_t n, uint8_t* text, uint64_t text_cap,
               hipEvent_t t0 = nullptr, hipEvent_t t1 = nullptr);
    // once the caller has synchronised with that decode: the first member that failed a check and its status, or -1
    int64_t first_refused(uint32_t* status) const;
};
// The device backend of pfgz::large_call: the find, marker, chain and byte passes as separate launches in stream order, no
// workgroup waiting for another.  Device memory per call, whatever the file's size: the bytes the call looks at
// (MAX_CUTS * piece_bytes at most: 48 MiB at the default piece), per start (MAX_PIECES at most) a ring of 64 KiB and 48 bytes
// of results, per live piece a window of 32 KiB, one carried window -- under MAX_PIECES * 96 KiB + the bytes = 240 MiB at the
// default piece; the text buffer is the caller's (`place`), LARGE_MAX_TEXT at most.
struct PfGzLarge {
    hipStream_t st = nullptr;
    // asked before the byte pass: room for text_n bytes of text; -> where they go (device memory)
    std::function<int(uint64_t text_n, uint8_t** dst)> place;
    DevBuf data, d_cuts, d_hits, d_starts, d_res, rings, wins, d_live, d_br, window;
    HipEvent e0, e1, e2;
    float ms[4] = {0, 0, 0, 0};               // device time of the find, marker, chain and byte passes
    uint32_t limit = 0;
    bool ready = false;                       // the carried window exists, gz_marker_kernel's dynamic LDS limit is raised
    uint64_t device_bytes() const {
        return data.cap + d_cuts.cap + d_hits.cap + d_starts.cap + d_res.cap + rings.cap + wins.cap + d_live.cap + d_br.cap + window.cap;
    }
    int begin(const uint8_t* bytes, uint64_t n);
    int find(const uint64_t* cuts, uint32_t n_cuts, uint32_t piece_bytes, uint64_t* hit);
    int marker(const uint64_t* starts, uint32_t n_starts, pfgz::PieceResult* res);
    int bytes_pass(const pfgz::LivePiece* live, uint32_t n_live, uint64_t text_n, pfgz::ByteResult* br);
};
#endif
