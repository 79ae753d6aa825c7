// pf_deflate.hip -- the deflate encoder and decoder on the device (format logic: pf_deflate.h) and the host models' entry points.
//
// gz_encode_kernel: one workgroup of 256 threads per chunk of at most CHUNK bytes (a grid of two workgroups per CU walks
// the chunks).  The chunks come from a plan in device memory (pfgz::chunk_plan): a chunk starts at any byte and may be
// followed by another segment's text, of which nothing is staged -- every read of the text is a read of the chunk's own
// bytes in LDS.  The chunk's text is staged in LDS beside a hash table of 4 096 positions.  Matches are found in steps of 256
// positions, one per thread.  The positions look their 4-byte hash up and go into the table eight at a time, in text
// order, by atomicMax: a position's candidate is the largest position with its hash among the groups of eight before its
// own, whatever order the lanes ran in -- the same text gives the same bytes.  The compares then run 256 wide.  One lane
// walks the step's match lengths greedily (a match, or one literal, then the position behind it); the token starts it
// lists become tokens, in parallel, in a stream in global memory, and the histograms are kept by LDS atomics.
// The coding pass sorts the used symbols by rank counting, builds the two length-limited codes (one lane each), sums
// the exact sizes of the three block types, and places the tokens' bits by wave prefix sums into a staging area that
// takes the place of the text and the table; the member leaves LDS in whole words.
// LDS: 48 KiB of text + table, 10 KiB of tables -- under 64 KiB, two workgroups per CU within its 160 KiB.
// Under PF_GZ_DEEP the kernel's second instantiation runs: a second candidate from the row before and a parse that is
// lazy by one step (the rule: pf_deflate.h; how the kernel finds the row starts and the next step's first length: the
// comment in front of the kernel).
// gz_scan_kernel / gz_gather_kernel: the member sizes summed from an append cursor, the offset of every segment's first
// member noted behind the cursor, the members copied from their worst-case slots to their places, contiguous, so that one
// copy takes them to the host.  Under PF_GZ_BGZF these two also make every member a BGZF member, 8 bytes of head longer.
// gz_inflate_kernel / gz_inflate64_kernel: the decoder, one wave per member, further down with its own comment.
#include "pf_deflate.h"

#include <cstdlib>
#include <cstring>

namespace pfgz {

constexpr int THREADS = 256;
constexpr uint32_t TEXT_WORDS = (CHUNK + 16) / 4, TAB_WORDS = 1u << HASH_BITS;
static_assert(CHUNK == THREADS * CRC_SUB, "one CRC piece per thread");
static_assert(SLOT_WORDS <= TEXT_WORDS + TAB_WORDS, "the staging area takes the place of the text and the table");
static_assert(CHUNK <= 32768, "distances reach 32 768 at most, a stored block 65 535 bytes");

struct EncParams {
    const uint8_t* text; const ChunkDesc* plan; uint32_t nchunks, flags;      // the launch's chunks: plan[0 .. nchunks)
    uint8_t* slots; uint32_t* sizes; uint32_t* tokens;
};

__device__ inline uint32_t wave_inclusive_sum(uint32_t x, uint32_t lane) {
    for (uint32_t d = 1; d < 64; d <<= 1) {
        const uint32_t t = __shfl_up(x, d, 64);
        if (lane >= d) x += t;
    }
    return x;
}

__device__ inline uint32_t load4(const uint8_t* p) {
    uint32_t w;
    __builtin_memcpy(&w, p, 4);
    return w;
}

// symbols tid and tid + 256 of a histogram of nsym entries into `sorted`, by ascending (frequency, symbol), the unused
// ones left out; returns through *n_used (zeroed by the caller before the barrier in front of this)
__device__ inline void rank_sort(const uint32_t* hist, uint32_t nsym, SymFreq* sorted, uint32_t* n_used, uint32_t tid) {
    for (uint32_t s = tid; s < nsym; s += THREADS) {
        const uint32_t f = hist[s];
        if (!f) continue;
        uint32_t rank = 0;
        for (uint32_t j = 0; j < nsym; j++) {
            const uint32_t g = hist[j];
            rank += (g != 0 && (g < f || (g == f && j < s))) ? 1u : 0u;
        }
        sorted[rank] = SymFreq{f, s};
        atomicAdd(n_used, 1u);
    }
}

// the last two set bits of `m`, whose bit 0 is position `base`, pushed onto (s, r) = 1 + the last and the second-to-last
// '\n' seen so far (0: none)
__device__ inline void push_newlines(uint64_t m, uint32_t base, uint32_t* s, uint32_t* r) {
    if (!m) return;
    const uint32_t top = 63u - (uint32_t)__builtin_clzll(m);
    const uint64_t rest = m ^ (1ull << top);
    *r = rest ? base + (63u - (uint32_t)__builtin_clzll(rest)) + 1 : *s;
    *s = base + top + 1;
}

// DEEP: the PF_GZ_DEEP variant (pf_deflate.h: deep_length, deep_defers); the plain instantiation keeps its code.
// Row starts: every wave's ballot of "my byte is '\n'" goes into LDS, four 64-bit words a step, and a lane reads its row
// start and the one before from the bits below its own, or from the last two newlines of the earlier steps, carried in
// registers -- no list of newline positions is kept.  The deferral asks for L(q + 1) at a token start q; where q is a
// step's last position the walking lane works that one length out itself: the table then holds exactly the candidates of
// the next step's first position, whose row starts are the carry.  The next step computes the same value again.
template <bool DEEP>
__global__ __launch_bounds__(THREADS, 2) void gz_encode_kernel(EncParams P) {
    __shared__ uint32_t s_buf[TEXT_WORDS + TAB_WORDS];       // the text, the hash table; later the member's staging
    __shared__ uint64_t s_nl[DEEP ? THREADS / 64 : 1];
    __shared__ uint16_t s_mlen[2][THREADS], s_mdist[2][THREADS], s_tokpos[2][THREADS];
    __shared__ uint32_t s_cnt[2], s_carry, s_nused[2], s_bits[3], s_wsum[2][4];
    __shared__ uint32_t s_ll_hist[288], s_d_hist[32];
    __shared__ Codes s_dyn;
    __shared__ SymFreq s_sort_ll[288], s_sort_d[32];
    __shared__ uint32_t s_crc[THREADS], s_crclen[THREADS];
    const uint32_t tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    uint8_t* s_text = reinterpret_cast<uint8_t*>(s_buf);
    uint32_t* s_tab = s_buf + TEXT_WORDS;
    uint32_t* tokens = P.tokens + (size_t)blockIdx.x * CHUNK;
    const bool lit_only = (P.flags & PF_GZ_LITERALS_ONLY) != 0;

    for (uint32_t chunk = blockIdx.x; chunk < P.nchunks; chunk += gridDim.x) {
        const ChunkDesc d = P.plan[chunk];
        const uint32_t n = min(d.len, CHUNK);
        const uint8_t* src = P.text + d.start;
        uint8_t* slot = P.slots + (size_t)chunk * SLOT_BYTES;
        // ---- stage the text, clear the table and the histograms.  Whole words come from aligned loads: a chunk that
        // starts `a` bytes behind a word boundary takes every staged word from two neighbouring words of the text (the
        // text's buffer starts on a word boundary, so the first of them is the buffer's own; the last word taken this
        // way is the last that lies wholly inside the chunk), and its last few bytes one by one
        {
            const uint32_t a = (uint32_t)(reinterpret_cast<uintptr_t>(src) & 3);
            uint32_t nw = n / 4;
            if (a == 0) {
                const uint32_t* src4 = reinterpret_cast<const uint32_t*>(src);
                for (uint32_t i = tid; i < nw; i += THREADS) s_buf[i] = src4[i];
            } else {
                const uint32_t* src4 = reinterpret_cast<const uint32_t*>(src - a);
                const uint32_t sh = 8 * a;
                nw = n + a >= 8 ? (n + a - 8) / 4 + 1 : 0;
                for (uint32_t i = tid; i < nw; i += THREADS) s_buf[i] = (src4[i] >> sh) | (src4[i + 1] << (32 - sh));
            }
            for (uint32_t i = 4 * nw + tid; i < n; i += THREADS) s_text[i] = src[i];
        }
        for (uint32_t i = tid; i < TAB_WORDS; i += THREADS) s_tab[i] = 0;
        for (uint32_t i = tid; i < 288; i += THREADS) { s_ll_hist[i] = i == 256 ? 1u : 0u; s_dyn.ll_len[i] = 0; }
        if (tid < 32) { s_d_hist[tid] = 0; s_dyn.d_len[tid] = 0; }
        if (tid == 0) { s_carry = 0; s_nused[0] = s_nused[1] = 0; s_bits[0] = s_bits[1] = s_bits[2] = 0; }
        __syncthreads();

        // ---- matches and the greedy parse, 256 positions a step
        uint32_t ntok = 0;
        uint32_t nl1 = 0, nl2 = 0;                            // DEEP: 1 + the last and the second-to-last '\n' before the step
        for (uint32_t s0 = 0, par = 0; s0 < n; s0 += THREADS, par ^= 1) {
            const uint32_t p = s0 + tid;
            uint32_t L = 0, D = 0, cand = 0;
            if constexpr (DEEP) {
                const uint64_t m = __ballot(p < n && s_text[p] == '\n');
                if (lane == 0) s_nl[wave] = m;                // (read behind the barriers of the table's groups)
            }
            const bool hashed = p + 3 < n;
            const uint32_t h = hashed ? hash4(load4(s_text + p)) : 0;
            // look up, then insert, eight positions at a time in text order: a group's candidates are the positions of
            // the groups before it, two positions of one group with the same hash leave the larger (atomicMax).  Between
            // waves a barrier keeps that order; inside a wave the groups are eight masked sequences, kept apart by a
            // wave-level fence and executed in the order they were issued.  Were the groups ever merged into one, a
            // position would only lose the candidates of its own step's earlier groups: the bytes would still depend on
            // the text alone and decode to it, and the files would grow (the row before, 60 to 230 bytes back, is these
            // texts' nearest repeat) -- tools/gzip_device_bench.py's ratio against zlib level 1 shows it.
            for (uint32_t w = 0; w < THREADS / 64; w++) {
                if (wave == w)
                    for (uint32_t g = 0; g < 8; g++) {
                        if ((lane >> 3) == g && hashed) {
                            cand = __hip_atomic_load(&s_tab[h], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
                            atomicMax(&s_tab[h], p + 1);
                        }
                        __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
                    }
                __syncthreads();
            }
            uint32_t row = nl1, prev = nl2;                   // DEEP: s(p), r(p); then the carry of the next step
            if constexpr (DEEP) {
                for (uint32_t w = 0; w < wave; w++) push_newlines(s_nl[w], s0 + 64 * w, &row, &prev);
                push_newlines(s_nl[wave] & ((1ull << lane) - 1), s0 + 64 * wave, &row, &prev);
                if (p < n && p >= s_carry && !lit_only) deep_length(s_text, n, p, cand, row, prev, &L, &D);
                for (uint32_t w = 0; w < THREADS / 64; w++) push_newlines(s_nl[w], s0 + 64 * w, &nl1, &nl2);
            }
            if (!DEEP && cand && p >= s_carry && !lit_only) { // (a position inside the match carried in needs none)
                const uint32_t c = cand - 1, maxl = min(MAX_MATCH, n - p);
                uint32_t l = 0;
                while (l + 4 <= maxl && load4(s_text + c + l) == load4(s_text + p + l)) l += 4;
                while (l < maxl && s_text[c + l] == s_text[p + l]) l++;
                if (match_ok(l, p - c)) { L = l; D = p - c; }
            }
            s_mlen[par][tid] = (uint16_t)L; s_mdist[par][tid] = (uint16_t)(D ? D - 1 : 0);
            __syncthreads();
            if (tid == 0) {
                const uint32_t end = min(s0 + THREADS, n);
                uint32_t q = max(s0, s_carry), cnt = 0;
                while (q < end) {
                    uint32_t l = s_mlen[par][q - s0];
                    if constexpr (DEEP) {
                        if (l && q + 1 < n) {
                            uint32_t l1, d1;
                            if (q + 1 < end) l1 = s_mlen[par][q + 1 - s0];
                            else {
                                const uint32_t a = q + 4 < n ? __hip_atomic_load(&s_tab[hash4(load4(s_text + q + 1))], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP) : 0;
                                deep_length(s_text, n, q + 1, a, nl1, nl2, &l1, &d1);
                            }
                            if (deep_defers(l, l1)) s_mlen[par][q - s0] = (uint16_t)(l = 0);      // (a literal; behind the walk)
                        }
                    }
                    s_tokpos[par][cnt++] = (uint16_t)(q - s0);
                    q += l ? l : 1;
                }
                s_cnt[par] = cnt; s_carry = q;
            }
            __syncthreads();
            const uint32_t cnt = s_cnt[par];
            if (tid < cnt) {
                const uint32_t q = s_tokpos[par][tid], l = s_mlen[par][q];
                uint32_t tok;
                if (l) {
                    uint32_t eb, ev;
                    const uint32_t d = s_mdist[par][q];
                    tok = 0x80000000u | ((l - 3) << 16) | d;
                    atomicAdd(&s_ll_hist[len_sym(l, &eb, &ev)], 1u);
                    atomicAdd(&s_d_hist[dist_sym(d, &eb, &ev)], 1u);
                } else {
                    tok = s_text[s0 + q];
                    atomicAdd(&s_ll_hist[tok], 1u);
                }
                tokens[ntok + tid] = tok;
            }
            ntok += cnt;
        }
        __syncthreads();

        // ---- the chunk's CRC: a piece per thread, combined pairwise
        {
            const uint32_t at = tid * CRC_SUB, m = at < n ? min(CRC_SUB, n - at) : 0;
            s_crc[tid] = m ? crc32_bytes(s_text + at, m) : 0;
            s_crclen[tid] = m;
        }
        // ---- the dynamic codes: used symbols sorted by rank counting, then one lane per code
        rank_sort(s_ll_hist, N_LL, s_sort_ll, &s_nused[0], tid);
        rank_sort(s_d_hist, N_D, s_sort_d, &s_nused[1], tid);
        __syncthreads();
        for (uint32_t step = 1; step < THREADS; step <<= 1) {
            if ((tid & (2 * step - 1)) == 0 && s_crclen[tid + step]) {
                s_crc[tid] = s_crclen[tid] ? crc_combine(s_crc[tid], s_crc[tid + step], s_crclen[tid + step]) : s_crc[tid + step];
                s_crclen[tid] += s_crclen[tid + step];
            }
            if (step == 1) {
                if (tid == 0) { build_lengths(s_sort_ll, (int)s_nused[0], s_dyn.ll_len); canonical_codes(s_dyn.ll_len, N_LL, s_dyn.ll_code); }
                if (tid == 64) { build_lengths(s_sort_d, (int)s_nused[1], s_dyn.d_len); canonical_codes(s_dyn.d_len, N_D, s_dyn.d_code); }
            }
            __syncthreads();
        }
        // ---- the exact sizes of the block types
        {
            uint32_t b[3] = {0, 0, 0};
            for (uint32_t s = tid; s < N_LL; s += THREADS) ll_sym_bits(s, s_ll_hist[s], s_dyn, b);
            if (tid < N_D) d_sym_bits(tid, s_d_hist[tid], s_dyn, b);
            for (int k = 0; k < 3; k++) {
                uint32_t v = wave_inclusive_sum(b[k], lane);
                if (lane == 63 && v) atomicAdd(&s_bits[k], v);
            }
        }
        __syncthreads();
        uint32_t coded = 0;
        const uint32_t bits[3] = {s_bits[0], s_bits[1], s_bits[2]};
        const Mode mode = choose_mode(bits, n, P.flags, &coded);
        const uint32_t crc = s_crc[0], mbytes = member_bytes(coded);
        if (mode == STORED) {
            // the member straight from the staged text: head, 01 LEN NLEN, the bytes, CRC32, ISIZE
            if (tid < 23) {
                const uint8_t head[15] = {0x1F, 0x8B, 8, 0, 0, 0, 0, 0, 0, 0xFF, 1, (uint8_t)n, (uint8_t)(n >> 8), (uint8_t)~n, (uint8_t)(~n >> 8)};
                if (tid < 15) slot[tid] = head[tid];
                else if (tid < 19) slot[15 + n + (tid - 15)] = (uint8_t)(crc >> (8 * (tid - 15)));
                else slot[15 + n + (tid - 15)] = (uint8_t)(n >> (8 * (tid - 19)));
            }
            for (uint32_t i = tid; i < n; i += THREADS) slot[15 + i] = s_text[i];
        } else {
            __syncthreads();                                   // (the text's last readers: the CRC pieces, long done)
            for (uint32_t i = tid; i < SLOT_WORDS; i += THREADS) s_buf[i] = 0;
            if (mode == FIXED) {
                for (uint32_t s = tid; s < 288; s += THREADS) { s_dyn.ll_len[s] = (uint8_t)fixed_ll_len(s); s_dyn.ll_code[s] = (uint16_t)fixed_ll_code(s); }
                if (tid < 32) { s_dyn.d_len[tid] = 5; s_dyn.d_code[tid] = (uint16_t)bit_reverse(tid, 5); }
            }
            __syncthreads();
            uint32_t base = 8 * MEMBER_HEAD + 3 + (mode == DYNAMIC ? DYN_HEADER_FIXED_BITS + bits[2] : 0);
            if (tid == 0) {
                put_member_head(s_buf);
                put_bits(s_buf, 8 * MEMBER_HEAD, 1 | (uint32_t)mode << 1, 3);
                if (mode == DYNAMIC) (void)put_dyn_header(s_buf, 8 * MEMBER_HEAD + 3, s_dyn);
                put_member_tail(s_buf, coded, crc, n);
            }
            for (uint32_t r = 0, par = 0; r < ntok; r += THREADS, par ^= 1) {
                uint64_t val = 0;
                const uint32_t nb = r + tid < ntok ? token_bits(tokens[r + tid], s_dyn, &val) : 0;
                const uint32_t incl = wave_inclusive_sum(nb, lane);
                if (lane == 63) s_wsum[par][wave] = incl;
                __syncthreads();
                uint32_t before = 0, total = 0;
                for (uint32_t w = 0; w < 4; w++) { const uint32_t x = s_wsum[par][w]; total += x; before += w < wave ? x : 0; }
                // (the sizes are exact, so the tokens end where the count said; a bit past it would be a bug, never a write)
                if (base + before + incl <= 8 * MEMBER_HEAD + coded) put_bits(s_buf, base + before + incl - nb, val, nb);
                base += total;
            }
            if (tid == 0 && base + s_dyn.ll_len[256] <= 8 * MEMBER_HEAD + coded) put_bits(s_buf, base, s_dyn.ll_code[256], s_dyn.ll_len[256]);
            __syncthreads();
            uint32_t* slot4 = reinterpret_cast<uint32_t*>(slot);
            for (uint32_t i = tid; i < (mbytes + 3) / 4; i += THREADS) slot4[i] = s_buf[i];
        }
        if (tid == 0) P.sizes[chunk] = mbytes;
        __syncthreads();                                       // the next chunk's text goes where this one's member stood
    }
}

// offs[i] = *cursor + the sizes before chunk i; *cursor advances by their sum.  One workgroup; thread 0 alone reads and
// writes the cursor, the others get its value through LDS.  seg_first[s] = the offset of segment s's first chunk: chunk i
// is one if chunk i - 1 is another segment's (for the launch's first chunk the host says: first0).
// `frame`: the bytes the gather adds to every member's head (BGZF_EXTRA under PF_GZ_BGZF, else 0): every offset, every
// segment's first and the cursor then count the framed members.
__global__ __launch_bounds__(THREADS) void gz_scan_kernel(const uint32_t* sizes, const ChunkDesc* plan, uint32_t n, uint32_t first0,
                                                          uint64_t* offs, uint64_t* cursor, uint64_t* seg_first, uint32_t frame) {
    __shared__ uint32_t s_w[4];
    __shared__ uint64_t s_base;
    const uint32_t tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    if (tid == 0) s_base = *cursor;
    __syncthreads();
    uint64_t base = s_base;
    for (uint32_t r = 0; r < n; r += THREADS) {
        const uint32_t v = r + tid < n ? sizes[r + tid] + frame : 0, incl = wave_inclusive_sum(v, lane);
        if (lane == 63) s_w[wave] = incl;
        __syncthreads();
        uint32_t before = 0, total = 0;
        for (uint32_t w = 0; w < 4; w++) { total += s_w[w]; before += w < wave ? s_w[w] : 0; }
        if (r + tid < n) {
            const uint32_t i = r + tid, seg = plan[i].segment;
            offs[i] = base + before + incl - v;
            if (i ? plan[i - 1].segment != seg : first0 != 0) seg_first[seg] = base + before + incl - v;
        }
        base += total;
        __syncthreads();
    }
    if (tid == 0) *cursor = base;
}

// chunk i's member from its slot to members + offs[i]; a member that would pass `cap` is left out (the host sized the
// buffer for the worst case: it never is).  The bytes up to the destination's next 16-byte boundary and the last few go
// one by one, the rest in 16-byte units, stored aligned.  `frame` (BGZF_EXTRA under PF_GZ_BGZF, else 0): the member leaves
// as a BGZF member of m + frame bytes -- the 18-byte head made of the slot's plain one (bgzf_head_byte), then the slot's
// bytes from MEMBER_HEAD on, each `frame` bytes further back; the bytes that go one by one then cover that head.
__global__ __launch_bounds__(THREADS) void gz_gather_kernel(const uint8_t* slots, const uint32_t* sizes, const uint64_t* offs,
                                                            uint8_t* members, uint64_t cap, uint32_t frame) {
    const uint32_t chunk = blockIdx.x, m = sizes[chunk] + frame, tid = threadIdx.x;
    const uint64_t at = offs[chunk];
    if (at + m > cap) return;
    const uint8_t* src = slots + (size_t)chunk * SLOT_BYTES;
    uint8_t* dst = members + at;
    uint32_t head = (uint32_t)(-reinterpret_cast<uintptr_t>(dst) & 15);
    if (frame) {
        while (head < BGZF_HEAD) head += 16;                   // (at most 33 bytes: fewer than the threads)
        head = min(m, head);
        if (tid < head) dst[tid] = tid < BGZF_HEAD ? bgzf_head_byte(src, m, tid) : src[tid - frame];
    } else {
        head = min(m, head);
        if (tid < head) dst[tid] = src[tid];
    }
    src -= frame;                                              // (read at BGZF_HEAD and beyond only: src[MEMBER_HEAD ..] of the slot)
    const uint32_t nvec = (m - head) / 16, done = head + 16 * nvec;
    for (uint32_t i = tid; i < nvec; i += THREADS) {
        uint4 v;
        __builtin_memcpy(&v, src + head + 16 * i, 16);
        *reinterpret_cast<uint4*>(dst + head + 16 * i) = v;
    }
    if (done + tid < m) dst[done + tid] = src[done + tid];
}

// ---- the decoder.  gz_inflate_kernel: one wave (a workgroup of 64 threads) per member.  A member is a serial bit chain, so
// the wave's lanes all read the same bits (inflate_blocks, pf_deflate.h) and keep the same state; what the wave shares out
// is a token's work: a match's or a stored block's bytes go one per lane.  The member's text is built in a CHUNK-byte
// window in LDS: a match reads bytes that other lanes of the wave wrote a moment before, and in LDS the wave's accesses
// are served in the order they were issued -- a fence in front of every match copy keeps the compiler to that order and
// waits for the writes; nothing of this has to become visible through the caches of global memory.  The CRC32 is taken
// from the window, a piece per lane, the pieces combined by shuffles, and the text leaves in 16-byte stores.
// LDS: 32 KiB + 32 B of window, 1.3 KiB of tables -- four workgroups per CU within its 160 KiB; more waves per CU would
// need the window in HBM, and then every match would wait on a round trip through L2 for bytes its own wave just wrote.
// No wave waits for another: there is no barrier between workgroups, no flag, no loop without a bound.
//
// gz_inflate64_kernel: the same wave-per-member decode for the BGZF members of more than CHUNK bytes of text -- up to
// BGZF_MAX_TEXT = 65 536, what bgzip cuts a file into.  The member's whole text again stays in LDS while it is decoded:
// text offsets run to 65 535, a distance of 32 768 may reach from the window's second half into its first, a stored
// block may fill the member.  Its window of 64 KiB + 32 B and the tables are 66 592 bytes, over the 64 KiB a kernel
// may declare, so the LDS is dynamic and the limit is raised once per decoder (hipFuncSetAttribute).  Occupancy: two such
// workgroups fit a CU's 160 KiB, against four of gz_inflate_kernel -- half the resident waves for members of twice the
// text, so that per CU as many bytes are in flight; a third workgroup would need the window cut or kept in HBM.  So
// members of at most CHUNK bytes of text -- bgzip's last block of a file, the end marker, this project's own BGZF members
// -- keep the kernel of four per CU, and only the larger ones come here: two launches over one descriptor list, each
// with the list of its members' indices (`idx`; none: the launch's workgroup i takes member i).
constexpr uint32_t WIN_WORDS = CHUNK / 4 + 8;       // (the copy out reads up to four words past a 16-byte unit's first)
constexpr uint32_t WIN64_WORDS = BGZF_MAX_TEXT / 4 + 8;
constexpr uint32_t INFLATE64_LDS = WIN64_WORDS * 4 + (uint32_t)sizeof(DecodeTables);
static_assert(WIN64_WORDS * 4 % 16 == 0 && 2 * INFLATE64_LDS <= 160 * 1024, "the tables stand aligned behind the window; two workgroups per CU");

struct DecParams { const uint8_t* members; const DecMember* m; const uint32_t* idx; uint32_t n; uint8_t* text; DecResult* res; };

struct WaveSink {
    uint8_t* w; uint32_t lane;
    __device__ bool leader() const { return lane == 0; }
    __device__ void sync() { __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "workgroup"); __builtin_amdgcn_wave_barrier(); }
    __device__ uint32_t share(uint32_t v) const { return (uint32_t)__shfl((int)v, 0, 64); }
    __device__ void literal(uint32_t o, uint8_t b) { if (lane == 0) w[o] = b; }
    // byte o + i is byte o - dist + i mod dist: the bytes [o - dist, o) are all there before the copy starts, which is
    // what the byte-serial copy of an overlapping match (dist < len) comes to
    __device__ void copy(uint32_t o, uint32_t dist, uint32_t len) {
        sync();
        const uint8_t* from = w + o - dist;
        if (dist >= len) { for (uint32_t i = lane; i < len; i += 64) w[o + i] = from[i]; }
        else { for (uint32_t i = lane; i < len; i += 64) w[o + i] = from[i % dist]; }
    }
    __device__ void stored(uint32_t o, const uint8_t* src, uint32_t len) { for (uint32_t i = lane; i < len; i += 64) w[o + i] = src[i]; }
};

// one member by one wave: s_win holds MAX_TEXT bytes and the copy-out's slack, a member of more text is INF_TOO_LARGE
template <uint32_t MAX_TEXT>
__device__ __forceinline__ void inflate_member(const DecParams& P, uint32_t mi, uint32_t* s_win, DecodeTables& s_T, uint32_t lane) {
    const DecMember m = P.m[mi];
    uint8_t* win = reinterpret_cast<uint8_t*>(s_win);
    WaveSink sink{win, lane};
    uint32_t produced = 0;
    uint32_t st = m.isize <= MAX_TEXT ? inflate_blocks(P.members + m.src, m.csize, m.isize, s_T, sink, &produced) : (uint32_t)INF_TOO_LARGE;
    sink.sync();
    uint32_t crc = 0;
    if (st == INF_OK) {
        const uint32_t piece = (m.isize + 63) / 64, at = lane * piece;
        uint32_t len = at < m.isize ? min(piece, m.isize - at) : 0;
        crc = len ? crc32_bytes(win + at, len) : 0;
        for (uint32_t d = 1; d < 64; d <<= 1) {
            const uint32_t oc = (uint32_t)__shfl_down((int)crc, d, 64), ol = (uint32_t)__shfl_down((int)len, d, 64);
            if ((lane & (2 * d - 1)) == 0 && ol) { crc = len ? crc_combine(crc, oc, ol) : oc; len += ol; }
        }
        crc = (uint32_t)__shfl((int)crc, 0, 64);
        if (crc != m.crc) st = INF_BAD_CRC;
    }
    if (lane == 0) P.res[mi] = DecResult{st, produced, crc, 0};
    if (st != INF_OK) return;
    // the text to its place: single bytes up to the destination's next 16-byte boundary, 16-byte units, single bytes
    uint8_t* dst = P.text + m.dst;
    const uint32_t head = min(m.isize, (uint32_t)(-reinterpret_cast<uintptr_t>(dst) & 15));
    if (lane < head) dst[lane] = win[lane];
    const uint32_t nvec = (m.isize - head) / 16, done = head + 16 * nvec;
    for (uint32_t v = lane; v < nvec; v += 64) {
        const uint32_t s = head + 16 * v, wi = s >> 2, sh = 8 * (s & 3);
        uint32_t x[5];
        for (int k = 0; k < 5; k++) x[k] = s_win[wi + k];
        uint4 o;
        o.x = (uint32_t)((((uint64_t)x[1] << 32) | x[0]) >> sh); o.y = (uint32_t)((((uint64_t)x[2] << 32) | x[1]) >> sh);
        o.z = (uint32_t)((((uint64_t)x[3] << 32) | x[2]) >> sh); o.w = (uint32_t)((((uint64_t)x[4] << 32) | x[3]) >> sh);
        *reinterpret_cast<uint4*>(dst + s) = o;
    }
    if (done + lane < m.isize) dst[done + lane] = win[done + lane];
}

__global__ __launch_bounds__(64) void gz_inflate_kernel(DecParams P) {
    __shared__ uint32_t s_win[WIN_WORDS];
    __shared__ DecodeTables s_T;
    if (blockIdx.x >= P.n) return;
    inflate_member<CHUNK>(P, P.idx ? P.idx[blockIdx.x] : blockIdx.x, s_win, s_T, threadIdx.x);
}

__global__ __launch_bounds__(64) void gz_inflate64_kernel(DecParams P) {
    extern __shared__ __align__(16) uint32_t s_dyn64[];          // WIN64_WORDS of window, then the tables: INFLATE64_LDS bytes
    if (blockIdx.x >= P.n) return;
    inflate_member<BGZF_MAX_TEXT>(P, P.idx[blockIdx.x], s_dyn64, *reinterpret_cast<DecodeTables*>(s_dyn64 + WIN64_WORDS), threadIdx.x);
}

// ---- large members (pf_deflate.h: large_call): the four passes.  Every loop is bounded by the input's bits or by a cap on
// the output stated where it is passed; every offset into a ring is masked, every text write stands under inflate_run's
// cap, which is the piece's own size.
//
// gz_find_kernel: one wave per cut, a lane per bit offset, 64 offsets at a time, until one lane's offset holds a dynamic
// block's header (block_start_ok) or the next cut comes.  The tables a lane builds to judge a header are its own (scratch).
__global__ __launch_bounds__(64) void gz_find_kernel(const uint8_t* p, uint32_t n, const uint64_t* cuts, uint32_t n_cuts, uint32_t piece_bytes,
                                                      uint64_t* hit) {
    const uint32_t k = blockIdx.x, lane = threadIdx.x;
    if (k >= n_cuts) return;
    DecodeTables T;
    const uint64_t from = cuts[k] * 8, end = min((uint64_t)n, cuts[k] + piece_bytes) * 8;
    uint64_t found = ~0ull;
    for (uint64_t base = from; base < end; base += 64) {
        const uint64_t bit = base + lane;
        const bool ok = bit < end && block_start_ok(p, n, bit, T);
        const uint64_t m = __ballot(ok);
        if (m) { found = base + (uint64_t)(__ffsll((long long)m) - 1); break; }
    }
    if (lane == 0) hit[k] = found;
}

// the wave's form of HostRing: a match copy spread over the lanes.  In the ring a copy's sources never stand where an
// earlier lane's destination does: a source WINDOW - d entries before a destination (distances near WINDOW) is read by a
// lower lane index than the one that writes it, in the same or an earlier step of the loop
template <class E> struct WaveRing {
    E* w; uint8_t* text; uint32_t lane;
    __device__ bool leader() const { return lane == 0; }
    __device__ void sync() { __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "workgroup"); __builtin_amdgcn_wave_barrier(); }
    __device__ uint32_t share(uint32_t v) const { return (uint32_t)__shfl((int)v, 0, 64); }
    __device__ void put(uint32_t o, E v) { w[o & WMASK] = v; if (text) text[o] = (uint8_t)v; }
    __device__ void literal(uint32_t o, uint8_t b) { if (lane == 0) put(o, b); }
    __device__ void copy(uint32_t o, uint32_t dist, uint32_t len) {
        sync();
        for (uint32_t i = lane; i < len; i += 64) put(o + i, w[(o - dist + (dist >= len ? i : i % dist)) & WMASK]);
    }
    // (a stored block may be longer than the ring: only its last WINDOW bytes stay in it)
    __device__ void stored(uint32_t o, const uint8_t* src, uint32_t len) {
        for (uint32_t i = lane; i < len; i += 64) {
            if (len - i <= WINDOW) w[(o + i) & WMASK] = src[i];
            if (text) text[o + i] = src[i];
        }
    }
};

// gz_marker_kernel: one wave per found start decodes without the text before it; its ring of WINDOW 16-bit entries (64 KiB
// of LDS, with the tables over what a kernel may declare: dynamic, two workgroups per CU as gz_inflate64_kernel) goes out
// as it stands when the run ends
constexpr uint32_t MARKER_LDS = WINDOW * 2 + (uint32_t)sizeof(DecodeTables);
static_assert(WINDOW * 2 % 16 == 0 && 2 * MARKER_LDS <= 160 * 1024, "the tables stand aligned behind the ring; two workgroups per CU");
__global__ __launch_bounds__(64) void gz_marker_kernel(const uint8_t* p, uint32_t n, const uint64_t* starts, uint32_t n_starts, PieceResult* res,
                                                        uint32_t* rings) {
    extern __shared__ __align__(16) uint32_t s_dynm[];           // WINDOW entries, then the tables: MARKER_LDS bytes
    const uint32_t i = blockIdx.x, lane = threadIdx.x;
    if (i >= n_starts) return;
    for (uint32_t j = lane; j < WINDOW / 2; j += 64) s_dynm[j] = (MARK | (2 * j)) | (MARK | (2 * j + 1)) << 16;
    WaveRing<uint16_t> sink{reinterpret_cast<uint16_t*>(s_dynm), nullptr, lane};
    sink.sync();
    const PieceResult R = marker_run(p, n, starts, n_starts, i, *reinterpret_cast<DecodeTables*>(s_dynm + WINDOW / 2), sink);
    sink.sync();
    if (lane == 0) res[i] = R;
    if (R.status != INF_OK) return;
    uint32_t* out = rings + (size_t)i * (WINDOW / 2);
    for (uint32_t j = lane; j < WINDOW / 2; j += 64) out[j] = s_dynm[j];
}

// gz_chain_kernel: one workgroup per chain -- per member whose first piece is in the call (chain_starts) -- walks its live
// pieces in order, WINDOW bytes a step: wins[0] is the window carried into the call, wins[i + 1] the one live piece i
// leaves.  A chain's first piece with no text before it reads no window, so no workgroup reads what another writes.
__global__ __launch_bounds__(1024) void gz_chain_kernel(const LivePiece* live, uint32_t n_live, const uint16_t* rings, uint8_t* wins) {
    __shared__ uint32_t s_from;
    if (threadIdx.x == 0) {
        uint32_t chain = 0, from = n_live;
        for (uint32_t i = 0; i < n_live; i++)
            if (chain_starts(live, i) && chain++ == blockIdx.x) { from = i; break; }
        s_from = from;
    }
    __syncthreads();
    for (uint32_t i = s_from; i < n_live && (i == s_from || !chain_starts(live, i)); i++) {
        const uint16_t* ring = rings + (size_t)live[i].piece * WINDOW;
        const uint8_t* before = live[i].hist ? wins + (size_t)i * WINDOW : nullptr;
        uint8_t* after = wins + (size_t)(i + 1) * WINDOW;
        for (uint32_t j = threadIdx.x; j < WINDOW; j += 1024) after[j] = chain_byte(ring, live[i].produced, before, j);
        __threadfence_block();
        __syncthreads();
    }
}

// gz_bytes_kernel: one wave per live piece decodes it again as bytes -- the window before it preset in LDS (32 KiB and the
// tables: four workgroups per CU, as gz_inflate_kernel), the text to its place as it is made -- and takes its CRC32
__global__ __launch_bounds__(64) void gz_bytes_kernel(const uint8_t* p, uint32_t n, const LivePiece* live, uint32_t n_live, const uint8_t* wins,
                                                       uint8_t* text, ByteResult* br) {
    __shared__ __align__(16) uint32_t s_ring[WINDOW / 4];
    __shared__ DecodeTables s_T;
    const uint32_t i = blockIdx.x, lane = threadIdx.x;
    if (i >= n_live) return;
    const LivePiece L = live[i];
    const uint4* before = reinterpret_cast<const uint4*>(wins + (size_t)i * WINDOW);
    for (uint32_t j = lane; j < WINDOW / 16; j += 64) reinterpret_cast<uint4*>(s_ring)[j] = before[j];
    uint8_t* dst = text + L.dst;
    WaveRing<uint8_t> sink{reinterpret_cast<uint8_t*>(s_ring), dst, lane};
    sink.sync();
    ByteResult B = byte_run(p, n, L, s_T, sink);
    __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "agent");           // (the lanes read back what other lanes wrote)
    __builtin_amdgcn_wave_barrier();
    if (B.status == INF_OK) {
        const uint32_t piece = (L.produced + 63) / 64, at = lane * piece;
        uint32_t len = at < L.produced ? min(piece, L.produced - at) : 0;
        uint32_t crc = len ? crc32_bytes(dst + at, len) : 0;
        for (uint32_t d = 1; d < 64; d <<= 1) {
            const uint32_t oc = (uint32_t)__shfl_down((int)crc, d, 64), ol = (uint32_t)__shfl_down((int)len, d, 64);
            if ((lane & (2 * d - 1)) == 0 && ol) { crc = len ? crc_combine(crc, oc, ol) : oc; len += ol; }
        }
        B.crc = crc;
    }
    if (lane == 0) br[i] = B;
}

}  // namespace pfgz

int PfGzEncoder::ensure(int n_cu) {
    const uint32_t grid = (uint32_t)std::max(1, n_cu) * 2;
    const uint64_t nch = BLOCK / pfgz::CHUNK;
    PFCHK(slots.ensure(nch * pfgz::SLOT_BYTES, true));
    PFCHK(sizes.ensure(nch * 4, true));
    PFCHK(offs.ensure(nch * 8, true));
    PFCHK(tokens.ensure((uint64_t)grid * pfgz::CHUNK * 4, true));
    for (int w = 0; w < N_CURSORS; w++) {                 // (a one-segment text of a launch; a longer plan grows them)
        PFCHK(plan_dev[w].ensure(nch * sizeof(pfgz::ChunkDesc), true));
        PFCHK(plan_pin[w].ensure(nch * sizeof(pfgz::ChunkDesc), true));
        PFCHK(seg_dev[w].ensure(64, true));
        PFCHK(seg_pin[w].ensure(64, true));
    }
    grid_cap = grid;
    return PF_OK;
}

int PfGzEncoder::encode(hipStream_t st, Cursor w, const char* text, uint64_t n, uint32_t flags, char* members, uint64_t cap,
                        hipEvent_t t0, hipEvent_t t1) {
    const uint64_t end = n;
    return encode_segments(st, w, text, n, &end, n ? 1 : 0, flags, members, cap, t0, t1);
}

int PfGzEncoder::encode_segments(hipStream_t st, Cursor w, const char* text, uint64_t n, const uint64_t* seg_end, uint64_t n_seg,
                                 uint32_t flags, char* members, uint64_t cap, hipEvent_t t0, hipEvent_t t1) {
    if (!grid_cap) return fail(PF_ERR_STATE, "gzip encoder: not set up");
    if (!pfgz::chunk_plan(seg_end, n_seg, n, plan))
        return fail(PF_ERR_ARG, "gzip encoder: the segment ends must not decrease and the last must be the text's size");
    // every chunk of the plan may fill its slot: the members' buffer holds them all, or nothing is launched
    if (plan.size() * (uint64_t)pfgz::SLOT_BYTES > cap)
        return fail(PF_ERR_ARG, "gzip encoder: %zu chunks in %llu segments do not fit a buffer of %llu bytes", plan.size(),
                    (unsigned long long)n_seg, (unsigned long long)cap);
    const size_t plan_bytes = plan.size() * sizeof(pfgz::ChunkDesc), seg_bytes = (size_t)(1 + n_seg) * 8;
    PFCHK(plan_dev[w].ensure(plan_bytes));
    PFCHK(plan_pin[w].ensure(plan_bytes));
    PFCHK(seg_dev[w].ensure(seg_bytes));
    PFCHK(seg_pin[w].ensure(seg_bytes));
    caps[w] = cap; n_segs[w] = n_seg;
    uint64_t* cursor = seg_dev[w].as<uint64_t>();
    uint64_t* seg_first = cursor + 1;
    const pfgz::ChunkDesc* dplan = plan_dev[w].as<pfgz::ChunkDesc>();
    if (plan_bytes) {
        memcpy(plan_pin[w].p, plan.data(), plan_bytes);
        HIPCHK(hipMemcpyAsync(plan_dev[w].p, plan_pin[w].p, plan_bytes, hipMemcpyHostToDevice, st));
    }
    if (t0) HIPCHK(hipEventRecord(t0, st));
    HIPCHK(hipMemsetAsync(cursor, 0, 8, st));
    if (n_seg) HIPCHK(hipMemsetAsync(seg_first, 0xFF, (size_t)n_seg * 8, st));      // (a segment without a chunk keeps this)
    const size_t per_launch = (size_t)(BLOCK / pfgz::CHUNK);
    const uint32_t frame = flags & PF_GZ_BGZF ? pfgz::BGZF_EXTRA : 0;       // (the encode kernel's members are the same either way)
    for (size_t c0 = 0; c0 < plan.size(); c0 += per_launch) {
        const uint32_t nch = (uint32_t)std::min(per_launch, plan.size() - c0);
        const uint32_t first0 = c0 == 0 || plan[c0 - 1].segment != plan[c0].segment;
        pfgz::EncParams P{reinterpret_cast<const uint8_t*>(text), dplan + c0, nch, flags, slots.as<uint8_t>(), sizes.as<uint32_t>(),
                          tokens.as<uint32_t>()};
        if (flags & PF_GZ_DEEP) hipLaunchKernelGGL(pfgz::gz_encode_kernel<true>, dim3(std::min(nch, grid_cap)), dim3(pfgz::THREADS), 0, st, P);
        else hipLaunchKernelGGL(pfgz::gz_encode_kernel<false>, dim3(std::min(nch, grid_cap)), dim3(pfgz::THREADS), 0, st, P);
        HIPCHK(hipGetLastError());
        hipLaunchKernelGGL(pfgz::gz_scan_kernel, dim3(1), dim3(pfgz::THREADS), 0, st, sizes.as<uint32_t>(), dplan + c0, nch, first0,
                           offs.as<uint64_t>(), cursor, seg_first, frame);
        HIPCHK(hipGetLastError());
        hipLaunchKernelGGL(pfgz::gz_gather_kernel, dim3(nch), dim3(pfgz::THREADS), 0, st, slots.as<uint8_t>(), sizes.as<uint32_t>(),
                           offs.as<uint64_t>(), reinterpret_cast<uint8_t*>(members), cap, frame);
        HIPCHK(hipGetLastError());
    }
    if (t1) HIPCHK(hipEventRecord(t1, st));
    HIPCHK(hipMemcpyAsync(seg_pin[w].p, cursor, seg_bytes, hipMemcpyDeviceToHost, st));
    return PF_OK;
}

int PfGzEncoder::member_bytes(Cursor w, uint64_t* z) const {
    if (!seg_pin[w].p) return fail(PF_ERR_STATE, "gzip encoder: not set up");
    *z = seg_pin[w].as<uint64_t>()[0];
    if (*z > caps[w]) return fail(PF_ERR_STATE, "device gzip: a text's members exceed their bound");
    return PF_OK;
}

int PfGzEncoder::segment_ends(Cursor w, uint64_t* member_end) const {
    uint64_t next = 0;
    PFCHK(member_bytes(w, &next));
    const uint64_t* first = seg_pin[w].as<uint64_t>() + 1;
    for (uint64_t i = n_segs[w]; i-- > 0;) {
        member_end[i] = next;
        if (first[i] != ~0ull) next = first[i];
    }
    return PF_OK;
}

int PfGzDecoder::decode(hipStream_t st, const uint8_t* bytes, const pfgz::MemberRef* ms, uint32_t n, uint8_t* text, uint64_t text_cap,
                        hipEvent_t t0, hipEvent_t t1) {
    if (n > MAX_MEMBERS) return fail(PF_ERR_ARG, "gzip decoder: more than %u members in a call", MAX_MEMBERS);
    n_last = n;
    if (!n) return PF_OK;
    const uint64_t lo = ms[0].at, hi = ms[n - 1].at + ms[n - 1].size;
    desc_host.resize(n);
    index_host.resize(n);
    uint64_t dst = 0;
    uint32_t n_small = 0, n_large = 0;
    for (uint32_t i = 0; i < n; i++) {
        const uint32_t head = ms[i].head;
        if (ms[i].status != pfgz::INF_OK || (head != pfgz::MEMBER_HEAD && head != pfgz::BGZF_HEAD) || ms[i].size < head + pfgz::MEMBER_TAIL ||
            ms[i].at + ms[i].size > hi || ms[i].at < lo || ms[i].isize > pfgz::BGZF_MAX_TEXT)
            return fail(PF_ERR_ARG, "gzip decoder: member %u was not listed as taken", i);
        desc_host[i] = pfgz::DecMember{ms[i].at - lo + head, dst, ms[i].size - head - pfgz::MEMBER_TAIL, ms[i].isize, ms[i].crc, 0};
        dst += ms[i].isize;
        // the members of at most CHUNK bytes of text from the front of the index list, the larger ones from its end
        if (ms[i].isize <= pfgz::CHUNK) index_host[n_small++] = i;
        else index_host[n - ++n_large] = i;
    }
    if (dst > text_cap) return fail(PF_ERR_ARG, "gzip decoder: the members' text exceeds its buffer");
    if (n_large && !large_ready) {
        HIPCHK(hipFuncSetAttribute(reinterpret_cast<const void*>(pfgz::gz_inflate64_kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                                   (int)pfgz::INFLATE64_LDS));
        large_ready = true;
    }
    const size_t desc_bytes = (size_t)n * sizeof(pfgz::DecMember), index_bytes = n_large ? (size_t)n * 4 : 0;
    PFCHK(members.ensure(hi - lo + 16));
    PFCHK(desc.ensure(desc_bytes + index_bytes));
    PFCHK(results.ensure((size_t)n * sizeof(pfgz::DecResult)));
    PFCHK(pin.ensure((size_t)n * sizeof(pfgz::DecResult)));
    HIPCHK(hipMemcpyAsync(members.p, bytes + lo, hi - lo, hipMemcpyHostToDevice, st));
    HIPCHK(hipMemcpyAsync(desc.p, desc_host.data(), desc_bytes, hipMemcpyHostToDevice, st));
    const uint32_t* index = reinterpret_cast<const uint32_t*>(desc.as<char>() + desc_bytes);
    if (index_bytes) HIPCHK(hipMemcpyAsync(desc.as<char>() + desc_bytes, index_host.data(), index_bytes, hipMemcpyHostToDevice, st));
    if (t0) HIPCHK(hipEventRecord(t0, st));
    // (a call without larger members is one launch over the descriptors as they stand, without an index list)
    pfgz::DecParams P{members.as<uint8_t>(), desc.as<pfgz::DecMember>(), n_large ? index : nullptr, n_small, text, results.as<pfgz::DecResult>()};
    if (n_small) {
        hipLaunchKernelGGL(pfgz::gz_inflate_kernel, dim3(n_small), dim3(64), 0, st, P);
        HIPCHK(hipGetLastError());
    }
    if (n_large) {
        P.idx = index + n_small; P.n = n_large;
        hipLaunchKernelGGL(pfgz::gz_inflate64_kernel, dim3(n_large), dim3(64), pfgz::INFLATE64_LDS, st, P);
        HIPCHK(hipGetLastError());
    }
    if (t1) HIPCHK(hipEventRecord(t1, st));
    HIPCHK(hipMemcpyAsync(pin.p, results.p, (size_t)n * sizeof(pfgz::DecResult), hipMemcpyDeviceToHost, st));
    return PF_OK;
}

int64_t PfGzDecoder::first_refused(uint32_t* status) const {
    const pfgz::DecResult* r = pin.as<pfgz::DecResult>();
    for (uint32_t i = 0; i < n_last; i++)
        if (r[i].status != pfgz::INF_OK) { *status = r[i].status; return i; }
    return -1;
}

// ---- the large-member route's passes on the device: each uploads what it needs, launches, and reads its small answer
// back behind a synchronisation -- the host decides between them (pfgz::large_call)
int PfGzLarge::begin(const uint8_t* bytes, uint64_t n) {
    if (n >= (1ull << 32)) return fail(PF_ERR_ARG, "gzip decoder: a call over 4 GiB of compressed bytes");
    if (!ready) {
        PFCHK(window.ensure(pfgz::WINDOW, true));
        HIPCHK(hipMemsetAsync(window.p, 0, pfgz::WINDOW, st));
        HIPCHK(hipFuncSetAttribute(reinterpret_cast<const void*>(pfgz::gz_marker_kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                                   (int)pfgz::MARKER_LDS));
        PFCHK(e0.ensure()); PFCHK(e1.ensure()); PFCHK(e2.ensure());
        ready = true;
    }
    limit = (uint32_t)n;
    PFCHK(data.ensure(n + 16));
    HIPCHK(hipMemcpyAsync(data.p, bytes, n, hipMemcpyHostToDevice, st));
    return PF_OK;
}

int PfGzLarge::find(const uint64_t* cuts, uint32_t n_cuts, uint32_t piece_bytes, uint64_t* hit) {
    PFCHK(d_cuts.ensure((size_t)n_cuts * 8));
    PFCHK(d_hits.ensure((size_t)n_cuts * 8));
    HIPCHK(hipMemcpyAsync(d_cuts.p, cuts, (size_t)n_cuts * 8, hipMemcpyHostToDevice, st));
    HIPCHK(hipEventRecord(e0, st));
    hipLaunchKernelGGL(pfgz::gz_find_kernel, dim3(n_cuts), dim3(64), 0, st, data.as<uint8_t>(), limit, d_cuts.as<uint64_t>(), n_cuts, piece_bytes,
                       d_hits.as<uint64_t>());
    HIPCHK(hipGetLastError());
    HIPCHK(hipEventRecord(e1, st));
    HIPCHK(hipMemcpyAsync(hit, d_hits.p, (size_t)n_cuts * 8, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    float t = 0;
    if (hipEventElapsedTime(&t, e0, e1) == hipSuccess) ms[0] += t;
    return PF_OK;
}

int PfGzLarge::marker(const uint64_t* starts, uint32_t n_starts, pfgz::PieceResult* res) {
    PFCHK(d_starts.ensure((size_t)n_starts * 8));
    PFCHK(d_res.ensure((size_t)n_starts * sizeof(pfgz::PieceResult)));
    PFCHK(rings.ensure((size_t)n_starts * pfgz::WINDOW * 2));
    HIPCHK(hipMemcpyAsync(d_starts.p, starts, (size_t)n_starts * 8, hipMemcpyHostToDevice, st));
    HIPCHK(hipEventRecord(e0, st));
    hipLaunchKernelGGL(pfgz::gz_marker_kernel, dim3(n_starts), dim3(64), pfgz::MARKER_LDS, st, data.as<uint8_t>(), limit, d_starts.as<uint64_t>(),
                       n_starts, d_res.as<pfgz::PieceResult>(), rings.as<uint32_t>());
    HIPCHK(hipGetLastError());
    HIPCHK(hipEventRecord(e1, st));
    HIPCHK(hipMemcpyAsync(res, d_res.p, (size_t)n_starts * sizeof(pfgz::PieceResult), hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    float t = 0;
    if (hipEventElapsedTime(&t, e0, e1) == hipSuccess) ms[1] += t;
    return PF_OK;
}

int PfGzLarge::bytes_pass(const pfgz::LivePiece* live, uint32_t n_live, uint64_t text_n, pfgz::ByteResult* br) {
    uint8_t* text = nullptr;
    PFCHK(place(text_n, &text));
    PFCHK(d_live.ensure((size_t)n_live * sizeof(pfgz::LivePiece)));
    PFCHK(d_br.ensure((size_t)n_live * sizeof(pfgz::ByteResult)));
    PFCHK(wins.ensure((size_t)(n_live + 1) * pfgz::WINDOW));
    HIPCHK(hipMemcpyAsync(d_live.p, live, (size_t)n_live * sizeof(pfgz::LivePiece), hipMemcpyHostToDevice, st));
    HIPCHK(hipMemcpyAsync(wins.p, window.p, pfgz::WINDOW, hipMemcpyDeviceToDevice, st));
    HIPCHK(hipEventRecord(e0, st));
    uint32_t n_chains = 0;
    for (uint32_t i = 0; i < n_live; i++) n_chains += pfgz::chain_starts(live, i) ? 1 : 0;
    hipLaunchKernelGGL(pfgz::gz_chain_kernel, dim3(n_chains), dim3(1024), 0, st, d_live.as<pfgz::LivePiece>(), n_live, rings.as<uint16_t>(), wins.as<uint8_t>());
    HIPCHK(hipGetLastError());
    HIPCHK(hipEventRecord(e1, st));
    hipLaunchKernelGGL(pfgz::gz_bytes_kernel, dim3(n_live), dim3(64), 0, st, data.as<uint8_t>(), limit, d_live.as<pfgz::LivePiece>(), n_live,
                       wins.as<uint8_t>(), text, d_br.as<pfgz::ByteResult>());
    HIPCHK(hipGetLastError());
    HIPCHK(hipEventRecord(e2, st));
    HIPCHK(hipMemcpyAsync(window.p, wins.as<uint8_t>() + (size_t)n_live * pfgz::WINDOW, pfgz::WINDOW, hipMemcpyDeviceToDevice, st));
    HIPCHK(hipMemcpyAsync(br, d_br.p, (size_t)n_live * sizeof(pfgz::ByteResult), hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    float t = 0;
    if (hipEventElapsedTime(&t, e0, e1) == hipSuccess) ms[2] += t;
    if (hipEventElapsedTime(&t, e1, e2) == hipSuccess) ms[3] += t;
    return PF_OK;
}

extern "C" {

uint32_t pf_gzip_device_chunk_bytes(void) { return pfgz::CHUNK; }

int pf_gunzip_host_model_large(const char* members, uint64_t n, uint32_t piece_bytes, char** out, uint64_t* out_n, int* taken, uint64_t* pieces) {
    if ((!members && n) || !out || !out_n || !taken) return fail(PF_ERR_ARG, "pf_gunzip_host_model_large: null argument");
    *out = nullptr; *out_n = 0; *taken = 0;
    if (piece_bytes && piece_bytes < pfgz::PIECE_MIN) return fail(PF_ERR_ARG, "pf_gunzip_host_model_large: piece_bytes is 0 or at least %u", pfgz::PIECE_MIN);
    std::vector<uint8_t> text;
    pfgz::LargeStats stats;
    uint64_t bad = 0;
    uint32_t status = 0;
    const bool ok = pfgz::host_inflate_large(reinterpret_cast<const uint8_t*>(members), n, piece_bytes, text, stats, &bad, &status);
    if (pieces) { pieces[0] = stats.found; pieces[1] = stats.live; pieces[2] = stats.dropped; pieces[3] = stats.members; }
    if (!ok) {
        (void)fail(PF_OK, "pf_gunzip_host_model_large: not taken: member %llu: %s", (unsigned long long)bad, pfgz::inf_status_name(status));
        return PF_OK;
    }
    char* buf = (char*)malloc(text.size() ? text.size() : 1);
    if (!buf) return fail(PF_ERR_OOM, "pf_gunzip_host_model_large: out of memory");
    if (!text.empty()) memcpy(buf, text.data(), text.size());
    *out = buf; *out_n = text.size(); *taken = 1;
    return PF_OK;
}

int pf_gzip_host_model(const char* data, uint64_t n, uint32_t flags, char** out, uint64_t* out_n) {
    if ((!data && n) || !out || !out_n) return fail(PF_ERR_ARG, "pf_gzip_host_model: null argument");
    *out = nullptr; *out_n = 0;
    std::vector<uint8_t> members;
    if (!pfgz::host_model(reinterpret_cast<const uint8_t*>(data), n, flags, members))
        return fail(PF_ERR_STATE, "pf_gzip_host_model: a block's size differs from its count");
    char* buf = (char*)malloc(members.size() ? members.size() : 1);
    if (!buf) return fail(PF_ERR_OOM, "pf_gzip_host_model: out of memory");
    if (!members.empty()) memcpy(buf, members.data(), members.size());
    *out = buf; *out_n = members.size();
    return PF_OK;
}

int pf_gzip_host_model_segments(const char* data, uint64_t n, const uint64_t* seg_end, uint64_t n_seg, uint32_t flags, char** out,
                                uint64_t* out_n, uint64_t* member_end) {
    if ((!data && n) || (!seg_end && n_seg) || (!member_end && n_seg) || !out || !out_n)
        return fail(PF_ERR_ARG, "pf_gzip_host_model_segments: null argument");
    *out = nullptr; *out_n = 0;
    std::vector<uint8_t> members;
    const int rc = pfgz::host_model_segments(reinterpret_cast<const uint8_t*>(data), n, seg_end, n_seg, flags, members, member_end);
    if (rc == 1) return fail(PF_ERR_ARG, "pf_gzip_host_model_segments: the segment ends must not decrease and the last must be n");
    if (rc) return fail(PF_ERR_STATE, "pf_gzip_host_model_segments: a block's size differs from its count");
    char* buf = (char*)malloc(members.size() ? members.size() : 1);
    if (!buf) return fail(PF_ERR_OOM, "pf_gzip_host_model_segments: out of memory");
    if (!members.empty()) memcpy(buf, members.data(), members.size());
    *out = buf; *out_n = members.size();
    return PF_OK;
}

int pf_gunzip_host_model(const char* members, uint64_t n, char** out, uint64_t* out_n, int* taken) {
    if ((!members && n) || !out || !out_n || !taken) return fail(PF_ERR_ARG, "pf_gunzip_host_model: null argument");
    *out = nullptr; *out_n = 0; *taken = 0;
    std::vector<uint8_t> text;
    uint64_t bad = 0;
    uint32_t status = 0;
    if (!pfgz::host_inflate_model(reinterpret_cast<const uint8_t*>(members), n, text, &bad, &status)) {
        (void)fail(PF_OK, "pf_gunzip_host_model: not taken: member %llu: %s", (unsigned long long)bad, pfgz::inf_status_name(status));
        return PF_OK;
    }
    char* buf = (char*)malloc(text.size() ? text.size() : 1);
    if (!buf) return fail(PF_ERR_OOM, "pf_gunzip_host_model: out of memory");
    if (!text.empty()) memcpy(buf, text.data(), text.size());
    *out = buf; *out_n = text.size(); *taken = 1;
    return PF_OK;
}

int pf_gunzip_host_model_bgzf(const char* members, uint64_t n, char** out, uint64_t* out_n, int* taken) {
    if ((!members && n) || !out || !out_n || !taken) return fail(PF_ERR_ARG, "pf_gunzip_host_model_bgzf: null argument");
    *out = nullptr; *out_n = 0; *taken = 0;
    std::vector<uint8_t> text;
    uint64_t bad = 0;
    uint32_t status = 0;
    if (!pfgz::host_inflate_model_bgzf(reinterpret_cast<const uint8_t*>(members), n, text, &bad, &status)) {
        (void)fail(PF_OK, "pf_gunzip_host_model_bgzf: not taken: member %llu: %s", (unsigned long long)bad, pfgz::inf_status_name(status));
        return PF_OK;
    }
    char* buf = (char*)malloc(text.size() ? text.size() : 1);
    if (!buf) return fail(PF_ERR_OOM, "pf_gunzip_host_model_bgzf: out of memory");
    if (!text.empty()) memcpy(buf, text.data(), text.size());
    *out = buf; *out_n = text.size(); *taken = 1;
    return PF_OK;
}

}  // extern "C"
