// pf_rowfilter.hip -- SURVEY 8f row N4: the row filter of the reference's downstream tools on the device.
//
//   panfeed-get-clusters  /root/reference/panfeed/get_clusters.py:89-94   rows of kmers_to_hashes.tsv whose
//                                                                          hashed_pattern is in a set of hashes
//   panfeed-get-kmers     /root/reference/panfeed/get_kmers.py:103-106    the same, and
//                         /root/reference/panfeed/get_kmers.py:131-134    rows of kmers.tsv whose cluster is in a set
//
// The reference streams the file through pandas in 100 000-row chunks and keeps `x[x[col].isin(keys)]`.  Here a block
// of the file's text goes to HBM as it is; every thread looks at 16 bytes, and for every line end it finds there it
// hashes that line's key field (the LAST field of the line for hashed_pattern -- 24 base64 characters -- or the FIRST
// field of the line that starts behind it for cluster), probes a device hash set of the keys' 64-bit hashes and appends
// the position to a list.  The host then checks every candidate against the exact key strings (so a 64-bit hash
// collision cannot add a row) and hands back the matching lines in file order.  Byte work, HBM/PCIe-bound; no parsing
// of the other fields.
#include <hip/hip_runtime.h>

#include "../../include/panfeed_hip.h"
#include "pf_buf.h"
#include "pf_deflate.h"
#include "pf_host.h"

#include <algorithm>
#include <cstdio>
#include <cstring>
#include <memory>
#include <string>
#include <string_view>
#include <unordered_set>
#include <thread>
#include <vector>

namespace {

constexpr uint64_t RF_EMPTY = 0;
constexpr uint32_t RF_MAX_FIELD = 4096;       // a key field longer than this never matches (nor do the keys)

__host__ __device__ inline uint64_t rf_hash_step(uint64_t h, unsigned char c) { return (h ^ c) * 0x100000001B3ull; }
// weak-hash test build (-DPF_WEAK_HASH, see pf_kernels.h): the key / name hash keeps only the bits of a mask that the host
// and the device copy of rf_hash_fin read alike; rejected candidates are counted
#ifdef PF_WEAK_HASH
static __device__ unsigned long long rf_wh_mask = ~0ull;
static __device__ unsigned long long rf_wh_strain_rejects;
static uint64_t rf_wh_mask_host = ~0ull;
static uint64_t rf_wh_rowfilter_rejects;
#if defined(__HIP_DEVICE_COMPILE__)
#define RF_WEAK(h) ((h) & rf_wh_mask)
#else
#define RF_WEAK(h) ((h) & rf_wh_mask_host)
#endif
#else
#define RF_WEAK(h) (h)
#endif
__host__ __device__ inline uint64_t rf_hash_fin(uint64_t h) {
    h ^= h >> 32; h *= 0xD6E8FEB86659FD93ull; h ^= h >> 32;
    h = RF_WEAK(h);
    return h ? h : 1;                                   // 0 marks an empty slot
}
inline uint64_t rf_hash(const char* s, size_t n) {
    uint64_t h = 0xCBF29CE484222325ull;
    for (size_t i = 0; i < n; i++) h = rf_hash_step(h, (unsigned char)s[i]);
    return rf_hash_fin(h);
}

struct RfParams {
    const unsigned char* text;   // device copy of the block
    uint64_t n;                  // bytes of complete lines (text[n - 1] == '\n')
    const uint64_t* set;         // open addressing, RF_EMPTY = free
    uint64_t cap;                // power of two
    int first_field;             // 1: key = first field of the line; 0: last field
    uint64_t* out;               // candidate positions: first_field ? line start : position of the line's '\n'
    unsigned long long* count;
    uint64_t out_cap;
};

__device__ __forceinline__ bool rf_probe(const RfParams& p, uint64_t h) {
    uint64_t slot = h & (p.cap - 1);
    for (uint64_t probes = 0; probes < p.cap; probes++) {
        const uint64_t cur = p.set[slot];
        if (cur == h) return true;
        if (cur == RF_EMPTY) return false;
        slot = (slot + 1) & (p.cap - 1);
    }
    return false;
}

// one line whose key field is to be tested; `at` = position of the '\n' that ends it (last field) or of the
// '\n' in front of it (first field; -1 for the line at the start of the block)
__device__ __forceinline__ void rf_line(const RfParams& p, int64_t at) {
    uint64_t h = 0xCBF29CE484222325ull;
    uint64_t pos;
    if (p.first_field) {
        const uint64_t s = (uint64_t)(at + 1);
        if (s >= p.n) return;
        uint64_t e = s;
        while (e < p.n && e - s < RF_MAX_FIELD && p.text[e] != '\t' && p.text[e] != '\n') { h = rf_hash_step(h, p.text[e]); e++; }
        if (e - s >= RF_MAX_FIELD) return;
        pos = s;
    } else {
        if (at < 0) return;
        int64_t s = at;                                  // field = (s, at)
        while (s > 0 && at - s < (int64_t)RF_MAX_FIELD && p.text[s - 1] != '\t' && p.text[s - 1] != '\n') s--;
        if (at - s >= (int64_t)RF_MAX_FIELD) return;
        for (int64_t i = s; i < at; i++) h = rf_hash_step(h, p.text[i]);
        pos = (uint64_t)at;
    }
    if (!rf_probe(p, rf_hash_fin(h))) return;
    const unsigned long long k = atomicAdd(p.count, 1ull);
    if (k < p.out_cap) p.out[k] = pos;
}

// the bytes of a 32-bit word that are '\n', as bit 7 of each such byte.  The sum never carries from one byte into the
// next (both operands have bit 7 clear), so a byte is flagged by its own value alone: the shorter (x - 0x01010101) & ~x
// form lets the borrow of a matching byte flag a 0x0B that stands above it in the word
__device__ __forceinline__ uint32_t rf_newlines(uint32_t w) {
    const uint32_t x = w ^ 0x0A0A0A0Au;
    return ~(((x & 0x7F7F7F7Fu) + 0x7F7F7F7Fu) | x) & 0x80808080u;
}

// line_end(at) for every '\n' of the 16 bytes at text + 16 * v, in their order.  The caller sees to v < ceil(n / 16) and to a
// buffer that reaches to the next multiple of 16 bytes, padded with zeros, and tests `at` against its own bound
template <class F> __device__ __forceinline__ void rf_each_newline(const unsigned char* text, uint64_t v, F&& line_end) {
    const uint4 w = reinterpret_cast<const uint4*>(text)[v];
    const uint32_t ws[4] = {w.x, w.y, w.z, w.w};
#pragma unroll
    for (int q = 0; q < 4; q++) {
        uint32_t m = rf_newlines(ws[q]);
        while (m) {
            const int b = (__ffs((int)m) - 1) >> 3;
            m &= m - 1;
            line_end(v * 16 + q * 4 + b);
        }
    }
}

__global__ __launch_bounds__(256) void rowfilter_kernel(RfParams p) {
    const uint64_t nvec = (p.n + 15) / 16;
    for (uint64_t v = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x; v < nvec; v += (uint64_t)gridDim.x * blockDim.x) {
        if (v == 0 && p.first_field) rf_line(p, -1);     // the line that starts the block
        rf_each_newline(p.text, v, [&](uint64_t at) { if (at < p.n) rf_line(p, (int64_t)at); });
    }
}

// ---- the scan of text that never was on the host (pf_rowfilter_scan_members): where its complete lines end, and the
// candidates' lines gathered into one buffer for the host's exact check
// out[0] = bytes of complete lines of text[0 .. total), out[1] = total; with `last`, a final line without a newline is
// given one first (the buffer has room for it).  One workgroup; it walks back from the end 4 096 bytes a step until a
// step holds a newline.
__global__ __launch_bounds__(256) void rf_tail_kernel(unsigned char* text, uint64_t total, int last, uint64_t* out) {
    __shared__ unsigned long long s_best;
    const uint32_t tid = threadIdx.x;
    if (last && total && text[total - 1] != '\n') {       // (every thread reads the same byte: the branch is uniform)
        if (tid == 0) { text[total] = '\n'; out[0] = total + 1; out[1] = total + 1; }
        return;
    }
    if (tid == 0) s_best = 0;
    __syncthreads();
    for (uint64_t end = total; end > 0; end = end > 4096 ? end - 4096 : 0) {
        const uint64_t lo = end > 4096 ? end - 4096 : 0;
        const uint64_t a = lo + 16ull * tid, b = a + 16 < end ? a + 16 : end;
        for (uint64_t i = b; i > a; i--)
            if (text[i - 1] == '\n') { atomicMax(&s_best, (unsigned long long)i); break; }
        __syncthreads();
        const unsigned long long best = s_best;
        __syncthreads();                              // (nobody adds to it for the next step before all have read it)
        if (best) break;
    }
    if (tid == 0) { out[0] = s_best; out[1] = total; }
}

// the line of text[0 .. n) at a candidate's position -- its start (first_field) or its '\n' --: [*begin, *end), the
// newline part of it.  For the host's exact check of the plain route and, on the device, for the member route's gather
__host__ __device__ inline void rf_line_extent(const unsigned char* text, uint64_t n, uint64_t pos, int first_field,
                                               uint64_t* begin, uint64_t* end) {
    const uint64_t q = pos < n ? pos : n - 1;
    uint64_t b = q, e = q;
    if (first_field) { while (e < n && text[e] != '\n') e++; }
    else { while (b > 0 && text[b - 1] != '\n') b--; }
    *begin = b; *end = e + 1 <= n ? e + 1 : n;
}

__global__ __launch_bounds__(256) void rf_extent_kernel(const unsigned char* text, uint64_t n, const uint64_t* pos, uint64_t cnt,
                                                         int first_field, uint64_t* begin, uint64_t* end) {
    const uint64_t k = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x;
    if (k < cnt) rf_line_extent(text, n, pos[k], first_field, &begin[k], &end[k]);
}

// line k to lines + off[k]; a workgroup of 64 per line
__global__ __launch_bounds__(64) void rf_gather_kernel(const unsigned char* text, const uint64_t* begin, const uint64_t* end,
                                                        const uint64_t* off, unsigned char* lines) {
    const uint64_t k = blockIdx.x, b = begin[k], m = end[k] - b;
    for (uint64_t i = threadIdx.x; i < m; i += 64) lines[off[k] + i] = text[b + i];
}

// ---- what the row filter and the plot grid (below) own alike.  A block's text -- complete lines only, the caller carries
// the rest over -- on the device and the pinned buffer host text goes through.  The scans read 16 bytes at a time: d_text
// reaches to the next multiple of 16 bytes and 16 more; a buffer that is re-made gets an eighth more
struct BlockText {
    DevBuf d_text;
    PinBuf pin;
    static uint64_t complete_lines(const char* text, uint64_t n) { while (n && text[n - 1] != '\n') n--; return n; }
    static size_t padded(uint64_t bytes) { return (bytes + 15) / 16 * 16 + 16; }
    int reserve(uint64_t bytes, bool pinned_too = false) {
        const size_t want = padded(bytes);
        auto grow = [want](auto& buf) -> int { return want > buf.cap ? buf.ensure(want + want / 8, true) : PF_OK; };
        if (int rc = grow(d_text)) return rc;
        return pinned_too ? grow(pin) : PF_OK;
    }
    int upload(hipStream_t stream, const char* text, uint64_t n) {
        PFCHK(reserve(n, true));
        // into pinned memory on a few threads (one memcpy of 256 MB is slower than the rest of the call)
        char* const to = pin.as<char>();
        const unsigned nt = (unsigned)std::max<uint64_t>(1, std::min<uint64_t>(8, n >> 22));
        std::vector<std::thread> th;
        const uint64_t step = (n + nt - 1) / nt;
        for (unsigned t = 1; t < nt; t++) {
            const uint64_t a = t * step, b = std::min<uint64_t>(n, a + step);
            if (a < b) th.emplace_back([=] { memcpy(to + a, text + a, (size_t)(b - a)); });
        }
        memcpy(to, text, (size_t)std::min<uint64_t>(n, step));
        for (auto& t : th) t.join();
        memset(to + n, 0, padded(n) - n);
        HIPCHK(hipMemcpyAsync(d_text.p, pin.p, padded(n), hipMemcpyHostToDevice, stream));
        return PF_OK;
    }
};

// ---- TextFeed::members, stage by stage: what a call's plan, inflate and header stages find out
struct RfMembers {
    const uint8_t* bytes; uint64_t nbytes; bool last;     // the call's arguments
    std::vector<pfgz::MemberRef> ms;                     // plan: the members listed; how many of them this call takes,
    size_t take = 0; uint64_t text_n = 0, used = 0;      // their text's bytes, the compressed bytes they use up; whether the
    bool end = false, none_yet = false;                  // file's text ends with them; no whole member yet: the caller reads on
    uint64_t total = 0, n = 0;     // inflate: d_text[0 .. total) is the carried line and the members' text, [0 .. n) its complete lines
    uint64_t skip = 0;             // header: the header line's bytes: no line of it is a row
    bool refused = false;          // any of them: the block is not one for this route, "not taken"
    bool go_large = false;         // plan, inflate: not for the small-member kernels -- with the feed's switch on, the large-member route's
};

// Complete lines of a table's text on the device, text.d_text[0 .. n), for the row filter, the plot grid and the k-mer join
// alike.  A block comes as host text (plain) or as whole gzip members of the compressed file, inflated where they land
// (members): then the unfinished line is carried over on the device and the file's first line, the header line, is kept
// apart.  One stream, the owner's work included.  The owner declares the feed last (see TimedStream).
struct TextFeed {
    int device = 0;
    BlockText text;                            // the block
    PfGzDecoder dec;
    DevBuf d_carry, d_tail;                    // the unfinished line carried from one members call to the next; rf_tail_kernel's answer
    uint64_t carry_n = 0;
    bool want_header = false;
    std::string header;
    uint64_t gz_members = 0, gz_text_bytes = 0;
    float gz_ms = 0;
    // the large-member route (pf_deflate.h: large_call), off unless the owner's pf_*_set_large_members turns it on: the
    // member that is open between calls, the route's counters, its passes on the device
    bool large_on = false;
    uint32_t piece_bytes = 0;
    pfgz::LargeState lg_state;
    pfgz::LargeStats lg_stats;
    PfGzLarge lg;
    TimedStream ts;

    // the complete lines of host text: *n bytes of them, uploaded unless there are none.  `before(*n)`: what the owner has to
    // check and reserve for a block of that many bytes in front of the upload
    int plain(const char* t, uint64_t nbytes, uint64_t* n) { return plain(t, nbytes, n, [](uint64_t) { return PF_OK; }); }
    template <class F> int plain(const char* t, uint64_t nbytes, uint64_t* n, F&& before) {
        *n = BlockText::complete_lines(t, nbytes);
        if (!*n) return PF_OK;
        PFCHK(before(*n));
        return text.upload(ts.stream, t, *n);
    }

    // a file of members starts: nothing carried; with `with_header`, its first line is not a row
    int members_begin(int with_header) {
        carry_n = 0; want_header = with_header != 0; header.clear(); lg_state = pfgz::LargeState{};
        return PF_OK;
    }
    int set_large(int on, uint32_t piece) {
        if (piece && piece < pfgz::PIECE_MIN) return fail(PF_ERR_ARG, "set_large_members: piece_bytes is 0 (the default) or at least %u", pfgz::PIECE_MIN);
        large_on = on != 0; piece_bytes = piece; lg_state = pfgz::LargeState{};
        return PF_OK;
    }
    // that line, with its newline, once a members call has seen it (the messages are the row filter's for every owner)
    int header_line(const char** line, uint64_t* nbytes) const {
        if (!line || !nbytes) return fail(PF_ERR_ARG, "pf_rowfilter_members_header: null argument");
        *line = header.data(); *nbytes = header.size();
        return PF_OK;
    }

    // A block of the compressed file from a member start on.  *taken = 0, with PF_OK and the reason as the error text:
    // the block is not one for this route.  Else
    // `work(n, skip)` has scanned the lines of d_text[skip .. n) and *consumed compressed bytes are used up; none of them,
    // and no work, while the block holds no whole member yet: the caller reads on
    template <class F> int members(const char* bytes, uint64_t nbytes, int last, uint64_t* consumed, int* taken, F&& work) {
        *consumed = 0; *taken = 0;
        RfMembers c{reinterpret_cast<const uint8_t*>(bytes), nbytes, last != 0};
        // a member of the large route that is open goes on there; else the block's head and its listed members say which
        // route takes it, and what the small-member kernels refuse the large route tries from the block's first byte
        c.go_large = large_on && lg_state.open;
        if (!c.go_large) {
            PFCHK(plan(c));
            if (!c.go_large && (c.refused || c.none_yet)) { *taken = !c.refused; return PF_OK; }
            if (!c.go_large) PFCHK(inflate(c));
        }
        if (c.go_large) {
            PFCHK(inflate_large(c));
            if (c.refused || c.none_yet) { *taken = !c.refused; return PF_OK; }
        }
        if (!c.refused) PFCHK(peel_header(c));
        if (c.refused) return PF_OK;
        gz_members += c.take; gz_text_bytes += c.text_n;
        PFCHK(work(c.n, c.skip));
        PFCHK(save_carry(c));
        *consumed = c.used; *taken = 1;
        return PF_OK;
    }

private:
    // (whatever refuses the block leaves no line carried: the caller starts over another way)
    // what the small-member route's plan and inflate stages refuse: with the switch on it is the large route's to try, from
    // the block's first byte; a refusal for real otherwise
    int reroute(RfMembers& c, uint64_t member, uint32_t status) {
        if (large_on && !c.go_large) { c.go_large = true; return PF_OK; }
        return refuse(c, member, status);
    }
    int refuse(RfMembers& c, uint64_t member, uint32_t status) {
        carry_n = 0; c.refused = true; lg_state = pfgz::LargeState{};
        return fail(PF_OK, "pf_rowfilter_scan_members: not taken: member %llu of the block: %s", (unsigned long long)member,
                    pfgz::inf_status_name(status));
    }

    int plan(RfMembers& c) {
        uint64_t listed = 0;
        // the block's first head says which container it is: a BGZF head (FLG = 4 with the one BC subfield) has the
        // members listed by their BSIZE chain, anything else by the signature search, as ever
        const bool bgzf = pfgz::bgzf_head_ok(c.bytes, c.nbytes);
        if (!(bgzf ? pfgz::list_members_bgzf(c.bytes, c.nbytes, c.last, c.ms, &listed) : pfgz::list_members(c.bytes, c.nbytes, c.last, c.ms, &listed)))
            return reroute(c, 0, pfgz::INF_BAD_HEAD);
        const bool none = c.ms.empty() && !c.last;
        // a member this decoder takes would have ended by now
        if (none && c.nbytes >= (bgzf ? pfgz::BGZF_MAX_MEMBER : pfgz::SLOT_BYTES + pfgz::MEMBER_HEAD)) return reroute(c, 0, pfgz::INF_TOO_LARGE);
        if (none) { c.none_yet = true; return PF_OK; }
        // at most the decoder's call: the rest is the caller's to give again
        while (c.take < c.ms.size() && c.take < PfGzDecoder::MAX_MEMBERS) {
            if (c.ms[c.take].status != pfgz::INF_OK && large_on && c.take) break;      // (the run before it now, that member in a call of its own)
            if (c.ms[c.take].status != pfgz::INF_OK) return reroute(c, c.take, c.ms[c.take].status);
            if (c.take && c.text_n + c.ms[c.take].isize > PfGzDecoder::MAX_TEXT) break;
            c.text_n += c.ms[c.take].isize; c.take++;
        }
        const bool all = c.take == c.ms.size();
        c.used = all ? listed : c.ms[c.take].at;
        c.end = c.last && all;
        return PF_OK;
    }

    // the device text: the line carried over, then the members' text; room for a final newline.  Where its complete lines end
    int inflate(RfMembers& c) {
        hipStream_t st = ts.stream;
        c.total = carry_n + c.text_n;
        PFCHK(text.reserve(c.total + 1));
        PFCHK(d_tail.ensure(16, true));
        unsigned char* const to = text.d_text.as<unsigned char>();
        if (carry_n) HIPCHK(hipMemcpyAsync(to, d_carry.p, carry_n, hipMemcpyDeviceToDevice, st));
        PFCHK(dec.decode(st, c.bytes, c.ms.data(), (uint32_t)c.take, to + carry_n, c.text_n, ts.e0, ts.e1));
        hipLaunchKernelGGL(rf_tail_kernel, dim3(1), dim3(256), 0, st, to, c.total, c.end ? 1 : 0, d_tail.as<uint64_t>());
        HIPCHK(hipGetLastError());
        uint64_t tail[2] = {0, 0};
        HIPCHK(hipMemcpyAsync(tail, d_tail.p, 16, hipMemcpyDeviceToHost, st));
        HIPCHK(hipStreamSynchronize(st));
        if (c.take) {
            ts.add_elapsed(&gz_ms);
            uint32_t status = 0;
            const int64_t bad = dec.first_refused(&status);
            if (bad >= 0) return reroute(c, (uint64_t)bad, status);
        }
        c.n = tail[0]; c.total = tail[1];
        return PF_OK;
    }

    // The same by the large-member route: one member, or as much of it as this call confirms, from the block's first byte
    // on; the text lands behind the carried line once the marker pass has told its size
    int inflate_large(RfMembers& c) {
        hipStream_t st = ts.stream;
        PFCHK(d_tail.ensure(16, true));
        lg.st = st;
        lg.place = [this, st](uint64_t text_n, uint8_t** dst) -> int {
            PFCHK(text.reserve(carry_n + text_n + 1));
            unsigned char* const to = text.d_text.as<unsigned char>();
            if (carry_n) HIPCHK(hipMemcpyAsync(to, d_carry.p, carry_n, hipMemcpyDeviceToDevice, st));
            *dst = to + carry_n;
            return PF_OK;
        };
        const float before = lg.ms[0] + lg.ms[1] + lg.ms[2] + lg.ms[3];
        const uint64_t members_before = lg_stats.members;
        pfgz::LargeOut o;
        PFCHK(pfgz::large_call(lg, lg_state, lg_stats, c.bytes, c.nbytes, c.last, piece_bytes, o));
        gz_ms += lg.ms[0] + lg.ms[1] + lg.ms[2] + lg.ms[3] - before;
        if (!o.taken) return refuse(c, 0, o.status);
        if (o.none_yet) { c.none_yet = true; return PF_OK; }
        c.take = (size_t)(lg_stats.members - members_before); c.text_n = o.text_n; c.used = o.consumed;
        c.end = c.last && o.consumed == c.nbytes;
        c.total = carry_n + c.text_n;
        return text_tail(c);
    }

    // where the complete lines of d_text[0 .. c.total) end; the file's last line gets its newline
    int text_tail(RfMembers& c) {
        hipStream_t st = ts.stream;
        unsigned char* const to = text.d_text.as<unsigned char>();
        hipLaunchKernelGGL(rf_tail_kernel, dim3(1), dim3(256), 0, st, to, c.total, c.end ? 1 : 0, d_tail.as<uint64_t>());
        HIPCHK(hipGetLastError());
        uint64_t tail[2] = {0, 0};
        HIPCHK(hipMemcpyAsync(tail, d_tail.p, 16, hipMemcpyDeviceToHost, st));
        HIPCHK(hipStreamSynchronize(st));
        c.n = tail[0]; c.total = tail[1];
        return PF_OK;
    }

    // the first call's first line is the header line
    int peel_header(RfMembers& c) {
        if (!want_header) return PF_OK;
        std::string front((size_t)std::min<uint64_t>(c.n, 1 << 16), '\0');
        if (!front.empty()) HIPCHK(hipMemcpy(&front[0], text.d_text.p, front.size(), hipMemcpyDeviceToHost));
        const size_t nl = front.find('\n');
        // (no line end: a header line over 64 KiB or over a call's text -- unless the file is empty)
        if (nl == std::string::npos && !(c.end && c.total == 0)) return refuse(c, 0, pfgz::INF_NOT_DECODED);
        if (nl != std::string::npos) { header.assign(front, 0, nl + 1); c.skip = nl + 1; }
        want_header = false;
        return PF_OK;
    }

    // the unfinished line stays on the device for the next call
    int save_carry(const RfMembers& c) {
        carry_n = c.total - c.n;
        if (!carry_n) return PF_OK;
        PFCHK(d_carry.ensure(carry_n));
        HIPCHK(hipMemcpyAsync(d_carry.p, text.d_text.as<char>() + c.n, carry_n, hipMemcpyDeviceToDevice, ts.stream));
        HIPCHK(hipStreamSynchronize(ts.stream));
        return PF_OK;
    }
};

// What the feed's owners' entry points pf_*_members_begin, pf_*_members_header and pf_*_gunzip_stats do, each under its own
// name `fn`.  H: an owner, a handle with a `feed`
template <class H> int feed_members_begin(H* h, const char* fn, int header) {
    return h ? h->feed.members_begin(header) : fail(PF_ERR_ARG, "%s: null argument", fn);
}
template <class H> int feed_members_header(H* h, const char* fn, const char** line, uint64_t* nbytes) {
    return h ? h->feed.header_line(line, nbytes) : fail(PF_ERR_ARG, "%s: null argument", fn);
}
template <class H> int feed_gunzip_stats(H* h, const char* fn, uint64_t* members, uint64_t* text_bytes, float* inflate_ms, uint64_t* device_bytes) {
    if (!h) return fail(PF_ERR_ARG, "%s: null argument", fn);
    if (members) *members = h->feed.gz_members;
    if (text_bytes) *text_bytes = h->feed.gz_text_bytes;
    if (inflate_ms) *inflate_ms = h->feed.gz_ms;
    if (device_bytes) *device_bytes = h->feed.dec.device_bytes() + h->feed.lg.device_bytes();
    return PF_OK;
}
// pf_*_set_large_members and pf_*_large_stats: the large-member route's switch and its counters -- pieces[4]: found starts,
// live pieces, dropped starts, members taken by the route; ms[4]: device time of the find, marker, chain and byte passes
template <class H> int feed_set_large(H* h, const char* fn, int on, uint32_t piece_bytes) {
    return h ? h->feed.set_large(on, piece_bytes) : fail(PF_ERR_ARG, "%s: null argument", fn);
}
template <class H> int feed_large_stats(H* h, const char* fn, uint64_t* pieces, float* ms) {
    if (!h) return fail(PF_ERR_ARG, "%s: null argument", fn);
    const pfgz::LargeStats& t = h->feed.lg_stats;
    if (pieces) { pieces[0] = t.found; pieces[1] = t.live; pieces[2] = t.dropped; pieces[3] = t.members; }
    if (ms) for (int i = 0; i < 4; i++) ms[i] = h->feed.lg.ms[i];
    return PF_OK;
}
// ... and what their pf_*_create and pf_*_destroy share.  Create: the device checked and made current, the handle made --
// destroyed again should the rest of its create fail -- and its feed's stream and events.  Destroy: on the handle's device
template <class H> using FeedHandle = std::unique_ptr<H, void (*)(H*)>;
template <class H> void feed_destroy(H* h) { if (h) { (void)hipSetDevice(h->feed.device); delete h; } }
template <class H> int feed_create(int device, const char* fn, FeedHandle<H>& h) {
    int ndev = 0;
    HIPCHK(hipGetDeviceCount(&ndev));
    if (device < 0 || device >= ndev) return fail(PF_ERR_ARG, "%s: no such device", fn);
    HIPCHK(hipSetDevice(device));
    h.reset(new H());
    h->feed.device = device;
    return h->feed.ts.create();
}

}  // namespace

struct pf_rowfilter {
    int first_field = 0;
    std::unordered_set<std::string> keys;
    std::string key;                           // a candidate's key field, for the look-up in keys
    DevBuf d_set;                              // the keys' hashes (uint64), cap slots
    uint64_t cap = 0;
    DevBuf d_out;                              // candidate positions (uint64)
    DevBuf d_count;
    std::vector<uint64_t> begin, end;          // result of the last scan
    uint64_t bytes_scanned = 0;
    float device_ms = 0;
    // pf_rowfilter_scan_members: the candidates' lines (extents and offsets on the device, the bytes on both sides), the kept lines
    DevBuf d_ext, d_lines;
    std::string raw_lines, lines;
    TextFeed feed;
};

namespace {

// The text is on the device -- the feed's d_text[0 .. n), complete lines -- scan it: the candidates' positions, sorted.  On
// the feed's stream, behind whatever put the text there.
int rf_scan_device(pf_rowfilter* f, uint64_t n, std::vector<uint64_t>& pos) {
    TimedStream& ts = f->feed.ts;
    // room for the candidates: the filter keeps few rows, so the room is a guess (a position per 64 bytes of text, a
    // million at least) and the kernel is run again with what it asked for should the guess be too small -- counting
    // the lines of the block on the host to size it for the worst case cost more than the kernel itself
    const size_t guess = std::max<size_t>((size_t)1 << 20, (size_t)(n / 64));
    PFCHK(f->d_out.ensure(guess * 8, true));
    unsigned long long cnt = 0;
    for (int attempt = 0; attempt < 2; attempt++) {
        HIPCHK(hipMemsetAsync(f->d_count.p, 0, 8, ts.stream));
        RfParams p{};
        p.text = f->feed.text.d_text.as<unsigned char>(); p.n = n; p.set = f->d_set.as<uint64_t>(); p.cap = f->cap;
        p.first_field = f->first_field;
        p.out = f->d_out.as<uint64_t>(); p.count = f->d_count.as<unsigned long long>(); p.out_cap = f->d_out.cap / 8;
        const uint64_t nvec = (n + 15) / 16;
        const uint32_t blocks = (uint32_t)std::min<uint64_t>((nvec + 255) / 256, 256 * 16);
        PFCHK(ts.timed([&]() -> int {
            hipLaunchKernelGGL(rowfilter_kernel, dim3(blocks), dim3(256), 0, ts.stream, p);
            HIPCHK(hipGetLastError()); return PF_OK;
        }));
        HIPCHK(hipMemcpyAsync(&cnt, f->d_count.p, 8, hipMemcpyDeviceToHost, ts.stream));
        HIPCHK(hipStreamSynchronize(ts.stream));
        ts.add_elapsed(&f->device_ms);
        if (cnt <= f->d_out.cap / 8) break;
        // more candidates than room (the kernel counted them all and kept what fitted): again, with room for all
        PFCHK(f->d_out.ensure(((size_t)cnt + (size_t)cnt / 8) * 8, true));
    }
    f->bytes_scanned += n;
    if (cnt > f->d_out.cap / 8) return fail(PF_ERR_STATE, "pf_rowfilter_scan: more candidates than room, twice");
    pos.resize((size_t)cnt);
    if (cnt) HIPCHK(hipMemcpy(pos.data(), f->d_out.p, (size_t)cnt * 8, hipMemcpyDeviceToHost));
    std::sort(pos.begin(), pos.end());
    return PF_OK;
}

// ---- the host's exact check (a 64-bit hash collision must not add a row): the key field of the line [b, t), t at its newline
std::string_view rf_key_field(const char* b, const char* t, int first_field) {
    const char* q = first_field ? b : t;
    if (first_field) while (q < t && *q != '\t') q++;
    else while (q > b && q[-1] != '\t') q--;
    return first_field ? std::string_view(b, (size_t)(q - b)) : std::string_view(q, (size_t)(t - q));
}

// and whether the line [b, e), with its newline, is a row: that field is one of the keys
bool rf_keep(pf_rowfilter* f, const char* b, const char* e) {
    const std::string_view key = rf_key_field(b, e > b && e[-1] == '\n' ? e - 1 : e, f->first_field);
    f->key.assign(key.data(), key.size());
    const bool keep = f->keys.count(f->key) != 0;
#ifdef PF_WEAK_HASH
    if (!keep) rf_wh_rowfilter_rejects++;
#endif
    return keep;
}

// ---- the work of pf_rowfilter_scan_members on the feed's d_text[0 .. n).  The candidates' lines: extents on the device
// (ext: their begins, then their ends), offsets in raw_lines by the host (off), one gather, one copy down into raw_lines
int rf_members_candidates(pf_rowfilter* f, uint64_t n, std::vector<uint64_t>& ext, std::vector<uint64_t>& off) {
    if (!n || f->keys.empty()) return PF_OK;
    hipStream_t st = f->feed.ts.stream;
    std::vector<uint64_t> pos;
    PFCHK(rf_scan_device(f, n, pos));
    const uint64_t cnt = pos.size();
    if (!cnt) return PF_OK;
    const unsigned char* const text = f->feed.text.d_text.as<const unsigned char>();
    PFCHK(f->d_ext.ensure((size_t)cnt * 24, true));
    uint64_t* const d_begin = f->d_ext.as<uint64_t>(), *const d_end = d_begin + cnt, *const d_off = d_end + cnt;
    HIPCHK(hipMemcpyAsync(f->d_out.p, pos.data(), (size_t)cnt * 8, hipMemcpyHostToDevice, st));
    hipLaunchKernelGGL(rf_extent_kernel, dim3((uint32_t)((cnt + 255) / 256)), dim3(256), 0, st, text, n,
                       f->d_out.as<const uint64_t>(), cnt, f->first_field, d_begin, d_end);
    HIPCHK(hipGetLastError());
    ext.resize((size_t)cnt * 2); off.resize((size_t)cnt);
    HIPCHK(hipMemcpyAsync(ext.data(), d_begin, (size_t)cnt * 16, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    uint64_t sum = 0;
    for (uint64_t k = 0; k < cnt; k++) { off[k] = sum; sum += ext[cnt + k] - ext[k]; }
    PFCHK(f->d_lines.ensure(sum + 16));
    HIPCHK(hipMemcpyAsync(d_off, off.data(), (size_t)cnt * 8, hipMemcpyHostToDevice, st));
    hipLaunchKernelGGL(rf_gather_kernel, dim3((uint32_t)cnt), dim3(64), 0, st, text, d_begin, d_end, d_off,
                       f->d_lines.as<unsigned char>());
    HIPCHK(hipGetLastError());
    f->raw_lines.resize((size_t)sum);
    if (sum) HIPCHK(hipMemcpyAsync(&f->raw_lines[0], f->d_lines.p, (size_t)sum, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    return PF_OK;
}

// the candidates behind the header line's `skip` bytes that are rows, appended to lines; how many
uint64_t rf_members_keep(pf_rowfilter* f, uint64_t skip, const std::vector<uint64_t>& ext, const std::vector<uint64_t>& off) {
    const uint64_t cnt = off.size(); uint64_t kept = 0;
    for (uint64_t k = 0; k < cnt; k++) {
        if (ext[k] < skip) continue;
        const char* b = f->raw_lines.data() + off[k];
        const char* e = b + (ext[cnt + k] - ext[k]);
        if (rf_keep(f, b, e)) { f->lines.append(b, (size_t)(e - b)); kept++; }
    }
    return kept;
}

}  // namespace

extern "C" {

void pf_rowfilter_destroy(pf_rowfilter* f) { feed_destroy(f); }

int pf_rowfilter_create(int device, int first_field, const char* const* keys, const uint32_t* key_len, uint64_t n_keys,
                        pf_rowfilter** out) {
    if (!out || (n_keys && (!keys || !key_len))) return fail(PF_ERR_ARG, "pf_rowfilter_create: null argument");
    *out = nullptr;
    FeedHandle<pf_rowfilter> f(nullptr, pf_rowfilter_destroy); PFCHK(feed_create(device, "pf_rowfilter_create", f));
    f->first_field = first_field ? 1 : 0;
    const uint64_t cap = f->cap = pf_table_room(n_keys, 4);
    std::vector<uint64_t> table(cap, RF_EMPTY);
    for (uint64_t i = 0; i < n_keys; i++) {
        if (key_len[i] >= RF_MAX_FIELD) continue;        // cannot match: the kernel gives up on fields this long
        if (!f->keys.emplace(keys[i], key_len[i]).second) continue;
        pf_table_insert(table, rf_hash(keys[i], key_len[i]), [](uint64_t) { return true; });     // a set: equal hashes share a slot
    }
    if (f->d_set.ensure(cap * 8, true) != PF_OK || f->d_count.ensure(8, true) != PF_OK)
        return fail(PF_ERR_HIP, "pf_rowfilter_create: device allocation failed");
    if (hipMemcpy(f->d_set.p, table.data(), cap * 8, hipMemcpyHostToDevice) != hipSuccess)
        return fail(PF_ERR_HIP, "pf_rowfilter_create: upload failed");
    *out = f.release();
    return PF_OK;
}

int pf_rowfilter_scan(pf_rowfilter* f, const char* text, uint64_t nbytes, const uint64_t** line_begin,
                      const uint64_t** line_end, uint64_t* n_lines, uint64_t* consumed) {
    if (!f || !line_begin || !line_end || !n_lines || !consumed || (nbytes && !text))
        return fail(PF_ERR_ARG, "pf_rowfilter_scan: null argument");
    HIPCHK(hipSetDevice(f->feed.device));
    f->begin.clear(); f->end.clear();
    *line_begin = nullptr; *line_end = nullptr; *n_lines = 0;
    // (without keys no line is a row: the block's lines are counted and stay where they are)
    if (f->keys.empty()) { *consumed = BlockText::complete_lines(text, nbytes); return PF_OK; }
    PFCHK(f->feed.plain(text, nbytes, consumed));
    const uint64_t n = *consumed;
    if (!n) return PF_OK;
    std::vector<uint64_t> pos;
    PFCHK(rf_scan_device(f, n, pos));
    for (uint64_t q : pos) {
        uint64_t b, e;
        rf_line_extent(reinterpret_cast<const unsigned char*>(text), n, q, f->first_field, &b, &e);
        if (rf_keep(f, text + b, text + e)) { f->begin.push_back(b); f->end.push_back(e); }
    }
    *line_begin = f->begin.data(); *line_end = f->end.data(); *n_lines = f->begin.size();
    return PF_OK;
}

int pf_rowfilter_members_begin(pf_rowfilter* f, int header) { return feed_members_begin(f, "pf_rowfilter_members_begin", header); }
int pf_rowfilter_set_large_members(pf_rowfilter* f, int on, uint32_t piece_bytes) { return feed_set_large(f, "pf_rowfilter_set_large_members", on, piece_bytes); }
int pf_rowfilter_large_stats(pf_rowfilter* f, uint64_t* pieces, float* ms) { return feed_large_stats(f, "pf_rowfilter_large_stats", pieces, ms); }

int pf_rowfilter_members_header(pf_rowfilter* f, const char** line, uint64_t* nbytes) {
    return feed_members_header(f, "pf_rowfilter_members_header", line, nbytes);
}

int pf_rowfilter_scan_members(pf_rowfilter* f, const char* members, uint64_t nbytes, int last, const char** lines,
                              uint64_t* lines_bytes, uint64_t* n_lines, uint64_t* consumed, int* taken) {
    if (!f || !lines || !lines_bytes || !n_lines || !consumed || !taken || (nbytes && !members))
        return fail(PF_ERR_ARG, "pf_rowfilter_scan_members: null argument");
    HIPCHK(hipSetDevice(f->feed.device));
    f->lines.clear();
    *lines = f->lines.data(); *lines_bytes = 0; *n_lines = 0;
    PFCHK(f->feed.members(members, nbytes, last, consumed, taken, [&](uint64_t n, uint64_t skip) -> int {
        std::vector<uint64_t> ext, off;
        PFCHK(rf_members_candidates(f, n, ext, off));
        *n_lines = rf_members_keep(f, skip, ext, off);
        return PF_OK;
    }));
    *lines = f->lines.data(); *lines_bytes = f->lines.size();      // (nothing, unless the block was taken and had rows)
    return PF_OK;
}

int pf_rowfilter_gunzip_stats(pf_rowfilter* f, uint64_t* members, uint64_t* text_bytes, float* inflate_ms, uint64_t* device_bytes) {
    return feed_gunzip_stats(f, "pf_rowfilter_gunzip_stats", members, text_bytes, inflate_ms, device_bytes);
}

int pf_rowfilter_stats(pf_rowfilter* f, uint64_t* bytes_scanned, float* device_ms) {
    if (!f) return fail(PF_ERR_ARG, "pf_rowfilter_stats: null argument");
    if (bytes_scanned) *bytes_scanned = f->bytes_scanned;
    if (device_ms) *device_ms = f->device_ms;
    return PF_OK;
}

}  // extern "C"

// ---------------------------------------------------------------------------------------------------------------------
// panfeed-plot's grids: /root/reference/panfeed/plot.py:195-222 (the table, the strain filter, the
// base scalar) and :261-305 (three pivot_tables per cluster) on the device.
//
// pf_plotgrid_scan takes blocks of complete lines of the annotated k-mer table.  One thread per line end finds the
// line behind it and its six fields; a row whose strain is a phenotype strain (device hash set, verified by bytes)
// gets its cluster name found or inserted in a device name table, its gene_start / strand parsed, its base letter
// taken from the k-mer, the --start/--stop zoom applied and its p-value TEXT found or inserted in a dictionary of
// distinct strings; then one 16-byte record goes to an HBM buffer.  Both tables are open addressing on 64-bit hashes:
// the slot is the id, the thread that claims a slot copies its bytes to an arena, and a second kernel checks every
// row's bytes against its slot's (a 64-bit collision stops the run instead of merging two names).  No arithmetic on
// floats happens on the device: the significance of every distinct p-value string is computed by the host and comes
// back as a 64-bit ordered integer key, and the grid kernel reduces with integer atomics only (atomicMax of the key,
// atomicAdd of a count | letter word), so grids are the same bits whatever the order of the rows.
// ---------------------------------------------------------------------------------------------------------------------
namespace {

constexpr uint32_t PG_MAX_FIELD = 4095;          // longer name / p-value fields drop the row (PG_ERR_LONG)
constexpr uint32_t PG_NONE = 0xFFFFFFFFu;
enum : uint32_t { PG_ERR_CLUSTER = 1, PG_ERR_PVALUE = 2, PG_ERR_LONG = 4, PG_ERR_RANGE = 8 };

struct PgTable {              // open addressing; hash 0 = free; str = arena offset << 16 | length
    unsigned long long* hash;
    unsigned long long* str;
    uint64_t cap;             // power of two
    unsigned char* arena;
    unsigned long long* arena_used;
    unsigned long long* count;
};

struct PgRecord {             // 16 B per kept row
    uint32_t cluster;         // cluster table slot
    uint32_t strain_letter;   // phenotype strain id << 8 | base letter (0: no letter)
    int32_t pos;              // gene_start
    uint32_t pvalue;          // p-value dictionary slot
};

struct PgCheck {              // one row that passed the strain filter: its fields, to be checked against the tables
    uint32_t cl_off, cl_len, cl_slot, pv_off, pv_len, pv_slot;
};

struct PgScanParams {
    const unsigned char* text;
    uint64_t n, begin;        // lines that start in [begin, n)
    int32_t col[6];           // cluster, strain, gene_start, k-mer, strand, p-value
    int32_t max_col;
    const unsigned long long* strain_hash;   // static set: hash, strain id
    const uint32_t* strain_id;
    uint64_t strain_cap;
    const unsigned char* strain_bytes;
    const uint64_t* strain_str;              // offset << 16 | length, by strain id
    PgTable clusters, pvalues;
    int zoom;
    int64_t start, stop;
    PgRecord* rec;
    unsigned long long* n_rec;
    PgCheck* chk;
    unsigned long long* n_chk;
    unsigned long long* n_lines;
    unsigned int* err;
};

__device__ __forceinline__ uint64_t pg_hash(const unsigned char* s, uint32_t n) {
    uint64_t h = 0xCBF29CE484222325ull;
    for (uint32_t i = 0; i < n; i++) h = rf_hash_step(h, s[i]);
    return rf_hash_fin(h);
}

// an integer field as pandas reads an int column ("12", "-3"; "12.0" as a float column holds it); false if it is not one
__device__ __forceinline__ bool pg_int(const unsigned char* s, uint32_t n, int64_t* v) {
    uint32_t i = 0;
    bool neg = false;
    if (i < n && (s[i] == '-' || s[i] == '+')) { neg = s[i] == '-'; i++; }
    const uint32_t d0 = i;
    int64_t x = 0;
    while (i < n && s[i] >= '0' && s[i] <= '9') {
        if (x > ((int64_t)1 << 40)) return false;
        x = x * 10 + (s[i] - '0');
        i++;
    }
    if (i == d0) return false;
    if (i < n && s[i] == '.') { i++; while (i < n && s[i] == '0') i++; }
    if (i != n) return false;
    *v = neg ? -x : x;
    return true;
}

__device__ __forceinline__ unsigned char pg_upper(unsigned char c) { return (c >= 'a' && c <= 'z') ? c - 32 : c; }

// find or insert; returns the slot.  The claimer copies the bytes; others are checked later (pg_check_kernel).
__device__ uint32_t pg_find_insert(const PgTable& t, const unsigned char* s, uint32_t n) {
    const unsigned long long h = pg_hash(s, n);
    uint64_t slot = h & (t.cap - 1);
    for (uint64_t probes = 0; probes < t.cap; probes++) {
        unsigned long long cur = t.hash[slot];
        if (cur == 0) cur = atomicCAS(&t.hash[slot], 0ull, h);
        if (cur == 0) {                                         // claimed: this thread's bytes name the slot
            const unsigned long long off = atomicAdd(t.arena_used, (unsigned long long)n);
            for (uint32_t i = 0; i < n; i++) t.arena[off + i] = s[i];
            t.str[slot] = (off << 16) | n;
            atomicAdd(t.count, 1ull);
            return (uint32_t)slot;
        }
        if (cur == h) return (uint32_t)slot;
        slot = (slot + 1) & (t.cap - 1);
    }
    return PG_NONE;                                             // cannot happen: the host keeps the load under 1/2
}

__device__ __forceinline__ int64_t pg_strain(const PgScanParams& p, const unsigned char* s, uint32_t n) {
    const uint64_t h = pg_hash(s, n);
    uint64_t slot = h & (p.strain_cap - 1);
    for (uint64_t probes = 0; probes < p.strain_cap; probes++) {
        const unsigned long long cur = p.strain_hash[slot];
        if (cur == 0) return -1;
        if (cur == h) {
            const uint32_t id = p.strain_id[slot];
            const uint64_t st = p.strain_str[id];
            if ((uint32_t)(st & 0xFFFF) == n) {
                const unsigned char* b = p.strain_bytes + (st >> 16);
                uint32_t i = 0;
                while (i < n && b[i] == s[i]) i++;
                if (i == n) return id;
            }
#ifdef PF_WEAK_HASH
            atomicAdd(&rf_wh_strain_rejects, 1ull);
#endif
        }
        slot = (slot + 1) & (p.strain_cap - 1);
    }
    return -1;
}

__device__ void pg_line(const PgScanParams& p, uint64_t s) {
    if (s >= p.n || p.text[s] == '\n') return;                  // a blank line: pandas skips it
    atomicAdd(p.n_lines, 1ull);
    uint64_t fs[6], fe[6];
    int found = 0;
    int f = 0;
    uint64_t b = s;
    for (uint64_t e = s; e < p.n; e++) {
        const unsigned char c = p.text[e];
        if (c != '\t' && c != '\n') continue;
#pragma unroll
        for (int q = 0; q < 6; q++)
            if (p.col[q] == f) { fs[q] = b; fe[q] = e; found |= 1 << q; }
        f++;
        b = e + 1;
        if (c == '\n' || f > p.max_col) break;
    }
    if (found != 0x3F) return;                                  // a short line: no strain to keep it by
    const unsigned char* t = p.text;
    const int64_t sid = pg_strain(p, t + fs[1], (uint32_t)(fe[1] - fs[1]));
    if (sid < 0) return;                                        // plot.py:200, the isin
    const uint32_t cl_len = (uint32_t)(fe[0] - fs[0]), pv_len = (uint32_t)(fe[5] - fs[5]);
    if (cl_len > PG_MAX_FIELD || pv_len > PG_MAX_FIELD) { atomicOr(p.err, PG_ERR_LONG); return; }
    const uint32_t cslot = pg_find_insert(p.clusters, t + fs[0], cl_len);
    int64_t pos;
    const bool pos_ok = pg_int(t + fs[2], (uint32_t)(fe[2] - fs[2]), &pos);
    if (pos_ok && (pos < -2147483647ll || pos > 2147483647ll)) atomicOr(p.err, PG_ERR_RANGE);
    const bool keep = pos_ok && pos >= -2147483647ll && pos <= 2147483647ll && (!p.zoom || (pos >= p.start && pos <= p.stop));
    uint32_t pslot = PG_NONE;
    if (keep) {
        int64_t strand = 0;
        const bool minus = pg_int(t + fs[4], (uint32_t)(fe[4] - fs[4]), &strand) && strand == -1;
        unsigned char letter = 0;                               // an empty k-mer is NaN: no letter, no scalar
        if (fe[3] > fs[3]) {
            if (minus) {                                        // plot.py:215-220: complement of the last letter
                const unsigned char c = pg_upper(t[fe[3] - 1]);
                letter = c == 'A' ? 'T' : c == 'T' ? 'A' : c == 'G' ? 'C' : c == 'C' ? 'G' : 'N';
            } else {
                letter = pg_upper(t[fs[3]]);
            }
        }
        pslot = pg_find_insert(p.pvalues, t + fs[5], pv_len);
        const unsigned long long r = atomicAdd(p.n_rec, 1ull);
        p.rec[r] = PgRecord{cslot, ((uint32_t)sid << 8) | letter, (int32_t)pos, pslot};
    }
    const unsigned long long k = atomicAdd(p.n_chk, 1ull);
    p.chk[k] = PgCheck{(uint32_t)fs[0], cl_len, cslot, (uint32_t)fs[5], pv_len, pslot};
}

__global__ __launch_bounds__(256) void pg_scan_kernel(PgScanParams p) {
    const uint64_t nvec = (p.n + 15) / 16;
    for (uint64_t v = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x; v < nvec; v += (uint64_t)gridDim.x * blockDim.x) {
        if (v == 0 && p.begin == 0) pg_line(p, 0);
        rf_each_newline(p.text, v, [&](uint64_t at) { if (at + 1 < p.n && at + 1 >= p.begin) pg_line(p, at + 1); });
    }
}

__device__ __forceinline__ bool pg_same(const PgTable& t, uint32_t slot, const unsigned char* s, uint32_t n) {
    if (slot == PG_NONE) return false;
    const unsigned long long st = t.str[slot];
    if ((uint32_t)(st & 0xFFFF) != n) return false;
    const unsigned char* b = t.arena + (st >> 16);
    for (uint32_t i = 0; i < n; i++)
        if (b[i] != s[i]) return false;
    return true;
}

__global__ __launch_bounds__(256) void pg_check_kernel(const unsigned char* text, const PgCheck* chk, uint64_t n_chk,
                                                        PgTable clusters, PgTable pvalues, unsigned int* err) {
    for (uint64_t i = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x; i < n_chk; i += (uint64_t)gridDim.x * blockDim.x) {
        const PgCheck c = chk[i];
        if (!pg_same(clusters, c.cl_slot, text + c.cl_off, c.cl_len)) atomicOr(err, PG_ERR_CLUSTER);
        if (c.pv_slot != PG_NONE && !pg_same(pvalues, c.pv_slot, text + c.pv_off, c.pv_len)) atomicOr(err, PG_ERR_PVALUE);
    }
}

// a table grown to a new capacity: every entry re-inserted (all hashes are distinct), remap[old slot] = new slot
__global__ __launch_bounds__(256) void pg_rehash_kernel(PgTable from, PgTable to, uint32_t* remap) {
    for (uint64_t i = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x; i < from.cap; i += (uint64_t)gridDim.x * blockDim.x) {
        const unsigned long long h = from.hash[i];
        if (!h) continue;
        uint64_t slot = h & (to.cap - 1);
        while (atomicCAS(&to.hash[slot], 0ull, h) != 0ull) slot = (slot + 1) & (to.cap - 1);
        to.str[slot] = from.str[i];
        remap[i] = (uint32_t)slot;
    }
}

__global__ __launch_bounds__(256) void pg_remap_kernel(PgRecord* rec, uint64_t n, const uint32_t* remap, int field) {
    for (uint64_t i = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x; i < n; i += (uint64_t)gridDim.x * blockDim.x) {
        uint32_t& id = field == 0 ? rec[i].cluster : rec[i].pvalue;
        if (id != PG_NONE) id = remap[id];
    }
}

// per cluster slot: smallest and largest gene_start, row count (plot.py:266 / :297, the reindexed column range)
__global__ __launch_bounds__(256) void pg_stats_kernel(const PgRecord* rec, uint64_t n, int* mn, int* mx,
                                                        unsigned long long* cnt) {
    for (uint64_t i = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x; i < n; i += (uint64_t)gridDim.x * blockDim.x) {
        const PgRecord r = rec[i];
        if (r.cluster == PG_NONE) continue;
        atomicMin(&mn[r.cluster], r.pos);
        atomicMax(&mx[r.cluster], r.pos);
        atomicAdd(&cnt[r.cluster], 1ull);
    }
}

struct PgGridParams {
    const PgRecord* rec;
    uint64_t n;
    const int32_t* slot_item;                  // cluster slot -> item of this batch, -1 if not in it
    const uint64_t* item_off;                  // first cell of the item's grid (strain-major, n_strains x width)
    const int32_t* item_min;
    const uint32_t* item_width;
    uint32_t n_strains;
    const unsigned long long* sig_key;         // p-value slot -> ordered key of its significance; 0 = NaN
    unsigned long long* key;                   // per cell: max key (0: no non-NaN significance)
    unsigned long long* cnt;                   // per cell: rows << 32 | sum of their letters
    unsigned int* err;
};

__global__ __launch_bounds__(256) void pg_grid_kernel(PgGridParams p) {
    for (uint64_t i = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x; i < p.n; i += (uint64_t)gridDim.x * blockDim.x) {
        const PgRecord r = p.rec[i];
        if (r.cluster == PG_NONE || r.pvalue == PG_NONE) { atomicOr(p.err, PG_ERR_RANGE); continue; }
        const int32_t item = p.slot_item[r.cluster];
        if (item < 0) continue;
        const uint32_t strain = r.strain_letter >> 8;
        const int64_t col = (int64_t)r.pos - p.item_min[item];
        if (strain >= p.n_strains || col < 0 || col >= (int64_t)p.item_width[item]) { atomicOr(p.err, PG_ERR_RANGE); continue; }
        const uint64_t cell = p.item_off[item] + (uint64_t)strain * p.item_width[item] + (uint64_t)col;
        const unsigned long long k = p.sig_key[r.pvalue];
        if (k) atomicMax(&p.key[cell], k);                     // pandas' NaN-skipping max (plot.py:261-264)
        atomicAdd(&p.cnt[cell], (1ull << 32) | (r.strain_letter & 0xFF));   // handle_paralogs: the count decides
    }
}

inline uint32_t pg_blocks(uint64_t n) { return (uint32_t)std::max<uint64_t>(1, std::min<uint64_t>((n + 255) / 256, 256 * 16)); }

}  // namespace

struct pf_plotgrid {
    float device_ms = 0;
    int32_t col[6] = {};
    int32_t max_col = 0;
    int zoom = 0;
    int64_t start = 0, stop = 0;
    uint32_t n_strains = 0;
    // the phenotype strains (static): hash set (unsigned long long, uint32 ids), the names, offset << 16 | length per id
    DevBuf d_strain_hash, d_strain_id, d_strain_bytes, d_strain_str;
    uint64_t strain_cap = 0;
    // the two growing tables (PgTable)
    struct Tab {
        DevBuf hash, str;                        // cap slots each (unsigned long long)
        uint64_t cap = 0;
        DevBuf arena;
        DevBuf ctr;                              // [0] arena bytes used, [1] entries
        uint64_t used = 0, count = 0;            // host copies after the last scan
    } cl, pv;
    DevBuf d_rec;                               // PgRecord
    uint64_t n_rec = 0;
    DevBuf d_chk;                               // PgCheck
    DevBuf d_ctr;                               // [0] records [1] checks [2] lines ; err as [3]
    uint64_t bytes_scanned = 0, lines = 0;
    // after pf_plotgrid_finish
    int finished = 0;
    std::vector<uint32_t> cl_slot, pv_slot;     // dense id -> slot
    std::vector<int32_t> cl_min, cl_max;
    std::vector<uint64_t> cl_rows;
    std::string cl_names, pv_texts;
    std::vector<uint64_t> cl_off, pv_off;
    DevBuf d_sig;                              // significance key by p-value slot
    int sig_set = 0;
    DevBuf d_key, d_cnt;                       // the grids' cells
    DevBuf d_slot_item;
    DevBuf d_item;                             // off[n] | min[n] | width[n], packed in one buffer
    TextFeed feed;                             // the block: host text (pf_plotgrid_scan) or gzip members (pf_plotgrid_scan_members)
};

namespace {

using ull = unsigned long long;

PgTable pg_view(pf_plotgrid::Tab& t) {
    return PgTable{t.hash.as<ull>(), t.str.as<ull>(), t.cap, t.arena.as<unsigned char>(), t.ctr.as<ull>(), t.ctr.as<ull>() + 1};
}

// room for `more` new entries (and `bytes` new arena bytes) at a load of at most 1/2; records' slots follow a move
int pg_tab_reserve(pf_plotgrid* g, pf_plotgrid::Tab& t, uint64_t more, uint64_t bytes, int field) {
    if (t.used + bytes > t.arena.cap) {
        uint64_t want = std::max<uint64_t>((t.used + bytes) * 2, 1 << 20);
        if (want >= ((uint64_t)1 << 47)) return fail(PF_ERR_CAPACITY, "pf_plotgrid: name arena over 2^47 bytes");
        DevBuf a;
        PFCHK(a.ensure(want, true));
        if (t.used) HIPCHK(hipMemcpyAsync(a.p, t.arena.p, t.used, hipMemcpyDeviceToDevice, g->feed.ts.stream));
        HIPCHK(hipStreamSynchronize(g->feed.ts.stream));
        std::swap(t.arena, a);                  // (the old arena goes at the end of this block)
    }
    uint64_t cap = std::max<uint64_t>(t.cap, 1024);
    while (cap < 2 * (t.count + more)) cap <<= 1;
    if (cap >= ((uint64_t)1 << 32)) return fail(PF_ERR_CAPACITY, "pf_plotgrid: over 2^31 distinct names in a table");
    if (cap == t.cap) return PF_OK;
    DevBuf hash, str;
    PFCHK(hash.ensure(cap * 8, true));
    PFCHK(str.ensure(cap * 8, true));
    HIPCHK(hipMemsetAsync(hash.p, 0, cap * 8, g->feed.ts.stream));
    if (t.hash.p) {
        DevBuf remap;
        PFCHK(remap.ensure(t.cap * 4, true));
        PgTable n = pg_view(t);
        n.hash = hash.as<ull>(); n.str = str.as<ull>(); n.cap = cap;
        hipLaunchKernelGGL(pg_rehash_kernel, dim3(pg_blocks(t.cap)), dim3(256), 0, g->feed.ts.stream, pg_view(t), n, remap.as<uint32_t>());
        HIPCHK(hipGetLastError());
        if (g->n_rec) {
            hipLaunchKernelGGL(pg_remap_kernel, dim3(pg_blocks(g->n_rec)), dim3(256), 0, g->feed.ts.stream, g->d_rec.as<PgRecord>(), g->n_rec,
                               (const uint32_t*)remap.p, field);
            HIPCHK(hipGetLastError());
        }
        HIPCHK(hipStreamSynchronize(g->feed.ts.stream));
    }
    std::swap(t.hash, hash); std::swap(t.str, str);   // (the old ones go on return)
    t.cap = cap;
    return PF_OK;
}

// the table's entries in slot order: dense id -> slot, their bytes joined, offsets (n + 1)
int pg_tab_list(pf_plotgrid* g, pf_plotgrid::Tab& t, std::vector<uint32_t>& slots, std::string& bytes, std::vector<uint64_t>& off) {
    std::vector<unsigned long long> h(t.cap), st(t.cap);
    std::string arena(t.used, '\0');
    if (t.cap) {
        HIPCHK(hipMemcpy(h.data(), t.hash.p, t.cap * 8, hipMemcpyDeviceToHost));
        HIPCHK(hipMemcpy(st.data(), t.str.p, t.cap * 8, hipMemcpyDeviceToHost));
    }
    if (t.used) HIPCHK(hipMemcpy(&arena[0], t.arena.p, t.used, hipMemcpyDeviceToHost));
    slots.clear(); bytes.clear(); off.assign(1, 0);
    for (uint64_t i = 0; i < t.cap; i++) {
        if (!h[i]) continue;
        slots.push_back((uint32_t)i);
        bytes.append(arena, (size_t)(st[i] >> 16), (size_t)(st[i] & 0xFFFF));
        off.push_back(bytes.size());
    }
    return PF_OK;
}

// a block's text is addressed in 32 bits (PgCheck) -- the inflated text, for a block of members
int pg_block_fits(uint64_t n) {
    return n >= ((uint64_t)1 << 32) ? fail(PF_ERR_ARG, "pf_plotgrid_scan: a block of 4 GiB or more") : PF_OK;
}

// The scan of the feed's d_text[skip .. n), complete lines, for the plain route and the member route alike: room for what
// a block of that many bytes may add, pg_scan_kernel, pg_check_kernel, the counters read back.  On the feed's stream, behind
// whatever put the text there.
int pg_scan_device(pf_plotgrid* g, uint64_t n, uint64_t skip) {
    if (n <= skip) return PF_OK;
    PFCHK(pg_block_fits(n));
    const uint64_t bytes = n - skip;
    // every row needs max_col tabs and a newline: at most this many rows pass
    const uint64_t rows = bytes / ((uint64_t)g->max_col + 1) + 1;
    PFCHK(g->d_chk.ensure(rows * sizeof(PgCheck), true));
    if (g->n_rec + rows > g->d_rec.cap / sizeof(PgRecord)) {
        const uint64_t want = std::max<uint64_t>((g->n_rec + rows) * 3 / 2, 1 << 16);
        DevBuf r;
        PFCHK(r.ensure(want * sizeof(PgRecord), true));
        if (g->n_rec) HIPCHK(hipMemcpyAsync(r.p, g->d_rec.p, g->n_rec * sizeof(PgRecord), hipMemcpyDeviceToDevice, g->feed.ts.stream));
        HIPCHK(hipStreamSynchronize(g->feed.ts.stream));
        std::swap(g->d_rec, r);                 // (the old records go at the end of this block)
    }
    PFCHK(pg_tab_reserve(g, g->cl, rows, bytes, 0));
    PFCHK(pg_tab_reserve(g, g->pv, rows, bytes, 1));
    unsigned long long* const d_ctr = g->d_ctr.as<ull>();
    unsigned long long ctr[4] = {g->n_rec, 0, 0, 0};
    HIPCHK(hipMemcpyAsync(d_ctr, ctr, 3 * 8, hipMemcpyHostToDevice, g->feed.ts.stream));   // records continue; checks, lines restart
    PgScanParams p{};
    p.text = g->feed.text.d_text.as<unsigned char>(); p.n = n; p.begin = skip;
    for (int q = 0; q < 6; q++) p.col[q] = g->col[q];
    p.max_col = g->max_col;
    p.strain_hash = g->d_strain_hash.as<ull>(); p.strain_id = g->d_strain_id.as<uint32_t>(); p.strain_cap = g->strain_cap;
    p.strain_bytes = g->d_strain_bytes.as<unsigned char>(); p.strain_str = g->d_strain_str.as<uint64_t>();
    p.clusters = pg_view(g->cl); p.pvalues = pg_view(g->pv);
    p.zoom = g->zoom; p.start = g->start; p.stop = g->stop;
    p.rec = g->d_rec.as<PgRecord>(); p.n_rec = d_ctr; p.chk = g->d_chk.as<PgCheck>(); p.n_chk = d_ctr + 1; p.n_lines = d_ctr + 2;
    p.err = (unsigned int*)(d_ctr + 3);
    PFCHK(g->feed.ts.timed([&]() -> int {
        hipLaunchKernelGGL(pg_scan_kernel, dim3(pg_blocks((n + 15) / 16)), dim3(256), 0, g->feed.ts.stream, p);
        HIPCHK(hipGetLastError());
        unsigned long long n_chk = 0;
        HIPCHK(hipMemcpyAsync(&n_chk, d_ctr + 1, 8, hipMemcpyDeviceToHost, g->feed.ts.stream));
        HIPCHK(hipStreamSynchronize(g->feed.ts.stream));
        if (n_chk) {
            hipLaunchKernelGGL(pg_check_kernel, dim3(pg_blocks(n_chk)), dim3(256), 0, g->feed.ts.stream, p.text, g->d_chk.as<const PgCheck>(),
                               (uint64_t)n_chk, pg_view(g->cl), pg_view(g->pv), (unsigned int*)(d_ctr + 3));
            HIPCHK(hipGetLastError());
        }
        return PF_OK;
    }));
    HIPCHK(hipMemcpyAsync(ctr, d_ctr, 4 * 8, hipMemcpyDeviceToHost, g->feed.ts.stream));
    unsigned long long tc[2][2];
    HIPCHK(hipMemcpyAsync(tc[0], g->cl.ctr.p, 16, hipMemcpyDeviceToHost, g->feed.ts.stream));
    HIPCHK(hipMemcpyAsync(tc[1], g->pv.ctr.p, 16, hipMemcpyDeviceToHost, g->feed.ts.stream));
    HIPCHK(hipStreamSynchronize(g->feed.ts.stream));
    g->feed.ts.add_elapsed(&g->device_ms);
    g->cl.used = tc[0][0]; g->cl.count = tc[0][1];
    g->pv.used = tc[1][0]; g->pv.count = tc[1][1];
    g->n_rec = ctr[0];
    g->lines += ctr[2];
    g->bytes_scanned += bytes;
    const unsigned err = (unsigned)(ctr[3] & 0xFFFFFFFFu);
    if (err & (PG_ERR_CLUSTER | PG_ERR_PVALUE))
        return fail(PF_ERR_CAPACITY, "pf_plotgrid_scan: two different cluster names or p-value texts share a 64-bit hash");
    if (err & PG_ERR_LONG) return fail(PF_ERR_ARG, "pf_plotgrid_scan: a cluster name or p-value field over 4095 bytes");
    if (err & PG_ERR_RANGE) return fail(PF_ERR_ARG, "pf_plotgrid_scan: a gene_start outside the 32-bit range");
    return PF_OK;
}

}  // namespace

extern "C" {

void pf_plotgrid_destroy(pf_plotgrid* g) { feed_destroy(g); }

int pf_plotgrid_create(int device, const char* const* strains, const uint32_t* strain_len, uint32_t n_strains,
                       const int32_t* columns, int zoom, int64_t start, int64_t stop, pf_plotgrid** out) {
    if (!out || !columns || (n_strains && (!strains || !strain_len))) return fail(PF_ERR_ARG, "pf_plotgrid_create: null argument");
    *out = nullptr;
    if (n_strains >= (1u << 24)) return fail(PF_ERR_ARG, "pf_plotgrid_create: at most 2^24 - 1 phenotype strains");
    FeedHandle<pf_plotgrid> g(nullptr, pf_plotgrid_destroy); PFCHK(feed_create(device, "pf_plotgrid_create", g));
    g->zoom = zoom ? 1 : 0;
    g->start = start; g->stop = stop;
    g->n_strains = n_strains;
    for (int q = 0; q < 6; q++) {
        if (columns[q] < 0) return fail(PF_ERR_ARG, "pf_plotgrid_create: negative column index");
        g->col[q] = columns[q];
        g->max_col = std::max(g->max_col, columns[q]);
    }
    // the strain set: distinct names (a repeated phenotype name keeps its first id)
    const uint64_t cap = pf_table_room(n_strains, 2);
    std::vector<unsigned long long> hs(cap, 0);
    std::vector<uint32_t> ids(cap, 0);
    std::string bytes;
    std::vector<uint64_t> str(std::max<uint32_t>(n_strains, 1), 0);
    for (uint32_t i = 0; i < n_strains; i++) {
        if (strain_len[i] > 0xFFFF) return fail(PF_ERR_ARG, "pf_plotgrid_create: strain name over 65535 bytes");
        str[i] = ((uint64_t)bytes.size() << 16) | strain_len[i];
        bytes.append(strains[i], strain_len[i]);
        const int64_t slot = pf_table_insert(hs, rf_hash(strains[i], strain_len[i]), [&](uint64_t at) {
            const uint64_t o = str[ids[at]];
            return (o & 0xFFFF) == strain_len[i] && !memcmp(bytes.data() + (o >> 16), strains[i], strain_len[i]);
        });
        if (slot >= 0) ids[slot] = i;
    }
    g->strain_cap = cap;
    PFCHK(g->d_strain_hash.ensure(cap * 8, true));
    PFCHK(g->d_strain_id.ensure(cap * 4, true));
    PFCHK(g->d_strain_bytes.ensure(std::max<size_t>(bytes.size(), 1), true));
    PFCHK(g->d_strain_str.ensure(str.size() * 8, true));
    HIPCHK(hipMemcpy(g->d_strain_hash.p, hs.data(), cap * 8, hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(g->d_strain_id.p, ids.data(), cap * 4, hipMemcpyHostToDevice));
    if (!bytes.empty()) HIPCHK(hipMemcpy(g->d_strain_bytes.p, bytes.data(), bytes.size(), hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(g->d_strain_str.p, str.data(), str.size() * 8, hipMemcpyHostToDevice));
    PFCHK(g->d_ctr.ensure(4 * 8, true));
    HIPCHK(hipMemset(g->d_ctr.p, 0, 4 * 8));
    for (auto* t : {&g->cl, &g->pv}) {
        PFCHK(t->ctr.ensure(2 * 8, true));
        HIPCHK(hipMemset(t->ctr.p, 0, 2 * 8));
    }
    *out = g.release();
    return PF_OK;
}

int pf_plotgrid_scan(pf_plotgrid* g, const char* text, uint64_t nbytes, uint64_t* consumed) {
    if (!g || !consumed || (nbytes && !text)) return fail(PF_ERR_ARG, "pf_plotgrid_scan: null argument");
    if (g->finished) return fail(PF_ERR_STATE, "pf_plotgrid_scan: after pf_plotgrid_finish");
    HIPCHK(hipSetDevice(g->feed.device));
    // (a block this scan cannot take is turned away in front of its upload)
    PFCHK(g->feed.plain(text, nbytes, consumed, [](uint64_t n) { return pg_block_fits(n); }));
    return pg_scan_device(g, *consumed, 0);
}

int pf_plotgrid_members_begin(pf_plotgrid* g, int header) { return feed_members_begin(g, "pf_plotgrid_members_begin", header); }
int pf_plotgrid_set_large_members(pf_plotgrid* g, int on, uint32_t piece_bytes) { return feed_set_large(g, "pf_plotgrid_set_large_members", on, piece_bytes); }
int pf_plotgrid_large_stats(pf_plotgrid* g, uint64_t* pieces, float* ms) { return feed_large_stats(g, "pf_plotgrid_large_stats", pieces, ms); }

int pf_plotgrid_members_header(pf_plotgrid* g, const char** line, uint64_t* nbytes) {
    return feed_members_header(g, "pf_plotgrid_members_header", line, nbytes);
}

int pf_plotgrid_scan_members(pf_plotgrid* g, const char* members, uint64_t nbytes, int last, uint64_t* consumed, int* taken) {
    if (!g || !consumed || !taken || (nbytes && !members)) return fail(PF_ERR_ARG, "pf_plotgrid_scan_members: null argument");
    if (g->finished) return fail(PF_ERR_STATE, "pf_plotgrid_scan_members: after pf_plotgrid_finish");
    HIPCHK(hipSetDevice(g->feed.device));
    // (the feed calls the scan only once the block is taken: a block that is not leaves records and tables as they were)
    return g->feed.members(members, nbytes, last, consumed, taken, [g](uint64_t n, uint64_t skip) { return pg_scan_device(g, n, skip); });
}

int pf_plotgrid_gunzip_stats(pf_plotgrid* g, uint64_t* members, uint64_t* text_bytes, float* inflate_ms, uint64_t* device_bytes) {
    return feed_gunzip_stats(g, "pf_plotgrid_gunzip_stats", members, text_bytes, inflate_ms, device_bytes);
}

int pf_plotgrid_finish(pf_plotgrid* g, uint32_t* n_clusters, uint64_t* n_pvalues, uint64_t* n_records) {
    if (!g || !n_clusters || !n_pvalues || !n_records) return fail(PF_ERR_ARG, "pf_plotgrid_finish: null argument");
    HIPCHK(hipSetDevice(g->feed.device));
    if (!g->finished) {
        if (int rc = pg_tab_list(g, g->cl, g->cl_slot, g->cl_names, g->cl_off)) return rc;
        if (int rc = pg_tab_list(g, g->pv, g->pv_slot, g->pv_texts, g->pv_off)) return rc;
        const uint64_t cap = std::max<uint64_t>(g->cl.cap, 1);
        DevBuf mn, mx, cnt;
        PFCHK(mn.ensure(cap * 4, true));
        PFCHK(mx.ensure(cap * 4, true));
        PFCHK(cnt.ensure(cap * 8, true));
        std::vector<int> init(cap, 0x7FFFFFFF);
        HIPCHK(hipMemcpy(mn.p, init.data(), cap * 4, hipMemcpyHostToDevice));
        init.assign(cap, (int)0x80000000);
        HIPCHK(hipMemcpy(mx.p, init.data(), cap * 4, hipMemcpyHostToDevice));
        HIPCHK(hipMemset(cnt.p, 0, cap * 8));
        if (g->n_rec) {
            hipLaunchKernelGGL(pg_stats_kernel, dim3(pg_blocks(g->n_rec)), dim3(256), 0, g->feed.ts.stream, g->d_rec.as<const PgRecord>(),
                               g->n_rec, mn.as<int>(), mx.as<int>(), cnt.as<ull>());
            HIPCHK(hipGetLastError());
            HIPCHK(hipStreamSynchronize(g->feed.ts.stream));
        }
        std::vector<int> hmn(cap), hmx(cap);
        std::vector<unsigned long long> hc(cap);
        HIPCHK(hipMemcpy(hmn.data(), mn.p, cap * 4, hipMemcpyDeviceToHost));
        HIPCHK(hipMemcpy(hmx.data(), mx.p, cap * 4, hipMemcpyDeviceToHost));
        HIPCHK(hipMemcpy(hc.data(), cnt.p, cap * 8, hipMemcpyDeviceToHost));
        g->cl_min.clear(); g->cl_max.clear(); g->cl_rows.clear();
        for (uint32_t s : g->cl_slot) {
            g->cl_min.push_back(hmn[s]);
            g->cl_max.push_back(hmx[s]);
            g->cl_rows.push_back(hc[s]);
        }
        g->finished = 1;
    }
    *n_clusters = (uint32_t)g->cl_slot.size();
    *n_pvalues = g->pv_slot.size();
    *n_records = g->n_rec;
    return PF_OK;
}

int pf_plotgrid_clusters(pf_plotgrid* g, const char** names, const uint64_t** name_off, const int32_t** min_pos,
                         const int32_t** max_pos, const uint64_t** rows) {
    if (!g || !names || !name_off || !min_pos || !max_pos || !rows) return fail(PF_ERR_ARG, "pf_plotgrid_clusters: null argument");
    if (!g->finished) return fail(PF_ERR_STATE, "pf_plotgrid_clusters: before pf_plotgrid_finish");
    *names = g->cl_names.data(); *name_off = g->cl_off.data();
    *min_pos = g->cl_min.data(); *max_pos = g->cl_max.data(); *rows = g->cl_rows.data();
    return PF_OK;
}

int pf_plotgrid_pvalues(pf_plotgrid* g, const char** texts, const uint64_t** text_off) {
    if (!g || !texts || !text_off) return fail(PF_ERR_ARG, "pf_plotgrid_pvalues: null argument");
    if (!g->finished) return fail(PF_ERR_STATE, "pf_plotgrid_pvalues: before pf_plotgrid_finish");
    *texts = g->pv_texts.data(); *text_off = g->pv_off.data();
    return PF_OK;
}

int pf_plotgrid_set_significance(pf_plotgrid* g, const uint64_t* keys) {
    if (!g || (!keys && !g->pv_slot.empty())) return fail(PF_ERR_ARG, "pf_plotgrid_set_significance: null argument");
    if (!g->finished) return fail(PF_ERR_STATE, "pf_plotgrid_set_significance: before pf_plotgrid_finish");
    HIPCHK(hipSetDevice(g->feed.device));
    const uint64_t cap = std::max<uint64_t>(g->pv.cap, 1);
    std::vector<unsigned long long> by_slot(cap, 0);
    for (size_t i = 0; i < g->pv_slot.size(); i++) by_slot[g->pv_slot[i]] = keys[i];
    PFCHK(g->d_sig.ensure(cap * 8, true));
    HIPCHK(hipMemcpy(g->d_sig.p, by_slot.data(), cap * 8, hipMemcpyHostToDevice));
    g->sig_set = 1;
    return PF_OK;
}

int pf_plotgrid_grids(pf_plotgrid* g, const uint32_t* ids, uint32_t n, uint64_t* key_out, uint64_t* cnt_out) {
    if (!g || (n && (!ids || !key_out || !cnt_out))) return fail(PF_ERR_ARG, "pf_plotgrid_grids: null argument");
    if (!g->finished || !g->sig_set) return fail(PF_ERR_STATE, "pf_plotgrid_grids: before pf_plotgrid_set_significance");
    if (!n) return PF_OK;
    HIPCHK(hipSetDevice(g->feed.device));
    const uint64_t cap = std::max<uint64_t>(g->cl.cap, 1);
    std::vector<int32_t> slot_item(cap, -1);
    std::vector<uint64_t> item(3 * (size_t)n);
    uint64_t cells = 0;
    for (uint32_t i = 0; i < n; i++) {
        if (ids[i] >= g->cl_slot.size()) return fail(PF_ERR_ARG, "pf_plotgrid_grids: no such cluster");
        if (!g->cl_rows[ids[i]]) return fail(PF_ERR_ARG, "pf_plotgrid_grids: a cluster without rows has no grid");
        const uint32_t s = g->cl_slot[ids[i]];
        if (slot_item[s] >= 0) return fail(PF_ERR_ARG, "pf_plotgrid_grids: a cluster twice in one call");
        slot_item[s] = (int32_t)i;
        const uint64_t width = (uint64_t)((int64_t)g->cl_max[ids[i]] - g->cl_min[ids[i]] + 1);
        item[i] = cells;
        item[n + i] = (uint64_t)(int64_t)g->cl_min[ids[i]];
        item[2 * (size_t)n + i] = width;
        cells += width * g->n_strains;
    }
    PFCHK(g->d_key.ensure(cells * 8, true));
    PFCHK(g->d_cnt.ensure(cells * 8, true));
    PFCHK(g->d_item.ensure(3 * (size_t)n * 8, true));
    PFCHK(g->d_slot_item.ensure(cap * 4, true));
    // the device-side item table: off (u64), min (i32), width (u32)
    std::vector<int32_t> imin(n);
    std::vector<uint32_t> iwidth(n);
    for (uint32_t i = 0; i < n; i++) { imin[i] = (int32_t)(int64_t)item[n + i]; iwidth[i] = (uint32_t)item[2 * (size_t)n + i]; }
    char* dit = g->d_item.as<char>();
    HIPCHK(hipMemcpyAsync(dit, item.data(), (size_t)n * 8, hipMemcpyHostToDevice, g->feed.ts.stream));
    HIPCHK(hipMemcpyAsync(dit + (size_t)n * 8, imin.data(), (size_t)n * 4, hipMemcpyHostToDevice, g->feed.ts.stream));
    HIPCHK(hipMemcpyAsync(dit + (size_t)n * 12, iwidth.data(), (size_t)n * 4, hipMemcpyHostToDevice, g->feed.ts.stream));
    unsigned long long* const d_err = g->d_ctr.as<ull>() + 3;
    HIPCHK(hipMemcpyAsync(g->d_slot_item.p, slot_item.data(), cap * 4, hipMemcpyHostToDevice, g->feed.ts.stream));
    HIPCHK(hipMemsetAsync(g->d_key.p, 0, cells * 8, g->feed.ts.stream));
    HIPCHK(hipMemsetAsync(g->d_cnt.p, 0, cells * 8, g->feed.ts.stream));
    HIPCHK(hipMemsetAsync(d_err, 0, 8, g->feed.ts.stream));
    PgGridParams p{};
    p.rec = g->d_rec.as<PgRecord>(); p.n = g->n_rec; p.slot_item = g->d_slot_item.as<int32_t>();
    p.item_off = (const uint64_t*)dit; p.item_min = (const int32_t*)(dit + (size_t)n * 8);
    p.item_width = (const uint32_t*)(dit + (size_t)n * 12);
    p.n_strains = g->n_strains; p.sig_key = g->d_sig.as<ull>(); p.key = g->d_key.as<ull>(); p.cnt = g->d_cnt.as<ull>();
    p.err = (unsigned int*)d_err;
    PFCHK(g->feed.ts.timed([&]() -> int {
        hipLaunchKernelGGL(pg_grid_kernel, dim3(pg_blocks(g->n_rec)), dim3(256), 0, g->feed.ts.stream, p);
        HIPCHK(hipGetLastError()); return PF_OK;
    }));
    unsigned long long err = 0;
    HIPCHK(hipMemcpyAsync(key_out, g->d_key.p, cells * 8, hipMemcpyDeviceToHost, g->feed.ts.stream));
    HIPCHK(hipMemcpyAsync(cnt_out, g->d_cnt.p, cells * 8, hipMemcpyDeviceToHost, g->feed.ts.stream));
    HIPCHK(hipMemcpyAsync(&err, d_err, 8, hipMemcpyDeviceToHost, g->feed.ts.stream));
    HIPCHK(hipStreamSynchronize(g->feed.ts.stream));
    g->feed.ts.add_elapsed(&g->device_ms);
    if (err) return fail(PF_ERR_STATE, "pf_plotgrid_grids: a record outside its cluster's grid");
    return PF_OK;
}

int pf_plotgrid_stats(pf_plotgrid* g, uint64_t* bytes_scanned, uint64_t* lines, uint64_t* records, float* device_ms) {
    if (!g) return fail(PF_ERR_ARG, "pf_plotgrid_stats: null argument");
    if (bytes_scanned) *bytes_scanned = g->bytes_scanned;
    if (lines) *lines = g->lines;
    if (records) *records = g->n_rec;
    if (device_ms) *device_ms = g->device_ms;
    return PF_OK;
}

}  // extern "C"

// ---------------------------------------------------------------------------------------------------------------------
// The row pack: "select some lines of a block and write them, packed and in file order, into one device buffer", for the
// k-mer join and the associations filter (both below).  Every thread owns 256 bytes of the text (16 vectors of 16) and the
// lines whose preceding newline lies in them; a workgroup's 64 KiB are a tile.  A client brings two kernels of its own:
//   plan     counts each thread's selected rows and their output bytes and ends in row_plan: the counts to thr, the
//            workgroup's sums to tile.  row_tiles_kernel then makes the tiles' sums exclusive prefixes
//   place    finds the same rows again through row_place, which gives every one a record (RowRec: source, destination, its
//            pieces) at its place in file order -- or raises the client's complaint bit: the two passes disagree
// and row_write_kernel copies by the records: a wave per group of 16 consecutive rows, lanes striding over a row's bytes.
// RowPack owns the buffers and runs the sequence; RowHandout brings the text to the host.
// ---------------------------------------------------------------------------------------------------------------------
namespace {

constexpr uint32_t ROW_TILE_VECS = 4096;         // vectors of a workgroup: 256 threads x 16
constexpr uint32_t ROW_GROUP = 16;               // rows of a wave's step in the writer
constexpr uint64_t ROW_PIECE = 32ull << 20;      // bytes of output handed out at a time

// a row of the output: text[src ..) as it stands, len0 bytes (raw), or  field 0 \t field 10 \t arena text \t fields 1..9 \n
struct RowRec { uint64_t src, dst; uint32_t len0, f1, mid, f10, len10, t_off, t_len, raw; };

__device__ __forceinline__ uint32_t row_out_len(const RowRec& r) { return r.raw ? r.len0 : r.len0 + r.len10 + r.t_len + r.mid + 4; }

// what the pack's own code reads of a client's parameters: the client's parameter struct begins with it
struct RowSpan {
    const unsigned char* text;   // the block, complete lines, zero-padded to the next multiple of 16 bytes
    uint64_t n, begin;           // lines that start in [begin, n)
    uint2* thr;                  // per thread, rows and output bytes
    unsigned long long* tile;    // per tile, rows and bytes (then their exclusive prefixes), and the totals behind
    RowRec* rec;
    unsigned char* out;
    const unsigned char* arena;  // the bytes a record's t_off speaks of (none where all rows are raw)
};

inline uint32_t row_tiles(uint64_t n) { return (uint32_t)(((n + 15) / 16 + ROW_TILE_VECS - 1) / ROW_TILE_VECS); }

// line_start(s) for every line of [begin, n) whose preceding newline -- or, for the line at 0, the block's start -- is in
// this thread's 16 vectors, in file order
template <class F> __device__ __forceinline__ void row_each_line(const RowSpan& p, F&& line_start) {
    const uint64_t nvec = (p.n + 15) / 16;
    const uint64_t v0 = ((uint64_t)blockIdx.x * blockDim.x + threadIdx.x) * 16;
    if (v0 == 0 && p.begin == 0 && p.n) line_start(0);
    for (uint64_t v = v0; v < v0 + 16 && v < nvec; v++)
        rf_each_newline(p.text, v, [&](uint64_t at) { if (at + 1 < p.n && at + 1 >= p.begin) line_start(at + 1); });
}

// an exclusive prefix sum over the workgroup's 256 threads of (a, b); the totals to all
__device__ void row_block_exscan(unsigned long long& a, unsigned long long& b, unsigned long long* tot_a, unsigned long long* tot_b) {
    __shared__ unsigned long long sa[256], sb[256];
    const uint32_t t = threadIdx.x;
    const unsigned long long a0 = a, b0 = b;
    sa[t] = a; sb[t] = b;
    __syncthreads();
    for (uint32_t d = 1; d < 256; d <<= 1) {
        const unsigned long long xa = t >= d ? sa[t - d] : 0, xb = t >= d ? sb[t - d] : 0;
        __syncthreads();
        sa[t] += xa; sb[t] += xb;
        __syncthreads();
    }
    a = sa[t] - a0; b = sb[t] - b0;
    *tot_a = sa[255]; *tot_b = sb[255];
    __syncthreads();
}

// the end of a client's plan kernel: this thread's selected rows and their output bytes to thr, the workgroup's to tile
// (whatever the workgroup wrote to LDS before is visible to all behind it)
__device__ __forceinline__ void row_plan(const RowSpan& p, unsigned long long rows, unsigned long long bytes) {
    p.thr[(uint64_t)blockIdx.x * 256 + threadIdx.x] = make_uint2((uint32_t)rows, (uint32_t)bytes);
    unsigned long long ta, tb;
    row_block_exscan(rows, bytes, &ta, &tb);
    if (threadIdx.x == 0) { p.tile[2 * (uint64_t)blockIdx.x] = ta; p.tile[2 * (uint64_t)blockIdx.x + 1] = tb; }
}

// tile[2 i], tile[2 i + 1] -> their exclusive prefixes; the totals to tile[2 n], tile[2 n + 1].  One workgroup
__global__ __launch_bounds__(256) void row_tiles_kernel(unsigned long long* tile, uint64_t n) {
    const uint64_t per = (n + 255) / 256, lo = threadIdx.x * per, hi = lo + per < n ? lo + per : n;
    unsigned long long a = 0, b = 0;
    for (uint64_t i = lo; i < hi; i++) { a += tile[2 * i]; b += tile[2 * i + 1]; }
    unsigned long long ta, tb;
    row_block_exscan(a, b, &ta, &tb);
    for (uint64_t i = lo; i < hi; i++) {
        const unsigned long long xa = tile[2 * i], xb = tile[2 * i + 1];
        tile[2 * i] = a; tile[2 * i + 1] = b;
        a += xa; b += xb;
    }
    if (threadIdx.x == 0) { tile[2 * n] = ta; tile[2 * n + 1] = tb; }
}

// the body of a client's place kernel: the thread's first row and byte from thr and tile, then row(s, r) -> whether the line
// at s is a selected row, r all of its record but dst.  A row the plan left no room for raises `bit` of *err instead
template <class F> __device__ __forceinline__ void row_place(const RowSpan& p, uint64_t n_rows, uint64_t n_bytes, unsigned int* err,
                                                             unsigned int bit, F&& row) {
    const uint2 mine = p.thr[(uint64_t)blockIdx.x * 256 + threadIdx.x];
    unsigned long long k = mine.x, at = mine.y, ta, tb;
    row_block_exscan(k, at, &ta, &tb);
    k += p.tile[2 * (uint64_t)blockIdx.x]; at += p.tile[2 * (uint64_t)blockIdx.x + 1];
    row_each_line(p, [&](uint64_t s) {
        RowRec r;
        if (!row(s, r)) return;
        r.dst = at;
        const uint32_t len = row_out_len(r);
        if (k < n_rows && at + len <= n_bytes) p.rec[k] = r; else atomicOr(err, bit);
        k++; at += len;
    });
}

__global__ __launch_bounds__(256) void row_write_kernel(RowSpan p, uint64_t n_rows) {
    const uint32_t lane = threadIdx.x & 63;
    const uint64_t wave = ((uint64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6, n_waves = ((uint64_t)gridDim.x * blockDim.x) >> 6;
    for (uint64_t g = wave * ROW_GROUP; g < n_rows; g += n_waves * ROW_GROUP) {
        for (uint64_t k = g; k < g + ROW_GROUP && k < n_rows; k++) {
            const RowRec r = p.rec[k];
            const unsigned char* const src = p.text + r.src;
            unsigned char* const dst = p.out + r.dst;
            if (r.raw) { for (uint32_t i = lane; i < r.len0; i += 64) dst[i] = src[i]; continue; }
            // cluster \t k-mer \t text \t fields 1..9 \n
            const uint32_t e0 = r.len0, e1 = e0 + 1 + r.len10, e2 = e1 + 1 + r.t_len, e3 = e2 + 1 + r.mid;
            for (uint32_t i = lane; i <= e3; i += 64) {
                unsigned char c;
                if (i < e0) c = src[i];
                else if (i == e0 || i == e1 || i == e2) c = '\t';
                else if (i < e1) c = src[r.f10 + (i - e0 - 1)];
                else if (i < e2) c = p.arena[r.t_off + (i - e1 - 1)];
                else if (i < e3) c = src[r.f1 + (i - e2 - 1)];
                else c = '\n';
                dst[i] = c;
            }
        }
    }
}

// The text a pass wrote on the device, d_out[0 .. bytes), handed out piece by piece through two pinned buffers
struct RowHandout {
    DevBuf d_out;
    PinBuf pin[2];
    uint64_t bytes = 0, pos = 0, flying = 0;      // the text's bytes, those handed out or on their way, the piece on its way
    int cur = 0;
    void reset() { bytes = pos = flying = 0; }
    // *nbytes = 0: no more; a piece is valid until the next call, which returns the other buffer and starts the copy of the
    // piece behind it into this one
    int next(hipStream_t st, const char** piece, uint64_t* nbytes) {
        *piece = nullptr; *nbytes = 0;
        auto start = [&]() -> int {                    // the next piece on its way into pin[cur]
            flying = std::min<uint64_t>(ROW_PIECE, bytes - pos);
            if (!flying) return PF_OK;
            PFCHK(pin[cur].ensure((size_t)std::min<uint64_t>(ROW_PIECE, bytes), true));
            HIPCHK(hipMemcpyAsync(pin[cur].p, d_out.as<char>() + pos, (size_t)flying, hipMemcpyDeviceToHost, st));
            pos += flying;
            return PF_OK;
        };
        if (!flying) PFCHK(start());
        if (!flying) return PF_OK;
        HIPCHK(hipStreamSynchronize(st));
        *piece = pin[cur].as<char>(); *nbytes = flying;
        cur ^= 1;
        return start();                                // (into the other buffer, while the caller writes this one)
    }
};

// The pack's buffers and its sequence on the client's stream.  run(): p holds the client's text, n and begin; plan(tiles)
// and place(tiles) launch the client's two kernels with p, which has its thr and tile by the first and its rec and out by
// the second.  The plan, the tile sums and the totals are waited for, their time added to *plan_ms; with rows, the place and
// the writer are put on the stream inside the timed bracket and NOT waited for: the client reads its complaint word behind
// them, synchronises once for both and then has the bracket's time from ts.add_elapsed.  out.bytes stays 0: the client
// sets it once the call has succeeded
struct RowPack {
    DevBuf d_thr, d_tile, d_rec;
    RowHandout out;
    template <class Plan, class Place>
    int run(TimedStream& ts, RowSpan& p, float* plan_ms, uint64_t* n_rows, uint64_t* n_bytes, Plan&& plan, Place&& place) {
        const uint32_t tiles = row_tiles(p.n);
        PFCHK(d_thr.ensure((size_t)tiles * 256 * sizeof(uint2)));
        PFCHK(d_tile.ensure(((size_t)tiles + 1) * 16));
        p.thr = d_thr.as<uint2>(); p.tile = d_tile.as<unsigned long long>();
        PFCHK(ts.timed([&]() -> int {
            plan(tiles);
            HIPCHK(hipGetLastError());
            hipLaunchKernelGGL(row_tiles_kernel, dim3(1), dim3(256), 0, ts.stream, p.tile, (uint64_t)tiles);
            HIPCHK(hipGetLastError()); return PF_OK;
        }));
        uint64_t totals[2] = {0, 0};
        HIPCHK(hipMemcpyAsync(totals, p.tile + 2 * (uint64_t)tiles, 16, hipMemcpyDeviceToHost, ts.stream));
        HIPCHK(hipStreamSynchronize(ts.stream));
        ts.add_elapsed(plan_ms);
        *n_rows = totals[0]; *n_bytes = totals[1];
        if (!*n_rows) return PF_OK;
        PFCHK(d_rec.ensure((size_t)*n_rows * sizeof(RowRec)));
        PFCHK(out.d_out.ensure((size_t)*n_bytes));
        p.rec = d_rec.as<RowRec>(); p.out = out.d_out.as<unsigned char>();
        return ts.timed([&]() -> int {
            place(tiles);
            HIPCHK(hipGetLastError());
            const uint64_t groups = (*n_rows + ROW_GROUP - 1) / ROW_GROUP;
            hipLaunchKernelGGL(row_write_kernel, dim3((uint32_t)std::min<uint64_t>((groups + 3) / 4, 256 * 32)), dim3(256), 0, ts.stream, p, *n_rows);
            HIPCHK(hipGetLastError()); return PF_OK;
        });
    }
};

template <class T> int dev_upload(DevBuf& d, const std::vector<T>& v) {
    PFCHK(d.ensure(std::max<size_t>(v.size() * sizeof(T), 16), true));
    if (!v.empty()) HIPCHK(hipMemcpy(d.p, v.data(), v.size() * sizeof(T), hipMemcpyHostToDevice));
    return PF_OK;
}

}  // namespace

// ---------------------------------------------------------------------------------------------------------------------
// panfeed-get-kmers' join: /root/reference/panfeed/get_kmers.py:131-141 on the device.
//
// The reference parses every kmers.tsv row of a bunch of clusters and joins the small table of passing (cluster, k-mer)
// pairs to it (`how="right"`: every row comes out, in file order, with the table's columns or empty fields in front of
// its own).  Here the host renders the table's columns as text once per key (downstream.rendered_texts) and the device
// does the per-row work: find the row's cluster in a table of the selected clusters, its (cluster, k-mer) in a table of
// the keys -- both open addressing on rf_hash values, both verified by bytes HERE, since a written row never reaches the
// host before it is output -- and write  cluster \t k-mer \t <text> \t <fields 2..10 as they stand> \n.
//
// Two kinds of pass over blocks of complete lines, both by the row pack's division of the text (row_each_line).
//   survey   all bunches at once: per bunch, rows, rows without a key, output bytes under either rendering, and the OR
//            of the rows' plainness flags (KJ_*): a flagged row is one pandas' read_csv -> to_csv might not print as it
//            stands, and its bunch goes through pandas
//   join     one bunch, a client of the row pack: kj_plan_kernel counts each thread's rows of the bunch and their output
//            bytes (kj_row, row_plan), kj_place_kernel makes their records (kj_row, row_place); row_tiles_kernel and
//            row_write_kernel are the pack's.  mode 2 keeps the raw rows that have a key instead (--only-passing: pandas
//            joins those few).
// A row of more than KJ_MAX_LINE bytes, or with a field of RF_MAX_FIELD bytes or more, is a flag (KJ_LONG), never a fault.
// ---------------------------------------------------------------------------------------------------------------------
namespace {

constexpr uint32_t KJ_MAX_LINE = 1u << 16;
enum : uint32_t { KJ_TABS = 1, KJ_BYTES = 2, KJ_INT = 4, KJ_EMPTY = 8, KJ_NA = 16, KJ_NUMERIC = 32, KJ_WORD = 64, KJ_LONG = 128 };
enum { KJ_ROWS = 0, KJ_UNMATCHED = 1, KJ_BYTES0 = 2, KJ_BYTES1 = 3, KJ_FLAGS = 4, KJ_COUNTERS = 5 };

struct KjCluster { uint32_t off, len, bunch; };
struct KjKey { uint32_t cl_off, cl_len, km_off, km_len, t_off[2], t_len[2]; };

struct KjParams : RowSpan {      // (arena: the clusters', keys' and texts' bytes)
    const unsigned long long* chash; const uint32_t* cslot; uint64_t ccap; const KjCluster* clusters;
    const unsigned long long* khash; const uint32_t* kslot; uint64_t kcap; const KjKey* keys;
    uint32_t empty_off, empty_len;
    int32_t bunch;               // join: the bunch whose rows are written
    int mode;                    // join: rendering 0 / 1, or 2: the raw rows that have a key
    unsigned long long* counters;        // survey: KJ_COUNTERS per bunch
    unsigned long long* rejects;         // look-ups whose hash was equal and whose bytes were not
    unsigned long long* unmatched;       // join: rows written with the empty text
    unsigned int* err;
};

__device__ __forceinline__ bool kj_same(const unsigned char* a, const unsigned char* b, uint32_t n) {
    for (uint32_t i = 0; i < n; i++) if (a[i] != b[i]) return false;
    return true;
}

// the bunch of the line at s by its first field, -1 if that is no selected cluster; *len0 = the field's length
__device__ int32_t kj_cluster(const KjParams& p, uint64_t s, uint32_t* len0, uint64_t* hash) {
    uint64_t h = 0xCBF29CE484222325ull, e = s;
    while (e - s < RF_MAX_FIELD && p.text[e] != '\t' && p.text[e] != '\n') { h = rf_hash_step(h, p.text[e]); e++; }
    if (e - s >= RF_MAX_FIELD) return -1;                      // (as the row filter: a field this long matches nothing)
    *len0 = (uint32_t)(e - s); *hash = h;
    const uint64_t hf = rf_hash_fin(h);
    uint64_t slot = hf & (p.ccap - 1);
    for (uint64_t probes = 0; probes < p.ccap; probes++) {
        const unsigned long long cur = p.chash[slot];
        if (cur == 0) return -1;
        if (cur == hf) {
            const KjCluster c = p.clusters[p.cslot[slot]];
            if (c.len == *len0 && kj_same(p.arena + c.off, p.text + s, c.len)) return (int32_t)c.bunch;
            atomicAdd(p.rejects, 1ull);
        }
        slot = (slot + 1) & (p.ccap - 1);
    }
    return -1;
}

// the key of (cluster, k-mer), -1 if there is none; h = the unfinished hash of the cluster's bytes
__device__ int64_t kj_key(const KjParams& p, uint64_t h, const unsigned char* cl, uint32_t cl_len, const unsigned char* km, uint32_t km_len) {
    h = rf_hash_step(h, '\t');
    for (uint32_t i = 0; i < km_len; i++) h = rf_hash_step(h, km[i]);
    const uint64_t hf = rf_hash_fin(h);
    uint64_t slot = hf & (p.kcap - 1);
    for (uint64_t probes = 0; probes < p.kcap; probes++) {
        const unsigned long long cur = p.khash[slot];
        if (cur == 0) return -1;
        if (cur == hf) {
            const uint32_t id = p.kslot[slot];
            const KjKey k = p.keys[id];
            if (k.cl_len == cl_len && k.km_len == km_len && kj_same(p.arena + k.cl_off, cl, cl_len) && kj_same(p.arena + k.km_off, km, km_len))
                return id;
            atomicAdd(p.rejects, 1ull);
        }
        slot = (slot + 1) & (p.kcap - 1);
    }
    return -1;
}

__device__ __forceinline__ unsigned char kj_lower(unsigned char c) { return (c >= 'A' && c <= 'Z') ? c + 32 : c; }

// s[0 .. n) is one of the strings of `list` (each ended by a 0, the list by another), case folded or not
__device__ bool kj_in_list(const char* list, const unsigned char* s, uint32_t n, bool fold) {
    while (*list) {
        uint32_t i = 0;
        while (list[i] && i < n && (unsigned char)list[i] == (fold ? kj_lower(s[i]) : s[i])) i++;
        if (!list[i] && i == n) return true;
        while (list[i]) i++;
        list += i + 1;
    }
    return false;
}

// pandas' default NA strings but the empty one, and the words its parsers read as a float or a bool
__device__ const char kj_na_strings[] = "#N/A\0#N/A N/A\0#NA\0-1.#IND\0-1.#QNAN\0-NaN\0-nan\0001.#IND\0001.#QNAN\0<NA>\0N/A\0NA\0NULL\0NaN\0None\0n/a\0nan\0null\0";
__device__ const char kj_words[] = "inf\0infinity\0nan\0true\0false\0";

// the plainness flags of field `idx` of a row
__device__ uint32_t kj_field_flags(const unsigned char* s, uint32_t n, uint32_t idx) {
    if (idx > 10) return 0;                                    // (KJ_TABS says it)
    uint32_t f = n >= RF_MAX_FIELD ? KJ_LONG : 0;
    if (idx >= 4 && idx <= 9) {                                // canonical decimal: -?(0|[1-9][0-9]{0,17}), no -0
        uint32_t i = (n && s[0] == '-') ? 1 : 0;
        const uint32_t digits = n - i;
        bool ok = digits >= 1 && digits <= 18 && !(digits > 1 && s[i] == '0') && !(i && s[i] == '0');
        for (; ok && i < n; i++) ok = s[i] >= '0' && s[i] <= '9';
        return f | (ok ? 0 : KJ_INT);
    }
    if (!n) return f | KJ_EMPTY;
    bool numeric = true;
    for (uint32_t i = 0; numeric && i < n; i++) {
        const unsigned char c = s[i];
        numeric = (c >= '0' && c <= '9') || c == '+' || c == '-' || c == '.' || c == 'e' || c == 'E';
    }
    if (numeric) f |= KJ_NUMERIC;
    if (n <= 9) {
        if (kj_in_list(kj_na_strings, s, n, false)) f |= KJ_NA;
        const uint32_t sign = (s[0] == '+' || s[0] == '-') ? 1 : 0;
        if (kj_in_list(kj_words, s + sign, n - sign, true)) f |= KJ_WORD;
    }
    return f;
}

struct KjWalk { uint32_t len, f1, end9, f10, flags; };     // len without the newline; field 1's start, field 9's end, field 10's start

// the line at s (text[n - 1] is a newline).  FLAGS: all plainness flags; otherwise KJ_TABS and KJ_LONG only
template <bool FLAGS> __device__ void kj_walk(const unsigned char* t, uint64_t s, KjWalk& w) {
    uint32_t tabs = 0, fb = 0, flags = 0, i = 0;
    w.f1 = w.end9 = w.f10 = 0;
    for (;; i++) {
        if (i >= KJ_MAX_LINE) { flags |= KJ_LONG; break; }
        const unsigned char c = t[s + i];
        if (c == '\t' || c == '\n') {
            if (FLAGS) flags |= kj_field_flags(t + s + fb, i - fb, tabs);
            else if (i - fb >= RF_MAX_FIELD) flags |= KJ_LONG;
            if (tabs == 0) w.f1 = i + 1;
            if (tabs == 9) { w.end9 = i; w.f10 = i + 1; }
            if (c == '\n') break;
            tabs++; fb = i + 1;
        } else if (FLAGS && (c < 0x20 || c >= 0x80 || c == '"')) flags |= KJ_BYTES;
    }
    if (tabs != 10) flags |= KJ_TABS;
    w.len = i; w.flags = flags;
}

__global__ __launch_bounds__(256) void kj_survey_kernel(KjParams p) {
    // the workgroup's 64 KiB of text are nearly always rows of one bunch: that bunch's counters are kept in LDS
    __shared__ unsigned long long s_cnt[KJ_COUNTERS];
    __shared__ int s_bunch;
    if (threadIdx.x < KJ_COUNTERS) s_cnt[threadIdx.x] = 0;
    if (threadIdx.x == 0) s_bunch = -1;
    __syncthreads();
    row_each_line(p, [&](uint64_t s) {
        uint32_t len0; uint64_t h;
        const int32_t bunch = kj_cluster(p, s, &len0, &h);
        if (bunch < 0) return;
        KjWalk w;
        kj_walk<true>(p.text, s, w);
        uint64_t bytes[2] = {0, 0};
        bool unmatched = false;
        if (!(w.flags & (KJ_TABS | KJ_LONG))) {
            const int64_t id = kj_key(p, h, p.text + s, len0, p.text + s + w.f10, w.len - w.f10);
            unmatched = id < 0;
            const uint64_t fixed = (uint64_t)len0 + (w.len - w.f10) + (w.end9 - w.f1) + 4;
            for (int r = 0; r < 2; r++) bytes[r] = fixed + (id < 0 ? p.empty_len : p.keys[id].t_len[r]);
        }
        int mine = s_bunch;
        if (mine < 0) { const int old = atomicCAS(&s_bunch, -1, bunch); mine = old < 0 ? bunch : old; }
        unsigned long long* const c = mine == bunch ? s_cnt : p.counters + (uint64_t)bunch * KJ_COUNTERS;
        atomicAdd(&c[KJ_ROWS], 1ull);
        if (unmatched) atomicAdd(&c[KJ_UNMATCHED], 1ull);
        atomicAdd(&c[KJ_BYTES0], (unsigned long long)bytes[0]);
        atomicAdd(&c[KJ_BYTES1], (unsigned long long)bytes[1]);
        if (w.flags) atomicOr(&c[KJ_FLAGS], (unsigned long long)w.flags);
    });
    __syncthreads();
    if (threadIdx.x < KJ_COUNTERS && s_bunch >= 0 && s_cnt[threadIdx.x]) {
        unsigned long long* const c = p.counters + (uint64_t)s_bunch * KJ_COUNTERS + threadIdx.x;
        if (threadIdx.x == KJ_FLAGS) atomicOr(c, s_cnt[threadIdx.x]); else atomicAdd(c, s_cnt[threadIdx.x]);
    }
}

// the row of this join's output the line at s makes, if it makes one (its dst is the pack's); *keyed: it has a key
__device__ bool kj_row(const KjParams& p, uint64_t s, RowRec& r, bool* keyed) {
    uint32_t len0; uint64_t h;
    if (kj_cluster(p, s, &len0, &h) != p.bunch) return false;
    KjWalk w;
    kj_walk<false>(p.text, s, w);
    if (w.flags) { atomicOr(p.err, w.flags); return false; }       // not the file the survey saw
    const int64_t id = kj_key(p, h, p.text + s, len0, p.text + s + w.f10, w.len - w.f10);
    *keyed = id >= 0;
    r.src = s; r.f1 = w.f1; r.mid = w.end9 - w.f1; r.f10 = w.f10; r.len10 = w.len - w.f10;
    if (p.mode == 2) {
        if (id < 0) return false;
        r.raw = 1; r.len0 = w.len + 1; r.t_off = 0; r.t_len = 0;
        return true;
    }
    r.raw = 0; r.len0 = len0;
    r.t_off = id < 0 ? p.empty_off : p.keys[id].t_off[p.mode];
    r.t_len = id < 0 ? p.empty_len : p.keys[id].t_len[p.mode];
    return true;
}

__global__ __launch_bounds__(256) void kj_plan_kernel(KjParams p) {
    unsigned long long rows = 0, bytes = 0, unmatched = 0;
    row_each_line(p, [&](uint64_t s) {
        RowRec r; bool keyed;
        if (kj_row(p, s, r, &keyed)) { rows++; bytes += row_out_len(r); unmatched += !keyed; }
    });
    if (unmatched) atomicAdd(p.unmatched, unmatched);
    row_plan(p, rows, bytes);
}

__global__ __launch_bounds__(256) void kj_place_kernel(KjParams p, uint64_t n_rows, uint64_t n_bytes) {
    row_place(p, n_rows, n_bytes, p.err, 0x80000000u, [&](uint64_t s, RowRec& r) { bool keyed; return kj_row(p, s, r, &keyed); });
}

}  // namespace

struct pf_kmerjoin {
    uint32_t n_bunches = 0;
    uint64_t ccap = 0, kcap = 0;
    uint32_t empty_off = 0, empty_len = 0;
    DevBuf d_chash, d_cslot, d_clusters, d_khash, d_kslot, d_keys, d_arena, d_counters, d_misc;     // d_misc: rejects, err, unmatched
    std::vector<uint64_t> counters;
    RowPack pack;                                // pack.out: the join's text
    uint64_t bytes_scanned = 0, rows_written = 0, raw_rows = 0;
    float survey_ms = 0, write_ms = 0;
    // pf_kmerjoin_set_gzip: the text of a mode 0 / 1 call leaves as gzip members.  The encoder is made on first use; a call's
    // text is encoded a slice of at most PfGzEncoder::BLOCK bytes at a time, slice by slice as its members are handed out,
    // so the encoder's buffers and gz.d_out, the slice's members, take PfGzEncoder::bound(BLOCK) bytes each at most
    bool gz_on = false, gz_now = false;          // the switch; whether the last join call's text is one to encode
    uint32_t gz_flags = 0;
    PfGzEncoder enc;
    RowHandout gz;                               // the members of the slice pack.out.d_out[gz_at - its bytes .. gz_at)
    uint64_t gz_at = 0;                          // text bytes of the call encoded so far
    uint64_t gz_text_bytes = 0, gz_member_bytes = 0;
    float gz_ms = 0;
    TextFeed feed;                               // (its stream goes first: a piece of text may be on its way down into pin)
};

namespace {

// nothing of an earlier join call is left to hand out
void kj_reset_out(pf_kmerjoin* j) { j->pack.out.reset(); j->gz.reset(); j->gz_at = 0; j->gz_now = false; }

KjParams kj_params(pf_kmerjoin* j, uint64_t n, uint64_t begin) {
    KjParams p{};
    p.text = j->feed.text.d_text.as<unsigned char>(); p.n = n; p.begin = begin;
    p.chash = j->d_chash.as<unsigned long long>(); p.cslot = j->d_cslot.as<uint32_t>(); p.ccap = j->ccap; p.clusters = j->d_clusters.as<KjCluster>();
    p.khash = j->d_khash.as<unsigned long long>(); p.kslot = j->d_kslot.as<uint32_t>(); p.kcap = j->kcap; p.keys = j->d_keys.as<KjKey>();
    p.arena = j->d_arena.as<unsigned char>(); p.empty_off = j->empty_off; p.empty_len = j->empty_len;
    p.counters = j->d_counters.as<unsigned long long>();
    p.rejects = j->d_misc.as<unsigned long long>(); p.err = reinterpret_cast<unsigned int*>(j->d_misc.as<unsigned long long>() + 1);
    p.unmatched = j->d_misc.as<unsigned long long>() + 2;
    return p;
}

// the survey of d_text[begin .. n)
int kj_survey_device(pf_kmerjoin* j, uint64_t n, uint64_t begin) {
    if (n <= begin) return PF_OK;
    TimedStream& ts = j->feed.ts;
    const KjParams p = kj_params(j, n, begin);
    PFCHK(ts.timed([&]() -> int {
        hipLaunchKernelGGL(kj_survey_kernel, dim3(row_tiles(n)), dim3(256), 0, ts.stream, p);
        HIPCHK(hipGetLastError()); return PF_OK;
    }));
    HIPCHK(hipStreamSynchronize(ts.stream));
    ts.add_elapsed(&j->survey_ms);
    j->bytes_scanned += n - begin;
    return PF_OK;
}

// the join of d_text[begin .. n) for one bunch: the text in pack.out.d_out[0 .. pack.out.bytes), ready to be handed out
int kj_join_device(pf_kmerjoin* j, uint64_t n, uint64_t begin, uint32_t bunch, int mode) {
    kj_reset_out(j);
    if (n <= begin) return PF_OK;
    if (bunch >= j->n_bunches || mode < 0 || mode > 2) return fail(PF_ERR_ARG, "pf_kmerjoin_join: no such bunch or mode");
    TimedStream& ts = j->feed.ts;
    KjParams p = kj_params(j, n, begin);
    p.bunch = (int32_t)bunch; p.mode = mode;
    HIPCHK(hipMemsetAsync(p.err, 0, 4, ts.stream));      // (kj_row complains in either pass: the word is this call's alone)
    float ms = 0;
    uint64_t n_rows = 0, n_bytes = 0;
    PFCHK(j->pack.run(ts, p, &ms, &n_rows, &n_bytes,
                      [&](uint32_t tiles) { hipLaunchKernelGGL(kj_plan_kernel, dim3(tiles), dim3(256), 0, ts.stream, p); },
                      [&](uint32_t tiles) { hipLaunchKernelGGL(kj_place_kernel, dim3(tiles), dim3(256), 0, ts.stream, p, n_rows, n_bytes); }));
    j->bytes_scanned += n - begin;
    unsigned int err = 0;                                  // (read even when no row was placed: the plan may have complained)
    HIPCHK(hipMemcpyAsync(&err, p.err, 4, hipMemcpyDeviceToHost, ts.stream));
    HIPCHK(hipStreamSynchronize(ts.stream));
    if (n_rows) ts.add_elapsed(&ms);
    j->write_ms += ms;
    if (err) return fail(PF_ERR_STATE, "pf_kmerjoin_join: a row of the bunch is not one the survey passed (flags 0x%x): the file has changed", err);
    j->pack.out.bytes = n_bytes;
    j->gz_now = j->gz_on && mode != 2;            // (the raw rows go to pandas: they stay text)
    if (mode == 2) j->raw_rows += n_rows; else j->rows_written += n_rows;
    return PF_OK;
}

// With the switch on: the next piece of the members of the last join call's text.  A slice's members are handed out to
// their end, then the next slice is encoded in their place (the pieces handed out are in pinned memory by then)
int kj_next_members(pf_kmerjoin* j, const char** piece, uint64_t* nbytes) {
    TimedStream& ts = j->feed.ts;
    constexpr PfGzEncoder::Cursor W = PfGzEncoder::STREAM_BLOCK0;
    for (;;) {
        PFCHK(j->gz.next(ts.stream, piece, nbytes));
        if (*nbytes || j->gz_at >= j->pack.out.bytes) return PF_OK;
        const uint64_t m = std::min<uint64_t>(PfGzEncoder::BLOCK, j->pack.out.bytes - j->gz_at), cap = PfGzEncoder::bound(m);
        if (!j->enc.grid_cap) {
            int n_cu = 0;
            HIPCHK(hipDeviceGetAttribute(&n_cu, hipDeviceAttributeMultiprocessorCount, j->feed.device));
            PFCHK(j->enc.ensure(n_cu > 0 ? n_cu : 256));
        }
        // (a buffer that is re-made gets a quarter more, up to what a whole slice may take)
        if (cap > j->gz.d_out.cap) PFCHK(j->gz.d_out.ensure((size_t)std::min<uint64_t>(PfGzEncoder::bound(PfGzEncoder::BLOCK), cap + cap / 4), true));
        j->gz.reset();
        PFCHK(j->enc.encode(ts.stream, W, j->pack.out.d_out.as<char>() + j->gz_at, m, j->gz_flags, j->gz.d_out.as<char>(), cap, ts.e0, ts.e1));
        HIPCHK(hipStreamSynchronize(ts.stream));
        ts.add_elapsed(&j->gz_ms);
        PFCHK(j->enc.member_bytes(W, &j->gz.bytes));
        j->gz_at += m; j->gz_text_bytes += m; j->gz_member_bytes += j->gz.bytes;
    }
}

}  // namespace

extern "C" {

void pf_kmerjoin_destroy(pf_kmerjoin* j) { feed_destroy(j); }

int pf_kmerjoin_create(int device, const char* const* clusters, const uint32_t* cluster_len, const uint32_t* cluster_bunch,
                       uint64_t n_clusters, uint32_t n_bunches, const char* const* key_cluster, const uint32_t* key_cluster_len,
                       const char* const* key_kmer, const uint32_t* key_kmer_len, const char* const* text0, const uint32_t* text0_len,
                       const char* const* text1, const uint32_t* text1_len, uint64_t n_keys, const char* empty_text,
                       uint32_t empty_len, pf_kmerjoin** out) {
    if (!out || (n_clusters && (!clusters || !cluster_len || !cluster_bunch)) || (empty_len && !empty_text) ||
        (n_keys && (!key_cluster || !key_cluster_len || !key_kmer || !key_kmer_len || !text0 || !text0_len || !text1 || !text1_len)))
        return fail(PF_ERR_ARG, "pf_kmerjoin_create: null argument");
    *out = nullptr;
    FeedHandle<pf_kmerjoin> j(nullptr, pf_kmerjoin_destroy); PFCHK(feed_create(device, "pf_kmerjoin_create", j));
    j->n_bunches = std::max<uint32_t>(n_bunches, 1);
    std::string arena;
    auto put = [&arena](const char* s, uint32_t n) { const size_t at = arena.size(); arena.append(s, n); return (uint32_t)at; };
    auto insert = [](std::vector<unsigned long long>& hash, std::vector<uint32_t>& slot_id, uint64_t h, uint32_t id) {
        slot_id[pf_table_insert(hash, h, [](uint64_t) { return false; })] = id;     // (equal hashes take slots of their own: the bytes tell them apart)
    };
    j->empty_off = put(empty_text, empty_len); j->empty_len = empty_len;
    // the selected clusters (one that comes twice keeps its first bunch)
    std::vector<KjCluster> cl;
    std::vector<unsigned long long> chash(j->ccap = pf_table_room(n_clusters, 4), RF_EMPTY);
    std::vector<uint32_t> cslot(j->ccap, 0);
    std::unordered_set<std::string> seen;
    for (uint64_t i = 0; i < n_clusters; i++) {
        if (cluster_len[i] >= RF_MAX_FIELD || cluster_bunch[i] >= j->n_bunches) continue;      // cannot match, as in the row filter
        if (!seen.emplace(clusters[i], cluster_len[i]).second) continue;
        insert(chash, cslot, rf_hash(clusters[i], cluster_len[i]), (uint32_t)cl.size());
        cl.push_back(KjCluster{put(clusters[i], cluster_len[i]), cluster_len[i], cluster_bunch[i]});
    }
    // the keys: the hash runs over cluster, a tab, k-mer
    std::vector<KjKey> keys;
    std::vector<unsigned long long> khash(j->kcap = pf_table_room(n_keys, 4), RF_EMPTY);
    std::vector<uint32_t> kslot(j->kcap, 0);
    seen.clear();
    for (uint64_t i = 0; i < n_keys; i++) {
        if (key_cluster_len[i] >= RF_MAX_FIELD || key_kmer_len[i] >= RF_MAX_FIELD) continue;
        // (a thread's rows -- 17 at most, of KJ_MAX_LINE bytes and a text each -- are counted in 32 bits)
        if (text0_len[i] >= (1u << 24) || text1_len[i] >= (1u << 24)) return fail(PF_ERR_CAPACITY, "pf_kmerjoin_create: a key's text takes 16 MiB or more");
        std::string both(key_cluster[i], key_cluster_len[i]);
        both.push_back('\t'); both.append(key_kmer[i], key_kmer_len[i]);
        if (!seen.insert(both).second) return fail(PF_ERR_ARG, "pf_kmerjoin_create: key %llu comes twice", (unsigned long long)i);
        insert(khash, kslot, rf_hash(both.data(), both.size()), (uint32_t)keys.size());
        KjKey k{};
        k.cl_off = put(key_cluster[i], key_cluster_len[i]); k.cl_len = key_cluster_len[i];
        k.km_off = put(key_kmer[i], key_kmer_len[i]); k.km_len = key_kmer_len[i];
        k.t_off[0] = put(text0[i], text0_len[i]); k.t_len[0] = text0_len[i];
        k.t_off[1] = put(text1[i], text1_len[i]); k.t_len[1] = text1_len[i];
        keys.push_back(k);
    }
    if (arena.size() >= (1ull << 32)) return fail(PF_ERR_CAPACITY, "pf_kmerjoin_create: the keys and their texts take 4 GiB or more");
    j->counters.assign((size_t)j->n_bunches * KJ_COUNTERS, 0);
    PFCHK(dev_upload(j->d_chash, chash)); PFCHK(dev_upload(j->d_cslot, cslot)); PFCHK(dev_upload(j->d_clusters, cl));
    PFCHK(dev_upload(j->d_khash, khash)); PFCHK(dev_upload(j->d_kslot, kslot)); PFCHK(dev_upload(j->d_keys, keys));
    PFCHK(dev_upload(j->d_arena, std::vector<char>(arena.begin(), arena.end())));
    PFCHK(dev_upload(j->d_counters, j->counters));
    PFCHK(dev_upload(j->d_misc, std::vector<uint64_t>(3, 0)));
    *out = j.release();
    return PF_OK;
}

int pf_kmerjoin_survey(pf_kmerjoin* j, const char* text, uint64_t nbytes, uint64_t* consumed) {
    if (!j || !consumed || (nbytes && !text)) return fail(PF_ERR_ARG, "pf_kmerjoin_survey: null argument");
    HIPCHK(hipSetDevice(j->feed.device));
    PFCHK(j->feed.plain(text, nbytes, consumed));
    return kj_survey_device(j, *consumed, 0);
}

int pf_kmerjoin_members_begin(pf_kmerjoin* j, int header) { return feed_members_begin(j, "pf_kmerjoin_members_begin", header); }
int pf_kmerjoin_set_large_members(pf_kmerjoin* j, int on, uint32_t piece_bytes) { return feed_set_large(j, "pf_kmerjoin_set_large_members", on, piece_bytes); }
int pf_kmerjoin_large_stats(pf_kmerjoin* j, uint64_t* pieces, float* ms) { return feed_large_stats(j, "pf_kmerjoin_large_stats", pieces, ms); }

int pf_kmerjoin_members_header(pf_kmerjoin* j, const char** line, uint64_t* nbytes) {
    return feed_members_header(j, "pf_kmerjoin_members_header", line, nbytes);
}

int pf_kmerjoin_survey_members(pf_kmerjoin* j, const char* members, uint64_t nbytes, int last, uint64_t* consumed, int* taken) {
    if (!j || !consumed || !taken || (nbytes && !members)) return fail(PF_ERR_ARG, "pf_kmerjoin_survey_members: null argument");
    HIPCHK(hipSetDevice(j->feed.device));
    return j->feed.members(members, nbytes, last, consumed, taken, [j](uint64_t n, uint64_t skip) { return kj_survey_device(j, n, skip); });
}

int pf_kmerjoin_reset_counters(pf_kmerjoin* j) {
    if (!j) return fail(PF_ERR_ARG, "pf_kmerjoin_reset_counters: null argument");
    HIPCHK(hipSetDevice(j->feed.device));
    HIPCHK(hipMemset(j->d_counters.p, 0, j->counters.size() * 8));
    return PF_OK;
}

int pf_kmerjoin_counters(pf_kmerjoin* j, const uint64_t** counters, uint32_t* n_bunches) {
    if (!j || !counters || !n_bunches) return fail(PF_ERR_ARG, "pf_kmerjoin_counters: null argument");
    HIPCHK(hipSetDevice(j->feed.device));
    HIPCHK(hipMemcpy(j->counters.data(), j->d_counters.p, j->counters.size() * 8, hipMemcpyDeviceToHost));
    *counters = j->counters.data(); *n_bunches = j->n_bunches;
    return PF_OK;
}

int pf_kmerjoin_join(pf_kmerjoin* j, const char* text, uint64_t nbytes, uint32_t bunch, int mode, uint64_t* out_bytes, uint64_t* consumed) {
    if (!j || !out_bytes || !consumed || (nbytes && !text)) return fail(PF_ERR_ARG, "pf_kmerjoin_join: null argument");
    HIPCHK(hipSetDevice(j->feed.device));
    *out_bytes = 0; kj_reset_out(j);
    PFCHK(j->feed.plain(text, nbytes, consumed));
    PFCHK(kj_join_device(j, *consumed, 0, bunch, mode));
    *out_bytes = j->pack.out.bytes;
    return PF_OK;
}

int pf_kmerjoin_join_members(pf_kmerjoin* j, const char* members, uint64_t nbytes, int last, uint32_t bunch, int mode,
                             uint64_t* out_bytes, uint64_t* consumed, int* taken) {
    if (!j || !out_bytes || !consumed || !taken || (nbytes && !members)) return fail(PF_ERR_ARG, "pf_kmerjoin_join_members: null argument");
    HIPCHK(hipSetDevice(j->feed.device));
    *out_bytes = 0; kj_reset_out(j);
    PFCHK(j->feed.members(members, nbytes, last, consumed, taken,
                           [j, bunch, mode](uint64_t n, uint64_t skip) { return kj_join_device(j, n, skip, bunch, mode); }));
    *out_bytes = j->pack.out.bytes;
    return PF_OK;
}

int pf_kmerjoin_next_text(pf_kmerjoin* j, const char** piece, uint64_t* nbytes) {
    if (!j || !piece || !nbytes) return fail(PF_ERR_ARG, "pf_kmerjoin_next_text: null argument");
    HIPCHK(hipSetDevice(j->feed.device));
    return j->gz_now ? kj_next_members(j, piece, nbytes) : j->pack.out.next(j->feed.ts.stream, piece, nbytes);
}

int pf_kmerjoin_set_gzip(pf_kmerjoin* j, int on, uint32_t flags) {
    if (!j) return fail(PF_ERR_ARG, "pf_kmerjoin_set_gzip: null argument");
    if (flags & ~(PF_GZ_FIXED_ONLY | PF_GZ_DYNAMIC_ONLY | PF_GZ_LITERALS_ONLY | PF_GZ_DEEP)) return fail(PF_ERR_ARG, "pf_kmerjoin_set_gzip: unknown flag");
    kj_reset_out(j);                              // (a text half handed out would change its kind)
    j->gz_on = on != 0; j->gz_flags = flags;
    return PF_OK;
}

int pf_kmerjoin_gzip_stats(pf_kmerjoin* j, uint64_t* text_bytes, uint64_t* member_bytes, float* encode_ms, uint64_t* device_bytes) {
    if (!j) return fail(PF_ERR_ARG, "pf_kmerjoin_gzip_stats: null argument");
    if (text_bytes) *text_bytes = j->gz_text_bytes;
    if (member_bytes) *member_bytes = j->gz_member_bytes;
    if (encode_ms) *encode_ms = j->gz_ms;
    if (device_bytes) *device_bytes = j->enc.device_bytes() + j->gz.d_out.cap;
    return PF_OK;
}

int pf_kmerjoin_stats(pf_kmerjoin* j, uint64_t stats[8], float ms[3]) {
    if (!j) return fail(PF_ERR_ARG, "pf_kmerjoin_stats: null argument");
    HIPCHK(hipSetDevice(j->feed.device));
    if (stats) {
        uint64_t misc[3] = {0, 0, 0};                          // rejects, err, unmatched
        HIPCHK(hipMemcpy(misc, j->d_misc.p, sizeof misc, hipMemcpyDeviceToHost));
        stats[0] = j->bytes_scanned; stats[1] = j->rows_written; stats[2] = j->raw_rows; stats[3] = j->feed.gz_members;
        stats[4] = j->feed.gz_text_bytes; stats[5] = j->feed.dec.device_bytes() + j->feed.lg.device_bytes(); stats[6] = misc[0]; stats[7] = misc[2];
    }
    if (ms) { ms[0] = j->survey_ms; ms[1] = j->write_ms; ms[2] = j->feed.gz_ms; }
    return PF_OK;
}

}  // extern "C"

// ---------------------------------------------------------------------------------------------------------------------
// The associations filter: the first step of both downstream tools,
//   /root/reference/panfeed/get_clusters.py:76-88, /root/reference/panfeed/get_kmers.py:93-106
//     a = pd.read_csv(associations, sep='\t', index_col=0);  a = a[a[column] <= threshold]
// as one pass over the file's text, a third owner of the TextFeed.  The host parses with pandas only the lines this pass
// keeps; that the table comes out as from the whole file rests on two things the pass finds out:
//   the kept lines   every data line whose p-value cell MAY satisfy value <= threshold, as it stands, in file order.  The
//                    decision is a superset: the cell's text becomes a double within 2^-48 of the decimal it spells (see
//                    af_value) and the row is dropped only above thr_hi, the threshold widened by 2^-30; pandas decides
//                    exactly on what is left
//   the classes      per column, the OR over ALL data rows of each cell's class (AF_INT ...): they tell the dtype pandas
//                    would have inferred for the column from the whole file, and so how to_csv prints the kept rows
// and the OR of the rows' flags (AF_ROW_*): a flagged table, one with an AF_ODD cell or one whose classes pandas would mix
// goes through pandas whole (the routing is the caller's).
// Kernels: the second client of the row pack.  af_plan_kernel walks every line once -- classes, flags, keep or drop,
// per-thread rows and bytes -- and ends in row_plan; af_place_kernel is the walk of the p-value cell alone under row_place;
// row_tiles_kernel between them and row_write_kernel behind them, all rows raw, are the pack's.
// ---------------------------------------------------------------------------------------------------------------------
namespace {

enum : uint32_t { AF_INT = PF_AF_INT, AF_FLOAT = PF_AF_FLOAT, AF_NA = PF_AF_NA, AF_ODD = PF_AF_ODD, AF_TEXT = PF_AF_TEXT };
enum : uint32_t { AF_ROW_FIELDS = PF_AF_ROW_FIELDS, AF_ROW_EMPTY = PF_AF_ROW_EMPTY, AF_ROW_BYTES = PF_AF_ROW_BYTES, AF_ROW_LONG = PF_AF_ROW_LONG };
constexpr uint32_t AF_LDS_COLS = 256;            // columns whose class bits a workgroup gathers in LDS; the rest go to HBM
constexpr uint32_t AF_DIGITS = 17;               // digits of a number's text that count, leading zeros among them, as in pandas
constexpr uint32_t AF_INT_DIGITS = 18;           // an integer of more digits may not fit int64
constexpr uint32_t AF_EXP_DIGITS = 5;
constexpr int32_t AF_DECADES = 300;              // |value| within 1e-300 .. 1e300 is decided here

struct AfParams : RowSpan {      // (no arena: every kept line is a raw row)
    uint32_t pvalue_field, n_fields;
    double thr_hi;
    unsigned int* cols;          // n_fields words of class bits
    unsigned int* flags;         // [0] the OR of the rows' flags, [1] a place kernel that found other rows than the plan
    unsigned long long* rows;    // data lines
};

// One cell, byte by byte: the number grammar  [+-]?([0-9]+\.?[0-9]*|\.[0-9]+)([eE][+-]?[0-9]+)?  and what its value needs.
// st: 0 nothing yet, 1 sign, 2 integer digits, 3 behind the point with a digit somewhere, 4 a point and no digit yet, 6 e,
// 7 the exponent's sign, 8 exponent digits, 9 no number; a number ends in 2, 3 or 8
struct AfCell {
    uint32_t st = 0, n_int = 0, taken = 0, sig = 0, n_exp = 0, len = 0;
    int32_t adj = 0, ex = 0;
    bool neg = false, eneg = false;
    unsigned char first = 0, last = 0;
    uint64_t m = 0;
    __device__ __forceinline__ void step(unsigned char c) {
        if (!len) first = c;
        last = c; len++;
        const uint32_t d = (uint32_t)c - '0';
        if (d < 10) {
            const bool take = taken < AF_DIGITS;
            if (st <= 2) { st = 2; n_int++; if (!take) adj++; }
            else if (st == 3 || st == 4) { st = 3; if (take) adj--; }
            else if (st >= 6 && st <= 8) { st = 8; n_exp++; if (ex < 100000) ex = ex * 10 + (int32_t)d; return; }
            else { st = 9; return; }
            if (take) { m = m * 10 + d; taken++; if (m) sig++; }
        } else if (c == '+' || c == '-') {
            if (st == 0) { st = 1; neg = c == '-'; } else if (st == 6) { st = 7; eneg = c == '-'; } else st = 9;
        } else if (c == '.') {
            st = st == 2 ? 3 : st <= 1 ? 4 : 9;
        } else if (c == 'e' || c == 'E') {
            st = (st == 2 || st == 3) ? 6 : 9;
        } else st = 9;
    }
};

// the class of a finished cell; s: its bytes.  AF_ODD: a cell pandas may read otherwise in a subset of the file than in the
// whole -- a word of kj_words, a space at either end, an integer of more than 18 digits, and a number its float parser
// may refuse or overflow (more than 18 integer digits, more than 5 exponent digits, 1e300 or more by its exponent)
__device__ uint32_t af_class(const AfCell& c, const unsigned char* s) {
    if (!c.len) return AF_NA;
    if (c.first == ' ' || c.last == ' ') return AF_ODD;
    if (c.st == 2) return c.n_int <= AF_INT_DIGITS ? AF_INT : AF_ODD;
    if (c.st == 3 || c.st == 8)
        return (c.n_int > AF_INT_DIGITS || c.n_exp > AF_EXP_DIGITS || (!c.eneg && c.ex + (int32_t)c.n_int > AF_DECADES)) ? AF_ODD : AF_FLOAT;
    if (c.len <= 9) {
        if (kj_in_list(kj_na_strings, s, c.len, false)) return AF_NA;
        const uint32_t sign = (s[0] == '+' || s[0] == '-') ? 1 : 0;
        if (kj_in_list(kj_words, s + sign, c.len - sign, true)) return AF_ODD;
    }
    return AF_TEXT;
}

// Whether a p-value cell of class AF_INT or AF_FLOAT may be <= the threshold.  Its value as pandas' parser takes it is
// m * 10^e: m the first 17 digits of the text (leading zeros count, an integer digit behind them raises e, a fraction digit
// behind them is dropped).  m = 0 is exactly +-0.  Else m has `sig` digits and |value| lies in [10^(sig-1+e), 10^(sig+e)):
// outside 1e-300 .. 1e300 the row is undecided and kept.  Inside, v = double(m) times at most nine of 10^(+-2^k):
// the conversion rounds once (m < 10^17 has up to 57 bits), every factor is within 2^-53 of its power and every product rounds
// once, no product leaves the normal range (they move from m >= 1 towards the result monotonically): |v / (m 10^e) - 1| <=
// (1 + 2 * 9) * 2^-53 < 2^-48.  The row is dropped only if v > thr_hi
__device__ bool af_keep(const AfCell& c, double thr_hi) {
    double v = 0.0;
    if (c.m) {
        const int32_t e = c.adj + (c.eneg ? -c.ex : c.ex), lo = (int32_t)c.sig - 1 + e;
        if (lo < -AF_DECADES || lo + 1 > AF_DECADES) return true;
        v = (double)(long long)c.m;
        const uint32_t a = (uint32_t)(e < 0 ? -e : e);
        const double up[9] = {1e1, 1e2, 1e4, 1e8, 1e16, 1e32, 1e64, 1e128, 1e256};
        const double dn[9] = {1e-1, 1e-2, 1e-4, 1e-8, 1e-16, 1e-32, 1e-64, 1e-128, 1e-256};
#pragma unroll
        for (int b = 0; b < 9; b++) if ((a >> b) & 1) v *= e < 0 ? dn[b] : up[b];
    }
    return (c.neg ? -v : v) <= thr_hi;
}

struct AfRow { uint32_t len, flags; bool keep; };       // len with the newline

// the line at s (text[n - 1] is a newline), read a 32-bit word every four bytes.  SURVEY: every cell's class goes to
// col(field, class) and the row's flags are found; otherwise the p-value cell alone is looked at
template <bool SURVEY, class C> __device__ void af_walk(const AfParams& p, uint64_t s, AfRow& r, C&& col) {
    const uint32_t* const words = reinterpret_cast<const uint32_t*>(p.text);
    uint32_t word = words[s >> 2];
    uint32_t field = 0, fb = 0, flags = 0, i = 0;
    AfCell cell;
    r.keep = false;
    for (;; i++) {
        if (i >= KJ_MAX_LINE) { flags |= AF_ROW_LONG; break; }
        const uint64_t pos = s + i;
        if (i && !(pos & 3)) word = words[pos >> 2];
        const unsigned char c = (unsigned char)(word >> ((pos & 3) * 8));
        if (c == '\t' || c == '\n') {
            if (i - fb >= RF_MAX_FIELD) flags |= AF_ROW_LONG;
            if (SURVEY || field == p.pvalue_field) {
                const uint32_t cls = af_class(cell, p.text + s + fb);
                if (SURVEY && field < p.n_fields) col(field, cls);
                if (field == p.pvalue_field) r.keep = (cls & (AF_INT | AF_FLOAT)) && af_keep(cell, p.thr_hi);
            }
            if (c == '\n') break;
            field++; fb = i + 1; cell = AfCell();
        } else {
            if (SURVEY && (c < 0x20 || c == '"')) flags |= AF_ROW_BYTES;
            if (SURVEY || field == p.pvalue_field) cell.step(c);
        }
    }
    if (field + 1 != p.n_fields) flags |= AF_ROW_FIELDS;
    if (i == 0) flags |= AF_ROW_EMPTY;
    if (flags & AF_ROW_LONG) r.keep = false;
    r.len = i + 1; r.flags = flags;
}

__global__ __launch_bounds__(256) void af_plan_kernel(AfParams p) {
    __shared__ unsigned int s_cols[AF_LDS_COLS];
    __shared__ unsigned int s_flags;
    __shared__ unsigned long long s_lines;
    for (uint32_t k = threadIdx.x; k < AF_LDS_COLS; k += 256) s_cols[k] = 0;
    if (threadIdx.x == 0) { s_flags = 0; s_lines = 0; }
    __syncthreads();
    unsigned long long rows = 0, bytes = 0, lines = 0;
    uint32_t flags = 0;
    // (a bit once set stays set: a stale look can only cost an atomic, never lose a bit)
    auto col = [&](uint32_t field, uint32_t cls) {
        unsigned int* const at = field < AF_LDS_COLS ? &s_cols[field] : &p.cols[field];
        if ((*at & cls) != cls) atomicOr(at, cls);
    };
    row_each_line(p, [&](uint64_t s) {
        AfRow r;
        af_walk<true>(p, s, r, col);
        lines++; flags |= r.flags;
        if (r.keep) { rows++; bytes += r.len; }
    });
    if (flags) atomicOr(&s_flags, flags);
    if (lines) atomicAdd(&s_lines, lines);
    row_plan(p, rows, bytes);
    if (threadIdx.x == 0) {
        if (s_flags) atomicOr(&p.flags[0], s_flags);
        if (s_lines) atomicAdd(p.rows, s_lines);
    }
    for (uint32_t k = threadIdx.x; k < AF_LDS_COLS && k < p.n_fields; k += 256)
        if (s_cols[k] & ~p.cols[k]) atomicOr(&p.cols[k], s_cols[k]);
}

__global__ __launch_bounds__(256) void af_place_kernel(AfParams p, uint64_t n_rows, uint64_t n_bytes) {
    row_place(p, n_rows, n_bytes, &p.flags[1], 1u, [&](uint64_t s, RowRec& r) {
        AfRow w;
        af_walk<false>(p, s, w, [](uint32_t, uint32_t) {});
        if (!w.keep) return false;
        r = RowRec{};
        r.src = s; r.len0 = w.len; r.raw = 1;
        return true;
    });
}

}  // namespace

struct pf_assocfilter {
    uint32_t pvalue_field = 0, n_fields = 0;
    double thr_hi = 0;
    DevBuf d_cols, d_misc;                       // d_misc: data lines (8 bytes), the rows' flags and the place kernel's complaint (4 each)
    std::vector<uint32_t> cols;
    RowPack pack;                                // pack.out: the kept lines of the last scan
    uint64_t bytes_scanned = 0, kept = 0;
    float device_ms = 0;
    TextFeed feed;                               // (its stream goes first: a piece of text may be on its way down into pin)
};

namespace {

// the scan of d_text[begin .. n): the kept lines in pack.out.d_out[0 .. pack.out.bytes), ready to be handed out
int af_scan_device(pf_assocfilter* f, uint64_t n, uint64_t begin) {
    f->pack.out.reset();
    if (n <= begin) return PF_OK;
    TimedStream& ts = f->feed.ts;
    AfParams p{};
    p.text = f->feed.text.d_text.as<unsigned char>(); p.n = n; p.begin = begin;
    p.pvalue_field = f->pvalue_field; p.n_fields = f->n_fields; p.thr_hi = f->thr_hi;
    p.cols = f->d_cols.as<unsigned int>();
    p.rows = f->d_misc.as<unsigned long long>(); p.flags = reinterpret_cast<unsigned int*>(f->d_misc.as<unsigned long long>() + 1);
    uint64_t n_rows = 0, n_bytes = 0;
    PFCHK(f->pack.run(ts, p, &f->device_ms, &n_rows, &n_bytes,
                      [&](uint32_t tiles) { hipLaunchKernelGGL(af_plan_kernel, dim3(tiles), dim3(256), 0, ts.stream, p); },
                      [&](uint32_t tiles) { hipLaunchKernelGGL(af_place_kernel, dim3(tiles), dim3(256), 0, ts.stream, p, n_rows, n_bytes); }));
    f->bytes_scanned += n - begin;
    if (!n_rows) return PF_OK;                      // (only the place pass complains, and the word is never cleared)
    unsigned int err = 0;
    HIPCHK(hipMemcpyAsync(&err, p.flags + 1, 4, hipMemcpyDeviceToHost, ts.stream));
    HIPCHK(hipStreamSynchronize(ts.stream));
    ts.add_elapsed(&f->device_ms);
    if (err) return fail(PF_ERR_STATE, "pf_assocfilter_scan: the place pass found other rows than the plan pass");
    f->pack.out.bytes = n_bytes; f->kept += n_rows;
    return PF_OK;
}

}  // namespace

extern "C" {

void pf_assocfilter_destroy(pf_assocfilter* f) { feed_destroy(f); }

int pf_assocfilter_create(int device, uint32_t pvalue_field, uint32_t n_fields, double thr_hi, pf_assocfilter** out) {
    if (!out) return fail(PF_ERR_ARG, "pf_assocfilter_create: null argument");
    *out = nullptr;
    if (!n_fields || pvalue_field >= n_fields) return fail(PF_ERR_ARG, "pf_assocfilter_create: the p-value field is not one of the header's");
    FeedHandle<pf_assocfilter> f(nullptr, pf_assocfilter_destroy); PFCHK(feed_create(device, "pf_assocfilter_create", f));
    f->pvalue_field = pvalue_field; f->n_fields = n_fields; f->thr_hi = thr_hi;
    f->cols.assign(n_fields, 0);
    PFCHK(dev_upload(f->d_cols, f->cols));
    PFCHK(dev_upload(f->d_misc, std::vector<uint64_t>(2, 0)));
    *out = f.release();
    return PF_OK;
}

int pf_assocfilter_scan(pf_assocfilter* f, const char* text, uint64_t nbytes, uint64_t* out_bytes, uint64_t* consumed) {
    if (!f || !out_bytes || !consumed || (nbytes && !text)) return fail(PF_ERR_ARG, "pf_assocfilter_scan: null argument");
    HIPCHK(hipSetDevice(f->feed.device));
    *out_bytes = 0; f->pack.out.reset();
    PFCHK(f->feed.plain(text, nbytes, consumed));
    PFCHK(af_scan_device(f, *consumed, 0));
    *out_bytes = f->pack.out.bytes;
    return PF_OK;
}

int pf_assocfilter_members_begin(pf_assocfilter* f, int header) { return feed_members_begin(f, "pf_assocfilter_members_begin", header); }
int pf_assocfilter_set_large_members(pf_assocfilter* f, int on, uint32_t piece_bytes) { return feed_set_large(f, "pf_assocfilter_set_large_members", on, piece_bytes); }
int pf_assocfilter_large_stats(pf_assocfilter* f, uint64_t* pieces, float* ms) { return feed_large_stats(f, "pf_assocfilter_large_stats", pieces, ms); }

int pf_assocfilter_members_header(pf_assocfilter* f, const char** line, uint64_t* nbytes) {
    return feed_members_header(f, "pf_assocfilter_members_header", line, nbytes);
}

int pf_assocfilter_scan_members(pf_assocfilter* f, const char* members, uint64_t nbytes, int last, uint64_t* out_bytes,
                                uint64_t* consumed, int* taken) {
    if (!f || !out_bytes || !consumed || !taken || (nbytes && !members)) return fail(PF_ERR_ARG, "pf_assocfilter_scan_members: null argument");
    HIPCHK(hipSetDevice(f->feed.device));
    *out_bytes = 0; f->pack.out.reset();
    PFCHK(f->feed.members(members, nbytes, last, consumed, taken, [f](uint64_t n, uint64_t skip) { return af_scan_device(f, n, skip); }));
    *out_bytes = f->pack.out.bytes;
    return PF_OK;
}

int pf_assocfilter_next_lines(pf_assocfilter* f, const char** piece, uint64_t* nbytes) {
    if (!f || !piece || !nbytes) return fail(PF_ERR_ARG, "pf_assocfilter_next_lines: null argument");
    HIPCHK(hipSetDevice(f->feed.device));
    return f->pack.out.next(f->feed.ts.stream, piece, nbytes);
}

int pf_assocfilter_columns(pf_assocfilter* f, const uint32_t** class_bits, uint32_t* n_fields, uint32_t* row_flags, uint64_t counters[2]) {
    if (!f || !class_bits || !n_fields || !row_flags || !counters) return fail(PF_ERR_ARG, "pf_assocfilter_columns: null argument");
    HIPCHK(hipSetDevice(f->feed.device));
    uint64_t misc[2] = {0, 0};
    HIPCHK(hipMemcpy(f->cols.data(), f->d_cols.p, f->cols.size() * 4, hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(misc, f->d_misc.p, sizeof misc, hipMemcpyDeviceToHost));
    *class_bits = f->cols.data(); *n_fields = f->n_fields; *row_flags = (uint32_t)(misc[1] & 0xFFFFFFFFu);
    counters[0] = misc[0]; counters[1] = f->kept;
    return PF_OK;
}

int pf_assocfilter_stats(pf_assocfilter* f, uint64_t stats[4], float ms[2]) {
    if (!f) return fail(PF_ERR_ARG, "pf_assocfilter_stats: null argument");
    if (stats) { stats[0] = f->bytes_scanned; stats[1] = f->feed.gz_members; stats[2] = f->feed.gz_text_bytes; stats[3] = f->feed.dec.device_bytes() + f->feed.lg.device_bytes(); }
    if (ms) { ms[0] = f->device_ms; ms[1] = f->feed.gz_ms; }
    return PF_OK;
}

}  // extern "C"

#ifdef PF_WEAK_HASH
extern "C" {
// weak-hash test build only (not part of the ABI): this file's share of pf_debug_set_hash_mask / pf_debug_weakhash_counts
int pf_rowfilter_weakhash_mask(uint64_t mask) {
    rf_wh_mask_host = mask;
    const unsigned long long m = mask;
    return hipMemcpyToSymbol(HIP_SYMBOL(rf_wh_mask), &m, sizeof m) == hipSuccess ? PF_OK : PF_ERR_HIP;
}
int pf_rowfilter_weakhash_counts(uint64_t* rowfilter_rejects, uint64_t* strain_rejects, int reset) {
    unsigned long long d = 0;
    if (hipMemcpyFromSymbol(&d, HIP_SYMBOL(rf_wh_strain_rejects), sizeof d) != hipSuccess) return PF_ERR_HIP;
    *rowfilter_rejects = rf_wh_rowfilter_rejects; *strain_rejects = d;
    if (reset) {
        rf_wh_rowfilter_rejects = 0; d = 0;
        if (hipMemcpyToSymbol(HIP_SYMBOL(rf_wh_strain_rejects), &d, sizeof d) != hipSuccess) return PF_ERR_HIP;
    }
    return PF_OK;
}
}  // extern "C"
#endif
