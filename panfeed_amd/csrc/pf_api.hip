// pf_api.hip -- C ABI (include/panfeed_hip.h) over the kernels in pf_kernels.h.
//
// Host orchestration of one batch (pf_submit):
//   dedup (identical sequences) -> per-cluster counts back to the host -> unit classes (identical units) ->
//   work items (cluster x key partition, plus prebuilt items for slow-path rows) -> sub-batches of <= max_items
//   items, each: scan -> fused finish, or rows -> base -> emit -> pattern rows; clusters whose LDS table overflowed are
//   re-run with the partitions the failed scan asked for; MD5 of new patterns last.  A batch of >= 8 192 clusters goes
//   through in two parts so that the host builds a part's items while the GPU is on the other.
// Everything is stream-ordered on one HIP stream; the host syncs are the dedup results per part, the overflow / cursor /
// pattern-counter read-back of the last pass and the end of the batch.
#include "pf_host.h"
#include "pf_kernels.h"
#include "../../include/panfeed_hip.h"
#include "pf_ingest.h"
#include "pf_buf.h"
#include "pf_deflate.h"

#include <sys/stat.h>
#include <condition_variable>
#include <mutex>
#include <algorithm>
#include <array>
#include <cmath>
#include <chrono>
#include <cstdio>
#include <cstring>
#include <memory>
#include <new>
#include <numeric>
#include <thread>
#include <string>
#include <unordered_map>
#include <unordered_set>
#include <atomic>
#include <vector>

namespace {

thread_local std::string g_err;

struct Arena {
    DevBuf key, pid, first;
    uint64_t cap = 0;        // entries
    uint64_t base = 0;       // global index of entry 0
    uint64_t used = 0;
};

// what a timed stretch of the stream counts towards (pf_timing); the extra-row fill counts as emit
enum class TimeCat { scan, rows, emit, dedup, pattern_rows, md5, finish };

struct EvPair { HipEvent a, b; TimeCat cat; };

// What this context has seen of its clusters of many distinct sequences: g = new k-mers per further sequence against
// L = windows of one sequence, as running sums for the line g = a + b L (related alleles: a few tens whatever L is;
// SURVEY 8d's: flanks + a share of L) -- see the key-partition estimate (first_nparts)
struct PartModel {
    double n = 0, x = 0, y = 0, xx = 0, xy = 0, yy = 0;
    struct Fit { double a = 0.0, b = 0.0, half_sd = 0.0; bool ready = false; };
    void add(double L, double g) { n += 1; x += L; y += g; xx += L * L; xy += L * g; yy += g * g; }
    void halve() { n *= 0.5; x *= 0.5; y *= 0.5; xx *= 0.5; xy *= 0.5; yy *= 0.5; }
    Fit fit() const {
        Fit f{0.0, 0.0, 0.0, n >= 16};
        if (!f.ready) return f;
        const double den = n * xx - x * x;
        f.a = y / n;
        if (den > 1e-6 * n * xx) { f.b = (n * xy - x * y) / den; f.a = (y - f.b * x) / n; }
        const double ss = std::max(0.0, yy - f.a * y - f.b * xy);     // residual sum of squares
        // (half a residual standard deviation on top: with `room` at 0.9 of the table's limit that left no
        // cluster of the headline workload, with or without 'N's, to overflow; 0 left 6, 1 to 3 standard
        // deviations cost 0.5 % to 5 % in surplus partitions -- profiles/r02/partition_margin_experiment.txt)
        f.half_sd = 0.5 * std::sqrt(ss / std::max(1.0, n - 2.0));
        return f;
    }
};

// The owning groups of the submit path's device buffers.  Each states its members once besides their declaration (a table
// or a list), sizes and releases them from that, and hands out the kernels' argument groups (pf_kernels.h) that point into
// them.  A pf:: group is built at the launch that uses it and never kept across an ensure, which may move a buffer.
// The scratch slices: what a work item (cluster x key partition) keeps while its sub-batch is in flight.
struct Scratch {
    DevBuf tab_key, tab_ord, chunkbits, chunkmask, slot_hash, sorted_pair, kept_prefix, bm4, bm2, mrows, slot_out, cmask_lo, cmask_hi;
    struct Dims { uint64_t NS, KW, W; };  // table slots of a slice, key words, presence words: the context's
    struct Slice { DevBuf Scratch::*buf; uint64_t per_slot, per_item; };   // bytes per table slot, and beside them per item
    static std::array<Slice, 13> slices(uint64_t KW, uint64_t W) {
        return {{{&Scratch::tab_key, 8 * KW, 0}, {&Scratch::tab_ord, 4, 0}, {&Scratch::chunkbits, 4 * W, 0}, {&Scratch::chunkmask, 0, 8 * 4},
                 {&Scratch::slot_hash, 16, 0}, {&Scratch::sorted_pair, 8, 0}, {&Scratch::kept_prefix, 4, 4},
                 {&Scratch::bm4, 0, pf::DENSE_WORDS_BIG * 16}, {&Scratch::bm2, 0, pf::DENSE_WORDS_BIG * 8}, {&Scratch::mrows, 0, pf::DEDUP_MROWS * 4},
                 {&Scratch::slot_out, 4, 0}, {&Scratch::cmask_lo, 4, 0}, {&Scratch::cmask_hi, 4, 0}}};
    }
    // what max_items is sized by (28 bytes of margin: with chunkmask's 32 and kept_prefix's 4 the 64 it always had)
    static uint64_t bytes_per_item(Dims d) {
        uint64_t n = 28;
        for (const Slice& s : slices(d.KW, d.W)) n += d.NS * s.per_slot + s.per_item;
        return n;
    }
    int ensure(uint32_t items, Dims d) {  // (DevBuf::ensure: buffers that are large enough stay)
        for (const Slice& s : slices(d.KW, d.W)) PFCHK((this->*s.buf).ensure(items * (d.NS * s.per_slot + s.per_item)));
        return PF_OK;
    }
    void release() { for (const Slice& s : slices(0, 0)) (this->*s.buf).release(); }     // (which buffers, whatever their size)
    pf::SlotDump slot_dump(uint32_t* item_count) const {       // (the key counts go beside the pass's items)
        return pf::SlotDump{cmask_lo.as<uint32_t>(), cmask_hi.as<uint32_t>(), tab_key.as<uint64_t>(), tab_ord.as<uint32_t>(),
                            chunkbits.as<uint32_t>(), chunkmask.as<uint32_t>(), item_count};
    }
    pf::RowScratch row_scratch(uint32_t* item_unique, uint32_t* item_kept) const {
        return pf::RowScratch{slot_hash.as<uint4>(), sorted_pair.as<uint64_t>(), kept_prefix.as<uint32_t>(), bm4.as<uint4>(),
                              bm2.as<uint2>(), mrows.as<uint32_t>(), slot_out.as<uint32_t>(), item_unique, item_kept};
    }
};
// A host-planned pass: its work items by column, its work lists and the lists of its sub-batches as the host writes them
// (capacity persists between calls: no allocation / page faults in steady state), each with its device view into the
// staging block that one copy fills (staged_upload).
struct Staged { std::vector<uint32_t> h; DevBuf d; };
struct HostPass {
    // compact = fused at all, binned = its cluster's windows are binned
    enum Col { it_cluster, it_part, it_nparts, it_nslots, it_slice, it_sib0, it_nsib, it_extra_first, it_is_extra, it_compact, it_binned, N_COLS };
    enum List { work_scan, work_extra, work_fin, work_fin2, work_fin3, work_fin5, work_rows, N_LISTS };   // of the sub-batches, concatenated
    Staged col[N_COLS], list[N_LISTS];
    Staged sub_cluster, sub_item0, sub_nitems;   // the general path's clusters, per sub-batch: cluster, first item, items
    Staged bin_block;                    // the binned clusters: cluster | first item | partitions | first queue entry
    std::vector<uint32_t> bin_cluster, bin_item0, bin_nparts, bin_base;   // ... its four stretches while they are built
    std::vector<uint8_t> fused;          // per item: 0 general path; 1 / 2 / 5 one item, fused small / large / huge class;
                                         // 3 the first of several partitions (fused large class), 4 the others
    DevBuf it_count, it_unique, it_kept; // [item] what the kernels count: keys in the table, k-mers, kept ones
    size_t n_items() const { return fused.size(); }
    void begin(size_t room) {            // room for so many items: push writes the columns by index, end cuts them to size
        for (Staged& s : col) s.h.resize(room, 0);
        for (Staged* s : {&sub_cluster, &sub_item0, &sub_nitems, &bin_block}) s->h.clear();
        for (auto* v : {&bin_cluster, &bin_item0, &bin_nparts, &bin_base}) v->clear();
        fused.clear(); fused.reserve(room);
    }
    void push(uint32_t cluster, uint32_t part, uint32_t nparts, uint32_t nslots, uint32_t slice, uint32_t sib0, uint32_t nsib,
              uint32_t extra_first, uint32_t is_extra, uint8_t fuse, uint32_t binned) {
        const uint32_t v[N_COLS] = {cluster, part, nparts, nslots, slice, sib0, nsib, extra_first, is_extra, fuse ? 1u : 0u, binned};
        for (int k = 0; k < N_COLS; k++) col[k].h[fused.size()] = v[k];
        fused.push_back(fuse);
    }
    void end() { for (Staged& s : col) s.h.resize(fused.size()); }
    std::vector<Staged*> staged() {       // in the order they lie in the staging block
        std::vector<Staged*> v = {&bin_block};
        for (Staged& s : col) v.push_back(&s);
        v.insert(v.end(), {&sub_cluster, &sub_item0, &sub_nitems});
        for (Staged& s : list) v.push_back(&s);
        return v;
    }
    pf::Items items() const {
        auto p = [&](Col k) { return col[k].d.as<uint32_t>(); };
        return pf::Items{p(it_cluster), p(it_part), p(it_nparts), p(it_nslots), p(it_slice), p(it_compact), p(it_binned),
                         p(it_is_extra), p(it_extra_first), p(it_sib0), p(it_nsib)};
    }
};
// Per batch: the scan view cluster_dedup_kernel builds and the per-cluster outputs.
struct BatchBufs {
    DevBuf cl_overflow, cl_kmer_off, cl_kmer_cnt, cl_unique, cl_pattern, cl_first, cl_rec, view_off, v_nseg, v_nstr, v_mode, v_dense;   // [C]
    DevBuf v_word_off, v_len, v_sample, v_ord, v_bits, seg_distinct, extra_dense;       // [NSEG]; the last [n_extra]
    DevBuf cursor, extra_off;            // sized apart: 64 bytes at pf_create; [C + 1] (+ 1) where the CSR is made
    int ensure(uint32_t C, uint32_t NSEG, uint32_t n_extra) {
        const size_t C1 = std::max(C, 1u), NSEG1 = std::max(NSEG, 1u), NEX1 = std::max(n_extra, 1u);
        const std::pair<DevBuf*, size_t> bufs[] = {
            {&cl_overflow, C1 * 4}, {&cl_kmer_off, C1 * 8}, {&cl_kmer_cnt, C1 * 4}, {&cl_unique, C1 * 4}, {&cl_pattern, C1 * 4},
            {&cl_first, C1 * 8}, {&cl_rec, C1 * sizeof(pf::ClusterRec)}, {&v_word_off, NSEG1 * 8}, {&v_len, NSEG1 * 4},
            {&v_sample, NSEG1 * 4}, {&v_ord, NSEG1 * 4}, {&v_bits, NSEG1 * 4}, {&view_off, C1 * 4}, {&seg_distinct, NSEG1 * 4},
            {&v_nseg, C1 * 4}, {&v_nstr, C1 * 4}, {&v_mode, C1 * 4}, {&v_dense, C1 * 4}, {&extra_dense, NEX1 * 4}};
        for (const auto& [buf, bytes] : bufs) PFCHK(buf->ensure(bytes));
        return PF_OK;
    }
    pf::View view() const {              // (the plain entries: a launch adds its unit pool's)
        pf::View v{};
        v.plain = pf::ViewSegs{v_word_off.as<uint64_t>(), v_len.as<uint32_t>(), v_sample.as<uint32_t>(), v_ord.as<uint32_t>(),
                               v_bits.as<uint32_t>()};
        v.view_off = view_off.as<uint32_t>(); v.v_nseg = v_nseg.as<uint32_t>();
        return v;
    }
    void dedup_outputs(pf::DedupParams& dp) const {    // what cluster_dedup_kernel writes, and the extra-row CSR it reads
        dp.view = view(); dp.seg_distinct = seg_distinct.as<uint32_t>(); dp.extra_off = extra_off.as<uint32_t>();
        dp.cl_overflow = cl_overflow.as<uint32_t>(); dp.cl_kmer_cnt = cl_kmer_cnt.as<uint32_t>(); dp.cl_unique = cl_unique.as<uint32_t>();
        dp.cl_pattern = cl_pattern.as<uint32_t>(); dp.v_nstr = v_nstr.as<uint32_t>(); dp.v_mode = v_mode.as<uint32_t>();
        dp.v_dense = v_dense.as<uint32_t>(); dp.extra_dense = extra_dense.as<uint32_t>();
    }
    pf::ViewFacts view_facts(const uint32_t* extra_bits) const {      // (the slow-path rows themselves are the caller's)
        return pf::ViewFacts{v_nstr.as<uint32_t>(), v_mode.as<uint32_t>(), v_dense.as<uint32_t>(), cl_overflow.as<uint32_t>(),
                             extra_off.as<uint32_t>(), extra_dense.as<uint32_t>(), extra_bits};
    }
    pf::Outputs outputs(const Arena& ar) const {   // (of the arena of the pass being launched)
        return pf::Outputs{ar.key.as<uint64_t>(), ar.pid.as<uint32_t>(), ar.first.as<uint64_t>(), ar.base, ar.cap,
                           cl_kmer_off.as<uint64_t>(), cl_kmer_cnt.as<uint32_t>(), cl_unique.as<uint32_t>(),
                           cl_pattern.as<uint32_t>(), cl_first.as<uint64_t>(), cursor.as<uint64_t>()};
    }
};
// The run-global pattern table (`cap` slots, a power of two) and the pool arrays indexed by pattern id (cap / 2 ids).
struct PatternBufs {
    DevBuf lo, val, first, bits, nan, n, md5, b64;   // (nan: only with consider_missing; b64: once a device renderer asked)
    uint64_t cap = 0; uint32_t pool = 0;
    pf::PatternPool pattern_pool() const { return pf::PatternPool{bits.as<uint32_t>(), nan.as<uint32_t>(), n.as<uint32_t>()}; }
};
// The caller's batch on the device (when it passes host pointers), and the per-batch gather lists
struct CallerBufs {
    DevBuf b_packed, b_seg_word_off, b_seg_len, b_seg_sample, b_seg_ord, b_cl_seg_off, b_cl_nstr, b_cl_npres, b_cl_presab,
        b_cl_ordinal, b_extra_ord, b_extra_bits, b_seg_strand_off, b_literal, g_src_off, g_src_start, g_src_flags;
};
// host scratch of pf_submit besides the pass's (HostPass), kept between calls like it
struct SubmitScratch {
    // a part's clusters for the wide dedup class; key counts read back for the key-partition estimate (host items, plan_kernel's)
    std::vector<uint32_t> wide, count, plan;
};

// kmers.tsv of target strains.  What the host renderer's measure pass leaves for its write pass, per sequence:
struct KtHostText {
    std::vector<uint8_t> rcflags;        // canonical mode, a byte per window: 0 forward, 1 the reverse complement is the
                                         // canonical one, 2 unknown
    std::vector<uint64_t> fl_off, size;  // the sequence's first flag; the bytes of its rows
    uint64_t bytes = 0;                  // of all rows
};
// The device text's plan (kt_plan): where every tile and every host-rendered sequence starts, and the ranges
struct KtPlan {
    struct Range { uint32_t t0, t1, h0, h1; uint64_t base, bytes; };   // tiles [t0, t1), host sequences [h0, h1)
    std::vector<uint64_t> toff, hoff;
    std::vector<uint64_t> seq_end;       // per sequence given: the offset just behind its rows (no window: the end before)
    std::vector<Range> ranges;
    uint64_t total = 0, cap = 0, max_unit = 0, max_range = 0, peak = 0;   // peak: of two neighbouring ranges
};

// The text path's state.  The render of kmers_to_hashes / hashes_to_patterns on the device (beside pats.b64): the text
// and its per-row tables; the pinned host copies of the rendered text, used alternately so that a writer thread may
// still be on the previous batch's; pf_render_pattern_rows' id list, row lengths and row offsets.
struct RenderText {
    DevBuf dev, meta, rp_order, rp_rlen, rp_rowoff;
    PinBuf pins[2];
    int slot = 0;
    uint32_t b64_done = 0;               // patterns whose base64 is in pats.b64
    int next_pin(size_t bytes, char** pin) {     // the other pinned block, of at least `bytes`
        PFCHK(pins[slot ^= 1].ensure(bytes));
        *pin = pins[slot].as<char>();
        return PF_OK;
    }
};
// A device text handed out in blocks (pf_kmers_tsv_stream_*, pf_pattern_rows_stream_*): the only owner of what a text in
// flight needs.  Range r is written into text[r & 1] on `stream` while the range before it leaves through the pinned
// blocks on `side`: as it is, or under device gzip as its members from GzMode::block_members.  One text is open at a
// time, and `kind` says whose: its producer writes the ranges and keeps only what its text needs beyond that.
struct TextStream {
    enum Kind { NONE, KMERS_TSV, PATTERN_ROWS };
    struct Range { uint64_t base, bytes; };
    struct Producer {
        Kind kind;
        int (*write)(pf_ctx*, uint32_t r, char* buf, int b);   // range r into buf (text[b]), queued on `stream`
        void (*drop)(pf_ctx*);                                 // the stream has ended: its host state goes
    };
    Kind kind = NONE;
    Producer by{};
    DevBuf text[2];
    PinBuf pins[2];
    uint64_t kept = 0;                     // bytes of text[0] that pf_render_kmers_tsv_device left for pf_device_text_chunk
    // the one block on its way, on `side`: n bytes from `off` of the text into pins[slot] -- or, a stream's block under
    // device gzip, their members into GzMode::block_members[slot], the members' size into the slot's pinned cursor word
    struct { bool valid = false; int slot = 0; uint64_t off = 0, n = 0; } flight;
    std::vector<Range> ranges;
    uint32_t cur = 0;                      // the block to queue next: range cur, bytes from cur_off
    uint64_t cur_off = 0, pin_bytes = 0;
    HipEvent ev_prod[2];                   // on `stream`: the range in buffer b is written
    HipEvent ev_copied[2];                 // on `side`: the range in buffer b has left the device
    // device gzip with cuts (pf_kmers_tsv_stream_cuts): the text offsets inside the text behind which a member must
    // end, ascending and distinct; per slot the block encoded into it -- its text, its cuts [lo, hi) and their
    // places in its text -- and, once handed out, behind which member byte each of them lies
    std::vector<uint64_t> cuts;
    struct Block { uint64_t off = 0, n = 0; size_t lo = 0, hi = 0; std::vector<uint64_t> seg_end, member_end; } blk[2];
    int handed = -1;                       // the slot of the block handed out last
};
// kmers.tsv written on the device: descriptors and tiles, and what the stream's kmers.tsv producer keeps while its text
// is open.  pf_kmers_tsv_stream_begin / _next hand the ranges out in order; pf_render_kmers_tsv_device writes the whole
// text as one range into the stream's text[0], where `kept` bytes of it stay for pf_device_text_chunk.
struct KtHostFilter;
struct TargetText {
    DevBuf seqs, tiles, prefix, tbytes, toff;
    // pf_kmers_tsv_seq_ends: the offset behind every sequence's rows in the last text planned (kt_plan), kept beyond the
    // stream's end; gone with the next pf_submit
    std::vector<uint64_t> seq_end;
    bool have_seq_end = false;
    std::vector<pf_target_seq> hseqs;      // the host-rendered sequences (the caller's strings, until the stream ends)
    KtHostText host;                       // their one measurement
    KtPlan plan;
    pf::KtParams kp{};
    bool filter = false;                   // the text is the filtered one: kf beside kp, hfilter for the host's share
    pf::KtFilter kf{};
    std::unique_ptr<KtHostFilter> hfilter;
    std::unique_ptr<char[]> htext[2];      // the host's share of the range being written into each buffer
};
// gzip on the device (pf_set_device_gzip): the mode, the encoder, the members of a render and of the stream's two blocks
// in flight (block j + 1 is encoded while block j is written out by the caller), the text sizes behind the members
struct GzMode {
    bool on = false;
    uint32_t flags = 0;
    PfGzEncoder enc;
    DevBuf render_members, block_members[2];
    uint64_t block_bound = 0;                 // bytes of each of block_members
    HipEvent ev_copy;                         // on `side`: a block's members have arrived in pinned memory
    uint64_t raw[3] = {0, 0, 0};              // text bytes of the last render's two texts, of the stream's blocks so far
    float encode_ms = 0.0f;                   // the last pf_gzip_device's encode, scan and gather launches (hipEvent)
    PfGzDecoder dec;
    float decode_ms = 0.0f;                   // the last pf_gunzip_device's inflate launches (hipEvent)
    PfGzLarge large;                          // pf_gunzip_device_large's passes
};
// hashes_to_patterns rows of a list of patterns (pf_pattern_rows_stream_begin / _next), the stream's other producer: the
// ids and their row lengths on the device, the text cut into slices at row boundaries.  A slice is a range of the stream
// and one block of it.
struct PatternRows {
    DevBuf order, rlen, rowoff[2];            // the ids, their row lengths; a slice's row offsets (from the slice's start)
    PinBuf pin_rowoff[2];
    std::vector<uint64_t> row_off;            // of the whole text, n + 1
    std::vector<uint64_t> cut;                // slice i holds rows [cut[i], cut[i + 1])
};
int gz_check_flags(uint32_t flags, const char* who) {
    if (flags & ~(PF_GZ_FIXED_ONLY | PF_GZ_DYNAMIC_ONLY | PF_GZ_LITERALS_ONLY | PF_GZ_BGZF | PF_GZ_DEEP)) return fail(PF_ERR_ARG, "%s: unknown flag", who);
    return PF_OK;
}

}  // namespace

namespace {
// Rows of passing patterns only (pf_set_passing_hashes).  The set: the caller's distinct digests and their table on the
// device.  Per batch: the clusters' names and the slow-path rows' text (pf_passing_batch_names), and what the text's
// opening (kt_filter_prepare) leaves -- the marks of the kept k-mers of the clusters that own a target sequence, the
// index of the passing ones, the row kernels' keep bits -- with the counts pf_passing_stats reports.
struct PassingRows {
    bool on = false;
    uint32_t bits = 64;                       // pf_debug_passing_hash_bits
    std::vector<uint8_t> digests;             // n x 16, distinct
    DevBuf set;                               // pf::PassSlot [set_mask + 1]
    uint64_t set_mask = 0;
    bool have_names = false;                  // since the last pf_submit
    std::unordered_map<std::string, uint32_t> name_idx;
    std::string extra;                        // klength bytes per slow-path row of the batch
    DevBuf ref, hsh, mark, counters, mark_cluster, mark_off, koff, arena_of, seq_cluster, keep_bits, tile_rows;
    uint64_t marked = 0, considered = 0, kept = 0;
    uint64_t index_slots = 0;                 // ref / hsh of the last filtered text (0: none since the set or the batch changed)
    float mark_ms = 0.0f;                     // the last text's mark and index kernel (hipEvent)
    HipEvent ev0, ev1;
    uint64_t device_bytes() const {
        uint64_t n = 0;
        for (const DevBuf* b : {&set, &ref, &hsh, &mark, &counters, &mark_cluster, &mark_off, &koff, &arena_of, &seq_cluster, &keep_bits, &tile_rows}) n += b->cap;
        return n;
    }
};
// the host's statement of the filter for the sequences it renders: per such sequence the text of its cluster's passing
// k-mers (built from the marks and keys of those clusters only), and the rows it looked at and kept
struct KtHostFilter {
    std::vector<std::unordered_set<std::string>> sets;     // per cluster that owns a host-rendered sequence
    std::vector<uint32_t> seq_set;                         // per host-rendered sequence: its cluster's set
    std::atomic<uint64_t> considered{0}, kept{0};
};
}  // namespace

struct pf_ctx {
    int device = 0;
    HipStream stream;
    HipStream side;                        // the fused finish kernels of a SMALL launch run here, beside the general path's kernels
    HipEvent ev_fork, ev_join;
    pf_opts o{};
    int KW = 1;
    uint32_t NS = 0, W = 0, max_items = 0;
    std::vector<uint32_t> maf_lo, maf_hi;
    DevBuf d_maf_lo, d_maf_hi;
    PatternBufs pats;              // pattern table + pool, its counters, and the kernels' view of both (sync_pattern_table)
    DevBuf pt_counters;
    pf::PatternTable pt{};
    PartModel part_model;
    uint64_t n_submits = 0;
    uint32_t n_patterns = 0;       // patterns allocated after the last submit
    uint32_t pid0 = 0;             // first pattern id of the last submit
    Scratch scratch;                       // the scratch slices of max_items work items
    Scratch::Dims dims() const { return {NS, (uint64_t)KW, W}; }
    CallerBufs caller;
    BatchBufs batch;
    HostPass pass;                            // the host-planned pass being built or in flight
    DevBuf strand_bits, scan_desc, md5_list, wide_list;
    // unit view (unit_class_kernel): one pool of view entries per part of a batch's first pass, and the list
    // {clusters, their places in the pool} that goes up with it
    struct UPool { DevBuf word_off, len, sample, ord, bits, list; PinBuf pin; };
    RenderText txt;                        // the text path: the render's state,
    TextStream ts;                         // the one text handed out in blocks, and its two producers:
    TargetText kt;                         // the target text's (kmers.tsv)
    PatternRows pr;                        // and the pattern rows';
    GzMode gz;                             // the gzip mode
    PassingRows passing;                   // the filter of kmers.tsv rows (pf_set_passing_hashes)
    pf_batch last{};                      // the last pf_submit's batch arrays as device pointers (valid until the next submit)
    uint32_t last_nseg = 0;
    uint64_t last_words = 0;              // words of last.packed: the batch's, or the buffer pf_submit_gather filled
    DevBuf g_store;                       // genomes resident in HBM
    uint64_t g_words = 0;
    const pf_gather* pending_gather = nullptr;
    SubmitScratch hs;
    int n_cu = 256;
    DevBuf q_key, q_ord, q_bit, q_off;    // key-partition queues of binned clusters (bin_kernel)
    std::vector<std::unique_ptr<Arena>> arenas;
    uint32_t n_passes = 0;                 // arenas the last pf_submit used (arenas[] itself only ever grows)
    uint32_t n_grown = 0;                  // times the pattern table / pool were enlarged
    uint32_t n_scratch_grown = 0;          // times the scratch slices were re-made for a cluster of more items than max_items
    uint64_t pt_slot_limit = 0;            // test hook (pf_debug_limit_pattern_slots): allocations above it fail as if out of memory
    uint32_t pregrow_failed_pool = 0;      // pool size at which growing ahead of need failed: not tried again at this size
    bool pt_stale = false;                 // a batch failed and its patterns could not be dropped (growth failed): reset first
    DevBuf mg_lo, mg_cnt;   // pf_merge_patterns scratch table ([cap][4] words) and its counter
    // the small per-pass arrays: one device block + its pinned host mirror, two of each because the two halves of a
    // batch's first pass are in flight together (stage_slot picks the pair)
    DevBuf stage_devs[2];
    PinBuf stage_pins[2];
    int stage_slot = 0;
    PinBuf pin_dedup;              // pinned host copies of the per-cluster arrays the dedup kernel leaves
    PinBuf pin_small;              // pinned scratch (uint64): cursor values going up [0..15], cursor read-backs of deferred
                                   // passes [16..47], the last pass's cursor triple [48..50] and pattern counters [52..53]
    PinBuf pin_ovf;                // pinned: the per-cluster overflow words of the last pass (a pageable destination makes
                                   // hipMemcpyAsync a staged, blocking copy)
    static constexpr int MAX_PARTS = 8;
    UPool upool[2 * MAX_PARTS];            // [2 h]: the device-planned clusters of part h, [2 h + 1]: the host-planned rest
    HipEvent ev_part[MAX_PARTS];           // a part's dedup results have arrived in pinned memory
    // plan_kernel's output per part: item arrays, work lists, unit-view list (one device block), its 40-byte summary in
    // pinned memory; and the constant item arrays (zeros | ones | 0, 1, 2, ...) every device-planned pass shares
    struct DPlan { DevBuf block, it_count, out; PinBuf pin_out; uint32_t n = 0; };
    DPlan dplan[MAX_PARTS];
    DevBuf dp_const, plan_room, plan_arena;
    uint32_t dp_const_n = 0;
    HipEvent ev_stage[2];                  // a staging slot's upload has left the pinned block

    // last batch bookkeeping
    bool have_batch = false;
    bool h_strand_fresh = false;        // h_strand holds the strand bits of the last submit
    uint32_t n_clusters = 0;
    uint64_t n_strand_words = 0;
    std::vector<uint32_t> cluster_arena;   // arena index per cluster
    struct Route { uint32_t nparts, nslots, attempts; uint8_t cls, first, mode; };
    std::vector<Route> routes;             // per cluster, for pf_debug_cluster_routes (host bookkeeping only)
    pf_result counters{};
    pf_timing timing{};
    std::vector<EvPair> events;
    std::vector<HipEvent> ev_pool;
    HipEvent ev_t0, ev_t1;
    // host result storage
    std::vector<uint64_t> h_kmer_off, h_kmer_key, h_first_seen, h_strand;
    std::vector<uint32_t> h_kmer_cnt, h_cl_pattern, h_cl_unique, h_kmer_pid, h_new_pid, h_pat_bits, h_pat_nan, h_pat_n;
    std::vector<uint8_t> h_pat_md5;
    std::vector<char> h_b64;       // 24 chars per pattern
};

namespace {

// the end of the open stream (its last block handed out, a kmers.tsv text begun, the next pf_submit, pf_set_device_gzip,
// pf_destroy): nothing of it is in flight afterwards, its producer's host state is freed.  `only`: a stream of that kind
void ts_end(pf_ctx* c, TextStream::Kind only = TextStream::NONE) {
    TextStream& S = c->ts;
    if (S.kind == TextStream::NONE || (only != TextStream::NONE && S.kind != only)) return;
    (void)hipStreamSynchronize(c->side);
    (void)hipStreamSynchronize(c->stream);
    S.by.drop(c);
    S.kind = TextStream::NONE; S.flight.valid = false;
    S.ranges.clear(); S.cuts.clear(); S.handed = -1;
}
// a stream being opened ends with the step that fails
struct EndUnlessOpen { pf_ctx* c; bool ok = false; ~EndUnlessOpen() { if (!ok) ts_end(c); } };

int get_event(pf_ctx* c, HipEvent* ev) {
    if (!c->ev_pool.empty()) { *ev = std::move(c->ev_pool.back()); c->ev_pool.pop_back(); return PF_OK; }
    return ev->ensure();
}
// a timed stretch of one category on `s` (the context's stream unless the launches go to the side stream); the pairs are
// read after the batch's last synchronisation, when both streams have drained
int mark_begin(pf_ctx* c, TimeCat cat, hipStream_t s = nullptr) {
    EvPair e; e.cat = cat;
    PFCHK(get_event(c, &e.a));
    PFCHK(get_event(c, &e.b));
    HIPCHK(hipEventRecord(e.a, s ? s : c->stream));
    c->events.push_back(std::move(e));
    return PF_OK;
}
int mark_end(pf_ctx* c, hipStream_t s = nullptr) {
    HIPCHK(hipEventRecord(c->events.back().b, s ? s : c->stream));
    return PF_OK;
}

template <class T>
int upload(pf_ctx* c, DevBuf& b, const T* src, size_t n, const T** out) {
    PFCHK(b.ensure(std::max<size_t>(n, 1) * sizeof(T)));
    if (n) HIPCHK(hipMemcpyAsync(b.p, src, n * sizeof(T), hipMemcpyHostToDevice, c->stream));
    *out = b.as<T>();
    return PF_OK;
}
template <class T>
int upload_vec(pf_ctx* c, DevBuf& b, const std::vector<T>& v) {
    const T* dummy;
    return upload(c, b, v.data(), v.size(), &dummy);
}

int fill_u64(pf_ctx* c, void* p, uint64_t v, uint64_t n) {
    if (!n) return PF_OK;
    uint32_t blocks = (uint32_t)std::min<uint64_t>((n + 255) / 256, 4096);
    hipLaunchKernelGGL(pf::fill_u64_kernel, dim3(blocks), dim3(256), 0, c->stream, (uint64_t*)p, v, n);
    HIPCHK(hipGetLastError());
    return PF_OK;
}

int reset_patterns(pf_ctx* c) {
    PFCHK(fill_u64(c, c->pats.lo.p, pf::EMPTY64, c->pats.cap));
    PFCHK(fill_u64(c, c->pats.val.p, pf::EMPTY64, c->pats.cap));
    PFCHK(fill_u64(c, c->pats.first.p, pf::EMPTY64, c->pats.pool));
    HIPCHK(hipMemsetAsync(c->pt_counters.p, 0, 16, c->stream));
    c->n_patterns = 0;
    c->pid0 = 0;
    c->txt.b64_done = 0;
    c->pt_stale = false;
    c->h_pat_bits.clear(); c->h_pat_nan.clear(); c->h_pat_n.clear(); c->h_pat_md5.clear(); c->h_first_seen.clear();
    c->h_b64.clear();
    return PF_OK;
}

// Upload many small uint32 arrays with ONE pinned-host -> device copy; each DevBuf becomes a view into stage_dev.
int staged_upload(pf_ctx* c, const std::vector<Staged*>& arrs) {
    size_t total = 0;
    std::vector<size_t> off(arrs.size());
    for (size_t i = 0; i < arrs.size(); i++) {
        off[i] = total;
        total += (std::max<size_t>(arrs[i]->h.size(), 1) * 4 + 255) & ~(size_t)255;
    }
    for (Staged* a : arrs) if (!a->d.view) a->d.release();
    DevBuf& stage_dev = c->stage_devs[c->stage_slot];
    PinBuf& stage_pin = c->stage_pins[c->stage_slot];
    // several passes are queued without a host sync in between: the copy that last used this slot (two passes ago) has
    // to have left the pinned block before it is written again
    HIPCHK(hipEventSynchronize(c->ev_stage[c->stage_slot]));
    PFCHK(stage_dev.ensure(total));
    PFCHK(stage_pin.ensure(total));
    for (size_t i = 0; i < arrs.size(); i++) {
        const auto& v = arrs[i]->h;
        if (!v.empty()) memcpy(stage_pin.as<char>() + off[i], v.data(), v.size() * 4);
        arrs[i]->d.p = (char*)stage_dev.p + off[i];
        arrs[i]->d.cap = 0;
        arrs[i]->d.view = true;
    }
    HIPCHK(hipMemcpyAsync(stage_dev.p, stage_pin.p, total, hipMemcpyHostToDevice, c->stream));
    HIPCHK(hipEventRecord(c->ev_stage[c->stage_slot], c->stream));
    return PF_OK;
}

// a table of `slots` (a power of two) and its pool
int alloc_pattern_bufs(pf_ctx* c, uint64_t slots, bool with_b64, PatternBufs& pb) {
    if (c->pt_slot_limit && slots > c->pt_slot_limit)
        return fail(PF_ERR_OOM, "pattern table of %llu slots refused (limit %llu set by pf_debug_limit_pattern_slots)",
                    (unsigned long long)slots, (unsigned long long)c->pt_slot_limit);
    pb.cap = slots;
    pb.pool = (uint32_t)std::min<uint64_t>(slots / 2, 0x7FFFFFF0ull);
    const size_t W = c->W, pool = pb.pool;
    PFCHK(pb.lo.ensure(slots * 8));
    PFCHK(pb.val.ensure(slots * 8));
    PFCHK(pb.first.ensure(pool * 8));
    PFCHK(pb.bits.ensure(pool * W * 4));
    PFCHK(pb.n.ensure(pool * 4));
    PFCHK(pb.md5.ensure(pool * 16));
    if (c->o.consider_missing) PFCHK(pb.nan.ensure(pool * W * 4));
    if (with_b64) PFCHK(pb.b64.ensure(pool * 24));
    return PF_OK;
}
// the kernels' view of the table, from its owner: after every change of c->pats
void sync_pattern_table(pf_ctx* c) {
    c->pt = pf::PatternTable{c->pats.lo.as<uint64_t>(), c->pats.val.as<uint64_t>(), c->pats.first.as<uint64_t>(),
                             c->pt_counters.as<uint32_t>(), c->pats.cap, c->pats.pool};
}

// The reference's `patterns` is an unbounded set (panfeed.py:146-150): when a batch runs out of pattern ids (or
// comes close), the table and the pool are re-made larger, the patterns of earlier batches re-inserted
// (pattern_rehash_kernel; whatever the failed batch added is dropped) and the batch is run again.  The new table is
// built beside the old one and takes its place only when every step has succeeded: on a failure (out of memory with
// both resident, a failed copy) the context keeps the table it had and the error is returned.
int grow_patterns(pf_ctx* c, uint64_t min_pool) {
    uint64_t slots = c->pt.cap * 2;
    while (slots / 2 < min_pool + min_pool / 4) slots <<= 1;
    if (slots / 2 > 0x7FFFFFF0ull) return fail(PF_ERR_CAPACITY, "more than 2^31 distinct patterns");
    const uint32_t keep = c->n_patterns;            // ids of the batches that completed
    const size_t W = c->W;
    PatternBufs nb;
    int rc = alloc_pattern_bufs(c, slots, c->pats.b64.p != nullptr, nb);
    auto copy = [&](DevBuf& dst, const DevBuf& src, size_t bytes) -> int {
        if (bytes && src.p) HIPCHK(hipMemcpyAsync(dst.p, src.p, bytes, hipMemcpyDeviceToDevice, c->stream));
        return PF_OK;
    };
    if (rc == PF_OK) rc = fill_u64(c, nb.lo.p, pf::EMPTY64, slots);
    if (rc == PF_OK) rc = fill_u64(c, nb.val.p, pf::EMPTY64, slots);
    if (rc == PF_OK) rc = fill_u64(c, nb.first.p, pf::EMPTY64, nb.pool);
    const PatternBufs& ob = c->pats;
    if (rc == PF_OK) rc = copy(nb.first, ob.first, (size_t)keep * 8);
    if (rc == PF_OK) rc = copy(nb.bits, ob.bits, (size_t)keep * W * 4);
    if (rc == PF_OK && c->o.consider_missing) rc = copy(nb.nan, ob.nan, (size_t)keep * W * 4);
    if (rc == PF_OK) rc = copy(nb.n, ob.n, (size_t)keep * 4);
    if (rc == PF_OK) rc = copy(nb.md5, ob.md5, (size_t)keep * 16);
    if (rc == PF_OK && nb.b64.p) rc = copy(nb.b64, ob.b64, (size_t)std::min(c->txt.b64_done, keep) * 24);
    if (rc == PF_OK) {
        pf::RehashParams rp{};
        rp.old_lo = ob.lo.as<uint64_t>(); rp.old_val = ob.val.as<uint64_t>(); rp.old_cap = ob.cap;
        rp.new_lo = nb.lo.as<uint64_t>(); rp.new_val = nb.val.as<uint64_t>(); rp.new_cap = slots; rp.keep_below = keep;
        const uint32_t blocks = (uint32_t)std::min<uint64_t>((c->pt.cap + 255) / 256, 8192);
        hipLaunchKernelGGL(pf::pattern_rehash_kernel, dim3(blocks), dim3(256), 0, c->stream, rp);
        if (hipGetLastError() != hipSuccess) rc = fail(PF_ERR_HIP, "pattern_rehash_kernel launch failed");
    }
    if (rc == PF_OK && hipStreamSynchronize(c->stream) != hipSuccess) rc = fail(PF_ERR_HIP, "growing the pattern table failed");
    const uint32_t cnt[4] = {keep, 0, 0, 0};
    if (rc != PF_OK) {
        (void)hipStreamSynchronize(c->stream);       // nothing queued above may still touch nb's buffers when they go
        // the failed batch's additions are still in the old table: forget them, as the successful path does
        (void)hipMemcpy(c->pt_counters.p, cnt, 16, hipMemcpyHostToDevice);
        return rc;
    }
    std::swap(c->pats, nb);                          // nb now holds the old buffers, and frees them
    sync_pattern_table(c);
    HIPCHK(hipMemcpy(c->pt_counters.p, cnt, 16, hipMemcpyHostToDevice));
    c->txt.b64_done = std::min(c->txt.b64_done, keep);
    c->n_grown++;
    return PF_OK;
}

// A cluster asks for more work items than a sub-batch holds (a very divergent or very wide cluster; an overflow retry
// multiplies its key partitions): the scratch is re-made for `need` items -- when that fits half of the device memory
// that is free once the old scratch is gone -- instead of failing the run.  Nothing may be in flight: the caller's
// earlier passes keep their results in the arenas, not in the scratch.
int grow_scratch(pf_ctx* c, uint32_t need) {
    HIPCHK(hipStreamSynchronize(c->stream));
    size_t free_b = 0, total_b = 0;
    HIPCHK(hipMemGetInfo(&free_b, &total_b));
    const uint64_t sb = Scratch::bytes_per_item(c->dims());
    const uint64_t have = (uint64_t)c->max_items * sb;
    uint64_t want = std::max<uint64_t>(need, std::min<uint64_t>(2ull * c->max_items, 65536));
    if (want * sb > (free_b + have) / 2) want = need;
    if (want * sb > (free_b + have) / 2)
        return fail(PF_ERR_CAPACITY, "a cluster needs %u work items (%.1f GB of scratch); %.1f GB of device memory are free",
                    need, (double)need * sb / 1e9, (double)(free_b + have) / 1e9);
    c->scratch.release();                         // (freed first: old and new need not fit side by side)
    const int rc = c->scratch.ensure((uint32_t)want, c->dims());
    if (rc != PF_OK) {                            // back to what it was; if even that fails the context is unusable
        c->scratch.release();
        if (c->scratch.ensure(c->max_items, c->dims()) != PF_OK) c->max_items = 0;
        return rc;
    }
    c->max_items = (uint32_t)want;
    c->n_scratch_grown++;
    return PF_OK;
}

template <int KW, bool CANON>
int scan_attr_t(pf_ctx* c) {
    // ~100-160 KB of dynamic LDS: the limit is raised once per context (= per device), at pf_create
    const uint32_t lds = c->NS * (8u * KW + 8u) + pf::MISC_WORDS * 4;
    HIPCHK(hipFuncSetAttribute(reinterpret_cast<const void*>(pf::kmer_scan_kernel<KW, CANON>),
                               hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    return PF_OK;
}
int scan_attr(pf_ctx* c) {
    switch (c->KW) {
        case 1: return c->o.canon ? scan_attr_t<1, true>(c) : scan_attr_t<1, false>(c);
        case 2: return c->o.canon ? scan_attr_t<2, true>(c) : scan_attr_t<2, false>(c);
        case 3: return c->o.canon ? scan_attr_t<3, true>(c) : scan_attr_t<3, false>(c);
        default: return c->o.canon ? scan_attr_t<4, true>(c) : scan_attr_t<4, false>(c);
    }
}

template <int KW, bool CANON>
int launch_scan_t(pf_ctx* c, const pf::ScanParams& sp, uint32_t n) {
    auto kern = pf::kmer_scan_kernel<KW, CANON>;
    const uint32_t lds = c->NS * (8u * KW + 8u) + pf::MISC_WORDS * 4;
    // descriptors first (one thread per work entry), then one persistent workgroup per CU
    PFCHK(c->scan_desc.ensure((size_t)n * sizeof(pf::ScanDesc)));
    pf::ScanParams q = sp;
    q.n_work = n;
    q.desc = c->scan_desc.as<pf::ScanDesc>();
    hipLaunchKernelGGL(pf::scan_desc_kernel, dim3((n + 255) / 256), dim3(256), 0, c->stream, q, c->scan_desc.as<pf::ScanDesc>());
    HIPCHK(hipGetLastError());
    const uint32_t grid = n < (uint32_t)c->n_cu ? n : (uint32_t)c->n_cu;
    hipLaunchKernelGGL(kern, dim3(grid), dim3(pf::SCAN_THREADS), lds, c->stream, q);
    HIPCHK(hipGetLastError());
    return PF_OK;
}
int launch_bin(pf_ctx* c, const pf::ScanParams& sp, uint32_t n) {
    const dim3 g(n), b(pf::BIN_THREADS);
    switch (c->KW) {
        case 1:
            if (c->o.canon) hipLaunchKernelGGL((pf::bin_kernel<1, true>), g, b, 0, c->stream, sp);
            else hipLaunchKernelGGL((pf::bin_kernel<1, false>), g, b, 0, c->stream, sp);
            break;
        case 2:
            if (c->o.canon) hipLaunchKernelGGL((pf::bin_kernel<2, true>), g, b, 0, c->stream, sp);
            else hipLaunchKernelGGL((pf::bin_kernel<2, false>), g, b, 0, c->stream, sp);
            break;
        default: return fail(PF_ERR_STATE, "bin_kernel: keys of more than two words are not binned");
    }
    HIPCHK(hipGetLastError());
    return PF_OK;
}
int launch_scan(pf_ctx* c, const pf::ScanParams& sp, uint32_t n) {
    switch (c->KW) {
        case 1: return c->o.canon ? launch_scan_t<1, true>(c, sp, n) : launch_scan_t<1, false>(c, sp, n);
        case 2: return c->o.canon ? launch_scan_t<2, true>(c, sp, n) : launch_scan_t<2, false>(c, sp, n);
        case 3: return c->o.canon ? launch_scan_t<3, true>(c, sp, n) : launch_scan_t<3, false>(c, sp, n);
        default: return c->o.canon ? launch_scan_t<4, true>(c, sp, n) : launch_scan_t<4, false>(c, sp, n);
    }
}

}  // namespace

namespace {
template <class F>
void parallel_for(uint64_t n, F f) {
    const unsigned nt = pf_host_threads(32u);
    if (n < 4096 || nt == 1) { f(0, n); return; }
    std::vector<std::thread> th;
    const uint64_t chunk = (n + nt - 1) / nt;
    for (unsigned t = 0; t < nt; t++) {
        const uint64_t a = t * chunk, b = std::min<uint64_t>(n, a + chunk);
        if (a < b) th.emplace_back([=] { f(a, b); });
    }
    for (auto& x : th) x.join();
}
void ensure_b64(pf_ctx* c) {
    // 24-char base64 of every pattern's digest (panfeed.py:176, 207), extended incrementally
    const size_t have = c->h_b64.size() / 24, want = c->h_pat_md5.size() / 16;
    c->h_b64.resize(want * 24);
    for (size_t p = have; p < want; p++) pf_b64_digest(c->h_pat_md5.data() + p * 16, c->h_b64.data() + p * 24);
}
}  // namespace

namespace {
inline char* put_i64(char* w, long long v) {
    char tmp[24];
    int n = 0;
    unsigned long long u = v < 0 ? 0ull - (unsigned long long)v : (unsigned long long)v;
    do { tmp[n++] = (char)('0' + u % 10); u /= 10; } while (u);
    if (v < 0) *w++ = '-';
    while (n) *w++ = tmp[--n];
    return w;
}
inline size_t len_i64(long long v) { char t[24]; return (size_t)(put_i64(t, v) - t); }

// the host renderer of kmers.tsv (pf_render_kmers_tsv).  Where the fields of a row go: counted (the measure pass), or
// written
struct RowCount {
    uint64_t n = 0;
    void text(const char*, size_t l) { n += l; }
    void ch(char) { n++; }
    void num(long long v) { n += len_i64(v); }
    void revcomp(const char*, uint32_t k) { n += k; }
};
struct RowWrite {
    char* w;
    void text(const char* p, size_t l) { memcpy(w, p, l); w += l; }
    void ch(char x) { *w++ = x; }
    void num(long long v) { w = put_i64(w, v); }
    void revcomp(const char* last, uint32_t k) { for (uint32_t q = 0; q < k; q++) w[q] = *(last - q); w += k; }   // complement letters, backwards
};

// Under the passing-rows filter: a row gathered until its line end, then handed on as one piece if its k-mer -- the k
// bytes before the line end -- is among the cluster's passing k-mers
template <class Inner>
struct RowFilter {
    Inner& in; const std::unordered_set<std::string>& set; uint32_t k;
    std::string row; uint64_t seen = 0, kept = 0;
    void text(const char* p, size_t l) { row.append(p, l); }
    void num(long long v) { char t[24]; row.append(t, (size_t)(put_i64(t, v) - t)); }
    void revcomp(const char* last, uint32_t n) { for (uint32_t q = 0; q < n; q++) row.push_back(*(last - q)); }
    void ch(char x) {
        row.push_back(x);
        if (x != '\n') return;
        seen++;
        if (row.size() > k && set.count(row.substr(row.size() - 1 - k, k))) { kept++; in.text(row.data(), row.size()); }
        row.clear();
    }
};

// The rows of target sequence s, in order, field by field into `out` (two rows per window in non-canonical mode).
// rcflag, canonical mode only: per window 0 forward, 1 the reverse complement is the canonical one, 2 unknown; a non-ACGT
// window takes strand column and letters from the caller's list instead.  False: a window had neither.
template <class Out>
bool kt_host_rows(const pf_target_seq& s, uint32_t k, bool canon, const uint8_t* rcflag, Out& out) {
    const long long nk = (long long)s.len - k + 1;
    if (nk <= 0) return true;                    // no window, no row (panfeed.py:59,64)
    const size_t lc = strlen(s.cluster), ls = strlen(s.strain), li = strlen(s.id), lh = strlen(s.chromosome);
    bool ok = true;
    uint32_t ai = 0;
    for (long long pos = 0; pos < nk; pos++) {
        long long ts, te;
        if (s.strand > 0) { ts = s.start + pos; te = s.start + pos + k; }       // panfeed.py:91-94
        else { te = s.end - pos; ts = s.end - pos - k; }                         // panfeed.py:96-99
        for (int rep = 0; rep < (canon ? 1 : 2); rep++) {
            out.text(s.cluster, lc); out.ch('\t');
            out.text(s.strain, ls); out.ch('\t');
            out.text(s.id, li); out.ch('\t');
            out.text(s.chromosome, lh); out.ch('\t');
            out.num(s.strand); out.ch('\t');
            out.num(ts); out.ch('\t');
            out.num(te); out.ch('\t');
            out.num(pos - s.offset); out.ch('\t');                               // panfeed.py:101
            out.num(pos + k - s.offset); out.ch('\t');                           // panfeed.py:102
            // strand column and letters: the window's own, or what the caller worked out for a non-ACGT window
            bool rc = rep == 1;
            const char* given = nullptr;
            if (canon) {
                while (ai < s.n_ambig && s.ambig_pos[ai] < (uint64_t)pos) ai++;
                if (ai < s.n_ambig && s.ambig_pos[ai] == (uint64_t)pos) { out.num(s.ambig_used[ai]); given = s.ambig_key[ai]; }
                else { if (rcflag[pos] > 1) ok = false; rc = rcflag[pos] == 1; out.num(rc ? -1 : 1); }
            } else {
                out.num(rc ? -(long long)s.strand : s.strand);                   // panfeed.py:106-107
            }
            out.ch('\t');
            if (given) out.text(given, k);
            else if (rc) out.revcomp(s.compsequence + pos + k - 1, k);
            else out.text(s.sequence + pos, k);
            out.ch('\n');
        }
    }
    return ok;
}
}  // namespace

extern "C" {

const char* pf_last_error(void) { return g_err.c_str(); }
void pf_set_error_(const char* msg) { g_err = msg; }   /* for the other translation units of the library */
#ifdef PF_WEAK_HASH
const char* pf_version(void) { return "panfeed_hip 0.1 (gfx950) weak-hash test build"; }
#else
const char* pf_version(void) { return "panfeed_hip 0.1 (gfx950)"; }
#endif

int pf_device_count(void) {
    int n = 0;
    hipError_t e = hipGetDeviceCount(&n);
    if (e != hipSuccess) return fail(PF_ERR_HIP, "hipGetDeviceCount: %s", hipGetErrorString(e));
    return n;
}

void pf_destroy(pf_ctx* c) {
    if (!c) return;
    (void)hipSetDevice(c->device);
    // Both streams are idle before any member goes, so the order in which pf_ctx declares its buffers, events and streams
    // does not matter to their owners.  (`side` by name as well: the stream ends wait for it only while a stream is open,
    // and a block of a rendered text that nobody asked for may be on its way into a pinned block without one.)
    if (c->stream) (void)hipStreamSynchronize(c->stream);
    ts_end(c);
    if (c->side) (void)hipStreamSynchronize(c->side);
    delete c;
}

int pf_create(pf_ctx** out, int device, const pf_opts* o) {
    if (!out || !o) return fail(PF_ERR_ARG, "pf_create: null argument");
    *out = nullptr;
    if (o->klength < 1 || o->klength > PF_MAX_K)
        return fail(PF_ERR_ARG, "klength %u unsupported (1..%d)", o->klength, PF_MAX_K);
    if (o->max_strains < 1 || o->max_strains > pf::MAX_CHUNKS * 32)
        return fail(PF_ERR_ARG, "max_strains %u unsupported (1..%u)", o->max_strains, pf::MAX_CHUNKS * 32);
    if (!o->maf_lo || !o->maf_hi) return fail(PF_ERR_ARG, "maf_lo / maf_hi tables are required");
    int ndev = 0;
    HIPCHK(hipGetDeviceCount(&ndev));
    if (device < 0 || device >= ndev) return fail(PF_ERR_ARG, "device %d not present (%d devices)", device, ndev);
    HIPCHK(hipSetDevice(device));
    hipDeviceProp_t prop;
    HIPCHK(hipGetDeviceProperties(&prop, device));
    if (strncmp(prop.gcnArchName, "gfx950", 6) != 0)
        return fail(PF_ERR_ARG, "device %d is %s; this library is built for gfx950 only", device, prop.gcnArchName);

    // (a step that fails leaves no context behind, and its error text is the one pf_last_error returns afterwards)
    struct Unmake { void operator()(pf_ctx* c) const { const std::string keep = g_err; pf_destroy(c); g_err = keep; } };
    std::unique_ptr<pf_ctx, Unmake> held(new pf_ctx());
    pf_ctx* const c = held.get();
    c->device = device;
    c->n_cu = prop.multiProcessorCount > 0 ? prop.multiProcessorCount : 256;
    c->o = *o;
    c->KW = (int)((2 * o->klength + 62) / 63);       // 63 key bits per word: k <= 31 one word ... k <= 126 four
    c->NS = pf::nslots_max(c->KW);
    c->W = (o->max_strains + 31) / 32;
    c->max_items = o->max_items ? o->max_items : 2048;
    {
        // work items of one launch = scratch slices resident at once; keep them within half of the free HBM
        size_t free_b = 0, total_b = 0;
        if (hipMemGetInfo(&free_b, &total_b) == hipSuccess && free_b) {
            const uint64_t fit = (free_b / 2) / Scratch::bytes_per_item(c->dims());
            if (c->max_items > fit) c->max_items = (uint32_t)std::max<uint64_t>(fit, 64);
        }
    }
    c->maf_lo.assign(o->maf_lo, o->maf_lo + o->max_strains + 1);
    c->maf_hi.assign(o->maf_hi, o->maf_hi + o->max_strains + 1);
    c->o.maf_lo = c->maf_lo.data();
    c->o.maf_hi = c->maf_hi.data();
    PFCHK(c->stream.create()); PFCHK(c->side.create());
    PFCHK(c->ev_fork.ensure(hipEventDisableTiming)); PFCHK(c->ev_join.ensure(hipEventDisableTiming));
    for (HipEvent& ev : c->ev_part) PFCHK(ev.ensure(hipEventDisableTiming));
    for (HipEvent& ev : c->ev_stage) PFCHK(ev.ensure(hipEventDisableTiming));
    PFCHK(c->pin_small.ensure(512, true));
    PFCHK(c->ev_t0.ensure()); PFCHK(c->ev_t1.ensure());
    PFCHK(scan_attr(c));
    PFCHK(upload_vec(c, c->d_maf_lo, c->maf_lo)); PFCHK(upload_vec(c, c->d_maf_hi, c->maf_hi));
    uint64_t cap = o->pattern_capacity ? o->pattern_capacity : (1ull << 24);
    uint64_t p2 = 1024;
    while (p2 < cap) p2 <<= 1;
    PFCHK(alloc_pattern_bufs(c, p2, false, c->pats)); PFCHK(c->pt_counters.ensure(16));
    sync_pattern_table(c);
    PFCHK(reset_patterns(c));
    PFCHK(c->batch.cursor.ensure(64)); PFCHK(c->scratch.ensure(c->max_items, c->dims()));
    if (const hipError_t e = hipStreamSynchronize(c->stream); e != hipSuccess)
        return fail(PF_ERR_HIP, "pf_create sync: %s", hipGetErrorString(e));
    *out = held.release();
    return PF_OK;
}

int pf_reset_patterns(pf_ctx* c) {
    if (!c) return fail(PF_ERR_ARG, "null context");
    HIPCHK(hipSetDevice(c->device));
    ts_end(c, TextStream::PATTERN_ROWS);  // (its rows were measured in the pool that goes now)
    PFCHK(reset_patterns(c));
    HIPCHK(hipStreamSynchronize(c->stream));
    return PF_OK;
}

int pf_dev_alloc(pf_ctx* c, uint64_t bytes, void** dptr) {
    if (!c || !dptr) return fail(PF_ERR_ARG, "null argument");
    HIPCHK(hipSetDevice(c->device));
    HIPCHK(hipMalloc(dptr, bytes ? bytes : 16));
    return PF_OK;
}
int pf_dev_free(pf_ctx* c, void* dptr) {
    if (!c) return fail(PF_ERR_ARG, "null context");
    HIPCHK(hipSetDevice(c->device));
    HIPCHK(hipFree(dptr));
    return PF_OK;
}
int pf_dev_upload(pf_ctx* c, void* dptr, const void* src, uint64_t bytes) {
    if (!c) return fail(PF_ERR_ARG, "null context");
    HIPCHK(hipSetDevice(c->device));
    HIPCHK(hipMemcpy(dptr, src, bytes, hipMemcpyHostToDevice));
    return PF_OK;
}
int pf_dev_download(pf_ctx* c, void* dst, const void* dptr, uint64_t bytes) {
    if (!c) return fail(PF_ERR_ARG, "null context");
    HIPCHK(hipSetDevice(c->device));
    HIPCHK(hipStreamSynchronize(c->stream));
    HIPCHK(hipMemcpy(dst, dptr, bytes, hipMemcpyDeviceToHost));
    return PF_OK;
}

int pf_synth_expand(pf_ctx* c, const uint64_t* allele_words, const uint64_t* allele_word_off,
                    const uint32_t* seg_allele, const uint64_t* seg_word_off, const uint32_t* seg_len,
                    uint32_t n_segs, uint64_t* packed) {
    if (!c) return fail(PF_ERR_ARG, "null context");
    HIPCHK(hipSetDevice(c->device));
    if (!n_segs) return PF_OK;
    hipLaunchKernelGGL(pf::synth_expand_kernel, dim3(2048), dim3(256), 0, c->stream, allele_words, allele_word_off,
                       seg_allele, seg_word_off, seg_len, n_segs, packed);
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(c->stream));
    return PF_OK;
}

uint64_t pf_pack_acgt(const char* seq, uint32_t len, uint64_t* dst) {
    const uint64_t nw = 2ull * ((len + 63) / 64);
    for (uint64_t i = 0; i < nw; i++) dst[i] = 0;
    for (uint32_t i = 0; i < len; i++) {
        uint64_t code;
        switch (seq[i]) {
            case 'A': code = 0; break;
            case 'C': code = 1; break;
            case 'G': code = 2; break;
            default: code = 3; break;
        }
        dst[i >> 5] |= code << (62 - 2 * (i & 31));
    }
    return nw;
}

void pf_b64_digest(const uint8_t d[16], char out[24]) {
    static const char* T = "ABCDEFGHIJKLMNOPQRSTUVWXYZabcdefghijklmnopqrstuvwxyz0123456789+/";
    int o = 0;
    for (int i = 0; i < 15; i += 3) {
        uint32_t v = ((uint32_t)d[i] << 16) | ((uint32_t)d[i + 1] << 8) | d[i + 2];
        out[o++] = T[(v >> 18) & 63]; out[o++] = T[(v >> 12) & 63]; out[o++] = T[(v >> 6) & 63]; out[o++] = T[v & 63];
    }
    uint32_t v = (uint32_t)d[15] << 16;
    out[o++] = T[(v >> 18) & 63]; out[o++] = T[(v >> 12) & 63]; out[o++] = '='; out[o++] = '=';
}

// ---------------------------------------------------------------------------------------------
namespace {
constexpr int PF_RETRY_PATTERNS = 1;   // internal: the batch ran out of pattern ids, *need = ids it asked for

// A cluster of three or more key partitions (a dedup view, keys of up to two words) has its windows sorted by
// partition first (bin_kernel): its items then read their own windows instead of each walking the whole view.
// The entry arrays belong to a sub-batch; a sub-batch ends where they would pass BIN_MAX_ENTRIES.
constexpr uint32_t BIN_MIN_PARTS = 3;      // (at two, a cluster's own bin_kernel workgroup takes longer than the second walk it saves)
constexpr uint64_t BIN_MAX_ENTRIES = 1ull << 28;

// plan_kernel's output block of a part: item arrays, work lists, unit-view list, the scan's block sums
struct DPtrs { uint32_t *it_cluster, *it_nslots, *w_scan, *w_fin, *w_fin2, *w_fin5, *unit_cluster, *unit_base, *blk; };
DPtrs dplan_ptrs(const pf_ctx::DPlan& plan) {
    uint32_t* b = plan.block.as<uint32_t>();
    const size_t n = plan.n;
    return DPtrs{b, b + n, b + 2 * n, b + 3 * n, b + 4 * n, b + 5 * n, b + 6 * n, b + 7 * n, b + 8 * n};
}
struct FinWork { const uint32_t* work; uint32_t n; };   // a launch's stretch of a work list (one class of the fused finish kernels)
// a host-planned pass: its sub-batches (one launch each) and their stretches of the work lists (off[s] to off[s + 1])
struct Sub { uint32_t item0, nitems, cl0, ncl, pool, bin0, nbin; uint64_t q_total; };
struct SubLists { uint32_t at[HostPass::N_LISTS]; };     // by HostPass::List
struct Pass { std::vector<Sub> subs; std::vector<SubLists> off; uint64_t arena_cap = 0; size_t NB = 0; };

// What one submit_once call carries from stage to stage (what outlives the call is in pf_ctx).  The member functions
// are the stages and their shared launches, in the order a batch meets them.
struct SubmitRun {
    pf_ctx* c; const pf_batch* b; const pf_gather* gth;
    pf_batch d;                            // the batch as device pointers
    const uint32_t C, NSEG, W, NS, KW;
    const uint64_t mult;                   // a window's instances: both strands unless canonical
    uint32_t P = 1, part_end[pf_ctx::MAX_PARTS] = {};   // part h: clusters [part_end[h - 1], part_end[h])
    pf::ClusterRec* rec = nullptr;         // the dedup pass's record per cluster, in pinned memory
    uint32_t* h_exfirst = nullptr;         // [C + 1] + the "bad list" flag, in pinned memory (device-side CSR only)
    bool ex_on_device = false; std::vector<uint32_t> ex_first;     // extras per cluster (CSR)
    std::vector<uint32_t> nparts, todo;    // key partitions per cluster; the clusters of the pass being built
    pf::DedupParams dp{};
    bool use_plan = false; pf::PlanClassify pcls{};   // what cluster_ninst_kernel works out per cluster for plan_kernel
    double share = 0.0; PartModel::Fit fit;           // the key-partition estimate (first_nparts) and the line it learned
    struct Deferred { Arena* ar; uint32_t pin; }; std::vector<Deferred> deferred;   // passes not yet waited for (read-backs queued)
    uint64_t arena_base = 0; uint32_t arena_i = 0;    // arenas used so far: one per launched pass, the device-planned ones included
    Arena* ar = nullptr;                   // the arena of the pass being launched
    uint32_t cnt2[3] = {0, 0, 0};          // pattern counters {ids handed out, pool overflow, arena overflow}
    uint64_t total_inst = 0;
    const bool dbg = getenv("PF_DEBUG_TIMING") != nullptr;
    std::chrono::steady_clock::time_point t_host0 = std::chrono::steady_clock::now();

    SubmitRun(pf_ctx* c_, const pf_batch* b_, const pf_gather* g_)
        : c(c_), b(b_), gth(g_), d(*b_), C(b_->n_clusters), NSEG(b_->n_segs), W(c_->W), NS(c_->NS), KW((uint32_t)c_->KW), mult(c_->o.canon ? 1 : 2) {}
    void lap(const char* what) {
        if (!dbg) return;
        auto t = std::chrono::steady_clock::now();
        fprintf(stderr, "[pf_submit] %-28s %8.3f ms\n", what, std::chrono::duration<double, std::milli>(t - t_host0).count());
        t_host0 = t;
    }
    uint32_t part_begin(uint32_t h) const { return h ? part_end[h - 1] : 0; }
    // an attempt's route, for pf_debug_cluster_routes
    void note_route(uint32_t ci, uint32_t cls, uint32_t np, uint32_t ns) {
        pf_ctx::Route& rt = c->routes[ci];
        if (!rt.attempts++) rt.first = (uint8_t)cls;
        rt.cls = (uint8_t)cls; rt.mode = (uint8_t)(rec[ci].mode & 3u); rt.nparts = np; rt.nslots = ns;
    }

    // ---- batch arrays on the device
    int upload_batch() {
        std::vector<uint32_t> h_extra_cluster;
        if (gth && b->on_device) return fail(PF_ERR_ARG, "pf_submit_gather takes host arrays");
        const uint64_t total_words = gth ? gth->n_words : b->n_words;
        if (!b->on_device) {
            // validate what the kernels index with (host copies are at hand)
            for (uint32_t i = 0; i < C; i++) {
                if (b->cluster_seg_off[i] > b->cluster_seg_off[i + 1] || b->cluster_seg_off[i + 1] > NSEG)
                    return fail(PF_ERR_ARG, "cluster_seg_off not monotone / out of range at %u", i);
                if (b->cluster_nstrains[i] > c->o.max_strains || b->cluster_npresab[i] > c->o.max_strains)
                    return fail(PF_ERR_ARG, "cluster %u has more strains than max_strains", i);
                // init_presabs_vector, panfeed.py:19: a boolean mask must have the vector's length (numpy IndexError)
                if (c->o.consider_missing && b->cluster_nstrains[i] != b->cluster_npresab[i])
                    return fail(PF_ERR_ARG, "cluster %u: consider_missing needs len(clusterpresab) == number of strains "
                                "(%u != %u)", i, b->cluster_npresab[i], b->cluster_nstrains[i]);
            }
            if (C && b->cluster_seg_off[0] != 0) return fail(PF_ERR_ARG, "cluster_seg_off[0] must be 0");
            const uint32_t pad_words = KW <= 2 ? 2u : 4u;     // a lane reads KW + 1 words from its window's first word
            for (uint32_t s = 0; s < NSEG; s++) {
                const uint64_t nw = 2ull * ((b->seg_len[s] + 63) / 64);
                if ((b->seg_word_off[s] & 1) || b->seg_word_off[s] + nw + pad_words > total_words)
                    return fail(PF_ERR_ARG, "segment %u: misaligned or outside packed[] (needs %u words of tail padding)", s, pad_words);
            }
            for (uint32_t i = 0; i < C; i++)
                for (uint32_t s = b->cluster_seg_off[i]; s < b->cluster_seg_off[i + 1]; s++) {
                    if (b->seg_sample[s] >= b->cluster_nstrains[i])
                        return fail(PF_ERR_ARG, "segment %u: sample column %u >= n_strains %u", s, b->seg_sample[s],
                                    b->cluster_nstrains[i]);
                    if (s > b->cluster_seg_off[i] && b->seg_sample[s] < b->seg_sample[s - 1])
                        return fail(PF_ERR_ARG, "segments of cluster %u are not sorted by sample", i);
                }
            if (!gth) PFCHK(upload(c, c->caller.b_packed, b->packed, (size_t)b->n_words, &d.packed));
            PFCHK(upload(c, c->caller.b_seg_word_off, b->seg_word_off, NSEG, &d.seg_word_off));
            PFCHK(upload(c, c->caller.b_seg_len, b->seg_len, NSEG, &d.seg_len));
            if (gth) {
                // the packed input is produced on the device: segments copied (or reverse-complemented) out of the
                // resident genomes, plus the few the host packed itself (b->packed = the literal words)
                if (NSEG && (!gth->src_off || !gth->src_start || !gth->src_flags)) return fail(PF_ERR_ARG, "gather arrays missing");
                for (uint32_t s = 0; s < NSEG; s++) {
                    const uint64_t nw = 2ull * ((b->seg_len[s] + 63) / 64);
                    const uint64_t last = (uint64_t)gth->src_start[s] + b->seg_len[s];         // bases
                    if (gth->src_flags[s] & 1u) {
                        if (gth->src_off[s] + nw + 1 > b->n_words || gth->src_start[s] != 0 || (gth->src_flags[s] & 2u))
                            return fail(PF_ERR_ARG, "segment %u: literal source outside packed[]", s);
                    } else if (gth->src_off[s] + (last + 31) / 32 + 1 > c->g_words) {
                        return fail(PF_ERR_ARG, "segment %u: source range outside the resident genomes", s);
                    }
                }
                PFCHK(c->caller.b_packed.ensure((size_t)std::max<uint64_t>(total_words, 4) * 8));
                d.packed = c->caller.b_packed.as<uint64_t>();
                const uint64_t* lit; const uint64_t* so; const uint32_t* ss; const uint32_t* sf;
                PFCHK(upload(c, c->caller.b_literal, b->packed, (size_t)b->n_words, &lit));
                PFCHK(upload(c, c->caller.g_src_off, gth->src_off, NSEG, &so));
                PFCHK(upload(c, c->caller.g_src_start, gth->src_start, NSEG, &ss));
                PFCHK(upload(c, c->caller.g_src_flags, gth->src_flags, NSEG, &sf));
                if (total_words >= 4)
                    HIPCHK(hipMemsetAsync(c->caller.b_packed.as<uint64_t>() + (total_words - 4), 0, 32, c->stream));
                if (NSEG) {
                    pf::GatherParams gp{};
                    gp.store = c->g_store.as<uint64_t>(); gp.literal = lit; gp.src_off = so; gp.src_start = ss; gp.src_flags = sf;
                    gp.seg_word_off = d.seg_word_off; gp.seg_len = d.seg_len; gp.packed = c->caller.b_packed.as<uint64_t>(); gp.n_segs = NSEG;
                    hipLaunchKernelGGL(pf::gather_segments_kernel, dim3((NSEG + 15) / 16), dim3(256), 0, c->stream, gp);
                    HIPCHK(hipGetLastError());
                }
            }
            PFCHK(upload(c, c->caller.b_seg_sample, b->seg_sample, NSEG, &d.seg_sample));
            PFCHK(upload(c, c->caller.b_seg_ord, b->seg_ord_base, NSEG, &d.seg_ord_base));
            PFCHK(upload(c, c->caller.b_cl_seg_off, b->cluster_seg_off, (size_t)C + 1, &d.cluster_seg_off));
            PFCHK(upload(c, c->caller.b_cl_nstr, b->cluster_nstrains, C, &d.cluster_nstrains));
            PFCHK(upload(c, c->caller.b_cl_npres, b->cluster_npresab, C, &d.cluster_npresab));
            PFCHK(upload(c, c->caller.b_cl_presab, b->cluster_presab, (size_t)C * W, &d.cluster_presab));
            PFCHK(upload(c, c->caller.b_cl_ordinal, b->cluster_ordinal, C, &d.cluster_ordinal));
            PFCHK(upload(c, c->caller.b_extra_ord, b->extra_ord, b->n_extra, &d.extra_ord));
            PFCHK(upload(c, c->caller.b_extra_bits, b->extra_bits, (size_t)b->n_extra * W, &d.extra_bits));
            if (b->seg_strand_off) PFCHK(upload(c, c->caller.b_seg_strand_off, b->seg_strand_off, NSEG, &d.seg_strand_off));
            if (b->n_extra) h_extra_cluster.assign(b->extra_cluster, b->extra_cluster + b->n_extra);
        }
        // extras per cluster (CSR).  A batch that is in device memory already has its list checked and counted there
        // (extra_csr_kernel); the counts come back with the first dedup results -- reading the list back and walking it here
        // was 1 ms in front of the first kernel with SURVEY 8d's share of 'N's (1.5 M rows per 50 000 clusters).
        ex_on_device = b->on_device && b->n_extra;
        if (ex_on_device && !C) return fail(PF_ERR_ARG, "extra_cluster must be non-decreasing and < n_clusters");
        ex_first.assign((size_t)C + 1, 0);
        if (!ex_on_device) {
            for (uint32_t e = 0; e < b->n_extra; e++) {
                if (h_extra_cluster[e] >= C || (e && h_extra_cluster[e] < h_extra_cluster[e - 1]))
                    return fail(PF_ERR_ARG, "extra_cluster must be non-decreasing and < n_clusters");
            }
            for (uint32_t e = 0; e < b->n_extra; e++) ex_first[h_extra_cluster[e] + 1]++;
            for (uint32_t i = 0; i < C; i++) ex_first[i + 1] += ex_first[i];
            PFCHK(upload_vec(c, c->batch.extra_off, ex_first));
        }
        return PF_OK;
    }
    // ---- per batch outputs
    int ensure_batch_outputs() {
        PFCHK(c->batch.ensure(C, NSEG, b->n_extra));   // (cl_overflow / cl_kmer_cnt / cl_unique / cl_pattern: start values from the dedup kernel)
        HIPCHK(hipMemsetAsync(c->batch.cursor.p, 0, 64, c->stream));
        return PF_OK;
    }
    // ---- the device plan (plan_kernel) of part h: the simple clusters' work items laid out behind the part's dedup, a
    // 40-byte summary on its way to pinned memory
    int launch_plan(uint32_t h, uint32_t c0, uint32_t c1) {
        pf_ctx::DPlan& plan = c->dplan[h];
        plan.n = c1 - c0;
        const uint32_t nblk = (plan.n + pf::PLAN_THREADS - 1) / pf::PLAN_THREADS;
        PFCHK(plan.block.ensure(((size_t)plan.n * 8 + (size_t)nblk * pf::PLAN_BLK_WORDS) * 4));
        PFCHK(plan.it_count.ensure((size_t)plan.n * 4));
        PFCHK(plan.out.ensure(sizeof(pf::PlanOut)));
        PFCHK(plan.pin_out.ensure(64, true));
        const DPtrs q = dplan_ptrs(plan);
        pf::PlanParams pp{};
        pp.rec = c->batch.cl_rec.as<pf::ClusterRec>(); pp.plan_room = c->plan_room.as<uint32_t>(); pp.plan_arena = c->plan_arena.as<uint32_t>();
        pp.c0 = c0; pp.c1 = c1; pp.NS = NS; pp.max_items = c->max_items;
        pp.it_cluster = q.it_cluster; pp.it_nslots = q.it_nslots; pp.w_scan = q.w_scan; pp.w_fin = q.w_fin; pp.w_fin2 = q.w_fin2;
        pp.w_fin5 = q.w_fin5; pp.unit_cluster = q.unit_cluster; pp.unit_base = q.unit_base; pp.blk = q.blk;
        pp.out = plan.out.as<pf::PlanOut>();
        hipLaunchKernelGGL(pf::plan_count_kernel, dim3(nblk), dim3(pf::PLAN_THREADS), 0, c->stream, pp);
        hipLaunchKernelGGL(pf::plan_scan_kernel, dim3(1), dim3(256), 0, c->stream, pp, nblk);
        hipLaunchKernelGGL(pf::plan_scatter_kernel, dim3(nblk), dim3(pf::PLAN_THREADS), 0, c->stream, pp);
        HIPCHK(hipGetLastError());
        HIPCHK(hipMemcpyAsync(plan.pin_out.p, plan.out.p, sizeof(pf::PlanOut), hipMemcpyDeviceToHost, c->stream));
        return PF_OK;
    }
    // the dedup of part h and its results on their way to pinned memory (ev_part[h])
    int launch_dedup_part(uint32_t h) {
        const uint32_t c0 = part_begin(h), c1 = part_end[h], n = c1 - c0;
        if (n) {
            dp.cluster_base = c0;
            PFCHK(mark_begin(c, TimeCat::dedup));
            hipLaunchKernelGGL(pf::cluster_dedup_kernel<pf::DedupSmall>, dim3(n), dim3(pf::DEDUP_THREADS), 0, c->stream, dp);
            HIPCHK(hipGetLastError());
            PFCHK(mark_end(c));
            PFCHK(launch_ninst(c0, n, nullptr, pcls));
            if (use_plan) PFCHK(launch_plan(h, c0, c1));
            HIPCHK(hipMemcpyAsync(rec + c0, c->batch.cl_rec.as<pf::ClusterRec>() + c0, (size_t)n * sizeof(pf::ClusterRec), hipMemcpyDeviceToHost, c->stream));
        }
        HIPCHK(hipEventRecord(c->ev_part[h], c->stream));
        return PF_OK;
    }
    // what the host (and plan_kernel, by `cls`) needs of the dedup pass, a record per cluster: `count` from `first` on, or `list`'s
    int launch_ninst(uint32_t first, uint32_t count, const uint32_t* list, const pf::PlanClassify& cls) {
        const pf::View v = view(nullptr); const pf::ViewFacts vf = view_facts();
        hipLaunchKernelGGL(pf::cluster_ninst_kernel, dim3((count + 3) / 4), dim3(256), 0, c->stream, d.cluster_seg_off, d.seg_len,
                           v.plain.len, v.v_nseg, c->o.klength, first, first + count, list, vf.v_mode, vf.v_dense, vf.v_nstr,
                           c->batch.cl_rec.as<pf::ClusterRec>(), cls);
        HIPCHK(hipGetLastError());
        return PF_OK;
    }
    // ---- identical segments -> scan view (mode 1) or the caller's list as it is (mode 0); then the strand bits
    // The dedup kernel's per-cluster results come back into pinned memory, in two halves for a large batch: the
    // host builds and launches the first half's work items while the GPU is still on the second half's dedup, and the
    // second half's while the first half's scan runs -- otherwise the GPU idles for the ~1.2 ms that takes.
    int launch_dedup_parts() {
        const size_t C8 = ((size_t)C + 1) & ~(size_t)1;
        PFCHK(c->pin_dedup.ensure(C8 * sizeof(pf::ClusterRec) + 64 + ((size_t)C + 2) * 4));
        // what the host needs of the dedup pass per cluster, one 40-byte record each (pf::ClusterRec, written by
        // cluster_ninst_kernel): ONE copy per part brings them over -- six small copies in a row were 40 us of the part's
        // critical path
        rec = c->pin_dedup.as<pf::ClusterRec>();
        h_exfirst = reinterpret_cast<uint32_t*>(rec + C8);
        if (ex_on_device) {
            PFCHK(c->batch.extra_off.ensure(((size_t)C + 2) * 4));
            uint32_t* exo = c->batch.extra_off.as<uint32_t>();
            HIPCHK(hipMemsetAsync(exo + C + 1, 0, 4, c->stream));
            hipLaunchKernelGGL(pf::extra_csr_kernel, dim3(std::min<uint32_t>((std::max(C + 1, b->n_extra) + 255) / 256, 2048u)), dim3(256), 0,
                               c->stream, b->extra_cluster, b->n_extra, C, exo, exo + C + 1);
            HIPCHK(hipGetLastError());
            HIPCHK(hipMemcpyAsync(h_exfirst, exo, ((size_t)C + 2) * 4, hipMemcpyDeviceToHost, c->stream));
        }
        // A large batch goes through in parts, all queued without a host sync in between: the host builds and launches a
        // part's work items while the GPU is on earlier parts (otherwise it idles for the ~1.2 ms that takes).  Two parts,
        // a quarter first: enough GPU work to hide building the rest.  (More, equal parts with the MD5 of part i on a second
        // stream beside part i + 1's finish kernels or part i + 2's dedup were measured and lose: DESIGN.md section 6.)
        P = C >= 8192 ? 2u : 1u;
        for (uint32_t q = 0; q < P; q++) part_end[q] = q + 1 == P ? C : (uint32_t)((uint64_t)C * (q + 1) / (2 * P));
        if (C) {
            dp.packed = d.packed; dp.seg_word_off = d.seg_word_off; dp.seg_len = d.seg_len;
            dp.seg_sample = d.seg_sample; dp.seg_ord_base = d.seg_ord_base;
            dp.cluster_seg_off = d.cluster_seg_off; dp.cluster_nstrains = d.cluster_nstrains;
            dp.extra_ord = d.extra_ord;
            c->batch.dedup_outputs(dp);
            dp.k = c->o.klength; dp.W = W; dp.canon = c->o.canon; dp.enable = (c->o.flags & PF_FLAG_NO_DEDUP) ? 0u : 1u;
        }
        // ---- the device plan: the estimate's learned line is what this context knew when the batch came in (the host's
        // own estimate for the rest of the part reads the same sums: they change at the end of a submit only)
        use_plan = (c->o.flags & PF_FLAG_DEVICE_PLAN) && C > 0 && c->max_items < (1u << 22);
        share = 1.0 - std::pow(0.99, (double)c->o.klength) + 0.06;
        fit = c->part_model.fit();
        if (use_plan) {
            if (C > c->dp_const_n) {
                // zeros | ones | 0, 1, 2, ...: item_part / extra_first / is_extra / binned, item_nparts / nsib / compact, slice / sib0
                const uint32_t n = C + C / 4 + 64;
                std::vector<uint32_t> h(3 * (size_t)n, 0u);
                for (uint32_t i = 0; i < n; i++) { h[n + i] = 1u; h[2 * (size_t)n + i] = i; }
                PFCHK(c->dp_const.ensure(h.size() * 4));
                HIPCHK(hipMemcpy(c->dp_const.p, h.data(), h.size() * 4, hipMemcpyHostToDevice));
                c->dp_const_n = n;
            }
            PFCHK(c->plan_room.ensure((size_t)C * 4));
            PFCHK(c->plan_arena.ensure((size_t)C * 4));
            pcls.extra_off = c->batch.extra_off.as<uint32_t>(); pcls.plan_room = c->plan_room.as<uint32_t>(); pcls.plan_arena = c->plan_arena.as<uint32_t>();
            pcls.mult = c->o.canon ? 1u : 2u; pcls.NS = NS; pcls.W = W; pcls.unit_view = (c->o.flags & PF_FLAG_NO_UNIT_DEDUP) ? 0u : 1u;
            pcls.reg_ready = fit.ready ? 1u : 0u; pcls.share = share; pcls.reg_a = fit.a; pcls.reg_b = fit.b; pcls.reg_half_sd = fit.half_sd;
        }
        if (C)
            for (uint32_t h = 0; h < P; h++) PFCHK(launch_dedup_part(h));   // all parts are queued up front
        // ---- strand bits of target-strain segments (canonical mode)
        c->n_strand_words = (b->seg_strand_off && c->o.canon) ? b->n_strand_words : 0;
        if (c->n_strand_words && NSEG) {
            PFCHK(c->strand_bits.ensure((size_t)c->n_strand_words * 8));
            HIPCHK(hipMemsetAsync(c->strand_bits.p, 0, (size_t)c->n_strand_words * 8, c->stream));
            const uint32_t blocks = (uint32_t)std::min<uint64_t>(((uint64_t)NSEG + 3) / 4, 4096);
            auto strand = [&](auto kern) {
                hipLaunchKernelGGL(kern, dim3(blocks), dim3(256), 0, c->stream, d.packed, d.seg_word_off, d.seg_len,
                                   d.seg_strand_off, NSEG, c->o.klength, c->strand_bits.as<uint64_t>());
            };
            switch (KW) {
                case 1: strand(pf::strand_bits_kernel<1>); break;
                case 2: strand(pf::strand_bits_kernel<2>); break;
                case 3: strand(pf::strand_bits_kernel<3>); break;
                default: strand(pf::strand_bits_kernel<4>); break;
            }
            HIPCHK(hipGetLastError());
        }
        return PF_OK;
    }
    // clusters the small dedup class gave up on for lack of room (more than 64 distinct sequences, a sample-set
    // matrix or an ordinal bitmap that does not fit): the wide class on those alone, then their counts again
    int retry_wide(uint32_t c0, uint32_t c1) {
        std::vector<uint32_t>& wide_list = c->hs.wide;
        wide_list.clear();
        for (uint32_t i = c0; i < c1; i++) if (rec[i].mode & pf::MODE_RETRY_WIDE) wide_list.push_back(i);
        if (wide_list.empty()) return PF_OK;
        const uint32_t nw = (uint32_t)wide_list.size();
        PFCHK(c->wide_list.ensure((size_t)nw * 4));
        HIPCHK(hipMemcpyAsync(c->wide_list.p, wide_list.data(), (size_t)nw * 4, hipMemcpyHostToDevice, c->stream));
        pf::DedupParams dw = dp;
        dw.cluster_base = 0; dw.cluster_list = c->wide_list.as<uint32_t>();
        PFCHK(mark_begin(c, TimeCat::dedup));
        hipLaunchKernelGGL(pf::cluster_dedup_kernel<pf::DedupWide>, dim3(nw), dim3(pf::DEDUP_THREADS), 0, c->stream, dw);
        HIPCHK(hipGetLastError());
        PFCHK(mark_end(c));
        PFCHK(launch_ninst(0, nw, c->wide_list.as<uint32_t>(), pf::PlanClassify{}));   // (the wide class's clusters are the host's: no plan bits)
        HIPCHK(hipMemcpyAsync(rec + c0, c->batch.cl_rec.as<pf::ClusterRec>() + c0, (size_t)(c1 - c0) * sizeof(pf::ClusterRec), hipMemcpyDeviceToHost, c->stream));
        HIPCHK(hipStreamSynchronize(c->stream));
        c->timing.n_wide_clusters += nw;
        return PF_OK;
    }
    // ---- unit view: identical 64-window units among the distinct sequences of a cluster are scanned once
    // (unit_class_kernel): the clusters of up to 64 distinct sequences first (one wave each, no table), then the wider
    // ones.  Their list {clusters | places in the pool} is plan_kernel's (`plan`), or the host's in up.pin (plan null).
    int launch_unit_classes(pf_ctx::UPool& up, uint32_t nsmall, uint32_t nwide, uint64_t room, const DPtrs* plan) {
        const uint32_t nu = nsmall + nwide;
        // (twice the room: the wide kernel parks a cluster's pieces in the second stretch before it orders them by chunk)
        const size_t R = (size_t)room + 1, R2 = 2 * R;
        if (R2 > 0xFFFFFFF0ull) return fail(PF_ERR_CAPACITY, "unit view of %zu pieces: submit fewer clusters at a time", R);
        PFCHK(up.word_off.ensure(R2 * 8)); PFCHK(up.len.ensure(R2 * 4)); PFCHK(up.sample.ensure(R2 * 4));
        PFCHK(up.ord.ensure(R2 * 4)); PFCHK(up.bits.ensure(R2 * 4));
        pf::UnitParams q{};
        if (plan) {
            q.list_cluster = plan->unit_cluster; q.list_base = plan->unit_base;
        } else {
            PFCHK(up.list.ensure((size_t)nu * 8));
            HIPCHK(hipMemcpyAsync(up.list.p, up.pin.p, (size_t)nu * 8, hipMemcpyHostToDevice, c->stream));
            q.list_cluster = up.list.as<uint32_t>(); q.list_base = up.list.as<uint32_t>() + nu;
        }
        q.packed = d.packed; q.cluster_seg_off = d.cluster_seg_off; q.v_nstr = c->batch.v_nstr.as<uint32_t>();
        q.view = view(&up); q.k = c->o.klength; q.tmp_off = (uint32_t)R;
        PFCHK(mark_begin(c, TimeCat::dedup));
        if (nsmall) {
            const dim3 g((nsmall + 3) / 4), b(256);
            switch ((63 + c->o.klength + 31) / 32) {       // words a unit's 63 + k bases take
                case 2: hipLaunchKernelGGL(pf::unit_class_small_kernel<2>, g, b, 0, c->stream, q, nsmall); break;
                case 3: hipLaunchKernelGGL(pf::unit_class_small_kernel<3>, g, b, 0, c->stream, q, nsmall); break;
                case 4: hipLaunchKernelGGL(pf::unit_class_small_kernel<4>, g, b, 0, c->stream, q, nsmall); break;
                case 5: hipLaunchKernelGGL(pf::unit_class_small_kernel<5>, g, b, 0, c->stream, q, nsmall); break;
                default: hipLaunchKernelGGL(pf::unit_class_small_kernel<6>, g, b, 0, c->stream, q, nsmall); break;
            }
            HIPCHK(hipGetLastError());
        }
        if (nwide) {
            pf::UnitParams qw = q;
            qw.list_cluster += nsmall; qw.list_base += nsmall;
            hipLaunchKernelGGL(pf::unit_class_kernel, dim3(nwide), dim3(pf::UNIT_THREADS), 0, c->stream, qw);
            HIPCHK(hipGetLastError());
        }
        PFCHK(mark_end(c));
        return PF_OK;
    }
    // ---- the kernels' argument groups (pf_kernels.h): the owning groups' own with what this batch adds, built at the launch
    // that uses them and never kept across a DevBuf::ensure, which may move a buffer (q_key, the arenas, the unit pools).
    pf::CallerSegs caller_segs() const {
        return pf::CallerSegs{d.cluster_seg_off, d.seg_sample, c->batch.seg_distinct.as<uint32_t>(), d.cluster_nstrains,
                              d.cluster_npresab, d.cluster_presab, d.cluster_ordinal};
    }
    pf::View view(const pf_ctx::UPool* up) const {     // (the dedup pass has no pool yet)
        pf::View v = c->batch.view();
        if (up) v.pool = pf::ViewSegs{up->word_off.as<uint64_t>(), up->len.as<uint32_t>(), up->sample.as<uint32_t>(),
                                      up->ord.as<uint32_t>(), up->bits.as<uint32_t>()};
        return v;
    }
    pf::ViewFacts view_facts() const { return c->batch.view_facts(d.extra_bits); }
    pf::Outputs outputs() const { return c->batch.outputs(*ar); }
    pf::SlotDump slot_dump(uint32_t* item_count) const { return c->scratch.slot_dump(item_count); }
    pf::RowScratch row_scratch() const { return c->scratch.row_scratch(c->pass.it_unique.as<uint32_t>(), c->pass.it_kept.as<uint32_t>()); }
    pf::PatternPool pattern_pool() const { return c->pats.pattern_pool(); }
    // plan_kernel's items (the host's: HostPass::items()), all "one partition, own slice, compact, nothing else": constant arrays stand in
    static pf::Items planned_items(const uint32_t* cluster, const uint32_t* nslots, const uint32_t* zeros, const uint32_t* ones, const uint32_t* iota) {
        return pf::Items{cluster, zeros, ones, nslots, iota, ones, zeros, zeros, zeros, iota, ones};
    }
    pf::RowOpts row_opts() const {
        return pf::RowOpts{c->d_maf_lo.as<uint32_t>(), c->d_maf_hi.as<uint32_t>(), W, NS, KW,
                           (uint32_t)c->o.consider_missing, (uint32_t)c->o.patfilt, (uint32_t)c->o.multiple_files};
    }
    // ---- parameter blocks of the scan and the fused finish kernels, from a pass's items and their key counts
    pf::ScanParams scan_params(const pf::Items& items, uint32_t* item_count, const pf_ctx::UPool& up, const uint32_t* work) const {
        pf::ScanParams sp{};
        const pf::ViewFacts vf = view_facts();
        sp.packed = d.packed; sp.view = view(&up); sp.v_nstr = vf.v_nstr; sp.cluster_overflow = vf.cluster_overflow;
        sp.item_cluster = items.item_cluster; sp.item_part = items.item_part; sp.item_nparts = items.item_nparts;
        sp.item_nslots = items.item_nslots; sp.item_scratch = items.item_scratch; sp.item_compact = items.item_compact;
        sp.item_binned = items.item_binned;
        sp.dump = slot_dump(item_count);
        sp.work = work;
        sp.k = c->o.klength; sp.W = W; sp.NS = NS;
        return sp;
    }
    pf::FinishParams finish_params(const pf::Items& items, uint32_t* item_count) const {
        pf::FinishParams fp{};
        // (flat, in the order it always had: finish_kernel's register allocation follows the block's layout)
        const pf::CallerSegs cl = caller_segs();
        const pf::ViewFacts vf = view_facts();
        const pf::SlotDump dump = slot_dump(item_count);
        const pf::Outputs out = outputs();
        const pf::PatternPool pats = pattern_pool();
        const pf::RowOpts opt = row_opts();
        fp.item_cluster = items.item_cluster; fp.item_nslots = items.item_nslots; fp.item_scratch = items.item_scratch;
        fp.item_nparts = items.item_nparts; fp.cluster_overflow = vf.cluster_overflow;
        fp.cluster_seg_off = cl.cluster_seg_off; fp.seg_sample = cl.seg_sample; fp.seg_distinct = cl.seg_distinct;
        fp.v_nstr = vf.v_nstr; fp.v_dense = vf.v_dense;
        fp.cluster_nstrains = cl.cluster_nstrains; fp.cluster_npresab = cl.cluster_npresab;
        fp.cluster_presab = cl.cluster_presab; fp.cluster_ordinal = cl.cluster_ordinal;
        fp.maf_lo = opt.maf_lo; fp.maf_hi = opt.maf_hi;
        fp.item_count = dump.item_count; fp.tab_key = dump.tab_key; fp.tab_ord = dump.tab_ord;
        fp.cmask_lo = dump.cmask_lo; fp.cmask_hi = dump.cmask_hi;
        fp.extra_off = vf.extra_off; fp.extra_dense = vf.extra_dense; fp.extra_bits = vf.extra_bits;
        fp.out_key = out.out_key; fp.out_pid = out.out_pid;
        fp.cluster_kmer_off = out.cluster_kmer_off; fp.cluster_kmer_cnt = out.cluster_kmer_cnt;
        fp.cluster_unique = out.cluster_unique; fp.cluster_pattern = out.cluster_pattern;
        fp.cursor = out.cursor; fp.pt = c->pt;
        fp.pat_bits = pats.pat_bits; fp.pat_nan = pats.pat_nan; fp.pat_n = pats.pat_n;
        fp.out_base = out.out_base; fp.out_cap = out.out_cap; fp.W = opt.W; fp.NS = opt.NS; fp.KW = opt.KW;
        fp.consider_missing = opt.consider_missing; fp.patfilt = opt.patfilt; fp.multiple_files = opt.multiple_files;
        return fp;
    }
    // the fused finish kernels of a launch on stream `s`, the heaviest clusters first
    int launch_fused_finish(pf::FinishParams fp, hipStream_t s, FinWork huge, FinWork large_m, FinWork large, FinWork small) {
        PFCHK(mark_begin(c, TimeCat::finish, s));      // (on the side stream too: finish_ms must not leave these launches out)
        const FinWork order[4] = {huge, large_m, large, small};
        for (int k = 0; k < 4; k++) {
            if (!order[k].n) continue;
            fp.work = order[k].work;
            const dim3 g(order[k].n);
            switch (k) {      // (the cases in this order keep the kernels' order in the device code object)
                case 0: hipLaunchKernelGGL((pf::finish_kernel<pf::FinHuge, true>), g, dim3(pf::FinHuge::THREADS), 0, s, fp); break;
                case 2: hipLaunchKernelGGL((pf::finish_kernel<pf::FinLarge, false>), g, dim3(pf::FinLarge::THREADS), 0, s, fp); break;
                case 3: hipLaunchKernelGGL((pf::finish_kernel<pf::FinSmall, false>), g, dim3(pf::FinSmall::THREADS), 0, s, fp); break;
                default: hipLaunchKernelGGL((pf::finish_kernel<pf::FinLargeM, true>), g, dim3(pf::FinLargeM::THREADS), 0, s, fp); break;
            }
            HIPCHK(hipGetLastError());
        }
        PFCHK(mark_end(c, s));
        return PF_OK;
    }
    // ---- output arenas: the next pass's, `cap` entries from the batch's next free index on
    int begin_arena(uint64_t cap) {
        while (c->arenas.size() <= arena_i) c->arenas.push_back(std::make_unique<Arena>());
        ar = c->arenas[arena_i].get();
        ar->cap = std::max<uint64_t>(cap, 1);
        ar->base = arena_base;
        PFCHK(ar->key.ensure((size_t)ar->cap * 8 * KW));
        PFCHK(ar->pid.ensure((size_t)ar->cap * 4));
        PFCHK(ar->first.ensure((size_t)ar->cap * 8));
        return PF_OK;
    }
    // the cursor's next free index restarts at the arena's base (a host-planned pass queues its item upload first)
    int upload_cursor_start() {
        c->pin_small.as<uint64_t>()[arena_i & 15] = arena_base;
        HIPCHK(hipMemcpyAsync(c->batch.cursor.p, c->pin_small.as<uint64_t>() + (arena_i & 15), 8, hipMemcpyHostToDevice, c->stream));
        return PF_OK;
    }
    // a pass not waited for: its cursor comes back with the last pass's results
    int defer_pass() {
        const uint32_t pin = 16 + (arena_i & 31);
        HIPCHK(hipMemcpyAsync(c->pin_small.as<uint64_t>() + pin, c->batch.cursor.p, 8, hipMemcpyDeviceToHost, c->stream));
        deferred.push_back(Deferred{ar, pin});
        arena_base += ar->cap;
        arena_i++;
        return PF_OK;
    }
    // what a waited-for pass wrote (`cursor`: the next free index it left)
    static int close_arena(Arena* a, uint64_t cursor) {
        a->used = cursor - a->base;
        if (a->used > a->cap) return fail(PF_ERR_CAPACITY, "output arena overflow (%llu > %llu)", (unsigned long long)a->used, (unsigned long long)a->cap);
        return PF_OK;
    }
    // ---- the device-planned clusters of part h: unit view, scan, fused finish -- launched from plan_kernel's 40-byte summary
    int launch_planned(uint32_t h) {
        const pf_ctx::DPlan& plan = c->dplan[h];
        const pf::PlanOut po = *plan.pin_out.as<pf::PlanOut>();
        const uint32_t n = po.n_items;
        if (!n) return PF_OK;
        if (n > c->max_items || n > plan.n || po.n_fin + po.n_fin2 + po.n_fin5 != n || po.n_unit > n)
            return fail(PF_ERR_STATE, "plan_kernel summary out of range (%u items of %u clusters)", n, plan.n);
        const DPtrs q = dplan_ptrs(plan);
        const uint32_t* zeros = c->dp_const.as<uint32_t>();
        const uint32_t* ones = zeros + c->dp_const_n;
        const uint32_t* iota = zeros + 2 * (size_t)c->dp_const_n;
        const pf::Items ip = planned_items(q.it_cluster, q.it_nslots, zeros, ones, iota);
        uint32_t* const count = plan.it_count.as<uint32_t>();
        PFCHK(begin_arena(po.arena_cap));
        PFCHK(upload_cursor_start());
        pf_ctx::UPool& up = c->upool[2 * h];
        if (po.n_unit) PFCHK(launch_unit_classes(up, po.n_unit, 0, po.unit_room, &q));
        PFCHK(mark_begin(c, TimeCat::scan));
        PFCHK(launch_scan(c, scan_params(ip, count, up, q.w_scan), n));
        PFCHK(mark_end(c));
        c->timing.scan_launches++;
        PFCHK(launch_fused_finish(finish_params(ip, count), c->stream, {q.w_fin5, po.n_fin5}, {nullptr, 0}, {q.w_fin2, po.n_fin2},
                                  {q.w_fin, po.n_fin}));
        c->timing.n_items += n;
        c->timing.n_device_planned += n;
        return defer_pass();
    }
    // A deduplicated cluster whose distinct sequences alone carry far more windows than one table holds will
    // overflow it: start it with two key partitions instead of paying for a failed first scan (a wrong guess
    // only costs time: an overflow still triggers the doubling retry)
    // Estimate of the distinct windows of D near-identical sequences of average length L = vinst / D: the first
    // contributes all of its windows, every further one the share a 1 % divergence touches (1 - 0.99^k: 27 % of the
    // 31-mers, 40 % of the 51-mers) plus a margin.
    uint32_t first_nparts(const pf::ClusterRec& cr) const {
        if (!cr.mode || !cr.vnstr) return 1;
        const double D = (double)cr.vnstr, L = (double)(cr.vinst * mult) / D;
        const double est = L * (1.0 + share * (D - 1.0));
        const double room = 0.9 * (double)pf::insert_limit(NS);
        // The estimate is right for SURVEY 8d's alleles, each with its own substitutions and flanks.  The many
        // alleles of a population descend from one another and share far more (tens of new k-mers each, not
        // hundreds): past 24 distinct sequences the cluster starts as ONE item instead, and if that overflows
        // the scan reports how far it came and the retry gets the partitions it needs.  A failed first attempt
        // costs 1/P of the P scans that follow; an over-partitioned cluster costs every surplus scan in full.
        // Once the context has scanned enough such clusters it knows what a further sequence brings in THIS
        // pangenome (the line through what it observed, plus a margin) and the first
        // attempt is sized by that.
        if (D >= 2.0 && fit.ready) {
            const double g = std::max(0.0, fit.a + fit.b * L) + fit.half_sd;      // (the line: see launch_plan)
            const double est2 = L + g * (D - 1.0);
            // (an estimate never asks for more items than a sub-batch holds: the cluster then starts with what
            // fits and an overflowing scan says how many partitions it really needs)
            if (est2 > room)
                return (uint32_t)std::min<double>(std::ceil(est2 / room), (double)std::min(4096u, std::max(1u, c->max_items / 2)));
        } else if (est > room) {
            return D > 24.0 ? 1u : (uint32_t)std::min<double>(std::ceil(est / room), (double)std::min(64u, std::max(1u, c->max_items / 2)));
        }
        return 1;
    }
    // ---- the first pass of part h: its dedup results (queued with the others up front) have to be here
    int begin_part(uint32_t h) {
        const uint32_t c0 = part_begin(h), c1 = part_end[h];
        HIPCHK(hipEventSynchronize(c->ev_part[h]));
        if (h == 0) lap("first part's dedup results");
        if (h == 0 && ex_on_device) {
            if (h_exfirst[C + 1]) {
                HIPCHK(hipStreamSynchronize(c->stream));
                return fail(PF_ERR_ARG, "extra_cluster must be non-decreasing and < n_clusters");
            }
            ex_first.assign(h_exfirst, h_exfirst + C + 1);
        }
        // the clusters plan_kernel laid out go first: the GPU starts on them while the rest of the part is built here
        const uint32_t planned_arena = arena_i;
        if (use_plan) PFCHK(launch_planned(h));
        PFCHK(retry_wide(c0, c1));
        for (uint32_t i = c0; i < c1; i++) {
            rec[i].mode &= 3u;
            if (rec[i].ninst * mult >= 0xFFFFFFF0ull) return fail(PF_ERR_ARG, "cluster %u has too many k-mer instances", i);
            total_inst += rec[i].ninst * mult;
            c->timing.n_dedup_clusters += rec[i].mode ? 1u : 0u;
            if (rec[i].pad & pf::PLAN_PLANNED) {                  // laid out by plan_kernel: one key partition
                const uint32_t nsi = (rec[i].pad >> pf::PLAN_NS_SHIFT) & 15u;
                note_route(i, (rec[i].pad >> pf::PLAN_CLS_SHIFT) & 15u, 1, nsi == 1 ? 4096u : nsi == 2 ? 6144u : NS);
                continue;
            }
            nparts[i] = first_nparts(rec[i]);
        }
        // the host-planned clusters' unit view.  A cluster's pieces number at most the units of its plain view: that is
        // its room in this part's pool.
        if (!(c->o.flags & PF_FLAG_NO_UNIT_DEDUP)) {
            pf_ctx::UPool& up = c->upool[2 * h + 1];
            PFCHK(up.pin.ensure((size_t)(c1 - c0) * 8 + 64));
            uint32_t nu = 0;
            uint64_t room = 0;
            uint32_t* lc = up.pin.as<uint32_t>();
            auto takes = [&](uint32_t i) { return !(rec[i].pad & pf::PLAN_PLANNED) && rec[i].mode && rec[i].vnstr >= 2 && rec[i].words && room + rec[i].words / 2 < 0x7FFFFFF0ull; };
            for (uint32_t i = c0; i < c1; i++)
                if (rec[i].vnstr <= pf::UNIT_SMALL_MAX_D && takes(i)) { lc[nu++] = i; room += rec[i].words / 2; }
            const uint32_t nsmall = nu;
            for (uint32_t i = c0; i < c1; i++)
                if (rec[i].vnstr > pf::UNIT_SMALL_MAX_D && takes(i)) { lc[nu++] = i; room += rec[i].words / 2; }
            uint32_t* lb = lc + nu;
            room = 0;
            for (uint32_t j = 0; j < nu; j++) { lb[j] = (uint32_t)room; room += rec[lc[j]].words / 2; }
            if (nu) PFCHK(launch_unit_classes(up, nsmall, nu - nsmall, room, nullptr));
        }
        lap("  prep (records, unit view)");
        todo.clear();
        for (uint32_t ci = c0; ci < c1; ci++) {
            if (!(rec[ci].pad & pf::PLAN_PLANNED)) { todo.push_back(ci); continue; }
            c->timing.scan_packed_bytes += rec[ci].words * 8;
            c->cluster_arena[ci] = planned_arena;
        }
        return PF_OK;
    }
    // which unit-view pool a cluster's view lies in: its part's device-planned one or the host-planned one
    uint32_t pool_of(uint32_t ci) const {
        uint32_t q = 0;
        while (q + 1 < P && ci >= part_end[q]) q++;
        return 2 * q + ((rec[ci].pad & pf::PLAN_PLANNED) ? 0u : 1u);
    }
    // ---- items of this pass: the todo clusters' key partitions and extra-row items, cut into sub-batches
    int build_items(Pass& ps) {
        HostPass& hpass = c->pass;
        const uint32_t lim_full = pf::insert_limit(NS);
        size_t room = 0;                   // (an item per key partition, and at most the slow-path items of the general path)
        for (uint32_t ci : todo) room += nparts[ci] + (ex_first[ci + 1] - ex_first[ci] + lim_full - 1) / lim_full;
        hpass.begin(room);
        Sub cur{0, 0, 0, 0, todo.empty() ? 0u : pool_of(todo[0]), 0, 0, 0};
        for (uint32_t ci : todo) {
            const uint32_t np = nparts[ci];
            const uint32_t nex = ex_first[ci + 1] - ex_first[ci];
            // a deduplicated cluster that is one work item (or a few key partitions) is finished by one fused kernel
            // (rows + emit in LDS); its slow-path rows (a few k-mers around an 'N') are folded in by that kernel
            const uint32_t mwords = rec[ci].vnstr * ((W + 3) & ~3u);
            uint8_t fused = 0;   // (SubmitScratch::fused)
            if (rec[ci].mode == 1 && nex <= pf::FUSED_MAX_EXTRA && NS <= 9600) {
                const bool fits_large = rec[ci].dense < pf::FinLarge::DW * 32 - 1 && mwords <= pf::FinLarge::MR;
                const bool fits_huge = rec[ci].dense < pf::FinHuge::DW * 32 - 1 && mwords <= pf::FinHuge::MR;
                if (np == 1) {
                    if (rec[ci].dense < pf::FinSmall::DW * 32 - 1 && mwords <= pf::FinSmall::MR) fused = 1;
                    else if (fits_large) fused = 2;
                    else if (fits_huge) fused = 5;
                } else if (fits_large) fused = 3;
                // (several partitions of a cluster that large stay on the general path, one workgroup each: the one
                // workgroup of the fused kernel took 15.9 ms where rows + emit + pattern rows take 4.5, 2 000 clusters
                // of 60 SURVEY alleles)
            }
            const uint32_t nex_items = fused ? 0 : (nex + lim_full - 1) / lim_full;
            const uint32_t nit = np + nex_items;
            if (nit > c->max_items) {
                if (c->max_items == 0) return fail(PF_ERR_STATE, "the context lost its scratch in a failed enlargement");
                // (sub-batches already built for this pass hold at most the old max_items items each: still valid)
                PFCHK(grow_scratch(c, nit));
            }
            const uint64_t qn = rec[ci].vinst * mult;          // entries of the cluster's queue at most (its view's windows)
            const uint32_t vch = (rec[ci].vnstr + 31) / 32;
            const bool binned = !(c->o.flags & PF_FLAG_NO_KEY_BINNING) && np >= BIN_MIN_PARTS && KW <= 2 && rec[ci].mode != 0 &&
                                vch <= pf::BIN_CHUNKS && (uint64_t)np * vch <= pf::BIN_CELLS && qn && qn <= BIN_MAX_ENTRIES;
            // (a launch reads one unit-view pool: a re-run pass does not mix the pools' clusters in a sub-batch)
            if (cur.nitems + nit > c->max_items || (cur.nitems && pool_of(ci) != cur.pool) ||
                (binned && cur.q_total + qn > BIN_MAX_ENTRIES)) {
                ps.subs.push_back(cur);
                cur = Sub{(uint32_t)hpass.n_items(), 0, (uint32_t)hpass.sub_cluster.h.size(), 0, pool_of(ci), (uint32_t)hpass.bin_cluster.size(), 0, 0};
            }
            if (!cur.nitems) cur.pool = pool_of(ci);
            const uint32_t sib0 = (uint32_t)hpass.n_items();
            // table size: a cluster that cannot overflow a small table gets one (less flush traffic)
            uint32_t ns = NS;
            const uint64_t inst = rec[ci].vinst * mult;
            if (np == 1 && NS > 4096 + pf::INSERT_SLACK && inst <= pf::insert_limit(4096)) ns = 4096;
            else if (np == 1 && NS > 6144 + pf::INSERT_SLACK && inst <= pf::insert_limit(6144)) ns = 6144;
            note_route(ci, fused, np, ns);
            for (uint32_t q = 0; q < np; q++)
                hpass.push(ci, q, np, ns, cur.nitems + q, sib0, nit, 0, 0, fused == 3 && q > 0 ? 4 : fused, binned ? 1u : 0u);
            if (binned) {
                hpass.bin_cluster.push_back(ci); hpass.bin_item0.push_back(sib0); hpass.bin_nparts.push_back(np);
                hpass.bin_base.push_back((uint32_t)cur.q_total);
                cur.q_total += qn; cur.nbin++;
                c->timing.n_binned_clusters++;
            }
            for (uint32_t q = 0; q < nex_items; q++) {
                const uint32_t first = ex_first[ci] + q * lim_full;
                const uint32_t cnt = std::min(lim_full, ex_first[ci + 1] - first);
                hpass.push(ci, 0, 1, cnt, cur.nitems + np + q, sib0, nit, first, 1, 0, 0);
            }
            for (uint32_t q = 0; q < np; q++) ps.arena_cap += std::min<uint64_t>(pf::insert_limit(ns), inst);
            ps.arena_cap += nex;
            if (!fused) {
                hpass.sub_cluster.h.push_back(ci); hpass.sub_item0.h.push_back(sib0); hpass.sub_nitems.h.push_back(nit);
                cur.ncl++;
            }
            cur.nitems += nit;
            c->cluster_arena[ci] = arena_i;
        }
        if (cur.nitems) ps.subs.push_back(cur);
        hpass.end(); lap("  items");
        return PF_OK;
    }
    // ---- the work lists of this pass; items and lists up in one staged copy
    int build_work_lists(Pass& ps) {
        HostPass& hpass = c->pass;
        const size_t NI = hpass.n_items();
        const uint32_t* const it_cl = hpass.col[hpass.it_cluster].h.data();
        const uint32_t* const it_extra = hpass.col[hpass.it_is_extra].h.data();
        for (Staged& l : hpass.list) { l.h.clear(); l.h.reserve(NI); }
        auto list = [&](HostPass::List l) -> std::vector<uint32_t>& { return hpass.list[l].h; };
        lap("  arena");
        for (DevBuf* v : {&hpass.it_count, &hpass.it_unique, &hpass.it_kept}) PFCHK(v->ensure(std::max<size_t>(NI, 1) * 4));
        // work lists per sub-batch, concatenated; heaviest items first inside each launch (the grid then drains evenly):
        // a coarse O(n) order by log2(scan instances) is enough
        ps.off.assign(ps.subs.size() + 1, SubLists{});
        auto wclass = [&](uint32_t it) -> int {
            const uint64_t w = rec[it_cl[it]].vinst;
            return w ? 63 - __builtin_clzll(w) : 0;
        };
        std::vector<uint32_t> tmp_scan, tmp_fin, tmp_fin2;
        auto append_by_weight = [&](std::vector<uint32_t>& src, std::vector<uint32_t>& dst) {
            if (src.size() > 64) {
                size_t cnt[65] = {0};
                for (uint32_t it : src) cnt[64 - wclass(it)]++;
                size_t run = dst.size();
                for (int b = 0; b < 65; b++) { const size_t n = cnt[b]; cnt[b] = run; run += n; }
                dst.resize(run);
                for (uint32_t it : src) dst[cnt[64 - wclass(it)]++] = it;
            } else {
                dst.insert(dst.end(), src.begin(), src.end());
            }
            src.clear();
        };
        for (size_t s = 0; s < ps.subs.size(); s++) {
            for (uint32_t i = ps.subs[s].item0; i < ps.subs[s].item0 + ps.subs[s].nitems; i++) {
                if (it_extra[i]) list(hpass.work_extra).push_back(i); else tmp_scan.push_back(i);
                if (hpass.fused[i] == 1) tmp_fin.push_back(i);
                else if (hpass.fused[i] == 2) tmp_fin2.push_back(i);
                else if (hpass.fused[i] == 3) list(hpass.work_fin3).push_back(i);
                else if (hpass.fused[i] == 5) list(hpass.work_fin5).push_back(i);
                else if (hpass.fused[i] == 0) list(hpass.work_rows).push_back(i);
            }
            append_by_weight(tmp_scan, list(hpass.work_scan));
            append_by_weight(tmp_fin, list(hpass.work_fin));
            append_by_weight(tmp_fin2, list(hpass.work_fin2));
            for (int l = 0; l < HostPass::N_LISTS; l++) ps.off[s + 1].at[l] = (uint32_t)hpass.list[l].h.size();
        }
        ps.NB = hpass.bin_cluster.size();      // the four lists of the binned clusters travel as one block
        if (ps.NB) {
            std::vector<uint32_t>& block = hpass.bin_block.h;
            for (auto* v : {&hpass.bin_cluster, &hpass.bin_item0, &hpass.bin_nparts, &hpass.bin_base}) block.insert(block.end(), v->begin(), v->end());
            PFCHK(c->q_off.ensure(NI * (pf::BIN_CHUNKS + 1) * 4));
        }
        lap("  work lists");
        return staged_upload(c, hpass.staged());
    }
    // ---- sub-batch s of a host-planned pass: extra-row fill, (bin and) scan, the fused finish beside or in line, then
    // the general path: rows -> cluster base (+ bitmap merge) -> emit -> pattern rows
    int launch_sub_batch(const Pass& ps, size_t s) {
        const Sub& sb = ps.subs[s];
        const SubLists &o0 = ps.off[s], &o1 = ps.off[s + 1];
        const HostPass& hpass = c->pass;
        uint32_t* const it_count = hpass.it_count.as<uint32_t>();
        FinWork w[HostPass::N_LISTS];         // this sub-batch's stretch of every work list
        for (int l = 0; l < HostPass::N_LISTS; l++) w[l] = FinWork{hpass.list[l].d.as<uint32_t>() + o0.at[l], o1.at[l] - o0.at[l]};
        const FinWork w_scan = w[hpass.work_scan], w_extra = w[hpass.work_extra], w_rows = w[hpass.work_rows];
        const uint32_t n_scan = w_scan.n, n_rows = w_rows.n;
        if (w_extra.n) {
            pf::ExtraParams ep{};
            ep.vf = view_facts(); ep.items = hpass.items(); ep.dump = slot_dump(it_count); ep.opt = row_opts();
            ep.work = w_extra.work;
            PFCHK(mark_begin(c, TimeCat::emit));
            hipLaunchKernelGGL(pf::extra_fill_kernel, dim3(w_extra.n), dim3(256), 0, c->stream, ep);
            HIPCHK(hipGetLastError());
            PFCHK(mark_end(c));
        }
        if (n_scan) {
            pf::ScanParams sp = scan_params(hpass.items(), it_count, c->upool[sb.pool], w_scan.work);
            PFCHK(mark_begin(c, TimeCat::scan));
            if (sb.nbin) {
                const size_t qcap = (size_t)sb.q_total + 64, NB = ps.NB;
                PFCHK(c->q_key.ensure(qcap * 8 * KW)); PFCHK(c->q_ord.ensure(qcap * 4)); PFCHK(c->q_bit.ensure(qcap * 4));
                sp.q_key = c->q_key.as<uint64_t>(); sp.q_ord = c->q_ord.as<uint32_t>(); sp.q_bit = c->q_bit.as<uint32_t>();
                sp.q_stride = qcap; sp.q_off = c->q_off.as<uint32_t>();
                const uint32_t* const bin = hpass.bin_block.d.as<uint32_t>() + sb.bin0;
                sp.bin_cluster = bin; sp.bin_item0 = bin + NB; sp.bin_nparts = bin + 2 * NB; sp.bin_base = bin + 3 * NB;
                PFCHK(launch_bin(c, sp, sb.nbin));
            }
            PFCHK(launch_scan(c, sp, n_scan));
            PFCHK(mark_end(c));
            c->timing.scan_launches++;
        }
        // A launch whose fused-finish workgroups do not fill the GPU while general-path items wait behind them (a batch
        // of many-allele clusters with a few dozen simple ones: two 1 024-thread workgroups took 0.4 ms each with the
        // other 250 CUs idle; any batch of a few hundred clusters): the finish kernels go to the context's second
        // stream and run BESIDE rows / emit / pattern rows -- they share nothing but atomically claimed output room
        // and the run-global pattern table.  (Not for full launches: two latency-bound kernels that each fill the GPU
        // take each other's wave slots -- five such pairings lost in rounds 2-3.)
        const FinWork w_fin = w[hpass.work_fin], w_fin2 = w[hpass.work_fin2], w_fin3 = w[hpass.work_fin3], w_fin5 = w[hpass.work_fin5];
        const uint32_t n_fused_wg = w_fin.n + w_fin2.n + w_fin3.n + w_fin5.n;
        const bool beside = n_fused_wg && n_rows && n_fused_wg <= 2u * (uint32_t)c->n_cu;
        if (n_fused_wg) {
            hipStream_t fs = c->stream;
            if (beside) {
                HIPCHK(hipEventRecord(c->ev_fork, c->stream));
                HIPCHK(hipStreamWaitEvent(c->side, c->ev_fork, 0));
                fs = c->side;
                c->timing.n_side_launches++;
            }
            PFCHK(launch_fused_finish(finish_params(hpass.items(), it_count), fs, w_fin5, w_fin3, w_fin2, w_fin));
            if (beside) HIPCHK(hipEventRecord(c->ev_join, c->side));
        }
        if (!n_rows) return PF_OK;
        // the general path's four kernels read the same groups (nothing between here and the last launch resizes a buffer)
        const pf::CallerSegs cl = caller_segs();
        const pf::ViewFacts vf = view_facts();
        const pf::Items items = hpass.items();
        const pf::SlotDump dump = slot_dump(it_count);
        const pf::RowScratch rs = row_scratch();
        const pf::Outputs out = outputs();
        const pf::RowOpts opt = row_opts();
        const uint32_t* const work = w_rows.work;
        pf::RowsParams rp{};
        rp.cl = cl; rp.vf = vf; rp.items = items; rp.dump = dump; rp.rs = rs; rp.opt = opt; rp.work = work;
        PFCHK(mark_begin(c, TimeCat::rows));
        hipLaunchKernelGGL(pf::rows_kernel, dim3(n_rows), dim3(pf::ROWS_THREADS), 0, c->stream, rp);
        HIPCHK(hipGetLastError());
        PFCHK(mark_end(c));

        pf::BaseParams bp{};
        bp.sub_cluster = hpass.sub_cluster.d.as<uint32_t>() + sb.cl0;
        bp.cluster_item0 = hpass.sub_item0.d.as<uint32_t>() + sb.cl0;
        bp.cluster_nitems = hpass.sub_nitems.d.as<uint32_t>() + sb.cl0;
        bp.vf = vf; bp.rs = rs; bp.out = out;
        bp.n = sb.ncl;
        PFCHK(mark_begin(c, TimeCat::emit));
        hipLaunchKernelGGL(pf::cluster_base_kernel, dim3(1), dim3(1024), 0, c->stream, bp);
        HIPCHK(hipGetLastError());
        if (sb.nitems > sb.ncl) {     // some cluster of this sub-batch has several items
            pf::BitmapMergeParams bm{};
            bm.sub_cluster = bp.sub_cluster; bm.cluster_item0 = bp.cluster_item0; bm.cluster_nitems = bp.cluster_nitems;
            bm.vf = vf; bm.items = items; bm.rs = rs;
            hipLaunchKernelGGL(pf::bitmap_merge_kernel, dim3(sb.ncl), dim3(256), 0, c->stream, bm);
            HIPCHK(hipGetLastError());
        }

        pf::EmitParams em{};
        em.cl = cl; em.vf = vf; em.items = items; em.dump = dump; em.rs = rs; em.out = out; em.pt = c->pt; em.opt = opt;
        em.work = work;
        hipLaunchKernelGGL(pf::emit_kernel, dim3(n_rows), dim3(pf::EMIT_THREADS), 0, c->stream, em);
        HIPCHK(hipGetLastError());
        PFCHK(mark_end(c));
        PFCHK(mark_begin(c, TimeCat::pattern_rows));

        pf::PatRowsParams pr{};
        pr.cl = cl; pr.vf = vf; pr.items = items; pr.dump = dump; pr.rs = rs; pr.out = out; pr.pt = c->pt;
        pr.pats = pattern_pool(); pr.opt = opt; pr.work = work;
        hipLaunchKernelGGL(pf::pattern_rows_kernel, dim3(n_rows), dim3(pf::PR_THREADS), 0, c->stream, pr);
        HIPCHK(hipGetLastError());
        PFCHK(mark_end(c));
        if (beside) HIPCHK(hipStreamWaitEvent(c->stream, c->ev_join, 0));   // the next sub-batch takes the scratch slices over
        return PF_OK;
    }
    // ---- the pass waited for (the last part's, or a re-run): who overflowed?  Read-back, learning, the next pass's clusters
    int finish_pass(const Pass& ps, uint32_t pass, bool rerun) {
        SubmitScratch& hs = c->hs;
        const HostPass& hpass = c->pass;
        const size_t NI = hpass.n_items();
        PFCHK(c->pin_ovf.ensure((size_t)C * 4 + 64));
        uint32_t* const ovf = c->pin_ovf.as<uint32_t>();
        uint64_t* const cur3 = c->pin_small.as<uint64_t>() + 48;
        uint32_t* const cnt_pin = reinterpret_cast<uint32_t*>(c->pin_small.as<uint64_t>() + 52);
        // clusters of this pass the key-partition estimate can learn from: their items' key counts come along
        bool learn = false;
        // (8 192 clusters settle the line; after that every 16th submit still looks, at half the old weight, so that a
        // pangenome whose later clusters differ from its first is followed -- the read-back is not free)
        // (not in the re-run of a batch after the pattern table grew: its clusters have been counted)
        uint32_t learn_planned = 0;            // ... and plan_kernel's items of the last part (their clusters, their key counts)
        if (!rerun && (c->part_model.n < 8192 || (c->n_submits & 15) == 0)) {
            for (uint32_t ci : todo) if (rec[ci].mode && rec[ci].vnstr >= 2) { learn = true; break; }
            if (use_plan && pass + 1 == P) learn_planned = std::min<uint32_t>(c->dplan[pass].pin_out.as<pf::PlanOut>()->n_items, 4096u);
        }
        if (learn) {
            hs.count.resize(NI);
            HIPCHK(hipMemcpyAsync(hs.count.data(), hpass.it_count.p, NI * 4, hipMemcpyDeviceToHost, c->stream));
        }
        if (learn_planned) {
            hs.plan.resize(2 * (size_t)learn_planned);
            HIPCHK(hipMemcpyAsync(hs.plan.data(), dplan_ptrs(c->dplan[pass]).it_cluster, (size_t)learn_planned * 4, hipMemcpyDeviceToHost, c->stream));
            HIPCHK(hipMemcpyAsync(hs.plan.data() + learn_planned, c->dplan[pass].it_count.p, (size_t)learn_planned * 4, hipMemcpyDeviceToHost, c->stream));
        }
        HIPCHK(hipMemcpyAsync(ovf, c->batch.cl_overflow.p, (size_t)C * 4, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(hipMemcpyAsync(cur3, c->batch.cursor.p, 24, hipMemcpyDeviceToHost, c->stream));
        // (the pattern counters come along: when this was the last pass the MD5 launch needs no round trip of its own)
        HIPCHK(hipMemcpyAsync(cnt_pin, c->pt_counters.p, 12, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(hipStreamSynchronize(c->stream));
        cnt2[0] = cnt_pin[0]; cnt2[1] = cnt_pin[1]; cnt2[2] = cnt_pin[2];
        c->counters.n_unique = cur3[1]; c->counters.n_kept = cur3[2];
        lap("sync pass");
        PFCHK(close_arena(ar, cur3[0]));
        arena_base += ar->cap;
        arena_i++;
        if (!deferred.empty()) {                   // the earlier passes finished before this one
            for (const Deferred& df : deferred) PFCHK(close_arena(df.ar, c->pin_small.as<uint64_t>()[df.pin]));
            deferred.clear();
            todo.resize(C);                        // every cluster has been through its first pass now
            std::iota(todo.begin(), todo.end(), 0u);
        }
        if (learn || learn_planned) {
            PartModel& m = c->part_model;
            if (m.n >= 8192) m.halve();
            uint32_t looked = 0;               // (the GPU waits while this runs: a few thousand clusters say enough)
            // a cluster that did not overflow: what each of its further distinct sequences brought in
            auto look = [&](uint32_t ci, uint64_t keys) {
                if (ovf[ci] || !rec[ci].mode || rec[ci].vnstr < 2 || !rec[ci].vinst) return;
                looked++;
                const double D = (double)rec[ci].vnstr, L = (double)(rec[ci].vinst * mult) / D;
                m.add(L, std::max(0.0, ((double)keys - L) / (D - 1.0)));
            };
            for (uint32_t i = 0; i < learn_planned && looked < 4096; i++)
                if (hs.plan[i] < C) look(hs.plan[i], hs.plan[learn_planned + i]);
            auto col = [&](HostPass::Col k) { return hpass.col[k].h.data(); };
            if (learn)
                for (size_t i = 0; i < NI && looked < 4096; i++) {
                    if (col(hpass.it_is_extra)[i] || col(hpass.it_part)[i] != 0) continue;
                    uint64_t keys = 0;
                    for (uint32_t q = 0; q < col(hpass.it_nparts)[i]; q++) keys += hs.count[i + q];
                    look(col(hpass.it_cluster)[i], keys);
                }
        }
        std::vector<uint32_t> next;
        for (uint32_t ci : todo)
            if (ovf[ci]) {
                next.push_back(ci);
                // ovf = 64 * (the item's units / the units scanned when its table was full): that many times the keys
                // of one partition are to be expected (an overestimate: a cluster's first sequence brings more new keys
                // than its later ones), and key hashing spreads them evenly: a small margin is enough
                // (a view of distinct sequences only: among the copies of an every-copy cluster new keys stop coming
                // early and nothing can be extrapolated -- those double, as does a cluster that asks for more than 16x)
                double want = std::ceil((double)nparts[ci] * ((double)ovf[ci] / 64.0) * 1.06);
                if (!rec[ci].mode || want > 16.0 * nparts[ci]) want = 2.0 * nparts[ci];
                nparts[ci] = (uint32_t)std::min<double>(std::max<double>(want, (double)nparts[ci] + 1.0), 65537.0);
                if (nparts[ci] > 65536) return fail(PF_ERR_CAPACITY, "cluster %u does not fit 65536 key partitions", ci);
            }
        if (!next.empty()) {
            c->timing.n_retried += (uint32_t)next.size();
            HIPCHK(hipMemsetAsync(c->batch.cl_overflow.p, 0, (size_t)std::max(C, 1u) * 4, c->stream));
        }
        todo.swap(next);
        return PF_OK;
    }
    // ---- MD5 of the patterns this batch created, ids [pid0, pid1)
    int launch_md5(uint32_t pid1) {
        pf::Md5Params mp{};
        mp.pats = pattern_pool(); mp.pat_md5 = c->pats.md5.as<uint8_t>();
        mp.pid0 = c->pid0; mp.pid1 = pid1; mp.W = W; mp.range = nullptr;
        // int64 rows are the clusters' own rows: the int pass goes by cluster (cl_pattern) and runs BESIDE the float pass, on
        // the side stream, instead of behind it
        mp.cluster_pattern = c->batch.cl_pattern.as<uint32_t>(); mp.n_clusters = C;
        PFCHK(mark_begin(c, TimeCat::md5));
        // A small launch is spread over the chip: the float pass's workgroups (four waves, one per SIMD) number a few per
        // CU, and the dispatcher fills CUs with up to eight before it moves on -- a SIMD gets through its rows at one rate
        // however many waves share it, so the pass took as long as the FULLEST SIMD (a rank's share of configs[3]: 5 waves
        // per SIMD on average, 8 on two thirds of the CUs, none on the rest).  Dynamic LDS the kernel never touches caps the
        // workgroups per CU at what an even spread needs.
        const uint32_t n_float = (pid1 - c->pid0 + pf::MD5_THREADS - 1) / pf::MD5_THREADS;
        const uint32_t per_cu = (n_float + (uint32_t)c->n_cu - 1) / (uint32_t)c->n_cu;
        uint32_t lds_cap = 0;
        if (per_cu < 8) lds_cap = std::min<uint32_t>(64u << 10, ((160u << 10) / std::max(per_cu, 1u)) & ~1023u);
        const dim3 g_float(n_float);
        const dim3 g_int(std::min<uint32_t>((C + pf::MD5_THREADS - 1) / pf::MD5_THREADS, 1024u));
        HIPCHK(hipEventRecord(c->ev_fork, c->stream));
        HIPCHK(hipStreamWaitEvent(c->side, c->ev_fork, 0));
        if (mp.pats.pat_nan) {
            hipLaunchKernelGGL((pf::md5_kernel<false, true>), g_int, dim3(pf::MD5_THREADS), 0, c->side, mp);
            HIPCHK(hipGetLastError());
            hipLaunchKernelGGL((pf::md5_kernel<true, true>), g_float, dim3(pf::MD5_THREADS), lds_cap, c->stream, mp);
        } else {
            hipLaunchKernelGGL((pf::md5_kernel<false, false>), g_int, dim3(pf::MD5_THREADS), 0, c->side, mp);
            HIPCHK(hipGetLastError());
            hipLaunchKernelGGL((pf::md5_kernel<true, false>), g_float, dim3(pf::MD5_THREADS), lds_cap, c->stream, mp);
        }
        HIPCHK(hipGetLastError());
        HIPCHK(hipEventRecord(c->ev_join, c->side));
        HIPCHK(hipStreamWaitEvent(c->stream, c->ev_join, 0));
        PFCHK(mark_end(c));
        return PF_OK;
    }
    // ---- timing (both streams have drained) and the batch's results, which become the context's
    int publish_batch(uint32_t pid1, pf_result* counters) {
        HIPCHK(hipEventElapsedTime(&c->timing.total_ms, c->ev_t0, c->ev_t1));
        for (auto& e : c->events) {
            float ms = 0;
            HIPCHK(hipEventElapsedTime(&ms, e.a, e.b));
            switch (e.cat) {
                case TimeCat::scan: c->timing.scan_ms += ms; break;
                case TimeCat::rows: c->timing.rows_ms += ms; break;
                case TimeCat::emit: c->timing.emit_ms += ms; break;
                case TimeCat::dedup: c->timing.dedup_ms += ms; break;
                case TimeCat::pattern_rows: c->timing.patrows_ms += ms; break;
                case TimeCat::md5: c->timing.md5_ms += ms; break;
                case TimeCat::finish: c->timing.finish_ms += ms; break;
            }
        }
        c->n_clusters = C; c->last = d; c->last_nseg = NSEG;
        c->last_words = gth ? gth->n_words : b->n_words;
        if (!c->n_strand_words) c->last.seg_strand_off = nullptr;
        c->ts.kept = 0; c->ts.flight.valid = false;
        pf_result res{};
        res.n_instances = total_inst; res.n_unique = c->counters.n_unique; res.n_kept = c->counters.n_kept;   // (the last pass's cursor)
        res.n_new_patterns = pid1 - c->pid0; res.n_patterns = pid1; res.W = W; res.key_words = KW;
        c->counters = res;
        c->have_batch = true;
        c->h_strand_fresh = false;
        if (counters) *counters = c->counters;
        return PF_OK;
    }
};

int submit_once(pf_ctx* c, const pf_batch* b, const pf_gather* gth, pf_result* counters, uint64_t* need, bool rerun) {
    c->have_batch = false;
    c->kt.have_seq_end = false;
    c->passing.have_names = false;
    c->passing.index_slots = 0;
    ts_end(c);                            // a stream of the batch before, of either text, is over
    // whatever way this call ends, nothing it queued is still reading the caller's arrays or the pinned staging
    // blocks afterwards (the successful path has waited already; an error return may come with work in flight)
    struct Drain { hipStream_t s, s2; ~Drain() { (void)hipStreamSynchronize(s2); (void)hipStreamSynchronize(s); } } drain{c->stream, c->side};
    if (b->n_segs && (!b->packed || !b->seg_word_off || !b->seg_len || !b->seg_sample || !b->seg_ord_base))
        return fail(PF_ERR_ARG, "segment arrays missing");
    if (b->n_clusters && (!b->cluster_seg_off || !b->cluster_nstrains || !b->cluster_npresab || !b->cluster_presab ||
                          !b->cluster_ordinal))
        return fail(PF_ERR_ARG, "cluster arrays missing");
    if (b->n_extra && (!b->extra_cluster || !b->extra_ord || !b->extra_bits))
        return fail(PF_ERR_ARG, "extra arrays missing");
    for (auto& e : c->events) { c->ev_pool.push_back(std::move(e.a)); c->ev_pool.push_back(std::move(e.b)); }
    c->events.clear();
    c->timing = pf_timing{};
    SubmitRun r(c, b, gth);
    HIPCHK(hipEventRecord(c->ev_t0, c->stream));

    PFCHK(r.upload_batch());
    PFCHK(r.ensure_batch_outputs());
    PFCHK(r.launch_dedup_parts());
    r.lap("upload+dedup launch");

    c->pid0 = c->n_patterns;
    if (!rerun) c->n_submits++;
    c->cluster_arena.assign(r.C, 0);
    c->routes.assign(r.C, pf_ctx::Route{});
    r.nparts.assign(r.C, 1);
    c->counters = pf_result{};
    // host-planned passes: the parts' (what plan_kernel left of them, queued back to back), then the re-runs
    for (uint32_t pass = 0;; pass++) {
        c->stage_slot = (int)(pass & 1);
        if (pass < r.P) PFCHK(r.begin_part(pass));
        if (r.todo.empty() && pass >= r.P) break;
        Pass ps;
        PFCHK(r.build_items(ps));
        PFCHK(r.begin_arena(ps.arena_cap));
        PFCHK(r.build_work_lists(ps));
        PFCHK(r.upload_cursor_start());
        r.lap("upload items");
        for (size_t s = 0; s < ps.subs.size(); s++) PFCHK(r.launch_sub_batch(ps, s));
        c->timing.n_items += (uint32_t)c->pass.n_items();
        for (uint32_t ci : r.todo) c->timing.scan_packed_bytes += r.rec[ci].words * 8 * r.nparts[ci];
        r.lap("launch pass");
        if (pass + 1 < r.P) {
            PFCHK(r.defer_pass());   // no wait: the next part's pass is built now and goes in behind this one
            continue;
        }
        PFCHK(r.finish_pass(ps, pass, rerun));
        if (r.todo.empty()) break;
    }
    for (size_t a = r.arena_i; a < c->arenas.size(); a++) c->arenas[a]->used = 0;   // arenas of an earlier, longer batch
    c->n_passes = r.arena_i;

    // ---- MD5 of the patterns this batch created (cnt2: read with the last pass's results)
    if (!r.C) {
        HIPCHK(hipMemcpyAsync(r.cnt2, c->pt_counters.p, 12, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(hipStreamSynchronize(c->stream));
    }
    if (r.cnt2[2]) return fail(PF_ERR_CAPACITY, "output arena overflow inside a kernel");
    if (r.cnt2[1] || r.cnt2[0] > c->pt.pool) { *need = r.cnt2[0]; return PF_RETRY_PATTERNS; }
    const uint32_t pid1 = r.cnt2[0];
    if (pid1 > c->pid0) PFCHK(r.launch_md5(pid1));
    c->n_patterns = pid1;
    HIPCHK(hipEventRecord(c->ev_t1, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    r.lap("md5 + final sync");
    return r.publish_batch(pid1, counters);
}
}  // namespace

int pf_submit(pf_ctx* c, const pf_batch* b, pf_result* counters) {
    if (!c || !b) return fail(PF_ERR_ARG, "null argument");
    HIPCHK(hipSetDevice(c->device));
    const pf_gather* gth = c->pending_gather;
    c->pending_gather = nullptr;
    if (c->o.multiple_files) {
        // the pattern set starts empty in every cluster (panfeed.py:165) and ids are salted by the cluster ordinal:
        // nothing of an earlier batch can ever be matched again
        PFCHK(reset_patterns(c));
    } else if (c->pt_stale) {
        return fail(PF_ERR_STATE, "the pattern table holds entries of a batch that failed while it was being enlarged; "
                                  "pf_reset_patterns (a new run) first");
    } else if ((uint64_t)c->n_patterns * 2 > c->pt.pool && c->pregrow_failed_pool != c->pt.pool) {
        // ahead of need: a re-run costs a whole batch.  No batch has failed here, so a growth that does not succeed
        // (out of memory with both tables resident) leaves a table that is whole: carry on with it -- and do not try
        // again at this pool size (every try is an allocation, a fill and a free of the larger table): the next
        // growth is the one a batch that really runs out of ids asks for.
        const int rc = grow_patterns(c, (uint64_t)c->n_patterns * 2);
        if (rc == PF_ERR_OOM) { c->pregrow_failed_pool = c->pt.pool; g_err.clear(); }
        else if (rc != PF_OK) return rc;
    }
    const uint64_t submits0 = c->n_submits;
    for (int attempt = 0;; attempt++) {
        uint64_t need = 0;
        const int rc = submit_once(c, b, gth, counters, &need, attempt > 0);
        if (rc != PF_RETRY_PATTERNS) return rc;
        int rg = attempt >= 8 ? fail(PF_ERR_CAPACITY, "pattern table still too small after %d enlargements", attempt)
                              : grow_patterns(c, std::max<uint64_t>(need, (uint64_t)c->pt.pool + 1));
        if (rg != PF_OK) {
            // the failed batch's patterns are still in the table; the batch itself does not count as submitted
            c->pt_stale = true;
            c->n_submits = submits0;
            c->timing = pf_timing{};
            return rg;
        }
    }
}

int pf_debug_limit_pattern_slots(pf_ctx* c, uint64_t max_slots) {
    if (!c) return fail(PF_ERR_ARG, "null context");
    c->pt_slot_limit = max_slots;
    c->pregrow_failed_pool = 0;
    return PF_OK;
}

int pf_debug_limit_alloc(uint64_t max_bytes, uint64_t stats[2]) {
    if (stats) {
        stats[0] = g_alloc_max_request.exchange(0);
        stats[1] = g_alloc_exact_retries.exchange(0);
    }
    g_alloc_limit.store(max_bytes);
    return PF_OK;
}

int pf_debug_read_words(pf_ctx* c, int which, uint64_t first, uint64_t n, uint64_t* out) {
    if (!c || (n && !out)) return fail(PF_ERR_ARG, "pf_debug_read_words: null argument");
    if (which != 0 && which != 1) return fail(PF_ERR_ARG, "pf_debug_read_words: which must be 0 (genome store) or 1 (packed segments)");
    if (which == 1 && !c->have_batch) return fail(PF_ERR_STATE, "pf_debug_read_words without a successful pf_submit");
    HIPCHK(hipSetDevice(c->device));
    HIPCHK(hipStreamSynchronize(c->stream));
    const uint64_t bound = which == 0 ? c->g_words : c->last_words;
    const uint64_t* src = which == 0 ? c->g_store.as<uint64_t>() : c->last.packed;
    if (first > bound || n > bound - first) return fail(PF_ERR_ARG, "pf_debug_read_words: words [%llu, +%llu) outside the %llu held",
                                                        (unsigned long long)first, (unsigned long long)n, (unsigned long long)bound);
    if (n) HIPCHK(hipMemcpy(out, src + first, (size_t)n * 8, hipMemcpyDeviceToHost));
    return PF_OK;
}

int pf_debug_cluster_routes(pf_ctx* c, uint32_t n_clusters, uint8_t* route, uint32_t* nparts, uint32_t* nslots, uint32_t* attempts) {
    if (!c) return fail(PF_ERR_ARG, "pf_debug_cluster_routes: null context");
    if (!c->have_batch) return fail(PF_ERR_STATE, "pf_debug_cluster_routes without a successful pf_submit");
    if (n_clusters != c->n_clusters || c->routes.size() != n_clusters)
        return fail(PF_ERR_ARG, "pf_debug_cluster_routes: %u clusters asked for, the last batch had %u", n_clusters, c->n_clusters);
    for (uint32_t i = 0; i < n_clusters; i++) {
        const pf_ctx::Route& rt = c->routes[i];
        if (route) route[i] = (uint8_t)((rt.cls & 7u) | ((rt.mode & 3u) << 3) | ((rt.first & 7u) << 5));
        if (nparts) nparts[i] = rt.nparts;
        if (nslots) nslots[i] = rt.nslots;
        if (attempts) attempts[i] = rt.attempts;
    }
    return PF_OK;
}

int pf_get_timing(pf_ctx* c, pf_timing* t) {
    if (!c || !t) return fail(PF_ERR_ARG, "null argument");
    *t = c->timing;
    t->n_scratch_grown = c->n_scratch_grown;
    return PF_OK;
}

namespace {
// used_strand bits of the last submit's target windows (strand_bits_kernel) to the host, once per batch
int fetch_strand_bits(pf_ctx* c) {
    if (c->h_strand_fresh) return PF_OK;
    c->h_strand.resize((size_t)c->n_strand_words);
    if (c->n_strand_words)
        HIPCHK(hipMemcpy(c->h_strand.data(), c->strand_bits.p, (size_t)c->n_strand_words * 8, hipMemcpyDeviceToHost));
    c->h_strand_fresh = true;
    return PF_OK;
}
}  // namespace

int pf_fetch(pf_ctx* c, pf_result* res) {
    if (!c || !res) return fail(PF_ERR_ARG, "null argument");
    if (!c->have_batch) return fail(PF_ERR_STATE, "pf_fetch without a successful pf_submit");
    HIPCHK(hipSetDevice(c->device));
    const uint32_t C = c->n_clusters, W = c->W, KW = (uint32_t)c->KW;
    c->h_kmer_off.resize(C); c->h_kmer_cnt.resize(C); c->h_cl_pattern.resize(C); c->h_cl_unique.resize(C);
    if (C) {
        HIPCHK(hipMemcpy(c->h_kmer_off.data(), c->batch.cl_kmer_off.p, (size_t)C * 8, hipMemcpyDeviceToHost));
        HIPCHK(hipMemcpy(c->h_kmer_cnt.data(), c->batch.cl_kmer_cnt.p, (size_t)C * 4, hipMemcpyDeviceToHost));
        HIPCHK(hipMemcpy(c->h_cl_pattern.data(), c->batch.cl_pattern.p, (size_t)C * 4, hipMemcpyDeviceToHost));
        HIPCHK(hipMemcpy(c->h_cl_unique.data(), c->batch.cl_unique.p, (size_t)C * 4, hipMemcpyDeviceToHost));
    }
    // concatenate the used prefixes of the arenas; remap cluster offsets
    uint64_t total = 0;
    std::vector<uint64_t> host_base(c->arenas.size(), 0);
    for (size_t a = 0; a < c->arenas.size(); a++) { host_base[a] = total; total += c->arenas[a]->used; }
    c->h_kmer_key.resize((size_t)total * KW);
    c->h_kmer_pid.resize((size_t)total);
    for (size_t a = 0; a < c->arenas.size(); a++) {
        const Arena* ar = c->arenas[a].get();
        if (!ar->used) continue;
        HIPCHK(hipMemcpy(c->h_kmer_key.data() + host_base[a] * KW, ar->key.p, (size_t)ar->used * 8 * KW, hipMemcpyDeviceToHost));
        HIPCHK(hipMemcpy(c->h_kmer_pid.data() + host_base[a], ar->pid.p, (size_t)ar->used * 4, hipMemcpyDeviceToHost));
    }
    for (uint32_t i = 0; i < C; i++) {
        const uint32_t a = c->cluster_arena[i];
        if (c->h_kmer_cnt[i]) c->h_kmer_off[i] = c->h_kmer_off[i] - c->arenas[a]->base + host_base[a];
        else c->h_kmer_off[i] = 0;
    }
    // pattern pool: extend the host mirror by the patterns of this batch
    const uint32_t p0 = c->pid0, p1 = c->n_patterns;
    c->h_pat_bits.resize((size_t)p1 * W); c->h_pat_n.resize(p1); c->h_pat_md5.resize((size_t)p1 * 16);
    c->h_first_seen.resize(p1);
    if (c->o.consider_missing) c->h_pat_nan.resize((size_t)p1 * W);
    if (p1 > p0) {
        const size_t n = p1 - p0;
        HIPCHK(hipMemcpy(c->h_pat_bits.data() + (size_t)p0 * W, c->pats.bits.as<uint32_t>() + (size_t)p0 * W, n * W * 4, hipMemcpyDeviceToHost));
        HIPCHK(hipMemcpy(c->h_pat_n.data() + p0, c->pats.n.as<uint32_t>() + p0, n * 4, hipMemcpyDeviceToHost));
        HIPCHK(hipMemcpy(c->h_pat_md5.data() + (size_t)p0 * 16, c->pats.md5.as<uint8_t>() + (size_t)p0 * 16, n * 16, hipMemcpyDeviceToHost));
        HIPCHK(hipMemcpy(c->h_first_seen.data() + p0, c->pt.first_seen + p0, n * 8, hipMemcpyDeviceToHost));
        if (c->o.consider_missing)
            HIPCHK(hipMemcpy(c->h_pat_nan.data() + (size_t)p0 * W, c->pats.nan.as<uint32_t>() + (size_t)p0 * W, n * W * 4, hipMemcpyDeviceToHost));
    }
    c->h_new_pid.resize(p1 - p0);
    std::iota(c->h_new_pid.begin(), c->h_new_pid.end(), p0);
    std::sort(c->h_new_pid.begin(), c->h_new_pid.end(),
              [&](uint32_t x, uint32_t y) { return c->h_first_seen[x] < c->h_first_seen[y]; });
    PFCHK(fetch_strand_bits(c));

    *res = c->counters;
    res->cluster_kmer_off = c->h_kmer_off.data();
    res->cluster_kmer_cnt = c->h_kmer_cnt.data();
    res->cluster_pattern = c->h_cl_pattern.data();
    res->cluster_unique = c->h_cl_unique.data();
    res->kmer_key = c->h_kmer_key.data();
    res->kmer_pattern = c->h_kmer_pid.data();
    res->new_pattern_id = c->h_new_pid.data();
    res->n_patterns = p1;
    res->pattern_md5 = c->h_pat_md5.data();
    res->pattern_bits = c->h_pat_bits.data();
    res->pattern_nan = c->o.consider_missing ? c->h_pat_nan.data() : nullptr;
    res->pattern_n = c->h_pat_n.data();
    res->pattern_first_seen = c->h_first_seen.data();
    res->strand_bits = c->n_strand_words ? c->h_strand.data() : nullptr;
    return PF_OK;
}

int pf_export_patterns(pf_ctx* c, uint64_t* n, const uint8_t** md5, const uint64_t** first_seen) {
    if (!c || !n || !md5 || !first_seen) return fail(PF_ERR_ARG, "null argument");
    HIPCHK(hipSetDevice(c->device));
    const uint32_t p1 = c->n_patterns;
    c->h_pat_md5.resize((size_t)p1 * 16);
    c->h_first_seen.resize(p1);
    if (p1) {
        HIPCHK(hipStreamSynchronize(c->stream));
        HIPCHK(hipMemcpy(c->h_pat_md5.data(), c->pats.md5.p, (size_t)p1 * 16, hipMemcpyDeviceToHost));
        HIPCHK(hipMemcpy(c->h_first_seen.data(), c->pt.first_seen, (size_t)p1 * 8, hipMemcpyDeviceToHost));
    }
    *n = p1;
    *md5 = c->h_pat_md5.data();
    *first_seen = c->h_first_seen.data();
    return PF_OK;
}

int pf_export_patterns_dev(pf_ctx* c, uint64_t cap, void* d_md5, void* d_first_seen, uint64_t* n) {
    if (!c || !n) return fail(PF_ERR_ARG, "null argument");
    HIPCHK(hipSetDevice(c->device));
    const uint64_t m = std::min<uint64_t>(cap, c->n_patterns);
    if (m) {
        if (!d_md5 || !d_first_seen) return fail(PF_ERR_ARG, "null destination");
        HIPCHK(hipMemcpyAsync(d_md5, c->pats.md5.p, (size_t)m * 16, hipMemcpyDeviceToDevice, c->stream));
        HIPCHK(hipMemcpyAsync(d_first_seen, c->pt.first_seen, (size_t)m * 8, hipMemcpyDeviceToDevice, c->stream));
        HIPCHK(hipStreamSynchronize(c->stream));
    }
    *n = m;
    return PF_OK;
}

int pf_render_kmers_to_hashes(pf_ctx* c, const char* const* names, const char* const* extra_keys, char** out,
                              uint64_t* nbytes, uint64_t* cluster_end) {
    if (!c || !names || !out || !nbytes) return fail(PF_ERR_ARG, "null argument");
    if (!c->have_batch || c->h_kmer_off.size() != c->n_clusters) return fail(PF_ERR_STATE, "pf_render_* needs pf_fetch first");
    ensure_b64(c);
    const uint32_t C = c->n_clusters, k = c->o.klength, KW = (uint32_t)c->KW;
    std::vector<uint64_t> off(C + 1, 0);
    std::vector<uint32_t> nlen(C);
    for (uint32_t i = 0; i < C; i++) {
        nlen[i] = (uint32_t)strlen(names[i]);
        off[i + 1] = off[i] + (nlen[i] + 2 + 24 + 1) + (uint64_t)c->h_kmer_cnt[i] * (nlen[i] + 1 + k + 1 + 24 + 1);
    }
    char* buf = (char*)malloc(off[C] + 1);
    if (!buf) return fail(PF_ERR_OOM, "malloc(%llu) failed", (unsigned long long)off[C]);
    const char* b64 = c->h_b64.data();
    const uint64_t npat = c->h_b64.size() / 24;
    bool bad = false;
    parallel_for(C, [&](uint64_t a, uint64_t b) {
        for (uint64_t i = a; i < b; i++) {
            char* w = buf + off[i];
            const uint32_t L = nlen[i];
            const uint32_t cp = c->h_cl_pattern[i];
            if (cp >= npat) { bad = true; continue; }
            memcpy(w, names[i], L); w += L; *w++ = '\t'; *w++ = '\t';
            memcpy(w, b64 + (size_t)cp * 24, 24); w += 24; *w++ = '\n';
            const uint64_t o = c->h_kmer_off[i];
            for (uint32_t j = 0; j < c->h_kmer_cnt[i]; j++) {
                memcpy(w, names[i], L); w += L; *w++ = '\t';
                const uint64_t* key = c->h_kmer_key.data() + (o + j) * KW;
                if (key[0] >> 63) {
                    if (!extra_keys) { bad = true; memset(w, '?', k); }
                    else memcpy(w, extra_keys[(uint32_t)key[0]], k);
                } else {
                    // 2k-bit value, first base most significant, in KW words of 63 bits: bit b lives in word
                    // KW - 1 - b / 63 at bit b % 63
                    for (uint32_t q = 0; q < k; q++) {
                        const uint32_t b0 = 2 * (k - 1 - q), b1 = b0 + 1;
                        const uint32_t code = (uint32_t)((key[KW - 1 - b0 / 63] >> (b0 % 63)) & 1) |
                                              ((uint32_t)((key[KW - 1 - b1 / 63] >> (b1 % 63)) & 1) << 1);
                        w[q] = "ACGT"[code];
                    }
                }
                w += k; *w++ = '\t';
                const uint32_t pid = c->h_kmer_pid[o + j];
                if (pid >= npat) { bad = true; memset(w, '?', 24); }
                else memcpy(w, b64 + (size_t)pid * 24, 24);
                w += 24; *w++ = '\n';
            }
        }
    });
    if (bad) { free(buf); return fail(PF_ERR_STATE, "pf_render_kmers_to_hashes: inconsistent result (pattern id / extra key)"); }
    buf[off[C]] = 0;
    if (cluster_end) for (uint32_t i = 0; i < C; i++) cluster_end[i] = off[i + 1];
    *out = buf;
    *nbytes = off[C];
    return PF_OK;
}

int pf_render_hashes_to_patterns(pf_ctx* c, char** out, uint64_t* nbytes) {
    if (!c || !out || !nbytes) return fail(PF_ERR_ARG, "null argument");
    if (!c->have_batch || c->h_new_pid.size() != c->n_patterns - c->pid0) return fail(PF_ERR_STATE, "pf_render_* needs pf_fetch first");
    ensure_b64(c);
    const uint32_t W = c->W;
    const size_t P = c->h_new_pid.size();
    const bool miss = c->o.consider_missing != 0;
    std::vector<uint64_t> off(P + 1, 0);
    for (size_t i = 0; i < P; i++) {
        const uint32_t pid = c->h_new_pid[i];
        const uint32_t nk = c->h_pat_n[pid], n = nk & 0x7FFFFFFFu;
        uint32_t nn = 0;
        if (miss && !(nk >> 31))
            for (uint32_t w = 0; w < W; w++) nn += __builtin_popcount(c->h_pat_nan[(size_t)pid * W + w]);
        off[i + 1] = off[i] + 24 + n + (n - nn) + 1;
    }
    char* buf = (char*)malloc(off[P] + 1);
    if (!buf) return fail(PF_ERR_OOM, "malloc(%llu) failed", (unsigned long long)off[P]);
    parallel_for(P, [&](uint64_t a, uint64_t b) {
        for (uint64_t i = a; i < b; i++) {
            char* w = buf + off[i];
            const uint32_t pid = c->h_new_pid[i];
            const uint32_t nk = c->h_pat_n[pid], n = nk & 0x7FFFFFFFu;
            const bool use_nan = miss && !(nk >> 31);
            const uint32_t* bits = c->h_pat_bits.data() + (size_t)pid * W;
            const uint32_t* nan = use_nan ? c->h_pat_nan.data() + (size_t)pid * W : nullptr;
            memcpy(w, c->h_b64.data() + (size_t)pid * 24, 24); w += 24;
            for (uint32_t e = 0; e < n; e++) {
                *w++ = '\t';
                if (nan && ((nan[e >> 5] >> (e & 31)) & 1)) continue;          // '' for NaN (panfeed.py:220)
                *w++ = ((bits[e >> 5] >> (e & 31)) & 1) ? '1' : '0';
            }
            *w++ = '\n';
        }
    });
    buf[off[P]] = 0;
    *out = buf;
    *nbytes = off[P];
    return PF_OK;
}

namespace {
// Measure: which strand every window of the n target sequences uses, taken once from the device's strand bits, and with
// that the exact size of every sequence's rows -- no worst-case sizing, no compaction afterwards.
int kt_host_measure(pf_ctx* c, const pf_target_seq* seqs, uint32_t n, const uint32_t* seg_strand_off, KtHostText& M, KtHostFilter* F = nullptr) {
    if (!c || (n && !seqs)) return fail(PF_ERR_ARG, "null argument");
    if (!c->have_batch) return fail(PF_ERR_STATE, "pf_render_kmers_tsv without a successful pf_submit");
    HIPCHK(hipSetDevice(c->device));
    PFCHK(fetch_strand_bits(c));          // all this renderer needs from the device (pf_fetch is not required)
    const uint32_t k = c->o.klength;
    const bool canon = c->o.canon != 0;
    M.fl_off.assign((size_t)n + 1, 0);
    for (uint32_t i = 0; i < n; i++) {
        const long long nk = (long long)seqs[i].len - k + 1;
        M.fl_off[i + 1] = M.fl_off[i] + (canon && nk > 0 ? (uint64_t)nk : 0);
    }
    M.rcflags.assign(M.fl_off[n], 2);
    M.size.assign(n, 0);
    std::atomic<bool> bad{false};
    parallel_for(n, [&](uint64_t a, uint64_t b) {
        for (uint64_t i = a; i < b; i++) {
            const pf_target_seq& s = seqs[i];
            const long long nk = (long long)s.len - k + 1;
            if (nk <= 0) continue;
            uint8_t* rcflag = canon ? M.rcflags.data() + M.fl_off[i] : nullptr;
            if (canon) {
                for (uint32_t j = 0; j < s.n_segs; j++) {
                    if (!seg_strand_off || c->h_strand.empty()) { bad = true; break; }
                    const uint32_t so = seg_strand_off[s.seg_index[j]];
                    for (uint32_t q = 0; q < s.seg_nwin[j]; q++) {
                        const size_t word = (size_t)so + (q >> 6);
                        if (so == 0xFFFFFFFFu || word >= c->h_strand.size() || s.seg_start[j] + q >= (uint64_t)nk) { bad = true; break; }
                        rcflag[s.seg_start[j] + q] = (uint8_t)((c->h_strand[word] >> (q & 63)) & 1);
                    }
                }
            }
            RowCount cnt;
            if (F) {                                   // the filtered text: only the kept rows count
                RowFilter<RowCount> f{cnt, F->sets[F->seq_set[i]], k};
                if (!kt_host_rows(s, k, canon, rcflag, f)) bad = true;
                F->considered += f.seen; F->kept += f.kept;
            } else if (!kt_host_rows(s, k, canon, rcflag, cnt)) bad = true;
            M.size[i] = cnt.n;
        }
    });
    if (bad) return fail(PF_ERR_STATE, "pf_render_kmers_tsv: strand bits missing for a target window");
    M.bytes = std::accumulate(M.size.begin(), M.size.end(), (uint64_t)0);
    return PF_OK;
}

// Write: the rows of the measured sequences [i0, i1), back to back from dst on, each sequence at its exact place
int kt_host_write(pf_ctx* c, const pf_target_seq* seqs, const KtHostText& M, uint32_t i0, uint32_t i1, char* dst, const KtHostFilter* F = nullptr) {
    const uint32_t k = c->o.klength;
    const bool canon = c->o.canon != 0;
    std::vector<uint64_t> off((size_t)(i1 - i0) + 1, 0);
    for (uint32_t i = i0; i < i1; i++) off[i - i0 + 1] = off[i - i0] + M.size[i];
    std::atomic<bool> bad{false};
    parallel_for(i1 - i0, [&](uint64_t a, uint64_t b) {
        for (uint64_t j = a; j < b; j++) {
            RowWrite wr{dst + off[j]};
            const uint8_t* rcflag = canon ? M.rcflags.data() + M.fl_off[i0 + j] : nullptr;
            if (F) {
                RowFilter<RowWrite> f{wr, F->sets[F->seq_set[i0 + j]], k};
                kt_host_rows(seqs[i0 + j], k, canon, rcflag, f);
            } else kt_host_rows(seqs[i0 + j], k, canon, rcflag, wr);
            if ((uint64_t)(wr.w - (dst + off[j])) != M.size[i0 + j]) bad = true;
        }
    });
    if (bad) return fail(PF_ERR_STATE, "pf_render_kmers_tsv: row sizes of the two passes differ");
    return PF_OK;
}
}  // namespace

int pf_render_kmers_tsv(pf_ctx* c, const pf_target_seq* seqs, uint32_t n, const uint32_t* seg_strand_off, char** out,
                        uint64_t* nbytes) {
    if (!out || !nbytes) return fail(PF_ERR_ARG, "null argument");
    KtHostText M;
    PFCHK(kt_host_measure(c, seqs, n, seg_strand_off, M));
    char* buf = (char*)malloc(M.bytes + 1);
    if (!buf) return fail(PF_ERR_OOM, "malloc(%llu) failed", (unsigned long long)M.bytes);
    const int rc = kt_host_write(c, seqs, M, 0, n, buf);
    if (rc != PF_OK) { free(buf); return rc; }
    buf[M.bytes] = 0;
    *out = buf;
    *nbytes = M.bytes;
    return PF_OK;
}

namespace {
// Which of the n target sequences the device writes: those that are pure A/C/G/T -- one segment of the batch covering
// every window -- and whose rows fit kt_text_kernel's tile; the others (a target sequence with an 'N', a row too long
// for the tile) are left to the host renderer.  The device's sequences go up as descriptors, one text prefix each, and
// tiles of KT_ROWS rows; kt_len_kernel sizes every tile.  kp is set up for kt_text_kernel but for tile_off / text.
struct KtLayout {
    std::vector<uint2> tiles;
    std::vector<uint32_t> tbytes;       // bytes of every tile
    std::vector<uint32_t> host_idx;     // sequences left to the host renderer
    std::vector<uint8_t> on_dev;
    pf::KtParams kp{};
    // under the passing-rows filter: the kernels' second argument, the kept rows of every tile, the candidate rows of the
    // device's sequences, and the host's sets
    bool filter = false;
    pf::KtFilter kf{};
    std::vector<uint32_t> trows;
    uint64_t dev_rows = 0;
    std::unique_ptr<KtHostFilter> hfilter;
};

// The passing set's table from the digests the context holds, at the hash width in force
int passing_build_set(pf_ctx* c) {
    PassingRows& F = c->passing;
    const uint64_t n = F.digests.size() / 16;
    uint64_t cap = 16;
    while (cap < 2 * n + 2) cap <<= 1;
    std::vector<pf::PassSlot> slots(cap, pf::PassSlot{0, 0, 0, 0});
    for (uint64_t i = 0; i < n; i++) {
        uint64_t d[2];
        memcpy(d, F.digests.data() + i * 16, 16);
        const uint64_t h = pf::pass_digest_hash(d[0], d[1], F.bits);
        uint64_t at = h & (cap - 1);
        while (slots[at].used) at = (at + 1) & (cap - 1);
        slots[at] = pf::PassSlot{d[0], d[1], h, 1};
    }
    HIPCHK(hipSetDevice(c->device));
    PFCHK(F.set.ensure(cap * sizeof(pf::PassSlot)));
    HIPCHK(hipMemcpy(F.set.p, slots.data(), cap * sizeof(pf::PassSlot), hipMemcpyHostToDevice));
    F.set_mask = cap - 1;
    return PF_OK;
}

// Mark and index, once per text: the kept k-mers of the clusters that own one of the text's sequences are marked by
// their patterns' digests (pass_mark_kernel), the passing ones entered into the batch index the row kernels probe.  For
// the clusters of the host-rendered sequences the marks and keys come down and become the text of their passing k-mers.
// all_cl: the cluster of every sequence that has a window (~0u: none); dev_cl: of the device-written ones, in order.
int kt_filter_prepare(pf_ctx* c, const std::vector<uint32_t>& all_cl, const std::vector<uint32_t>& dev_cl, KtLayout& L) {
    PassingRows& F = c->passing;
    const uint32_t C = c->n_clusters, KW = (uint32_t)c->KW, k = c->o.klength, NT = (uint32_t)L.tiles.size();
    hipStream_t st = c->stream;
    std::vector<uint64_t> koff(C);
    std::vector<uint32_t> kcnt(C), arena_of(C);
    if (C) {
        HIPCHK(hipMemcpyAsync(koff.data(), c->batch.cl_kmer_off.p, (size_t)C * 8, hipMemcpyDeviceToHost, st));
        HIPCHK(hipMemcpyAsync(kcnt.data(), c->batch.cl_kmer_cnt.p, (size_t)C * 4, hipMemcpyDeviceToHost, st));
        HIPCHK(hipStreamSynchronize(st));
    }
    std::vector<uint8_t> owns(C, 0);
    for (uint32_t cl : all_cl) if (cl != ~0u) owns[cl] = 1;
    std::vector<uint32_t> mcl, mark_of(C, ~0u);
    std::vector<uint64_t> moff{0};
    for (uint32_t i = 0; i < C; i++) {
        const uint32_t a = c->cluster_arena[i];
        arena_of[i] = a;
        koff[i] = kcnt[i] ? koff[i] - c->arenas[a]->base : 0;
        if (!owns[i]) continue;
        mark_of[i] = (uint32_t)mcl.size();
        mcl.push_back(i);
        moff.push_back(moff.back() + kcnt[i]);
    }
    const uint64_t M = moff.back();
    uint64_t cap = 64;
    while (cap < 2 * M + 2) cap <<= 1;
    if ((M + 255) / 256 > 0x7FFFFFFFull) return fail(PF_ERR_CAPACITY, "passing rows: %llu kept k-mers to mark", (unsigned long long)M);
    PFCHK(F.ref.ensure(cap * 8)); PFCHK(F.hsh.ensure(cap * 8)); PFCHK(F.mark.ensure(std::max<uint64_t>(M, 1)));
    PFCHK(F.counters.ensure(16));
    PFCHK(F.mark_cluster.ensure(std::max<size_t>(mcl.size(), 1) * 4)); PFCHK(F.mark_off.ensure(moff.size() * 8));
    PFCHK(F.koff.ensure(std::max<size_t>(C, 1) * 8)); PFCHK(F.arena_of.ensure(std::max<size_t>(C, 1) * 4));
    PFCHK(F.seq_cluster.ensure(std::max<size_t>(dev_cl.size(), 1) * 4));
    PFCHK(F.keep_bits.ensure(std::max<size_t>(NT, 1) * (pf::KT_ROWS / 64) * 8)); PFCHK(F.tile_rows.ensure(std::max<size_t>(NT, 1) * 4));
    if (!mcl.empty()) HIPCHK(hipMemcpyAsync(F.mark_cluster.p, mcl.data(), mcl.size() * 4, hipMemcpyHostToDevice, st));
    HIPCHK(hipMemcpyAsync(F.mark_off.p, moff.data(), moff.size() * 8, hipMemcpyHostToDevice, st));
    if (C) {
        HIPCHK(hipMemcpyAsync(F.koff.p, koff.data(), (size_t)C * 8, hipMemcpyHostToDevice, st));
        HIPCHK(hipMemcpyAsync(F.arena_of.p, arena_of.data(), (size_t)C * 4, hipMemcpyHostToDevice, st));
    }
    if (!dev_cl.empty()) HIPCHK(hipMemcpyAsync(F.seq_cluster.p, dev_cl.data(), dev_cl.size() * 4, hipMemcpyHostToDevice, st));
    HIPCHK(hipMemsetAsync(F.counters.p, 0, 16, st));
    PFCHK(fill_u64(c, F.ref.p, pf::EMPTY64, cap));
    PFCHK(F.ev0.ensure()); PFCHK(F.ev1.ensure());
    HIPCHK(hipEventRecord(F.ev0, st));
    if (M) {
        pf::PassMarkParams mp{};
        mp.mark_cluster = F.mark_cluster.as<uint32_t>(); mp.mark_off = F.mark_off.as<uint64_t>();
        mp.n_mark = (uint32_t)mcl.size(); mp.n_patterns = c->n_patterns;
        mp.kmer_off = F.koff.as<uint64_t>(); mp.cluster_arena = F.arena_of.as<uint32_t>();
        for (size_t a = 0; a < c->n_passes; a++) { mp.arena_key[a] = c->arenas[a]->key.as<uint64_t>(); mp.arena_pid[a] = c->arenas[a]->pid.as<uint32_t>(); }
        mp.md5 = c->pats.md5.as<uint8_t>();
        mp.set = F.set.as<pf::PassSlot>(); mp.set_mask = F.set_mask;
        mp.ref = F.ref.as<uint64_t>(); mp.hsh = F.hsh.as<uint64_t>(); mp.mask = cap - 1;
        mp.mark = F.mark.as<uint8_t>(); mp.counters = F.counters.as<unsigned long long>();
        mp.KW = KW; mp.bits = F.bits;
        hipLaunchKernelGGL(pf::pass_mark_kernel, dim3((uint32_t)((M + 255) / 256)), dim3(256), 0, st, mp);
        HIPCHK(hipGetLastError());
    }
    HIPCHK(hipEventRecord(F.ev1, st));
    uint64_t cnt[2] = {0, 0};
    HIPCHK(hipMemcpyAsync(cnt, F.counters.p, 16, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));            // (the vectors above have gone up; the marks are written)
    F.marked = cnt[0];
    F.mark_ms = 0.0f;
    (void)hipEventElapsedTime(&F.mark_ms, F.ev0, F.ev1);
    pf::KtFilter& kf = L.kf;
    kf.seq_cluster = F.seq_cluster.as<uint32_t>();
    kf.ref = F.ref.as<uint64_t>(); kf.hsh = F.hsh.as<uint64_t>(); kf.mask = cap - 1;
    F.index_slots = cap;
    kf.kmer_off = F.koff.as<uint64_t>(); kf.cluster_arena = F.arena_of.as<uint32_t>();
    for (size_t a = 0; a < c->n_passes; a++) kf.arena_key[a] = c->arenas[a]->key.as<uint64_t>();
    kf.keep_bits = F.keep_bits.as<uint64_t>(); kf.tile_rows = F.tile_rows.as<uint32_t>();
    kf.counters = F.counters.as<unsigned long long>();
    kf.KW = KW; kf.bits = F.bits;
    // ---- the host's share: the passing k-mers, as text, of the clusters whose sequences it renders
    L.hfilter.reset(new KtHostFilter);
    KtHostFilter& H = *L.hfilter;
    std::vector<uint32_t> set_of(C, ~0u);
    std::vector<uint8_t> marks;
    std::vector<uint64_t> keys;
    for (uint32_t i : L.host_idx) {
        const uint32_t cl = all_cl[i];
        if (set_of[cl] == ~0u) {
            set_of[cl] = (uint32_t)H.sets.size();
            H.sets.emplace_back();
            std::unordered_set<std::string>& set = H.sets.back();
            const uint32_t n = kcnt[cl];
            if (n) {
                marks.resize(n); keys.resize((size_t)n * KW);
                HIPCHK(hipMemcpy(marks.data(), F.mark.as<uint8_t>() + moff[mark_of[cl]], n, hipMemcpyDeviceToHost));
                HIPCHK(hipMemcpy(keys.data(), c->arenas[arena_of[cl]]->key.as<uint64_t>() + koff[cl] * KW, (size_t)n * KW * 8, hipMemcpyDeviceToHost));
            }
            std::string t(k, 'A');
            for (uint32_t j = 0; j < n; j++) {
                if (!marks[j]) continue;
                const uint64_t* key = keys.data() + (size_t)j * KW;
                if (key[0] >> 63) {
                    const uint64_t e = (uint32_t)key[0];
                    if ((e + 1) * k > F.extra.size()) return fail(PF_ERR_STATE, "passing rows: a slow-path row's text was not given (pf_passing_batch_names)");
                    t.assign(F.extra, (size_t)e * k, k);
                } else {
                    for (uint32_t q = 0; q < k; q++) {
                        const uint32_t b0 = 2 * (k - 1 - q), b1 = b0 + 1;
                        const uint32_t code = (uint32_t)((key[KW - 1 - b0 / 63] >> (b0 % 63)) & 1) | ((uint32_t)((key[KW - 1 - b1 / 63] >> (b1 % 63)) & 1) << 1);
                        t[q] = "ACGT"[code];
                    }
                }
                set.insert(t);
            }
        }
        H.seq_set.push_back(set_of[cl]);
    }
    return PF_OK;
}

int kt_layout(pf_ctx* c, const pf_target_seq* seqs, uint32_t n, KtLayout& L) {
    const uint32_t k = c->o.klength;
    const bool canon = c->o.canon != 0;
    const uint32_t reps = canon ? 1u : 2u;
    if (canon && n && (!c->last.seg_strand_off || !c->n_strand_words))
        for (uint32_t i = 0; i < n; i++) if ((long long)seqs[i].len - k + 1 > 0 && seqs[i].n_segs) return fail(PF_ERR_STATE, "the last pf_submit carried no strand bits for target segments");
    std::vector<pf::KtSeq> ks;
    std::vector<uint2>& tiles = L.tiles;
    L.on_dev.assign(n, 0);
    std::string prefix;
    auto digits = [](long long v) { return len_i64(v); };
    PassingRows& F = c->passing;
    L.filter = F.on;
    std::vector<uint32_t> all_cl, dev_cl;
    if (L.filter) {
        if (!F.have_names) return fail(PF_ERR_STATE, "the passing-rows filter is on: pf_passing_batch_names must follow pf_submit before a kmers.tsv text");
        if (c->n_passes > pf::TEXT_MAX_ARENAS) return fail(PF_ERR_CAPACITY, "passing rows: the batch took %u passes, the filter's kernels read %u arenas", c->n_passes, pf::TEXT_MAX_ARENAS);
        if ((uint32_t)c->KW > pf::PASS_MAX_KW) return fail(PF_ERR_ARG, "passing rows: keys of %d words", c->KW);
        all_cl.assign(n, ~0u);
    }
    for (uint32_t i = 0; i < n; i++) {
        const pf_target_seq& s = seqs[i];
        const long long nk = (long long)s.len - k + 1;
        if (nk <= 0) continue;                   // no window, no row (panfeed.py:59,64)
        if (L.filter) {
            const auto it = F.name_idx.find(s.cluster);
            if (it == F.name_idx.end()) return fail(PF_ERR_ARG, "passing rows: target sequence %u names cluster '%s', which is not of the last batch", i, s.cluster);
            all_cl[i] = it->second;
        }
        bool dev = s.n_segs == 1 && s.n_ambig == 0 && s.seg_start[0] == 0 && s.seg_nwin[0] == (uint64_t)nk &&
                   s.seg_index[0] < c->last_nseg && (uint64_t)nk * reps < 0xFFFFFF00ull;
        size_t plen = 0;
        if (dev) {
            plen = strlen(s.cluster) + strlen(s.strain) + strlen(s.id) + strlen(s.chromosome) + 5 + digits(s.strand);
            // the longest row this sequence can have must fit the tile KT_ROWS times over
            const long long far = s.strand > 0 ? s.start + nk + k : s.end - nk - k;
            const size_t num = std::max(digits(s.strand > 0 ? s.start : s.end), digits(far));
            const size_t gnum = std::max(digits(-s.offset), digits(nk + k - s.offset));
            const size_t rowmax = plen + 2 * num + 2 * gnum + std::max(digits(s.strand), digits(-(long long)s.strand)) + 5 + k + 1;
            if (rowmax * pf::KT_ROWS > pf::KT_TILE || prefix.size() + plen > 0x7FFFFFF0u) dev = false;
        }
        if (!dev) { L.host_idx.push_back(i); continue; }
        L.on_dev[i] = 1;
        if (L.filter) { dev_cl.push_back(all_cl[i]); L.dev_rows += (uint64_t)nk * reps; }
        pf::KtSeq q{};
        q.base = s.strand > 0 ? s.start : s.end; q.offset = s.offset; q.strand = s.strand;
        q.seg = s.seg_index[0]; q.nk = (uint32_t)nk; q.prefix_off = (uint32_t)prefix.size(); q.prefix_len = (uint32_t)plen;
        prefix += s.cluster; prefix += '\t'; prefix += s.strain; prefix += '\t'; prefix += s.id; prefix += '\t';
        prefix += s.chromosome; prefix += '\t';
        { char t[24]; prefix.append(t, put_i64(t, s.strand) - t); }
        prefix += '\t';
        const uint32_t rows = (uint32_t)nk * reps, si = (uint32_t)ks.size();
        for (uint32_t r0 = 0; r0 < rows; r0 += pf::KT_ROWS) tiles.push_back(make_uint2(si, r0));
        ks.push_back(q);
    }
    // ---- tile sizes
    const uint32_t NT = (uint32_t)tiles.size();
    pf::KtParams& kp = L.kp;
    L.tbytes.assign(NT, 0);
    if (L.filter) { L.trows.assign(NT, 0); PFCHK(kt_filter_prepare(c, all_cl, dev_cl, L)); }
    if (NT) {
        PFCHK(c->kt.seqs.ensure(ks.size() * sizeof(pf::KtSeq)));
        PFCHK(c->kt.tiles.ensure((size_t)NT * 8));
        PFCHK(c->kt.prefix.ensure(prefix.size() + 16));
        PFCHK(c->kt.tbytes.ensure((size_t)NT * 4));
        PFCHK(c->kt.toff.ensure((size_t)NT * 8));
        HIPCHK(hipMemcpyAsync(c->kt.seqs.p, ks.data(), ks.size() * sizeof(pf::KtSeq), hipMemcpyHostToDevice, c->stream));
        HIPCHK(hipMemcpyAsync(c->kt.tiles.p, tiles.data(), (size_t)NT * 8, hipMemcpyHostToDevice, c->stream));
        HIPCHK(hipMemcpyAsync(c->kt.prefix.p, prefix.data(), prefix.size(), hipMemcpyHostToDevice, c->stream));
        kp.seqs = c->kt.seqs.as<pf::KtSeq>(); kp.tiles = c->kt.tiles.as<uint2>(); kp.prefix = c->kt.prefix.as<char>();
        kp.packed = c->last.packed; kp.seg_word_off = c->last.seg_word_off; kp.seg_strand_off = c->last.seg_strand_off;
        kp.strand_bits = c->strand_bits.as<uint64_t>();
        kp.tile_bytes = c->kt.tbytes.as<uint32_t>(); kp.tile_off = c->kt.toff.as<uint64_t>();
        kp.k = k; kp.canon = canon ? 1u : 0u;
        if (L.filter) hipLaunchKernelGGL(pf::kt_len_passing_kernel, dim3(NT), dim3(pf::KT_ROWS), 0, c->stream, kp, L.kf);
        else hipLaunchKernelGGL(pf::kt_len_kernel, dim3(NT), dim3(pf::KT_ROWS), 0, c->stream, kp);
        HIPCHK(hipGetLastError());
        if (L.filter) HIPCHK(hipMemcpyAsync(L.trows.data(), c->passing.tile_rows.p, (size_t)NT * 4, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(hipMemcpyAsync(L.tbytes.data(), c->kt.tbytes.p, (size_t)NT * 4, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(hipStreamSynchronize(c->stream));
    }
    return PF_OK;
}

// the batch's strand offsets, host side (the caller's array went to the device with the batch), for the host renderer
int kt_host_sso(pf_ctx* c, std::vector<uint32_t>& sso) {
    sso.clear();
    if (c->o.canon && c->last.seg_strand_off && c->last_nseg) {
        sso.resize(c->last_nseg);
        HIPCHK(hipMemcpy(sso.data(), c->last.seg_strand_off, (size_t)c->last_nseg * 4, hipMemcpyDeviceToHost));
    }
    return PF_OK;
}

// The plan of a text: its units in the order of the sequences -- a tile of a device-written sequence, or a whole
// host-rendered sequence; a sequence with no window is neither and drops out -- each unit's offset, and the ranges the
// text is produced in: the whole text when it fits the budget, else pieces of at most budget / 2 (with the 64 bytes of
// slack every text buffer has), cut between units.
void kt_plan(const KtLayout& L, const std::vector<uint64_t>& hsizes, uint64_t budget, KtPlan& P) {
    const size_t NT = L.tiles.size(), NH = L.host_idx.size();
    P = KtPlan{};
    P.toff.resize(NT); P.hoff.resize(NH); P.seq_end.resize(L.on_dev.size());
    const uint64_t all = std::accumulate(L.tbytes.begin(), L.tbytes.end(), (uint64_t)0) + std::accumulate(hsizes.begin(), hsizes.end(), (uint64_t)0);
    P.cap = all + 64 <= budget ? all : (budget / 2 > 64 ? budget / 2 - 64 : 0);
    KtPlan::Range cur{0, 0, 0, 0, 0, 0};
    auto unit = [&](uint64_t bytes, uint64_t& off) {
        if (cur.bytes && cur.bytes + bytes > P.cap) {
            P.ranges.push_back(cur);
            cur = KtPlan::Range{cur.t1, cur.t1, cur.h1, cur.h1, cur.base + cur.bytes, 0};
        }
        off = cur.base + cur.bytes;
        cur.bytes += bytes;
        P.max_unit = std::max(P.max_unit, bytes);
    };
    size_t ti = 0, hi = 0;
    uint32_t si = 0;                             // device-written sequences so far: tiles[].x counts those
    for (uint32_t i = 0; i < (uint32_t)L.on_dev.size(); i++) {
        if (L.on_dev[i]) {
            for (; ti < NT && L.tiles[ti].x == si; cur.t1 = (uint32_t)++ti) unit(L.tbytes[ti], P.toff[ti]);
            si++;
        } else if (hi < NH && L.host_idx[hi] == i) {
            unit(hsizes[hi], P.hoff[hi]);
            cur.h1 = (uint32_t)++hi;
        }
        P.seq_end[i] = cur.base + cur.bytes;
    }
    if (cur.bytes) P.ranges.push_back(cur);
    P.total = cur.base + cur.bytes;
    for (size_t r = 0; r < P.ranges.size(); r++) {
        P.max_range = std::max(P.max_range, P.ranges[r].bytes);
        P.peak = std::max(P.peak, P.ranges[r].bytes + (r + 1 < P.ranges.size() ? P.ranges[r + 1].bytes : 0));
    }
}
}  // namespace

namespace {
constexpr uint64_t KT_BLOCK = 64ull << 20;    // bytes per block a stream hands out (DeviceText.chunks' default too)

// Range r of the open stream written into its buffer (text[r & 1]) on c->stream, by the stream's producer.  From r = 2
// on the buffer's range before (r - 2) must be done with: the host waits until that range was written, so that the
// producer may reuse the host memory it was uploaded from, and c->stream waits for that range's last copy on c->side.
int ts_produce(pf_ctx* c, uint32_t r) {
    TextStream& S = c->ts;
    const int b = (int)(r & 1);
    if (r >= 2) {
        HIPCHK(hipEventSynchronize(S.ev_prod[b]));
        HIPCHK(hipStreamWaitEvent(c->stream, S.ev_copied[b], 0));
    }
    PFCHK(S.by.write(c, r, S.text[b].as<char>(), b));
    HIPCHK(hipEventRecord(S.ev_prod[b], c->stream));
    return PF_OK;
}

// A text begun: a stream that is open ends, pf_device_text_chunk's text is gone (the buffers are reused) with the block of
// it that nobody asked for, and the stream is `by`'s from here on.
int ts_begin(pf_ctx* c, const TextStream::Producer& by) {
    TextStream& S = c->ts;
    ts_end(c);
    if (S.flight.valid) HIPCHK(hipStreamSynchronize(c->side));
    S.kept = 0; S.flight.valid = false;
    S.kind = by.kind; S.by = by;
    return PF_OK;
}

// The stream begun takes its ranges: the buffers (one range: all of it in text[0]; several: two of the largest), the
// events, the position at the start, blocks of at most pin_bytes, and the first two ranges on their way.
int ts_open(pf_ctx* c, std::vector<TextStream::Range> ranges, uint64_t pin_bytes) {
    TextStream& S = c->ts;
    S.ranges.swap(ranges);
    const uint32_t NR = (uint32_t)S.ranges.size();
    uint64_t max_range = 0;
    for (const TextStream::Range& R : S.ranges) max_range = std::max(max_range, R.bytes);
    if (NR <= 1) PFCHK(S.text[0].ensure((size_t)max_range + 64));
    else for (DevBuf& t : S.text) PFCHK(t.ensure((size_t)max_range + 64, true));
    for (int b = 0; b < 2; b++) { PFCHK(S.ev_prod[b].ensure(hipEventDisableTiming)); PFCHK(S.ev_copied[b].ensure(hipEventDisableTiming)); }
    S.cur = 0; S.cur_off = 0;
    S.pin_bytes = std::max<uint64_t>(1, pin_bytes);
    for (uint32_t r = 0; r < std::min(NR, 2u); r++) PFCHK(ts_produce(c, r));
    return PF_OK;
}

// The kmers.tsv producer.  Range r: its tiles by kt_text_kernel, its host-rendered sequences written by the host now, from
// their one measurement, and copied up (the text of the buffer's range before has been: it is freed).
int kt_write(pf_ctx* c, uint32_t r, char* buf, int b) {
    TargetText& S = c->kt;
    const KtPlan::Range& R = S.plan.ranges[r];
    S.htext[b].reset();
    if (R.t1 > R.t0) {
        pf::KtParams kp = S.kp;
        kp.text = buf; kp.tile_first = R.t0; kp.text_base = R.base;
        if (S.filter) hipLaunchKernelGGL(pf::kt_text_passing_kernel, dim3(R.t1 - R.t0), dim3(pf::KT_ROWS), 0, c->stream, kp, S.kf);
        else hipLaunchKernelGGL(pf::kt_text_kernel, dim3(R.t1 - R.t0), dim3(pf::KT_ROWS), 0, c->stream, kp);
        HIPCHK(hipGetLastError());
    }
    if (R.h1 > R.h0) {
        const uint64_t* hsize = S.host.size.data();
        const uint64_t hbytes = std::accumulate(hsize + R.h0, hsize + R.h1, (uint64_t)0);
        S.htext[b].reset(new (std::nothrow) char[hbytes + 1]);
        if (!S.htext[b]) return fail(PF_ERR_OOM, "malloc(%llu) failed", (unsigned long long)hbytes);
        PFCHK(kt_host_write(c, S.hseqs.data(), S.host, R.h0, R.h1, S.htext[b].get(), S.hfilter.get()));
        uint64_t at = 0;
        for (uint32_t j = R.h0; j < R.h1; j++) {
            if (hsize[j]) HIPCHK(hipMemcpyAsync(buf + (S.plan.hoff[j] - R.base), S.htext[b].get() + at, (size_t)hsize[j], hipMemcpyHostToDevice, c->stream));
            at += hsize[j];
        }
    }
    return PF_OK;
}
void kt_drop(pf_ctx* c) {
    TargetText& S = c->kt;
    for (auto& t : S.htext) t.reset();
    S.hseqs.clear(); S.host = KtHostText{}; S.plan = KtPlan{};
    S.filter = false; S.hfilter.reset();
}

// What the two device texts share: the checks of their arguments and of the context's state, the layout, the host's
// share measured, the plan within `budget`, and the stream opened over the plan's ranges (there is only one when the
// text fits the budget).  The stream is open afterwards, whatever stream was before is not; a failure leaves none.
int kt_open(pf_ctx* c, const pf_target_seq* seqs, uint32_t n, uint64_t budget, bool outputs_given, const char* who) {
    if (!c || !outputs_given || (n && !seqs)) return fail(PF_ERR_ARG, "null argument");
    if (!c->have_batch) return fail(PF_ERR_STATE, "%s without a successful pf_submit", who);
    HIPCHK(hipSetDevice(c->device));
    c->kt.have_seq_end = false;
    EndUnlessOpen guard{c};
    PFCHK(ts_begin(c, {TextStream::KMERS_TSV, kt_write, kt_drop}));
    TargetText& S = c->kt;
    KtLayout L;
    PFCHK(kt_layout(c, seqs, n, L));
    S.filter = L.filter; S.kf = L.kf; S.hfilter = std::move(L.hfilter);
    // ---- the host's share: measured here, written range by range
    S.hseqs.resize(L.host_idx.size());
    for (size_t j = 0; j < L.host_idx.size(); j++) S.hseqs[j] = seqs[L.host_idx[j]];
    if (!S.hseqs.empty()) {
        std::vector<uint32_t> sso;
        PFCHK(kt_host_sso(c, sso));
        PFCHK(kt_host_measure(c, S.hseqs.data(), (uint32_t)S.hseqs.size(), sso.empty() ? nullptr : sso.data(), S.host, S.hfilter.get()));
    }
    if (S.filter) {
        c->passing.considered = L.dev_rows + S.hfilter->considered;
        c->passing.kept = std::accumulate(L.trows.begin(), L.trows.end(), (uint64_t)0) + S.hfilter->kept;
    }
    const KtPlan& P = S.plan;
    kt_plan(L, S.host.size, budget, S.plan);
    if (P.max_unit > P.cap)
        return fail(PF_ERR_ARG, "kmers.tsv budget of %llu bytes is too small for this batch: its largest tile or host-rendered "
                    "sequence is %llu bytes, the smallest budget that works is %llu", (unsigned long long)budget,
                    (unsigned long long)P.max_unit, (unsigned long long)(2 * (P.max_unit + 64)));
    // ---- the tiles' places up, and the stream over the plan's ranges
    const uint32_t NT = (uint32_t)L.tiles.size();
    if (NT) HIPCHK(hipMemcpyAsync(c->kt.toff.p, P.toff.data(), (size_t)NT * 8, hipMemcpyHostToDevice, c->stream));
    S.kp = L.kp;
    std::vector<TextStream::Range> ranges;
    for (const KtPlan::Range& R : P.ranges) ranges.push_back({R.base, R.bytes});
    PFCHK(ts_open(c, std::move(ranges), std::min(KT_BLOCK, P.max_range)));
    c->kt.seq_end.swap(S.plan.seq_end);            // (the plan goes with the stream; the ends stay until the next submit)
    c->kt.have_seq_end = true;
    guard.ok = true;
    return PF_OK;
}

// n bytes at src, which start at byte `off` of the text, on their way into pinned slot `slot` (of `block` bytes) on
// c->side: the one block in flight that pf_device_text_chunk or a stream's next picks up next
int ts_prefetch(pf_ctx* c, int slot, const char* src, uint64_t off, uint64_t n, uint64_t block) {
    TextStream& S = c->ts;
    PFCHK(S.pins[slot].ensure(block, true));
    if (n) HIPCHK(hipMemcpyAsync(S.pins[slot].p, src, n, hipMemcpyDeviceToHost, c->side));
    S.flight = {true, slot, off, n};
    return PF_OK;
}

// The stream's block at (S.cur, S.cur_off) queued on c->side behind its range's writing, and the stream's position moved
// past it.  Plain: its copy into pinned slot `slot`.  Device gzip: its encode into block_members[slot], the members'
// size on its way into the slot's pinned cursor word.  The last block of range r also marks the range's buffer free, and
// range r + 2 is queued into it.
int ts_block(pf_ctx* c, int slot) {
    TextStream& S = c->ts;
    GzMode& G = c->gz;
    const TextStream::Range& R = S.ranges[S.cur];
    const int b = (int)(S.cur & 1);
    const char* src = S.text[b].as<char>() + S.cur_off;
    const uint64_t off = R.base + S.cur_off, n = std::min<uint64_t>(S.pin_bytes, R.bytes - S.cur_off);
    HIPCHK(hipStreamWaitEvent(c->side, S.ev_prod[b], 0));
    if (G.on) {
        // the block's segments: what lies between the cuts inside it (none: one segment, the block as a whole)
        TextStream::Block& B = S.blk[slot];
        B.off = off; B.n = n;
        B.lo = (size_t)(std::upper_bound(S.cuts.begin(), S.cuts.end(), off) - S.cuts.begin());
        B.hi = (size_t)(std::lower_bound(S.cuts.begin(), S.cuts.end(), off + n) - S.cuts.begin());
        B.seg_end.clear();
        for (size_t i = B.lo; i < B.hi; i++) B.seg_end.push_back(S.cuts[i] - off);
        if (n) B.seg_end.push_back(n);
        PFCHK(G.enc.encode_segments(c->side, slot ? PfGzEncoder::STREAM_BLOCK1 : PfGzEncoder::STREAM_BLOCK0, src, n, B.seg_end.data(),
                                    B.seg_end.size(), G.flags, G.block_members[slot].as<char>(), G.block_bound));
        S.flight = {true, slot, off, n};
    } else PFCHK(ts_prefetch(c, slot, src, off, n, S.pin_bytes));
    S.cur_off += n;
    if (S.cur_off == R.bytes) {
        HIPCHK(hipEventRecord(S.ev_copied[b], c->side));
        if (S.cur + 2 < S.ranges.size()) PFCHK(ts_produce(c, S.cur + 2));
        S.cur++; S.cur_off = 0;
    }
    return PF_OK;
}

// The open stream is to be handed out: the count of its text bytes starts, and under device gzip the buffers of its two
// blocks in flight are there, for blocks of at most pin_bytes of text with n_cuts cuts among them
int ts_hand_out(pf_ctx* c, uint64_t n_cuts = 0) {
    GzMode& G = c->gz;
    G.raw[2] = 0;
    if (!G.on) return PF_OK;
    PFCHK(G.enc.ensure(c->n_cu));
    G.block_bound = PfGzEncoder::bound_segments(c->ts.pin_bytes, n_cuts);     // (every cut may add a short chunk)
    for (int s = 0; s < 2; s++) {
        PFCHK(G.block_members[s].ensure(G.block_bound, true));
        PFCHK(c->ts.pins[s].ensure(G.block_bound, true));
    }
    PFCHK(G.ev_copy.ensure(hipEventDisableTiming));
    return PF_OK;
}

// Device gzip, a block of `text` bytes whose encode into block_members[slot] the caller has synchronised with: only the
// members cross to the host.  *n: their size; their copy into the slot's pinned block is queued on c->side with ev_copy
// behind it, for the caller to wait for once the next block is on its way.
int gz_block_down(pf_ctx* c, int slot, uint64_t text, uint64_t* n) {
    TextStream& S = c->ts;
    GzMode& G = c->gz;
    const PfGzEncoder::Cursor w = slot ? PfGzEncoder::STREAM_BLOCK1 : PfGzEncoder::STREAM_BLOCK0;
    PFCHK(G.enc.member_bytes(w, n));
    if (!S.cuts.empty()) {                                 // (the stream's cuts: their places came with the size)
        TextStream::Block& B = S.blk[slot];
        B.member_end.resize(B.seg_end.size());
        if (!B.seg_end.empty()) PFCHK(G.enc.segment_ends(w, B.member_end.data()));
    }
    G.raw[2] += text;
    HIPCHK(hipMemcpyAsync(S.pins[slot].p, G.block_members[slot].p, *n, hipMemcpyDeviceToHost, c->side));
    HIPCHK(hipEventRecord(G.ev_copy, c->side));
    return PF_OK;
}

// The next block of the open stream: its text, or under device gzip its members.  While the caller holds block j, block
// j + 1 is already queued: its copy into the other pinned slot, or its encode into the other block of members.  A step
// that fails leaves the stream open as it stands, of either producer: whatever begins or ends a stream next ends it.
int ts_next(pf_ctx* c, const char** ptr, uint64_t* nbytes) {
    TextStream& S = c->ts;
    GzMode& G = c->gz;
    HIPCHK(hipSetDevice(c->device));
    if (!S.flight.valid) {
        if (S.cur >= S.ranges.size()) { ts_end(c); return PF_OK; }
        PFCHK(ts_block(c, 0));
    }
    HIPCHK(hipStreamSynchronize(c->side));                 // the block has arrived (gzip: is encoded, its size has arrived)
    const int slot = S.flight.slot;
    uint64_t n = S.flight.n;
    // their copy goes behind the encode and before the next block's, which runs while they arrive
    if (G.on) PFCHK(gz_block_down(c, slot, n, &n));
    S.flight.valid = false;
    if (S.cur < S.ranges.size()) PFCHK(ts_block(c, slot ^ 1));      // the next block on its way meanwhile
    if (G.on) HIPCHK(hipEventSynchronize(G.ev_copy));
    S.handed = slot;
    *ptr = S.pins[slot].as<char>();
    *nbytes = n;
    return PF_OK;
}
}  // namespace

// The same rows written by the GPU (kt_len_kernel / kt_text_kernel) for the sequences kt_layout gives it and by the host
// renderer above for the others, which are copied to their places in the device text: the text of all n sequences, in
// order, stays in device memory and is handed out block by block (pf_device_text_chunk).  It is the stream's plan with
// no budget -- one range, written into text[0] -- and no stream is left open: the caller's seqs die with the call.
int pf_render_kmers_tsv_device(pf_ctx* c, const pf_target_seq* seqs, uint32_t n, uint64_t* nbytes) {
    PFCHK(kt_open(c, seqs, n, ~0ull, nbytes != nullptr, "pf_render_kmers_tsv_device"));
    const uint64_t total = c->kt.plan.total;
    const hipError_t text_written = hipStreamSynchronize(c->stream);
    ts_end(c);
    HIPCHK(text_written);
    c->ts.kept = total;
    *nbytes = total;
    return PF_OK;
}

// The text of pf_render_kmers_tsv_device in ranges: cut at tile and host-sequence boundaries so that each range takes at
// most half the budget, written range by range into two device buffers used alternately, range r + 1 written while range
// r leaves the device.  A batch whose text fits the budget is one range, the single-buffer path's work.
int pf_kmers_tsv_stream_begin(pf_ctx* c, const pf_target_seq* seqs, uint32_t n, uint64_t budget_bytes,
                              uint64_t* total_bytes, uint32_t* n_ranges, uint64_t* peak_text_bytes) {
    if (total_bytes) *total_bytes = 0;
    if (n_ranges) *n_ranges = 0;
    if (peak_text_bytes) *peak_text_bytes = 0;
    PFCHK(kt_open(c, seqs, n, budget_bytes, total_bytes && n_ranges, "pf_kmers_tsv_stream_begin"));
    const KtPlan& P = c->kt.plan;
    uint64_t peak = P.peak;
    if (const int rc = ts_hand_out(c); rc != PF_OK) { ts_end(c); return rc; }
    // the encoder's buffers and the two blocks of members count as the text's memory
    if (c->gz.on) peak += c->gz.enc.device_bytes() + 2 * c->gz.block_bound;
    *total_bytes = P.total;
    *n_ranges = (uint32_t)P.ranges.size();
    if (peak_text_bytes) *peak_text_bytes = peak;
    return PF_OK;
}

int pf_kmers_tsv_stream_next(pf_ctx* c, const char** ptr, uint64_t* nbytes) {
    if (!c || !ptr || !nbytes) return fail(PF_ERR_ARG, "null argument");
    *ptr = nullptr; *nbytes = 0;
    if (c->ts.kind != TextStream::KMERS_TSV) return fail(PF_ERR_STATE, "pf_kmers_tsv_stream_next without an open pf_kmers_tsv_stream_begin");
    return ts_next(c, ptr, nbytes);
}

int pf_kmers_tsv_stream_cuts(pf_ctx* c, const uint64_t* cuts, uint64_t n) {
    if (!c || (n && !cuts)) return fail(PF_ERR_ARG, "pf_kmers_tsv_stream_cuts: null argument");
    TextStream& S = c->ts;
    if (S.kind != TextStream::KMERS_TSV) return fail(PF_ERR_STATE, "pf_kmers_tsv_stream_cuts without an open pf_kmers_tsv_stream_begin");
    if (!c->gz.on) return fail(PF_ERR_STATE, "pf_kmers_tsv_stream_cuts: the stream hands out text, which is cut anywhere; the cuts are for pf_set_device_gzip");
    if (S.flight.valid || S.cur || S.cur_off || S.handed >= 0)
        return fail(PF_ERR_STATE, "pf_kmers_tsv_stream_cuts: the stream's first block is on its way already");
    const uint64_t total = c->kt.plan.total;
    std::vector<uint64_t> in;
    for (uint64_t i = 0; i < n; i++) {
        if ((i && cuts[i] < cuts[i - 1]) || cuts[i] > total) return fail(PF_ERR_ARG, "pf_kmers_tsv_stream_cuts: the offsets must not decrease nor pass the text's end");
        if (cuts[i] && cuts[i] < total && (in.empty() || in.back() != cuts[i])) in.push_back(cuts[i]);
    }
    HIPCHK(hipSetDevice(c->device));
    PFCHK(ts_hand_out(c, in.size()));
    S.cuts.swap(in);
    return PF_OK;
}

int pf_kmers_tsv_stream_block_cuts(pf_ctx* c, uint64_t* text_off, uint64_t* text_bytes, uint64_t* cut_text, uint64_t* cut_member,
                                   uint64_t cap, uint64_t* n_cuts) {
    if (!c || !text_off || !text_bytes || !n_cuts) return fail(PF_ERR_ARG, "pf_kmers_tsv_stream_block_cuts: null argument");
    TextStream& S = c->ts;
    if (S.kind != TextStream::KMERS_TSV || S.handed < 0 || !c->gz.on) return fail(PF_ERR_STATE, "pf_kmers_tsv_stream_block_cuts without a block of members handed out");
    const TextStream::Block& B = S.blk[S.handed];
    const uint64_t k = B.hi - B.lo;
    *text_off = B.off; *text_bytes = B.n; *n_cuts = k;
    if (k > cap || (k && (!cut_text || !cut_member))) return fail(PF_ERR_ARG, "pf_kmers_tsv_stream_block_cuts: %llu cuts inside the block, room for %llu", (unsigned long long)k, (unsigned long long)cap);
    if (k && B.member_end.size() != k + 1) return fail(PF_ERR_STATE, "pf_kmers_tsv_stream_block_cuts: the block's member offsets are missing");
    for (uint64_t i = 0; i < k; i++) { cut_text[i] = S.cuts[B.lo + i]; cut_member[i] = B.member_end[i]; }
    return PF_OK;
}

int pf_kmers_tsv_seq_ends(pf_ctx* c, uint64_t* ends, uint32_t n) {
    if (!c || (n && !ends)) return fail(PF_ERR_ARG, "pf_kmers_tsv_seq_ends: null argument");
    if (!c->have_batch || !c->kt.have_seq_end)
        return fail(PF_ERR_STATE, "pf_kmers_tsv_seq_ends without a pf_render_kmers_tsv_device or pf_kmers_tsv_stream_begin since the last pf_submit");
    if ((size_t)n != c->kt.seq_end.size())
        return fail(PF_ERR_ARG, "pf_kmers_tsv_seq_ends: %u sequences asked for, the text was planned for %zu", n, c->kt.seq_end.size());
    if (n) memcpy(ends, c->kt.seq_end.data(), (size_t)n * 8);
    return PF_OK;
}

int pf_set_passing_hashes(pf_ctx* c, const uint8_t* md5, uint64_t n) {
    if (!c || (n && !md5)) return fail(PF_ERR_ARG, "pf_set_passing_hashes: null argument");
    if (c->ts.kind == TextStream::KMERS_TSV) return fail(PF_ERR_STATE, "pf_set_passing_hashes while a kmers.tsv stream is open");
    PassingRows& F = c->passing;
    std::vector<std::array<uint8_t, 16>> d(n);
    if (n) memcpy(d.data(), md5, n * 16);
    std::sort(d.begin(), d.end());
    d.erase(std::unique(d.begin(), d.end()), d.end());
    F.digests.resize(d.size() * 16);
    if (!d.empty()) memcpy(F.digests.data(), d.data(), d.size() * 16);
    PFCHK(passing_build_set(c));
    F.on = true;
    F.marked = F.considered = F.kept = 0;
    F.index_slots = 0;
    return PF_OK;
}

int pf_clear_passing_hashes(pf_ctx* c) {
    if (!c) return fail(PF_ERR_ARG, "pf_clear_passing_hashes: null argument");
    if (c->ts.kind == TextStream::KMERS_TSV) return fail(PF_ERR_STATE, "pf_clear_passing_hashes while a kmers.tsv stream is open");
    PassingRows& F = c->passing;
    F.on = false;
    F.digests.clear();
    for (DevBuf* b : {&F.set, &F.ref, &F.hsh, &F.mark, &F.counters, &F.mark_cluster, &F.mark_off, &F.koff, &F.arena_of, &F.seq_cluster, &F.keep_bits, &F.tile_rows}) b->release();
    F.marked = F.considered = F.kept = 0;
    F.index_slots = 0;
    return PF_OK;
}

int pf_passing_batch_names(pf_ctx* c, const char* const* cluster_names, const char* extra_keys, uint64_t n_extra) {
    if (!c || (c->n_clusters && !cluster_names) || (n_extra && !extra_keys)) return fail(PF_ERR_ARG, "pf_passing_batch_names: null argument");
    if (!c->have_batch) return fail(PF_ERR_STATE, "pf_passing_batch_names without a successful pf_submit");
    if (c->ts.kind == TextStream::KMERS_TSV) return fail(PF_ERR_STATE, "pf_passing_batch_names while a kmers.tsv stream is open");
    PassingRows& F = c->passing;
    F.name_idx.clear();
    for (uint32_t i = 0; i < c->n_clusters; i++) {
        if (!cluster_names[i]) return fail(PF_ERR_ARG, "pf_passing_batch_names: null name");
        F.name_idx.emplace(cluster_names[i], i);
    }
    F.extra.assign(extra_keys ? extra_keys : "", (size_t)n_extra * c->o.klength);
    F.have_names = true;
    return PF_OK;
}

int pf_passing_stats(pf_ctx* c, uint64_t out[6]) {
    if (!c || !out) return fail(PF_ERR_ARG, "pf_passing_stats: null argument");
    PassingRows& F = c->passing;
    uint64_t cnt[2] = {0, 0};
    if (F.on && F.counters.p) {
        HIPCHK(hipSetDevice(c->device));
        HIPCHK(hipStreamSynchronize(c->stream));
        HIPCHK(hipMemcpy(cnt, F.counters.p, 16, hipMemcpyDeviceToHost));
    }
    out[0] = F.digests.size() / 16; out[1] = F.marked; out[2] = F.considered; out[3] = F.kept; out[4] = cnt[1];
    out[5] = F.device_bytes();
    return PF_OK;
}

int pf_passing_mark_ms(pf_ctx* c, float* ms) {
    if (!c || !ms) return fail(PF_ERR_ARG, "pf_passing_mark_ms: null argument");
    *ms = c->passing.mark_ms;
    return PF_OK;
}

int pf_debug_passing_hash_bits(pf_ctx* c, uint32_t bits) {
    if (!c || bits > 64) return fail(PF_ERR_ARG, "pf_debug_passing_hash_bits: 0 .. 64 bits");
    if (c->ts.kind == TextStream::KMERS_TSV) return fail(PF_ERR_STATE, "pf_debug_passing_hash_bits while a kmers.tsv stream is open");
    c->passing.bits = bits;
    c->passing.index_slots = 0;
    if (c->passing.on) PFCHK(passing_build_set(c));
    return PF_OK;
}

int pf_debug_passing_tables(pf_ctx* c, int which, uint64_t first, uint64_t n, uint64_t* out, uint64_t* slots) {
    if (!c || (n && !out)) return fail(PF_ERR_ARG, "pf_debug_passing_tables: null argument");
    if (which < 0 || which > 2) return fail(PF_ERR_ARG, "pf_debug_passing_tables: which must be 0 (the passing set), 1 (the index's ref) or 2 (its hsh)");
    PassingRows& F = c->passing;
    if (!F.on) return fail(PF_ERR_STATE, "pf_debug_passing_tables: the passing-rows filter is off");
    if (which != 0 && (!c->have_batch || !F.index_slots))
        return fail(PF_ERR_STATE, "pf_debug_passing_tables: no filtered kmers.tsv text since the last pf_submit, pf_set_passing_hashes or pf_debug_passing_hash_bits");
    const uint64_t bound = which == 0 ? F.set_mask + 1 : F.index_slots, words = which == 0 ? sizeof(pf::PassSlot) / 8 : 1;
    if (slots) *slots = bound;
    if (first > bound || n > bound - first) return fail(PF_ERR_ARG, "pf_debug_passing_tables: slots [%llu, +%llu) outside the %llu held",
                                                        (unsigned long long)first, (unsigned long long)n, (unsigned long long)bound);
    HIPCHK(hipSetDevice(c->device));
    HIPCHK(hipStreamSynchronize(c->stream));
    const uint64_t* src = which == 0 ? F.set.as<uint64_t>() : which == 1 ? F.ref.as<uint64_t>() : F.hsh.as<uint64_t>();
    if (n) HIPCHK(hipMemcpy(out, src + first * words, (size_t)(n * words) * 8, hipMemcpyDeviceToHost));
    return PF_OK;
}

// Bytes [offset, offset + n) of the text the last pf_render_kmers_tsv_device left on the device, n = min(max_bytes, what
// remains), in pinned host memory; the block after it is already on its way when the call returns.
int pf_device_text_chunk(pf_ctx* c, uint64_t offset, uint64_t max_bytes, const char** ptr, uint64_t* nbytes) {
    if (!c || !ptr || !nbytes || !max_bytes) return fail(PF_ERR_ARG, "null argument");
    TextStream& T = c->ts;
    if (offset > T.kept) return fail(PF_ERR_ARG, "offset beyond the text");
    HIPCHK(hipSetDevice(c->device));
    const uint64_t n = std::min<uint64_t>(max_bytes, T.kept - offset);
    const char* text = T.text[0].as<char>();
    if (!n) {                                         // (nothing to copy, and the block in flight, if any, stays)
        PFCHK(T.pins[0].ensure(max_bytes, true));
        *ptr = T.pins[0].as<char>(); *nbytes = 0;
        return PF_OK;
    }
    if (!(T.flight.valid && T.flight.off == offset && T.flight.n == n)) {
        HIPCHK(hipStreamSynchronize(c->side));        // (a block in flight that nobody asked for)
        PFCHK(ts_prefetch(c, 0, text + offset, offset, n, max_bytes));
    }
    HIPCHK(hipStreamSynchronize(c->side));            // requested by the call before, or just now: wait for it
    const int slot = T.flight.slot;
    T.flight.valid = false;
    const uint64_t next = offset + n;
    if (next < T.kept) PFCHK(ts_prefetch(c, slot ^ 1, text + next, next, std::min<uint64_t>(max_bytes, T.kept - next), max_bytes));
    *ptr = T.pins[slot].as<char>();
    *nbytes = n;
    return PF_OK;
}

void pf_free_text(char* p) { free(p); }

namespace {
int merge_impl(pf_ctx* c, const void* d_gathered, uint64_t n_total, uint64_t my_first, uint64_t my_count,
               const void* d_slot_counts, uint64_t slot_rows, void* d_keep, uint64_t* n_global) {
    HIPCHK(hipSetDevice(c->device));
    *n_global = 0;
    if (!n_total) return PF_OK;
    if (!d_gathered || (my_count && !d_keep) || my_first + my_count > n_total) return fail(PF_ERR_ARG, "pf_merge_patterns: bad range");
    uint64_t cap = 1024;
    while (cap < 2 * n_total) cap <<= 1;
    PFCHK(c->mg_lo.ensure(cap * 32));
    PFCHK(c->mg_cnt.ensure(8));
    PFCHK(fill_u64(c, c->mg_lo.p, pf::EMPTY64, cap * 4));
    HIPCHK(hipMemsetAsync(c->mg_cnt.p, 0, 8, c->stream));
    pf::MergeParams mp{};
    mp.gathered = (const uint64_t*)d_gathered; mp.n = n_total;
    mp.tab = c->mg_lo.as<uint64_t>();
    mp.cap = cap; mp.my_first = my_first; mp.my_count = my_count; mp.keep = (uint8_t*)d_keep;
    mp.slot_counts = (const int64_t*)d_slot_counts; mp.slot_rows = d_slot_counts ? slot_rows : 0;
    mp.n_global = c->mg_cnt.as<unsigned long long>();
    const uint32_t blocks = (uint32_t)std::min<uint64_t>((n_total + 255) / 256, 8192);
    hipLaunchKernelGGL(pf::merge_insert_kernel, dim3(blocks), dim3(256), 0, c->stream, mp);
    HIPCHK(hipGetLastError());
    if (my_count) {
        const uint32_t b2 = (uint32_t)std::min<uint64_t>((my_count + 255) / 256, 8192);
        hipLaunchKernelGGL(pf::merge_lookup_kernel, dim3(b2), dim3(256), 0, c->stream, mp);
        HIPCHK(hipGetLastError());
    }
    HIPCHK(hipMemcpyAsync(n_global, c->mg_cnt.p, 8, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    return PF_OK;
}
}  // namespace

int pf_merge_patterns(pf_ctx* c, const void* d_gathered, uint64_t n_total, uint64_t my_first, uint64_t my_count,
                      void* d_keep, uint64_t* n_global) {
    if (!c || !n_global) return fail(PF_ERR_ARG, "null argument");
    return merge_impl(c, d_gathered, n_total, my_first, my_count, nullptr, 0, d_keep, n_global);
}

int pf_merge_patterns_padded(pf_ctx* c, const void* d_gathered, uint64_t world, uint64_t slot_rows,
                             const void* d_slot_counts, uint64_t rank, uint64_t my_count, void* d_keep,
                             uint64_t* n_global) {
    if (!c || !n_global || !d_slot_counts || rank >= world || my_count > slot_rows) return fail(PF_ERR_ARG, "pf_merge_patterns_padded: bad argument");
    return merge_impl(c, d_gathered, world * slot_rows, rank * slot_rows, my_count, d_slot_counts, slot_rows, d_keep, n_global);
}

int pf_result_checksum(pf_ctx* c, uint64_t out[3]) {
    if (!c || !out) return fail(PF_ERR_ARG, "null argument");
    if (!c->have_batch) return fail(PF_ERR_STATE, "pf_result_checksum without a successful pf_submit");
    HIPCHK(hipSetDevice(c->device));
    const uint32_t C = c->n_clusters, KW = (uint32_t)c->KW;
    out[0] = out[1] = out[2] = 0;
    if (!C) return PF_OK;
    // where each cluster's k-mers stand: arena of the cluster + offset inside it
    std::vector<uint64_t> off(C);
    HIPCHK(hipMemcpy(off.data(), c->batch.cl_kmer_off.p, (size_t)C * 8, hipMemcpyDeviceToHost));
    std::vector<const uint64_t*> kp(C);
    std::vector<const uint32_t*> pp(C);
    for (uint32_t i = 0; i < C; i++) {
        const Arena* ar = c->arenas[c->cluster_arena[i]].get();
        const uint64_t local = off[i] >= ar->base ? off[i] - ar->base : 0;      // clusters without k-mers: never read
        kp[i] = ar->key.as<uint64_t>() + local * KW;
        pp[i] = ar->pid.as<uint32_t>() + local;
    }
    DevBuf d_kp, d_pp, d_acc;
    PFCHK(d_kp.ensure((size_t)C * 8)); PFCHK(d_pp.ensure((size_t)C * 8)); PFCHK(d_acc.ensure(24));
    int rc = PF_OK;
    if (hipMemcpy(d_kp.p, kp.data(), (size_t)C * 8, hipMemcpyHostToDevice) != hipSuccess ||
        hipMemcpy(d_pp.p, pp.data(), (size_t)C * 8, hipMemcpyHostToDevice) != hipSuccess ||
        hipMemsetAsync(d_acc.p, 0, 24, c->stream) != hipSuccess) rc = fail(PF_ERR_HIP, "pf_result_checksum: copy failed");
    if (rc == PF_OK) {
        hipLaunchKernelGGL(pf::result_checksum_kernel, dim3(C), dim3(256), 0, c->stream,
                           (const uint64_t* const*)d_kp.p, (const uint32_t* const*)d_pp.p, c->batch.cl_kmer_cnt.as<uint32_t>(),
                           c->batch.cl_unique.as<uint32_t>(), c->batch.cl_pattern.as<uint32_t>(), c->pats.md5.as<uint8_t>(), KW,
                           (unsigned long long*)d_acc.p);
        if (hipGetLastError() != hipSuccess || hipStreamSynchronize(c->stream) != hipSuccess ||
            hipMemcpy(out, d_acc.p, 24, hipMemcpyDeviceToHost) != hipSuccess)
            rc = fail(PF_ERR_HIP, "pf_result_checksum: kernel failed");
    }
    return rc;
}

int pf_pattern_count(pf_ctx* c, uint64_t* n) {
    if (!c || !n) return fail(PF_ERR_ARG, "null argument");
    *n = c->n_patterns;
    return PF_OK;
}

int pf_submit_gather(pf_ctx* c, const pf_batch* b, const pf_gather* g, pf_result* r) {
    if (!c || !b || !g) return fail(PF_ERR_ARG, "pf_submit_gather: null argument");
    c->pending_gather = g;
    const int rc = pf_submit(c, b, r);
    c->pending_gather = nullptr;
    return rc;
}

// ---------------------------------------------------------------------------------------------------------------------------
// One-pass ingest: the reader's sink (pf_ingest.h).  A ring of blocks, each a pinned host block with a device twin: a reader
// thread read()s a genome's file straight into a pinned block, parses the GFF lines there, measures the contigs without
// copying a base, and gives the block back with one piece per contig; the block goes to its twin (one copy over PCIe) and
// genome_pack_text_kernel de-wraps, upper-cases and packs the pieces into the genome store, while other threads are still
// reading other files.  The host never touches a base of a pure-A/C/G/T contig: rounds 1-4 made three passes over every
// genome on the host (read, upper-casing copy into contig strings, copy into pinned blocks) before the same pack.
namespace {
struct IngestSlot {
    RegBuf pin;               // its blocks are views into the ring's two blocks, or its own (a file larger than the ring's slots)
    DevBuf dev, dpieces;
    PinBuf pin_pieces;
    HipEvent ev;
    bool held = false;        // a reader thread is filling it
    bool inflight = false;    // its copy / kernel may not have finished (ev)
};
struct Ingest {
    pf_ctx* c = nullptr;
    const pf_pangenome_opts* o = nullptr;
    pf_ctx* (*get_ctx)(void*) = nullptr;
    void* user = nullptr;
    std::once_flag once;
    bool setup_ok = false;
    RegBuf ring_pin;
    DevBuf ring_dev;
    std::mutex mu;
    std::condition_variable cv;
    std::vector<IngestSlot> slots;
    uint64_t store_cap = 0;
    std::atomic<uint64_t> store_used{0};
    std::string err;
    int rc = PF_OK;
    uint64_t bytes_up = 0;
    int failed(int code, const std::string& m) { if (rc == PF_OK) { rc = code; err = m; } return code; }   // (caller holds mu)
};
int ingest_ready(Ingest* I);
int ingest_acquire(void* self, size_t bytes, char** host, uint32_t* slot) {
    Ingest* I = (Ingest*)self;
    if (ingest_ready(I) != PF_OK) return I->rc != PF_OK ? I->rc : PF_ERR_STATE;
    if (hipSetDevice(I->c->device) != hipSuccess) return PF_ERR_HIP;
    std::unique_lock<std::mutex> lk(I->mu);
    for (;;) {
        if (I->rc != PF_OK) return I->rc;
        int pick = -1, waitable = -1;
        for (size_t i = 0; i < I->slots.size(); i++) {
            IngestSlot& s = I->slots[i];
            if (s.held) continue;
            if (s.inflight && hipEventQuery(s.ev) == hipSuccess) s.inflight = false;
            if (!s.inflight) { if (pick < 0 || (s.pin.cap >= bytes && I->slots[pick].pin.cap < bytes)) pick = (int)i; }
            else if (waitable < 0) waitable = (int)i;
        }
        if (pick >= 0) {
            IngestSlot& s = I->slots[pick];
            s.held = true;
            if (s.pin.cap < bytes) {
                lk.unlock();                                   // (the slot is ours: nobody else looks at it while it is held)
                const size_t want = bytes + bytes / 4 + 4096;  // (a block of its own, with its own device twin)
                const bool ok = s.pin.ensure(want) == PF_OK && s.dev.ensure(want) == PF_OK;
                if (!ok) s.pin.release();
                lk.lock();
                if (!ok) { s.held = false; I->cv.notify_all(); return I->failed(PF_ERR_OOM, "no pinned / device block of " + std::to_string(want) + " bytes for a genome's text"); }
            }
            *host = s.pin.p; *slot = (uint32_t)pick;
            return PF_OK;
        }
        if (waitable >= 0) {                                    // every free block is still on its way to the device
            hipEvent_t ev = I->slots[waitable].ev;
            lk.unlock();
            (void)hipEventSynchronize(ev);
            lk.lock();
            continue;
        }
        I->cv.wait(lk);
    }
}
uint64_t ingest_claim(void* self, uint64_t nwords) {
    Ingest* I = (Ingest*)self;
    if (ingest_ready(I) != PF_OK) return UINT64_MAX;
    const uint64_t at = I->store_used.fetch_add(nwords);
    return at + nwords <= I->store_cap ? at : UINT64_MAX;
}
int ingest_submit(void* self, uint32_t slot, size_t text_bytes, const pf_ingest_piece* pieces, uint32_t n) {
    Ingest* I = (Ingest*)self;
    IngestSlot& s = I->slots[slot];
    std::unique_lock<std::mutex> lk(I->mu);
    auto done = [&](int rc) { s.held = false; I->cv.notify_all(); return rc; };
    if (!n || !text_bytes || I->rc != PF_OK) return done(I->rc);
    if (hipSetDevice(I->c->device) != hipSuccess) return done(I->failed(PF_ERR_HIP, "hipSetDevice failed"));
    // the pieces travel behind the text in the same block when there is room (one copy instead of two per file)
    const size_t tail = (text_bytes + 63) & ~(size_t)63;
    const bool inline_pieces = tail + (size_t)n * sizeof(pf::TextPiece) <= s.pin.cap;
    pf::TextPiece* const pcs = inline_pieces ? reinterpret_cast<pf::TextPiece*>(s.pin.p + tail) : nullptr;
    if (!inline_pieces && (size_t)n * sizeof(pf::TextPiece) > s.pin_pieces.cap &&
        s.pin_pieces.ensure(((size_t)n + n / 2 + 64) * sizeof(pf::TextPiece), true) != PF_OK)
        return done(I->failed(PF_ERR_OOM, "ingest pieces: " + g_err));
    uint64_t lo = text_bytes, blocks = 0;
    for (uint32_t i = 0; i < n; i++) {
        pf::TextPiece& t = (inline_pieces ? pcs : s.pin_pieces.as<pf::TextPiece>())[i];
        t.text_off = pieces[i].text_off; t.dst_word = pieces[i].dst_word; t.nbases = (uint32_t)pieces[i].nbases;
        t.nwords = (uint32_t)(2 * ((pieces[i].nbases + 63) / 64) + 4);
        t.width = pieces[i].width; t.eol = pieces[i].eol; t.block0 = (uint32_t)blocks; t.pad = 0;
        blocks += (t.nwords + 255) / 256;
        lo = std::min<uint64_t>(lo, pieces[i].text_off);
        // the last letter's byte must lie inside the block
        const uint64_t lines = pieces[i].width && pieces[i].nbases ? (pieces[i].nbases - 1) / pieces[i].width : 0;
        if (pieces[i].text_off + pieces[i].nbases + lines * pieces[i].eol > text_bytes || pieces[i].dst_word + t.nwords > I->store_cap)
            return done(I->failed(PF_ERR_STATE, "ingest: a contig's letters lie outside its block"));
    }
    if (blocks > 0x7FFFFFFFull) return done(I->failed(PF_ERR_CAPACITY, "ingest: too many words in one file"));
    lo &= ~(uint64_t)63;
    hipStream_t st = I->c->stream;
    const pf::TextPiece* dpcs;
    if (getenv("PF_DEBUG_INGEST_SKIP_UPLOAD")) return done(PF_OK);        // (timing experiment: the reader alone; nothing reaches the store)
    if (inline_pieces) {
        if (hipMemcpyAsync((char*)s.dev.p + lo, s.pin.p + lo, tail + (size_t)n * sizeof(pf::TextPiece) - lo, hipMemcpyHostToDevice, st) != hipSuccess)
            return done(I->failed(PF_ERR_HIP, "ingest: upload of a genome's text failed"));
        dpcs = reinterpret_cast<const pf::TextPiece*>((char*)s.dev.p + tail);
    } else {
        if (s.dpieces.ensure((size_t)n * sizeof(pf::TextPiece)) != PF_OK) return done(I->failed(PF_ERR_OOM, "device block for ingest pieces"));
        if (hipMemcpyAsync((char*)s.dev.p + lo, s.pin.p + lo, text_bytes - lo, hipMemcpyHostToDevice, st) != hipSuccess ||
            hipMemcpyAsync(s.dpieces.p, s.pin_pieces.p, (size_t)n * sizeof(pf::TextPiece), hipMemcpyHostToDevice, st) != hipSuccess)
            return done(I->failed(PF_ERR_HIP, "ingest: upload of a genome's text failed"));
        dpcs = (const pf::TextPiece*)s.dpieces.p;
    }
    hipLaunchKernelGGL(pf::genome_pack_text_kernel, dim3((uint32_t)blocks), dim3(256), 0, st, (const uint8_t*)s.dev.p,
                       dpcs, n, I->c->g_store.as<uint64_t>());
    if (hipGetLastError() != hipSuccess || hipEventRecord(s.ev, st) != hipSuccess) return done(I->failed(PF_ERR_HIP, "genome_pack_text_kernel launch failed"));
    s.inflight = true;
    I->bytes_up += text_bytes - lo;
    return done(PF_OK);
}
}  // namespace

namespace {
// what the first callback of the reader sets up (the context may still be in the making while the reader parses the table:
// it is asked for here, when the first genome needs it): the store, the events, the ring's two blocks
int ingest_setup(Ingest* I) {
    const pf_pangenome_opts* o = I->o;
    pf_ctx* c = I->get_ctx ? I->get_ctx(I->user) : nullptr;
    if (!c) return fail(PF_ERR_ARG, "pf_pangenome_open_device: no context");
    I->c = c;
    HIPCHK(hipSetDevice(c->device));
    HIPCHK(hipStreamSynchronize(c->stream));
    // the store's room: 2 bits per letter, and 2 * ceil(len / 64) + 4 words per contig -- the letters are at most the files'
    // bytes; half a byte of store per byte of text covers contigs down to ~200 letters on average (smaller ones: the
    // claim fails, PF_ERR_CAPACITY, and the caller takes pf_pangenome_open + pf_genomes_upload)
    uint64_t text_bytes = 0;
    size_t biggest = 0;
    for (uint32_t i = 0; i < o->n_genomes; i++) {
        const char* path = (o->fasta_paths && o->fasta_paths[i]) ? o->fasta_paths[i] : (o->gff_paths ? o->gff_paths[i] : nullptr);
        struct stat st;
        if (path && ::stat(path, &st) == 0 && S_ISREG(st.st_mode)) { text_bytes += (uint64_t)st.st_size; biggest = std::max<size_t>(biggest, (size_t)st.st_size); }
        else text_bytes += 64ull << 20;
    }
    I->store_cap = text_bytes / 16 + (8ull << 20);            // words
    c->g_store.release();
    c->g_words = 0;
    PFCHK(c->g_store.ensure((size_t)I->store_cap * 8));
    const unsigned nt = pf_host_threads(32u);
    // (a slot is held for one memcpy and handed to the copy engine, which empties it in a fifth of a millisecond: half as many
    // slots as reader threads, plus a few, are never all busy -- and 64 slots of 10 MB were 0.6 GB to allocate and page-lock
    // in front of the first upload)
    I->slots.resize(std::max<size_t>(4, std::min<size_t>((size_t)nt / 2 + 4, (size_t)o->n_genomes + 1)));
    for (auto& s : I->slots) PFCHK(s.ev.ensure(hipEventDisableTiming));
    // the ring's blocks: ONE page-locked allocation and ONE device allocation, cut into slots that hold the largest file (an
    // allocation per slot was 2 x 32 calls into the driver, one after the other, in front of the first upload).  Ordinary
    // memory, page-locked where it lies (RegBuf): the reader only COPIES the FASTA text into these blocks -- it
    // parses in its threads' own buffers.
    const size_t slot_bytes = (std::min<size_t>(biggest, 256u << 20) + 64 + (64u << 10) + 4095) & ~(size_t)4095;   // (+ room for the pieces)
    const size_t total = slot_bytes * I->slots.size();
    if (I->ring_pin.ensure(total) == PF_OK && I->ring_dev.ensure(total) == PF_OK) {
        for (size_t i = 0; i < I->slots.size(); i++) {
            IngestSlot& s = I->slots[i];
            s.pin.p = I->ring_pin.p + i * slot_bytes; s.pin.cap = slot_bytes; s.pin.view = true;
            s.dev.p = (char*)I->ring_dev.p + i * slot_bytes; s.dev.cap = 0; s.dev.view = true;
        }
    } else { I->ring_pin.release(); I->ring_dev.release(); }   // (slots then allocate their own)
    return PF_OK;
}
// every callback starts here: PF_OK once the set-up has succeeded (it runs once, on whichever reader thread comes first)
int ingest_ready(Ingest* I) {
    std::call_once(I->once, [I] {
        const int rc = ingest_setup(I);
        if (rc != PF_OK) { std::lock_guard<std::mutex> g(I->mu); I->failed(rc, pf_last_error()); }
        I->setup_ok = rc == PF_OK;
    });
    return I->setup_ok ? PF_OK : (I->rc != PF_OK ? I->rc : PF_ERR_STATE);
}
}  // namespace

int pf_pangenome_open_device_cb(const pf_pangenome_opts* o, pf_ctx* (*get_ctx)(void*), void* user, pf_pangenome** out) {
    if (!o || !get_ctx || !out) return fail(PF_ERR_ARG, "pf_pangenome_open_device: null argument");
    *out = nullptr;
    Ingest I;
    I.o = o; I.get_ctx = get_ctx; I.user = user;
    const bool dbg = getenv("PF_DEBUG_TIMING") != nullptr;
    auto T0 = std::chrono::steady_clock::now();
    auto lap = [&](const char* what) {
        if (!dbg) return;
        auto t = std::chrono::steady_clock::now();
        fprintf(stderr, "[open_device] %-28s %8.3f ms\n", what, std::chrono::duration<double, std::milli>(t - T0).count());
        T0 = t;
    };
    pf_pangenome* P = nullptr;
    pf_ingest_sink sink{&I, ingest_acquire, ingest_claim, ingest_submit};
    int rc = pf_pangenome_open_sink(o, &sink, &P);           // (its error text is this thread's: the reader sets it here)
    if (I.rc != PF_OK) rc = fail(I.rc, "%s", I.err.c_str());
    lap("reader (table, files -> pieces)");
    if (rc == PF_OK && ingest_ready(&I) != PF_OK) rc = fail(I.rc != PF_OK ? I.rc : PF_ERR_STATE, "%s", I.err.c_str());   // (a pangenome without a genome)
    pf_ctx* c = I.c;
    if (c) {
        (void)hipSetDevice(c->device);
        if (hipStreamSynchronize(c->stream) != hipSuccess && rc == PF_OK) rc = fail(PF_ERR_HIP, "the genomes' upload failed");
    }
    lap("last uploads");                  // (the stream is idle: the ring, the slots' own blocks and their events go with I)
    if (rc != PF_OK) {
        if (P) pf_pangenome_close(P);
        if (c) c->g_store.release();
        return rc;
    }
    c->g_words = std::min<uint64_t>(I.store_used.load(), I.store_cap);
    *out = P;
    return PF_OK;
}

int pf_pangenome_open_device(const pf_pangenome_opts* o, pf_ctx* c, pf_pangenome** out) {
    if (!c) return fail(PF_ERR_ARG, "pf_pangenome_open_device: null context");
    return pf_pangenome_open_device_cb(o, [](void* u) { return (pf_ctx*)u; }, c, out);
}

int pf_genomes_clear(pf_ctx* c) {
    if (!c) return fail(PF_ERR_ARG, "pf_genomes_clear: null context");
    HIPCHK(hipSetDevice(c->device));
    HIPCHK(hipStreamSynchronize(c->stream));
    c->g_store.release();
    c->g_words = 0;
    return PF_OK;
}

int pf_genomes_upload(pf_ctx* c, uint32_t n, const char* const* ascii, const uint64_t* len, uint64_t* word_off) {
    if (!c || (n && (!ascii || !len || !word_off))) return fail(PF_ERR_ARG, "pf_genomes_upload: null argument");
    HIPCHK(hipSetDevice(c->device));
    HIPCHK(hipStreamSynchronize(c->stream));
    uint64_t total = 0;
    for (uint32_t i = 0; i < n; i++) {
        if (len[i] >= 0xFFFFFF00ull) return fail(PF_ERR_ARG, "contig %u is too long for 32-bit coordinates", i);
        word_off[i] = total;
        total += 2 * ((len[i] + 63) / 64) + 4;
    }
    c->g_store.release();
    PFCHK(c->g_store.ensure((size_t)std::max<uint64_t>(total, 2) * 8));
    c->g_words = total;
    // staged in blocks: pinned host block -> device ASCII block -> 2-bit words.  Two sets of staging buffers: the host
    // threads copy block i + 1 into its pinned block while block i is on its way to the device and being packed there.
    const size_t BLOCK = 64u << 20;
    struct Src { const char* p; size_t n, at; };
    struct Blk { std::vector<pf::PackPiece> pieces; std::vector<Src> src; size_t fill = 0; uint32_t blocks = 0; };
    std::vector<Blk> blks(1);
    for (uint32_t i = 0; i < n; i++) {
        uint64_t done = 0;
        const uint64_t L = len[i];
        do {
            if (BLOCK - blks.back().fill < 64) blks.emplace_back();
            Blk& bk = blks.back();
            const uint64_t room = (BLOCK - bk.fill - 32) / 32 * 32;               // bases this block still takes
            const uint64_t take = std::min<uint64_t>(L - done, room);
            const bool last = done + take == L;
            bk.src.push_back(Src{ascii[i] + done, (size_t)take, bk.fill});
            const size_t padded = (take + 31) / 32 * 32;
            pf::PackPiece pc{};
            pc.ascii_off = bk.fill; pc.dst_word = word_off[i] + done / 32; pc.nbases = (uint32_t)take;
            const uint64_t contig_words = 2 * ((L + 63) / 64) + 4;
            pc.nwords = (uint32_t)(last ? contig_words - done / 32 : take / 32);
            pc.block0 = bk.blocks;
            bk.blocks += (pc.nwords + 255) / 256;
            if (pc.nwords) bk.pieces.push_back(pc);
            bk.fill += padded;
            done += take;
            if (!last) blks.emplace_back();
        } while (done < L);
    }
    PinBuf pin[2];
    DevBuf dasc[2], dpieces[2];
    HipEvent ev[2];
    // (declared after the staging buffers, it goes before them: however this call ends, the stream is idle when they are freed)
    struct Idle { hipStream_t s; bool done; ~Idle() { if (!done) (void)hipStreamSynchronize(s); } } idle{c->stream, false};
    for (int q = 0; q < 2; q++) { PFCHK(pin[q].ensure(BLOCK, true)); PFCHK(dasc[q].ensure(BLOCK)); PFCHK(ev[q].ensure(hipEventDisableTiming)); }
    for (size_t bi = 0; bi < blks.size(); bi++) {
        Blk& bk = blks[bi];
        if (bk.pieces.empty()) continue;
        const int q = (int)(bi & 1);
        if (hipEventSynchronize(ev[q]) != hipSuccess) return fail(PF_ERR_HIP, "hipEventSynchronize failed");   // the slot's last block has left it
        // the block's pieces into the pinned block, on the host threads (padding bases are 'A')
        char* dst = pin[q].as<char>();
        parallel_for(bk.fill, [&](uint64_t a, uint64_t e) {          // every thread takes a byte range of the block
            for (const Src& sp : bk.src) {
                const uint64_t lo = std::max<uint64_t>(a, sp.at), hi = std::min<uint64_t>(e, sp.at + sp.n);
                if (lo < hi) memcpy(dst + lo, sp.p + (lo - sp.at), hi - lo);
            }
        });
        for (const Src& sp : bk.src) { const size_t padded = (sp.n + 31) / 32 * 32; memset(dst + sp.at + sp.n, 'A', padded - sp.n); }
        PFCHK(dpieces[q].ensure(bk.pieces.size() * sizeof(pf::PackPiece)));
        if (hipMemcpyAsync(dasc[q].p, pin[q].p, bk.fill, hipMemcpyHostToDevice, c->stream) != hipSuccess ||
            hipMemcpyAsync(dpieces[q].p, bk.pieces.data(), bk.pieces.size() * sizeof(pf::PackPiece), hipMemcpyHostToDevice, c->stream) != hipSuccess)
            return fail(PF_ERR_HIP, "genome upload failed");
        hipLaunchKernelGGL(pf::genome_pack_kernel, dim3(bk.blocks), dim3(256), 0, c->stream, (const uint8_t*)dasc[q].p,
                           (const pf::PackPiece*)dpieces[q].p, (uint32_t)bk.pieces.size(), c->g_store.as<uint64_t>());
        if (hipGetLastError() != hipSuccess || hipEventRecord(ev[q], c->stream) != hipSuccess) return fail(PF_ERR_HIP, "genome_pack_kernel launch failed");
    }
    idle.done = true;
    if (hipStreamSynchronize(c->stream) != hipSuccess) return fail(PF_ERR_HIP, "genome upload failed");
    return PF_OK;
}

namespace {
// base64 of every digest up to n_patterns, on the device (incremental)
int ensure_b64_dev(pf_ctx* c) {
    if (!c->pats.b64.p) PFCHK(c->pats.b64.ensure((size_t)c->pt.pool * 24));
    const uint32_t p1 = c->n_patterns;
    if (c->txt.b64_done < p1) {
        hipLaunchKernelGGL(pf::b64_kernel, dim3((p1 - c->txt.b64_done + 255) / 256), dim3(256), 0, c->stream,
                           c->pats.md5.as<uint8_t>(), c->txt.b64_done, p1, c->pats.b64.as<char>());
        HIPCHK(hipGetLastError());
        c->txt.b64_done = p1;
    }
    return PF_OK;
}
// hashes_to_patterns rows on the device.  The lengths of n rows into d_len: of the patterns order[0 .. n) (a device
// list), or of patterns pid0 .. pid0 + n without a list
int hp_rowlen(pf_ctx* c, const uint32_t* order, uint32_t pid0, uint32_t n, uint32_t* d_len) {
    hipLaunchKernelGGL(pf::hp_rowlen_kernel, dim3((n + 255) / 256), dim3(256), 0, c->stream, c->pats.n.as<uint32_t>(),
                       c->o.consider_missing ? c->pats.nan.as<uint32_t>() : (const uint32_t*)nullptr, c->W, pid0, order, n, d_len);
    HIPCHK(hipGetLastError());
    return PF_OK;
}
// the rows of the patterns order[0 .. n), row i written at text + row_off[i] (device arrays)
int hp_text(pf_ctx* c, const uint32_t* order, const uint64_t* row_off, uint32_t n, char* text) {
    pf::HpTextParams hpp{};
    hpp.order = order; hpp.row_off = row_off;
    hpp.pat_bits = c->pats.bits.as<uint32_t>();
    hpp.pat_nan = c->o.consider_missing ? c->pats.nan.as<uint32_t>() : nullptr;
    hpp.pat_n = c->pats.n.as<uint32_t>(); hpp.b64 = c->pats.b64.as<char>();
    hpp.text = text; hpp.n = n; hpp.W = c->W;
    hipLaunchKernelGGL(pf::hp_text_kernel, dim3(n), dim3(256), 0, c->stream, hpp);
    HIPCHK(hipGetLastError());
    return PF_OK;
}
}  // namespace

namespace {
// The rows of the patterns pids[0 .. n) measured (one launch, and c->stream idle afterwards): the ids checked, then up
// in `order`, every row's length through `rlen` and down, row i's offset in their text in row_off[i], the text's size
// in row_off[n]
int hp_measure(pf_ctx* c, const char* who, const uint32_t* pids, uint32_t n, DevBuf& order, DevBuf& rlen, std::vector<uint64_t>& row_off) {
    row_off.assign((size_t)n + 1, 0);
    if (!n) return PF_OK;
    for (uint32_t i = 0; i < n; i++)
        if (pids[i] >= c->n_patterns) return fail(PF_ERR_ARG, "%s: pattern id %u out of range (%u patterns)", who, pids[i], c->n_patterns);
    PFCHK(ensure_b64_dev(c));
    PFCHK(order.ensure((size_t)n * 4));
    PFCHK(rlen.ensure((size_t)n * 4));
    HIPCHK(hipMemcpyAsync(order.p, pids, (size_t)n * 4, hipMemcpyHostToDevice, c->stream));
    PFCHK(hp_rowlen(c, order.as<uint32_t>(), 0u, n, rlen.as<uint32_t>()));
    std::vector<uint32_t> len(n);
    HIPCHK(hipMemcpyAsync(len.data(), rlen.p, (size_t)n * 4, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    for (uint32_t i = 0; i < n; i++) row_off[i + 1] = row_off[i] + len[i];
    return PF_OK;
}
}  // namespace

int pf_render_pattern_rows(pf_ctx* c, const uint32_t* pids, uint64_t n, const char** text, uint64_t* nbytes) {
    if (!c || !text || !nbytes || (n && !pids)) return fail(PF_ERR_ARG, "pf_render_pattern_rows: null argument");
    HIPCHK(hipSetDevice(c->device));
    *text = nullptr; *nbytes = 0;
    if (!n) return PF_OK;
    if (n > 0x7FFFFFFFull) return fail(PF_ERR_ARG, "pf_render_pattern_rows: too many rows in one call");
    hipStream_t st = c->stream;
    const uint32_t P = (uint32_t)n;
    std::vector<uint64_t> row_off;
    PFCHK(hp_measure(c, "pf_render_pattern_rows", pids, P, c->txt.rp_order, c->txt.rp_rlen, row_off));
    const uint64_t total = row_off[P];
    PFCHK(c->txt.rp_rowoff.ensure(((size_t)P + 1) * 8));
    PFCHK(c->txt.dev.ensure(total + 16));
    char* pin;
    PFCHK(c->txt.next_pin(total + 16, &pin));
    HIPCHK(hipMemcpyAsync(c->txt.rp_rowoff.p, row_off.data(), ((size_t)P + 1) * 8, hipMemcpyHostToDevice, st));
    PFCHK(hp_text(c, c->txt.rp_order.as<uint32_t>(), c->txt.rp_rowoff.as<uint64_t>(), P, c->txt.dev.as<char>()));
    HIPCHK(hipMemcpyAsync(pin, c->txt.dev.p, total, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    *text = pin; *nbytes = total;
    return PF_OK;
}

namespace {
// The pattern-row producer.  Range r is slice r: its row offsets up (the pinned block they go up from is free: the
// buffer's slice before has been written), its rows written into the buffer by hp_text_kernel.
int pr_write(pf_ctx* c, uint32_t r, char* buf, int b) {
    PatternRows& S = c->pr;
    const uint64_t r0 = S.cut[r], rows = S.cut[r + 1] - r0;
    uint64_t* ro = S.pin_rowoff[b].as<uint64_t>();
    for (uint64_t j = 0; j <= rows; j++) ro[j] = S.row_off[r0 + j] - S.row_off[r0];
    HIPCHK(hipMemcpyAsync(S.rowoff[b].p, ro, (size_t)(rows + 1) * 8, hipMemcpyHostToDevice, c->stream));
    return hp_text(c, S.order.as<uint32_t>() + r0, S.rowoff[b].as<uint64_t>(), (uint32_t)rows, buf);
}
void pr_drop(pf_ctx* c) { c->pr.row_off.clear(); c->pr.cut.clear(); }
}  // namespace

int pf_pattern_rows_stream_begin(pf_ctx* c, const uint32_t* pids, uint64_t n, uint64_t slice_bytes, uint64_t* total_text_bytes,
                                 uint32_t* n_slices) {
    if (!c || !total_text_bytes || !n_slices || (n && !pids)) return fail(PF_ERR_ARG, "pf_pattern_rows_stream_begin: null argument");
    *total_text_bytes = 0; *n_slices = 0;
    PatternRows& S = c->pr;
    if (c->ts.kind != TextStream::NONE)
        return fail(PF_ERR_STATE, "pf_pattern_rows_stream_begin: a stream of this context (%s) is not at its end",
                    c->ts.kind == TextStream::PATTERN_ROWS ? "pattern rows" : "kmers.tsv");
    if (n > 0x7FFFFFFFull) return fail(PF_ERR_ARG, "pf_pattern_rows_stream_begin: too many rows in one stream");
    HIPCHK(hipSetDevice(c->device));
    const uint32_t P = (uint32_t)n;
    const uint64_t cap = slice_bytes && slice_bytes < PfGzEncoder::BLOCK ? slice_bytes : PfGzEncoder::BLOCK;
    std::vector<uint64_t> row_off;
    PFCHK(hp_measure(c, "pf_pattern_rows_stream_begin", pids, P, S.order, S.rlen, row_off));
    EndUnlessOpen guard{c};
    PFCHK(ts_begin(c, {TextStream::PATTERN_ROWS, pr_write, pr_drop}));
    // ---- the slices: cut between rows, a slice of at most `cap` bytes or of one row; each is a range and one block
    S.row_off.swap(row_off);
    S.cut.assign(1, 0);
    std::vector<TextStream::Range> ranges;
    uint64_t max_bytes = 0, max_rows = 0;
    for (uint32_t i = 1; i <= P; i++)
        if (i == P || S.row_off[i + 1] - S.row_off[S.cut.back()] > cap) {
            const uint64_t first = S.cut.back();
            ranges.push_back({S.row_off[first], S.row_off[i] - S.row_off[first]});
            max_bytes = std::max(max_bytes, ranges.back().bytes);
            max_rows = std::max(max_rows, i - first);
            S.cut.push_back(i);
        }
    for (int b = 0; b < 2 && P; b++) {
        PFCHK(S.rowoff[b].ensure((size_t)(max_rows + 1) * 8));
        PFCHK(S.pin_rowoff[b].ensure((size_t)(max_rows + 1) * 8));
    }
    PFCHK(ts_open(c, std::move(ranges), max_bytes));
    PFCHK(ts_hand_out(c));
    *total_text_bytes = S.row_off[P];
    *n_slices = (uint32_t)S.cut.size() - 1;
    guard.ok = true;
    return PF_OK;
}

int pf_pattern_rows_stream_next(pf_ctx* c, const char** ptr, uint64_t* nbytes) {
    if (!c || !ptr || !nbytes) return fail(PF_ERR_ARG, "pf_pattern_rows_stream_next: null argument");
    *ptr = nullptr; *nbytes = 0;
    if (c->ts.kind != TextStream::PATTERN_ROWS) return fail(PF_ERR_STATE, "pf_pattern_rows_stream_next without an open pf_pattern_rows_stream_begin");
    return ts_next(c, ptr, nbytes);
}

int pf_render_device(pf_ctx* c, const char* const* names, const char* extra_keys, uint64_t n_extra,
                     const char** kh, uint64_t* kh_bytes, const char** hp, uint64_t* hp_bytes) {
    return pf_render_device_ex(c, names, extra_keys, n_extra, 0, kh, kh_bytes, hp, hp_bytes);
}

namespace {
// pf_render_device's host layout: the counts come down, then rows per cluster and workgroups per cluster
// (kmers_to_hashes), the new patterns in first-seen order (hashes_to_patterns), and the one block of tables (`meta`, with
// the o_* offsets into it) both kernels read
struct RenderLayout {
    uint32_t C = 0, P = 0, n_blocks = 0, rows_per_block = 256;
    uint64_t kh_n = 0, hp_n = 0, hp_at = 0;        // the two texts' bytes; the second starts 256-byte aligned
    size_t o_text = 0, o_koff = 0, o_rowoff = 0, o_name = 0, o_kcnt = 0, o_arena = 0, o_bc = 0, o_br = 0, o_order = 0, o_blob = 0, o_extra = 0;
    std::vector<char> meta;
    // multiple_files (cluster_ends asked for): per cluster, the offset behind its rows in each text
    bool cluster_ends = false;
    std::vector<uint64_t> kh_end, hp_end;
};
int render_layout(pf_ctx* c, const char* const* names, const char* extra_keys, uint64_t n_extra, bool want_hp, RenderLayout& L) {
    const uint32_t C = L.C = c->n_clusters, k = c->o.klength;
    hipStream_t st = c->stream;
    // ---- small per-cluster / per-pattern arrays to the host: counts and the first-seen order
    std::vector<uint64_t> koff(C);
    std::vector<uint32_t> kcnt(C);
    if (C) {
        HIPCHK(hipMemcpyAsync(koff.data(), c->batch.cl_kmer_off.p, (size_t)C * 8, hipMemcpyDeviceToHost, st));
        HIPCHK(hipMemcpyAsync(kcnt.data(), c->batch.cl_kmer_cnt.p, (size_t)C * 4, hipMemcpyDeviceToHost, st));
    }
    const uint32_t p0 = c->pid0, p1 = c->n_patterns, P = L.P = want_hp ? p1 - p0 : 0;
    std::vector<uint64_t> fs(P);
    std::vector<uint32_t> rlen(P);
    DevBuf d_rlen;
    if (P) {
        PFCHK(d_rlen.ensure((size_t)P * 4));
        PFCHK(hp_rowlen(c, nullptr, p0, P, d_rlen.as<uint32_t>()));
        HIPCHK(hipMemcpyAsync(fs.data(), c->pt.first_seen + p0, (size_t)P * 8, hipMemcpyDeviceToHost, st));
        HIPCHK(hipMemcpyAsync(rlen.data(), d_rlen.p, (size_t)P * 4, hipMemcpyDeviceToHost, st));
    }
    uint64_t ord0 = 0;                             // the batch's first ordinal: first_seen >> 32 counts from it
    if (L.cluster_ends && C) HIPCHK(hipMemcpyAsync(&ord0, c->last.cluster_ordinal, 8, hipMemcpyDeviceToHost, st));
    PFCHK(ensure_b64_dev(c));
    HIPCHK(hipStreamSynchronize(st));
    // ---- kmers_to_hashes layout: rows per cluster, workgroups per cluster
    std::vector<uint64_t> text_off(C + 1, 0);
    std::vector<uint32_t> name_off(C + 1, 0), arena_of(C), blk_cluster, blk_row0;
    std::string blob;
    for (uint32_t i = 0; i < C; i++) {
        const uint32_t len = (uint32_t)strlen(names[i]);
        blob.append(names[i], len);
        name_off[i + 1] = (uint32_t)blob.size();
        const uint64_t head = pf::kh_head_len(len), rowlen = pf::kh_row_len(len, k);
        if (head + rowlen > pf::TEXT_TILE) return fail(PF_ERR_ARG, "cluster name too long for the text kernel (%u bytes)", len);
        L.rows_per_block = std::min<uint32_t>(L.rows_per_block, (uint32_t)((pf::TEXT_TILE - head) / rowlen));
        text_off[i + 1] = text_off[i] + head + (uint64_t)kcnt[i] * rowlen;
        const uint32_t a = c->cluster_arena[i];
        arena_of[i] = a;
        koff[i] = kcnt[i] ? koff[i] - c->arenas[a]->base : 0;
    }
    for (uint32_t i = 0; i < C; i++)
        for (uint32_t r = 0; r < kcnt[i] + 1; r += L.rows_per_block) { blk_cluster.push_back(i); blk_row0.push_back(r); }
    L.n_blocks = (uint32_t)blk_cluster.size();
    // ---- hashes_to_patterns layout: new patterns in first-seen order
    std::vector<uint32_t> order(P);
    std::iota(order.begin(), order.end(), 0u);
    std::sort(order.begin(), order.end(), [&](uint32_t x, uint32_t y) { return fs[x] < fs[y]; });
    std::vector<uint64_t> row_off(P + 1, 0);
    if (L.cluster_ends) {
        // the new patterns in first-seen order (ordinal << 32 | rank) stand cluster by cluster: cut where the ordinal changes
        L.kh_end.assign(text_off.begin() + 1, text_off.end());
        L.hp_end.assign(C, 0);
        uint32_t ci = 0;
        for (uint32_t i = 0; i < P; i++) {
            const uint64_t at = (uint32_t)((fs[order[i]] >> 32) - ord0);     // (the ordinal's low 32 bits are in first_seen)
            if (at >= C || at < ci) return fail(PF_ERR_STATE, "a pattern's first_seen names no cluster of this batch");
            for (; ci < at; ci++) L.hp_end[ci] = row_off[i];
            row_off[i + 1] = row_off[i] + rlen[order[i]];
        }
        for (; ci < C; ci++) L.hp_end[ci] = row_off[P];
        for (uint32_t i = 0; i < P; i++) order[i] += p0;
    } else
        for (uint32_t i = 0; i < P; i++) { row_off[i + 1] = row_off[i] + rlen[order[i]]; order[i] += p0; }
    L.kh_n = text_off[C]; L.hp_n = row_off[P];
    L.hp_at = (L.kh_n + 255) & ~(uint64_t)255;
    // ---- one block of tables for both kernels
    auto pad8 = [](size_t x) { return (x + 7) & ~(size_t)7; };
    size_t o = 0;
    L.o_text = o; o += pad8((size_t)(C + 1) * 8);
    L.o_koff = o; o += pad8((size_t)C * 8);
    L.o_rowoff = o; o += pad8((size_t)(P + 1) * 8);
    L.o_name = o; o += pad8((size_t)(C + 1) * 4);
    L.o_kcnt = o; o += pad8((size_t)C * 4);
    L.o_arena = o; o += pad8((size_t)C * 4);
    L.o_bc = o; o += pad8(blk_cluster.size() * 4);
    L.o_br = o; o += pad8(blk_row0.size() * 4);
    L.o_order = o; o += pad8((size_t)P * 4);
    L.o_blob = o; o += pad8(blob.size() + 1);
    L.o_extra = o; o += pad8((size_t)n_extra * k + 1);
    std::vector<char>& meta = L.meta;
    meta.assign(o, 0);
    memcpy(&meta[L.o_text], text_off.data(), (size_t)(C + 1) * 8);
    if (C) memcpy(&meta[L.o_koff], koff.data(), (size_t)C * 8);
    memcpy(&meta[L.o_rowoff], row_off.data(), (size_t)(P + 1) * 8);
    memcpy(&meta[L.o_name], name_off.data(), (size_t)(C + 1) * 4);
    if (C) { memcpy(&meta[L.o_kcnt], kcnt.data(), (size_t)C * 4); memcpy(&meta[L.o_arena], arena_of.data(), (size_t)C * 4); }
    if (!blk_cluster.empty()) { memcpy(&meta[L.o_bc], blk_cluster.data(), blk_cluster.size() * 4); memcpy(&meta[L.o_br], blk_row0.data(), blk_row0.size() * 4); }
    if (P) memcpy(&meta[L.o_order], order.data(), (size_t)P * 4);
    if (!blob.empty()) memcpy(&meta[L.o_blob], blob.data(), blob.size());
    if (n_extra && extra_keys) memcpy(&meta[L.o_extra], extra_keys, (size_t)n_extra * k);
    return PF_OK;
}

// the tables up and the two launches: kmers_to_hashes from txt.dev on, hashes_to_patterns from txt.dev + hp_at
int render_launch(pf_ctx* c, const RenderLayout& L) {
    hipStream_t st = c->stream;
    PFCHK(c->txt.dev.ensure(L.hp_at + L.hp_n + 16));
    PFCHK(c->txt.meta.ensure(L.meta.size()));
    HIPCHK(hipMemcpyAsync(c->txt.meta.p, L.meta.data(), L.meta.size(), hipMemcpyHostToDevice, st));
    const char* dm = c->txt.meta.as<char>();
    if (L.n_blocks) {
        pf::KhTextParams kp{};
        kp.text_off = (const uint64_t*)(dm + L.o_text); kp.name_off = (const uint32_t*)(dm + L.o_name); kp.names = dm + L.o_blob;
        kp.kmer_off = (const uint64_t*)(dm + L.o_koff); kp.kmer_cnt = (const uint32_t*)(dm + L.o_kcnt);
        kp.cluster_pattern = c->batch.cl_pattern.as<uint32_t>(); kp.cluster_arena = (const uint32_t*)(dm + L.o_arena);
        kp.block_cluster = (const uint32_t*)(dm + L.o_bc); kp.block_row0 = (const uint32_t*)(dm + L.o_br);
        for (size_t a = 0; a < c->n_passes; a++) { kp.arena_key[a] = c->arenas[a]->key.as<uint64_t>(); kp.arena_pid[a] = c->arenas[a]->pid.as<uint32_t>(); }
        kp.b64 = c->pats.b64.as<char>(); kp.extra_keys = dm + L.o_extra; kp.text = c->txt.dev.as<char>();
        kp.k = c->o.klength; kp.KW = (uint32_t)c->KW; kp.rows_per_block = L.rows_per_block;
        hipLaunchKernelGGL(pf::kh_text_kernel, dim3(L.n_blocks), dim3(256), 0, st, kp);
        HIPCHK(hipGetLastError());
    }
    if (L.P) PFCHK(hp_text(c, (const uint32_t*)(dm + L.o_order), (const uint64_t*)(dm + L.o_rowoff), L.P, c->txt.dev.as<char>() + L.hp_at));
    return PF_OK;
}

// The hand-out of a render: two spans of device text, written on c->stream, leave through one pinned block, the second
// at a 256-aligned offset -- as they are, or under device gzip as their members: both texts go through the encoder behind
// their kernels, the two compressed sizes come back, then only members cross to the host.
struct Span { const char* p; uint64_t n; };
// (under device gzip) where the members of each text must end: n text offsets per text, and where the offsets behind
// each segment's members go
struct MemberCuts { uint64_t n; const uint64_t* end0; const uint64_t* end1; uint64_t* member_end0; uint64_t* member_end1; };
int render_handout(pf_ctx* c, Span text0, Span text1, Span* out0, Span* out1, const MemberCuts* cuts = nullptr) {
    hipStream_t st = c->stream;
    GzMode& G = c->gz;
    if (G.on) {
        HIPCHK(hipStreamSynchronize(c->side));             // (the encoder's scratch is one: no block of a stream in flight)
        const uint64_t one0 = text0.n, one1 = text1.n, nseg0 = cuts ? cuts->n : (one0 ? 1 : 0), nseg1 = cuts ? cuts->n : (one1 ? 1 : 0);
        const uint64_t* end0 = cuts ? cuts->end0 : &one0;
        const uint64_t* end1 = cuts ? cuts->end1 : &one1;
        const uint64_t b0 = PfGzEncoder::bound_segments(text0.n, cuts ? cuts->n : 0), b1 = PfGzEncoder::bound_segments(text1.n, cuts ? cuts->n : 0);
        PFCHK(G.render_members.ensure(b0 + b1 + 16));
        char* M = G.render_members.as<char>();
        PFCHK(G.enc.encode_segments(st, PfGzEncoder::RENDER_KMERS_TO_HASHES, text0.p, text0.n, end0, nseg0, G.flags, M, b0));
        PFCHK(G.enc.encode_segments(st, PfGzEncoder::RENDER_HASHES_TO_PATTERNS, text1.p, text1.n, end1, nseg1, G.flags, M + b0, b1));
        HIPCHK(hipStreamSynchronize(st));
        G.raw[0] = text0.n; G.raw[1] = text1.n;
        text0.p = M; text1.p = M + b0;
        PFCHK(G.enc.member_bytes(PfGzEncoder::RENDER_KMERS_TO_HASHES, &text0.n));
        PFCHK(G.enc.member_bytes(PfGzEncoder::RENDER_HASHES_TO_PATTERNS, &text1.n));
        if (cuts && cuts->n) {
            PFCHK(G.enc.segment_ends(PfGzEncoder::RENDER_KMERS_TO_HASHES, cuts->member_end0));
            PFCHK(G.enc.segment_ends(PfGzEncoder::RENDER_HASHES_TO_PATTERNS, cuts->member_end1));
        }
    }
    const uint64_t at1 = (text0.n + 255) & ~(uint64_t)255;
    char* pin;
    PFCHK(c->txt.next_pin(at1 + text1.n + 16, &pin));
    if (text0.n) HIPCHK(hipMemcpyAsync(pin, text0.p, text0.n, hipMemcpyDeviceToHost, st));
    if (text1.n) HIPCHK(hipMemcpyAsync(pin + at1, text1.p, text1.n, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    *out0 = Span{pin, text0.n}; *out1 = Span{pin + at1, text1.n};
    return PF_OK;
}
}  // namespace

namespace {
// pf_render_device_ex and pf_render_device_clusters behind their own checks: the layout (L.cluster_ends set by the
// caller), the two launches, the hand-out
int render_device(pf_ctx* c, const char* const* names, const char* extra_keys, uint64_t n_extra, bool want_hp, RenderLayout& L,
                  const char** kh, uint64_t* kh_bytes, const char** hp, uint64_t* hp_bytes, uint64_t* kh_member_end = nullptr,
                  uint64_t* hp_member_end = nullptr) {
    if (!c->have_batch) return fail(PF_ERR_STATE, "pf_render_device needs a successful pf_submit");
    HIPCHK(hipSetDevice(c->device));
    if (c->n_clusters && !names) return fail(PF_ERR_ARG, "pf_render_device: cluster names missing");
    if (c->n_passes > pf::TEXT_MAX_ARENAS) return fail(PF_ERR_CAPACITY, "pf_render_device: too many passes (%u)", c->n_passes);
    PFCHK(render_layout(c, names, extra_keys, n_extra, want_hp, L));
    PFCHK(render_launch(c, L));
    Span out0, out1;
    // (members cut at the clusters' ends: the ends render_layout has just computed)
    const MemberCuts cuts{c->n_clusters, L.kh_end.data(), L.hp_end.data(), kh_member_end, hp_member_end};
    PFCHK(render_handout(c, Span{c->txt.dev.as<char>(), L.kh_n}, Span{c->txt.dev.as<char>() + L.hp_at, L.hp_n}, &out0, &out1,
                         kh_member_end ? &cuts : nullptr));
    *kh = out0.p; *kh_bytes = out0.n;
    *hp = out1.p; *hp_bytes = out1.n;
    return PF_OK;
}
}  // namespace

int pf_render_device_ex(pf_ctx* c, const char* const* names, const char* extra_keys, uint64_t n_extra, uint32_t flags,
                        const char** kh, uint64_t* kh_bytes, const char** hp, uint64_t* hp_bytes) {
    if (!c || !kh || !kh_bytes || !hp || !hp_bytes) return fail(PF_ERR_ARG, "pf_render_device: null argument");
    if (c->have_batch && c->o.multiple_files) return fail(PF_ERR_ARG, "pf_render_device writes one pair of texts per batch; pf_render_device_clusters says where to cut them under multiple_files");
    RenderLayout L;
    return render_device(c, names, extra_keys, n_extra, !(flags & PF_RENDER_NO_PATTERN_ROWS), L, kh, kh_bytes, hp, hp_bytes);
}

int pf_render_device_clusters(pf_ctx* c, const char* const* names, const char* extra_keys, uint64_t n_extra,
                              const char** kh, uint64_t* kh_bytes, const char** hp, uint64_t* hp_bytes,
                              uint64_t* kh_end, uint64_t* hp_end) {
    if (!c || !kh || !kh_bytes || !hp || !hp_bytes) return fail(PF_ERR_ARG, "pf_render_device_clusters: null argument");
    if (!c->o.multiple_files) return fail(PF_ERR_ARG, "pf_render_device_clusters is for a context made with multiple_files; pf_render_device otherwise");
    if (c->have_batch && c->n_clusters && (!kh_end || !hp_end)) return fail(PF_ERR_ARG, "pf_render_device_clusters: null argument");
    if (c->gz.on) return fail(PF_ERR_STATE, "pf_render_device_clusters hands out text, not gzip members: the clusters' files are cut from it");
    RenderLayout L;
    L.cluster_ends = true;
    PFCHK(render_device(c, names, extra_keys, n_extra, true, L, kh, kh_bytes, hp, hp_bytes));
    if (c->n_clusters) {
        memcpy(kh_end, L.kh_end.data(), (size_t)c->n_clusters * 8);
        memcpy(hp_end, L.hp_end.data(), (size_t)c->n_clusters * 8);
    }
    return PF_OK;
}

int pf_render_device_cluster_members(pf_ctx* c, const char* const* names, const char* extra_keys, uint64_t n_extra,
                                     const char** kh, uint64_t* kh_bytes, const char** hp, uint64_t* hp_bytes,
                                     uint64_t* kh_end, uint64_t* hp_end, uint64_t* kh_text_end, uint64_t* hp_text_end) {
    if (!c || !kh || !kh_bytes || !hp || !hp_bytes) return fail(PF_ERR_ARG, "pf_render_device_cluster_members: null argument");
    if (!c->o.multiple_files) return fail(PF_ERR_ARG, "pf_render_device_cluster_members is for a context made with multiple_files");
    if (!c->gz.on) return fail(PF_ERR_STATE, "pf_render_device_cluster_members hands out gzip members: pf_set_device_gzip first, or pf_render_device_clusters for text");
    if (c->have_batch && c->n_clusters && (!kh_end || !hp_end || !kh_text_end || !hp_text_end))
        return fail(PF_ERR_ARG, "pf_render_device_cluster_members: null argument");
    RenderLayout L;
    L.cluster_ends = true;
    uint64_t none = 0;              // (a batch without clusters: no segment, nothing to report)
    PFCHK(render_device(c, names, extra_keys, n_extra, true, L, kh, kh_bytes, hp, hp_bytes, kh_end ? kh_end : &none, hp_end ? hp_end : &none));
    if (c->n_clusters) {
        memcpy(kh_text_end, L.kh_end.data(), (size_t)c->n_clusters * 8);
        memcpy(hp_text_end, L.hp_end.data(), (size_t)c->n_clusters * 8);
    }
    return PF_OK;
}

int pf_set_device_gzip(pf_ctx* c, int on, uint32_t flags) {
    if (!c) return fail(PF_ERR_ARG, "pf_set_device_gzip: null argument");
    PFCHK(gz_check_flags(flags, "pf_set_device_gzip"));
    HIPCHK(hipSetDevice(c->device));
    ts_end(c);                            // (an open stream would change its kind half way)
    if (on) PFCHK(c->gz.enc.ensure(c->n_cu));
    c->gz.on = on != 0; c->gz.flags = flags;
    return PF_OK;
}

int pf_device_gzip_text_bytes(pf_ctx* c, uint64_t out[3]) {
    if (!c || !out) return fail(PF_ERR_ARG, "pf_device_gzip_text_bytes: null argument");
    for (int i = 0; i < 3; i++) out[i] = c->gz.raw[i];
    return PF_OK;
}

int pf_gzip_device_last_ms(pf_ctx* c, float* ms) {
    if (!c || !ms) return fail(PF_ERR_ARG, "pf_gzip_device_last_ms: null argument");
    *ms = c->gz.encode_ms;
    return PF_OK;
}

int pf_gzip_device(pf_ctx* c, const char* data, uint64_t n, uint32_t flags, char** out, uint64_t* out_n) {
    if (!c || (!data && n) || !out || !out_n) return fail(PF_ERR_ARG, "pf_gzip_device: null argument");
    PFCHK(gz_check_flags(flags, "pf_gzip_device"));
    *out = nullptr; *out_n = 0;
    if (!n) {
        if (!(*out = (char*)malloc(1))) return fail(PF_ERR_OOM, "pf_gzip_device: out of memory");
        return PF_OK;
    }
    HIPCHK(hipSetDevice(c->device));
    PfGzEncoder& enc = c->gz.enc;
    constexpr PfGzEncoder::Cursor W = PfGzEncoder::RENDER_KMERS_TO_HASHES;      // (a render's: neither is on its way now)
    PFCHK(enc.ensure(c->n_cu));
    HIPCHK(hipStreamSynchronize(c->side));
    hipStream_t st = c->stream;
    DevBuf text, members;
    const uint64_t cap = PfGzEncoder::bound(n);
    PFCHK(text.ensure(n + 16, true));
    PFCHK(members.ensure(cap, true));
    HIPCHK(hipMemcpyAsync(text.p, data, n, hipMemcpyHostToDevice, st));
    HipEvent e0, e1;
    PFCHK(get_event(c, &e0)); PFCHK(get_event(c, &e1));
    // (the two events go back to the pool whichever step fails)
    auto encode = [&]() -> int {
        PFCHK(enc.encode(st, W, text.as<char>(), n, flags, members.as<char>(), cap, e0, e1));
        HIPCHK(hipStreamSynchronize(st));
        c->gz.encode_ms = 0.f;
        HIPCHK(hipEventElapsedTime(&c->gz.encode_ms, e0, e1));
        return PF_OK;
    };
    const int enc_rc = encode();
    c->ev_pool.push_back(std::move(e0)); c->ev_pool.push_back(std::move(e1));
    PFCHK(enc_rc);
    uint64_t z = 0;
    PFCHK(enc.member_bytes(W, &z));
    char* buf = (char*)malloc(z ? z : 1);
    if (!buf) return fail(PF_ERR_OOM, "pf_gzip_device: out of memory");
    const hipError_t e = hipMemcpy(buf, members.p, z, hipMemcpyDeviceToHost);
    if (e != hipSuccess) { free(buf); return fail(PF_ERR_HIP, "pf_gzip_device: copy failed: %s", hipGetErrorString(e)); }
    *out = buf; *out_n = z;
    return PF_OK;
}

int pf_gzip_device_segments(pf_ctx* c, const char* data, uint64_t n, const uint64_t* seg_end, uint64_t n_seg, uint32_t flags,
                            char** out, uint64_t* out_n, uint64_t* member_end) {
    if (!c || (!data && n) || (!seg_end && n_seg) || (!member_end && n_seg) || !out || !out_n)
        return fail(PF_ERR_ARG, "pf_gzip_device_segments: null argument");
    PFCHK(gz_check_flags(flags, "pf_gzip_device_segments"));
    *out = nullptr; *out_n = 0;
    HIPCHK(hipSetDevice(c->device));
    PfGzEncoder& enc = c->gz.enc;
    constexpr PfGzEncoder::Cursor W = PfGzEncoder::RENDER_KMERS_TO_HASHES;      // (a render's: neither is on its way now)
    PFCHK(enc.ensure(c->n_cu));
    HIPCHK(hipStreamSynchronize(c->side));
    hipStream_t st = c->stream;
    DevBuf text, members;
    const uint64_t cap = PfGzEncoder::bound_segments(n, n_seg);
    PFCHK(text.ensure(n + 16, true));
    PFCHK(members.ensure(cap + 16, true));
    if (n) HIPCHK(hipMemcpyAsync(text.p, data, n, hipMemcpyHostToDevice, st));
    PFCHK(enc.encode_segments(st, W, text.as<char>(), n, seg_end, n_seg, flags, members.as<char>(), cap));
    HIPCHK(hipStreamSynchronize(st));
    uint64_t z = 0;
    PFCHK(enc.member_bytes(W, &z));
    if (n_seg) PFCHK(enc.segment_ends(W, member_end));
    char* buf = (char*)malloc(z ? z : 1);
    if (!buf) return fail(PF_ERR_OOM, "pf_gzip_device_segments: out of memory");
    const hipError_t e = z ? hipMemcpy(buf, members.p, z, hipMemcpyDeviceToHost) : hipSuccess;
    if (e != hipSuccess) { free(buf); return fail(PF_ERR_HIP, "pf_gzip_device_segments: copy failed: %s", hipGetErrorString(e)); }
    *out = buf; *out_n = z;
    return PF_OK;
}

int pf_gunzip_device_last_ms(pf_ctx* c, float* ms) {
    if (!c || !ms) return fail(PF_ERR_ARG, "pf_gunzip_device_last_ms: null argument");
    *ms = c->gz.decode_ms;
    return PF_OK;
}

// pf_gunzip_device and pf_gunzip_device_bgzf, each under its own name `fn`: the members listed by signature, or by the BSIZE chain
static int gunzip_device(pf_ctx* c, const char* members, uint64_t n, char** out, uint64_t* out_n, int* taken, bool bgzf, const char* fn) {
    if (!c || (!members && n) || !out || !out_n || !taken) return fail(PF_ERR_ARG, "%s: null argument", fn);
    *out = nullptr; *out_n = 0; *taken = 0;
    c->gz.decode_ms = 0.f;
    const uint8_t* bytes = reinterpret_cast<const uint8_t*>(members);
    std::vector<pfgz::MemberRef> ms;
    uint64_t consumed = 0;
    if (!(bgzf ? pfgz::list_members_bgzf(bytes, n, true, ms, &consumed) : pfgz::list_members(bytes, n, true, ms, &consumed))) {
        (void)fail(PF_OK, "%s: not taken: member 0: %s", fn, pfgz::inf_status_name(pfgz::INF_BAD_HEAD));
        return PF_OK;
    }
    const int64_t bad = pfgz::first_refused(ms);
    if (bad >= 0) {
        (void)fail(PF_OK, "%s: not taken: member %lld: %s", fn, (long long)bad, pfgz::inf_status_name(ms[(size_t)bad].status));
        return PF_OK;
    }
    uint64_t total = 0;
    for (const auto& m : ms) total += m.isize;
    std::unique_ptr<char, void (*)(void*)> buf((char*)malloc(total ? total : 1), free);
    if (!buf) return fail(PF_ERR_OOM, "%s: out of memory", fn);
    HIPCHK(hipSetDevice(c->device));
    hipStream_t st = c->stream;
    DevBuf text;
    HipEvent e0, e1;
    PFCHK(get_event(c, &e0)); PFCHK(get_event(c, &e1));
    // a call of the decoder per MAX_MEMBERS members and MAX_TEXT bytes of text (what is on the device at a time)
    auto decode = [&]() -> int {
        uint64_t at = 0;
        for (size_t i = 0, k = 0; i < ms.size(); i += k) {
            uint64_t part = 0;
            for (k = 0; i + k < ms.size() && k < PfGzDecoder::MAX_MEMBERS && (!k || part + ms[i + k].isize <= PfGzDecoder::MAX_TEXT); k++)
                part += ms[i + k].isize;
            PFCHK(text.ensure(part + 16));
            PFCHK(c->gz.dec.decode(st, bytes, ms.data() + i, (uint32_t)k, text.as<uint8_t>(), part, e0, e1));
            HIPCHK(hipStreamSynchronize(st));
            float t = 0.f;
            HIPCHK(hipEventElapsedTime(&t, e0, e1));
            c->gz.decode_ms += t;
            uint32_t status = 0;
            const int64_t r = c->gz.dec.first_refused(&status);
            if (r >= 0) {
                (void)fail(PF_OK, "%s: not taken: member %lld: %s", fn, (long long)(i + (size_t)r), pfgz::inf_status_name(status));
                return 1;
            }
            if (part) HIPCHK(hipMemcpy(buf.get() + at, text.p, part, hipMemcpyDeviceToHost));
            at += part;
        }
        return PF_OK;
    };
    const int rc = decode();
    c->ev_pool.push_back(std::move(e0)); c->ev_pool.push_back(std::move(e1));
    if (rc == 1) return PF_OK;                  // not taken
    PFCHK(rc);
    *out = buf.release(); *out_n = total; *taken = 1;
    return PF_OK;
}

int pf_gunzip_device(pf_ctx* c, const char* members, uint64_t n, char** out, uint64_t* out_n, int* taken) {
    return gunzip_device(c, members, n, out, out_n, taken, false, "pf_gunzip_device");
}

int pf_gunzip_device_bgzf(pf_ctx* c, const char* members, uint64_t n, char** out, uint64_t* out_n, int* taken) {
    return gunzip_device(c, members, n, out, out_n, taken, true, "pf_gunzip_device_bgzf");
}

// The whole buffer by the large-member route, every member alone, call after call as a text feed gives them (last = 1:
// all the bytes are there), the text of each call copied out behind it
int pf_gunzip_device_large(pf_ctx* c, const char* members, uint64_t n, uint32_t piece_bytes, char** out, uint64_t* out_n, int* taken,
                           uint64_t* pieces) {
    if (!c || (!members && n) || !out || !out_n || !taken) return fail(PF_ERR_ARG, "pf_gunzip_device_large: null argument");
    *out = nullptr; *out_n = 0; *taken = 0;
    if (piece_bytes && piece_bytes < pfgz::PIECE_MIN) return fail(PF_ERR_ARG, "pf_gunzip_device_large: piece_bytes is 0 or at least %u", pfgz::PIECE_MIN);
    HIPCHK(hipSetDevice(c->device));
    PfGzLarge& be = c->gz.large;
    be.st = c->stream;
    DevBuf text;
    be.place = [&](uint64_t text_n, uint8_t** dst) -> int { PFCHK(text.ensure(text_n + 16)); *dst = text.as<uint8_t>(); return PF_OK; };
    std::vector<char> all;
    pfgz::LargeState s;
    pfgz::LargeStats stats;
    const float before = be.ms[0] + be.ms[1] + be.ms[2] + be.ms[3];
    const uint8_t* bytes = reinterpret_cast<const uint8_t*>(members);
    uint32_t status = pfgz::INF_OK;
    bool ok = true;
    for (uint64_t at = 0; at < n && ok;) {
        pfgz::LargeOut o;
        PFCHK(pfgz::large_call(be, s, stats, bytes + at, n - at, true, piece_bytes, o));
        if (!o.taken || !o.consumed) { ok = false; status = o.status ? o.status : (uint32_t)pfgz::INF_NOT_DECODED; break; }
        const size_t had = all.size();
        all.resize(had + o.text_n);
        if (o.text_n) HIPCHK(hipMemcpy(all.data() + had, text.p, o.text_n, hipMemcpyDeviceToHost));
        at += o.consumed;
    }
    if (ok && s.open) { ok = false; status = pfgz::INF_TRUNCATED; }
    be.place = nullptr;
    c->gz.decode_ms = be.ms[0] + be.ms[1] + be.ms[2] + be.ms[3] - before;
    if (pieces) { pieces[0] = stats.found; pieces[1] = stats.live; pieces[2] = stats.dropped; pieces[3] = stats.members; }
    if (!ok) {
        (void)fail(PF_OK, "pf_gunzip_device_large: not taken: member %llu: %s", (unsigned long long)stats.members, pfgz::inf_status_name(status));
        return PF_OK;
    }
    char* buf = (char*)malloc(all.size() ? all.size() : 1);
    if (!buf) return fail(PF_ERR_OOM, "pf_gunzip_device_large: out of memory");
    if (!all.empty()) memcpy(buf, all.data(), all.size());
    *out = buf; *out_n = all.size(); *taken = 1;
    return PF_OK;
}

#ifdef PF_PROF
/* profiling builds only (not part of the ABI): cycles per kernel phase, see PF_PROF_STAMP in pf_kernels.h */
int pf_debug_prof(uint64_t* out, int reset) {
    if (out && hipMemcpyFromSymbol(out, HIP_SYMBOL(pf::pf_prof), sizeof(uint64_t) * 64) != hipSuccess) return PF_ERR_HIP;
    if (reset) {
        static const uint64_t zero[64] = {};
        if (hipMemcpyToSymbol(HIP_SYMBOL(pf::pf_prof), zero, sizeof zero) != hipSuccess) return PF_ERR_HIP;
    }
    return PF_OK;
}
#endif

#ifdef PF_WEAK_HASH
/* weak-hash test builds only (not part of the ABI): the mask the verified content hashes are ANDed with -- all sites, or one
   of PF_WHS_* -- and the counts of compares that failed behind an equal hash, see PF_WEAK in pf_kernels.h */
int pf_rowfilter_weakhash_mask(uint64_t mask);
int pf_rowfilter_weakhash_counts(uint64_t* rowfilter_rejects, uint64_t* strain_rejects, int reset);

int pf_debug_set_hash_mask_site(int site, uint64_t mask) {
    if (site < 0 || site >= pf::PF_WHS_N) return fail(PF_ERR_ARG, "pf_debug_set_hash_mask_site: no such site");
    if (site == pf::PF_WHS_TEXT) return pf_rowfilter_weakhash_mask(mask);
    const unsigned long long m = mask;
    if (hipMemcpyToSymbol(HIP_SYMBOL(pf::pf_wh_mask), &m, sizeof m, sizeof m * (size_t)site) != hipSuccess) return PF_ERR_HIP;
    return PF_OK;
}

int pf_debug_set_hash_mask(uint64_t mask) {
    for (int site = 0; site < pf::PF_WHS_N; site++) PFCHK(pf_debug_set_hash_mask_site(site, mask));
    return PF_OK;
}

int pf_debug_weakhash_counts(uint64_t out[8], int reset) {
    unsigned long long d[pf::PF_WHC_N] = {};
    if (hipMemcpyFromSymbol(d, HIP_SYMBOL(pf::pf_wh_count), sizeof d) != hipSuccess) return PF_ERR_HIP;
    uint64_t rf = 0, strain = 0;
    PFCHK(pf_rowfilter_weakhash_counts(&rf, &strain, reset));
    d[pf::PF_WHC_ROWFILTER] = rf; d[pf::PF_WHC_STRAIN] = strain;
    if (out) for (int i = 0; i < pf::PF_WHC_N; i++) out[i] = d[i];
    if (reset) {
        static const unsigned long long zero[pf::PF_WHC_N] = {};
        if (hipMemcpyToSymbol(HIP_SYMBOL(pf::pf_wh_count), zero, sizeof zero) != hipSuccess) return PF_ERR_HIP;
    }
    return PF_OK;
}
#endif

}  // extern "C"
