/*
 * panfeed_hip.h -- C ABI of libpanfeed_hip.so: panfeed's per-gene-cluster k-mer extraction and
 * presence/absence pattern hashing hot path on MI355X (gfx950).
 *
 * The reference has no FFI: the path sits behind two Python callables,
 *   cluster_cutter  /root/reference/panfeed/panfeed.py:23-113
 *   pattern_hasher  /root/reference/panfeed/panfeed.py:132-235
 * bound with functools.partial at /root/reference/panfeed/__main__.py:277-297 and called at
 * :352-356 (serial) / :47,:81 (worker, writer).  This header is what a binding for those two call
 * sites talks to (ctypes stub: INTEGRATION.md; in-repo mirror: panfeed_amd/panfeed.py).
 *
 * Conventions: every function returns 0 on success or a negative pf_status; the message of the
 * last failure on the calling thread is pf_last_error().  No C++ exception crosses the ABI.  All
 * pointers are plain host pointers unless a field says "device".  One pf_ctx per GPU, used from
 * one host thread at a time.
 */
#ifndef PANFEED_HIP_H
#define PANFEED_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct pf_ctx pf_ctx;

enum pf_status {
    PF_OK = 0,
    PF_ERR_ARG = -1,      /* bad argument / unsupported option */
    PF_ERR_OOM = -2,      /* host or device allocation failed */
    PF_ERR_HIP = -3,      /* a HIP runtime call failed */
    PF_ERR_CAPACITY = -4, /* a capacity that cannot grow was exceeded (work items per cluster, 2^31 patterns) */
    PF_ERR_STATE = -5     /* call order violated */
};

#define PF_MAX_K 126 /* 2 bits/base in at most four 63-bit key words */

/* Options of one run = the arguments functools.partial freezes at __main__.py:277-297. */
typedef struct {
    uint32_t klength;          /* -k ; 1..PF_MAX_K */
    uint32_t canon;            /* canon == True  (panfeed.py:69); 0 = --non-canonical */
    uint32_t consider_missing; /* consider_missing_cluster (panfeed.py:17-19, 193-196, 220-222) */
    uint32_t patfilt;          /* the value handed to pattern_hasher: the same-as-cluster filter
                                  runs when it is 0 (panfeed.py:202-204) */
    uint32_t multiple_files;   /* patterns set reset per cluster (panfeed.py:165) */
    uint32_t max_strains;      /* upper bound of len(cluster.keys()) and len(clusterpresab) */
    /* MAF filter (panfeed.py:190-200) as exact float64 semantics precomputed by the caller:
       a k-mer with `count` ones among `n` non-missing strains is kept iff
       maf_lo[n] <= count <= maf_hi[n]; arrays of max_strains+1 entries. */
    const uint32_t* maf_lo;
    const uint32_t* maf_hi;
    uint64_t pattern_capacity; /* initial slots of the run-global pattern table; 0 = default (2^24).  The table and
                                  its pool grow on demand (the reference's `patterns` is an unbounded set,
                                  panfeed.py:146-150): a batch that runs out of ids is re-run with a larger table */
    uint32_t max_items;        /* work items (cluster x key partition) in flight per internal sub-batch; 0 = default;
                                  clamped so that their scratch slices take at most half of the free device memory */
    uint32_t flags;            /* PF_FLAG_* */
} pf_opts;

/* Scan every segment even when a cluster holds identical copies of a sequence (same output, slower:
   by default only one representative per distinct sequence is scanned). */
#define PF_FLAG_NO_DEDUP 1u
/* With the shortcut above on: scan every 64-window unit of every distinct sequence even when distinct sequences of a
   cluster share it (same output, slower on clusters of many alleles: by default a unit that several alleles of a gene
   hold unchanged at the same place is scanned once for all of them). */
#define PF_FLAG_NO_UNIT_DEDUP 2u
/* A cluster whose distinct k-mers take three or more passes of the on-chip table (key partitions) has its windows sorted
   by partition first, so that every pass reads its own windows only.  With this flag every pass walks the whole cluster
   and keeps its share (same output, slower on clusters of many alleles). */
#define PF_FLAG_NO_KEY_BINNING 4u
/* Opt-in: the work items of a batch's simple clusters (at most 64 distinct sequences, one key partition, a fused finish
   class) are laid out by three small kernels right behind the dedup pass, and the host reads a 40-byte summary before it
   launches their scan (the reference's hand-off is a queue, __main__.py:39-52), building only the rest of the batch from
   the per-cluster records.  Same output.  What it is for: batches of a few thousand SIMPLE clusters that go through in one
   part, where the host's work lies on the critical path -- configs[1] (5 000 x 200) 1.337 -> 1.30 ms a pass, a rank's
   share of configs[3] (6 250 clusters) 2.53 -> 2.51 (profiles/r05/device_plan_ab_small_batches.txt).  Not the default: a
   50 000-cluster batch hides the host's work behind its other part's kernels (14.98 -> 15.18 ms with the plan), and in a
   batch that mixes simple clusters with many-allele ones the planned clusters' finish kernels run in front of the general
   path instead of beside it (the second stream). */
#define PF_FLAG_DEVICE_PLAN 8u

/*
 * One batch of gene clusters = the records iter_gene_clusters yields
 * (/root/reference/panfeed/input.py:455-468), already packed by the caller.
 *
 * A "segment" is a maximal run of A/C/G/T inside one Seqinfo.sequence (non-ACGT bases split a
 * sequence; the windows that contain one are the caller's slow path and come back in as
 * `extra_*` rows).  Packing: 2 bits per base (A=0 C=1 G=2 T=3), 32 bases per uint64 word, the first
 * base in bits 63:62; every segment starts on a 16-byte boundary; the buffer carries 16 bytes
 * of padding after the last segment (32 bytes when klength > 63: a lane reads up to four words past its window's
 * first one).
 *
 * Padding bits inside a segment's last 16 bytes are zero.  cluster_seg_off[0] == 0.
 * Inside a cluster the segments are sorted by seg_sample (stable).  A window starting at base
 * `pos` of a segment is instance number  seg_ord_base + pos  of the cluster in the reference's
 * iteration order (panfeed.py:54-64); in non-canonical mode the forward k-mer is instance
 * 2*(seg_ord_base+pos) and the reverse complement 2*(seg_ord_base+pos)+1 (panfeed.py:82-88).
 */
typedef struct {
    uint32_t n_clusters;
    uint32_t n_segs;
    uint64_t n_words;               /* uint64 words in `packed`, padding included */
    uint32_t on_device;             /* 1: every array below is a device pointer (bench / tests) */
    uint32_t reserved;
    const uint64_t* packed;
    const uint64_t* seg_word_off;   /* [n_segs]   word offset of the segment (even) */
    const uint32_t* seg_len;        /* [n_segs]   bases */
    const uint32_t* seg_sample;     /* [n_segs]   column in sorted(cluster.keys()) order (panfeed.py:47-49) */
    const uint32_t* seg_ord_base;   /* [n_segs] */
    const uint32_t* cluster_seg_off;  /* [n_clusters+1] */
    const uint32_t* cluster_nstrains; /* [n_clusters] len(cluster.keys()) */
    const uint32_t* cluster_npresab;  /* [n_clusters] len(clusterpresab) */
    const uint32_t* cluster_presab;   /* [n_clusters * W] clusterpresab as bits, W = ceil(max_strains/32) */
    const uint64_t* cluster_ordinal;  /* [n_clusters] position in the run's processing order */
    /* slow-path rows (k-mers containing a non-ACGT base), grouped by cluster, any order inside: */
    uint32_t n_extra;
    uint32_t reserved2;
    const uint32_t* extra_cluster;  /* [n_extra] batch-local cluster index, non-decreasing */
    const uint32_t* extra_ord;      /* [n_extra] first-occurrence instance number */
    const uint32_t* extra_bits;     /* [n_extra * W] presence bits */
    /* strand bits for positional rows (panfeed.py:69-75 used_strand; canonical mode only):
       seg_strand_off[s] = index of the first uint64 of segment s in the strand-bit stream, or
       0xFFFFFFFF to skip the segment; window pos -> bit (pos & 63) of word (pos >> 6);
       bit = 1 when the reverse complement is the canonical k-mer.  NULL = none wanted. */
    const uint32_t* seg_strand_off;
    uint64_t n_strand_words;
} pf_batch;

/* Result of pf_submit, valid until the next pf_submit / pf_destroy on the context. */
typedef struct {
    uint64_t n_instances;      /* trip count of panfeed.py:64 (x2 non-canonical), slow path excluded */
    uint64_t n_unique;         /* unique k-mers over all clusters (len(cluster_dict) summed) */
    uint64_t n_kept;           /* rows of kmers_to_hashes.tsv minus the per-cluster rows */
    uint64_t n_new_patterns;   /* rows this batch adds to hashes_to_patterns.tsv */
    uint32_t W;                /* uint32 words per presence row */
    uint32_t key_words;        /* KW = ceil(2k / 63): 1 (k <= 31), 2 (<= 63), 3 (<= 94), 4 (<= 126) */
    /* per cluster (batch order) */
    const uint64_t* cluster_kmer_off;  /* [n_clusters] first kept k-mer in kmer_* */
    const uint32_t* cluster_kmer_cnt;  /* [n_clusters] */
    const uint32_t* cluster_pattern;   /* [n_clusters] pattern id of the cluster row (panfeed.py:175-187) */
    const uint32_t* cluster_unique;    /* [n_clusters] len(cluster_dict) */
    /* per kept k-mer, in dict insertion order inside each cluster (panfeed.py:189) */
    const uint64_t* kmer_key;          /* [n_kept_total * key_words]: the k-mer's 2k-bit value (first base most
                                          significant), most significant word first, 63 bits per word; bit 63 of
                                          word 0 set: slow-path row, low 32 bits = index into the batch's extra_* arrays */
    const uint32_t* kmer_pattern;      /* [n_kept_total] pattern id */
    /* patterns first seen in this batch, sorted by first_seen = the order of hashes_to_patterns.tsv */
    const uint32_t* new_pattern_id;    /* [n_new_patterns] */
    /* run-global pattern pool, indexed by pattern id */
    uint64_t n_patterns;
    const uint8_t* pattern_md5;        /* [n_patterns * 16] md5 of the int64 / float64 image */
    const uint32_t* pattern_bits;      /* [n_patterns * W] */
    const uint32_t* pattern_nan;       /* [n_patterns * W] NaN positions (consider_missing), else NULL */
    const uint32_t* pattern_n;         /* [n_patterns] vector length; bit 31 set: int64 image (cluster row) */
    const uint64_t* pattern_first_seen;/* [n_patterns] cluster_ordinal << 32 | rank inside the cluster */
    const uint64_t* strand_bits;       /* [n_strand_words] or NULL */
} pf_result;

/* device-side timing of the last pf_submit, milliseconds (hipEvent on the context's stream) */
typedef struct {
    float total_ms;
    float scan_ms;     /* kmer_scan_kernel launches */
    float rows_ms;     /* rows_kernel */
    float emit_ms;     /* cluster_base_kernel + emit_kernel (+ extra_fill_kernel) */
    uint32_t scan_launches;
    uint32_t n_items;  /* (cluster, key-partition) work items scanned, retries included */
    uint32_t n_retried;/* clusters whose table overflowed and were re-run with more partitions */
    uint32_t n_dedup_clusters; /* clusters scanned through distinct-sequence representatives */
    uint64_t scan_packed_bytes; /* packed sequence bytes the scan kernels were asked to read */
    float dedup_ms;    /* cluster_dedup_kernel */
    float patrows_ms;  /* pattern_rows_kernel (emit_ms excludes it) */
    float md5_ms;      /* md5_kernel (emit_ms excludes it) */
    float finish_ms;   /* finish_kernel (fused rows+emit of single-item deduplicated clusters) */
    uint32_t n_wide_clusters;  /* clusters that went through the wide dedup class (more than 64 distinct sequences, ...) */
    uint32_t n_binned_clusters;/* clusters whose windows were sorted by key partition before the scan, retries included */
    uint32_t n_scratch_grown;  /* times the context re-made its scratch for a cluster of more work items than max_items (since pf_create) */
    uint32_t n_device_planned; /* clusters whose work items were laid out on the device (no host round trip before their scan) */
    uint32_t n_side_launches;  /* launches whose fused finish kernels ran on the context's second stream, beside the general path's */
    uint32_t reserved;
} pf_timing;

const char* pf_last_error(void);
const char* pf_version(void);

/* Number of visible HIP devices, or a negative pf_status. */
int pf_device_count(void);

int pf_create(pf_ctx** out, int device, const pf_opts* opts);
void pf_destroy(pf_ctx* ctx);

/* Forget the run-global patterns (a new run on the same context). */
int pf_reset_patterns(pf_ctx* ctx);

/* Run cluster_cutter + pattern_hasher over one batch.  Results stay on the device until
 * pf_fetch; `res` (may be NULL) receives the counters only. */
int pf_submit(pf_ctx* ctx, const pf_batch* batch, pf_result* counters);

/*
 * Genomes resident in HBM (SURVEY 8f N1 on the device).  pf_genomes_upload packs the contigs (A/C/G/T in either
 * case -> 2 bits, anything else -> an arbitrary code the caller must never ask for) into the context's genome
 * store and returns each contig's word offset.  pf_submit_gather is pf_submit for a batch whose packed input is
 * produced on the device: segment s is the range [src_start, src_start + seg_len) of the source at src_off --
 * the genome store, or (flag bit 0) b->packed, the words the host packed itself -- copied, or (flag bit 1)
 * reverse-complemented (what `-seq` of input.py:431,443 yields), to b->seg_word_off[s] of a device buffer of
 * g->n_words words.  Replaces the per-base host work of input.py:413-446 + the packing of the boundary.
 */
typedef struct {
    uint64_t n_words;
    const uint64_t* src_off; const uint32_t* src_start; const uint32_t* src_flags;   /* [b->n_segs] */
} pf_gather;
int pf_genomes_upload(pf_ctx* ctx, uint32_t n_contigs, const char* const* ascii, const uint64_t* len,
                      uint64_t* word_off_out);
int pf_genomes_clear(pf_ctx* ctx);
int pf_submit_gather(pf_ctx* ctx, const pf_batch* b, const pf_gather* g, pf_result* counters);

/* Copy the arrays of the last batch's result to host memory owned by the context. */
int pf_fetch(pf_ctx* ctx, pf_result* res);

int pf_get_timing(pf_ctx* ctx, pf_timing* t);

/* Multi-GPU (one process per GPU): first-seen bookkeeping for the run-global pattern dedup.
 * pf_export_patterns: (md5[16], first_seen) of every pattern this rank holds;
 * the driver all-gathers them (RCCL) and keeps, per digest, the rank with the lowest first_seen. */
int pf_export_patterns(pf_ctx* ctx, uint64_t* n, const uint8_t** md5, const uint64_t** first_seen);
/* Same, device to device: copies min(count, cap) entries into caller-owned DEVICE buffers
 * (d_md5: 16 B each, d_first_seen: 8 B each) so the all-gather can start from HBM. */
int pf_export_patterns_dev(pf_ctx* ctx, uint64_t cap, void* d_md5, void* d_first_seen, uint64_t* n);
/* After the all-gather: d_gathered (DEVICE) holds n_total rows {md5[0:8], md5[8:16], first_seen} (3 x uint64) of all
 * ranks; this rank's rows are [my_first, my_first+my_count).  Writes d_keep[j] = 1 (DEVICE, uint8) when this rank's
 * row j holds the lowest first_seen of its digest, and *n_global = number of distinct digests.  O(n_total) atomics
 * in a scratch hash table, no sort. */
int pf_merge_patterns(pf_ctx* ctx, const void* d_gathered, uint64_t n_total, uint64_t my_first, uint64_t my_count,
                      void* d_keep, uint64_t* n_global);
/* Same on the padded buffer all_gather_into_tensor leaves: `world` slots of slot_rows rows, of which the first
 * d_slot_counts[r] (DEVICE int64) are real; this rank's rows are the first my_count of slot `rank`. */
int pf_merge_patterns_padded(pf_ctx* ctx, const void* d_gathered, uint64_t world, uint64_t slot_rows,
                             const void* d_slot_counts, uint64_t rank, uint64_t my_count, void* d_keep,
                             uint64_t* n_global);
/* A checksum of checksums of the last pf_submit's results, computed on the device (no pf_fetch): out[0] = wrapping sum
 * over every kept k-mer of h(cluster index in the batch, its position in the cluster's output order, key words, MD5
 * digest of its pattern) -- i.e. of what its kmers_to_hashes.tsv row holds and where it stands (panfeed.py:208);
 * out[1] = the same per cluster over (kept, unique, digest of the cluster's own row, :177); out[2] = kept k-mers.
 * Independent of arena placement and pattern ids: two runs that would write the same files give the same three
 * numbers.  For parity checks at sizes no CPU checker covers (bench.py: identical-sequence shortcut on vs off at
 * BASELINE's full size; tests). */
int pf_result_checksum(pf_ctx* ctx, uint64_t out[3]);
/* Number of patterns in the run-global set after the last pf_submit. */
int pf_pattern_count(pf_ctx* ctx, uint64_t* n);
/* Test hook: pattern tables of more than max_slots slots are refused as if the device were out of memory (0: no
 * limit) -- the growth paths of the reference's unbounded `patterns` set (panfeed.py:146-150) have failure branches
 * that a 288 GB device never takes on its own. */
int pf_debug_limit_pattern_slots(pf_ctx* ctx, uint64_t max_slots);
/* Test hook, process-wide: a single device allocation of the library's growable buffers above max_bytes is refused as if
 * the device were out of memory (0: no limit).  stats (may be NULL) receives, and resets, what was seen since the last
 * call: stats[0] = the largest buffer size asked for, stats[1] = allocations whose size-plus-slack request failed and
 * whose exact-size retry succeeded.  A buffer's slack is a convenience: a run must not fail while the bytes it needs
 * exist (the reference's structures grow until the machine is full, panfeed.py:146-150). */
int pf_debug_limit_alloc(uint64_t max_bytes, uint64_t stats[2]);
/* Test hook, read-only: out[0 .. n) = words [first, first + n) of the genome store (which = 0: what pf_genomes_upload /
 * pf_pangenome_open_device packed, g_words of them) or of the device's packed-segment buffer of the last pf_submit /
 * pf_submit_gather (which = 1: that call's n_words, tails and padding included -- the input the dedup pass compares word
 * by word, which no output text shows).  Waits for the context's stream, copies with hipMemcpy; a range outside the
 * buffer is PF_ERR_ARG.  The buffer of which = 1 is the one the batch was scanned from: no stage writes to it.  It is the
 * context's own for a batch of host arrays and for pf_submit_gather; for a batch with on_device = 1 it is the caller's
 * `packed`, which the context does not own: read it only while the caller keeps that buffer alive. */
int pf_debug_read_words(pf_ctx* ctx, int which, uint64_t first, uint64_t n, uint64_t* out);
/* Test hook, read-only: how the host (or, under PF_FLAG_DEVICE_PLAN, cluster_ninst_kernel) routed every cluster of the
 * last pf_submit after the dedup pass.  n_clusters must be that batch's.  Each array may be NULL; each has n_clusters
 * elements.  route[c] = class | mode << 3 | first << 5: `class` is the finish class of the cluster's last, successful
 * attempt (1: fused small, 2: fused large, 3: fused large over several key partitions, 5: fused huge, 0: the general path
 * of rows_kernel and emit_kernel), `mode` its view (0: every copy, 1: distinct sequences, 2: the wide class) and `first`
 * the class of its first attempt (equal to `class` unless a scan overflowed its table).  nparts[c] and nslots[c] are the
 * key partitions and the table slots per partition of the last attempt, attempts[c] how many attempts the cluster took.
 * For a host-planned cluster these are what the item builder computed; for a device-planned one the class and table bits
 * the kernel left in its record, read back with the records the host fetches anyway.  Nothing is recorded on the device
 * for this hook and the package never calls it. */
int pf_debug_cluster_routes(pf_ctx* ctx, uint32_t n_clusters, uint8_t* route, uint32_t* nparts, uint32_t* nslots,
                            uint32_t* attempts);

/* Device buffers for callers that keep batches resident (bench.py, tests): plain hipMalloc /
 * hipMemcpy / hipFree on the context's device. */
int pf_dev_alloc(pf_ctx* ctx, uint64_t bytes, void** dptr);
int pf_dev_free(pf_ctx* ctx, void* dptr);
int pf_dev_upload(pf_ctx* ctx, void* dptr, const void* src, uint64_t bytes);
int pf_dev_download(pf_ctx* ctx, void* dst, const void* dptr, uint64_t bytes);

/* Synthetic-input helper (bench.py): expand allele pools into per-sample packed segments on the
 * device.  seg i becomes a copy of allele seg_allele[i]: words
 * [allele_word_off[a], allele_word_off[a] + ceil16(len)) -> packed[seg_word_off[i] ...].
 * All pointers are device pointers. */
int pf_synth_expand(pf_ctx* ctx, const uint64_t* allele_words, const uint64_t* allele_word_off,
                    const uint32_t* seg_allele, const uint64_t* seg_word_off, const uint32_t* seg_len,
                    uint32_t n_segs, uint64_t* packed);

/* Host helper: pack ASCII A/C/G/T (upper case) to the layout above.  dst must hold
 * 2*ceil(len/64) words; returns the number of words written. */
uint64_t pf_pack_acgt(const char* seq, uint32_t len, uint64_t* dst);

/*
 * Host-side batch packer (no GPU involved): the Seqinfo records of a batch of clusters
 * (/root/reference/panfeed/classes.py:11-18, iteration order of panfeed.py:54-55, cluster-major) -> the segment
 * arrays of pf_batch, the slow-path rows for windows with a non-ACGT base (grouped as panfeed.py:64-88 does),
 * strand-bit offsets for target strains, and what the kmers.tsv writer needs per target sequence.
 */
typedef struct {
    uint32_t n_clusters, n_seqs;
    const char* const* seq;           /* [n_seqs] Seqinfo.sequence (upper case), seq_len bytes */
    const char* const* comp;          /* [n_seqs] Seqinfo.compsequence; checked to be the complement on A/C/G/T */
    const uint32_t* seq_len;          /* [n_seqs] */
    const uint32_t* seq_col;          /* [n_seqs] column of the strain in sorted(cluster.keys()) (panfeed.py:47-49) */
    const uint8_t* seq_target;        /* [n_seqs] `strain in stroi` (panfeed.py:90), may be NULL */
    const uint32_t* cluster_seq_off;  /* [n_clusters+1] */
    uint32_t klength, canon, W, want_strand;
    /* optional (NULL = every sequence is given as text): sequences that are ranges of the genomes resident in HBM
     * (pf_genomes_upload).  seq_flags bit 0: by reference -- seq/comp of that sequence are not read, the range is
     * pure A/C/G/T and not a target strain's; bit 1: the sequence is the reverse complement of the range. */
    const uint64_t* seq_src_off;      /* [n_seqs] word offset of the contig in the genome store */
    const uint32_t* seq_src_start;    /* [n_seqs] lowest base coordinate of the range in the contig */
    const uint32_t* seq_flags;        /* [n_seqs] */
} pf_pack_in;

typedef struct pf_packed pf_packed;

typedef struct {
    uint32_t n_segs, n_extra, n_targets, reserved;
    uint64_t n_words, n_strand_words, n_instances;
    const uint64_t* packed; const uint64_t* seg_word_off;
    const uint32_t* seg_len; const uint32_t* seg_sample; const uint32_t* seg_ord_base; const uint32_t* seg_strand_off;
    const uint32_t* cluster_seg_off;  /* [n_clusters+1] */
    const uint64_t* cluster_ninst;    /* [n_clusters] trip count of panfeed.py:64 (x2 non-canonical) */
    const uint32_t* extra_cluster; const uint32_t* extra_ord; const uint32_t* extra_bits;
    const char* extra_keys;           /* n_extra * klength bytes */
    /* target sequences (input index), their pure segments and slow-path windows (CSR) */
    const uint32_t* target_seq; const uint32_t* target_seg_off; const uint32_t* target_seg_index;
    const uint32_t* target_seg_start; const uint32_t* target_seg_nwin;
    const uint32_t* target_ambig_off; const uint32_t* target_ambig_pos; const int8_t* target_ambig_used;
    const char* target_ambig_keys;    /* klength bytes per slow-path window */
    /* with by-reference sequences: `packed` / n_words hold only the segments packed on the host ("literal"),
     * seg_word_off are offsets in the DEVICE buffer of n_words_dev words that pf_submit_gather fills; NULL / 0
     * when every sequence was given as text */
    uint64_t n_words_dev;
    const uint64_t* gather_src_off; const uint32_t* gather_src_start; const uint32_t* gather_src_flags;
} pf_packed_view_t;

int pf_pack_records(const pf_pack_in* in, pf_packed** out);
/* Binding helper for a CPython host side (panfeed_amd/packing.py hands Seqinfo.sequence / .compsequence,
 * classes.py:11-18, to pf_pack_records by address): out[i] = as_utf8(objs[i]) for an array of n object pointers, where
 * as_utf8 is the interpreter's PyUnicode_AsUTF8 -- one C loop instead of one FFI call per string, no assumption about the
 * object layout.  Call it with the GIL held (ctypes.PyDLL).  out[i] == 0: the API refused that object. */
int pf_py_str_addresses(void* const* objs, uint64_t n, const char* (*as_utf8)(void*), uint64_t* out);
/* The same for the two str attributes of every object of a Python list in one pass (Seqinfo.sequence / .compsequence,
 * classes.py:11-18; what pattern_hasher's records carry, panfeed.py:54-67): addresses of their UTF-8 bytes, their length,
 * flags[i] bit 0 = both str, equal length, all ASCII.  The interpreter's API comes as function pointers (PyList_GetItem,
 * PyObject_GetAttr, PyUnicode_AsUTF8AndSize, PyUnicode_GetLength, Py_DecRef, PyErr_Clear); the attribute objects stay
 * referenced in held[2 n] until pf_py_release.  Call both with the GIL held. */
typedef struct pf_py_api {
    void* (*list_get_item)(void*, long long);                 /* PyList_GetItem (borrowed reference) */
    void* (*get_attr)(void*, void*);                          /* PyObject_GetAttr (new reference) */
    const char* (*as_utf8_and_size)(void*, long long*);       /* PyUnicode_AsUTF8AndSize */
    long long (*get_length)(void*);                           /* PyUnicode_GetLength */
    void (*dec_ref)(void*);                                   /* Py_DecRef */
    void (*err_clear)(void);                                  /* PyErr_Clear */
} pf_py_api;
int pf_py_seqinfo_columns(void* list, uint64_t n, void* attr_seq, void* attr_comp, const pf_py_api* api,
                          uint64_t* a_seq, uint64_t* a_comp, uint32_t* len, uint8_t* flags, void** held);
int pf_py_release(void** held, uint64_t n, const pf_py_api* api);
int pf_packed_view(const pf_packed* p, pf_packed_view_t* view);
void pf_packed_free(pf_packed* p);

/*
 * Native reader in front of the path: the panaroo presence/absence table, GFF3 features and
 * FASTA sequences -> the Seqinfo records iter_gene_clusters yields
 * (/root/reference/panfeed/input.py:274-332 parse_gff, :335-468 iter_gene_clusters), as flat arrays whose
 * sequence pointers feed pf_pack_records directly.  PARITY UNPINNED at the pyfaidx boundary.
 */
typedef struct {
    const char* presence_absence_csv;       /* -p */
    uint32_t n_genomes, reserved;
    const char* const* genome_names;        /* file name minus ".gff" (input.py:31) */
    const char* const* gff_paths;
    const char* const* fasta_paths;         /* NULL, or per genome NULL = sequences embedded after ##FASTA */
    uint32_t upstream, downstream, downstream_start_codon, raise_missing;
    const char* const* target_strains; uint32_t n_targets, n_genes;
    const char* const* gene_list;           /* --genes; NULL = every cluster */
} pf_pangenome_opts;

typedef struct pf_pangenome pf_pangenome;
typedef struct pf_records pf_records;

typedef struct { uint32_t n_clusters, n_strains, next_cluster, reserved; } pf_pangenome_info_t;

typedef struct {
    uint32_t n_clusters, n_seqs, W, reserved;
    /* per Seqinfo, in the iteration order of panfeed.py:54-55, cluster-major */
    const char* const* seq; const char* const* comp; const char* const* id; const char* const* chromosome;
    const uint32_t* seq_len; const uint32_t* seq_col; const uint32_t* seq_strain;   /* strain: index in the cluster's dict */
    const uint8_t* seq_target; const int32_t* seq_strand;
    const int64_t* seq_start; const int64_t* seq_end; const int64_t* seq_offset;
    /* per cluster */
    const uint32_t* cluster_seq_off;        /* [n_clusters+1] */
    const char* const* cluster_name;
    const uint32_t* cluster_nstrains;       /* len(cluster.keys()) */
    const uint32_t* cluster_npresab;        /* len(clusterpresab) = strains of the table */
    const uint32_t* cluster_presab;         /* [n_clusters * W] bits over sorted(strains) */
    const uint32_t* cluster_strain_off;     /* [n_clusters+1] into cluster_strain: the dict keys in insertion order */
    const char* const* cluster_strain;
    /* after pf_pangenome_set_store: sequences given as ranges of the resident genomes (seq/comp NULL for those);
     * same meaning as the fields of pf_pack_in; NULL before */
    const uint64_t* seq_src_off; const uint32_t* seq_src_start; const uint32_t* seq_flags;
} pf_records_view_t;

int pf_pangenome_open(const pf_pangenome_opts* opts, pf_pangenome** out);
/* The same reader with the genomes going to the device AS THE FILES ARE READ (one pass over the input instead of
 * pf_pangenome_open's read + upper-casing copy and pf_genomes_upload's second copy): every file is read straight into
 * pinned memory, its GFF lines parsed there (input.py:274-332), its contigs measured without copying a base, and a kernel
 * de-wraps, upper-cases and packs the letters to 2 bits per base in the context's genome store while other files are
 * still being read.  Contig text stays on the host only for contigs with a letter other than A/C/G/T and for target
 * strains (what iter_gene_clusters cuts out of text, input.py:427-452).  The reader comes back in by-reference mode
 * (as after pf_pangenome_contigs / pf_genomes_upload / pf_pangenome_set_store); pf_pangenome_contigs is refused on it.
 * PF_ERR_CAPACITY: the store's estimate (half a byte per byte of input) did not hold -- contigs of a few letters each;
 * use pf_pangenome_open + pf_genomes_upload. */
int pf_pangenome_open_device(const pf_pangenome_opts* opts, pf_ctx* ctx, pf_pangenome** out);
/* The same with the context asked for when the first genome needs it (get_ctx(user), called once, from one of the reader's
 * threads): the caller may still be creating it while the reader parses the presence/absence table. */
int pf_pangenome_open_device_cb(const pf_pangenome_opts* opts, pf_ctx* (*get_ctx)(void*), void* user, pf_pangenome** out);
/* Test hook: the reader side of pf_pangenome_open_device without a device -- blocks of ordinary memory, the store filled
 * on the host by the kernel's addressing (letter j of a contig = byte text_off + j + (j / width) * eol of its block).
 * *store (pf_free_text) holds *nwords words; the reader is in by-reference mode. */
int pf_debug_open_hostsink(const pf_pangenome_opts* opts, pf_pangenome** out, uint64_t** store, uint64_t* nwords);
void pf_pangenome_close(pf_pangenome* p);
/* The same on a thread of its own: returns at once, the reader's memory (tables, features, gigabytes of contigs) is
 * given back in the background.  For a caller that has finished its run. */
void pf_pangenome_close_async(pf_pangenome* p);
int pf_pangenome_info(pf_pangenome* p, pf_pangenome_info_t* info);
const char* pf_pangenome_strain(pf_pangenome* p, uint32_t i, int sorted);
const char* pf_pangenome_take_log(pf_pangenome* p);   /* warnings the reference sends to logger.warning */
/* Records of the next (at most) max_clusters rows of the table; n_clusters == 0 at the end. */
int pf_pangenome_next(pf_pangenome* p, uint32_t max_clusters, pf_records** out, pf_records_view_t* view);
/* Multi-GPU sharding of the processing order (contiguous ranges of table rows per rank).  The clusters a
 * run processes are the table rows that pass --genes, in table order (input.py:352-355); pf_pangenome_weights gives
 * each one's number of gene entries (paralogs counted: the sequences iter_gene_clusters will cut, a proxy for its
 * k-mer instances) so that ranks can balance their ranges; pf_pangenome_set_range restricts pf_pangenome_next to
 * processed clusters [first, first + count) and rewinds the reader to `first`. */
int pf_pangenome_weights(pf_pangenome* p, uint32_t cap, uint32_t* weights, uint32_t* n_processed);
int pf_pangenome_set_range(pf_pangenome* p, uint32_t first, uint32_t count);
/* Contigs of all genomes in one flat order (upper-cased text), for pf_genomes_upload; then the word offsets it
 * returned: from here on pf_pangenome_next hands out non-target, pure-ACGT sequences by reference. */
int pf_pangenome_contigs(pf_pangenome* p, uint32_t* n, const char* const** ascii, const uint64_t** len);
int pf_pangenome_set_store(pf_pangenome* p, const uint64_t* contig_word_off, uint32_t n);
void pf_records_free(pf_records* r);

/* Host helper: md5 + base64 of a digest -- panfeed.py:175-176 -- for writers. */
void pf_b64_digest(const uint8_t md5[16], char out[24]);

/* Writers (host threads, after pf_fetch): the bytes pattern_hasher appends to kmers_to_hashes.tsv for the last
 * batch -- "idx\t\thash\n" per cluster then "idx\tkmer\thash\n" per kept k-mer (panfeed.py:177, 208) -- and to
 * hashes_to_patterns.tsv -- "hash\tv0\tv1...\n" per pattern first seen in this batch, in first-seen order
 * (panfeed.py:181-187, 217-223).  cluster_names: n_clusters NUL-terminated names (batch order); extra_keys: the
 * k-mer strings of the batch's slow-path rows (klength bytes each), may be NULL without such rows.
 * cluster_end (may be NULL): [n_clusters] byte offset where each cluster's rows end.
 * The buffers are malloc'ed; release them with pf_free_text. */
int pf_render_kmers_to_hashes(pf_ctx* ctx, const char* const* cluster_names, const char* const* extra_keys,
                              char** out, uint64_t* nbytes, uint64_t* cluster_end);
int pf_render_hashes_to_patterns(pf_ctx* ctx, char** out, uint64_t* nbytes);

/* One Seqinfo of a target strain (panfeed/classes.py:11-18) for the positional rows of kmers.tsv
 * (panfeed.py:90-107).  Its pure-ACGT windows take used_strand from the strand bits of the last fetched batch
 * (segment `seg_index[j]` covers windows seg_start[j] .. seg_start[j]+seg_nwin[j]-1 of the sequence); windows
 * that contain another base come with their canonical k-mer and used_strand from the caller's slow path. */
typedef struct {
    const char* cluster; const char* strain; const char* id; const char* chromosome;   /* NUL-terminated */
    const char* sequence; const char* compsequence;                                    /* `len` bytes each */
    uint32_t len;
    int32_t strand;
    int64_t start, end, offset;
    uint32_t n_segs; uint32_t n_ambig;
    const uint32_t* seg_index; const uint32_t* seg_start; const uint32_t* seg_nwin;
    const uint32_t* ambig_pos; const int8_t* ambig_used; const char* const* ambig_key;   /* sorted by ambig_pos */
} pf_target_seq;

/* Rows of kmers.tsv for `n` target sequences, in the given order: one row per window ("cluster, strain,
 * feature_id, contig, feature_strand, contig_start, contig_end, gene_start, gene_end, strand, k-mer"), two per
 * window in non-canonical mode (panfeed.py:104-107).  seg_strand_off: the batch's array.  Needs the last pf_submit
 * only (the windows' used_strand bits are copied from the device by the call itself; no pf_fetch).  Sizes and rows are
 * both produced by all host threads; *out is malloc'd (pf_free_text). */
int pf_render_kmers_tsv(pf_ctx* ctx, const pf_target_seq* seqs, uint32_t n, const uint32_t* seg_strand_off,
                        char** out, uint64_t* nbytes);
void pf_free_text(char* p);
/* The same rows (panfeed.py:90-107) written ON THE DEVICE: the used_strand bits and the packed bases of the last
 * pf_submit are there already, so neither they nor the sequences' letters cross PCIe -- per sequence only its five
 * constant fields, as text, and four numbers go up.  Sequences that are pure A/C/G/T (one segment covering every
 * window) are written by the GPU; the others (an 'N' inside, an over-long name) by the host renderer above and copied
 * to their places, so that the text is that of pf_render_kmers_tsv byte for byte, in the order of `seqs`.  The text
 * stays in device memory; *nbytes is its size.  With every sample a target (BASELINE configs[4]'s second pass) it is
 * the largest output of a run. */
int pf_render_kmers_tsv_device(pf_ctx* ctx, const pf_target_seq* seqs, uint32_t n, uint64_t* nbytes);
/* Bytes [offset, offset + *nbytes) of that text, *nbytes = min(max_bytes, what is left), in pinned host memory owned by
 * the context: valid until the next call of this function (the block after it is already being copied when the call
 * returns, so that the caller's write of one block overlaps the copy of the next). */
int pf_device_text_chunk(pf_ctx* ctx, uint64_t offset, uint64_t max_bytes, const char** ptr, uint64_t* nbytes);
/* The same text (same bytes, same order as pf_render_kmers_tsv_device) in device memory of at most budget_bytes: cut
 * into ranges at tile boundaries and at boundaries of host-rendered sequences, each range at most budget_bytes / 2, written
 * by the GPU into two buffers used alternately (range r + 1 is written while range r is copied out).  A text that fits
 * the budget is one range.  *total_bytes: the text's size; *n_ranges: the ranges; *peak_text_bytes (may be NULL): the
 * most text the device holds at one time.  A tile or host-rendered sequence larger than budget_bytes / 2 (less 64 bytes)
 * is PF_ERR_ARG; the message names the smallest budget that works.  `seqs` must stay valid until the stream ends (its
 * last block handed out, the next pf_submit or stream begin).  Ends the text of pf_render_kmers_tsv_device. */
int pf_kmers_tsv_stream_begin(pf_ctx* ctx, const pf_target_seq* seqs, uint32_t n, uint64_t budget_bytes,
                              uint64_t* total_bytes, uint32_t* n_ranges, uint64_t* peak_text_bytes);
/* The next block of that text (at most 64 MiB) in pinned host memory owned by the context, valid until the next call;
 * the block after it is already being copied.  *nbytes == 0 at the end (the stream is then over). */
int pf_kmers_tsv_stream_next(pf_ctx* ctx, const char** ptr, uint64_t* nbytes);
/* Under pf_set_device_gzip, between pf_kmers_tsv_stream_begin and the first pf_kmers_tsv_stream_next: text offsets behind
 * which a gzip member must end (non-decreasing, none past the text's size, else PF_ERR_ARG; repeats, 0 and the text's
 * size say nothing new and are dropped) -- the ends of the clusters' rows under multiple_files, so that each cluster's
 * file is made of whole members.  Every block ends on a member boundary anyway; the cuts add boundaries inside blocks.
 * Without this call the stream is as before.  PF_ERR_STATE: no open stream, no device gzip, or a block already queued. */
int pf_kmers_tsv_stream_cuts(pf_ctx* ctx, const uint64_t* cuts, uint64_t n);
/* The block pf_kmers_tsv_stream_next handed out last, under device gzip: *text_off, *text_bytes -- the text behind its
 * members; *n_cuts -- the cuts that lie strictly inside that text; cut_text[i] / cut_member[i] (caller arrays of `cap`
 * entries; PF_ERR_ARG if there are more cuts) -- their text offsets, ascending, and the offset in the block's members
 * behind which the members of the text before the cut end.  PF_ERR_STATE without such a block. */
int pf_kmers_tsv_stream_block_cuts(pf_ctx* ctx, uint64_t* text_off, uint64_t* text_bytes, uint64_t* cut_text, uint64_t* cut_member,
                                   uint64_t cap, uint64_t* n_cuts);
/* Where the rows of each of the n target sequences given to the last pf_render_kmers_tsv_device or
 * pf_kmers_tsv_stream_begin end in the whole text: ends[i] is the offset just behind sequence i's rows (a sequence with
 * no window repeats the end before it; ends[n - 1] is the text's size).  The caller cuts the text where its sequences
 * change cluster (panfeed.py:104-110, 225-226 under multiple_files).  Valid until the next pf_submit or the next of
 * those two calls, also after the stream has ended.  n must be that call's n (else PF_ERR_ARG); PF_ERR_STATE when
 * there is no such text. */
int pf_kmers_tsv_seq_ends(pf_ctx* ctx, uint64_t* ends, uint32_t n);

/* Rows of passing patterns only.  pf_set_passing_hashes turns the filter on with the n digests at md5 (16 bytes each, the
 * bytes whose base64 the files print; repeats count once; n = 0 is allowed: no row passes).  While it is on, the text of
 * pf_render_kmers_tsv_device and of pf_kmers_tsv_stream_begin / _next -- its size, ranges, budget check, peak, the
 * offsets of pf_kmers_tsv_seq_ends (a sequence none of whose rows are kept repeats the end before it) and of
 * pf_kmers_tsv_stream_cuts / _block_cuts -- is the unfiltered text with exactly those rows kept, in their order, whose
 * (cluster, k-mer) pair is a kept k-mer of the last pf_submit with a pattern digest in the set: the pairs
 * kmers_to_hashes.tsv lists with such a hash.  The GPU decides before a byte of a dropped row is written.
 * pf_render_kmers_tsv (the host renderer), kmers_to_hashes and hashes_to_patterns are not affected.
 * pf_clear_passing_hashes turns the filter off and frees what it held.  Both are PF_ERR_STATE while a kmers.tsv
 * stream is open. */
int pf_set_passing_hashes(pf_ctx* ctx, const uint8_t* md5, uint64_t n);
int pf_clear_passing_hashes(pf_ctx* ctx);
/* While the filter is on, after every pf_submit and before the batch's first kmers.tsv text (else that text's call is
 * PF_ERR_STATE): the batch's cluster names (n_clusters NUL-terminated strings, batch order; a pf_target_seq's `cluster`
 * is looked up among them, an unknown one is PF_ERR_ARG) and the text of its slow-path rows, as pf_render_device takes
 * them (klength bytes each, back to back; NULL without such rows).  Both are copied.  PF_ERR_STATE without a
 * successful pf_submit or while a kmers.tsv stream is open. */
int pf_passing_batch_names(pf_ctx* ctx, const char* const* cluster_names, const char* extra_keys, uint64_t n_extra);
/* out[0] digests in the set, [1] kept k-mers marked as passing for the last filtered text, [2] rows that text
 * considered, [3] rows it kept, [4] lookups since that text's marking whose slot hash matched and whose bytes did not,
 * [5] device bytes the filter holds (its tables are not part of a stream's text budget). */
int pf_passing_stats(pf_ctx* ctx, uint64_t out[6]);
/* Milliseconds (hipEvent) of the last filtered text's mark and index kernel. */
int pf_passing_mark_ms(pf_ctx* ctx, float* ms);
/* Test hook: the passing set's and the batch index's lookups keep only the low `bits` bits of their slot hash (64: all
 * of it, the product; 0: one chain), so that the compare-and-reject branch runs in the shipped library.  The value is a
 * kernel argument.  PF_ERR_ARG above 64, PF_ERR_STATE while a kmers.tsv stream is open. */
int pf_debug_passing_hash_bits(pf_ctx* ctx, uint32_t bits);
/* Test hook, read-only: slots [first, first + n) of the filter's device tables as they stand, after the stream's work
 * (hipMemcpy).  which = 0: the passing set, four words a slot (d0, d1, h, used); 1: the batch index's ref (cluster << 32 |
 * place, ~0 = free) and 2: its hsh, one word a slot, as the last filtered kmers.tsv text of the last pf_submit left
 * them.  *slots (may be NULL): the table's size.  May be called after that text has been opened, a stream open or not.
 * PF_ERR_ARG outside the table; PF_ERR_STATE with the filter off, or for 1 and 2 with no such text since the last
 * pf_submit, pf_set_passing_hashes or pf_debug_passing_hash_bits.  The package never calls it. */
int pf_debug_passing_tables(pf_ctx* ctx, int which, uint64_t first, uint64_t n, uint64_t* out, uint64_t* slots);

/* The bodies of kmers_to_hashes.tsv and hashes_to_patterns.tsv of the last pf_submit written ON THE DEVICE
 * (panfeed.py:177,208 and :181-187,217-223): rows assembled in LDS, coalesced stores, one copy to pinned host memory.
 * No pf_fetch needed; the k-mer keys and pattern rows never cross PCIe, only the text does.  names: cluster names in
 * batch order; extra_keys: n_extra * klength bytes, the k-mer text of the batch's slow-path rows (NULL if none).
 * *kh / *hp point into pinned memory owned by the context (two blocks used alternately): valid until the call after
 * the next one, so that a writer thread can still be on the previous batch.  Not under multiple_files
 * (PF_ERR_ARG): pf_render_device_clusters is the call for that. */
int pf_render_device(pf_ctx* ctx, const char* const* names, const char* extra_keys, uint64_t n_extra,
                     const char** kh, uint64_t* kh_bytes, const char** hp, uint64_t* hp_bytes);
/* Same with flags: PF_RENDER_NO_PATTERN_ROWS leaves hashes_to_patterns.tsv out (*hp_bytes = 0) -- a rank of a
 * multi-GPU run writes its pattern rows only after the run-global merge has said which ones are its own. */
#define PF_RENDER_NO_PATTERN_ROWS 1u
int pf_render_device_ex(pf_ctx* ctx, const char* const* names, const char* extra_keys, uint64_t n_extra, uint32_t flags,
                        const char** kh, uint64_t* kh_bytes, const char** hp, uint64_t* hp_bytes);
/* pf_render_device for a context made with multiple_files (panfeed.py:35-43, 159-167: one directory per gene cluster):
 * the same two bodies, written by the same kernels in one pair of launches, plus where to cut them into the clusters'
 * files.  kh_end / hp_end: caller arrays of n_clusters entries.  kh_end[i] is the offset just behind cluster i's rows in
 * *kh; hp_end[i] the offset just behind the rows of the patterns first seen in cluster i in *hp (the pattern set
 * starts empty in every cluster, and a batch's new patterns in first-seen order stand cluster by cluster).  A cluster
 * without rows repeats the end before it; the last ends are *kh_bytes and *hp_bytes.  Bodies only: the files' header
 * lines are the caller's.  Pinned-block lifetime and errors as pf_render_device (PF_ERR_CAPACITY: too many passes,
 * PF_ERR_ARG: an over-long cluster name -- the host renderers take such a batch); PF_ERR_ARG without multiple_files. */
int pf_render_device_clusters(pf_ctx* ctx, const char* const* names, const char* extra_keys, uint64_t n_extra,
                              const char** kh, uint64_t* kh_bytes, const char** hp, uint64_t* hp_bytes,
                              uint64_t* kh_end, uint64_t* hp_end);
/* pf_render_device_clusters under pf_set_device_gzip (PF_ERR_STATE without it, PF_ERR_ARG without multiple_files): the
 * same two bodies from the same pair of launches, encoded so that no gzip member holds rows of two clusters, and handed
 * out as members.  kh_end[i] / hp_end[i]: the offset just behind cluster i's members in *kh / *hp -- a cluster's piece
 * is a complete gzip file's body, appended behind the header line's member as it is; a cluster without rows repeats the
 * end before it.  kh_text_end / hp_text_end: the text offsets pf_render_device_clusters gives (the text sizes behind
 * the pieces).  All four: caller arrays of n_clusters entries. */
int pf_render_device_cluster_members(pf_ctx* ctx, const char* const* names, const char* extra_keys, uint64_t n_extra,
                                     const char** kh, uint64_t* kh_bytes, const char** hp, uint64_t* hp_bytes,
                                     uint64_t* kh_end, uint64_t* hp_end, uint64_t* kh_text_end, uint64_t* hp_text_end);
/* Rows of hashes_to_patterns.tsv ("hash\tv0\tv1...\n", panfeed.py:181-187, 217-223) for ANY patterns of the
 * run-global pool, in the order given, written on the device: pids[n] are pattern ids (< pf_pattern_count).  The
 * multi-GPU driver calls it after pf_merge_patterns with the ids whose first_seen is the global minimum of their
 * digest, sorted by first_seen (rank-ordered concatenation then equals the --cores 1 file; reference writer:
 * __main__.py:67-81).  *text points into the context's pinned memory, valid until the call after the next one of
 * this function / pf_render_device. */
int pf_render_pattern_rows(pf_ctx* ctx, const uint32_t* pids, uint64_t n, const char** text, uint64_t* nbytes);
/* The same rows (the bytes pf_render_pattern_rows gives for the same ids: any ids of the pool, in this order, repeats
 * allowed) as a stream, in device memory of two slices of text plus 8 bytes per row (the ids and the row lengths; the
 * host keeps 12 bytes per row), whatever the size of the text: the text is cut at row boundaries into slices
 * of at most slice_bytes (0, or more than 64 MiB: 64 MiB; a row longer than slice_bytes is a slice of its own), written
 * into two device buffers used alternately.  begin checks the ids (one at or beyond pf_pattern_count is PF_ERR_ARG),
 * copies them (pids need not outlive the call) and measures every row; *total_text_bytes: the text's size, *n_slices:
 * the slices.  PF_ERR_STATE while a kmers.tsv stream or another stream of pattern rows of the context has not reached
 * its end: the streams share their buffers.  Ends the text of pf_render_kmers_tsv_device. */
int pf_pattern_rows_stream_begin(pf_ctx* ctx, const uint32_t* pids, uint64_t n, uint64_t slice_bytes,
                                 uint64_t* total_text_bytes, uint32_t* n_slices);
/* The next slice in pinned host memory owned by the context, valid until the next call; the slice after it has been
 * queued on the context's stream already (rows, encode, copy).  Under pf_set_device_gzip the slice's gzip members are
 * handed out in its place, and out[2] of pf_device_gzip_text_bytes counts the text behind them.  *nbytes == 0 at the end
 * (the stream is then over).  A pf_submit, pf_reset_patterns, a kmers.tsv text begun or pf_set_device_gzip ends the
 * stream: the next call is PF_ERR_STATE.  (pf_merge_patterns only reads the pool and leaves the stream alone.) */
int pf_pattern_rows_stream_next(pf_ctx* ctx, const char** ptr, uint64_t* nbytes);

/* Parallel gzip of a block of output text (the reference: gzip.open(..., "wt", compresslevel=9),
 * /root/reference/panfeed/input.py:239-241,255-258 -- one core).  `data` is cut at line ends into chunks of about
 * chunk_bytes, each deflated as its own gzip member on its own host thread; *out (pf_free_text) is the members
 * concatenated, to be appended to the .gz file.  Decompresses to exactly `data`. */
int pf_gzip_members(const char* data, uint64_t n, int level, uint64_t chunk_bytes, char** out, uint64_t* out_n);

/*
 * gzip ON THE DEVICE (opt-in: larger files than pf_gzip_members' level 9 in less time; measured: profiles/gzip_device/).  The text is cut
 * into independent chunks of pf_gzip_device_chunk_bytes() bytes; each becomes one complete gzip member (RFC 1952) of one
 * deflate block -- stored, fixed or dynamic Huffman, the smallest by exact bit count -- with matches found through a
 * hash table in LDS (one candidate per position, greedy parse, no match reaching before its chunk), its CRC32 computed on
 * the device.  Any gzip reader gets back exactly the text; the same text gives the same bytes on every run.
 * flags: 0 is the product setting and PF_GZ_DEEP the product's second effort level; FIXED_ONLY, DYNAMIC_ONLY and
 * LITERALS_ONLY are test hooks.
 */
#define PF_GZ_FIXED_ONLY 1u     /* every block with the fixed codes */
#define PF_GZ_DYNAMIC_ONLY 2u   /* every block with dynamic codes */
#define PF_GZ_LITERALS_ONLY 4u  /* no match is accepted */
/* Not a test hook: every member leaves as a BGZF member (SAM specification 4.1: the 18-byte head with FLG = 4 and the BC
 * subfield, BSIZE = the member's size - 1) -- the same member, 8 bytes longer.  Offsets, member_end[] and sizes count the
 * framed members.  The 28-byte end-of-file member is the file writer's to append.  Taken by pf_gzip_device[_segments],
 * pf_gzip_host_model[_segments] and pf_set_device_gzip; pf_kmerjoin_set_gzip refuses it. */
#define PF_GZ_BGZF 8u
/* Not a test hook: the second effort level (`--gpu-compress-level 2`).  Same container, same cuts, same decoders; the
 * match search looks further.  Beside the hash table's candidate every position tries the same column of the row before
 * it -- the position as far behind the previous line's start as it is behind its own line's, if that lies before the
 * previous line's end; only the chunk's own bytes are looked at -- and takes the longer of the two matches (on a tie the
 * nearer), a 3-byte one only within 4 096 bytes, so length symbol 257 may appear.  The parse is lazy by one step: a match
 * is put off for one literal when the next position's match is longer.  The rule depends on the chunk's text alone: the
 * same text gives the same bytes.  PF_GZ_LITERALS_ONLY wins over it; it combines with the other flags.  Smaller files
 * for more encoder time: measured in profiles/gzip_deep/.  Taken by pf_gzip_device[_segments],
 * pf_gzip_host_model[_segments], pf_set_device_gzip and pf_kmerjoin_set_gzip. */
#define PF_GZ_DEEP 16u
uint32_t pf_gzip_device_chunk_bytes(void);
/* Host text in, members out (malloc'd: pf_free_text): uploaded, encoded on the GPU, copied back.  n == 0 gives
 * *out_n == 0.  For tests, tools and text rendered on the host. */
int pf_gzip_device(pf_ctx* ctx, const char* data, uint64_t n, uint32_t flags, char** out, uint64_t* out_n);
/* The same for a text made of segments, one behind the other: seg_end[0 .. n_seg) are the offsets behind them
 * (non-decreasing, the last one n; n_seg == 0 needs n == 0; else PF_ERR_ARG).  No member holds bytes of two segments:
 * every segment is cut into chunks from its own start, an empty one has no member, and the bytes of a segment's members
 * are those pf_gzip_device gives for the segment's text alone.  member_end[i] (caller array of n_seg entries): the
 * offset in *out behind segment i's members. */
int pf_gzip_device_segments(pf_ctx* ctx, const char* data, uint64_t n, const uint64_t* seg_end, uint64_t n_seg, uint32_t flags,
                            char** out, uint64_t* out_n, uint64_t* member_end);
/* Device time of the last pf_gzip_device's kernels (encode, size scan, gather; hipEvent on the context's stream), ms. */
int pf_gzip_device_last_ms(pf_ctx* ctx, float* ms);
/* The same container and coder run serially on the host, with a plain one-candidate greedy matcher: no context, no GPU.
 * Its bytes need not equal the device's; both decode to `data`. */
int pf_gzip_host_model(const char* data, uint64_t n, uint32_t flags, char** out, uint64_t* out_n);
/* and over segments, as pf_gzip_device_segments cuts them: the same chunk plan, the same refusals */
int pf_gzip_host_model_segments(const char* data, uint64_t n, const uint64_t* seg_end, uint64_t n_seg, uint32_t flags, char** out,
                                uint64_t* out_n, uint64_t* member_end);
/*
 * gunzip ON THE DEVICE, for files made of small members such as pf_gzip_device writes: every member at most
 * pf_gzip_device_chunk_bytes() of text (its ISIZE) and at most a ninth more than that compressed, with the plain 10-byte
 * header (CM = 8, FLG = 0).  Inside such a member all of RFC 1951 is taken: stored, fixed and dynamic blocks, several
 * blocks, the run codes 16 / 17 / 18.  Where members start is found without decoding: the first member's first eight
 * header bytes (up to MTIME) are the signature, every place they stand at is a candidate, a member's tail is the 8 bytes before the next one.  One wave
 * inflates one member; every member is verified on the device (it ends exactly at its tail, gives exactly ISIZE bytes,
 * its CRC32 matches).  *taken = 0 with PF_OK: not a run of such members, or a member failed a check -- pf_last_error()
 * names the first such member and why; nothing is repaired, the caller reads the file another way.
 * Host bytes in, text out (malloc'd: pf_free_text).  n == 0 gives *out_n == 0, *taken = 1.  Device memory: the members
 * and the text of at most 256 MiB of text at a time.
 */
int pf_gunzip_device(pf_ctx* ctx, const char* members, uint64_t n, char** out, uint64_t* out_n, int* taken);
/* Device time of the last pf_gunzip_device's inflate kernels (hipEvent on the context's stream), ms. */
int pf_gunzip_device_last_ms(pf_ctx* ctx, float* ms);
/* The same format functions run serially on the host: no context, no GPU. */
int pf_gunzip_host_model(const char* members, uint64_t n, char** out, uint64_t* out_n, int* taken);
/*
 * The same for BGZF, what bgzip and htslib write: a chain of members of at most 65 536 bytes, of at most 65 536 bytes of
 * text each, every one with the 18-byte head FLG = 4, XLEN = 6, 'B' 'C' 02 00 BSIZE.  Only that head is taken: any other
 * extra field (XLEN != 6, another or a second subfield) is "not taken".  The members are found by their BSIZE chain;
 * a head in the chain that is not such a head (a plain gzip member among them: mixed files are not supported), a BSIZE
 * smaller than a frame or past the end, an ISIZE over 65 536 are "not taken" before anything is decoded.  The end marker
 * is a member of no text; a file without it is taken, as gzip reads it.  Members of more than
 * pf_gzip_device_chunk_bytes() of text are inflated by a kernel with a 64 KiB window in LDS (two workgroups per CU), the
 * others by pf_gunzip_device's (four).  Large gzip members, such as the 4 MiB ones of pf_gzip_members, are not taken by
 * either call: one wave inflates one member, and a member of megabytes would take it most of a second.
 * Results, refusals, memory and pf_gunzip_device_last_ms as for pf_gunzip_device.
 */
int pf_gunzip_device_bgzf(pf_ctx* ctx, const char* members, uint64_t n, char** out, uint64_t* out_n, int* taken);
int pf_gunzip_host_model_bgzf(const char* members, uint64_t n, char** out, uint64_t* out_n, int* taken);
/*
 * LARGE gzip members on the device, parallel inside a member: what gzip, pigz and Python's gzip.open write (one member a
 * file, any RFC 1952 head: FEXTRA, FNAME, FCOMMENT, FHCRC are skipped) and the 4 MiB zlib members of pf_gzip_members.  The
 * member's payload is cut every piece_bytes (0: 32 KiB; else at least 64); from every cut on, a wave looks for the next
 * dynamic block's header by trial; every found start is decoded once without the text before it (back-references into it
 * stay markers), the windows are chained in order, and every live piece is decoded again as bytes to its place, its CRC32
 * taken; CRC32 and ISIZE are checked against the member's tail.  Not taken: a reserved FLG bit or CM != 8, a damaged or
 * truncated member, a piece of more than 256 MiB of text or of more than 1 536 * piece_bytes compressed bytes (a member
 * of fixed or stored blocks only is one piece).  Every member of the buffer goes this route, one after the other.
 * pieces (may be NULL): [0] starts found, [1] live pieces, [2] starts dropped (false or redundant), [3] members taken.
 * Results and refusals as for pf_gunzip_device; pf_gunzip_device_last_ms: the four passes' device time.  Device memory:
 * under 1 536 * piece_bytes + 2 048 * 96 KiB and the text of a call, 256 MiB at most.
 * pf_gunzip_host_model_large: the same find, marker, chain and byte steps run serially on the host: no context, no GPU.
 */
int pf_gunzip_device_large(pf_ctx* ctx, const char* members, uint64_t n, uint32_t piece_bytes, char** out, uint64_t* out_n, int* taken,
                           uint64_t* pieces);
int pf_gunzip_host_model_large(const char* members, uint64_t n, uint32_t piece_bytes, char** out, uint64_t* out_n, int* taken,
                               uint64_t* pieces);
/* Off by default.  While on, pf_render_device[_ex] hands out gzip members in place of text (*kh, *kh_bytes, *hp,
 * *hp_bytes describe the compressed bytes) and so does pf_kmers_tsv_stream_next: every block of a range is encoded as it
 * is produced and its compressed size read back before it is copied (the host-rendered sequences are in the device text
 * and go the same way); a block's members decode to a block of the text, in order.  The stream's *total_bytes stays the
 * text's size and *peak_text_bytes includes the encoder's buffers.  pf_device_text_chunk, pf_render_pattern_rows and the
 * host renderers are not affected.  Under multiple_files the render call is pf_render_device_cluster_members (its
 * members end where a cluster's rows end) and the stream takes the clusters' ends through pf_kmers_tsv_stream_cuts. */
int pf_set_device_gzip(pf_ctx* ctx, int on, uint32_t flags);
/* The text sizes behind the compressed bytes: out[0], out[1] = bytes of kmers_to_hashes / hashes_to_patterns text of the
 * last pf_render_device[_ex]; out[2] = text bytes the open (or last) kmers.tsv or pattern-row stream has handed out so
 * far. */
int pf_device_gzip_text_bytes(pf_ctx* ctx, uint64_t out[3]);

/*
 * Row filter of the downstream tools on the device: the rows of kmers_to_hashes.tsv whose
 * hashed_pattern is one of a set of hashes (/root/reference/panfeed/get_clusters.py:89-94, get_kmers.py:103-106:
 * `x[x['hashed_pattern'].isin(passing_hashes)]` over 100 000-row pandas chunks) and the rows of kmers.tsv whose cluster
 * is one of a set of clusters (get_kmers.py:131-134).  first_field = 1: the key is the first tab-separated field of a
 * line (cluster); 0: the last one (hashed_pattern).  pf_rowfilter_scan takes a block of the file that starts at a line
 * start, tests every complete line of it on the GPU (64-bit hashes of the key field against a device hash set, every
 * candidate then checked against the exact keys on the host) and returns the matching lines, in file order, as
 * [begin, end) byte ranges of `text` (end includes the newline; valid until the next call); *consumed = bytes of complete
 * lines: the caller puts text[consumed:] in front of its next block.  The file's header line is the caller's business.
 */
typedef struct pf_rowfilter pf_rowfilter;
int pf_rowfilter_create(int device, int first_field, const char* const* keys, const uint32_t* key_len, uint64_t n_keys,
                        pf_rowfilter** out);
int pf_rowfilter_scan(pf_rowfilter* f, const char* text, uint64_t nbytes, const uint64_t** line_begin,
                      const uint64_t** line_end, uint64_t* n_lines, uint64_t* consumed);
int pf_rowfilter_stats(pf_rowfilter* f, uint64_t* bytes_scanned, float* device_ms);
/*
 * The same filter over a file of small gzip members (see pf_gunzip_device), inflated on the device and scanned where
 * the inflate left the text.  pf_rowfilter_members_begin starts a file (header = 1: its first line is no row; it is kept
 * for pf_rowfilter_members_header, valid until the next begin).  pf_rowfilter_scan_members takes a block of the
 * COMPRESSED file that starts at a member start: the whole members in it are uploaded and inflated behind the unfinished
 * line the call before left on the device, the complete lines are scanned, the candidates' lines are gathered on the
 * device and checked against the exact keys on the host.  *lines: the matching lines joined, in file order (valid until
 * the next call); *consumed: the compressed bytes of the members taken -- the caller puts members[consumed:] in front
 * of its next block.  last = 1: the block ends the file; once all of it is consumed, a final line without a newline is
 * given one.  *taken = 0 with PF_OK: as pf_gunzip_device; nothing is carried over then.
 * A block whose first head is a BGZF head (see pf_gunzip_device_bgzf) has its members listed by their BSIZE chain and is
 * taken in the same way, by this and by every other owner of the feed -- pf_assocfilter_scan_members,
 * pf_kmerjoin_survey_members / _join_members, pf_plotgrid_scan_members: there is no entry point of its own for BGZF.
 */
int pf_rowfilter_members_begin(pf_rowfilter* f, int header);
int pf_rowfilter_members_header(pf_rowfilter* f, const char** line, uint64_t* nbytes);
int pf_rowfilter_scan_members(pf_rowfilter* f, const char* members, uint64_t nbytes, int last, const char** lines,
                              uint64_t* lines_bytes, uint64_t* n_lines, uint64_t* consumed, int* taken);
/* Members and text bytes inflated by this filter, its inflate kernels' ms, the decoder's device bytes (any may be NULL). */
int pf_rowfilter_gunzip_stats(pf_rowfilter* f, uint64_t* members, uint64_t* text_bytes, float* inflate_ms, uint64_t* device_bytes);
/*
 * The large-member route (see pf_gunzip_device_large) behind pf_rowfilter_scan_members, off by default: while on, a
 * block the small-member kernels do not take -- any other RFC 1952 head, a member over their size limits -- is tried as
 * a large member from its first byte on; the members that follow it under the same first eight bytes are decoded beside
 * it in the same call, up to the next one the small-member kernels take.  A member may span calls: a call with last = 0 takes the
 * pieces whose end it can confirm and reports *consumed up to the byte that holds the next block; one that can confirm
 * nothing yet consumes nothing and is taken (the caller reads on).  With last = 1 the member must end at its tail.
 * piece_bytes: 0 for the default of 32 KiB of compressed bytes, else at least 64.  Setting it forgets an open member;
 * so does pf_rowfilter_members_begin.  pf_rowfilter_large_stats: pieces[4] as pf_gunzip_device_large's, ms[4] the device
 * time of the find, marker, chain and byte passes (either may be NULL).  The other owners of the feed have the same two
 * calls: pf_kmerjoin_*, pf_assocfilter_*, pf_plotgrid_*.
 */
int pf_rowfilter_set_large_members(pf_rowfilter* f, int on, uint32_t piece_bytes);
int pf_rowfilter_large_stats(pf_rowfilter* f, uint64_t* pieces, float* ms);
void pf_rowfilter_destroy(pf_rowfilter* f);

/*
 * panfeed-get-kmers' join on the device: /root/reference/panfeed/get_kmers.py:131-141.  The rows of
 * kmers.tsv whose cluster is a selected one come out as `cluster \t k-mer \t <text> \t <fields 2..10> \n`, in file order,
 * where <text> is what the host rendered for the row's (cluster, k-mer) -- one of two renderings -- or `empty_text` for a
 * row that has no key.  Clusters and keys are looked up by 64-bit hash and verified by their bytes on the device.
 * create: the selected clusters, each with the number (< n_bunches) of the bunch it is joined in; the keys with their two
 * texts.  A cluster or key field of 4 096 bytes or more matches nothing (as in the row filter); a key that comes twice is
 * an error.
 * survey: one pass for all bunches.  Blocks as pf_rowfilter_scan takes them (or blocks of members, as
 * pf_rowfilter_scan_members: the three *_members* calls mirror the row filter's); pf_kmerjoin_counters then gives five
 * numbers per bunch (valid until the next call): rows, rows without a key, output bytes under rendering 0 and under
 * rendering 1, and the OR of the rows' plainness flags (PF_KJ_*).  A flagged row is one that pandas' read_csv -> to_csv
 * might not print as it stands; the caller joins such a bunch another way.
 * join: the rows of one bunch of a block, in rendering `mode` 0 or 1; mode 2 keeps, as they stand, the rows that have a
 * key.  *out_bytes = the bytes of text made; pf_kmerjoin_next_text hands them out piece by piece through pinned memory
 * (*nbytes = 0: no more; a piece is valid until the next call: that call starts the copy of the piece behind its own
 * into the buffer this one lies in, as pf_kmers_tsv_stream_next does).  A row that would have been flagged is
 * PF_ERR_STATE here.
 * stats (either may be NULL): stats[0] bytes scanned, [1] rows written, [2] raw rows kept (mode 2), [3] members and
 * [4] text bytes inflated, [5] the decoder's device bytes, [6] look-ups whose hash was equal and whose bytes were not
 * (above zero only under a weakened hash, in practice), [7] rows written with the empty text; ms[0] survey kernels, [1] join kernels, [2] inflate.
 * set_gzip (off by default): while on, the text of a join call in mode 0 or 1 leaves as gzip members, as pf_gzip_device
 * makes them, and pf_kmerjoin_next_text hands out the members' bytes in place of the text.  The call's text is encoded on
 * the join's stream in slices of at most 64 MiB, a slice when the one before is handed out: the encoder (made on first use)
 * and the slice's members take device memory for 64 MiB of text at most, whatever the call wrote, and only members go to the
 * host.  A member never spans two join calls (a call's last member may be short); a call that wrote no row hands out none;
 * mode 2 stays text.  *out_bytes stays the bytes of TEXT made.  flags: pf_gzip_device's test hooks.  Switching drops what
 * is left of the last call's text.
 * gzip_stats (any may be NULL): text bytes encoded, member bytes made, the encoder's kernels' ms, the device bytes of the
 * encoder and the members' buffer.
 */
#define PF_KJ_TABS 1u      /* not exactly 10 tabs */
#define PF_KJ_BYTES 2u     /* a byte below 0x20 other than tab, of 0x80 or above, or a double quote */
#define PF_KJ_INT 4u       /* one of the six integer fields is not canonical decimal of at most 18 digits */
#define PF_KJ_EMPTY 8u     /* one of the five text fields is empty */
#define PF_KJ_NA 16u       /* a text field is one of pandas' default NA strings */
#define PF_KJ_NUMERIC 32u  /* a text field has only bytes of 0123456789+-.eE */
#define PF_KJ_WORD 64u     /* a text field is, ignoring case and a sign, inf, infinity, nan, true or false */
#define PF_KJ_LONG 128u    /* a row of more than 65 536 bytes, or a field of 4 096 bytes or more */
typedef struct pf_kmerjoin pf_kmerjoin;
int pf_kmerjoin_create(int device, const char* const* clusters, const uint32_t* cluster_len, const uint32_t* cluster_bunch,
                       uint64_t n_clusters, uint32_t n_bunches, const char* const* key_cluster, const uint32_t* key_cluster_len,
                       const char* const* key_kmer, const uint32_t* key_kmer_len, const char* const* text0, const uint32_t* text0_len,
                       const char* const* text1, const uint32_t* text1_len, uint64_t n_keys, const char* empty_text,
                       uint32_t empty_len, pf_kmerjoin** out);
int pf_kmerjoin_survey(pf_kmerjoin* j, const char* text, uint64_t nbytes, uint64_t* consumed);
int pf_kmerjoin_members_begin(pf_kmerjoin* j, int header);
int pf_kmerjoin_set_large_members(pf_kmerjoin* j, int on, uint32_t piece_bytes);
int pf_kmerjoin_large_stats(pf_kmerjoin* j, uint64_t* pieces, float* ms);
int pf_kmerjoin_members_header(pf_kmerjoin* j, const char** line, uint64_t* nbytes);
int pf_kmerjoin_survey_members(pf_kmerjoin* j, const char* members, uint64_t nbytes, int last, uint64_t* consumed, int* taken);
int pf_kmerjoin_reset_counters(pf_kmerjoin* j);
int pf_kmerjoin_counters(pf_kmerjoin* j, const uint64_t** counters, uint32_t* n_bunches);
int pf_kmerjoin_join(pf_kmerjoin* j, const char* text, uint64_t nbytes, uint32_t bunch, int mode, uint64_t* out_bytes,
                     uint64_t* consumed);
int pf_kmerjoin_join_members(pf_kmerjoin* j, const char* members, uint64_t nbytes, int last, uint32_t bunch, int mode,
                             uint64_t* out_bytes, uint64_t* consumed, int* taken);
int pf_kmerjoin_next_text(pf_kmerjoin* j, const char** piece, uint64_t* nbytes);
int pf_kmerjoin_stats(pf_kmerjoin* j, uint64_t stats[8], float ms[3]);
int pf_kmerjoin_set_gzip(pf_kmerjoin* j, int on, uint32_t flags);
int pf_kmerjoin_gzip_stats(pf_kmerjoin* j, uint64_t* text_bytes, uint64_t* member_bytes, float* encode_ms, uint64_t* device_bytes);
void pf_kmerjoin_destroy(pf_kmerjoin* j);

/*
 * The associations filter on the device: the first step of both downstream tools,
 * /root/reference/panfeed/get_clusters.py:76-88 and /root/reference/panfeed/get_kmers.py:93-106
 * (`a = pd.read_csv(associations, sep='\t', index_col=0); a = a[a[column] <= threshold]`), as one pass over the file's
 * text.  It keeps, as they stand and in file order, the data lines whose cell in field `pvalue_field` MAY be <= the
 * threshold: a superset, decided on an approximation of the cell's number against thr_hi, the threshold widened by the
 * caller (threshold + |threshold| * 2^-30); a cell whose magnitude is outside 1e-300 .. 1e300 keeps its row, an NA cell drops
 * it.  Over ALL data lines it ORs, per column of the header's n_fields, the class of every cell (PF_AF_INT ...) -- what
 * tells the dtype pandas would have inferred from the whole file -- and the rows' flags (PF_AF_ROW_*).  The caller parses
 * the kept lines alone and takes the file through pandas whole when a flag, an ODD cell or a mix of classes says so.
 * create (get_clusters.py:76-84, get_kmers.py:93-101: the column and the threshold): pvalue_field < n_fields.
 * scan (get_clusters.py:76, get_kmers.py:93: the file's text): a block of data lines that starts at a line start, as
 * pf_rowfilter_scan takes it; *out_bytes = the bytes of kept lines, *consumed = the bytes of complete lines.
 * members_begin / members_header / scan_members (the same lines, for a .gz of device-made members): as the row
 * filter's three calls; the header line is peeled off by the feed.
 * next_lines (get_clusters.py:85-88, get_kmers.py:102-106: the rows that stay): the kept lines of the last scan piece by
 * piece, as pf_kmerjoin_next_text (*nbytes = 0: no more; a piece is valid until the next call).
 * columns (the dtypes read_csv infers at get_clusters.py:76 / get_kmers.py:93): n_fields words of class bits, the OR of
 * the rows' flags, counters[0] data lines and counters[1] kept lines so far (the pointer is valid until the next call).
 * stats (either may be NULL): stats[0] bytes scanned, [1] members and [2] text bytes inflated, [3] the decoder's device
 * bytes; ms[0] the filter's kernels, ms[1] inflate.
 */
#define PF_AF_INT 1u         /* [+-]?[0-9]{1,18} */
#define PF_AF_FLOAT 2u       /* [+-]?([0-9]+\.?[0-9]*|\.[0-9]+)([eE][+-]?[0-9]+)? that is neither INT nor ODD */
#define PF_AF_NA 4u          /* the empty cell or one of pandas' default NA strings */
#define PF_AF_ODD 8u         /* inf / infinity / nan / true / false with an optional sign in any case (and no NA string), a space at
                                either end, an integer of more than 18 digits, a number of more than 18 integer digits or more than
                                5 exponent digits or whose exponent plus integer digits exceed 300 */
#define PF_AF_TEXT 16u       /* everything else */
#define PF_AF_ROW_FIELDS 1u  /* not as many fields as the header */
#define PF_AF_ROW_EMPTY 2u   /* an empty line */
#define PF_AF_ROW_BYTES 4u   /* a byte below 0x20 other than tab and newline, or a double quote */
#define PF_AF_ROW_LONG 8u    /* a row of more than 65 536 bytes, or a field of 4 096 bytes or more */
typedef struct pf_assocfilter pf_assocfilter;
int pf_assocfilter_create(int device, uint32_t pvalue_field, uint32_t n_fields, double thr_hi, pf_assocfilter** out);
int pf_assocfilter_scan(pf_assocfilter* f, const char* text, uint64_t nbytes, uint64_t* out_bytes, uint64_t* consumed);
int pf_assocfilter_members_begin(pf_assocfilter* f, int header);
int pf_assocfilter_set_large_members(pf_assocfilter* f, int on, uint32_t piece_bytes);
int pf_assocfilter_large_stats(pf_assocfilter* f, uint64_t* pieces, float* ms);
int pf_assocfilter_members_header(pf_assocfilter* f, const char** line, uint64_t* nbytes);
int pf_assocfilter_scan_members(pf_assocfilter* f, const char* members, uint64_t nbytes, int last, uint64_t* out_bytes,
                                uint64_t* consumed, int* taken);
int pf_assocfilter_next_lines(pf_assocfilter* f, const char** piece, uint64_t* nbytes);
int pf_assocfilter_columns(pf_assocfilter* f, const uint32_t** class_bits, uint32_t* n_fields, uint32_t* row_flags, uint64_t counters[2]);
int pf_assocfilter_stats(pf_assocfilter* f, uint64_t stats[4], float ms[2]);
void pf_assocfilter_destroy(pf_assocfilter* f);

/*
 * panfeed-plot's per-cluster grids on the device, over the annotated k-mer table that
 * panfeed-get-kmers writes.  Replaces /root/reference/panfeed/plot.py:195-222 (the whole table in one pandas frame, the
 * `isin` strain filter at :200, the base letter / scalar at :209-222) and the three pivot_tables per cluster at
 * :261-305 (max of the significances, handle_paralogs, handle_paralogs_text).
 *
 * pf_plotgrid_create: the phenotype strains (their index is the grid row), the column indices of cluster, strain,
 * gene_start, k-mer, strand and the p-value column (columns[6], in that order), and the --start/--stop zoom (zoom != 0).
 * pf_plotgrid_scan: a block of the table's data lines (no header) that starts at a line start; the complete lines are
 * read, *consumed = their bytes (the caller puts the rest in front of its next block).  Rows of other strains are
 * dropped; the cluster names of the rest, before the zoom, make the cluster table; rows inside the zoom become records.
 * A row whose gene_start is not an integer is dropped.  Cluster names and p-value texts are matched by their bytes.
 * pf_plotgrid_finish ends the scan.  Clusters and distinct p-value texts then have dense ids (arbitrary order): names /
 * texts are the joined bytes, offsets n + 1 entries, min / max gene_start and row count per cluster (pointers valid
 * until destroy).  pf_plotgrid_set_significance: per p-value id, the 64-bit ordered key of -log10(p) computed by the
 * caller (bits ^ 0x8000... for a positive double, ~bits for a negative one; 0 for NaN) -- the device never computes it.
 * pf_plotgrid_grids: the grids of n clusters (ids), one after the other, n_strains x (max - min + 1) cells each,
 * strain-major: key_out = the largest key of the cell's rows (0: none but NaN), cnt_out = rows << 32 | sum of the
 * rows' base letters (with one row: its letter; 0 for an empty k-mer).  Integer atomics only: the same bits every run.
 * members_begin / members_header / scan_members / gunzip_stats: the same scan over a .gz of small gzip members -- what
 * panfeed-get-kmers --gz-output writes -- as the row filter's four calls: blocks of the COMPRESSED file from a member start
 * on, inflated on the device behind the line the call before left unfinished and scanned where they land; the header line
 * (members_begin's header = 1) is peeled off by the feed and is no row.  Room for records and names is made from the
 * INFLATED bytes, and those stay under 4 GiB a call (a call inflates 256 MiB of text at most).  *taken = 0 with PF_OK: as
 * pf_gunzip_device; the grid's records and tables are then as they were before the call.
 */
typedef struct pf_plotgrid pf_plotgrid;
int pf_plotgrid_create(int device, const char* const* strains, const uint32_t* strain_len, uint32_t n_strains,
                       const int32_t* columns, int zoom, int64_t start, int64_t stop, pf_plotgrid** out);
int pf_plotgrid_scan(pf_plotgrid* g, const char* text, uint64_t nbytes, uint64_t* consumed);
int pf_plotgrid_members_begin(pf_plotgrid* g, int header);
int pf_plotgrid_set_large_members(pf_plotgrid* g, int on, uint32_t piece_bytes);
int pf_plotgrid_large_stats(pf_plotgrid* g, uint64_t* pieces, float* ms);
int pf_plotgrid_members_header(pf_plotgrid* g, const char** line, uint64_t* nbytes);
int pf_plotgrid_scan_members(pf_plotgrid* g, const char* members, uint64_t nbytes, int last, uint64_t* consumed, int* taken);
int pf_plotgrid_gunzip_stats(pf_plotgrid* g, uint64_t* members, uint64_t* text_bytes, float* inflate_ms, uint64_t* device_bytes);
int pf_plotgrid_finish(pf_plotgrid* g, uint32_t* n_clusters, uint64_t* n_pvalues, uint64_t* n_records);
int pf_plotgrid_clusters(pf_plotgrid* g, const char** names, const uint64_t** name_off, const int32_t** min_pos,
                         const int32_t** max_pos, const uint64_t** rows);
int pf_plotgrid_pvalues(pf_plotgrid* g, const char** texts, const uint64_t** text_off);
int pf_plotgrid_set_significance(pf_plotgrid* g, const uint64_t* keys);
int pf_plotgrid_grids(pf_plotgrid* g, const uint32_t* ids, uint32_t n, uint64_t* key_out, uint64_t* cnt_out);
int pf_plotgrid_stats(pf_plotgrid* g, uint64_t* bytes_scanned, uint64_t* lines, uint64_t* records, float* device_ms);
void pf_plotgrid_destroy(pf_plotgrid* g);

#ifdef __cplusplus
}
#endif
#endif
