"""Batched host driver of the HIP hot path: packs cluster records, calls libpanfeed_hip through
ctypes, and renders the three TSV bodies exactly as the reference writes them
(/root/reference/panfeed/panfeed.py:104-107, 177, 187, 208, 223).

One ``Engine`` = one panfeed run on one GPU: it owns the run-global pattern set
(panfeed.py:149-150) in device memory, so clusters must be fed in processing order.
"""
import binascii
import collections
import contextlib
import ctypes as C
import time

import numpy as np

from . import _lib
from .packing import _release_held, _seqinfo_columns, build_batch_native, decode_keys, maf_tables

KMERS_TSV_HEADER = ("cluster\tstrain\tfeature_id\tcontig\tfeature_strand\tcontig_start\tcontig_end\t"
                    "gene_start\tgene_end\tstrand\tk-mer\n")           # input.py:243
KMERS_TO_HASHES_HEADER = "cluster\tk-mer\thashed_pattern\n"            # panfeed.py:127


def hashes_to_patterns_header(strains):
    return "hashed_pattern" + "".join(f"\t{s}" for s in sorted(strains)) + "\n"   # panfeed.py:120-123


def _ptr(a):
    return a.ctypes.data_as(C.c_void_p) if a is not None and a.size else None


def _mem(ptr, n):
    """n bytes at `ptr` as a memoryview of bytes: no copy, valid as long as the memory is"""
    p = ptr.value if isinstance(ptr, C.c_void_p) else ptr
    return memoryview((C.c_char * int(n)).from_address(p)).cast("B") if n else memoryview(b"")


def _take(ptr, n):
    """n bytes at `ptr` as `bytes` (ctypes.string_at takes a C int: texts beyond 2 GiB need this)"""
    return bytes(_mem(ptr, n))


def passing_digests(hashes):
    """the 16-byte digests of `hashes`, an iterable of 24-character `hashed_pattern` strings (as the files print them) or
    of 16-byte values: a sorted list without repeats.  Anything else is a ValueError."""
    out = set()
    for h in hashes:
        if isinstance(h, str) and len(h) == 24:
            try:
                d = binascii.a2b_base64(h)
            except (binascii.Error, ValueError):
                d = b""
            if len(d) != 16 or binascii.b2a_base64(d)[:24].decode() != h:
                raise ValueError(f"not a hashed_pattern: {h!r}")
        elif isinstance(h, (bytes, bytearray, memoryview, np.ndarray)) and len(bytes(h)) == 16:
            d = bytes(h)
        else:
            raise ValueError(f"a passing hash is 24 base64 characters or 16 bytes, not {h!r}")
        out.add(d)
    return sorted(out)


def filter_passing_rows(kmers_tsv, kmers_to_hashes, passing):
    """The host's statement of the passing-rows filter, on text alone: the rows of the kmers.tsv body `kmers_tsv` whose
    (cluster, k-mer) stands in a k-mer row of the kmers_to_hashes body with a hash in `passing` (a set of 24-character
    strings).  Returns (text, rows considered, rows kept)."""
    pairs = set()
    for line in kmers_to_hashes.split("\n"):
        if line:
            idx, kmer, h = line.rsplit("\t", 2)
            if kmer and h in passing:
                pairs.add((idx, kmer))
    rows = kmers_tsv.split("\n")[:-1]
    kept = [r for r in rows if (r.split("\t", 1)[0], r.rsplit("\t", 1)[1]) in pairs]
    return "".join(r + "\n" for r in kept), len(rows), len(kept)


# pf_batch's array fields, under the names HostBatch gives them too: Engine.submit_host_batch hands them over by host
# pointer, devbatch.from_host_batch uploads them (the last three only when the batch has slow-path rows)
BATCH_ARRAYS = ("packed", "seg_word_off", "seg_len", "seg_sample", "seg_ord_base", "cluster_seg_off", "cluster_nstrains",
                "cluster_npresab", "cluster_presab", "cluster_ordinal", "extra_cluster", "extra_ord", "extra_bits")


class OwnedText:
    """a block of text the library malloc'd (pf_free_text), handed on without a copy: `view` for the writer, `release()`
    (or garbage collection) to give it back"""

    def __init__(self, L, ptr, n):
        self._L, self._p, self._n = L, (ptr.value if isinstance(ptr, C.c_void_p) else ptr), int(n)
        self.view = _mem(self._p, self._n)

    def __len__(self):
        return self._n

    def __bytes__(self):
        return bytes(self.view)

    def release(self):
        if self._p:
            self.view = memoryview(b"")
            self._L.pf_free_text(C.c_void_p(self._p))
            self._p = None

    def __del__(self):
        try:
            self.release()
        except Exception:   # noqa: BLE001  (interpreter shutdown)
            pass


class DeviceText:
    """Text the GPU wrote and still holds (pf_render_kmers_tsv_device): handed out block by block through pinned memory
    (`chunks`, each block valid until the next is asked for), or as one `bytes` (`bytes(x)`).  Belongs to the engine's
    last submit: use it before the next one."""

    def __init__(self, engine, nbytes):
        self._eng, self._n = engine, int(nbytes)

    def __len__(self):
        return self._n

    def chunks(self, max_bytes=64 << 20):
        eng, off = self._eng, 0
        ptr, nb = C.c_void_p(), C.c_uint64()
        while off < self._n:
            _lib.check(eng.L.pf_device_text_chunk(eng.ctx, off, int(max_bytes), C.byref(ptr), C.byref(nb)))
            yield _mem(ptr, nb.value)
            off += int(nb.value)

    def __bytes__(self):
        out = bytearray(self._n)
        at = 0
        for blk in self.chunks():
            out[at:at + len(blk)] = blk
            at += len(blk)
        return bytes(out)


class GzipMembers:
    """complete gzip members the GPU made of a text (Engine(device_gzip=True)): `view` holds them (as long-lived as
    the text it stands for would be), `text_bytes` is the size of the text they decode to -- None where the producer does
    not know it per block (the stream's blocks: the stream reports its text bytes as a whole); len() is the compressed
    size"""

    def __init__(self, view, text_bytes=None):
        self.view, self.text_bytes = view, None if text_bytes is None else int(text_bytes)

    def __len__(self):
        return len(self.view)

    def __bytes__(self):
        return bytes(self.view)


def text_len(data):
    """bytes of text `data` stands for: its own length, or what a GzipMembers decodes to"""
    if not isinstance(data, GzipMembers):
        return len(data)
    if data.text_bytes is None:
        raise ValueError("these gzip members' text size is not known")
    return data.text_bytes


def _view(ptr, n, dtype):
    if n == 0:
        return np.zeros(0, dtype=dtype)
    return np.ctypeslib.as_array(ptr, shape=(n,)).view(dtype) if ptr else np.zeros(0, dtype=dtype)


class BatchOutput:
    """Texts of one batch (bodies only, no headers) plus counters."""

    def __init__(self):
        self.kmers_tsv = ""
        self.kmers_to_hashes = ""
        self.hashes_to_patterns = ""
        # multiple_files: [(idx, kmers_tsv, kmers_to_hashes, hashes_to_patterns)], str or slices of the device-written
        # bodies; kmers_tsv None: the rows went to run_batches' cluster_targets_sink
        self.per_cluster = []
        self.stats = {}
        self.timing = {}

    @property
    def gzip_members(self):
        """whether kmers_to_hashes and hashes_to_patterns are gzip members (GzipMembers) instead of text"""
        return isinstance(self.kmers_to_hashes, GzipMembers) and isinstance(self.hashes_to_patterns, GzipMembers)

    @property
    def text_bytes(self):
        """bytes of text the batch stands for: its three bodies and the kmers.tsv rows that went to a sink"""
        return (text_len(self.kmers_tsv) + text_len(self.kmers_to_hashes) + text_len(self.hashes_to_patterns) +
                self.stats.get("kmers_tsv_streamed", 0))


def _batch_stats(hb, res, patterns, **streamed):
    """the counters of one batch (BatchOutput.stats); `streamed`: the kmers_tsv_* counters of a device-text batch"""
    return {"clusters": int(hb.n_clusters), "instances": int(hb.n_instances), **streamed,
            "device_instances": int(res.n_instances), "unique_kmers": int(res.n_unique), "kept_kmers": int(res.n_kept),
            "new_patterns": int(res.n_new_patterns), "patterns": int(patterns)}


def _cut(view, ends):
    """`view` cut at the offsets `ends` (non-decreasing, the last one its length): one slice per end, no copy"""
    parts, prev = [], 0
    for e in ends:
        parts.append(view[prev:int(e)])
        prev = int(e)
    return parts


def _cut_members(view, ends, text_ends):
    """gzip members cut at `ends`, where the text they decode to is cut at `text_ends`: (the whole, its pieces), each a
    GzipMembers that carries its text size"""
    pieces = [GzipMembers(piece, size) for piece, size in zip(_cut(view, ends), np.diff(text_ends, prepend=np.uint64(0)))]
    return GzipMembers(view, text_ends[-1] if len(text_ends) else 0), pieces


# the two bodies of a batch the device wrote (views, or GzipMembers) and, under multiple_files, each one's pieces per cluster
BatchBodies = collections.namedtuple("BatchBodies", "kh hp kh_parts hp_parts")


def add_batch_stats(totals, out, keys=("clusters", "instances", "kept_kmers", "device_ms")):
    """add a finished batch's counters to the totals a run reports; "device_ms": its device time, "bytes": the text it
    stands for"""
    for key in keys:
        totals[key] = totals.get(key, 0) + (out.timing.get("total_ms", 0.0) if key == "device_ms" else
                                            out.text_bytes if key == "bytes" else out.stats.get(key, 0))


def gzip_modes(compress, device_gzip, multiple_files, device_gzip_clusters=False):
    """(compress, device_gzip, device_gzip_clusters) as a run uses them: either device switch implies compress;
    per-cluster directories keep the host's gzip under device_gzip and have the device's under device_gzip_clusters,
    which means nothing without them"""
    clusters = bool(device_gzip_clusters) and bool(multiple_files)
    return bool(compress or device_gzip or clusters), bool(device_gzip) and not multiple_files, clusters


class Engine:
    def __init__(self, klength=31, canon=True, consider_missing=False, patfilt=True, maf=0.01,
                 multiple_files=False, max_strains=1024, stroi=(), device=0, pattern_capacity=0,
                 max_items=0, dedup=True, unit_dedup=True, key_binning=True, device_plan=False,
                 targets_text_budget=8 << 30, device_gzip=False, device_gzip_flags=0, device_gzip_clusters=False, bgzf=False,
                 passing_hashes=None):
        self.L = _lib.load()
        # device memory a batch's kmers.tsv text may take when it is streamed to a targets_sink (stream_targets_device)
        self.targets_text_budget = int(targets_text_budget)
        self.k = int(klength)
        self.canon = bool(canon)
        self.consider_missing = bool(consider_missing)
        self.patfilt = bool(patfilt)
        self.maf = float(maf)
        self.multiple_files = bool(multiple_files)
        self.max_strains = int(max_strains)
        self.W = (self.max_strains + 31) // 32
        self.stroi = stroi if stroi else ()
        self._lo, self._hi = maf_tables(self.maf, self.max_strains)
        o = _lib.Opts(self.k, int(self.canon), int(self.consider_missing), int(self.patfilt),
                      int(self.multiple_files), self.max_strains,
                      self._lo.ctypes.data_as(C.POINTER(C.c_uint32)), self._hi.ctypes.data_as(C.POINTER(C.c_uint32)),
                      int(pattern_capacity), int(max_items),
                      (0 if dedup else _lib.FLAG_NO_DEDUP) | (0 if unit_dedup else _lib.FLAG_NO_UNIT_DEDUP) |
                      (0 if key_binning else _lib.FLAG_NO_KEY_BINNING) | (_lib.FLAG_DEVICE_PLAN if device_plan else 0))
        self.ctx = C.c_void_p()
        _lib.check(self.L.pf_create(C.byref(self.ctx), int(device), C.byref(o)))
        # device_gzip: the texts the GPU writes (render_device, stream_targets_device) leave it as gzip members; the host
        # renderers are not affected, nor is a --multiple-files run: its device text is cut into the clusters' files, whose
        # gzip stays the host's
        # device_gzip_clusters (multiple_files only): the per-cluster files' bodies leave the GPU as gzip members that end
        # where a cluster's rows end (render_device_cluster_members, stream_targets_device's cluster sink)
        _, self.device_gzip, self.device_gzip_clusters = gzip_modes(False, device_gzip, self.multiple_files, device_gzip_clusters)
        # bgzf (with device_gzip, not for multiple_files): those members are BGZF members (PF_GZ_BGZF), for a file that
        # output.BgzfMemberWriter writes
        self.bgzf = bool(bgzf)
        if self.bgzf and not self.device_gzip:
            self.close()
            raise ValueError("bgzf is for device_gzip without multiple_files")
        if self.device_gzip or self.device_gzip_clusters:
            _lib.check(self.L.pf_set_device_gzip(self.ctx, 1, int(device_gzip_flags) | (_lib.GZ_BGZF if self.bgzf else 0)))
        # passing_hashes (None: off; an empty iterable: on, no row passes): kmers.tsv holds the rows of passing patterns
        # only -- those whose (cluster, k-mer) kmers_to_hashes lists with one of these hashes
        self.passing = None
        if passing_hashes is not None:
            try:
                self.set_passing_hashes(passing_hashes)
            except Exception:
                self.close()
                raise
        self.next_ordinal = 0
        self._md5_b64 = {}      # pattern id -> 24-char hash string (patterns seen so far)
        self.n_patterns = 0

    def close(self):
        if getattr(self, "ctx", None):
            self.L.pf_destroy(self.ctx)
            self.ctx = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # ------------------------------------------------------------------ rows of passing patterns only
    def set_passing_hashes(self, hashes):
        """turn the passing-rows filter on (pf_set_passing_hashes) with `hashes` (see passing_digests); None: off"""
        if hashes is None:
            _lib.check(self.L.pf_clear_passing_hashes(self.ctx))
            self.passing = None
            return
        digests = passing_digests(hashes)
        blob = b"".join(digests)
        _lib.check(self.L.pf_set_passing_hashes(self.ctx, blob if blob else None, len(digests)))
        self.passing = frozenset(binascii.b2a_base64(d)[:24].decode() for d in digests)

    def passing_stats(self):
        """pf_passing_stats: (digests, kept k-mers marked, rows considered, rows kept, hash equal and bytes not, device bytes)"""
        out = (C.c_uint64 * 6)()
        _lib.check(self.L.pf_passing_stats(self.ctx, out))
        return tuple(int(x) for x in out)

    def _passing_names(self, hb):
        """before a filtered kmers.tsv text of `hb`: the batch's names and slow-path rows for the library's filter"""
        if self.passing is None:
            return
        names = (C.c_char_p * max(hb.n_clusters, 1))(*[s.encode() for s in hb.idx])
        extra = "".join(hb.extra_keys).encode("latin-1") if hb.extra_keys else None
        _lib.check(self.L.pf_passing_batch_names(self.ctx, names, extra, len(hb.extra_keys)))

    def _passing_rows(self, hb):
        """what the filtered device text of `hb` adds to the batch's counters"""
        if self.passing is None:
            return {}
        st = self.passing_stats() if hb.n_targets else (0,) * 6
        return {"kmers_rows_considered": st[2], "kmers_rows_kept": st[3], "passing_digests": len(self.passing)}

    # ------------------------------------------------------------------ device calls
    def submit_host_batch(self, hb):
        if self.consider_missing and not np.array_equal(hb.cluster_nstrains, hb.cluster_npresab):
            # the reference stops in init_presabs_vector (panfeed.py:19): a boolean mask of another length
            ci = int(np.flatnonzero(np.asarray(hb.cluster_nstrains) != np.asarray(hb.cluster_npresab))[0])
            raise IndexError(f"cluster {hb.idx[ci]}: boolean index did not match indexed array along axis 0; size of "
                             f"axis is {int(hb.cluster_nstrains[ci])} but size of corresponding boolean axis is "
                             f"{int(hb.cluster_npresab[ci])}")
        if self.multiple_files:
            # the library starts every batch with an empty pattern pool (ids are cluster-local, panfeed.py:165)
            self._md5_b64 = {}
            self.n_patterns = 0
        b = _lib.Batch()
        b.n_clusters = hb.n_clusters
        b.n_segs = len(hb.seg_len)
        b.n_words = len(hb.packed)
        b.on_device = 0
        b.n_extra = len(hb.extra_ord)
        for f in BATCH_ARRAYS:
            setattr(b, f, _ptr(getattr(hb, f)))
        if hb.n_strand_words:
            b.seg_strand_off = _ptr(hb.seg_strand_off)
            b.n_strand_words = hb.n_strand_words
        res = _lib.Result()
        if hb.gather_src_off is not None:
            # segments are ranges of the genomes resident in HBM; b.packed = the few the host packed itself
            g = _lib.Gather(int(hb.n_words_dev), hb.gather_src_off.ctypes.data, hb.gather_src_start.ctypes.data,
                            hb.gather_src_flags.ctypes.data)
            _lib.check(self.L.pf_submit_gather(self.ctx, C.byref(b), C.byref(g), C.byref(res)))
        else:
            _lib.check(self.L.pf_submit(self.ctx, C.byref(b), C.byref(res)))
        return res

    def fetch(self):
        res = _lib.Result()
        _lib.check(self.L.pf_fetch(self.ctx, C.byref(res)))
        return res

    def timing(self):
        t = _lib.Timing()
        _lib.check(self.L.pf_get_timing(self.ctx, C.byref(t)))
        return {f: getattr(t, f) for f, _ in _lib.Timing._fields_ if f != "reserved"}

    # ------------------------------------------------------------------ one batch, text out
    def run(self, records):
        """cluster_cutter + pattern_hasher over `records` (in processing order)."""
        records = list(records)
        hb = build_batch_native(records, self.k, self.canon, self.W, stroi=self.stroi,
                                first_ordinal=self.next_ordinal)
        self.next_ordinal += len(records)
        self.submit_host_batch(hb)
        res = self.fetch()
        return self._render(hb, res)

    def run_stream(self, records, batch_clusters=256, prefetch=2, defer_patterns=False, device_text=False,
                   targets_sink=None, cluster_targets_sink=None):
        """Generator over BatchOutput: packs batch i+1 (host threads, pf_pack_records) while the GPU works on
        batch i and the caller writes batch i-1 -- the reference's reader / workers / writer pipeline
        (__main__.py:39-81,299-344) with the GPU in the workers' place and a deterministic order
        (always the --cores 1 order, whatever finishes first).  device_text: the two big files' text written by the GPU
        and handed over as bytes-like blocks (see run_batches) instead of `str`."""
        import itertools
        it = iter(records)

        def host_batches():
            ordinal = self.next_ordinal
            while True:
                chunk = list(itertools.islice(it, batch_clusters))
                if not chunk:
                    return
                yield build_batch_native(chunk, self.k, self.canon, self.W, stroi=self.stroi, first_ordinal=ordinal)
                ordinal += len(chunk)
        return self.run_batches(host_batches(), prefetch, device_text, defer_patterns=defer_patterns,
                                targets_sink=targets_sink, cluster_targets_sink=cluster_targets_sink)

    def run_pangenome(self, pangenome, batch_clusters=256, prefetch=2, device_text=False, defer_patterns=False,
                      before_first_submit=None, targets_sink=None, cluster_targets_sink=None):
        """run_stream fed by the native reader (native_input.Pangenome): table rows -> records -> packed batches
        without leaving the library, then the GPU; yields BatchOutput in table order."""
        if tuple(sorted(pangenome.targets)) != tuple(sorted(self.stroi or ())):
            raise ValueError("the pangenome reader and the engine were given different target strains")
        return self.run_batches(pangenome.batches(self.k, self.canon, self.W, max_clusters=batch_clusters,
                                                  first_ordinal=self.next_ordinal), prefetch, device_text,
                                defer_patterns=defer_patterns, before_first_submit=before_first_submit,
                                targets_sink=targets_sink, cluster_targets_sink=cluster_targets_sink)

    def run_batches(self, host_batches, prefetch=2, device_text=False, defer_patterns=False, before_first_submit=None,
                    targets_sink=None, cluster_targets_sink=None):
        """GPU over an iterator of HostBatch, the next ones being prepared on one host thread meanwhile.
        device_text: kmers_to_hashes / hashes_to_patterns of a batch without target-strain rows come back as
        memoryviews of text the GPU wrote (render_device; valid until the batch after the next one has been rendered)
        instead of str.  Under multiple_files the same two bodies come with their cluster boundaries
        (render_device_clusters): `out.per_cluster[i] = (idx, kt, kh_i, hp_i)` holds slices of them, and
        `out.stats["device_cluster_files"]` says for how many of the batch's clusters (0: the batch fell back to the host
        renderers).  With device_gzip_clusters those slices are GzipMembers (render_device_cluster_members) and
        `out.stats["compressed_bytes"]` is the encoder's count of the batch's members.
        defer_patterns: leave hashes_to_patterns empty -- a rank of a sharded run renders its pattern rows after the
        run-global merge (`render_pattern_rows`).
        before_first_submit: called once, right before the first pf_submit (pipeline.run_files joins the thread that
        uploads the genomes there: the packer has been at work on the first batches meanwhile).
        targets_sink (with device_text): called with every block of a batch's kmers.tsv rows as it leaves the device
        (a bytes-like view, valid during the call) instead of the rows being gathered into `out.kmers_tsv` -- with every
        strain a target a batch's rows are tens of gigabytes (BASELINE configs[4]'s second pass: 256 clusters x 5 000
        samples = 150 GB), which neither a host buffer nor one device buffer should hold: the GPU writes them in ranges of
        at most `targets_text_budget` bytes of device memory (stream_targets_device); `out.stats["kmers_tsv_streamed"]`
        says how many bytes went, `"kmers_tsv_ranges"` / `"kmers_tsv_peak_device_bytes"` in how many ranges and with how
        much device memory at most.
        cluster_targets_sink (multiple_files): called as `sink(idx, block)` with the kmers.tsv rows of cluster `idx` -- at
        least once for every cluster of a batch, in order, with an empty block where a cluster has no target row -- instead
        of the rows standing in `out.per_cluster` (their place holds None).  With device_text the rows are streamed within
        `targets_text_budget` like targets_sink's and cut at the cluster ends as they arrive (output.ClusterSplitter)."""
        from concurrent.futures import ThreadPoolExecutor
        it = iter(host_batches)
        # where the wall time of this run goes (seconds; bench.py's end-to-end leg): the packer thread's busy time
        # (read + pack, overlapped with the GPU), the time this thread waited for it, pf_submit (upload + kernels),
        # the text stage (device text + its copy to the host, or pf_fetch + the host renderers)
        st = self.stages = {"pack_busy_s": 0.0, "pack_wait_s": 0.0, "submit_s": 0.0, "device_ms": 0.0, "text_s": 0.0,
                            "batches": 0}
        sink = cluster_targets_sink if self.multiple_files else targets_sink      # (each mode has its own; the other's is not used)

        def pack_next():
            t0 = time.perf_counter()
            hb = next(it, None)
            st["pack_busy_s"] += time.perf_counter() - t0
            return hb

        with ThreadPoolExecutor(max_workers=1) as pool:      # one packer thread keeps the record order
            pending = [pool.submit(pack_next) for _ in range(max(1, prefetch))]
            while pending:
                t0 = time.perf_counter()
                hb = pending.pop(0).result()
                st["pack_wait_s"] += time.perf_counter() - t0
                if hb is None:
                    break
                pending.append(pool.submit(pack_next))
                self.next_ordinal = int(hb.cluster_ordinal[-1]) + 1 if hb.n_clusters else self.next_ordinal
                if before_first_submit is not None:
                    t0 = time.perf_counter()
                    before_first_submit()
                    before_first_submit = None
                    st["first_submit_wait_s"] = time.perf_counter() - t0
                t0 = time.perf_counter()
                res = self.submit_host_batch(hb)
                t1 = time.perf_counter()
                st["submit_s"] += t1 - t0
                st["batches"] += 1
                out = self._batch_text(hb, res, device_text, defer_patterns, sink)
                st["text_s"] += time.perf_counter() - t1
                st["device_ms"] += out.timing.get("total_ms", 0.0)
                yield out

    # ------------------------------------------------------------------ the text stage of one batch
    def _batch_text(self, hb, res, device_text, defer_patterns, sink):
        """the BatchOutput of the batch just submitted: its text written by the device (device_text), or -- without it,
        or for a batch the text kernels cannot lay out (too many passes, an over-long cluster name) -- by the host
        renderers.  sink: the run's targets_sink, or under multiple_files its cluster_targets_sink."""
        if device_text:
            try:
                bodies = self._device_bodies(hb, defer_patterns)
            except _lib.PanfeedHipError as e:
                if e.status not in (_lib.ERR_CAPACITY, _lib.ERR_ARG):
                    raise
            else:
                return self._device_batch(hb, res, bodies, sink)
            # pf_fetch mirrors the digests of this batch's new patterns only: those of the batches the device rendered
            # were never fetched, and the host's kmers_to_hashes rows name them -- the whole pool's digests come over first
            self.export_patterns()
        return self._host_batch(hb, defer_patterns, sink)

    def _device_bodies(self, hb, defer_patterns):
        """kmers_to_hashes and hashes_to_patterns of the last submit by the render call of the engine's mode"""
        if self.device_gzip_clusters:       # the clusters' pieces are GzipMembers that carry their text sizes
            kh, hp, kh_end, hp_end, kh_text_end, hp_text_end = self.render_device_cluster_members(hb)
            (kh, kh_parts), (hp, hp_parts) = _cut_members(kh, kh_end, kh_text_end), _cut_members(hp, hp_end, hp_text_end)
            return BatchBodies(kh, hp, kh_parts, hp_parts)
        if self.multiple_files:
            kh, hp, kh_end, hp_end = self.render_device_clusters(hb)
            return BatchBodies(kh, hp, _cut(kh, kh_end), _cut(hp, hp_end))
        return BatchBodies(*self.render_device(hb, defer_patterns), None, None)

    def _device_rows(self, hb, sink):
        """the kmers.tsv rows of a device-text batch, written by the GPU too (the next submit reuses the device's text
        block, so the rows come over now): streamed to `sink` in ranges of at most targets_text_budget bytes of device
        memory, or gathered.  Returns (kmers_tsv, its per-cluster pieces under multiple_files -- None each where they went
        to the sink --, streamed, ranges, peak, compressed)."""
        per_cluster = self.multiple_files
        text, parts, counts, compressed = b"", None, (0, 0, 0), 0
        if sink is not None and hb.n_targets:
            counts = self.stream_targets_device(hb, sink, cluster_sink=True) if per_cluster else self.stream_targets_device(hb, sink)
            compressed = self.stream_compressed
        elif sink is not None and per_cluster:
            for idx in hb.idx:
                sink(idx, b"")
        elif hb.n_targets:
            text = bytes(self.render_targets_device(hb))
        if per_cluster and sink is not None:
            parts = [None] * hb.n_clusters
        elif per_cluster:
            parts = _cut(memoryview(text), self.target_cluster_ends(hb)) if hb.n_targets else [b""] * hb.n_clusters
        return (text, parts) + tuple(counts) + (compressed,)

    def _device_batch(self, hb, res, bodies, sink):
        """the BatchOutput of a batch whose text the device wrote"""
        out = BatchOutput()
        out.kmers_to_hashes, out.hashes_to_patterns = bodies.kh, bodies.hp
        out.kmers_tsv, kt_parts, streamed, ranges, peak, compressed = self._device_rows(hb, sink)
        more = {}
        if self.multiple_files:
            out.per_cluster = list(zip(hb.idx, kt_parts, bodies.kh_parts, bodies.hp_parts))
            more["device_cluster_files"] = hb.n_clusters
        more.update(self._passing_rows(hb))
        out.stats = _batch_stats(hb, res, self.pattern_count(), kmers_tsv_streamed=streamed, kmers_tsv_ranges=ranges,
                                 kmers_tsv_peak_device_bytes=peak, **more)
        if self.device_gzip or self.device_gzip_clusters:      # the members the GPU made of this batch, by the encoder's own count
            out.stats["compressed_bytes"] = len(bodies.kh) + len(bodies.hp) + compressed
        out.timing = self.timing()
        return out

    def _host_batch(self, hb, defer_patterns, sink):
        """the BatchOutput of a batch by the host renderers; its kmers.tsv rows go to `sink` now (the rows of this batch
        must not overtake, or be overtaken by, the streamed rows of its neighbours)"""
        out = self._render(hb, self.fetch(), defer_patterns)
        if self.multiple_files:
            out.stats["device_cluster_files"] = 0
        if sink is not None and (self.multiple_files or out.kmers_tsv):
            out.stats["kmers_tsv_streamed"] = len(out.kmers_tsv)
            if self.multiple_files:
                for i, (idx, kt, kh, hp) in enumerate(out.per_cluster):
                    sink(idx, kt.encode())
                    out.per_cluster[i] = (idx, None, kh, hp)
            else:
                sink(out.kmers_tsv)
            out.kmers_tsv = ""
        return out

    def result_checksum(self):
        """(k-mer rows, cluster rows, kept) checksums of the last submit, computed on the device (pf_result_checksum)"""
        out = (C.c_uint64 * 3)()
        _lib.check(self.L.pf_result_checksum(self.ctx, out))
        return tuple(int(x) for x in out)

    def pattern_count(self):
        n = C.c_uint64()
        _lib.check(self.L.pf_pattern_count(self.ctx, C.byref(n)))
        return int(n.value)

    def _hash_strings(self, res):
        p0, p1 = self.n_patterns, int(res.n_patterns)
        if p1 > p0:
            md5 = _view(res.pattern_md5, p1 * 16, np.uint8).reshape(p1, 16)
            buf = C.create_string_buffer(24)
            for pid in range(p0, p1):
                d = md5[pid].tobytes()
                self.L.pf_b64_digest(d, buf)
                self._md5_b64[pid] = buf.raw[:24].decode()
            self.n_patterns = p1
        return self._md5_b64

    def _pattern_row(self, res, pid):
        """'<hash>\\t<patterntup>\\n'  (panfeed.py:181-187, 217-223)"""
        W = self.W
        nk = int(res.pattern_n[pid])
        n = nk & 0x7FFFFFFF
        bits = _view(res.pattern_bits, (pid + 1) * W, np.uint32)[pid * W:(pid + 1) * W]
        b = (bits[np.arange(n) >> 5] >> (np.arange(n, dtype=np.uint32) & 31)) & 1 if n else np.zeros(0, np.uint32)
        cells = [str(int(x)) for x in b]
        if self.consider_missing and not (nk >> 31) and res.pattern_nan:
            nan = _view(res.pattern_nan, (pid + 1) * W, np.uint32)[pid * W:(pid + 1) * W]
            isn = (nan[np.arange(n) >> 5] >> (np.arange(n, dtype=np.uint32) & 31)) & 1
            cells = ["" if isn[i] else cells[i] for i in range(n)]
        return self._md5_b64[pid] + "\t" + "\t".join(cells) + "\n"

    def _render(self, hb, res, defer_patterns=False):
        out = BatchOutput()
        C_ = hb.n_clusters
        first_seen = _view(res.pattern_first_seen, int(res.n_patterns), np.uint64)
        new_ids = _view(res.new_pattern_id, int(res.n_new_patterns), np.uint32)

        # kmers_to_hashes.tsv body (panfeed.py:177, 208): rendered by the library's host threads
        names = (C.c_char_p * max(C_, 1))(*[s.encode() for s in hb.idx])
        extra = (C.c_char_p * len(hb.extra_keys))(*[k.encode() for k in hb.extra_keys]) if hb.extra_keys else None
        buf, nb = C.c_void_p(), C.c_uint64()
        ends = (C.c_uint64 * max(C_, 1))()
        _lib.check(self.L.pf_render_kmers_to_hashes(self.ctx, names, extra, C.byref(buf), C.byref(nb), ends))
        kh_bytes = _take(buf, nb.value)
        self.L.pf_free_text(buf)
        kh_all = kh_bytes.decode()
        kh_parts = []
        if self.multiple_files:
            prev = 0
            for ci in range(C_):
                kh_parts.append(kh_bytes[prev:ends[ci]].decode())
                prev = ends[ci]
        # hashes_to_patterns.tsv body: new patterns in first-seen order (panfeed.py:179-187, 210-223)
        hp_by_cluster = [[] for _ in range(C_)]
        if self.multiple_files:
            hashes = self._hash_strings(res)
            ord0 = int(hb.cluster_ordinal[0]) if C_ else 0
            for pid in new_ids:
                pid = int(pid)
                ci = int(first_seen[pid] >> np.uint64(32)) - ord0
                hp_by_cluster[ci].append(self._pattern_row(res, pid))
            hp_all = "".join("".join(x) for x in hp_by_cluster)
        elif defer_patterns:
            hp_all = ""
        else:
            buf, nb = C.c_void_p(), C.c_uint64()
            _lib.check(self.L.pf_render_hashes_to_patterns(self.ctx, C.byref(buf), C.byref(nb)))
            hp_all = _take(buf, nb.value).decode()
            self.L.pf_free_text(buf)
        # kmers.tsv body (panfeed.py:90-107): one row per window of the target strains' sequences
        kt_by_cluster = [[] for _ in range(C_)]
        considered = kept = 0
        if hb.n_targets and self.passing is not None:
            # the filter's second, independent statement: the host renderer's rows (pf_render_kmers_tsv knows no filter)
            # against the pairs the fetched k-mers and digests put into kmers_to_hashes
            by_cl = {}
            for meta in hb.targets:
                by_cl.setdefault(meta.cluster if self.multiple_files else 0, []).append(meta)
            for ci, metas in by_cl.items():
                text, n_rows, n_kept = filter_passing_rows(self._render_targets(hb, metas), kh_all, self.passing)
                kt_by_cluster[ci].append(text)
                considered, kept = considered + n_rows, kept + n_kept
        elif hb.n_targets:
            if self.multiple_files:
                by_cl = {}
                for meta in hb.targets:
                    by_cl.setdefault(meta.cluster, []).append(meta)
                for ci, metas in by_cl.items():
                    kt_by_cluster[ci].append(self._render_targets(hb, metas))
            else:
                # written by the GPU (kt_text_kernel); sequences with a letter outside A/C/G/T by the host renderer, in place
                kt_by_cluster[0].append(bytes(self.render_targets_device(hb)).decode())
        if self.multiple_files:
            for ci in range(C_):
                out.per_cluster.append((hb.idx[ci], "".join(kt_by_cluster[ci]), kh_parts[ci],
                                        "".join(hp_by_cluster[ci])))
        out.kmers_to_hashes = kh_all
        out.hashes_to_patterns = hp_all
        out.kmers_tsv = "".join("".join(x) for x in kt_by_cluster)
        out.stats = _batch_stats(hb, res, res.n_patterns)
        if self.passing is not None:
            out.stats.update(kmers_rows_considered=considered, kmers_rows_kept=kept, passing_digests=len(self.passing))
        out.timing = self.timing()
        return out

    def _render_call(self, fn, hb, flags=(), n_ends=0):
        """one render of the last submit's two bodies on the device by `fn` (pf_render_device_ex after `flags`, or one
        of its per-cluster kin with `n_ends` arrays of per-cluster ends behind the texts): the two memoryviews, then the
        ends, one uint64 per cluster of `hb` in each"""
        n_cl = hb.n_clusters
        names = (C.c_char_p * max(n_cl, 1))(*[s.encode() for s in hb.idx])
        extra = "".join(hb.extra_keys).encode("latin-1") if hb.extra_keys else None
        kh, kn, hp, hn = C.c_void_p(), C.c_uint64(), C.c_void_p(), C.c_uint64()
        ends = [np.zeros(max(n_cl, 1), dtype=np.uint64) for _ in range(n_ends)]
        _lib.check(fn(self.ctx, names, extra, len(hb.extra_keys), *flags, C.byref(kh), C.byref(kn), C.byref(hp), C.byref(hn),
                      *[e.ctypes.data for e in ends]))
        return (_mem(kh, kn.value), _mem(hp, hn.value)) + tuple(e[:n_cl] for e in ends)

    def render_device(self, hb, defer_patterns=False):
        """(kmers_to_hashes body, hashes_to_patterns body) of the last submit as memoryviews over pinned host memory,
        the text having been written by the GPU (pf_render_device): no pf_fetch, no bytes -> str; valid until the
        render after the next one.  kmers.tsv rows (target strains) still come from `_render` / `_render_targets`."""
        kh, hp = self._render_call(self.L.pf_render_device_ex, hb, (_lib.RENDER_NO_PATTERN_ROWS if defer_patterns else 0,))
        if self.device_gzip:
            raw = (C.c_uint64 * 3)()
            _lib.check(self.L.pf_device_gzip_text_bytes(self.ctx, raw))
            return GzipMembers(kh, raw[0]), GzipMembers(hp, raw[1])
        return kh, hp

    def render_device_clusters(self, hb):
        """render_device for an engine made with multiple_files (pf_render_device_clusters): (kmers_to_hashes body,
        hashes_to_patterns body, kh_end, hp_end) of the last submit -- the two memoryviews over pinned host memory (valid
        until the render after the next one) and, per cluster of `hb`, the offset just behind its rows in each (uint64
        arrays; a cluster without rows repeats the end before it).  Bodies only: the headers are the writer's."""
        return self._render_call(self.L.pf_render_device_clusters, hb, n_ends=2)

    def render_device_cluster_members(self, hb):
        """render_device_clusters for an engine made with device_gzip_clusters (pf_render_device_cluster_members): the
        two bodies as gzip members no one of which holds rows of two clusters -- (kh members, hp members, kh_end, hp_end,
        kh_text_end, hp_text_end): per cluster of `hb` the offset just behind its members in each view, and behind its
        rows in the text they decode to.  A cluster's piece is a gzip file's body as it stands."""
        return self._render_call(self.L.pf_render_device_cluster_members, hb, n_ends=4)

    def target_cluster_ends(self, hb):
        """per cluster of `hb`, the offset just behind its rows in the kmers.tsv text last written on the device for `hb`
        (render_targets_device, or a stream_targets_device under way or over): the library's per-sequence ends
        (pf_kmers_tsv_seq_ends) at the places where the sequences' cluster index changes.  A cluster without target rows
        repeats the end before it."""
        n = hb.n_targets
        ends = np.zeros(max(n, 1), dtype=np.uint64)
        _lib.check(self.L.pf_kmers_tsv_seq_ends(self.ctx, ends.ctypes.data, n))
        ci = self._target_clusters
        if len(ci) != n or (n > 1 and bool(np.any(ci[1:] < ci[:-1]))):
            raise ValueError("the target sequences of the batch do not stand cluster by cluster")
        upto = np.searchsorted(ci, np.arange(hb.n_clusters), side="right")      # sequences of clusters 0 .. i
        return np.where(upto > 0, ends[np.maximum(upto, 1) - 1], 0).astype(np.uint64)

    # ------------------------------------------------------------------ run-global patterns (multi-GPU)
    def export_patterns(self):
        """(md5 uint8 [n,16], first_seen uint64 [n]) of every pattern this engine holds, as numpy arrays"""
        n = C.c_uint64()
        p_md5 = C.POINTER(C.c_uint8)()
        p_fs = C.POINTER(C.c_uint64)()
        _lib.check(self.L.pf_export_patterns(self.ctx, C.byref(n), C.byref(p_md5), C.byref(p_fs)))
        n = int(n.value)
        if n == 0:
            return np.zeros((0, 16), dtype=np.uint8), np.zeros(0, dtype=np.uint64)
        md5 = np.ctypeslib.as_array(p_md5, shape=(n * 16,)).reshape(n, 16).copy()
        return md5, np.ctypeslib.as_array(p_fs, shape=(n,)).copy()

    def render_pattern_rows(self, pids, chunk_bytes=256 << 20):
        """hashes_to_patterns.tsv rows of the patterns `pids` (any ids of the pool, in this order), written on the
        device (pf_render_pattern_rows); yields `bytes` blocks of about chunk_bytes."""
        pids = np.ascontiguousarray(pids, dtype=np.uint32)
        per_row = 24 + 2 * self.max_strains + 1
        step = max(1, int(chunk_bytes // per_row))
        for a in range(0, len(pids), step):
            part = pids[a:a + step]
            txt, nb = C.c_void_p(), C.c_uint64()
            _lib.check(self.L.pf_render_pattern_rows(self.ctx, part.ctypes.data_as(C.c_void_p), len(part),
                                                     C.byref(txt), C.byref(nb)))
            yield _take(txt, nb.value)

    def stream_pattern_rows(self, pids, sink, slice_bytes=0):
        """the same rows (the bytes of `render_pattern_rows(pids)`) handed to `sink` slice by slice as they leave the
        device (pf_pattern_rows_stream_begin / _next): a memoryview of pinned memory, or under device_gzip a GzipMembers
        of the slice's members, valid during the call; slice i + 1 is written (and encoded) while the sink has slice i.
        Device memory: two slices of at most `slice_bytes` (0: 64 MiB) plus 8 bytes per row (the ids, the row lengths),
        whatever the size of the text.  Returns (text bytes, bytes handed out, slices)."""
        pids = np.ascontiguousarray(pids, dtype=np.uint32)
        total, slices = C.c_uint64(), C.c_uint32()
        _lib.check(self.L.pf_pattern_rows_stream_begin(self.ctx, pids.ctypes.data_as(C.c_void_p), len(pids),
                                                       int(slice_bytes), C.byref(total), C.byref(slices)))
        text, handed = self._drain_stream(self.L.pf_pattern_rows_stream_next, sink, self.device_gzip, total.value,
                                          "pattern-row stream")
        return text, handed, int(slices.value)

    def _drain_stream(self, next_block, take, gzip_on, total, what, close=None):
        """the blocks of the device text stream just begun, from `next_block` (a *_stream_next entry point) until it
        hands out none, each given to `take` as a memoryview of pinned memory, or under gzip_on as a GzipMembers of its
        members (the text bytes behind them are the library's count); `close`, where given, is called after the last.
        Returns (text bytes, bytes handed out); text bytes other than `total` are an error."""
        ptr, nb = C.c_void_p(), C.c_uint64()
        handed = 0
        while True:
            _lib.check(next_block(self.ctx, C.byref(ptr), C.byref(nb)))
            if not nb.value:
                break
            view = _mem(ptr, nb.value)
            take(GzipMembers(view, None) if gzip_on else view)
            handed += int(nb.value)
        text = handed
        if gzip_on:
            raw = (C.c_uint64 * 3)()
            _lib.check(self.L.pf_device_gzip_text_bytes(self.ctx, raw))
            text = int(raw[2])
        if close is not None:
            close()
        if text != int(total):
            raise _lib.PanfeedHipError(_lib.ERR_STATE, f"{what}: {text} bytes handed out of {total}")
        return text, handed

    def render_targets_device(self, hb):
        """kmers.tsv rows of every target sequence of `hb` (the last submit), written on the device
        (pf_render_kmers_tsv_device): a DeviceText.  Same bytes as `_render_targets(hb, hb.targets)`."""
        t0 = time.time()
        nb = C.c_uint64()
        self._passing_names(hb)
        with self._target_records(hb) as (arr, n):
            t1 = time.time()
            _lib.check(self.L.pf_render_kmers_tsv_device(self.ctx, arr, n, C.byref(nb)))
        self.render_targets_timing = {"marshal_s": t1 - t0, "render_s": time.time() - t1, "copy_s": 0.0}
        return DeviceText(self, nb.value)

    def stream_targets_device(self, hb, sink, budget=None, cluster_sink=False):
        """kmers.tsv rows of every target sequence of `hb` (the last submit), written on the device in ranges that take
        at most `budget` bytes of device memory (default: targets_text_budget) and handed to `sink` block by block (a
        memoryview of pinned memory, valid during the call) -- pf_kmers_tsv_stream_begin / _next.  The blocks joined are
        the bytes of `render_targets_device(hb)`.  cluster_sink: `sink` is a cluster sink, `sink(idx, block)` -- the blocks are
        cut at the cluster ends as they arrive, and every cluster of `hb` gets at least one call (output.ClusterSplitter).
        Under device_gzip_clusters the stream is told the cluster ends (pf_kmers_tsv_stream_cuts), so that members end
        there, and the cluster sink gets GzipMembers of whole members with their text sizes (output.ClusterMemberSplitter).
        Returns (bytes, ranges, peak device text bytes)."""
        t0 = time.time()
        budget = self.targets_text_budget if budget is None else int(budget)
        self.stream_compressed = 0
        # (the records and the strings they point to are read until the last block: the host renders its share of
        # every range when the range is written)
        self._passing_names(hb)
        with self._target_records(hb) as (arr, n):
            total, ranges, peak = C.c_uint64(), C.c_uint32(), C.c_uint64()
            t1 = time.time()
            _lib.check(self.L.pf_kmers_tsv_stream_begin(self.ctx, arr, n, budget, C.byref(total), C.byref(ranges),
                                                        C.byref(peak)))
            gzip_on = self.device_gzip or self.device_gzip_clusters
            take, close = self._cluster_blocks(hb, sink, gzip_on) if cluster_sink else (sink, None)

            def counted(block):
                take(block)
                self.stream_compressed += len(block) if gzip_on else 0
            streamed, _ = self._drain_stream(self.L.pf_kmers_tsv_stream_next, counted, gzip_on, total.value, "kmers.tsv stream", close)
        self.render_targets_timing = {"marshal_s": t1 - t0, "render_s": time.time() - t1, "copy_s": 0.0}
        return streamed, int(ranges.value), int(peak.value)

    def _cluster_blocks(self, hb, sink, gzip_on):
        """(take, close) for the blocks of the kmers.tsv stream just begun for `hb` where `sink` is a cluster sink: a
        splitter of the output module that cuts them at the clusters' ends.  Text can be cut anywhere
        (output.ClusterSplitter takes the blocks as they are); members must end where a cluster's rows end, so under
        gzip_on the stream is told the ends and asked of every block where they fell in its members
        (output.ClusterMemberSplitter)."""
        from . import output
        ends = np.ascontiguousarray(self.target_cluster_ends(hb), dtype=np.uint64)
        if not gzip_on:
            splitter = output.ClusterSplitter(ends, hb.idx, sink)
            return splitter, splitter.close
        _lib.check(self.L.pf_kmers_tsv_stream_cuts(self.ctx, ends.ctypes.data if len(ends) else None, len(ends)))
        splitter = output.ClusterMemberSplitter(ends, hb.idx, sink)
        cut_text, cut_member = (np.zeros(max(len(ends), 1), dtype=np.uint64) for _ in range(2))
        t_off, t_n, n_cuts = C.c_uint64(), C.c_uint64(), C.c_uint64()

        def take(block):
            _lib.check(self.L.pf_kmers_tsv_stream_block_cuts(self.ctx, C.byref(t_off), C.byref(t_n), cut_text.ctypes.data,
                                                             cut_member.ctypes.data, len(cut_text), C.byref(n_cuts)))
            k = int(n_cuts.value)
            splitter(block.view, t_off.value, t_n.value, zip(cut_text[:k].tolist(), cut_member[:k].tolist()))
        return take, splitter.close

    def _render_targets(self, hb, metas, owned=False):
        """kmers.tsv rows of `metas` (packing.SeqMeta, in order) through pf_render_kmers_tsv: str, or the library's own
        block without a copy (owned: an OwnedText)"""
        t0 = time.time()
        buf, nb = C.c_void_p(), C.c_uint64()
        sso = hb.seg_strand_off.ctypes.data_as(C.c_void_p) if hb.n_strand_words else None
        with self._target_records(hb, metas) as (arr, n):
            t1 = time.time()
            _lib.check(self.L.pf_render_kmers_tsv(self.ctx, arr, n, sso, C.byref(buf), C.byref(nb)))
        t2 = time.time()
        if owned:
            self.render_targets_timing = {"marshal_s": t1 - t0, "render_s": t2 - t1, "copy_s": 0.0}
            return OwnedText(self.L, buf, nb.value)
        text = _take(buf, nb.value)
        self.L.pf_free_text(buf)
        # where the time of the last call went: Python marshalling of the records, the library's renderer, the copy out
        self.render_targets_timing = {"marshal_s": t1 - t0, "render_s": t2 - t1, "copy_s": time.time() - t2}
        return text.decode()

    _TS = np.dtype([("cluster", "u8"), ("strain", "u8"), ("id", "u8"), ("chromosome", "u8"), ("sequence", "u8"),
                    ("compsequence", "u8"), ("len", "u4"), ("strand", "i4"), ("start", "i8"), ("end", "i8"),
                    ("offset", "i8"), ("n_segs", "u4"), ("n_ambig", "u4"), ("seg_index", "u8"), ("seg_start", "u8"),
                    ("seg_nwin", "u8"), ("ambig_pos", "u8"), ("ambig_used", "u8"), ("ambig_key", "u8")])

    @staticmethod
    def _target_columns(hb, metas):
        """What the pf_target_seq records of a batch are made of: the packer's flat arrays (t_so, t_si, t_ss, t_sn, t_ao,
        t_ap, t_au, the ambiguous windows' keys back to back) and, per sequence, (cluster indices, strain names,
        Seqinfos).  metas=None: every target sequence of `hb`, straight from packing.TargetTable where the records behind
        it are still there -- no per-sequence Python objects; else from the SeqMeta objects, flattened."""
        tt = hb.target_table
        if metas is None and tt is not None and tt.resolve is not None and hb._targets is None:
            return (tt.t_so, tt.t_si, tt.t_ss, tt.t_sn, tt.t_ao, tt.t_ap, tt.t_au, bytes(tt.akeys)), tt.resolve(tt.t_seq)
        metas = hb.targets if metas is None else metas
        who = (np.fromiter((m.cluster for m in metas), dtype=np.int64, count=len(metas)), [m.strain for m in metas],
               [m.seq for m in metas])
        # ACGT runs: (segment index, first window, windows) per run, flat
        t_so = np.concatenate(([0], np.cumsum([len(m.segs) for m in metas], dtype=np.int64)))
        runs = np.array([x for m in metas for t in m.segs for x in t], dtype=np.uint32).reshape(-1, 3)
        # windows with a non-ACGT letter (rare): position, strand used and text, as the packer worked them out
        t_ao = np.concatenate(([0], np.cumsum([len(m.ambig) for m in metas], dtype=np.int64)))
        amb = [(q, m.ambig[q]) for m in metas if m.ambig for q in sorted(m.ambig)]
        t_ap = np.array([q for q, _ in amb], dtype=np.uint32)
        t_au = np.array([a[1] for _, a in amb], dtype=np.int8)
        akeys = "".join(a[0] for _, a in amb).encode("latin-1")
        if len(akeys) != hb.k * len(amb):
            raise ValueError("an ambiguous window's text is not k letters long")
        return (t_so, runs[:, 0], runs[:, 1], runs[:, 2], t_ao, t_ap, t_au, akeys), who

    @contextlib.contextmanager
    def _target_records(self, hb, metas=None):
        """`with` this: (pf_target_seq array, n) of the target sequences of `hb` -- all of them, or `metas`
        (packing.SeqMeta, in order).  The records, and the strings and arrays they point into, live as long as the
        block; the references `_seqinfo_columns` holds on the sequences' str objects go back when it ends, error or not."""
        # The C structs are filled column by column (numpy) instead of sequence by sequence (ctypes): every kind of
        # string goes into ONE NUL-separated block whose pieces are addressed by offset, the few per-sequence lists
        # (ACGT runs, non-ACGT windows) into flat arrays.  23 -> ~4 us per target sequence.
        TS = self._TS
        assert TS.itemsize == C.sizeof(_lib.TargetSeq)
        n = len(metas) if metas is not None else hb.n_targets
        rec = np.zeros(max(n, 1), dtype=TS)
        arr = C.cast(rec.ctypes.data, C.POINTER(_lib.TargetSeq))
        self._target_clusters = np.zeros(0, dtype=np.int64)     # the sequences' cluster indices (target_cluster_ends)
        if not n:
            yield arr, 0
            return
        keep = []

        def block(strings):
            """(addresses, lengths) of `strings` laid out NUL-terminated in one bytes object"""
            blob = ("\0".join(strings) + "\0").encode()
            ends = np.flatnonzero(np.frombuffer(blob, dtype=np.uint8) == 0)
            if len(ends) != len(strings):
                raise ValueError("a NUL byte inside a name or sequence")
            starts = np.concatenate(([0], ends[:-1] + 1)).astype(np.uint64)
            keep.append(blob)
            base = C.cast(C.c_char_p(blob), C.c_void_p).value
            return starts + np.uint64(base), (ends - starts.astype(np.int64)).astype(np.uint32)

        (t_so, t_si, t_ss, t_sn, t_ao, t_ap, t_au, akeys), (ci, strains, seqs) = self._target_columns(hb, metas)
        rec["cluster"] = block(list(hb.idx))[0][ci]
        self._target_clusters = np.asarray(ci, dtype=np.int64)
        # names repeat (a strain, a contig): one copy each
        for field, values in (("strain", [str(x) for x in strains]), ("id", [str(s.id) for s in seqs]),
                              ("chromosome", [str(s.chromosome) for s in seqs])):
            uniq = {}
            idx = np.fromiter((uniq.setdefault(v, len(uniq)) for v in values), dtype=np.int64, count=n)
            rec[field] = block(list(uniq))[0][idx]
        rec["strand"] = np.fromiter((int(s.strand) for s in seqs), dtype=np.int32, count=n)
        rec["start"] = np.fromiter((int(s.start) for s in seqs), dtype=np.int64, count=n)
        rec["end"] = np.fromiter((int(s.end) for s in seqs), dtype=np.int64, count=n)
        rec["offset"] = np.fromiter((int(s.offset) for s in seqs), dtype=np.int64, count=n)
        so, ao = np.asarray(t_so).astype(np.uint64), np.asarray(t_ao).astype(np.uint64)
        cols = [np.ascontiguousarray(x, dtype=np.uint32) if len(x) else np.zeros(1, np.uint32) for x in (t_si, t_ss, t_sn)]
        rec["n_segs"] = np.diff(so.astype(np.int64))
        for field, col in zip(("seg_index", "seg_start", "seg_nwin"), cols):
            rec[field] = np.uint64(col.ctypes.data) + so[:-1] * np.uint64(4)
        rec["n_ambig"] = np.diff(ao.astype(np.int64))
        ap = np.ascontiguousarray(t_ap, dtype=np.uint32) if len(t_ap) else np.zeros(1, np.uint32)
        au = np.ascontiguousarray(t_au, dtype=np.int8) if len(t_au) else np.zeros(1, np.int8)
        akeys += b"\0"
        # (the library copies k bytes from each key's address, pf_render_kmers_tsv: no terminator between the keys)
        kaddr = np.ascontiguousarray(np.uint64(C.cast(C.c_char_p(akeys), C.c_void_p).value) +
                                     np.arange(max(len(t_ap), 1), dtype=np.uint64) * np.uint64(hb.k))
        keep += cols + [ap, au, akeys, kaddr]
        rec["ambig_pos"] = np.uint64(ap.ctypes.data) + ao[:-1] * np.uint64(4)
        rec["ambig_used"] = np.uint64(au.ctypes.data) + ao[:-1]
        rec["ambig_key"] = np.uint64(kaddr.ctypes.data) + ao[:-1] * np.uint64(8)
        # the sequences last: from here to the end of the block the str objects are held by reference
        fast = _seqinfo_columns(seqs)
        if fast is None:
            held = None
            rec["sequence"], rec["len"] = block([s.sequence for s in seqs])
            rec["compsequence"], lens2 = block([s.compsequence for s in seqs])
            if not np.array_equal(rec["len"], lens2):
                raise ValueError("sequence and compsequence of different lengths")
        else:
            rec["sequence"], rec["compsequence"], rec["len"], held = fast
        try:
            yield arr, n
        finally:
            if held is not None:
                _release_held(held)
