"""Host pipeline of a whole run: files on disk -> the three output files.

Stands where the reference's reader / worker / writer processes do (/root/reference/panfeed/__main__.py:39-81 and the
serial loop :350-356): the native reader hands out table rows (host threads), the next batch is packed while the GPU
works on the current one (`Engine.run_batches`), the texts of a finished batch are written -- and, under `compress`,
deflated on all host threads -- by a writer thread while the GPU has the next batch.  Output order is the table order
(the reference's --cores 1 order) whatever finishes first."""
import csv
import functools
import os
import queue
import threading
import time

from . import _lib
from .engine import Engine, add_batch_stats, gzip_modes
from .native_input import Pangenome
from .output import (ClusterKmersFiles, create_hash_files, create_kmer_stroi, write_cluster_dirs, write_strain_headers,
                     write_text)


# ---------------------------------------------------------------------- the start-up both file pipelines share
def _peek_n_strains(presence_absence):
    """strain columns of the panaroo table, from its header record alone (input.py:188-191: index_col=0, the columns
    'Non-unique Gene name' and 'Annotation' dropped); 0 when the file cannot be read that way"""
    try:
        with open(presence_absence, newline="") as fh:
            header = next(csv.reader(fh))
        return sum(1 for h in header[1:] if h not in ("Non-unique Gene name", "Annotation"))
    except Exception:       # noqa: BLE001
        return 0


def existing_output_error(output):
    """the reference refuses an existing directory (input.py:213-216): the error to raise, or None"""
    if os.path.isdir(output):
        return FileExistsError(f"Output directory {output} already exists; remove it or change the output path")
    return None


def sized_engine(n_strains, batch_clusters, max_items=0, **options):
    """The context of a files -> files run, sized for that run; `options`: Engine's other keyword arguments."""
    return Engine(max_strains=max(32, (n_strains + 31) // 32 * 32),
                  # work items in flight = scratch slices (1.9 MB each at 1 000 strains): sized for the batches of this
                  # run, not the library's default of 2 048 -- creating and freeing 4 GB of scratch was a third of a
                  # one-second run's time (a cluster that needs more makes the library re-make its scratch)
                  max_items=max_items or max(512, 2 * int(batch_clusters)), **options)


def settle_context(pg, eng, open_reader):
    """`(pg, eng)` once the reader knows the number of strains: a context made from the table's header line (`eng`, or
    None) that turns out too small is closed -- the header was not what the reader made of it -- and a reader whose
    genomes went into that context's store is opened again the classic two-step way (`open_reader(engine=None)`).
    Where `eng` comes back None the caller makes the context from `pg.n_strains`."""
    if eng is None or eng.max_strains >= pg.n_strains:
        return pg, eng
    if pg.resident:
        pg.close()
        pg = None
    eng.close()
    return pg or open_reader(engine=None), None


# ---------------------------------------------------------------------- one run_files call
class _FileRun:
    """What the steps of one `run_files` call share."""

    def __init__(self, output, compress, multiple_files, device_gzip=False, device_gzip_clusters=False, bgzf=False):
        self.output, self.multiple_files, self.bgzf = output, multiple_files, bool(bgzf)
        # (per-cluster files keep the host's gzip under device_gzip: they have a switch of their own)
        self.compress, self.device_gzip, self.device_gzip_clusters = gzip_modes(compress, device_gzip, multiple_files,
                                                                                device_gzip_clusters)
        self.host_member_bytes = 0                      # per-cluster files: the members the writer thread compressed behind the headers
        self.t_start = time.perf_counter()
        # where the wall time went: opening + parsing the inputs, creating the context, uploading the genomes, then the
        # overlapped stages of the batches (Engine.run_batches: read + pack on its thread, pf_submit = upload + kernels,
        # text = device text + D2H or fetch + host renderers) and the writer thread's busy time
        self.stages = {"open_parse_s": 0.0, "write_busy_s": 0.0}
        self.context_thread = None                      # "panfeed-context": what it made (or its error), in how long
        self.context, self.context_err, self.context_s = None, None, 0.0
        self.uploader, self.upload_err = None, None     # "panfeed-genomes" and its error
        self.write_err = None                           # the first failure of "panfeed-writer"
        self.strains = ()
        self.kmer_stroi = self.kmer_hash = self.hash_pat = None     # the run's three files (not under multiple_files)

    def start_context(self, make_engine, n_strains):
        """the context (stream, tables, ~1 GB of scratch: 7 ms) is made on a thread of its own while the reader opens
        the pangenome; it needs the number of strains, which the table's header line says"""
        def make():
            t0 = time.perf_counter()
            try:
                self.context = make_engine(n_strains)
            except Exception as e:       # noqa: BLE001  (made again in _open, where the error belongs)
                self.context_err = e
            self.context_s = time.perf_counter() - t0
        self.context_thread = threading.Thread(target=make, name="panfeed-context")
        self.context_thread.start()

    def join_context(self):
        """the early context, or None when there is none (not started, or it could not be made)"""
        if self.context_thread is not None:
            self.context_thread.join()
        return self.context

    def context_when_needed(self):
        """for the one-pass reader, which asks when the first genome needs the context"""
        if self.join_context() is None:
            raise self.context_err
        return self.context

    def wait_for_genomes(self):
        if self.uploader is not None:
            self.uploader.join()
        if self.upload_err is not None:
            raise self.upload_err

    def write_one(self, o):
        if not self.multiple_files:
            write_text(self.kmer_stroi, o.kmers_tsv)
            write_text(self.kmer_hash, o.kmers_to_hashes)
            write_text(self.hash_pat, o.hashes_to_patterns)
            return
        self.host_member_bytes += write_cluster_dirs(self.output, self.strains, o, self.compress, self.device_gzip_clusters)

    def writer(self, q, slots):
        while True:
            o = q.get()
            if o is None:
                return
            try:
                if self.write_err is None:
                    tw = time.perf_counter()
                    self.write_one(o)
                    self.stages["write_busy_s"] += time.perf_counter() - tw
            except Exception as e:          # keep draining so that the producer never blocks on a dead writer
                self.write_err = e
            finally:
                slots.release()


def _open(run, open_reader, make_engine, n_peek, one_pass):
    """Reader and context, `(pg, eng)`.  With the strain count of the header line (`n_peek`) the context is made on its
    thread meanwhile; one_pass: one pass over the input -- the genomes go into the context's store as their files are
    read, the reader asking for the context when the first genome needs it."""
    if n_peek:
        run.start_context(make_engine, n_peek)
    pg = eng = None
    try:
        pg = open_reader(engine=run.context_when_needed if n_peek and one_pass else None)
        run.stages["open_parse_s"] = time.perf_counter() - run.t_start
        t0 = time.perf_counter()
        pg, eng = settle_context(pg, run.join_context(), open_reader)
        early = eng is not None
        if not early:
            eng = make_engine(pg.n_strains)
        run.stages["context_s"] = run.context_s if early else time.perf_counter() - t0
        run.stages["context_wait_s"] = time.perf_counter() - t0
        return pg, eng
    except BaseException:
        for x in (pg, run.join_context(), eng):
            if x is not None:
                x.close()
        raise


def _start_upload(run, pg, eng, resident, overlap):
    """The genomes of a reader that was opened the two-step way go to the GPU: at once, or on a thread of their own."""
    run.stages["genome_upload_s"] = 0.0
    run.stages["one_pass_ingest"] = bool(pg.one_pass)
    if not resident or pg.resident:
        return
    t0 = time.perf_counter()
    if not overlap:
        pg.make_resident(eng)
        run.stages["genome_upload_s"] = time.perf_counter() - t0
        return
    # The genome store's layout follows from the contig lengths: the reader switches to by-reference records at
    # once and the packer thread starts on the first batches while the contigs go up on a thread of their own
    # (the library packs them to 2 bits per base on the device); the first pf_submit waits for that thread.
    pg.assign_store()

    def upload():
        t1 = time.perf_counter()
        try:
            pg.upload_store(eng)
        except Exception as e:       # noqa: BLE001
            run.upload_err = e
        run.stages["genome_upload_s"] = time.perf_counter() - t1
    run.uploader = threading.Thread(target=upload, name="panfeed-genomes")
    run.uploader.start()


def _open_outputs(run, strains):
    run.strains = list(strains)
    if not run.multiple_files:
        run.kmer_stroi = create_kmer_stroi(run.output, run.compress, run.device_gzip, run.bgzf)
        run.hash_pat, run.kmer_hash = create_hash_files(run.output, run.compress, run.device_gzip, run.bgzf)
        write_strain_headers(run.hash_pat, run.kmer_hash, run.strains)


def _write_batches(run, eng, pg, stats, batch_clusters, device_text):
    """The batches, in table order, through the writer thread; closes the run's files."""
    q = queue.Queue(maxsize=4)
    # text the GPU wrote lives in two pinned blocks used alternately: a batch may only be rendered once the batch
    # before the previous one has been written out
    slots = threading.Semaphore(2)
    wt = threading.Thread(target=run.writer, args=(q, slots), name="panfeed-writer")
    wt.start()
    try:
        # (target strains' rows go to kmers.tsv block by block as they leave the device, from this thread: the file is
        # the writer thread's only when a batch's rows come as one object -- the host renderers' path)
        # (under multiple_files each cluster's rows into its own directory's kmers.tsv, cut at the cluster ends)
        sink = cluster_sink = None
        if device_text and run.multiple_files:
            cluster_sink = ClusterKmersFiles(run.output, run.compress, run.device_gzip_clusters)
        elif device_text:
            sink = functools.partial(write_text, run.kmer_stroi)
        # what a batch adds to the run's counters: "bytes" its text; the clusters whose files are cut from text the GPU
        # wrote; under device gzip the members the GPU made of it, by the encoder's own count
        keys = (("clusters", "instances", "kept_kmers", "device_ms", "bytes") +
                (("device_cluster_files",) if run.multiple_files else ()) +
                (("compressed_bytes",) if run.device_gzip or run.device_gzip_clusters else ()) +
                (("kmers_rows_considered", "kmers_rows_kept") if eng.passing is not None else ()))
        if eng.passing is not None:
            stats.update(kmers_rows_considered=0, kmers_rows_kept=0, passing_digests=len(eng.passing))
        batches = eng.run_pangenome(pg, batch_clusters=batch_clusters, device_text=device_text,
                                    before_first_submit=run.wait_for_genomes, targets_sink=sink,
                                    cluster_targets_sink=cluster_sink)
        while True:
            slots.acquire()
            try:
                o = next(batches, None)
            finally:
                if cluster_sink is not None:
                    cluster_sink.close()        # the batch's last kmers.tsv
            if o is None:
                break
            add_batch_stats(stats, o, keys)
            stats["patterns"] = o.stats.get("patterns", stats["patterns"])
            q.put(o)
    finally:
        q.put(None)
        wt.join()
        for fh in (run.kmer_stroi, run.kmer_hash, run.hash_pat):
            if fh is not None:
                fh.close()
                if run.device_gzip:             # and the members the host compressed behind the header (fallback batches)
                    stats["compressed_bytes"] = stats.get("compressed_bytes", 0) + fh.host_bytes
        if run.device_gzip_clusters:            # the same for the per-cluster files: what their two writers compressed
            stats["compressed_bytes"] = (stats.get("compressed_bytes", 0) + run.host_member_bytes +
                                         (cluster_sink.host_bytes if cluster_sink is not None else 0))
    if run.write_err is not None:
        raise run.write_err


def run_files(presence_absence, gffdir, output, fastadir=None, klength=31, canon=True, consider_missing=False,
              patfilt=True, maf=0.01, upstream=0, downstream=0, downstream_start_codon=False, targets=(), genes=None,
              compress=False, multiple_files=False, batch_clusters=256, resident=True, device_text=True, device=0,
              max_items=0, pattern_capacity=0, overlap=True, one_pass=True, raise_missing=False, device_gzip=False,
              targets_text_budget=None, device_gzip_clusters=False, bgzf=False, passing_hashes=None, device_gzip_level=1):
    """One directory of outputs (`kmers.tsv`, `kmers_to_hashes.tsv`, `hashes_to_patterns.tsv`, `.gz` under
    `compress`; under `multiple_files` one such directory per gene cluster, `<output>/<cluster>/`, the pattern set
    starting empty in each: `panfeed.py:35-43,153-167`) from a panaroo table and a directory (or file of files) of GFFs.  Option names and meaning follow
    the reference's (`__main__.py:86-186`); `patfilt` is what `pattern_hasher` receives (`--no-filter` inverted,
    `__main__.py:283-297`).  one_pass (with resident): the genomes go to the GPU as their files are read
    (pf_pangenome_open_device) instead of being read into host strings first and uploaded afterwards.  raise_missing
    (`--stop-on-missing`): a strain, contig or gene of the table that is not found is an error instead of a warning.
    device_gzip (`--gpu-compress`): the `.gz` files are compressed on the GPU -- it implies `compress`; the text the GPU
    writes leaves it as gzip members (larger files than `compress` writes, in less time -- profiles/gzip_device/ -- that read back as
    the same text), `stats["bytes"]` keeps counting text and `stats["compressed_bytes"]` is what the files hold behind their
    header members: the encoder's own count of every batch's members plus the members the host compressed.  Under `multiple_files` it changes nothing: the per-cluster files are cut from text the GPU wrote (device_text) and keep the host's gzip.
    device_gzip_clusters (`--gpu-compress-clusters`): the per-cluster files of `multiple_files` compressed on the GPU -- it
    implies `compress` and changes nothing without `multiple_files`; every cluster's bodies leave the GPU as gzip members
    that end where the cluster's rows end and are appended behind the header line's member as they are;
    `stats["compressed_bytes"]` as above.
    bgzf (`--bgzf`, with device_gzip, not for multiple_files: ValueError): the three files are BGZF -- the GPU's members
    leave it as BGZF members, host text is written in BGZF members of at most 65 280 bytes, every file ends with the
    end-of-file member; htslib's readers take them, and so does the device gunzip route of the downstream tools.
    device_gzip_level (`--gpu-compress-level`; 1 or 2, else ValueError): the effort of the GPU's encoder wherever
    device_gzip or device_gzip_clusters has it compress, BGZF included -- 2 (PF_GZ_DEEP) also tries the same column of the
    row before and parses lazily: smaller files, hashes_to_patterns.tsv most of all, for more encoder time
    (profiles/gzip_deep/).  Without either switch it changes nothing.
    targets_text_budget: device memory a batch's kmers.tsv text may take (default: the engine's).
    passing_hashes (`--passing-hashes` / `--passing-associations`; None: off): an iterable of `hashed_pattern` strings or
    16-byte digests -- kmers.tsv holds only the rows whose (cluster, k-mer) kmers_to_hashes.tsv lists with one of them,
    decided on the GPU before a dropped row is written; the other two files are not affected.  `stats` gains
    `kmers_rows_considered`, `kmers_rows_kept` and `passing_digests`.
    Returns a dict of counters."""
    run = _FileRun(output, compress, multiple_files, device_gzip, device_gzip_clusters, bgzf)
    if run.bgzf and not run.device_gzip:
        raise ValueError("bgzf is for device_gzip without multiple_files")
    gzip_flags = _lib.gzip_level_flags(device_gzip_level)
    err = existing_output_error(output)
    if err is not None:
        raise err
    os.makedirs(output)
    targets = tuple(targets or ())
    make_engine = functools.partial(sized_engine, batch_clusters=batch_clusters, max_items=max_items, klength=klength,
                                    canon=canon, consider_missing=consider_missing, patfilt=patfilt, maf=maf,
                                    multiple_files=multiple_files, stroi=set(targets), device=device,
                                    pattern_capacity=pattern_capacity, device_gzip=run.device_gzip,
                                    device_gzip_clusters=run.device_gzip_clusters, bgzf=run.bgzf,
                                    device_gzip_flags=gzip_flags,
                                    **({} if passing_hashes is None else {"passing_hashes": list(passing_hashes)}),
                                    **({} if targets_text_budget is None else {"targets_text_budget": targets_text_budget}))
    open_reader = functools.partial(Pangenome, presence_absence, gffdir, fastadir, upstream, downstream,
                                    downstream_start_codon, targets=targets, genes=genes, raise_missing=raise_missing)
    n_peek = _peek_n_strains(presence_absence) if overlap else 0
    _lib.load()        # once, on this thread, before two threads could both make the process's first call to it
    pg, eng = _open(run, open_reader, make_engine, n_peek, one_pass=resident and one_pass)
    stats = {"clusters": 0, "instances": 0, "kept_kmers": 0, "patterns": 0, "device_ms": 0.0, "bytes": 0}
    try:
        _start_upload(run, pg, eng, resident, overlap)
        _open_outputs(run, pg.strains)
        _write_batches(run, eng, pg, stats, batch_clusters, device_text)
        run.wait_for_genomes()  # a run that submitted nothing (empty table, --genes matching nothing) still reports a failed upload
        stats["log"] = pg.take_log()
        run.stages.update(getattr(eng, "stages", {}))
        run.stages["total_s"] = time.perf_counter() - run.t_start
        stats["stages"] = run.stages
        return stats
    finally:
        if run.uploader is not None:
            run.uploader.join()              # (an error on the way: the upload reads the reader's contigs)
        t0 = time.perf_counter()
        pg.close(wait=False)                 # the run is over: the reader's memory goes back in the background
        t1 = time.perf_counter()
        eng.close()
        if "stages" in stats:                                             # reader and context given back
            stats["stages"]["close_reader_s"] = t1 - t0
            stats["stages"]["close_context_s"] = time.perf_counter() - t1
