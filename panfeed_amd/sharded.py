"""A whole run on N GPUs (one process per GPU) whose files equal the single-GPU / `--cores 1` files byte for byte.

What the reference does with one writer process (/root/reference/panfeed/__main__.py:67-81: `pattern_hasher` owns the
run-global `patterns` set and the three file handles, panfeed.py:146-150, 179-187, 210-226) is split like this:

* rank r processes the contiguous range `shard_range(...)` of the processing order with the GLOBAL cluster ordinals
  (`Engine.next_ordinal` = start of its range), so `first_seen = ordinal << 32 | rank inside the cluster` is unique
  over the run and monotone in the `--cores 1` order;
* `kmers_to_hashes.tsv` / `kmers.tsv` bodies: per rank, as the batches finish -> `<file>.part<r>`; the `kmers.tsv` rows
  block by block as they leave the device (`targets_sink`: a batch's rows never stand in one buffer);
* `hashes_to_patterns.tsv`: nothing is written while the shard runs (`defer_patterns`); at the end the ranks exchange
  {md5, first_seen} (`distributed.merge_pattern_tensors`: RCCL on the GPUs, gloo in rehearsals), every rank keeps the
  patterns whose `first_seen` is the run-wide minimum of their digest, sorts them by `first_seen` and renders those rows
  (`pf_pattern_rows_stream_begin/_next`: slice by slice) -> `hashes_to_patterns.tsv.part<r>`.  All `first_seen` of
  rank r precede all of rank
  r + 1, so the parts concatenated in rank order are the reference's first-seen order;
* rank 0 writes header + parts in rank order into the final files (`assemble`).  Under `compress` every part is a
  sequence of gzip members and so is the concatenation; under `device_gzip` the members are the GPU's, or small ones
  made on the host, and the file is one the device decoder takes.
* `--multiple-files`: the pattern set restarts in every cluster (panfeed.py:165): no exchange at all, every rank writes
  its clusters' directories, cut from its batches' device text like a single-GPU run's.

`PatternSource` is the little a rank needs from its engine after the shard has run; `Engine` provides it, and the CPU
tests drive the same merge / assembly code with a stand-in.
"""
import functools
import os
import shutil

import numpy as np

from .engine import (KMERS_TO_HASHES_HEADER, KMERS_TSV_HEADER, add_batch_stats, gzip_modes, hashes_to_patterns_header,
                     text_len)
from .output import ClusterKmersFiles, ParallelGzipWriter, SmallMemberGzipWriter, write_cluster_dirs, write_text

FILES = ("kmers.tsv", "kmers_to_hashes.tsv", "hashes_to_patterns.tsv")


def _part_path(output, name, rank, compress):
    return os.path.join(output, ".parts", f"{name}{'.gz' if compress else ''}.part{rank:04d}")


class ShardWriter:
    """The part files of one rank (bodies only; headers are rank 0's business in `assemble`).  device_gzip: a part takes
    the GPU's gzip members as they are (a GzipMembers); text made on the host -- a batch that fell back to the host
    renderers, rows of a source without a stream -- goes in as members of at most pf_gzip_device_chunk_bytes() of text,
    so that every member of the assembled file is one the device decoder takes."""

    def __init__(self, output, rank, compress=False, device_gzip=False):
        compress = bool(compress or device_gzip)
        self.output, self.rank, self.compress, self.device_gzip = output, rank, compress, bool(device_gzip)
        os.makedirs(os.path.join(output, ".parts"), exist_ok=True)
        self.handles = {}
        for name in FILES:
            path = _part_path(output, name, rank, compress)
            if device_gzip:
                from . import _lib
                self.handles[name] = SmallMemberGzipWriter(path, _lib.load().pf_gzip_device_chunk_bytes(), compresslevel=9,
                                                           part=True)
            elif compress:
                h = ParallelGzipWriter(path, compresslevel=9)
                h.wrote = True            # an empty part adds nothing (no empty gzip member in the middle of the file)
                self.handles[name] = h
            else:
                self.handles[name] = open(path, "wb")
        self.bytes = 0

    def write_batch(self, kmers_tsv, kmers_to_hashes):
        write_text(self.handles["kmers.tsv"], kmers_tsv)
        write_text(self.handles["kmers_to_hashes.tsv"], kmers_to_hashes)
        self.bytes += text_len(kmers_tsv) + text_len(kmers_to_hashes)

    def write_patterns(self, blocks):
        for b in blocks:
            write_text(self.handles["hashes_to_patterns.tsv"], b)
            self.bytes += text_len(b)

    def sink(self, name):
        """what a stream hands its blocks to (Engine.run_batches' targets_sink, Engine.stream_pattern_rows): each block --
        text, or the GPU's members -- goes into the part of `name` as it comes.  A stream says how much text it was when
        it is over (members do not): the caller adds that to `bytes`."""
        fh = self.handles[name]
        return lambda block: write_text(fh, block)

    def close(self):
        for h in self.handles.values():
            h.close()


def kept_pattern_ids(md5, first_seen, dist=None, engine=None, device=None, method="owner"):
    """ids (into this rank's pool) of the patterns this rank has to write, in first-seen order, and the number of
    run-global patterns.  md5: uint8 [n,16], first_seen: uint64 [n] (numpy)."""
    import torch

    from .distributed import merge_pattern_tensors
    t_md5 = torch.from_numpy(np.ascontiguousarray(md5))
    t_fs = torch.from_numpy(np.ascontiguousarray(first_seen).view(np.int64))
    if device is not None and device.type == "cuda":
        t_md5, t_fs = t_md5.to(device), t_fs.to(device)
    keep, n_global = merge_pattern_tensors(t_md5, t_fs, dist, engine=engine if t_md5.is_cuda else None, method=method)
    keep = keep.cpu().numpy().astype(bool)
    ids = np.flatnonzero(keep)
    ids = ids[np.argsort(np.asarray(first_seen)[ids], kind="stable")]
    return ids.astype(np.uint32), int(n_global)


def check_first_seen_disjoint(first_seen, dist, device=None):
    """Ranks must not share cluster ordinals (every rank running with ordinals from 0 would make ties that keep a
    digest twice): the ordinal ranges [min, max] of the ranks have to be disjoint and ascending with the rank.
    `device`: this rank's GPU -- under RCCL the gathered tensors have to live on it (every rank on cuda:0 is a
    duplicate-GPU communicator error or a hang)."""
    if dist is None or not dist.is_initialized() or dist.get_world_size() == 1:
        return
    import torch
    fs = np.asarray(first_seen, dtype=np.uint64)
    lo = int(fs.min() >> np.uint64(32)) if len(fs) else -1
    hi = int(fs.max() >> np.uint64(32)) if len(fs) else -1
    mine = torch.tensor([lo, hi], dtype=torch.int64)
    allr = [torch.zeros(2, dtype=torch.int64) for _ in range(dist.get_world_size())]
    backend = dist.get_backend()
    if backend == "nccl":
        dev = device if device is not None and device.type == "cuda" else torch.device("cuda", torch.cuda.current_device())
        allr = [t.to(dev) for t in allr]
        mine = mine.to(dev)
    dist.all_gather(allr, mine)
    prev = -1
    for r, t in enumerate(allr):
        a, b = (int(x) for x in t.tolist())
        if a < 0:
            continue
        if a <= prev:
            raise RuntimeError(f"rank {r} holds cluster ordinals {a}..{b} overlapping an earlier rank's (<= {prev}): "
                               "every rank of a sharded run must number its clusters with the run's global ordinals")
        prev = b


def finish_shard(source, writer, dist=None, device=None, method="owner"):
    """After the shard's batches: exchange digests, write this rank's pattern rows.  `source`: export_patterns() and
    stream_pattern_rows(ids, sink) (an Engine: the rows leave the device slice by slice, the next one being written
    meanwhile) or, without that, render_pattern_rows(ids).  Returns (rows written by this rank, run-global pattern
    count)."""
    md5, fs = source.export_patterns()
    check_first_seen_disjoint(fs, dist, device)
    eng = source if hasattr(source, "ctx") else None
    ids, n_global = kept_pattern_ids(md5, fs, dist, engine=eng, device=device, method=method)
    if hasattr(source, "stream_pattern_rows"):
        writer.bytes += source.stream_pattern_rows(ids, writer.sink("hashes_to_patterns.tsv"))[0]
    else:
        writer.write_patterns(source.render_pattern_rows(ids))
    return len(ids), n_global


def assemble(output, world, strains, compress=False, keep_parts=False, device_gzip=False):
    """Rank 0, after every rank has closed its parts: header + parts in rank order -> the three files.  device_gzip: the
    header line is a member of its own with MTIME = 0, as output.MemberGzipWriter writes it: every member of the file then
    starts with the same eight bytes, which is how the device decoder finds them."""
    compress = bool(compress or device_gzip)
    headers = {"kmers.tsv": KMERS_TSV_HEADER, "kmers_to_hashes.tsv": KMERS_TO_HASHES_HEADER,
               "hashes_to_patterns.tsv": hashes_to_patterns_header(strains)}
    for name in FILES:
        final = os.path.join(output, name + (".gz" if compress else ""))
        with open(final, "wb") as out:
            if device_gzip:
                import gzip
                out.write(gzip.compress(headers[name].encode(), compresslevel=9, mtime=0))
            elif compress:
                import gzip
                out.write(gzip.compress(headers[name].encode(), compresslevel=9))
            else:
                out.write(headers[name].encode())
            for r in range(world):
                with open(_part_path(output, name, r, compress), "rb") as part:
                    shutil.copyfileobj(part, out, 16 << 20)
    if not keep_parts:
        shutil.rmtree(os.path.join(output, ".parts"), ignore_errors=True)


def _barrier(dist, device=None):
    if dist is not None and dist.is_initialized() and dist.get_world_size() > 1:
        if device is not None and device.type == "cuda" and dist.get_backend() == "nccl":
            dist.barrier(device_ids=[device.index if device.index is not None else 0])
        else:
            dist.barrier()


def _bind_device(device):
    """one process per GPU: collectives of this process run on `device` (RCCL picks torch's current device)"""
    if device is not None and device.type == "cuda":
        import torch
        torch.cuda.set_device(device)


def run_records_sharded(records, output, strains, rank, world, dist=None, device=None, klength=31, canon=True,
                        consider_missing=False, patfilt=True, maf=0.01, targets=(), compress=False,
                        multiple_files=False, batch_clusters=256, weights=None, method="owner", gpu=0,
                        max_items=0, pattern_capacity=0, dedup=True, device_gzip=False, targets_text_budget=None,
                        device_gzip_clusters=False, device_gzip_level=1):
    """One rank of a sharded run over in-memory reference-shaped records (the tuples input.py:468 yields; every rank
    is given the same list).  Returns a dict of counters; the files are complete once rank 0 returns.  device_gzip,
    device_gzip_clusters, device_gzip_level, targets_text_budget: as in `run_files_sharded`; where either is given the batches' texts are written on the device
    (the members and the ranges are the device's), else by the host renderers as before."""
    from . import _lib
    from .distributed import shard_range
    from .engine import Engine
    _bind_device(device)
    records = list(records)
    start, stop = shard_range(len(records), rank, world, weights)
    max_strains = max([len(strains)] + [max(len(r[0]), len(r[2])) for r in records] + [1])
    compress, device_gzip, device_gzip_clusters = gzip_modes(compress, device_gzip, multiple_files, device_gzip_clusters)
    eng = Engine(klength=klength, canon=canon, consider_missing=consider_missing, patfilt=patfilt, maf=maf,
                 multiple_files=multiple_files, max_strains=(max_strains + 31) // 32 * 32, stroi=set(targets) if targets else (),
                 device=gpu, max_items=max_items, pattern_capacity=pattern_capacity, dedup=dedup, device_gzip=device_gzip,
                 device_gzip_clusters=device_gzip_clusters, device_gzip_flags=_lib.gzip_level_flags(device_gzip_level),
                 **_budget(targets_text_budget))
    try:
        eng.next_ordinal = start                          # global ordinals: first_seen is unique over the run
        batches = functools.partial(eng.run_stream, records[start:stop], batch_clusters=batch_clusters,
                                    defer_patterns=not multiple_files,
                                    device_text=device_gzip or device_gzip_clusters or targets_text_budget is not None)
        return _drive(eng, batches, output, strains, rank, world, dist, device, compress, multiple_files, method,
                      (start, stop), device_gzip, device_gzip_clusters)
    finally:
        eng.close()


def run_files_sharded(presence_absence, gffdir, output, rank, world, dist=None, device=None, fastadir=None, klength=31,
                      canon=True, consider_missing=False, patfilt=True, maf=0.01, upstream=0, downstream=0,
                      downstream_start_codon=False, targets=(), genes=None, compress=False, multiple_files=False,
                      batch_clusters=256, resident=True, device_text=True, method="owner", gpu=0, max_items=0,
                      pattern_capacity=0, device_gzip=False, raise_missing=False, targets_text_budget=None,
                      device_gzip_clusters=False, device_gzip_level=1):
    """`pipeline.run_files` on N GPUs: every rank opens the pangenome, takes its range of the processing order
    (balanced by the number of gene entries per table row) and writes its parts; rank 0 assembles.  Option names as
    in the reference's CLI (`__main__.py:86-186`).
    device_gzip (`--gpu-compress`): implies `compress`; the text a rank's GPU writes leaves it as gzip members, and the
    assembled files are ones the device decoder takes (under `multiple_files` the host's gzip stays, as on one GPU).
    device_gzip_clusters (`--gpu-compress-clusters`): with `multiple_files`, the per-cluster files compressed on each
    rank's GPU, as in `pipeline.run_files`; implies `compress`.
    device_gzip_level (`--gpu-compress-level`; 1 or 2, else ValueError): the effort of every rank's encoder, as in
    `pipeline.run_files`.
    raise_missing (`--stop-on-missing`): the reader's; a rank that fails in its shard makes every rank fail before the
    pattern exchange, `.parts/` is removed, and so is the output directory where that leaves it empty (under
    `multiple_files` the clusters written until then stay, and the directory with them).  targets_text_budget: device memory a batch's kmers.tsv text may take (default: the engine's) --
    the rows go into the rank's part range by range as they leave the device, never as one text."""
    from .distributed import shard_range
    from .native_input import Pangenome
    from . import _lib
    from .pipeline import _peek_n_strains, existing_output_error, settle_context, sized_engine
    _bind_device(device)
    targets = tuple(targets or ())
    compress, device_gzip, device_gzip_clusters = gzip_modes(compress, device_gzip, multiple_files, device_gzip_clusters)
    gzip_flags = _lib.gzip_level_flags(device_gzip_level)
    err = existing_output_error(output)
    _barrier(dist, device)                                        # every rank has looked before rank 0 creates it
    if err is not None:
        raise err
    if rank == 0:
        os.makedirs(output)
    _barrier(dist, device)
    make_engine = functools.partial(sized_engine, batch_clusters=batch_clusters, max_items=max_items, klength=klength,
                                    canon=canon, consider_missing=consider_missing, patfilt=patfilt, maf=maf,
                                    multiple_files=multiple_files, stroi=set(targets), device=gpu,
                                    pattern_capacity=pattern_capacity, device_gzip=device_gzip,
                                    device_gzip_clusters=device_gzip_clusters, device_gzip_flags=gzip_flags,
                                    **_budget(targets_text_budget))
    open_reader = functools.partial(Pangenome, presence_absence, gffdir, fastadir, upstream, downstream,
                                    downstream_start_codon, targets=targets, genes=genes, raise_missing=raise_missing)
    # every rank reads every genome (a cluster's sequences come from all of them): with resident genomes the files go to
    # the rank's GPU as they are read (pf_pangenome_open_device), as in pipeline.run_files; the context is made first, on
    # this thread, from the table's header line
    n_peek = _peek_n_strains(presence_absence) if resident else 0
    eng = make_engine(n_peek) if n_peek else None
    try:
        pg = open_reader(engine=eng)
    except BaseException:
        if eng is not None:
            eng.close()
        raise
    pg, eng = settle_context(pg, eng, open_reader)
    try:
        w = pg.weights()
        start, stop = shard_range(len(w), rank, world, w)
        pg.set_range(start, stop - start)
        if eng is None:
            eng = make_engine(pg.n_strains)
        if resident and not pg.resident:
            pg.make_resident(eng)
        eng.next_ordinal = start
        batches = functools.partial(eng.run_pangenome, pg, batch_clusters=batch_clusters, device_text=device_text,
                                    defer_patterns=not multiple_files)
        try:
            stats = _drive(eng, batches, output, pg.strains, rank, world, dist, device, compress, multiple_files, method,
                           (start, stop), device_gzip, device_gzip_clusters)
        except Exception:
            if rank == 0:                                 # (made above: it goes again where the failed run left it empty,
                try:                                      # so that the command can be run again)
                    os.rmdir(output)
                except OSError:
                    pass
            raise
        stats["log"] = pg.take_log()
        return stats
    finally:
        pg.close()
        if eng is not None:
            eng.close()


def _budget(targets_text_budget):
    return {} if targets_text_budget is None else {"targets_text_budget": int(targets_text_budget)}


def _all_ok(ok, dist, device=None):
    """whether every rank says ok (one small all-reduce): a rank whose shard failed must not leave the others waiting in
    the pattern exchange"""
    if dist is None or not dist.is_initialized() or dist.get_world_size() == 1:
        return ok
    import torch
    t = torch.tensor([1 if ok else 0], dtype=torch.int64)
    if dist.get_backend() == "nccl":
        t = t.to(device if device is not None and device.type == "cuda" else torch.device("cuda", torch.cuda.current_device()))
    dist.all_reduce(t, op=dist.ReduceOp.MIN)
    return bool(int(t.item()))


def _shard_batches(batches, each, dist, device, after_failure=None):
    """`each(o)` for every BatchOutput of this rank's shard; then the ranks agree (`_all_ok`).  Where some rank's shard
    failed every rank raises -- that rank its own error, the others a RuntimeError -- after `after_failure()`, which
    every rank runs (it may use collectives)."""
    failure = None
    try:
        for o in batches:
            each(o)
    except Exception as e:                                # noqa: BLE001  (raised again below, once every rank knows)
        failure = e
    if _all_ok(failure is None, dist, device):
        return
    if after_failure is not None:
        after_failure()
    raise failure if failure is not None else RuntimeError("another rank of this run failed in its shard")


def _drive(eng, make_batches, output, strains, rank, world, dist, device, compress, multiple_files, method, rng,
           device_gzip=False, device_gzip_clusters=False):
    """`make_batches(targets_sink=...)`: the engine's generator of BatchOutput over this rank's range.  A run in which a
    rank's shard failed assembles nothing and leaves no `.parts/` behind; under `multiple_files` the directories of the
    clusters written until then stay."""
    stats = {"rank": rank, "clusters": 0, "instances": 0, "kept_kmers": 0, "range": list(rng), "device_ms": 0.0}
    if multiple_files:
        # a cluster's kmers.tsv rows go into its directory as they leave the device, its other two files when the batch
        # is handed over (slices of the device text, or the host renderers' strings)
        kmers_files = ClusterKmersFiles(output, compress, device_gzip_clusters)
        if device_gzip_clusters:
            stats["compressed_bytes"] = 0     # the GPU's members by the encoder's count, and the host's behind the headers

        def each(o):
            kmers_files.close()
            host = write_cluster_dirs(output, list(strains), o, compress, device_gzip_clusters)
            add_batch_stats(stats, o, ("clusters", "instances"))
            if device_gzip_clusters:
                stats["compressed_bytes"] += o.stats.get("compressed_bytes", 0) + host
        try:
            _shard_batches(make_batches(cluster_targets_sink=kmers_files), each, dist, device)
        finally:
            kmers_files.close()
        if device_gzip_clusters:
            stats["compressed_bytes"] += kmers_files.host_bytes
        _barrier(dist, device)
        return stats
    stats.update(kmers_tsv_streamed=0, kmers_tsv_ranges=0, kmers_tsv_peak_device_bytes=0, bytes=0)
    writer = ShardWriter(output, rank, compress, device_gzip)
    kmers_tsv, kmers_to_hashes = writer.sink("kmers.tsv"), writer.sink("kmers_to_hashes.tsv")

    def each(o):
        kmers_tsv(o.kmers_tsv)                            # (what a sink takes is counted by the batch: "bytes")
        kmers_to_hashes(o.kmers_to_hashes)
        add_batch_stats(stats, o, ("clusters", "instances", "kept_kmers", "device_ms", "kmers_tsv_streamed",
                                   "kmers_tsv_ranges", "bytes"))
        stats["kmers_tsv_peak_device_bytes"] = max(stats["kmers_tsv_peak_device_bytes"],
                                                   o.stats.get("kmers_tsv_peak_device_bytes", 0))

    def drop_parts():
        writer.close()
        _barrier(dist, device)                            # every rank has closed its parts
        if rank == 0:
            shutil.rmtree(os.path.join(output, ".parts"), ignore_errors=True)
    try:
        # a batch's kmers.tsv rows go into the part block by block as they leave the device (or, from a batch that fell
        # back to the host renderers, as one text, in its place)
        _shard_batches(make_batches(targets_sink=kmers_tsv), each, dist, device, drop_parts)
        stats["local_patterns"] = eng.pattern_count()
        stats["pattern_rows"], stats["patterns"] = finish_shard(eng, writer, dist, device, method)
    finally:
        writer.close()
    _barrier(dist, device)
    if rank == 0:
        assemble(output, world, strains, compress, device_gzip=device_gzip)
    _barrier(dist, device)
    stats["bytes"] += writer.bytes                        # the pattern rows, behind the batches' text
    return stats
