"""The reference's two downstream tools over the files the hot path writes, same options, same
output:

    panfeed-get-clusters  /root/reference/panfeed/get_clusters.py:71-101
    panfeed-get-kmers     /root/reference/panfeed/get_kmers.py:88-145

What costs time in them is streaming `kmers_to_hashes.tsv` (one row per kept k-mer of the whole pangenome) and
`kmers.tsv` through pandas in 100 000-row chunks only to keep the few rows whose hash / cluster is in a set.  Here that
row filter runs on the GPU over the raw text (`RowFilter` -> pf_rowfilter_scan, or pf_rowfilter_scan_members for a
device-gzipped file, csrc/pf_rowfilter.hip); the small
tables that remain (the associations, the kept rows) go through the same pandas statements as the reference's, so the
printed tables are the same bytes.  There is no CPU fallback for the filter.

One thing the reference leaves to chance is kept out of the comparison: it iterates over Python `set`s of cluster
names, so the order of its printed clusters / blocks changes with PYTHONHASHSEED.  Here clusters come in order of their
first appearance in kmers_to_hashes.tsv.
"""
import argparse
import ctypes as C
import gzip
import io
import logging
import sys

import pandas as pd

from . import _lib

logger = logging.getLogger("panfeed")

BLOCK_BYTES = 256 << 20
# the device gunzip route reads COMPRESSED bytes: an eighth of the text block, which these texts' ratio of 6 to 8 makes
# about one block of text a call (a call takes 256 MiB of text at most and hands the rest back)
GZ_BLOCK_DIVISOR = 8
GZ_HEAD = b"\x1f\x8b\x08\x00"          # ID1 ID2 CM=8 FLG=0: the only header the device decoder takes


class NotTaken(RuntimeError):
    """device_gunzip=True and the file is not one the device decoder takes"""


class RowFilter:
    """rows of a TSV whose first (`first_field=True`) or last field is one of `keys`, filtered on the device"""

    device_gunzip_files = 0         # files, over all filters, that went the device gunzip route to their end
    fallback_files = 0              # and files the automatic mode began there and read again through gzip

    def __init__(self, keys, first_field, device=0):
        self.L = _lib.load()
        ks = [k.encode() if isinstance(k, str) else bytes(k) for k in keys]
        arr = (C.c_char_p * max(len(ks), 1))(*ks)
        lens = (C.c_uint32 * max(len(ks), 1))(*[len(k) for k in ks])
        self.h = C.c_void_p()
        self.fallbacks = 0              # files the automatic mode began on the device and read again through gzip
        _lib.check(self.L.pf_rowfilter_create(int(device), 1 if first_field else 0, arr, lens, len(ks), C.byref(self.h)))

    def close(self):
        if self.h:
            self.L.pf_rowfilter_destroy(self.h)
            self.h = C.c_void_p()

    __del__ = close

    def stats(self):
        n, ms = C.c_uint64(), C.c_float()
        _lib.check(self.L.pf_rowfilter_stats(self.h, C.byref(n), C.byref(ms)))
        gm, gt, gms, gdev = C.c_uint64(), C.c_uint64(), C.c_float(), C.c_uint64()
        _lib.check(self.L.pf_rowfilter_gunzip_stats(self.h, C.byref(gm), C.byref(gt), C.byref(gms), C.byref(gdev)))
        return {"bytes_scanned": int(n.value), "device_ms": float(ms.value),
                "members_inflated": int(gm.value), "text_bytes_inflated": int(gt.value), "inflate_ms": float(gms.value),
                "inflate_device_bytes": int(gdev.value), "gunzip_fallbacks": self.fallbacks}

    def scan_block(self, data, n=None):
        """(matching lines of the complete lines of `data` (bytes, or the first n bytes of a bytearray), joined; number of
        bytes consumed)"""
        b, e = C.POINTER(C.c_uint64)(), C.POINTER(C.c_uint64)()
        cnt, used = C.c_uint64(), C.c_uint64()
        if isinstance(data, bytearray):
            n = len(data) if n is None else n
            ptr = (C.c_char * len(data)).from_buffer(data)          # no copy
        else:
            n, ptr = len(data), data
        _lib.check(self.L.pf_rowfilter_scan(self.h, ptr, n, C.byref(b), C.byref(e), C.byref(cnt), C.byref(used)))
        view = memoryview(data)
        got = b"".join(view[b[i]:e[i]] for i in range(cnt.value))
        del ptr, view
        return got, int(used.value)

    def scan_members(self, data, last):
        """(matching lines of the text of the whole gzip members in `data` (bytes of the compressed file from a member
        start on), joined; compressed bytes consumed; whether the device decoder took them)"""
        lines, nb, cnt, used, taken = C.c_void_p(), C.c_uint64(), C.c_uint64(), C.c_uint64(), C.c_int()
        _lib.check(self.L.pf_rowfilter_scan_members(self.h, data, len(data), 1 if last else 0, C.byref(lines), C.byref(nb),
                                                    C.byref(cnt), C.byref(used), C.byref(taken)))
        got = C.string_at(lines, nb.value) if nb.value else b""
        return got, int(used.value), bool(taken.value)

    def _filter_members(self, path, block_bytes):
        """filter_file's device gunzip route: (header, rows), or None with the library's reason logged when a block was
        not taken.  Blocks of the compressed file go up as they are; what follows a block's last whole member is put in
        front of the next block."""
        block = max(1, block_bytes or BLOCK_BYTES // GZ_BLOCK_DIVISOR)
        out = []
        _lib.check(self.L.pf_rowfilter_members_begin(self.h, 1))
        with open(path, "rb") as fh:
            carry, eof = b"", False
            while True:
                if not eof:
                    chunk = fh.read(block)
                    eof = len(chunk) < block
                    carry = carry + chunk if carry else chunk
                got, used, taken = self.scan_members(carry, eof)
                if not taken:
                    logger.debug("%s: %s", path, self.L.pf_last_error().decode(errors="replace"))
                    return None
                out.append(got)
                carry = carry[used:]
                if eof and not carry:
                    break
        line, n = C.c_void_p(), C.c_uint64()
        _lib.check(self.L.pf_rowfilter_members_header(self.h, C.byref(line), C.byref(n)))
        return (C.string_at(line, n.value) if n.value else b""), b"".join(out)

    def filter_file(self, path, block_bytes=None, device_gunzip=None):
        """(header line, matching data lines) of a TSV file.  A .gz file made of small members with the plain gzip header
        (--gpu-compress writes such) is inflated on the device and scanned there: device_gunzip=None tries that for a
        name ending in .gz whose first bytes are such a header, and reads the whole file again through gzip, as pandas
        does by the name, when a block is not taken; False never tries; True raises NotTaken instead of reading again.
        block_bytes then counts compressed bytes.  Otherwise the file is read block by block straight into one buffer;
        what follows a block's last complete line is moved to the front for the next block."""
        if device_gunzip is None:
            device_gunzip = False
            if str(path).endswith(".gz"):
                with open(path, "rb") as fh:
                    device_gunzip = fh.read(10)[:4] == GZ_HEAD
            auto = True
        else:
            auto = False
        if device_gunzip:
            got = self._filter_members(path, block_bytes)
            if got is not None:
                RowFilter.device_gunzip_files += 1
                return got
            if not auto:
                raise NotTaken(f"{path}: {self.L.pf_last_error().decode(errors='replace')}")
            self.fallbacks += 1
            RowFilter.fallback_files += 1
        out = []

        def scan(buf, n):
            got, used = self.scan_block(buf, n)
            out.append(got)
            return used

        with open_table(path) as fh:
            header = fh.readline()
            scan_lines(fh, scan, block_bytes)
        return header, b"".join(out)


def open_table(path):
    """a TSV file for reading bytes (.gz through gzip, as pandas does by the name)"""
    return (gzip.open if str(path).endswith(".gz") else open)(path, "rb")


def scan_lines(fh, scan, block_bytes=None):
    """Feed the rest of `fh` to `scan(buf, n)` block by block, read straight into one buffer; scan looks at the complete
    lines of buf[:n] and returns the bytes it consumed.  What follows a block's last complete line is moved to the front
    for the next block; a last line without its newline is given one."""
    block_bytes = block_bytes or BLOCK_BYTES
    buf = bytearray(block_bytes + (1 << 16))
    have = 0                                         # bytes carried over, at the front of buf
    while True:
        if have + block_bytes > len(buf):            # a line longer than the slack
            buf.extend(bytes(have + block_bytes - len(buf)))
        got_n = fh.readinto(memoryview(buf)[have:have + block_bytes])
        if not got_n:
            break
        total = have + got_n
        used = scan(buf, total)
        have = total - used
        buf[:have] = buf[used:total]
    if have:                                         # a last line without its newline
        tail = bytearray(buf[:have]) + b"\n"
        scan(tail, len(tail))


def _table(header, rows):
    return pd.read_csv(io.BytesIO(header + rows), sep="\t")


def _options(description, kmers):
    p = argparse.ArgumentParser(description=description)
    p.add_argument("-a", "--associations", required=True)
    p.add_argument("-p", "--kmers-to-hashes", required=True)
    if kmers:
        p.add_argument("-k", "--kmers", required=True)
    p.add_argument("-t", "--threshold", type=float, default=1)
    p.add_argument("-c", "--column", default="lrt-pvalue")
    p.add_argument("-o", "--output", default=None)
    if kmers:
        p.add_argument("--only-passing", action="store_true", default=False)
        p.add_argument("--clusters-per-iteration", type=int, default=15)
    p.add_argument("-v", action="count", default=0)
    p.add_argument("--device", type=int, default=0, help="GPU the row filter runs on")
    p.add_argument("--host-gunzip", action="store_true", default=False,
                   help="inflate .gz inputs on the host (by default files of small members, as --gpu-compress writes, are inflated on the GPU)")
    return p


def _associations(args, index_name=None):
    """the filtered associations table and the passing hashes (get_clusters.py:76-88, get_kmers.py:93-106)"""
    a = pd.read_csv(args.associations, sep="\t", index_col=0)
    if index_name:
        a.index.name = index_name
    if args.column not in a.columns:
        logger.warning(f"Associations file does not have the {args.column} column")
        sys.exit(1)
    a = a[a[args.column] <= args.threshold]
    if args.output is not None:
        a.to_csv(args.output, sep="\t")
    return a, [str(x) for x in a.index.unique()]


_NAN_KEY = float("nan")      # ONE object for every NaN a column holds (tolist() makes a new one per cell, and nan != nan)


def _key(v):
    return _NAN_KEY if isinstance(v, float) and v != v else v


def _ordered_unique(series):
    return list(dict.fromkeys(_key(v) for v in series.tolist()))


def _filtered(keys, first_field, path, args):
    """(header line, matching data lines) of one table by a filter of its own; .gz inputs go the device gunzip route when
    they are files it takes, unless --host-gunzip"""
    f = RowFilter(keys, first_field=first_field, device=args.device)
    try:
        return f.filter_file(path, device_gunzip=False if args.host_gunzip else None)
    finally:
        f.close()


def _first_fields(rows):
    """the literal first field of every line of `rows` (bytes), in order"""
    return [ln.split(b"\t", 1)[0] for ln in rows.split(b"\n") if ln]


def get_clusters(argv=None, out=None):
    """panfeed-get-clusters: the gene clusters that have a k-mer whose pattern passes the threshold, one per line"""
    out = out or sys.stdout
    args = _options("Indicate which genes clusters have significantly associated patterns", False).parse_args(argv)
    a, passing = _associations(args)
    header, rows = _filtered(passing, False, args.kmers_to_hashes, args)
    h = _table(header, rows)
    for c in _ordered_unique(h["cluster"]):
        print(c, file=out)
    return 0


def get_kmers(argv=None, out=None):
    """panfeed-get-kmers: association results joined with the k-mers' clusters and positions"""
    out = out or sys.stdout
    args = _options("Annotate association results with positional information", True).parse_args(argv)
    a, passing = _associations(args, index_name="hashed_pattern")
    header, rows = _filtered(passing, False, args.kmers_to_hashes, args)
    h = _table(header, rows).set_index("hashed_pattern")
    clusters = _ordered_unique(h["cluster"])
    # The device filter compares the TEXT of a row's cluster field, the reference the values pandas parsed on both sides
    # (get_kmers.py:131-134): a cluster named '007' or '1e3' parses as a number whose str() is not the file's bytes.  The
    # keys given to the filter are therefore the literal fields of the kept kmers_to_hashes rows, grouped by the value
    # pandas made of them (row i of `h` is line i of `rows`).
    # (a value pandas read as NaN -- numeric cluster ids plus an 'NA' -- is a different object at every look: _key)
    literal = {}
    for val, lit in zip(h["cluster"].tolist(), _first_fields(rows)):
        literal.setdefault(_key(val), {})[lit] = None
    first = True
    b = a.join(h, how="inner") if clusters else None                       # get_kmers.py:136
    for idx in range(0, len(clusters), args.clusters_per_iteration):
        bunch = clusters[idx: idx + args.clusters_per_iteration]
        # (a NaN among the bunch selects nothing: the reference's `x['cluster'].isin(bunch)`, get_kmers.py:131-134, is False
        # for a NaN cell when the bunch is a list of the column's unique() values -- such rows are dropped, not matched)
        kheader, krows = _filtered([lit for c in bunch if c is not _NAN_KEY for lit in literal[_key(c)]], True, args.kmers, args)
        k = _table(kheader, krows).set_index(["cluster", "k-mer"])
        how = "left" if args.only_passing else "right"                      # get_kmers.py:137-141
        t = b.reset_index().set_index(["cluster", "k-mer"]).join(k, how=how)
        t.to_csv(out, sep="\t", header=first)
        first = False
    return 0


def main_get_clusters():
    sys.exit(get_clusters())


def main_get_kmers():
    sys.exit(get_kmers())
