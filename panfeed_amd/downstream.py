"""The reference's two downstream tools over the files the hot path writes, same options, same
output:

    panfeed-get-clusters  /root/reference/panfeed/get_clusters.py:71-101
    panfeed-get-kmers     /root/reference/panfeed/get_kmers.py:88-145

What costs time in them is streaming `kmers_to_hashes.tsv` (one row per kept k-mer of the whole pangenome) and
`kmers.tsv` through pandas in 100 000-row chunks only to keep the few rows whose hash / cluster is in a set.  Here that
row filter runs on the GPU over the raw text (`RowFilter` -> pf_rowfilter_scan, csrc/pf_rowfilter.hip); the small
tables that remain (the associations, the kept rows) go through the same pandas statements as the reference's, so the
printed tables are the same bytes.  There is no CPU fallback for the filter.

panfeed-get-kmers' second step, the join of every kmers.tsv row of a bunch of clusters to the small table of passing
(cluster, k-mer) pairs, runs on the GPU as well (`KmerJoin` -> pf_kmerjoin_*): pandas renders the small table's columns
as text once per key (`rendered_texts`), one survey pass over kmers.tsv counts every bunch's rows and tells whether
pandas could print any of them other than as they stand, and one pass per bunch writes the annotated rows on the device.
A bunch the survey flags, and a run whose table the device cannot take, goes through the pandas statements of the
reference (`--host-join` sends everything there).

Both tools begin by thresholding the associations table (`_associations`).  That too is one pass on the GPU
(`AssocFilter` -> pf_assocfilter_*): it keeps the lines whose p-value may pass -- a superset, pandas makes the exact
comparison on what is left -- and tells, per column, which classes of cells the WHOLE file holds, so that the few kept
lines are parsed with the dtypes pandas would have inferred from all of them (`assoc_plan`).  A table the pass flags, or
whose classes pandas would mix, goes through the reference's two statements whole (`--host-associations` sends every
table there).

All three, and panfeed-plot's `plot.GridBuilder`, read a table the same two ways, written once here: a device-gzipped
file goes up compressed and is inflated where it lands (`pass_member_file` -> pf_*_members), any other is read block by
block through the host (`scan_lines`); `route_file` chooses, and falls back to the second when the device decoder does not
take a block.  What the four wrap around that -- the handle's life, the pointer to a block, the pass either way with the
call's own arguments and what drains its output, the header line -- is `DeviceTable`, their base.

panfeed-get-kmers --gz-output writes the annotated table as such a file itself: the device join's rows are gzipped where
they were written (pf_kmerjoin_set_gzip) and only the members come to the host; text made on the host -- the header line,
a bunch or a run that went through pandas -- goes into the same file as small members (output.SmallMemberGzipWriter), so
that panfeed-plot reads all of it on the device.

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

from . import _lib

logger = logging.getLogger("panfeed")

BLOCK_BYTES = 256 << 20
# the device gunzip route reads COMPRESSED bytes: an eighth of the text block, which these texts' ratio of 6 to 8 makes
# about one block of text a call (a call takes 256 MiB of text at most and hands the rest back)
GZ_BLOCK_DIVISOR = 8
GZ_HEAD = b"\x1f\x8b\x08\x00"          # ID1 ID2 CM=8 FLG=0: the plain header the device decoder takes
BGZF_HEAD = b"\x1f\x8b\x08\x04"        # and FLG=4 with the one extra subfield BC of two bytes: BGZF, what bgzip writes


class NotTaken(RuntimeError):
    """device_gunzip=True and the file is not one the device decoder takes"""


def _last_error():
    return _lib.load().pf_last_error().decode(errors="replace")


def _gz_members_file(path):
    """whether the file is a .gz whose first bytes are the only header the device decoder takes"""
    if not str(path).endswith(".gz"):
        return False
    with open(path, "rb") as fh:
        return fh.read(10)[:4] == GZ_HEAD


def _bgzf_file(path):
    """whether the file is a .gz that starts with a BGZF head: 1f 8b 08 04, and BC 02 00 at bytes 12 to 15"""
    if not str(path).endswith(".gz"):
        return False
    with open(path, "rb") as fh:
        head = fh.read(18)
    return len(head) == 18 and head[:4] == BGZF_HEAD and head[12:16] == b"BC\x02\x00"


def _gz_any_file(path):
    """whether the file is a .gz of any RFC 1952 head (1f 8b 08): what the large-member route (large_members=True) tries"""
    if not str(path).endswith(".gz"):
        return False
    with open(path, "rb") as fh:
        return fh.read(3) == GZ_HEAD[:3]


def pass_member_file(path, block_bytes, begin, call, after=None, reason=_last_error):
    """One pass over a file of gzip members through a device text feed (TextFeed, csrc/pf_rowfilter.hip): begin(), then
    blocks of the COMPRESSED file go to call(data, last) -> (compressed bytes used, whether the block was taken) as they
    are, what follows a block's last whole member put in front of the next block; `last` from the read that met the end
    of the file on; after() behind every call that was taken.  -> whether the file went through to its end: False, with
    reason() -- the library's -- logged, as soon as a block is not taken."""
    block = max(1, block_bytes or BLOCK_BYTES // GZ_BLOCK_DIVISOR)
    begin()
    with open(path, "rb") as fh:
        carry, eof = b"", False
        while True:
            if not eof:
                chunk = fh.read(block)
                eof = len(chunk) < block
                carry = carry + chunk if carry else chunk
            used, taken = call(carry, eof)
            if not taken:
                logger.debug("%s: %s", path, reason())
                return False
            if after:
                after()
            carry = carry[used:]
            if eof and not carry:
                return True


def route_file(path, device_gunzip, members, host, counts, again=None, reason=_last_error, large_members=False):
    """A file by the device gunzip route, members(), or through gzip as pandas reads it by the name, host(); -> what that
    returned.  device_gunzip=None tries members() for a .gz of a header the device decoder takes (plain, or BGZF) and, when it returns
    None -- a block was not taken --, runs again() (what the owner undoes before the file is read once more) and host();
    True tries members() whatever the file and raises NotTaken instead; False never tries.  `counts`: the owner's class,
    whose device_gunzip_files or fallback_files moves.  large_members: the owner's large-member route is on
    (DeviceTable.set_large_members), so the automatic mode tries members() for a .gz of any gzip head."""
    auto = device_gunzip is None
    if auto:
        device_gunzip = _gz_members_file(path) or _bgzf_file(path) or (large_members and _gz_any_file(path))
    if device_gunzip:
        got = members()
        if got is not None:
            counts.device_gunzip_files += 1
            return got
        if not auto:
            raise NotTaken(f"{path}: {reason()}")
        counts.fallback_files += 1
        if again:
            again()
    return host()


class DeviceTable:
    """What the four owners of a device text feed -- RowFilter, KmerJoin, AssocFilter here, plot.GridBuilder -- are alike: the
    life of the handle and the pass over a table file either way.  The counters route_file moves stay on each subclass:
    it does `counts.x += 1` on the class it is given, and one inherited from here would be all four's."""

    entry = None                    # the owner's entry points by name: create, destroy, members_begin, members_header

    def __init__(self):
        self.L = _lib.load()
        self.h = C.c_void_p()
        self._create_fn, self._destroy_fn, self._begin_fn, self._header_fn = (getattr(self.L, name) for name in self.entry)
        owner = self.entry[0][:-len("create")]
        self._set_large_fn, self._large_stats_fn = getattr(self.L, owner + "set_large_members"), getattr(self.L, owner + "large_stats")
        self.large_members, self.piece_bytes = False, 0

    def _create(self, *args):
        """a fresh handle, create(*args, &handle), in place of the one there may be (the large-member switch stays as set)"""
        self.close()
        _lib.check(self._create_fn(*args, C.byref(self.h)))
        if self.large_members:
            _lib.check(self._set_large_fn(self.h, 1, self.piece_bytes))

    def set_large_members(self, on, piece_bytes=0):
        """the large-member gunzip route (csrc/pf_deflate.h: large_call) for this owner's members passes: off by default.
        While on, what the small-member kernels do not take -- gzip's, pigz's and Python's whole-file members, 4 MiB zlib
        members, any RFC 1952 head -- is inflated on the device too, parallel inside a member.  piece_bytes: the compressed
        bytes between two places a block start is looked for from; 0: the default of 32 KiB, else at least 64"""
        self.large_members, self.piece_bytes = bool(on), int(piece_bytes)
        _lib.check(self._set_large_fn(self.h, 1 if on else 0, self.piece_bytes))

    def large_stats(self):
        """the large-member route so far (a fresh handle counts from zero): starts found, live pieces, starts dropped as false
        or redundant, members taken, and the device time of its four passes"""
        pieces, ms = (C.c_uint64 * 4)(), (C.c_float * 4)()
        _lib.check(self._large_stats_fn(self.h, pieces, ms))
        return {"pieces_found": int(pieces[0]), "pieces_live": int(pieces[1]), "pieces_dropped": int(pieces[2]),
                "large_members": int(pieces[3]), "find_ms": float(ms[0]), "marker_ms": float(ms[1]), "chain_ms": float(ms[2]),
                "bytes_ms": float(ms[3])}

    def _large(self, large_members, piece_bytes=None):
        """a file call's large_members / piece_bytes arguments: None leaves the switch (the piece) as set_large_members left
        it, anything else sets it; -> whether the route is on"""
        if large_members is not None or piece_bytes is not None:
            on = self.large_members if large_members is None else bool(large_members)
            piece = self.piece_bytes if piece_bytes is None else int(piece_bytes)
            if (on, piece) != (self.large_members, self.piece_bytes):
                self.set_large_members(on, piece)
        return self.large_members

    def close(self):
        if self.h:
            self._destroy_fn(self.h)
            self.h = C.c_void_p()

    __del__ = close

    @staticmethod
    def _pointer(data, n=None):
        """(what ctypes passes for `data`, the bytes of it that count): bytes as they are, a bytearray -- its first n bytes
        count -- without a copy.  The export holds the bytearray's size: the caller drops the pointer (`del`) before
        anything may resize the buffer, as scan_lines' buf.extend does"""
        if isinstance(data, bytearray):
            return (C.c_char * len(data)).from_buffer(data), len(data) if n is None else n
        return data, len(data)

    def _members_pass(self, path, block_bytes, fn, args=(), drain=None):
        """one pass over a file of device members, fn(handle, block, its bytes, last, *args, &used, &taken) a block, then
        drain() if the block was taken (pass_member_file's `after`); False when one was not"""
        def call(data, last):
            used, taken = C.c_uint64(), C.c_int()
            _lib.check(fn(self.h, data, len(data), 1 if last else 0, *args, C.byref(used), C.byref(taken)))
            return used.value, taken.value

        return pass_member_file(path, block_bytes, lambda: _lib.check(self._begin_fn(self.h, 1)), call, drain)

    def _plain_pass(self, path, block_bytes, fn, args=(), drain=None):
        """one pass over a table file through the host, fn(handle, block, its bytes, *args, &used) a block of lines, then
        drain(block) -- the block for a drain whose output speaks of it --; -> the header line, which is no block's"""
        def scan(buf, n):
            used = C.c_uint64()
            ptr, n = self._pointer(buf, n)
            _lib.check(fn(self.h, ptr, n, *args, C.byref(used)))
            del ptr
            if drain:
                drain(buf)
            return int(used.value)

        with open_table(path) as fh:
            header = fh.readline()
            scan_lines(fh, scan, block_bytes)
        return header

    def _drain(self, next_fn, sink):
        """the text the last call left on the device to sink(a view of it), piece by piece: next_fn(handle, &piece, &bytes)"""
        piece, n = C.c_void_p(), C.c_uint64()
        while True:
            _lib.check(next_fn(self.h, C.byref(piece), C.byref(n)))
            if not n.value:
                return
            sink(memoryview((C.c_char * n.value).from_address(piece.value)))

    def _header(self):
        """the header line the members pass peeled off"""
        line, n = C.c_void_p(), C.c_uint64()
        _lib.check(self._header_fn(self.h, C.byref(line), C.byref(n)))
        return C.string_at(line, n.value) if n.value else b""


class RowFilter(DeviceTable):
    """rows of a TSV whose first (`first_field=True`) or last field is one of `keys`, filtered on the device"""

    entry = ("pf_rowfilter_create", "pf_rowfilter_destroy", "pf_rowfilter_members_begin", "pf_rowfilter_members_header")
    device_gunzip_files = 0         # files, over all filters, that went the device gunzip route to their end
    fallback_files = 0              # and files the automatic mode began there and read again through gzip

    def __init__(self, keys, first_field, device=0):
        super().__init__()
        ks = [k.encode() if isinstance(k, str) else bytes(k) for k in keys]
        arr, lens = _lib.c_strings(ks)
        self.fallbacks = 0              # files the automatic mode began on the device and read again through gzip
        self._create(int(device), 1 if first_field else 0, arr, lens, len(ks))

    def stats(self):
        n, ms = C.c_uint64(), C.c_float()
        _lib.check(self.L.pf_rowfilter_stats(self.h, C.byref(n), C.byref(ms)))
        gm, gt, gms, gdev = C.c_uint64(), C.c_uint64(), C.c_float(), C.c_uint64()
        _lib.check(self.L.pf_rowfilter_gunzip_stats(self.h, C.byref(gm), C.byref(gt), C.byref(gms), C.byref(gdev)))
        return {"bytes_scanned": int(n.value), "device_ms": float(ms.value),
                "members_inflated": int(gm.value), "text_bytes_inflated": int(gt.value), "inflate_ms": float(gms.value),
                "inflate_device_bytes": int(gdev.value), "gunzip_fallbacks": self.fallbacks}

    @staticmethod
    def _rows(data, b, e, cnt):
        """the lines data[b[i]:e[i]] of pf_rowfilter_scan's answer, joined (the view goes with the call)"""
        view = memoryview(data)
        return b"".join(view[b[i]:e[i]] for i in range(cnt.value))

    def scan_block(self, data, n=None):
        """(matching lines of the complete lines of `data` (bytes, or the first n bytes of a bytearray), joined; number of
        bytes consumed)"""
        b, e = C.POINTER(C.c_uint64)(), C.POINTER(C.c_uint64)()
        cnt, used = C.c_uint64(), C.c_uint64()
        ptr, n = self._pointer(data, n)
        _lib.check(self.L.pf_rowfilter_scan(self.h, ptr, n, C.byref(b), C.byref(e), C.byref(cnt), C.byref(used)))
        del ptr
        return self._rows(data, b, e, cnt), int(used.value)

    def scan_members(self, data, last):
        """(matching lines of the text of the whole gzip members in `data` (bytes of the compressed file from a member
        start on), joined; compressed bytes consumed; whether the device decoder took them)"""
        lines, nb, cnt, used, taken = C.c_void_p(), C.c_uint64(), C.c_uint64(), C.c_uint64(), C.c_int()
        _lib.check(self.L.pf_rowfilter_scan_members(self.h, data, len(data), 1 if last else 0, C.byref(lines), C.byref(nb),
                                                    C.byref(cnt), C.byref(used), C.byref(taken)))
        got = C.string_at(lines, nb.value) if nb.value else b""
        return got, int(used.value), bool(taken.value)

    def _fell_back(self):
        self.fallbacks += 1

    def filter_file(self, path, block_bytes=None, device_gunzip=None, large_members=None, piece_bytes=None):
        """(header line, matching data lines) of a TSV file.  large_members: True sends a .gz of any head through the
        large-member route as well, False does not, None (the default) leaves the owner's switch as set_large_members set it;
        piece_bytes likewise.  A .gz file made of small members with the plain gzip header
        (--gpu-compress writes such) is inflated on the device and scanned there, as device_gunzip says (route_file);
        block_bytes then counts compressed bytes.  Otherwise the file is read block by block straight into one buffer;
        what follows a block's last complete line is moved to the front for the next block."""
        def members():                               # (header, rows), or None when a block was not taken
            out, lines, nb, cnt = [], C.c_void_p(), C.c_uint64(), C.c_uint64()
            took = self._members_pass(path, block_bytes, self.L.pf_rowfilter_scan_members, (C.byref(lines), C.byref(nb), C.byref(cnt)),
                                      lambda: out.append(C.string_at(lines, nb.value) if nb.value else b""))
            return (self._header(), b"".join(out)) if took else None

        def host():
            out, b, e, cnt = [], C.POINTER(C.c_uint64)(), C.POINTER(C.c_uint64)(), C.c_uint64()
            header = self._plain_pass(path, block_bytes, self.L.pf_rowfilter_scan, (C.byref(b), C.byref(e), C.byref(cnt)),
                                      lambda buf: out.append(self._rows(buf, b, e, cnt)))
            return header, b"".join(out)

        return route_file(path, device_gunzip, members, host, RowFilter, self._fell_back, large_members=self._large(large_members, piece_bytes))


KJ_FLAG_NAMES = ((1, "not 10 tabs"), (2, "a control, non-ASCII or quote byte"), (4, "an integer field that is not canonical decimal"),
                 (8, "an empty text field"), (16, "an NA string"), (32, "a text field of number characters only"),
                 (64, "inf / nan / true / false"), (128, "a row over 65 536 or a field of 4 096 bytes or more"))
KJ_RAW = 2                          # KmerJoin.join_file's mode: the rows that have a key, as they stand


class KmerJoin(DeviceTable):
    """the rows of kmers.tsv whose cluster is a selected one, annotated with the rendered text of their (cluster, k-mer)
    on the device.  clusters: (literal bytes, bunch number) pairs; keys: (cluster bytes, k-mer bytes) pairs with their two
    renderings text0 / text1; empty: the text of a row that has no key"""

    device_bunches = 0              # bunches, over all joins, written by the device
    host_bunches = 0                # bunches the survey flagged: joined by pandas
    host_runs = 0                   # runs whose table the device route refused: every bunch joined by pandas
    device_gunzip_files = 0         # passes over a file that went the device gunzip route to their end
    fallback_files = 0              # and passes the automatic mode began there and read again through gzip
    last_stats = None               # stats() of the last run's join, with the survey's rows and unmatched rows over all bunches
    entry = ("pf_kmerjoin_create", "pf_kmerjoin_destroy", "pf_kmerjoin_members_begin", "pf_kmerjoin_members_header")

    def __init__(self, clusters, n_bunches, keys, text0, text1, empty, device=0):
        super().__init__()
        self.n_bunches = max(int(n_bunches), 1)
        self.members = {}               # path -> whether the survey went the device gunzip route to the end
        strs = _lib.c_strings
        cl, cl_len = strs([c for c, _ in clusters])
        bunch = (C.c_uint32 * max(len(clusters), 1))(*[b for _, b in clusters])
        kc, kc_len = strs([c for c, _ in keys])
        kk, kk_len = strs([k for _, k in keys])
        t0, t0_len = strs(list(text0))
        t1, t1_len = strs(list(text1))
        self._create(int(device), cl, cl_len, bunch, len(clusters), self.n_bunches, kc, kc_len, kk, kk_len, t0, t0_len, t1, t1_len,
                     len(keys), empty, len(empty))

    def stats(self):
        st, ms = (C.c_uint64 * 8)(), (C.c_float * 3)()
        _lib.check(self.L.pf_kmerjoin_stats(self.h, st, ms))
        gt, gm, gms, gdev = C.c_uint64(), C.c_uint64(), C.c_float(), C.c_uint64()
        _lib.check(self.L.pf_kmerjoin_gzip_stats(self.h, C.byref(gt), C.byref(gm), C.byref(gms), C.byref(gdev)))
        return {"bytes_scanned": int(st[0]), "rows_written": int(st[1]), "raw_rows": int(st[2]), "members_inflated": int(st[3]),
                "text_bytes_inflated": int(st[4]), "inflate_device_bytes": int(st[5]), "hash_rejects": int(st[6]),
                "unmatched_written": int(st[7]),
                "survey_ms": float(ms[0]), "write_ms": float(ms[1]), "inflate_ms": float(ms[2]),
                "gzip_text_bytes": int(gt.value), "gzip_member_bytes": int(gm.value), "gzip_ms": float(gms.value),
                "gzip_device_bytes": int(gdev.value)}

    def set_gzip(self, on, flags=0):
        """while on, join_file's write() gets gzip members of the annotated rows (modes 0 and 1; KJ_RAW stays text).  flags:
        the device encoder's effort (_lib.GZ_DEEP) and test hooks (_lib.GZ_*)"""
        _lib.check(self.L.pf_kmerjoin_set_gzip(self.h, 1 if on else 0, int(flags)))

    def counters(self):
        """per bunch: rows, unmatched rows, output bytes under either rendering, plainness flags"""
        p, n = C.POINTER(C.c_uint64)(), C.c_uint32()
        _lib.check(self.L.pf_kmerjoin_counters(self.h, C.byref(p), C.byref(n)))
        return [{"rows": int(p[5 * i]), "unmatched": int(p[5 * i + 1]), "bytes": (int(p[5 * i + 2]), int(p[5 * i + 3])),
                 "flags": int(p[5 * i + 4])} for i in range(n.value)]

    def survey_file(self, path, block_bytes=None, device_gunzip=None, large_members=None, piece_bytes=None):
        """one pass over kmers.tsv for all bunches: counters().  device_gunzip and large_members as RowFilter.filter_file's
        (join_file reads the file the way the survey found for it, with the switch as the survey left it)"""
        def members():
            self.members[path] = self._members_pass(path, block_bytes, self.L.pf_kmerjoin_survey_members)
            return True if self.members[path] else None

        def host():
            self._plain_pass(path, block_bytes, self.L.pf_kmerjoin_survey)
            return True

        self.members[path] = False
        # (a survey that stopped half way has counted rows: they go before the file is read again)
        route_file(path, device_gunzip, members, host, KmerJoin, lambda: _lib.check(self.L.pf_kmerjoin_reset_counters(self.h)),
                   large_members=self._large(large_members, piece_bytes))
        return self.counters()

    def join_file(self, path, bunch, mode, write, block_bytes=None):
        """one pass over kmers.tsv for one bunch: its annotated rows (mode 0 / 1: the rendering) or its raw rows that have
        a key (KJ_RAW) go to write(), in file order.  The file goes the way the survey found for it."""
        args = (bunch, mode, C.byref(C.c_uint64()))

        def drain(_block=None):                      # the text the block's join call made, piece by piece
            self._drain(self.L.pf_kmerjoin_next_text, write)

        if not self.members.get(path):
            self._plain_pass(path, block_bytes, self.L.pf_kmerjoin_join, args, drain)
        elif self._members_pass(path, block_bytes, self.L.pf_kmerjoin_join_members, args, drain):
            KmerJoin.device_gunzip_files += 1
        else:
            raise NotTaken(f"{path}: {self.L.pf_last_error().decode(errors='replace')} (the survey pass took the file)")


AF_INT, AF_FLOAT, AF_NA, AF_ODD, AF_TEXT = 1, 2, 4, 8, 16
AF_FLAG_NAMES = ((1, "a row with another number of fields than the header"), (2, "an empty line"),
                 (4, "a control byte or a quote"), (8, "a row over 65 536 or a field of 4 096 bytes or more"))
AF_MARGIN = 2.0 ** -30              # the device drops a row only above threshold + |threshold| * AF_MARGIN


class AssocFilter(DeviceTable):
    """the data lines of an associations table whose cell in field `pvalue_field` may be <= threshold, kept on the device
    as they stand, with the classes of all cells per column and the rows' flags"""

    device_files = 0                # tables, over all filters, whose kept lines alone went to pandas
    host_files = 0                  # tables that went through pandas whole
    device_gunzip_files = 0         # passes over a file that went the device gunzip route to their end
    fallback_files = 0              # and passes the automatic mode began there and read again through gzip
    last_stats = None               # stats() of the last table that had a device pass
    entry = ("pf_assocfilter_create", "pf_assocfilter_destroy", "pf_assocfilter_members_begin", "pf_assocfilter_members_header")

    def __init__(self, pvalue_field, n_fields, threshold, device=0):
        super().__init__()
        self.args = (int(device), int(pvalue_field), int(n_fields), float(threshold) + abs(float(threshold)) * AF_MARGIN)
        self.header = None              # the header line the device gunzip route peeled off
        self._create(*self.args)

    def stats(self):
        st, ms = (C.c_uint64 * 4)(), (C.c_float * 2)()
        _lib.check(self.L.pf_assocfilter_stats(self.h, st, ms))
        c = self.columns()
        return {"bytes_scanned": int(st[0]), "rows": c["rows"], "kept": c["kept"], "members_inflated": int(st[1]),
                "text_bytes_inflated": int(st[2]), "inflate_device_bytes": int(st[3]), "device_ms": float(ms[0]),
                "inflate_ms": float(ms[1])}

    def columns(self):
        """over all lines scanned so far: the class bits of every column, the OR of the rows' flags, data and kept lines"""
        bits, n, flags, cnt = C.POINTER(C.c_uint32)(), C.c_uint32(), C.c_uint32(), (C.c_uint64 * 2)()
        _lib.check(self.L.pf_assocfilter_columns(self.h, C.byref(bits), C.byref(n), C.byref(flags), cnt))
        return {"classes": [int(bits[i]) for i in range(n.value)], "flags": int(flags.value), "rows": int(cnt[0]), "kept": int(cnt[1])}

    def _take(self, out):
        """the kept lines of the last scan call, appended to `out`"""
        self._drain(self.L.pf_assocfilter_next_lines, lambda piece: out.append(bytes(piece)))

    def scan_block(self, data, n=None):
        """(kept lines of the complete lines of `data` (bytes, or the first n bytes of a bytearray), joined; bytes consumed)"""
        kept, used, out = C.c_uint64(), C.c_uint64(), []
        ptr, n = self._pointer(data, n)
        _lib.check(self.L.pf_assocfilter_scan(self.h, ptr, n, C.byref(kept), C.byref(used)))
        del ptr
        self._take(out)
        return b"".join(out), int(used.value)

    def scan_members(self, data, last):
        """(kept lines of the text of the whole gzip members in `data`, joined; compressed bytes consumed; whether the
        device decoder took them)"""
        kept, used, taken, out = C.c_uint64(), C.c_uint64(), C.c_int(), []
        _lib.check(self.L.pf_assocfilter_scan_members(self.h, data, len(data), 1 if last else 0, C.byref(kept), C.byref(used),
                                                      C.byref(taken)))
        if taken.value:
            self._take(out)
        return b"".join(out), int(used.value), bool(taken.value)

    def filter_file(self, path, block_bytes=None, device_gunzip=None, large_members=None, piece_bytes=None):
        """the kept data lines of a table file, joined; columns() then speaks of the whole file.  device_gunzip and large_members as
        RowFilter.filter_file's (a pass that stopped half way has ORed classes in: the filter is made anew before the file
        is read again)"""
        args = (C.byref(C.c_uint64()),)

        def members():                               # the kept lines, or None when a block was not taken
            out = []
            if not self._members_pass(path, block_bytes, self.L.pf_assocfilter_scan_members, args, lambda: self._take(out)):
                return None
            self.header = self._header()
            return b"".join(out)

        def host():
            out = []
            self._plain_pass(path, block_bytes, self.L.pf_assocfilter_scan, args, lambda _block: self._take(out))
            return b"".join(out)

        return route_file(path, device_gunzip, members, host, AssocFilter, lambda: self._create(*self.args),
                          large_members=self._large(large_members, piece_bytes))


def assoc_header(line):
    """the column names of an associations table's header line (bytes), the index column's first; None for a header the
    device route leaves to pandas: no line, a name twice, an empty name, a quote or control byte, a byte-order mark, text
    that is not UTF-8"""
    if not line.endswith(b"\n"):
        return None
    try:
        text = line[:-1].decode()
    except UnicodeDecodeError:
        return None
    names = text.split("\t")
    if len(set(names)) != len(names) or "" in names or any(ord(ch) < 0x20 and ch != "\t" or ch == '"' for ch in text):
        return None
    if text.startswith("\ufeff"):
        return None
    return names


def assoc_plan(names, pvalue_field, classes, flags, rows):
    """What the classes of a whole table's cells and its rows' flags say: (dtype per column name, None) -- the dtypes
    pandas infers from the whole file, to be forced on the kept lines --, or (None, why the table goes through pandas
    whole)."""
    if flags:
        return None, ", ".join(t for f, t in AF_FLAG_NAMES if flags & f)
    dtypes = {}
    for i, (name, c) in enumerate(zip(names, classes)):
        if c & AF_ODD:
            return None, f"column {name!r} holds a cell pandas may read otherwise in a part of the file"
        if c & AF_TEXT and c & (AF_INT | AF_FLOAT):
            return None, f"column {name!r} mixes text and numbers"
        if c & AF_TEXT and i == pvalue_field:
            return None, f"column {name!r} holds text"
        dtypes[name] = object if c & AF_TEXT else "int64" if c == AF_INT and rows else "float64"
    return dtypes, None


def assoc_table(header, kept, dtypes):
    """the kept lines as pandas reads them under the whole file's dtypes"""
    import pandas as pd
    return pd.read_csv(io.BytesIO(header + kept), sep="\t", index_col=0, dtype=dtypes)


def _isnan(v):
    return isinstance(v, float) and v != v


def rendered_texts(B, other_columns):
    """What the device join prints for the columns of B (indexed by cluster, k-mer), taken from pandas itself: B is
    joined (`how="right"`) to a probe frame of one row per key and one dummy integer column, printed, and the key and
    dummy fields are cut off each line -- once as it is (text0) and once with a probe row that has no key in B, which
    makes pandas promote B's integer columns to float and its bool columns to object as an unmatched kmers.tsv row does
    (text1).  Keys that hold a NaN match no plain row and are left out.
    -> dict(keys, text0, text1, empty, header), or a str: why the device route cannot take this table"""
    import pandas as pd
    keys = [k for k in B.index.tolist() if not (_isnan(k[0]) or _isnan(k[1]))]
    if len(set(keys)) != len(keys):
        return "the table has a (cluster, k-mer) twice"
    if not all(isinstance(c, str) and isinstance(k, str) for c, k in keys):
        return "a cluster or k-mer of the table is not text"
    clash = set(B.columns) & (set(other_columns) | {"cluster", "k-mer"})
    if clash:
        return f"column {sorted(clash)[0]!r} is in both tables"
    dummy = "probe"
    while dummy in B.columns:
        dummy += "_"
    nokey = "!"
    while any(c == nokey for c, _ in keys):
        nokey += "!"
    texts = []
    for extra in ([], [(nokey, nokey)]):
        probe_keys = keys + extra
        if not probe_keys:
            texts.append(([], None))
            continue
        probe = pd.DataFrame({dummy: 0}, index=pd.MultiIndex.from_tuples(probe_keys, names=["cluster", "k-mer"]))
        lines = B.join(probe, how="right").to_csv(sep="\t", header=True).split("\n")
        if len(lines) != len(probe_keys) + 2 or lines[-1] != "" or not lines[0].endswith("\t" + dummy):
            return "the table's text has line breaks of its own"
        got = []
        for (c, k), line in zip(probe_keys, lines[1:]):
            prefix = f"{c}\t{k}\t"
            if not (line.startswith(prefix) and line.endswith("\t0") and len(line) >= len(prefix) + 2):
                return f"pandas does not print the key ({c!r}, {k!r}) as it stands"
            got.append(line[len(prefix):-2].encode())
        texts.append((got, lines[0]))
    (text0, _), (text1, header) = texts
    empty = text1.pop()
    if empty != b"\t" * (len(B.columns) - 1):
        return "the text of a row without a key is not empty fields"
    if max([len(t) for t in text0 + text1] + [0]) >= 1 << 20:
        return "a key's text is 1 MiB or more"
    header = header[:-len(dummy)] + "\t".join(other_columns) + "\n"
    return {"keys": keys, "text0": text0, "text1": text1, "empty": empty, "header": header}


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
    import pandas as pd
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
        p.add_argument("--clusters-per-iteration", type=int, default=15,
                       help="clusters joined per pass over kmers.tsv (memory does not grow with it: a value as large as the "
                            "number of clusters makes the whole run two passes over the file, one survey and one join)")
        p.add_argument("--host-join", action="store_true", default=False,
                       help="join kmers.tsv to the associations in pandas, bunch by bunch (by default the GPU looks the rows up and writes them)")
        p.add_argument("--gz-output", default=None, metavar="PATH",
                       help="write the annotated table to PATH (ending in .gz) as small gzip members, compressed on the GPU where "
                            "the GPU wrote the rows, in place of printing it; panfeed-plot inflates such a file on the GPU")
        p.add_argument("--gz-level", type=int, choices=(1, 2), default=None,
                       help="with --gz-output: the effort of the GPU's encoder (default: 1); 2 looks for each position's match "
                            "in the row before as well and parses lazily: a smaller file for more encoder time")
    p.add_argument("--host-associations", action="store_true", default=False,
                   help="read the whole associations table with pandas (by default the GPU keeps the lines that may pass the "
                        "threshold and pandas reads those)")
    p.add_argument("-v", action="count", default=0)
    p.add_argument("--device", type=int, default=0, help="GPU the row filter runs on")
    p.add_argument("--host-gunzip", action="store_true", default=False,
                   help="inflate .gz inputs on the host (by default files of small members, as --gpu-compress writes, and BGZF files, "
                        "as bgzip or --gpu-compress --bgzf write, are inflated on the GPU)")
    p.add_argument("--gpu-gunzip-large", action="store_true", default=False,
                   help="inflate every other .gz input on the GPU as well -- what gzip, pigz or --compress wrote: large members, "
                        "decoded in parallel inside a member (off by default; --host-gunzip wins over it)")
    return p


def _missing_column(args):
    logger.warning(f"Associations file does not have the {args.column} column")
    sys.exit(1)


def _passing(a, args, index_name):
    """the reference's statements on a table as read_csv made it: (the filtered table, the passing hashes)"""
    if index_name:
        a.index.name = index_name
    if args.column not in a.columns:
        _missing_column(args)
    a = a[a[args.column] <= args.threshold]
    if args.output is not None:
        a.to_csv(args.output, sep="\t")
    return a, [str(x) for x in a.index.unique()]


def _device_scan(args, field, names):
    """one device pass over the associations file: (kept lines, AssocFilter.columns(), the header line if the device
    peeled it off)"""
    f = AssocFilter(field, len(names), args.threshold, device=args.device)
    try:
        kept = f.filter_file(args.associations, device_gunzip=False if args.host_gunzip else None, large_members=getattr(args, "gpu_gunzip_large", False))
        cols = f.columns()
        AssocFilter.last_stats = f.stats()
        return kept, cols, f.header
    finally:
        f.close()


def _associations(args, index_name=None, scan=_device_scan):
    """the filtered associations table and the passing hashes (get_clusters.py:76-88, get_kmers.py:93-106).  The file goes
    through the device filter (`scan`) and pandas reads the kept lines under the dtypes of the whole file; it reads the
    whole file, as the reference does, when the pass says the two could differ or --host-associations asks for it"""
    import pandas as pd
    a, why = None, "--host-associations"
    if not getattr(args, "host_associations", False):
        with open_table(args.associations) as fh:
            header = fh.readline()
        names = assoc_header(header)
        if names is None:
            why = "the header line is not plain"
        elif args.column not in names[1:]:
            _missing_column(args)
        else:
            field = names.index(args.column)
            kept, cols, peeled = scan(args, field, names)
            dtypes, why = assoc_plan(names, field, cols["classes"], cols["flags"], cols["rows"])
            if peeled is not None and peeled != header:
                dtypes, why = None, "the header line the device peeled off is not the file's first line"
            if dtypes is not None:
                a = assoc_table(header, kept, dtypes)
    if a is None:
        logger.debug("the associations go through pandas whole: %s", why)
        AssocFilter.host_files += 1
        a = pd.read_csv(args.associations, sep="\t", index_col=0)
    else:
        AssocFilter.device_files += 1
    return _passing(a, args, index_name)


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
        return f.filter_file(path, device_gunzip=False if args.host_gunzip else None, large_members=getattr(args, "gpu_gunzip_large", False))
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
    parser = _options("Annotate association results with positional information", True)
    args = parser.parse_args(argv)
    if args.gz_output is not None and not args.gz_output.endswith(".gz"):
        parser.error("--gz-output: the path must end in .gz (the downstream tools choose the device route by that suffix)")
    if args.gz_level is not None and args.gz_output is None:
        parser.error("--gz-level sets the effort of the encoder behind --gz-output: give --gz-output with it")
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
    b = a.join(h, how="inner") if clusters else None                       # get_kmers.py:136
    bunches = [clusters[idx: idx + args.clusters_per_iteration] for idx in range(0, len(clusters), args.clusters_per_iteration)]
    # (a NaN among the bunch selects nothing: the reference's `x['cluster'].isin(bunch)`, get_kmers.py:131-134, is False
    # for a NaN cell when the bunch is a list of the column's unique() values -- such rows are dropped, not matched)
    bunch_keys = [[lit for c in bunch if c is not _NAN_KEY for lit in literal[_key(c)]] for bunch in bunches]
    join, plan = (None, None) if args.host_join or not bunches else _device_join(args, b, bunch_keys)
    first = True
    sink = None
    try:
        if args.gz_output is not None:               # (the table goes there and nothing to `out`)
            from .output import SmallMemberGzipWriter
            out = sink = SmallMemberGzipWriter(args.gz_output, _lib.load().pf_gzip_device_chunk_bytes())
        for n, keys in enumerate(bunch_keys):
            if join is not None and not plan[n]["flags"]:
                first = _device_bunch(args, join, plan, n, b, out, first)
                KmerJoin.device_bunches += 1
                continue
            if join is not None:
                KmerJoin.host_bunches += 1
                logger.debug("bunch %d goes through pandas: %s", n, ", ".join(t for f, t in KJ_FLAG_NAMES if plan[n]["flags"] & f))
            kheader, krows = _filtered(keys, True, args.kmers, args)
            k = _table(kheader, krows).set_index(["cluster", "k-mer"])
            how = "left" if args.only_passing else "right"                      # get_kmers.py:137-141
            t = b.reset_index().set_index(["cluster", "k-mer"]).join(k, how=how)
            t.to_csv(out, sep="\t", header=first)
            first = False
    finally:
        if sink is not None:
            sink.close()
        if join is not None:
            KmerJoin.last_stats = dict(join.stats(), rows=sum(c["rows"] for c in plan), unmatched=sum(c["unmatched"] for c in plan))
            join.close()
    return 0


def _device_join(args, b, bunch_keys):
    """(a KmerJoin over the run's table, the survey's counters per bunch), or (None, None) with the reason logged when the
    device route cannot take the run"""
    from .engine import KMERS_TSV_HEADER
    columns = KMERS_TSV_HEADER.rstrip("\n").split("\t")
    with open_table(args.kmers) as fh:
        header = fh.readline()
    texts = "kmers.tsv does not have the header panfeed writes" if header != KMERS_TSV_HEADER.encode() else None
    if texts is None:
        B = b.reset_index().set_index(["cluster", "k-mer"])
        texts = rendered_texts(B, columns[1:10])
    if not isinstance(texts, str):
        literals = {lit for keys in bunch_keys for lit in keys}
        if not all(c.encode() in literals for c, _ in texts["keys"]):
            texts = "a cluster of the table is not printed as kmers_to_hashes spells it"
    if isinstance(texts, str):
        logger.debug("the join goes through pandas: %s", texts)
        KmerJoin.host_runs += 1
        return None, None
    join = KmerJoin([(lit, n) for n, keys in enumerate(bunch_keys) for lit in keys], len(bunch_keys),
                    [(c.encode(), k.encode()) for c, k in texts["keys"]], texts["text0"], texts["text1"], texts["empty"],
                    device=args.device)
    try:
        if args.gz_output is not None:
            join.set_gzip(True, _lib.gzip_level_flags(1 if getattr(args, "gz_level", None) is None else args.gz_level))
        plan = join.survey_file(args.kmers, device_gunzip=False if args.host_gunzip else None, large_members=getattr(args, "gpu_gunzip_large", False))
    except BaseException:
        join.close()
        raise
    join.header = texts["header"]
    return join, plan


def _writer(out, members=False):
    """bytes -> out: to its .buffer when it has one that takes UTF-8 as it is; `members`: they are gzip members for a
    writer of such"""
    if members:
        return out.write_members
    raw = getattr(out, "buffer", None)
    if raw is not None and str(getattr(out, "encoding", "")).lower().replace("-", "").replace("_", "") == "utf8":
        out.flush()
        return raw.write
    return lambda piece: out.write(bytes(piece).decode())


def _device_bunch(args, join, plan, n, b, out, first):
    """one bunch by the device route; -> `first` for the next bunch"""
    if not args.only_passing:
        if first:
            out.write(join.header)
        # (an unmatched row makes pandas promote the table's integer columns: the survey counted them)
        join.join_file(args.kmers, n, 1 if plan[n]["unmatched"] else 0, _writer(out, members=args.gz_output is not None))
        return False
    # how="left" stays a pandas join, over the rows of the bunch that have a key only: a left join drops the others
    kept = []
    join.join_file(args.kmers, n, KJ_RAW, lambda piece: kept.append(bytes(piece)))
    from .engine import KMERS_TSV_HEADER
    k = _table(KMERS_TSV_HEADER.encode(), b"".join(kept)).set_index(["cluster", "k-mer"])
    t = b.reset_index().set_index(["cluster", "k-mer"]).join(k, how="left")
    t.to_csv(out, sep="\t", header=first)
    return False


def main_get_clusters():
    sys.exit(get_clusters())


def main_get_kmers():
    sys.exit(get_kmers())
