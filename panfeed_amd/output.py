"""Output file surface of the hot path (names, headers, gzip mode), as the reference fixes it in
/root/reference/panfeed/input.py:235-259 and /root/reference/panfeed/panfeed.py:116-129."""
import ctypes as C
import io
import os

from . import _lib
from .engine import KMERS_TSV_HEADER, KMERS_TO_HASHES_HEADER, GzipMembers, _mem, hashes_to_patterns_header, text_len


class _GzipWriter:
    """What the writers of .gz files share: `write` takes str or bytes-like text (`_take` gets its bytes, never empty),
    `close` is done once -- the rest of the text goes out (`_finish`), and a file that needs it (`_is_empty`) gets one
    empty member, so that it is a valid gzip stream --, `with` closes.  MTIME: of the members made here (None: the time
    of writing, like gzip.open's)."""
    MTIME = 0

    def __init__(self, path, compresslevel):
        self.fh = open(path, "wb")
        self.level = compresslevel
        self.closed = False

    def _compress(self, data):
        import gzip
        return gzip.compress(bytes(data), compresslevel=self.level, mtime=self.MTIME)

    def write(self, text):
        b = text.encode() if isinstance(text, str) else bytes(text)
        if b:
            self._take(b)
        return len(text)

    def flush(self):
        # a flush of the reference's GzipFile only empties Python-side buffers into the deflate stream; members are
        # cut when enough text has gathered, so nothing is forced out here except at close
        self.fh.flush()

    def _finish(self):
        pass

    def close(self):
        if self.closed:
            return
        self._finish()
        if self._is_empty():
            self.fh.write(self._compress(b""))
        self.fh.close()
        self.closed = True

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()


class ParallelGzipWriter(_GzipWriter):
    """Text handle over a .gz file, like gzip.open(path, "wt", compresslevel=9) (input.py:239-241, 255-258), whose
    deflate work is done by the library's host threads: what is written is buffered, cut at line ends into chunks
    and compressed as independent gzip members (pf_gzip_members).  Reads back as the same text with any gzip reader."""
    MTIME = None

    def __init__(self, path, compresslevel=9, buffer_bytes=64 << 20, chunk_bytes=4 << 20):
        super().__init__(path, compresslevel)
        self.L = _lib.load()
        self.buffer_bytes, self.chunk_bytes = buffer_bytes, chunk_bytes
        self.parts, self.pending = [], 0
        self.wrote = False

    def _take(self, b):
        self.parts.append(b)
        self.pending += len(b)
        if self.pending >= self.buffer_bytes:
            self._finish()

    def _finish(self):
        data = b"".join(self.parts)
        self.parts, self.pending = [], 0
        if not data:
            return
        out, n = C.c_void_p(), C.c_uint64()
        _lib.check(self.L.pf_gzip_members(data, len(data), self.level, self.chunk_bytes, C.byref(out), C.byref(n)))
        try:
            self.fh.write(_mem(out, n.value))
        finally:
            self.L.pf_free_text(out)
        self.wrote = True

    def _is_empty(self):
        return not self.wrote


class MemberGzipWriter(_GzipWriter):
    """A .gz file made of gzip members from two sources: `write(text)` compresses the text on the host into one member
    (the header line; the batches that fell back to the host renderers), `write_members(view)` appends members that are
    complete already -- the GPU's (Engine(device_gzip=True)) -- as they are.  The first write is the file's header, so an
    output with no rows is still a valid gzip file.  `bytes_written` / `header_bytes` / `host_bytes`: the file's size, its
    first member's, and that of the members compressed here behind the header."""

    def __init__(self, path, compresslevel=9):
        super().__init__(path, compresslevel)
        self.bytes_written = 0
        self.header_bytes = None
        self.host_bytes = 0

    def _take(self, b):
        member = self._compress(b)
        if self.header_bytes is None:
            self.header_bytes = len(member)
        else:
            self.host_bytes += len(member)
        self.fh.write(member)
        self.bytes_written += len(member)

    def write_members(self, view):
        if len(view):
            if self.header_bytes is None:
                self.header_bytes = 0
            self.fh.write(view)
            self.bytes_written += len(view)

    def _is_empty(self):
        return not self.bytes_written


BGZF_BLOCK = 65280                   # text bytes per host-made BGZF member: bgzip's, so that a stored member still fits BSIZE
BGZF_EOF = bytes.fromhex("1f8b08040000000000ff0600424302001b0003000000000000000000")      # SAM specification 4.1


def bgzf_member(text, level):
    """one BGZF member of at most BGZF_BLOCK bytes of text: raw deflate by zlib under the 18-byte head (MTIME = 0, the one
    subfield BC, BSIZE = the member's size - 1)"""
    import struct
    import zlib
    z = zlib.compressobj(level, zlib.DEFLATED, -15)
    body = z.compress(text) + z.flush()
    size = 18 + len(body) + 8
    if len(text) > BGZF_BLOCK or size > 65536:
        raise ValueError("a BGZF member holds at most 65 536 bytes")
    return (bytes([0x1F, 0x8B, 8, 4, 0, 0, 0, 0, 0, 0xFF]) + struct.pack("<H2sHH", 6, b"BC", 2, size - 1) + body
            + struct.pack("<II", zlib.crc32(text), len(text)))


class BgzfMemberWriter(MemberGzipWriter):
    """MemberGzipWriter's file as BGZF (Engine(device_gzip=True, bgzf=True)): `write(text)` cuts host text into blocks of
    at most BGZF_BLOCK bytes and writes each as a BGZF member, `write_members(view)` appends the GPU's members, which are
    BGZF members under PF_GZ_BGZF, as they are, and `close` appends the 28-byte end-of-file member: htslib's readers and
    this project's device decoder walk the file by its BSIZE chain."""

    def _take(self, b):
        data = memoryview(b)
        n = 0
        for at in range(0, data.nbytes, BGZF_BLOCK):
            member = bgzf_member(bytes(data[at:at + BGZF_BLOCK]), self.level)
            self.fh.write(member)
            n += len(member)
        if self.header_bytes is None:
            self.header_bytes = n
        else:
            self.host_bytes += n
        self.bytes_written += n

    def _finish(self):
        self.fh.write(BGZF_EOF)
        self.bytes_written += len(BGZF_EOF)

    def _is_empty(self):
        return False                     # (the end marker is a member: the file is a valid gzip stream as it is)


class SmallMemberGzipWriter(_GzipWriter):
    """A .gz file every member of which the device decoder takes (pf_gunzip_device): panfeed-get-kmers --gz-output's.
    `write_members(view)` appends the GPU's members as they are; `write(text)` takes text made on the host -- the header
    line, what pandas printed -- and compresses it into members of at most `chunk_bytes` of text each, the file's first
    line in a member of its own.  Every member starts with the same eight bytes (FLG = 0, MTIME = 0), which is how the
    decoder finds them.  Host text is held back until a member's worth has gathered, and goes out in front of the next
    members or at close; a file nothing was written to is one empty member.  part: the file is a piece of such a file
    (a rank's share of a sharded run's, sharded.ShardWriter) -- its first line is a line like any other, and a part nothing
    was written to stays empty."""

    def __init__(self, path, chunk_bytes, compresslevel=6, part=False):
        super().__init__(path, compresslevel)
        self.chunk, self.part = int(chunk_bytes), bool(part)
        self.held = b""                          # host text not yet in a member
        self.first_line = not self.part          # the file's first line has not gone out yet
        self.bytes_written = self.text_bytes = self.host_members = 0

    def _member(self, text):
        member = self._compress(text)
        self.fh.write(member)
        self.bytes_written += len(member)
        self.text_bytes += len(text)
        self.host_members += 1

    def _emit(self, everything):
        data, at = memoryview(self.held), 0
        if self.first_line and data.nbytes:
            nl = self.held.find(b"\n")
            if nl < 0 and not everything:
                return
            at = nl + 1 if nl >= 0 else data.nbytes
            for a in range(0, at, self.chunk):   # (a first line over a member's size takes several)
                self._member(data[a:min(at, a + self.chunk)])
            self.first_line = False
        while data.nbytes - at >= (1 if everything else self.chunk):
            self._member(data[at:at + self.chunk])
            at += self.chunk
        self.held = bytes(data[at:])

    def _take(self, b):
        self.held = self.held + b if self.held else b
        if self.first_line or len(self.held) >= self.chunk:
            self._emit(False)

    def write_members(self, view):
        if len(view):
            self._emit(True)
            self.first_line = False
            self.fh.write(view)
            self.bytes_written += len(view)

    def _finish(self):
        self._emit(True)

    def _is_empty(self):
        return not self.bytes_written and not self.part


def _create(output, name, compress, device_gzip, bgzf=False):
    """the file `name` of an output directory: `name`.gz under device_gzip -- a writer that also takes the GPU's members,
    BGZF ones under bgzf -- or under compress, else a text file"""
    if device_gzip:
        return (BgzfMemberWriter if bgzf else MemberGzipWriter)(os.path.join(output, name + ".gz"))
    if compress:
        return ParallelGzipWriter(os.path.join(output, name + ".gz"), compresslevel=9)
    return open(os.path.join(output, name), "w")


def create_kmer_stroi(output, compress=False, device_gzip=False, bgzf=False):
    """kmers.tsv[.gz] with its header written (input.py:235-247).  device_gzip: a writer that also takes the GPU's
    members; bgzf: as BGZF."""
    fh = _create(output, "kmers.tsv", compress, device_gzip, bgzf)
    fh.write(KMERS_TSV_HEADER)
    fh.flush()
    return fh


def create_hash_files(output, compress=False, device_gzip=False, bgzf=False):
    """(hashes_to_patterns, kmers_to_hashes) handles, no headers yet (input.py:249-259)."""
    return (_create(output, "hashes_to_patterns.tsv", compress, device_gzip, bgzf),
            _create(output, "kmers_to_hashes.tsv", compress, device_gzip, bgzf))


def write_headers(hash_pat, kmer_hash, genepres):
    """panfeed.py:116-129; `genepres` only needs `.columns` (the strain names)."""
    write_strain_headers(hash_pat, kmer_hash, list(genepres.columns))


def write_strain_headers(hash_pat, kmer_hash, strains):
    """write_headers for callers that have the strain names and no table"""
    hash_pat.write(hashes_to_patterns_header(strains))
    hash_pat.flush()
    kmer_hash.write(KMERS_TO_HASHES_HEADER)
    kmer_hash.flush()


def write_cluster_dir(output, idx, strains, kmers_tsv, kmers_to_hashes, hashes_to_patterns, compress=False, device_gzip=False):
    """--multiple-files: the three files of gene cluster `idx`, headers and all, in `<output>/<idx>/`
    (panfeed.py:38-43, 159-167).  The bodies: str, or the bytes-like text the GPU wrote (slices of a batch's device
    text).  kmers_tsv None: `kmers.tsv` has been written already, by a ClusterKmersFiles sink.
    device_gzip: `.gz` files made of members (MemberGzipWriter) -- the header line is a member the host makes, a body that
    is a GzipMembers (Engine(device_gzip_clusters=True)) is appended as it is, a body that is text becomes a member made
    here.  Returns the bytes of those host-made members behind the headers (0 without device_gzip)."""
    path = os.path.join(output, idx)
    os.makedirs(path, exist_ok=True)
    files = []
    if kmers_tsv is not None:
        ks = create_kmer_stroi(path, compress, device_gzip)
        write_text(ks, kmers_tsv)
        files.append(ks)
    hash_pat, kmer_hash = create_hash_files(path, compress, device_gzip)
    write_strain_headers(hash_pat, kmer_hash, strains)
    write_text(hash_pat, hashes_to_patterns)
    write_text(kmer_hash, kmers_to_hashes)
    files += [hash_pat, kmer_hash]
    for fh in files:
        fh.close()
    return sum(fh.host_bytes for fh in files) if device_gzip else 0


def write_cluster_dirs(output, strains, out, compress=False, device_gzip=False):
    """write_cluster_dir for every cluster of a multiple_files batch (`out`: its BatchOutput); returns their sum"""
    return sum(write_cluster_dir(output, idx, strains, kt, kh, hp, compress, device_gzip) for idx, kt, kh, hp in out.per_cluster)


class _ClusterCursor:
    """What the two splitters share: `ends[i]` is the offset just behind cluster `names[i]`'s bytes in the whole text
    (non-decreasing); the cluster the next byte belongs to, and whether it has had a call; `close()` checks that the
    text reached the last end and gives every cluster left its call -- with `_empty()` where it has no byte."""

    def __init__(self, ends, names, sink):
        self.ends, self.names, self.sink = [int(e) for e in ends], list(names), sink
        if len(self.ends) != len(self.names) or any(b < a for a, b in zip(self.ends, self.ends[1:])):
            raise ValueError("one end per cluster, non-decreasing")
        self.at = 0             # text bytes taken so far
        self.cluster = 0        # the cluster the next byte belongs to, if it has any left
        self.called = False     # whether that cluster has had a call

    def _next_cluster(self):
        if not self.called:
            self.sink(self.names[self.cluster], self._empty())
        self.cluster += 1
        self.called = False

    def close(self):
        if self.ends and self.at != self.ends[-1]:
            raise ValueError(f"the text ended at byte {self.at}, the last cluster's end is {self.ends[-1]}")
        while self.cluster < len(self.ends):
            self._next_cluster()


class ClusterSplitter(_ClusterCursor):
    """Cuts a text that arrives block by block (a batch's kmers.tsv rows as they leave the device) into its clusters'
    shares: `ends[i]` is the offset just behind cluster `names[i]`'s bytes in the whole text (non-decreasing).  Call it
    with every block, in order, then `close()`: `sink(name, piece)` is called at least once for every cluster, in order,
    with an empty piece where a cluster has no byte.  Blocks and ends fall wherever they fall; a piece is a slice of the
    block it came in, valid as long as that is."""

    def _empty(self):
        return b""

    def __call__(self, block):
        view = memoryview(block)
        off, n = 0, len(view)
        while off < n:
            while self.cluster < len(self.ends) and self.ends[self.cluster] <= self.at:
                self._next_cluster()
            if self.cluster == len(self.ends):
                raise ValueError(f"{n - off} bytes of text behind the last cluster's end")
            take = min(n - off, self.ends[self.cluster] - self.at)
            self.sink(self.names[self.cluster], view[off:off + take])
            self.called = True
            off += take
            self.at += take


class ClusterMemberSplitter(_ClusterCursor):
    """ClusterSplitter for a text that arrives as gzip members (the kmers.tsv stream under device gzip, told the clusters'
    ends by pf_kmers_tsv_stream_cuts): a member cannot be cut, so every block comes with the places where the ends fall
    in it.  Call it with every block, in order -- `(members, text_off, text_bytes, cuts)`: the block's members, the text
    they decode to as an offset into the whole text and a size, and `(text offset, member offset)` of every cluster end
    strictly inside that text, ascending -- then `close()`.  `sink(name, GzipMembers(piece, text bytes))` is called with
    whole members only, at least once for every cluster, in order, with an empty piece where a cluster has no byte.
    ValueError where the pieces do not add up: a block out of place, a cut outside its block, a piece over a cluster's
    end, text missing at the close."""

    def _empty(self):
        return GzipMembers(memoryview(b""), 0)

    def __call__(self, members, text_off, text_bytes, cuts=()):
        view = memoryview(members)
        text_off, text_bytes = int(text_off), int(text_bytes)
        if text_off != self.at:
            raise ValueError(f"a block of the text from byte {text_off}, the text so far ends at byte {self.at}")
        points = [(text_off, 0)] + [(int(t), int(m)) for t, m in cuts] + [(text_off + text_bytes, len(view))]
        for (t0, m0), (t1, m1) in zip(points, points[1:]):
            if t1 < t0 or m1 < m0 or (t1 == t0) != (m1 == m0):
                raise ValueError(f"text bytes {t0}..{t1} in member bytes {m0}..{m1} of a block of {len(view)}: not a piece")
            if t1 == t0:
                continue
            while self.cluster < len(self.ends) and self.ends[self.cluster] <= t0:
                self._next_cluster()
            if self.cluster == len(self.ends):
                raise ValueError(f"{t1 - t0} bytes of text behind the last cluster's end")
            if t1 > self.ends[self.cluster]:
                raise ValueError(f"members of text bytes {t0}..{t1} pass the end of cluster {self.names[self.cluster]} "
                                 f"at byte {self.ends[self.cluster]}")
            self.sink(self.names[self.cluster], GzipMembers(view[m0:m1], t1 - t0))
            self.called = True
        self.at = text_off + text_bytes


class ClusterKmersFiles:
    """A cluster_targets_sink (Engine.run_batches) that writes `<output>/<idx>/kmers.tsv[.gz]`: the file is made, header
    first, at a cluster's first call and closed when the next cluster's first call comes, or by `close()` -- the calls of
    one cluster stand together.  `bytes`: the rows written so far.  device_gzip: the files are MemberGzipWriters -- a
    block that is a GzipMembers is appended as it is, text becomes a member made here; `host_bytes`: the bytes of those
    host-made members behind the headers, in the files closed so far."""

    def __init__(self, output, compress=False, device_gzip=False):
        self.output, self.compress, self.device_gzip = output, compress, device_gzip
        self.idx, self.fh = None, None
        self.bytes = self.host_bytes = 0

    def __call__(self, idx, block):
        if self.fh is None or idx != self.idx:
            self.close()
            path = os.path.join(self.output, idx)
            os.makedirs(path, exist_ok=True)
            self.idx, self.fh = idx, create_kmer_stroi(path, self.compress, self.device_gzip)
        write_text(self.fh, block)
        self.bytes += text_len(block)

    def close(self):
        if self.fh is not None:
            self.fh.close()
            if self.device_gzip:
                self.host_bytes += self.fh.host_bytes
            self.fh = None


def write_text(fh, data):
    """`data` -- str, or the bytes-like text the GPU wrote -- into `fh`: a text file, a binary file or a
    ParallelGzipWriter.  Bytes go straight into a text file's binary layer.  Gzip members the GPU made (a GzipMembers:
    the batch output says what it carries, the bytes are not looked at) are appended by a MemberGzipWriter as they are."""
    if isinstance(data, GzipMembers):
        fh.write_members(data.view)
    elif isinstance(data, str):
        fh.write(data.encode() if isinstance(fh, io.BufferedIOBase) else data)
    elif len(data):
        raw = getattr(fh, "buffer", None)
        if raw is not None:
            fh.flush()
            raw.write(data)
        else:
            fh.write(data)
