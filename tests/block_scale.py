"""Tables at the product's block size for the downstream text path (the row pack, its hand-out, the join's gzip slices and
the device text feed of csrc/pf_rowfilter.hip), the constants they stand on, and what every pass over them must give.

TEST INFRASTRUCTURE: pure Python on `bytes`.  Nothing here calls the library.  The downstream tools read their tables in
blocks of 256 MiB, and several steps of the path are capped or two-level by a compile-time constant that no argument
shrinks: row_tiles_kernel is one workgroup of 256 threads (a thread sums ceil(tiles / 256) tiles), row_write_kernel is
launched with at most 256 * 32 workgroups (a second sweep of its grid-stride loop from 524 288 rows on), RowHandout hands
out ROW_PIECE bytes at a time through two pinned buffers, kj_next_members encodes PfGzEncoder::BLOCK bytes of text a slice,
and TextFeed::plan takes PfGzDecoder::MAX_MEMBERS members and MAX_TEXT bytes of text a call.  The constants are mirrored
here (`MIRROR`, held against the source text by `source_constants`) and every case is built to cross one of them.

No expected text comes from a full run of a model: the rows are made one by one and their fate is known as they are made
(a model -- assoc_tables.may_pass / classify -- is asked once per distinct cell; the join's output row is put together
from the pieces of the row it was made of; a periodic member file's answer is the models' answer on one period,
replicated).  tests/test_block_scale.py (CPU) holds every case to its claimed quantity and the shortcut to the models
(assoc_tables.scan, join_tables.join_rows / kept_rows, text_tables.filter_rows); tests/test_gpu_block_scale.py holds the
kernels to the cases."""
import os
import re
import struct
import sys
from collections import namedtuple

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import assoc_tables as at  # noqa: E402
import bgzf_cases as bc  # noqa: E402
import inflate_cases as ic  # noqa: E402
import join_tables as jt  # noqa: E402
import text_tables as tt  # noqa: E402

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# ----------------------------------------------------------------------------------------------- mirrored constants
MIRROR = {
    "ROW_TILE_VECS": 4096, "ROW_GROUP": 16, "ROW_PIECE": 32 << 20,
    "WRITE_WORKGROUPS": 256 * 32, "WRITE_THREADS": 256,        # row_write_kernel's launch cap and its workgroup
    "TILES_THREADS": 256,                                      # row_tiles_kernel's one workgroup
    "GZ_BLOCK": 64 << 20,                                      # PfGzEncoder::BLOCK
    "MAX_TEXT": 256 << 20,                                     # PfGzDecoder::MAX_TEXT
    "BGZF_MAX_TEXT": 65536,
}
# expressions the cases rest on: the source must still hold them, letter for letter
SOURCE_LINES = {
    "pf_rowfilter.hip": [
        "inline uint32_t row_tiles(uint64_t n) { return (uint32_t)(((n + 15) / 16 + ROW_TILE_VECS - 1) / ROW_TILE_VECS); }",
        "const uint64_t per = (n + 255) / 256, lo = threadIdx.x * per, hi = lo + per < n ? lo + per : n;",
        "const uint64_t wave = ((uint64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6, n_waves = ((uint64_t)gridDim.x * blockDim.x) >> 6;",
        "for (uint64_t g = wave * ROW_GROUP; g < n_rows; g += n_waves * ROW_GROUP) {",
        "const uint64_t groups = (*n_rows + ROW_GROUP - 1) / ROW_GROUP;",
        "PinBuf pin[2];",
        "flying = std::min<uint64_t>(ROW_PIECE, bytes - pos);",
        "const uint64_t m = std::min<uint64_t>(PfGzEncoder::BLOCK, j->pack.out.bytes - j->gz_at), cap = PfGzEncoder::bound(m);",
        "while (c.take < c.ms.size() && c.take < PfGzDecoder::MAX_MEMBERS) {",
        "if (c.take && c.text_n + c.ms[c.take].isize > PfGzDecoder::MAX_TEXT) break;",
        "c.used = all ? listed : c.ms[c.take].at;",
    ],
    "pf_deflate.h": [
        "static constexpr uint32_t MAX_MEMBERS = (uint32_t)(MAX_TEXT / pfgz::CHUNK);",
    ],
    "pf_api.hip": [
        "for (k = 0; i + k < ms.size() && k < PfGzDecoder::MAX_MEMBERS && (!k || part + ms[i + k].isize <= PfGzDecoder::MAX_TEXT); k++)",
    ],
}


def _read(name):
    with open(os.path.join(REPO, "panfeed_amd", "csrc", name)) as f:
        return f.read()


def source_constants():
    """the mirrored numbers as the source states them today, and the restated expressions it no longer holds"""
    texts = {name: _read(name) for name in SOURCE_LINES}
    rf, dh = texts["pf_rowfilter.hip"], texts["pf_deflate.h"]

    def find(text, pattern):
        m = re.search(pattern, text)
        assert m, f"{pattern} not found"
        return m.groups()

    def shifted(text, pattern):                        # "32ull << 20"
        a, b = find(text, pattern)
        return int(a) << int(b)

    out = {}
    out["ROW_TILE_VECS"] = int(find(rf, r"constexpr uint32_t ROW_TILE_VECS = (\d+);")[0])
    out["ROW_GROUP"] = int(find(rf, r"constexpr uint32_t ROW_GROUP = (\d+);")[0])
    out["ROW_PIECE"] = shifted(rf, r"constexpr uint64_t ROW_PIECE = (\d+)ull << (\d+);")
    a, b, threads = find(rf, r"hipLaunchKernelGGL\(row_write_kernel, dim3\(\(uint32_t\)std::min<uint64_t>\(\(groups \+ 3\) / 4, "
                             r"(\d+) \* (\d+)\)\), dim3\((\d+)\)")
    out["WRITE_WORKGROUPS"], out["WRITE_THREADS"] = int(a) * int(b), int(threads)
    out["TILES_THREADS"] = int(find(rf, r"hipLaunchKernelGGL\(row_tiles_kernel, dim3\(1\), dim3\((\d+)\)")[0])
    out["GZ_BLOCK"] = shifted(dh, r"static constexpr uint64_t BLOCK = (\d+)ull << (\d+);")
    out["MAX_TEXT"] = shifted(dh, r"static constexpr uint64_t MAX_TEXT = (\d+)ull << (\d+);")
    out["BGZF_MAX_TEXT"] = int(find(dh, r"BGZF_MAX_TEXT = (\d+);")[0])
    gone = [f"{name}: {ln}" for name, lines in SOURCE_LINES.items() for ln in lines if ln not in texts[name]]
    return out, gone


M = MIRROR
TILE = M["ROW_TILE_VECS"] * 16                                              # bytes of text a workgroup of a plan kernel owns
SWEEP = M["WRITE_WORKGROUPS"] * (M["WRITE_THREADS"] // 64) * M["ROW_GROUP"]   # rows one sweep of the writer's grid takes
ROW_PIECE, GZ_BLOCK, MAX_TEXT = M["ROW_PIECE"], M["GZ_BLOCK"], M["MAX_TEXT"]


def row_tiles(n):
    return ((n + 15) // 16 + M["ROW_TILE_VECS"] - 1) // M["ROW_TILE_VECS"]


def tiles_per_thread(tiles):
    return (tiles + M["TILES_THREADS"] - 1) // M["TILES_THREADS"]


def max_members(chunk):
    """PfGzDecoder::MAX_MEMBERS for CHUNK = pf_gzip_device_chunk_bytes()"""
    return MAX_TEXT // chunk


# ----------------------------------------------------------------------------------------------- associations tables
THR = 0.05
# p-value cells, (one the filter keeps, one of the same length it drops) at THR: a row's length does not depend on its fate
PVALUE_PAIRS = ((b"0.01", b"0.90"), (b"1e-9", b"1e+1"), (b"5E-02", b"6E-02"), (b"0", b"3"), (b"0.05", b"0.06"), (b"-0", b"NA"))
LONG_NOTES = (b"", b"bad-chisq-in-the-fit-of-this-pattern", b"NA", b"high-bse-and-a-remark-as-long-as-that")

AfCase = namedtuple("AfCase", "name text thr keep kept classes flags rows n_kept")
# text: the table, header line first; keep: a byte per data row, 1 where the filter keeps it; kept: the kept lines joined


class _Decide:
    """a model's answer per distinct cell, asked once"""

    def __init__(self, thr):
        self.thr, self.passes, self.classes, self.asked = thr, {}, {}, 0

    def may_pass(self, cell):
        if cell not in self.passes:
            self.passes[cell] = at.may_pass(cell, self.thr)
            self.asked += 1
        return self.passes[cell]

    def classify(self, cell):
        if cell not in self.classes:
            self.classes[cell] = at.classify(cell)
        return self.classes[cell]


def _af_case(name, rows, keep, decide):
    """the case of these data rows (no newlines): the classes from every distinct cell of every column"""
    n_fields = len(at.HEADER.split(b"\t"))
    distinct = [set() for _ in range(n_fields)]
    for r in rows:
        for col, cell in zip(distinct, r.split(b"\t")):
            col.add(cell)
    classes = [0] * n_fields
    for i, col in enumerate(distinct):
        for cell in col:
            classes[i] |= decide.classify(cell)
    text = at.HEADER + b"\n".join(rows) + b"\n"
    kept = b"".join(r + b"\n" for r, k in zip(rows, keep) if k)
    return AfCase(name, text, decide.thr, bytes(keep), kept, classes, 0, len(rows), sum(keep))


def af_tiles_257():
    """data lines of 256 tiles and a few hundred bytes: row_tiles_kernel's threads sum two tiles each (per = 2), the last
    working thread one, the others none.  One row in 4 001 is kept, and so are the first row, the rows that lie across the
    starts of tiles 255 and 256, every row of the last tile and the last row"""
    decide = _Decide(THR)
    t255, t256 = 255 * TILE, 256 * TILE
    rows, keep, pos, i = [], bytearray(), 0, 0
    while pos < t256 + 200:
        good, bad = PVALUE_PAIRS[i % len(PVALUE_PAIRS)]
        row = at._row(i, bad, variant=b"H%07dabcdefghijklmnopq==" % i)
        end = pos + len(row) + 1
        if i % 4001 == 0 or pos <= t255 < end or pos <= t256 < end or pos >= t256:
            row = at._row(i, good, variant=b"H%07dabcdefghijklmnopq==" % i)
        rows.append(row)
        keep.append(decide.may_pass(row.split(b"\t")[at.PVALUE_FIELD]))
        pos, i = end, i + 1
    return _af_case("af_tiles_257", rows, keep, decide)


def af_sweep_and_pieces():
    """one table whose kept rows are more than one sweep of the writer's grid and whose kept bytes are more than two
    pieces of the hand-out; every seventh row is dropped, so every later row's place depends on the counts before it.
    Over 1 000 tiles: row_tiles_kernel's threads sum five each, and the tile count is no multiple of five"""
    decide = _Decide(THR)
    rows, keep, pos, i, n_kept, kept_bytes = [], bytearray(), 0, 0, 0, 0
    while True:
        tiles = row_tiles(pos)
        if n_kept >= SWEEP + 17 and kept_bytes >= 2 * ROW_PIECE + 1 and tiles % tiles_per_thread(tiles):
            break
        good, bad = PVALUE_PAIRS[i % len(PVALUE_PAIRS)]
        cell = bad if i % 7 == 3 else good
        row = at._row(i, cell, variant=b"H%07d-abcdefghijklmnopqrstuvwxyz012345==" % i, notes=LONG_NOTES[i % 4])
        k = decide.may_pass(cell)
        rows.append(row)
        keep.append(k)
        pos += len(row) + 1
        if k:
            n_kept, kept_bytes = n_kept + 1, kept_bytes + len(row) + 1
        i += 1
    return _af_case("af_sweep_and_pieces", rows, keep, decide)


# ----------------------------------------------------------------------------------------------- kmers.tsv tables
KJ_KEY = (b"sel", b"ACG")
KJ_CLUSTERS = [(b"sel", 0), (b"oth", 1)]
KjCase = namedtuple("KjCase", "name header body keys text0 text1 empty want rows unmatched")
# want: {0: the join under rendering 0, 1: under rendering 1, 2: the raw rows that have a key} of bunch 0 (`sel`)


def _kj_out(row, kmer, text):
    """the join's row of a plain row of `sel` with a three-letter k-mer: cluster, k-mer, text, fields 1 .. 9"""
    return b"sel\t" + kmer + b"\t" + text + b"\t" + row[4:-4] + b"\n"


def kj_rows_sweep():
    """a kmers.tsv body in which bunch 0 (`sel`) has one sweep of the writer's grid and 17 rows; every fifth row is of `oth`
    (bunch 1) or of `zz` (not selected); every other row of `sel` has the key (sel, ACG).  Over 256 tiles of input"""
    body, want, sel, keyed, i = [], {0: [], 1: [], 2: []}, 0, 0, 0
    while sel < SWEEP + 17:
        if i % 5 == 4:
            body.append(jt.kmers_row(("oth", "zz")[(i // 5) % 2], "ACG" if i % 2 else "TTT", i) + b"\n")
        else:
            has_key = sel % 2 == 1
            kmer = "ACG" if has_key else "TTT"
            row = jt.kmers_row("sel", kmer, i)
            body.append(row + b"\n")
            want[0].append(_kj_out(row, kmer.encode(), b"t0" if has_key else b""))
            want[1].append(_kj_out(row, kmer.encode(), b"t1.0" if has_key else b""))
            if has_key:
                want[2].append(row + b"\n")
                keyed += 1
            sel += 1
        i += 1
    return KjCase("kj_rows_sweep", jt.KMERS_HEADER, b"".join(body), [KJ_KEY], [b"t0"], [b"t1.0"], b"",
                  {m: b"".join(w) for m, w in want.items()}, sel, sel - keyed)


def kj_long_texts(n_rows=20000):
    """rows of `sel` that all have the one key, whose two rendered texts are 3 500 and 3 501 printable bytes: more output
    than PfGzEncoder::BLOCK, so three pieces or more by the plain hand-out and two encoder slices by the gzip route"""
    t0 = bytes(33 + (j * 7 + j // 90) % 90 for j in range(3500))
    t1 = t0 + b"~"
    assert b"\t" not in t1 and b"\n" not in t1 and all(32 < c < 127 for c in t1)
    body, want = [], {0: [], 1: [], 2: []}
    for i in range(n_rows):
        row = jt.kmers_row("sel", "ACG", i)
        body.append(row + b"\n")
        want[0].append(_kj_out(row, b"ACG", t0))
        want[1].append(_kj_out(row, b"ACG", t1))
        want[2].append(row + b"\n")
    return KjCase("kj_long_texts", jt.KMERS_HEADER, b"".join(body), [KJ_KEY], [t0], [t1], b"",
                  {m: b"".join(w) for m, w in want.items()}, n_rows, 0)


# ----------------------------------------------------------------------------------------------- member files
RF_HEADER = b"first\tmiddle\tlast\n"
RF_KEYS = tt.RF_KEYS
_RF_FIELDS = RF_KEYS + (b"abc", b"a", b"", b"zz", RF_KEYS[1] + b"!", RF_KEYS[2][:-1])
_AF_CELLS = (b"0.01", b"0.90", b"1e-9", b"0.06", b"5E-02", b"3", b"NA", b"0.05", b"1e+1", b"0")
_AF_CELLS_ABOVE = (b"0.90", b"0.06", b"3", b"NA", b"1e+1", b"0.0500001", b"7E-02")
UNIT = 20                                            # bytes of text per member of `members_over_the_count`
PERIODS = 2048                                       # (A, B) pairs of `members_over_the_text`


def rf_line(i, pad=0, sparse=False):
    """line i of the three-column table: key fields and near misses in its first and in its last field; `sparse`: near
    misses alone in 39 lines of 40, so that 256 MiB of them keep a few MB"""
    fields = _RF_FIELDS[len(RF_KEYS):] if sparse and i % 40 else _RF_FIELDS
    n = len(fields)
    return fields[i % n] + b"\tm%d" % i + b"p" * pad + b"\t" + fields[(i // n + 2 * i) % n] + b"\n"


def af_line(i, pad=0, sparse=False):
    """line i of the associations table: the numbers repeat every 64 lines, the variant does not; `sparse` as rf_line's"""
    cells = _AF_CELLS_ABOVE if sparse and i % 40 else _AF_CELLS
    return at._row(i % 64, cells[i % len(cells)], variant=b"V%07d==" % i, notes=(b"", b"note", b"NA", b"n")[i % 4] + b"p" * pad) + b"\n"


def _sparse(line):
    return lambda i, pad=0: line(i, pad, sparse=True)


def exact_lines(line, total, first=0):
    """complete lines line(first), line(first + 1), ... of exactly `total` bytes together: the last one padded"""
    out, n, i = [], 0, first
    assert total >= 400
    while total - n - len(line(i)) >= 200:
        out.append(line(i))
        n += len(out[-1])
        i += 1
    out.append(line(i, total - n - len(line(i))))
    text = b"".join(out)
    assert len(text) == total and text.endswith(b"\n")
    return text


def rf_expect(text, first_field):
    """the row filter's rows of a table's text, header line first"""
    return tt.filter_rows(text[text.index(b"\n") + 1:], RF_KEYS, first_field)


def af_expect(text):
    return at.scan(text, at.PVALUE_FIELD, THR)


def bgzf_offsets(data):
    """where the members of a BGZF file start, by the BSIZE chain alone"""
    out, pos = [], 0
    while pos < len(data):
        out.append(pos)
        pos += struct.unpack_from("<H", data, pos + 16)[0] + 1
    assert pos == len(data)
    return out


def plain_offsets(data):
    """where the members of a file of plain-header members start"""
    out, pos = [], 0
    while pos >= 0:
        out.append(pos)
        pos = data.find(ic.HEAD[:8], pos + 1)
    return out


MemberFile = namedtuple("MemberFile", "name table text plain bgzf n_members")
# table: "rf" or "af"; text: header line first; plain / bgzf: the two spellings (None where there is none); n_members: the
# members that hold text, the header line's among them (the BGZF spelling has its end marker behind them)


def members_over_the_count(table, chunk):
    """the header line's member, then 2 * MAX_MEMBERS + 5 members of 20 bytes of text each: three calls of the feed, both
    call seams inside a line, most lines across a member seam.  The last line, which the filter keeps, is the third call's"""
    header, line = (RF_HEADER, rf_line) if table == "rf" else (at.HEADER, af_line)
    last = RF_KEYS[0] + b"\tthe last line of the file, in the third call\t" + RF_KEYS[0] + b"\n" if table == "rf" else at._row(3, b"0.01", variant=b"Vlast==") + b"\n"
    n = 2 * max_members(chunk) + 5
    body = exact_lines(line, n * UNIT - len(last)) + last
    assert 2 * UNIT < len(last) < 5 * UNIT
    parts = [header] + [body[k:k + UNIT] for k in range(0, len(body), UNIT)]
    assert len(parts) == n + 1
    return MemberFile(f"members_over_the_count[{table}]", table, header + body, b"".join(ic.zlib_member(p, 6) for p in parts),
                      b"".join(bc.member(p) for p in parts) + bc.EOF, n + 1)


def count_seams(mf, chunk):
    """the text offsets at which the feed's first and second call end: MAX_MEMBERS members each, the header's among the first"""
    head = mf.text.index(b"\n") + 1
    first = head + (max_members(chunk) - 1) * UNIT
    return first, first + max_members(chunk) * UNIT


TextUnits = namedtuple("TextUnits", "table C A B straddler")


def text_units(table):
    """the three member texts of `members_over_the_text`, BGZF_MAX_TEXT bytes each: C the header line and complete lines, A
    complete lines and the first half of `straddler`, B its other half and complete lines.  The filter keeps `straddler`"""
    size = M["BGZF_MAX_TEXT"]
    if table == "rf":
        header, line = RF_HEADER, _sparse(rf_line)
        straddler = RF_KEYS[1] + b"\tthe-line-across-the-call-seam\t" + RF_KEYS[2] + b"\n"      # a key first and a key last
        cut = len(straddler) // 2
    else:
        header, line = at.HEADER, _sparse(af_line)
        straddler = at._row(7, b"0.0123", variant=b"Vacross-the-call-seam==") + b"\n"
        cut = sum(len(f) + 1 for f in straddler.split(b"\t")[:at.PVALUE_FIELD]) + 3             # inside the p-value cell
    c = header + exact_lines(line, size - len(header), first=0)
    a = exact_lines(line, size - cut, first=100000) + straddler[:cut]
    b = straddler[cut:] + exact_lines(line, size - (len(straddler) - cut), first=200000)
    assert len(c) == len(a) == len(b) == size
    return TextUnits(table, c, a, b, straddler)


def members_over_the_text(table):
    """BGZF: C, then (A, B) 2 048 times, then the end marker: 4 097 members of 64 KiB of text each, 256 MiB + 64 KiB.  A
    call of the feed takes 4 096 of them: member 4 095 is an A, so the call seam lies inside the straddling line"""
    u = text_units(table)
    data = bc.member(u.C) + (bc.member(u.A) + bc.member(u.B)) * PERIODS + bc.EOF
    return u, data


def over_the_text_expect(u):
    """what a pass over `members_over_the_text` gives, from the models' answers on one period: the row filter's rows by its
    first and by its last field, or the associations filter's Scan"""
    if u.table == "rf":
        return {first: rf_expect(u.C, first) + PERIODS * tt.filter_rows(u.A + u.B, RF_KEYS, first) for first in (True, False)}
    c, ab = af_expect(u.C), af_expect(at.HEADER + u.A + u.B)
    return at.Scan(c.kept + PERIODS * ab.kept, [x | y for x, y in zip(c.classes, ab.classes)], c.flags | ab.flags,
                   c.rows + PERIODS * ab.rows, c.n_kept + PERIODS * ab.n_kept)
