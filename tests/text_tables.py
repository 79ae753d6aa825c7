"""The two text scanners of csrc/pf_rowfilter.hip, stated without the library: which lines of a tab-separated table a
set of keys selects (rowfilter_kernel behind RowFilter), what panfeed-plot's table scan keeps of an annotated k-mer table
(pg_scan_kernel and its table kernels behind GridBuilder), a classifier of where a line and its key field lie in the
16-byte vectors and 32-bit words the kernels read, and the case lists that put lines on every such place.

TEST INFRASTRUCTURE: pure Python on `bytes`.  Nothing here calls the library, pandas or the package's own parsing, and
nothing is derived from panfeed_amd/csrc: tests/test_text_tables.py (CPU) holds these models against pandas and checks
that the case lists reach every class, tests/test_gpu_text_tables.py holds the kernels against the models.

A table is split on b"\\n" and b"\\t" only: carriage returns, quotes and every other byte are ordinary bytes of a field.
"""
import math
import re
from collections import namedtuple

MAX_FIELD = 4096            # the documented limit of both scanners: a field of 4 096 bytes or more is never a key field
INT32 = 2 ** 31 - 1


# ------------------------------------------------------------------------------------------------ row filter model
def as_file(text):
    """the lines a reader of a file with these bytes sees: a last line without its newline is given one"""
    return text if not text or text.endswith(b"\n") else text + b"\n"


def lines_of(text):
    """the complete lines of `text`, without their newline; what follows the last newline is not a line"""
    return text.split(b"\n")[:-1]


def filter_rows(text, keys, first_field):
    """the lines of `text`, each with its newline and joined, whose first (or last) field is one of `keys`"""
    ks = {bytes(k) for k in keys if len(k) < MAX_FIELD}
    out = []
    for ln in lines_of(text):
        fields = ln.split(b"\t")
        f = fields[0] if first_field else fields[-1]
        if len(f) < MAX_FIELD and f in ks:
            out.append(ln + b"\n")
    return b"".join(out)


def blocks_of(body, block_bytes):
    """the blocks of complete lines a reader hands on that reads `block_bytes` at a time and carries what follows a
    block's last newline over to the next; a read that completes no line hands on nothing"""
    out, have = [], b""
    for at in range(0, len(body), block_bytes):
        chunk = have + body[at:at + block_bytes]
        cut = chunk.rfind(b"\n") + 1
        if cut:
            out.append(chunk[:cut])
        have = chunk[cut:]
    if have:
        out.append(have + b"\n")
    return out


# ------------------------------------------------------------------------------------------------ plot scan model
Cell = namedtuple("Cell", "count letters texts")            # rows, the letter of each row (file order), set of p-value texts
PlotModel = namedtuple("PlotModel", "clusters cells texts lines records")
# clusters: {name: (min, max, rows)}, min = max = None where rows == 0;  cells: {(name, strain id, gene_start): Cell}

_INT = re.compile(rb"[+-]?[0-9]+\Z")
_COMPLEMENT = {ord("A"): ord("T"), ord("T"): ord("A"), ord("G"): ord("C"), ord("C"): ord("G")}


class ModelArgumentError(ValueError):
    """an input the scan refuses as a whole: a gene_start outside 32 bits, a name or p-value text of 4 096 bytes or more"""


def letter_of(kmer, strand):
    if not kmer:
        return 0
    try:
        minus = float(strand) == -1
    except ValueError:
        minus = False
    if minus:
        return _COMPLEMENT.get(kmer.upper()[-1], ord("N"))
    return kmer.upper()[0]


def plot_model(text, columns, strains, start=None, stop=None):
    """what the plot scan keeps of the data lines `text` (no header line).  columns: the indices of cluster, strain,
    gene_start, k-mer, strand, p-value.  strains: the phenotype names (bytes); a repeated name keeps its first id."""
    ids = {}
    for i, s in enumerate(strains):
        ids.setdefault(bytes(s), i)
    clusters, cells, texts = {}, {}, set()
    lines = records = 0
    for ln in lines_of(text):
        if ln == b"":
            continue
        lines += 1
        f = ln.split(b"\t")
        if len(f) <= max(columns):
            continue                                            # too short: counted, not kept
        cluster, strain, pos, kmer, strand, pv = (f[c] for c in columns)
        if strain not in ids:
            continue
        if len(cluster) >= MAX_FIELD or len(pv) >= MAX_FIELD:
            raise ModelArgumentError("a cluster name or p-value text of 4 096 bytes or more")
        clusters.setdefault(cluster, [None, None, 0])
        if not _INT.match(pos):
            continue
        x = int(pos)
        if abs(x) > INT32:
            raise ModelArgumentError("a gene_start outside 32 bits")
        if start is not None and not (start <= x <= stop):
            continue
        c = clusters[cluster]
        c[0] = x if c[0] is None else min(c[0], x)
        c[1] = x if c[1] is None else max(c[1], x)
        c[2] += 1
        cell = cells.setdefault((cluster, ids[strain], x), Cell([0], [], set()))
        cell.count[0] += 1
        cell.letters.append(letter_of(kmer, strand))
        cell.texts.add(pv)
        texts.add(pv)
        records += 1
    return PlotModel({k: tuple(v) for k, v in clusters.items()},
                     {k: Cell(v.count[0], v.letters, v.texts) for k, v in cells.items()}, texts, lines, records)


def ieee_max(values):
    """the IEEE maximum of the non-NaN doubles among `values` (-0 below +0), None if there is none"""
    vals = [v for v in values if not math.isnan(v)]
    return max(vals, key=lambda v: (v, math.copysign(1.0, v))) if vals else None


# ------------------------------------------------------------------------------------------------ classifier
END_MOD = tuple(f"end%16={i}" for i in range(16))
NL_BYTE = ("nl_low", "nl_mid", "nl_top")                     # the line end as byte 0, 1 or 2, 3 of its 32-bit word
FIELD_SPAN = ("field_inside", "field_straddle", "field_span")
PLACE = ("first_in_block", "last_in_block", "alone_in_block")
KEY_RELATION = ("key_equal", "key_prefix_of_field", "field_prefix_of_key")
BLOCK_MOD = ("block%16=0", "block%16=1", "block%16=15")
OTHER = ("field_empty", "blank", "tabs_only")


def _field_extent(ln, at, field):
    """[begin, end) in the block of the line's key field: "first", "last" or a column index; None if the line has no
    such column"""
    f = ln.split(b"\t")
    if field == "first":
        return at, at + len(f[0])
    if field == "last":
        return at + len(ln) - len(f[-1]), at + len(ln)
    if field >= len(f):
        return None
    b = at + sum(len(x) + 1 for x in f[:field])
    return b, b + len(f[field])


def line_classes(block, keys=(), field="first"):
    """one frozenset per complete line of `block`, drawn from END_MOD, NL_BYTE, FIELD_SPAN, PLACE, KEY_RELATION and OTHER.
    The kernels read the block as 16-byte vectors of four 32-bit words from its first byte, so a position's place is its
    offset in the block.  field_inside: the key field lies in one vector; field_straddle: it crosses one vector boundary;
    field_span: it crosses two or more, so a whole vector lies inside it."""
    out, at = [], 0
    lines = lines_of(block)
    for i, ln in enumerate(lines):
        end = at + len(ln)                                      # the position of the line's newline
        cls = {END_MOD[end % 16], NL_BYTE[(0, 1, 1, 2)[end % 4]]}
        if i == 0:
            cls.add("first_in_block")
        if i == len(lines) - 1:
            cls.add("last_in_block")
        if len(lines) == 1:
            cls.add("alone_in_block")
        if ln == b"":
            cls.add("blank")
        elif ln.strip(b"\t") == b"":
            cls.add("tabs_only")
        ext = _field_extent(ln, at, field)
        if ext is not None:
            b, e = ext
            if b == e:
                cls.add("field_empty")
            else:
                cls.add(FIELD_SPAN[min(2, (e - 1) // 16 - b // 16)])
            f = block[b:e]
            for k in keys:
                if k == f:
                    cls.add("key_equal")
                elif f.startswith(k):
                    cls.add("key_prefix_of_field")
                elif k.startswith(f):
                    cls.add("field_prefix_of_key")
        out.append(frozenset(cls))
        at = end + 1
    return out


def block_classes(block):
    return frozenset(c for c in BLOCK_MOD if c == f"block%16={len(block) % 16}")


# ------------------------------------------------------------------------------------------------ row filter cases
BLOCK_SIZES = (16, 17, 31, 64, 257)                           # filter_file / scan_file block sizes of the alignment sweeps
RF_KEYS = (b"ab", b"Kq" * 10 + b"z", b"0123456789" * 4)       # 2, 21 and 40 bytes: inside, straddling, spanning
_RF_FIELDS = RF_KEYS + (b"abc", b"a", b"", b"zz", RF_KEYS[1] + b"!", RF_KEYS[2][:-1])


def rowfilter_alignment_text():
    """a table of a few KB whose first and last fields are keys, keys with a byte more or less, empty or other, behind
    and in front of middle fields of every length from 0 to 18; blank lines and lines of tabs at the start, inside and
    at the end; a line that is one field"""
    lines = [b"", b"\t", b"ab"]
    for pad in range(19):
        for j, first in enumerate(_RF_FIELDS):
            last = _RF_FIELDS[(j + pad) % len(_RF_FIELDS)]
            lines.append(first + b"\t" + b"m" * ((pad * 7 + j * 3) % 19) + b"\t" + last)
        lines += [b"", b"\t\t\t", RF_KEYS[pad % 3], b"\t" * (pad % 5 + 1)][:1 + pad % 4]
    lines += [b"\t\t", b""]
    return b"".join(ln + b"\n" for ln in lines)


SWEEP_KEY = b"Key7"


def _pad_for(at, r, fixed):
    """the length k >= 1 of a padding such that a line of k + `fixed` bytes (newline not counted) that begins at `at`
    has its newline at a position = r (mod 4)"""
    return (r - at - fixed) % 4 or 4


def rowfilter_byte_sweep_text():
    """for every byte c but tab and newline: four lines  c KEY \\t c<hex> \\t KEY , the newline in front of each at
    byte 0, 1, 2 and 3 of its 32-bit word (a filler line in front is padded to put it there), and one line whose first
    and last fields are KEY c; then two and three 0x0B bytes in front of the key, at the four places again.  The middle
    field names the case."""
    out = bytearray()

    def at_word_byte(r, line):
        out.extend(b"f" * _pad_for(len(out), r, 10) + b"\tq\tnomatch\n")
        assert (len(out) - 1) % 4 == r
        out.extend(line)

    for c in range(256):
        if c in (9, 10):
            continue
        for r in range(4):
            at_word_byte(r, bytes([c]) + SWEEP_KEY + b"\tc%02x\t" % c + SWEEP_KEY + b"\n")
        out.extend(SWEEP_KEY + bytes([c]) + b"\te%02x\t" % c + SWEEP_KEY + bytes([c]) + b"\n")
    for run in (2, 3):
        for r in range(4):
            at_word_byte(r, b"\x0b" * run + SWEEP_KEY + b"\trun%d\t" % run + SWEEP_KEY + b"\n")
    return bytes(out)


def sweep_case(line):
    """the case a line of a byte sweep belongs to: its middle field; the line itself if it is not such a line"""
    f = line.rstrip(b"\n").split(b"\t")
    return f[1] if len(f) == 3 else line


# ------------------------------------------------------------------------------------------------ plot scan cases
PLOT_HEADER = b"cluster\tstrain\tgene_start\tk-mer\tstrand\tlrt-pvalue\n"
PLOT_COLUMNS = [0, 1, 2, 3, 4, 5]
PLOT_STRAINS = (b"s0", b"s1", b"s22", b"t", b"u_long_strain_name", b"s5")
PLOT_NAME = b"Name"


def plot_alignment_text():
    """23 clusters whose names are 4 to 34 bytes long, rows on seven strains (one is no phenotype strain), 11 positions,
    five k-mers, both strands and nine p-value texts, so that cells hold one row and several; blank lines, lines of tabs
    and lines that are too short in between"""
    lines = [b"", b"\t\t\t\t\t"]
    for i in range(150):
        j = i % 23
        name = b"cl%02d" % j + b"n" * (j * 5 % 31)
        strain = (PLOT_STRAINS + (b"zz",))[i * 5 % 7]
        pos = b"%d" % (i * 3 % 11 - 4)
        kmers = (b"ACGT", b"cgta", b"N", b"tTgA", b"")
        lines.append(b"\t".join([name, strain, pos, kmers[i % 5], (b"1", b"-1")[i % 2], b"p%d" % (i % 9)]))
        for extra in range((0, 1, 0, 0, 0, 2, 0, 0)[i % 8]):              # a second and a third row of the same cell
            lines.append(b"\t".join([name, strain, pos, kmers[(i + extra) % 5], b"-1", b"p%d" % ((i + 4 * extra) % 9)]))
        if i % 29 == 7:
            lines += [b"", b"\t" * (i % 7 + 1), name + b"\ts0\t3"][:1 + i % 3]
    lines += [b"\t", b""]
    return b"".join(ln + b"\n" for ln in lines)


def plot_byte_sweep_text():
    """for every byte c of 0x01-0x7F but tab and newline: four rows of the cluster  c Name , the newline in front of each
    at byte 0, 1, 2 and 3 of its 32-bit word (a kept filler row of the cluster `fill` in front is padded to put it there);
    then two and three 0x0B bytes in front of the name"""
    out = bytearray()

    def rows(name, pos):
        for r in range(4):
            out.extend(b"fill\ts0\t0\t" + b"A" * _pad_for(len(out), r, 15) + b"\t1\tpf\n")
            assert (len(out) - 1) % 4 == r
            out.extend(b"\t".join([name, PLOT_STRAINS[r], b"%d" % pos, b"ACGT", b"1", b"pv"]) + b"\n")

    for c in range(1, 128):
        if c not in (9, 10):
            rows(bytes([c]) + PLOT_NAME, c)
    for run in (2, 3):
        rows(b"\x0b" * run + PLOT_NAME, 200 + run)
    return bytes(out)
