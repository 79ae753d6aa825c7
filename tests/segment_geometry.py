"""Segment geometry of the resident-genome path, stated without the library: the packed layout (2 bits per base, 32
bases per uint64 word, first base in bits 63:62, zero behind the last base), the case split of gather_segments_kernel
per destination word, and the case lists that reach every branch of the three kernels that fill and read the genome
store (genome_pack_kernel, genome_pack_text_kernel, gather_segments_kernel).

TEST INFRASTRUCTURE: numpy only.  Nothing here calls the library or the oracle, and nothing is derived from
panfeed_amd/csrc: tests/test_segment_geometry.py (CPU) holds this reference against the host packer and the one-pass
reader's host sink, tests/test_gpu_segment_geometry.py holds the kernels against it word for word.
"""
import os
from collections import namedtuple

import numpy as np

_CODE = np.full(256, 255, dtype=np.uint8)
for _i, _c in enumerate(b"ACGT"):
    _CODE[_c] = _i
    _CODE[_c | 0x20] = _i                      # lower case packs as upper case
_ACGT = np.frombuffer(b"ACGT", dtype=np.uint8)
_COMP = bytes.maketrans(b"ACGTacgt", b"TGCAtgca")


# ------------------------------------------------------------------------------------------------ reference
def pack(seq):
    """bytes / uint8 array of A/C/G/T (either case) -> ceil(len / 32) uint64 words: base j in bits 63 - 2 (j % 32) and
    62 - 2 (j % 32) of word j // 32, zero behind the last base.  Four codes make a byte by shifts, eight bytes a
    big-endian word."""
    raw = np.frombuffer(seq, dtype=np.uint8) if isinstance(seq, (bytes, bytearray, memoryview)) else np.asarray(seq, np.uint8)
    n = len(raw)
    c = np.zeros((n + 31) // 32 * 32, dtype=np.uint8)
    c[:n] = _CODE[raw]
    if n and int(c[:n].max()) > 3:
        raise ValueError("pack: a letter other than A/C/G/T")
    q = c.reshape(-1, 4)
    b = (q[:, 0] << 6) | (q[:, 1] << 4) | (q[:, 2] << 2) | q[:, 3]
    return np.ascontiguousarray(b).view(">u8").astype(np.uint64)


def unpack(words, word_off, start, n):
    """n upper-case letters from base `start` of the packed sequence whose words begin at word_off"""
    j = np.arange(start, start + n, dtype=np.uint64)
    w = np.asarray(words, dtype=np.uint64)[(np.uint64(word_off) + (j >> np.uint64(5))).astype(np.int64)]
    code = (w >> (np.uint64(62) - np.uint64(2) * (j & np.uint64(31)))) & np.uint64(3)
    return _ACGT[code.astype(np.int64)].tobytes()


def revcomp(seq):
    return bytes(seq)[::-1].translate(_COMP)


def segment_letters(contig, start, length, rev):
    s = bytes(contig[start:start + length]).upper()
    assert len(s) == length, "segment outside its contig"
    return revcomp(s) if rev else s


def segment_words(contig, start, length, rev):
    """the 2 * ceil(len / 64) words a segment takes in a packed batch: sliced, reverse-complemented if rev, packed,
    zero to the end of its last 16 bytes"""
    out = np.zeros(2 * ((length + 63) // 64), dtype=np.uint64)
    w = pack(segment_letters(contig, start, length, rev))
    out[:len(w)] = w
    return out


def store_layout(lengths):
    """word offset of every contig in the genome store and the store's size: 2 * ceil(len / 64) + 4 words each, one
    after the other"""
    words = [2 * ((int(n) + 63) // 64) + 4 for n in lengths]
    off = np.concatenate(([0], np.cumsum(words, dtype=np.uint64)[:-1])).astype(np.uint64) if words else np.zeros(0, np.uint64)
    return off, int(sum(words))


def store_words(contigs):
    """the whole store for these contigs (pure A/C/G/T): pack(contig), then zeros up to the contig's share"""
    off, total = store_layout([len(c) for c in contigs])
    out = np.zeros(total, dtype=np.uint64)
    for c, o in zip(contigs, off):
        w = pack(c)
        out[int(o):int(o) + len(w)] = w
    return out, off


# ------------------------------------------------------------------------------------------------ classifier
KINDS = ("F0", "F1", "F1pad", "R0", "R1", "Rneg")
# What cannot happen (test_segment_geometry.py checks both on an exhaustive sweep of small shapes):
#  * F1pad with `full`.  A forward word of 32 bases at a start phase other than 0 takes its last bases from the second
#    word it reads, so that word holds bases of the contig and is not padding.
#  * Rneg with `full`.  The source window of a reverse word begins at  start + (len - 32 w) - 32 ; that is negative only
#    when the word holds fewer than 32 - start <= 32 bases.
UNREACHABLE = {("F1pad", "full"), ("Rneg", "full")}


def word_classes(start, length, rev, contig_len=None):
    """The kernel's case split, restated from its comment, for every destination word w of a segment -- 16 lanes per
    segment, lane g writes words g, g + 16, g + 32, ...; a word at or behind the last base is zero; a forward word
    reads the source word that holds base start + 32 w and, at a start phase other than 0, the one behind it; reverse
    word w is the complement, reversed, of the 32 source bases that END at base start + len - 1 - 32 w, read the same
    way unless that window begins in front of the contig, where only the contig's first word is read; a word of fewer
    than 32 bases is masked.  One frozenset per word, drawn from KINDS, full / tail / zero, trip2 (w >= 16), trip3
    (w >= 32).  F1pad (the second word read lies behind the contig's last word) needs contig_len."""
    out = []
    for w in range(2 * ((length + 63) // 64)):
        cls = set()
        if w >= 16:
            cls.add("trip2")
        if w >= 32:
            cls.add("trip3")
        if 32 * w >= length:
            cls.add("zero")
        else:
            cls.add("full" if length - 32 * w >= 32 else "tail")
            if not rev:
                pos = start + 32 * w
                if pos % 32 == 0:
                    cls.add("F0")
                else:
                    cls.add("F1")
                    if contig_len is not None and pos // 32 + 1 >= (contig_len + 31) // 32:
                        cls.add("F1pad")
            else:
                ws = start + length - 1 - 32 * w - 31
                cls.add("Rneg" if ws < 0 else ("R0" if ws % 32 == 0 else "R1"))
        out.append(frozenset(cls))
    return out


def gather_classes(start, length, rev, contig_len=None):
    """every class some word of the segment belongs to"""
    return frozenset().union(*word_classes(start, length, rev, contig_len)) if length else frozenset()


def last_fill(length):
    """bases in the segment's last non-zero word"""
    return (length - 1) % 32 + 1


# ------------------------------------------------------------------------------------------------ gather cases
Seg = namedtuple("Seg", "contig start len rev literal")
GatherCases = namedtuple("GatherCases", "contigs segs")

CONTIG_LENGTHS = [3333, 1, 31, 32, 33, 63, 64, 65, 127, 128, 129, 8063, 8064, 8065, 8066, 2100, 4097]
PER_CLUSTER = 37            # segments per cluster of gather_records: not a multiple of 16
LITERAL_AT = 17             # the segment at this place of every cluster is a literal one (and its strain a target)
FILLS = (1, 31, 32)
END_REMAINDERS = (0, 1, 32, 33, 63)
LENGTHS = (1, 2, 31, 32, 33, 64, 65, 511, 512, 513, 1023, 1024, 1025)


def random_acgt(rng, n):
    return _ACGT[rng.integers(0, 4, int(n))].tobytes()


def gather_cases(seed=20):
    """contigs (bytes) and segments Seg(contig index, start, len, rev, literal); see the module's tests for what the
    list must hold"""
    rng = np.random.default_rng(seed)
    contigs = [random_acgt(rng, n) for n in CONTIG_LENGTHS]
    big = [i for i, n in enumerate(CONTIG_LENGTHS) if n >= 2000]            # the first contig of the store among them
    segs = []

    def add(ci, start, length, rev):
        assert 0 <= start and length >= 1 and start + length <= len(contigs[ci]), (ci, start, length)
        segs.append((ci, int(start), int(length), bool(rev)))

    # every start phase x strand x fill of the last word, on one to three whole words in front of it
    n = 0
    for phase in range(32):
        for rev in (False, True):
            for fill in FILLS:
                ci = big[n % len(big)]
                n += 1
                length = 32 * int(rng.integers(1, 4)) + fill
                q = int(rng.integers(0, (len(contigs[ci]) - length - phase) // 32))
                add(ci, 32 * q + phase, length, rev)
    # the reverse window that begins in front of the contig: at every start 0..30, the longest and the shortest tail
    # that still does (fill < 32 - start), behind 1 whole word; some with no whole word, some on the second lane trip
    for start in range(31):
        for fill in sorted({1, 31 - start}):
            add(big[start % len(big)], start, 32 + fill, True)
        if 31 - start >= 5:
            add(big[(start + 1) % len(big)], start, 31 - start, True)
        if start % 5 == 0:
            add(0, start, 32 * 16 + max(1, (31 - start) // 2), True)
            add(big[-1], start, 32 * 33 + 1, True)
    # whole contigs, both strands
    for ci in range(len(contigs)):
        for rev in (False, True):
            add(ci, 0, len(contigs[ci]), rev)
    # segments that end on the contig's last base
    for ci in (CONTIG_LENGTHS.index(129), 0, CONTIG_LENGTHS.index(8064), CONTIG_LENGTHS.index(8065), CONTIG_LENGTHS.index(2100)):
        for r in END_REMAINDERS:
            for rev in (False, True):
                length = 64 + r if len(contigs[ci]) > 64 + r else r
                if length:
                    add(ci, len(contigs[ci]) - length, length, rev)
    # a forward two-word read whose second word is the contig's padding: the segment runs to the contig's end and its
    # last word begins inside the contig's last word, at phase p -- short, and on the second and third lane trips
    for ci, w_last, p in ((CONTIG_LENGTHS.index(31), 0, 1), (CONTIG_LENGTHS.index(31), 0, 7), (CONTIG_LENGTHS.index(31), 0, 30),
                          (CONTIG_LENGTHS.index(63), 0, 3), (CONTIG_LENGTHS.index(63), 1, 3), (CONTIG_LENGTHS.index(127), 3, 30),
                          (0, 18, 1), (0, 31, 4), (0, 104, 1), (0, 104, 3), (CONTIG_LENGTHS.index(2100), 20, 13)):
        start = 32 * (len(contigs[ci]) // 32 - w_last) + p
        add(ci, start, len(contigs[ci]) - start, False)
    # the lengths around every word, 16-byte and lane-trip boundary, in the first contig and in a later one
    for length in LENGTHS:
        for rev in (False, True):
            for ci in (0, big[1 + (length % (len(big) - 1))]):
                add(ci, int(rng.integers(0, len(contigs[ci]) - length + 1)), length, rev)
    # a literal segment reaches the device as words the host packed: what it was in the list for comes again, by reference
    for x in [x for i, x in enumerate(segs) if i % PER_CLUSTER == LITERAL_AT]:
        if len(segs) % PER_CLUSTER == LITERAL_AT:
            segs.append((0, 0, 40, False))
        segs.append(x)
    return GatherCases(contigs, [Seg(c, s, n, r, i % PER_CLUSTER == LITERAL_AT) for i, (c, s, n, r) in enumerate(segs)])


def strain_name(j):
    return f"s{j:03d}"


TARGET_STRAIN = strain_name(LITERAL_AT)


def gather_strings(cases):
    return [segment_letters(cases.contigs[s.contig], s.start, s.len, s.rev) for s in cases.segs]


def batch_order(cases, k):
    """the segments a batch of gather_records holds at k-mer length k, in the batch's order: one sequence per strain,
    strain names in sorted order, so the order of the list -- less the sequences too short for one k-mer"""
    return [s for s in cases.segs if s.len >= k]


def gather_records(cases, seqinfo):
    """reference-shaped records of the expected strings, PER_CLUSTER strains a cluster, one sequence each;
    seqinfo(sequence, compsequence, id, chromosome, start, end, strand, offset) makes a record's sequence object"""
    strings = gather_strings(cases)
    comp = bytes.maketrans(b"ACGT", b"TGCA")
    recs = []
    for c0 in range(0, len(strings), PER_CLUSTER):
        gs = {}
        for j, s in enumerate(strings[c0:c0 + PER_CLUSTER]):
            sg = cases.segs[c0 + j]
            gs[strain_name(j)] = [seqinfo(s.decode(), s.translate(comp).decode(), f"g{c0 + j}", f"contig{sg.contig}",
                                          sg.start + 1, sg.start + sg.len, -1 if sg.rev else 1, 0)]
        recs.append((gs, f"cl{c0 // PER_CLUSTER:02d}", np.ones(len(gs), dtype=np.int64)))
    return recs


def gather_arrays(cases, k, word_off, seg_word_off):
    """(literal words, src_off, src_start, src_flags, expected device buffer) of the batch of batch_order(cases, k):
    word_off = the contigs' places in the store, seg_word_off = the segments' places in the device buffer.  Literal
    segments go through the host's words (flag bit 0, start 0), the others by (contig, start) with flag bit 1 for the
    reverse strand."""
    order = batch_order(cases, k)
    assert len(order) == len(seg_word_off)
    lit, src_off, src_start, src_flags = [], [], [], []
    n_lit = 0
    total = (int(seg_word_off[-1]) + 2 * ((order[-1].len + 63) // 64) if order else 0) + 4
    expect = np.zeros(total, dtype=np.uint64)
    for s, wo in zip(order, seg_word_off):
        w = segment_words(cases.contigs[s.contig], s.start, s.len, s.rev)
        expect[int(wo):int(wo) + len(w)] = w
        if s.literal:
            src_off.append(n_lit); src_start.append(0); src_flags.append(1)
            lit.append(w)
            n_lit += len(w)
        else:
            src_off.append(int(word_off[s.contig])); src_start.append(s.start); src_flags.append(2 if s.rev else 0)
    lit.append(np.zeros(4, dtype=np.uint64))
    return (np.ascontiguousarray(np.concatenate(lit)), np.asarray(src_off, dtype=np.uint64),
            np.asarray(src_start, dtype=np.uint32), np.asarray(src_flags, dtype=np.uint32), expect)


# ------------------------------------------------------------------------------------------------ ASCII pack cases
def pack_contig_lengths():
    """contig lengths for genome_pack_kernel: the word, 16-byte and 256-word thread-block seams (a piece of 8 064 bases
    is 252 words + the four pad words = one whole block; 8 065 needs a second block), and some 300 short ones so that
    the search for a block's piece has depth"""
    rng = np.random.default_rng(5)
    edge = [0, 1, 31, 32, 33, 63, 64, 65, 8063, 8064, 8065, 16127, 16128, 16129]
    more = [int(x) for x in rng.integers(2, 400, 300)]
    out = more[:100] + edge[:8] + more[100:200] + edge[8:] + more[200:]
    return out


def pack_contigs(seed=6):
    """A/C/G/T contigs of pack_contig_lengths() with lower-case stretches"""
    rng = np.random.default_rng(seed)
    out = []
    for i, n in enumerate(pack_contig_lengths()):
        a = np.frombuffer(random_acgt(rng, n), dtype=np.uint8).copy()
        if n and i % 3 != 1:
            for _ in range(1 + n // 3000):
                at = int(rng.integers(0, n))
                a[at:at + int(rng.integers(1, 70))] |= 0x20
        out.append(a.tobytes())
    return out


# ------------------------------------------------------------------------------------------------ FASTA cases
WIDTHS = (1, 2, 31, 32, 33, 60, 64, 70, 255)
EOLS = (b"\n", b"\r\n")
PRIME = 4999
BIG = 20011                 # the contig that keeps a genome's letters per contig near the store's estimate

FastaContig = namedtuple("FastaContig", "name letters width eol final_eol")     # width 0: one line
FastaGenome = namedtuple("FastaGenome", "name contigs separate pad")


def fasta_lengths(width):
    return [1, width - 1, width, width + 1, 32 * width, 32 * width + 1, PRIME]


def _with_lower(rng, letters):
    a = np.frombuffer(letters, dtype=np.uint8).copy()
    for _ in range(4):
        at = int(rng.integers(0, len(a)))
        a[at:at + 90] |= 0x20
    return a.tobytes()


def fasta_cases(seed=8):
    """genomes whose FASTA text puts genome_pack_text_kernel's line arithmetic on its edges: every width x line end,
    with contigs of 1, width - 1 (an empty record at width 1), width, width + 1, 32 width, 32 width + 1 and a prime
    number of letters beside one long contig; unwrapped contigs with and without a newline at the end of the file; a
    last line that is exactly full at the end of the file, with and without its newline.  Every other genome keeps its
    FASTA in a file of its own; the others have it behind ##FASTA, at a byte offset that differs from genome to genome
    (`pad` bytes of comment in front)."""
    rng = np.random.default_rng(seed)
    genomes = []

    def contig(g, i, n, width, eol, final=True):
        return FastaContig(f"{g}_c{i}", random_acgt(rng, n), width, eol, final)

    for wi, width in enumerate(WIDTHS):
        for ei, eol in enumerate(EOLS):
            g = f"w{width:03d}{'crlf' if ei else 'lf'}"
            cs = [contig(g, i, n, width, eol) for i, n in enumerate(fasta_lengths(width))]
            big = contig(g, len(cs), BIG, width if width >= 31 else 60, eol)
            cs.insert(3 + (wi + ei) % 4, big._replace(letters=_with_lower(rng, big.letters)))
            genomes.append(FastaGenome(g, cs, (wi + ei) % 2 == 1, 7 * wi + 3 * ei))
    for ei, eol in enumerate(EOLS):
        tag = "crlf" if ei else "lf"
        for final in (True, False):
            g = f"oneline_{tag}_{'nl' if final else 'eof'}"
            cs = [contig(g, 0, BIG, 60, eol), contig(g, 1, 777, 0, eol), contig(g, 2, 1, 0, eol), contig(g, 3, PRIME, 0, eol, final)]
            genomes.append(FastaGenome(g, cs, final, 11 + ei))
            g = f"fulllast_{tag}_{'nl' if final else 'eof'}"
            cs = [contig(g, 0, BIG, 80, eol), contig(g, 1, 33, 33, eol), contig(g, 2, 3 * 60, 60, eol, final)]
            genomes.append(FastaGenome(g, cs, not final, 29 + ei))
    return genomes


def fasta_text(contigs):
    out = []
    for i, c in enumerate(contigs):
        out.append(b">" + c.name.encode() + (b" len=%d wrapped" % len(c.letters) if i % 2 else b"") + c.eol)
        step = c.width or max(len(c.letters), 1)
        lines = [c.letters[a:a + step] for a in range(0, len(c.letters), step)]
        body = c.eol.join(lines)
        if lines and c.final_eol:
            body += c.eol
        out.append(body)
    return b"".join(out)


def parse_fasta_text(text):
    """{name: upper-case letters} of FASTA text, read the plain way: header up to the first blank, lines joined, a
    line's trailing carriage returns dropped"""
    out, name = {}, None
    for line in text.split(b"\n"):
        line = line.rstrip(b"\r")
        if line.startswith(b">"):
            name = line[1:].split()[0].decode()
            out[name] = []
        elif name is not None:
            out[name].append(line)
    return {k: b"".join(v).upper() for k, v in out.items()}


def genes_of(genome):
    """(gene id, contig name, first base, last base (1-based, inclusive), strand) of the genome's features: every
    contig with a letter as a whole, on alternating strands, and, in its long contig, stretches across line ends"""
    genes = []
    for i, c in enumerate(genome.contigs):
        n = len(c.letters)
        if n == 0:
            continue
        if n < 10000:
            genes.append((f"{genome.name}_g{len(genes):02d}", c.name, 1, n, 1 if i % 2 else -1))
            continue
        w = c.width or n
        for a, b in ((1, 5), (w - 1, w + 3), (w, 2 * w), (7 * w + 5, 40 * w + 6), (n - 2 * w - 1, n), (n - 4, n), (1, n)):
            genes.append((f"{genome.name}_g{len(genes):02d}", c.name, a, b, 1 if len(genes) % 2 else -1))
    return genes


def write_fasta_pangenome(root, genomes):
    """the genomes as files (GFF3 with CDS features, FASTA behind ##FASTA or beside it) and a presence/absence table whose
    row j holds gene j of every genome that has one.  Returns dict(csv, genomes, gff, fasta, clusters) -- clusters: per
    table row, per strain in sorted order, the expected sequence (gene cut out of the parsed file, reverse-complemented
    on the - strand)."""
    os.makedirs(os.path.join(root, "gffs"), exist_ok=True)
    names = sorted(g.name for g in genomes)
    by_name = {g.name: g for g in genomes}
    gff, fasta, genes, letters = [], [], {}, {}
    for nm in names:
        g = by_name[nm]
        text = fasta_text(g.contigs)
        parsed = parse_fasta_text(text)
        assert parsed == {c.name: c.letters.upper() for c in g.contigs}
        letters[nm] = parsed
        genes[nm] = genes_of(g)
        lines = ["##gff-version 3", "#" + "p" * g.pad]
        for gid, cname, a, b, strand in genes[nm]:
            lines.append(f"{cname}\tProdigal\tCDS\t{a}\t{b}\t.\t{'+' if strand > 0 else '-'}\t0\tID={gid};product=x")
        path = os.path.join(root, "gffs", nm + ".gff")
        with open(path, "wb") as fh:
            fh.write(("\n".join(lines) + "\n").encode())
            if not g.separate:
                fh.write(b"##FASTA\n" + text)
        fa = None
        if g.separate:
            fa = os.path.join(root, "gffs", nm + ".fasta")
            with open(fa, "wb") as fh:
                fh.write(text)
        gff.append(path)
        fasta.append(fa)
    nrows = max(len(v) for v in genes.values())
    csv = os.path.join(root, "gene_presence_absence.csv")
    clusters = []
    with open(csv, "w") as fh:
        fh.write(",".join(["Gene", "Non-unique Gene name", "Annotation"] + names) + "\n")
        for j in range(nrows):
            cells, row = [], []
            for nm in names:
                if j < len(genes[nm]):
                    gid, cname, a, b, strand = genes[nm][j]
                    cells.append(gid)
                    s = letters[nm][cname][a - 1:b]
                    row.append((nm, revcomp(s) if strand < 0 else s))
                else:
                    cells.append("")
            fh.write(",".join([f"row{j:02d}", "", "x"] + cells) + "\n")
            clusters.append(row)
    return dict(csv=csv, genomes=names, gff=gff, fasta=fasta, clusters=clusters)


# ------------------------------------------------------------------------------------------------ staging blocks
def staging_lengths(seed=3, scale=1 << 20):
    """contig lengths for an upload of more than two 64 MiB staging blocks: about 40, 50 and 45 `scale` bases with 200
    short contigs behind each of the first two"""
    rng = np.random.default_rng(seed)
    lens = []
    for i, big in enumerate((40 * scale + 11, 50 * scale - 7, 45 * scale + 31)):
        lens.append(big)
        if i < 2:
            lens += [int(x) for x in rng.integers(1, 3000, 200)]
    return np.asarray(lens, dtype=np.uint64)


def staging_contigs(seed=3, scale=1 << 20):
    """(ascii uint8 array, offsets, lengths) of staging_lengths: one draw and one table look-up for all letters"""
    lens = staging_lengths(seed, scale)
    offs = np.concatenate(([0], np.cumsum(lens)[:-1])).astype(np.uint64)
    ascii_ = _ACGT[np.random.default_rng(seed + 1).integers(0, 4, int(lens.sum()), dtype=np.uint8)]
    return ascii_, offs, lens
