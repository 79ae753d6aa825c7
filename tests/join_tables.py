"""panfeed-get-kmers' device join (KmerJoin, the kj_* kernels of csrc/pf_rowfilter.hip), stated without the library:
`plainness` is the rule by which the survey kernel flags a kmers.tsv row that pandas might not print as it stands,
`join_rows` the rows the writer kernel makes of a bunch, and `join_model` the whole tool -- the host half of the feature
(the package's own pandas statements and its `rendered_texts`) with these two in the kernels' place.

TEST INFRASTRUCTURE: pure Python on `bytes` for the kernels' part; nothing here calls the library, and nothing is
derived from panfeed_amd/csrc.  tests/test_join_model.py (CPU) holds the model against the reference's recorded outputs
and `plainness` against pandas; tests/test_gpu_kmerjoin.py holds the kernels against the model.
"""
import io
import re

MAX_FIELD = 4096             # a field of 4 096 bytes or more: never a key, and a flag in a selected row
MAX_LINE = 1 << 16           # a row of more than 65 536 bytes, newline included, is a flag
TABS, BYTES, INT, EMPTY, NA, NUMERIC, WORD, LONG = 1, 2, 4, 8, 16, 32, 64, 128
FLAG_BITS = (TABS, BYTES, INT, EMPTY, NA, NUMERIC, WORD, LONG)

# pandas' default NA strings (pandas._libs.parsers.STR_NA_VALUES), but the empty one
NA_STRINGS = (b"#N/A", b"#N/A N/A", b"#NA", b"-1.#IND", b"-1.#QNAN", b"-NaN", b"-nan", b"1.#IND", b"1.#QNAN", b"<NA>",
              b"N/A", b"NA", b"NULL", b"NaN", b"None", b"n/a", b"nan", b"null")
WORDS = (b"inf", b"infinity", b"nan", b"true", b"false")
INT_FIELDS = range(4, 10)    # feature_strand .. strand
_CANONICAL = re.compile(rb"-?(0|[1-9][0-9]{0,17})\Z")
_NUMBER_BYTES = re.compile(rb"[0-9+\-.eE]+\Z")
_BAD_BYTE = re.compile(rb'[\x00-\x08\x0a-\x1f\x80-\xff"]')


def plainness(row):
    """the flags of one row (bytes, without its newline): 0 for a row that read_csv -> to_csv prints as it stands
    whatever the other rows of its column are"""
    flags = 0
    if len(row) + 1 > MAX_LINE:          # (with its newline; the kernel stops there: which other flags it has set is open)
        return LONG
    fields = row.split(b"\t")
    if len(fields) != 11:
        flags |= TABS
    if _BAD_BYTE.search(row):
        flags |= BYTES
    for i, f in enumerate(fields[:11]):
        if len(f) >= MAX_FIELD:
            flags |= LONG
        if i in INT_FIELDS:
            if not _CANONICAL.match(f) or f == b"-0":
                flags |= INT
            continue
        if not f:
            flags |= EMPTY
            continue
        if _NUMBER_BYTES.match(f):
            flags |= NUMERIC
        if f in NA_STRINGS:
            flags |= NA
        if (f[1:] if f[:1] in (b"+", b"-") else f).lower() in WORDS:
            flags |= WORD
    return flags


def rows_of(text):
    """the data rows of a table's text (bytes, header line first), without their newlines; a last line without its
    newline is a row"""
    body = text.split(b"\n", 1)[1] if b"\n" in text else b""
    rows = body.split(b"\n")
    return rows[:-1] if rows and rows[-1] == b"" else rows


def selected(row, clusters):
    """whether the row's first field is one of `clusters` (a field of MAX_FIELD bytes or more never is)"""
    c = row.split(b"\t", 1)[0]
    return len(c) < MAX_FIELD and c in clusters


def survey(rows, bunch_clusters, keys):
    """per bunch: rows, rows without a key, OR of the rows' flags"""
    out = [{"rows": 0, "unmatched": 0, "flags": 0} for _ in bunch_clusters]
    for row in rows:
        for n, clusters in enumerate(bunch_clusters):
            if not selected(row, clusters):
                continue
            f = plainness(row)
            out[n]["rows"] += 1
            out[n]["flags"] |= f
            if not f & (TABS | LONG):
                fields = row.split(b"\t")
                out[n]["unmatched"] += (fields[0], fields[10]) not in keys
            break
    return out


def join_rows(rows, clusters, texts, empty):
    """the writer's text for one bunch of plain rows: texts maps (cluster, k-mer) to the rendered columns"""
    out = []
    for row in rows:
        if not selected(row, clusters):
            continue
        f = row.split(b"\t")
        out.append(b"\t".join([f[0], f[10], texts.get((f[0], f[10]), empty)] + f[1:10]) + b"\n")
    return b"".join(out)


def kept_rows(rows, clusters, keys):
    """the raw rows of a bunch that have a key (--only-passing hands these to pandas)"""
    return b"".join(r + b"\n" for r in rows if selected(r, clusters) and (r.split(b"\t")[0], r.split(b"\t")[10]) in keys)


def join_model(assoc_path, kh_text, kmers_text, threshold=1.0, column="lrt-pvalue", per_iteration=15, only_passing=False, host=False):
    """panfeed-get-kmers' stdout (str) and, per bunch, whether the device route takes it: the package's host half with
    the kernels' part done here.  kh_text / kmers_text: the bytes of kmers_to_hashes.tsv and kmers.tsv.  host: every bunch
    through the pandas statements (what --host-join does)"""
    import pandas as pd

    from panfeed_amd import downstream as ds
    from panfeed_amd.engine import KMERS_TSV_HEADER

    a = pd.read_csv(assoc_path, sep="\t", index_col=0)
    a.index.name = "hashed_pattern"
    a = a[a[column] <= threshold]
    passing = {str(x).encode() for x in a.index.unique()}
    kh_header = kh_text.split(b"\n", 1)[0] + b"\n"
    kept = [r for r in rows_of(kh_text) if r.rsplit(b"\t", 1)[-1] in passing and len(r.rsplit(b"\t", 1)[-1]) < MAX_FIELD]
    h = pd.read_csv(io.BytesIO(kh_header + b"".join(r + b"\n" for r in kept)), sep="\t").set_index("hashed_pattern")
    clusters = ds._ordered_unique(h["cluster"])
    literal = {}
    for val, row in zip(h["cluster"].tolist(), kept):
        literal.setdefault(ds._key(val), {})[row.split(b"\t", 1)[0]] = None
    out, routes = io.StringIO(), []
    if not clusters:
        return "", routes
    b = a.join(h, how="inner")
    B = b.reset_index().set_index(["cluster", "k-mer"])
    bunches = [clusters[i: i + per_iteration] for i in range(0, len(clusters), per_iteration)]
    bunch_clusters = [{lit for c in bunch if c is not ds._NAN_KEY for lit in literal[ds._key(c)]} for bunch in bunches]
    columns = KMERS_TSV_HEADER.rstrip("\n").split("\t")
    k_header = kmers_text.split(b"\n", 1)[0] + b"\n"
    texts = "host" if host else "header" if k_header != KMERS_TSV_HEADER.encode() else ds.rendered_texts(B, columns[1:10])
    if not isinstance(texts, str) and not all(c.encode() in set().union(*bunch_clusters) for c, _ in texts["keys"]):
        texts = "literal"
    rows = rows_of(kmers_text)
    plan = None
    if not isinstance(texts, str):
        keys = [(c.encode(), k.encode()) for c, k in texts["keys"]]
        plan = survey(rows, bunch_clusters, set(keys))
    first = True
    for n, cl in enumerate(bunch_clusters):
        device = plan is not None and not plan[n]["flags"]
        routes.append(device)
        if device and not only_passing:
            if first:
                out.write(texts["header"])
            t = texts["text1" if plan[n]["unmatched"] else "text0"]
            out.write(join_rows(rows, cl, dict(zip(keys, t)), texts["empty"]).decode())
            first = False
            continue
        body = kept_rows(rows, cl, set(keys)) if device else b"".join(r + b"\n" for r in rows if selected(r, cl))
        k = pd.read_csv(io.BytesIO(k_header + body), sep="\t").set_index(["cluster", "k-mer"])
        B.join(k, how="left" if only_passing else "right").to_csv(out, sep="\t", header=first)
        first = False
    return out.getvalue(), routes


# ------------------------------------------------------------------------------------------------ handmade tables
KH_HEADER = b"cluster\tk-mer\thashed_pattern\n"
KMERS_HEADER = b"cluster\tstrain\tfeature_id\tcontig\tfeature_strand\tcontig_start\tcontig_end\tgene_start\tgene_end\tstrand\tk-mer\n"


def kmers_row(cluster, kmer, i, strain=None):
    """a plain row; the strain's length goes through 1 .. 33 with i, so rows begin and end at every offset of a vector"""
    strain = strain if strain is not None else "s" + "x" * (i % 33)
    return "\t".join([cluster, strain, f"gene_{i}", "NODE_1", "1" if i % 2 else "-1", str(100 + i), str(131 + i), str(i), str(i + 31),
                      "1", kmer]).encode()


def handmade(int_column=True, rows_per_cluster=70, long_notes=300, final_newline=False):
    """associations (str), kmers_to_hashes.tsv and kmers.tsv (bytes), one bunch per cluster with
    --clusters-per-iteration 1:
      g, gx, gxy   clusters that are prefixes of one another; the k-mers ACG, ACGT, ACGTA are too.  (g, ACG), (gx, ACGT) and
                   (gxy, ACGTA) are keys: ACG under gx, ACGT under g ... are in the table under another cluster only
      alone        every row without a key (its one key's k-mer is in no row)
      full         every row with a key
      absent       selected, and not in kmers.tsv
      other        in kmers.tsv, not selected
    The notes column's texts have lengths from 0 to long_notes; with int_column the associations have an integer column,
    so the two renderings differ: `full` has no unmatched row, the others have.  The last row has no newline."""
    passing = [("H1", "g", "ACG"), ("H2", "gx", "ACGT"), ("H3", "gxy", "ACGTA"), ("H4", "alone", "TTTT"), ("H5", "full", "CCA"),
               ("H6", "full", "CCAG"), ("H7", "absent", "GGG"), ("H1", "full", "CCAGT")]
    failing = [("X1", "other", "ACG"), ("X2", "g", "ACGT"), ("X1", "gx", "ACG")]
    kh = KH_HEADER + b"".join(f"{c}\t{k}\t{h}\n".encode() for h, c, k in passing + failing)
    hashes = list(dict.fromkeys(h for h, _, _ in passing)) + ["X1", "X2"]
    assoc = "variant\tlrt-pvalue" + ("\tcount" if int_column else "") + "\tnotes\n"
    for i, h in enumerate(hashes):
        note = "n" * (long_notes * i // 6 if h[0] == "H" else 3)
        assoc += f"{h}\t{'0.9' if h[0] == 'X' else f'1e-{i + 2}'}" + (f"\t{i + 3}" if int_column else "") + f"\t{note}\n"
    rows = []
    kmers_of = {"g": ["ACG", "ACGT", "ACGTA"], "gx": ["ACGT", "ACG", "ACGTA"], "gxy": ["ACGTA", "ACGT", "AC"],
                "alone": ["TTT", "TTTTT", "ACG"], "full": ["CCA", "CCAG", "CCAGT"], "other": ["ACG", "CCA", "GGG"]}
    i = 0
    for cluster in ("g", "other", "gx", "alone", "gxy", "full"):
        for r in range(rows_per_cluster):
            rows.append(kmers_row(cluster, kmers_of[cluster][r % 3], i))
            i += 1
    kmers = KMERS_HEADER + b"\n".join(rows) + (b"\n" if final_newline else b"")
    return {"assoc": assoc, "kh": kh, "kmers": kmers}


def vector_places(kmers):
    """(offsets within their 16-byte vector at which the rows of the body begin, at which their newlines lie)"""
    body = kmers.split(b"\n", 1)[1]
    begins, ends, at = set(), set(), 0
    for row in body.split(b"\n"):
        begins.add(at % 16)
        at += len(row)
        ends.add(at % 16)
        at += 1
    return begins, ends
