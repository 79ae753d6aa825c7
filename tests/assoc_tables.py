"""The associations filter (AssocFilter, the af_* kernels of csrc/pf_rowfilter.hip), stated without the library: the class of
a cell, the flags of a row, which rows may pass a threshold, and the case tables that reach every class, flag and spelling.

TEST INFRASTRUCTURE: pure Python on `bytes`.  Nothing here calls the library or pandas and nothing is derived from
panfeed_amd/csrc: tests/test_assoc_tables.py (CPU) holds the model against pandas -- the dtypes the classes predict, the
rows pandas keeps, the bytes the tools print --, tests/test_gpu_assoc_filter.py holds the kernels against the model.

A table is split on b"\\n" and b"\\t" only; its first line is the header line.

The value of a number's text is taken the way pandas' default float parser takes it: the first 17 digits count, leading
zeros among them; an integer digit behind them raises the decimal exponent, a fraction digit behind them is dropped.  (So
0.<18 zeros>5 is 0 to pandas, and to this model.)  With m those digits as an integer and e the exponent, the value is
m * 10^e exactly -- a Fraction here; pandas is within 2^-50 of it, the kernel within 2^-48 -- and a row is dropped only if
it is above thr_hi = thr + |thr| * 2^-30.  A value that is not 0 and whose leading digit stands outside the decades
1e-300 .. 1e300 is `undecided`: its row is kept whatever the threshold.
"""
import math
import random
import re
from collections import namedtuple
from fractions import Fraction

MAX_FIELD = 4096             # a field of 4 096 bytes or more is a flag
MAX_LINE = 1 << 16           # a row of more than 65 536 bytes, newline included, is a flag
INT, FLOAT, NA, ODD, TEXT = 1, 2, 4, 8, 16
CLASS_BITS = (INT, FLOAT, NA, ODD, TEXT)
ROW_FIELDS, ROW_EMPTY, ROW_BYTES, ROW_LONG = 1, 2, 4, 8
ROW_BITS = (ROW_FIELDS, ROW_EMPTY, ROW_BYTES, ROW_LONG)
MARGIN = 2.0 ** -30
DIGITS = 17
DECADES = 300

# pandas' default NA strings (pandas._libs.parsers.STR_NA_VALUES)
NA_STRINGS = (b"", b"#N/A", b"#N/A N/A", b"#NA", b"-1.#IND", b"-1.#QNAN", b"-NaN", b"-nan", b"1.#IND", b"1.#QNAN", b"<NA>",
              b"N/A", b"NA", b"NULL", b"NaN", b"None", b"n/a", b"nan", b"null")
WORDS = (b"inf", b"infinity", b"nan", b"true", b"false")
_INT = re.compile(rb"[+-]?[0-9]{1,18}\Z")
_DIGITS = re.compile(rb"[+-]?[0-9]+\Z")
_FLOAT = re.compile(rb"([+-]?)(?:([0-9]+)\.?([0-9]*)|\.([0-9]+))(?:[eE]([+-]?)([0-9]+))?\Z")
_BAD_BYTE = re.compile(rb'[\x00-\x08\x0a-\x1f"]')


def _float_parts(cell):
    """(negative, integer digits, fraction digits, exponent) of a cell of the number grammar, None for any other"""
    m = _FLOAT.match(cell)
    if not m:
        return None
    sign, ip, fp, lone, esign, ex = m.groups()
    ip, fp = (ip or b""), (fp if lone is None else lone) or b""
    return sign == b"-", ip, fp, (-1 if esign == b"-" else 1) * int(ex) if ex else 0, len(ex or b"")


def classify(cell):
    """the class of one cell.  ODD, a cell pandas may read otherwise in a part of the file than in the whole: a word of
    WORDS with an optional sign in any case that is no NA string; a space at either end; an integer of more than 18 digits;
    a number with more than 18 integer digits, more than 5 exponent digits, or whose exponent plus integer digits exceed
    300 (pandas' parser refuses or overflows on some of these, and the column turns to text)"""
    if cell == b"":
        return NA
    if cell[:1] == b" " or cell[-1:] == b" ":
        return ODD
    if _INT.match(cell):
        return INT
    if _DIGITS.match(cell):
        return ODD
    parts = _float_parts(cell)
    if parts:
        _neg, ip, _fp, ex, ex_digits = parts
        return ODD if len(ip) > 18 or ex_digits > 5 or (ex > 0 and ex + len(ip) > DECADES) else FLOAT
    if cell in NA_STRINGS:
        return NA
    if (cell[1:] if cell[:1] in (b"+", b"-") else cell).lower() in WORDS:
        return ODD
    return TEXT


def row_flags(row, n_fields):
    """the flags of one data row (bytes, without its newline) of a table whose header has n_fields names"""
    if len(row) + 1 > MAX_LINE:              # (the kernel stops there: which other flags it has set is open)
        return ROW_LONG
    flags = 0
    fields = row.split(b"\t")
    if len(fields) != n_fields:
        flags |= ROW_FIELDS
    if row == b"":
        flags |= ROW_EMPTY
    if _BAD_BYTE.search(row):
        flags |= ROW_BYTES
    if any(len(f) >= MAX_FIELD for f in fields):
        flags |= ROW_LONG
    return flags


def value_of(cell):
    """(the value of a cell of class INT or FLOAT as a Fraction, whether it is undecided)"""
    neg, ip, fp, ex, _ = _float_parts(cell)
    taken = (ip + fp)[:DIGITS]
    m = int(taken) if taken else 0
    e = ex + max(0, len(ip) - DIGITS) - max(0, len(taken) - len(ip))
    if m == 0:
        return Fraction(0), False
    lead = len(str(m)) - 1 + e                                 # the decade of the leading digit
    if lead < -DECADES or lead + 1 > DECADES:
        return None, True
    v = Fraction(m) * Fraction(10) ** e
    return (-v if neg else v), False


def thr_hi(thr):
    return thr + abs(thr) * MARGIN


def may_pass(cell, thr):
    """whether the filter keeps a row whose p-value cell is this: a number that is undecided or not above thr_hi"""
    if not classify(cell) & (INT | FLOAT):
        return False
    v, undecided = value_of(cell)
    if undecided:
        return True
    hi = thr_hi(thr)
    if math.isnan(hi):
        return False
    if math.isinf(hi):
        return hi > 0
    return v <= Fraction(hi)


Scan = namedtuple("Scan", "kept classes flags rows n_kept")


def data_lines(text):
    """the data rows of a table's text (header line first), without their newlines; a last line without its newline is one"""
    body = text.split(b"\n", 1)[1] if b"\n" in text else b""
    rows = body.split(b"\n")
    return rows[:-1] if rows and rows[-1] == b"" else rows


def as_scanned(text):
    """the data lines' bytes as a pass scans them: a last line without its newline is given one"""
    body = text.split(b"\n", 1)[1] if b"\n" in text else b""
    return body if not body or body.endswith(b"\n") else body + b"\n"


def scan(text, pvalue_field, thr):
    """what one pass over the table's data lines returns: the kept lines joined, each with a newline; per column of the
    header the OR of its cells' classes; the OR of the rows' flags; data lines; kept lines"""
    n_fields = len(text.split(b"\n", 1)[0].split(b"\t"))
    classes, flags, kept = [0] * n_fields, 0, []
    rows = data_lines(text)
    for row in rows:
        f = row_flags(row, n_fields)
        flags |= f
        fields = row.split(b"\t")
        if len(row) + 1 <= MAX_LINE:
            for i, cell in enumerate(fields[:n_fields]):
                classes[i] |= classify(cell)
        if not f & ROW_LONG and pvalue_field < len(fields) and may_pass(fields[pvalue_field], thr):
            kept.append(row + b"\n")
    return Scan(b"".join(kept), classes, flags, len(rows), len(kept))


def dtype_of(bits, rows=1):
    """the dtype pandas infers for a column whose cells have these classes; None where the model does not say"""
    if bits & ODD or (bits & TEXT and bits & (INT | FLOAT)):
        return None
    if bits & TEXT:
        return "object"
    return "int64" if bits == INT and rows else "float64"


# ------------------------------------------------------------------------------------------------ cases
THRESHOLDS = (1.0, 0.05, 1e-12, 0.0, -1.0, math.inf, math.nan)
HEADER = b"variant\taf\tfilter-pvalue\tlrt-pvalue\tbeta\tbeta-std-err\tintercept\tnotes\n"
PVALUE_FIELD = 3

# one cell per class and per way into it; ODD cells are kept apart: a table that holds one goes through pandas whole
CELLS = {
    INT: (b"0", b"7", b"-0", b"+5", b"007", b"123456789012345678", b"-123456789012345678"),
    FLOAT: (b"5E-02", b"0.05", b".05", b"5.e-2", b"+0.05", b"5.", b"00.0500", b"-1.5e+3", b"1e-320", b"0.1234567890123456789012345",
            b"0.0000000000000000005", b"1e299", b"123456789012345678.5", b"1e-99999", b"0e-400"),
    NA: NA_STRINGS,
    TEXT: (b"abc", b"1e", b".", b"+", b"-", b"e5", b"1.2.3", b"1e+", b"--1", b"1 2", b"0x10", b"1_0", b"1d5", b"1,0", b"1e5.", b".e1",
           b"none", b"NONE", b"Na", b"<na>", b"t", b"yes", b"caf\xc3\xa9", b"a b", b"x" * 40),
    ODD: (b"inf", b"-Infinity", b"+nan", b"NAN", b"True", b"FALSE", b"-true", b" 1", b"1 ", b" ", b"1234567890123456789",
          b"+1234567890123456789012", b"1234567890123456789012345e-30", b"1234567890123456789.5", b"1e400", b"0e400", b"1e000005",
          b"12345e296"),
}
# every spelling class of a p-value cell the filter decides on (1e400 and an integer mantissa of 25 digits are ODD cells:
# pandas turns their column to text; they stand in the table `odd_pvalue`)
PVALUE_SPELLINGS = (b"5E-02", b"0.05", b".05", b"5.e-2", b"+0.05", b"-0", b"0", b"00.0500", b"0.1234567890123456789012345",
                    b"0.04999999999999999999999999", b"1e-320", b"-1e-320", b"0.0000000000000000005", b"1e-13", b"1", b"1.0", b"-1",
                    b"-1.0000000001", b"3", b"", b"NA", b"nan")


def threshold_cells(thr):
    """the threshold's own text, its two neighbours at 17 digits, and texts 2^-31 and 2^-29 relative above it"""
    if thr == 0 or math.isinf(thr) or math.isnan(thr):
        return [b"0", b"0.0", b"-0.0", b"1e-17", b"-1e-17"]
    own = repr(thr).encode()
    mant, ex = ("%.16e" % thr).split("e")
    digits = int(mant.replace(".", "").replace("-", ""))
    sign = "-" if thr < 0 else ""
    out = [own]
    for d in (digits - 1, digits + 1):
        t = str(d)
        out.append(f"{sign}{t[0]}.{t[1:]}e{ex}".encode())
    for k in (31, 29):
        v = Fraction(thr) * (1 + Fraction(1, 2 ** k)) if thr > 0 else Fraction(thr) * (1 - Fraction(1, 2 ** k))
        n = 0
        while abs(v) * 10 ** n < 10 ** 24:
            n += 1
        q = str(abs(v) * 10 ** n // 1)                        # 25 digits
        out.append(f"{sign}{q[0]}.{q[1:]}e{24 - n}".encode())
    return out


def _row(i, pvalue, variant=None, af=None, notes=None, beta=None):
    variant = variant if variant is not None else b"H%04dabcdefghijklmnopqr==" % i
    return b"\t".join([variant, af if af is not None else b"%.2E" % (0.01 * (i % 50 + 1)), b"%.2E" % (0.5 / (i + 1)), pvalue,
                       beta if beta is not None else b"%.2E" % (-1.5 + i * 0.1), b"%.2E" % (0.1 + i * 0.01), b"%d" % (i % 7),
                       notes if notes is not None else (b"", b"bad-chisq", b"NA", b"high-bse")[i % 4]])


def _table(rows, newline=b"\n", last_newline=True):
    body = newline.join(rows) + (newline if last_newline else b"")
    return HEADER.replace(b"\n", newline) + body


def case_tables(thr=0.05):
    """name -> table text.  `intercept` is an INT column, `notes` one of words, blanks and NA; the spellings table holds
    every p-value spelling and the threshold's own cells"""
    cells = list(PVALUE_SPELLINGS) + threshold_cells(thr)
    t = {}
    t["spellings"] = _table([_row(i, c) for i, c in enumerate(cells)])
    t["no_final_newline"] = _table([_row(i, c) for i, c in enumerate(cells[:9])], last_newline=False)
    # an INT column whose only blank lies in a dropped row: the kept rows must print 1.0, not 1
    t["int_blank_in_dropped_row"] = HEADER + b"".join(
        _row(i, b"0.9" if i == 3 else b"1e-20").rsplit(b"\t", 2)[0] + (b"\t\tn\n" if i == 3 else b"\t1\tn\n") for i in range(6))
    t["all_blank_column"] = _table([_row(i, b"1e-%d" % i, beta=b"") for i in range(8)])
    t["duplicate_hashes"] = _table([_row(i, b"1e-%d" % i, variant=b"Hdup%d" % (i % 3)) for i in range(9)])
    t["blank_hash"] = _table([_row(i, b"1e-%d" % i, variant=b"" if i == 2 else None) for i in range(5)])
    t["numeric_index"] = _table([_row(i, b"1e-%d" % i, variant=b"%d" % (100 - i)) for i in range(5)])
    t["float_index_with_na"] = _table([_row(i, b"1e-%d" % i, variant=(b"1", b"2.5", b"NA", b"4")[i % 4]) for i in range(8)])
    t["int_and_float_mixed"] = _table([_row(i, (b"1", b"0", b"0.5", b"1e-30")[i % 4], af=(b"1", b"0.5")[i % 2]) for i in range(8)])
    t["int_pvalues"] = _table([_row(i, (b"1", b"0", b"-1", b"2")[i % 4]) for i in range(8)])
    t["header_only"] = HEADER
    t["nothing_passes"] = _table([_row(i, b"2e200") for i in range(4)])
    # these go through pandas whole
    t["word_in_pvalue"] = _table([_row(i, b"failed" if i == 2 else b"1e-%d" % i) for i in range(5)])
    t["odd_pvalue"] = _table([_row(i, (b"1e400", b"1234567890123456789012345e-30", b"inf", b"0.01")[i % 4]) for i in range(8)])
    t["text_and_numbers"] = _table([_row(i, b"1e-%d" % i, af=b"high" if i == 1 else None) for i in range(5)])
    t["short_row"] = _table([_row(0, b"0.01"), b"Hshort\t0.5\t0.1", _row(2, b"0.02")])
    t["long_row"] = _table([_row(0, b"0.01"), _row(1, b"0.02") + b"\textra", _row(2, b"0.9")])
    t["quoted_cell"] = _table([_row(0, b"0.01", notes=b'"a quoted note"'), _row(1, b"0.02")])
    t["crlf"] = _table([_row(i, b"1e-%d" % i) for i in range(4)], newline=b"\r\n")
    t["blank_line"] = _table([_row(0, b"0.01"), b"", _row(2, b"0.02")])
    t["control_byte"] = _table([_row(0, b"0.01", notes=b"a\x01b"), _row(1, b"0.02")])
    return t


FLAGGED = {"short_row": ROW_FIELDS, "long_row": ROW_FIELDS, "quoted_cell": ROW_BYTES, "crlf": ROW_BYTES, "blank_line": ROW_EMPTY | ROW_FIELDS,
           "control_byte": ROW_BYTES}
HOST_TABLES = ("word_in_pvalue", "odd_pvalue", "text_and_numbers") + tuple(FLAGGED)


def long_tables():
    """a field of 5 000 bytes and a line of 70 000 bytes, each between plain rows"""
    return {"field_5000": _table([_row(0, b"0.01"), _row(1, b"0.02", notes=b"n" * 5000), _row(2, b"0.9")]),
            "line_70000": _table([_row(0, b"0.01"), _row(1, b"0.02", notes=b"\t".join([b"n" * 4000] * 18)[:70000 - 120]), _row(2, b"0.03")])}


# ------------------------------------------------------------------------------------------------ seams
SEAMS = ("word", "vector", "span", "tile")          # 4 bytes, 16 bytes, a thread's 256 bytes, a workgroup's 64 KiB
PARTS = ("start", "cell", "end")
TILE = 1 << 16


def _seam_of(offset):
    """the widest seam that lies right in front of the byte at `offset` of the scanned text"""
    if offset == 0:
        return None
    for name, unit in (("tile", TILE), ("span", 256), ("vector", 16), ("word", 4)):
        if offset % unit == 0:
            return name
    return None


def seam_classes(body, pvalue_field=PVALUE_FIELD, skew=0):
    """the (seam, part) pairs the data lines `body` (no header line) reach, `skew` bytes into the scanned text: a line that
    starts behind a seam, a p-value cell a seam cuts in two, a newline that is the last byte in front of a seam"""
    got, at = set(), skew
    for row in body.split(b"\n")[:-1]:
        if _seam_of(at):
            got.add((_seam_of(at), "start"))
        fields = row.split(b"\t")
        if pvalue_field < len(fields):
            b = at + sum(len(f) + 1 for f in fields[:pvalue_field])
            for off in range(b + 1, b + len(fields[pvalue_field])):
                if _seam_of(off):
                    got.add((_seam_of(off), "cell"))
        at += len(row) + 1
        if _seam_of(at):
            got.add((_seam_of(at), "end"))
    return got


def seeded_table(seed, skew=0, tiles=3):
    """a pyseer-shaped table of about 200 KB with log-uniform p-values, into which rows are padded so that a line start,
    the inside of a p-value cell and a line end fall on every kind of seam of the data lines' text (`skew`: bytes in front
    of the data lines in the scanned text, the header line's where it is scanned along)"""
    rnd = random.Random(seed)
    body = bytearray()
    n = [0]

    def row(notes=None):
        n[0] += 1
        p = b"%.2E" % 10 ** rnd.uniform(-12, 0)
        return _row(n[0], p, variant=b"%024x" % rnd.getrandbits(96), notes=notes) + b"\n"

    def cell_offset(r):
        return sum(len(f) + 1 for f in r.split(b"\t")[:PVALUE_FIELD])

    wanted = []
    at = 3000
    for unit, name in ((4, "word"), (16, "vector"), (256, "span")):
        for part in PARTS:
            t = (at + unit - 1) // unit * unit
            while _seam_of(t) != name:
                t += unit
            wanted.append((t, part))
            at = t + 2500
    for k, part in zip(range(1, tiles + 1), PARTS):
        wanted.append((k * TILE, part))
    for target, part in sorted(wanted):
        target -= skew
        while len(body) < target - 600:
            body += row()
        r = row()
        want = {"start": target, "cell": target - cell_offset(r) - 2, "end": target - len(r)}[part]
        filler = row(notes=b"")
        body += filler[:-1] + b"p" * (want - len(body) - len(filler)) + b"\n"
        assert len(body) == want, (len(body), want)
        body += r
    for _ in range(20):
        body += row()
    return HEADER + bytes(body)
