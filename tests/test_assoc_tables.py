"""The model of the associations filter (tests/assoc_tables.py) against pandas, and the package's routing fed with the
model's answers in the device's place: no GPU.  What is checked of pandas is what the device route rests on -- the dtype a
column's classes predict, that the model never drops a row pandas keeps, and that the kept lines read under the predicted
dtypes print as the whole file does."""
import argparse
import gzip
import io
import json
import math
import os
import sys
import warnings

import pandas as pd
import pytest

from conftest import GOLDEN

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import assoc_tables as at  # noqa: E402

THR_IDS = [repr(t) for t in at.THRESHOLDS]


def _one_column(cells):
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        # (an empty cell is a line of its own here: it must not be skipped as a blank line)
        return pd.read_csv(io.BytesIO(b"x\n" + b"".join(c + b"\n" for c in cells)), sep="\t", skip_blank_lines=False)["x"]


def test_na_strings_are_pandas_own():
    from pandas._libs.parsers import STR_NA_VALUES
    assert {s.decode() for s in at.NA_STRINGS} == set(STR_NA_VALUES)


@pytest.mark.parametrize("bit", [at.INT, at.FLOAT, at.NA, at.TEXT])
def test_a_class_predicts_the_dtype(bit):
    """every non-ODD case cell, with a cell of the same class beside it, makes the column the dtype its class says"""
    for cell in at.CELLS[bit]:
        assert at.classify(cell) == bit, cell
        got = _one_column([cell, at.CELLS[bit][1], cell])
        assert str(got.dtype) == at.dtype_of(bit), (cell, got.dtype)


def test_odd_cells_are_odd_and_every_class_is_reached():
    for cell in at.CELLS[at.ODD]:
        assert at.classify(cell) == at.ODD, cell
    assert set(at.CELLS) == set(at.CLASS_BITS)


@pytest.mark.parametrize("bits", [at.INT | at.FLOAT, at.INT | at.NA, at.FLOAT | at.NA, at.INT | at.FLOAT | at.NA, at.TEXT | at.NA])
def test_mixed_classes_predict_the_dtype(bits):
    cells = [c for b in (at.INT, at.FLOAT, at.NA, at.TEXT) if bits & b for c in at.CELLS[b]]
    assert str(_one_column(cells).dtype) == at.dtype_of(bits)


def test_the_value_is_pandas_value():
    """the model's value of every INT and FLOAT cell that is decided is within 2^-50 of what pandas parses"""
    for cell in at.CELLS[at.INT] + at.CELLS[at.FLOAT] + tuple(c for t in at.THRESHOLDS for c in at.threshold_cells(t)):
        v, undecided = at.value_of(cell)
        got = float(_one_column([cell, b"0.5"])[0])
        if undecided:
            assert got == 0 or abs(got) < 1e-299 or abs(got) > 1e299, cell
        elif v == 0:
            assert got == 0, cell
        else:
            assert abs(got / float(v) - 1) <= 2.0 ** -50, (cell, got, float(v))


def _pandas_keeps(text, thr):
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        a = pd.read_csv(io.BytesIO(text), sep="\t", index_col=0)
    col = a.columns[at.PVALUE_FIELD - 1]
    return a[col].tolist(), (a[col] <= thr).tolist()


@pytest.mark.parametrize("thr", at.THRESHOLDS, ids=THR_IDS)
def test_the_model_keeps_a_superset_of_pandas(thr):
    """on every case table whose rows are pandas' rows one to one (no flag) and whose p-values pandas can compare (no text
    or ODD cell among them): every row pandas keeps is kept, and a row kept beside those is undecided -- outside 1e-300 ..
    1e300, kept whatever the threshold -- or within the 2^-30 band above the threshold"""
    seen = set()
    for name, text in at.case_tables(thr).items():
        m = at.scan(text, at.PVALUE_FIELD, thr)
        if name in at.FLAGGED or m.classes[at.PVALUE_FIELD] & (at.TEXT | at.ODD):
            assert name in at.HOST_TABLES      # (pandas reads such p-values as text: its comparison raises, here as in the tools)
            continue
        rows = at.data_lines(text)
        values, keeps = _pandas_keeps(text, thr)
        assert len(keeps) == len(rows), name
        assert m.flags == 0, name
        kept = set(m.kept.split(b"\n"))
        for row, value, keep in zip(rows, values, keeps):
            cell = row.split(b"\t")[at.PVALUE_FIELD]
            if keep:
                assert row in kept, (name, cell)
                seen.add("kept")
            elif row in kept:
                undecided = at.classify(cell) & (at.INT | at.FLOAT) and at.value_of(cell)[1]
                assert undecided or abs(value - thr) <= abs(thr) * 2.0 ** -29, (name, cell)
                seen.add("undecided" if undecided else "band")
            else:
                seen.add("dropped")
    # (1e-320 is undecided: pandas keeps it too down to 1e-12, and drops it at 0, -1 and nan, where the model's row is an extra)
    want = {"dropped", "undecided"} if math.isnan(thr) else {"kept"} if math.isinf(thr) else {"kept", "dropped"}
    if thr in (1.0, 0.05, 1e-12, -1.0):
        want = want | {"band"}
    if thr in (0.0, -1.0):
        want = want | {"undecided"}
    assert want <= seen


def test_the_case_tables_reach_every_class_flag_and_spelling():
    tables = dict(at.case_tables(), **at.long_tables())
    classes, flags = 0, 0
    for name, text in tables.items():
        m = at.scan(text, at.PVALUE_FIELD, 0.05)
        classes |= m.classes[at.PVALUE_FIELD] | m.classes[7] | m.classes[0]
        flags |= m.flags
        assert (m.flags != 0) == (name in at.FLAGGED or name in at.long_tables()), name
        if name in at.FLAGGED:
            assert m.flags == at.FLAGGED[name], name
    assert classes == sum(at.CLASS_BITS) and flags == sum(at.ROW_BITS)
    assert at.scan(at.long_tables()["field_5000"], at.PVALUE_FIELD, 0.05).flags == at.ROW_LONG
    assert at.scan(at.long_tables()["line_70000"], at.PVALUE_FIELD, 0.05).flags == at.ROW_LONG
    cells = {r.split(b"\t")[at.PVALUE_FIELD] for r in at.data_lines(tables["spellings"])}
    assert set(at.PVALUE_SPELLINGS) <= cells and set(at.threshold_cells(0.05)) <= cells
    odd = {r.split(b"\t")[at.PVALUE_FIELD] for r in at.data_lines(tables["odd_pvalue"])}
    assert {b"1e400", b"1234567890123456789012345e-30"} <= odd


def test_the_seeded_table_reaches_every_seam():
    for skew in (0, len(at.HEADER)):
        text = at.seeded_table(5, skew=skew)
        assert 190_000 < len(text) < 215_000
        body = text[len(at.HEADER):]
        assert at.seam_classes(body, skew=skew) >= {(s, p) for s in at.SEAMS for p in at.PARTS}
        m = at.scan(text, at.PVALUE_FIELD, 1e-8)
        assert m.flags == 0 and 0 < m.n_kept < m.rows and at.dtype_of(m.classes[at.PVALUE_FIELD]) == "float64"


# ------------------------------------------------------------------------------------------------ the package's routing
def _args(path, thr, output=None, column="lrt-pvalue", host=False):
    return argparse.Namespace(associations=str(path), threshold=thr, column=column, output=output, device=0, host_gunzip=False,
                              host_associations=host)


def _whole_file(path, thr, output, index_name):
    """the reference's statements (get_clusters.py:76-88, get_kmers.py:93-106)"""
    a = pd.read_csv(path, sep="\t", index_col=0)
    if index_name:
        a.index.name = index_name
    a = a[a["lrt-pvalue"] <= thr]
    a.to_csv(output, sep="\t")
    return a, [str(x) for x in a.index.unique()]


def _outcome(fn):
    try:
        a, passing = fn()
        return a.to_csv(sep="\t"), passing, None
    except Exception as e:                        # (a word among the p-values: the comparison itself fails, either way)
        return None, None, type(e)


@pytest.mark.parametrize("thr", at.THRESHOLDS, ids=THR_IDS)
@pytest.mark.parametrize("index_name", [None, "hashed_pattern"])
def test_the_routing_prints_what_the_whole_file_prints(tmp_path, thr, index_name):
    """_associations with the model's kept lines and class bits in the device's place: the table, the -o file and the
    passing list are those of the reference's statements on the whole file; the tables take the route their cells say"""
    from panfeed_amd import downstream as ds
    for name, text in at.case_tables(thr).items():
        path = tmp_path / f"{name}.tsv"
        path.write_bytes(text)

        def model_scan(args, field, names):
            assert field == at.PVALUE_FIELD and len(names) == 8
            m = at.scan(text, field, args.threshold)
            return m.kept, {"classes": m.classes, "flags": m.flags, "rows": m.rows, "kept": m.n_kept}, None

        o1, o2 = tmp_path / f"{name}.got", tmp_path / f"{name}.exp"
        before = (ds.AssocFilter.device_files, ds.AssocFilter.host_files)
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            got = _outcome(lambda: ds._associations(_args(path, thr, str(o1)), index_name, scan=model_scan))
            exp = _outcome(lambda: _whole_file(str(path), thr, str(o2), index_name))
        moved = (ds.AssocFilter.device_files - before[0], ds.AssocFilter.host_files - before[1])
        assert got == exp, name
        assert moved == ((0, 1) if name in at.HOST_TABLES else (1, 0)), name
        if exp[2] is None:
            assert o1.read_bytes() == o2.read_bytes(), name
    t = at.case_tables(thr)["int_blank_in_dropped_row"]
    if thr == 0.05:
        path = tmp_path / "int_blank_in_dropped_row.got"
        assert b"\t1.0\tn\n" in path.read_bytes() and b"\t1\tn\n" in t


def test_host_option_missing_column_and_odd_headers(tmp_path):
    from panfeed_amd import downstream as ds
    text = at.case_tables()["spellings"]
    path = tmp_path / "a.tsv"
    path.write_bytes(text)

    def no_scan(args, field, names):
        raise AssertionError("a device pass")

    before = ds.AssocFilter.host_files
    a, passing = ds._associations(_args(path, 0.05, host=True), scan=no_scan)
    assert ds.AssocFilter.host_files == before + 1 and passing == _whole_file(str(path), 0.05, str(tmp_path / "o"), None)[1]
    for column in ("no-such-column", "variant"):
        with pytest.raises(SystemExit) as ei:
            ds._associations(_args(path, 0.05, column=column), scan=no_scan)
        assert ei.value.code == 1
    for header in (b"variant\taf\taf\tlrt-pvalue\n", b"variant\t\tlrt-pvalue\n", b'variant\t"af"\tlrt-pvalue\n', b"variant\tlrt-pvalue\r\n"):
        assert ds.assoc_header(header) is None
        path.write_bytes(header + b"h1\t1\t0.5\t0.01\n"[:None if header.count(b"\t") == 3 else -5] )
    assert ds.assoc_header(at.HEADER) == at.HEADER.decode().rstrip("\n").split("\t")
    assert ds.assoc_header(b"") is None and ds.assoc_header(b"a\tb") is None
    for opts in (ds._options("x", False), ds._options("x", True)):
        argv = ["-a", "a", "-p", "p", "--host-associations"] + (["-k", "k"] if any(a.dest == "kmers" for a in opts._actions) else [])
        assert opts.parse_args(argv).host_associations is True


def test_the_golden_associations_take_the_device_route():
    """the four associations texts of tests/golden/n4.json.gz have no flag and no cell that sends them through pandas whole:
    the GPU tests over them cannot pass by falling back"""
    from panfeed_amd import downstream as ds
    with gzip.open(os.path.join(GOLDEN, "n4.json.gz"), "rb") as fh:
        fixtures = json.loads(fh.read().decode())["fixtures"]
    texts = {f["associations"] for f in fixtures}
    assert len(fixtures) == 4
    for text in texts:
        raw = text.encode()
        names = ds.assoc_header(raw.split(b"\n", 1)[0] + b"\n")
        assert names is not None and "lrt-pvalue" in names[1:]
        field = names.index("lrt-pvalue")
        for thr in (1.0, 0.01, 1e-30):
            m = at.scan(raw, field, thr)
            dtypes, why = ds.assoc_plan(names, field, m.classes, m.flags, m.rows)
            assert m.flags == 0 and dtypes is not None, why
