"""kmers.tsv rows of passing patterns only (pf_set_passing_hashes, Engine(passing_hashes=), run_files(passing_hashes=),
--passing-hashes / --passing-associations): the GPU marks the kept k-mers whose pattern digest is in the passing set,
indexes them by (cluster, key) and the row kernels drop every row whose pair is not there.  Expected texts are the CPU
oracle's, filtered by passing_cases.filter_rows -- never by the code under test."""
import contextlib
import ctypes as C
import gzip
import io
import os

import numpy as np
import pytest

import passing_cases as pc

pytestmark = pytest.mark.gpu

BUDGET = 768 << 10
NO_ROW_HAS = "AAAAAAAAAAAAAAAAAAAAAA=="          # the digest of sixteen zero bytes


def _run(c, passing, budget, sink, device_text=True):
    from panfeed_amd import native_input as ni
    from panfeed_amd.engine import Engine
    eng = Engine(klength=c.k, canon=c.canon, max_strains=32, stroi=set(c.targets), targets_text_budget=budget,
                 passing_hashes=passing)
    try:
        with ni.Pangenome(c.csvp, c.gffdir, None, pc.UP, pc.DOWN, False, targets=c.targets) as pg:
            outs = list(eng.run_pangenome(pg, batch_clusters=256, device_text=device_text, targets_sink=sink))
    finally:
        eng.close()
    assert len(outs) == 1
    return outs[0]


@contextlib.contextmanager
def _submitted(c, passing=None):
    """(engine, the case's one batch) with the batch submitted: texts of it may be asked for any number of times"""
    from panfeed_amd import native_input as ni
    from panfeed_amd.engine import Engine
    eng = Engine(klength=c.k, canon=c.canon, max_strains=32, stroi=set(c.targets), passing_hashes=passing)
    try:
        with ni.Pangenome(c.csvp, c.gffdir, None, pc.UP, pc.DOWN, False, targets=c.targets) as pg:
            hbs = list(pg.batches(c.k, c.canon, eng.W, max_clusters=256, first_ordinal=0))
            assert len(hbs) == 1
            eng.submit_host_batch(hbs[0])
            yield eng, hbs[0]
    finally:
        eng.close()


@pytest.mark.parametrize("k", sorted(pc.TABLE), ids=lambda k: f"k{k}")
def test_ranges_single_range_and_single_buffer_equal_the_oracles_filter(k):
    c = pc.case(k)
    want = pc.text_of(pc.check_conditions(c))
    passing = pc.every_second(c)
    got = bytearray()
    st = _run(c, passing, BUDGET, got.extend).stats
    print(k, "ranges", st["kmers_tsv_ranges"], "peak", st["kmers_tsv_peak_device_bytes"], "considered",
          st["kmers_rows_considered"], "kept", st["kmers_rows_kept"], "bytes", len(got), "want", len(want))
    assert st["kmers_tsv_ranges"] > 1
    assert got.decode() == want
    assert (st["kmers_rows_considered"], st["kmers_rows_kept"]) == pc.TABLE[k][2:3] + pc.TABLE[k][4:5]
    assert st["passing_digests"] == len(passing)
    assert 0 < st["kmers_tsv_peak_device_bytes"] <= BUDGET
    assert st["kmers_tsv_streamed"] == len(got)
    one = bytearray()
    st = _run(c, passing, 8 << 30, one.extend).stats
    assert st["kmers_tsv_ranges"] == 1 and bytes(one) == bytes(got)
    out = _run(c, passing, 8 << 30, None)
    assert bytes(out.kmers_tsv) == bytes(got)
    assert out.stats["kmers_rows_kept"] == pc.TABLE[k][4]


def test_lists_of_one_none_no_and_every_hash():
    c = pc.case(21)
    first = c.kh.split("\n")
    first = next(ln.split("\t")[2] for ln in first if ln and ln.split("\t")[1])
    assert NO_ROW_HAS not in c.hashes
    with _submitted(c, []) as (eng, hb):
        for name, passing in (("one", [first]), ("no row has", [NO_ROW_HAS]), ("empty", []), ("every", c.hashes)):
            want = pc.filter_rows(c, passing)
            eng.set_passing_hashes(passing)
            got = bytearray()
            n, ranges, peak = eng.stream_targets_device(hb, got.extend, budget=BUDGET)
            stats = eng.passing_stats()
            print(name, "rows", len(want), "bytes", n, "ranges", ranges, "stats", stats)
            assert got.decode() == pc.text_of(want), name
            assert stats[0] == len(set(passing)) and stats[2] == len(c.rows) and stats[3] == len(want)
            assert bytes(eng.render_targets_device(hb)).decode() == pc.text_of(want), name
        # most tiles came out empty under the list of one: a tile holds rows of one sequence, and few sequences keep any
        seq_of = lambda r: tuple(r.split("\t", 3)[:3])
        assert 0 < 4 * len({seq_of(r) for r in pc.filter_rows(c, [first])}) < len({seq_of(r) for r in c.rows})
        assert len(pc.filter_rows(c, c.hashes)) == pc.TABLE[21][3] < len(c.rows)


def test_filter_off_after_on_and_state_rules():
    from panfeed_amd import _lib
    c = pc.case(21)
    with _submitted(c, pc.every_second(c)) as (eng, hb):
        assert bytes(eng.render_targets_device(hb)).decode() == pc.text_of(pc.filter_rows(c, pc.every_second(c)))
        eng.set_passing_hashes(None)
        assert bytes(eng.render_targets_device(hb)).decode() == c.kt
        got = bytearray()
        eng.stream_targets_device(hb, got.extend, budget=BUDGET)
        assert got.decode() == c.kt
        # while a stream is open the set cannot change
        eng.set_passing_hashes(pc.every_second(c))
        eng._passing_names(hb)
        with eng._target_records(hb) as (arr, n):
            total, ranges, peak = C.c_uint64(), C.c_uint32(), C.c_uint64()
            _lib.check(eng.L.pf_kmers_tsv_stream_begin(eng.ctx, arr, n, BUDGET, C.byref(total), C.byref(ranges), C.byref(peak)))
            assert eng.L.pf_set_passing_hashes(eng.ctx, None, 0) == _lib.ERR_STATE
            assert eng.L.pf_clear_passing_hashes(eng.ctx) == _lib.ERR_STATE
            assert eng.L.pf_debug_passing_hash_bits(eng.ctx, 8) == _lib.ERR_STATE
            ptr, nb = C.c_void_p(), C.c_uint64()
            size = 0
            while True:
                _lib.check(eng.L.pf_kmers_tsv_stream_next(eng.ctx, C.byref(ptr), C.byref(nb)))
                if not nb.value:
                    break
                size += nb.value
            assert size == total.value == len(pc.text_of(pc.filter_rows(c, pc.every_second(c))))
        assert eng.L.pf_debug_passing_hash_bits(eng.ctx, 65) == _lib.ERR_ARG


@pytest.mark.parametrize("k", [21, 33], ids=lambda k: f"k{k}")
def test_narrow_hashes_reach_the_compare_and_reject_branch(k):
    from panfeed_amd import _lib
    c = pc.case(k)
    passing = pc.every_second(c)
    want = pc.text_of(pc.filter_rows(c, passing))
    with _submitted(c, passing) as (eng, hb):
        for bits in (64, 4, 0):
            _lib.check(eng.L.pf_debug_passing_hash_bits(eng.ctx, bits))
            got = bytes(eng.render_targets_device(hb)).decode()
            stats = eng.passing_stats()
            print(k, "bits", bits, "stats", stats)
            assert got == want, bits
            if bits < 64:
                assert stats[4] > 0
        _lib.check(eng.L.pf_debug_passing_hash_bits(eng.ctx, 64))


@pytest.mark.parametrize("k", [21, 17], ids=lambda k: f"k{k}")
def test_host_route_gives_the_device_routes_bytes(k):
    c = pc.case(k)
    passing = pc.every_second(c)
    want = pc.text_of(pc.filter_rows(c, passing))
    host = _run(c, passing, 8 << 30, None, device_text=False)
    assert host.kmers_tsv == want
    assert (host.stats["kmers_rows_considered"], host.stats["kmers_rows_kept"]) == (len(c.rows), pc.TABLE[k][4])
    assert bytes(_run(c, passing, 8 << 30, None).kmers_tsv).decode() == host.kmers_tsv
    assert host.kmers_to_hashes == c.kh and host.hashes_to_patterns == c.hp


def test_sequence_ends_under_the_filter():
    from panfeed_amd import _lib
    c = pc.case(21)
    first = next(ln.split("\t")[2] for ln in c.kh.split("\n") if ln and ln.split("\t")[1])
    for passing in (pc.every_second(c), [first]):
        kept = pc.filter_rows(c, passing)
        by_seq = {}
        for r in kept:
            by_seq.setdefault(tuple(r.split("\t", 3)[:3]), []).append(r)
        with _submitted(c, passing) as (eng, hb):
            text = bytes(eng.render_targets_device(hb))
            n = hb.n_targets
            ends = np.zeros(n, dtype=np.uint64)
            _lib.check(eng.L.pf_kmers_tsv_seq_ends(eng.ctx, ends.ctypes.data, n))
            keys = [(hb.idx[m.cluster], str(m.strain), str(m.seq.id)) for m in hb.targets]
        assert len(set(keys)) == n and set(by_seq) <= set(keys)
        prev, repeats = 0, 0
        for key, e in zip(keys, ends.tolist()):
            assert text[prev:e].decode() == pc.text_of(by_seq.get(key, [])), key
            repeats += e == prev
            prev = e
        assert prev == len(text) and repeats >= n - len(by_seq)
    assert repeats >= n - len(by_seq) > 0   # the list of one: a sequence none of whose rows are kept repeats the end before it


def _inflate(path):
    with open(path, "rb") as fh:
        data = fh.read()
    return gzip.decompress(data).decode() if path.endswith(".gz") else data.decode()


def _files(out, gz):
    sfx = ".gz" if gz else ""
    return [_inflate(os.path.join(out, name + sfx)) for name in ("kmers.tsv", "kmers_to_hashes.tsv", "hashes_to_patterns.tsv")]


def test_run_files_end_to_end(tmp_path):
    from panfeed_amd.engine import KMERS_TSV_HEADER
    from panfeed_amd.pipeline import run_files
    c = pc.case(21)
    common = dict(klength=21, upstream=pc.UP, downstream=pc.DOWN, targets=c.targets)
    passing = pc.every_second(c)
    want = KMERS_TSV_HEADER + pc.text_of(pc.filter_rows(c, passing))
    run_files(c.csvp, c.gffdir, str(tmp_path / "base"), **common)
    base = _files(str(tmp_path / "base"), False)
    assert base[0] == KMERS_TSV_HEADER + c.kt
    for name, opts in (("plain", {}), ("compress", {"compress": True}), ("gpu", {"device_gzip": True}),
                       ("bgzf", {"device_gzip": True, "bgzf": True})):
        out = str(tmp_path / name)
        stats = run_files(c.csvp, c.gffdir, out, passing_hashes=passing, **common, **opts)
        got = _files(out, bool(opts))
        assert got[0] == want, name
        assert got[1:] == base[1:], name
        assert (stats["kmers_rows_considered"], stats["kmers_rows_kept"], stats["passing_digests"]) == \
            (len(c.rows), pc.TABLE[21][4], len(passing)), name
    # per-cluster directories; the first cluster keeps no row
    first_cluster = c.rows[0].split("\t", 1)[0]
    passing = [h for h in passing if h not in {h2 for (idx, _), h2 in c.pairs.items() if idx == first_cluster}]
    kept = pc.rows_by_cluster(pc.filter_rows(c, passing))
    assert first_cluster not in kept and 1 < len(kept) < len(pc.rows_by_cluster(c.rows))
    run_files(c.csvp, c.gffdir, str(tmp_path / "mbase"), multiple_files=True, **common)
    for name, opts in (("multi", {}), ("multi_gpu", {"device_gzip_clusters": True})):
        out = str(tmp_path / name)
        run_files(c.csvp, c.gffdir, out, multiple_files=True, passing_hashes=passing, **common, **opts)
        clusters = sorted(os.listdir(str(tmp_path / "mbase")))
        assert sorted(os.listdir(out)) == clusters and set(kept) <= set(clusters)
        for idx in clusters:
            got = _files(os.path.join(out, idx), bool(opts))
            assert got[0] == KMERS_TSV_HEADER + pc.text_of(kept.get(idx, [])), (name, idx)
            assert got[1:] == _files(os.path.join(str(tmp_path / "mbase"), idx), False)[1:], (name, idx)


def test_get_kmers_only_passing_prints_the_same_from_the_filtered_file(tmp_path):
    from panfeed_amd import downstream
    from panfeed_amd.cli import main
    c = pc.case(21)
    assoc = tmp_path / "associations.tsv"
    with open(assoc, "w") as fh:
        fh.write("hashed_pattern\tlrt-pvalue\n")
        for i, h in enumerate(c.hashes):
            fh.write(f"{h}\t{0.001 if i % 2 == 0 else 0.5}\n")
    targets = tmp_path / "targets.txt"
    targets.write_text("".join(t + "\n" for t in c.targets))
    argv = ["-g", c.gffdir, "-p", c.csvp, "--targets", str(targets), "-k", "21", "--upstream", str(pc.UP),
            "--downstream", str(pc.DOWN)]
    assert main(argv + ["-o", str(tmp_path / "all")]) == 0
    assert main(argv + ["-o", str(tmp_path / "some"), "--passing-associations", str(assoc), "--passing-threshold", "0.05"]) == 0
    with open(tmp_path / "some" / "kmers.tsv") as fh:
        some = fh.read()
    from panfeed_amd.engine import KMERS_TSV_HEADER
    assert some == KMERS_TSV_HEADER + pc.text_of(pc.filter_rows(c, pc.every_second(c)))
    printed = []
    for run in ("all", "some"):
        out = io.StringIO()
        assert downstream.get_kmers(["-a", str(assoc), "-p", str(tmp_path / run / "kmers_to_hashes.tsv"), "-k",
                                     str(tmp_path / run / "kmers.tsv"), "-t", "0.05", "--only-passing"], out=out) == 0
        printed.append(out.getvalue())
    assert printed[0] == printed[1] and len(printed[0].splitlines()) > pc.TABLE[21][4]
