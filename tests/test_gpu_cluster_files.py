"""--multiple-files from device text: the per-cluster files cut from the bodies the GPU wrote
(Engine.render_device_clusters, pf_kmers_tsv_seq_ends, output.ClusterSplitter) against the reference's own files, the
host renderers' trees and the oracle."""
import gzip
import os

import numpy as np
import pytest

from conftest import all_cases, case_records

pytestmark = pytest.mark.gpu

FILES = ("kmers.tsv", "kmers_to_hashes.tsv", "hashes_to_patterns.tsv")
GOLDEN = [c for c in all_cases() if c["name"] in ("rand12_mf", "edge_k5_mf")]


def _headers(strains):
    from panfeed_amd.engine import KMERS_TO_HASHES_HEADER, KMERS_TSV_HEADER, hashes_to_patterns_header
    return dict(zip(FILES, (KMERS_TSV_HEADER, KMERS_TO_HASHES_HEADER, hashes_to_patterns_header(strains))))


def _engine(o, max_strains, **kw):
    from panfeed_amd.engine import Engine
    return Engine(klength=o["klength"], canon=o["canon"], consider_missing=o["consider_missing"], patfilt=o["patfilt"],
                  maf=o["maf"], multiple_files=True, max_strains=max_strains, stroi=set(o["stroi"]) if o["stroi"] else (), **kw)


def _tree(root):
    """{relative path: bytes} of every file under root"""
    out = {}
    for d, _dirs, files in os.walk(root):
        for f in files:
            p = os.path.join(d, f)
            with open(p, "rb") as fh:
                out[os.path.relpath(p, root)] = fh.read()
    return out


def _check_ends(text, ends, n_clusters):
    ends = [int(e) for e in ends]
    assert len(ends) == n_clusters
    assert all(a <= b for a, b in zip(ends, ends[1:]))
    assert (ends[-1] if ends else 0) == len(text)
    assert b"".join(bytes(text[a:b]) for a, b in zip([0] + ends, ends)) == bytes(text)


# ---------------------------------------------------------------------------------------------- reference goldens
@pytest.mark.parametrize("case", GOLDEN, ids=[c["name"] for c in GOLDEN])
def test_reference_goldens(case):
    assert len(GOLDEN) == 2 and case["opts"]["multiple_files"]
    ms = max(32, (len(case["all_strains"]) + 31) // 32 * 32)
    heads = _headers(case["all_strains"])
    recs = case_records(case)
    eng = _engine(case["opts"], ms)
    seen, on_device = [], 0
    for out in eng.run_stream(recs, batch_clusters=3, device_text=True):
        on_device += out.stats["device_cluster_files"]
        assert out.stats["device_cluster_files"] == out.stats["clusters"] == len(out.per_cluster)
        assert b"".join(bytes(kh) for _i, _kt, kh, _hp in out.per_cluster) == bytes(out.kmers_to_hashes)
        assert b"".join(bytes(hp) for _i, _kt, _kh, hp in out.per_cluster) == bytes(out.hashes_to_patterns)
        for idx, kt, kh, hp in out.per_cluster:
            seen.append(idx)
            for f, body in zip(FILES, (kt, kh, hp)):
                assert heads[f] + bytes(body).decode() == case["expect"]["dirs"][idx][f], (idx, f)
    assert seen == [r[1] for r in recs] and on_device == len(recs)
    eng.close()


@pytest.mark.parametrize("case", GOLDEN, ids=[c["name"] for c in GOLDEN])
def test_render_device_clusters_directly(case):
    from panfeed_amd import _lib
    from panfeed_amd.engine import Engine
    from panfeed_amd.packing import build_batch_native
    ms = max(32, (len(case["all_strains"]) + 31) // 32 * 32)
    o = case["opts"]
    recs = case_records(case)
    eng = _engine(o, ms)
    hb = build_batch_native(recs, o["klength"], o["canon"], eng.W, stroi=eng.stroi, first_ordinal=5)
    eng.submit_host_batch(hb)
    kh, hp, kh_end, hp_end = eng.render_device_clusters(hb)
    assert isinstance(kh, memoryview) and isinstance(hp, memoryview)
    assert kh_end.dtype == np.uint64 and hp_end.dtype == np.uint64
    _check_ends(kh, kh_end, len(recs))
    _check_ends(hp, hp_end, len(recs))
    heads = _headers(case["all_strains"])
    for i, (a, b) in enumerate(zip([0] + list(hp_end), hp_end)):
        assert heads[FILES[2]] + bytes(hp[int(a):int(b)]).decode() == case["expect"]["dirs"][recs[i][1]][FILES[2]]
    # the target strains' rows: per-sequence ends from the library, per-cluster ends from the engine
    text = bytes(eng.render_targets_device(hb))
    kt_end = eng.target_cluster_ends(hb)
    _check_ends(text, kt_end, len(recs))
    n = hb.n_targets
    ends = np.zeros(max(n, 1), dtype=np.uint64)
    _lib.check(eng.L.pf_kmers_tsv_seq_ends(eng.ctx, ends.ctypes.data, n))
    assert n > 0 and all(a <= b for a, b in zip(ends[:n], ends[1:n])) and int(ends[n - 1]) == len(text)
    assert set(int(e) for e in kt_end) <= {0} | set(int(e) for e in ends[:n])
    for e in ends[:n]:
        assert int(e) == 0 or text[int(e) - 1:int(e)] == b"\n"       # every end stands behind a row
    for i, (a, b) in enumerate(zip([0] + list(kt_end), kt_end)):
        assert heads[FILES[0]] + text[int(a):int(b)].decode() == case["expect"]["dirs"][recs[i][1]][FILES[0]]
    with pytest.raises(_lib.PanfeedHipError) as e:                     # another number of sequences than the text's
        _lib.check(eng.L.pf_kmers_tsv_seq_ends(eng.ctx, ends.ctypes.data, n + 1))
    assert e.value.status == _lib.ERR_ARG
    eng.submit_host_batch(hb)                                           # a new batch: the ends are gone
    with pytest.raises(_lib.PanfeedHipError) as e:
        _lib.check(eng.L.pf_kmers_tsv_seq_ends(eng.ctx, ends.ctypes.data, n))
    assert e.value.status == _lib.ERR_STATE
    eng.close()
    # the call is the multiple_files one; pf_render_device keeps refusing that mode
    one = Engine(klength=o["klength"], canon=o["canon"], max_strains=ms, stroi=eng.stroi)
    one.submit_host_batch(hb)
    with pytest.raises(_lib.PanfeedHipError) as e:
        one.render_device_clusters(hb)
    assert e.value.status == _lib.ERR_ARG
    one.close()
    mf = _engine(o, ms)
    mf.submit_host_batch(hb)
    with pytest.raises(_lib.PanfeedHipError) as e:
        mf.render_device(hb)
    assert e.value.status == _lib.ERR_ARG
    mf.close()


# ---------------------------------------------------------------------------------------------- device against host
UP, DOWN = 40, 30


@pytest.fixture(scope="module")
def pangenome(tmp_path_factory):
    from panfeed_amd import synth
    root = tmp_path_factory.mktemp("pg")
    # n_rate: a fifth of the sequences have an 'N' (slow-path k-mers, host-rendered target sequences)
    cl = synth.generate(14, 24, first=921, flank=0, mean_len=450, min_len=80, max_len=1000, n_rate=0.2, paralog_rate=0.05)
    names = cl[0].names
    csvp, gffs, _fas = synth.write_pangenome(str(root), cl)
    return {"csv": csvp, "gffs": str(root / "gffs"), "gff_of": gffs, "clusters": cl, "names": names,
            "targets": tuple(names[i] for i in range(0, 24, 2)), "host": {}}


def _run(pg, out, k=21, canon=True, targets=None, **kw):
    from panfeed_amd.pipeline import run_files
    return run_files(pg["csv"], pg["gffs"], str(out), klength=k, canon=canon, multiple_files=True,
                     targets=pg["targets"] if targets is None else targets, upstream=UP, downstream=DOWN, **kw)


def _host_tree(pg, tmp_path_factory, k, canon, missing):
    """the tree the host renderers write (computed once per mode, left unchanged)"""
    key = (k, canon, missing)
    if key not in pg["host"]:
        out = tmp_path_factory.mktemp("host") / "out"
        st = _run(pg, out, k, canon, consider_missing=missing, device_text=False)
        assert st["device_cluster_files"] == 0
        pg["host"][key] = (_tree(out), st)
    return pg["host"][key]


MODES = [(21, True, False), (17, False, False), (21, True, True)]
MODE_IDS = ["k21_canonical", "k17_non_canonical", "k21_consider_missing"]


@pytest.mark.parametrize("batch_clusters", [1, 4, 256])
@pytest.mark.parametrize("k,canon,missing", MODES, ids=MODE_IDS)
def test_device_tree_equals_host_tree(pangenome, tmp_path, tmp_path_factory, k, canon, missing, batch_clusters):
    host, hst = _host_tree(pangenome, tmp_path_factory, k, canon, missing)
    out = tmp_path / "out"
    st = _run(pangenome, out, k, canon, consider_missing=missing, device_text=True, batch_clusters=batch_clusters)
    assert st["clusters"] == 14 and st["device_cluster_files"] == 14
    got = _tree(out)
    assert sorted(got) == sorted(host) and len(got) == 3 * 14
    for name in host:
        assert got[name] == host[name], name
    assert st["bytes"] == hst["bytes"]
    if missing:
        # NaN cells make rows of varying length: the case is only worth its name if some row has one
        rows = b"".join(v for n, v in got.items() if n.endswith(FILES[2]))
        assert b"\t\t" in rows or b"\t\n" in rows


def test_device_tree_equals_the_oracle(pangenome, tmp_path):
    from oracle import input_restatement as ir
    from oracle import oracle as po
    out = tmp_path / "out"
    st = _run(pangenome, out, 21, True, device_text=True, batch_clusters=4)
    assert st["device_cluster_files"] == 14
    gffs = pangenome["gff_of"]
    gn = sorted(gffs)
    strains, table = ir.load_table(pangenome["csv"])
    recs = list(ir.iter_gene_clusters(strains, table, ir.load_genomes(gn, [gffs[n] for n in gn]), UP, DOWN, False))
    assert sorted(os.listdir(out)) == sorted(r[1] for r in recs) and len(recs) == 14
    heads = _headers(strains)
    for rec in recs:
        run = po.OracleRun(klength=21, stroi=set(pangenome["targets"]), multiple_files=True)
        run.feed([rec])
        for f, body in zip(FILES, run.texts()):
            with open(out / rec[1] / f, newline="") as fh:
                assert fh.read() == heads[f] + body, (rec[1], f)


# ---------------------------------------------------------------------------------------------- pattern reset
def test_pattern_set_starts_empty_in_every_cluster():
    """two clusters of identical content under different names in one batch: the second one's hashes_to_patterns.tsv
    holds every row again, and hp_end cuts where the oracle does"""
    from oracle import oracle as po
    from panfeed_amd import synth
    from panfeed_amd.engine import Engine
    from panfeed_amd.packing import build_batch_native
    cl = synth.generate(2, 40, first=311, mean_len=300, min_len=100, max_len=600, n_rate=0.02, paralog_rate=0.05)
    a, other = cl[0].record(), cl[1].record()
    recs = [a, (a[0], "the_same_again", a[2]), other]
    want = []
    for rec in recs:
        run = po.OracleRun(klength=21, multiple_files=True)
        run.feed([rec])
        want.append(run.texts())
    assert want[0][2] == want[1][2] and want[0][2].count("\n") > 1
    eng = Engine(klength=21, max_strains=64, multiple_files=True)
    outs = list(eng.run_stream(recs, batch_clusters=3, device_text=True))
    assert len(outs) == 1 and outs[0].stats["device_cluster_files"] == 3
    for (idx, kt, kh, hp), rec, (ek, ekh, ehp) in zip(outs[0].per_cluster, recs, want):
        assert idx == rec[1]
        assert (bytes(kh).decode(), bytes(hp).decode()) == (ekh, ehp), idx
    hb = build_batch_native(recs, 21, True, eng.W, first_ordinal=eng.next_ordinal)
    eng.submit_host_batch(hb)
    _kh, hp, kh_end, hp_end = eng.render_device_clusters(hb)
    sizes = [len(w[2]) for w in want]
    assert [int(e) for e in hp_end] == [sizes[0], 2 * sizes[0], 2 * sizes[0] + sizes[2]]
    assert [int(e) for e in kh_end] == list(np.cumsum([len(w[1]) for w in want]))
    eng.close()


# ---------------------------------------------------------------------------------------------- ranged kmers.tsv
def test_ranged_kmers_tsv(pangenome, tmp_path, tmp_path_factory):
    from panfeed_amd import engine, output
    host, _ = _host_tree(pangenome, tmp_path_factory, 21, True, False)
    streams, blocks = [], []
    real_stream, real_splitter = engine.Engine.stream_targets_device, output.ClusterSplitter

    def spy_stream(self, hb, sink, budget=None, **kw):
        r = real_stream(self, hb, sink, budget, **kw)
        streams.append(r)
        return r

    class SpySplitter(real_splitter):
        """which clusters every block's pieces went to"""

        def __init__(self, ends, names, sink):
            def spy(name, piece):
                if len(piece):
                    blocks[-1].append(name)
                sink(name, piece)
            super().__init__(ends, names, spy)

        def __call__(self, block):
            blocks.append([])
            super().__call__(block)

    engine.Engine.stream_targets_device, output.ClusterSplitter = spy_stream, SpySplitter
    try:
        out = tmp_path / "out"
        st = _run(pangenome, out, 21, True, device_text=True, targets_text_budget=768 << 10)
    finally:
        engine.Engine.stream_targets_device, output.ClusterSplitter = real_stream, real_splitter
    assert st["device_cluster_files"] == 14
    assert max(r[1] for r in streams) > 1                                  # kmers_tsv_ranges
    assert any(len(set(b)) >= 2 for b in blocks)                            # a block with rows of two clusters
    per_cluster = {}
    for b in blocks:
        for name in set(b):
            per_cluster[name] = per_cluster.get(name, 0) + 1
    assert max(per_cluster.values()) >= 2                                   # a cluster that received two blocks
    got = _tree(out)
    assert sorted(got) == sorted(host)
    for name in host:
        assert got[name] == host[name], name


# ---------------------------------------------------------------------------------------------- no target rows
def test_cluster_without_target_rows(pangenome, tmp_path):
    from panfeed_amd.engine import KMERS_TSV_HEADER
    cl, names = pangenome["clusters"], pangenome["names"]
    # from the synthetic table: the cluster fewest strains have, and targets among the strains it lacks
    least = min(cl, key=lambda c: int(c.present.sum()))
    targets = tuple(names[i] for i in np.flatnonzero(~least.present)[:3])
    assert targets
    without = [c.idx for c in cl if not any(c.present[names.index(t)] for t in targets)]
    with_rows = [c.idx for c in cl if any(c.present[names.index(t)] for t in targets)]
    assert least.idx in without and with_rows
    outs = {}
    for device_text in (True, False):
        outs[device_text] = tmp_path / f"out{int(device_text)}"
        st = _run(pangenome, outs[device_text], 21, True, targets=targets, device_text=device_text, batch_clusters=4)
        assert st["device_cluster_files"] == (14 if device_text else 0)
    for idx in without:
        assert (outs[True] / idx / "kmers.tsv").read_bytes() == KMERS_TSV_HEADER.encode(), idx
    assert any(len((outs[True] / idx / "kmers.tsv").read_bytes()) > len(KMERS_TSV_HEADER) for idx in with_rows)
    assert _tree(outs[True]) == _tree(outs[False])


# ---------------------------------------------------------------------------------------------- compress
def test_compress_keeps_the_hosts_gzip(pangenome, tmp_path, tmp_path_factory):
    host, _ = _host_tree(pangenome, tmp_path_factory, 21, True, False)
    for name, kw in (("gz", {"compress": True}), ("gpu", {"device_gzip": True})):
        out = tmp_path / name
        st = _run(pangenome, out, 21, True, device_text=True, **kw)
        assert st["device_cluster_files"] == 14
        assert "compressed_bytes" not in st
        got = _tree(out)
        assert sorted(got) == sorted(n + ".gz" for n in host)
        for n in host:
            assert gzip.decompress(got[n + ".gz"]) == host[n], n


# ---------------------------------------------------------------------------------------------- word boundaries
@pytest.mark.parametrize("missing", [False, True], ids=["plain", "consider_missing"])
@pytest.mark.parametrize("strains", [33, 65])
def test_last_word_of_one_cell(strains, missing):
    """33 and 65 strains: the last 32-cell word of a pattern row is one cell long"""
    from panfeed_amd import synth
    from panfeed_amd.engine import Engine
    cl = synth.generate(5, strains, first=4242, mean_len=250, min_len=80, max_len=500, n_rate=0.05, paralog_rate=0.05)
    recs = [c.record() for c in cl]
    stroi = {cl[0].names[0], cl[0].names[strains - 1]}
    got = {}
    for device_text in (True, False):
        eng = Engine(klength=21, max_strains=(strains + 31) // 32 * 32, multiple_files=True, consider_missing=missing,
                     stroi=stroi)
        got[device_text] = []
        for out in eng.run_stream(recs, batch_clusters=2, device_text=device_text):
            assert out.stats["device_cluster_files"] == (out.stats["clusters"] if device_text else 0)
            for idx, kt, kh, hp in out.per_cluster:
                got[device_text].append((idx,) + tuple(x if isinstance(x, str) else bytes(x).decode() for x in (kt, kh, hp)))
        eng.close()
    assert len(got[True]) == 5 and got[True] == got[False]
    width = {row.count("\t") for _i, _kt, _kh, hp in got[True] for row in hp.splitlines()}
    assert strains in width                                                 # rows of all `strains` cells were written
