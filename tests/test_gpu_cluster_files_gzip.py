"""--multiple-files --gpu-compress-clusters: the per-cluster files gzipped on the GPU (run_files(multiple_files=True,
device_gzip_clusters=True): Engine.render_device_cluster_members, the kmers.tsv stream's cuts, output.ClusterMemberSplitter,
MemberGzipWriter) against the plain run's tree, on the synthetic pangenome of tests/test_gpu_cluster_files.py remade here."""
import ctypes as C
import gzip
import json
import os
import subprocess
import sys
import zlib

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FILES = ("kmers.tsv", "kmers_to_hashes.tsv", "hashes_to_patterns.tsv")
UP, DOWN = 40, 30


def _tree(root):
    """{relative path: bytes} of every file under root"""
    out = {}
    for d, _dirs, files in os.walk(root):
        for f in files:
            p = os.path.join(d, f)
            with open(p, "rb") as fh:
                out[os.path.relpath(p, root)] = fh.read()
    return out


def _members(data):
    """[(member bytes, its text)] of a .gz file, member by member"""
    out = []
    while data:
        d = zlib.decompressobj(wbits=31)
        text = d.decompress(data) + d.flush()
        assert d.eof
        out.append((data[:len(data) - len(d.unused_data)], text))
        data = d.unused_data
    return out


def _headers(strains):
    from panfeed_amd.engine import KMERS_TO_HASHES_HEADER, KMERS_TSV_HEADER, hashes_to_patterns_header
    return dict(zip(FILES, (KMERS_TSV_HEADER, KMERS_TO_HASHES_HEADER, hashes_to_patterns_header(strains))))


def _header_member(text):
    return gzip.compress(text.encode(), compresslevel=9, mtime=0)


def chunk_bytes():
    from panfeed_amd import _lib
    return int(_lib.load().pf_gzip_device_chunk_bytes())


@pytest.fixture(scope="module")
def pangenome(tmp_path_factory):
    from panfeed_amd import synth
    root = tmp_path_factory.mktemp("pg")
    # n_rate: a fifth of the sequences have an 'N' (slow-path k-mers, host-rendered target sequences)
    cl = synth.generate(14, 24, first=921, flank=0, mean_len=450, min_len=80, max_len=1000, n_rate=0.2, paralog_rate=0.05)
    names = cl[0].names
    csvp, gffs, _fas = synth.write_pangenome(str(root), cl)
    return {"csv": csvp, "gffs": str(root / "gffs"), "clusters": cl, "names": names,
            "targets": tuple(names[i] for i in range(0, 24, 2)), "plain": {}}


def _run(pg, out, k=21, canon=True, targets=None, **kw):
    from panfeed_amd.pipeline import run_files
    return run_files(pg["csv"], pg["gffs"], str(out), klength=k, canon=canon, multiple_files=True,
                     targets=pg["targets"] if targets is None else targets, upstream=UP, downstream=DOWN, **kw)


def _plain_tree(pg, tmp_path_factory, k, canon):
    """the plain run's tree and counters (computed once per mode, left unchanged)"""
    key = (k, canon)
    if key not in pg["plain"]:
        out = tmp_path_factory.mktemp("plain") / "out"
        st = _run(pg, out, k, canon, device_text=True)
        assert st["device_cluster_files"] == 14 and "compressed_bytes" not in st
        pg["plain"][key] = (_tree(out), st)
    return pg["plain"][key]


def _check_tree(got, plain):
    """every <cluster>/<file>.gz decompresses to the plain run's file; names as with compress=True"""
    assert sorted(got) == sorted(n + ".gz" for n in plain) and len(got) == 3 * 14
    for n in plain:
        assert gzip.decompress(got[n + ".gz"]) == plain[n], n


MODES = [(21, True), (17, False)]
MODE_IDS = ["k21_canonical", "k17_non_canonical"]


@pytest.mark.parametrize("batch_clusters", [1, 4, 256])
@pytest.mark.parametrize("k,canon", MODES, ids=MODE_IDS)
def test_gzip_tree_decompresses_to_the_plain_tree(pangenome, tmp_path, tmp_path_factory, k, canon, batch_clusters):
    plain, pst = _plain_tree(pangenome, tmp_path_factory, k, canon)
    out = tmp_path / "out"
    st = _run(pangenome, out, k, canon, device_gzip_clusters=True, batch_clusters=batch_clusters)
    got = _tree(out)
    _check_tree(got, plain)
    assert st["clusters"] == 14 and st["device_cluster_files"] == 14
    assert st["bytes"] == pst["bytes"]
    print(f"k={k} batch_clusters={batch_clusters}: {st['bytes']} bytes of text, {st['compressed_bytes']} compressed")
    assert 0 < st["compressed_bytes"] < st["bytes"]
    # the count is the encoder's (and the writers', for host-made members): what the files hold behind their header members
    heads = _headers(pangenome["names"])
    C_ = chunk_bytes()
    behind = 0
    for name, data in got.items():
        ms = _members(data)
        head = _header_member(heads[os.path.basename(name)[:-3]])
        assert ms[0][0] == head, name                       # the header line: a member the host made
        behind += len(data) - len(head)
        # every member behind it is one the device decoder takes
        assert all(len(text) <= C_ for _m, text in ms[1:]), name
    assert st["compressed_bytes"] == behind


def test_device_decoder_takes_a_clusters_file(pangenome, tmp_path, tmp_path_factory):
    from panfeed_amd import _lib
    from panfeed_amd.engine import Engine
    plain, _ = _plain_tree(pangenome, tmp_path_factory, 21, True)
    out = tmp_path / "out"
    _run(pangenome, out, 21, True, device_gzip_clusters=True, batch_clusters=4)
    name = max((n for n in plain if n.endswith(FILES[1])), key=lambda n: len(plain[n]))
    data = (out / (name + ".gz")).read_bytes()
    eng = Engine(klength=21, max_strains=32)
    try:
        text, n, taken = C.c_void_p(), C.c_uint64(), C.c_int()
        _lib.check(eng.L.pf_gunzip_device(eng.ctx, data, len(data), C.byref(text), C.byref(n), C.byref(taken)))
        try:
            assert taken.value == 1, eng.L.pf_last_error()
            assert C.string_at(text, n.value) == plain[name]
        finally:
            eng.L.pf_free_text(text)
    finally:
        eng.close()


def test_ranged_kmers_tsv(pangenome, tmp_path, tmp_path_factory):
    from panfeed_amd import engine, output
    plain, _ = _plain_tree(pangenome, tmp_path_factory, 21, True)
    streams, blocks = [], []
    real_stream, real_splitter = engine.Engine.stream_targets_device, output.ClusterMemberSplitter

    def spy_stream(self, hb, sink, budget=None, **kw):
        r = real_stream(self, hb, sink, budget, **kw)
        streams.append(r)
        return r

    class SpySplitter(real_splitter):
        """which clusters every block's pieces went to"""

        def __init__(self, ends, names, sink):
            def spy(name, piece):
                assert isinstance(piece, engine.GzipMembers)
                if len(piece):
                    blocks[-1].append(name)
                    assert len(gzip.decompress(bytes(piece.view))) == piece.text_bytes      # whole members, their text size
                sink(name, piece)
            super().__init__(ends, names, spy)

        def __call__(self, members, text_off, text_bytes, cuts=()):
            blocks.append([])
            super().__call__(members, text_off, text_bytes, cuts)

    engine.Engine.stream_targets_device, output.ClusterMemberSplitter = spy_stream, SpySplitter
    try:
        out = tmp_path / "out"
        st = _run(pangenome, out, 21, True, device_gzip_clusters=True, targets_text_budget=768 << 10)
    finally:
        engine.Engine.stream_targets_device, output.ClusterMemberSplitter = real_stream, real_splitter
    assert st["device_cluster_files"] == 14
    assert max(r[1] for r in streams) > 1                                  # kmers_tsv_ranges
    assert any(len(set(b)) >= 2 for b in blocks)                            # a block with members of two clusters
    per_cluster = {}
    for b in blocks:
        for name in set(b):
            per_cluster[name] = per_cluster.get(name, 0) + 1
    assert max(per_cluster.values()) >= 2                                   # a cluster that received pieces of two blocks
    _check_tree(_tree(out), plain)


def test_cluster_without_target_rows(pangenome, tmp_path):
    from panfeed_amd.engine import KMERS_TSV_HEADER
    cl, names = pangenome["clusters"], pangenome["names"]
    least = min(cl, key=lambda c: int(c.present.sum()))
    targets = tuple(names[i] for i in np.flatnonzero(~least.present)[:3])
    assert targets
    without = [c.idx for c in cl if not any(c.present[names.index(t)] for t in targets)]
    with_rows = [c.idx for c in cl if any(c.present[names.index(t)] for t in targets)]
    assert least.idx in without and with_rows
    out, ref = tmp_path / "out", tmp_path / "ref"
    st = _run(pangenome, out, 21, True, targets=targets, device_gzip_clusters=True, batch_clusters=4)
    assert st["device_cluster_files"] == 14
    _run(pangenome, ref, 21, True, targets=targets, batch_clusters=4)
    for idx in without:
        assert (out / idx / "kmers.tsv.gz").read_bytes() == _header_member(KMERS_TSV_HEADER), idx      # the header member alone
    assert any(len(_members((out / idx / "kmers.tsv.gz").read_bytes())) > 1 for idx in with_rows)
    _check_tree(_tree(out), _tree(ref))


def test_host_text_goes_in_as_host_made_members(pangenome, tmp_path, tmp_path_factory):
    plain, pst = _plain_tree(pangenome, tmp_path_factory, 21, True)
    out = tmp_path / "out"
    st = _run(pangenome, out, 21, True, device_gzip_clusters=True, device_text=False)
    assert st["device_cluster_files"] == 0
    got = _tree(out)
    _check_tree(got, plain)
    assert st["bytes"] == pst["bytes"]
    heads = _headers(pangenome["names"])
    assert st["compressed_bytes"] == sum(len(d) - len(_header_member(heads[os.path.basename(n)[:-3]])) for n, d in got.items())


def test_device_gzip_alone_stays_the_hosts(pangenome, tmp_path, tmp_path_factory):
    plain, _ = _plain_tree(pangenome, tmp_path_factory, 21, True)
    out = tmp_path / "out"
    st = _run(pangenome, out, 21, True, device_gzip=True)
    assert st["device_cluster_files"] == 14 and "compressed_bytes" not in st
    _check_tree(_tree(out), plain)


def test_sharded_world_2(pangenome, tmp_path, tmp_path_factory):
    plain, _ = _plain_tree(pangenome, tmp_path_factory, 21, True)
    out = str(tmp_path / "out")
    world = 2
    port = str(29600 + (os.getpid() * 7 + 977) % 3000)
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0")
    procs = [subprocess.Popen([sys.executable, os.path.join(REPO, "tests", "cluster_gzip_worker.py"), str(r), str(world), port, out,
                               pangenome["csv"], pangenome["gffs"], "21", str(UP), str(DOWN), ",".join(pangenome["targets"])],
                              cwd=REPO, env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
             for r in range(world)]
    stats = {}
    for r, p in enumerate(procs):
        o, err = p.communicate(timeout=600)
        assert p.returncode == 0, f"rank {r} failed:\n{o[-2000:]}\n{err[-4000:]}"
        stats[r] = json.loads([x for x in o.splitlines() if x.startswith("STATS ")][-1][6:])
    assert sum(s["clusters"] for s in stats.values()) == 14 and all(s["clusters"] for s in stats.values())
    assert all(s["compressed_bytes"] > 0 for s in stats.values())
    _check_tree(_tree(out), plain)
