"""A sharded run with its kmers.tsv streamed, its rows and texts gzipped on the GPU, and the command that starts it: one
process per rank, each with its own Engine, all on cuda:0 with gloo collectives on host tensors (a one-GPU machine
exercises the control flow and the bytes, never a multi-GPU time).  The assembled files must be the single-rank files and
the oracle's byte for byte; the device-gzip files must be ones the row filter inflates on the GPU without falling back."""
import gzip
import os
import subprocess
import sys

import pytest

from test_sharded_members_cpu import FILES, REPO, run_stream_world

pytestmark = pytest.mark.gpu

# the smallest kmers.tsv budget every batch accepts: two ranges of one LDS tile of text each (pf_kernels.h: KT_TILE = 61 440
# bytes, and the 64 bytes of slack a text buffer has).  A batch of the seeded case -- 3 clusters x 2 target strains, a few
# hundred windows each, rows of about 110 bytes -- is several times that, so its rows leave in more than one range
BUDGET = 2 * (61440 + 64)


def read_files(out, gz=False):
    texts = {}
    for f in FILES:
        with open(os.path.join(out, f + (".gz" if gz else "")), "rb") as fh:
            texts[f] = gzip.decompress(fh.read()) if gz else fh.read()
    return texts


@pytest.fixture(scope="module")
def seeded(tmp_path_factory):
    """the seeded case through one rank, plain: (its files, its stats) -- the yardstick of the other worlds"""
    out = str(tmp_path_factory.mktemp("w1") / "out")
    os.mkdir(out)
    stats = run_stream_world("gpu", 1, out, "seeded", {"targets_text_budget": BUDGET})
    return read_files(out), stats


def test_single_rank_streams_in_ranges_and_equals_the_oracle(seeded):
    texts, stats = seeded
    batches = -(-stats[0]["clusters"] // 3)                     # (the worker's batch_clusters)
    assert stats[0]["kmers_tsv_ranges"] > batches and stats[0]["kmers_tsv_streamed"] > BUDGET
    assert stats[0]["kmers_tsv_streamed"] == len(texts["kmers.tsv"].split(b"\n", 1)[1])
    assert 0 < stats[0]["kmers_tsv_peak_device_bytes"] <= BUDGET
    from oracle import oracle as po
    from panfeed_amd.engine import KMERS_TO_HASHES_HEADER, KMERS_TSV_HEADER, hashes_to_patterns_header
    from sharded_stream_worker import seeded_case
    records, strains, opts = seeded_case()
    run = po.OracleRun(klength=opts["klength"], stroi=set(opts["stroi"]), threads=4)
    run.feed(records)
    ek, ekh, ehp = run.texts()
    assert texts["kmers_to_hashes.tsv"].decode() == KMERS_TO_HASHES_HEADER + ekh
    assert texts["hashes_to_patterns.tsv"].decode() == hashes_to_patterns_header(strains) + ehp
    assert texts["kmers.tsv"].decode() == KMERS_TSV_HEADER + ek
    assert stats[0]["bytes"] == len(ek) + len(ekh) + len(ehp)


@pytest.mark.parametrize("world", [2, 3])
def test_worlds_write_the_single_rank_files(seeded, tmp_path, world):
    texts, one = seeded
    out = str(tmp_path / "out")
    os.mkdir(out)
    stats = run_stream_world("gpu", world, out, "seeded", {"targets_text_budget": BUDGET})
    got = read_files(out)
    for f in FILES:
        assert got[f] == texts[f], f
    assert sorted(os.listdir(out)) == sorted(FILES)
    # some rank dropped patterns an earlier rank had seen: the exchange had something to find
    assert sum(s["local_patterns"] for s in stats.values()) > stats[0]["patterns"] == one[0]["patterns"]
    assert any(s["kmers_tsv_ranges"] > 1 and s["kmers_tsv_streamed"] > 0 for s in stats.values())
    assert sum(s["kmers_tsv_streamed"] for s in stats.values()) == one[0]["kmers_tsv_streamed"]
    assert sum(s["bytes"] for s in stats.values()) == one[0]["bytes"]
    assert all(s["kmers_tsv_peak_device_bytes"] <= BUDGET for s in stats.values())


def test_device_gzip_files_go_through_the_device_gunzip(seeded, tmp_path):
    from panfeed_amd.downstream import RowFilter
    from sharded_stream_worker import seeded_case
    texts, one = seeded
    out = str(tmp_path / "gz")
    os.mkdir(out)
    stats = run_stream_world("gpu", 2, out, "seeded", {"targets_text_budget": BUDGET, "device_gzip": True})
    assert sorted(os.listdir(out)) == sorted(f + ".gz" for f in FILES)
    got = read_files(out, gz=True)
    for f in FILES:
        assert got[f] == texts[f], f
    assert sum(s["bytes"] for s in stats.values()) == one[0]["bytes"]            # text bytes, not members
    assert any(s["kmers_tsv_ranges"] > 1 for s in stats.values())
    records = seeded_case()[0]
    keys = [records[1][1], records[4][1], records[-1][1]]
    for name in ("kmers_to_hashes.tsv", "kmers.tsv"):
        plain = tmp_path / name
        plain.write_bytes(texts[name])
        rf = RowFilter(keys, True)
        try:
            want = rf.filter_file(str(plain))
        finally:
            rf.close()
        before = (RowFilter.device_gunzip_files, RowFilter.fallback_files)
        rf = RowFilter(keys, True)
        try:
            rows = rf.filter_file(os.path.join(out, name + ".gz"))
        finally:
            rf.close()
        assert (RowFilter.device_gunzip_files, RowFilter.fallback_files) == (before[0] + 1, before[1]), name
        assert rows == want and len(want[1]) > 0, name


@pytest.fixture(scope="module")
def pangenome(tmp_path_factory):
    """a small panaroo table + GFFs on disk, and the same with a last row naming a gene no GFF has"""
    from panfeed_amd import synth
    cl = synth.generate(23, 40, first=500, flank=0, mean_len=300, min_len=50, max_len=900, n_rate=0.03, paralog_rate=0.05)
    names = cl[0].names
    src = tmp_path_factory.mktemp("pangenome") / "in"
    csvp, gffs, fas = synth.write_pangenome(str(src), cl, missing_gene_rate=0.0)      # (the one missing gene is made below)
    with open(csvp) as fh:
        lines = fh.read().splitlines()
    cells = lines[-1].split(",")
    cells[0], cells[-1] = "group_missing", "no_such_gene_0"
    bad = str(src / "missing_gene.csv")
    with open(bad, "w") as fh:
        fh.write("\n".join(lines + [",".join(cells)]) + "\n")
    return csvp, str(src / "gffs"), bad, (names[3], names[20])


def test_run_files_sharded_streams_and_equals_run_files(pangenome, tmp_path):
    from panfeed_amd.pipeline import run_files
    csvp, gffs, bad, targets = pangenome
    single = str(tmp_path / "single")
    run_files(csvp, gffs, single, klength=23, targets=targets, batch_clusters=5)
    out = str(tmp_path / "sharded")
    stats = run_stream_world("gpu", 2, out, f"files:{csvp}:{gffs}:23:{','.join(targets)}", {"targets_text_budget": BUDGET})
    assert read_files(out) == read_files(single)
    assert sum(s["clusters"] for s in stats.values()) == 23 and sum(s["kmers_tsv_streamed"] for s in stats.values()) > 0


def test_stop_on_missing_reaches_every_rank(pangenome, tmp_path):
    """the bad row is the table's last: rank 1 owns it and raises the reader's error in its shard; rank 0, whose shard is
    fine, is told before the pattern exchange and ends by itself -- nobody ends it -- and nothing is assembled or left"""
    csvp, gffs, bad, targets = pangenome
    out = str(tmp_path / "stop")
    res = run_stream_world("gpu", 2, out, f"files:{bad}:{gffs}:23:{','.join(targets)}", {"raise_missing": True},
                           timeout=120, expect_failure=True)
    (rc0, out0, err0), (rc1, out1, err1) = res[0], res[1]
    assert rc1 > 0 and "Could not find gene no_such_gene_0" in err1, (rc1, err1[-3000:])
    assert rc0 > 0 and "another rank of this run failed in its shard" in err0, (rc0, err0[-3000:])
    assert "Could not find gene" not in err0
    # neither rank reached the pattern exchange (finish_shard) or the assembly: no rank reports, no file, no part, and
    # the directory the run made is gone, so the command can be run again
    for o, e in ((out0, err0), (out1, err1)):
        assert "STATS" not in o and "finish_shard" not in e and "assemble" not in e
    assert not os.path.exists(out)


def test_a_failing_rank_under_multiple_files_stops_the_others(pangenome, tmp_path):
    """per-cluster directories: no exchange follows the shard, and still the rank whose shard is fine ends by itself"""
    csvp, gffs, bad, targets = pangenome
    out = str(tmp_path / "mf")
    res = run_stream_world("gpu", 2, out, f"files:{bad}:{gffs}:23:{','.join(targets)}",
                           {"raise_missing": True, "multiple_files": True}, timeout=120, expect_failure=True)
    assert res[1][0] > 0 and "Could not find gene no_such_gene_0" in res[1][2], res[1][2][-3000:]
    assert res[0][0] > 0 and "another rank of this run failed in its shard" in res[0][2], res[0][2][-3000:]


def test_the_command_rehearsed_on_one_gpu(pangenome, tmp_path):
    """`python -m panfeed_amd --gpus 2` with PANFEED_SHARED_GPU=1: the parent starts two ranks on this GPU; the files are
    those of the same command without --gpus"""
    csvp, gffs, bad, targets = pangenome
    (tmp_path / "targets.txt").write_text("".join(t + "\n" for t in targets))
    base = [sys.executable, "-m", "panfeed_amd", "-p", csvp, "-g", gffs, "-k", "23", "--targets", "targets.txt",
            "--batch-clusters", "5"]
    env = dict(os.environ, PYTHONPATH=REPO, PANFEED_SHARED_GPU="1", PANFEED_DIST_TIMEOUT_S="120")
    for name in ("WORLD_SIZE", "RANK", "LOCAL_RANK"):
        env.pop(name, None)
    one = subprocess.run(base + ["-o", "one"], cwd=tmp_path, env=env, capture_output=True, text=True, timeout=300)
    assert one.returncode == 0, one.stderr[-3000:]
    two = subprocess.run(base + ["-o", "two", "--gpus", "2"], cwd=tmp_path, env=env, capture_output=True, text=True, timeout=300)
    assert two.returncode == 0, two.stderr[-4000:]
    assert read_files(tmp_path / "two") == read_files(tmp_path / "one")
    assert sorted(os.listdir(tmp_path / "two")) == sorted(FILES)
    assert "23 gene clusters" in two.stderr and "patterns written to two" in two.stderr
    # a directory that exists is refused before any rank starts
    again = subprocess.run(base + ["-o", "two", "--gpus", "2"], cwd=tmp_path, env=env, capture_output=True, text=True, timeout=120)
    assert again.returncode == 1 and "exists" in again.stderr
