"""The pangenomes of the passing-rows tests (tests/test_gpu_passing_rows.py) and the oracle's side of them: the CPU
oracle's three texts, and the filter stated in a dozen lines of Python on those texts alone.  A case is computed once per
test session and never changed."""
import atexit
import collections
import functools
import shutil
import tempfile

UP, DOWN = 40, 30
# k -> (canonical, seed, rows, rows whose pair kmers_to_hashes lists, rows kept by EVERY SECOND distinct hash,
#       k-mers that pass in one cluster and fail in another)
TABLE = {21: (True, 921, 60360, 50955, 29693, 68),
         17: (False, 917, 134228, 107638, 66000, 316),
         33: (True, 933, 61565, 57437, 28322, 22),
         126: (True, 1026, 58363, 58363, 32459, 0)}

Case = collections.namedtuple("Case", "k canon csvp gffdir gffs targets kt kh hp rows pairs hashes n_with_n n_seqs")


def filter_rows(case, passing):
    """the contract: the data rows of kmers.tsv, in order, whose (field 1, field 11) kmers_to_hashes lists with a hash of
    `passing`"""
    passing = set(passing)
    ok = {pair for pair, h in case.pairs.items() if h in passing}
    return [r for r in case.rows if (r.split("\t", 1)[0], r.rsplit("\t", 1)[1]) in ok]


def text_of(rows):
    return "".join(r + "\n" for r in rows)


def rows_by_cluster(rows):
    by = collections.OrderedDict()
    for r in rows:
        by.setdefault(r.split("\t", 1)[0], []).append(r)
    return by


@functools.lru_cache(maxsize=None)
def case(k):
    from oracle import input_restatement as ir
    from oracle import oracle as po
    from panfeed_amd import synth
    canon, seed = TABLE[k][:2]
    root = tempfile.mkdtemp(prefix=f"passing_k{k}_")
    atexit.register(shutil.rmtree, root, ignore_errors=True)
    cl = synth.generate(14, 24, first=seed, flank=0, mean_len=450, min_len=80, max_len=1000, n_rate=0.2, paralog_rate=0.05)
    names = cl[0].names
    csvp, gffs, _fas = synth.write_pangenome(root, cl)
    targets = tuple(names[i] for i in range(0, 24, 2))
    strains, table = ir.load_table(csvp)
    gn = sorted(gffs)
    recs = list(ir.iter_gene_clusters(strains, table, ir.load_genomes(gn, [gffs[n] for n in gn]), UP, DOWN, False))
    run = po.OracleRun(klength=k, stroi=set(targets), canon=canon)
    run.feed(recs)
    kt, kh, hp = run.texts()
    n_with_n = sum(1 for r in recs for nm, seqs in r[0].items() if nm in targets for s in seqs if "N" in s.sequence.upper())
    n_seqs = sum(1 for r in recs for nm, seqs in r[0].items() if nm in targets for s in seqs)
    pairs, hashes = {}, {}
    for line in kh.split("\n"):
        if line:
            idx, kmer, h = line.split("\t")
            if kmer:
                pairs[(idx, kmer)] = h
                hashes[h] = None
    return Case(k, canon, csvp, root + "/gffs", gffs, targets, kt, kh, hp, kt.split("\n")[:-1], pairs, list(hashes),
                n_with_n, n_seqs)


def every_second(c):
    """every second distinct hash of the k-mer rows of kmers_to_hashes, in file order"""
    return c.hashes[::2]


def check_conditions(c):
    """what keeps a test on this case from hiding a failure, on the oracle's side"""
    n_rows, n_listed, n_kept, n_mixed = TABLE[c.k][2:]
    kept = filter_rows(c, every_second(c))
    assert len(c.rows) == n_rows and len(filter_rows(c, c.hashes)) == n_listed and len(kept) == n_kept
    assert 0 < len(kept) < len(c.rows)
    all_by, kept_by = rows_by_cluster(c.rows), rows_by_cluster(kept)
    assert all(0 < len(kept_by.get(idx, ())) < len(rows) for idx, rows in all_by.items())
    passing = set(every_second(c))
    status = collections.defaultdict(set)
    for (idx, kmer), h in c.pairs.items():
        status[kmer].add(h in passing)
    assert sum(1 for s in status.values() if len(s) == 2) == n_mixed
    assert 0 < c.n_with_n < c.n_seqs, "the batch must mix device-written and host-rendered sequences"
    assert len(c.kt) > 4 * (768 << 10)
    return kept
