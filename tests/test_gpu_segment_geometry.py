"""Segment geometry on the GPU: the three kernels of the resident-genome path against the numpy reference of
tests/segment_geometry.py, word for word, read back through pf_debug_read_words -- the genome store after
genome_pack_kernel (ASCII contigs, more than two staging blocks) and genome_pack_text_kernel (FASTA text as it lies in
the file), and the packed-segment buffer gather_segments_kernel fills, tails and pad words included: the scan reads a
segment by its length, so bits behind its last base change no output text, but the dedup pass compares packed words.
Every result is compared bit for bit; the case lists' coverage is asserted without a GPU in test_segment_geometry.py."""
import copy
import ctypes as C

import numpy as np
import pytest

import segment_geometry as sg

from panfeed_amd.classes import Seqinfo

pytestmark = pytest.mark.gpu

SMALL = dict(max_items=64)               # a few work items a batch: the default scratch is most of an engine's cost


def _engine(**kw):
    from panfeed_amd.engine import Engine
    return Engine(**SMALL, **kw)


def _read_words(eng, which, n, first=0):
    from panfeed_amd import _lib
    out = np.zeros(max(int(n), 1), dtype=np.uint64)
    _lib.check(eng.L.pf_debug_read_words(eng.ctx, which, int(first), int(n), out.ctypes.data_as(C.c_void_p)))
    return out[:int(n)]


def _refused(eng, which, first, n):
    """the status pf_debug_read_words refuses this range with"""
    from panfeed_amd import _lib
    buf = np.zeros(1, dtype=np.uint64)                    # (a refused call writes nothing)
    with pytest.raises(_lib.PanfeedHipError) as e:
        _lib.check(eng.L.pf_debug_read_words(eng.ctx, which, int(first), int(n), buf.ctypes.data_as(C.c_void_p)))
    return e.value.status


def _upload(eng, contigs):
    """pf_genomes_upload of a list of bytes: the word offsets it returns"""
    from panfeed_amd import _lib
    n = len(contigs)
    ptrs = (C.c_char_p * n)(*contigs)
    lens = (C.c_uint64 * n)(*[len(c) for c in contigs])
    off = (C.c_uint64 * n)()
    _lib.check(eng.L.pf_genomes_upload(eng.ctx, n, ptrs, lens, off))
    return np.array(off[:], dtype=np.uint64)


def _store_mismatches(got, want, off, lengths, limit=8):
    """which contigs' words differ, and where"""
    out = []
    for i, (o, n) in enumerate(zip(off, lengths)):
        o, nw = int(o), 2 * ((int(n) + 63) // 64) + 4
        bad = np.flatnonzero(got[o:o + nw] != want[o:o + nw])
        if len(bad):
            w = int(bad[0])
            out.append(f"contig {i} ({int(n)} bases, {(int(n) + 31) // 32} words + padding to {nw}): {len(bad)} words differ, "
                       f"first word {w}: got {int(got[o + w]):016x} want {int(want[o + w]):016x}")
            if len(out) >= limit:
                break
    return out


def _segment_mismatches(cases, order, seg_word_off, got, want, limit=8):
    """the words that differ, by segment and by the classifier's class of the word"""
    out = []
    for s, wo in zip(order, seg_word_off):
        wo, nw = int(wo), 2 * ((s.len + 63) // 64)
        bad = np.flatnonzero(got[wo:wo + nw] != want[wo:wo + nw])
        if len(bad):
            w = int(bad[0])
            cls = sorted(sg.word_classes(s.start, s.len, s.rev, len(cases.contigs[s.contig]))[w])
            out.append(f"{s}: word {w} {cls}: got {int(got[wo + w]):016x} want {int(want[wo + w]):016x} ({len(bad)} words differ)")
            if len(out) >= limit:
                break
    return out


@pytest.fixture(scope="module")
def cases():
    return sg.gather_cases()


def _twin_and_gather(cases, k, canon, W):
    """the host-packed batch of the expected strings, and the same batch with its segments given by reference"""
    from panfeed_amd.packing import build_batch_native
    twin = build_batch_native(sg.gather_records(cases, Seqinfo), k, canon, W, stroi={sg.TARGET_STRAIN})
    order = sg.batch_order(cases, k)
    assert twin.seg_len.tolist() == [s.len for s in order]
    off, _total = sg.store_layout([len(c) for c in cases.contigs])
    lit, src_off, src_start, src_flags, expect = sg.gather_arrays(cases, k, off, twin.seg_word_off)
    assert np.array_equal(twin.packed, expect)            # (two statements of one layout: test_segment_geometry.py)
    gb = copy.copy(twin)
    gb.packed, gb.n_words_dev = lit, len(expect)
    gb.gather_src_off, gb.gather_src_start, gb.gather_src_flags = src_off, src_start, src_flags
    return twin, gb, order, off


def _texts(out):
    return out.kmers_tsv, out.kmers_to_hashes, out.hashes_to_patterns


def _fetched(res, hb):
    """what pf_fetch hands back, as plain values that do not depend on where a run put things: per cluster its counts, its
    own row's digest and its kept k-mers' keys with their patterns' digests and presence bits, in output order; the new
    patterns' digests, lengths and bits in first-seen order; the strand bits.  (Arena offsets and pattern ids are places,
    not results: they are followed, not compared.)"""
    from panfeed_amd.engine import _view
    nc, KW, W, P = hb.n_clusters, int(res.key_words), int(res.W), int(res.n_patterns)
    off, cnt = _view(res.cluster_kmer_off, nc, np.uint64), _view(res.cluster_kmer_cnt, nc, np.uint32)
    n = int((off + cnt).max()) if nc else 0
    keys, pid = _view(res.kmer_key, n * KW, np.uint64).reshape(-1, KW), _view(res.kmer_pattern, n, np.uint32)
    md5, bits = _view(res.pattern_md5, P * 16, np.uint8).reshape(-1, 16), _view(res.pattern_bits, P * W, np.uint32).reshape(-1, W)
    pn = _view(res.pattern_n, P, np.uint32)
    new = _view(res.new_pattern_id, int(res.n_new_patterns), np.uint32)
    out = [cnt.tolist(), _view(res.cluster_unique, nc, np.uint32).tolist(), md5[_view(res.cluster_pattern, nc, np.uint32)].tobytes()]
    for c in range(nc):
        a, b = int(off[c]), int(off[c]) + int(cnt[c])
        out += [keys[a:b].tobytes(), md5[pid[a:b]].tobytes(), bits[pid[a:b]].tobytes()]
    out += [md5[new].tobytes(), pn[new].tolist(), bits[new].tobytes()]
    out.append(_view(res.strand_bits, int(hb.n_strand_words), np.uint64).tobytes() if hb.n_strand_words else b"")
    return out


def _gather_against_twin(cases, k, canon):
    """upload, gather, read the device buffer back: it is the twin's `packed`; then the results of the gather submit are
    the twin's on a fresh engine -- checksum, counters, the fetched arrays, the rendered texts.  Returns the gather engine's
    BatchOutput."""
    from panfeed_amd import _lib
    opts = dict(klength=k, canon=canon, max_strains=64, stroi={sg.TARGET_STRAIN})
    twin, gb, order, off = _twin_and_gather(cases, k, canon, 2)
    eng = _engine(**opts)
    assert np.array_equal(_upload(eng, cases.contigs), off)
    res = eng.submit_host_batch(gb)
    got = _read_words(eng, 1, gb.n_words_dev)
    wrong = _segment_mismatches(cases, order, twin.seg_word_off, got, twin.packed)
    assert not wrong, "gathered words differ from the reference:\n" + "\n".join(wrong)
    assert np.array_equal(got, twin.packed)               # the four tail words too
    assert _refused(eng, 1, 0, gb.n_words_dev + 1) == _lib.ERR_ARG and _refused(eng, 1, gb.n_words_dev, 1) == _lib.ERR_ARG
    sums = eng.result_checksum()
    counters = (int(res.n_instances), int(res.n_unique), int(res.n_kept), int(res.n_new_patterns))
    res = eng.fetch()
    fetched = _fetched(res, gb)
    out = eng._render(gb, res)
    eng.close()
    eng = _engine(**opts)
    res = eng.submit_host_batch(twin)
    assert np.array_equal(_read_words(eng, 1, len(twin.packed)), twin.packed)
    assert eng.result_checksum() == sums
    assert (int(res.n_instances), int(res.n_unique), int(res.n_kept), int(res.n_new_patterns)) == counters
    res = eng.fetch()
    assert _fetched(res, twin) == fetched
    assert _texts(eng._render(twin, res)) == _texts(out)
    eng.close()
    return out


def test_hook_returns_the_submitted_words(cases):
    """pf_debug_read_words: after a plain pf_submit of a host-packed batch the device's packed-segment buffer is the
    batch's `packed`, word for word, also after the results were fetched and rendered (no stage writes to it); ranges
    outside a buffer, another `which` and a context without a batch are refused"""
    from panfeed_amd import _lib
    from panfeed_amd.packing import build_batch_native
    eng = _engine(klength=31, max_strains=64, stroi={sg.TARGET_STRAIN})
    assert _refused(eng, 1, 0, 0) == _lib.ERR_STATE                       # nothing submitted yet
    assert len(_read_words(eng, 0, 0)) == 0 and _refused(eng, 0, 0, 1) == _lib.ERR_ARG        # no genomes: an empty store
    twin = build_batch_native(sg.gather_records(cases, Seqinfo), 31, True, 2, stroi={sg.TARGET_STRAIN})
    eng.submit_host_batch(twin)
    n = len(twin.packed)
    assert np.array_equal(_read_words(eng, 1, n), twin.packed)
    eng._render(twin, eng.fetch())
    assert np.array_equal(_read_words(eng, 1, n), twin.packed)
    assert np.array_equal(_read_words(eng, 1, 5, first=n - 5), twin.packed[n - 5:])
    assert len(_read_words(eng, 1, 0, first=n)) == 0
    for first, cnt in ((0, n + 1), (n, 1), (n + 1, 0), (1 << 63, 1 << 63), (2, (1 << 64) - 1)):
        assert _refused(eng, 1, first, cnt) == _lib.ERR_ARG
    assert _refused(eng, 2, 0, 1) == _lib.ERR_ARG and _refused(eng, -1, 0, 0) == _lib.ERR_ARG
    eng.close()


@pytest.mark.parametrize("canon", [True, False], ids=["canon", "both_strands"])
@pytest.mark.parametrize("k", [31, 5])
def test_gather_word_for_word(cases, k, canon):
    """gather_segments_kernel over the case list: every word of the device buffer -- forward and reverse at every start
    phase, the reverse window in front of the contig, second and third lane trips, masked tails, zero pad words, literal
    segments -- equals the host-packed twin; its results equal the twin's and the oracle's.  k = 5: the short segments
    are in the batch."""
    from test_gpu_parity import _oracle_texts
    out = _gather_against_twin(cases, k, canon)
    expect, st = _oracle_texts(sg.gather_records(cases, Seqinfo), stroi={sg.TARGET_STRAIN}, klength=k, canon=canon)
    assert _texts(out) == tuple(expect)
    assert out.stats["unique_kmers"] == st["unique_kmers"] and len(out.kmers_tsv) > 0


def test_gather_of_the_shortest_segments(cases):
    """k = 1: every segment of the list is in the batch, those of 1 to 4 bases too (one word of nb < 5 bases, forward,
    reverse and in front of the contig) -- the device buffer and the results against the host-packed twin"""
    order = sg.batch_order(cases, 1)
    assert len(order) == len(cases.segs) and {(s.len, s.rev) for s in order if not s.literal} >= {(n, r) for n in (1, 2) for r in (False, True)}
    out = _gather_against_twin(cases, 1, True)
    assert out.stats["instances"] == sum(s.len for s in order) and out.stats["unique_kmers"] >= 2


def test_ascii_pack_whole_store():
    """genome_pack_kernel: the whole store after pf_genomes_upload of contigs on every word, 16-byte and thread-block
    seam, 300 short ones among them (the piece search), lower-case stretches: per contig pack(contig), then zeros up to
    2 * ceil(L / 64) + 4 words, at the offsets the layout rule gives"""
    from panfeed_amd import _lib
    contigs = sg.pack_contigs()
    want, off = sg.store_words(contigs)
    eng = _engine(klength=31, max_strains=32)
    assert np.array_equal(_upload(eng, contigs), off)
    got = _read_words(eng, 0, len(want))
    wrong = _store_mismatches(got, want, off, [len(c) for c in contigs])
    assert not wrong, "the genome store differs from the reference:\n" + "\n".join(wrong)
    assert np.array_equal(got, want)
    assert _refused(eng, 0, 0, len(want) + 1) == _lib.ERR_ARG
    assert eng.L.pf_genomes_clear(eng.ctx) == 0 and _refused(eng, 0, 0, 1) == _lib.ERR_ARG
    eng.close()


def test_segments_beside_an_n_gather_correctly():
    """a letter other than A/C/G/T packs to an unspecified code, and the host never asks for it: segments that end on
    the base before it or start on the base behind it -- at the word's last base, the next word's first, mid-word --
    come out of the store as if the contig held nothing else"""
    rng = np.random.default_rng(41)
    contigs, segs = [sg.random_acgt(rng, 200)], []
    for at in (31, 32, 33, 63, 64, 95, 150):
        L = at + 1 + int(rng.integers(40, 90))
        c = bytearray(sg.random_acgt(rng, L))
        c[at] = ord("N") if at % 2 else ord("n")
        contigs.append(bytes(c))
        ci = len(contigs) - 1
        for rev in (False, True):
            segs += [(ci, 0, at, rev), (ci, at - 7, 7, rev), (ci, at + 1, L - at - 1, rev), (ci, at + 1, 33, rev)]
    cases = sg.GatherCases(contigs, [sg.Seg(c, s, n, r, i % sg.PER_CLUSTER == sg.LITERAL_AT) for i, (c, s, n, r) in enumerate(segs)])
    out = _gather_against_twin(cases, 7, True)
    assert out.stats["instances"] == sum(n - 6 for _c, _s, n, _r in segs)


def test_three_staging_blocks():
    """pf_genomes_upload of more than two 64 MiB staging blocks: contigs of about 40, 50 and 45 Mi bases with 200 short
    ones behind each of the first two -- the second and the third long one are split at a block's end, and slot 0 is
    used a second time, once its event has fired.  The whole store equals the reference."""
    from panfeed_amd import _lib
    ascii_, offs, lens = sg.staging_contigs()
    assert len(ascii_) > 2 * (64 << 20)
    n = len(lens)
    addr = np.ascontiguousarray(np.uint64(ascii_.ctypes.data) + offs)
    lens = np.ascontiguousarray(lens)
    got_off = np.zeros(n, dtype=np.uint64)
    eng = _engine(klength=31, max_strains=32)
    _lib.check(eng.L.pf_genomes_upload(eng.ctx, n, addr.ctypes.data_as(C.POINTER(C.c_char_p)),
                                       lens.ctypes.data_as(C.POINTER(C.c_uint64)), got_off.ctypes.data_as(C.POINTER(C.c_uint64))))
    off, total = sg.store_layout(lens)
    assert np.array_equal(got_off, off)
    got = _read_words(eng, 0, total)
    eng.close()
    wrong = []
    for i in range(n):
        o, L = int(off[i]), int(lens[i])
        w = sg.pack(ascii_[int(offs[i]):int(offs[i]) + L])
        end = o + 2 * ((L + 63) // 64) + 4
        if not (np.array_equal(got[o:o + len(w)], w) and not got[o + len(w):end].any()):
            bad = np.flatnonzero(got[o:o + len(w)] != w)
            wrong.append(f"contig {i} ({L} bases at word {o}): " + (f"{len(bad)} words differ, first {int(bad[0])} (base {32 * int(bad[0])})"
                                                                    if len(bad) else "its padding is not zero"))
    assert not wrong, "\n".join(wrong[:8])


def test_text_pack_of_the_fasta_cases(tmp_path):
    """genome_pack_text_kernel through the one-pass ingest of the FASTA cases (every width x line end x length on a line
    boundary, unwrapped records, a full last line at the end of the file, FASTA behind ##FASTA at varying byte offsets):
    every by-reference sequence decodes from the device's store to the letters of the file -- per sequence: reader
    threads claim store space in any order.  The decode goes by a pass of the reader at k = 1, where no sequence is too
    short for a segment: one-letter contigs at every width and line end are compared too.  The run itself is at k = 5, and
    its three texts equal the oracle's over the restated records"""
    from oracle import input_restatement as ir
    from oracle import oracle as po
    from panfeed_amd import _lib
    from panfeed_amd import native_input as ni
    k = 5
    genomes = sg.fasta_cases()
    p = sg.write_fasta_pangenome(str(tmp_path), genomes)
    eng = _engine(klength=k, max_strains=32)
    assert len(p["genomes"]) <= 32
    with ni.Pangenome(p["csv"], None, genome_names=p["genomes"], gff_paths=p["gff"], fasta_paths=p["fasta"], engine=eng) as pg:
        assert pg.one_pass and pg.resident
        refs = list(pg.batches(1, True, eng.W, max_clusters=4))
        pg.set_range(0, pg.n_clusters)                    # back to the first row
        hbs = list(pg.batches(k, True, eng.W, max_clusters=4))
    total = sg.store_layout([len(c.letters) for g in genomes for c in g.contigs])[1]
    store = _read_words(eng, 0, total)                    # every contig claimed its share once: nothing more is held
    assert _refused(eng, 0, 0, total + 1) == _lib.ERR_ARG
    want = p["clusters"]
    assert all(len(s) >= 1 for row in want for _nm, s in row)
    assert sum(hb.n_clusters for hb in hbs) == len(want)
    assert [n for hb in hbs for n in hb.seg_len.tolist()] == [len(s) for row in want for _nm, s in row if len(s) >= k]
    wrong, n_seen, ci = [], 0, 0
    for hb in refs:
        assert hb.gather_src_off is not None and not (hb.gather_src_flags & 1).any()
        for c in range(hb.n_clusters):
            a, b = int(hb.cluster_seg_off[c]), int(hb.cluster_seg_off[c + 1])
            assert hb.seg_len[a:b].tolist() == [len(s) for _nm, s in want[ci]], ci
            for s, (nm, letters) in zip(range(a, b), want[ci]):
                got = sg.unpack(store, hb.gather_src_off[s], int(hb.gather_src_start[s]), len(letters))
                if hb.gather_src_flags[s] & 2:
                    got = sg.revcomp(got)
                if got != letters:
                    first = next(i for i in range(len(letters)) if got[i] != letters[i])
                    wrong.append(f"row {ci} genome {nm} ({len(letters)} letters from base {int(hb.gather_src_start[s])}): first "
                                 f"difference at letter {first}")
                n_seen += 1
            ci += 1
    assert not wrong, f"{len(wrong)} of {n_seen} sequences differ:\n" + "\n".join(wrong[:10])
    n_contigs = sum(len(c.letters) > 0 for g in genomes for c in g.contigs)
    assert ci == len(want) and n_seen == sum(len(r) for r in want) > 300 and n_seen >= n_contigs
    outs = list(eng.run_batches(iter(hbs)))
    eng.close()
    strains, table = ir.load_table(p["csv"])
    data = ir.load_genomes(p["genomes"], p["gff"], p["fasta"])
    run = po.OracleRun(klength=k)
    run.feed(list(ir.iter_gene_clusters(strains, table, data, 0, 0, False)))
    ek, ekh, ehp = run.texts()
    assert "".join(o.kmers_to_hashes for o in outs) == ekh
    assert "".join(o.hashes_to_patterns for o in outs) == ehp
    assert "".join(o.kmers_tsv for o in outs) == ek
