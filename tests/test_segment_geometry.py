"""Segment geometry without a GPU: the case lists of tests/segment_geometry.py reach every branch of the kernels they
are made for (so that thinning a list cannot quietly lose an edge), the numpy reference and the host packer are two
independent statements of one layout, and the one-pass reader's pieces address the FASTA cases letter for letter (host
sink: the text kernel's addressing run on the host)."""
import ctypes as C

import numpy as np
import pytest

import segment_geometry as sg

from panfeed_amd.classes import Seqinfo

K_RUNS = (5, 31)                         # k-mer lengths the GPU test gathers the list at


@pytest.fixture(scope="module")
def cases():
    return sg.gather_cases()


def test_reference_layout_by_hand():
    """first base in bits 63:62, 32 bases a word, zero behind the last base; reverse complement; 16-byte segments"""
    assert sg.pack(b"").size == 0
    assert sg.pack(b"C").tolist() == [1 << 62]
    assert sg.pack(b"ACGT").tolist() == [0b00011011 << 56]
    assert sg.pack(b"t" * 32 + b"g").tolist() == [(1 << 64) - 1, 2 << 62]
    assert sg.revcomp(b"AACGT") == b"ACGTT"
    assert sg.segment_words(b"GGAACGTCC", 2, 5, True).tolist() == [0b0001101111 << 54, 0]
    assert len(sg.segment_words(b"A" * 65, 0, 65, False)) == 4
    assert sg.unpack(sg.pack(b"ACGTTGCA" * 9), 0, 30, 7) == (b"ACGTTGCA" * 9)[30:37]
    with pytest.raises(ValueError):
        sg.pack(b"ACNT")
    off, total = sg.store_layout([0, 1, 64, 65])
    assert off.tolist() == [0, 4, 10, 16] and total == 24


def test_classifier_by_hand():
    assert sg.word_classes(0, 32, False) == [{"F0", "full"}, {"zero"}]
    assert sg.word_classes(5, 33, False, contig_len=38) == [{"F1", "full"}, {"F1", "F1pad", "tail"}]
    assert sg.word_classes(5, 33, False, contig_len=65) == [{"F1", "full"}, {"F1", "tail"}]
    assert sg.word_classes(0, 33, True) == [{"R1", "full"}, {"Rneg", "tail"}]
    assert sg.word_classes(31, 33, True) == [{"R0", "full"}, {"R0", "tail"}]
    assert sg.word_classes(30, 33, True)[1] == {"Rneg", "tail"}
    assert sg.word_classes(0, 1025, False)[32] == {"F0", "tail", "trip2", "trip3"} and sg.word_classes(0, 1025, False)[33] == {"zero", "trip2", "trip3"}
    assert sg.gather_classes(3, 513, True) == {"R1", "Rneg", "full", "tail", "zero", "trip2"}
    assert sg.gather_classes(3, 510, True) == {"R1", "full", "tail"}


def test_what_the_classifier_calls_unreachable_is():
    """every (start, len, strand) of small shapes on every contig length that holds it: a padded second read and a
    source window in front of the contig come with a tail only"""
    seen = set()
    for clen in (31, 33, 64, 95, 130):
        for start in range(min(clen, 66)):
            for length in range(1, clen - start + 1):
                for rev in (False, True):
                    for cls in sg.word_classes(start, length, rev, clen):
                        seen |= {(kind, fill) for kind in sg.KINDS for fill in ("full", "tail") if kind in cls and fill in cls}
    assert seen == {(kind, fill) for kind in sg.KINDS for fill in ("full", "tail")} - sg.UNREACHABLE


def test_gather_list_reaches_every_class(cases):
    """every kind of word with a full and with a partial last word and on the second lane trip, every phase x strand x
    fill cell, the lengths and contig ends the list is made for -- at both k-mer lengths the GPU test runs"""
    contigs, segs = cases
    lens = {len(c) for c in contigs}
    assert lens >= {1, 31, 32, 33, 63, 64, 65, 127, 128, 129, 8063, 8064, 8065, 8066} and sum(2000 <= n < 5000 for n in lens) >= 3
    assert 200 <= len(segs) <= 600
    for k in K_RUNS:
        order = sg.batch_order(cases, k)
        combos, cells, rev_shift, rneg_starts = set(), set(), set(), set()
        for s in order:
            if s.literal:
                continue                                      # (a literal segment is copied: forward, phase 0)
            for cls in sg.word_classes(s.start, s.len, s.rev, len(contigs[s.contig])):
                for kind in sg.KINDS:
                    if kind in cls:
                        combos |= {(kind, x) for x in ("full", "tail", "trip2", "trip3") if x in cls}
                if "Rneg" in cls:
                    rneg_starts.add(s.start)
                if "zero" in cls:
                    combos.add(("zero", "trip2") if "trip2" in cls else ("zero", "trip1"))
            cells.add((s.start % 32, s.rev, sg.last_fill(s.len)))
            if s.rev:
                rev_shift.add((s.start + s.len) % 32)
        want = {(kind, x) for kind in sg.KINDS for x in ("full", "tail", "trip2")} - sg.UNREACHABLE
        assert want <= combos, f"k={k}: the list lost {sorted(want - combos)}"
        assert {("F0", "trip3"), ("F1", "trip3"), ("F1pad", "trip3"), ("R0", "trip3"), ("R1", "trip3"), ("Rneg", "trip3")} <= combos
        assert {("zero", "trip1"), ("zero", "trip2")} <= combos
        assert cells >= {(p, r, f) for p in range(32) for r in (False, True) for f in sg.FILLS}, k
        assert rev_shift == set(range(32))
        assert rneg_starts >= set(range(31)), k
        # whole contigs, ends on the last base, lengths, sources at word offset 0 and behind, literals, lane groups
        whole = {(s.contig, s.rev) for s in order if s.start == 0 and s.len == len(contigs[s.contig])}
        assert whole == {(i, r) for i, c in enumerate(contigs) for r in (False, True) if len(c) >= k}
        ends = {(s.len % 64, s.rev) for s in order if s.start + s.len == len(contigs[s.contig]) and s.start > 0}
        assert ends >= {(r, rev) for r in sg.END_REMAINDERS for rev in (False, True)}
        for n in sg.LENGTHS:
            if n >= k:
                assert {(s.rev, s.contig == 0) for s in order if s.len == n} == {(r, f) for r in (False, True) for f in (False, True)}, n
        n_lit = sum(s.literal for s in order)
        assert 5 <= n_lit <= len(order) // 20 and {s.rev for s in order if s.literal} == {False, True}
        assert len(order) % 16 != 0 and sg.PER_CLUSTER % 16 != 0
        for rev in (False, True):
            assert {i % 16 for i, s in enumerate(order) if s.rev == rev and not s.literal} == set(range(16))
    assert {s.len for s in segs} >= set(sg.LENGTHS)           # (the shortest are in no batch of K_RUNS: the CPU test below)


def test_reference_equals_host_packer_on_every_segment(cases):
    """pf_pack_acgt (the host packer's per-sequence routine) and the numpy reference give the same words for every
    segment of the list, and for the whole batch pf_pack_records lays out"""
    from panfeed_amd import _lib
    from panfeed_amd.packing import build_batch_native
    L = _lib.load()
    contigs, segs = cases
    for s in segs:
        want = sg.segment_words(contigs[s.contig], s.start, s.len, s.rev)
        buf = (C.c_uint64 * len(want))()
        assert L.pf_pack_acgt(sg.segment_letters(contigs[s.contig], s.start, s.len, s.rev), s.len, buf) == len(want)
        assert np.array_equal(np.ctypeslib.as_array(buf), want), s
    off, _total = sg.store_layout([len(c) for c in contigs])
    for k in K_RUNS + (1,):
        twin = build_batch_native(sg.gather_records(cases, Seqinfo), k, True, 2, stroi={sg.TARGET_STRAIN})
        order = sg.batch_order(cases, k)
        assert twin.seg_len.tolist() == [s.len for s in order]
        lit, src_off, src_start, src_flags, expect = sg.gather_arrays(cases, k, off, twin.seg_word_off)
        assert np.array_equal(twin.packed, expect)
        assert (src_flags & 1).sum() == sum(s.literal for s in order) and len(lit) >= 4
        assert len({t.strain for t in twin.targets}) == 1 and len(twin.targets) == sum(s.literal for s in sg.batch_order(cases, 1))


def test_pack_contig_lengths_hold_the_seams():
    lens = sg.pack_contig_lengths()
    assert set(lens) >= {0, 1, 31, 32, 33, 63, 64, 65, 8063, 8064, 8065, 16127, 16128, 16129}
    assert sum(n < 400 for n in lens) >= 300 and len(lens) > 256                 # nine halvings in the piece search
    assert 0 not in (lens[0], lens[-1])                                          # (an empty contig between others)
    contigs = sg.pack_contigs()
    assert [len(c) for c in contigs] == lens
    assert sum(c != c.upper() for c in contigs) > 100 and sum(c == c.upper() for c in contigs) > 50
    words, off = sg.store_words(contigs)
    for c, o in list(zip(contigs, off))[::17]:
        assert sg.unpack(words, o, 0, len(c)) == c.upper()


def test_staging_list_fills_three_blocks():
    """the three-block upload's lengths: more than two 64 MiB staging blocks of letters, the second and the third long
    contig each across a block's end (a block takes its pieces padded to 32 letters); the letters themselves at a
    thousandth of the size"""
    lens = sg.staging_lengths()
    block = 64 << 20
    at = np.concatenate(([0], np.cumsum((lens + np.uint64(31)) // np.uint64(32) * np.uint64(32)))).astype(np.int64)
    assert 2 * block < int(lens.sum()) and int(at[-1]) < 3 * block - (1 << 20)
    big = np.flatnonzero(lens > (30 << 20))
    assert len(big) == 3 and len(lens) == 403
    assert [int(at[i]) // block for i in big] == [0, 0, 1] and [int(at[i + 1] - 1) // block for i in big] == [0, 1, 2]
    ascii_, offs, small = sg.staging_contigs(scale=1 << 10)
    assert len(small) == 403 and int(small.sum()) == len(ascii_) and int(offs[-1] + small[-1]) == len(ascii_)
    assert set(np.unique(ascii_).tolist()) == set(b"ACGT")


# ------------------------------------------------------------------------------------------------ FASTA cases
def test_fasta_cases_are_the_cross():
    genomes = sg.fasta_cases()
    cross = {(c.width, c.eol, len(c.letters)) for g in genomes for c in g.contigs}
    for w in sg.WIDTHS:
        for eol in sg.EOLS:
            assert {(w, eol, n) for n in sg.fasta_lengths(w)} <= cross
    assert sg.fasta_lengths(1)[1] == 0                                           # a record without a letter
    last = {(c.width, c.final_eol, len(c.letters) % (c.width or 1) == 0) for g in genomes for c in g.contigs[-1:]}
    assert {(0, True, True), (0, False, True), (60, True, True), (60, False, True)} <= last
    assert {g.separate for g in genomes} == {False, True}
    assert all(sum(len(c.letters) for c in g.contigs) / len(g.contigs) > 1500 for g in genomes)
    assert all(any(len(c.letters) > 20000 for c in g.contigs) for g in genomes)


def test_one_pass_reader_addresses_every_fasta_case(tmp_path):
    """the FASTA cases through the one-pass reader's host sink: every contig by reference (no letter but A/C/G/T, no
    target strain), and every sequence -- whole contigs down to one letter, stretches across line ends -- decodes from
    the sink's store to the letters of the file.  k = 1: no sequence is too short for a segment."""
    from panfeed_amd import native_input as ni
    p = sg.write_fasta_pangenome(str(tmp_path), sg.fasta_cases())
    W = (len(p["genomes"]) + 31) // 32
    with ni.Pangenome(p["csv"], None, genome_names=p["genomes"], gff_paths=p["gff"], fasta_paths=p["fasta"],
                      debug_hostsink=True) as pg:
        store = pg.store_words                            # (that the open succeeds is the check: a store too small is an error here)
        hbs = list(pg.batches(1, True, W, max_clusters=4))
        assert pg.take_log() == ""
    want = [row for row in p["clusters"]]
    n_seen, ci = 0, 0
    for hb in hbs:
        assert hb.gather_src_off is not None and not (hb.gather_src_flags & 1).any()
        assert len(hb.packed) == 4 and not hb.packed.any()
        for c in range(hb.n_clusters):
            a, b = int(hb.cluster_seg_off[c]), int(hb.cluster_seg_off[c + 1])
            assert hb.seg_len[a:b].tolist() == [len(s) for _nm, s in want[ci]], ci
            for s, (nm, letters) in zip(range(a, b), want[ci]):
                got = sg.unpack(store, hb.gather_src_off[s], int(hb.gather_src_start[s]), len(letters))
                if hb.gather_src_flags[s] & 2:
                    got = sg.revcomp(got)
                assert got == letters, (ci, nm)
                n_seen += 1
            ci += 1
    assert ci == len(want) and n_seen == sum(len(r) for r in want) > 300
