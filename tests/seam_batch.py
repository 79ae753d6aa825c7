"""The hand-made ten-sequence batch whose kmers.tsv text fixes the order of the text's units where the plan decides it
(test_gpu_targets_stream, test_gpu_text_handout): sequences with no window first, last and between a device unit and a
host unit, host-rendered sequences next to each other, a tile seam inside a sequence, a one-window sequence, a
host-rendered sequence as the last text.  100-400 KB of text; the expected bytes are the oracle's."""
import re
import zlib

import numpy as np

K = 31


def build(canon):
    """(records, target strains, the oracle's kmers.tsv bytes) of the batch"""
    from oracle import oracle as po
    from panfeed_amd.classes import Seqinfo
    rng = np.random.default_rng(31)
    comp = bytes.maketrans(b"ACGTN", b"TGCAN")

    def seq(n, n_at=None):
        s = bytearray(rng.choice(np.frombuffer(b"ACGT", dtype=np.uint8), n).tobytes())
        if n_at is not None:
            s[n_at] = ord("N")
        return bytes(s)
    seqs = [seq(20),                 # no window: the batch's first sequence drops out
            seq(400, 200),           # host-rendered
            seq(1000),               # 970 windows: 4 tiles canonical, 8 not
            seq(25),                 # no window, between a device unit and a host unit
            seq(300, 150),           # host next to host
            seq(200, 199),           # ... its last base an 'N'
            seq(159),                # 129 windows: 258 rows when not canonical, a tile seam after row 256
            seq(31),                 # exactly one window
            seq(100, 50),            # host-rendered, the last text of the batch
            seq(10)]                 # no window: the batch's last sequence
    names = [f"s{i:02d}" for i in range(1, 11)]
    gs = {nm: [Seqinfo(s.decode(), s.translate(comp).decode(), f"{nm}_g", f"{nm}_c", 100 + i, 100 + i + len(s) - 1,
                       -1 if i % 2 else 1, i)]
          for i, (nm, s) in enumerate(zip(names, seqs))}
    recs = [(gs, "grp1", np.ones(10, dtype=np.int64))]
    stroi = set(names)
    run = po.OracleRun(klength=K, stroi=stroi, canon=canon)
    run.feed(recs)
    ek = run.texts()[0].encode()
    assert 100_000 < len(ek) < 400_000
    return recs, stroi, ek


def smallest_budget(eng, hb):
    """the smallest kmers.tsv budget that works for `hb`, as the error for a budget below one tile names it"""
    import pytest
    from panfeed_amd import _lib
    seen = []
    with pytest.raises(_lib.PanfeedHipError) as ei:
        eng.stream_targets_device(hb, seen.append, budget=4096)
    assert ei.value.status == _lib.ERR_ARG and not seen
    return int(re.search(r"smallest budget that works is (\d+)", str(ei.value)).group(1))


def inflate(raw):
    """the text of gzip members, inflated member by member (every member complete: its CRC32 and ISIZE checked)"""
    raw, text = bytes(raw), bytearray()
    while raw:
        d = zlib.decompressobj(31)
        text += d.decompress(raw)
        assert d.eof
        raw = d.unused_data
    return bytes(text)
