"""The segmented gzip without a GPU: the chunk plan and its serial host model (pf_gzip_host_model_segments: no member
holds bytes of two segments, csrc/pf_deflate.h), the splitter that hands a stream's members to the clusters' files
(output.ClusterMemberSplitter), and the --gpu-compress-clusters option."""
import gzip
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import deflate_segments as ds  # noqa: E402
from test_deflate_host_model import host_model  # noqa: E402

from panfeed_amd import _lib, cli  # noqa: E402
from panfeed_amd.engine import GzipMembers  # noqa: E402
from panfeed_amd.output import ClusterMemberSplitter  # noqa: E402

SHAPES = sorted(set(ds.shapes(32768)) - {"residues"})       # (the issue's list; `residues` is the device's concern, run too)


@pytest.mark.parametrize("flags", [0, 1, 2, 4])
@pytest.mark.parametrize("shape", SHAPES + ["residues"])
def test_segments_are_their_texts_members(shape, flags):
    lengths = ds.shapes(ds.chunk_bytes())[shape]
    ends = ds.ends_of(lengths)
    text = ds.text_of(int(ends[-1]))
    members, member_end = ds.host_segments(text, ends, flags)
    want, sizes, at = [], [], 0
    for e in ends.tolist():
        want.append(host_model(text[at:e], flags))
        sizes.append(len(want[-1]))
        at = e
    assert members == b"".join(want)
    assert member_end == np.cumsum(sizes).tolist()
    assert (gzip.decompress(members) if members else b"") == text


def test_one_segment_is_the_plain_container():
    c = ds.chunk_bytes()
    text = ds.text_of(3 * c + 17)
    members, member_end = ds.host_segments(text, [len(text)])
    assert members == host_model(text, 0) and member_end == [len(members)]


def test_short_chunks_count_from_the_segments_start():
    """a segment of C + 1 bytes behind one of 5: members of 5, C and 1 bytes of text -- not cut at multiples of C of the
    whole text"""
    c = ds.chunk_bytes()
    text = ds.text_of(c + 6)
    members, member_end = ds.host_segments(text, [5, c + 6])
    isizes, at = [], 0
    while at < len(members):
        nxt = members.find(members[:8], at + 1)
        nxt = len(members) if nxt < 0 else nxt
        isizes.append(int.from_bytes(members[nxt - 4:nxt], "little"))
        at = nxt
    assert isizes == [5, c, 1]
    assert gzip.decompress(members[:member_end[0]]) == text[:5]


def test_no_segment_no_text():
    assert ds.host_segments(b"", np.zeros(0, dtype=np.uint64)) == (b"", [])


@pytest.mark.parametrize("ends", [[5, 3, 10], [4, 9], [4, 11], []], ids=["decreasing", "last_below_n", "last_above_n", "none_with_text"])
def test_refusals(ends):
    with pytest.raises(_lib.PanfeedHipError) as e:
        ds.host_segments(b"0123456789", np.asarray(ends, dtype=np.uint64))
    assert e.value.status == _lib.ERR_ARG


# ---------------------------------------------------------------------------------------------- the splitter
def _pieces(texts):
    """(members, sizes) of texts, each one gzip member"""
    ms = [gzip.compress(t, mtime=0) for t in texts]
    return ms, [len(m) for m in ms]


class Sink:
    def __init__(self):
        self.calls = []

    def __call__(self, name, piece):
        assert isinstance(piece, GzipMembers)
        self.calls.append((name, bytes(piece.view), piece.text_bytes))

    def text(self, name):
        return b"".join(gzip.decompress(m) if m else b"" for n, m, _ in self.calls if n == name)

    def order(self):
        out = []
        for n, _, _ in self.calls:
            if not out or out[-1] != n:
                out.append(n)
        return out


def test_splitter_cuts_at_a_blocks_start_and_end():
    # cluster a = block 0, cluster b = block 1: the ends fall on the blocks' edges, no cut inside either
    (ma, mb), _ = _pieces([b"aaaa\n", b"bbbbbb\n"])
    sink = Sink()
    sp = ClusterMemberSplitter([5, 12], ["a", "b"], sink)
    sp(ma, 0, 5)
    sp(mb, 5, 7)
    sp.close()
    assert sink.calls == [("a", ma, 5), ("b", mb, 7)]


def test_splitter_several_clusters_in_one_block():
    texts = [b"a\n", b"bb\n", b"ccc\n"]
    ms, sizes = _pieces(texts)
    sink = Sink()
    sp = ClusterMemberSplitter([2, 5, 9], ["a", "b", "c"], sink)
    sp(b"".join(ms), 0, 9, [(2, sizes[0]), (5, sizes[0] + sizes[1])])
    sp.close()
    assert sink.calls == [("a", ms[0], 2), ("b", ms[1], 3), ("c", ms[2], 4)]


def test_splitter_one_cluster_over_three_blocks():
    texts = [b"x" * 10, b"y" * 20, b"z" * 5 + b"\n"]
    ms, _ = _pieces(texts)
    sink = Sink()
    sp = ClusterMemberSplitter([36], ["only"], sink)
    at = 0
    for t, m in zip(texts, ms):
        sp(m, at, len(t))
        at += len(t)
    sp.close()
    assert [c[0] for c in sink.calls] == ["only"] * 3
    assert sink.text("only") == b"".join(texts) and sum(c[2] for c in sink.calls) == 36


def test_splitter_clusters_without_bytes():
    # e0 (empty), a, e1, e2 (empty, between), b over two blocks, e3 (empty, behind)
    ms, sizes = _pieces([b"aa\n", b"b1\n", b"b2\n"])
    names, ends = ["e0", "a", "e1", "e2", "b", "e3"], [0, 3, 3, 3, 9, 9]
    sink = Sink()
    sp = ClusterMemberSplitter(ends, names, sink)
    sp(ms[0] + ms[1], 0, 6, [(3, sizes[0])])
    sp(ms[2], 6, 3)
    sp.close()
    assert sink.order() == names                          # every cluster, once, in order
    assert [(n, t) for n, m, t in sink.calls if not m] == [("e0", 0), ("e1", 0), ("e2", 0), ("e3", 0)]
    assert sink.text("a") == b"aa\n" and sink.text("b") == b"b1\nb2\n"


def test_splitter_refuses_pieces_that_do_not_add_up():
    (ma, mb), sizes = _pieces([b"aaaa\n", b"bbbbbb\n"])
    both = ma + mb
    with pytest.raises(ValueError):                       # a member over a cluster's end: the cut is missing
        ClusterMemberSplitter([5, 12], ["a", "b"], Sink())(both, 0, 12)
    with pytest.raises(ValueError):                       # a block out of place
        ClusterMemberSplitter([5, 12], ["a", "b"], Sink())(mb, 5, 7)
    with pytest.raises(ValueError):                       # a cut beyond the block's members
        ClusterMemberSplitter([5, 12], ["a", "b"], Sink())(both, 0, 12, [(5, len(both) + 1)])
    with pytest.raises(ValueError):                       # text without members
        ClusterMemberSplitter([5, 12], ["a", "b"], Sink())(both, 0, 12, [(5, 0)])
    with pytest.raises(ValueError):                       # text behind the last cluster's end
        ClusterMemberSplitter([5], ["a"], Sink())(both, 0, 12, [(5, sizes[0])])
    sp = ClusterMemberSplitter([5, 12], ["a", "b"], Sink())
    sp(ma, 0, 5)
    with pytest.raises(ValueError):                       # the text ends early
        sp.close()
    with pytest.raises(ValueError):
        ClusterMemberSplitter([5, 3], ["a", "b"], Sink())


# ---------------------------------------------------------------------------------------------- the option
def test_cli_option_reaches_run(tmp_path):
    calls = []

    def stub(*a, **kw):
        calls.append((a, kw))
        return {"clusters": 0, "instances": 0, "patterns": 0, "log": ""}
    old = os.getcwd()
    os.chdir(tmp_path)
    try:
        assert cli.main(["-g", "gffs", "-p", "t.csv", "--multiple-files", "--gpu-compress-clusters"], run=stub) == 0
        assert len(calls) == 1
        # refused before any file is read: the targets file named here does not exist
        assert cli.main(["-g", "gffs", "-p", "t.csv", "--targets", "no_such_file", "--gpu-compress-clusters"], run=stub) == 2
        assert cli.main(["-g", "gffs", "-p", "t.csv", "--multiple-files", "--gpu-compress"], run=stub) == 0
    finally:
        os.chdir(old)
    assert len(calls) == 2
    kw = calls[0][1]
    assert kw["device_gzip_clusters"] is True and kw["compress"] is True and kw["multiple_files"] is True
    assert "device_gzip" not in kw
    assert "device_gzip_clusters" not in calls[1][1] and calls[1][1]["device_gzip"] is True
