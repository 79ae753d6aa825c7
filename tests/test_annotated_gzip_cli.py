"""The command lines around the compressed annotated table (panfeed-get-kmers --gz-output, panfeed-plot --host-gunzip)
and the host writer of its small members, without a GPU."""
import gzip
import os
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from device_gz_files import member_sizes  # noqa: E402

MISSING = ["-a", "/no/such/dir/assoc.tsv", "-p", "/no/such/dir/kmers_to_hashes.tsv", "-k", "/no/such/dir/kmers.tsv"]
CHUNK = 32768


def test_gz_output_wants_a_gz_suffix_before_any_file_is_read(tmp_path, capsys):
    """the inputs do not exist: a run that opened one would end with FileNotFoundError, not with argparse's status 2"""
    from panfeed_amd import downstream
    out = tmp_path / "out.tsv"
    with pytest.raises(SystemExit) as ei:
        downstream.get_kmers(MISSING + ["--gz-output", str(out)])
    assert ei.value.code == 2
    assert "--gz-output" in capsys.readouterr().err and not out.exists()


def test_gz_output_with_the_suffix_goes_on_to_read_its_inputs(tmp_path):
    from panfeed_amd import downstream
    with pytest.raises(FileNotFoundError):
        downstream.get_kmers(MISSING + ["--gz-output", str(tmp_path / "out.tsv.gz")])
    assert not (tmp_path / "out.tsv.gz").exists()


def test_get_clusters_has_no_such_option(capsys):
    from panfeed_amd import downstream
    with pytest.raises(SystemExit) as ei:
        downstream.get_clusters(MISSING[:4] + ["--gz-output", "out.tsv.gz"])
    assert ei.value.code == 2 and "unrecognized arguments" in capsys.readouterr().err


def test_plot_takes_host_gunzip():
    from panfeed_amd.plot import get_options
    assert get_options(["-k", "x", "-p", "y", "--host-gunzip"]).host_gunzip is True
    assert get_options(["-k", "x", "-p", "y"]).host_gunzip is False


def _members(raw):
    out, at = [], 0
    for n in member_sizes(raw):
        out.append(raw[at:at + n])
        at += n
    return out


@pytest.mark.parametrize("first", ["host", "members"])
def test_small_member_writer(tmp_path, first):
    """host text in writes of every size, members in between: the file inflates to all of it in order, the first line has a
    member of its own, no host member holds more than a chunk of text or is empty, and every member starts alike"""
    from panfeed_amd.output import SmallMemberGzipWriter
    p = tmp_path / "t.tsv.gz"
    ready = gzip.compress(b"made\telsewhere\n" * 3, mtime=0)
    body = b"".join(b"row%d\t%s\n" % (i, b"x" * (i * 37 % 900)) for i in range(400))
    exp = b""
    with SmallMemberGzipWriter(str(p), CHUNK) as w:
        if first == "host":
            w.write("cluster\tk-mer\n" + body[:10].decode())
            exp += b"cluster\tk-mer\n" + body[:10]
        w.write_members(ready)
        exp += b"made\telsewhere\n" * 3
        for at in range(10, len(body), 7001):
            w.write(body[at:at + 7001])
        exp += body[10:]
        w.write_members(memoryview(ready))
        exp += b"made\telsewhere\n" * 3
        w.write("no newline at the end")
        exp += b"no newline at the end"
    raw = p.read_bytes()
    assert gzip.decompress(raw) == exp and len(body) > 3 * CHUNK
    ms = _members(raw)
    texts = [gzip.decompress(m) for m in ms]
    assert b"".join(texts) == exp and all(texts) and max(len(t) for t in texts) == CHUNK
    assert all(m[:8] == raw[:8] and m[3] == 0 and m[4:8] == bytes(4) for m in ms)
    assert texts[0] == (b"cluster\tk-mer\n" if first == "host" else b"made\telsewhere\n" * 3)
    assert w.text_bytes == len(exp) - 2 * len(b"made\telsewhere\n" * 3) and w.bytes_written == len(raw)


def test_small_member_writer_with_nothing_written(tmp_path):
    from panfeed_amd.output import SmallMemberGzipWriter
    p = tmp_path / "empty.tsv.gz"
    SmallMemberGzipWriter(str(p), CHUNK).close()
    raw = p.read_bytes()
    assert raw[:4] == b"\x1f\x8b\x08\x00" and gzip.decompress(raw) == b""
