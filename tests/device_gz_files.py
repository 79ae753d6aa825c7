"""Device-gzipped table files for the tests of the row filter's member route: the bytes pf_gzip_device makes, a file as
--gpu-compress writes it, and the sizes of such a file's members."""
import ctypes as C
import gzip

import inflate_cases as ic


def device_gzip(eng, data):
    from panfeed_amd import _lib
    out, n = C.c_void_p(), C.c_uint64()
    _lib.check(eng.L.pf_gzip_device(eng.ctx, data, len(data), 0, C.byref(out), C.byref(n)))
    try:
        return C.string_at(out, n.value) if n.value else b""
    finally:
        eng.L.pf_free_text(out)


def write_device_gz(eng, path, header, rows):
    """as --gpu-compress writes it: the header line's member from the host, the rows' members from the device"""
    from panfeed_amd.output import MemberGzipWriter
    with MemberGzipWriter(str(path)) as w:
        w.write(header)
        w.write_members(device_gzip(eng, rows))
    with gzip.open(path, "rb") as fh:
        assert fh.read() == header + rows


def member_sizes(raw):
    at, sizes = 0, []
    while at < len(raw):
        nxt = raw.find(ic.HEAD[:8], at + 1)
        nxt = len(raw) if nxt < 0 else nxt
        sizes.append(nxt - at)
        at = nxt
    return sizes
