#!/usr/bin/env python3
"""A measuring script, not a test: it stands here because it uses the CPU oracle, which only tests/ may.  Sizes of the
device gzip encoder's two effort levels by its serial host model, without a GPU: a `hashes_to_patterns` text at --samples
strains (12 `synth` clusters, flanks 100, k = 31, as tools/gzip_device_bench.py makes its input, with empty cells for
missing genes) made by the CPU oracle, cut and coded as the device does it at level 1 (flags 0) and level 2 (PF_GZ_DEEP),
beside zlib 1 / 4 / 6 / 9 over the same cuts.  At 5 000 strains a row is 10 KB and a 32 KiB chunk holds three of them:
only the rows behind a chunk's first newline have a row before them.  Results: profiles/gzip_deep/README.md.

Usage: python tests/deflate_deep_sizes.py [--clusters 12] [--samples 5000] [--bytes 4194304] [--out FILE.json]
"""
import argparse
import ctypes as C
import json
import os
import sys
import zlib

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)


def host_model(L, _lib, data, flags):
    out, n = C.c_void_p(), C.c_uint64()
    _lib.check(L.pf_gzip_host_model(data, len(data), flags, C.byref(out), C.byref(n)))
    size = int(n.value)
    L.pf_free_text(out)
    return size


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--clusters", type=int, default=12)
    ap.add_argument("--samples", type=int, default=5000)
    ap.add_argument("--bytes", type=int, default=4 << 20, help="of the text, from its start")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    from oracle import oracle as po
    from panfeed_amd import _lib, synth
    L = _lib.load()
    cut = int(L.pf_gzip_device_chunk_bytes())
    clusters = synth.generate(args.clusters, args.samples, flank=100)     # (as tools/gzip_device_bench.py makes its n1 input)
    run = po.OracleRun(klength=31, stroi=set(), canon=True, consider_missing=True, patfilt=True, maf=0.01)
    run.feed([c.record() for c in clusters])
    text = run.texts()[2].encode()[:args.bytes]
    rows = text.count(b"\n")
    res = {"samples": args.samples, "clusters": args.clusters, "text_bytes": len(text), "rows": rows,
           "row_bytes": len(text) / max(1, rows), "chunk_bytes": cut,
           "host_model_level1_bytes": host_model(L, _lib, text, 0), "host_model_level2_bytes": host_model(L, _lib, text, 16)}
    for level in (1, 4, 6, 9):
        total = 0
        for at in range(0, len(text), cut):
            z = zlib.compressobj(level, zlib.DEFLATED, 31)
            total += len(z.compress(text[at:at + cut])) + len(z.flush())
        res[f"zlib{level}_on_cuts_bytes"] = total
    res["level2_over_level1"] = res["host_model_level2_bytes"] / res["host_model_level1_bytes"]
    print(json.dumps(res, indent=1))
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
