"""panfeed-get-kmers' device join under the weak-hash variant of the library, in a process of its own, started once by
tests/test_gpu_kmerjoin.py.

    python tests/kmerjoin_weakhash_worker.py OUTDIR

Points panfeed_amd._lib.LIB_PATH at libpanfeed_hip_weakhash.so before anything loads the library and runs the handmade
table of tests/join_tables.py with the text site's mask at 0, 0x7 and ~0; writes OUTDIR/results.json: per mask the text,
how many bunches went each way and the join's count of look-ups whose hash was equal and whose bytes were not.  Asserts
nothing about the results: the test module does.
"""
import ctypes as C
import io
import json
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))

import join_tables as jt  # noqa: E402

VARIANT = "libpanfeed_hip_weakhash.so"
TEXT_SITE = 3
MASKS = (0, 0x7, 0xFFFFFFFFFFFFFFFF)


def main(outdir):
    from panfeed_amd import _lib
    _lib.LIB_PATH = os.path.join(os.path.dirname(_lib.LIB_PATH), VARIANT)
    L = _lib.load()
    assert b"weak-hash" in L.pf_version(), L.pf_version()
    L.pf_debug_set_hash_mask_site.argtypes = [C.c_int, C.c_uint64]
    from panfeed_amd import downstream
    from panfeed_amd.downstream import KmerJoin
    t = jt.handmade()
    paths = {}
    for name, data in (("assoc.tsv", t["assoc"].encode()), ("kh.tsv", t["kh"]), ("kmers.tsv", t["kmers"])):
        paths[name] = os.path.join(outdir, name)
        with open(paths[name], "wb") as fh:
            fh.write(data)
    argv = ["-a", paths["assoc.tsv"], "-p", paths["kh.tsv"], "-k", paths["kmers.tsv"], "-t", "0.5", "--clusters-per-iteration", "2"]
    results = {}
    for mask in MASKS:
        _lib.check(L.pf_debug_set_hash_mask_site(TEXT_SITE, mask))
        before = (KmerJoin.device_bunches, KmerJoin.host_bunches, KmerJoin.host_runs)
        out = io.StringIO()
        rc = downstream.get_kmers(argv, out=out)
        after = (KmerJoin.device_bunches, KmerJoin.host_bunches, KmerJoin.host_runs)
        results[f"{mask:#x}"] = {"rc": rc, "text": out.getvalue(), "routes": [b - a for a, b in zip(before, after)],
                                 "hash_rejects": KmerJoin.last_stats["hash_rejects"]}
    with open(os.path.join(outdir, "results.json"), "w") as fh:
        json.dump(results, fh)


if __name__ == "__main__":
    main(sys.argv[1])
