"""One rank of a sharded run with the stream / device-gzip options, started by tests/test_sharded_members_cpu.py (mode
oracle: no GPU; the CPU oracle stands in for the engine and hands the part writer gzip members made by the host model of
the device encoder) and tests/test_gpu_sharded_stream.py (mode gpu: a real Engine per rank, all on cuda:0, gloo
collectives on host tensors).

    python tests/sharded_stream_worker.py MODE RANK WORLD PORT OUTDIR CASE OPTIONS_JSON

CASE: a golden case name, `empty` (no cluster at all), `seeded` (the worker's own records, `seeded_case`), or (mode gpu)
files:<table.csv>:<gff dir>:<k>:<target,target> for `run_files_sharded`.  OPTIONS_JSON: device_gzip, targets_text_budget,
raise_missing.
"""
import base64
import ctypes as C
import json
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))

SEEDED = dict(n_clusters=6, samples=64, k=21, flank=30, seed=977)


def seeded_case():
    """(records, all strains, options): 6 clusters x 64 samples, k = 21, +-30 bp, two target strains, and the first two
    clusters once more at the end under other names -- every pattern of theirs has been seen by an earlier rank"""
    from panfeed_amd import synth
    cl = synth.generate(SEEDED["n_clusters"], SEEDED["samples"], first=SEEDED["seed"], flank=SEEDED["flank"], mean_len=400,
                        min_len=90, max_len=900, n_rate=0.004, paralog_rate=0.02)
    names = cl[0].names
    opts = {"klength": SEEDED["k"], "canon": True, "consider_missing": False, "patfilt": True, "maf": 0.01,
            "multiple_files": False, "stroi": [names[1], names[len(names) // 2]]}
    recs = [c.record() for c in cl]
    recs += [(r[0], r[1] + "_again", r[2]) for r in recs[:2]]
    return recs, names, opts


def load_case(spec):
    if spec == "seeded":
        return seeded_case()
    if spec == "empty":
        return [], ["s1", "s2", "s3"], {"klength": 31, "canon": True, "consider_missing": False, "patfilt": True, "maf": 0.01,
                                        "multiple_files": False, "stroi": []}
    from conftest import all_cases, case_records
    case = {c["name"]: c for c in all_cases()}[spec]
    return case_records(case), case["all_strains"], case["opts"]


def host_model_members(text):
    """the gzip members the host model of the device encoder makes of `text`"""
    from panfeed_amd import _lib
    from panfeed_amd.engine import GzipMembers, _mem
    L = _lib.load()
    data = text.encode()
    out, n = C.c_void_p(), C.c_uint64()
    _lib.check(L.pf_gzip_host_model(data, len(data), 0, C.byref(out), C.byref(n)))
    try:
        return GzipMembers(memoryview(bytes(_mem(out, n.value))), len(data))
    finally:
        L.pf_free_text(out)


class OracleMemberShard:
    """PatternSource stand-in: the oracle's texts of this rank's clusters -- the two batch files as members (what an
    Engine(device_gzip=True) hands over), the pattern rows through render_pattern_rows only, so that they take the part
    writer's host-member path"""

    def __init__(self, records, start, opts):
        self.start = start
        if not records:
            self.kmers_tsv = self.kmers_to_hashes = host_model_members("")
            self.rows = []
            return
        from oracle import oracle as po
        run = po.OracleRun(klength=opts["klength"], stroi=set(opts["stroi"]) if opts["stroi"] else (), canon=opts["canon"],
                           consider_missing=opts["consider_missing"], patfilt=opts["patfilt"], maf=opts["maf"])
        run.feed(records)
        kt, kh, hp = run.texts()
        self.kmers_tsv, self.kmers_to_hashes = host_model_members(kt), host_model_members(kh)
        self.rows = [r + "\n" for r in hp.split("\n") if r]

    def export_patterns(self):
        md5 = np.zeros((len(self.rows), 16), dtype=np.uint8)
        for i, r in enumerate(self.rows):
            md5[i] = np.frombuffer(base64.b64decode(r[:24]), dtype=np.uint8)
        fs = (np.uint64(self.start) << np.uint64(32)) + np.arange(len(self.rows), dtype=np.uint64)
        return md5, fs

    def render_pattern_rows(self, ids):
        yield "".join(self.rows[int(i)] for i in ids).encode()


def main():
    mode, rank, world, port, outdir, spec = sys.argv[1], int(sys.argv[2]), int(sys.argv[3]), sys.argv[4], sys.argv[5], sys.argv[6]
    more = json.loads(sys.argv[7]) if len(sys.argv) > 7 else {}
    import datetime

    import torch.distributed as dist
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = port
    if world > 1:
        dist.init_process_group("gloo", rank=rank, world_size=world, timeout=datetime.timedelta(seconds=120))
    d = dist if world > 1 else None
    from panfeed_amd import sharded
    from panfeed_amd.distributed import shard_range
    if spec.startswith("files:"):
        _, csvp, gffdir, k, tg = spec.split(":")
        stats = sharded.run_files_sharded(csvp, gffdir, outdir, rank, world, d, None, klength=int(k),
                                          targets=tuple(t for t in tg.split(",") if t), batch_clusters=5, **more)
        stats.pop("log", None)
    elif mode == "oracle":
        records, strains, opts = load_case(spec)
        start, stop = shard_range(len(records), rank, world)
        src = OracleMemberShard(records[start:stop], start, opts)
        w = sharded.ShardWriter(outdir, rank, device_gzip=True)
        w.write_batch(src.kmers_tsv, src.kmers_to_hashes)
        rows, n_global = sharded.finish_shard(src, w, d, None)
        w.close()
        if d:
            d.barrier()
        if rank == 0:
            sharded.assemble(outdir, world, strains, device_gzip=True)
        stats = {"rank": rank, "pattern_rows": rows, "patterns": n_global, "range": [start, stop], "bytes": w.bytes}
    else:
        records, strains, opts = load_case(spec)
        stats = sharded.run_records_sharded(records, outdir, strains, rank, world, d, None, klength=opts["klength"],
                                            canon=opts["canon"], consider_missing=opts["consider_missing"],
                                            patfilt=opts["patfilt"], maf=opts["maf"], targets=opts["stroi"] or (),
                                            batch_clusters=3, **more)
    if d:
        d.barrier()
        d.destroy_process_group()
    print("STATS " + json.dumps(stats), flush=True)


if __name__ == "__main__":
    main()
