"""One rank of a sharded --multiple-files run with the per-cluster files gzipped on the GPU, started by
tests/test_gpu_cluster_files_gzip.py the way tests/sharded_worker.py starts its ranks: one process per rank, each with its
own Engine, all on cuda:0, gloo collectives on host tensors.

    python tests/cluster_gzip_worker.py RANK WORLD PORT OUTDIR TABLE GFFDIR K UPSTREAM DOWNSTREAM TARGET,TARGET
"""
import json
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)


def main():
    rank, world, port, outdir, csvp, gffdir, k, up, down, tg = sys.argv[1:11]
    rank, world = int(rank), int(world)
    import torch.distributed as dist
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = port
    dist.init_process_group("gloo", rank=rank, world_size=world)
    from panfeed_amd import sharded
    stats = sharded.run_files_sharded(csvp, gffdir, outdir, rank, world, dist, None, klength=int(k), upstream=int(up),
                                      downstream=int(down), targets=tuple(t for t in tg.split(",") if t),
                                      multiple_files=True, device_gzip_clusters=True, batch_clusters=5)
    stats.pop("log", None)
    dist.barrier()
    dist.destroy_process_group()
    print("STATS " + json.dumps(stats), flush=True)


if __name__ == "__main__":
    main()
