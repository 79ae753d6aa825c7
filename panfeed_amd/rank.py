"""One rank of `python -m panfeed_amd --gpus N`, and what starts the ranks.

`launch` is the parent's side: it makes no HIP call, starts N fresh child processes through `torch.distributed.run` (one
per GPU, each `python -m panfeed_amd.rank <options>`), lets their log lines through and returns their exit status --
non-zero if any rank's was; the launcher ends the other ranks once one has failed.  `run_rank` is a child's side, and
also what `python -m panfeed_amd` does when a launcher of the user's own has put `WORLD_SIZE` and `RANK` into the
environment: the process group (RCCL, with a finite timeout: a rank that died cannot leave the others waiting for ever),
`sharded.run_files_sharded` on the rank's GPU, the run's summary line from rank 0.

`PANFEED_SHARED_GPU=1` is a rehearsal for a machine with fewer GPUs than ranks: every rank runs on the one device given
(`gpu`), the collectives are gloo's on host tensors.  It exercises the control flow only; nothing it takes is a multi-GPU
time.
"""
import datetime
import json
import logging
import os
import socket
import subprocess
import sys

logger = logging.getLogger("panfeed")

TIMEOUT_S = 1800        # of every collective, unless PANFEED_DIST_TIMEOUT_S says otherwise


def shared_gpu():
    return os.environ.get("PANFEED_SHARED_GPU") == "1"


def launched():
    """whether a launcher has made this process one rank of a world"""
    return "WORLD_SIZE" in os.environ and "RANK" in os.environ


def run_rank(presence_absence, gffdir, output, gpu=0, **options):
    """this process as the rank the environment says (RANK, WORLD_SIZE, LOCAL_RANK, MASTER_ADDR, MASTER_PORT):
    `options` are `run_files_sharded`'s.  Returns the run's summary (rank 0's counters with the clusters and instances of
    all ranks); raises what the rank raised."""
    import torch
    import torch.distributed as dist

    from . import sharded
    rank, world = int(os.environ["RANK"]), int(os.environ["WORLD_SIZE"])
    timeout = datetime.timedelta(seconds=float(os.environ.get("PANFEED_DIST_TIMEOUT_S", TIMEOUT_S)))
    if shared_gpu():
        device, gpu = None, int(gpu)
        dist.init_process_group("gloo", rank=rank, world_size=world, timeout=timeout)
    else:
        gpu = int(os.environ.get("LOCAL_RANK", rank))
        device = torch.device("cuda", gpu)
        dist.init_process_group("nccl", rank=rank, world_size=world, timeout=timeout, device_id=device)
    try:
        stats = sharded.run_files_sharded(presence_absence, gffdir, output, rank, world, dist, device, gpu=gpu, **options)
        totals = torch.tensor([stats.get("clusters", 0), stats.get("instances", 0)], dtype=torch.int64)
        if device is not None:
            totals = totals.to(device)
        dist.all_reduce(totals)
        stats["clusters"], stats["instances"] = (int(x) for x in totals.tolist())
        return stats
    finally:
        dist.destroy_process_group()


def report(stats, output):
    """the warnings of this rank's reader, and from rank 0 the run's summary line"""
    for line in (stats.get("log") or "").splitlines():
        logger.warning(line)
    if stats.get("rank", 0) == 0:
        logger.info(f"{stats.get('clusters', 0)} gene clusters, {stats.get('instances', 0)} k-mer instances, "
                    f"{stats.get('patterns', 0)} patterns written to {output}")


def launch(world, presence_absence, gffdir, output, verbose=0, **options):
    """`world` fresh child processes, one rank each; returns their exit status.  This process never touches the GPU."""
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    spec = json.dumps({"args": [presence_absence, gffdir, output], "options": options, "verbose": verbose})
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={int(world)}", "--master-addr",
           "127.0.0.1", "--master-port", str(port), "-m", "panfeed_amd.rank", spec]
    env = dict(os.environ)
    if shared_gpu():                      # (several processes on one device: the rehearsal's setting, not an RCCL run's)
        env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env["PYTHONPATH"] = root + (os.pathsep + env["PYTHONPATH"] if env.get("PYTHONPATH") else "")
    return subprocess.run(cmd, env=env).returncode


def main(argv=None):
    """`python -m panfeed_amd.rank <json>`: the child `launch` starts"""
    from ._lib import PanfeedHipError
    from .cli import set_logging
    spec = json.loads((sys.argv[1:] if argv is None else argv)[0])
    set_logging(spec.get("verbose", 0))
    options = spec["options"]
    options["targets"] = tuple(options.get("targets") or ())
    try:
        stats = run_rank(*spec["args"], **options)
    except (PanfeedHipError, FileExistsError, RuntimeError) as e:
        logger.error(f"rank {os.environ.get('RANK', '?')}: {e}")
        return 1
    report(stats, spec["args"][2])
    return 0


if __name__ == "__main__":
    sys.exit(main())
