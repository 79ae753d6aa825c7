"""`python -m panfeed_amd --gpus N` without a GPU: the refusals and their exit statuses, the mapping onto
`sharded.run_files_sharded`'s arguments, what a launcher's environment makes of the command.  The work is recording
stand-ins for `pipeline.run_files`, `rank.launch` and `rank.run_rank`; the number of devices is a stand-in too
(tests/test_gpu_sharded_stream.py runs the real command)."""
import os

import pytest

from panfeed_amd import cli

BASE = ["-g", "gffs", "-p", "table.csv"]


class Recorder:
    def __init__(self, result):
        self.calls, self.result = [], result

    def __call__(self, *a, **kw):
        self.calls.append((a, kw))
        return self.result


@pytest.fixture
def command(tmp_path, monkeypatch):
    """run(argv, devices=...) -> (exit status, run recorder, launch recorder, rank recorder), in an empty directory, with
    no launcher and no rehearsal in the environment unless the test puts one there"""
    import torch
    for name in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "PANFEED_SHARED_GPU"):
        monkeypatch.delenv(name, raising=False)
    monkeypatch.chdir(tmp_path)

    def run(argv, devices=1, launch_status=0):
        monkeypatch.setattr(torch.cuda, "device_count", lambda: devices)
        one = Recorder({"clusters": 0, "instances": 0, "patterns": 0, "log": ""})
        launch = Recorder(launch_status)
        rank = Recorder({"rank": 1, "clusters": 0, "instances": 0, "patterns": 0, "log": ""})
        rc = cli.main(argv, run=one, launch=launch, rank_entry=rank)
        return rc, one, launch, rank
    return run


def test_fewer_devices_than_ranks_is_refused(command, tmp_path, caplog):
    import logging
    caplog.set_level(logging.ERROR, logger="panfeed")
    rc, one, launch, rank = command(BASE + ["--gpus", "2"], devices=1)
    assert rc == 2 and not one.calls and not launch.calls and not rank.calls
    assert os.listdir(tmp_path) == []
    assert any("one rank per GPU" in r.getMessage() for r in caplog.records)


@pytest.mark.parametrize("extra", [["--gpus", "0"], ["--gpus", "-3"], ["--gpus", "2", "--device", "3"]])
def test_bad_gpus_and_device_are_refused(command, tmp_path, extra):
    rc, one, launch, rank = command(BASE + extra, devices=8)
    assert rc == 2 and not one.calls and not launch.calls and not rank.calls
    assert os.listdir(tmp_path) == []


def test_gpus_maps_onto_run_files_sharded(command, tmp_path):
    (tmp_path / "t.txt").write_text("s2\ns1\n")
    (tmp_path / "g.txt").write_text("grp_b\ngrp_a\n")
    rc, one, launch, rank = command(BASE + ["--gpus", "2", "-o", "out", "-k", "21", "--gpu-compress", "--stop-on-missing",
                                            "--targets", "t.txt", "--genes", "g.txt", "--upstream", "5"], devices=2)
    assert rc == 0 and not one.calls and not rank.calls and len(launch.calls) == 1
    a, kw = launch.calls[0]
    assert a == (2, "table.csv", "gffs", "out")
    kw.pop("verbose")
    assert kw == dict(fastadir=None, klength=21, canon=True, consider_missing=False, patfilt=True, maf=0.01, upstream=5,
                      downstream=0, downstream_start_codon=False, targets=("s1", "s2"), genes=["grp_a", "grp_b"],
                      compress=True, multiple_files=False, batch_clusters=256, gpu=0, raise_missing=True, device_gzip=True)
    # every one of them is an argument of run_files_sharded
    import inspect

    from panfeed_amd import sharded
    assert set(kw) <= set(inspect.signature(sharded.run_files_sharded).parameters)
    assert not (tmp_path / "out").exists()


def test_launch_status_is_the_commands(command):
    rc, one, launch, rank = command(BASE + ["--gpus", "4"], devices=4, launch_status=3)
    assert rc == 3 and launch.calls[0][0][0] == 4


def test_one_gpu_is_todays_call(command):
    rc, one, launch, rank = command(BASE + ["--gpus", "1"], devices=0)
    assert rc == 0 and not launch.calls and not rank.calls and len(one.calls) == 1
    a, kw = one.calls[0]
    assert a == ("table.csv", "gffs", "panfeed")
    assert kw == dict(fastadir=None, klength=31, canon=True, consider_missing=False, patfilt=True, maf=0.01, upstream=0,
                      downstream=0, downstream_start_codon=False, targets=(), genes=None, compress=False,
                      multiple_files=False, batch_clusters=256, device=0, raise_missing=False)
    rc, one, launch, rank = command(BASE, devices=0)
    assert rc == 0 and one.calls[0][1] == kw and not launch.calls


@pytest.mark.parametrize("extra,status", [
    (["--downstream-start-codon", "--upstream", "10", "--downstream", "20"], 1),
    (["--maf", "0.51"], 1),
    (["-k", "127"], 2),
    (["-k", "0"], 2),
])
def test_todays_refusals_come_first(command, tmp_path, extra, status):
    """with fewer devices than ranks too: the reference's refusals and the k range are what the user is told"""
    rc, one, launch, rank = command(BASE + ["--gpus", "2", "--targets", "no_such_file.txt"] + extra, devices=1)
    assert rc == status and not one.calls and not launch.calls and not rank.calls
    assert os.listdir(tmp_path) == []


def test_existing_output_is_refused_before_the_ranks_start(command, tmp_path):
    (tmp_path / "out").mkdir()
    rc, one, launch, rank = command(BASE + ["--gpus", "2", "-o", "out"], devices=2)
    assert rc == 1 and not launch.calls


def test_rehearsal_needs_no_second_device(command, monkeypatch):
    monkeypatch.setenv("PANFEED_SHARED_GPU", "1")
    rc, one, launch, rank = command(BASE + ["--gpus", "2", "--device", "0"], devices=1)
    assert rc == 0 and len(launch.calls) == 1 and launch.calls[0][0][0] == 2 and not one.calls


def test_under_a_launcher_the_command_is_one_rank(command, monkeypatch, tmp_path):
    monkeypatch.setenv("WORLD_SIZE", "2")
    monkeypatch.setenv("RANK", "1")
    (tmp_path / "out").mkdir()            # rank 0 may have made it already: the ranks look together, later
    rc, one, launch, rank = command(BASE + ["-o", "out", "--compress"], devices=0)
    assert rc == 0 and not one.calls and not launch.calls and len(rank.calls) == 1
    a, kw = rank.calls[0]
    assert a == ("table.csv", "gffs", "out") and kw["compress"] is True and kw["raise_missing"] is False
    assert "device" not in kw and "device_gzip" not in kw


def test_help_says_what_a_rehearsal_is(capsys):
    with pytest.raises(SystemExit):
        cli.get_options(["--help"])
    text = " ".join(capsys.readouterr().out.split())
    assert "--gpus" in text and "PANFEED_SHARED_GPU" in text and "control flow only" in text


@pytest.mark.parametrize("shared", [True, False])
def test_every_process_group_gets_a_finite_timeout(monkeypatch, shared):
    """what `run_rank` hands to init_process_group, RCCL run and rehearsal: a timedelta, the default or the environment's"""
    import datetime

    import torch.distributed as dist

    from panfeed_amd import rank

    class Stop(Exception):
        pass
    seen = []

    def init(backend, **kw):
        seen.append((backend, kw))
        raise Stop
    monkeypatch.setattr(dist, "init_process_group", init)
    monkeypatch.setenv("RANK", "1")
    monkeypatch.setenv("WORLD_SIZE", "2")
    monkeypatch.setenv("LOCAL_RANK", "1")
    monkeypatch.delenv("PANFEED_DIST_TIMEOUT_S", raising=False)
    (monkeypatch.setenv("PANFEED_SHARED_GPU", "1") if shared else monkeypatch.delenv("PANFEED_SHARED_GPU", raising=False))
    with pytest.raises(Stop):
        rank.run_rank("table.csv", "gffs", "out")
    monkeypatch.setenv("PANFEED_DIST_TIMEOUT_S", "90")
    with pytest.raises(Stop):
        rank.run_rank("table.csv", "gffs", "out")
    assert [b for b, _ in seen] == ["gloo" if shared else "nccl"] * 2
    assert [kw["timeout"] for _, kw in seen] == [datetime.timedelta(seconds=rank.TIMEOUT_S), datetime.timedelta(seconds=90)]
    assert all(kw["rank"] == 1 and kw["world_size"] == 2 for _, kw in seen)


def test_only_a_rehearsal_sets_the_ipc_mode(monkeypatch):
    import subprocess

    from panfeed_amd import rank
    envs = []

    class Done:
        returncode = 0
    monkeypatch.setattr(subprocess, "run", lambda cmd, env: envs.append((cmd, env)) or Done())
    monkeypatch.delenv("HSA_ENABLE_IPC_MODE_LEGACY", raising=False)
    monkeypatch.delenv("PANFEED_SHARED_GPU", raising=False)
    assert rank.launch(2, "table.csv", "gffs", "out", klength=21) == 0
    monkeypatch.setenv("PANFEED_SHARED_GPU", "1")
    assert rank.launch(2, "table.csv", "gffs", "out", klength=21) == 0
    assert "HSA_ENABLE_IPC_MODE_LEGACY" not in envs[0][1] and envs[1][1]["HSA_ENABLE_IPC_MODE_LEGACY"] == "0"
    assert "--nproc-per-node=2" in envs[0][0] and envs[0][0][-3:-1] == ["-m", "panfeed_amd.rank"]
