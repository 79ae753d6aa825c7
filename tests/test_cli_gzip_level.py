"""The effort level of the device gzip encoder on the command lines (`panfeed --gpu-compress-level`, `panfeed-get-kmers
--gz-level`) without a GPU: how the option reaches run_files and the ranks of `--gpus N`, the refusals and their status,
the default.  The work itself is a recording stand-in, as in tests/test_cli.py."""
import inspect
import os

import pytest

from panfeed_amd import cli

BASE = ["-g", "gffs", "-p", "table.csv"]
MISSING = ["-a", "/no/such/dir/assoc.tsv", "-p", "/no/such/dir/kmers_to_hashes.tsv", "-k", "/no/such/dir/kmers.tsv"]


class Recorder:
    def __init__(self, result):
        self.calls, self.result = [], result

    def __call__(self, *a, **kw):
        self.calls.append((a, kw))
        return self.result


@pytest.fixture
def command(tmp_path, monkeypatch):
    import torch
    for name in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "PANFEED_SHARED_GPU"):
        monkeypatch.delenv(name, raising=False)
    monkeypatch.chdir(tmp_path)

    def run(argv, devices=1):
        monkeypatch.setattr(torch.cuda, "device_count", lambda: devices)
        one = Recorder({"clusters": 0, "instances": 0, "patterns": 0, "log": ""})
        launch = Recorder(0)
        rc = cli.main(argv, run=one, launch=launch)
        return rc, one, launch
    return run


@pytest.mark.parametrize("switches", [["--gpu-compress"], ["--gpu-compress", "--bgzf"],
                                      ["--multiple-files", "--gpu-compress-clusters"]])
@pytest.mark.parametrize("level", [1, 2])
def test_level_reaches_run_files(command, switches, level):
    rc, one, launch = command(BASE + switches + ["--gpu-compress-level", str(level)])
    assert rc == 0 and not launch.calls and len(one.calls) == 1
    kw = one.calls[0][1]
    assert kw["device_gzip_level"] == level
    assert kw.get("device_gzip", False) == ("--gpu-compress" in switches)
    assert kw.get("device_gzip_clusters", False) == ("--gpu-compress-clusters" in switches)
    assert kw.get("bgzf", False) == ("--bgzf" in switches)
    from panfeed_amd import pipeline
    assert set(kw) <= set(inspect.signature(pipeline.run_files).parameters)


def test_level_reaches_the_ranks(command):
    rc, one, launch = command(BASE + ["--gpus", "2", "--gpu-compress", "--gpu-compress-level", "2"], devices=2)
    assert rc == 0 and not one.calls and len(launch.calls) == 1
    a, kw = launch.calls[0]
    assert a[0] == 2 and kw["device_gzip"] is True and kw["device_gzip_level"] == 2
    from panfeed_amd import sharded
    kw.pop("verbose")
    assert set(kw) <= set(inspect.signature(sharded.run_files_sharded).parameters)
    assert "device_gzip_level" in inspect.signature(sharded.run_records_sharded).parameters
    import json
    json.dumps(kw)                          # (the launcher hands the options to the ranks as JSON)


def test_default_is_level_1(command):
    """without the option the run gets level 1: the call leaves it out, as it leaves out every option not given, and
    run_files' and run_files_sharded's own default is 1, which is today's encoder"""
    from panfeed_amd import _lib, pipeline, sharded
    rc, one, launch = command(BASE + ["--gpu-compress"])
    assert rc == 0 and one.calls[0][1].get("device_gzip_level", 1) == 1
    for fn in (pipeline.run_files, sharded.run_files_sharded, sharded.run_records_sharded):
        assert inspect.signature(fn).parameters["device_gzip_level"].default == 1
    assert _lib.gzip_level_flags(1) == 0


@pytest.mark.parametrize("extra", [["--gpu-compress-level", "2"], ["--gpu-compress-level", "1"],
                                   ["--compress", "--gpu-compress-level", "2"],
                                   ["--gpus", "2", "--gpu-compress-level", "2"]])
def test_level_without_a_device_gzip_switch_is_refused(command, tmp_path, extra):
    """status 2 before any file is read (the inputs do not exist), like --bgzf without --gpu-compress"""
    rc, one, launch = command(BASE + ["--targets", "no_such_file.txt"] + extra, devices=2)
    assert rc == 2 and not one.calls and not launch.calls
    assert os.listdir(tmp_path) == []


@pytest.mark.parametrize("value", ["0", "3", "two"])
def test_other_levels_are_refused_by_the_parser(command, value):
    with pytest.raises(SystemExit) as ei:
        command(BASE + ["--gpu-compress", "--gpu-compress-level", value])
    assert ei.value.code == 2


@pytest.mark.parametrize("level", [0, 3, None, "2", True])
def test_run_files_refuses_another_level(tmp_path, level):
    """ValueError before anything is read or made: the inputs do not exist"""
    from panfeed_amd import pipeline, sharded
    with pytest.raises(ValueError):
        pipeline.run_files("no_such.csv", "no_such_gffs", str(tmp_path / "out"), device_gzip=True, device_gzip_level=level)
    with pytest.raises(ValueError):
        sharded.run_files_sharded("no_such.csv", "no_such_gffs", str(tmp_path / "out"), 0, 1, device_gzip=True,
                                  device_gzip_level=level)
    assert not (tmp_path / "out").exists()


def test_gz_level_without_gz_output_is_refused_before_any_file_is_read(capsys):
    from panfeed_amd import downstream
    with pytest.raises(SystemExit) as ei:
        downstream.get_kmers(MISSING + ["--gz-level", "2"])
    assert ei.value.code == 2 and "--gz-output" in capsys.readouterr().err


def test_gz_level_with_gz_output_goes_on_to_read_its_inputs(tmp_path):
    from panfeed_amd import downstream
    for level in ("1", "2"):
        with pytest.raises(FileNotFoundError):
            downstream.get_kmers(MISSING + ["--gz-output", str(tmp_path / "out.tsv.gz"), "--gz-level", level])
    with pytest.raises(SystemExit) as ei:
        downstream.get_kmers(MISSING + ["--gz-output", str(tmp_path / "out.tsv.gz"), "--gz-level", "3"])
    assert ei.value.code == 2 and not (tmp_path / "out.tsv.gz").exists()


def test_get_clusters_has_no_such_option(capsys):
    from panfeed_amd import downstream
    with pytest.raises(SystemExit) as ei:
        downstream.get_clusters(MISSING[:4] + ["--gz-level", "2"])
    assert ei.value.code == 2 and "unrecognized arguments" in capsys.readouterr().err
