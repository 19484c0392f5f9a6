"""bench.py as every change is measured with it: a plain run sets up, warms up, times --steps launches and prints the line, nothing
else; --dump-outputs DIR writes what the last timed launch computed -- the oracle's poses, in the caller's instance order, a fixed sample
of rows where the batch is larger than the dump -- and the same file from run to run, whatever order the device chose. Needs a GPU."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from oracle import bindings as ob
import bench

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _plain_run(tmp_path, label, *arguments):
    """one plain `bench.py --gpus 1 --steps 5 --warmup 2 --dump-outputs DIR` run; returns (the line, DIR/poses.npy)"""
    directory = tmp_path / label
    env = dict(os.environ, ACLHIP_BENCH_DETAILS=str(tmp_path / f"{label}_details.json"))
    command = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "5", "--warmup", "2", "--dump-outputs", str(directory), *arguments]
    completed = subprocess.run(command, cwd=ROOT, env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=300)
    assert completed.returncode == 0, completed.stderr[-3000:]
    lines = [line for line in completed.stdout.splitlines() if line.startswith("{")]
    assert len(lines) == 1, completed.stdout[-2000:]
    assert sorted(os.listdir(directory)) == ["poses.npy"]
    return json.loads(lines[0]), np.load(directory / "poses.npy")


def _same_bits(a, b):
    return a.shape == b.shape and np.array_equal(np.ascontiguousarray(a).view(np.uint32), np.ascontiguousarray(b).view(np.uint32))


def _oracle_poses(workload, instances, rows):
    clips, clip_indices, times = bench.build_workload(workload, 0, instances)
    expected = ob.oracle_decompress_tracks_batch([c.blob for c in clips], clip_indices[rows], times[rows], max(c.num_tracks for c in clips))
    return expected.reshape(rows.size, -1)


def test_a_plain_run_times_its_steps_and_dumps_the_last_step(tmp_path):
    """the headline batch (64k instances x 100 bones, 314 MB of poses): the line carries the contract's figures for exactly --steps
    timed launches and none of the --full legs; the dump is the seeded row sample, bit exact against the oracle"""
    line, poses = _plain_run(tmp_path, "one_clip")
    assert line["steps"] == 5 and line["warmup"] == 2 and line["n_gpus"] == 1
    assert line["value"] > 0 and line["ms_per_step"] > 0 and line["unit"] == "poses/s" and line["higher_is_better"] is True and line["dtype"] == "f32"
    assert abs(line["value"] * line["ms_per_step"] * 1e-3 / bench.INSTANCES_PER_GPU - 1.0) < 1e-3      # poses/s = instances per step / step time
    for leg in ("cpu_baseline", "self_check", "checks", "gather"):
        assert leg not in line, leg
    assert line["workloads"] == {} and "kernel_ms_back_to_back" not in line["roofline"]

    rows = bench.dump_rows(bench.INSTANCES_PER_GPU, 100 * 48)
    assert 0 < rows.size < bench.INSTANCES_PER_GPU and poses.nbytes <= bench.DUMP_BYTES
    assert poses.dtype == np.float32 and poses.shape == (rows.size, 100 * 12)
    assert _same_bits(poses, _oracle_poses("one_clip", bench.INSTANCES_PER_GPU, rows))


@pytest.mark.parametrize("order", ["device", "list"])
def test_dumps_of_device_chosen_orders_are_in_instance_order(tmp_path, order):
    """orders the device picks by atomics (aclhip_order_instances_device; an instance list's slots): the poses come back in the caller's
    instance order, so two runs dump the same bits; the device order's clips never change, so its dump is the oracle's too"""
    instances = 4096
    first_line, first = _plain_run(tmp_path, "first", "--workload", "256_clips", "--order", order, "--instances", str(instances))
    _, second = _plain_run(tmp_path, "second", "--workload", "256_clips", "--order", order, "--instances", str(instances))
    assert first.shape == (instances, 100 * 12) and first_line["config"]["instances_per_gpu"] == instances
    assert _same_bits(first, second)
    if order == "device":
        assert _same_bits(first, _oracle_poses("256_clips", instances, np.arange(instances)))
