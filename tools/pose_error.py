#!/usr/bin/env python3
"""Measurement aid: the shell error of two pose buffers (aclhip_measure_pose_error_batch), HIP events on one stream. One batch:
65 536 instances x 100 bones (the humanoid hierarchy), object space, three cases:
  records               the 8 byte record per instance alone
  records_worst         and the launch's worst record (the second, one workgroup launch)
  records_bones_worst   and every bone's error (4 bytes per bone more written)
The yardstick is what a caller pays today before it has compared anything, measured in the same process on the same buffers, interleaved
with the cases: TWO aclhip_transform_poses_batch launches with object space, one per buffer, each from its buffer into an output buffer.
Before anything is timed every case is CHECKED bit for bit on a sample of instances (POSE_ERROR_SAMPLE, spread over the batch) against the
composition of tests/test_pose_error_oracle.py (the CPU oracle's functions plus numpy float32 operations), and the worst record against
the scan of ALL the records the device wrote. A mismatch or a refused instance exits non-zero.
Time is reported, never judged: per case the median of POSE_ERROR_ROUNDS interleaved rounds of POSE_ERROR_REPEATS launches each, the
spread (max - min) / median, the ratio to the yardstick's median, and the algorithmic bytes (two row reads, 8 bytes per instance and the
optional outputs written) as a rate and as a fraction of the HBM peak of the specification (8 TB/s). Prints one JSON line."""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import torch  # noqa: E402
from acl_amd import runtime, synth  # noqa: E402
from test_pose_error_oracle import expected_measure  # noqa: E402  (the checker's composition)

N = int(os.environ.get("POSE_ERROR_INSTANCES", "65536"))
BONES = int(os.environ.get("POSE_ERROR_BONES", "100"))
ROUNDS = int(os.environ.get("POSE_ERROR_ROUNDS", "3"))
REPEATS = int(os.environ.get("POSE_ERROR_REPEATS", "20"))
SAMPLE = int(os.environ.get("POSE_ERROR_SAMPLE", "48"))
SHELL = 3.0
POOL = 2048          # distinct random rows per buffer; the batch repeats them (every row has its own address: the traffic is the batch's)
HBM_PEAK_BYTES_PER_SECOND = 8.0e12


def timed(stream, launch, repeats):
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record(stream)
    for _ in range(repeats):
        launch()
    stop.record(stream)
    stop.synchronize()
    return start.elapsed_time(stop) * 1000.0 / repeats


def random_rows(rng, count):
    rows = np.zeros((count, BONES, 12), dtype=np.float32)
    rotations = rng.normal(size=(count, BONES, 4))
    rows[..., 0:4] = rotations / np.linalg.norm(rotations, axis=2, keepdims=True)
    rows[..., 4:7] = rng.uniform(-10.0, 10.0, size=(count, BONES, 3))
    rows[..., 8:11] = rng.uniform(0.9, 1.1, size=(count, BONES, 3))
    return rows


def main():
    if not torch.cuda.is_available():
        raise SystemExit("tools/pose_error.py needs a GPU: nothing is measured without one")
    stride = BONES * 48
    parents = np.array(synth.humanoid_hierarchy(BONES), dtype=np.uint32)
    identity = np.zeros((BONES, 12), dtype=np.float32)
    identity[:, 3], identity[:, 8:11] = 1.0, 1.0
    rng = np.random.default_rng(7300 + BONES)
    stream = torch.cuda.Stream()
    s = stream.cuda_stream
    ctx = runtime.Context(0)
    skeleton = ctx.register_skeleton(parents, identity)
    repeats_of_pool = (N + POOL - 1) // POOL
    raw_pool = random_rows(rng, min(POOL, N))
    # the lossy rows: the raw ones as a codec leaves them, a relative error of up to 1e-3 per float
    lossy_pool = (raw_pool * (1.0 + rng.uniform(-1.0e-3, 1.0e-3, size=raw_pool.shape))).astype(np.float32)
    with torch.cuda.stream(stream):
        raw, lossy = (torch.from_numpy(pool).cuda().repeat(repeats_of_pool, 1, 1)[:N].contiguous() for pool in (raw_pool, lossy_pool))
        yardstick_out = torch.zeros((N, BONES, 12), dtype=torch.float32, device="cuda")
        errors = torch.zeros((N, 2), dtype=torch.int32, device="cuda")
        bone_errors = torch.zeros((N, BONES), dtype=torch.float32, device="cuda")
        worst = torch.zeros(4, dtype=torch.int32, device="cuda")
    sample = np.unique(np.linspace(0, N - 1, min(SAMPLE, N)).astype(np.int64))
    d_sample = torch.from_numpy(sample).cuda()

    def desc_of(with_bones, with_worst):
        desc = runtime.PoseErrorDesc()
        desc.skeleton, desc.object_space, desc.shell_distance = skeleton, 1, SHELL
        if with_bones:
            desc.bone_errors, desc.bone_error_stride_bytes = bone_errors.data_ptr(), BONES * 4
        if with_worst:
            desc.worst = worst.data_ptr()
        return desc

    descs = {"records": desc_of(False, False), "records_worst": desc_of(False, True), "records_bones_worst": desc_of(True, True)}
    forward = runtime.PoseBufferConsumers()
    forward.skeleton, forward.object_space = skeleton, 1

    def measure(key):
        return lambda: ctx.measure_pose_error(raw.data_ptr(), stride, lossy.data_ptr(), stride, N, descs[key], errors.data_ptr(), stream=s)

    def two_transforms():
        ctx.transform_poses_batch(raw.data_ptr(), stride, N, forward, yardstick_out.data_ptr(), stride, stream=s)
        ctx.transform_poses_batch(lossy.data_ptr(), stride, N, forward, yardstick_out.data_ptr(), stride, stream=s)

    cases = {key: measure(key) for key in descs}
    cases["yardstick_two_transforms_object"] = two_transforms
    traffic = {"records": 2 * N * stride + 8 * N, "records_worst": 2 * N * stride + 8 * N + 8 * N + 16, "records_bones_worst": 2 * N * stride + 8 * N + 4 * BONES * N + 8 * N + 16,
               "yardstick_two_transforms_object": 4 * N * stride}

    # ---- checked before it is timed (the clears, the launch and the gathers on ONE stream: in order)
    wanted = [expected_measure(parents, raw_pool[i % POOL], lossy_pool[i % POOL], SHELL) for i in sample]
    for key in descs:
        with torch.cuda.stream(stream):
            errors.zero_(), bone_errors.fill_(-5.0), worst.zero_()
            cases[key]()
            got_records = errors.cpu().numpy().view(runtime.POSE_ERROR_DTYPE).reshape(N)
            got_bones = bone_errors[d_sample].cpu().numpy()
            got_worst = worst.cpu().numpy().view(runtime.POSE_ERROR_WORST_DTYPE)[0]
        for index, i in enumerate(sample):
            bone_row, (error, bone), _ = wanted[index]
            same = got_records[i]["error"].view(np.uint32) == np.float32(error).view(np.uint32) and int(got_records[i]["bone"]) == bone
            if key == "records_bones_worst":
                same = same and np.array_equal(got_bones[index].view(np.uint32), bone_row.view(np.uint32))
            if not same:
                print(f"MISMATCH in {key}, instance {i}", flush=True)
                sys.exit(1)
        if key != "records":
            # the scan of the host over every record the device wrote: the greatest error, the lowest instance that has it
            greatest = got_records["error"].max()
            first = int(np.flatnonzero(got_records["error"] == greatest)[0])
            if (got_worst["error"], int(got_worst["instance"]), int(got_worst["bone"]), int(got_worst["reserved"])) != (greatest, first, int(got_records[first]["bone"]), 0):
                print(f"MISMATCH in the worst record of {key}: {got_worst}", flush=True)
                sys.exit(1)
    if ctx.rejected_instance_count() != 0:
        print(f"refused instances: {ctx.rejected_instance_count()}", flush=True)
        sys.exit(1)

    for launch in cases.values():          # warm-up: every shape of the timed window
        timed(stream, launch, 3)
    samples = {key: [] for key in cases}
    for _ in range(ROUNDS):
        for key, launch in cases.items():
            samples[key].append(timed(stream, launch, REPEATS))
    result = {"instances": N, "bones": BONES, "rounds": ROUNDS, "repeats": REPEATS, "checked_instances": int(sample.size), "us": {}, "traffic": {}}
    for key, values in samples.items():
        values = np.array(values)
        result["us"][key] = {"median": round(float(np.median(values)), 2), "min": round(float(values.min()), 2), "max": round(float(values.max()), 2),
                             "spread": round(float((values.max() - values.min()) / np.median(values)), 4)}
    for key, bytes_moved in traffic.items():
        rate = bytes_moved / (result["us"][key]["median"] * 1e-6)
        result["traffic"][key] = {"bytes": bytes_moved, "gb_per_second": round(rate / 1e9, 1), "fraction_of_hbm_peak": round(rate / HBM_PEAK_BYTES_PER_SECOND, 3)}
        result["us"][key]["over_yardstick"] = round(result["us"][key]["median"] / result["us"]["yardstick_two_transforms_object"]["median"], 3)
    ctx.close()
    print(json.dumps(result), flush=True)


if __name__ == "__main__":
    main()
