#!/usr/bin/env python3
"""Measurement aid: object -> local space and make-additive over a caller's pose buffers (aclhip_inverse_transform_poses_batch), HIP events
on one stream. One batch: 65 536 instances x 100 bones (the humanoid hierarchy), three cases:
  local                 local_space, from one buffer into another
  local_in_place        local_space, in place (the buffer is rewritten by every launch: after the first one its rows are no object space
                        pose any more, only numbers of the same kind -- the launch has no data dependent path but the matrix route, and
                        the rows hold no negative scale)
  local_relative        local_space and convert_to_relative against a base buffer, from one buffer into another
The yardstick is measured in the same process on the same buffers, interleaved with them: aclhip_transform_poses_batch with object space
and no additive buffer from the source buffer into the output (one row read, one written -- the bytes of `local`).
Before anything is timed every case is CHECKED bit for bit on a sample of rows (POSE_BUFFER_INVERSE_SAMPLE, spread over the batch) against
the composition of tests/test_pose_buffer_inverse_oracle.py (the CPU oracle's functions plus numpy float32 operations). A mismatch or a
refused instance exits non-zero.
Time is reported, never judged: per case the median of POSE_BUFFER_INVERSE_ROUNDS interleaved rounds of POSE_BUFFER_INVERSE_REPEATS launches
each, the spread (max - min) / median, the ratio to the yardstick's median, and the algorithmic bytes as a rate and as a fraction of the HBM
peak of the specification (8 TB/s). Prints one JSON line."""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import torch  # noqa: E402
from acl_amd import runtime, synth  # noqa: E402
from oracle import bindings as ob  # noqa: E402  (the checker)
from test_pose_buffer_inverse_oracle import expected_inverse_row  # noqa: E402  (the checker's composition)

N = int(os.environ.get("POSE_BUFFER_INVERSE_INSTANCES", "65536"))
BONES = int(os.environ.get("POSE_BUFFER_INVERSE_BONES", "100"))
ROUNDS = int(os.environ.get("POSE_BUFFER_INVERSE_ROUNDS", "3"))
REPEATS = int(os.environ.get("POSE_BUFFER_INVERSE_REPEATS", "20"))
SAMPLE = int(os.environ.get("POSE_BUFFER_INVERSE_SAMPLE", "48"))
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
        raise SystemExit("tools/pose_buffer_inverse.py needs a GPU: nothing is measured without one")
    stride = BONES * 48
    parents = np.array(synth.humanoid_hierarchy(BONES), dtype=np.uint32)
    identity = np.zeros((BONES, 12), dtype=np.float32)
    identity[:, 3], identity[:, 8:11] = 1.0, 1.0
    rng = np.random.default_rng(7100 + BONES)
    stream = torch.cuda.Stream()
    s = stream.cuda_stream
    ctx = runtime.Context(0)
    skeleton = ctx.register_skeleton(parents, identity)
    repeats_of_pool = (N + POOL - 1) // POOL
    pools = [random_rows(rng, min(POOL, N)) for _ in range(2)]
    with torch.cuda.stream(stream):
        source, base = (torch.from_numpy(pool).cuda().repeat(repeats_of_pool, 1, 1)[:N].contiguous() for pool in pools)
        rewritten = source.clone()
        out, yardstick_out = (torch.zeros((N, BONES, 12), dtype=torch.float32, device="cuda") for _ in range(2))
    sample = np.unique(np.linspace(0, N - 1, min(SAMPLE, N)).astype(np.int64))
    d_sample = torch.from_numpy(sample).cuda()

    to_local = runtime.PoseBufferInverse()
    to_local.skeleton, to_local.local_space = skeleton, 1
    to_relative = runtime.PoseBufferInverse()
    to_relative.skeleton, to_relative.local_space, to_relative.additive_format = skeleton, 1, runtime.ADDITIVE_RELATIVE
    to_relative.base_poses, to_relative.base_pose_stride_bytes = base.data_ptr(), stride
    forward = runtime.PoseBufferConsumers()
    forward.skeleton, forward.object_space = skeleton, 1

    cases = {
        "local": lambda: ctx.inverse_transform_poses_batch(source.data_ptr(), stride, N, to_local, out.data_ptr(), stride, stream=s),
        "local_in_place": lambda: ctx.inverse_transform_poses_batch(rewritten.data_ptr(), stride, N, to_local, rewritten.data_ptr(), stride, stream=s),
        "local_relative": lambda: ctx.inverse_transform_poses_batch(source.data_ptr(), stride, N, to_relative, out.data_ptr(), stride, stream=s),
        "yardstick_transform_object": lambda: ctx.transform_poses_batch(source.data_ptr(), stride, N, forward, yardstick_out.data_ptr(), stride, stream=s),
    }
    traffic = {"local": 2 * N * stride, "local_in_place": 2 * N * stride, "local_relative": 3 * N * stride, "yardstick_transform_object": 2 * N * stride}

    # ---- checked before it is timed (the clear, the launch and the gather on ONE stream: in order)
    def rows_of(key, buffer):
        with torch.cuda.stream(stream):
            if buffer is not rewritten:
                buffer.zero_()
            cases[key]()
            return buffer[d_sample].cpu().numpy()

    got = {"local": rows_of("local", out), "local_in_place": rows_of("local_in_place", rewritten), "local_relative": rows_of("local_relative", out),
           "yardstick_transform_object": rows_of("yardstick_transform_object", yardstick_out)}
    for index, i in enumerate(sample):
        row = pools[0][i % POOL]
        local, _ = expected_inverse_row(parents, row)
        want = {"local": local, "local_in_place": local, "local_relative": expected_inverse_row(parents, row, True, runtime.ADDITIVE_RELATIVE, pools[1][i % POOL])[0],
                "yardstick_transform_object": ob.oracle_local_to_object_space(parents, row)}
        for key in cases:
            if not np.array_equal(got[key][index].view(np.uint32), want[key].view(np.uint32)):
                print(f"MISMATCH in {key}, instance {i}", flush=True)
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
    result = {"instances": N, "bones": BONES, "rounds": ROUNDS, "repeats": REPEATS, "checked_rows": int(sample.size), "us": {}, "traffic": {}}
    for key, values in samples.items():
        values = np.array(values)
        result["us"][key] = {"median": round(float(np.median(values)), 2), "min": round(float(values.min()), 2), "max": round(float(values.max()), 2),
                             "spread": round(float((values.max() - values.min()) / np.median(values)), 4)}
    for key, bytes_moved in traffic.items():
        rate = bytes_moved / (result["us"][key]["median"] * 1e-6)
        result["traffic"][key] = {"bytes": bytes_moved, "gb_per_second": round(rate / 1e9, 1), "fraction_of_hbm_peak": round(rate / HBM_PEAK_BYTES_PER_SECOND, 3)}
        result["us"][key]["over_yardstick"] = round(result["us"][key]["median"] / result["us"]["yardstick_transform_object"]["median"], 3)
    ctx.close()
    print(json.dumps(result), flush=True)


if __name__ == "__main__":
    main()
