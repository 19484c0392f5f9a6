#!/usr/bin/env python3
"""Measurement aid: the masked blend over a caller's pose buffers (aclhip_blend_poses_batch), HIP events on one stream. One batch: 65 536
instances x 100 bones (the humanoid hierarchy), K = 2 and K = 4 input buffers, weighted without masks and layered with masks, local and
object space: eight cases. The yardstick is measured in the same process on the same rows, interleaved with them:
aclhip_transform_poses_batch with object space and no additive buffer from one of the input buffers into the output (one row read, one
written).
Before anything is timed every case is CHECKED bit for bit on a sample of rows (POSE_BUFFER_BLEND_SAMPLE, spread over the batch) against the
CPU oracle: the per slot weights in numpy float32 as include/aclhip.h states them, oracle_blend_poses per group of slots with one weight
tuple, oracle_local_to_object_space. A mismatch or a refused instance exits non-zero.
Time is reported, never judged: per case the median of POSE_BUFFER_BLEND_ROUNDS interleaved rounds of POSE_BUFFER_BLEND_REPEATS launches
each, the spread (max - min) / median, and the algorithmic bytes -- (K + 1) x rows, plus the weights and the mask handles (the mask values
themselves are a few hundred bytes that stay in the caches) -- as a rate and as a fraction of the HBM peak of the specification (8 TB/s).
Prints one JSON line."""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402
from acl_amd import runtime, synth  # noqa: E402
from oracle import bindings as ob  # noqa: E402  (the checker)

N = int(os.environ.get("POSE_BUFFER_BLEND_INSTANCES", "65536"))
BONES = int(os.environ.get("POSE_BUFFER_BLEND_BONES", "100"))
ROUNDS = int(os.environ.get("POSE_BUFFER_BLEND_ROUNDS", "9"))
REPEATS = int(os.environ.get("POSE_BUFFER_BLEND_REPEATS", "20"))
SAMPLE = int(os.environ.get("POSE_BUFFER_BLEND_SAMPLE", "48"))
POOL = 2048          # distinct random rows per buffer; the batch repeats them (every row has its own address: the traffic is the batch's)
HBM_PEAK_BYTES_PER_SECOND = 8.0e12
WEIGHTED, LAYERED = runtime.BLEND_WEIGHTED, runtime.BLEND_LAYERED
ONE = np.float32(1.0)


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


def slot_weights(weights, masks, mode):
    """steps 1 and 2 of the header's definition, float32, one operation at a time"""
    opacity = np.stack([np.full(BONES, np.float32(w), dtype=np.float32) if mask is None else np.float32(w) * mask for w, mask in zip(weights, masks)])
    if mode == WEIGHTED:
        return opacity
    layered = np.empty_like(opacity)
    for k in range(len(weights)):
        rest = np.ones(BONES, dtype=np.float32)
        for j in range(len(weights) - 1, k, -1):
            rest = rest * (ONE - opacity[j])
        layered[k] = opacity[k] * rest
    return layered


def expected_row(poses, weights, masks, mode, parents):
    per_slot = slot_weights(weights, masks, mode)
    columns = np.ascontiguousarray(per_slot.T).view(np.uint32)
    tuples, inverse = np.unique(columns, axis=0, return_inverse=True)
    inverse = np.asarray(inverse).reshape(-1)
    row = np.empty_like(poses[0])
    for index in range(tuples.shape[0]):
        slots = np.flatnonzero(inverse == index)
        row[slots] = ob.oracle_blend_poses([np.ascontiguousarray(pose[slots]) for pose in poses], np.ascontiguousarray(tuples[index]).view(np.float32))
    return ob.oracle_local_to_object_space(parents, row) if parents is not None else row


def main():
    if not torch.cuda.is_available():
        raise SystemExit("tools/pose_buffer_blend.py needs a GPU: nothing is measured without one")
    stride = BONES * 48
    parents = np.array(synth.humanoid_hierarchy(BONES), dtype=np.uint32)
    identity = np.zeros((BONES, 12), dtype=np.float32)
    identity[:, 3], identity[:, 8:11] = 1.0, 1.0
    rng = np.random.default_rng(7000 + BONES)
    stream = torch.cuda.Stream()
    s = stream.cuda_stream
    ctx = runtime.Context(0)
    skeleton = ctx.register_skeleton(parents, identity)
    # masks: the bottom layer is 1 everywhere (e_0 == 1), the layers above are an upper body, an arm and a head with soft edges
    mask_values = [np.ones(BONES, dtype=np.float32)]
    for begin, end in ((BONES // 2, BONES), (BONES // 4, BONES // 2), (BONES - BONES // 8, BONES)):
        mask = np.zeros(BONES, dtype=np.float32)
        mask[begin:end] = 1.0
        mask[begin:min(begin + 4, end)] = np.linspace(0.2, 0.8, min(4, end - begin), dtype=np.float32)
        mask_values.append(mask)
    mask_handles = [ctx.register_blend_mask(mask) for mask in mask_values]
    repeats_of_pool = (N + POOL - 1) // POOL
    pools = [random_rows(rng, min(POOL, N)) for _ in range(4)]
    with torch.cuda.stream(stream):
        inputs = [torch.from_numpy(pool).cuda().repeat(repeats_of_pool, 1, 1)[:N].contiguous() for pool in pools]
        out, yardstick_out = (torch.zeros((N, BONES, 12), dtype=torch.float32, device="cuda") for _ in range(2))
    sample = np.unique(np.linspace(0, N - 1, min(SAMPLE, N)).astype(np.int64))

    cases, checks = {}, []
    keep = []
    for num_buffers in (2, 4):
        for name, mode, masked in (("weighted", WEIGHTED, False), ("layered_masked", LAYERED, True)):
            if mode == WEIGHTED:
                weights = rng.dirichlet(np.ones(num_buffers), size=N).astype(np.float32)
            else:
                weights = rng.uniform(0.0, 1.0, size=(N, num_buffers)).astype(np.float32)
                weights[:, 0] = 1.0
            handles = np.tile(np.array(mask_handles[:num_buffers], dtype=np.uint32), (N, 1)) if masked else None
            with torch.cuda.stream(stream):
                d_weights = torch.from_numpy(weights).cuda()
                d_handles = torch.from_numpy(handles.view(np.int32)).cuda() if masked else None
            keep += [d_weights, d_handles]
            for object_space in (False, True):
                blend = runtime.PoseBufferBlend()
                blend.skeleton, blend.num_buffers, blend.mode, blend.object_space = skeleton, num_buffers, mode, int(object_space)
                for k in range(num_buffers):
                    blend.buffers[k], blend.buffer_stride_bytes[k] = inputs[k].data_ptr(), stride
                blend.weights = d_weights.data_ptr()
                blend.instance_masks = d_handles.data_ptr() if masked else None
                key = "k%u_%s_%s" % (num_buffers, name, "object" if object_space else "local")
                cases[key] = (lambda blend=blend: ctx.blend_poses_batch(blend, N, out.data_ptr(), stride, stream=s))
                traffic = (num_buffers + 1) * N * stride + N * num_buffers * 4 * (2 if masked else 1)
                checks.append((key, num_buffers, mode, weights, mask_values[:num_buffers] if masked else [None] * num_buffers, object_space, traffic))

    on_buffers = runtime.PoseBufferConsumers()
    on_buffers.skeleton, on_buffers.object_space = skeleton, 1

    def yardstick():
        ctx.transform_poses_batch(inputs[0].data_ptr(), stride, N, on_buffers, yardstick_out.data_ptr(), stride, stream=s)

    # ---- checked before it is timed
    for key, num_buffers, mode, weights, masks, object_space, _ in checks:
        with torch.cuda.stream(stream):          # (the clear, the launch and the gather on ONE stream: in order)
            out.zero_()
            cases[key]()
            got = out[torch.from_numpy(sample).cuda()].cpu().numpy()
        for index, i in enumerate(sample):
            want = expected_row([pools[k][i % POOL] for k in range(num_buffers)], weights[i], masks, mode, parents if object_space else None)
            if not np.array_equal(got[index].view(np.uint32), want.view(np.uint32)):
                print(f"MISMATCH in {key}, instance {i}", flush=True)
                sys.exit(1)
    with torch.cuda.stream(stream):
        yardstick()
        yardstick_rows = yardstick_out[torch.from_numpy(sample[:8]).cuda()].cpu().numpy()
    for index, i in enumerate(sample[:8]):
        want = ob.oracle_local_to_object_space(parents, pools[0][i % POOL])
        if not np.array_equal(yardstick_rows[index].view(np.uint32), want.view(np.uint32)):
            print(f"MISMATCH in the yardstick, instance {i}", flush=True)
            sys.exit(1)
    if ctx.rejected_instance_count() != 0:
        print(f"refused instances: {ctx.rejected_instance_count()}", flush=True)
        sys.exit(1)

    timed_cases = dict(cases, yardstick_transform_object=yardstick)
    for launch in timed_cases.values():          # warm-up: every shape of the timed window
        timed(stream, launch, 3)
    samples = {key: [] for key in timed_cases}
    for _ in range(ROUNDS):
        for key, launch in timed_cases.items():
            samples[key].append(timed(stream, launch, REPEATS))
    result = {"instances": N, "bones": BONES, "rounds": ROUNDS, "repeats": REPEATS, "checked_rows": int(sample.size), "us": {}, "traffic": {}}
    for key, values in samples.items():
        values = np.array(values)
        result["us"][key] = {"median": round(float(np.median(values)), 2), "min": round(float(values.min()), 2), "max": round(float(values.max()), 2),
                             "spread": round(float((values.max() - values.min()) / np.median(values)), 4)}
    traffic = {key: bytes_moved for key, _, _, _, _, _, bytes_moved in checks}
    traffic["yardstick_transform_object"] = 2 * N * stride
    for key, bytes_moved in traffic.items():
        rate = bytes_moved / (result["us"][key]["median"] * 1e-6)
        result["traffic"][key] = {"bytes": bytes_moved, "gb_per_second": round(rate / 1e9, 1), "fraction_of_hbm_peak": round(rate / HBM_PEAK_BYTES_PER_SECOND, 3)}
        result["us"][key]["over_yardstick"] = round(result["us"][key]["median"] / result["us"]["yardstick_transform_object"]["median"], 3)
    ctx.close()
    print(json.dumps(result), flush=True)


if __name__ == "__main__":
    main()
