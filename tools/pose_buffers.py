#!/usr/bin/env python3
"""Measurement aid: the pose consumers over a caller's pose buffers (aclhip_transform_poses_batch) against the fused route, HIP events on one
stream. One batch: 65 536 instances of the bench's 100-bone clip, object space. Interleaved in ONE process over POSE_BUFFERS_ROUNDS rounds of
POSE_BUFFERS_REPEATS launches each:
  (a) decode + walk     aclhip_decompress_tracks_batch into a row buffer, then aclhip_transform_poses_batch in place over it
  (b) fused             aclhip_decompress_poses_batch(object_space = 1) on the same batch -- through a library built from the PARENT commit
                        too when POSE_BUFFERS_PARENT_LIBRARY=<path of its libaclhip.so> is set (b_parent: the yardstick), loaded side by
                        side into the same process with a context of its own
  (c) walk alone        aclhip_transform_poses_batch from one buffer into another, against its traffic: num_instances x B x 48 bytes read
                        plus as much written -- and (c_additive) once more read with an additive buffer (additive1, object space)
Before anything is timed every case is CHECKED bit for bit: the rows of (a), (c) and b_parent against (b); the rows of (c_additive)
against the fused aclhip_decompress_poses_batch with the same base_poses buffer. A mismatch or a refused instance exits non-zero.
Time is reported, never judged: per case the median of the rounds' per-launch times and the spread (max - min) / median; a / b, and (c) as a
fraction of the HBM peak of the specification (8 TB/s). Prints one JSON line."""
import ctypes
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402
from acl_amd import runtime, synth  # noqa: E402

N = int(os.environ.get("POSE_BUFFERS_INSTANCES", "65536"))
ROUNDS = int(os.environ.get("POSE_BUFFERS_ROUNDS", "9"))
REPEATS = int(os.environ.get("POSE_BUFFERS_REPEATS", "20"))
HBM_PEAK_BYTES_PER_SECOND = 8.0e12
SPEC = dict(seed=2, num_tracks=100, num_samples=301, sample_rate=30.0)


def parent_context(path):
    """A context of a second build of the library in this process: the functions this tool calls, with the binding's own signatures"""
    current = runtime.load_library()
    lib = ctypes.CDLL(path)
    for name in ("aclhip_create", "aclhip_destroy", "aclhip_register_clip", "aclhip_set_clip_hierarchy", "aclhip_decompress_poses_batch", "aclhip_get_rejected_instance_count",
                 "aclhip_last_error_message", "aclhip_status_string", "aclhip_default_params"):
        getattr(lib, name).argtypes, getattr(lib, name).restype = getattr(current, name).argtypes, getattr(current, name).restype
    context = runtime.Context.__new__(runtime.Context)
    context._lib, context.device_index, handle = lib, 0, ctypes.c_void_p()
    status = lib.aclhip_create(0, ctypes.byref(handle))
    if status != 0:
        raise RuntimeError(f"aclhip_create of {path}: status {status}")
    context._handle = handle
    return context


def timed(stream, launch, repeats):
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record(stream)
    for _ in range(repeats):
        launch()
    stop.record(stream)
    stop.synchronize()
    return start.elapsed_time(stop) * 1000.0 / repeats


def same_bits(a, b):
    return bool(torch.equal(a.view(torch.int32), b.view(torch.int32)))


def main():
    if not torch.cuda.is_available():
        raise SystemExit("tools/pose_buffers.py needs a GPU: nothing is measured without one")
    clip = synth.build_clip(**SPEC)
    bones = clip.num_tracks
    stride = bones * 48
    parents = np.array(synth.humanoid_hierarchy(bones), dtype=np.uint32)
    identity = np.zeros((bones, 12), dtype=np.float32)
    identity[:, 3], identity[:, 8:11] = 1.0, 1.0
    rng = np.random.default_rng(4100 + bones)
    times = rng.uniform(0.0, clip.duration, size=N).astype(np.float32)
    stream = torch.cuda.Stream()
    s = stream.cuda_stream
    contexts = {"this": runtime.Context(0)}
    parent_path = os.environ.get("POSE_BUFFERS_PARENT_LIBRARY")
    if parent_path:
        contexts["parent"] = parent_context(parent_path)
    handles = {}
    for key, context in contexts.items():
        handles[key] = context.register_clip(clip.blob)
        context.set_clip_hierarchy(handles[key], parents)
    ctx = contexts["this"]
    skeleton = ctx.register_skeleton(parents, identity)
    with torch.cuda.stream(stream):
        d_clips = {key: torch.full((N,), handle, dtype=torch.int32, device="cuda") for key, handle in handles.items()}
        d_times = torch.from_numpy(times).cuda()
        fused_rows, staged, local, walked, other = (torch.zeros((N, bones, 12), dtype=torch.float32, device="cuda") for _ in range(5))
    object_space = runtime.PoseConsumers()
    object_space.object_space = 1
    on_buffers = runtime.PoseBufferConsumers()
    on_buffers.skeleton, on_buffers.object_space = skeleton, 1
    with_additive = runtime.PoseBufferConsumers()
    with_additive.skeleton, with_additive.object_space, with_additive.additive_format = skeleton, 1, runtime.ADDITIVE_ADDITIVE1
    with_additive.additive_poses, with_additive.additive_pose_stride_bytes = local.data_ptr(), stride

    def fused(key="this", out=fused_rows):
        contexts[key].decompress_poses_batch(d_clips[key].data_ptr(), d_times.data_ptr(), N, out.data_ptr(), stride, object_space, stream=s)

    def decode(out):
        ctx.decompress_tracks_batch(d_clips["this"].data_ptr(), d_times.data_ptr(), N, out.data_ptr(), stride, stream=s)

    def decode_then_walk():
        decode(staged)
        ctx.transform_poses_batch(staged.data_ptr(), stride, N, on_buffers, staged.data_ptr(), stride, stream=s)

    def walk_alone():
        ctx.transform_poses_batch(local.data_ptr(), stride, N, on_buffers, walked.data_ptr(), stride, stream=s)

    def walk_with_additive():
        # the base is the decoded pose as well (any finite pose serves): additive1 of the local pose onto itself, then the walk
        ctx.transform_poses_batch(local.data_ptr(), stride, N, with_additive, walked.data_ptr(), stride, stream=s)

    # ---- checked before it is timed
    fused()
    decode(local)
    decode_then_walk()
    walk_alone()
    stream.synchronize()
    ok = same_bits(staged, fused_rows) and same_bits(walked, fused_rows)
    base_buffer = runtime.PoseConsumers()
    base_buffer.object_space, base_buffer.additive_format, base_buffer.base_poses, base_buffer.base_pose_stride_bytes = 1, runtime.ADDITIVE_ADDITIVE1, local.data_ptr(), stride
    ctx.decompress_poses_batch(d_clips["this"].data_ptr(), d_times.data_ptr(), N, other.data_ptr(), stride, base_buffer, stream=s)
    walk_with_additive()
    stream.synchronize()
    ok = ok and same_bits(walked, other)
    if "parent" in contexts:
        fused("parent", other)
        stream.synchronize()
        ok = ok and same_bits(other, fused_rows)
    refused = sum(c.rejected_instance_count() for c in contexts.values())
    if not ok or refused != 0:
        print(f"MISMATCH (refused instances: {refused})", flush=True)
        sys.exit(1)

    cases = {"a_decode_walk": decode_then_walk, "b_fused": fused, "c_walk": walk_alone, "c_additive": walk_with_additive, "decode": lambda: decode(staged)}
    if "parent" in contexts:
        cases["b_parent"] = lambda: fused("parent", other)
    for launch in cases.values():          # warm-up: every shape of the timed window
        timed(stream, launch, 3)
    samples = {key: [] for key in cases}
    for _ in range(ROUNDS):
        for key, launch in cases.items():
            samples[key].append(timed(stream, launch, REPEATS))
    result = {"instances": N, "bones": bones, "rounds": ROUNDS, "repeats": REPEATS, "checked": True, "us": {}}
    for key, values in samples.items():
        values = np.array(values)
        result["us"][key] = {"median": round(float(np.median(values)), 2), "min": round(float(values.min()), 2), "max": round(float(values.max()), 2),
                             "spread": round(float((values.max() - values.min()) / np.median(values)), 4)}
    median = {key: result["us"][key]["median"] for key in cases}
    result["a_over_b"] = round(median["a_decode_walk"] / median["b_fused"], 3)
    if "b_parent" in median:
        result["a_over_b_parent"] = round(median["a_decode_walk"] / median["b_parent"], 3)
        result["b_over_b_parent"] = round(median["b_fused"] / median["b_parent"], 3)
    row_bytes = N * bones * 48
    for key, passes in (("c_walk", 2), ("c_additive", 3)):
        rate = passes * row_bytes / (median[key] * 1e-6)
        result[key + "_traffic"] = {"bytes": passes * row_bytes, "gb_per_second": round(rate / 1e9, 1), "fraction_of_hbm_peak": round(rate / HBM_PEAK_BYTES_PER_SECOND, 3)}
    for c in contexts.values():
        c.close()
    print(json.dumps(result), flush=True)


if __name__ == "__main__":
    main()
