#!/usr/bin/env python3
"""Measurement aid: character bounds (aclhip_decompress_poses_batch_bounds) against today's route, HIP events on one stream. Batches:
65 536 instances of the bench's 100-bone clip and of its 300-bone rig (with scale), object space. Per batch, interleaved in ONE process
over BOUNDS_ROUNDS rounds of BOUNDS_REPEATS launches each:
  (a) rows           aclhip_decompress_poses_batch, the rows alone
  (b) rows + torch   (a) followed by torch amin / amax over the translations of the rows: what a caller does today
  (c) rows + bounds  the fused launch with a pose buffer
  (d) bounds         the fused launch with poses == NULL
  (e) parent rows    (a) through a library built from the PARENT commit (BOUNDS_PARENT_LIBRARY=<path of its libaclhip.so>), loaded side by
                     side into the same process with a context of its own; left out when the variable is not set
Before anything is timed every case is CHECKED: the rows of (c) and (e) bit for bit against (a), the boxes of (c) and (d) with
np.array_equal against numpy's min / max over the rows of (a) and against torch's of (b); a mismatch or a refused instance exits non-zero.
Time is reported, never judged: per case the median of the rounds' per-launch times and the spread (max - min) / median. Prints one JSON
line per batch."""
import ctypes
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402
from acl_amd import runtime, synth  # noqa: E402

N = int(os.environ.get("BOUNDS_INSTANCES", "65536"))
ROUNDS = int(os.environ.get("BOUNDS_ROUNDS", "9"))
REPEATS = int(os.environ.get("BOUNDS_REPEATS", "20"))

BATCHES = {
    "one_clip_100": dict(seed=2, num_tracks=100, num_samples=301, sample_rate=30.0),
    "cinematic_300": dict(seed=4, num_tracks=300, num_samples=451, sample_rate=30.0, has_scale=1, scale_default=0.7, scale_constant=0.1, rotation_constant=0.45, translation_constant=0.8),
}


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


def measure(name, spec, parent_path):
    clip = synth.build_clip(**spec)
    bones = clip.num_tracks
    parents = np.array(synth.humanoid_hierarchy(bones), dtype=np.uint32)
    rng = np.random.default_rng(4100 + bones)
    times = rng.uniform(0.0, clip.duration, size=N).astype(np.float32)
    stream = torch.cuda.Stream()
    s = stream.cuda_stream
    contexts = {"this": runtime.Context(0)}
    if parent_path:
        contexts["parent"] = parent_context(parent_path)
    handles = {}
    for key, ctx in contexts.items():
        handles[key] = ctx.register_clip(clip.blob)
        ctx.set_clip_hierarchy(handles[key], parents)
    with torch.cuda.stream(stream):
        d_clips = {key: torch.full((N,), handle, dtype=torch.int32, device="cuda") for key, handle in handles.items()}
        d_times = torch.from_numpy(times).cuda()
        rows = torch.zeros((N, bones, 12), dtype=torch.float32, device="cuda")
        other_rows = torch.zeros_like(rows)
        boxes = torch.zeros((N, 8), dtype=torch.float32, device="cuda")
    consumers, bounds = runtime.PoseConsumers(), runtime.PoseBounds()
    consumers.object_space, bounds.bounds = 1, boxes.data_ptr()
    ctx = contexts["this"]

    def rows_launch(key="this", out=rows):
        contexts[key].decompress_poses_batch(d_clips[key].data_ptr(), d_times.data_ptr(), N, out.data_ptr(), bones * 48, consumers, stream=s)

    def rows_then_torch():
        rows_launch()
        with torch.cuda.stream(stream):
            translations = rows[:, :, 4:7]
            return torch.amin(translations, dim=1), torch.amax(translations, dim=1)

    def fused(out):
        ctx.decompress_poses_batch_bounds(d_clips["this"].data_ptr(), d_times.data_ptr(), N, bounds, out.data_ptr() if out is not None else None, bones * 48, consumers, stream=s)

    # ---- checked before it is timed
    minimum, maximum = rows_then_torch()
    stream.synchronize()
    host_rows = rows.cpu().numpy()
    expected = np.zeros((N, 8), dtype=np.float32)
    expected[:, 0:3], expected[:, 4:7] = host_rows[:, :, 4:7].min(axis=1), host_rows[:, :, 4:7].max(axis=1)
    ok = np.array_equal(expected[:, 0:3], minimum.cpu().numpy()) and np.array_equal(expected[:, 4:7], maximum.cpu().numpy())
    for out in (other_rows, None):
        with torch.cuda.stream(stream):
            boxes.fill_(-7777.25)
        fused(out)
        stream.synchronize()
        ok = ok and np.array_equal(boxes.cpu().numpy(), expected)
        if out is not None:
            ok = ok and np.array_equal(other_rows.cpu().numpy().view(np.uint32), host_rows.view(np.uint32))
    if "parent" in contexts:
        with torch.cuda.stream(stream):
            other_rows.zero_()
        rows_launch("parent", other_rows)
        stream.synchronize()
        ok = ok and np.array_equal(other_rows.cpu().numpy().view(np.uint32), host_rows.view(np.uint32))
    refused = sum(c.rejected_instance_count() for c in contexts.values())
    if not ok or refused != 0:
        print(f"MISMATCH in batch {name!r} (refused instances: {refused})", flush=True)
        return None

    cases = {"a_rows": rows_launch, "b_rows_torch": rows_then_torch, "c_rows_bounds": lambda: fused(other_rows), "d_bounds": lambda: fused(None)}
    if "parent" in contexts:
        cases["e_parent_rows"] = lambda: rows_launch("parent", other_rows)
    for launch in cases.values():          # warm-up: every shape of the timed window
        timed(stream, launch, 3)
    samples = {key: [] for key in cases}
    for _ in range(ROUNDS):
        for key, launch in cases.items():
            samples[key].append(timed(stream, launch, REPEATS))
    result = {"batch": name, "instances": N, "bones": bones, "rounds": ROUNDS, "repeats": REPEATS, "checked": True, "us": {}}
    for key, values in samples.items():
        values = np.array(values)
        result["us"][key] = {"median": round(float(np.median(values)), 2), "min": round(float(values.min()), 2), "max": round(float(values.max()), 2),
                             "spread": round(float((values.max() - values.min()) / np.median(values)), 4)}
    for c in contexts.values():
        c.close()
    return result


def main():
    if not torch.cuda.is_available():
        raise SystemExit("tools/pose_bounds.py needs a GPU: nothing is measured without one")
    parent_path = os.environ.get("BOUNDS_PARENT_LIBRARY")
    failed = False
    for name, spec in BATCHES.items():
        result = measure(name, spec, parent_path)
        failed = failed or result is None
        if result is not None:
            print(json.dumps(result), flush=True)
    sys.exit(1 if failed else 0)


if __name__ == "__main__":
    main()
