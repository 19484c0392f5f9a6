#!/usr/bin/env python3
"""Measurement aid: sampling raw track arrays (aclhip_sample_raw_tracks_batch), HIP events on one stream. One batch: 65 536 instances of
ONE raw track array of 100 tracks x 301 samples (RAW_TRACKS_TRACKS=300 for the rig shape) at uniformly drawn times, rows of 48 bytes per
track:
  sample_raw_tracks          two 16 byte loads per quad from the array's two key frames, one 16 byte store
The yardstick is measured in the same process into the same output buffer, interleaved with the case:
  yardstick_decode_tracks    aclhip_decompress_tracks_batch of a COMPRESSED clip of the same shape (synthetic, variable bit rates) at the
                             same times: what fills such rows everywhere else in the library
Before anything is timed the case is CHECKED bit for bit on a sample of instances (RAW_TRACKS_SAMPLE, spread over the batch) against the
restatement of tests/test_raw_tracks_oracle.py (numpy float32 operations in the header's order). A mismatch or a refused instance exits
non-zero.
Time is reported, never judged: per case the median of RAW_TRACKS_ROUNDS interleaved rounds of RAW_TRACKS_REPEATS launches each, the
spread (max - min) / median, the ratio to the yardstick's median, and the algorithmic bytes (rows written plus the array's, or the
clip's, bytes once) as a rate and as a fraction of the HBM peak of the specification (8 TB/s). Prints one JSON line.
With ACLHIP_LIBRARY pointing at libaclhip_lab.so, ACLHIP_RAW_SAMPLE_WAVES=K shapes the launch with at most K waves per instance (1: one
wave loops over the whole row); the line says which value was set."""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import torch  # noqa: E402
from acl_amd import runtime, synth  # noqa: E402
from test_raw_tracks_oracle import sample_tracks  # noqa: E402  (the checker's restatement)

N = int(os.environ.get("RAW_TRACKS_INSTANCES", "65536"))
TRACKS = int(os.environ.get("RAW_TRACKS_TRACKS", "100"))
SAMPLES = int(os.environ.get("RAW_TRACKS_SAMPLES", "301"))
ROUNDS = int(os.environ.get("RAW_TRACKS_ROUNDS", "3"))
REPEATS = int(os.environ.get("RAW_TRACKS_REPEATS", "20"))
SAMPLE = int(os.environ.get("RAW_TRACKS_SAMPLE", "48"))
RATE = 30.0
HBM_PEAK_BYTES_PER_SECOND = 8.0e12
CASE, YARDSTICK = "sample_raw_tracks", "yardstick_decode_tracks"


def timed(stream, launch, repeats):
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record(stream)
    for _ in range(repeats):
        launch()
    stop.record(stream)
    stop.synchronize()
    return start.elapsed_time(stop) * 1000.0 / repeats


def random_array(rng):
    """a clip that drifts from key frame to key frame: unit rotations, translations within a few units, scales near 1"""
    clip = np.zeros((SAMPLES, TRACKS, 12), dtype=np.float32)
    rotations = rng.normal(size=(1, TRACKS, 4)) + np.cumsum(rng.normal(scale=0.03, size=(SAMPLES, TRACKS, 4)), axis=0)
    clip[..., 0:4] = rotations / np.linalg.norm(rotations, axis=2, keepdims=True)
    clip[..., 4:7] = rng.uniform(-3.0, 3.0, size=(1, TRACKS, 3)) + np.cumsum(rng.normal(scale=0.01, size=(SAMPLES, TRACKS, 3)), axis=0)
    clip[..., 8:11] = 1.0 + np.cumsum(rng.normal(scale=0.002, size=(SAMPLES, TRACKS, 3)), axis=0)
    return clip


def main():
    if not torch.cuda.is_available():
        raise SystemExit("tools/raw_tracks.py needs a GPU: nothing is measured without one")
    stride = TRACKS * 48
    rng = np.random.default_rng(7800 + TRACKS)
    array = random_array(rng)
    clip = synth.build_clip(seed=78, num_tracks=TRACKS, num_samples=SAMPLES, sample_rate=RATE)
    stream = torch.cuda.Stream()
    s = stream.cuda_stream
    ctx = runtime.Context(0)
    raw = ctx.register_raw_tracks(array, RATE)
    handle = ctx.register_clip(clip.blob)
    info = ctx.raw_tracks_info(raw)
    times = rng.uniform(0.0, info.duration, size=N).astype(np.float32)
    with torch.cuda.stream(stream):
        d_raws = torch.full((N,), raw, dtype=torch.int32, device="cuda")
        d_clips = torch.full((N,), handle, dtype=torch.int32, device="cuda")
        d_times = torch.from_numpy(times).cuda()
        out = torch.zeros((N, TRACKS * 12), dtype=torch.float32, device="cuda")
    sample = np.unique(np.linspace(0, N - 1, min(SAMPLE, N)).astype(np.int64))
    d_sample = torch.from_numpy(sample).cuda()

    cases = {
        CASE: lambda: ctx.sample_raw_tracks_batch(d_raws.data_ptr(), d_times.data_ptr(), N, out.data_ptr(), stride, stream=s),
        YARDSTICK: lambda: ctx.decompress_tracks_batch(d_clips.data_ptr(), d_times.data_ptr(), N, out.data_ptr(), stride, stream=s),
    }
    traffic = {CASE: N * stride + array.nbytes, YARDSTICK: N * stride + int(ctx.clip_info(handle).compressed_size)}

    # ---- checked before it is timed (the clear, the launch and the gather on ONE stream: in order)
    with torch.cuda.stream(stream):
        out.fill_(-5.0)
        cases[CASE]()
        got = out[d_sample].cpu().numpy()
    for index, i in enumerate(sample):
        want = sample_tracks(array, RATE, runtime.LOOP_CLAMP, float(times[i]))
        if not np.array_equal(got[index].view(np.uint32), want.view(np.uint32).reshape(-1)):
            print(f"MISMATCH in {CASE}, instance {i}", flush=True)
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
    result = {"instances": N, "tracks": TRACKS, "samples": SAMPLES, "rounds": ROUNDS, "repeats": REPEATS, "checked_instances": int(sample.size),
              "raw_sample_waves": os.environ.get("ACLHIP_RAW_SAMPLE_WAVES", "default"), "us": {}, "traffic": {}}
    for key, values in samples.items():
        values = np.array(values)
        result["us"][key] = {"median": round(float(np.median(values)), 2), "min": round(float(values.min()), 2), "max": round(float(values.max()), 2),
                             "spread": round(float((values.max() - values.min()) / np.median(values)), 4)}
    for key, bytes_moved in traffic.items():
        rate = bytes_moved / (result["us"][key]["median"] * 1e-6)
        result["traffic"][key] = {"bytes": bytes_moved, "gb_per_second": round(rate / 1e9, 1), "fraction_of_hbm_peak": round(rate / HBM_PEAK_BYTES_PER_SECOND, 3)}
    result["us"][CASE]["over_yardstick"] = round(result["us"][CASE]["median"] / result["us"][YARDSTICK]["median"], 3)
    ctx.close()
    print(json.dumps(result), flush=True)


if __name__ == "__main__":
    main()
