#!/usr/bin/env python3
"""Measurement aid: sampling raw scalar track arrays (aclhip_sample_raw_scalar_tracks_batch and aclhip_sample_raw_scalar_track_batch), HIP
events on one stream. One batch: 65 536 instances of ONE raw scalar track array of the bench's scalar list shape (256 float1f curves x 120
samples at 60 Hz) at uniformly drawn times:
  sample_tracks_stride16     rows of 1 024 bytes: base and stride 16 byte aligned
  sample_tracks_stride4      rows of 1 028 bytes: every row but each fourth starts off a 16 byte boundary
  sample_track               one request per instance, a uniformly drawn track, 4 bytes per request
The yardsticks are measured in the same process into the same output buffer at the same times, interleaved with the cases:
  yardstick_decode_tracks_stride16 / _stride4     aclhip_decompress_scalar_tracks_batch of the COMPRESSED clip of the same array (the
                             reference's compressor at precision 1e-4 where its library is built, else a synthetic clip of the same shape;
                             the line says which)
  yardstick_decode_track     aclhip_decompress_scalar_track_batch of that clip, the same requests
Before anything is timed every case is CHECKED bit for bit on a sample of instances (RAW_SCALAR_SAMPLE, spread over the batch) against
the restatement of tests/test_raw_scalar_tracks_oracle.py. A mismatch or a refused instance exits non-zero.
Time is reported, never judged: per case the median of RAW_SCALAR_ROUNDS interleaved rounds of RAW_SCALAR_REPEATS launches each, the
spread (max - min) / median, the ratio to its yardstick's median, and the algorithmic bytes (values written plus the array's, or the
clip's, bytes once) as a rate and as a fraction of the HBM peak of the specification (8 TB/s). Prints one JSON line.
With ACLHIP_LIBRARY pointing at libaclhip_lab.so, ACLHIP_RAW_SCALAR_DWORD=1 keeps every row on the dword path (what the 16 byte path of
aligned rows buys); the line says which value was set."""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import torch  # noqa: E402
from acl_amd import runtime, synth  # noqa: E402
from oracle import bindings as ob  # noqa: E402
from test_raw_scalar_tracks_oracle import sample_tracks  # noqa: E402  (the checker's restatement)

N = int(os.environ.get("RAW_SCALAR_INSTANCES", "65536"))
TRACK_TYPE = int(os.environ.get("RAW_SCALAR_TRACK_TYPE", "0"))
TRACKS = int(os.environ.get("RAW_SCALAR_TRACKS", "256"))
SAMPLES = int(os.environ.get("RAW_SCALAR_SAMPLES", "120"))
ROUNDS = int(os.environ.get("RAW_SCALAR_ROUNDS", "3"))
REPEATS = int(os.environ.get("RAW_SCALAR_REPEATS", "20"))
SAMPLE = int(os.environ.get("RAW_SCALAR_SAMPLE", "48"))
RATE = 60.0
HBM_PEAK_BYTES_PER_SECOND = 8.0e12


def timed(stream, launch, repeats):
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record(stream)
    for _ in range(repeats):
        launch()
    stop.record(stream)
    stop.synchronize()
    return start.elapsed_time(stop) * 1000.0 / repeats


def main():
    if not torch.cuda.is_available():
        raise SystemExit("tools/raw_scalar_tracks.py needs a GPU: nothing is measured without one")
    components = runtime.SCALAR_TRACK_COMPONENTS[TRACK_TYPE]
    row_bytes = TRACKS * components * 4
    rng = np.random.default_rng(7900 + TRACKS)
    # curves that drift from key frame to key frame, as blend shape weights do
    array = (rng.uniform(0.0, 1.0, size=(1, TRACKS, components)) + np.cumsum(rng.normal(scale=0.01, size=(SAMPLES, TRACKS, components)), axis=0)).astype(np.float32)
    if ob.have_ref_scalar():
        blob, clip_source = ob.ref_scalar_compress(array, TRACK_TYPE, RATE, precision=1.0e-4), "reference compressor, precision 1e-4"
    else:
        blob = synth.build_scalar_clip(seed=79, track_type=TRACK_TYPE, num_tracks=TRACKS, num_samples=SAMPLES, sample_rate=RATE, raw_fraction=0.01).blob
        clip_source = "synthetic clip of the same shape"
    stream = torch.cuda.Stream()
    s = stream.cuda_stream
    ctx = runtime.Context(0)
    raw = ctx.register_raw_scalar_tracks(array, TRACK_TYPE, RATE)
    handle = ctx.register_clip(blob)
    info = ctx.raw_scalar_tracks_info(raw)
    times = rng.uniform(0.0, info.duration, size=N).astype(np.float32)
    tracks = rng.integers(0, TRACKS, size=N).astype(np.int32)
    strides = {"stride16": (row_bytes + 15) // 16 * 16, "stride4": (row_bytes + 15) // 16 * 16 + 4}
    with torch.cuda.stream(stream):
        d_raws = torch.full((N,), raw, dtype=torch.int32, device="cuda")
        d_clips = torch.full((N,), handle, dtype=torch.int32, device="cuda")
        d_times = torch.from_numpy(times).cuda()
        d_tracks = torch.from_numpy(tracks).cuda()
        out = torch.zeros((N * strides["stride4"] // 4,), dtype=torch.float32, device="cuda")
    sample = np.unique(np.linspace(0, N - 1, min(SAMPLE, N)).astype(np.int64))
    params = runtime.default_params()

    cases, traffic, yardstick_of = {}, {}, {}
    clip_bytes = int(ctx.clip_info(handle).compressed_size)
    for name, stride in strides.items():
        cases["sample_tracks_" + name] = lambda stride=stride: ctx.sample_raw_scalar_tracks_batch(d_raws.data_ptr(), d_times.data_ptr(), N, out.data_ptr(), stride, stream=s)
        cases["yardstick_decode_tracks_" + name] = lambda stride=stride: ctx.decompress_scalar_tracks_batch(d_clips.data_ptr(), d_times.data_ptr(), N, out.data_ptr(), stride,
                                                                                                           params=params, stream=s)
        traffic["sample_tracks_" + name], traffic["yardstick_decode_tracks_" + name] = N * row_bytes + array.nbytes, N * row_bytes + clip_bytes
        yardstick_of["sample_tracks_" + name] = "yardstick_decode_tracks_" + name
    request_stride = 4 * components
    cases["sample_track"] = lambda: ctx.sample_raw_scalar_track_batch(d_raws.data_ptr(), d_times.data_ptr(), d_tracks.data_ptr(), N, out.data_ptr(), request_stride, stream=s)
    cases["yardstick_decode_track"] = lambda: ctx.decompress_scalar_track_batch(d_clips.data_ptr(), d_times.data_ptr(), d_tracks.data_ptr(), N, out.data_ptr(), request_stride,
                                                                                params=params, stream=s)
    traffic["sample_track"], traffic["yardstick_decode_track"] = N * request_stride + array.nbytes, N * request_stride + clip_bytes
    yardstick_of["sample_track"] = "yardstick_decode_track"

    # ---- checked before it is timed (the clear, the launch and the copy on ONE stream: in order)
    for name, stride in list(strides.items()) + [("track", request_stride)]:
        key = "sample_track" if name == "track" else "sample_tracks_" + name
        with torch.cuda.stream(stream):
            out.fill_(-5.0)
            cases[key]()
            got = out[: N * stride // 4].reshape(N, stride // 4)[torch.from_numpy(sample).cuda()].cpu().numpy()
        for index, i in enumerate(sample):
            want = sample_tracks(array, RATE, runtime.LOOP_CLAMP, float(times[i]))
            want = want[tracks[i]] if name == "track" else want
            if not np.array_equal(got[index, : want.size].view(np.uint32), want.view(np.uint32).reshape(-1)) or np.any(got[index, want.size:] != -5.0):
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
    result = {"instances": N, "track_type": TRACK_TYPE, "tracks": TRACKS, "samples": SAMPLES, "rounds": ROUNDS, "repeats": REPEATS, "checked_instances": int(sample.size),
              "strides": strides, "yardstick_clip": clip_source, "dword_only": os.environ.get("ACLHIP_RAW_SCALAR_DWORD", "default"), "us": {}, "traffic": {}}
    for key, values in samples.items():
        values = np.array(values)
        result["us"][key] = {"median": round(float(np.median(values)), 2), "min": round(float(values.min()), 2), "max": round(float(values.max()), 2),
                             "spread": round(float((values.max() - values.min()) / np.median(values)), 4)}
    for key, bytes_moved in traffic.items():
        rate = bytes_moved / (result["us"][key]["median"] * 1e-6)
        result["traffic"][key] = {"bytes": bytes_moved, "gb_per_second": round(rate / 1e9, 1), "fraction_of_hbm_peak": round(rate / HBM_PEAK_BYTES_PER_SECOND, 3)}
    for key, yardstick in yardstick_of.items():
        result["us"][key]["over_yardstick"] = round(result["us"][key]["median"] / result["us"][yardstick]["median"], 3)
    ctx.close()
    print(json.dumps(result), flush=True)


if __name__ == "__main__":
    main()
