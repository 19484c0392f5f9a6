#!/usr/bin/env python3
"""Measurement aid: aclhip_compress_raw_scalar_tracks_batch, HIP events on one stream. One batch: SCALAR_COMPRESS_INSTANCES instances
over SCALAR_COMPRESS_ARRAYS distinct float1f arrays of the bench's scalar list shape (256 curves x 120 samples at 60 Hz; a context holds
at most 4 095 live arrays, so handles repeat), compressed at a precision at which the rates spread (the line carries the histogram).
Before anything is timed every distinct array's blob is CHECKED byte for byte against the reference's compress_track_list where its
library is built (else against the restatement of tests/scalar_compress_restatement.py; the line says which). A mismatch, a refused
instance or a status that is not ok exits non-zero.
Time is reported, never judged: the median of SCALAR_COMPRESS_ROUNDS interleaved rounds of SCALAR_COMPRESS_REPEATS launches each and the
spread (max - min) / median, next to the reference's compressor over the same instances on this box's CPUs, single thread and
SCALAR_COMPRESS_THREADS threads (its calls release the interpreter lock), in the same rounds.
With ACLHIP_LIBRARY pointing at libaclhip_lab.so the line also carries the per-phase split: ACLHIP_SCALAR_COMPRESS_PHASES=k stops the
call behind its k-th launch (vote, analysis, layout, bit stream, hash), and a phase's time is the difference of two medians measured in
the same rounds -- the share of the hash among them. Prints one JSON line."""
import json
import os
import sys
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import torch  # noqa: E402
from acl_amd import runtime  # noqa: E402
from oracle import bindings as ob  # noqa: E402
import scalar_compress_restatement as restatement  # noqa: E402  (the checker's restatement)

N = int(os.environ.get("SCALAR_COMPRESS_INSTANCES", "4096"))
ARRAYS = int(os.environ.get("SCALAR_COMPRESS_ARRAYS", "256"))
TRACKS = int(os.environ.get("SCALAR_COMPRESS_TRACKS", "256"))
SAMPLES = int(os.environ.get("SCALAR_COMPRESS_SAMPLES", "120"))
PRECISION = float(os.environ.get("SCALAR_COMPRESS_PRECISION", "1e-4"))
ROUNDS = int(os.environ.get("SCALAR_COMPRESS_ROUNDS", "3"))
REPEATS = int(os.environ.get("SCALAR_COMPRESS_REPEATS", "20"))
THREADS = int(os.environ.get("SCALAR_COMPRESS_THREADS", "16"))
TRACK_TYPE, RATE = 0, 60.0
PHASES = ("vote", "analysis", "layout", "bit_stream", "hash")


def timed(stream, launch, repeats):
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record(stream)
    for _ in range(repeats):
        launch()
    stop.record(stream)
    stop.synchronize()
    return start.elapsed_time(stop) * 1000.0 / repeats


def make_array(rng):
    """curves that drift from key frame to key frame, as blend shape weights do, with amplitudes over five decades: the rates spread"""
    scale = 10.0 ** rng.uniform(-4.0, 1.0, size=(1, TRACKS, 1))
    return (rng.uniform(0.0, 1.0, size=(1, TRACKS, 1)) + scale * np.cumsum(rng.normal(scale=0.05, size=(SAMPLES, TRACKS, 1)), axis=0)).astype(np.float32)


def main():
    if not torch.cuda.is_available():
        raise SystemExit("tools/scalar_compress.py needs a GPU: nothing is measured without one")
    rng = np.random.default_rng(8300 + TRACKS)
    arrays = [make_array(rng) for _ in range(ARRAYS)]
    order = rng.integers(0, ARRAYS, size=N)
    order[:ARRAYS] = np.arange(ARRAYS)[: min(ARRAYS, N)]        # every distinct array is in the batch
    have_reference = ob.have_ref_scalar()
    compress_on_cpu = (lambda a: ob.ref_scalar_compress(a, TRACK_TYPE, RATE, precision=PRECISION)) if have_reference \
        else (lambda a: restatement.compress(a, TRACK_TYPE, RATE, precision=PRECISION))
    expected = [np.asarray(compress_on_cpu(a)).view(np.uint8) for a in arrays]

    stream = torch.cuda.Stream()
    s = stream.cuda_stream
    ctx = runtime.Context(0)
    handles = np.array([ctx.register_raw_scalar_tracks(a, TRACK_TYPE, RATE) for a in arrays], dtype=np.uint32)
    stride = runtime.scalar_compress_bound(TRACK_TYPE, TRACKS, SAMPLES)
    with torch.cuda.stream(stream):
        d_raws = torch.from_numpy(handles[order].view(np.int32)).cuda()
        d_blobs = torch.zeros((N, stride), dtype=torch.uint8, device="cuda")
        d_results = torch.zeros((N, 2), dtype=torch.int32, device="cuda")
        d_workspace = torch.zeros(runtime.scalar_compress_workspace_bytes(N, TRACKS), dtype=torch.uint8, device="cuda")
    desc = runtime.ScalarCompressDesc()
    desc.precision, desc.max_tracks, desc.workspace = PRECISION, TRACKS, d_workspace.data_ptr()

    def launch():
        ctx.compress_raw_scalar_tracks_batch(d_raws.data_ptr(), N, desc, d_blobs.data_ptr(), stride, d_results.data_ptr(), stream=s)

    # ---- checked before it is timed
    os.environ.pop("ACLHIP_SCALAR_COMPRESS_PHASES", None)
    with torch.cuda.stream(stream):
        launch()
        results = d_results.cpu().numpy().view(np.uint32)
        first = d_blobs[:ARRAYS].cpu().numpy()
    if ctx.rejected_instance_count() != 0 or np.any(results[:, 0] != runtime.COMPRESS_OK):
        print(f"refused or failed instances: {ctx.rejected_instance_count()}, statuses {np.unique(results[:, 0])}", flush=True)
        sys.exit(1)
    for i in range(min(ARRAYS, N)):
        if results[i, 1] != expected[i].size or not np.array_equal(first[i, : expected[i].size], expected[i]):
            print(f"MISMATCH in the blob of array {i}", flush=True)
            sys.exit(1)
    rates = np.concatenate([restatement.parse(blob)["rates"] for blob in expected])
    blob_bytes = int(results[:, 1].astype(np.int64).sum())

    lab = "lab" in os.path.basename(runtime.library_path())
    cases = {"compress": None}
    if lab:
        for k in range(1, 5):
            cases["phases_%d" % k] = str(k)

    def run(knob, repeats):
        if knob is None:
            os.environ.pop("ACLHIP_SCALAR_COMPRESS_PHASES", None)
        else:
            os.environ["ACLHIP_SCALAR_COMPRESS_PHASES"] = knob
        return timed(stream, launch, repeats)

    def cpu_pass(threads):
        begin = time.perf_counter()
        if threads == 1:
            for k in order:
                compress_on_cpu(arrays[k])
        else:
            with ThreadPoolExecutor(max_workers=threads) as pool:
                list(pool.map(lambda k: compress_on_cpu(arrays[k]), order, chunksize=16))
        return (time.perf_counter() - begin) * 1.0e6

    for knob in cases.values():
        run(knob, 3)
    samples = {key: [] for key in cases}
    cpu = {"cpu_1_thread": [], "cpu_%d_threads" % THREADS: []}
    for _ in range(ROUNDS):
        for key, knob in cases.items():
            samples[key].append(run(knob, REPEATS))
        if have_reference:
            cpu["cpu_1_thread"].append(cpu_pass(1))
            cpu["cpu_%d_threads" % THREADS].append(cpu_pass(THREADS))
    os.environ.pop("ACLHIP_SCALAR_COMPRESS_PHASES", None)

    def summary(values):
        values = np.array(values)
        return {"median": round(float(np.median(values)), 2), "min": round(float(values.min()), 2), "max": round(float(values.max()), 2),
                "spread": round(float((values.max() - values.min()) / np.median(values)), 4)}

    result = {"instances": N, "distinct_arrays": ARRAYS, "tracks": TRACKS, "samples": SAMPLES, "precision": PRECISION, "rounds": ROUNDS, "repeats": REPEATS,
              "checked_against": "reference compressor" if have_reference else "restatement", "library": os.path.basename(runtime.library_path()),
              "raw_bytes": int(N * TRACKS * SAMPLES * 4), "blob_bytes": blob_bytes, "row_stride": stride,
              "rate_histogram": {str(rate): int(count) for rate, count in zip(*np.unique(rates, return_counts=True))},
              "us": {key: summary(values) for key, values in samples.items()}}
    if have_reference:
        result["cpu_us"] = {key: summary(values) for key, values in cpu.items()}
        for key in cpu:
            result["cpu_us"][key]["over_gpu"] = round(result["cpu_us"][key]["median"] / result["us"]["compress"]["median"], 1)
    if lab:
        total = result["us"]["compress"]["median"]
        upto = [result["us"]["phases_%d" % k]["median"] for k in range(1, 5)] + [total]
        split = [upto[0]] + [upto[k] - upto[k - 1] for k in range(1, 5)]
        result["phase_us"] = {name: round(value, 2) for name, value in zip(PHASES, split)}
        result["phase_share"] = {name: round(value / total, 3) for name, value in zip(PHASES, split)}
    ctx.close()
    print(json.dumps(result), flush=True)


if __name__ == "__main__":
    main()
