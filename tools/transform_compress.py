#!/usr/bin/env python3
"""Measurement aid: aclhip_compress_raw_tracks_batch, HIP events on one stream. One batch: TRANSFORM_COMPRESS_INSTANCES instances over
TRANSFORM_COMPRESS_ARRAYS distinct raw track arrays of the bench's pose shape (100 tracks x 301 samples at 30 Hz; a context holds at
most 4 095 live arrays, so handles repeat): a third of the sub-tracks constant, a few default, the rest animated, as a cleaned mocap
take has them.
Before anything is timed every distinct array's blob is CHECKED byte for byte against the reference's compress_track_list with the raw
compression settings where its library is built (else against the restatement of tests/transform_compress_restatement.py; the line
says which). A mismatch, a refused instance or a status that is not ok exits non-zero.
Time is reported, never judged: the median of TRANSFORM_COMPRESS_ROUNDS interleaved rounds of TRANSFORM_COMPRESS_REPEATS launches each
and the spread (max - min) / median, next to the reference's compressor over the same instances on this box's CPUs, single thread and
TRANSFORM_COMPRESS_THREADS threads (its calls release the interpreter lock), in the same rounds; the single thread pass may take the
first TRANSFORM_COMPRESS_SINGLE_THREAD_INSTANCES instances only, its time scaled to the batch (the line says how many it took).
With ACLHIP_LIBRARY pointing at libaclhip_lab.so the line also carries the per-phase split: ACLHIP_TRANSFORM_COMPRESS_PHASES=k stops the
call behind its k-th launch (analysis, layout, stream, hash), and a phase's time is the difference of two medians measured in the same
rounds. Prints one JSON line."""
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
import transform_compress_restatement as restatement  # noqa: E402  (the checker's restatement)

N = int(os.environ.get("TRANSFORM_COMPRESS_INSTANCES", "4096"))
ARRAYS = int(os.environ.get("TRANSFORM_COMPRESS_ARRAYS", "256"))
TRACKS = int(os.environ.get("TRANSFORM_COMPRESS_TRACKS", "100"))
SAMPLES = int(os.environ.get("TRANSFORM_COMPRESS_SAMPLES", "301"))
ROUNDS = int(os.environ.get("TRANSFORM_COMPRESS_ROUNDS", "3"))
REPEATS = int(os.environ.get("TRANSFORM_COMPRESS_REPEATS", "20"))
THREADS = int(os.environ.get("TRANSFORM_COMPRESS_THREADS", "16"))
SINGLE_THREAD_INSTANCES = int(os.environ.get("TRANSFORM_COMPRESS_SINGLE_THREAD_INSTANCES", str(N)))     # the single thread pass takes the first so many, scaled to N
RATE = 30.0
PHASES = ("analysis", "layout", "stream", "hash")
RAW_FORMATS = {"rotation_format": "quatf_full", "translation_format": "vector3f_full", "scale_format": "vector3f_full"}


def timed(stream, launch, repeats):
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record(stream)
    for _ in range(repeats):
        launch()
    stop.record(stream)
    stop.synchronize()
    return start.elapsed_time(stop) * 1000.0 / repeats


def make_array(rng):
    """every rotation animated but a tenth, two thirds of the translations constant (bone lengths), scales the default but for a tenth"""
    samples = np.zeros((SAMPLES, TRACKS, 12), dtype=np.float32)
    samples[:, :, 0:4] = restatement.unit_quaternions(rng, (SAMPLES, TRACKS))
    samples[:, :, 4:7] = rng.uniform(-1.0, 1.0, size=(SAMPLES, TRACKS, 3))
    samples[:, :, 8:11] = 1.0
    constant_rotation = rng.uniform(size=TRACKS) < 0.1
    samples[:, constant_rotation, 0:4] = samples[:1, constant_rotation, 0:4]
    constant_translation = rng.uniform(size=TRACKS) < 0.66
    samples[:, constant_translation, 4:7] = samples[:1, constant_translation, 4:7]
    scaled = rng.uniform(size=TRACKS) < 0.1
    samples[:, scaled, 8:11] = rng.uniform(0.8, 1.2, size=(SAMPLES, int(scaled.sum()), 3))
    return samples


def main():
    if not torch.cuda.is_available():
        raise SystemExit("tools/transform_compress.py needs a GPU: nothing is measured without one")
    rng = np.random.default_rng(9100 + TRACKS)
    arrays = [make_array(rng) for _ in range(ARRAYS)]
    order = rng.integers(0, ARRAYS, size=N)
    order[:ARRAYS] = np.arange(ARRAYS)[: min(ARRAYS, N)]        # every distinct array is in the batch
    have_reference = os.path.exists(ob.REF_COMPRESS_PATH)
    identity = np.tile(restatement.IDENTITY, (TRACKS, 1))
    roots = np.full(TRACKS, -1, dtype=np.int32)
    compress_on_cpu = (lambda a: ob.ref_compress_ex(a, RATE, parents=roots, bind_pose=identity, **RAW_FORMATS)) if have_reference \
        else (lambda a: restatement.compress(a, RATE))
    expected = [np.asarray(compress_on_cpu(a)).view(np.uint8) for a in arrays]

    stream = torch.cuda.Stream()
    s = stream.cuda_stream
    ctx = runtime.Context(0)
    handles = np.array([ctx.register_raw_tracks(a, RATE) for a in arrays], dtype=np.uint32)
    stride = runtime.transform_compress_bound(TRACKS, SAMPLES, 0)
    with torch.cuda.stream(stream):
        d_raws = torch.from_numpy(handles[order].view(np.int32)).cuda()
        d_blobs = torch.zeros((N, stride), dtype=torch.uint8, device="cuda")
        d_results = torch.zeros((N, 2), dtype=torch.int32, device="cuda")
        d_workspace = torch.zeros(runtime.transform_compress_workspace_bytes(N, TRACKS), dtype=torch.uint8, device="cuda")
    desc = runtime.TransformCompressDesc()
    desc.precision, desc.shell_distance, desc.max_tracks, desc.workspace = 1.0e-4, 1.0, TRACKS, d_workspace.data_ptr()

    def launch():
        ctx.compress_raw_tracks_batch(d_raws.data_ptr(), N, desc, d_blobs.data_ptr(), stride, d_results.data_ptr(), stream=s)

    # ---- checked before it is timed
    os.environ.pop("ACLHIP_TRANSFORM_COMPRESS_PHASES", None)
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
    parsed = [restatement.parse(blob) for blob in expected]
    blob_bytes = int(results[:, 1].astype(np.int64).sum())

    lab = "lab" in os.path.basename(runtime.library_path())
    cases = {"compress": None}
    if lab:
        for k in range(1, 4):
            cases["phases_%d" % k] = str(k)

    def run(knob, repeats):
        if knob is None:
            os.environ.pop("ACLHIP_TRANSFORM_COMPRESS_PHASES", None)
        else:
            os.environ["ACLHIP_TRANSFORM_COMPRESS_PHASES"] = knob
        return timed(stream, launch, repeats)

    def cpu_pass(threads):
        begin = time.perf_counter()
        if threads == 1:
            taken = order[: max(1, min(SINGLE_THREAD_INSTANCES, N))]
            for k in taken:
                compress_on_cpu(arrays[k])
            return (time.perf_counter() - begin) * 1.0e6 * N / len(taken)
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
    os.environ.pop("ACLHIP_TRANSFORM_COMPRESS_PHASES", None)

    def summary(values):
        values = np.array(values)
        return {"median": round(float(np.median(values)), 2), "min": round(float(values.min()), 2), "max": round(float(values.max()), 2),
                "spread": round(float((values.max() - values.min()) / np.median(values)), 4)}

    result = {"instances": N, "distinct_arrays": ARRAYS, "tracks": TRACKS, "samples": SAMPLES, "rounds": ROUNDS, "repeats": REPEATS,
              "checked_against": "reference compressor" if have_reference else "restatement", "library": os.path.basename(runtime.library_path()),
              "raw_bytes": int(N * TRACKS * SAMPLES * 48), "blob_bytes": blob_bytes, "row_stride": stride,
              "animated_sub_tracks": [int(sum(p["num_animated"][kind] for p in parsed)) for kind in range(3)],
              "constant_sub_tracks": [int(sum(p["num_constant"][kind] for p in parsed)) for kind in range(3)],
              "us": {key: summary(values) for key, values in samples.items()}}
    result["gb_per_s"] = round((result["raw_bytes"] + blob_bytes) / result["us"]["compress"]["median"] / 1000.0, 1)
    if have_reference:
        result["cpu_us"] = {key: summary(values) for key, values in cpu.items()}
        result["cpu_us"]["cpu_1_thread"]["instances_taken"] = max(1, min(SINGLE_THREAD_INSTANCES, N))
        for key in cpu:
            result["cpu_us"][key]["over_gpu"] = round(result["cpu_us"][key]["median"] / result["us"]["compress"]["median"], 1)
    if lab:
        total = result["us"]["compress"]["median"]
        upto = [result["us"]["phases_%d" % k]["median"] for k in range(1, 4)] + [total]
        split = [upto[0]] + [upto[k] - upto[k - 1] for k in range(1, 4)]
        result["phase_us"] = {name: round(value, 2) for name, value in zip(PHASES, split)}
        result["phase_share"] = {name: round(value / total, 3) for name, value in zip(PHASES, split)}
    ctx.close()
    print(json.dumps(result), flush=True)


if __name__ == "__main__":
    main()
