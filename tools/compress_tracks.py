#!/usr/bin/env python3
"""Measurement aid: aclhip_compress_tracks_batch with quatf_drop_w_full, HIP events on one stream, on the workload of
tools/transform_compress.py: COMPRESS_TRACKS_INSTANCES instances over COMPRESS_TRACKS_ARRAYS distinct raw track arrays of the bench's pose
shape (100 tracks x 301 samples at 30 Hz) with a chain-and-branches parent table of as many bones: a spine, and limbs of seven bones
hanging off it. A tenth of the rotations are fixed and another tenth jitter by 1e-6 about a fixed rotation (locked joints of a mocap
take): the error metric makes them constant where the binary test of the raw formats keeps them animated.
Before anything is timed the blobs are CHECKED: the first COMPRESS_TRACKS_RESTATED distinct arrays byte for byte against the restatement
of tests/lossy_rotation_compress_restatement.py, and every distinct array against the reference's compress_track_list with the same
settings where its library is built -- every byte outside the rotation value words and the hash, the rotation value words within 1e-5.
A mismatch, a refused instance or a status that is not ok exits non-zero.
Time is reported, never judged: the median of COMPRESS_TRACKS_ROUNDS interleaved rounds of COMPRESS_TRACKS_REPEATS launches each and the
spread (max - min) / median; in the same rounds aclhip_compress_raw_tracks_batch on the same arrays, and the reference's compressor with
the same settings over the same instances on COMPRESS_TRACKS_THREADS threads of this box's CPUs (its calls release the interpreter lock).
With ACLHIP_LIBRARY pointing at libaclhip_lab.so the line also carries the per-phase split: ACLHIP_TRACKS_COMPRESS_PHASES=k stops the
call behind its k-th launch (shell, analysis, layout, stream, hash), and a phase's time is the difference of two medians measured in
the same rounds. Prints one JSON line."""
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
import lossy_rotation_compress_restatement as restatement  # noqa: E402  (the checker's restatement)

N = int(os.environ.get("COMPRESS_TRACKS_INSTANCES", "4096"))
ARRAYS = int(os.environ.get("COMPRESS_TRACKS_ARRAYS", "256"))
TRACKS = int(os.environ.get("COMPRESS_TRACKS_TRACKS", "100"))
SAMPLES = int(os.environ.get("COMPRESS_TRACKS_SAMPLES", "301"))
ROUNDS = int(os.environ.get("COMPRESS_TRACKS_ROUNDS", "3"))
REPEATS = int(os.environ.get("COMPRESS_TRACKS_REPEATS", "20"))
THREADS = int(os.environ.get("COMPRESS_TRACKS_THREADS", "16"))
RESTATED = int(os.environ.get("COMPRESS_TRACKS_RESTATED", "4"))
RATE = 30.0
PRECISION, SHELL = 0.01, 3.0
PHASES = ("shell", "analysis", "layout", "stream", "hash")
KNOB = "ACLHIP_TRACKS_COMPRESS_PHASES"
FORMATS = {"rotation_format": "quatf_drop_w_full", "translation_format": "vector3f_full", "scale_format": "vector3f_full"}


def timed(stream, launch, repeats):
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record(stream)
    for _ in range(repeats):
        launch()
    stop.record(stream)
    stop.synchronize()
    return start.elapsed_time(stop) * 1000.0 / repeats


def skeleton(num_tracks):
    """a spine of a fifth of the bones; the rest in limbs of seven, each hanging off a spine bone"""
    spine = max(1, num_tracks // 5)
    parents = [restatement.NO_PARENT] + list(range(spine - 1))
    while len(parents) < num_tracks:
        at = len(parents)
        parents.append((at * 7) % spine if (at - spine) % 7 == 0 else at - 1)
    return np.array(parents, dtype=np.int64).astype(np.uint32)


def make_array(rng):
    """tools/transform_compress.py's array with short bones (|t| < 0.2, so that the shells stay within a few units); of the rotations a
    tenth fixed and a tenth jittering by 1e-6"""
    samples = np.zeros((SAMPLES, TRACKS, 12), dtype=np.float32)
    samples[:, :, 0:4] = restatement.raw_restatement.unit_quaternions(rng, (SAMPLES, TRACKS))
    samples[:, :, 4:7] = rng.uniform(-0.2, 0.2, size=(SAMPLES, TRACKS, 3))
    samples[:, :, 8:11] = 1.0
    how = rng.uniform(size=TRACKS)
    fixed = how < 0.1
    samples[:, fixed, 0:4] = samples[:1, fixed, 0:4]
    for track in np.flatnonzero((how >= 0.1) & (how < 0.2)):
        jitter = samples[0, track, 0:4].astype(np.float64) + rng.standard_normal((SAMPLES, 4)) * 1.0e-6
        samples[:, track, 0:4] = (jitter / np.linalg.norm(jitter, axis=-1, keepdims=True)).astype(np.float32)
    constant_translation = rng.uniform(size=TRACKS) < 0.66
    samples[:, constant_translation, 4:7] = samples[:1, constant_translation, 4:7]
    scaled = rng.uniform(size=TRACKS) < 0.1
    samples[:, scaled, 8:11] = rng.uniform(0.8, 1.2, size=(SAMPLES, int(scaled.sum()), 3))
    return samples


def main():
    if not torch.cuda.is_available():
        raise SystemExit("tools/compress_tracks.py needs a GPU: nothing is measured without one")
    rng = np.random.default_rng(9100 + TRACKS)
    arrays = [make_array(rng) for _ in range(ARRAYS)]
    order = rng.integers(0, ARRAYS, size=N)
    order[:ARRAYS] = np.arange(ARRAYS)[: min(ARRAYS, N)]        # every distinct array is in the batch
    parents = skeleton(TRACKS)
    have_reference = os.path.exists(ob.REF_COMPRESS_PATH)
    identity = np.tile(restatement.IDENTITY, (TRACKS, 1))

    def compress_on_cpu(a):
        return ob.ref_compress_ex(a, RATE, parents=parents.view(np.int32), bind_pose=identity, precision=PRECISION, shell_distance=SHELL, **FORMATS)

    stream = torch.cuda.Stream()
    s = stream.cuda_stream
    ctx = runtime.Context(0)
    handles = np.array([ctx.register_raw_tracks(a, RATE) for a in arrays], dtype=np.uint32)
    stride = runtime.transform_compress_bound(TRACKS, SAMPLES, 0)
    with torch.cuda.stream(stream):
        d_raws = torch.from_numpy(handles[order].view(np.int32)).cuda()
        d_parents = torch.from_numpy(parents.view(np.int32)).cuda()
        d_blobs = torch.zeros((N, stride), dtype=torch.uint8, device="cuda")
        d_results = torch.zeros((N, 2), dtype=torch.int32, device="cuda")
        d_workspace = torch.zeros(runtime.compress_tracks_workspace_bytes(N, TRACKS), dtype=torch.uint8, device="cuda")
    desc = runtime.CompressTracksDesc()
    desc.rotation_format, desc.precision, desc.shell_distance, desc.max_tracks, desc.workspace = runtime.ROTATION_QUATF_DROP_W_FULL, PRECISION, SHELL, TRACKS, d_workspace.data_ptr()
    desc.parent_indices, desc.num_table_tracks = d_parents.data_ptr(), TRACKS
    raw_desc = runtime.TransformCompressDesc()
    raw_desc.precision, raw_desc.shell_distance, raw_desc.max_tracks, raw_desc.workspace = PRECISION, SHELL, TRACKS, d_workspace.data_ptr()

    def launch():
        ctx.compress_tracks_batch(d_raws.data_ptr(), N, desc, d_blobs.data_ptr(), stride, d_results.data_ptr(), stream=s)

    def launch_raw():
        ctx.compress_raw_tracks_batch(d_raws.data_ptr(), N, raw_desc, d_blobs.data_ptr(), stride, d_results.data_ptr(), stream=s)

    # ---- checked before it is timed
    os.environ.pop(KNOB, None)
    with torch.cuda.stream(stream):
        launch_raw()
        raw_blob_bytes = int(d_results.cpu().numpy().view(np.uint32)[:, 1].astype(np.int64).sum())
        launch()
        results = d_results.cpu().numpy().view(np.uint32)
        first = d_blobs[:ARRAYS].cpu().numpy()
    if ctx.rejected_instance_count() != 0 or np.any(results[:, 0] != runtime.COMPRESS_OK):
        print(f"refused or failed instances: {ctx.rejected_instance_count()}, statuses {np.unique(results[:, 0])}", flush=True)
        sys.exit(1)
    for i in range(min(ARRAYS, N, RESTATED)):
        expected = restatement.compress(arrays[i], RATE, parents=parents, precision=PRECISION, shell_distance=SHELL).blob
        if results[i, 1] != expected.size or not np.array_equal(first[i, : expected.size], expected):
            print(f"MISMATCH with the restatement in the blob of array {i}", flush=True)
            sys.exit(1)
    worst = 0.0
    if have_reference:
        for i in range(min(ARRAYS, N)):
            theirs = np.asarray(compress_on_cpu(arrays[i])).view(np.uint8)
            ours = first[i, : results[i, 1]]
            mask = restatement.rotation_bytes_of(theirs) if ours.size == theirs.size else None
            if mask is not None:
                mask[4:8] = True
            if mask is None or not np.array_equal(ours[~mask], theirs[~mask]):
                print(f"MISMATCH with the reference in the blob of array {i}", flush=True)
                sys.exit(1)
            mask[4:8] = False
            worst = max(worst, float(np.abs(restatement.rotation_values(ours, mask) - restatement.rotation_values(theirs, mask)).max()))
        if worst > 1.0e-5:
            print(f"rotation value words {worst} from the reference's", flush=True)
            sys.exit(1)
    parsed = [restatement.raw_restatement.parse(first[i, : results[i, 1]]) for i in range(min(ARRAYS, N))]
    blob_bytes = int(results[:, 1].astype(np.int64).sum())

    lab = "lab" in os.path.basename(runtime.library_path())
    cases = {"compress": (launch, None), "raw_call": (launch_raw, None)}
    if lab:
        for k in range(1, 5):
            cases["phases_%d" % k] = (launch, str(k))

    def run(case, repeats):
        call, knob = case
        if knob is None:
            os.environ.pop(KNOB, None)
        else:
            os.environ[KNOB] = knob
        return timed(stream, call, repeats)

    def cpu_pass(threads):
        begin = time.perf_counter()
        with ThreadPoolExecutor(max_workers=threads) as pool:
            list(pool.map(lambda k: compress_on_cpu(arrays[k]), order, chunksize=16))
        return (time.perf_counter() - begin) * 1.0e6

    for case in cases.values():
        run(case, 3)
    samples = {key: [] for key in cases}
    cpu = {"cpu_%d_threads" % THREADS: []}
    for _ in range(ROUNDS):
        for key, case in cases.items():
            samples[key].append(run(case, REPEATS))
        if have_reference:
            cpu["cpu_%d_threads" % THREADS].append(cpu_pass(THREADS))
    os.environ.pop(KNOB, None)

    def summary(values):
        values = np.array(values)
        return {"median": round(float(np.median(values)), 2), "min": round(float(values.min()), 2), "max": round(float(values.max()), 2),
                "spread": round(float((values.max() - values.min()) / np.median(values)), 4)}

    result = {"instances": N, "distinct_arrays": ARRAYS, "tracks": TRACKS, "samples": SAMPLES, "rounds": ROUNDS, "repeats": REPEATS,
              "checked_against": ("reference compressor and " if have_reference else "") + "restatement (%d arrays)" % min(ARRAYS, N, RESTATED),
              "worst_rotation_word_difference": worst, "library": os.path.basename(runtime.library_path()),
              "raw_bytes": int(N * TRACKS * SAMPLES * 48), "blob_bytes": blob_bytes, "raw_call_blob_bytes": raw_blob_bytes, "row_stride": stride,
              "animated_sub_tracks": [int(sum(p["num_animated"][kind] for p in parsed)) for kind in range(3)],
              "constant_sub_tracks": [int(sum(p["num_constant"][kind] for p in parsed)) for kind in range(3)],
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
