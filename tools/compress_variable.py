#!/usr/bin/env python3
"""Measurement aid: aclhip_compress_tracks_variable_batch at a uniform bit rate (COMPRESS_VARIABLE_RATE, 16), HIP events on one stream,
on the workload of tools/compress_tracks.py -- its arrays, its parent table, its settings: COMPRESS_TRACKS_INSTANCES instances over
COMPRESS_TRACKS_ARRAYS distinct raw track arrays of 100 tracks x 301 samples.
Before anything is timed the blobs are CHECKED: the first COMPRESS_TRACKS_RESTATED distinct arrays byte for byte against the restatement
of tests/variable_compress_restatement.py, every distinct blob through aclhip_check_clip with its hash. A mismatch, a refused instance
or a status that is not ok exits non-zero.
Time is reported, never judged: the median of COMPRESS_TRACKS_ROUNDS interleaved rounds of COMPRESS_TRACKS_REPEATS launches each and the
spread (max - min) / median; in the same rounds aclhip_compress_tracks_batch (quatf_drop_w_full) on the same arrays, so that the two are
measured side by side. With ACLHIP_LIBRARY pointing at libaclhip_lab.so the line also carries the per-phase split:
ACLHIP_VARIABLE_COMPRESS_PHASES=k stops the call behind its k-th launch (shell, analysis, layout, segment ranges, stream, hash), and a
phase's time is the difference of two medians measured in the same rounds. --metric {0,1}: the aclhip_error_metric of both calls (1:
the _metric entry points with the reference's matrix metric, checked against tests/matrix_metric_compress_restatement.py).
--additive-format {relative,additive0,additive1}: every array is an additive clip on a drawn base clip of its own (another array of the
workload's; under additive1 the clips' scales are moved by -1 and the default scale is 0) and both calls go through the _additive entry
points, checked against tests/additive_compress_restatement.py; the calls without a base are timed in the same rounds (compress_no_base,
drop_w_call_no_base). Prints one JSON line."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import torch  # noqa: E402
from acl_amd import runtime  # noqa: E402
import compress_tracks as workload  # noqa: E402  (the arrays, the skeleton, the timer)
import variable_compress_restatement as restatement  # noqa: E402  (the checker's restatement)
import matrix_metric_compress_restatement as metric_restatement  # noqa: E402  (and with the metric as an argument)
import additive_compress_restatement as additive_restatement  # noqa: E402  (and with an additive base)

N, ARRAYS, TRACKS, SAMPLES = workload.N, workload.ARRAYS, workload.TRACKS, workload.SAMPLES
ROUNDS, REPEATS, RESTATED = workload.ROUNDS, workload.REPEATS, workload.RESTATED
BIT_RATE = int(os.environ.get("COMPRESS_VARIABLE_RATE", "16"))
RATE, PRECISION, SHELL = workload.RATE, workload.PRECISION, workload.SHELL
PHASES = ("shell", "analysis", "layout", "segment_ranges", "stream", "hash")
KNOB = "ACLHIP_VARIABLE_COMPRESS_PHASES"


def main():
    parser = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    parser.add_argument("--metric", type=int, choices=(0, 1), default=0, help="aclhip_error_metric: 0 qvvf (the entry points without a metric), 1 qvvf_matrix3x4f")
    parser.add_argument("--additive-format", choices=("none", "relative", "additive0", "additive1"), default="none",
                        help="compress every array as an additive clip against a drawn base clip, through the _additive entry points")
    arguments = parser.parse_args()
    metric = arguments.metric
    additive_format = {"none": runtime.ADDITIVE_NONE, "relative": runtime.ADDITIVE_RELATIVE, "additive0": runtime.ADDITIVE_ADDITIVE0, "additive1": runtime.ADDITIVE_ADDITIVE1}[arguments.additive_format]
    with_base = additive_format != runtime.ADDITIVE_NONE
    if with_base and metric != runtime.ERROR_METRIC_QVVF:
        parser.error("an additive base goes with the qvvf error metric: the reference has no additive matrix metric")
    if not torch.cuda.is_available():
        raise SystemExit("tools/compress_variable.py needs a GPU: nothing is measured without one")
    rng = np.random.default_rng(9100 + TRACKS)
    arrays = [workload.make_array(rng) for _ in range(ARRAYS)]
    base_arrays, default_pose = [], None
    if with_base:
        base_rng = np.random.default_rng(9300 + TRACKS)
        base_arrays = [workload.make_array(base_rng) for _ in range(ARRAYS)]
        if additive_format == runtime.ADDITIVE_ADDITIVE1:
            default_pose = np.tile(restatement.IDENTITY, (TRACKS, 1)).astype(np.float32)
            default_pose[:, 8:11] = 0.0
            for samples in arrays:
                samples[:, :, 8:11] = samples[:, :, 8:11] - np.float32(1.0)
    order = rng.integers(0, ARRAYS, size=N)
    order[:ARRAYS] = np.arange(ARRAYS)[: min(ARRAYS, N)]        # every distinct array is in the batch
    parents = workload.skeleton(TRACKS)

    stream = torch.cuda.Stream()
    s = stream.cuda_stream
    ctx = runtime.Context(0)
    handles = np.array([ctx.register_raw_tracks(a, RATE) for a in arrays], dtype=np.uint32)
    stride = max(runtime.variable_compress_bound(TRACKS, SAMPLES, 0), runtime.transform_compress_bound(TRACKS, SAMPLES, 0))
    with torch.cuda.stream(stream):
        d_raws = torch.from_numpy(handles[order].view(np.int32)).cuda()
        d_parents = torch.from_numpy(parents.view(np.int32)).cuda()
        d_blobs = torch.zeros((N, stride), dtype=torch.uint8, device="cuda")
        d_results = torch.zeros((N, 2), dtype=torch.int32, device="cuda")
        d_workspace = torch.zeros(runtime.compress_variable_workspace_bytes(N, TRACKS, SAMPLES), dtype=torch.uint8, device="cuda")
        d_pose = torch.from_numpy(default_pose).cuda() if default_pose is not None else None
    base_handles = np.array([ctx.register_raw_tracks(a, RATE) for a in base_arrays], dtype=np.uint32)
    # the entry points of both calls: the runtime's own route
    route = dict(metric=metric, additive_base=base_handles[order] if with_base else None, additive_format=additive_format)
    variable_call, _, _, variable_alive = runtime.transform_compress_route(ctx, "variable", handles[order], **route)
    drop_w_call, _, _, drop_w_alive = runtime.transform_compress_route(ctx, "tracks", handles[order], **route)
    desc = runtime.CompressVariableDesc()
    desc.precision, desc.shell_distance, desc.max_tracks, desc.max_samples, desc.workspace = PRECISION, SHELL, TRACKS, SAMPLES, d_workspace.data_ptr()
    desc.parent_indices, desc.num_table_tracks = d_parents.data_ptr(), TRACKS
    desc.rotation_bit_rate = desc.translation_bit_rate = desc.scale_bit_rate = BIT_RATE
    drop_w = runtime.CompressTracksDesc()
    drop_w.rotation_format, drop_w.precision, drop_w.shell_distance, drop_w.max_tracks, drop_w.workspace = runtime.ROTATION_QUATF_DROP_W_FULL, PRECISION, SHELL, TRACKS, d_workspace.data_ptr()
    drop_w.parent_indices, drop_w.num_table_tracks = d_parents.data_ptr(), TRACKS
    if default_pose is not None:
        desc.default_pose = drop_w.default_pose = d_pose.data_ptr()

    # timed beside under a base, named here on purpose: the entry points without one
    def launch_no_base():
        ctx.compress_tracks_variable_batch(d_raws.data_ptr(), N, desc, d_blobs.data_ptr(), stride, d_results.data_ptr(), stream=s)

    def launch_drop_w_no_base():
        ctx.compress_tracks_batch(d_raws.data_ptr(), N, drop_w, d_blobs.data_ptr(), stride, d_results.data_ptr(), stream=s)

    def launch():
        variable_call(d_raws.data_ptr(), N, desc, d_blobs.data_ptr(), stride, d_results.data_ptr(), stream=s)

    def launch_drop_w():
        drop_w_call(d_raws.data_ptr(), N, drop_w, d_blobs.data_ptr(), stride, d_results.data_ptr(), stream=s)

    # ---- checked before it is timed
    os.environ.pop(KNOB, None)
    with torch.cuda.stream(stream):
        launch_drop_w()
        drop_w_blob_bytes = int(d_results.cpu().numpy().view(np.uint32)[:, 1].astype(np.int64).sum())
        launch()
        results = d_results.cpu().numpy().view(np.uint32)
        first = d_blobs[:ARRAYS].cpu().numpy()
    if ctx.rejected_instance_count() != 0 or np.any(results[:, 0] != runtime.COMPRESS_OK):
        print(f"refused or failed instances: {ctx.rejected_instance_count()}, statuses {np.unique(results[:, 0])}", flush=True)
        sys.exit(1)
    for i in range(min(ARRAYS, N, RESTATED)):
        if with_base:
            expected = additive_restatement.compress_variable(arrays[i], RATE, (BIT_RATE,) * 3, additive_restatement.Base(base_arrays[i], RATE, additive_format), parents=parents,
                                                              precision=PRECISION, shell_distance=SHELL, **({"default_pose": default_pose} if default_pose is not None else {})).blob
        else:
            expected = metric_restatement.compress_variable(arrays[i], RATE, (BIT_RATE,) * 3, metric, parents=parents, precision=PRECISION, shell_distance=SHELL).blob
        if results[i, 1] != expected.size or not np.array_equal(first[i, : expected.size], expected):
            print(f"MISMATCH with the restatement in the blob of array {i}", flush=True)
            sys.exit(1)
    from acl_amd.synth import aligned_bytes
    for i in range(min(ARRAYS, N)):
        blob = aligned_bytes(int(results[i, 1]))
        blob[:] = first[i, : results[i, 1]]
        status, message = runtime.check_clip(blob, check_hash=True)
        if status != 0:
            print(f"aclhip_check_clip refuses the blob of array {i}: {message}", flush=True)
            sys.exit(1)
    blob_bytes = int(results[:, 1].astype(np.int64).sum())

    lab = "lab" in os.path.basename(runtime.library_path())
    cases = {"compress": (launch, None), "drop_w_call": (launch_drop_w, None)}
    if with_base:
        cases.update({"compress_no_base": (launch_no_base, None), "drop_w_call_no_base": (launch_drop_w_no_base, None)})
    if lab:
        for k in range(1, 6):
            cases["phases_%d" % k] = (launch, str(k))

    def run(case, repeats):
        call, knob = case
        if knob is None:
            os.environ.pop(KNOB, None)
        else:
            os.environ[KNOB] = knob
        return workload.timed(stream, call, repeats)

    for case in cases.values():
        run(case, 3)
    samples = {key: [] for key in cases}
    for _ in range(ROUNDS):
        for key, case in cases.items():
            samples[key].append(run(case, REPEATS))
    os.environ.pop(KNOB, None)

    def summary(values):
        values = np.array(values)
        return {"median": round(float(np.median(values)), 2), "min": round(float(values.min()), 2), "max": round(float(values.max()), 2),
                "spread": round(float((values.max() - values.min()) / np.median(values)), 4)}

    result = {"metric": metric, "additive_format": arguments.additive_format, "instances": N, "distinct_arrays": ARRAYS, "tracks": TRACKS, "samples": SAMPLES, "rounds": ROUNDS, "repeats": REPEATS, "bit_rate": BIT_RATE,
              "checked_against": "restatement (%d arrays), aclhip_check_clip with the hash (%d)" % (min(ARRAYS, N, RESTATED), min(ARRAYS, N)),
              "library": os.path.basename(runtime.library_path()), "raw_bytes": int(N * TRACKS * SAMPLES * 48), "blob_bytes": blob_bytes,
              "drop_w_blob_bytes": drop_w_blob_bytes, "row_stride": stride, "segments": runtime.variable_compress_num_segments(SAMPLES),
              "us": {key: summary(values) for key, values in samples.items()}}
    if lab:
        total = result["us"]["compress"]["median"]
        upto = [result["us"]["phases_%d" % k]["median"] for k in range(1, 6)] + [total]
        split = [upto[0]] + [upto[k] - upto[k - 1] for k in range(1, 6)]
        result["phase_us"] = {name: round(value, 2) for name, value in zip(PHASES, split)}
        result["phase_share"] = {name: round(value / total, 3) for name, value in zip(PHASES, split)}
    ctx.close()
    print(json.dumps(result), flush=True)


if __name__ == "__main__":
    main()
