#!/usr/bin/env python3
"""Measurement aid: aclhip_find_bit_rates_batch, HIP events on one stream, on the workload of tools/compress_tracks.py -- its arrays,
its parent table, its settings: COMPRESS_TRACKS_INSTANCES instances over COMPRESS_TRACKS_ARRAYS distinct raw track arrays of 100
tracks x 301 samples.
Before anything is timed the table is CHECKED: the rows of the first FIND_BIT_RATES_RESTATED distinct arrays byte for byte against the
restatement of tests/bit_rate_search_restatement.py. A mismatch, a refused instance or a status that is not ok exits non-zero.
Time is reported, never judged: the median of FIND_BIT_RATES_ROUNDS interleaved rounds of FIND_BIT_RATES_REPEATS launches each and the
spread (max - min) / median; in the same rounds aclhip_compress_tracks_variable_batch at the table the search found, so that the two
are measured side by side; the bytes of those blobs next to the bytes at a uniform rate of 16. With ACLHIP_LIBRARY pointing at
libaclhip_lab.so the line also carries the per-phase split: ACLHIP_FIND_BIT_RATES_PHASES=k stops the call behind its k-th launch (shell,
analysis, segments, local, object), and a phase's time is the difference of two medians measured in the same rounds. With
FIND_BIT_RATES_AT_PRECISION=1 the first array also goes through runtime.compress_tracks_at_precision, for its blob's size and rate.
--metric {0,1}: the aclhip_error_metric of the search and of the compress call. With 1 (the reference's matrix metric, through the
_metric entry points, checked against tests/matrix_metric_compress_restatement.py) the qvvf calls are timed IN THE SAME ROUNDS, their
blob bytes reported beside, and every key of metric 0 carries the suffix _qvvf. --scales nonuniform: every scale of the workload's
arrays drawn anew per sample and component within 0.9 .. 1.1, so that has_scale holds in every array and shear builds up down the
chains -- the workload the matrix metric is for. --level: the compression level of the search; lowest, low and medium go through
aclhip_find_bit_rates_batch (or its _metric form), high, highest and automatic through aclhip_find_bit_rates_level_batch with its
workspace, checked against tests/bit_rate_search_levels_restatement.py; the lab library's knob is then
ACLHIP_FIND_BIT_RATES_LEVEL_PHASES and the split has a sixth phase, the level per instance, in front of the object phase. The
workload's spine makes chains of 26 bones, where the wider levels are at their most expensive (automatic picks medium for it): size
the batch with COMPRESS_TRACKS_INSTANCES. --additive-format {relative,additive0,additive1}: every array is an additive clip on a drawn
base clip of its own (another array of the workload's; under additive1 the clips' scales are moved by -1 and the default scale is 0):
the search and the compress call go through the _additive entry points (the search is then the level search at every level), checked
against tests/additive_compress_restatement.py, and the calls WITHOUT a base are timed in the same rounds on the same arrays, every
key of theirs with the suffix _no_base. Prints one JSON line."""
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
import bit_rate_search_restatement as restatement  # noqa: E402  (the checker's restatement)
import bit_rate_search_levels_restatement as levels_restatement  # noqa: E402  (and at every level)
import matrix_metric_compress_restatement as metric_restatement  # noqa: E402  (and with the metric as an argument)
import additive_compress_restatement as additive_restatement  # noqa: E402  (and with an additive base)

N, ARRAYS, TRACKS, SAMPLES = workload.N, workload.ARRAYS, workload.TRACKS, workload.SAMPLES
ROUNDS = int(os.environ.get("FIND_BIT_RATES_ROUNDS", "3"))
REPEATS = int(os.environ.get("FIND_BIT_RATES_REPEATS", "3"))
RESTATED = int(os.environ.get("FIND_BIT_RATES_RESTATED", "1"))
AT_PRECISION = os.environ.get("FIND_BIT_RATES_AT_PRECISION", "0") == "1"
RATE, PRECISION, SHELL = workload.RATE, workload.PRECISION, workload.SHELL
PHASES = ("shell", "analysis", "segments", "local", "object")
KNOB = "ACLHIP_FIND_BIT_RATES_PHASES"
LEVEL_PHASES = ("shell", "analysis", "segments", "local", "level", "object")         # aclhip_find_bit_rates_level_batch
LEVEL_KNOB = "ACLHIP_FIND_BIT_RATES_LEVEL_PHASES"


def main():
    parser = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    parser.add_argument("--metric", type=int, choices=(0, 1), default=0, help="aclhip_error_metric: 0 qvvf (the entry points without a metric), 1 qvvf_matrix3x4f")
    parser.add_argument("--scales", choices=("workload", "nonuniform"), default="workload", help="nonuniform: every scale within 0.9 .. 1.1, per sample and component")
    parser.add_argument("--level", choices=sorted(runtime.COMPRESSION_LEVELS, key=runtime.COMPRESSION_LEVELS.get), default="medium",
                        help="the compression level; high, highest and automatic go through aclhip_find_bit_rates_level_batch")
    parser.add_argument("--additive-format", choices=("none", "relative", "additive0", "additive1"), default="none",
                        help="compress every array as an additive clip against a drawn base clip, through the _additive entry points")
    arguments = parser.parse_args()
    metric = arguments.metric
    level = runtime.COMPRESSION_LEVELS[arguments.level]
    additive_format = {"none": runtime.ADDITIVE_NONE, "relative": runtime.ADDITIVE_RELATIVE, "additive0": runtime.ADDITIVE_ADDITIVE0, "additive1": runtime.ADDITIVE_ADDITIVE1}[arguments.additive_format]
    with_base = additive_format != runtime.ADDITIVE_NONE
    if with_base and metric != runtime.ERROR_METRIC_QVVF:
        parser.error("an additive base goes with the qvvf error metric: the reference has no additive matrix metric")
    if not torch.cuda.is_available():
        raise SystemExit("tools/find_bit_rates.py needs a GPU: nothing is measured without one")
    rng = np.random.default_rng(9100 + TRACKS)
    arrays = [workload.make_array(rng) for _ in range(ARRAYS)]
    if arguments.scales == "nonuniform":
        scale_rng = np.random.default_rng(9200 + TRACKS)
        for samples in arrays:
            samples[:, :, 8:11] = scale_rng.uniform(0.9, 1.1, size=(SAMPLES, TRACKS, 3))
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
    segments = runtime.variable_compress_num_segments(SAMPLES)

    stream = torch.cuda.Stream()
    s = stream.cuda_stream
    ctx = runtime.Context(0)
    handles = np.array([ctx.register_raw_tracks(a, RATE) for a in arrays], dtype=np.uint32)
    base_handles = np.array([ctx.register_raw_tracks(a, RATE) for a in base_arrays], dtype=np.uint32)
    # the entry points of the search and of the compress call, their workspace and whether the results carry levels: the runtime's own route
    route = dict(metric=metric, additive_base=base_handles[order] if with_base else None, additive_format=additive_format)
    search_call, workspace_bytes, with_levels, search_alive = runtime.transform_compress_route(ctx, "search", handles[order], level=level, **route)
    compress_call, _, _, compress_alive = runtime.transform_compress_route(ctx, "variable", handles[order], **route)
    phases, knob_name = (LEVEL_PHASES, LEVEL_KNOB) if with_levels else (PHASES, KNOB)
    stride = runtime.variable_compress_bound(TRACKS, SAMPLES, 0)
    with torch.cuda.stream(stream):
        d_raws = torch.from_numpy(handles[order].view(np.int32)).cuda()
        d_parents = torch.from_numpy(parents.view(np.int32)).cuda()
        d_rates = torch.zeros((N, segments, TRACKS, 4), dtype=torch.uint8, device="cuda")
        d_blobs = torch.zeros((N, stride), dtype=torch.uint8, device="cuda")
        d_results = torch.zeros((N, 2), dtype=torch.int32, device="cuda")
        d_workspace = torch.zeros(workspace_bytes(N, TRACKS, SAMPLES), dtype=torch.uint8, device="cuda")
        d_pose = torch.from_numpy(default_pose).cuda() if default_pose is not None else None
    search = runtime.FindBitRatesDesc()
    search.precision, search.shell_distance, search.max_tracks, search.max_samples, search.workspace, search.level = PRECISION, SHELL, TRACKS, SAMPLES, d_workspace.data_ptr(), level
    search.parent_indices, search.num_table_tracks = d_parents.data_ptr(), TRACKS
    desc = runtime.CompressVariableDesc()
    desc.precision, desc.shell_distance, desc.max_tracks, desc.max_samples, desc.workspace = PRECISION, SHELL, TRACKS, SAMPLES, d_workspace.data_ptr()
    desc.parent_indices, desc.num_table_tracks = d_parents.data_ptr(), TRACKS
    desc.bit_rates, desc.bit_rate_segment_stride, desc.bit_rate_instance_stride = d_rates.data_ptr(), 4 * TRACKS, 4 * TRACKS * segments
    if default_pose is not None:
        search.default_pose = desc.default_pose = d_pose.data_ptr()

    search_arguments = (d_raws.data_ptr(), N, search, d_rates.data_ptr(), 4 * TRACKS * segments, 4 * TRACKS, d_results.data_ptr())
    compress_arguments = (d_raws.data_ptr(), N, desc, d_blobs.data_ptr(), stride, d_results.data_ptr())

    def launch_search():
        search_call(*search_arguments, stream=s)

    def launch_compress():
        compress_call(*compress_arguments, stream=s)

    # timed beside under --metric 1 or a base, named here on purpose: the qvvf entry points without a base that take the same desc and workspace
    def launch_search_qvvf():
        (ctx.find_bit_rates_level_batch if with_levels else ctx.find_bit_rates_batch)(*search_arguments, stream=s)

    def launch_compress_qvvf():
        ctx.compress_tracks_variable_batch(*compress_arguments, stream=s)

    # ---- checked before it is timed
    os.environ.pop(knob_name, None)
    qvvf_blob_bytes = None
    other = "_qvvf" if metric != runtime.ERROR_METRIC_QVVF else "_no_base" if with_base else None       # the calls timed beside: without the metric, or without the base
    if other is not None:         # (the other search's blobs, for their bytes; the table is searched again below)
        with torch.cuda.stream(stream):
            launch_search_qvvf()
            launch_compress_qvvf()
            qvvf_blob_bytes = int(d_results.cpu().numpy().view(np.uint32)[:, 1].astype(np.int64).sum())
    with torch.cuda.stream(stream):
        launch_search()
        results = d_results.cpu().numpy().view(np.uint32).copy()
        tables = d_rates[:ARRAYS].cpu().numpy()
    if ctx.rejected_instance_count() != 0 or np.any(results[:, 0] != runtime.COMPRESS_OK):
        print(f"refused or failed instances: {ctx.rejected_instance_count()}, statuses {np.unique(results[:, 0])}", flush=True)
        sys.exit(1)
    searched_levels = sorted(int(word) for word in np.unique(results[:, 1])) if with_levels else [level]
    evaluations = None
    for i in range(min(ARRAYS, N, RESTATED)):
        if with_base:
            restated = additive_restatement.find_bit_rates(arrays[i], RATE, additive_restatement.Base(base_arrays[i], RATE, additive_format), level=level, parents=parents,
                                                           precision=PRECISION, shell_distance=SHELL, **({"default_pose": default_pose} if default_pose is not None else {}))
        else:
            restated = levels_restatement.find_bit_rates_metric(arrays[i], RATE, metric, level=level, parents=parents, precision=PRECISION, shell_distance=SHELL)
        expected = restated.table
        if with_levels:
            evaluations = {"array": i, "with_the_memo": int(restated.evaluations), "without_the_memo": int(restated.evaluations_unmemoized)}
        if (with_levels and int(results[i, 1]) != restated.level) or not np.array_equal(tables[i], expected):
            print(f"MISMATCH with the restatement in the table of array {i}: {int((tables[i] != expected).sum())} bytes", flush=True)
            sys.exit(1)
    with torch.cuda.stream(stream):
        launch_compress()
        results = d_results.cpu().numpy().view(np.uint32).copy()
    if np.any(results[:, 0] != runtime.COMPRESS_OK):
        print(f"the compress call at the table the search found: statuses {np.unique(results[:, 0])}", flush=True)
        sys.exit(1)
    blob_bytes = int(results[:, 1].astype(np.int64).sum())
    animated = tables[:, :, :, 0:3][tables[:, :, :, 0:3] != 255]
    uniform = runtime.CompressVariableDesc.from_buffer_copy(desc)
    uniform.bit_rates, uniform.rotation_bit_rate, uniform.translation_bit_rate, uniform.scale_bit_rate = None, 16, 16, 16
    with torch.cuda.stream(stream):
        ctx.compress_tracks_variable_batch(d_raws.data_ptr(), N, uniform, d_blobs.data_ptr(), stride, d_results.data_ptr(), stream=s)
        uniform_bytes = int(d_results.cpu().numpy().view(np.uint32)[:, 1].astype(np.int64).sum())

    at_precision = None
    if AT_PRECISION:
        skeleton = ctx.register_skeleton(parents, np.tile(restatement.IDENTITY, (TRACKS, 1)))
        blob, rate = runtime.compress_tracks_at_precision(ctx, int(handles[0]), skeleton, SHELL, PRECISION, parents=parents, shell_distance=SHELL)
        searched = runtime.compress_tracks_variable(ctx, int(handles[0]), bit_rates="search", parents=parents, precision=PRECISION, shell_distance=SHELL)[0]
        clip = ctx.register_clip(searched)
        error = runtime.raw_clip_error(ctx, int(handles[0]), clip, skeleton, SHELL)[1]
        ctx.unregister_clip(clip)
        ctx.unregister_skeleton(skeleton)
        at_precision = {"uniform_rate": rate, "uniform_rate_blob_bytes": int(blob.size), "searched_blob_bytes": int(searched.size), "searched_raw_clip_error": round(float(error), 6)}

    lab = "lab" in os.path.basename(runtime.library_path())
    cases = {"search": (launch_search, None), "compress_at_the_table": (launch_compress, None)}
    if lab:
        for k in range(1, len(phases)):
            cases["phases_%d" % k] = (launch_search, str(k))
    if other is not None:         # (the compress call behind the other search reads this table: its time does not depend on how the rates were found)
        cases["search" + other] = (launch_search_qvvf, None)
        cases["compress_at_the_table" + other] = (launch_compress_qvvf, None)
        if lab:
            for k in range(1, len(phases)):
                cases["phases_%d%s" % (k, other)] = (launch_search_qvvf, str(k))

    def run(case, repeats):
        call, knob = case
        if knob is None:
            os.environ.pop(knob_name, None)
        else:
            os.environ[knob_name] = knob
        return workload.timed(stream, call, repeats)

    for case in cases.values():
        run(case, 1)
    samples = {key: [] for key in cases}
    for _ in range(ROUNDS):
        for key, case in cases.items():
            samples[key].append(run(case, REPEATS))
    os.environ.pop(knob_name, None)

    def summary(values):
        values = np.array(values)
        return {"median": round(float(np.median(values)), 2), "min": round(float(values.min()), 2), "max": round(float(values.max()), 2),
                "spread": round(float((values.max() - values.min()) / np.median(values)), 4)}

    result = {"metric": metric, "additive_format": arguments.additive_format, "level": arguments.level, "searched_levels": searched_levels, "scales": arguments.scales, "instances": N, "distinct_arrays": ARRAYS, "tracks": TRACKS, "samples": SAMPLES, "segments": segments, "rounds": ROUNDS, "repeats": REPEATS,
              "checked_against": "restatement (%d arrays)" % min(ARRAYS, N, RESTATED), "library": os.path.basename(runtime.library_path()),
              "raw_bytes": int(N * TRACKS * SAMPLES * 48), "searched_blob_bytes": blob_bytes, "uniform_16_blob_bytes": uniform_bytes,
              "rates": {"min": int(animated.min()), "max": int(animated.max()), "mean": round(float(animated.mean()), 2)} if animated.size else None,
              "us": {key: summary(values) for key, values in samples.items()}}
    if at_precision is not None:
        result["first_array"] = at_precision
    if qvvf_blob_bytes is not None:
        result["searched_blob_bytes" + other] = qvvf_blob_bytes
    if evaluations is not None:
        result["object_errors_in_the_restatement"] = evaluations
    for suffix in ("", "_qvvf", "_no_base") if lab else ():
        if "search" + suffix not in result["us"]:
            continue
        total = result["us"]["search" + suffix]["median"]
        upto = [result["us"]["phases_%d%s" % (k, suffix)]["median"] for k in range(1, len(phases))] + [total]
        split = [upto[0]] + [upto[k] - upto[k - 1] for k in range(1, len(phases))]
        result["phase_us" + suffix] = {name: round(value, 2) for name, value in zip(phases, split)}
        result["phase_share" + suffix] = {name: round(value / total, 3) for name, value in zip(phases, split)}
    ctx.close()
    print(json.dumps(result), flush=True)


if __name__ == "__main__":
    main()
