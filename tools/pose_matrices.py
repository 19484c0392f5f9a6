#!/usr/bin/env python3
"""Measurement aid: 3x4 pose matrices (aclhip_pose_matrices_batch) and the matrix error metric (aclhip_measure_pose_error_metric_batch,
ACLHIP_METRIC_QVVF_MATRIX3X4F), HIP events on one stream. One batch: 65 536 instances x 100 bones (the humanoid hierarchy), object space:
  matrices_object        the matrix walk, 64 bytes per bone written
  matrices_local         the conversion alone (no walk), for the difference
  error_matrix_records   the matrix metric, the 8 byte record per instance alone
The yardsticks are measured in the same process on the same buffers, interleaved with the cases:
  yardstick_transform_object   aclhip_transform_poses_batch with object space from the same input buffer (the QVV walk, 48 bytes per bone
                               written): what the matrix launch stands next to
  yardstick_error_qvvf         aclhip_measure_pose_error_batch over the same two buffers, records alone
Before anything is timed the three cases are CHECKED bit for bit on a sample of instances (POSE_MATRICES_SAMPLE, spread over the batch)
against the restatement of tests/test_pose_matrices_oracle.py (numpy float32 operations in the header's order). A mismatch or a refused
instance exits non-zero. The rows are those of tools/pose_error.py; POSE_MATRICES_NEGATIVE_SCALES=1 makes a sixth of the scales negative.
Time is reported, never judged: per case the median of POSE_MATRICES_ROUNDS interleaved rounds of POSE_MATRICES_REPEATS launches each, the
spread (max - min) / median, the ratio to its yardstick's median, and the algorithmic bytes (rows read, rows or records written) as a rate
and as a fraction of the HBM peak of the specification (8 TB/s). Prints one JSON line."""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import torch  # noqa: E402
from acl_amd import runtime, synth  # noqa: E402
from test_pose_matrices_oracle import expected_matrix_measure, object_matrices  # noqa: E402  (the checker's restatement)

N = int(os.environ.get("POSE_MATRICES_INSTANCES", "65536"))
BONES = int(os.environ.get("POSE_MATRICES_BONES", "100"))
ROUNDS = int(os.environ.get("POSE_MATRICES_ROUNDS", "3"))
REPEATS = int(os.environ.get("POSE_MATRICES_REPEATS", "20"))
SAMPLE = int(os.environ.get("POSE_MATRICES_SAMPLE", "48"))
NEGATIVE_SCALES = os.environ.get("POSE_MATRICES_NEGATIVE_SCALES", "0") != "0"
SHELL = 3.0
POOL = 2048          # distinct random rows per buffer; the batch repeats them (every row has its own address: the traffic is the batch's)
HBM_PEAK_BYTES_PER_SECOND = 8.0e12
YARDSTICK_OF = {"matrices_object": "yardstick_transform_object", "matrices_local": "yardstick_transform_object", "error_matrix_records": "yardstick_error_qvvf"}


def timed(stream, launch, repeats):
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record(stream)
    for _ in range(repeats):
        launch()
    stop.record(stream)
    stop.synchronize()
    return start.elapsed_time(stop) * 1000.0 / repeats


def random_rows(rng, count):
    """unit rotations, translations within +-10, scale magnitudes in [0.9, 1.1]: the rows of tools/pose_error.py, so the yardsticks are the
    launches that profiles/pose_error.md timed. With POSE_MATRICES_NEGATIVE_SCALES a sixth of the scale components are negative: the
    matrix launches do the same work, the QVV yardsticks take qvv_mul's matrix route at almost every bone and count it."""
    rows = np.zeros((count, BONES, 12), dtype=np.float32)
    rotations = rng.normal(size=(count, BONES, 4))
    rows[..., 0:4] = rotations / np.linalg.norm(rotations, axis=2, keepdims=True)
    rows[..., 4:7] = rng.uniform(-10.0, 10.0, size=(count, BONES, 3))
    scales = rng.uniform(0.9, 1.1, size=(count, BONES, 3))
    rows[..., 8:11] = np.where(rng.uniform(size=scales.shape) < 1.0 / 6.0, -scales, scales) if NEGATIVE_SCALES else scales
    return rows


def main():
    if not torch.cuda.is_available():
        raise SystemExit("tools/pose_matrices.py needs a GPU: nothing is measured without one")
    stride, matrix_stride = BONES * 48, BONES * 64
    parents = np.array(synth.humanoid_hierarchy(BONES), dtype=np.uint32)
    identity = np.zeros((BONES, 12), dtype=np.float32)
    identity[:, 3], identity[:, 8:11] = 1.0, 1.0
    rng = np.random.default_rng(7400 + BONES)
    stream = torch.cuda.Stream()
    s = stream.cuda_stream
    ctx = runtime.Context(0)
    skeleton = ctx.register_skeleton(parents, identity)
    repeats_of_pool = (N + POOL - 1) // POOL
    raw_pool = random_rows(rng, min(POOL, N))
    # the lossy rows: the raw ones as a codec leaves them, a relative error of up to 1e-3 per float
    lossy_pool = (raw_pool * (1.0 + rng.uniform(-1.0e-3, 1.0e-3, size=raw_pool.shape))).astype(np.float32)
    with torch.cuda.stream(stream):
        raw, lossy = (torch.from_numpy(pool).cuda().repeat(repeats_of_pool, 1, 1)[:N].contiguous() for pool in (raw_pool, lossy_pool))
        matrices = torch.zeros((N, BONES, 16), dtype=torch.float32, device="cuda")
        yardstick_out = torch.zeros((N, BONES, 12), dtype=torch.float32, device="cuda")
        errors = torch.zeros((N, 2), dtype=torch.int32, device="cuda")
    sample = np.unique(np.linspace(0, N - 1, min(SAMPLE, N)).astype(np.int64))
    d_sample = torch.from_numpy(sample).cuda()

    def matrices_desc(object_space):
        desc = runtime.PoseMatricesDesc()
        desc.skeleton, desc.object_space, desc.layout = skeleton, 1 if object_space else 0, runtime.MATRIX_3X4F_64
        return desc

    matrix_descs = {True: matrices_desc(True), False: matrices_desc(False)}
    error_desc = runtime.PoseErrorDesc()
    error_desc.skeleton, error_desc.object_space, error_desc.shell_distance = skeleton, 1, SHELL
    forward = runtime.PoseBufferConsumers()
    forward.skeleton, forward.object_space = skeleton, 1

    cases = {
        "matrices_object": lambda: ctx.pose_matrices_batch(raw.data_ptr(), stride, N, matrix_descs[True], matrices.data_ptr(), matrix_stride, stream=s),
        "matrices_local": lambda: ctx.pose_matrices_batch(raw.data_ptr(), stride, N, matrix_descs[False], matrices.data_ptr(), matrix_stride, stream=s),
        "error_matrix_records": lambda: ctx.measure_pose_error_metric(raw.data_ptr(), stride, lossy.data_ptr(), stride, N, error_desc, runtime.ERROR_METRIC_QVVF_MATRIX3X4F,
                                                                      errors.data_ptr(), stream=s),
        "yardstick_transform_object": lambda: ctx.transform_poses_batch(raw.data_ptr(), stride, N, forward, yardstick_out.data_ptr(), stride, stream=s),
        "yardstick_error_qvvf": lambda: ctx.measure_pose_error(raw.data_ptr(), stride, lossy.data_ptr(), stride, N, error_desc, errors.data_ptr(), stream=s),
    }
    traffic = {"matrices_object": N * stride + N * matrix_stride, "matrices_local": N * stride + N * matrix_stride, "error_matrix_records": 2 * N * stride + 8 * N,
               "yardstick_transform_object": 2 * N * stride, "yardstick_error_qvvf": 2 * N * stride + 8 * N}

    # ---- checked before it is timed (the clears, the launch and the gathers on ONE stream: in order)
    for object_space, key in ((True, "matrices_object"), (False, "matrices_local")):
        with torch.cuda.stream(stream):
            matrices.fill_(-5.0)
            cases[key]()
            got = matrices[d_sample].cpu().numpy()
        for index, i in enumerate(sample):
            want = object_matrices(parents, raw_pool[i % POOL], object_space)
            if not np.array_equal(got[index].view(np.uint32).reshape(-1), want.view(np.uint32).reshape(-1)):
                print(f"MISMATCH in {key}, instance {i}", flush=True)
                sys.exit(1)
    with torch.cuda.stream(stream):
        errors.zero_()
        cases["error_matrix_records"]()
        got_records = errors.cpu().numpy().view(runtime.POSE_ERROR_DTYPE).reshape(N)
    for i in sample:
        _, (error, bone) = expected_matrix_measure(parents, raw_pool[i % POOL], lossy_pool[i % POOL], SHELL)
        if got_records[i]["error"].view(np.uint32) != np.float32(error).view(np.uint32) or int(got_records[i]["bone"]) != bone:
            print(f"MISMATCH in error_matrix_records, instance {i}", flush=True)
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
    result = {"instances": N, "bones": BONES, "negative_scales": NEGATIVE_SCALES, "rounds": ROUNDS, "repeats": REPEATS, "checked_instances": int(sample.size), "us": {}, "traffic": {}}
    for key, values in samples.items():
        values = np.array(values)
        result["us"][key] = {"median": round(float(np.median(values)), 2), "min": round(float(values.min()), 2), "max": round(float(values.max()), 2),
                             "spread": round(float((values.max() - values.min()) / np.median(values)), 4)}
    for key, bytes_moved in traffic.items():
        rate = bytes_moved / (result["us"][key]["median"] * 1e-6)
        result["traffic"][key] = {"bytes": bytes_moved, "gb_per_second": round(rate / 1e9, 1), "fraction_of_hbm_peak": round(rate / HBM_PEAK_BYTES_PER_SECOND, 3)}
    for key, yardstick in YARDSTICK_OF.items():
        result["us"][key]["over_yardstick"] = round(result["us"][key]["median"] / result["us"][yardstick]["median"], 3)
    ctx.close()
    print(json.dumps(result), flush=True)


if __name__ == "__main__":
    main()
