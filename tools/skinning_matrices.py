#!/usr/bin/env python3
"""Measurement aid: skinning palettes (aclhip_skinning_matrices_batch), HIP events on one stream. One batch: 65 536 instances x 100 bones
(the humanoid hierarchy), a skin of 100 joints (a permutation of the bones, random finite inverse bind matrices), object space:
  palette_transposed48   three float4 rows per joint, 48 bytes written
  palette_64             rtm::matrix3x4f per joint, 64 bytes written
The yardstick is measured in the same process on the same input buffer, interleaved with the cases:
  yardstick_matrices_object   aclhip_pose_matrices_batch with object space (64 bytes per bone written, no product): what a caller ran before,
                              in front of a kernel of their own
Before anything is timed both cases are CHECKED bit for bit on a sample of instances (SKINNING_MATRICES_SAMPLE, spread over the batch)
against the restatement of tests/test_skinning_matrices_oracle.py (numpy float32 operations in the header's order). A mismatch or a
refused instance exits non-zero. The rows are those of tools/pose_matrices.py.
Time is reported, never judged: per case the median of SKINNING_MATRICES_ROUNDS interleaved rounds of SKINNING_MATRICES_REPEATS launches
each, the spread (max - min) / median, the ratio to the yardstick's median, and the algorithmic bytes (rows read, records written; the
skin is read once) as a rate and as a fraction of the HBM peak of the specification (8 TB/s). Prints one JSON line."""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import torch  # noqa: E402
from acl_amd import runtime, synth  # noqa: E402
from test_skinning_matrices_oracle import skinning_matrices  # noqa: E402  (the checker's restatement)

N = int(os.environ.get("SKINNING_MATRICES_INSTANCES", "65536"))
BONES = int(os.environ.get("SKINNING_MATRICES_BONES", "100"))
ROUNDS = int(os.environ.get("SKINNING_MATRICES_ROUNDS", "3"))
REPEATS = int(os.environ.get("SKINNING_MATRICES_REPEATS", "20"))
SAMPLE = int(os.environ.get("SKINNING_MATRICES_SAMPLE", "48"))
POOL = 2048          # distinct random rows; the batch repeats them (every row has its own address: the traffic is the batch's)
HBM_PEAK_BYTES_PER_SECOND = 8.0e12
LAYOUT_OF = {"palette_transposed48": runtime.PALETTE_3X4F_TRANSPOSED_48, "palette_64": runtime.PALETTE_3X4F_64}
YARDSTICK = "yardstick_matrices_object"


def timed(stream, launch, repeats):
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record(stream)
    for _ in range(repeats):
        launch()
    stop.record(stream)
    stop.synchronize()
    return start.elapsed_time(stop) * 1000.0 / repeats


def random_rows(rng, count):
    """unit rotations, translations within +-10, scale magnitudes in [0.9, 1.1]: the rows of tools/pose_matrices.py"""
    rows = np.zeros((count, BONES, 12), dtype=np.float32)
    rotations = rng.normal(size=(count, BONES, 4))
    rows[..., 0:4] = rotations / np.linalg.norm(rotations, axis=2, keepdims=True)
    rows[..., 4:7] = rng.uniform(-10.0, 10.0, size=(count, BONES, 3))
    rows[..., 8:11] = rng.uniform(0.9, 1.1, size=(count, BONES, 3))
    return rows


def main():
    if not torch.cuda.is_available():
        raise SystemExit("tools/skinning_matrices.py needs a GPU: nothing is measured without one")
    joints_count = BONES
    stride, matrix_stride = BONES * 48, BONES * 64
    parents = np.array(synth.humanoid_hierarchy(BONES), dtype=np.uint32)
    identity = np.zeros((BONES, 12), dtype=np.float32)
    identity[:, 3], identity[:, 8:11] = 1.0, 1.0
    rng = np.random.default_rng(7500 + BONES)
    joints = rng.permutation(BONES).astype(np.uint32)
    bind = rng.uniform(-1.0, 1.0, size=(joints_count, 4, 4)).astype(np.float32)
    stream = torch.cuda.Stream()
    s = stream.cuda_stream
    ctx = runtime.Context(0)
    skeleton = ctx.register_skeleton(parents, identity)
    skin = ctx.register_skin(joints, bind, BONES)
    repeats_of_pool = (N + POOL - 1) // POOL
    pool = random_rows(rng, min(POOL, N))
    with torch.cuda.stream(stream):
        poses = torch.from_numpy(pool).cuda().repeat(repeats_of_pool, 1, 1)[:N].contiguous()
        # one output buffer of the widest record for every case: the launches write the same addresses
        out = torch.zeros((N, BONES, 16), dtype=torch.float32, device="cuda")
    sample = np.unique(np.linspace(0, N - 1, min(SAMPLE, N)).astype(np.int64))
    d_sample = torch.from_numpy(sample).cuda()

    def skinning_desc(layout):
        desc = runtime.SkinningDesc()
        desc.skeleton, desc.skin, desc.object_space, desc.layout = skeleton, skin, 1, layout
        return desc

    descs = {key: skinning_desc(layout) for key, layout in LAYOUT_OF.items()}
    matrices_desc = runtime.PoseMatricesDesc()
    matrices_desc.skeleton, matrices_desc.object_space, matrices_desc.layout = skeleton, 1, runtime.MATRIX_3X4F_64
    record_bytes = {key: runtime.PALETTE_RECORD_BYTES[layout] for key, layout in LAYOUT_OF.items()}

    def palette_launch(key):
        return lambda: ctx.skinning_matrices_batch(poses.data_ptr(), stride, N, descs[key], out.data_ptr(), joints_count * record_bytes[key], stream=s)

    cases = {key: palette_launch(key) for key in LAYOUT_OF}
    cases[YARDSTICK] = lambda: ctx.pose_matrices_batch(poses.data_ptr(), stride, N, matrices_desc, out.data_ptr(), matrix_stride, stream=s)
    traffic = {key: N * stride + N * joints_count * record_bytes[key] for key in LAYOUT_OF}
    traffic[YARDSTICK] = N * stride + N * matrix_stride

    # ---- checked before it is timed (the clear, the launch and the gather on ONE stream: in order)
    for key, layout in LAYOUT_OF.items():
        row_floats = joints_count * record_bytes[key] // 4
        with torch.cuda.stream(stream):
            out.fill_(-5.0)
            cases[key]()
            got = out.view(-1)[: N * row_floats].view(N, row_floats)[d_sample].cpu().numpy()
        for index, i in enumerate(sample):
            want = skinning_matrices(parents, pool[i % POOL], joints, bind, True, layout)
            if not np.array_equal(got[index].view(np.uint32).reshape(-1), want.view(np.uint32).reshape(-1)):
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
    result = {"instances": N, "bones": BONES, "joints": joints_count, "rounds": ROUNDS, "repeats": REPEATS, "checked_instances": int(sample.size), "us": {}, "traffic": {}}
    for key, values in samples.items():
        values = np.array(values)
        result["us"][key] = {"median": round(float(np.median(values)), 2), "min": round(float(values.min()), 2), "max": round(float(values.max()), 2),
                             "spread": round(float((values.max() - values.min()) / np.median(values)), 4)}
    for key, bytes_moved in traffic.items():
        rate = bytes_moved / (result["us"][key]["median"] * 1e-6)
        result["traffic"][key] = {"bytes": bytes_moved, "gb_per_second": round(rate / 1e9, 1), "fraction_of_hbm_peak": round(rate / HBM_PEAK_BYTES_PER_SECOND, 3)}
    for key in LAYOUT_OF:
        result["us"][key]["over_yardstick"] = round(result["us"][key]["median"] / result["us"][YARDSTICK]["median"], 3)
    ctx.close()
    print(json.dumps(result), flush=True)


if __name__ == "__main__":
    main()
