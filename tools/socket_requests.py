#!/usr/bin/env python3
"""Measurement aid: single bone requests in object space (aclhip_decompress_track_object_batch) against today's route, HIP events on one
stream, the method of tools/skeleton_poses.py. Batch: 65 536 characters of 100-bone clips x {1, 4, 16} sockets each, character-major
request lists, sockets drawn among the SHALLOW bones (depth <= 3) or the DEEP ones (depth >= 10) of the synthetic humanoid; over one
clip and over the bench's 256 clips as drawn. Per case, interleaved over SOCKETS_ROUNDS rounds of SOCKETS_REPEATS launches:
  requests    (a) the request launch: 48 bytes per request
  whole pose  (b) what a caller does without it: aclhip_decompress_poses_batch with object space into full rows (the parent commit's
              kernels, unchanged), followed by a torch gather of the requested records
Before it is timed every case is CHECKED bit for bit: every request against the gathered records of (b), and the requests of
SOCKETS_CHECK characters (default 512) against the oracle's object space poses; a mismatch or a refused request exits non-zero. Time is
reported, never judged: median of the rounds, spread (max - min) / median, and the ratio b / a. The clocks (sysfs, read only) are
sampled UNDER LOAD, as tools/skeleton_poses.py does. SOCKETS_CASE=<index> runs one case only; SOCKETS_PROFILE=1 launches only (a) and
the pose launch of (b) of it, a few times (for a rocprofv3 --kernel-trace --stats run and, separately, a --pmc run)."""
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
from skeleton_poses import CLOCK_SAMPLES, clocks, timed  # noqa: E402  (tools/ is the script's directory)

TRACKS = 100


def measure(ctx, stream, name, clips, handles, parents, depth, n, sockets_per_character, deep, rounds, repeats, check):
    rng = np.random.default_rng(3000 + sockets_per_character + int(deep))
    pool = np.flatnonzero(depth >= 10) if deep else np.flatnonzero(depth <= 3)
    sockets = rng.choice(pool, size=sockets_per_character, replace=pool.size < sockets_per_character).astype(np.uint32)
    which = rng.integers(0, len(clips), size=n)
    durations = np.array([c.duration for c in clips], dtype=np.float32)
    character_times = (rng.uniform(0.0, 1.0, size=n).astype(np.float32) * durations[which]).astype(np.float32)
    requests = n * sockets_per_character
    with torch.cuda.stream(stream):
        def up(array, dtype):
            return torch.from_numpy(np.ascontiguousarray(array, dtype=dtype).view(np.int32 if dtype == np.uint32 else dtype)).cuda()
        d_character_clips, d_character_times = up(handles[which], np.uint32), up(character_times, np.float32)
        d_clips, d_times = up(np.repeat(handles[which], sockets_per_character), np.uint32), up(np.repeat(character_times, sockets_per_character), np.float32)
        d_bones = up(np.tile(sockets, n), np.uint32)
        d_gather = torch.from_numpy(sockets.astype(np.int64)).cuda()
        transforms = torch.zeros((requests, 12), dtype=torch.float32, device="cuda")
        poses = torch.zeros((n, TRACKS, 12), dtype=torch.float32, device="cuda")
    s = stream.cuda_stream
    consumers = runtime.PoseConsumers()
    consumers.object_space = 1

    def request_launch():
        ctx.decompress_track_object_batch(d_clips.data_ptr(), d_times.data_ptr(), d_bones.data_ptr(), requests, transforms.data_ptr(), stream=s)

    def pose_launch():
        ctx.decompress_poses_batch(d_character_clips.data_ptr(), d_character_times.data_ptr(), n, poses.data_ptr(), TRACKS * 48, consumers, stream=s)

    def whole_pose():
        pose_launch()
        with torch.cuda.stream(stream):
            return poses.index_select(1, d_gather)

    if os.environ.get("SOCKETS_PROFILE") == "1":
        for _ in range(5):
            request_launch()
            pose_launch()
        stream.synchronize()
        return {"case": name, "checked": True, "profile_only": True}

    request_launch()
    gathered = whole_pose()
    stream.synchronize()
    got = transforms.cpu().numpy().reshape(n, sockets_per_character, 12)
    ok = np.array_equal(got.view(np.uint32), gathered.cpu().numpy().view(np.uint32))
    sample = np.arange(n) if check == 0 else np.unique(np.concatenate([np.arange(min(n, 128)), np.random.default_rng(7).choice(n, size=min(n, max(check - 128, 1)), replace=False)]))
    for i in sample:
        expected = ob.oracle_local_to_object_space(parents, ob.oracle_decompress_tracks(clips[which[i]].blob, float(character_times[i])))[sockets.astype(np.int64)]
        if not np.array_equal(got[i].view(np.uint32), expected.view(np.uint32)):
            print(f"MISMATCH: case {name!r}, character {i}", flush=True)
            ok = False
            break
    for step in (request_launch, whole_pose):
        for _ in range(10):
            step()
    samples = {"requests": [], "whole_pose": []}
    for _ in range(rounds):
        samples["requests"].append(timed(stream, request_launch, repeats))
        samples["whole_pose"].append(timed(stream, whole_pose, repeats))
    result = {"case": name, "characters": n, "clips": len(clips), "sockets": sockets_per_character, "deep": bool(deep), "socket_depths": [int(depth[b]) for b in sockets],
              "checked": bool(ok), "characters_checked_against_oracle": int(len(sample))}
    for key, values in samples.items():
        median = float(np.median(values))
        result[key + "_us"] = round(median, 2)
        result[key + "_spread"] = round(float((max(values) - min(values)) / median), 4)
    result["whole_pose_over_requests"] = round(result["whole_pose_us"] / result["requests_us"], 3)
    return result


def main():
    rounds = int(os.environ.get("SOCKETS_ROUNDS", "7"))
    repeats = int(os.environ.get("SOCKETS_REPEATS", "50"))
    check = int(os.environ.get("SOCKETS_CHECK", "512"))
    num_clips = int(os.environ.get("SOCKETS_CLIPS", "256"))
    ctx = runtime.Context(0)
    stream = torch.cuda.Stream()
    parents = np.array(synth.humanoid_hierarchy(TRACKS), dtype=np.uint32)
    depth = np.array([runtime.plan_bone_chain(parents, b, query_length_only=True) - 1 for b in range(TRACKS)])
    clips = [synth.build_clip(seed=7 + k) for k in range(num_clips)]        # the bench's 100-bone clip shape (synth.default_spec)
    handles = np.array([ctx.register_clip(c.blob) for c in clips], dtype=np.uint32)
    for handle in handles:
        ctx.set_clip_hierarchy(int(handle), parents)
    print("clocks before", clocks(), flush=True)
    cases = [(f"{'1 clip' if many == 0 else str(num_clips) + ' clips'}, {count:2d} {'deep' if deep else 'shallow'}", many, count, deep)
             for many in (0, 1) for count in (1, 4, 16) for deep in (False, True)]
    if os.environ.get("SOCKETS_CASE") is not None:
        cases = [cases[int(os.environ["SOCKETS_CASE"])]]
    results = []
    for name, many, count, deep in cases:
        used = clips if many else clips[:1]
        result = measure(ctx, stream, name, used, handles[:len(used)], parents, depth, 65536, count, deep, rounds, repeats, check)
        results.append(result)
        if result.get("profile_only"):
            continue
        print(f"{name:24s} requests {result['requests_us']:8.1f} us (+-{result['requests_spread'] * 100:.1f} %)  whole pose + gather {result['whole_pose_us']:8.1f} us "
              f"(+-{result['whole_pose_spread'] * 100:.1f} %)  b/a {result['whole_pose_over_requests']:.2f}  depths {result['socket_depths']}  "
              + (f"exact ({result['characters_checked_against_oracle']} characters against the oracle)" if result["checked"] else "MISMATCH"), flush=True)
    print("clocks after", clocks(), flush=True)
    under_load = sorted({sample.get("pp_dpm_sclk", "?") + " / " + sample.get("pp_dpm_mclk", "?") for sample in CLOCK_SAMPLES})
    print(f"clocks under load ({len(CLOCK_SAMPLES)} samples, sclk / mclk):", under_load, flush=True)
    print(json.dumps({"socket_requests": results}))
    rejected = ctx.rejected_instance_count()
    ctx.close()
    if rejected != 0 or not all(r["checked"] for r in results):
        print("FAILED: rejected", rejected)
        sys.exit(1)


if __name__ == "__main__":
    main()
