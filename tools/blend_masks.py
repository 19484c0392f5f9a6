#!/usr/bin/env python3
"""Measurement aid: the masked blends of skeleton space (aclhip_decompress_poses_batch_masked) against their yardsticks, HIP events on one
stream, the method of tools/skeleton_poses.py. Batch: 65 536 instances, each a blend of three 100-bone clips, QVV48, object space, into
100 slots (identity maps) and into 128 slots. Per case, interleaved over BLEND_MASKS_ROUNDS rounds of BLEND_MASKS_REPEATS launches:
  masked     (a) the masked launch, ACLHIP_BLEND_WEIGHTED and ACLHIP_BLEND_LAYERED (per instance mask handles, a third of them null)
  mapped     (b) aclhip_decompress_poses_batch_mapped on the same batch: its kernels are instruction for instruction the parent commit's
  caller     (c) what a caller does without the launch: K launches of aclhip_decompress_tracks_batch_mapped with fill into K buffers, then
             the per bone weighted accumulate (sign aligned rotations) and the normalize as torch passes over those buffers, with the per
             (instance, clip, slot) weights ALREADY in a device tensor. The object space walk is NOT in it: the library has no launch that
             walks a pose buffer, so the caller's route ends in local space and (c) is a floor under it.
Before it is timed every case is CHECKED bit for bit against the expected poses of tests/test_gpu_blend_masks.py (the oracle route) on
BLEND_MASKS_CHECK instances (default 768: the first 256 and 512 drawn at random; 0 = every instance); a mismatch or a refused instance
exits non-zero. Time is reported, never judged: median of the rounds, spread (max - min) / median, and the ratios a / b and c / a.
The clocks (sysfs, read only) are sampled UNDER LOAD: in every timed window, after its launches are enqueued and before they are waited for.
BLEND_MASKS_CASE=<index> runs one case only; BLEND_MASKS_PROFILE=1 launches only the masked and the mapped launch of it, a few times (for a
rocprofv3 --kernel-trace --stats run and, separately, a --pmc run)."""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import torch  # noqa: E402
from acl_amd import runtime, synth  # noqa: E402
from skeleton_poses import CLOCK_SAMPLES, clocks, timed  # noqa: E402  (tools/ is the script's directory)

NO_PARENT = 0xFFFFFFFF
K = 3


def measure(ctx, stream, name, clips, n, num_slots, mode, rounds, repeats, check):
    import test_gpu_blend_masks as expected_of        # the oracle route of the tests
    rng = np.random.default_rng(2000)
    tracks = clips[0].num_tracks
    parents = np.array(synth.humanoid_hierarchy(tracks), dtype=np.uint32)
    handles = np.array([ctx.register_clip(c.blob) for c in clips], dtype=np.uint32)
    table = np.arange(tracks, dtype=np.uint32) if num_slots == tracks else np.sort(rng.choice(num_slots, size=tracks, replace=False)).astype(np.uint32)
    slot_parents = np.full(num_slots, NO_PARENT, dtype=np.uint32)
    slot_parents[table[1:]] = table[parents[1:]]
    reference = np.zeros((num_slots, 12), dtype=np.float32)
    reference[:, 0:4] = [0.5, 0.5, 0.5, 0.5]
    reference[:, 4:7] = rng.uniform(-1.0, 1.0, size=(num_slots, 3))
    reference[:, 8:11] = 1.0
    skeleton = ctx.register_skeleton(slot_parents, reference)
    track_map = ctx.register_track_map(table, num_slots)
    # an "upper body" mask, its complement above a floor, and two random ones; weighted mode keeps clip 0's mask >= 0.25, layered mode e_0 == 1
    masks = [np.where(np.arange(num_slots) < num_slots // 2, 1.0, 0.0), np.where(np.arange(num_slots) < num_slots // 2, 0.25, 1.0),
             rng.uniform(0.25, 1.0, size=num_slots), rng.uniform(0.0, 1.0, size=num_slots)]
    masks = [m.astype(np.float32) for m in masks]
    mask_handles = np.array([0] + [ctx.register_blend_mask(m) for m in masks], dtype=np.uint32)
    which = rng.choice([0, 0, 1, 2, 3, 4], size=(n, K))
    which[:, 0] = rng.choice([0, 2, 3], size=n) if mode == runtime.BLEND_WEIGHTED else 0
    weights = rng.dirichlet(np.ones(K), size=n).astype(np.float32) if mode == runtime.BLEND_WEIGHTED else rng.uniform(0.0, 1.0, size=(n, K)).astype(np.float32)
    if mode == runtime.BLEND_LAYERED:
        weights[:, 0] = 1.0
    times = rng.uniform(0.0, clips[0].duration, size=n).astype(np.float32)
    other_times = rng.uniform(0.0, min(c.duration for c in clips), size=(n, K - 1)).astype(np.float32)
    stride = num_slots * 48
    with torch.cuda.stream(stream):
        def up(array, dtype):
            return torch.from_numpy(np.ascontiguousarray(array, dtype=dtype).view(np.int32 if dtype == np.uint32 else dtype)).cuda()
        d_clips, d_times = up(np.full(n, handles[0]), np.uint32), up(times, np.float32)
        d_other_clips, d_other_times = up(np.tile(handles[1:K], (n, 1)), np.uint32), up(other_times, np.float32)
        d_weights, d_maps, d_masks = up(weights, np.float32), up(np.full((n, K - 1), track_map), np.uint32), up(mask_handles[which], np.uint32)
        poses = torch.zeros((n, stride // 4), dtype=torch.float32, device="cuda")
        poses_mapped = torch.zeros((n, stride // 4), dtype=torch.float32, device="cuda")
        caller_buffers = [torch.zeros((n, num_slots, 12), dtype=torch.float32, device="cuda") for _ in range(K)]
        fill_pose = up(reference, np.float32)
        # (c)'s weights, ready on the device: [K, n, num_slots, 1]
        mask_table = np.stack([np.ones(num_slots, dtype=np.float32)] + masks)
        per_slot = np.stack([weights[:, k, None] * mask_table[which[:, k]] for k in range(K)])
        if mode == runtime.BLEND_LAYERED:
            per_slot = np.stack([per_slot[k] * np.prod([1.0 - per_slot[j] for j in range(K - 1, k, -1)] or [np.ones_like(per_slot[k])], axis=0) for k in range(K)])
        d_per_slot = up(per_slot[..., None], np.float32)
    s = stream.cuda_stream
    consumers, mapping, masking = runtime.PoseConsumers(), runtime.PoseMapping(), runtime.BlendMasking()
    consumers.object_space, consumers.num_blend_clips = 1, K
    consumers.blend_clips, consumers.blend_sample_times, consumers.blend_weights = d_other_clips.data_ptr(), d_other_times.data_ptr(), d_weights.data_ptr()
    mapping.skeleton, mapping.map, mapping.blend_maps = skeleton, track_map, d_maps.data_ptr()
    masking.mode, masking.instance_masks = mode, d_masks.data_ptr()

    def masked():
        ctx.decompress_poses_batch_masked(d_clips.data_ptr(), d_times.data_ptr(), n, poses.data_ptr(), stride, consumers, mapping, masking, stream=s)

    def mapped():
        ctx.decompress_poses_batch_mapped(d_clips.data_ptr(), d_times.data_ptr(), n, poses_mapped.data_ptr(), stride, consumers, mapping, stream=s)

    caller_inputs = [(d_clips, d_times)] + [(d_other_clips[:, k].contiguous(), d_other_times[:, k].contiguous()) for k in range(K - 1)]

    def caller():
        for (clip_ids, clip_times), target in zip(caller_inputs, caller_buffers):
            ctx.decompress_tracks_batch_mapped(clip_ids, clip_times, target, stride, track_map=track_map, fill_pose=fill_pose, stream=s)
        with torch.cuda.stream(stream):
            total = caller_buffers[0] * d_per_slot[0]
            for k in range(1, K):
                dot = (total[..., 0:4] * caller_buffers[k][..., 0:4]).sum(dim=-1, keepdim=True)
                signed = torch.where(dot < 0, -d_per_slot[k], d_per_slot[k])
                total[..., 0:4] += caller_buffers[k][..., 0:4] * signed
                total[..., 4:12] += caller_buffers[k][..., 4:12] * d_per_slot[k]
            total[..., 0:4] /= torch.linalg.vector_norm(total[..., 0:4], dim=-1, keepdim=True)
        return total

    def release():
        for handle in mask_handles[1:]:
            ctx.unregister_blend_mask(int(handle))
        ctx.unregister_skeleton(skeleton)
        ctx.unregister_track_map(track_map)
        for handle in handles:
            ctx.unregister_clip(int(handle))

    if os.environ.get("BLEND_MASKS_PROFILE") == "1":
        for _ in range(5):
            masked()
            mapped()
        stream.synchronize()
        release()
        return {"case": name, "checked": True, "profile_only": True}

    masked()
    stream.synchronize()
    got = poses.cpu().numpy().reshape(n, num_slots, 12)
    sample = np.arange(n) if check == 0 else np.unique(np.concatenate([np.arange(min(n, 256)), np.random.default_rng(7).choice(n, size=min(n, check - 256), replace=False)]))
    ok = True
    for i in sample:
        members = [(clips[0].blob, times[i], table)] + [(clips[k].blob, other_times[i, k - 1], table) for k in range(1, K)]
        expected = expected_of.expected_masked_pose((reference, slot_parents), members, weights[i], [None if m == 0 else mask_table[m] for m in which[i]], mode,
                                                    runtime.ADDITIVE_NONE, None, True, 0, 2)
        if not np.isfinite(expected).all() or not np.array_equal(got[i].view(np.uint32), expected.view(np.uint32)):
            print(f"MISMATCH: case {name!r}, instance {i}", flush=True)
            ok = False
            break
    for step in (masked, mapped, caller):
        for _ in range(10):
            step()
    samples = {"masked": [], "mapped": [], "caller": []}
    for _ in range(rounds):
        samples["masked"].append(timed(stream, masked, repeats))
        samples["mapped"].append(timed(stream, mapped, repeats))
        samples["caller"].append(timed(stream, caller, max(1, repeats // 10)))
    result = {"case": name, "mode": "layered" if mode == runtime.BLEND_LAYERED else "weighted", "instances": n, "tracks": tracks, "num_slots": num_slots,
              "clips_per_instance": K, "checked": bool(ok), "instances_checked": int(len(sample))}
    for key, values in samples.items():
        median = float(np.median(values))
        result[key + "_us"] = round(median, 2)
        result[key + "_spread"] = round(float((max(values) - min(values)) / median), 4)
    result["masked_over_mapped"] = round(result["masked_us"] / result["mapped_us"], 4)
    result["caller_over_masked"] = round(result["caller_us"] / result["masked_us"], 4)
    release()
    return result


def main():
    rounds = int(os.environ.get("BLEND_MASKS_ROUNDS", "7"))
    repeats = int(os.environ.get("BLEND_MASKS_REPEATS", "100"))
    check = int(os.environ.get("BLEND_MASKS_CHECK", "768"))
    ctx = runtime.Context(0)
    stream = torch.cuda.Stream()
    clips = [synth.build_clip(seed=seed) for seed in (7, 8, 9)]        # the bench's 100-bone clip shape (synth.default_spec), three of them
    print("clocks before", clocks(), flush=True)
    cases = [("weighted 100 -> 100", 100, runtime.BLEND_WEIGHTED), ("layered 100 -> 100", 100, runtime.BLEND_LAYERED),
             ("weighted 100 -> 128", 128, runtime.BLEND_WEIGHTED), ("layered 100 -> 128", 128, runtime.BLEND_LAYERED)]
    if os.environ.get("BLEND_MASKS_CASE") is not None:
        cases = [cases[int(os.environ["BLEND_MASKS_CASE"])]]
    results = []
    for name, num_slots, mode in cases:
        result = measure(ctx, stream, name, clips, 65536, num_slots, mode, rounds, repeats, check)
        results.append(result)
        if result.get("profile_only"):
            continue
        print(f"{name:22s} masked {result['masked_us']:8.1f} us (+-{result['masked_spread'] * 100:.1f} %)  mapped {result['mapped_us']:8.1f} us (+-{result['mapped_spread'] * 100:.1f} %)  "
              f"a/b {result['masked_over_mapped']:.3f}  caller (no walk) {result['caller_us']:9.1f} us (+-{result['caller_spread'] * 100:.1f} %)  c/a {result['caller_over_masked']:.2f}  "
              + (f"exact on {result['instances_checked']}" if result["checked"] else "MISMATCH"), flush=True)
    print("clocks after", clocks(), flush=True)
    under_load = sorted({sample.get("pp_dpm_sclk", "?") + " / " + sample.get("pp_dpm_mclk", "?") for sample in CLOCK_SAMPLES})
    print(f"clocks under load ({len(CLOCK_SAMPLES)} samples, sclk / mclk):", under_load, flush=True)
    print(json.dumps({"blend_masks": results}))
    rejected = ctx.rejected_instance_count()
    ctx.close()
    if rejected != 0 or not all(r["checked"] for r in results):
        print("FAILED: rejected", rejected)
        sys.exit(1)


if __name__ == "__main__":
    main()
