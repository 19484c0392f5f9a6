#!/usr/bin/env python3
"""Measurement aid: the additive layer at a strength per (instance, slot) (aclhip_decompress_poses_batch_additive_weighted) against its
yardsticks, HIP events on one stream, the method of tools/blend_masks.py. Batch: 65 536 instances x 100 bones, additive1 onto a base clip,
QVV48, object space, identity maps. Interleaved over ADDITIVE_STRENGTH_ROUNDS rounds of ADDITIVE_STRENGTH_REPEATS launches:
  weighted   (a) the new launch with a weight array and an upper-body mask (a third of the handles null)
  mapped     (b) aclhip_decompress_poses_batch_mapped on the same batch (full strength): its kernels are the parent commit's
  caller     (c) a caller's route today: two launches of aclhip_decompress_tracks_batch_mapped with fill (the additive clip over the additive
             identity, the base clip over the reference pose) into two row buffers, then the weighting and transform_add1 as torch passes
             with the per (instance, slot) strengths ALREADY in a device tensor. The object space walk is NOT in it: the library has no
             launch that walks a pose buffer, so the caller's route ends in local space and (c) is a floor under it.
Before anything is timed (a) and (b) are CHECKED bit for bit against the expected rows of tests/test_gpu_additive_strength.py (the oracle
route) on ADDITIVE_STRENGTH_CHECK instances (default 768: the first 256 and 512 drawn at random; 0 = every instance) and (c) against (a)'s
local space rows within 1e-5 (torch's arithmetic is not the definition's); a mismatch or a refused instance exits non-zero. Time is
reported, never judged: median of the rounds, spread (max - min) / median, and the ratios a / b and c / a. The clocks (sysfs, read only) are
sampled UNDER LOAD. ADDITIVE_STRENGTH_PROFILE=1 launches only (a) and (b), a few times (for a rocprofv3 --kernel-trace --stats run and,
separately, a --pmc run)."""
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

ADDITIVE1 = runtime.ADDITIVE_ADDITIVE1


def quat_mul(lhs, rhs):
    """rtm::quat_mul(lhs, rhs) on [..., 4] tensors (x, y, z, w)"""
    lx, ly, lz, lw = lhs.unbind(-1)
    rx, ry, rz, rw = rhs.unbind(-1)
    return torch.stack([rw * lx + rx * lw + ry * lz - rz * ly, rw * ly - rx * lz + ry * lw + rz * lx, rw * lz + rx * ly - ry * lx + rz * lw,
                        rw * lw - rx * lx - ry * ly - rz * lz], dim=-1)


def main():
    import test_gpu_additive_strength as expected_of        # the oracle route of the tests
    rounds = int(os.environ.get("ADDITIVE_STRENGTH_ROUNDS", "7"))
    repeats = int(os.environ.get("ADDITIVE_STRENGTH_REPEATS", "100"))
    check = int(os.environ.get("ADDITIVE_STRENGTH_CHECK", "768"))
    n, num_bones = 65536, 100
    ctx = runtime.Context(0)
    stream = torch.cuda.Stream()
    rng = np.random.default_rng(3000)
    additive, base = synth.build_clip(seed=7), synth.build_clip(seed=8)        # the bench's 100-bone clip shape (synth.default_spec)
    parents = np.array(synth.humanoid_hierarchy(num_bones), dtype=np.uint32)
    reference = np.zeros((num_bones, 12), dtype=np.float32)
    reference[:, 0:4] = [0.5, 0.5, 0.5, 0.5]
    reference[:, 4:7] = rng.uniform(-1.0, 1.0, size=(num_bones, 3))
    reference[:, 8:11] = 1.0
    table = np.arange(num_bones, dtype=np.uint32)
    h_additive, h_base = ctx.register_clip(additive.blob), ctx.register_clip(base.blob)
    skeleton, track_map = ctx.register_skeleton(parents, reference), ctx.register_track_map(table, num_bones)
    upper_body = np.where(np.arange(num_bones) < num_bones // 2, 1.0, 0.0).astype(np.float32)
    mask = ctx.register_blend_mask(upper_body)
    weights = rng.uniform(0.0, 1.0, size=n).astype(np.float32)
    handles = rng.choice([0, mask, mask], size=n).astype(np.uint32)
    times = rng.uniform(0.0, additive.duration, size=n).astype(np.float32)
    base_times = rng.uniform(0.0, base.duration, size=n).astype(np.float32)
    stride = num_bones * 48
    print("clocks before", clocks(), flush=True)
    with torch.cuda.stream(stream):
        def up(array, dtype):
            return torch.from_numpy(np.ascontiguousarray(array, dtype=dtype).view(np.int32 if dtype == np.uint32 else dtype)).cuda()
        d_clips, d_times = up(np.full(n, h_additive), np.uint32), up(times, np.float32)
        d_base_clips, d_base_times, d_base_maps = up(np.full(n, h_base), np.uint32), up(base_times, np.float32), up(np.full(n, track_map), np.uint32)
        d_weights, d_handles = up(weights, np.float32), up(handles, np.uint32)
        poses = torch.zeros((n, num_bones, 12), dtype=torch.float32, device="cuda")
        poses_mapped = torch.zeros((n, num_bones, 12), dtype=torch.float32, device="cuda")
        caller_additive = torch.zeros((n, num_bones, 12), dtype=torch.float32, device="cuda")
        caller_base = torch.zeros((n, num_bones, 12), dtype=torch.float32, device="cuda")
        identity = expected_of.sk.additive_identity(num_bones, ADDITIVE1)
        d_identity, d_reference = up(identity, np.float32), up(reference, np.float32)
        # (c)'s strengths, ready on the device: [n, num_bones, 1]
        strength = np.where(handles[:, None] == 0, weights[:, None], weights[:, None] * upper_body[None, :]).astype(np.float32)
        d_strength = up(strength[..., None], np.float32)
    s = stream.cuda_stream
    consumers, mapping, layering = runtime.PoseConsumers(), runtime.PoseMapping(), runtime.AdditiveLayering()
    consumers.additive_format, consumers.object_space = ADDITIVE1, 1
    consumers.base_clips, consumers.base_sample_times = d_base_clips.data_ptr(), d_base_times.data_ptr()
    mapping.skeleton, mapping.map, mapping.base_maps = skeleton, track_map, d_base_maps.data_ptr()
    layering.instance_weights, layering.instance_masks = d_weights.data_ptr(), d_handles.data_ptr()

    def weighted():
        ctx.decompress_poses_batch_additive_weighted(d_clips.data_ptr(), d_times.data_ptr(), n, poses.data_ptr(), stride, consumers, mapping, layering, stream=s)

    def mapped():
        ctx.decompress_poses_batch_mapped(d_clips.data_ptr(), d_times.data_ptr(), n, poses_mapped.data_ptr(), stride, consumers, mapping, stream=s)

    def caller():
        ctx.decompress_tracks_batch_mapped(d_clips, d_times, caller_additive, stride, track_map=track_map, fill_pose=d_identity, stream=s)
        ctx.decompress_tracks_batch_mapped(d_base_clips, d_base_times, caller_base, stride, track_map=track_map, fill_pose=d_reference, stream=s)
        with torch.cuda.stream(stream):
            rest = 1.0 - d_strength
            rotation = caller_additive[..., 0:4] * torch.where(caller_additive[..., 3:4] * rest < 0, -d_strength, d_strength)      # (dot with I * u)
            rotation[..., 3:4] += rest
            rotation /= torch.linalg.vector_norm(rotation, dim=-1, keepdim=True)
            out = torch.empty_like(caller_base)
            out[..., 0:4] = quat_mul(rotation, caller_base[..., 0:4])
            out[..., 4:8] = caller_additive[..., 4:8] * d_strength + caller_base[..., 4:8]
            out[..., 8:12] = (1.0 + caller_additive[..., 8:12] * d_strength) * caller_base[..., 8:12]       # transform_add1, identity scale 0
        return out

    if os.environ.get("ADDITIVE_STRENGTH_PROFILE") == "1":
        for _ in range(5):
            weighted()
            mapped()
        stream.synchronize()
        print(json.dumps({"additive_strength": {"profile_only": True}}))
        ctx.close()
        return

    # every timed case is checked first
    weighted()
    mapped()
    stream.synchronize()
    got, got_mapped = poses.cpu().numpy(), poses_mapped.cpu().numpy()
    sample = np.arange(n) if check == 0 else np.unique(np.concatenate([np.arange(min(n, 256)), np.random.default_rng(7).choice(n, size=min(n, max(check - 256, 1)), replace=False)]))
    ok = True
    for i in sample:
        members, the_base = [(additive.blob, times[i], table)], (base.blob, base_times[i], table)
        row = expected_of.expected_row((reference, parents), members, None, strength[i], ADDITIVE1, the_base, True)
        full = expected_of.expected_row((reference, parents), members, None, None, ADDITIVE1, the_base, True)
        if not np.array_equal(got[i].view(np.uint32), row.view(np.uint32)) or not np.array_equal(got_mapped[i].view(np.uint32), full.view(np.uint32)):
            print(f"MISMATCH: instance {i}", flush=True)
            ok = False
            break
    consumers.object_space = 0
    weighted()
    local = caller()
    stream.synchronize()
    caller_error = float((local - poses).abs().max().item())
    consumers.object_space = 1
    if not caller_error <= 1.0e-5:
        print(f"MISMATCH: the caller's route differs from the launch's local space rows by {caller_error}", flush=True)
        ok = False

    for step in (weighted, mapped, caller):
        for _ in range(10):
            step()
    samples = {"weighted": [], "mapped": [], "caller": []}
    for _ in range(rounds):
        samples["weighted"].append(timed(stream, weighted, repeats))
        samples["mapped"].append(timed(stream, mapped, repeats))
        samples["caller"].append(timed(stream, caller, max(1, repeats // 10)))
    result = {"instances": n, "bones": num_bones, "additive_format": "additive1", "base": "clip", "object_space": True, "checked": bool(ok),
              "instances_checked": int(len(sample)), "caller_max_abs_error_local": caller_error}
    for key, values in samples.items():
        median = float(np.median(values))
        result[key + "_us"] = round(median, 2)
        result[key + "_spread"] = round(float((max(values) - min(values)) / median), 4)
    result["weighted_over_mapped"] = round(result["weighted_us"] / result["mapped_us"], 4)
    result["caller_over_weighted"] = round(result["caller_us"] / result["weighted_us"], 4)
    print(f"weighted {result['weighted_us']:8.1f} us (+-{result['weighted_spread'] * 100:.1f} %)  mapped {result['mapped_us']:8.1f} us (+-{result['mapped_spread'] * 100:.1f} %)  "
          f"a/b {result['weighted_over_mapped']:.3f}  caller (no walk) {result['caller_us']:9.1f} us (+-{result['caller_spread'] * 100:.1f} %)  c/a {result['caller_over_weighted']:.2f}  "
          + (f"exact on {result['instances_checked']}" if ok else "MISMATCH"), flush=True)
    print("clocks after", clocks(), flush=True)
    under_load = sorted({sample.get("pp_dpm_sclk", "?") + " / " + sample.get("pp_dpm_mclk", "?") for sample in CLOCK_SAMPLES})
    print(f"clocks under load ({len(CLOCK_SAMPLES)} samples, sclk / mclk):", under_load, flush=True)
    print(json.dumps({"additive_strength": result}))
    rejected = ctx.rejected_instance_count()
    ctx.close()
    if rejected != 0 or not ok:
        print("FAILED: rejected", rejected)
        sys.exit(1)


if __name__ == "__main__":
    main()
