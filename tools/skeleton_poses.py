#!/usr/bin/env python3
"""Measurement aid: the pose consumers in skeleton space (aclhip_decompress_poses_batch_mapped) against their two yardsticks, HIP events
on one stream, the method of tools/mapped_decode.py. Batch: 65 536 instances of 100-bone clips, QVV48. Per case, interleaved over
SKELETON_ROUNDS rounds of SKELETON_REPEATS launches:
  fused      the skeleton space launch
  unmapped   aclhip_decompress_poses_batch on the same batch (clips of equal shape, rows of 100 records): what the mapping costs
  floor      K launches of aclhip_decompress_tracks_batch_mapped with fill into K buffers: only the FIRST step of what a caller does today
             (the blend, apply and walk passes over HBM are not in it), so a floor under today's cost. K = 1 (object space) and K = 3
             (blend) only: the additive1 case has no floor
Cases: object space | additive1 onto a base clip + object space | blend of three + object space, each with identity maps (B == T == 100),
and object space and the blend of three into 128 slots. Before it is timed every case gets a SANITY check, no more: the mapped slots of the
fused result equal the unmapped launch's poses bit for bit (under the hierarchy carried over to slot space), and without a blend the other
slots hold the reference pose. It is not a comparison with the caller's whole route (mapped decodes plus blend, apply and walk passes), which
this tool does not build; tests/test_gpu_skeleton_poses.py holds the launch to the oracle.
Reports the median of the rounds and their spread ((max - min) / median). Exits non-zero when a check fails, or when a fused launch of the
object space (K = 1) or blend (K = 3) cases does not come in below its floor by more than the larger of the two spreads.
The clocks (sysfs, read only) are sampled UNDER LOAD: in every timed window, after its launches are enqueued and before they are waited for.
SKELETON_CASE=<index> runs one case only; SKELETON_PROFILE=1 launches only the fused and the unmapped launch of it, a few times (for a
rocprofv3 --kernel-trace --stats run and, separately, a --pmc run)."""
import glob
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402
from acl_amd import runtime, synth  # noqa: E402

NO_PARENT = 0xFFFFFFFF


def clocks():
    out = {}
    for card in glob.glob("/sys/class/drm/card*/device"):
        for name in ("pp_dpm_sclk", "pp_dpm_mclk"):
            try:
                active = [line for line in open(os.path.join(card, name)).read().splitlines() if line.endswith("*")]
            except OSError:
                continue
            if active:
                out[name] = active[0]
        if out:
            break
    return out


CLOCK_SAMPLES = []


def timed(stream, step, repeats):
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record(stream)
    for _ in range(repeats):
        step()
    stop.record(stream)
    CLOCK_SAMPLES.append(clocks())        # (the launches above are still running)
    stop.synchronize()
    return start.elapsed_time(stop) / repeats * 1000.0


def measure(ctx, stream, name, clips, n, num_slots, kind, rounds, repeats):
    """kind: 'object' (K = 1), 'additive1' (the second clip is the base), 'blend3'"""
    rng = np.random.default_rng(1000)
    tracks = clips[0].num_tracks
    parents = np.array(synth.humanoid_hierarchy(tracks), dtype=np.uint32)
    handles = [ctx.register_clip(c.blob) for c in clips]
    for handle in handles:
        ctx.set_clip_hierarchy(handle, parents)
    table = np.arange(tracks, dtype=np.uint32) if num_slots == tracks else np.sort(rng.choice(num_slots, size=tracks, replace=False)).astype(np.uint32)
    # the hierarchy in slot space: a mapped slot's parent is its track's parent's slot, every other slot is a root
    slot_parents = np.full(num_slots, NO_PARENT, dtype=np.uint32)
    slot_parents[table[1:]] = table[parents[1:]]
    reference = np.zeros((num_slots, 12), dtype=np.float32)
    reference[:, 0:4] = [0.5, 0.5, 0.5, 0.5]
    reference[:, 4:7] = rng.uniform(-1.0, 1.0, size=(num_slots, 3))
    reference[:, 8:11] = 1.0
    skeleton = ctx.register_skeleton(slot_parents, reference)
    track_map = ctx.register_track_map(table, num_slots)
    stride, unmapped_stride = num_slots * 48, tracks * 48
    num_clips = 3 if kind == "blend3" else 1
    with torch.cuda.stream(stream):
        def up(array, dtype):
            return torch.from_numpy(np.ascontiguousarray(array, dtype=dtype).view(np.int32 if dtype == np.uint32 else dtype)).cuda()
        d_clips = up(np.full(n, handles[0]), np.uint32)
        d_times = up(rng.uniform(0.0, clips[0].duration, size=n), np.float32)
        d_other_clips = up(np.tile(np.array(handles[1:3]), (n, 1)), np.uint32)
        d_other_times = up(rng.uniform(0.0, min(c.duration for c in clips), size=(n, 2)), np.float32)
        d_weights = up(rng.dirichlet(np.ones(3), size=n), np.float32)
        d_maps = up(np.full((n, 2), track_map), np.uint32)
        poses = torch.zeros((n, stride // 4), dtype=torch.float32, device="cuda")
        poses_unmapped = torch.zeros((n, unmapped_stride // 4), dtype=torch.float32, device="cuda")
        floor_buffers = [torch.zeros((n, stride // 4), dtype=torch.float32, device="cuda") for _ in range(num_clips)]
        fill_pose = up(reference, np.float32)
    s = stream.cuda_stream
    consumers, mapping = runtime.PoseConsumers(), runtime.PoseMapping()
    consumers.object_space = 1
    mapping.skeleton, mapping.map = skeleton, track_map
    if kind == "additive1":
        consumers.additive_format = runtime.ADDITIVE_ADDITIVE1
        base_inputs = (d_other_clips[:, 0].contiguous(), d_other_times[:, 0].contiguous(), d_maps[:, 0].contiguous())        # (kept alive by this tuple)
        consumers.base_clips, consumers.base_sample_times, mapping.base_maps = (tensor.data_ptr() for tensor in base_inputs)
    if kind == "blend3":
        consumers.num_blend_clips = 3
        consumers.blend_clips, consumers.blend_sample_times, consumers.blend_weights = d_other_clips.data_ptr(), d_other_times.data_ptr(), d_weights.data_ptr()
        mapping.blend_maps = d_maps.data_ptr()

    def fused():
        ctx.decompress_poses_batch_mapped(d_clips.data_ptr(), d_times.data_ptr(), n, poses.data_ptr(), stride, consumers, mapping, stream=s)

    def unmapped():
        ctx.decompress_poses_batch(d_clips.data_ptr(), d_times.data_ptr(), n, poses_unmapped.data_ptr(), unmapped_stride, consumers, stream=s)

    floor_inputs = [(d_clips, d_times)] + [(d_other_clips[:, k].contiguous(), d_other_times[:, k].contiguous()) for k in range(num_clips - 1)]

    has_floor = kind in ("object", "blend3")

    def floor():
        for (clip_ids, times), target in zip(floor_inputs, floor_buffers):
            ctx.decompress_tracks_batch_mapped(clip_ids, times, target, stride, track_map=track_map, fill_pose=fill_pose, stream=s)

    def release():
        ctx.unregister_skeleton(skeleton)
        ctx.unregister_track_map(track_map)
        for handle in handles:
            ctx.unregister_clip(handle)

    if os.environ.get("SKELETON_PROFILE") == "1":
        for _ in range(5):
            fused()
            unmapped()
        stream.synchronize()
        release()
        return {"case": name, "checked": True, "below_floor_beyond_spread": True, "profile_only": True}
    fused()
    unmapped()
    stream.synchronize()
    got = poses.view(torch.int32).view(n, num_slots, 12)
    d_table = torch.from_numpy(table.astype(np.int64)).cuda()
    ok = torch.equal(got[:, d_table], poses_unmapped.view(torch.int32).view(n, tracks, 12))
    others = torch.from_numpy(np.setdiff1d(np.arange(num_slots), table).astype(np.int64)).cuda()
    if others.numel() != 0 and kind != "blend3":        # (a blend of three reference transforms is normalized again: not the reference's bits)
        ok = ok and torch.equal(got[:, others], fill_pose.view(torch.int32)[others].unsqueeze(0).expand(n, -1, -1))
    for step in (fused, unmapped) + ((floor,) if has_floor else ()):
        for _ in range(10):
            step()
    samples = {"fused": [], "unmapped": []}
    if has_floor:
        samples["floor"] = []
    for _ in range(rounds):
        samples["fused"].append(timed(stream, fused, repeats))
        samples["unmapped"].append(timed(stream, unmapped, repeats))
        if has_floor:
            samples["floor"].append(timed(stream, floor, repeats))
    result = {"case": name, "instances": n, "tracks": tracks, "num_slots": num_slots, "clips_per_instance": num_clips, "checked": bool(ok)}
    for key, values in samples.items():
        median = float(np.median(values))
        result[key + "_us"] = round(median, 2)
        result[key + "_spread"] = round(float((max(values) - min(values)) / median), 4)
    result["fused_over_unmapped"] = round(result["fused_us"] / result["unmapped_us"], 4)
    result["floor_applies"] = has_floor
    if has_floor:
        result["floor_over_fused"] = round(result["floor_us"] / result["fused_us"], 4)
        result["below_floor_beyond_spread"] = bool(result["floor_us"] - result["fused_us"] > max(result["fused_spread"], result["floor_spread"]) * result["floor_us"])
    release()
    return result


def main():
    rounds = int(os.environ.get("SKELETON_ROUNDS", "7"))
    repeats = int(os.environ.get("SKELETON_REPEATS", "200"))
    ctx = runtime.Context(0)
    stream = torch.cuda.Stream()
    clips = [synth.build_clip(seed=seed) for seed in (7, 8, 9)]        # the bench's 100-bone clip shape (synth.default_spec), three of them
    print("clocks before", clocks(), flush=True)
    cases = [
        ("object space 100 -> 100", 100, "object"),
        ("additive1 + object space 100 -> 100", 100, "additive1"),
        ("blend of three + object space 100 -> 100", 100, "blend3"),
        ("object space 100 -> 128", 128, "object"),
        ("blend of three + object space 100 -> 128", 128, "blend3"),
    ]
    if os.environ.get("SKELETON_CASE") is not None:
        cases = [cases[int(os.environ["SKELETON_CASE"])]]
    results = []
    for name, num_slots, kind in cases:
        result = measure(ctx, stream, name, clips, 65536, num_slots, kind, rounds, repeats)
        results.append(result)
        if result.get("profile_only"):
            continue
        floor_text = (f"floor {result['floor_us']:8.1f} us (+-{result['floor_spread'] * 100:.1f} %)  floor/fused {result['floor_over_fused']:.2f}" if result["floor_applies"]
                      else "floor        -")
        print(f"{name:44s} fused {result['fused_us']:8.1f} us (+-{result['fused_spread'] * 100:.1f} %)  unmapped {result['unmapped_us']:8.1f} us  fused/unmapped {result['fused_over_unmapped']:.3f}  "
              f"{floor_text}  " + ("sane" if result["checked"] else "MISMATCH"), flush=True)
    print("clocks after", clocks(), flush=True)
    under_load = sorted({sample.get("pp_dpm_sclk", "?") + " / " + sample.get("pp_dpm_mclk", "?") for sample in CLOCK_SAMPLES})
    print(f"clocks under load ({len(CLOCK_SAMPLES)} samples, sclk / mclk):", under_load, flush=True)
    print(json.dumps({"skeleton_poses": results}))
    rejected = ctx.rejected_instance_count()
    ctx.close()
    if rejected != 0 or not all(r["checked"] for r in results):
        print("FAILED: rejected", rejected)
        sys.exit(1)
    losers = [r["case"] for r in results if r.get("floor_applies") and not r["below_floor_beyond_spread"]]
    if losers:
        print("FAILED: not below K mapped decodes by more than the spread:", losers)
        sys.exit(2)


if __name__ == "__main__":
    main()
