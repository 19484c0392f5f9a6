#!/usr/bin/env python3
"""Measurement aid: the mapped decode (aclhip_decompress_tracks_batch_mapped) against its two yardsticks, HIP events on one stream.
Batch: BASELINE.json configs[1] -- 65 536 instances of the 100-bone clip, QVV48 -- in rows of num_slots records (stride a multiple of 64
bytes). Cases: identity (100 slots), order-preserving into 128 slots with and without fill, a random permutation into 128 slots, and
the 300-bone rig order-preserving into 320 slots (16 384 instances). Per case, interleaved over MAPPED_ROUNDS rounds of MAPPED_REPEATS launches:
  mapped     the fused launch
  unmapped   aclhip_decompress_tracks_batch_out on the same batch and stride (records in track order: what the mapping costs)
  two_pass   what a caller does without track maps: that unmapped decode into a scratch buffer, then ONE pass that scatters record t of
             the scratch row to record table[t] of the pose row (torch index_copy_ on the record axis: no temporary, unmapped slots are
             not touched), plus a copy of the fill records where the case has fill
Reports the median of the rounds and their spread ((max - min) / median). Every case is first checked: mapped == two_pass, bit for bit.
Exits non-zero when a check fails or a mapped case does not beat its two-pass yardstick by more than the spread.
The clocks (sysfs, read only) are sampled UNDER LOAD: in every timed window, after its launches are enqueued and before they are waited for.
MAPPED_CASE=<index> runs one case only; MAPPED_PROFILE=1 launches only the mapped and the unmapped decode of it, a few times (for a
rocprofv3 --kernel-trace --stats run and, separately, a --pmc run)."""
import glob
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402
from acl_amd import runtime, synth  # noqa: E402


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


def measure(ctx, stream, name, clip, n, table, num_slots, fill, rounds, repeats):
    handle = ctx.register_clip(clip.blob)
    tracks = clip.num_tracks
    track_map = ctx.register_track_map(table, num_slots)
    stride = (num_slots * 48 + 63) // 64 * 64
    rng = np.random.default_rng(1000)
    with torch.cuda.stream(stream):
        d_clips = torch.full((n,), handle, dtype=torch.int32, device="cuda")
        d_times = torch.from_numpy(rng.uniform(0.0, clip.duration, size=n).astype(np.float32)).cuda()
        poses, poses2, scratch = (torch.zeros((n, stride // 4), dtype=torch.float32, device="cuda") for _ in range(3))
        fill_pose = torch.from_numpy(rng.uniform(-1.0, 1.0, size=(num_slots, 12)).astype(np.float32)).cuda()
        d_table = torch.from_numpy(table.astype(np.int64)).cuda()            # track -> slot
        unmapped = torch.from_numpy(np.setdiff1d(np.arange(num_slots), table).astype(np.int64)).cuda()
        fill_records = fill_pose[unmapped].unsqueeze(0).expand(n, -1, -1)
    s = stream.cuda_stream
    output = runtime.OutputDesc()

    def mapped():
        ctx.decompress_tracks_batch_mapped(d_clips, d_times, poses, stride, track_map=track_map, fill_pose=fill_pose if fill else None, stream=s)

    def unmapped_decode(target=scratch):
        ctx.decompress_tracks_batch_out(d_clips.data_ptr(), d_times.data_ptr(), n, target.data_ptr(), stride, output, stream=s)

    records2 = poses2[:, : num_slots * 12].view(n, num_slots, 12)
    scratch_records = scratch[:, : tracks * 12].view(n, tracks, 12)

    def two_pass():
        unmapped_decode()
        with torch.cuda.stream(stream):
            records2.index_copy_(1, d_table, scratch_records)
            if fill and unmapped.numel() != 0:
                records2.index_copy_(1, unmapped, fill_records)

    if os.environ.get("MAPPED_PROFILE") == "1":
        for _ in range(5):
            mapped()
            unmapped_decode()
        stream.synchronize()
        ctx.unregister_track_map(track_map)
        ctx.unregister_clip(handle)
        return {"case": name, "checked": True, "beats_two_pass_beyond_spread": True, "profile_only": True}
    mapped()
    two_pass()
    stream.synchronize()
    ok = torch.equal(poses.view(torch.int32), poses2.view(torch.int32))
    for step in (mapped, two_pass, unmapped_decode):
        for _ in range(10):
            step()
    samples = {"mapped": [], "two_pass": [], "unmapped": []}
    for _ in range(rounds):
        samples["mapped"].append(timed(stream, mapped, repeats))
        samples["two_pass"].append(timed(stream, two_pass, repeats))
        samples["unmapped"].append(timed(stream, unmapped_decode, repeats))
    result = {"case": name, "instances": n, "tracks": tracks, "num_slots": num_slots, "stride": stride, "fill": bool(fill), "checked": bool(ok)}
    for key, values in samples.items():
        median = float(np.median(values))
        result[key + "_us"] = round(median, 2)
        result[key + "_spread"] = round(float((max(values) - min(values)) / median), 4)
    result["mapped_over_unmapped"] = round(result["mapped_us"] / result["unmapped_us"], 4)
    result["two_pass_over_mapped"] = round(result["two_pass_us"] / result["mapped_us"], 4)
    result["beats_two_pass_beyond_spread"] = bool(result["two_pass_us"] - result["mapped_us"] > max(result["mapped_spread"], result["two_pass_spread"]) * result["two_pass_us"])
    ctx.unregister_track_map(track_map)
    ctx.unregister_clip(handle)
    return result


def main():
    rounds = int(os.environ.get("MAPPED_ROUNDS", "7"))
    repeats = int(os.environ.get("MAPPED_REPEATS", "300"))
    ctx = runtime.Context(0)
    stream = torch.cuda.Stream()
    clip = synth.build_clip()        # the bench's 100-bone clip (synth.default_spec)
    rig = synth.build_clip(num_tracks=300, has_scale=1, scale_default=0.5, scale_constant=0.1, rotation_constant=0.2, translation_constant=0.3, num_samples=200)
    rng = np.random.default_rng(7)
    ordered = np.sort(rng.choice(128, size=100, replace=False))
    print("clocks before", clocks(), flush=True)
    cases = [
        ("identity 100 -> 100", clip, 65536, np.arange(100), 100, 0),
        ("order-preserving 100 -> 128", clip, 65536, ordered, 128, 0),
        ("order-preserving 100 -> 128, fill", clip, 65536, ordered, 128, 1),
        ("random permutation 100 -> 128", clip, 65536, rng.choice(128, size=100, replace=False), 128, 0),
        ("rig order-preserving 300 -> 320, fill", rig, 16384, np.sort(rng.choice(320, size=300, replace=False)), 320, 1),
    ]
    results = []
    if os.environ.get("MAPPED_CASE") is not None:
        cases = [cases[int(os.environ["MAPPED_CASE"])]]
    for name, which, n, table, num_slots, fill in cases:
        result = measure(ctx, stream, name, which, n, np.asarray(table, dtype=np.uint32), num_slots, fill, rounds, repeats)
        results.append(result)
        if result.get("profile_only"):
            continue
        print(f"{name:40s} mapped {result['mapped_us']:8.1f} us (+-{result['mapped_spread'] * 100:.1f} %)  unmapped {result['unmapped_us']:8.1f} us  two-pass {result['two_pass_us']:8.1f} us "
              f"(+-{result['two_pass_spread'] * 100:.1f} %)  mapped/unmapped {result['mapped_over_unmapped']:.3f}  two-pass/mapped {result['two_pass_over_mapped']:.2f}  "
              + ("checked" if result["checked"] else "MISMATCH"), flush=True)
    print("clocks after", clocks(), flush=True)
    under_load = sorted({sample.get("pp_dpm_sclk", "?") + " / " + sample.get("pp_dpm_mclk", "?") for sample in CLOCK_SAMPLES})
    print(f"clocks under load ({len(CLOCK_SAMPLES)} samples, sclk / mclk):", under_load, flush=True)
    print(json.dumps({"mapped_decode": results}))
    rejected = ctx.rejected_instance_count()
    ctx.close()
    if rejected != 0 or not all(r["checked"] for r in results):
        print("FAILED: rejected", rejected)
        sys.exit(1)
    losers = [r["case"] for r in results if not r["beats_two_pass_beyond_spread"]]
    if losers:
        print("FAILED: does not beat decode + one scatter pass by more than the spread:", losers)
        sys.exit(2)


if __name__ == "__main__":
    main()
