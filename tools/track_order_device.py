#!/usr/bin/env python3
"""Measurement aid: single track requests ordered ON THE DEVICE (aclhip_order_track_requests_device) for the bench's
track_requests_256_clips shape -- 4 M random (instance, bone) requests over 256 100-bone clips -- HIP events on one stream:
  (a) the decode as drawn
  (b) the device ordering alone (order + permuted clips, times, track indices)
  (c) device ordering + decode of the ordered lists (transforms in decode order)
  (d) device ordering + aclhip_decompress_track_batch_rows with rows = order (transforms in the caller's order)
  (e) the decode of the host order's lists (aclhip_order_track_requests_for_locality), for reference
and (a) / (d) again for a character-major request list (runs of 16 bones of one instance: the scattered rows come in runs).
Every pattern is first checked: (c) is (a) permuted, (d) is (a), bit for bit. TRACK_ORDER_REQUESTS, TRACK_ORDER_REPEATS."""
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402
from acl_amd import runtime, synth  # noqa: E402


def crowd_clips():
    """the bench's 256-clip crowd (bench.py, workload 256_clips / track_requests_256_clips)"""
    clips = []
    spec_rng = np.random.default_rng(3)
    for i in range(256):
        animated = spec_rng.uniform(0.25, 0.5)
        clips.append(synth.build_clip(seed=300 + i, num_tracks=100, num_samples=int(spec_rng.integers(31, 601)), sample_rate=30.0,
                                      rotation_default=0.02, rotation_constant=float(0.98 - animated), wrap=int(spec_rng.uniform() < 0.1),
                                      strip_keyframes=int(spec_rng.uniform() < 0.1), min_bits=int(spec_rng.integers(5, 10)), max_bits=int(spec_rng.integers(12, 19))))
    return clips


def timed(stream, step, repeats):
    for _ in range(10):
        step()
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record(stream)
    for _ in range(repeats):
        step()
    stop.record(stream)
    stop.synchronize()
    return start.elapsed_time(stop) / repeats * 1000.0


def measure(ctx, stream, name, ids, times, tracks, repeats, with_host_order=True):
    n = ids.size
    d_ids, d_times, d_tracks = (torch.from_numpy(a).cuda() for a in (ids, times, tracks))
    d_order = torch.arange(n, dtype=torch.int32, device="cuda")         # (in bounds whatever an ordering leaves: the rows decode stores through it)
    d_ids2, d_tracks2 = (torch.empty(n, dtype=torch.int32, device="cuda") for _ in range(2))
    d_times2 = torch.empty(n, dtype=torch.float32, device="cuda")
    d_out, d_out2 = (torch.empty((n, 12), dtype=torch.float32, device="cuda") for _ in range(2))
    s = stream.cuda_stream

    def decode_as_drawn():
        ctx.decompress_track_batch(d_ids.data_ptr(), d_times.data_ptr(), d_tracks.data_ptr(), n, d_out.data_ptr(), stream=s)

    def order():
        ctx.order_track_requests_device(d_ids.data_ptr(), d_times.data_ptr(), d_tracks.data_ptr(), n, d_order.data_ptr(), d_ids2.data_ptr(), d_times2.data_ptr(),
                                        d_tracks2.data_ptr(), None, stream=s)

    def decode_ordered():
        ctx.decompress_track_batch(d_ids2.data_ptr(), d_times2.data_ptr(), d_tracks2.data_ptr(), n, d_out2.data_ptr(), stream=s)

    def decode_rows():
        ctx.decompress_track_batch_rows(d_ids2.data_ptr(), d_times2.data_ptr(), d_tracks2.data_ptr(), d_order.data_ptr(), n, d_out2.data_ptr(), stream=s)

    # checks: (c) is (a) permuted, (d) is (a)
    decode_as_drawn()
    order()
    decode_ordered()
    stream.synchronize()
    permutation = d_order.long()
    if not torch.equal(torch.sort(permutation).values, torch.arange(n, device="cuda")):
        raise SystemExit(f"{name}: the device ordering is not a permutation")
    ok_ordered = torch.equal(d_out2.view(torch.int32), d_out[permutation].view(torch.int32))
    d_out2.zero_()
    torch.cuda.synchronize()        # (zero_ ran on the current stream, the decode runs on `stream`)
    decode_rows()
    stream.synchronize()
    ok_rows = torch.equal(d_out2.view(torch.int32), d_out.view(torch.int32))

    result = {"pattern": name, "requests": n, "ok_ordered": ok_ordered, "ok_rows": ok_rows}
    result["a_as_drawn_us"] = timed(stream, decode_as_drawn, repeats)
    result["b_order_us"] = timed(stream, order, repeats)
    result["c_order_decode_us"] = timed(stream, lambda: (order(), decode_ordered()), repeats)
    result["d_order_rows_decode_us"] = timed(stream, lambda: (order(), decode_rows()), repeats)
    result["decode_ordered_alone_us"] = timed(stream, decode_ordered, repeats)
    result["rows_decode_alone_us"] = timed(stream, decode_rows, repeats)
    if with_host_order:
        host = runtime.order_track_requests_for_locality(ids.view(np.uint32)).astype(np.int64)
        h_ids, h_times, h_tracks = (torch.from_numpy(np.ascontiguousarray(a[host])).cuda() for a in (ids, times, tracks))
        result["e_host_order_decode_us"] = timed(stream, lambda: ctx.decompress_track_batch(h_ids.data_ptr(), h_times.data_ptr(), h_tracks.data_ptr(), n, d_out2.data_ptr(), stream=s), repeats)
    return result


def main():
    n = int(os.environ.get("TRACK_ORDER_REQUESTS", str(4 * 1024 * 1024)))
    repeats = int(os.environ.get("TRACK_ORDER_REPEATS", "50"))
    ctx = runtime.Context(0)
    clips = crowd_clips()
    handles = np.array([ctx.register_clip(c.blob) for c in clips], dtype=np.int32)
    durations = np.array([c.duration for c in clips], dtype=np.float32)
    stream = torch.cuda.Stream()

    # the bench's draw: clips from rng(1000), bones from rng(4000)
    rng = np.random.default_rng(1000)
    which = rng.integers(0, 256, size=n)
    times = (rng.uniform(0.0, 1.0, size=n) * durations[which]).astype(np.float32)
    tracks = np.random.default_rng(4000).integers(0, 100, size=n).astype(np.int32)
    results = [measure(ctx, stream, "256 clips as drawn", handles[which], times, tracks, repeats)]

    # character-major: n / 16 instances, 16 distinct bones each, the instance's clip and sample time shared by its run
    runs = n // 16
    run_clip = rng.integers(0, 256, size=runs)
    run_time = (rng.uniform(0.0, 1.0, size=runs) * durations[run_clip]).astype(np.float32)
    bones = np.argsort(rng.uniform(size=(runs, 100)), axis=1)[:, :16].astype(np.int32).reshape(-1)
    results.append(measure(ctx, stream, "256 clips, character-major runs of 16 bones", np.repeat(handles[run_clip], 16), np.repeat(run_time, 16), bones, repeats, with_host_order=False))

    for r in results:
        print(f"{r['pattern']:48s} {r['requests']:8d} requests  (a) as drawn {r['a_as_drawn_us']:7.1f} us  (b) device order {r['b_order_us']:6.1f} us  "
              f"(c) order + decode {r['c_order_decode_us']:7.1f} us  (d) order + rows decode {r['d_order_rows_decode_us']:7.1f} us  "
              + (f"(e) host order's decode {r['e_host_order_decode_us']:7.1f} us  " if "e_host_order_decode_us" in r else "")
              + f"[decode alone {r['decode_ordered_alone_us']:.1f} / rows {r['rows_decode_alone_us']:.1f} us]  "
              + ("checked" if r["ok_ordered"] and r["ok_rows"] else "MISMATCH"), flush=True)
    print(json.dumps({"track_order_device": results}))
    rejected = ctx.rejected_instance_count()
    ctx.close()
    if rejected != 0 or not all(r["ok_ordered"] and r["ok_rows"] for r in results):
        print("FAILED: rejected", rejected)
        sys.exit(1)


if __name__ == "__main__":
    main()
