"""aclhip_order_track_requests_device + aclhip_decompress_track_batch_rows: the locality order of a single track request list that lives on
the GPU (count per clip, scan, scatter on the caller's stream) and the decode that puts the transforms back in the caller's order.
The layout is the host order's (aclhip_order_track_requests_for_locality, tests/test_order_instances.py): at every position the clip is
the host order's, only which request of a clip takes which of its slots is decided by atomics. Needs a GPU."""
import numpy as np
import pytest
import torch

from acl_amd import runtime, synth
from oracle import bindings as ob
import helpers
from conftest import CLIP_SPECS
from test_order_instances import check_order

pytestmark = pytest.mark.gpu

UNKNOWN_HANDLE = 0x7FFFFFF0
_CLIPS = {}


def spec_clips():
    """one clip of every conftest shape, built once"""
    if not _CLIPS:
        for name in sorted(CLIP_SPECS):
            _CLIPS[name] = synth.build_clip(**CLIP_SPECS[name])
    return [_CLIPS[name] for name in sorted(CLIP_SPECS)]


def register(context, num_clips):
    """num_clips handles over the conftest shapes (a shape registered again is another handle); returns (handles, clip of each)"""
    shapes = spec_clips()
    clips = [shapes[i % len(shapes)] for i in range(num_clips)]
    handles = np.array([context.register_clip(c.blob, check_hash=False) for c in clips], dtype=np.uint32)
    return handles, clips


def draw(rng, handles, clips, n):
    which = rng.integers(0, handles.size, size=n)
    durations = np.array([c.duration for c in clips], dtype=np.float64)
    num_tracks = np.array([c.num_tracks for c in clips], dtype=np.int64)
    times = (rng.uniform(0.0, 1.0, size=n) * durations[which]).astype(np.float32)
    tracks = (rng.uniform(0.0, 1.0, size=n) * num_tracks[which]).astype(np.int64).clip(0, num_tracks[which] - 1).astype(np.uint32)
    return which, handles[which], times, tracks


def to_device(array, device):
    return torch.from_numpy(np.ascontiguousarray(array).view(np.int32) if array.dtype == np.uint32 else np.ascontiguousarray(array)).to(device)


def order_on_device(context, device, clip_ids, times, tracks, stream=None):
    """the ordering with every optional output; returns the device inputs and the host copies of the outputs"""
    n = clip_ids.size
    d_clips, d_times, d_tracks = to_device(clip_ids, device), to_device(times, device), to_device(tracks, device)
    d_order = torch.full((n,), -1, dtype=torch.int32, device=device)
    d_out_clips = torch.full((n,), -1, dtype=torch.int32, device=device)
    d_out_times = torch.full((n,), -1.0, dtype=torch.float32, device=device)
    d_out_tracks = torch.full((n,), -1, dtype=torch.int32, device=device)
    d_positions = torch.full((n,), -1, dtype=torch.int32, device=device)
    torch.cuda.synchronize(device)
    context.order_track_requests_device(d_clips.data_ptr(), d_times.data_ptr(), d_tracks.data_ptr(), n, d_order.data_ptr(), d_out_clips.data_ptr(),
                                        d_out_times.data_ptr(), d_out_tracks.data_ptr(), d_positions.data_ptr(), stream=None if stream is None else stream.cuda_stream)
    torch.cuda.synchronize(device)
    inputs = (d_clips, d_times, d_tracks)
    outputs = dict(order=d_order, clips=d_out_clips, times=d_out_times, tracks=d_out_tracks, positions=d_positions)
    return inputs, outputs


def check_device_order(clip_ids, times, tracks, outputs):
    n = clip_ids.size
    order = outputs["order"].cpu().numpy().view(np.uint32).astype(np.int64)
    assert np.array_equal(np.sort(order), np.arange(n)), "not a permutation"
    host_order = runtime.order_track_requests_for_locality(clip_ids).astype(np.int64)
    same = clip_ids[order] == clip_ids[host_order]
    assert same.all(), f"{int((~same).sum())} positions hold another clip than the host order's"
    assert np.array_equal(outputs["clips"].cpu().numpy().view(np.uint32), clip_ids[order])
    assert np.array_equal(outputs["times"].cpu().numpy().view(np.uint32), times[order].view(np.uint32))
    assert np.array_equal(outputs["tracks"].cpu().numpy().view(np.uint32), tracks[order])
    positions = outputs["positions"].cpu().numpy().view(np.uint32).astype(np.int64)
    assert np.array_equal(positions[order], np.arange(n)), "out_positions is not the inverse permutation"
    return order


@pytest.mark.parametrize("num_clips", [1, 5, 256])
def test_the_device_order_is_the_host_orders_layout(num_clips):
    with runtime.Context(0) as context:
        handles, clips = register(context, num_clips)
        device = torch.device("cuda", 0)
        rng = np.random.default_rng(num_clips)
        stream = torch.cuda.Stream(device)
        for n in (1, 5, 255, 256, 257, 2047, 2048, 4099, 70001, 4194304):
            _, clip_ids, times, tracks = draw(rng, handles, clips, n)
            _, outputs = order_on_device(context, device, clip_ids, times, tracks, stream)
            check_device_order(clip_ids, times, tracks, outputs)
        assert context.rejected_instance_count() == 0


@pytest.mark.parametrize("num_clips,n", [(5, 70001), (256, 4194304)])
def test_the_decode_that_follows_in_decode_order_and_in_the_callers_rows(num_clips, n):
    with runtime.Context(0) as context:
        handles, clips = register(context, num_clips)
        device = torch.device("cuda", 0)
        rng = np.random.default_rng(n)
        which, clip_ids, times, tracks = draw(rng, handles, clips, n)
        stream = torch.cuda.Stream(device)
        (d_clips, d_times, d_tracks), outputs = order_on_device(context, device, clip_ids, times, tracks, stream)
        order = check_device_order(clip_ids, times, tracks, outputs)

        d_as_drawn = torch.zeros((n, 12), dtype=torch.float32, device=device)
        d_ordered = torch.zeros((n, 12), dtype=torch.float32, device=device)
        d_rows = torch.zeros((n, 12), dtype=torch.float32, device=device)
        torch.cuda.synchronize(device)
        context.decompress_track_batch(d_clips.data_ptr(), d_times.data_ptr(), d_tracks.data_ptr(), n, d_as_drawn.data_ptr(), stream=stream.cuda_stream)
        context.decompress_track_batch(outputs["clips"].data_ptr(), outputs["times"].data_ptr(), outputs["tracks"].data_ptr(), n, d_ordered.data_ptr(), stream=stream.cuda_stream)
        context.decompress_track_batch_rows(outputs["clips"].data_ptr(), outputs["times"].data_ptr(), outputs["tracks"].data_ptr(), outputs["order"].data_ptr(), n,
                                            d_rows.data_ptr(), stream=stream.cuda_stream)
        stream.synchronize()
        as_drawn = d_as_drawn.cpu().numpy()
        assert np.array_equal(d_ordered.cpu().numpy().view(np.uint32), as_drawn[order].view(np.uint32))
        assert np.array_equal(d_rows.cpu().numpy().view(np.uint32), as_drawn.view(np.uint32))
        for i in rng.choice(n, size=40, replace=False):
            assert helpers.bit_equal(as_drawn[i], ob.oracle_decompress_track(clips[which[i]].blob, float(times[i]), int(tracks[i])))
        assert context.rejected_instance_count() == 0


def test_unknown_handles_and_bad_track_indices_are_ordered_and_refused_and_skipped_defaults_keep_their_bytes():
    with runtime.Context(0) as context:
        handles, clips = register(context, 40)
        device = torch.device("cuda", 0)
        rng = np.random.default_rng(77)
        n = 100003
        which, clip_ids, times, tracks = draw(rng, handles, clips, n)
        kind = rng.uniform(size=n)
        clip_ids[kind < 0.07] = UNKNOWN_HANDLE
        tracks[(kind >= 0.07) & (kind < 0.12)] = 5000
        registered = clip_ids != UNKNOWN_HANDLE
        refused = int((~registered).sum() + ((kind >= 0.07) & (kind < 0.12)).sum())
        (d_clips, d_times, d_tracks), outputs = order_on_device(context, device, clip_ids, times, tracks)
        check_device_order(clip_ids, times, tracks, outputs)       # (one unknown handle value: the host order has it in the last bucket too)

        fill = np.float32(-7.5)
        skipped = dict(default_rotation_mode=ob.DEFAULT_SKIPPED, default_translation_mode=ob.DEFAULT_SKIPPED, default_scale_mode=ob.DEFAULT_SKIPPED)
        for modes in (dict(), skipped):
            params = runtime.default_params(**modes)
            d_as_drawn = torch.full((n, 12), float(fill), dtype=torch.float32, device=device)
            d_rows = torch.full((n, 12), float(fill), dtype=torch.float32, device=device)
            torch.cuda.synchronize(device)
            before = context.rejected_instance_count()
            context.decompress_track_batch(d_clips.data_ptr(), d_times.data_ptr(), d_tracks.data_ptr(), n, d_as_drawn.data_ptr(), params=params)
            torch.cuda.synchronize(device)
            between = context.rejected_instance_count()
            context.decompress_track_batch_rows(outputs["clips"].data_ptr(), outputs["times"].data_ptr(), outputs["tracks"].data_ptr(), outputs["order"].data_ptr(), n,
                                                d_rows.data_ptr(), params=params)
            torch.cuda.synchronize(device)
            after = context.rejected_instance_count()
            assert between - before == refused and after - between == refused
            as_drawn, rows = d_as_drawn.cpu().numpy(), d_rows.cpu().numpy()
            assert np.array_equal(rows.view(np.uint32), as_drawn.view(np.uint32))
            bad = ~registered | (tracks >= 5000)
            assert (rows[bad] == fill).all(), "a refused request's row was written"
            options = ob.default_options(**modes)
            good = np.nonzero(~bad)[0]
            for i in rng.choice(good, size=40, replace=False):
                clip = clips[which[i]]
                pose = ob.oracle_decompress_tracks(clip.blob, float(times[i]), options=options, out=np.full((clip.num_tracks, 12), fill, dtype=np.float32))
                assert helpers.bit_equal(rows[i], pose[tracks[i]])
            if modes:
                # the skipped sub-tracks of the clips with default tracks kept the sentinel
                assert (rows[good] == fill).any(), "no skipped default sub-track among the requests"


@pytest.mark.parametrize("num_clips", [6000, 9000])
def test_a_registry_larger_than_the_lds_table(num_clips):
    """every workgroup's share meets more distinct clips than the LDS hash table holds at a load factor of 0.5 (2 048): 6 000 clips are
    counted one LDS word per clip, 9 000 -- more than those words -- in the hash table, flushed per 2 048 requests (order_table_insert
    would probe forever in a full table)"""
    clip = synth.build_clip(**CLIP_SPECS["two_samples_three_tracks"])
    with runtime.Context(0) as context:
        handles = np.array([context.register_clip(clip.blob, check_hash=False) for _ in range(num_clips)], dtype=np.uint32)
        device = torch.device("cuda", 0)
        rng = np.random.default_rng(num_clips)
        n = 1 << 20
        clip_ids = handles[rng.integers(0, num_clips, size=n)]
        times = rng.uniform(0.0, clip.duration, size=n).astype(np.float32)
        tracks = rng.integers(0, clip.num_tracks, size=n).astype(np.uint32)
        # the shares the library hands out (about one workgroup per CU, whole 2 048 request chunks)
        cus = torch.cuda.get_device_properties(device).multi_processor_count
        share = -(-(-(-n // 2048)) // cus) * 2048
        assert min(np.unique(clip_ids[b:b + share]).size for b in range(0, n, share)) > 2048
        (d_clips, d_times, d_tracks), outputs = order_on_device(context, device, clip_ids, times, tracks)
        order = check_device_order(clip_ids, times, tracks, outputs)
        d_as_drawn = torch.zeros((n, 12), dtype=torch.float32, device=device)
        d_rows = torch.zeros((n, 12), dtype=torch.float32, device=device)
        torch.cuda.synchronize(device)
        context.decompress_track_batch(d_clips.data_ptr(), d_times.data_ptr(), d_tracks.data_ptr(), n, d_as_drawn.data_ptr())
        context.decompress_track_batch_rows(outputs["clips"].data_ptr(), outputs["times"].data_ptr(), outputs["tracks"].data_ptr(), outputs["order"].data_ptr(), n, d_rows.data_ptr())
        torch.cuda.synchronize(device)
        as_drawn = d_as_drawn.cpu().numpy()
        assert np.array_equal(d_rows.cpu().numpy().view(np.uint32), as_drawn.view(np.uint32))
        for i in rng.choice(n, size=40, replace=False):
            assert helpers.bit_equal(as_drawn[i], ob.oracle_decompress_track(clip.blob, float(times[i]), int(tracks[i])))
        assert order.size == n and context.rejected_instance_count() == 0


def test_instance_and_track_orderings_share_a_streams_scratch():
    """one stream: instance ordering (one launch form), track ordering, instance ordering, track ordering -- every result valid"""
    with runtime.Context(0) as context:
        handles, clips = register(context, 64)
        max_tracks = max(c.num_tracks for c in clips)
        windows = -(-max_tracks * 3 // 312)
        device = torch.device("cuda", 0)
        rng = np.random.default_rng(64)
        stream = torch.cuda.Stream(device)
        for step in range(2):
            n = 65536 + step * 777
            instance_clips = handles[rng.integers(0, handles.size, size=n)]
            d_clips = to_device(instance_clips, device)
            d_times = torch.from_numpy(rng.uniform(0.0, 1.0, size=n).astype(np.float32)).to(device)
            d_order = torch.full((n,), -1, dtype=torch.int32, device=device)
            d_out_clips = torch.full((n,), -1, dtype=torch.int32, device=device)
            torch.cuda.synchronize(device)
            context.order_instances_device(d_clips.data_ptr(), d_times.data_ptr(), n, d_order.data_ptr(), d_out_clips.data_ptr(), stream=stream.cuda_stream)
            stream.synchronize()
            order = d_order.cpu().numpy().view(np.uint32).copy()
            check_order(instance_clips, order, windows, stable=False)
            assert np.array_equal(d_out_clips.cpu().numpy().view(np.uint32), instance_clips[order])

            _, clip_ids, times, tracks = draw(rng, handles, clips, 300001 + step)
            _, outputs = order_on_device(context, device, clip_ids, times, tracks, stream)
            check_device_order(clip_ids, times, tracks, outputs)


def test_order_and_rows_decode_captured_into_a_graph_replay_with_new_sample_times():
    with runtime.Context(0) as context:
        handles, clips = register(context, 32)
        device = torch.device("cuda", 0)
        rng = np.random.default_rng(32)
        n = 200000
        which, clip_ids, times, tracks = draw(rng, handles, clips, n)
        stream = torch.cuda.Stream(device)
        (d_clips, d_times, d_tracks), outputs = order_on_device(context, device, clip_ids, times, tracks, stream)     # allocates the stream's scratch
        check_device_order(clip_ids, times, tracks, outputs)
        d_rows = torch.zeros((n, 12), dtype=torch.float32, device=device)
        d_fresh = torch.zeros((n, 12), dtype=torch.float32, device=device)

        def order_and_decode():
            context.order_track_requests_device(d_clips.data_ptr(), d_times.data_ptr(), d_tracks.data_ptr(), n, outputs["order"].data_ptr(), outputs["clips"].data_ptr(),
                                                outputs["times"].data_ptr(), outputs["tracks"].data_ptr(), outputs["positions"].data_ptr(), stream=stream.cuda_stream)
            context.decompress_track_batch_rows(outputs["clips"].data_ptr(), outputs["times"].data_ptr(), outputs["tracks"].data_ptr(), outputs["order"].data_ptr(), n,
                                                d_rows.data_ptr(), stream=stream.cuda_stream)

        torch.cuda.synchronize(device)
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=stream):
            order_and_decode()
        for replay in range(3):
            new_times = (rng.uniform(0.0, 1.0, size=n) * np.array([c.duration for c in clips])[which]).astype(np.float32)
            d_times.copy_(torch.from_numpy(new_times))
            d_rows.fill_(0.0)
            torch.cuda.synchronize(device)
            with torch.cuda.stream(stream):         # (a captured ordering holds its stream's scratch: replay it there)
                graph.replay()
            stream.synchronize()
            context.decompress_track_batch(d_clips.data_ptr(), d_times.data_ptr(), d_tracks.data_ptr(), n, d_fresh.data_ptr(), stream=stream.cuda_stream)
            stream.synchronize()
            assert np.array_equal(d_rows.cpu().numpy().view(np.uint32), d_fresh.cpu().numpy().view(np.uint32)), replay
            order = outputs["order"].cpu().numpy().view(np.uint32).astype(np.int64)
            assert np.array_equal(np.sort(order), np.arange(n))
            assert np.array_equal(outputs["times"].cpu().numpy().view(np.uint32), new_times[order].view(np.uint32))
        del graph
        assert context.rejected_instance_count() == 0
