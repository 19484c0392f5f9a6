"""The raw scalar track table's lifetime: handles from 1 and recycled, a refused registration that takes none, an unregistration that is
stream ordered (what is already enqueued is served, what comes later is refused), and a captured graph of the three launches -- whole
list, single track, the error measure with its worst record -- that replays to the same bits after other arrays went and came: the table
never moves. Expectations are the restatement's (tests/test_raw_scalar_tracks_oracle.py), on bits. Needs a GPU."""
import numpy as np
import pytest

from acl_amd import runtime
from test_gpu_pose_buffers import SENTINEL, bits
from test_gpu_raw_scalar_tracks import N, RATE, check, expected, launch, make_curves, times_for
from test_raw_scalar_tracks_oracle import TYPES, error_record, track_errors, worst_record
from test_raw_tracks_oracle import CLAMP, NEAREST, WRAP

pytestmark = pytest.mark.gpu


def test_handles_start_at_1_are_recycled_and_a_refused_array_takes_none():
    import torch
    curves = [make_curves(TYPES[k % 5], 3 + k, 4) for k in range(5)]
    with runtime.Context(0) as ctx:
        with pytest.raises(runtime.AclHipError):
            ctx.raw_scalar_tracks_info(1)                               # nothing was registered yet
        handles = [ctx.register_raw_scalar_tracks(c, TYPES[k % 5], RATE + k, WRAP if k % 2 else CLAMP) for k, c in enumerate(curves)]
        assert handles == [1, 2, 3, 4, 5]                               # from 1: 0 is the null handle
        for k, (handle, c) in enumerate(zip(handles, curves)):
            info = ctx.raw_scalar_tracks_info(handle)
            assert (info.num_tracks, info.num_samples, info.sample_rate, info.looping_policy, info.track_type, info.num_components) \
                == (3 + k, 4, RATE + k, WRAP if k % 2 else CLAMP, TYPES[k % 5], c.shape[2])
        with pytest.raises(runtime.AclHipError):
            ctx.register_raw_scalar_tracks(curves[0], TYPES[0], 0.0)   # refused before any device call
        with pytest.raises(runtime.AclHipError):
            ctx.unregister_raw_scalar_tracks(0)
        with pytest.raises(runtime.AclHipError):
            ctx.unregister_raw_scalar_tracks(6)
        ctx.unregister_raw_scalar_tracks(2)
        with pytest.raises(runtime.AclHipError):
            ctx.unregister_raw_scalar_tracks(2)
        with pytest.raises(runtime.AclHipError):
            ctx.raw_scalar_tracks_info(2)
        torch.cuda.synchronize()
        again = [ctx.register_raw_scalar_tracks(curves[0], TYPES[0], RATE) for _ in range(2)]
        assert sorted(again) == [2, 6] or sorted(again) == [6, 7]       # a retired handle comes back once its retirement was collected
        # the caller's array may go when the call returns
        mine = curves[3].copy()
        raw = ctx.register_raw_scalar_tracks(mine, TYPES[3], RATE)
        mine[:] = np.nan
        times = times_for(4, CLAMP)
        check(launch(ctx, [raw] * N, times, 4 * 4 * 6 + 4, policy=NEAREST), expected(curves[3], CLAMP, times, NEAREST))


def test_a_captured_graph_of_the_three_launches_replays_after_arrays_went_and_came():
    import torch
    device = torch.device("cuda:0")
    track_type, num_tracks, components = TYPES[2], 22, 3
    curves, lossy_curves = make_curves(track_type, num_tracks, 7), make_curves(track_type, num_tracks, 7) * np.float32(1.001)
    times = np.random.default_rng(8601).uniform(-0.05, 0.3, size=N).astype(np.float32)
    track_ids = (np.arange(N) * 5 % num_tracks).astype(np.int32)
    want_raw, want_lossy = expected(curves, WRAP, times, NEAREST), expected(lossy_curves, CLAMP, times, NEAREST)
    want_records = [error_record(track_errors(r, y)) for r, y in zip(want_raw, want_lossy)]
    stride = 4 * components * num_tracks + 4
    with runtime.Context(0) as ctx:
        other = ctx.register_raw_scalar_tracks(make_curves(TYPES[0], 5, 2), TYPES[0], RATE)
        raw, lossy = ctx.register_raw_scalar_tracks(curves, track_type, RATE, WRAP), ctx.register_raw_scalar_tracks(lossy_curves, track_type, RATE, CLAMP)
        d_times, d_tracks = torch.from_numpy(times).to(device), torch.from_numpy(track_ids).to(device)
        d_raws, d_lossys = (torch.full((N,), handle, dtype=torch.int32, device=device) for handle in (raw, lossy))
        d_rows = [torch.full((N, stride // 4), float(SENTINEL), dtype=torch.float32, device=device) for _ in range(2)]
        d_single = torch.full((N, components + 1), float(SENTINEL), dtype=torch.float32, device=device)
        d_errors = torch.zeros((N, 2), dtype=torch.int32, device=device)
        d_worst = torch.zeros(4, dtype=torch.int32, device=device)
        sample_desc, error_desc = runtime.RawSampleDesc(), runtime.ScalarErrorDesc()
        sample_desc.rounding_policy = NEAREST
        error_desc.num_tracks, error_desc.num_components, error_desc.worst = num_tracks, components, d_worst.data_ptr()

        def launches(stream):
            ctx.sample_raw_scalar_tracks_batch(d_raws.data_ptr(), d_times.data_ptr(), N, d_rows[0].data_ptr(), stride, desc=sample_desc, stream=stream)
            ctx.sample_raw_scalar_tracks_batch(d_lossys.data_ptr(), d_times.data_ptr(), N, d_rows[1].data_ptr(), stride, desc=sample_desc, stream=stream)
            ctx.sample_raw_scalar_track_batch(d_raws.data_ptr(), d_times.data_ptr(), d_tracks.data_ptr(), N, d_single.data_ptr(), 4 * components + 4, desc=sample_desc, stream=stream)
            ctx.measure_scalar_error(d_rows[0].data_ptr(), stride, d_rows[1].data_ptr(), stride, N, error_desc, d_errors.data_ptr(), stream=stream)

        def results():
            torch.cuda.synchronize()
            return [tensor.cpu().numpy().copy() for tensor in (d_rows[0], d_rows[1], d_single, d_errors, d_worst)]

        side = torch.cuda.Stream(device=device)
        side.wait_stream(torch.cuda.current_stream(device))
        with torch.cuda.stream(side):
            launches(side.cuda_stream)                                  # warm-up, and the direct results
            direct = results()
            for tensor in (d_rows[0], d_rows[1], d_single):
                tensor.fill_(float(SENTINEL))
            d_errors.zero_()
            d_worst.zero_()
            side.synchronize()
            graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graph, stream=side):
                launches(side.cuda_stream)
        # another array goes, others come: the table does not move and the arrays of the graph stay
        ctx.unregister_raw_scalar_tracks(other)
        torch.cuda.synchronize()
        others = [ctx.register_raw_scalar_tracks(make_curves(TYPES[1], 3, 2), TYPES[1], RATE) for _ in range(3)]
        assert raw not in others and lossy not in others
        with torch.cuda.stream(side):
            graph.replay()
        replayed = results()
        for got in (direct, replayed):
            for rows, want in ((got[0], want_raw), (got[1], want_lossy)):
                assert np.array_equal(bits(rows[:, : components * num_tracks]), bits(np.stack(want).reshape(N, -1))) and np.all(rows[:, components * num_tracks:] == SENTINEL)
            assert np.array_equal(bits(got[2][:, :components]), bits(np.stack([row[b] for row, b in zip(want_raw, track_ids)]))) and np.all(got[2][:, components:] == SENTINEL)
            records = got[3].view(np.uint32).reshape(-1).view(runtime.TRACK_ERROR_DTYPE)
            assert [(bits(r["error"]), int(r["track"])) for r in records] == [(bits(error), track) for error, track in want_records]
            worst = got[4].view(np.uint32).view(runtime.TRACK_ERROR_WORST_DTYPE)[0]
            error, track, instance = worst_record(want_records)
            assert (bits(worst["error"]), int(worst["track"]), int(worst["instance"])) == (bits(error), track, instance) and error > 0.0
        del graph
        assert ctx.rejected_instance_count() == 0


def test_unregistration_is_stream_ordered():
    """enqueued, then retired without a wait in between: that launch is served; a launch behind the retirement is refused"""
    import torch
    device = torch.device("cuda:0")
    curves = make_curves(TYPES[4], 100, 7)
    times = times_for(7, CLAMP)
    stride = 4 * 4 * 100
    with runtime.Context(0) as ctx:
        keeps = ctx.register_raw_scalar_tracks(make_curves(TYPES[0], 5, 2), TYPES[0], RATE)
        raw = ctx.register_raw_scalar_tracks(curves, TYPES[4], RATE)
        d_raws = torch.full((N,), raw, dtype=torch.int32, device=device)
        d_times = torch.from_numpy(times).to(device)
        d_rows = torch.full((N, stride // 4), float(SENTINEL), dtype=torch.float32, device=device)
        stream = torch.cuda.current_stream(device).cuda_stream
        ctx.sample_raw_scalar_tracks_batch(d_raws.data_ptr(), d_times.data_ptr(), N, d_rows.data_ptr(), stride, stream=stream)
        ctx.unregister_raw_scalar_tracks(raw)
        torch.cuda.synchronize()
        assert np.array_equal(bits(d_rows.cpu().numpy()), bits(np.stack(expected(curves, CLAMP, times)).reshape(N, -1)))
        assert ctx.rejected_instance_count() == 0
        check(launch(ctx, [raw] * N, times, stride), [None] * N)
        assert ctx.rejected_instance_count() == N
        assert ctx.raw_scalar_tracks_info(keeps).num_tracks == 5
