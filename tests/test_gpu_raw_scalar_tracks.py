"""aclhip_sample_raw_scalar_tracks_batch and aclhip_sample_raw_scalar_track_batch through the C ABI: track_array's sample_tracks and
sample_track of registered raw scalar track arrays (float1f .. vector4f). The expected rows are the restatement of
tests/test_raw_scalar_tracks_oracle.py (numpy float32 element operations in the header's order), compared ON BITS wherever the expectation
is a number; where it is a NaN the output must be one, and the expected NaN words are counted first. The kernel and the restatement run
the same operation order, so there is no tolerance anywhere.

Every output region is one flat sentinel filled buffer: 64 guard floats, n rows of `stride` bytes from a base that is 16 byte aligned or
4 bytes past it, 64 guard floats. The same comparison holds the bytes behind the 4 * C * T of a row, the refused rows and the guards to
the sentinel: a wide access on an address that is not aligned, or one that runs past the row's end, shows there. The inputs are asserted
unchanged. Needs a GPU."""
import numpy as np
import pytest

from acl_amd import runtime
from test_gpu_pose_buffers import SENTINEL, bits
from test_raw_scalar_tracks_oracle import COMPONENTS, TYPE_IDS, TYPES, random_curves, sample_tracks
from test_raw_tracks_oracle import CEIL, CLAMP, FLOOR, NEAREST, NONE, PER_TRACK, WRAP, finite_duration, key_frames
from test_raw_tracks_oracle import random_clip
from test_raw_tracks_oracle import sample_tracks as sample_qvvf

pytestmark = pytest.mark.gpu

RATE = 30.0
GUARD = 64
TRACKS = [1, 5, 22, 100]            # C = 3: 22 tracks are 66 floats, a track across the 64 lane boundary; C = 4: 100 tracks are several turns of a wave
SAMPLES = [1, 2, 7]
POLICIES = [NONE, FLOOR, CEIL, NEAREST]
# the launch puts a wave on every 1024 floats of a row: 300 tracks of 4 floats need two
SHAPES = [(track_type, tracks) for track_type in TYPES for tracks in TRACKS] + [(TYPES[4], 300)]
SHAPE_IDS = ["%s-%d" % (TYPE_IDS[TYPES.index(track_type)], tracks) for track_type, tracks in SHAPES]


def times_for(num_samples, looping):
    """negative, -0, 0, on and between key frames, at and beyond the duration, the interval behind the last sample, 1e9"""
    duration = float(finite_duration(num_samples, RATE, looping))
    last = num_samples - 1
    times = [-0.5, -0.0, 0.0, duration, duration * 1.5 + 0.1, 1.0e9, (last + 0.5) / RATE, (last + 0.9) / RATE]
    times += [float(np.float32(k) / np.float32(RATE)) for k in (1, last // 2, last)]
    times += [(k + f) / RATE for k, f in ((0, 0.37), (0, 0.5), (last // 2, 0.71), (max(last - 1, 0), 0.5), (1, 0.499), (1, 0.501))]
    return np.array(times, dtype=np.float32)


N = len(times_for(7, CLAMP))


class Launched:
    pass


def launch(ctx, handles, times, stride, policy=NONE, instance_policies=None, table=None, rows=None, tracks=None, offset_floats=0, scalar=True):
    """One launch of len(handles) instances into rows of `stride` bytes; with `tracks` the single-track launch. Returns a Launched whose
    `flat` is the whole region on the host and `rows_at` its first row's float index."""
    import torch
    device = torch.device("cuda:0")
    n = len(handles)
    assert stride % 4 == 0
    keep = []

    def up(host):
        tensor = torch.from_numpy(host.view(np.int32) if host.dtype == np.uint32 else host).to(device)
        keep.append((tensor, host.view(np.int32) if host.dtype == np.uint32 else host))
        return tensor

    # (4 spare floats in front so that the base can sit 4 bytes past a 16 byte boundary)
    flat = torch.full((4 + GUARD + n * (stride // 4) + GUARD,), float(SENTINEL), dtype=torch.float32, device=device)
    assert flat.data_ptr() % 16 == 0
    first = GUARD + offset_floats
    base = flat.data_ptr() + 4 * first
    assert base % 16 == (4 * offset_floats) % 16
    d_handles, d_times = up(np.asarray(handles, dtype=np.uint32)), up(np.asarray(times, dtype=np.float32))
    desc = runtime.RawSampleDesc()
    desc.rounding_policy = policy
    for name, values, dtype in (("instance_rounding_policies", instance_policies, np.uint8), ("track_rounding_policies", table, np.uint8), ("rows", rows, np.uint32)):
        if values is not None:
            setattr(desc, name, up(np.asarray(values, dtype=dtype)).data_ptr())
    if table is not None:
        desc.num_track_rounding_policies = len(table)
    stream = torch.cuda.current_stream(device).cuda_stream
    if tracks is not None:
        ctx.sample_raw_scalar_track_batch(d_handles.data_ptr(), d_times.data_ptr(), up(np.asarray(tracks, dtype=np.uint32)).data_ptr(), n, base, stride, desc=desc, stream=stream)
    elif scalar:
        ctx.sample_raw_scalar_tracks_batch(d_handles.data_ptr(), d_times.data_ptr(), n, base, stride, desc=desc, stream=stream)
    else:
        ctx.sample_raw_tracks_batch(d_handles.data_ptr(), d_times.data_ptr(), n, base, stride, desc=desc, stream=stream)
    torch.cuda.current_stream(device).synchronize()
    out = Launched()
    out.flat, out.rows_at, out.stride_floats, out.n = flat.cpu().numpy(), first, stride // 4, n
    for tensor, host in keep:
        assert np.array_equal(tensor.cpu().numpy(), host)                   # the inputs are only read
    return out


def check(out, rows, expected_nan_words=0, row_of=None):
    """rows: per instance an array of floats or None (refused: the row stays the sentinel); row_of: the row instance i writes"""
    want = np.full(out.flat.shape, SENTINEL, dtype=np.float32)
    for i, row in enumerate(rows):
        if row is not None:
            at = out.rows_at + (i if row_of is None else int(row_of[i])) * out.stride_floats
            want[at: at + row.size] = row.reshape(-1)
    numbers = ~np.isnan(want)
    assert int((~numbers).sum()) == expected_nan_words
    assert np.array_equal(bits(out.flat)[numbers], bits(want)[numbers]), np.argwhere((bits(out.flat) != bits(want)) & numbers)[:8]
    assert np.all(np.isnan(out.flat[~numbers]))


def expected(curves, looping, times, policy=NONE, instance_policies=None, table=None):
    return [sample_tracks(curves, RATE, looping, float(t), policy if instance_policies is None else int(instance_policies[i]), table) for i, t in enumerate(times)]


def make_curves(track_type, num_tracks, num_samples):
    return random_curves(np.random.default_rng(8100 + 1000 * track_type + 31 * num_tracks + num_samples), num_samples, num_tracks, COMPONENTS[track_type])


def mixed_table(num_tracks):
    return (np.arange(num_tracks + 5) * 7 // 3 % 4).astype(np.uint8)             # all four policies, longer than the array has tracks


@pytest.mark.parametrize("track_type,num_tracks", SHAPES, ids=SHAPE_IDS)
def test_the_rows_are_the_restatement(track_type, num_tracks):
    """every sample count and both looping policies; every rounding policy per launch, per instance and per track, over the sweep of times"""
    components = COMPONENTS[track_type]
    stride = 4 * components * num_tracks + 8
    table = mixed_table(num_tracks)
    with runtime.Context(0) as ctx:
        for num_samples in SAMPLES:
            curves = make_curves(track_type, num_tracks, num_samples)
            for looping in (CLAMP, WRAP):
                times = times_for(num_samples, looping)
                if looping == WRAP and num_samples >= 2:
                    assert key_frames(num_samples, RATE, WRAP, float(times[6]))[0:2] == (num_samples - 1, 0)     # the wrap interval is read
                raw = ctx.register_raw_scalar_tracks(curves, track_type, RATE, looping)
                info = ctx.raw_scalar_tracks_info(raw)
                assert (info.num_tracks, info.num_samples, info.sample_rate, info.looping_policy, info.track_type, info.num_components) \
                    == (num_tracks, num_samples, RATE, looping, track_type, components)
                assert bits(np.float32(info.duration)) == bits(finite_duration(num_samples, RATE, looping))
                for policy in POLICIES:
                    check(launch(ctx, [raw] * N, times, stride, policy=policy), expected(curves, looping, times, policy))
                # per instance: every policy, PER_TRACK among them, and a device value above PER_TRACK, which is taken as NONE
                instance_policies = np.array([(i * 3 + 1) % 5 for i in range(N)], dtype=np.uint8)
                instance_policies[3] = 200
                out = launch(ctx, [raw] * N, times, stride, policy=FLOOR, instance_policies=instance_policies, table=table)
                check(out, expected(curves, looping, times, instance_policies=instance_policies, table=table))
                check(launch(ctx, [raw] * N, times, stride, policy=PER_TRACK, table=table), expected(curves, looping, times, PER_TRACK, table=table))
                ctx.unregister_raw_scalar_tracks(raw)
        assert ctx.rejected_instance_count() == 0


@pytest.mark.parametrize("track_type", TYPES, ids=TYPE_IDS)
def test_alignment_and_untouched_bytes(track_type):
    """row bytes 4CT, that plus 4, that rounded up to 16 plus 16; the base 16 byte aligned and 4 bytes past it: nothing behind a row's
    4 * C * T bytes and nothing behind the last row changes"""
    components = COMPONENTS[track_type]
    with runtime.Context(0) as ctx:
        for num_tracks in (5, 22):
            curves = make_curves(track_type, num_tracks, 7)
            raw = ctx.register_raw_scalar_tracks(curves, track_type, RATE, CLAMP)
            times = times_for(7, CLAMP)
            want = expected(curves, CLAMP, times, NEAREST)
            row_bytes = 4 * components * num_tracks
            for stride in (row_bytes, row_bytes + 4, (row_bytes + 15) // 16 * 16 + 16):
                for offset_floats in (0, 1):
                    check(launch(ctx, [raw] * N, times, stride, policy=NEAREST, offset_floats=offset_floats), want)
                    track_ids = np.arange(N, dtype=np.uint32) % num_tracks
                    single = launch(ctx, [raw] * N, times, stride, policy=NEAREST, tracks=track_ids, offset_floats=offset_floats)
                    check(single, [row[b] for row, b in zip(want, track_ids)])
        assert ctx.rejected_instance_count() == 0


def test_arrays_of_all_five_types_share_a_launch_with_permuted_rows():
    shapes = [(TYPES[0], 100, 7, CLAMP), (TYPES[1], 22, 2, WRAP), (TYPES[2], 22, 7, WRAP), (TYPES[3], 5, 1, CLAMP), (TYPES[4], 300, 7, CLAMP)]
    rng = np.random.default_rng(8301)
    times = rng.uniform(-0.05, 0.3, size=N).astype(np.float32)
    picks = [shapes[i % 5] for i in range(N)]
    rows = rng.permutation(N).astype(np.uint32)
    stride = 4 * 4 * 300 + 4
    with runtime.Context(0) as ctx:
        curves = {shape: make_curves(*shape[0:3]) for shape in shapes}
        handles = {shape: ctx.register_raw_scalar_tracks(curves[shape], shape[0], RATE, shape[3]) for shape in shapes}
        want = [sample_tracks(curves[shape], RATE, shape[3], float(t), NEAREST) for shape, t in zip(picks, times)]
        out = launch(ctx, [handles[shape] for shape in picks], times, stride, policy=NEAREST, rows=rows)
        check(out, want, row_of=rows)
        assert ctx.rejected_instance_count() == 0


def test_a_nan_in_a_key_frame_reaches_its_track_at_the_times_that_read_it_and_no_other_element():
    curves = make_curves(TYPES[2], 22, 7)
    curves[3, 21, 1] = np.nan                   # component y of the last track in key frame 3: element 64, the second turn's first lane
    times = (np.arange(N, dtype=np.float32) * np.float32(0.4) / np.float32(RATE)).astype(np.float32)
    reading = [3 in key_frames(7, RATE, CLAMP, float(t))[0:2] for t in times]
    assert 0 < sum(reading) < N
    with runtime.Context(0) as ctx:
        raw = ctx.register_raw_scalar_tracks(curves, TYPES[2], RATE, CLAMP)
        for policy in (NONE, FLOOR):
            rows = expected(curves, CLAMP, times, policy)
            for row, reads in zip(rows, reading):
                assert np.isnan(row).sum() == (1 if reads else 0) and (not reads or np.isnan(row[21, 1]))
            check(launch(ctx, [raw] * N, times, 4 * 66 + 4, policy=policy), rows, expected_nan_words=sum(reading))


def test_refused_instances_keep_their_rows_and_are_counted():
    import torch
    small, large = make_curves(TYPES[2], 5, 7), make_curves(TYPES[4], 22, 2)
    times = times_for(7, CLAMP)
    with runtime.Context(0) as ctx:
        handles = {5: ctx.register_raw_scalar_tracks(small, TYPES[2], RATE, CLAMP), 22: ctx.register_raw_scalar_tracks(large, TYPES[4], RATE, WRAP)}
        curves = {5: (small, CLAMP), 22: (large, WRAP)}
        retired = ctx.register_raw_scalar_tracks(small, TYPES[2], RATE, CLAMP)
        ctx.unregister_raw_scalar_tracks(retired)
        torch.cuda.synchronize()

        def serve(which, policy=NONE, table=None):
            return [None if key is None else sample_tracks(curves[key][0], RATE, curves[key][1], float(t), policy, table) for key, t in zip(which, times)]

        # handle 0, a handle past the table, one at its end, an unregistered one and a never registered one among served instances
        bad = {1: 0, 4: runtime.MAX_RAW_SCALAR_TRACKS, 6: 0xFFFFFFFF, 9: retired, 12: 100}
        which = [None if i in bad else (5 if i % 2 else 22) for i in range(N)]
        before = ctx.rejected_instance_count()
        out = launch(ctx, [bad[i] if i in bad else handles[which[i]] for i in range(N)], times, 4 * 4 * 22 + 4)
        check(out, serve(which))
        assert ctx.rejected_instance_count() - before == len(bad)

        # a stride one float short of the wider array: its instances are refused, the narrower array's are served
        which = [5 if i % 3 else 22 for i in range(N)]
        before = ctx.rejected_instance_count()
        out = launch(ctx, [handles[key] for key in which], times, 4 * 4 * 22 - 4)
        check(out, serve([key if key == 5 else None for key in which]))
        assert ctx.rejected_instance_count() - before == sum(key == 22 for key in which)

        # PER_TRACK with a table shorter than the wider array
        table = mixed_table(22)[:21]
        before = ctx.rejected_instance_count()
        out = launch(ctx, [handles[key] for key in which], times, 4 * 4 * 22, policy=PER_TRACK, table=table)
        check(out, serve([key if key == 5 else None for key in which], PER_TRACK, table))
        assert ctx.rejected_instance_count() - before == sum(key == 22 for key in which)

        # the single-track launch: a track index of T and a stride of 4 * C - 4 (float3f fits 8 bytes no more than vector4f does 12)
        track_ids = np.array([i % 5 for i in range(N)], dtype=np.uint32)
        track_ids[[2, 7]] = 5
        which = [5] * N
        rows = [None if b == 5 else row[b] for row, b in zip(serve(which), track_ids)]
        before = ctx.rejected_instance_count()
        check(launch(ctx, [handles[5]] * N, times, 12, tracks=track_ids), rows)
        assert ctx.rejected_instance_count() - before == 2
        before = ctx.rejected_instance_count()
        check(launch(ctx, [handles[5]] * N, times, 8, tracks=track_ids), [None] * N)
        assert ctx.rejected_instance_count() - before == N
        # PER_TRACK there: a track at or behind the table's end is refused, the others are served
        table = mixed_table(5)[:3]
        track_ids = np.array([i % 5 for i in range(N)], dtype=np.uint32)
        rows = [None if b >= 3 else sample_tracks(small, RATE, CLAMP, float(t), int(table[b]))[b] for t, b in zip(times, track_ids)]
        before = ctx.rejected_instance_count()
        check(launch(ctx, [handles[5]] * N, times, 16, policy=PER_TRACK, table=table, tracks=track_ids), rows)
        assert ctx.rejected_instance_count() - before == sum(b >= 3 for b in track_ids)


def test_a_handle_of_one_kind_names_no_array_of_the_other_kind():
    """both tables hand out handle 1, for arrays of different shapes: each launch serves its own kind's array, and a handle only the other
    table knows is refused"""
    import torch
    curves = make_curves(TYPES[1], 22, 7)
    clip = random_clip(np.random.default_rng(8501), 7, 5)
    times = times_for(7, CLAMP)
    with runtime.Context(0) as ctx:
        scalar, qvvf = ctx.register_raw_scalar_tracks(curves, TYPES[1], RATE, CLAMP), ctx.register_raw_tracks(clip, RATE, CLAMP)
        second = ctx.register_raw_tracks(clip, RATE, CLAMP)
        assert (scalar, qvvf, second) == (1, 1, 2)
        check(launch(ctx, [1] * N, times, 4 * 2 * 22 + 4), expected(curves, CLAMP, times))
        check(launch(ctx, [1] * N, times, 48 * 5 + 16, scalar=False), [sample_qvvf(clip, RATE, CLAMP, float(t)) for t in times])
        # handle 2 is a qvvf array only
        before = ctx.rejected_instance_count()
        check(launch(ctx, [2] * N, times, 48 * 22), [None] * N)
        assert ctx.rejected_instance_count() - before == N
        ctx.unregister_raw_tracks(second)
        third = ctx.register_raw_scalar_tracks(curves, TYPES[1], RATE, CLAMP)
        ctx.unregister_raw_scalar_tracks(scalar)
        torch.cuda.synchronize()
        before = ctx.rejected_instance_count()
        check(launch(ctx, [scalar] * N, times, 48 * 22), [None] * N)                     # retired here, still live in the other table
        check(launch(ctx, [third] * N, times, 48 * 22, scalar=False), [None] * N)        # (the qvvf table's handle 2 was retired)
        assert ctx.rejected_instance_count() - before == 2 * N
        check(launch(ctx, [qvvf] * N, times, 48 * 5, scalar=False), [sample_qvvf(clip, RATE, CLAMP, float(t)) for t in times])


@pytest.mark.parametrize("track_type", TYPES, ids=TYPE_IDS)
def test_the_single_track_launch_is_the_whole_list_rows_entry(track_type):
    """every track of every array at the sweep's times, under the launch's policies, per instance policies and PER_TRACK"""
    components = COMPONENTS[track_type]
    with runtime.Context(0) as ctx:
        for num_tracks, num_samples, looping in ((1, 1, CLAMP), (5, 7, WRAP), (22, 2, CLAMP), (100, 7, CLAMP)):
            curves = make_curves(track_type, num_tracks, num_samples)
            raw = ctx.register_raw_scalar_tracks(curves, track_type, RATE, looping)
            sweep = times_for(num_samples, looping)
            times = np.repeat(sweep, num_tracks)
            track_ids = np.tile(np.arange(num_tracks, dtype=np.uint32), len(sweep))
            n = len(times)
            table = mixed_table(num_tracks)
            stride = 4 * components + 4
            for policy, sweep_policies in ((NONE, None), (NEAREST, None), (PER_TRACK, None), (CEIL, (np.arange(len(sweep)) % 5).astype(np.uint8))):
                whole = launch(ctx, [raw] * len(sweep), sweep, 4 * components * num_tracks, policy=policy, table=table, instance_policies=sweep_policies)
                lists = whole.flat[whole.rows_at: whole.rows_at + len(sweep) * components * num_tracks].reshape(len(sweep), num_tracks, components)
                check(whole, expected(curves, looping, sweep, policy, sweep_policies, table))
                request_policies = None if sweep_policies is None else np.repeat(sweep_policies, num_tracks)
                single = launch(ctx, [raw] * n, times, stride, policy=policy, table=table, instance_policies=request_policies, tracks=track_ids)
                check(single, [lists[i // num_tracks, i % num_tracks] for i in range(n)])
        assert ctx.rejected_instance_count() == 0
