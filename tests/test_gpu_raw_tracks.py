"""aclhip_sample_raw_tracks_batch through the C ABI: track_array_qvvf::sample_tracks of registered raw track arrays. The expected rows
are the restatement of tests/test_raw_tracks_oracle.py (numpy float32 element operations in the header's order), compared on bits wherever
the expectation is a number; where it is a NaN the output must be one, and the expected NaN words are counted first: they are exactly
those of the tracks a NaN was planted in. The kernel and the restatement run the same operation order, so there is no tolerance anywhere.
Every output buffer is sentinel filled with a guard row before and behind its rows and a stride wider than the rows, so the same
comparison holds the bytes behind the 48 * T of a row, the refused rows and the guards to the sentinel. Every launch has 17 instances.
The input arrays are asserted unchanged. Needs a GPU.

Rotations: unit quaternions times a factor in 0.5 .. 2, about half of the key frame pairs with a negative dot product; one pair scaled by
1e-25 -- its squares underflow to zero in fp32, the general normalize gives infinities, on both sides -- and one by 1e-21, whose squared
norm (about 1e-42) is a denormal: the short exact forms are not proven there, the general 1.0f / sqrtf is."""
import numpy as np
import pytest

from acl_amd import runtime
from test_gpu_pose_buffers import SENTINEL, Buffers, bits
from test_raw_tracks_oracle import CEIL, CLAMP, FLOOR, NEAREST, NONE, PER_TRACK, WRAP, finite_duration, key_frames, random_clip, sample_tracks

pytestmark = pytest.mark.gpu

N = 17
RATE = 30.0
TRACKS = [1, 21, 22, 100, 342]          # 3, 63, 66, 300 and 1026 quads: both sides of a wave, and past a workgroup of 1024 lanes
SAMPLES = [1, 2, 31]
POLICIES = [NONE, FLOOR, CEIL, NEAREST]


def make_array(rng, num_samples, num_tracks):
    clip = random_clip(rng, num_samples, num_tracks)
    clip[..., 0:4] *= rng.uniform(0.5, 2.0, size=(num_samples, num_tracks, 1)).astype(np.float32)
    clip[..., 7] = rng.normal(size=(num_samples, num_tracks))             # the fourth lanes hold anything: they are not read
    clip[..., 11] = np.inf
    if num_samples >= 2:
        clip[0:2, 0, 0:4] *= np.float32(1e-25)
    if has_denormal_pair(num_samples, num_tracks):
        clip[num_samples - 2:, num_tracks - 1, 0:4] *= np.float32(1e-21)
    return clip


def has_denormal_pair(num_samples, num_tracks):
    """the last two key frames of the last track, where that is not the pair scaled by 1e-25"""
    return num_samples >= 2 and (num_tracks > 1 or num_samples >= 4)


def times_for(num_samples, looping):
    """17 times: negative, 0, exact key frames, mid intervals, the duration, beyond it, and the interval behind the last sample (which
    wraps to sample 0 or clamps to the last)"""
    duration = float(finite_duration(num_samples, RATE, looping))
    last = num_samples - 1
    times = [-0.5, 0.0, duration, duration * 1.5 + 0.1, 1.0e6, (last + 0.5) / RATE, (last + 0.9) / RATE]
    times += [float(np.float32(k) / np.float32(RATE)) for k in (1, last // 2, last)]
    times += [(k + f) / RATE for k, f in ((0, 0.37), (0, 0.5), (last // 2, 0.71), (max(last - 1, 0), 0.5), (max(last - 1, 0), 0.05), (1, 0.499), (1, 0.501))]
    assert len(times) == N
    return np.array(times, dtype=np.float32)


class Launched:
    pass


def launch(ctx, handles, times, row_tracks, policy=NONE, instance_policies=None, table=None, rows=None, exact_stride=False, stream=None):
    """One launch of len(handles) instances into rows of `row_tracks` records and 32 more bytes (unless exact_stride). Returns a Launched:
    poses [n + 2, row floats] with its guard rows, on the host."""
    n = len(handles)
    row_floats = row_tracks * 12 + (0 if exact_stride else 8)
    buffers = Buffers(n, row_floats)
    h_handles, h_times = np.asarray(handles, dtype=np.uint32), np.asarray(times, dtype=np.float32)
    d_handles, d_times, d_poses = buffers.up(h_handles), buffers.up(h_times), buffers.up(buffers.host(None))
    desc = runtime.RawSampleDesc()
    desc.rounding_policy = policy
    inputs = [(d_handles, h_handles.view(np.int32)), (d_times, h_times)]
    for name, values, dtype in (("instance_rounding_policies", instance_policies, np.uint8), ("track_rounding_policies", table, np.uint8), ("rows", rows, np.uint32)):
        if values is not None:
            host = np.asarray(values, dtype=dtype)
            tensor = buffers.up(host)
            setattr(desc, name, tensor.data_ptr())
            inputs.append((tensor, host.view(np.int32) if dtype == np.uint32 else host))
    if table is not None:
        desc.num_track_rounding_policies = len(table)
    out = Launched()
    out.buffers, out.tensor = buffers, d_poses
    out.arguments = (d_handles.data_ptr(), d_times.data_ptr(), n, d_poses[1].data_ptr(), row_floats * 4)
    out.desc = desc
    ctx.sample_raw_tracks_batch(*out.arguments, desc=desc, stream=stream if stream is not None else buffers.stream())
    if stream is not None:
        return out
    out.poses = buffers.down(d_poses)
    for tensor, host in inputs:
        assert np.array_equal(buffers.down(tensor), host)                   # the inputs are only read
    return out


def check(poses, rows, expected_nan_words=0, row_of=None):
    """rows: per instance [T, 12] or None (refused: the row stays the sentinel); row_of: the row instance i writes. On bits where the
    expectation is a number, a NaN where it is a NaN -- as many as were planted, counted first --, the sentinel everywhere else."""
    want = np.full(poses.shape, SENTINEL, dtype=np.float32)
    for i, row in enumerate(rows):
        if row is not None:
            want[1 + (i if row_of is None else int(row_of[i])), : row.size] = row.reshape(-1)
    numbers = ~np.isnan(want)
    assert int((~numbers).sum()) == expected_nan_words
    assert np.array_equal(bits(poses)[numbers], bits(want)[numbers]), np.argwhere((bits(poses) != bits(want)) & numbers)[:8]
    assert np.all(np.isnan(poses[~numbers]))


def expected(clip, looping, times, policy=NONE, instance_policies=None, table=None):
    return [sample_tracks(clip, RATE, looping, float(t), policy if instance_policies is None else int(instance_policies[i]), table) for i, t in enumerate(times)]


@pytest.fixture(scope="module")
def arrays():
    """(T, S) -> the clip, made once"""
    return {(tracks, samples): make_array(np.random.default_rng(7100 + 31 * tracks + samples), samples, tracks) for tracks in TRACKS for samples in SAMPLES}


def mixed_table(num_tracks):
    return (np.arange(num_tracks + 5) * 7 // 3 % 4).astype(np.uint8)             # all four policies, longer than the array has tracks


@pytest.mark.parametrize("looping", [CLAMP, WRAP], ids=["clamp", "wrap"])
@pytest.mark.parametrize("num_samples", SAMPLES)
@pytest.mark.parametrize("num_tracks", TRACKS)
def test_the_rows_are_the_restatement(arrays, num_tracks, num_samples, looping):
    """every rounding policy per launch, per instance and per track, at times on every side of the key frames, for both looping policies"""
    clip = arrays[(num_tracks, num_samples)]
    times = times_for(num_samples, looping)
    if num_samples >= 2:
        # the rotation cases are there: negative dot products between neighbours, and the two tiny pairs give infinities and numbers
        dots = (clip[:-1, :, 0:4] * clip[1:, :, 0:4]).sum(axis=2)
        assert dots.size < 8 or ((dots < 0).any() and (dots > 0).any())
        first = sample_tracks(clip, RATE, looping, 0.37 / RATE)
        assert np.isinf(first[0, 0:4]).all() and not np.isnan(first).any()
    if has_denormal_pair(num_samples, num_tracks):
        # (a denormal squared norm has a few hundred steps: the normalized rotation is a unit quaternion to that precision)
        last = sample_tracks(clip, RATE, CLAMP, (num_samples - 1.5) / RATE)[num_tracks - 1, 0:4]
        assert np.isfinite(last).all() and abs(float(np.linalg.norm(last)) - 1.0) < 1e-2
    # (the wrap interval is read: the last sample against sample 0)
    if looping == WRAP and num_samples >= 2:
        assert key_frames(num_samples, RATE, WRAP, float(times[5]))[0:2] == (num_samples - 1, 0)
    table = mixed_table(num_tracks)
    assert set(table.tolist()) == {NONE, FLOOR, CEIL, NEAREST}
    instance_policies = np.array([(i * 3 + 1) % 5 for i in range(N)], dtype=np.uint8)       # PER_TRACK among them
    with runtime.Context(0) as ctx:
        raw = ctx.register_raw_tracks(clip, RATE, looping)
        info = ctx.raw_tracks_info(raw)
        assert (info.num_tracks, info.num_samples, info.sample_rate, info.looping_policy) == (num_tracks, num_samples, RATE, looping)
        assert bits(np.float32(info.duration)) == bits(finite_duration(num_samples, RATE, looping))
        for policy in POLICIES:
            out = launch(ctx, [raw] * N, times, num_tracks, policy=policy)
            check(out.poses, expected(clip, looping, times, policy))
        out = launch(ctx, [raw] * N, times, num_tracks, policy=PER_TRACK, table=table)
        check(out.poses, expected(clip, looping, times, PER_TRACK, table=table))
        out = launch(ctx, [raw] * N, times, num_tracks, policy=CEIL, instance_policies=instance_policies, table=table)
        check(out.poses, expected(clip, looping, times, instance_policies=instance_policies, table=table))
        # without a desc: ROUND_NONE, row i
        buffers = Buffers(N, num_tracks * 12)
        d_handles, d_times, d_poses = buffers.up(np.full(N, raw, dtype=np.uint32)), buffers.up(times), buffers.up(buffers.host(None))
        ctx.sample_raw_tracks_batch(d_handles.data_ptr(), d_times.data_ptr(), N, d_poses[1].data_ptr(), num_tracks * 48, stream=buffers.stream())
        check(buffers.down(d_poses), expected(clip, looping, times))
        assert ctx.rejected_instance_count() == 0


def test_several_arrays_in_one_launch_and_rows_as_a_permutation(arrays):
    """arrays of 1, 21, 22 and 100 tracks, 2 and 31 samples, clamped and wrapped, inside one launch: a row is written up to its own
    48 * T bytes; `rows` sends instance i to a row of its own"""
    which = [(100, 31, CLAMP), (1, 31, WRAP), (21, 2, CLAMP), (22, 31, WRAP), (100, 2, WRAP), (21, 31, WRAP), (1, 1, CLAMP), (22, 2, CLAMP)]
    rng = np.random.default_rng(7201)
    picks = [which[i % len(which)] for i in range(N)]
    times = np.array([rng.uniform(-0.1, 1.2) * max(float(finite_duration(s, RATE, l)), 0.1) for _, s, l in picks], dtype=np.float32)
    permutation = rng.permutation(N).astype(np.uint32)
    with runtime.Context(0) as ctx:
        handles = {key: ctx.register_raw_tracks(arrays[key[0:2]], RATE, key[2]) for key in which}
        assert len(set(handles.values())) == len(which)
        rows = [sample_tracks(arrays[key[0:2]], RATE, key[2], float(t), NEAREST) for key, t in zip(picks, times)]
        out = launch(ctx, [handles[key] for key in picks], times, 100, policy=NEAREST)
        check(out.poses, rows)
        assert np.all(out.poses[2, 12:] == SENTINEL)                # (instance 1 has one track)
        out = launch(ctx, [handles[key] for key in picks], times, 100, policy=NEAREST, rows=permutation)
        check(out.poses, rows, row_of=permutation)
        assert ctx.rejected_instance_count() == 0


def test_a_nan_reaches_the_tracks_that_read_it_and_no_others():
    rng = np.random.default_rng(7301)
    clip = make_array(rng, 6, 22)
    clip[3, 7, 1] = np.nan              # a rotation component of track 7 in key frame 3: its four rotation words
    clip[3, 21, 9] = np.nan             # scale y of track 21 in key frame 3: that word
    times = (np.arange(N, dtype=np.float32) * np.float32(0.3) + np.float32(0.1)) / np.float32(RATE)
    reading = [3 in key_frames(6, RATE, CLAMP, float(t))[0:2] for t in times]
    assert 0 < sum(reading) < N
    with runtime.Context(0) as ctx:
        raw = ctx.register_raw_tracks(clip, RATE, CLAMP)
        for policy in (NONE, FLOOR):
            rows = expected(clip, CLAMP, times, policy)
            for row, reads in zip(rows, reading):
                nans = np.isnan(row)
                assert nans.sum() == (5 if reads else 0) and (not reads or (nans[7, 0:4].all() and nans[21, 9]))
            out = launch(ctx, [raw] * N, times, 22, policy=policy)
            check(out.poses, rows, expected_nan_words=5 * sum(reading))
        assert ctx.rejected_instance_count() == 0


def test_refusals_leave_the_row_and_are_counted(arrays):
    import torch
    small, large = arrays[(21, 31)], arrays[(100, 31)]
    rng = np.random.default_rng(7401)
    times = rng.uniform(0.0, 1.0, size=N).astype(np.float32)
    with runtime.Context(0) as ctx:
        handles = {21: ctx.register_raw_tracks(small, RATE, CLAMP), 100: ctx.register_raw_tracks(large, RATE, WRAP)}
        clips = {21: (small, CLAMP), 100: (large, WRAP)}
        retired = ctx.register_raw_tracks(small, RATE, CLAMP)
        ctx.unregister_raw_tracks(retired)
        torch.cuda.synchronize()

        def row(tracks, t, policy=NONE, table=None):
            return sample_tracks(clips[tracks][0], RATE, clips[tracks][1], float(t), policy, table)

        # the null handle, handles that were never registered (inside and outside the table), a retired one
        ids = [handles[21]] * N
        ids[1], ids[2], ids[4], ids[7], ids[16] = 0, 0x00ABCDEF, retired, runtime.MAX_RAW_TRACKS - 1, 0xFFFFFFFF
        refused = [handle != handles[21] for handle in ids]
        before = ctx.rejected_instance_count()
        out = launch(ctx, ids, times, 21)
        check(out.poses, [None if no else row(21, t) for no, t in zip(refused, times)])
        assert ctx.rejected_instance_count() - before == sum(refused) == 5

        # a stride one record too small for the larger array (several waves per instance: counted once each); the stride that holds it serves
        which = [21, 100] * 8 + [21]
        ids = [handles[tracks] for tracks in which]
        before = ctx.rejected_instance_count()
        out = launch(ctx, ids, times, 99, exact_stride=True)
        check(out.poses, [None if tracks == 100 else row(tracks, t) for tracks, t in zip(which, times)])
        assert ctx.rejected_instance_count() - before == 8
        out = launch(ctx, ids, times, 100, exact_stride=True)
        check(out.poses, [row(tracks, t) for tracks, t in zip(which, times)])
        assert ctx.rejected_instance_count() - before == 8

        # PER_TRACK with a table too short for the larger array: refused where the instance's policy is PER_TRACK, served elsewhere
        table = np.array([1, 2, 3, 0] * 25, dtype=np.uint8)[:99]
        before = ctx.rejected_instance_count()
        out = launch(ctx, ids, times, 100, policy=PER_TRACK, table=table)
        check(out.poses, [None if tracks == 100 else row(tracks, t, PER_TRACK, table) for tracks, t in zip(which, times)])
        assert ctx.rejected_instance_count() - before == 8
        instance_policies = np.array([PER_TRACK if i % 4 == 1 else NEAREST for i in range(N)], dtype=np.uint8)
        before = ctx.rejected_instance_count()
        out = launch(ctx, ids, times, 100, instance_policies=instance_policies, table=table)
        check(out.poses, [None if tracks == 100 and policy == PER_TRACK else row(tracks, t, int(policy), table) for tracks, t, policy in zip(which, times, instance_policies)])
        assert ctx.rejected_instance_count() - before == 4
        table = np.array([1, 2, 3, 0] * 25, dtype=np.uint8)
        out = launch(ctx, ids, times, 100, policy=PER_TRACK, table=table)
        check(out.poses, [row(tracks, t, PER_TRACK, table) for tracks, t in zip(which, times)])
        assert ctx.rejected_instance_count() - before == 4

        # every instance refused
        before = ctx.rejected_instance_count()
        out = launch(ctx, [retired] * N, times, 21)
        check(out.poses, [None] * N)
        assert ctx.rejected_instance_count() - before == N


def test_a_captured_launch_replays_after_another_array_is_unregistered(arrays):
    import torch
    clip = arrays[(100, 31)]
    rng = np.random.default_rng(7501)
    times = rng.uniform(-0.1, 1.1, size=N).astype(np.float32)
    want = expected(clip, WRAP, times, NEAREST)
    with runtime.Context(0) as ctx:
        other = ctx.register_raw_tracks(arrays[(22, 31)], RATE, CLAMP)
        raw = ctx.register_raw_tracks(clip, RATE, WRAP)
        direct = launch(ctx, [raw] * N, times, 100, policy=NEAREST)
        check(direct.poses, want)
        device = direct.buffers.device
        side = torch.cuda.Stream(device=device)
        side.wait_stream(torch.cuda.current_stream(device))
        with torch.cuda.stream(side):
            captured = launch(ctx, [raw] * N, times, 100, policy=NEAREST, stream=side.cuda_stream)      # warm-up
            side.synchronize()
            captured.tensor.fill_(float(SENTINEL))
            side.synchronize()
            graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graph, stream=side):
                ctx.sample_raw_tracks_batch(*captured.arguments, desc=captured.desc, stream=side.cuda_stream)
        # another array goes, others come: the table does not move and the array of the graph stays
        ctx.unregister_raw_tracks(other)
        torch.cuda.synchronize()
        others = [ctx.register_raw_tracks(arrays[(21, 2)], RATE, CLAMP) for _ in range(3)]
        assert raw not in others
        with torch.cuda.stream(side):
            graph.replay()
        torch.cuda.synchronize()
        replayed = captured.tensor.cpu().numpy()
        check(replayed, want)
        assert np.array_equal(bits(replayed), bits(direct.poses))
        del graph
        assert ctx.rejected_instance_count() == 0
