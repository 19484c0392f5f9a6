"""aclhip_compress_raw_scalar_tracks_batch through the C ABI: compress_track_list of registered raw scalar track arrays. The expected
blobs are the restatement's (tests/scalar_compress_restatement.py, which tests/test_scalar_compress_oracle.py holds to the reference's
compressor on every byte), and every comparison is on BYTES: the definition has no tolerance.

The output region is one flat buffer filled with a sentinel byte: a guard, n rows of `stride` bytes, a guard. One comparison holds
[0, size) of every row to the blob and everything else -- the bytes behind `size`, refused rows, the guards -- to the sentinel. Needs a GPU."""
import numpy as np
import pytest

from acl_amd import runtime
import scalar_compress_restatement as restatement
from scalar_compress_restatement import COMPONENTS, LAST_SAMPLES, PRECISIONS, SWEEP

pytestmark = pytest.mark.gpu

RATE = 30.0
SENTINEL = 0xA5
GUARD = 256
TYPES = (0, 1, 2, 3, 4)
TYPE_IDS = ("float1f", "float2f", "float3f", "float4f", "vector4f")
# the sweep, plus sample counts around a wave's 64 lanes (and around the 256 values a lane keeps in registers when C = 4) and track
# counts around the 64 tracks the layout takes at a time
SHAPES = SWEEP + ((63, 2), (64, 2), (65, 2), (5, 64), (5, 65))


class Launched:
    pass


@pytest.fixture(scope="module")
def ctx():
    context = runtime.Context(0)
    yield context
    context.close()


def launch(ctx, handles, precision=1.0e-5, track_precisions=None, optimize_loops=False, stride=None, max_tracks=None, shapes=None, graph=False):
    """One launch over `handles`. `shapes`: (track_type, T, S) per instance, for the default stride (the largest bound) and max_tracks."""
    import torch
    device = torch.device("cuda:0")
    n = len(handles)
    if stride is None:
        stride = max(runtime.scalar_compress_bound(t, tracks, samples) for t, tracks, samples in shapes)
    if max_tracks is None:
        max_tracks = max(tracks for _, tracks, _ in shapes)
    flat = torch.full((GUARD + n * stride + GUARD,), SENTINEL, dtype=torch.uint8, device=device)
    assert flat.data_ptr() % 16 == 0
    host_handles = np.asarray(handles, dtype=np.uint32)
    d_handles = torch.from_numpy(host_handles.view(np.int32)).to(device)
    d_results = torch.full((n, 2), 0x5A5A5A5A, dtype=torch.int32, device=device)
    workspace_bytes = runtime.scalar_compress_workspace_bytes(n, max_tracks)
    d_workspace = torch.full((workspace_bytes + GUARD,), SENTINEL, dtype=torch.uint8, device=device)
    desc = runtime.ScalarCompressDesc()
    desc.precision = precision
    desc.flags = runtime.COMPRESS_OPTIMIZE_LOOPS if optimize_loops else 0
    desc.max_tracks = max_tracks
    desc.workspace = d_workspace.data_ptr()
    d_precisions = None
    if track_precisions is not None:
        host_precisions = np.asarray(track_precisions, dtype=np.float32)
        d_precisions = torch.from_numpy(host_precisions).to(device)
        desc.track_precisions, desc.num_track_precisions = d_precisions.data_ptr(), len(host_precisions)
    rejected_before = ctx.rejected_instance_count()
    if graph:
        stream = torch.cuda.Stream(device)
        with torch.cuda.stream(stream):
            captured = torch.cuda.CUDAGraph()
            with torch.cuda.graph(captured, stream=stream):
                ctx.compress_raw_scalar_tracks_batch(d_handles.data_ptr(), n, desc, flat.data_ptr() + GUARD, stride, d_results.data_ptr(), stream=stream.cuda_stream)
            flat.fill_(SENTINEL)         # what the capture itself may have left does not count
            d_results.fill_(0x5A5A5A5A)
            captured.replay()
        stream.synchronize()
    else:
        stream = torch.cuda.current_stream(device)
        ctx.compress_raw_scalar_tracks_batch(d_handles.data_ptr(), n, desc, flat.data_ptr() + GUARD, stride, d_results.data_ptr(), stream=stream.cuda_stream)
        stream.synchronize()
    out = Launched()
    out.flat, out.stride, out.n = flat.cpu().numpy(), stride, n
    out.results = d_results.cpu().numpy().view(np.uint32).reshape(n, 2)
    out.rejected = ctx.rejected_instance_count() - rejected_before
    assert np.array_equal(d_handles.cpu().numpy().view(np.uint32), host_handles)                # the inputs are only read
    assert np.all(d_workspace.cpu().numpy()[workspace_bytes:] == SENTINEL)                      # the workspace is as large as it says
    if d_precisions is not None:
        assert np.array_equal(d_precisions.cpu().numpy().view(np.uint32), host_precisions.view(np.uint32))
    return out


def check(out, expected):
    """expected: per instance a blob (uint8), or the status of an instance that writes nothing"""
    want = np.full(out.flat.shape, SENTINEL, dtype=np.uint8)
    want_results = np.zeros((out.n, 2), dtype=np.uint32)
    for i, blob in enumerate(expected):
        if isinstance(blob, int):
            want_results[i] = (blob, 0)
        else:
            want[GUARD + i * out.stride: GUARD + i * out.stride + blob.size] = blob
            want_results[i] = (runtime.COMPRESS_OK, blob.size)
    assert np.array_equal(out.results, want_results), (out.results[:8], want_results[:8])
    different = np.flatnonzero(out.flat != want)
    assert different.size == 0, [(int(at - GUARD) // out.stride, int(at - GUARD) % out.stride, int(out.flat[at]), int(want[at])) for at in different[:8]]
    assert out.rejected == sum(1 for blob in expected if isinstance(blob, int) and blob == runtime.COMPRESS_REFUSED)


def make_curves(track_type, num_samples, num_tracks):
    return restatement.curves(5100 + 1000 * track_type + 31 * num_tracks + num_samples, num_samples, num_tracks, COMPONENTS[track_type])


class Registered:
    """arrays registered with one context, unregistered together"""
    def __init__(self, ctx):
        self.ctx, self.handles = ctx, []

    def add(self, samples, track_type, looping=runtime.LOOP_CLAMP):
        handle = self.ctx.register_raw_scalar_tracks(samples, track_type, RATE, looping)
        self.handles.append(handle)
        return handle

    def __enter__(self):
        return self

    def __exit__(self, *args):
        for handle in self.handles:
            self.ctx.unregister_raw_scalar_tracks(handle)


@pytest.mark.parametrize("track_type", TYPES, ids=TYPE_IDS)
def test_the_blobs_are_the_restatement(ctx, track_type):
    """every shape in one launch per setting: the four precisions without the vote; the vote at 1e-4 over the three last samples"""
    with Registered(ctx) as arrays:
        cases = []          # (handle, samples)
        for num_samples, num_tracks in SHAPES:
            for how in LAST_SAMPLES:
                samples = restatement.with_last_sample(make_curves(track_type, num_samples, num_tracks), how)
                cases.append((arrays.add(samples, track_type), samples, how))
        shapes = [(track_type, samples.shape[1], samples.shape[0]) for _, samples, _ in cases]
        plain = [i for i, case in enumerate(cases) if case[2] == "different"]
        for precision in PRECISIONS:
            out = launch(ctx, [cases[i][0] for i in plain], precision=precision, shapes=[shapes[i] for i in plain])
            check(out, [restatement.compress(cases[i][1], track_type, RATE, precision=precision) for i in plain])
        out = launch(ctx, [case[0] for case in cases], precision=1.0e-4, optimize_loops=True, shapes=shapes)
        expected = [restatement.compress(samples, track_type, RATE, precision=1.0e-4, optimize_loops=True) for _, samples, _ in cases]
        check(out, expected)
        wrapped = [restatement.parse(blob)["wrap"] for blob in expected]
        assert any(wrapped) and not all(wrapped)


@pytest.fixture(scope="module")
def mixed(ctx):
    """about 40 instances over 14 arrays of all five types: the amplitude lists, the special lists and curves; handles repeat"""
    with Registered(ctx) as arrays:
        lists = []
        for track_type in TYPES:
            c = COMPONENTS[track_type]
            for samples in (restatement.amplitude_list(c), restatement.special_list(c), make_curves(track_type, 37 + track_type, 12 - track_type)):
                lists.append((arrays.add(samples, track_type), samples, track_type))
        order = [(7 * i + 3) % len(lists) for i in range(41)]
        yield ctx, lists, order


def expected_of(lists, order, **settings):
    cache = {}
    for k in set(order):
        _, samples, track_type = lists[k]
        cache[k] = restatement.compress(samples, track_type, RATE, **settings)
    return [cache[k] for k in order]


def shapes_of(lists, order):
    return [(lists[k][2], lists[k][1].shape[1], lists[k][1].shape[0]) for k in order]


def test_a_mixed_launch_with_repeated_handles(mixed):
    ctx, lists, order = mixed
    for precision, loops in ((1.0e-4, False), (1.0e-2, True), (0.0, False)):
        expected = expected_of(lists, order, precision=precision, optimize_loops=loops)
        out = launch(ctx, [lists[k][0] for k in order], precision=precision, optimize_loops=loops, shapes=shapes_of(lists, order))
        check(out, expected)
    # what the lists are for: constant tracks, low and high rates and raw tracks in one blob; an odd number of bits per frame
    parsed = [restatement.parse(blob) for blob in expected_of(lists, order, precision=1.0e-4)]
    rates = np.concatenate([p["rates"] for p in parsed])
    assert (rates == 0).any() and (rates == 24).any() and rates[rates > 0].min() == 1 and rates[rates < 24].max() >= 21
    assert any(p["num_bits_per_frame"] % 2 == 1 for p in parsed)


def test_one_instance_and_an_odd_frame(ctx):
    """num_instances == 1; 3 tracks of one float whose rates sum to an odd number of bits: frames start at every bit of a byte"""
    samples = restatement.amplitude_list(1)[:, [2, 4, 5]]
    blob = restatement.compress(samples, 0, RATE, precision=1.0e-4)
    assert restatement.parse(blob)["num_bits_per_frame"] % 2 == 1
    with Registered(ctx) as arrays:
        out = launch(ctx, [arrays.add(samples, 0)], precision=1.0e-4, shapes=[(0, 3, samples.shape[0])])
        check(out, [blob])


def test_per_track_precisions_from_a_device_table(mixed):
    ctx, lists, order = mixed
    table = np.array([1.0e-2, 0.0, 1.0e-5, 1.0e-3, np.nan, 1.0e-4, 0.5] * 3, dtype=np.float32)        # longer than any list; a NaN: the track stays raw
    expected = expected_of(lists, order, track_precisions=table)
    out = launch(ctx, [lists[k][0] for k in order], track_precisions=table, shapes=shapes_of(lists, order))
    check(out, expected)
    assert any(restatement.parse(blob)["rates"][4] == 24 for blob in expected)


def test_a_wrapped_array_is_the_clamped_array_with_the_first_sample_repeated(ctx):
    """optimize_looping.scalar.h:81-103: the vote drops the repeated sample and marks the blob; an array registered as wrapping is
    marked without a vote, with or without the flag"""
    for track_type in (0, 2, 4):
        samples = make_curves(track_type, 9, 6)
        clamped = np.concatenate([samples, samples[:1]])
        with Registered(ctx) as arrays:
            handles = [arrays.add(samples, track_type, runtime.LOOP_WRAP), arrays.add(clamped, track_type, runtime.LOOP_CLAMP)]
            shapes = [(track_type, 6, 9), (track_type, 6, 10)]
            out = launch(ctx, handles, precision=1.0e-4, optimize_loops=True, shapes=shapes)
            blob = restatement.compress(clamped, track_type, RATE, precision=1.0e-4, optimize_loops=True)
            assert restatement.parse(blob)["wrap"] and restatement.parse(blob)["num_samples"] == 9
            check(out, [blob, blob])
            out = launch(ctx, handles, precision=1.0e-4, optimize_loops=False, shapes=shapes)
            check(out, [restatement.compress(samples, track_type, RATE, precision=1.0e-4, looping_wrap=True), restatement.compress(clamped, track_type, RATE, precision=1.0e-4)])


def test_refused_instances_leave_their_rows(ctx):
    """an unknown handle, 0, a retired handle; more tracks than max_tracks; more tracks than the table has precisions; a blob larger
    than the stride -- each with its row untouched, status 2, size 0 and one count; the neighbours are served"""
    small, large = make_curves(1, 12, 4), make_curves(1, 12, 9)
    with Registered(ctx) as arrays:
        h_small, h_large = arrays.add(small, 1), arrays.add(large, 1)
        retired = ctx.register_raw_scalar_tracks(small, 1, RATE)
        ctx.unregister_raw_scalar_tracks(retired)
        blob_small, blob_large = restatement.compress(small, 1, RATE, precision=1.0e-4), restatement.compress(large, 1, RATE, precision=1.0e-4)
        refused = runtime.COMPRESS_REFUSED
        handles = [h_small, 0, 4000, retired, 0xFFFFFFFF, h_large, h_small]
        shapes = [(1, 9, 12)]
        check(launch(ctx, handles, precision=1.0e-4, shapes=shapes), [blob_small, refused, refused, refused, refused, blob_large, blob_small])
        # max_tracks 4: the array of 9 tracks is refused
        check(launch(ctx, handles, precision=1.0e-4, shapes=shapes, max_tracks=4), [blob_small, refused, refused, refused, refused, refused, blob_small])
        # a table of 4 precisions
        table = np.full(4, 1.0e-4, dtype=np.float32)
        check(launch(ctx, handles, track_precisions=table, shapes=shapes), [blob_small, refused, refused, refused, refused, refused, blob_small])
        # a stride that holds the small blob and not the large one; and one that is 16 bytes short of the small one
        assert blob_small.size < blob_large.size
        stride = (blob_small.size + 15) & ~15
        assert stride < blob_large.size
        check(launch(ctx, handles, precision=1.0e-4, shapes=shapes, stride=stride), [blob_small, refused, refused, refused, refused, refused, blob_small])
        check(launch(ctx, [h_small, h_large], precision=1.0e-4, shapes=shapes, stride=stride - 16), [refused, refused])


def test_a_sample_that_is_not_finite_fails_its_instance_alone(ctx):
    good = make_curves(2, 70, 5)
    with Registered(ctx) as arrays:
        handles, expected = [], []
        for value, at in ((np.nan, (0, 0, 0)), (np.inf, (69, 4, 2)), (-np.inf, (33, 2, 1))):
            bad = good.copy()
            bad[at] = value
            handles += [arrays.add(bad, 2), arrays.add(good, 2)]
            expected += [runtime.COMPRESS_NOT_FINITE, restatement.compress(good, 2, RATE, precision=1.0e-4, optimize_loops=True)]
        # the last sample takes part in the check even when the vote would drop it
        looped = np.concatenate([good, good[:1]])
        looped[-1, 1, 1] = np.nan
        handles.append(arrays.add(looped, 2))
        expected.append(runtime.COMPRESS_NOT_FINITE)
        check(launch(ctx, handles, precision=1.0e-4, optimize_loops=True, shapes=[(2, 5, 71)]), expected)
        with pytest.raises(RuntimeError, match="Some samples are not finite"):
            runtime.compress_scalar_tracks(ctx, handles[:2], precision=1.0e-4)
        blobs = runtime.compress_scalar_tracks(ctx, [handles[1]], precision=1.0e-4, optimize_loops=True)
        assert blobs[0].ctypes.data % 16 == 0 and np.array_equal(blobs[0], expected[1])


def test_the_blobs_check_register_and_decode(mixed):
    """every ok blob passes aclhip_check_clip with the hash, registers, and decodes a sample time to the bits the host blob decodes to"""
    import torch
    ctx, lists, order = mixed
    device = torch.device("cuda:0")
    handles = [entry[0] for entry in lists]
    blobs = runtime.compress_scalar_tracks(ctx, handles, precision=1.0e-4)
    expected = [restatement.compress(samples, track_type, RATE, precision=1.0e-4) for _, samples, track_type in lists]
    for blob, want, (_, samples, track_type) in zip(blobs, expected, lists):
        assert np.array_equal(blob, want)
        status, message = runtime.check_clip(blob, check_hash=True)
        assert status == 0, message
        decoded = []
        for source in (blob, _aligned(want)):
            clip = ctx.register_clip(source)
            info = ctx.clip_info(clip)
            assert (info.num_tracks, info.num_samples) == (samples.shape[1], samples.shape[0])
            stride = samples.shape[1] * samples.shape[2] * 4
            d_clips = torch.full((1,), clip, dtype=torch.int32, device=device)
            d_times = torch.full((1,), 0.4, dtype=torch.float32, device=device)
            d_values = torch.zeros((1, stride // 4), dtype=torch.float32, device=device)
            stream = torch.cuda.current_stream(device)
            ctx.decompress_scalar_tracks_batch(d_clips.data_ptr(), d_times.data_ptr(), 1, d_values.data_ptr(), stride, stream=stream.cuda_stream)
            stream.synchronize()
            decoded.append(d_values.cpu().numpy().view(np.uint32))
            ctx.unregister_clip(clip)
        assert np.array_equal(decoded[0], decoded[1])


def _aligned(blob):
    from acl_amd.synth import aligned_bytes
    out = aligned_bytes(blob.size)
    out[:] = blob
    return out


def test_a_captured_launch_replays_to_the_same_bytes(mixed):
    ctx, lists, order = mixed
    expected = expected_of(lists, order, precision=1.0e-4, optimize_loops=True)
    out = launch(ctx, [lists[k][0] for k in order], precision=1.0e-4, optimize_loops=True, shapes=shapes_of(lists, order), graph=True)
    check(out, expected)


def test_two_runs_give_the_same_bytes(mixed):
    ctx, lists, order = mixed
    handles = [lists[k][0] for k in order] + [0]
    runs = [launch(ctx, handles, precision=1.0e-5, optimize_loops=True, shapes=shapes_of(lists, order)) for _ in range(2)]
    assert np.array_equal(runs[0].flat, runs[1].flat) and np.array_equal(runs[0].results, runs[1].results)
