"""aclhip_measure_scalar_error_batch through the C ABI -- calculate_scalar_track_error (compression/impl/track_error.impl.h:53-103,
:198-213) over two value buffers -- and runtime.raw_scalar_clip_error / runtime.scalar_clip_error, the reference's scalar overloads of
calculate_compression_error as launches. The expectation is the restatement of tests/test_raw_scalar_tracks_oracle.py (track_errors,
error_record, worst_record), compared ON BITS: a subtraction, a magnitude and comparisons have one result. Every output buffer is
sentinel filled with guards and a stride wider than its rows. The shapes are the smallest at which the kernel can go wrong: every C in
1 .. 4; T of 1, 5, 64, 65 and 200 (a wave's lanes exactly, a lane's second and fourth turn); 9 instances (more than the four waves of a
workgroup); rows that are tight, 4 and 20 bytes wider (4 but not 16 byte aligned). Needs a GPU."""
import numpy as np
import pytest

from acl_amd import runtime, synth
from oracle import bindings as ob
from test_gpu_pose_buffers import SENTINEL, bits
from test_raw_scalar_tracks_oracle import COMPONENTS, NO_TRACK, TYPE_IDS, TYPES, clip_error, error_record, random_curves, track_errors, worst_record

pytestmark = pytest.mark.gpu

N = 9
GUARD = 16


def measure(ctx, raw, lossy, num_tracks, num_components, pad_floats=1, with_track_errors=True, with_worst=True, same_buffer=False, n=None):
    """raw, lossy: [n, T, C]. Returns (records [n] of (error, track), track errors [n + 2, T + 3] with guard rows or None, worst or None)"""
    import torch
    device = torch.device("cuda:0")
    n = raw.shape[0] if n is None else n
    row_floats = num_tracks * num_components + pad_floats

    def rows_of(values):
        host = np.full((max(n, 1), row_floats), SENTINEL, dtype=np.float32)
        if n:
            host[:n, : num_tracks * num_components] = values[:n].reshape(n, -1)
        return host, torch.from_numpy(host).to(device)

    h_raw, d_raw = rows_of(raw)
    h_lossy, d_lossy = (h_raw, d_raw) if same_buffer else rows_of(lossy)
    d_errors = torch.full((GUARD + 2 * n + GUARD,), float(SENTINEL), dtype=torch.float32, device=device)
    d_track_errors = torch.full((n + 2, num_tracks + 3), float(SENTINEL), dtype=torch.float32, device=device)
    d_worst = torch.full((12,), float(SENTINEL), dtype=torch.float32, device=device)
    desc = runtime.ScalarErrorDesc()
    desc.num_tracks, desc.num_components = num_tracks, num_components
    if with_track_errors:
        desc.track_errors, desc.track_error_stride_bytes = d_track_errors[1].data_ptr(), 4 * (num_tracks + 3)
    if with_worst:
        desc.worst = d_worst[4:].data_ptr()
    ctx.measure_scalar_error(d_raw.data_ptr(), 4 * row_floats, d_lossy.data_ptr(), 4 * row_floats, n, desc, d_errors[GUARD:].data_ptr(),
                             stream=torch.cuda.current_stream(device).cuda_stream)
    torch.cuda.current_stream(device).synchronize()
    assert np.array_equal(bits(d_raw.cpu().numpy()), bits(h_raw)) and np.array_equal(bits(d_lossy.cpu().numpy()), bits(h_lossy))      # only read
    errors = d_errors.cpu().numpy()
    assert np.all(errors[:GUARD] == SENTINEL) and np.all(errors[GUARD + 2 * n:] == SENTINEL)
    records = errors[GUARD: GUARD + 2 * n].view(runtime.TRACK_ERROR_DTYPE)
    worst = d_worst.cpu().numpy()
    assert np.all(worst[:4] == SENTINEL) and np.all(worst[8:] == SENTINEL) and (with_worst or np.all(worst == SENTINEL))
    track_error_rows = d_track_errors.cpu().numpy()
    assert with_track_errors or np.all(track_error_rows == SENTINEL)
    return records, track_error_rows if with_track_errors else None, worst[4:8].view(runtime.TRACK_ERROR_WORST_DTYPE)[0] if with_worst else None


def check(records, track_error_rows, worst, raw, lossy):
    """against the restatement, on bits; the NaN errors are counted first and must be NaNs"""
    n, num_tracks = raw.shape[0], raw.shape[1]
    want_errors = [track_errors(raw[i], lossy[i]) for i in range(n)]
    want_records = [error_record(errors) for errors in want_errors]
    for i, (error, track) in enumerate(want_records):
        assert bits(records["error"][i]) == bits(error) and int(records["track"][i]) == track, (i, records[i], error, track)
    if track_error_rows is not None:
        want = np.full(track_error_rows.shape, SENTINEL, dtype=np.float32)
        want[1: 1 + n, :num_tracks] = np.stack(want_errors)
        numbers = ~np.isnan(want)
        assert np.array_equal(bits(track_error_rows)[numbers], bits(want)[numbers]) and np.all(np.isnan(track_error_rows[~numbers]))
    if worst is not None:
        error, track, instance = worst_record(want_records)
        assert (bits(worst["error"]), int(worst["track"]), int(worst["instance"]), int(worst["reserved"])) == (bits(error), track, instance, 0)
    return want_records


@pytest.mark.parametrize("num_components", [1, 2, 3, 4])
@pytest.mark.parametrize("num_tracks", [1, 5, 64, 65, 200])
def test_records_track_errors_and_worst_are_the_restatement(num_tracks, num_components):
    rng = np.random.default_rng(9100 + 7 * num_tracks + num_components)
    raw = random_curves(rng, N, num_tracks, num_components)
    lossy = (raw + rng.normal(scale=1.0e-3, size=raw.shape)).astype(np.float32)
    lossy[2] = raw[2]                                                   # an instance without error: { 0, track 0 }
    if num_tracks >= 5:
        # the same greatest error in two tracks of one instance and in two instances: the lowest track, the lowest instance
        # (values whose differences are exactly 64)
        lossy[4], lossy[7] = raw[4], raw[7]
        raw[4, 3, num_components - 1], lossy[4, 3, num_components - 1] = 1.0, 65.0
        raw[4, num_tracks - 1, 0], lossy[4, num_tracks - 1, 0] = 2.0, -62.0
        raw[7, 1, 0], lossy[7, 1, 0] = 0.5, 64.5
        # a NaN component: the track's error is a NaN and never wins, whatever its other components say
        lossy[5, 2, 0] = np.nan
        lossy[5, 2, num_components - 1] += np.float32(1000.0)
        raw[6, num_tracks - 1, num_components - 1] = np.inf                # an infinite error wins
    lossy[8] = np.nan                                                       # nothing measured: { -1, NO_TRACK }
    with runtime.Context(0) as ctx:
        for pad_floats in (0, 1, 5):
            records, track_error_rows, worst = measure(ctx, raw, lossy, num_tracks, num_components, pad_floats=pad_floats)
            want = check(records, track_error_rows, worst, raw, lossy)
        assert want[2] == (0.0, 0) and want[8] == (-1.0, NO_TRACK)
        if num_tracks >= 5:
            assert want[4][1] == 3 and want[7][1] == 1 and want[5][1] != 2 and want[6] == (np.inf, num_tracks - 1)
            assert int(worst["instance"]) == 6
        # the records alone, and without the infinity: the tie between instances 4 and 7 goes to 4
        finite = raw.copy()
        finite[6] = lossy[6]
        records, none, worst = measure(ctx, finite, lossy, num_tracks, num_components, with_track_errors=False)
        check(records, None, worst, finite, lossy)
        if num_tracks >= 5:
            assert (int(worst["instance"]), int(worst["track"])) == (4, 3)
        records, none, none = measure(ctx, raw, lossy, num_tracks, num_components, with_track_errors=False, with_worst=False)
        check(records, None, None, raw, lossy)
        assert ctx.rejected_instance_count() == 0


def test_the_same_buffer_twice_no_instances_and_nothing_measured():
    rng = np.random.default_rng(9201)
    raw = random_curves(rng, N, 22, 3)
    with runtime.Context(0) as ctx:
        records, track_error_rows, worst = measure(ctx, raw, raw, 22, 3, same_buffer=True)
        assert np.all(bits(records["error"]) == 0) and np.all(records["track"] == 0) and np.all(bits(track_error_rows[1:-1, :22]) == 0)
        assert (bits(worst["error"]), int(worst["track"]), int(worst["instance"])) == (0, 0, 0)
        # no instances: the call still writes the worst record
        records, track_error_rows, worst = measure(ctx, raw, raw, 22, 3, n=0)
        assert (float(worst["error"]), int(worst["track"]), int(worst["instance"]), int(worst["reserved"])) == (-1.0, NO_TRACK, 0xFFFFFFFF, 0)
        assert np.all(track_error_rows == SENTINEL)
        # every error a NaN
        records, track_error_rows, worst = measure(ctx, raw, np.full_like(raw, np.nan), 22, 3)
        assert np.all(records["error"] == -1.0) and np.all(records["track"] == NO_TRACK) and np.all(np.isnan(track_error_rows[1:-1, :22]))
        assert (float(worst["error"]), int(worst["track"]), int(worst["instance"])) == (-1.0, NO_TRACK, 0xFFFFFFFF)


# ---- the clip error helpers -------------------------------------------------------------------------------------------------------------------

RATE, SAMPLES, TRACKS = 30.0, 40, 6


def same(got, want):
    return got[0] == want[0] and bits(np.float32(got[1])) == bits(np.float32(want[1])) and got[2] == want[2]


@pytest.mark.parametrize("track_type", TYPES, ids=TYPE_IDS)
def test_raw_scalar_clip_error_is_the_host_loop(track_type):
    """the compressed form is the reference compressor's at precision 1e-4 and 0 where that library is built, and a synthetic clip of the
    same shape -- which differs from the raw curves by construction -- everywhere"""
    components = COMPONENTS[track_type]
    raw = random_curves(np.random.default_rng(9300 + track_type), SAMPLES, TRACKS, components, constant_track=2)
    blobs = {"synth": synth.build_scalar_clip(seed=931, track_type=track_type, num_tracks=TRACKS, num_samples=SAMPLES, sample_rate=RATE).blob}
    if ob.have_ref_scalar():
        blobs["lossy"] = ob.ref_scalar_compress(raw, track_type, RATE, precision=1.0e-4)
        blobs["exact"] = ob.ref_scalar_compress(raw, track_type, RATE, precision=0.0)
    with runtime.Context(0) as ctx:
        handle = ctx.register_raw_scalar_tracks(raw, track_type, RATE)
        for name, blob in blobs.items():
            clip = ctx.register_clip(blob)
            for rounding in (None, runtime.ROUND_NONE):
                policy = runtime.ROUND_NEAREST if rounding is None else rounding
                want = clip_error(raw, RATE, lambda t: ob.oracle_scalar_decompress_tracks(blob, t, policy), rounding=policy)
                got = runtime.raw_scalar_clip_error(ctx, handle, clip, rounding=rounding)
                assert same(got, want), (name, got, want)
            if name == "lossy":
                assert got[0] < TRACKS and 0.0 < got[1] <= 1.0e-4
            if name == "exact":
                assert got == (0, 0.0, 0.0)
            if name == "synth":
                assert got[1] > 1.0e-3
        # a clip of another track count or type is refused
        other_type = TYPES[(TYPES.index(track_type) + 1) % 4]
        for arguments in ({"track_type": track_type, "num_tracks": TRACKS + 1}, {"track_type": other_type, "num_tracks": TRACKS}):
            other = synth.build_scalar_clip(seed=932, num_samples=SAMPLES, sample_rate=RATE, **arguments)
            with pytest.raises(ValueError):
                runtime.raw_scalar_clip_error(ctx, handle, ctx.register_clip(other.blob))


def test_scalar_clip_error_is_the_two_context_loop():
    blobs = [synth.build_scalar_clip(seed=seed, track_type=2, num_tracks=TRACKS, num_samples=SAMPLES, sample_rate=RATE).blob for seed in (941, 942)]
    duration = np.float32(SAMPLES - 1) / np.float32(RATE)
    times = np.minimum(np.arange(SAMPLES, dtype=np.float32) / np.float32(RATE), duration)
    records = [error_record(track_errors(ob.oracle_scalar_decompress_tracks(blobs[0], float(t), ob.ROUND_NEAREST), ob.oracle_scalar_decompress_tracks(blobs[1], float(t), ob.ROUND_NEAREST)))
               for t in times]
    error, track, instance = worst_record(records)
    with runtime.Context(0) as ctx:
        clips = [ctx.register_clip(blob) for blob in blobs]
        assert same(runtime.scalar_clip_error(ctx, clips[0], clips[1]), (track, error, float(times[instance]))) and error > 0.0
        assert runtime.scalar_clip_error(ctx, clips[0], clips[0]) == (0, 0.0, 0.0)
        qvvf = ctx.register_clip(synth.build_clip(seed=943, num_tracks=TRACKS, num_samples=SAMPLES, sample_rate=RATE).blob)
        with pytest.raises(ValueError):
            runtime.scalar_clip_error(ctx, clips[0], qvvf)
