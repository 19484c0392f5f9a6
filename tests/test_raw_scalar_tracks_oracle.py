"""What aclhip_sample_raw_scalar_tracks_batch, aclhip_sample_raw_scalar_track_batch and aclhip_measure_scalar_error_batch compute --
acl::track_array's sample_tracks / sample_track for float1f .. vector4f (compression/impl/track_array.impl.h:209-438) and
calculate_scalar_track_error (compression/impl/track_error.impl.h:53-103, :198-213) -- restated on the CPU as numpy float32 element
operations (every operand is float32, nothing is evaluated in float64), in the order of the header's definitions:

  step 1   key_frames of tests/test_raw_tracks_oracle.py: the clamp, the two key frames, the unrounded alpha
  step 2   a_b = apply_rounding_policy(alpha, policy of track b)                                       (round_alpha, the same file)
  step 3   value = (V1[c] * a_b) + (V0[c] - (V0[c] * a_b)) per component                                (lerp, the same file)
  error    e_c = |R[b][c] - Y[b][c]|, error[b] = the greatest e_c (a NaN if any is), the record the first track of the greatest error

The restatement is pinned three ways: to the oracle's key frame function over the qvvf file's sweep of times; to the reference itself ON
BITS -- a precision 0 compression keeps every track at the raw rate, and both the reference's decoder and the oracle's return the
restatement's floats --; and the error loop to the greatest |raw - decoded| over the key frames of a precision 1e-4 clip.

Wrap: the reference's scalar decompression context takes a wrap policy for a clip that was not compressed as a loop (it decodes with the
clip's samples and the wrapped duration), so wrap is pinned to the reference's decoder on bits as well
(test_a_wrapped_array_is_the_references_wrapped_decode_on_bits), next to the oracle's key frame function.

tests/test_gpu_raw_scalar_tracks.py and tests/test_gpu_scalar_error.py compare the kernels with this file on bits."""
import ctypes

import numpy as np
import pytest

from oracle import bindings as ob
from test_raw_tracks_oracle import CLAMP, WRAP, NONE, FLOOR, CEIL, NEAREST, PER_TRACK, F32, bits, finite_duration, key_frames, round_alpha, lerp, oracle_key_frames, sweep_times

TYPES = (ob.TRACK_FLOAT1F, ob.TRACK_FLOAT2F, ob.TRACK_FLOAT3F, ob.TRACK_FLOAT4F, ob.TRACK_VECTOR4F)
TYPE_IDS = ("float1f", "float2f", "float3f", "float4f", "vector4f")
COMPONENTS = {ob.TRACK_FLOAT1F: 1, ob.TRACK_FLOAT2F: 2, ob.TRACK_FLOAT3F: 3, ob.TRACK_FLOAT4F: 4, ob.TRACK_VECTOR4F: 4}
NO_TRACK = 0xFFFFFFFF


def sample_tracks(samples, sample_rate, looping, sample_time, policy=NONE, track_policies=None):
    """steps 1 - 3 of one instance over samples [S, T, C]: the row, float32 [T, C]"""
    samples = np.ascontiguousarray(samples, dtype=np.float32)
    num_samples, num_tracks = samples.shape[0], samples.shape[1]
    k0, k1, alpha = key_frames(num_samples, sample_rate, looping, sample_time)
    if policy == PER_TRACK:
        policies = np.asarray(track_policies)[:num_tracks]
    else:
        policies = np.full(num_tracks, policy if policy < PER_TRACK else NONE)     # a device value above PER_TRACK is taken as NONE
    a = round_alpha(alpha, policies)[:, None]
    with np.errstate(all="ignore"):
        return lerp(samples[k0], samples[k1], a).astype(np.float32)


def sample_track(samples, sample_rate, looping, sample_time, track, policy=NONE, track_policies=None):
    """sample_track: the policy goes to the key frame search, which rounds with the same function -- the whole-list row's entry"""
    return sample_tracks(samples, sample_rate, looping, sample_time, policy, track_policies)[track]


def track_errors(raw, lossy):
    """steps 1 and 2 of the measure over two rows [T, C]: float32 [T]; max(a, b) = a > b ? a : b in ascending component order, a NaN if
    any component's error is one"""
    raw, lossy = np.asarray(raw, dtype=np.float32), np.asarray(lossy, dtype=np.float32)
    with np.errstate(all="ignore"):
        e = np.abs(raw - lossy).astype(np.float32)
        out = e[:, 0].copy()
        for c in range(1, e.shape[1]):
            out = np.where(out > e[:, c], out, e[:, c])
        out[np.isnan(e).any(axis=1)] = np.nan
    return out.astype(np.float32)


def error_record(errors):
    """step 3: (error, track) -- from (-1, NO_TRACK), ascending tracks, a strict >"""
    worst, track = F32(-1.0), NO_TRACK
    for b, error in enumerate(errors):
        if error > worst:
            worst, track = F32(error), b
    return worst, track


def worst_record(records):
    """step 5: (error, track, instance) over the instances' records in ascending order; (-1, NO_TRACK, 0xFFFFFFFF) when nothing was measured"""
    worst, track, instance = F32(-1.0), NO_TRACK, 0xFFFFFFFF
    for i, (error, b) in enumerate(records):
        if error > worst:
            worst, track, instance = F32(error), b, i
    return worst, track, instance


def clip_error(raw, sample_rate, decode, rounding=NEAREST):
    """calculate_compression_error's loop (track_error.impl.h:166-217) over `decode(t)` -> [T, C]: (track, error, sample_time); the raw
    side is sampled with `rounding` (the reference's choice for a clip without a database: nearest)"""
    num_samples = raw.shape[0]
    duration = finite_duration(num_samples, sample_rate, CLAMP)
    times = [min(F32(i) / F32(sample_rate), duration) for i in range(num_samples)]
    records = [error_record(track_errors(sample_tracks(raw, sample_rate, CLAMP, float(t), rounding), decode(float(t)))) for t in times]
    error, track, instance = worst_record(records)
    if instance == 0xFFFFFFFF:
        return NO_TRACK, -1.0, float("nan")
    return track, float(error), float(times[instance])


def random_curves(rng, num_samples, num_tracks, num_components, constant_track=None):
    """smooth curves plus noise in +-3; one track may be constant"""
    phase = rng.uniform(0.0, 6.28, size=(1, num_tracks, num_components))
    k = np.arange(num_samples, dtype=np.float64)[:, None, None]
    curves = 2.0 * np.sin(0.7 * k + phase) + rng.uniform(-1.0, 1.0, size=(num_samples, num_tracks, num_components))
    if constant_track is not None:
        curves[:, constant_track, :] = curves[0, constant_track, :]
    return curves.astype(np.float32)


# ---- key frames and alpha ---------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("looping", [CLAMP, WRAP], ids=["clamp", "wrap"])
@pytest.mark.parametrize("num_samples", [1, 2, 7])
def test_rows_follow_the_oracles_key_frames_over_the_sweep(num_samples, looping):
    """the restated row is the lerp of exactly the two key frames, with exactly the alpha, that the oracle's function names"""
    rng = np.random.default_rng(6101)
    raw = random_curves(rng, num_samples, 3, 3)
    for rate in (30.0, 0.7):
        duration = finite_duration(num_samples, rate, looping)
        for t in sweep_times(num_samples, rate, looping):
            clamped = min(max(F32(t), F32(0.0)), duration)
            k0, k1, alpha = oracle_key_frames(num_samples, rate, float(clamped), looping)
            assert (k0, k1) == key_frames(num_samples, rate, looping, t)[0:2] and bits(alpha) == bits(key_frames(num_samples, rate, looping, t)[2])
            for policy in (NONE, FLOOR, CEIL, NEAREST):
                a = F32(ob.oracle().aclo_apply_rounding_policy(ctypes.c_float(alpha), policy))
                with np.errstate(all="ignore"):
                    want = (raw[k1] * a) + (raw[k0] - (raw[k0] * a))
                assert np.array_equal(bits(sample_tracks(raw, rate, looping, t, policy)), bits(want)), (rate, t, policy)


# ---- the reference itself, on bits --------------------------------------------------------------------------------------------------------

RATE, SAMPLES, TRACKS = 30.0, 7, 5


@pytest.fixture(scope="module")
def clips():
    """per type: (raw [7, 5, C] with track 3 constant, the precision 0 blob, the precision 1e-4 blob)"""
    if not ob.have_ref_scalar():
        pytest.skip("the reference's scalar compressor library is not built")
    rng = np.random.default_rng(6201)
    out = {}
    for track_type in TYPES:
        raw = random_curves(rng, SAMPLES, TRACKS, COMPONENTS[track_type], constant_track=3)
        out[track_type] = (raw, ob.ref_scalar_compress(raw, track_type, RATE, precision=0.0), ob.ref_scalar_compress(raw, track_type, RATE, precision=1.0e-4))
    return out


def times_over(duration, count=41):
    """on key frames (k / 30 for k = 0 .. 6 are among them as float32 values) and between them"""
    return [float(t) for t in np.linspace(0.0, float(duration), count, dtype=np.float32)] + [float(F32(k) / F32(RATE)) for k in range(SAMPLES)]


@pytest.mark.parametrize("track_type", TYPES, ids=TYPE_IDS)
def test_the_restatement_is_the_references_decode_of_the_precision_0_clip_on_bits(clips, track_type):
    raw, blob, _ = clips[track_type]
    duration = finite_duration(SAMPLES, RATE, CLAMP)
    differing = words = 0
    for t in times_over(duration) + [-1.0, 1.0e9]:
        for policy in (NONE, FLOOR, CEIL, NEAREST):
            got = sample_tracks(raw, RATE, CLAMP, t, policy)
            differing += int((bits(got) != bits(ob.ref_scalar_decompress(blob, t, policy))).sum())
            differing += int((bits(got) != bits(ob.oracle_scalar_decompress_tracks(blob, t, policy))).sum())
            words += 2 * got.size
    assert words == 2 * 50 * 4 * TRACKS * COMPONENTS[track_type] and differing == 0


@pytest.mark.parametrize("track_type", TYPES, ids=TYPE_IDS)
def test_per_track_rounding_is_the_references_on_bits(clips, track_type):
    raw, blob, _ = clips[track_type]
    table = np.array([NONE, FLOOR, CEIL, NEAREST, NEAREST, CEIL, FLOOR], dtype=np.uint8)       # longer than the list
    for t in times_over(finite_duration(SAMPLES, RATE, CLAMP), 13):
        got = sample_tracks(raw, RATE, CLAMP, t, PER_TRACK, table)
        want = ob.ref_scalar_decompress(blob, t, PER_TRACK, settings=1, track_rounding=table[:TRACKS].copy())
        assert np.array_equal(bits(got), bits(want)), t
        for track in range(TRACKS):
            assert np.array_equal(bits(got[track]), bits(sample_tracks(raw, RATE, CLAMP, t, int(table[track]))[track]))
            assert np.array_equal(bits(sample_track(raw, RATE, CLAMP, t, track, PER_TRACK, table)), bits(got[track]))
            # the single-track form through the reference: decompress_track with the track's policy
            single = ob.ref_scalar_decompress(blob, t, int(table[track]), track_index=track)
            assert np.array_equal(bits(single[track]), bits(got[track])), (t, track)


@pytest.mark.parametrize("track_type", TYPES, ids=TYPE_IDS)
def test_a_wrapped_array_is_the_references_wrapped_decode_on_bits(clips, track_type):
    raw, blob, _ = clips[track_type]
    duration = finite_duration(SAMPLES, RATE, WRAP)
    assert bits(duration) == bits(F32(SAMPLES) / F32(RATE))
    between_last_and_first = 0
    for t in times_over(duration) + [(SAMPLES - 0.5) / RATE, 1.0e9]:
        k0, k1, _ = key_frames(SAMPLES, RATE, WRAP, t)
        between_last_and_first += (k0, k1) == (SAMPLES - 1, 0)
        for policy in (NONE, NEAREST):
            got = sample_tracks(raw, RATE, WRAP, t, policy)
            assert np.array_equal(bits(got), bits(ob.ref_scalar_decompress(blob, t, policy, looping=WRAP))), (t, policy)
    assert between_last_and_first >= 3


# ---- the error loop -------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("track_type", TYPES, ids=TYPE_IDS)
def test_the_error_loop_names_the_greatest_difference_over_the_key_frames(clips, track_type):
    raw, exact, lossy = clips[track_type]
    track, error, time = clip_error(raw, RATE, lambda t: ob.oracle_scalar_decompress_tracks(lossy, t, NEAREST))
    decoded = np.stack([ob.oracle_scalar_decompress_tracks(lossy, float(F32(k) / F32(RATE)), NEAREST) for k in range(SAMPLES)])
    difference = np.abs(raw - decoded).astype(np.float32)
    assert track < TRACKS and 0.0 < error <= 1.0e-4
    assert error == float(difference.max())
    k, b = np.argwhere(difference.max(axis=2) == difference.max())[0]         # the lowest sample, then the lowest track among equals
    assert (track, time) == (int(b), float(F32(k) / F32(RATE)))
    # the lossy decode is off the raw lerp between key frames by no more than the precision allows
    worst = max(np.abs(sample_tracks(raw, RATE, CLAMP, t) - ob.oracle_scalar_decompress_tracks(lossy, t)).max() for t in times_over(finite_duration(SAMPLES, RATE, CLAMP)))
    assert 0.0 < worst <= 1.0e-4
    assert clip_error(raw, RATE, lambda t: ob.oracle_scalar_decompress_tracks(exact, t, NEAREST)) == (0, 0.0, 0.0)


def test_error_rules_nan_ties_and_nothing_measured():
    raw = np.zeros((6, 3), dtype=np.float32)
    lossy = raw.copy()
    lossy[1] = (0.0, 0.5, 0.25)
    lossy[2] = (0.5, 0.0, 0.0)             # a tie with track 1: the lower track keeps the record
    lossy[3] = (np.nan, 9.0, 0.0)          # a NaN component makes the track's error a NaN, which never wins
    lossy[4] = (0.0, 0.0, -0.125)
    errors = track_errors(raw, lossy)
    assert np.array_equal(bits(errors[[0, 1, 2, 4, 5]]), bits(np.array([0.0, 0.5, 0.5, 0.125, 0.0], dtype=np.float32))) and np.isnan(errors[3])
    assert error_record(errors) == (0.5, 1)
    assert error_record(track_errors(raw, raw)) == (0.0, 0)
    assert error_record(np.full(4, np.nan, dtype=np.float32)) == (-1.0, NO_TRACK)
    assert worst_record([(F32(-1.0), NO_TRACK), (F32(0.25), 2), (F32(0.5), 1), (F32(0.5), 0)]) == (0.5, 1, 2)
    assert worst_record([]) == worst_record([(F32(-1.0), NO_TRACK)]) == (-1.0, NO_TRACK, 0xFFFFFFFF)
    # one component: the error is the difference's magnitude
    assert np.array_equal(bits(track_errors(np.array([[1.0], [-2.0]]), np.array([[1.5], [2.0]]))), bits(np.array([0.5, 4.0], dtype=np.float32)))


def test_a_nan_in_a_key_frame_reaches_its_track_at_the_times_that_read_it_and_no_other_element():
    rng = np.random.default_rng(6301)
    raw = random_curves(rng, 6, 5, 3)
    clean = raw.copy()
    raw[3, 2, 1] = np.nan
    for t in np.arange(0.0, 5.01, 0.25) / 30.0:
        k0, k1, _ = key_frames(6, 30.0, CLAMP, float(t))
        row, want = sample_tracks(raw, 30.0, CLAMP, float(t)), sample_tracks(clean, 30.0, CLAMP, float(t))
        nans = np.isnan(row)
        assert nans.sum() == (1 if 3 in (k0, k1) else 0) and (not nans.any() or nans[2, 1])
        assert np.array_equal(bits(row)[~nans], bits(want)[~nans])
