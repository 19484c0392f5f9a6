"""What aclhip_sample_raw_tracks_batch computes -- acl::track_array_qvvf::sample_tracks (compression/impl/track_array.impl.h:209-343) --
restated on the CPU as numpy float32 element operations (single, correctly rounded IEEE operations: every operand below is float32,
nothing is evaluated in float64), in the order of the header's definition:

  step 1   t = min(max(time, 0), D); k0 = uint32(t * r); k1 by the looping policy; alpha = t * r - k0            (key_frames)
  step 2   a_b = apply_rounding_policy(alpha, policy of track b)                                                (round_alpha)
  step 3   rotation = quat_normalize(quat_lerp_no_normalization(V0, V1, a_b)), translation and scale = lerp       (sample_tracks)
  step 4   the fourth lanes of translation and scale are +0

This file holds the restatement to the oracle's key frame functions, to the reference's compressor and the oracle's decoder of full
precision clips on bits, and to the properties the definition states; tests/test_gpu_raw_tracks.py compares the kernel with it on bits."""
import ctypes

import numpy as np
import pytest

from oracle import bindings as ob

CLAMP, WRAP = 0, 1
NONE, FLOOR, CEIL, NEAREST, PER_TRACK = ob.ROUND_NONE, ob.ROUND_FLOOR, ob.ROUND_CEIL, ob.ROUND_NEAREST, 4
F32 = np.float32


def bits(array):
    return np.ascontiguousarray(array, dtype=np.float32).view(np.uint32)


def finite_duration(num_samples, sample_rate, looping):
    """track_array::get_finite_duration (:113-124): calculate_finite_duration(S + (wrap ? 1 : 0), rate)"""
    count = num_samples + (1 if looping == WRAP else 0)
    return F32(0.0) if count <= 1 else F32(count - 1) / F32(sample_rate)


def key_frames(num_samples, sample_rate, looping, sample_time):
    """step 1: (k0, k1, the unrounded alpha)"""
    duration = finite_duration(num_samples, sample_rate, looping)
    t = min(max(F32(sample_time), F32(0.0)), duration)
    sample_index = F32(t * F32(sample_rate))
    k0, last = int(sample_index), num_samples - 1
    if looping == CLAMP:
        k1 = min(k0 + 1, last)
    elif k0 > last:
        sample_index, k0, k1 = F32(0.0), 0, 0
    else:
        k1 = 0 if k0 + 1 >= num_samples else k0 + 1
    return k0, k1, F32(sample_index - F32(k0))


def round_alpha(alpha, policies):
    """step 2 over an array of per track policies: float32 [T]"""
    policies = np.asarray(policies)
    alpha = F32(alpha)
    out = np.full(policies.shape, alpha, dtype=np.float32)
    out[policies == FLOOR] = 0.0
    out[policies == CEIL] = 1.0
    out[policies == NEAREST] = np.floor(alpha + F32(0.5))
    return out


def lerp(start, end, alpha):
    """rtm::vector_lerp in its stable form"""
    return (end * alpha) + (start - (start * alpha))


def normalize(rotations):
    """rtm::quat_normalize with the correctly rounded 1 / sqrt: [T, 4]"""
    x, y, z, w = (rotations[:, c] for c in range(4))
    with np.errstate(all="ignore"):
        dot = (w * w) + ((z * z) + ((y * y) + (x * x)))
        inv = F32(1.0) / np.sqrt(dot)
        return rotations * inv[:, None]


def sample_tracks(samples, sample_rate, looping, sample_time, policy=NONE, track_policies=None):
    """steps 1 - 4 of one instance over samples [S, T, 12]: the pose, float32 [T, 12]"""
    samples = np.ascontiguousarray(samples, dtype=np.float32)
    num_samples, num_tracks = samples.shape[0], samples.shape[1]
    k0, k1, alpha = key_frames(num_samples, sample_rate, looping, sample_time)
    policies = np.asarray(track_policies)[:num_tracks] if policy == PER_TRACK else np.full(num_tracks, policy)
    a = round_alpha(alpha, policies)[:, None]
    v0, v1 = samples[k0], samples[k1]
    out = np.zeros((num_tracks, 12), dtype=np.float32)
    with np.errstate(all="ignore"):
        q0, q1 = v0[:, 0:4], v1[:, 0:4]
        dot = (q0[:, 3] * q1[:, 3]) + ((q0[:, 2] * q1[:, 2]) + ((q0[:, 1] * q1[:, 1]) + (q0[:, 0] * q1[:, 0])))
        bias = bits(dot) & np.uint32(0x80000000)
        biased = (bits(q1) ^ bias[:, None]).view(np.float32)
        out[:, 0:4] = normalize(lerp(q0, biased, a))
        out[:, 4:7] = lerp(v0[:, 4:7], v1[:, 4:7], a)
        out[:, 8:11] = lerp(v0[:, 8:11], v1[:, 8:11], a)
    return out


def random_clip(rng, num_samples, num_tracks):
    """every sub-track animated: random unit rotations, translations in +-3, scales in 0.5 .. 2; the fourth lanes hold what a caller may
    have left there"""
    clip = np.zeros((num_samples, num_tracks, 12), dtype=np.float32)
    rotations = rng.normal(size=(num_samples, num_tracks, 4))
    clip[..., 0:4] = rotations / np.linalg.norm(rotations, axis=2, keepdims=True)
    clip[..., 4:7] = rng.uniform(-3.0, 3.0, size=(num_samples, num_tracks, 3))
    clip[..., 8:11] = rng.uniform(0.5, 2.0, size=(num_samples, num_tracks, 3))
    return clip


def oracle_key_frames(num_samples, rate, t, looping):
    k0, k1, alpha = ctypes.c_uint32(), ctypes.c_uint32(), ctypes.c_float()
    ob.oracle().aclo_find_linear_interpolation_samples_with_sample_rate(num_samples, ctypes.c_float(rate), ctypes.c_float(t), PER_TRACK, looping,
                                                                        ctypes.byref(k0), ctypes.byref(k1), ctypes.byref(alpha))
    return k0.value, k1.value, F32(alpha.value)


def sweep_times(num_samples, rate, looping):
    """negative, 0, on key frames, between them, at the duration and beyond it (and, wrapped, between the last sample and sample 0)"""
    duration = float(finite_duration(num_samples, rate, looping))
    times = [-1.0, -0.0, 0.0, duration, duration * 1.5 + 1.0, 1.0e9]
    for k in range(num_samples + 1):
        times += [float(F32(k) / F32(rate)), (k + 0.25) / rate, (k + 0.5) / rate, (k + 0.999) / rate]
    return times


# ---- key frames and alpha --------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("looping", [CLAMP, WRAP], ids=["clamp", "wrap"])
@pytest.mark.parametrize("num_samples", [1, 2, 3, 31])
def test_key_frames_and_alpha_are_the_oracles(num_samples, looping):
    oracle = ob.oracle()
    for rate in (30.0, 24.0, 0.7):
        duration = finite_duration(num_samples, rate, looping)
        assert bits(duration) == bits(F32(oracle.aclo_calculate_finite_duration(num_samples + (1 if looping == WRAP else 0), ctypes.c_float(rate))))
        for t in sweep_times(num_samples, rate, looping):
            clamped = min(max(F32(t), F32(0.0)), duration)
            k0, k1, alpha = key_frames(num_samples, rate, looping, t)
            want = oracle_key_frames(num_samples, rate, float(clamped), looping)
            assert (k0, k1) == want[0:2] and bits(alpha) == bits(want[2]), (rate, t)
            assert k0 < num_samples and k1 < num_samples and 0.0 <= alpha < 1.0
            for policy in (NONE, FLOOR, CEIL, NEAREST):
                assert bits(round_alpha(alpha, [policy]))[0] == bits(F32(oracle.aclo_apply_rounding_policy(ctypes.c_float(alpha), policy)))
    # the ends of a wrapped array: the interval behind the last sample leads back to sample 0, and the duration is sample 0 alone
    if looping == WRAP and num_samples > 1:
        k0, k1, alpha = key_frames(num_samples, 30.0, WRAP, (num_samples - 0.5) / 30.0)
        assert (k0, k1) == (num_samples - 1, 0) and 0.4 < alpha < 0.6
        assert key_frames(num_samples, 30.0, WRAP, 1.0e9) == (0, 0, 0.0)
    if looping == CLAMP:
        assert key_frames(num_samples, 30.0, CLAMP, 1.0e9) == (num_samples - 1, num_samples - 1, 0.0)


# ---- the reference's compressor and the decoder of what it wrote ----------------------------------------------------------------------------

@pytest.fixture(scope="module")
def full_precision_clip():
    if not ob.have_ref_compressor():
        pytest.skip("the reference's compressor library is not built")
    rng = np.random.default_rng(5101)
    raw = random_clip(rng, 21, 7)
    raw[..., 7] = raw[..., 11] = 0.0
    blob = ob.ref_compress_ex(raw, 30.0, rotation_format="quatf_full", translation_format="vector3f_full", scale_format="vector3f_full")
    return raw, blob


def test_the_restatement_is_the_decode_of_the_full_precision_clip_on_bits(full_precision_clip):
    """21 samples x 7 tracks at 57 times over the duration, clamp: a clip in the full formats stores its key frames as they are, and the
    decoder interpolates and normalizes them with these operations"""
    raw, blob = full_precision_clip
    duration = float(finite_duration(21, 30.0, CLAMP))
    differing = words = 0
    for t in np.linspace(0.0, duration, 57):
        want = ob.oracle_decompress_tracks(blob, float(t), ob.ROUND_NONE)
        got = sample_tracks(raw, 30.0, CLAMP, float(t))
        differing += int((bits(got) != bits(want)).sum())
        words += want.size
    assert words == 4788 and differing == 0


@pytest.mark.parametrize("policy", [FLOOR, CEIL, NEAREST], ids=["floor", "ceil", "nearest"])
def test_with_a_rounded_alpha_both_sides_normalize_the_key_frame(full_precision_clip, policy):
    """with floor / ceil / nearest the decoder of a quatf_full clip returns the key frame NORMALIZED, like sample_tracks (rtm::quat_lerp
    normalizes at alpha 0 and 1 too): the two agree on bits under every policy, and neither returns the rotation as it was stored"""
    raw, blob = full_precision_clip
    t = 7.3 / 30.0
    key = {FLOOR: 7, CEIL: 8, NEAREST: 7}[policy]
    decoded = ob.oracle_decompress_tracks(blob, t, policy)
    got = sample_tracks(raw, 30.0, CLAMP, t, policy)
    assert np.array_equal(bits(got), bits(decoded))
    # translations and scales are the key frame's
    assert np.array_equal(bits(got[:, 4:7]), bits(raw[key, :, 4:7])) and np.array_equal(bits(got[:, 8:11]), bits(raw[key, :, 8:11]))
    # the rotation is the key frame's up to the sign the other key frame gives it, normalized: not the stored bits
    flipped = np.where((got[:, 0:4] * raw[key, :, 0:4]).sum(axis=1, keepdims=True) < 0, -raw[key, :, 0:4], raw[key, :, 0:4])
    assert np.array_equal(bits(got[:, 0:4]), bits(normalize(flipped)))
    assert (bits(got[:, 0:4]) != bits(flipped)).any() and np.abs(got[:, 0:4] - flipped).max() < 2.0e-7


# ---- properties -------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("looping", [CLAMP, WRAP], ids=["clamp", "wrap"])
def test_vectors_are_exact_on_key_frames_and_the_fourth_lanes_are_zero(looping):
    rng = np.random.default_rng(5201)           # (a rate of 32: k / rate * rate is k exactly)
    clip = random_clip(rng, 9, 5)
    clip[..., 7] = rng.normal(size=(9, 5))
    clip[..., 11] = np.nan
    for k in range(9):
        pose = sample_tracks(clip, 32.0, looping, float(F32(k) / F32(32.0)))
        assert key_frames(9, 32.0, looping, float(F32(k) / F32(32.0)))[0::2] == (k, 0.0)
        assert np.array_equal(bits(pose[:, 4:7]), bits(clip[k, :, 4:7])) and np.array_equal(bits(pose[:, 8:11]), bits(clip[k, :, 8:11]))
        assert np.all(bits(pose[:, [7, 11]]) == 0)
        # alpha 1 through the policy: the next key frame's vectors, exactly
        following = min(k + 1, 8) if looping == CLAMP else (k + 1) % 9
        pose = sample_tracks(clip, 32.0, looping, float(F32(k) / F32(32.0)), CEIL)
        assert np.array_equal(bits(pose[:, 4:7]), bits(clip[following, :, 4:7])) and np.all(bits(pose[:, [7, 11]]) == 0)
        assert np.allclose(np.linalg.norm(pose[:, 0:4], axis=1), 1.0, atol=1e-6)


def test_per_track_policies_round_each_track_on_its_own():
    rng = np.random.default_rng(5301)
    clip = random_clip(rng, 4, 8)
    table = np.array([NONE, FLOOR, CEIL, NEAREST, NEAREST, CEIL, FLOOR, NONE], dtype=np.uint8)
    t = 1.7 / 30.0
    pose = sample_tracks(clip, 30.0, CLAMP, t, PER_TRACK, table)
    for track, policy in enumerate(table):
        assert np.array_equal(bits(pose[track]), bits(sample_tracks(clip, 30.0, CLAMP, t, int(policy))[track]))
    assert not np.array_equal(bits(pose[0]), bits(pose[1]))


def test_a_nan_in_a_key_frame_reaches_the_tracks_that_read_it_and_no_others():
    rng = np.random.default_rng(5401)
    clip = random_clip(rng, 6, 5)
    clean = clip.copy()
    clip[3, 2, 0] = np.nan          # rotation x of track 2 in key frame 3
    clip[3, 4, 5] = np.nan          # translation y of track 4 in key frame 3
    for i, t in enumerate(np.arange(0.0, 5.01, 0.25) / 30.0):
        k0, k1, _ = key_frames(6, 30.0, CLAMP, float(t))
        pose, want = sample_tracks(clip, 30.0, CLAMP, float(t)), sample_tracks(clean, 30.0, CLAMP, float(t))
        reads = 3 in (k0, k1)
        nans = np.isnan(pose)
        assert nans.sum() == (5 if reads else 0), i
        if reads:
            # (a key frame with weight 0 is still read: 0 * NaN is a NaN)
            assert nans[2, 0:4].all() and nans[4, 5]
        assert np.array_equal(bits(pose)[~nans], bits(want)[~nans])
