"""The restatement of tests/transform_compress_restatement.py -- the definition aclhip_compress_raw_tracks_batch is held to by
tests/test_gpu_transform_compress.py -- against the reference's own compress_track_list with the raw compression settings
(oracle/_ref/libaclref_compress.so, aclref_compress_ex with quatf_full / vector3f_full / vector3f_full) ON EVERY BYTE, hash included:
the sweep of track and sample counts, every mix of animated, constant and default sub-tracks, no scale section, non-identity default
values, zeros of both signs, non-finite fourth lanes, the optional metadata, the settings that change no byte, the reference's error for
a sample that is not finite, and rotation lengths on both sides of the reference's normalization threshold.

The bridge hands the reference records made by rtm::vector_load3: the fourth lanes of translations, scales and bind pose are +0 on both
sides. The default pose is therefore always given explicitly (the identity included): qvv_identity's own scale holds 1 in its fourth lane,
which the reference's four lane comparison would hold against a sample's +0. No GPU."""
import numpy as np
import pytest

from oracle import bindings as ob
import transform_compress_restatement as restatement
from transform_compress_restatement import IDENTITY, NO_PARENT, SAMPLE_COUNTS, TRACK_COUNTS

RATE = 30.0
RAW_FORMATS = {"rotation_format": "quatf_full", "translation_format": "vector3f_full", "scale_format": "vector3f_full"}
SHAPES = [(t, s) for t in TRACK_COUNTS for s in SAMPLE_COUNTS]


@pytest.fixture(autouse=True)
def reference_compressor():
    """(asked when a test runs: the session's build makes the library)"""
    import os
    if not os.path.exists(ob.REF_COMPRESS_PATH):
        pytest.skip("oracle/_ref/libaclref_compress.so not built (it is made from the reference's sources)")


def reference(samples, default_pose=None, parents=None, **settings):
    num_tracks = samples.shape[1]
    default_pose = np.tile(IDENTITY, (num_tracks, 1)) if default_pose is None else default_pose
    parents = np.full(num_tracks, NO_PARENT, dtype=np.uint32) if parents is None else parents
    return np.asarray(ob.ref_compress_ex(samples, RATE, parents=np.asarray(parents, dtype=np.uint32).view(np.int32), bind_pose=default_pose, **RAW_FORMATS, **settings)).view(np.uint8)


def same_bytes(ours, theirs):
    assert ours.size == theirs.size, (ours.size, theirs.size)
    different = np.flatnonzero(ours != theirs)
    assert different.size == 0, (different[:8], ours[different[:8]], theirs[different[:8]])
    return ours


@pytest.mark.parametrize("num_tracks,num_samples", SHAPES, ids=["%dx%d" % shape for shape in SHAPES])
def test_the_sweep_is_the_reference_on_every_byte(num_tracks, num_samples):
    """three seeds walk the 27 mixes of animated / constant / default over the tracks; identity and non-identity default values; every
    scale default (no scale section), also against a non-identity bind pose"""
    for seed in range(3):
        samples = restatement.clip(seed, num_samples, num_tracks)
        blob = same_bytes(restatement.compress(samples, RATE), reference(samples))
        # the input's own bytes are in the blob: the reference kept the rotations as they were
        parsed = restatement.parse(blob)
        if parsed["num_constant"][0] != 0:
            track = int(np.flatnonzero(restatement.classify(samples, np.tile(IDENTITY, (num_tracks, 1)))[0][0] == restatement.CONSTANT)[0])
            assert samples[0, track, 0:4].tobytes() in blob.tobytes()
        pose = restatement.bind_pose(seed, num_tracks)
        samples = restatement.clip(seed, num_samples, num_tracks, default_pose=pose)
        same_bytes(restatement.compress(samples, RATE, default_pose=pose), reference(samples, default_pose=pose))
        for default_pose in (None, pose):
            samples = restatement.clip(seed, num_samples, num_tracks, default_pose=default_pose, scales="default")
            blob = same_bytes(restatement.compress(samples, RATE, default_pose=default_pose), reference(samples, default_pose=default_pose))
            assert not restatement.parse(blob)["has_scale"]


def test_every_mix_of_sub_track_types_is_there():
    seen = set()
    for seed in range(3):
        types, has_scale = restatement.classify(restatement.clip(seed, 7, 65), np.tile(IDENTITY, (65, 1)))
        assert has_scale
        seen |= {tuple(column) for column in types.T.tolist()}
    assert len(seen) == 27


def test_the_sizes_of_a_small_clip():
    """5 tracks of 7 samples, everything animated: 100 bytes of headers, 3 words of sub-track types, 40 bytes per track and sample, the
    tail; every scale 1: the scale third of the types and of the stream is gone; one sample: everything is constant; both metadata
    sections: 4 + 48 bytes per track and the 20 byte header instead of the tail"""
    rng = np.random.default_rng(5)
    samples = np.zeros((7, 5, 12), dtype=np.float32)
    samples[:, :, 0:4] = restatement.unit_quaternions(rng, (7, 5))
    samples[:, :, 4:7] = rng.uniform(-1.0, 1.0, size=(7, 5, 3))
    samples[:, :, 8:11] = rng.uniform(0.5, 2.0, size=(7, 5, 3))
    assert same_bytes(restatement.compress(samples, RATE), reference(samples)).size == 100 + 12 + 40 * 5 * 7 + 15
    no_scale = samples.copy()
    no_scale[:, :, 8:11] = 1.0
    assert same_bytes(restatement.compress(no_scale, RATE), reference(no_scale)).size == 100 + 8 + 28 * 5 * 7 + 15
    assert same_bytes(restatement.compress(samples[:1], RATE), reference(samples[:1])).size == 100 + 12 + 40 * 5 + 15
    parents = restatement.chain_parents(5)
    flags = restatement.INCLUDE_PARENT_TRACK_INDICES | restatement.INCLUDE_TRACK_DESCRIPTIONS
    blob = same_bytes(restatement.compress(samples, RATE, parents=parents, flags=flags), reference(samples, parents=parents, include_parent_track_indices=True, include_track_descriptions=True))
    assert blob.size == 100 + 12 + 40 * 5 * 7 + 52 * 5 + 20


def test_a_constant_track_that_equals_a_non_identity_default():
    pose = restatement.bind_pose(11, 6)
    samples = restatement.clip(1, 9, 6, default_pose=pose)
    samples[:, 2] = pose[2]
    blob = same_bytes(restatement.compress(samples, RATE, default_pose=pose), reference(samples, default_pose=pose))
    types, _ = restatement.classify(samples, pose)
    assert (types[:, 2] == restatement.DEFAULT).all()
    # against the identity the same samples are constant, not default
    other = same_bytes(restatement.compress(samples, RATE), reference(samples))
    assert other.size > blob.size


def test_zeros_of_both_signs():
    """-0 == +0: a translation track of +0 whose sample 0 is -0 is default against a zero default; a track of zeros of both signs is
    constant and stores the bits of sample 0"""
    samples = restatement.clip(2, 7, 5)
    samples[:, 1, 4:7] = 0.0
    plain = same_bytes(restatement.compress(samples, RATE), reference(samples))
    samples[0, 1, 4:7] = -0.0
    signed = same_bytes(restatement.compress(samples, RATE), reference(samples))
    assert signed.size == plain.size
    assert restatement.classify(samples, np.tile(IDENTITY, (5, 1)))[0][1, 1] == restatement.DEFAULT
    # a constant track of mixed zeros: sample 0's sign is what the blob holds
    for first in (0.0, -0.0):
        samples[:, 3, 4:7] = np.float32(2.5)
        samples[:, 3, 5] = np.where(np.arange(7) % 2 == 0, np.float32(first), -np.float32(first))
        assert restatement.classify(samples, np.tile(IDENTITY, (5, 1)))[0][1, 3] == restatement.CONSTANT
        blob = same_bytes(restatement.compress(samples, RATE), reference(samples))
        assert samples[0, 3, 4:7].tobytes() in blob.tobytes()
    # and against a default of -0
    pose = np.tile(IDENTITY, (5, 1))
    pose[1, 4:7] = -0.0
    same_bytes(restatement.compress(samples, RATE, default_pose=pose), reference(samples, default_pose=pose))


def test_the_fourth_lanes_of_translations_and_scales_change_nothing():
    samples = restatement.clip(0, 7, 17)
    blob = restatement.compress(samples, RATE)
    same_bytes(blob, reference(samples))
    for value in (np.nan, np.inf, -np.inf, 1.0e30):
        other = samples.copy()
        other[:, :, 7] = value
        other[3, :, 11] = value
        same_bytes(restatement.compress(other, RATE), blob)
        same_bytes(reference(other), blob)


def test_the_metadata_is_the_reference_on_every_byte():
    for num_tracks, num_samples in ((1, 1), (5, 7), (17, 2), (65, 7)):
        pose = restatement.bind_pose(3, num_tracks)
        samples = restatement.clip(1, num_samples, num_tracks, default_pose=pose)
        parents = restatement.chain_parents(num_tracks)
        for flags, settings in ((restatement.INCLUDE_PARENT_TRACK_INDICES, {"include_parent_track_indices": True}),
                                (restatement.INCLUDE_TRACK_DESCRIPTIONS, {"include_track_descriptions": True}),
                                (restatement.INCLUDE_PARENT_TRACK_INDICES | restatement.INCLUDE_TRACK_DESCRIPTIONS, {"include_parent_track_indices": True, "include_track_descriptions": True})):
            for default_pose in (None, pose):
                ours = restatement.compress(samples, RATE, default_pose=default_pose, parents=parents, flags=flags, precision=0.01, shell_distance=3.0)
                blob = same_bytes(ours, reference(samples, default_pose=default_pose, parents=parents, precision=0.01, shell_distance=3.0, **settings))
                assert restatement.parse(blob)["has_metadata"] and blob.size % 4 == 0
    # the tables: one precision and one shell distance per track land where the reference puts its single ones
    samples = restatement.clip(1, 7, 5)
    flags = restatement.INCLUDE_TRACK_DESCRIPTIONS
    uniform = restatement.compress(samples, RATE, flags=flags, precision=0.25, shell_distance=2.0)
    tables = restatement.compress(samples, RATE, flags=flags, track_precisions=np.full(9, 0.25), track_shell_distances=np.full(9, 2.0))
    same_bytes(tables, uniform)


def test_the_settings_that_change_no_byte():
    samples = restatement.clip(1, 7, 17)
    samples[-1] = samples[0]            # a last key frame equal to the first: optimize_loops still removes nothing
    blob = same_bytes(restatement.compress(samples, RATE), reference(samples))
    assert restatement.parse(blob)["num_samples"] == 7 and not restatement.parse(blob)["wrap"]
    for settings in ({"optimize_loops": True}, {"level": "lowest"}, {"level": "highest"}, {"precision": 0.5}, {"shell_distance": 100.0},
                     {"parents": restatement.chain_parents(17)}):
        same_bytes(reference(samples, **settings), blob)


def test_a_sample_that_is_not_finite_raises_on_both_sides():
    """a NaN or an Inf in each used lane"""
    good = restatement.clip(0, 7, 5)
    for lane in (0, 1, 2, 3, 4, 5, 6, 8, 9, 10):
        for value in (np.nan, np.inf, -np.inf):
            samples = good.copy()
            samples[4, 2, lane] = value
            with pytest.raises(ValueError, match=restatement.NOT_FINITE_MESSAGE):
                restatement.compress(samples, RATE)
            with pytest.raises(RuntimeError, match=restatement.NOT_FINITE_MESSAGE):
                reference(samples)


def test_the_normalized_test_is_true_exactly_when_the_reference_keeps_the_rotation():
    """rotation lengths on both sides of the 1e-5 threshold, one constant rotation track per clip: where the restatement's predicate holds the blob
    holds the rotation's own bytes (and the restatement's blob is the reference's); where it does not, the reference has renormalized
    and the bytes are gone"""
    rng = np.random.default_rng(99)
    base = restatement.clip(2, 3, 4)
    kept = changed = 0
    for scale in (1.0 - 2.0e-5, 1.0 - 6.0e-6, 1.0 - 5.2e-6, 1.0 - 5.0e-6, 1.0 - 4.9e-6, 1.0 - 4.0e-6, 1.0, 1.0 + 4.0e-6, 1.0 + 4.9e-6, 1.0 + 5.0e-6, 1.0 + 5.1e-6, 1.0 + 6.0e-6, 1.0 + 2.0e-5):
        for _ in range(6):
            q = restatement.unit_quaternions(rng, ()).astype(np.float64) * scale
            samples = base.copy()
            samples[:, 2, 0:4] = q.astype(np.float32)       # a constant sub-track: its sample 0 is stored as it is
            theirs = reference(samples)
            needle = samples[0, 2, 0:4].tobytes()
            if restatement.rotations_normalized(samples[0, 2, 0:4]):
                kept += 1
                same_bytes(restatement.compress(samples, RATE), theirs)
                assert needle in theirs.tobytes()
            else:
                changed += 1
                assert needle not in theirs.tobytes()
                with pytest.raises(restatement.NotNormalized):
                    restatement.compress(samples, RATE)
    assert kept >= 30 and changed >= 30
    # not finite wins over not normalized
    samples = base.copy()
    samples[1, 2, 0:4] *= np.float32(1.5)
    samples[2, 0, 5] = np.inf
    with pytest.raises(ValueError, match=restatement.NOT_FINITE_MESSAGE):
        restatement.compress(samples, RATE)
