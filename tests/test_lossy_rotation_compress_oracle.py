"""The restatement of tests/lossy_rotation_compress_restatement.py -- the definition aclhip_compress_tracks_batch is held to by
tests/test_gpu_lossy_rotation_compress.py -- against the reference's own compress_track_list (oracle/_ref/libaclref_compress.so,
aclref_compress_ex) with quatf_drop_w_full / vector3f_full / vector3f_full:

  equal           every byte outside the rotation VALUE words and the hash field: sizes, headers, the sample count behind the looping
                  vote, the wrap bit, every sub-track type, every constant and animated translation and scale, the metadata
  within 1e-5     the rotation value words (the project's standing bar for rtm::quat_normalize, DESIGN.md 8: the reference starts from the
                  x86 reciprocal square root estimate, the definition from the correctly rounded 1 / sqrt). The worst difference seen
                  here is 1.2e-7 (profiles/compress_tracks.md).
  the hash        recomputed over the restatement's own bytes, and through aclhip_check_clip with check_hash

A decision (the vote of a track, constant, default) whose error lies within rounding of its precision may fall either way in two
implementations; no case here has one: every test asserts, from the restatement's own record, that every error is at most half or at
least twice the precision it was compared with.

Per-track precisions and shell distances cannot be held to the reference -- the bridge sets one value for all tracks --: the sibling
tie and the "+ precision" rule of the shell are pinned against shells computed by hand instead. The bridge cannot register a wrapping
array either: its blob is held to the reference's for the clamped array plus the wrap bit. No GPU."""
import struct

import numpy as np
import pytest

from acl_amd import runtime
from oracle import bindings as ob
import lossy_rotation_compress_restatement as restatement
from lossy_rotation_compress_restatement import ANIMATED, CONSTANT, DEFAULT, IDENTITY, NO_PARENT, OPTIMIZE_LOOPS

RATE = 30.0
FORMATS = {"rotation_format": "quatf_drop_w_full", "translation_format": "vector3f_full", "scale_format": "vector3f_full"}
PRECISION, SHELL = 0.01, 3.0
TRACK_COUNTS, SAMPLE_COUNTS = (1, 2, 5, 17, 65), (1, 2, 3, 9)
SHAPES = [(t, s) for t in TRACK_COUNTS for s in SAMPLE_COUNTS]
TOLERANCE = 1.0e-5
worst_seen = [0.0]


@pytest.fixture(autouse=True)
def reference_compressor():
    """(asked when a test runs: the session's build makes the library)"""
    import os
    if not os.path.exists(ob.REF_COMPRESS_PATH):
        pytest.skip("oracle/_ref/libaclref_compress.so not built (it is made from the reference's sources)")


def reference(samples, default_pose=None, parents=None, flags=0, **settings):
    num_tracks = samples.shape[1]
    default_pose = np.tile(IDENTITY, (num_tracks, 1)) if default_pose is None else default_pose
    parents = np.full(num_tracks, NO_PARENT, dtype=np.uint32) if parents is None else parents
    settings.setdefault("precision", PRECISION)
    settings.setdefault("shell_distance", SHELL)
    names = {"optimize_loops": OPTIMIZE_LOOPS, "include_parent_track_indices": restatement.INCLUDE_PARENT_TRACK_INDICES, "include_track_descriptions": restatement.INCLUDE_TRACK_DESCRIPTIONS}
    switches = {name: True for name, bit in names.items() if flags & bit}
    return np.asarray(ob.ref_compress_ex(samples, RATE, parents=np.asarray(parents, dtype=np.uint32).view(np.int32), bind_pose=default_pose, **FORMATS, **switches, **settings)).view(np.uint8)


def ours(samples, default_pose=None, parents=None, flags=0, **settings):
    settings.setdefault("precision", PRECISION)
    settings.setdefault("shell_distance", SHELL)
    compressed = restatement.compress(samples, RATE, default_pose=default_pose, parents=parents, flags=flags, **settings)
    assert restatement.decisions_are_clear(compressed), [d for d in compressed.decisions if not (d[2] <= 0.5 * d[3] or d[2] >= 2.0 * d[3])]
    return compressed


def hold(compressed, theirs):
    """the three comparisons of the docstring; returns the blob"""
    blob, rotation_bytes = compressed.blob, compressed.rotation_bytes
    assert blob.size == theirs.size, (blob.size, theirs.size)
    compared = ~rotation_bytes
    compared[4:8] = False
    different = np.flatnonzero((blob != theirs) & compared)
    assert different.size == 0, (different[:8], blob[different[:8]], theirs[different[:8]])
    mine, reference_values = restatement.rotation_values(blob, rotation_bytes), restatement.rotation_values(theirs, rotation_bytes)
    if mine.size:
        assert np.isfinite(mine).all()
        worst = float(np.abs(mine - reference_values).max())
        worst_seen[0] = max(worst_seen[0], worst)
        print("worst rotation word difference %.3g (so far %.3g)" % (worst, worst_seen[0]))
        assert worst <= TOLERANCE, worst
    size, stored_hash = struct.unpack_from("<II", blob.tobytes(), 0)
    assert size == blob.size and stored_hash == restatement.fnv1a32(blob[8:])
    aligned = runtime_aligned(blob)
    status, message = runtime.check_clip(aligned, check_hash=True)
    assert status == 0, message
    return blob


def runtime_aligned(blob):
    from acl_amd.synth import aligned_bytes
    aligned = aligned_bytes(blob.size)
    aligned[:] = blob
    return aligned


def types_word(blob, kind=0):
    """the first packed sub-track types word of a kind (0 rotations, 1 translations)"""
    parsed = restatement.raw_restatement.parse(blob)
    words = (parsed["num_tracks"] + 15) // 16
    return struct.unpack_from("<I", blob.tobytes(), 100 + 4 * words * kind)[0]


# ---- the hierarchy decides ----------------------------------------------------------------------------------------------------------------
def hierarchy_clip(x):
    """S = 8, T = 3: track 0's rotation leans 5e-4 about x away from the identity (w about 1, x 5e-4) and jitters 2e-5 about that; track 2's
    translation is (x, 0, 0); everything else is the identity. At a shell of d the rotation is about d * 1e-3 from the default and at
    most about d * 1e-4 from its own sample 0."""
    rng = np.random.default_rng(4)
    samples = np.tile(IDENTITY, (8, 3, 1))
    q = np.zeros((8, 4))
    q[:, 3] = 1.0
    q[:, 0] = 5.0e-4
    q[:, 0:3] += rng.uniform(-1.0, 1.0, size=(8, 3)) * 2.0e-5
    samples[:, 0, 0:4] = (q / np.linalg.norm(q, axis=1, keepdims=True)).astype(np.float32)
    samples[:, 2, 4] = x
    return samples


ROOTS = np.full(3, NO_PARENT, dtype=np.uint32)
CHAIN = np.array([NO_PARENT, 0, 1], dtype=np.uint32)


@pytest.mark.parametrize("parents,x,rotation_type,word,size", [(ROOTS, 1000.0, DEFAULT, 0x00000000, 135), (CHAIN, 30.0, CONSTANT, 0x40000000, 147), (CHAIN, 1000.0, ANIMATED, 0x80000000, 231)],
                         ids=["roots", "short_chain", "long_chain"])
def test_the_hierarchy_decides(parents, x, rotation_type, word, size):
    """the same jitter is default under its own shell of 3, constant under the 33 of a child 30 away, animated under the 1003 of a
    child 1000 away: 100 bytes of headers, 8 of types, 12 of track 2's constant translation, the 15 byte tail; 12 more for a constant
    rotation; 8 * 12 for an animated one"""
    samples = hierarchy_clip(x)
    compressed = ours(samples, parents=parents)
    blob = hold(compressed, reference(samples, parents=parents))
    assert compressed.types[0, 0] == rotation_type and (compressed.types[0, 1:] == DEFAULT).all()
    assert types_word(blob) == word and blob.size == size
    if parents is CHAIN:
        # by hand: track 2 stretches its shell of 3 to 3 + x, which is track 1's; track 1 is not dominant: its precision comes on top
        assert compressed.shells[1, 0] == np.float32(3.0 + x) and compressed.shells[0, 0] == np.float32(np.float32(3.0 + x) + np.float32(PRECISION))
    else:
        assert (compressed.shells[:, 0] == np.float32(3.0)).all()


# ---- the sweep ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("num_tracks,num_samples", SHAPES, ids=["%dx%d" % shape for shape in SHAPES])
def test_the_sweep_is_the_reference(num_tracks, num_samples):
    """random trees; three seeds walk the mixes of animated / jittering about a rotation / jittering about the default / fixed rotations
    and animated / constant / default translations and scales; loops on and off, with last == first and not"""
    voted = 0
    for seed in range(3):
        parents = restatement.tree(seed, num_tracks)
        for flags in (0, OPTIMIZE_LOOPS):
            for close_loop in (False, True):
                samples = restatement.clip(seed, num_samples, num_tracks, close_loop=close_loop)
                compressed = ours(samples, parents=parents, flags=flags)
                hold(compressed, reference(samples, parents=parents, flags=flags))
                voted += compressed.wrap
                if flags and close_loop and num_samples > 1:
                    assert compressed.wrap and compressed.num_samples == num_samples - 1
                if not flags:
                    assert not compressed.wrap and compressed.num_samples == num_samples
    assert voted >= (3 if num_samples > 1 else 0)


def test_every_rotation_type_is_there():
    compressed = ours(restatement.clip(0, 9, 17), parents=restatement.tree(0, 17))
    assert {DEFAULT, CONSTANT, ANIMATED} == set(compressed.types[0].tolist()) == set(compressed.types[1].tolist()) == set(compressed.types[2].tolist())
    kinds = {what for what, _, _, _ in ours(restatement.clip(0, 9, 17), flags=OPTIMIZE_LOOPS).decisions}
    assert kinds == {"vote", "constant", "default"}


def test_a_wrapping_array_keeps_its_samples_and_is_marked():
    samples = restatement.clip(1, 9, 5, close_loop=True)
    parents = restatement.tree(1, 5)
    clamped = ours(samples, parents=parents)
    for flags in (0, OPTIMIZE_LOOPS):
        wrapped = ours(samples, parents=parents, flags=flags, looping_wrap=True)
        assert wrapped.wrap and wrapped.num_samples == 9 and not [d for d in wrapped.decisions if d[0] == "vote"]
        expected = clamped.blob.copy()
        expected[8 + 20 + 3] |= 0x40                 # bit 30 of the tracks_header's packed word
        expected[4:8] = np.frombuffer(struct.pack("<I", restatement.fnv1a32(expected[8:])), dtype=np.uint8)
        assert np.array_equal(wrapped.blob, expected)
    hold(clamped, reference(samples, parents=parents))


def test_negative_w_on_whole_tracks_and_on_single_samples():
    samples = restatement.clip(2, 9, 17)
    parents = restatement.tree(2, 17)
    plain = ours(samples, parents=parents)
    flipped = samples.copy()
    flipped[:, 1::2, 0:4] = -flipped[:, 1::2, 0:4]          # whole tracks
    flipped[3, :, 0:4] = -flipped[3, :, 0:4]                # one sample of every track
    flipped[5, 4, 0:4] = -flipped[5, 4, 0:4]
    assert (flipped[:, :, 3] < 0).any() and (flipped[:, :, 3] > 0).any()
    compressed = ours(flipped, parents=parents)
    blob = hold(compressed, reference(flipped, parents=parents))
    # q and -q are one rotation: the same blob (normalizing commutes with the sign)
    assert np.array_equal(blob, plain.blob)
    # a w of -0 flips too
    zero_w = samples.copy()
    zero_w[:, 0, 0:4] = np.array([0.6, 0.0, 0.8, -0.0], dtype=np.float32)
    compressed = ours(zero_w, parents=parents)
    hold(compressed, reference(zero_w, parents=parents))
    assert compressed.types[0, 0] == CONSTANT and int((compressed.types[0] == CONSTANT).sum()) >= 4
    # the first constant rotation of a full group of four: x at word 0, y at word 4, z at word 8 (xxxx yyyy zzzz)
    stored = restatement.rotation_values(compressed.blob, compressed.rotation_bytes)[[0, 4, 8]]
    assert np.array_equal(stored.view(np.uint32), np.array([-0.6, -0.0, -0.8], dtype=np.float32).view(np.uint32))


def test_a_default_rotation_that_is_not_the_identity():
    pose = restatement.raw_restatement.bind_pose(21, 17)
    pose[::2, 0:4] = -pose[::2, 0:4]                        # (used as given: not converted)
    parents = restatement.tree(3, 17)
    samples = restatement.clip(0, 9, 17, default_pose=pose)
    compressed = ours(samples, default_pose=pose, parents=parents)
    hold(compressed, reference(samples, default_pose=pose, parents=parents))
    assert (compressed.types[0] == DEFAULT).any()
    against_identity = ours(samples, parents=parents)
    hold(against_identity, reference(samples, parents=parents))
    assert against_identity.blob.size > compressed.blob.size and not (against_identity.types[0] == DEFAULT).any()


def test_a_rotation_of_length_two_is_normalized_and_a_zero_quaternion_is_not_finite():
    samples = restatement.clip(1, 3, 5)
    parents = restatement.tree(1, 5)
    long = samples.copy()
    long[:, 2, 0:4] = np.array([0.0, 0.0, 0.0, 2.0], dtype=np.float32)
    long[1, 3, 0:4] *= np.float32(2.0)
    compressed = ours(long, parents=parents)
    hold(compressed, reference(long, parents=parents))
    assert compressed.types[0, 2] == DEFAULT
    unit = samples.copy()                                   # (a power of two scales every step of the normalization exactly)
    unit[:, 2, 0:4] = IDENTITY[0:4]
    assert np.array_equal(compressed.blob, ours(unit, parents=parents).blob)
    zero = samples.copy()
    zero[1, 3, 0:4] = 0.0
    with pytest.raises(ValueError, match=restatement.NOT_FINITE_MESSAGE):
        restatement.compress(zero, RATE, parents=parents, precision=PRECISION, shell_distance=SHELL)
    with pytest.raises(RuntimeError, match=restatement.NOT_FINITE_MESSAGE):
        reference(zero, parents=parents)
    for lane, value in ((0, np.nan), (5, np.inf), (9, -np.inf)):
        bad = samples.copy()
        bad[2, 1, lane] = value
        with pytest.raises(ValueError, match=restatement.NOT_FINITE_MESSAGE):
            restatement.compress(bad, RATE, parents=parents, precision=PRECISION, shell_distance=SHELL)
        with pytest.raises(RuntimeError, match=restatement.NOT_FINITE_MESSAGE):
            reference(bad, parents=parents)


def test_the_metadata_and_has_scale_both_ways():
    both = restatement.INCLUDE_PARENT_TRACK_INDICES | restatement.INCLUDE_TRACK_DESCRIPTIONS
    for num_tracks, num_samples in ((1, 1), (5, 9), (17, 2)):
        parents = restatement.tree(5, num_tracks)
        pose = restatement.raw_restatement.bind_pose(3, num_tracks)
        for scales in ("mixed", "default"):
            for default_pose in (None, pose):
                samples = restatement.clip(1, num_samples, num_tracks, default_pose=default_pose, scales=scales)
                for flags in (restatement.INCLUDE_PARENT_TRACK_INDICES, restatement.INCLUDE_TRACK_DESCRIPTIONS, both | OPTIMIZE_LOOPS):
                    compressed = ours(samples, default_pose=default_pose, parents=parents, flags=flags)
                    blob = hold(compressed, reference(samples, default_pose=default_pose, parents=parents, flags=flags))
                    parsed = restatement.raw_restatement.parse(blob)
                    assert parsed["has_metadata"] and parsed["has_scale"] == (scales == "mixed" and num_tracks > 1 or bool((compressed.types[2] != DEFAULT).any()))
                    assert (parsed["misc"] >> 4) & 15 == restatement.QUATF_DROP_W_FULL
        assert not restatement.raw_restatement.parse(ours(restatement.clip(1, num_samples, num_tracks, scales="default"), parents=parents).blob)["has_scale"]


def test_a_forward_parent_is_refused():
    samples = restatement.clip(0, 3, 5)
    for parents in ([NO_PARENT, 0, 3, 0, 0], [0, NO_PARENT, 1, 2, 3], [NO_PARENT, 0, 1, 2, 4]):
        with pytest.raises(restatement.Refused):
            restatement.compress(samples, RATE, parents=np.array(parents, dtype=np.uint32))
    # a parent that is no track of the array is no parent
    restatement.compress(samples, RATE, parents=np.array([NO_PARENT, 5, 77, 0, 1], dtype=np.uint32))


# ---- per-track precisions and shell distances: by hand ----------------------------------------------------------------------------------------
def leaning(num_samples, lean):
    """a rotation about x by about 2 * lean: at a shell of d it is about 2 * d * lean from the identity (the points on y and z move)"""
    q = np.zeros((num_samples, 4))
    q[:, 3] = 1.0
    q[1::2, 0] = lean
    return (q / np.linalg.norm(q, axis=1, keepdims=True)).astype(np.float32)


def test_of_siblings_with_the_same_stretch_the_highest_index_hands_its_precision_up():
    """tracks 1 and 2 hang below track 0 with identical samples, a translation of (1, 0, 0): both stretch their shell of 3 to 4, the
    comparison is strict, and the visit runs from the highest index down: track 2's precision becomes track 0's. Track 0's rotation
    moves 0.01 at that shell, between the two precisions: the type flips with the order of the two"""
    samples = np.tile(IDENTITY, (4, 3, 1))
    samples[:, 1:, 4] = 1.0
    samples[:, 0, 0:4] = leaning(4, 0.00125)           # 2 * 4 * 0.00125 = 0.01
    parents = np.array([NO_PARENT, 0, 0], dtype=np.uint32)
    for precisions, rotation_type in (((0.05, 0.001, 0.1), DEFAULT), ((0.05, 0.1, 0.001), ANIMATED)):
        compressed = ours(samples, parents=parents, track_precisions=np.array(precisions, dtype=np.float32))
        expected = np.array([[4.0, precisions[2]], [3.0, precisions[1]], [3.0, precisions[2]]], dtype=np.float32)
        assert np.array_equal(compressed.shells.view(np.uint32), expected.view(np.uint32))
        assert compressed.types[0, 0] == rotation_type
    # the parent's own distance wins a tie: a shell distance of 4 of its own keeps its own precision
    compressed = ours(samples, parents=parents, track_precisions=np.array((0.05, 0.001, 0.001), dtype=np.float32), track_shell_distances=np.array((4.0, 3.0, 3.0), dtype=np.float32))
    assert np.array_equal(compressed.shells[0], np.array([4.0, 0.05], dtype=np.float32)) and compressed.types[0, 0] == DEFAULT


def test_a_transform_that_is_not_dominant_adds_its_own_precision():
    """a chain 0 <- 1 <- 2: track 2 stretches 3 to 4 and hands { 4, its precision } to track 1; track 1's distance is no longer its own,
    so what it hands up is its stretch (4, it does not move) plus ITS OWN precision, with the precision it was handed"""
    samples = np.tile(IDENTITY, (4, 3, 1))
    samples[:, 2, 4] = 1.0
    parents = np.array([NO_PARENT, 0, 1], dtype=np.uint32)
    precisions = np.array((0.05, 0.25, 0.001), dtype=np.float32)
    compressed = ours(samples, parents=parents, track_precisions=precisions)
    expected = np.array([[np.float32(4.0) + np.float32(0.25), 0.001], [4.0, 0.001], [3.0, 0.001]], dtype=np.float32)
    assert np.array_equal(compressed.shells.view(np.uint32), expected.view(np.uint32))
    # per-track shell distances: a dominant child's own distance is what it stretches
    compressed = ours(samples, parents=parents, track_precisions=precisions, track_shell_distances=np.array((1.0, 1.0, 7.0), dtype=np.float32))
    expected = np.array([[np.float32(8.0) + np.float32(0.25), 0.001], [8.0, 0.001], [7.0, 0.001]], dtype=np.float32)
    assert np.array_equal(compressed.shells.view(np.uint32), expected.view(np.uint32))
    # the descriptions carry the tracks' own values, not the shell's
    flags = restatement.INCLUDE_TRACK_DESCRIPTIONS
    blob = ours(samples, parents=parents, track_precisions=precisions, flags=flags).blob
    descriptions = np.frombuffer(blob.tobytes(), dtype=np.float32, count=36, offset=blob.size - 20 - 48 * 3).reshape(3, 12)
    assert np.array_equal(descriptions[:, 0], precisions) and (descriptions[:, 1] == np.float32(SHELL)).all()
    uniform = ours(samples, parents=parents, precision=0.25, flags=flags)
    hold(uniform, reference(samples, parents=parents, precision=0.25, flags=flags))
