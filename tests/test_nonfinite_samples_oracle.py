"""Non-finite STORED samples, CPU side: the oracle against the reference's own decoder (oracle/_ref, built where the reference is
available) on every poisoned clip of nonfinite_clips.py, at the sample times around every poisoned key frame. No GPU.

Compared with same_numbers_and_nans: equal bits where the reference returns a number, a NaN where it returns a NaN. Before that,
every case asserts on the expected values alone that the NaN words lie in the poisoned sub-tracks only, that every NaN-word poison
shows, and that fewer than 5 % of the compared words are NaNs (nonfinite_clips.check_expectation). The W lanes of translations and
scales are unspecified in the reference and not compared (helpers.XYZ_LANES).

Under never-normalize (settings 5) the number lanes of a rotation that holds a NaN lane are decided by the SIGN of a NaN and are not
compared (nonfinite_clips.nan_sign_decided says why); they count towards the 5 %.

decompress_track and local_to_object_space are the comparisons with a tolerance: the reference normalizes from the x86 reciprocal
square root estimate there (test_oracle_vs_reference.py and test_pose_consumers_oracle.py state the tolerances), the oracle with a square
root and a division -- the project's documented choice. The NaN masks are equal EXCEPT for a rotation without a length
(its squared length overflowed or is 0): the estimate refines to four NaNs, the square root and division return zeros and infinities. Both
tests assert that relation in both directions, bone by bone; no rotation goes uncompared."""
import numpy as np
import pytest

from acl_amd import runtime
from oracle import bindings as ob
import helpers
import nonfinite_clips as nf
from test_pose_consumers_oracle import assert_object_space_close

needs_ref = pytest.mark.skipif(not ob.have_ref(), reason="oracle/_ref/libaclref.so not built (needs the reference checkout)")

CASES = nf.case_ids()
LANES = helpers.XYZ_LANES
TRACK_TOLERANCE = 1.0e-6       # decompress_track against the reference: test_oracle_vs_reference.py::test_decompress_track_close_to_reference


def reference(clip, t, rounding=ob.ROUND_NONE, **kwargs):
    return ob.ref_decompress(clip.blob, float(t), rounding, **kwargs)


def assert_same(got, want, what, never_normalized=False):
    if never_normalized:
        free = nf.nan_sign_decided(want)
        got, want = np.where(free, np.float32(0.0), got), np.where(free, np.float32(0.0), want)
    assert nf.same_numbers_and_nans(got[..., LANES], want[..., LANES]), f"{what}: {nf.describe_difference(got[..., LANES], want[..., LANES])}"


@needs_ref
@pytest.mark.parametrize("case", CASES)
def test_registration_accepts_the_poisoned_blob(case):
    """a refusal would be legitimate (the poison then leaves the builder); a silent difference is not. None is refused today."""
    clip = nf.poisoned_clip(case)
    status, message = runtime.check_clip(clip.blob, check_hash=False)
    assert status == 0, message
    assert ob.ref().aclref_is_valid(clip.blob.ctypes.data, 0) == 0
    assert len(clip.poisons) >= 2 and any(p.makes_nan for p in clip.poisons)


def test_every_poison_word_meets_every_placement():
    """over all cases: each of the 12 words is stored in a rotation x / y / z, a stored rotation W, a translation and a constant, each NaN word in a scale"""
    seen = {}
    for case in CASES:
        for poison in nf.poisoned_clip(case).poisons:
            where = "constant" if poison.constant else ("W" if poison.kind == 0 and poison.lane == 3 else ("rotation", "translation", "scale")[poison.kind])
            seen.setdefault(where, set()).add(poison.word)
    for where in ("rotation", "W", "translation", "constant"):
        assert seen.get(where, set()) == set(nf.POISON_WORDS), (where, [hex(w) for w in sorted(set(nf.POISON_WORDS) - seen.get(where, set()))])
    assert seen["scale"] >= {word for word in nf.POISON_WORDS if nf.is_nan_word(word)}         # (few clips animate a raw width scale)
    spans = {(p.window, p.ordinal) for case in CASES for p in nf.poisoned_clip(case).poisons if not p.constant}
    assert {(0, 63), (0, 64)} <= spans and any(window == 1 for window, _ in spans)


@needs_ref
@pytest.mark.parametrize("settings", [4, 1, 5])
@pytest.mark.parametrize("case", CASES)
def test_decompress_tracks_every_rounding_policy(case, settings):
    clip = nf.poisoned_clip(case)
    rng = np.random.default_rng(len(case))
    track_rounding = rng.integers(0, 4, size=clip.num_tracks).astype(np.uint8)
    policies = (0, 1, 2, 3, 4) if settings == 1 else (0, 1, 2, 3)
    options = helpers.oracle_options(settings, 0, None, track_rounding)
    for policy in policies:
        want = np.stack([reference(clip, t, policy, settings=settings, track_rounding=track_rounding) for t in clip.times])
        got = np.stack([ob.oracle_decompress_tracks(clip.blob, float(t), policy, options) for t in clip.times])
        never = settings == 5
        if policy == ob.ROUND_NONE:
            nf.check_expectation(clip, want, never_normalized=never)
            nf.check_expectation(clip, got, never_normalized=never)
        else:
            nf.check_expectation(clip, want, need_every_nan=False, never_normalized=never)
        assert_same(got, want, f"{clip.name} settings {settings} policy {policy}", never_normalized=never)


@needs_ref
@pytest.mark.parametrize("default_mode", [0, 1, 2, 3])
@pytest.mark.parametrize("case", CASES)
def test_default_sub_track_modes(case, default_mode):
    clip = nf.poisoned_clip(case)
    rng = np.random.default_rng(default_mode)
    defaults = rng.uniform(-1, 1, size=(clip.num_tracks if default_mode == 3 else 1, 12)).astype(np.float32)
    prefill = rng.uniform(-3, 3, size=(clip.num_tracks, 12)).astype(np.float32)
    options = helpers.oracle_options(4, default_mode, defaults)
    want = np.stack([reference(clip, t, settings=4, default_mode=default_mode, defaults=defaults, out=prefill.copy()) for t in clip.times])
    got = np.stack([ob.oracle_decompress_tracks(clip.blob, float(t), ob.ROUND_NONE, options, out=prefill.copy()) for t in clip.times])
    nf.check_expectation(clip, want)
    assert_same(got, want, f"{clip.name} default mode {default_mode}")


@needs_ref
@pytest.mark.parametrize("case", CASES)
def test_wrap_policy_override(case):
    """looping policy wrap for every clip: the interval behind the last sample interpolates towards the (poisoned) first one"""
    clip = nf.poisoned_clip(case)
    duration = ob.ref().aclref_get_duration(clip.blob.ctypes.data, ob.LOOP_WRAP)
    times = np.concatenate([clip.times, np.array([duration, (clip.duration + duration) / 2], dtype=np.float32)])
    options = helpers.oracle_options(4, looping=ob.LOOP_WRAP)
    want = np.stack([reference(clip, t, settings=4, looping=ob.LOOP_WRAP) for t in times])
    got = np.stack([ob.oracle_decompress_tracks(clip.blob, float(t), ob.ROUND_NONE, options) for t in times])
    nf.check_expectation(clip, want)
    assert_same(got, want, f"{clip.name} wrap")


@needs_ref
@pytest.mark.parametrize("case", CASES)
def test_decompress_track(case):
    clip = nf.poisoned_clip(case)
    tracks = sorted({t for p in clip.tracks for t in (p - 1, p, p + 1) if 0 <= t < clip.num_tracks})
    options = helpers.oracle_options(4)
    for t in clip.times:
        whole = ob.oracle_decompress_tracks(clip.blob, float(t), ob.ROUND_NONE, options)
        for track in tracks:
            want = np.zeros((clip.num_tracks, 12), dtype=np.float32)
            reference(clip, t, settings=4, track_index=track, out=want)
            got = ob.oracle_decompress_track(clip.blob, float(t), track, options=options)
            # Translations and scales: on bits. The rotation: the reference's decompress_track normalizes from a reciprocal square root
            # estimate -- close (1e-6, as test_oracle_vs_reference.py holds it) where the rotation has a length. Where it has none --
            # the squared length overflowed or is 0, so that every lane the whole-pose arithmetic returns is 0, an infinity or a NaN --
            # the estimate's refinement returns four NaNs, and the reference's two entry points disagree with each other; the library
            # returns the whole pose's row there ("decompress_track uses the whole-pose arithmetic"). Every rotation falls
            # under exactly one of the three assertions.
            what = f"{clip.name} track {track} t {t}"
            vectors = np.concatenate([np.zeros(4, dtype=np.float32), got[4:]]), np.concatenate([np.zeros(4, dtype=np.float32), want[track, 4:]])
            assert_same(vectors[0], vectors[1], what)
            rotation, theirs = whole[track, 0:4], want[track, 0:4]
            if np.isfinite(rotation).all() and rotation.any():
                assert np.abs(got[0:4] - theirs).max() <= TRACK_TOLERANCE, what
            elif nf.same_numbers_and_nans(got[0:4], theirs):
                pass                                                    # (a constant with a poisoned lane: neither side normalizes it)
            else:
                assert not (np.isfinite(rotation) & (rotation != 0)).any(), what + ": a lane with a length"
                assert nf.nan_mask(theirs).all(), what + ": the reference's rotation without a length is not four NaNs"
            assert_same(got, whole[track], what + " against the whole pose")


@needs_ref
@pytest.mark.skipif(not ob.have_ref_pose(), reason="oracle/_ref/libaclref_pose.so not built (needs the reference checkout)")
@pytest.mark.parametrize("case", CASES)
def test_pose_functions_on_poisoned_poses(case):
    clip = nf.poisoned_clip(case)
    # the reference's local_to_object_space knows one root, bone 0: the further roots of the clip's test forest hang off it here (where
    # bone 0 is poisoned itself, its NaNs then reach every bone; the 5 % cap is held on the forest below, the one the GPU tests use)
    parents = clip.parents.copy()
    parents[1:][parents[1:] == nf.NO_PARENT] = 0
    below = clip.descendants(parents)
    for index, t in enumerate(clip.times):
        poisoned = ob.oracle_decompress_tracks(clip.blob, float(t))
        clean = ob.oracle_decompress_tracks(clip.clean, float(clip.times[-1 - index]))
        for additive_format in range(4):
            for base, additive in ((poisoned, clean), (clean, poisoned)):
                want = ob.ref_apply_additive_to_base(additive_format, base, additive)
                got = ob.oracle_apply_additive_to_base(additive_format, base, additive)
                assert not nf.nan_mask(want)[~np.isin(np.arange(clip.num_tracks), clip.tracks)][:, LANES].any()
                assert_same(got, want, f"{clip.name} additive format {additive_format}")
        want = ob.ref_local_to_object_space(parents, poisoned)
        got = ob.oracle_local_to_object_space(parents, poisoned)
        # A rotation whose squared length overflows or is 0 (0x7F7FFFFF, the infinities) has no length: qvv_normalize's estimate refines to
        # four NaNs where the oracle's square root and division return zeros and infinities (acl_oracle.c, "restated with the
        # reference's own deterministic normalize"). Such a bone and everything below it is `tainted`; asserted both ways:
        #   the oracle's NaN words are NaN words of the reference;
        #   a NaN word of the reference that is a number in the oracle lies in a tainted bone;
        #   a bone without a length that the oracle did not already make NaNs of has four NaNs for a rotation in the reference;
        #   the bones that are not tainted hold numbers in both or in neither, and the numbers are close.
        ours, theirs = nf.nan_mask(got), nf.nan_mask(want)
        no_length = ~(np.isfinite(got[:, 0:4]) & (got[:, 0:4] != 0)).any(axis=1)
        tainted = no_length.copy()
        for bone in range(1, clip.num_tracks):
            tainted[bone] = tainted[bone] or tainted[parents[bone]]
        what = f"{clip.name} object space, t {t}"
        assert not (ours & ~theirs)[:, LANES].any(), what + ": a NaN the reference does not have"
        assert not (theirs & ~ours)[~tainted][:, LANES].any(), what + ": a NaN of the reference in a bone with a length"
        normalized = np.arange(clip.num_tracks) != 0                       # (bone 0, the root, is copied, not normalized, on both sides)
        assert theirs[normalized & no_length & ~ours[:, 0:4].all(axis=1)][:, 0:4].all(), what + ": the reference normalized a rotation without a length"
        assert not theirs[~below][:, LANES].any() and not tainted[~below].any(), what + ": outside the poisoned bones' subtrees"
        numbers = ~tainted & np.isfinite(want[:, LANES]).all(axis=1)
        assert np.array_equal(numbers, ~tainted & np.isfinite(got[:, LANES]).all(axis=1)), what
        if numbers.any():
            assert_object_space_close(got[numbers], want[numbers])
    want_all = np.stack([ob.oracle_local_to_object_space(clip.parents, ob.oracle_decompress_tracks(clip.blob, float(t))) for t in clip.times])
    nf.check_expectation(clip, want_all, object_space=True)
