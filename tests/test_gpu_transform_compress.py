"""aclhip_compress_raw_tracks_batch through the C ABI: compress_track_list with the reference's raw compression settings of registered
raw track arrays. The expected blobs are the restatement's (tests/transform_compress_restatement.py, which
tests/test_transform_compress_oracle.py holds to the reference's compressor on every byte), and every comparison of blobs is on BYTES:
the definition has no tolerance.

The output region is one flat buffer filled with a sentinel byte: a guard, n rows of `stride` bytes, a guard. One comparison holds
[0, size) of every row to the blob and everything else -- the bytes behind `size`, refused rows, the guards -- to the sentinel.
The sample rate is a power of two, so that the key times i / rate and their products with the rate are exact. Needs a GPU."""
import numpy as np
import pytest

from acl_amd import runtime
import compress_launches as launches
import transform_compress_restatement as restatement
from compress_launches import RATE, Entry, Registered, check_rows, ctx, same  # noqa: F401  (ctx: this module's fixture)
from transform_compress_restatement import IDENTITY, LANES, SAMPLE_COUNTS, TRACK_COUNTS

pytestmark = pytest.mark.gpu

PARENTS, DESCRIPTIONS = restatement.INCLUDE_PARENT_TRACK_INDICES, restatement.INCLUDE_TRACK_DESCRIPTIONS
SHAPES = [(t, s) for t in TRACK_COUNTS for s in SAMPLE_COUNTS] + [(2, 64), (2, 129), (130, 3)]      # samples around a wave's 64 lanes; three turns of 64 tracks


def launch(ctx, handles, shapes, flags=0, precision=1.0e-4, shell_distance=1.0, stride=None, max_tracks=None, **settings):
    """One launch of the raw call over `handles` (tests/compress_launches.py). `shapes`: (T, S) per instance, or one for all, for the
    default stride (the largest bound) and max_tracks."""
    if stride is None:
        stride = max(runtime.transform_compress_bound(tracks, samples, flags) for tracks, samples in shapes)
    if max_tracks is None:
        max_tracks = max(tracks for tracks, _ in shapes)
    return launches.launch(ctx, Entry("raw"), handles, max_tracks, stride=stride, flags=flags, precision=precision, shell_distance=shell_distance, **settings)


def shapes_of(clips):
    return [(samples.shape[1], samples.shape[0]) for samples in clips]


@pytest.fixture(scope="module")
def sweep(ctx):
    """every shape, one seed each (the seeds walk the 27 mixes of sub-track types), against the identity: one launch serves them all"""
    with Registered(ctx) as arrays:
        clips = [restatement.clip(k % 3, num_samples, num_tracks) for k, (num_tracks, num_samples) in enumerate(SHAPES)]
        yield ctx, [arrays.add(samples) for samples in clips], clips


def test_the_blobs_are_the_restatement(sweep):
    ctx, handles, clips = sweep
    expected = [restatement.compress(samples, RATE) for samples in clips]
    check_rows(launch(ctx, handles, shapes_of(clips)), expected)
    # ACLHIP_COMPRESS_OPTIMIZE_LOOPS is accepted and changes nothing
    check_rows(launch(ctx, handles, shapes_of(clips), flags=runtime.COMPRESS_OPTIMIZE_LOOPS), expected)
    kinds = np.array([restatement.parse(blob)["num_animated"] + restatement.parse(blob)["num_constant"] for blob in expected])
    assert (kinds.max(axis=0) > 0).all() and (kinds.min(axis=0) == 0).all()


def test_a_default_pose_that_is_not_the_identity_and_no_scale_section(ctx):
    """the tracks of every array compared with one shared bind pose of 130 records: defaults against it, constants that equal the
    identity instead; every scale the default: has_scale is off, against the identity and against the bind pose"""
    pose = restatement.bind_pose(21, 130)
    with Registered(ctx) as arrays:
        clips = []
        for k, (num_tracks, num_samples) in enumerate(SHAPES):
            clips.append(restatement.clip(k % 3, num_samples, num_tracks, default_pose=pose[:num_tracks], scales="default" if k % 2 else "mixed"))
        handles = [arrays.add(samples) for samples in clips]
        expected = [restatement.compress(samples, RATE, default_pose=pose) for samples in clips]
        check_rows(launch(ctx, handles, shapes_of(clips), default_pose=pose), expected)
        assert any(not restatement.parse(blob)["has_scale"] for blob in expected) and any(restatement.parse(blob)["has_scale"] for blob in expected)
        # the same arrays against the identity: what was default is constant now
        against_identity = [restatement.compress(samples, RATE) for samples in clips]
        check_rows(launch(ctx, handles, shapes_of(clips)), against_identity)
        assert sum(blob.size for blob in against_identity) > sum(blob.size for blob in expected)
        no_scale = [restatement.clip(k % 3, num_samples, num_tracks, scales="default") for k, (num_tracks, num_samples) in enumerate(SHAPES[::3])]
        expected = [restatement.compress(samples, RATE) for samples in no_scale]
        assert not any(restatement.parse(blob)["has_scale"] for blob in expected)
        check_rows(launch(ctx, [arrays.add(samples) for samples in no_scale], shapes_of(no_scale)), expected)


def test_zeros_of_both_signs_and_fourth_lanes_that_are_not_finite(ctx):
    samples = restatement.clip(2, 7, 5)
    samples[:, 1, 4:7] = 0.0
    samples[0, 1, 4:7] = -0.0                           # default: -0 == +0
    samples[:, 3, 4:7] = np.float32(2.5)
    samples[:, 3, 5] = np.where(np.arange(7) % 2 == 0, np.float32(-0.0), np.float32(0.0))       # constant: sample 0's -0 is stored
    poisoned = samples.copy()
    poisoned[:, :, 7] = np.nan
    poisoned[2, :, 11] = np.inf
    pose = np.tile(IDENTITY, (5, 1))
    pose[:, 7] = np.nan                                  # the fourth lanes of the default pose are not read either
    pose[1, 4:7] = -0.0
    with Registered(ctx) as arrays:
        handles = [arrays.add(samples), arrays.add(poisoned)]
        blob = restatement.compress(samples, RATE)
        types, _ = restatement.classify(samples, np.tile(IDENTITY, (5, 1)))
        assert types[1, 1] == restatement.DEFAULT and types[1, 3] == restatement.CONSTANT and samples[0, 3, 4:7].tobytes() in blob.tobytes()
        check_rows(launch(ctx, handles, [(5, 7)]), [blob, blob])
        check_rows(launch(ctx, handles, [(5, 7)], default_pose=pose), [blob, blob])


def test_the_metadata(ctx):
    """parent indices alone, descriptions (which imply them), both; with and without the tables; a parent that is no track is no parent"""
    with Registered(ctx) as arrays:
        clips = [restatement.clip(1, num_samples, num_tracks) for num_tracks, num_samples in ((1, 1), (5, 7), (17, 2), (65, 7), (130, 3))]
        handles = [arrays.add(samples) for samples in clips]
        pose = restatement.bind_pose(3, 130)
        parents = restatement.chain_parents(130)
        parents[3] = 4          # (no track of the array of one track; a forward reference elsewhere: written as it is)
        precisions = np.linspace(0.001, 0.01, 131).astype(np.float32)[:130]
        shells = np.linspace(1.0, 5.0, 130).astype(np.float32)
        for flags in (PARENTS, DESCRIPTIONS, PARENTS | DESCRIPTIONS):
            expected = [restatement.compress(samples, RATE, flags=flags, precision=0.01, shell_distance=3.0) for samples in clips]
            check_rows(launch(ctx, handles, shapes_of(clips), flags=flags, precision=0.01, shell_distance=3.0), expected)
            expected = [restatement.compress(samples, RATE, flags=flags, default_pose=pose, parents=parents, track_precisions=precisions, track_shell_distances=shells) for samples in clips]
            check_rows(launch(ctx, handles, shapes_of(clips), flags=flags, default_pose=pose, parents=parents, track_precisions=precisions, track_shell_distances=shells), expected)
            expected = [restatement.compress(samples, RATE, flags=flags, parents=parents, shell_distance=2.0) for samples in clips]
            check_rows(launch(ctx, handles, shapes_of(clips), flags=flags, parents=parents, shell_distance=2.0), expected)
            assert all(restatement.parse(blob)["has_metadata"] for blob in expected)
        # the tables without a flag: no metadata, the blobs of the plain launch
        check_rows(launch(ctx, handles, shapes_of(clips), parents=parents, track_precisions=precisions), [restatement.compress(samples, RATE) for samples in clips])


def decode(ctx, blob, times, rounding, looping=runtime.LOOP_AS_COMPRESSED, normalization=runtime.NORMALIZE_NEVER):
    """(NORMALIZE_NEVER: the stored bits of a rotation; the decode's default normalizes what it returns, which moves the last bits)"""
    status, message = runtime.check_clip(blob, check_hash=True)
    assert status == 0, message
    clip = ctx.register_clip(blob)
    try:
        info = ctx.clip_info(clip)
        poses = ctx.decompress_tracks(np.full(len(times), clip, dtype=np.uint32), np.asarray(times, dtype=np.float32),
                                      params=runtime.default_params(rounding_policy=rounding, looping_policy=looping, normalization=normalization))
        return info, poses
    finally:
        ctx.unregister_clip(clip)


def same_key_frames(poses, samples, types):
    """animated and constant sub-tracks bit for bit in the used lanes, default ones by =="""
    for kind, lanes in enumerate(LANES):
        got, want = poses[:, :, lanes], samples[:, :, lanes]
        stored = types[kind] != restatement.DEFAULT
        assert np.array_equal(got[:, stored].view(np.uint32), want[:, stored].view(np.uint32)), kind
        assert (got[:, ~stored] == want[:, ~stored]).all(), kind


def test_the_blobs_check_register_and_decode_to_the_key_frames(sweep):
    """the lossless property: every blob passes aclhip_check_clip with the hash, registers, and decodes at every key time with
    ROUND_FLOOR to the registered key frames"""
    ctx, handles, clips = sweep
    chosen = [k for k, (num_tracks, num_samples) in enumerate(SHAPES) if (num_tracks, num_samples) in ((1, 1), (3, 2), (5, 7), (17, 65), (65, 7), (130, 3), (2, 129))]
    blobs = runtime.compress_raw_tracks(ctx, [handles[k] for k in chosen])
    for blob, k in zip(blobs, chosen):
        samples = clips[k]
        assert blob.ctypes.data % 16 == 0 and np.array_equal(blob, restatement.compress(samples, RATE))
        num_samples, num_tracks = samples.shape[0], samples.shape[1]
        info, poses = decode(ctx, blob, np.arange(num_samples) / RATE, runtime.ROUND_FLOOR)
        assert (info.num_tracks, info.num_samples) == (num_tracks, num_samples)
        same_key_frames(poses, samples, restatement.classify(samples, np.tile(IDENTITY, (num_tracks, 1)))[0])
    # with the decode's default normalization a rotation moves by the rounding of a normalize of a unit quaternion: within 4 ulp of 1.0
    _, poses = decode(ctx, blob, np.arange(num_samples) / RATE, runtime.ROUND_FLOOR, normalization=runtime.NORMALIZE_LERP_ONLY)
    assert np.abs(poses[:, :, 0:4] - samples[:, :, 0:4]).max() <= 4 * np.finfo(np.float32).eps and np.array_equal(poses[:, :, 4:7], samples[:, :, 4:7])


def test_a_wrapping_array_keeps_its_samples_and_is_marked(ctx):
    """an array registered with ACLHIP_LOOP_WRAP: S stays, the header's wrap bit is set; decoded as compressed, a time inside the wrap
    interval -- behind the last key frame -- floors to the last key frame and ceils to the first, and the floored pose is what
    aclhip_sample_raw_tracks_batch gives for the array itself"""
    import torch
    samples = restatement.clip(2, 7, 5)
    with Registered(ctx) as arrays:
        handles = [arrays.add(samples, runtime.LOOP_WRAP), arrays.add(samples, runtime.LOOP_CLAMP)]
        wrapped, clamped = restatement.compress(samples, RATE, looping_wrap=True), restatement.compress(samples, RATE)
        assert restatement.parse(wrapped)["wrap"] and restatement.parse(wrapped)["num_samples"] == 7 and not restatement.parse(clamped)["wrap"]
        check_rows(launch(ctx, handles, [(5, 7)]), [wrapped, clamped])
        check_rows(launch(ctx, handles, [(5, 7)], flags=runtime.COMPRESS_OPTIMIZE_LOOPS), [wrapped, clamped])
        blob = runtime.compress_raw_tracks(ctx, handles[0])[0]
        assert np.array_equal(blob, wrapped)
        types = restatement.classify(samples, np.tile(IDENTITY, (5, 1)))[0]
        times = np.array([6.25, 6.5, 6.875], dtype=np.float32) / np.float32(RATE)
        info, floored = decode(ctx, blob, times, runtime.ROUND_FLOOR)
        assert info.duration == np.float32(7.0 / RATE)
        same_key_frames(floored, np.repeat(samples[6:7], 3, axis=0), types)
        # ROUND_CEIL is the interpolation at alpha 1 (rtm::quat_lerp): the end key frame, negated when its dot product with the start is
        # negative -- the same rotation, the sign of the shorter arc
        _, ceiled = decode(ctx, blob, times, runtime.ROUND_CEIL)
        first, products = np.repeat(samples[0:1], 3, axis=0), (samples[6, :, 0:4] * samples[0, :, 0:4]).astype(np.float32)
        dot = (((products[:, 0] + products[:, 1]).astype(np.float32) + products[:, 2]).astype(np.float32) + products[:, 3]).astype(np.float32)
        assert (dot < 0).any() and (dot > 0).any()
        first[:, dot < 0, 0:4] = -first[:, dot < 0, 0:4]
        same_key_frames(ceiled, first, types)
        # the raw array at the same times: translations and scales bit for bit; the raw sampler normalizes its rotations for every
        # policy (include/aclhip.h), which moves a component of a rotation whose squared length is within 2e-7 of 1 by less than
        # 2e-7: 4 ulp of 1.0 (4.8e-7) bound it
        device = torch.device("cuda:0")
        d_raws = torch.full((3,), handles[0], dtype=torch.int32, device=device)
        d_times = torch.from_numpy(times).to(device)
        d_poses = torch.zeros((3, 5, 12), dtype=torch.float32, device=device)
        sample_desc = runtime.RawSampleDesc()
        sample_desc.rounding_policy = runtime.ROUND_FLOOR
        stream = torch.cuda.current_stream(device)
        ctx.sample_raw_tracks_batch(d_raws.data_ptr(), d_times.data_ptr(), 3, d_poses.data_ptr(), 5 * 48, desc=sample_desc, stream=stream.cuda_stream)
        stream.synchronize()
        sampled = d_poses.cpu().numpy()
        assert np.array_equal(sampled[:, :, 4:7].view(np.uint32), floored[:, :, 4:7].view(np.uint32)) and np.array_equal(sampled[:, :, 8:11].view(np.uint32), floored[:, :, 8:11].view(np.uint32))
        assert np.abs(sampled[:, :, 0:4] - floored[:, :, 0:4]).max() <= 4 * np.finfo(np.float32).eps


def test_parent_metadata_gives_the_clip_its_hierarchy(ctx):
    samples = restatement.clip(1, 7, 17)
    parents = restatement.chain_parents(17)
    pose = restatement.bind_pose(8, 17)
    with Registered(ctx) as arrays:
        handle = arrays.add(samples)
        for descriptions in (False, True):
            blob = runtime.compress_raw_tracks(ctx, handle, default_pose=pose, parents=parents, precision=0.01, shell_distance=3.0, include_parent_track_indices=True,
                                               include_track_descriptions=descriptions)[0]
            flags = PARENTS | (DESCRIPTIONS if descriptions else 0)
            assert np.array_equal(blob, restatement.compress(samples, RATE, default_pose=pose, parents=parents, flags=flags, precision=0.01, shell_distance=3.0))
            status, message = runtime.check_clip(blob, check_hash=True)
            assert status == 0, message
            clip = ctx.register_clip(blob)
            ctx.set_clip_hierarchy_from_metadata(clip)
            ctx.unregister_clip(clip)


def test_mixed_shapes_and_repeated_handles_in_one_launch(sweep):
    ctx, handles, clips = sweep
    order = [(7 * i + 3) % len(handles) for i in range(2 * len(handles) + 5)]
    cache = {k: restatement.compress(clips[k], RATE, flags=PARENTS) for k in set(order)}
    check_rows(launch(ctx, [handles[k] for k in order], shapes_of(clips), flags=PARENTS), [cache[k] for k in order])


def test_one_instance(ctx):
    samples = restatement.clip(0, 65, 17)
    with Registered(ctx) as arrays:
        check_rows(launch(ctx, [arrays.add(samples)], [(17, 65)]), [restatement.compress(samples, RATE)])


def test_statuses_and_refusals_leave_their_rows(ctx):
    """not finite, not normalized, both (not finite wins); an unknown handle, 0, a retired handle; more tracks than max_tracks; more
    tracks than the tables hold; a stride one byte too small (the next multiple of 16 below the size) -- each with its row untouched,
    size 0, and one count where it is a refusal; the neighbours are served"""
    small, large = restatement.clip(0, 12, 4), restatement.clip(1, 12, 9)
    with Registered(ctx) as arrays:
        h_small, h_large = arrays.add(small), arrays.add(large)
        blob_small, blob_large = restatement.compress(small, RATE), restatement.compress(large, RATE)
        refused, not_finite, not_normalized = runtime.COMPRESS_REFUSED, runtime.COMPRESS_NOT_FINITE, runtime.COMPRESS_NOT_NORMALIZED

        bad = []
        for lane, value in ((0, np.nan), (3, np.inf), (4, -np.inf), (6, np.nan), (8, np.inf), (10, np.nan)):
            samples = large.copy()
            samples[11 if lane % 2 else 0, 8 if lane % 3 else 0, lane] = value
            bad.append((arrays.add(samples), not_finite))
        for scale in (1.0 + 2.0e-5, 1.0 - 2.0e-5, 0.0, 2.0):
            samples = large.copy()
            samples[5, 7, 0:4] *= np.float32(scale)
            assert not restatement.rotations_normalized(samples[5, 7, 0:4])
            bad.append((arrays.add(samples), not_normalized))
        samples = large.copy()
        samples[3, 2, 0:4] *= np.float32(1.5)
        samples[9, 6, 9] = np.inf
        bad.append((arrays.add(samples), not_finite))                 # both: not finite wins
        samples = large.copy()
        samples[3, 2, 0:4] *= np.float32(1.0 + 3.0e-6)                # inside the threshold: kept as it is
        assert restatement.rotations_normalized(samples[3, 2, 0:4])
        h_inside, blob_inside = arrays.add(samples), restatement.compress(samples, RATE)
        handles = [h_small] + [handle for handle, _ in bad] + [h_inside, h_large]
        check_rows(launch(ctx, handles, [(9, 12)]), [blob_small] + [status for _, status in bad] + [blob_inside, blob_large])
        with pytest.raises(RuntimeError, match="Some samples are not finite"):
            runtime.compress_raw_tracks(ctx, [h_small, bad[0][0]])
        with pytest.raises(ValueError, match="ACLHIP_COMPRESS_NOT_NORMALIZED"):
            runtime.compress_raw_tracks(ctx, [h_small, bad[6][0]])

        retired = ctx.register_raw_tracks(small, RATE)         # (behind every other registration: its slot is not handed out again here)
        ctx.unregister_raw_tracks(retired)
        handles = [h_small, 0, 4000, retired, 0xFFFFFFFF, h_large, h_small]
        check_rows(launch(ctx, handles, [(9, 12)]), [blob_small, refused, refused, refused, refused, blob_large, blob_small])
        # max_tracks 4: the array of 9 tracks is refused
        check_rows(launch(ctx, handles, [(9, 12)], max_tracks=4), [blob_small, refused, refused, refused, refused, refused, blob_small])
        # tables of 4 entries, each kind alone
        short = {"default_pose": np.tile(IDENTITY, (4, 1)), "parents": np.full(4, restatement.NO_PARENT, dtype=np.uint32),
                 "track_precisions": np.full(4, 0.01, dtype=np.float32), "track_shell_distances": np.ones(4, dtype=np.float32)}
        for name, table in short.items():
            check_rows(launch(ctx, handles, [(9, 12)], **{name: table}), [blob_small, refused, refused, refused, refused, refused, blob_small])
        # a stride that holds the small blob and not the large one; and the largest stride that does not hold the small one
        assert blob_small.size < blob_large.size
        stride = (blob_small.size + 15) & ~15
        assert stride < blob_large.size
        check_rows(launch(ctx, handles, [(9, 12)], stride=stride), [blob_small, refused, refused, refused, refused, refused, blob_small])
        assert blob_small.size % 16 != 0
        check_rows(launch(ctx, [h_small, h_large], [(9, 12)], stride=blob_small.size & ~15), [refused, refused])
        # with metadata: the stride that just holds the blob, and 16 bytes less
        with_parents = restatement.compress(small, RATE, flags=PARENTS | DESCRIPTIONS)
        stride = (with_parents.size + 15) & ~15
        check_rows(launch(ctx, [h_small, h_small], [(4, 12)], flags=PARENTS | DESCRIPTIONS, stride=stride), [with_parents, with_parents])
        check_rows(launch(ctx, [h_small, h_small], [(4, 12)], flags=PARENTS | DESCRIPTIONS, stride=stride - 16), [refused, refused])


def test_a_captured_launch_replays_to_the_same_bytes(sweep):
    ctx, handles, clips = sweep
    expected = [restatement.compress(samples, RATE, flags=DESCRIPTIONS) for samples in clips]
    plain, replayed = (launch(ctx, handles, shapes_of(clips), flags=DESCRIPTIONS, graph=graph) for graph in (False, True))
    check_rows(replayed, expected)
    assert same(plain, replayed)


def test_two_runs_give_the_same_bytes(sweep):
    ctx, handles, clips = sweep
    runs = [launch(ctx, handles + [0], shapes_of(clips)) for _ in range(2)]
    assert np.array_equal(runs[0].flat, runs[1].flat) and np.array_equal(runs[0].results, runs[1].results)
