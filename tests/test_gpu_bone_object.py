"""Single bone requests in object space (aclhip_decompress_track_object_batch, aclhip_decompress_bone_object_batch_mapped) through the C
ABI. Every comparison is bit for bit, against two yardsticks: (a) the oracle -- the decoded local pose taken to object space by
oracle_local_to_object_space, record picked with numpy (skeleton space: the expected-pose construction of test_gpu_skeleton_poses.py) --
and (b) the corresponding record of the existing whole-pose GPU launch on the same inputs, one row per request. Every launch writes into
a pattern filled buffer with guard records in front and behind. Needs a GPU."""
import itertools

import numpy as np
import pytest

from acl_amd import runtime, synth
from oracle import bindings as ob
import helpers

pytestmark = pytest.mark.gpu

DROPPED = runtime.TRACK_DROPPED
NO_PARENT = runtime.NO_PARENT
SENTINEL = np.float32(-7777.25)
GUARD = 5                       # records in front of and behind the transforms
POLICIES = list(itertools.product((0, 1, 2, 3), (0, 1, 2)))     # rounding none / floor / ceil / nearest x clamp / wrap / as compressed


def up(array, dtype):
    import torch
    array = np.ascontiguousarray(array, dtype=dtype)
    return torch.from_numpy(array.view(np.int32) if dtype == np.uint32 else array).cuda()


def request_params(rounding=0, looping=2, instance_rounding=None, instance_looping=None, keep=None, **overrides):
    params = runtime.default_params(rounding_policy=rounding, looping_policy=looping, **overrides)
    if instance_rounding is not None:
        keep.append(up(instance_rounding, np.uint8))
        params.instance_rounding_policies = keep[-1].data_ptr()
    if instance_looping is not None:
        keep.append(up(instance_looping, np.uint8))
        params.instance_looping_policies = keep[-1].data_ptr()
    return params


def launch_requests(ctx, handles, times, bones, params=None, mapping=None):
    """the launch under test: returns (transforms [n, 12], guards untouched?)"""
    import torch
    n = len(handles)
    buffer = torch.full((n + 2 * GUARD, 12), float(SENTINEL), dtype=torch.float32, device="cuda")
    d_handles, d_times, d_bones = up(handles, np.uint32), up(times, np.float32), up(bones, np.uint32)
    stream = torch.cuda.current_stream().cuda_stream
    if mapping is None:
        ctx.decompress_track_object_batch(d_handles.data_ptr(), d_times.data_ptr(), d_bones.data_ptr(), n, buffer[GUARD].data_ptr(), params=params, stream=stream)
    else:
        ctx.decompress_bone_object_batch_mapped(d_handles.data_ptr(), d_times.data_ptr(), d_bones.data_ptr(), n, buffer[GUARD].data_ptr(), mapping, params=params, stream=stream)
    torch.cuda.synchronize()
    out = buffer.cpu().numpy()
    guards = np.concatenate([out[:GUARD], out[GUARD + n:]])
    assert np.array_equal(guards.view(np.uint32), np.full_like(guards, SENTINEL).view(np.uint32)), "a request wrote outside the transforms"
    return out[GUARD:GUARD + n]


def whole_pose_rows(ctx, handles, times, num_records, params=None, mapping=None):
    """yardstick (b): the existing object space launch, one row per request; refused rows keep the pattern"""
    import torch
    n = len(handles)
    rows = torch.full((n, num_records, 12), float(SENTINEL), dtype=torch.float32, device="cuda")
    d_handles, d_times = up(handles, np.uint32), up(times, np.float32)
    consumers = runtime.PoseConsumers()
    consumers.object_space = 1
    stream = torch.cuda.current_stream().cuda_stream
    if mapping is None:
        ctx.decompress_poses_batch(d_handles.data_ptr(), d_times.data_ptr(), n, rows.data_ptr(), num_records * 48, consumers, params=params, stream=stream)
    else:
        ctx.decompress_poses_batch_mapped(d_handles.data_ptr(), d_times.data_ptr(), n, rows.data_ptr(), num_records * 48, consumers, mapping, params=params, stream=stream)
    torch.cuda.synchronize()
    return rows.cpu().numpy()


def pick(rows, bones):
    return rows[np.arange(len(bones)), np.asarray(bones, dtype=np.int64)]


class OraclePoses:
    """yardstick (a): object space poses of (clip, time, rounding, looping, normalization), computed once each"""

    def __init__(self):
        self.cache = {}

    def pose(self, blob, parents, time, rounding=0, looping=2, normalization=None):
        key = (blob.ctypes.data, parents.ctypes.data, float(time), rounding, looping, normalization)
        if key not in self.cache:
            options = ob.default_options(looping_policy=looping) if normalization is None else ob.default_options(looping_policy=looping, normalization=normalization)
            self.cache[key] = ob.oracle_local_to_object_space(parents, ob.oracle_decompress_tracks(blob, float(time), rounding, options))
        return self.cache[key]


def random_hierarchy(rng, num_tracks, parent_span, extra_roots=0):
    parents = np.zeros(num_tracks, dtype=np.uint32)
    parents[0] = NO_PARENT
    for i in range(1, num_tracks):
        parents[i] = rng.integers(max(0, i - parent_span), i)
    if extra_roots and num_tracks > 1:
        parents[rng.choice(np.arange(1, num_tracks), size=min(extra_roots, num_tracks - 1), replace=False)] = NO_PARENT
    return parents


def key_and_between_times(clip, num_samples, rng, count):
    """sample times at key frames (the first, the last and some in the middle), between them, and a little outside the clip"""
    rate = (num_samples - 1) / clip.duration
    at_keys = np.array([0, 1, num_samples // 2, num_samples - 2, num_samples - 1], dtype=np.float32) / np.float32(rate)
    between = rng.uniform(-0.02, clip.duration + 0.02, size=count).astype(np.float32)
    return np.concatenate([at_keys.astype(np.float32), between])


def check_every_bone(ctx, oracle, clip_blob, handle, parents, times, rounding=0, looping=2, params=None, normalization=None):
    num_tracks = parents.size
    bones = np.tile(np.arange(num_tracks, dtype=np.uint32), times.size)
    request_times = np.repeat(times, num_tracks).astype(np.float32)
    handles = np.full(bones.size, handle, dtype=np.uint32)
    got = launch_requests(ctx, handles, request_times, bones, params=params)
    expected = np.stack([oracle.pose(clip_blob, parents, t, rounding, looping, normalization)[b] for t, b in zip(request_times, bones)])
    assert helpers.exact(got, expected), ("oracle", rounding, looping)
    reference = whole_pose_rows(ctx, handles, request_times, num_tracks, params=params)
    assert helpers.exact(got, pick(reference, bones)), ("whole-pose launch", rounding, looping)


def test_humanoid_every_bone_every_policy():
    """the 100-bone synthetic humanoid: every bone at and between key frames under every rounding and looping policy, then with per
    request policy arrays (700 and 1100 requests: not multiples of 64)"""
    rng = np.random.default_rng(5)
    clip = synth.build_clip(seed=7, num_tracks=100, num_samples=61)
    parents = np.array(synth.humanoid_hierarchy(100), dtype=np.uint32)
    oracle = OraclePoses()
    with runtime.Context(0) as ctx:
        handle = ctx.register_clip(clip.blob)
        ctx.set_clip_hierarchy(handle, parents)
        times = key_and_between_times(clip, 61, rng, 2)
        for rounding, looping in POLICIES:
            check_every_bone(ctx, oracle, clip.blob, handle, parents, times, rounding, looping, params=runtime.default_params(rounding_policy=rounding, looping_policy=looping))
        # per request arrays
        times = key_and_between_times(clip, 61, rng, 6)
        bones = np.tile(np.arange(100, dtype=np.uint32), times.size)
        request_times = np.repeat(times, 100).astype(np.float32)
        roundings = rng.integers(0, 4, size=bones.size).astype(np.uint8)
        loopings = rng.integers(0, 3, size=bones.size).astype(np.uint8)
        handles = np.full(bones.size, handle, dtype=np.uint32)
        keep = []
        params = request_params(rounding=1, looping=0, instance_rounding=roundings, instance_looping=loopings, keep=keep)
        got = launch_requests(ctx, handles, request_times, bones, params=params)
        expected = np.stack([oracle.pose(clip.blob, parents, t, int(r), int(l))[b] for t, b, r, l in zip(request_times, bones, roundings, loopings)])
        assert helpers.exact(got, expected)
        assert helpers.exact(got, pick(whole_pose_rows(ctx, handles, request_times, 100, params=params), bones))
        assert ctx.rejected_instance_count() == 0


@pytest.mark.parametrize("name", ["multi_window_300_several_roots", "chain_of_depth_120", "single_bone", "scaled_37_two_roots"])
def test_shapes(name):
    rng = np.random.default_rng(len(name))
    if name == "multi_window_300_several_roots":
        spec, parents = dict(seed=31, num_tracks=300, num_samples=40, has_scale=1, scale_default=0.4), random_hierarchy(rng, 300, 12, extra_roots=4)
    elif name == "chain_of_depth_120":
        spec, parents = dict(seed=32, num_tracks=121, num_samples=25), np.arange(-1, 120, dtype=np.int64).astype(np.uint32)
    elif name == "single_bone":
        spec, parents = dict(seed=33, num_tracks=1, num_samples=12), np.array([NO_PARENT], dtype=np.uint32)
    else:
        spec, parents = dict(seed=34, num_tracks=37, num_samples=33, has_scale=1, scale_default=0.3), random_hierarchy(rng, 37, 4, extra_roots=1)
    clip = synth.build_clip(**spec)
    oracle = OraclePoses()
    with runtime.Context(0) as ctx:
        handle = ctx.register_clip(clip.blob)
        ctx.set_clip_hierarchy(handle, parents)
        if name == "chain_of_depth_120":
            assert runtime.plan_bone_chain(parents, 120, query_length_only=True) == 121
        times = key_and_between_times(clip, spec["num_samples"], rng, 3)
        check_every_bone(ctx, oracle, clip.blob, handle, parents, times)
        check_every_bone(ctx, oracle, clip.blob, handle, parents, times[-2:], rounding=3, looping=1, params=runtime.default_params(rounding_policy=3, looping_policy=1))
        assert ctx.rejected_instance_count() == 0


def test_mirrored_rig_takes_the_matrix_route():
    """a clip whose own scales are negative: the whole-pose launch counts matrix products (so the route is really exercised), the
    requests give its bits and add nothing to that counter; a plain clip in the same waves"""
    rng = np.random.default_rng(92)
    mirrored = synth.build_clip(seed=92, num_tracks=100, num_samples=45, has_scale=1, scale_default=0.3, scale_constant=0.3, mirrored_scale_fraction=0.3)
    plain = synth.build_clip(seed=93, num_tracks=100, num_samples=45, has_scale=1)
    parents = np.array(synth.humanoid_hierarchy(100), dtype=np.uint32)
    oracle = OraclePoses()
    with runtime.Context(0) as ctx:
        clips = [mirrored, plain]
        handles = np.array([ctx.register_clip(c.blob) for c in clips], dtype=np.uint32)
        for handle in handles:
            ctx.set_clip_hierarchy(int(handle), parents)
        n = 1000
        which = rng.integers(0, 2, size=n)
        which[:200] = 0
        bones = rng.integers(0, 100, size=n).astype(np.uint32)
        times = np.array([rng.uniform(0.0, clips[c].duration) for c in which], dtype=np.float32)
        before = ctx.negative_scale_count()
        reference = whole_pose_rows(ctx, handles[which], times, 100)
        counted = ctx.negative_scale_count()
        assert counted > before
        got = launch_requests(ctx, handles[which], times, bones)
        assert ctx.negative_scale_count() == counted
        assert helpers.exact(got, pick(reference, bones))
        expected = np.stack([oracle.pose(clips[c].blob, parents, t)[b] for c, t, b in zip(which, times, bones)])
        assert (expected[:, 8:11] < 0.0).any()
        assert helpers.exact(got, expected)
        assert ctx.rejected_instance_count() == 0


def _clip_that_fails_the_short_exact_proof():
    """tests/test_gpu_exact_math.py's clip: an animated rotation of exactly x = 1 next to y = 1e-20"""
    clip = synth.build_clip(seed=77, num_tracks=12, num_samples=20, rotation_default=0.0, rotation_constant=0.0, raw_fraction=0.0, width0_fraction=0.0)
    blob = clip.blob.copy()
    header = np.frombuffer(blob[32:32 + 52].tobytes(), dtype=np.uint32)
    num_animated_rotations, clip_range_offset = int(header[2]), int(header[12])
    group = min(4, num_animated_rotations)
    base = 32 + clip_range_offset
    values = blob[base: base + 6 * group * 4].view(np.float32)
    values[0 * group], values[1 * group], values[2 * group] = 1.0, 1.0e-20, 0.0
    values[3 * group], values[4 * group], values[5 * group] = 0.0, 0.0, 0.0
    aligned = synth.aligned_bytes(blob.size)
    aligned[:] = blob
    return aligned, clip.duration


@pytest.mark.parametrize("normalization", [ob.NORMALIZE_NEVER, ob.NORMALIZE_LERP_ONLY])
def test_mixed_clips_with_different_hierarchies_and_without_the_short_exact_proof(normalization):
    """waves of mixed clips: different sizes, different hierarchies (two clips share one), a clip registration refuses the short exact
    forms for, clips with raw rotations (whose walk keeps the compiler's normalize when the decode does not normalize)"""
    rng = np.random.default_rng(61 + normalization)
    unproven, unproven_duration = _clip_that_fails_the_short_exact_proof()
    assert runtime.analyze_clip(unproven, check_hash=False) & runtime.CLIP_FACT_SHORT_EXACT_MATH == 0
    built = [synth.build_clip(seed=610, num_tracks=140, num_samples=30, raw_fraction=0.5, has_scale=1, scale_default=0.6),
             synth.build_clip(seed=601, num_tracks=50, num_samples=30), synth.build_clip(seed=604, num_tracks=50, num_samples=20),
             synth.build_clip(seed=603, num_tracks=23, num_samples=30, has_scale=1)]
    blobs = [unproven] + [c.blob for c in built]
    durations = [unproven_duration] + [c.duration for c in built]
    shared = random_hierarchy(rng, 50, 5)
    parents = [random_hierarchy(rng, 12, 3), random_hierarchy(rng, 140, 6), shared, shared.copy(), random_hierarchy(rng, 23, 20, extra_roots=2)]
    oracle = OraclePoses()
    with runtime.Context(0) as ctx:
        handles = np.array([ctx.register_clip(blobs[0], check_hash=False)] + [ctx.register_clip(b) for b in blobs[1:]], dtype=np.uint32)
        for handle, clip_parents in zip(handles, parents):
            ctx.set_clip_hierarchy(int(handle), clip_parents)
        n = 1531
        which = rng.integers(0, len(blobs), size=n)
        which[64:128] = 0                   # a whole wave of the unproven clip, and waves that mix it with the others
        bones = np.array([rng.integers(0, parents[c].size) for c in which], dtype=np.uint32)
        times = np.array([rng.uniform(0.0, durations[c]) for c in which], dtype=np.float32)
        params = runtime.default_params(normalization=normalization)
        got = launch_requests(ctx, handles[which], times, bones, params=params)
        expected = np.stack([oracle.pose(blobs[c], parents[c], t, normalization=normalization)[b] for c, t, b in zip(which, times, bones)])
        assert helpers.exact(got, expected)
        assert helpers.exact(got, pick(whole_pose_rows(ctx, handles[which], times, 140, params=params), bones))
        assert ctx.rejected_instance_count() == 0


def test_database_bound_clips_before_and_after_stream_in():
    case = helpers.load_database_golden("three_clips_4k_chunks")
    rng = np.random.default_rng(17)
    with runtime.Context(0) as ctx:
        database = ctx.register_database(case["database"], case["bulk_medium"], case["bulk_low"])
        clips = [ctx.register_clip_with_database(clip, database) for clip in case["clips"]]
        num_tracks = [ob.oracle().aclo_num_tracks(clip.ctypes.data) for clip in case["clips"]]
        parents = [random_hierarchy(rng, n, parent_span=6, extra_roots=1) for n in num_tracks]
        for clip, clip_parents in zip(clips, parents):
            ctx.set_clip_hierarchy(clip, clip_parents)
        num_times = case["times"].shape[1]
        which = np.repeat(np.arange(len(clips)), num_times)
        times = case["times"].reshape(-1).astype(np.float32)
        # every (clip, time) three times over, each with a bone of its own
        which, times, time_index = np.tile(which, 3), np.tile(times, 3), np.tile(np.tile(np.arange(num_times), len(clips)), 3)
        bones = np.array([rng.integers(0, num_tracks[c]) for c in which], dtype=np.uint32)
        handles = np.array(clips, dtype=np.uint32)[which]

        def check(state):
            got = launch_requests(ctx, handles, times, bones)
            assert helpers.exact(got, pick(whole_pose_rows(ctx, handles, times, max(num_tracks)), bones)), state
            for k in range(which.size):
                local = case["poses"][state, which[k], 0, time_index[k], :num_tracks[which[k]]].copy()      # policy 0 = none
                local[:, 7] = 0.0
                local[:, 11] = 0.0
                assert helpers.exact(got[k], ob.oracle_local_to_object_space(parents[which[k]], local)[bones[k]]), (state, k)

        assert int(case["policies"][0]) == 0
        check(0)
        streamed_in = 0
        for state, (tier, num_chunks, stream_in) in enumerate(case["ops"]):
            (ctx.database_stream_in if stream_in else ctx.database_stream_out)(database, int(tier), int(num_chunks))
            streamed_in += int(stream_in)
            check(state + 1)
        assert streamed_in > 0
        assert ctx.rejected_instance_count() == 0


def test_corpus_blobs_with_parent_metadata():
    """clips the reference's compressor wrote with their parent indices: the hierarchy comes from aclhip_set_clip_hierarchy_from_metadata"""
    corpus = helpers.load_corpus()
    carried = [clip for clip in corpus if clip["spec"].get("include_parent_track_indices") or clip["spec"].get("include_track_descriptions")]
    assert len(carried) >= 3
    oracle = OraclePoses()
    with runtime.Context(0) as ctx:
        for clip in carried:
            handle = ctx.register_clip(clip["blob"])
            ctx.set_clip_hierarchy_from_metadata(handle)
            parents = clip["parents"].astype(np.uint32)
            all_times, _ = helpers.corpus_sample_times(clip["blob"])
            if parents.size == 0 or all_times.size == 0:
                continue
            times = all_times[:: max(1, all_times.size // 6)]
            check_every_bone(ctx, oracle, clip["blob"], handle, parents, times)
        assert ctx.rejected_instance_count() == 0


# ---- skeleton space --------------------------------------------------------------------------------------------------------------------

def reference_pose(rng, num_bones, mirrored=False):
    pose = np.zeros((num_bones, 12), dtype=np.float32)
    rotations = rng.normal(size=(num_bones, 4))
    pose[:, 0:4] = (rotations / np.linalg.norm(rotations, axis=1, keepdims=True)).astype(np.float32)
    pose[:, 4:7] = rng.uniform(-1.0, 1.0, size=(num_bones, 3))
    pose[:, 8:11] = rng.uniform(0.5, 1.5, size=(num_bones, 3))
    if mirrored:
        pose[rng.choice(num_bones, size=num_bones // 5, replace=False), 8] *= -1.0
    return pose


def make_map(rng, num_tracks, num_bones, kind):
    """identity | permutation (into more slots than tracks: filled slots in the middle of chains) | dropped (a third of the tracks)"""
    if kind == "identity":
        assert num_tracks == num_bones
        return np.arange(num_tracks, dtype=np.uint32)
    table = np.full(num_tracks, DROPPED, dtype=np.uint32)
    keep = min(num_tracks, num_bones) if kind != "dropped" else min(num_tracks - num_tracks // 3, num_bones)
    tracks = np.sort(rng.choice(num_tracks, size=keep, replace=False))
    table[tracks] = rng.choice(num_bones, size=keep, replace=False)
    return table


def skeleton_object_pose(blob, time, table, reference, parents, rounding, looping):
    decoded = ob.oracle_decompress_tracks(blob, float(time), rounding, ob.default_options(looping_policy=looping))
    pose = reference.copy()
    mapped = table != DROPPED
    pose[table[mapped]] = decoded[mapped]
    return ob.oracle_local_to_object_space(parents, pose)


@pytest.mark.parametrize("num_bones,kind,mirrored", [(100, "identity", False), (128, "permutation", False), (110, "dropped", False), (128, "permutation", True)])
def test_mapped_requests(num_bones, kind, mirrored):
    rng = np.random.default_rng(num_bones + len(kind) + int(mirrored))
    clips = [synth.build_clip(seed=900 + k, num_tracks=100, num_samples=61 + 3 * k) for k in range(3)]
    reference, parents = reference_pose(rng, num_bones, mirrored), np.array(synth.humanoid_hierarchy(num_bones), dtype=np.uint32)
    tables = [make_map(rng, 100, num_bones, kind) for _ in clips]
    if kind == "permutation":
        # a slot no track maps to in the MIDDLE of a chain: some filled slot has a child
        filled = np.setdiff1d(np.arange(num_bones), np.concatenate([t[t != DROPPED] for t in tables[:1]]))
        assert np.isin(parents[1:], filled).any()
    with runtime.Context(0) as ctx:
        handles = np.array([ctx.register_clip(c.blob) for c in clips], dtype=np.uint32)
        maps = np.array([ctx.register_track_map(t, num_bones) for t in tables], dtype=np.uint32)
        skeleton = ctx.register_skeleton(parents, reference)
        n = 2 * num_bones * 3 + 7
        which = rng.integers(0, 3, size=n)
        slots = (np.arange(n) % num_bones).astype(np.uint32)            # every slot, several times
        times = np.array([rng.uniform(-0.05, clips[c].duration + 0.05) for c in which], dtype=np.float32)
        for rounding, looping in ((0, 2), (1, 0), (2, 1), (3, 2)):
            keep = [up(maps[which], np.uint32)]
            mapping = runtime.PoseMapping()
            mapping.skeleton, mapping.instance_maps = skeleton, keep[0].data_ptr()
            params = runtime.default_params(rounding_policy=rounding, looping_policy=looping)
            before = ctx.negative_scale_count()
            reference_rows = whole_pose_rows(ctx, handles[which], times, num_bones, params=params, mapping=mapping)
            if mirrored:
                assert ctx.negative_scale_count() > before
            got = launch_requests(ctx, handles[which], times, slots, params=params, mapping=mapping)
            assert helpers.exact(got, pick(reference_rows, slots)), (rounding, looping)
            expected = np.stack([skeleton_object_pose(clips[c].blob, t, tables[c], reference, parents, rounding, looping)[s] for c, t, s in zip(which, times, slots)])
            assert helpers.exact(got, expected), (rounding, looping)
        assert ctx.rejected_instance_count() == 0


def test_mapped_requests_with_per_request_skeletons_and_maps():
    rng = np.random.default_rng(77)
    clips = [synth.build_clip(seed=950, num_tracks=100, num_samples=61), synth.build_clip(seed=951, num_tracks=37, num_samples=33, has_scale=1, scale_default=0.3)]
    bones_of = [128, 64]
    references = [reference_pose(rng, b) for b in bones_of]
    parents = [np.array(synth.humanoid_hierarchy(128), dtype=np.uint32), random_hierarchy(rng, 64, 5, extra_roots=2)]
    # clip c has a map into each skeleton
    tables = [[make_map(rng, clips[c].num_tracks, bones_of[s], "dropped" if (c + s) % 2 else "permutation") for s in range(2)] for c in range(2)]
    with runtime.Context(0) as ctx:
        handles = np.array([ctx.register_clip(c.blob) for c in clips], dtype=np.uint32)
        skeletons = np.array([ctx.register_skeleton(parents[s], references[s]) for s in range(2)], dtype=np.uint32)
        maps = np.array([[ctx.register_track_map(tables[c][s], bones_of[s]) for s in range(2)] for c in range(2)], dtype=np.uint32)
        n = 777
        which_clip, which_skeleton = rng.integers(0, 2, size=n), rng.integers(0, 2, size=n)
        slots = np.array([rng.integers(0, bones_of[s]) for s in which_skeleton], dtype=np.uint32)
        times = np.array([rng.uniform(0.0, clips[c].duration) for c in which_clip], dtype=np.float32)
        keep = [up(skeletons[which_skeleton], np.uint32), up(maps[which_clip, which_skeleton], np.uint32)]
        mapping = runtime.PoseMapping()
        mapping.instance_skeletons, mapping.instance_maps = keep[0].data_ptr(), keep[1].data_ptr()
        got = launch_requests(ctx, handles[which_clip], times, slots, mapping=mapping)
        assert helpers.exact(got, pick(whole_pose_rows(ctx, handles[which_clip], times, 128, mapping=mapping), slots))
        expected = np.stack([skeleton_object_pose(clips[c].blob, t, tables[c][s], references[s], parents[s], 0, 2)[b] for c, s, t, b in zip(which_clip, which_skeleton, times, slots)])
        assert helpers.exact(got, expected)
        assert ctx.rejected_instance_count() == 0


# ---- refusals ----------------------------------------------------------------------------------------------------------------------------

def assert_refusals(got, expected, refused):
    pattern = np.full(12, SENTINEL, dtype=np.float32).view(np.uint32)
    for k in range(got.shape[0]):
        if refused[k]:
            assert np.array_equal(got[k].view(np.uint32), pattern), ("a refused request was written", k)
        else:
            assert helpers.exact(got[k], expected[k]), ("the neighbour of a refused request", k)


def test_refused_requests_unmapped():
    rng = np.random.default_rng(3)
    clip = synth.build_clip(seed=7, num_tracks=100, num_samples=61)
    bare = synth.build_clip(seed=8, num_tracks=100, num_samples=30)
    scalar = synth.build_scalar_clip(**helpers.SCALAR_CLIP_SPECS["float1f_all_rates"])
    parents = np.array(synth.humanoid_hierarchy(100), dtype=np.uint32)
    oracle = OraclePoses()
    with runtime.Context(0) as ctx:
        handle, bare_handle, scalar_handle = ctx.register_clip(clip.blob), ctx.register_clip(bare.blob), ctx.register_clip(scalar.blob)
        gone = ctx.register_clip(bare.blob)
        ctx.set_clip_hierarchy(gone, parents)
        ctx.unregister_clip(gone)
        ctx.set_clip_hierarchy(handle, parents)
        for n in (200, 64, 3):
            handles = np.full(n, handle, dtype=np.uint32)
            bones = rng.integers(0, 100, size=n).astype(np.uint32)
            times = rng.uniform(0.0, clip.duration, size=n).astype(np.float32)
            refused = np.zeros(n, dtype=bool)
            bad = [(0, "bare"), (1, "scalar"), (2, "unknown")] if n == 3 else [(1, "bare"), (5, "scalar"), (6, "unknown"), (7, "huge"), (63, "bone"), (n - 1, "bone_huge"), (40, "retired")]
            for k, kind in bad:
                refused[k] = True
                if kind == "bare":
                    handles[k] = bare_handle                # no hierarchy
                elif kind == "scalar":
                    handles[k], bones[k] = scalar_handle, 0
                elif kind == "unknown":
                    handles[k] = 4000
                elif kind == "huge":
                    handles[k] = 0xFFFFFFFF
                elif kind == "bone":
                    bones[k] = 100                          # track_index == num_tracks
                elif kind == "bone_huge":
                    bones[k] = 0xFFFFFFFF
                else:
                    handles[k] = gone
            before = ctx.rejected_instance_count()
            got = launch_requests(ctx, handles, times, bones)
            assert ctx.rejected_instance_count() == before + int(refused.sum())
            expected = np.stack([oracle.pose(clip.blob, parents, t)[min(int(b), 99)] for t, b in zip(times, bones)])
            assert_refusals(got, expected, refused)

        # arguments
        import torch
        d = torch.zeros(64, dtype=torch.int32, device="cuda")
        out = torch.zeros((8, 12), dtype=torch.float32, device="cuda")
        for params in (runtime.default_params(per_track_rounding=1), runtime.default_params(normalization=ob.NORMALIZE_ALWAYS), runtime.default_params(default_scale_mode=ob.DEFAULT_SKIPPED)):
            with pytest.raises(runtime.AclHipError) as error:
                ctx.decompress_track_object_batch(d.data_ptr(), d.data_ptr(), d.data_ptr(), 4, out.data_ptr(), params=params)
            assert error.value.status == runtime.ERROR_INVALID_ARGUMENT
        for arguments in ((None, d.data_ptr(), d.data_ptr(), 4, out.data_ptr()), (d.data_ptr(), d.data_ptr(), None, 4, out.data_ptr()), (d.data_ptr(), d.data_ptr(), d.data_ptr(), 4, None),
                          (d.data_ptr(), d.data_ptr(), d.data_ptr(), 4, out.data_ptr() + 4)):
            with pytest.raises(runtime.AclHipError) as error:
                ctx.decompress_track_object_batch(*arguments)
            assert error.value.status == runtime.ERROR_INVALID_ARGUMENT
        ctx.decompress_track_object_batch(None, None, None, 0, None)       # nothing to do


def test_refused_requests_mapped():
    rng = np.random.default_rng(4)
    clip = synth.build_clip(seed=7, num_tracks=100, num_samples=61)
    other = synth.build_clip(seed=9, num_tracks=37, num_samples=20)
    num_bones = 128
    reference, parents = reference_pose(rng, num_bones), np.array(synth.humanoid_hierarchy(num_bones), dtype=np.uint32)
    table = make_map(rng, 100, num_bones, "permutation")
    with runtime.Context(0) as ctx:
        handle, other_handle = ctx.register_clip(clip.blob), ctx.register_clip(other.blob)
        skeleton = ctx.register_skeleton(parents, reference)
        flat = ctx.register_skeleton(None, reference)                            # registered without a hierarchy
        small = ctx.register_skeleton(parents[:64], reference[:64])
        retired_skeleton = ctx.register_skeleton(parents, reference)
        ctx.unregister_skeleton(retired_skeleton)
        good_map = ctx.register_track_map(table, num_bones)
        retired_map = ctx.register_track_map(table, num_bones)
        ctx.unregister_track_map(retired_map)
        n = 300
        handles = np.full(n, handle, dtype=np.uint32)
        skeletons = np.full(n, skeleton, dtype=np.uint32)
        maps = np.full(n, good_map, dtype=np.uint32)
        slots = rng.integers(0, num_bones, size=n).astype(np.uint32)
        times = rng.uniform(0.0, clip.duration, size=n).astype(np.float32)
        refused = np.zeros(n, dtype=bool)
        cases = {0: ("skeleton", flat), 3: ("skeleton", retired_skeleton), 64: ("skeleton", 0), 65: ("skeleton", runtime.MAX_SKELETONS + 5), 66: ("skeleton", small),      # map.num_slots != num_bones
                 100: ("map", retired_map), 101: ("map", 0), 102: ("map", 0x7FFFFFFF), 127: ("clip", other_handle),                                              # map.num_tracks != clip.num_tracks
                 128: ("clip", 5000), 200: ("slot", num_bones), 299: ("slot", 0xFFFFFFFF)}
        for k, (what, value) in cases.items():
            refused[k] = True
            {"skeleton": skeletons, "map": maps, "clip": handles, "slot": slots}[what][k] = value
        keep = [up(skeletons, np.uint32), up(maps, np.uint32)]
        mapping = runtime.PoseMapping()
        mapping.instance_skeletons, mapping.instance_maps = keep[0].data_ptr(), keep[1].data_ptr()
        before = ctx.rejected_instance_count()
        got = launch_requests(ctx, handles, times, slots, mapping=mapping)
        assert ctx.rejected_instance_count() == before + len(cases)
        expected = np.stack([skeleton_object_pose(clip.blob, t, table, reference, parents, 0, 2)[min(int(s), num_bones - 1)] for t, s in zip(times, slots)])
        assert_refusals(got, expected, refused)

        # arguments: no mapping, no skeleton, no map, blend_maps / base_maps set
        import torch
        d = torch.zeros(64, dtype=torch.int32, device="cuda")
        out = torch.zeros((8, 12), dtype=torch.float32, device="cuda")
        wrong = []
        for field, value in (("skeleton", 0), ("map", 0), ("blend_maps", d.data_ptr()), ("base_maps", d.data_ptr())):
            mapping = runtime.PoseMapping()
            mapping.skeleton, mapping.map = skeleton, good_map
            setattr(mapping, field, value)
            wrong.append(mapping)
        for mapping in wrong:
            with pytest.raises(runtime.AclHipError) as error:
                ctx.decompress_bone_object_batch_mapped(d.data_ptr(), d.data_ptr(), d.data_ptr(), 4, out.data_ptr(), mapping)
            assert error.value.status == runtime.ERROR_INVALID_ARGUMENT
        assert ctx._lib.aclhip_decompress_bone_object_batch_mapped(ctx._handle, d.data_ptr(), d.data_ptr(), d.data_ptr(), 4, None, None, out.data_ptr(), None) == runtime.ERROR_INVALID_ARGUMENT


# ---- captured graphs, full size ----------------------------------------------------------------------------------------------------------

def test_captured_launch_replays_after_the_registry_grew():
    import torch
    rng = np.random.default_rng(12)
    clip = synth.build_clip(seed=7, num_tracks=100, num_samples=61)
    parents = np.array(synth.humanoid_hierarchy(100), dtype=np.uint32)
    oracle = OraclePoses()
    with runtime.Context(0) as ctx:
        handle = ctx.register_clip(clip.blob)
        ctx.set_clip_hierarchy(handle, parents)
        n = 333
        bones = rng.integers(0, 100, size=n).astype(np.uint32)
        times = rng.uniform(0.0, clip.duration, size=n).astype(np.float32)
        d_handles, d_times, d_bones = up(np.full(n, handle), np.uint32), up(times, np.float32), up(bones, np.uint32)
        buffer = torch.full((n + 2 * GUARD, 12), float(SENTINEL), dtype=torch.float32, device="cuda")
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            ctx.decompress_track_object_batch(d_handles.data_ptr(), d_times.data_ptr(), d_bones.data_ptr(), n, buffer[GUARD].data_ptr(), stream=side.cuda_stream)    # warm-up
            side.synchronize()
            graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graph, stream=side):
                ctx.decompress_track_object_batch(d_handles.data_ptr(), d_times.data_ptr(), d_bones.data_ptr(), n, buffer[GUARD].data_ptr(), stream=side.cuda_stream)
        # further clips and hierarchies come and go; new sample times
        more = [ctx.register_clip(synth.build_clip(seed=300 + k, num_tracks=20 + k, num_samples=15).blob) for k in range(12)]
        for k, other in enumerate(more):
            ctx.set_clip_hierarchy(other, random_hierarchy(rng, 20 + k, 4))
        for other in more[::2]:
            ctx.unregister_clip(other)
        for replay in range(2):
            times = rng.uniform(0.0, clip.duration, size=n).astype(np.float32)
            d_times.copy_(torch.from_numpy(times))
            buffer.fill_(float(SENTINEL))
            torch.cuda.synchronize()
            graph.replay()
            torch.cuda.synchronize()
            expected = np.full((n + 2 * GUARD, 12), SENTINEL, dtype=np.float32)
            expected[GUARD:GUARD + n] = np.stack([oracle.pose(clip.blob, parents, t)[b] for t, b in zip(times, bones)])
            assert helpers.exact(buffer.cpu().numpy(), expected), replay
        del graph
        assert ctx.rejected_instance_count() == 0


def test_full_size_four_sockets_of_65536_characters():
    """65 536 instances x 4 sockets of one 100-bone clip, character-major: EVERY request against the oracle's object space poses"""
    rng = np.random.default_rng(0)
    clip = synth.build_clip(seed=7, num_tracks=100, num_samples=301)
    parents = np.array(synth.humanoid_hierarchy(100), dtype=np.uint32)
    depth = np.array([runtime.plan_bone_chain(parents, b, query_length_only=True) - 1 for b in range(100)])
    sockets = np.array([0, int(np.argmax(depth)), int(np.flatnonzero(depth >= 5)[0]), 99], dtype=np.uint32)
    n = 65536
    with runtime.Context(0) as ctx:
        handle = ctx.register_clip(clip.blob)
        ctx.set_clip_hierarchy(handle, parents)
        character_times = rng.uniform(0.0, clip.duration, size=n).astype(np.float32)
        times = np.repeat(character_times, sockets.size)
        bones = np.tile(sockets, n)
        got = launch_requests(ctx, np.full(times.size, handle, dtype=np.uint32), times, bones)
        poses = ob.oracle_decompress_poses_batch([clip.blob], np.zeros(n, dtype=np.uint32), character_times, 100, parent_indices=parents)
        expected = poses[:, sockets.astype(np.int64)].reshape(-1, 12)
        assert helpers.bit_equal(got, expected)
        assert not got[:, [7, 11]].any()                                       # the pads of translations and scales are 0
        assert ctx.rejected_instance_count() == 0
