"""The pose consumers in skeleton space (aclhip_register_skeleton, aclhip_decompress_poses_batch_mapped) through the C ABI. The expected
result is built from the existing oracle bindings and numpy indexing alone: per clip instance oracle_decompress_tracks, scattered by the
host copy of its map over the fill the header defines, then oracle_blend_poses, oracle_apply_additive_to_base and
oracle_local_to_object_space. Compared bit for bit over the whole sentinel filled buffer: guard rows before and after, and the bytes
between the skeleton's records and the stride. Needs a GPU."""
import itertools

import numpy as np
import pytest

from acl_amd import runtime, synth
from oracle import bindings as ob
import helpers

pytestmark = pytest.mark.gpu

DROPPED = runtime.TRACK_DROPPED
SENTINEL = np.float32(-7777.25)
NONE, RELATIVE, ADDITIVE0, ADDITIVE1 = runtime.ADDITIVE_NONE, runtime.ADDITIVE_RELATIVE, runtime.ADDITIVE_ADDITIVE0, runtime.ADDITIVE_ADDITIVE1

SHAPES = {
    "characters_100": dict(num_tracks=100, num_samples=61),
    "scaled_37": dict(num_tracks=37, num_samples=33, has_scale=1, scale_default=0.3),
    "two_windows_130": dict(num_tracks=130, num_samples=20, has_scale=1, scale_default=0.5),
    "stripped_wrap_50": dict(num_tracks=50, num_samples=100, strip_keyframes=1, wrap=1),
    "small_12": dict(num_tracks=12, num_samples=25),
}


def reference_pose(rng, num_bones):
    pose = np.zeros((num_bones, 12), dtype=np.float32)
    rotations = rng.normal(size=(num_bones, 4))
    pose[:, 0:4] = (rotations / np.linalg.norm(rotations, axis=1, keepdims=True)).astype(np.float32)
    pose[:, 4:7] = rng.uniform(-1.0, 1.0, size=(num_bones, 3))
    pose[:, 8:11] = rng.uniform(0.5, 1.5, size=(num_bones, 3))
    return pose


def additive_identity(num_bones, additive_format):
    pose = np.zeros((num_bones, 12), dtype=np.float32)
    pose[:, 3] = 1.0
    pose[:, 8:11] = 0.0 if additive_format == ADDITIVE1 else 1.0
    return pose


def make_map(rng, num_tracks, num_bones, kind):
    """identity | ordered (order preserving) | permutation | dropped (a third of the tracks, or whatever does not fit, dropped)"""
    table = np.full(num_tracks, DROPPED, dtype=np.uint32)
    if kind == "identity":
        assert num_tracks == num_bones
        return np.arange(num_tracks, dtype=np.uint32)
    keep = min(num_tracks, num_bones) if kind != "dropped" else min(num_tracks - num_tracks // 3, num_bones)
    tracks = np.sort(rng.choice(num_tracks, size=keep, replace=False))
    slots = rng.choice(num_bones, size=keep, replace=False)
    table[tracks] = np.sort(slots) if kind in ("ordered", "dropped") else slots
    return table


def skeleton_pose(blob, time, table, fill, rounding, options):
    decoded = ob.oracle_decompress_tracks(blob, float(time), rounding, options)
    pose = fill.copy()
    mapped = table != DROPPED
    pose[table[mapped]] = decoded[mapped]
    return pose


def expected_pose(skeleton, clips, weights, additive_format, base, object_space, rounding, looping):
    """skeleton: (R, parents); clips: [(blob, time, table)] -- the instance's clip and its blend partners; base: None, (blob, time, table) or a pose"""
    reference, parents = skeleton
    options = ob.default_options(looping_policy=looping)
    fill = reference if additive_format == NONE else additive_identity(reference.shape[0], additive_format)
    poses = [skeleton_pose(blob, time, table, fill, rounding, options) for blob, time, table in clips]
    pose = poses[0] if len(poses) == 1 else ob.oracle_blend_poses(poses, weights)
    if additive_format != NONE:
        base_pose = base if isinstance(base, np.ndarray) else skeleton_pose(base[0], base[1], base[2], reference, rounding, options)
        pose = ob.oracle_apply_additive_to_base(additive_format, base_pose, pose)
    if object_space:
        pose = ob.oracle_local_to_object_space(parents, pose)
    return pose


class Batch:
    """one mapped launch into a guarded, sentinel filled buffer; the device arrays are torch tensors"""

    def __init__(self, ctx, num_instances, num_bones, pad_floats=4):
        import torch
        self.torch, self.ctx, self.n, self.num_bones = torch, ctx, num_instances, num_bones
        self.device = torch.device("cuda:0")
        self.row_floats = num_bones * 12 + pad_floats
        self.consumers, self.mapping, self.keep = runtime.PoseConsumers(), runtime.PoseMapping(), []

    def up(self, array, dtype):
        array = np.ascontiguousarray(array, dtype=dtype)
        tensor = self.torch.from_numpy(array.view(np.int32) if dtype == np.uint32 else array).to(self.device)
        self.keep.append(tensor)
        return tensor.data_ptr()

    def launch(self, clips, times, params=None, stride_bytes=None, buffer=None):
        torch = self.torch
        if buffer is None:
            buffer = torch.full((self.n + 2, self.row_floats), float(SENTINEL), dtype=torch.float32, device=self.device)
        stream = torch.cuda.current_stream(self.device)
        self.ctx.decompress_poses_batch_mapped(self.up(clips, np.uint32), self.up(times, np.float32), self.n, buffer[1].data_ptr(),
                                               stride_bytes if stride_bytes is not None else self.row_floats * 4, self.consumers, self.mapping, params=params, stream=stream.cuda_stream)
        self.buffer = buffer
        return self

    def result(self):
        self.torch.cuda.current_stream(self.device).synchronize()
        return self.buffer.cpu().numpy()

    def expected(self, rows):
        """rows: per instance the expected pose [B_i, 12], or None for a refused instance"""
        out = np.full((self.n + 2, self.row_floats), SENTINEL, dtype=np.float32)
        for i, pose in enumerate(rows):
            if pose is not None:
                out[1 + i, : pose.size] = pose.reshape(-1)
        return out


def hierarchy(rng, num_bones):
    parents = np.zeros(num_bones, dtype=np.uint32)
    parents[0] = runtime.NO_PARENT
    for i in range(1, num_bones):
        parents[i] = rng.integers(max(0, i - 9), i)
    return parents


# (rounding, looping): every rounding policy a consumer takes (per track rounding is refused, as today) x clamp / wrap / as compressed
POLICIES = list(itertools.product((0, 1, 2, 3), (0, 1, 2)))


@pytest.mark.parametrize("name,num_bones,kind", [
    ("characters_100", 100, "identity"), ("characters_100", 128, "ordered"), ("characters_100", 128, "permutation"), ("characters_100", 110, "dropped"),
    ("scaled_37", 37, "identity"), ("scaled_37", 64, "permutation"), ("two_windows_130", 160, "ordered"), ("two_windows_130", 96, "dropped"),
    ("stripped_wrap_50", 70, "permutation"), ("stripped_wrap_50", 50, "dropped")])
def test_single_clip_local_and_object_space(name, num_bones, kind):
    rng = np.random.default_rng(len(name) * 1000 + num_bones)
    clips = [synth.build_clip(seed=900 + k, **dict(SHAPES[name], num_samples=SHAPES[name]["num_samples"] + 3 * k)) for k in range(3)]
    reference, parents = reference_pose(rng, num_bones), hierarchy(rng, num_bones)
    tables = [make_map(rng, SHAPES[name]["num_tracks"], num_bones, kind) for _ in clips]
    with runtime.Context(0) as ctx:
        handles = np.array([ctx.register_clip(c.blob) for c in clips], dtype=np.uint32)
        maps = np.array([ctx.register_track_map(t, num_bones) for t in tables], dtype=np.uint32)
        skeleton = ctx.register_skeleton(parents, reference)
        info = ctx.skeleton_info(skeleton)
        assert (info.num_bones, info.has_hierarchy) == (num_bones, 1)
        n = 37
        which = rng.integers(0, 3, size=n)
        times = np.array([rng.uniform(-0.05, clips[c].duration + 0.05) for c in which], dtype=np.float32)
        for rounding, looping in POLICIES:
            for object_space in (False, True):
                batch = Batch(ctx, n, num_bones)
                batch.consumers.object_space = int(object_space)
                batch.mapping.skeleton = skeleton
                batch.mapping.instance_maps = batch.up(maps[which], np.uint32)
                got = batch.launch(handles[which], times, params=runtime.default_params(rounding_policy=rounding, looping_policy=looping)).result()
                rows = [expected_pose((reference, parents), [(clips[c].blob, t, tables[c])], None, NONE, None, object_space, rounding, looping) for c, t in zip(which, times)]
                assert helpers.exact(got, batch.expected(rows)), (name, num_bones, kind, rounding, looping, object_space)
        assert ctx.rejected_instance_count() == 0


def blend_rig(rng, num_bones=128, shapes=("characters_100", "scaled_37", "small_12", "stripped_wrap_50")):
    """clips of different track counts, each with a map of its own: some bones animated by every clip, some by one, some by none"""
    clips = [synth.build_clip(seed=950 + k, **SHAPES[name]) for k, name in enumerate(shapes)]
    tables = []
    for k, name in enumerate(shapes):
        num_tracks = SHAPES[name]["num_tracks"]
        table = np.full(num_tracks, DROPPED, dtype=np.uint32)
        # the first 8 tracks of every clip animate bones 0..7; the rest lands anywhere in [8, num_bones - 16): the last 16 bones are nobody's
        table[:8] = np.arange(8)
        rest = min(num_tracks - 8, num_bones - 24)
        table[8:8 + rest] = 8 + rng.choice(num_bones - 24, size=rest, replace=False)
        if k == 1:
            table[8 + rest - 3:8 + rest] = DROPPED
        tables.append(table)
    return clips, tables


@pytest.mark.parametrize("num_blend", [2, 3, 4])
def test_blend_of_clips_with_different_track_counts(num_blend):
    rng = np.random.default_rng(40 + num_blend)
    num_bones = 128
    clips, tables = blend_rig(rng, num_bones)
    reference, parents = reference_pose(rng, num_bones), np.array(synth.humanoid_hierarchy(num_bones), dtype=np.uint32)
    with runtime.Context(0) as ctx:
        handles = np.array([ctx.register_clip(c.blob) for c in clips], dtype=np.uint32)
        maps = np.array([ctx.register_track_map(t, num_bones) for t in tables], dtype=np.uint32)
        skeleton = ctx.register_skeleton(parents, reference)
        n = 41
        first = rng.integers(0, 4, size=n)
        others = rng.integers(0, 4, size=(n, num_blend - 1))
        others[3, 0] = first[3]                                  # the same clip at the same time is decoded twice
        first[2], others[2, 0] = 0, 2                            # (the q / -q pair below)
        times = np.array([rng.uniform(0.0, clips[c].duration) for c in first], dtype=np.float32)
        other_times = np.array([[rng.uniform(0.0, clips[c].duration) for c in row] for row in others], dtype=np.float32)
        other_times[3, 0] = times[3]
        # a constructed q / -q pair: instance 2 blends the 100 track clip with the 12 track clip; on a bone only the first animates the
        # partner is FILLED, and that bone's reference rotation is the negated rotation the first clip decodes there
        flipped_track = int(np.flatnonzero((tables[0] != DROPPED) & ~np.isin(tables[0], tables[2]))[0])
        flipped_bone = int(tables[0][flipped_track])
        reference[flipped_bone, 0:4] = -ob.oracle_decompress_tracks(clips[0].blob, float(times[2]))[flipped_track, 0:4]
        ctx.unregister_skeleton(skeleton)
        skeleton = ctx.register_skeleton(parents, reference)
        pair = [skeleton_pose(clips[c].blob, times[2], tables[c], reference, 0, ob.default_options())[flipped_bone, 0:4] for c in (0, 2)]
        assert np.array_equal(pair[0], -pair[1]) and float(np.dot(pair[0], pair[1])) < -0.99
        weights = rng.dirichlet(np.ones(num_blend), size=n).astype(np.float32)
        weights[0] = 0.0
        weights[0, 0] = 1.0                                      # all the weight on the first clip
        weights[1] = 0.0
        weights[1, -1] = 1.0                                     # ... on the last
        base = rng.integers(0, 4, size=n)
        base_times = np.array([rng.uniform(0.0, clips[c].duration) for c in base], dtype=np.float32)
        base_buffer = np.stack([reference_pose(rng, num_bones) for _ in range(n)])
        # every additive format x {base clip with its own map, base buffer} x {local, object space} behind the blend, and the blend alone; the policies rotate
        combinations = [(NONE, False, False), (NONE, True, False)] + list(itertools.product((RELATIVE, ADDITIVE0, ADDITIVE1), (False, True), (False, True)))
        for index, (additive_format, object_space, base_as_buffer) in enumerate(combinations):
            rounding, looping = POLICIES[(5 * index + num_blend) % len(POLICIES)]
            batch = Batch(ctx, n, num_bones, pad_floats=0)
            consumers, mapping = batch.consumers, batch.mapping
            consumers.additive_format, consumers.object_space, consumers.num_blend_clips = additive_format, int(object_space), num_blend
            consumers.blend_clips, consumers.blend_sample_times, consumers.blend_weights = batch.up(handles[others], np.uint32), batch.up(other_times, np.float32), batch.up(weights, np.float32)
            mapping.skeleton, mapping.instance_maps, mapping.blend_maps = skeleton, batch.up(maps[first], np.uint32), batch.up(maps[others], np.uint32)
            if additive_format != NONE and base_as_buffer:
                consumers.base_poses, consumers.base_pose_stride_bytes = batch.up(base_buffer, np.float32), num_bones * 48
            elif additive_format != NONE:
                consumers.base_clips, consumers.base_sample_times, mapping.base_maps = batch.up(handles[base], np.uint32), batch.up(base_times, np.float32), batch.up(maps[base], np.uint32)
            got = batch.launch(handles[first], times, params=runtime.default_params(rounding_policy=rounding, looping_policy=looping)).result()
            rows = []
            for i in range(n):
                members = [(clips[first[i]].blob, times[i], tables[first[i]])] + [(clips[c].blob, t, tables[c]) for c, t in zip(others[i], other_times[i])]
                the_base = base_buffer[i] if base_as_buffer else (clips[base[i]].blob, base_times[i], tables[base[i]])
                rows.append(expected_pose((reference, parents), members, weights[i], additive_format, the_base, object_space, rounding, looping))
            assert helpers.exact(got, batch.expected(rows)), (num_blend, rounding, looping, additive_format, object_space, base_as_buffer)
        assert ctx.rejected_instance_count() == 0


@pytest.mark.parametrize("additive_format", [RELATIVE, ADDITIVE0, ADDITIVE1])
def test_additive_without_a_blend_and_unmapped_slots_are_the_identity(additive_format):
    rng = np.random.default_rng(70 + additive_format)
    num_bones = 100
    parents = np.array(synth.humanoid_hierarchy(num_bones), dtype=np.uint32)
    reference = reference_pose(rng, num_bones)
    base_clip = synth.build_clip(seed=981, num_tracks=100, num_samples=40, has_scale=1, scale_default=0.4)
    additive_clip = synth.build_clip(seed=982, num_tracks=37, num_samples=33, has_scale=1, scale_default=0.3)
    # the left arm of the humanoid: the first clavicle's chain -- bones the additive clip animates none of
    children = {i: [j for j in range(num_bones) if j != 0 and parents[j] == i] for i in range(num_bones)}
    arm_root = 20
    left_arm, stack = [], [arm_root]
    while stack:
        bone = stack.pop()
        left_arm.append(bone)
        stack += children[bone]
    left_arm = np.array(sorted(left_arm))
    free = np.setdiff1d(np.arange(num_bones), left_arm)
    additive_table = rng.choice(free, size=37, replace=False).astype(np.uint32)
    base_table = rng.permutation(num_bones).astype(np.uint32)
    with runtime.Context(0) as ctx:
        h_base, h_additive = ctx.register_clip(base_clip.blob), ctx.register_clip(additive_clip.blob)
        m_base, m_additive = ctx.register_track_map(base_table, num_bones), ctx.register_track_map(additive_table, num_bones)
        skeleton = ctx.register_skeleton(parents, reference)
        n = 24
        times = rng.uniform(0.0, additive_clip.duration, size=n).astype(np.float32)
        base_times = rng.uniform(0.0, base_clip.duration, size=n).astype(np.float32)
        base_buffer = np.stack([reference_pose(rng, num_bones) for _ in range(n)])
        for object_space in (False, True):
            for base_as_buffer in (False, True):
                batch = Batch(ctx, n, num_bones)
                batch.consumers.additive_format, batch.consumers.object_space = additive_format, int(object_space)
                batch.mapping.skeleton, batch.mapping.map = skeleton, m_additive
                if base_as_buffer:
                    batch.consumers.base_poses, batch.consumers.base_pose_stride_bytes = batch.up(base_buffer, np.float32), num_bones * 48
                else:
                    batch.consumers.base_clips, batch.consumers.base_sample_times = batch.up(np.full(n, h_base), np.uint32), batch.up(base_times, np.float32)
                    batch.mapping.base_maps = batch.up(np.full(n, m_base), np.uint32)
                got = batch.launch(np.full(n, h_additive), times).result()
                rows = [expected_pose((reference, parents), [(additive_clip.blob, times[i], additive_table)], None, additive_format,
                                      base_buffer[i] if base_as_buffer else (base_clip.blob, base_times[i], base_table), object_space, 0, 2) for i in range(n)]
                assert helpers.exact(got, batch.expected(rows)), (additive_format, object_space, base_as_buffer)
                if not object_space:
                    # independent of the oracle plumbing: bones the additive clip does not animate keep the base's local transform
                    poses = got[1:1 + n, : num_bones * 12].reshape(n, num_bones, 12)
                    for i in range(n):
                        base_pose = base_buffer[i] if base_as_buffer else skeleton_pose(base_clip.blob, base_times[i], base_table, reference, 0, ob.default_options())
                        assert np.abs(poses[i, left_arm] - base_pose[left_arm]).max() <= 1e-6, (additive_format, base_as_buffer, i)
        assert ctx.rejected_instance_count() == 0


def test_mixed_skeletons_share_workgroups():
    rng = np.random.default_rng(91)
    clip_a, clip_b = synth.build_clip(seed=991, **SHAPES["characters_100"]), synth.build_clip(seed=992, **SHAPES["scaled_37"])
    bones = (128, 60)
    references = [reference_pose(rng, b) for b in bones]
    parent_lists = [np.array(synth.humanoid_hierarchy(bones[0]), dtype=np.uint32), hierarchy(rng, bones[1])]
    tables = [[make_map(rng, 100, 128, "permutation"), make_map(rng, 37, 128, "ordered")], [make_map(rng, 100, 60, "dropped"), make_map(rng, 37, 60, "permutation")]]
    clips = (clip_a, clip_b)
    with runtime.Context(0) as ctx:
        handles = [ctx.register_clip(c.blob) for c in clips]
        skeletons = [ctx.register_skeleton(parent_lists[s], references[s]) for s in range(2)]
        maps = [[ctx.register_track_map(tables[s][c], bones[s]) for c in range(2)] for s in range(2)]
        n = 43
        which_skeleton = np.arange(n) % 2                        # adjacent instances, different skeletons: they share workgroups
        which_clip = rng.integers(0, 2, size=n)
        times = np.array([rng.uniform(0.0, clips[c].duration) for c in which_clip], dtype=np.float32)
        for object_space in (False, True):
            batch = Batch(ctx, n, 128)
            batch.consumers.object_space = int(object_space)
            batch.mapping.instance_skeletons = batch.up([skeletons[s] for s in which_skeleton], np.uint32)
            batch.mapping.instance_maps = batch.up([maps[s][c] for s, c in zip(which_skeleton, which_clip)], np.uint32)
            got = batch.launch([handles[c] for c in which_clip], times).result()
            rows = [expected_pose((references[s], parent_lists[s]), [(clips[c].blob, times[i], tables[s][c])], None, NONE, None, object_space, 0, 2)
                    for i, (s, c) in enumerate(zip(which_skeleton, which_clip))]
            assert helpers.exact(got, batch.expected(rows)), object_space
        assert ctx.rejected_instance_count() == 0


def test_a_negative_scale_in_the_reference_pose_is_counted_and_exact():
    rng = np.random.default_rng(93)
    num_bones = 64
    clip = synth.build_clip(seed=993, **SHAPES["scaled_37"])
    reference, parents = reference_pose(rng, num_bones), hierarchy(rng, num_bones)
    table = make_map(rng, 37, num_bones, "permutation")
    unmapped = np.setdiff1d(np.arange(num_bones), table)
    reference[unmapped[:5], 9] *= -1.0                           # mirrored bones no track overwrites
    with runtime.Context(0) as ctx:
        handle, track_map = ctx.register_clip(clip.blob), ctx.register_track_map(table, num_bones)
        skeleton = ctx.register_skeleton(parents, reference)
        assert ctx.skeleton_info(skeleton).has_negative_scale == 1
        n = 19
        times = rng.uniform(0.0, clip.duration, size=n).astype(np.float32)
        before = ctx.negative_scale_count()
        batch = Batch(ctx, n, num_bones)
        batch.consumers.object_space = 1
        batch.mapping.skeleton, batch.mapping.map = skeleton, track_map
        got = batch.launch(np.full(n, handle), times).result()
        rows = [expected_pose((reference, parents), [(clip.blob, t, table)], None, NONE, None, True, 0, 2) for t in times]
        assert helpers.exact(got, batch.expected(rows))
        assert ctx.negative_scale_count() > before
        assert ctx.rejected_instance_count() == 0
        # local space multiplies no transforms: a mirrored skeleton is served as it is -- alone, blended, under additive0 / additive1 onto a
        # base clip (scale x scale in one wave) and, through the matrix route, under the relative format
        partner = synth.build_clip(seed=994, **SHAPES["small_12"])
        partner_table = make_map(rng, 12, num_bones, "ordered")
        h_partner, m_partner = ctx.register_clip(partner.blob), ctx.register_track_map(partner_table, num_bones)
        partner_times = rng.uniform(0.0, partner.duration, size=n).astype(np.float32)
        weights = rng.dirichlet(np.ones(2), size=n).astype(np.float32)
        for blend, additive_format in ((False, NONE), (True, NONE), (False, ADDITIVE0), (False, ADDITIVE1), (False, RELATIVE), (True, ADDITIVE1)):
            batch = Batch(ctx, n, num_bones)
            batch.mapping.skeleton, batch.mapping.map = skeleton, track_map
            batch.consumers.additive_format = additive_format
            if blend:
                batch.consumers.num_blend_clips = 2
                batch.consumers.blend_clips, batch.consumers.blend_sample_times, batch.consumers.blend_weights = batch.up(np.full(n, h_partner), np.uint32), batch.up(partner_times, np.float32), batch.up(weights, np.float32)
                batch.mapping.blend_maps = batch.up(np.full(n, m_partner), np.uint32)
            if additive_format != NONE:
                batch.consumers.base_clips, batch.consumers.base_sample_times = batch.up(np.full(n, h_partner), np.uint32), batch.up(partner_times, np.float32)
                batch.mapping.base_maps = batch.up(np.full(n, m_partner), np.uint32)
            got = batch.launch(np.full(n, handle), times).result()
            rows = [expected_pose((reference, parents), [(clip.blob, times[i], table)] + ([(partner.blob, partner_times[i], partner_table)] if blend else []), weights[i],
                                  additive_format, (partner.blob, partner_times[i], partner_table), False, 0, 2) for i in range(n)]
            assert helpers.exact(got, batch.expected(rows)), (blend, additive_format)
            assert ctx.rejected_instance_count() == 0, (blend, additive_format)


def test_host_array_convenience_form():
    """Context.decompress_poses_mapped: host arrays in, host poses out -- a single clip in object space, and a blend of three onto a base clip"""
    rng = np.random.default_rng(94)
    num_bones = 128
    clips, tables = blend_rig(rng, num_bones)
    reference, parents = reference_pose(rng, num_bones), np.array(synth.humanoid_hierarchy(num_bones), dtype=np.uint32)
    with runtime.Context(0) as ctx:
        handles = np.array([ctx.register_clip(c.blob) for c in clips], dtype=np.uint32)
        maps = np.array([ctx.register_track_map(t, num_bones) for t in tables], dtype=np.uint32)
        skeleton = ctx.register_skeleton(parents, reference)
        n = 21
        first, others, base = rng.integers(0, 4, size=n), rng.integers(0, 4, size=(n, 2)), rng.integers(0, 4, size=n)
        times = np.array([rng.uniform(-0.05, clips[c].duration + 0.05) for c in first], dtype=np.float32)
        other_times = np.array([[rng.uniform(0.0, clips[c].duration) for c in row] for row in others], dtype=np.float32)
        base_times = np.array([rng.uniform(0.0, clips[c].duration) for c in base], dtype=np.float32)
        weights = rng.dirichlet(np.ones(3), size=n).astype(np.float32)
        rounding, looping = rng.integers(0, 4, size=n).astype(np.uint8), rng.integers(0, 3, size=n).astype(np.uint8)

        got = ctx.decompress_poses_mapped(handles[first], times, skeleton, maps[first], num_bones, object_space=True, instance_rounding=rounding, instance_looping=looping)
        for i in range(n):
            expected = expected_pose((reference, parents), [(clips[first[i]].blob, times[i], tables[first[i]])], None, NONE, None, True, int(rounding[i]), int(looping[i]))
            assert helpers.exact(got[i], expected), i

        got = ctx.decompress_poses_mapped(handles[first], times, skeleton, maps[first], num_bones, additive_format=RELATIVE, object_space=True,
                                          base_clips=handles[base], base_sample_times=base_times, base_maps=maps[base],
                                          blend_clips=handles[others], blend_sample_times=other_times, blend_maps=maps[others], blend_weights=weights)
        base_poses = np.empty((n, num_bones, 12), dtype=np.float32)
        for i in range(n):
            members = [(clips[first[i]].blob, times[i], tables[first[i]])] + [(clips[c].blob, t, tables[c]) for c, t in zip(others[i], other_times[i])]
            assert helpers.exact(got[i], expected_pose((reference, parents), members, weights[i], RELATIVE, (clips[base[i]].blob, base_times[i], tables[base[i]]), True, 0, 2)), i
            base_poses[i] = skeleton_pose(clips[base[i]].blob, base_times[i], tables[base[i]], reference, 0, ob.default_options())

        # a base pose buffer (already in skeleton order), local space
        got = ctx.decompress_poses_mapped(handles[first], times, skeleton, maps[first], num_bones, additive_format=ADDITIVE1, base_poses=base_poses)
        for i in range(n):
            assert helpers.exact(got[i], expected_pose((reference, parents), [(clips[first[i]].blob, times[i], tables[first[i]])], None, ADDITIVE1, base_poses[i], False, 0, 2)), i
        assert ctx.rejected_instance_count() == 0


def test_refusals_inside_an_otherwise_valid_batch():
    rng = np.random.default_rng(95)
    num_bones = 48
    clip, other = synth.build_clip(seed=995, **SHAPES["scaled_37"]), synth.build_clip(seed=996, **SHAPES["small_12"])
    scalars = synth.build_scalar_clip(seed=997, num_tracks=12, num_samples=25)
    reference, parents = reference_pose(rng, num_bones), hierarchy(rng, num_bones)
    table, other_table = make_map(rng, 37, num_bones, "permutation"), make_map(rng, 12, num_bones, "ordered")
    with runtime.Context(0) as ctx:
        h_clip, h_other = ctx.register_clip(clip.blob), ctx.register_clip(other.blob)
        m_clip, m_other = ctx.register_track_map(table, num_bones), ctx.register_track_map(other_table, num_bones)
        h_scalars = ctx.register_clip(scalars.blob)                                        # a scalar track list of 12 tracks: m_other has its track count
        assert ctx.clip_info(h_scalars).num_tracks == 12
        m_small = ctx.register_track_map(np.arange(37, dtype=np.uint32), 40)             # made for a skeleton of 40 bones
        m_retired = ctx.register_track_map(table, num_bones)
        skeleton = ctx.register_skeleton(parents, reference)
        flat = ctx.register_skeleton(None, reference)                                      # no hierarchy
        big_reference = reference_pose(rng, num_bones + 8)
        big = ctx.register_skeleton(hierarchy(rng, num_bones + 8), big_reference)          # more bones than a row holds
        m_big = ctx.register_track_map(make_map(rng, 37, num_bones + 8, "ordered"), num_bones + 8)
        retired = ctx.register_skeleton(parents, reference)
        ctx.unregister_track_map(m_retired)
        ctx.unregister_skeleton(retired)
        import torch
        torch.cuda.synchronize()
        garbage = 0xFFFFFFFF
        #            clip      map        skeleton   refused?
        cases = [(h_clip, m_clip, skeleton, False), (h_clip, garbage, skeleton, True), (h_clip, m_clip, garbage, True), (h_other, m_other, skeleton, False),
                 (h_clip, m_retired, skeleton, True), (h_clip, m_clip, retired, True), (h_clip, m_other, skeleton, True),       # a map of another track count
                 (h_clip, m_small, skeleton, True),                                                                         # a map into another slot count
                 (garbage, m_clip, skeleton, True), (h_clip, m_clip, flat, True),                                           # unknown clip; no hierarchy (object space)
                 (h_clip, m_big, big, True),                                                                                # 48 B > stride
                 (h_clip, 0, skeleton, True), (h_clip, m_clip, 0, True), (h_other, m_other, skeleton, False),
                 (h_scalars, m_other, skeleton, True), (h_clip, m_clip, skeleton, False)]                                   # a scalar clip, and a last good neighbour
        n = len(cases)
        times = rng.uniform(0.0, 0.3, size=n).astype(np.float32)
        tables_of = {m_clip: table, m_other: other_table}
        blobs_of = {h_clip: clip.blob, h_other: other.blob}
        before = ctx.rejected_instance_count()
        batch = Batch(ctx, n, num_bones)
        batch.consumers.object_space = 1
        batch.mapping.instance_skeletons = batch.up([c[2] for c in cases], np.uint32)
        batch.mapping.instance_maps = batch.up([c[1] for c in cases], np.uint32)
        got = batch.launch([c[0] for c in cases], times).result()
        rows = [None if refused else expected_pose((reference, parents), [(blobs_of[c], times[i], tables_of[m])], None, NONE, None, True, 0, 2)
                for i, (c, m, s, refused) in enumerate(cases)]
        assert helpers.exact(got, batch.expected(rows))
        assert ctx.rejected_instance_count() - before == sum(1 for c in cases if c[3])
        # local space: the skeleton without hierarchy serves
        before = ctx.rejected_instance_count()
        batch = Batch(ctx, 3, num_bones)
        batch.mapping.skeleton, batch.mapping.map = flat, m_clip
        got = batch.launch(np.full(3, h_clip), times[:3]).result()
        assert helpers.exact(got, batch.expected([expected_pose((reference, parents), [(clip.blob, t, table)], None, NONE, None, False, 0, 2) for t in times[:3]]))
        assert ctx.rejected_instance_count() == before
        # a blend partner and a base clip with a bad map refuse their instance; its neighbours are served
        before = ctx.rejected_instance_count()
        batch = Batch(ctx, 3, num_bones)
        weights = np.array([[0.25, 0.75]] * 3, dtype=np.float32)
        batch.consumers.num_blend_clips, batch.consumers.additive_format = 2, ADDITIVE0
        batch.consumers.blend_clips, batch.consumers.blend_sample_times, batch.consumers.blend_weights = batch.up(np.full(3, h_other), np.uint32), batch.up(times[:3], np.float32), batch.up(weights, np.float32)
        batch.consumers.base_clips, batch.consumers.base_sample_times = batch.up(np.full(3, h_clip), np.uint32), batch.up(times[3:6], np.float32)
        batch.mapping.skeleton, batch.mapping.map = skeleton, m_clip
        batch.mapping.blend_maps, batch.mapping.base_maps = batch.up([m_other, m_clip, m_other], np.uint32), batch.up([m_clip, m_clip, m_other], np.uint32)
        got = batch.launch(np.full(3, h_clip), times[:3]).result()
        good = expected_pose((reference, parents), [(clip.blob, times[0], table), (other.blob, times[0], other_table)], weights[0], ADDITIVE0, (clip.blob, times[3], table), False, 0, 2)
        assert helpers.exact(got, batch.expected([good, None, None]))
        assert ctx.rejected_instance_count() - before == 2
        # host side refusals
        for spoil in ("mapping", "skeleton", "map", "blend_maps", "base_maps"):
            batch = Batch(ctx, 3, num_bones)
            batch.mapping.skeleton, batch.mapping.map = skeleton, m_clip
            if spoil == "skeleton":
                batch.mapping.skeleton = 0
            if spoil == "map":
                batch.mapping.map = 0
            if spoil == "blend_maps":
                batch.consumers.num_blend_clips = 2
                batch.consumers.blend_clips, batch.consumers.blend_sample_times, batch.consumers.blend_weights = batch.up(np.full(3, h_other), np.uint32), batch.up(times[:3], np.float32), batch.up(weights, np.float32)
            if spoil == "base_maps":
                batch.consumers.additive_format = ADDITIVE1
                batch.consumers.base_clips, batch.consumers.base_sample_times = batch.up(np.full(3, h_clip), np.uint32), batch.up(times[:3], np.float32)
            if spoil == "mapping":
                batch.mapping = None
            with pytest.raises(runtime.AclHipError) as error:
                batch.launch(np.full(3, h_clip), times[:3])
            assert error.value.status == runtime.ERROR_INVALID_ARGUMENT, spoil


def test_lifetime_unregister_behind_a_launch_and_graph_replay():
    import torch
    rng = np.random.default_rng(97)
    num_bones = 128
    clips, tables = blend_rig(rng, num_bones)
    reference, parents = reference_pose(rng, num_bones), np.array(synth.humanoid_hierarchy(num_bones), dtype=np.uint32)
    with runtime.Context(0) as ctx:
        handles = np.array([ctx.register_clip(c.blob) for c in clips], dtype=np.uint32)
        n = 64
        which = rng.integers(0, 4, size=n)
        times = np.array([rng.uniform(0.0, clips[c].duration) for c in which], dtype=np.float32)
        rows = [expected_pose((reference, parents), [(clips[c].blob, t, tables[c])], None, NONE, None, True, 0, 2) for c, t in zip(which, times)]

        # unregistered right behind the enqueued launch: it still completes with the right bits
        maps = np.array([ctx.register_track_map(t, num_bones) for t in tables], dtype=np.uint32)
        skeleton = ctx.register_skeleton(parents, reference)
        batch = Batch(ctx, n, num_bones)
        batch.consumers.object_space = 1
        batch.mapping.skeleton, batch.mapping.instance_maps = skeleton, batch.up(maps[which], np.uint32)
        batch.launch(handles[which], times)
        ctx.unregister_skeleton(skeleton)
        for track_map in maps:
            ctx.unregister_track_map(int(track_map))
        assert helpers.exact(batch.result(), batch.expected(rows))
        assert ctx.rejected_instance_count() == 0

        # a captured graph replays correctly after other skeletons and maps came and went (the tables never move)
        maps = np.array([ctx.register_track_map(t, num_bones) for t in tables], dtype=np.uint32)
        skeleton = ctx.register_skeleton(parents, reference)
        batch = Batch(ctx, n, num_bones)
        batch.consumers.object_space = 1
        batch.mapping.skeleton, batch.mapping.instance_maps = skeleton, batch.up(maps[which], np.uint32)
        d_clips, d_times = batch.up(handles[which], np.uint32), batch.up(times, np.float32)
        buffer = torch.full((n + 2, batch.row_floats), float(SENTINEL), dtype=torch.float32, device=batch.device)
        side = torch.cuda.Stream(device=batch.device)
        side.wait_stream(torch.cuda.current_stream(batch.device))
        with torch.cuda.stream(side):
            ctx.decompress_poses_batch_mapped(d_clips, d_times, n, buffer[1].data_ptr(), batch.row_floats * 4, batch.consumers, batch.mapping, stream=side.cuda_stream)   # warm-up
            side.synchronize()
            graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graph, stream=side):
                ctx.decompress_poses_batch_mapped(d_clips, d_times, n, buffer[1].data_ptr(), batch.row_floats * 4, batch.consumers, batch.mapping, stream=side.cuda_stream)
        others = [ctx.register_skeleton(hierarchy(rng, 30 + k), reference_pose(rng, 30 + k)) for k in range(5)]
        other_maps = [ctx.register_track_map(make_map(rng, 12, 40, "ordered"), 40) for _ in range(9)]
        for handle in others[::2]:
            ctx.unregister_skeleton(handle)
        for handle in other_maps[1::2]:
            ctx.unregister_track_map(handle)
        buffer.fill_(float(SENTINEL))
        graph.replay()
        torch.cuda.synchronize()
        assert helpers.exact(buffer.cpu().numpy(), batch.expected(rows))
        del graph


def test_full_size_three_clip_blend_in_object_space_every_instance():
    """65 536 instances, each a blend of three differently shaped clips in a 128-bone skeleton, object space: every pose against the oracle"""
    import concurrent.futures
    rng = np.random.default_rng(99)
    num_bones, n, num_blend = 128, 65536, 3
    clips, tables = blend_rig(rng, num_bones, shapes=("characters_100", "scaled_37", "small_12"))
    reference, parents = reference_pose(rng, num_bones), np.array(synth.humanoid_hierarchy(num_bones), dtype=np.uint32)
    with runtime.Context(0) as ctx:
        handles = np.array([ctx.register_clip(c.blob) for c in clips], dtype=np.uint32)
        maps = np.array([ctx.register_track_map(t, num_bones) for t in tables], dtype=np.uint32)
        skeleton = ctx.register_skeleton(parents, reference)
        member = np.stack([rng.permutation(3) for _ in range(n)])            # every instance blends the three clips, in its own order
        times = np.stack([rng.uniform(0.0, clips[k].duration, size=n) for k in range(3)], axis=1).astype(np.float32)      # [n, clip]
        member_times = np.take_along_axis(times, member, axis=1)
        weights = rng.dirichlet(np.ones(num_blend), size=n).astype(np.float32)
        batch = Batch(ctx, n, num_bones, pad_floats=0)
        consumers, mapping = batch.consumers, batch.mapping
        consumers.object_space, consumers.num_blend_clips = 1, num_blend
        consumers.blend_clips, consumers.blend_sample_times, consumers.blend_weights = batch.up(handles[member[:, 1:]], np.uint32), batch.up(member_times[:, 1:], np.float32), batch.up(weights, np.float32)
        mapping.skeleton, mapping.instance_maps, mapping.blend_maps = skeleton, batch.up(maps[member[:, 0]], np.uint32), batch.up(maps[member[:, 1:]], np.uint32)
        got = batch.launch(handles[member[:, 0]], member_times[:, 0]).result()
        assert ctx.rejected_instance_count() == 0

        # the K decodes in batches (the oracle's own threads), scattered over the fill with numpy; blend and walk per instance on host threads
        skeleton_poses = np.empty((num_blend, n, num_bones, 12), dtype=np.float32)
        blobs = [c.blob for c in clips]
        for k in range(num_blend):
            decoded = ob.oracle_decompress_tracks_batch(blobs, member[:, k], member_times[:, k], 100)
            skeleton_poses[k] = reference
            for c in range(3):
                rows_of_clip = np.flatnonzero(member[:, k] == c)
                mapped = tables[c] != DROPPED
                skeleton_poses[k][np.ix_(rows_of_clip, tables[c][mapped])] = decoded[rows_of_clip][:, np.flatnonzero(mapped)]
            del decoded

        def finish(i):
            return ob.oracle_local_to_object_space(parents, ob.oracle_blend_poses([skeleton_poses[k, i] for k in range(num_blend)], weights[i]))

        poses = got[1:1 + n].reshape(n, num_bones, 12)
        with concurrent.futures.ThreadPoolExecutor(max_workers=16) as pool:
            for i, expected in enumerate(pool.map(finish, range(n), chunksize=512)):
                assert helpers.bit_equal(poses[i], expected), i
        assert np.all(got[0] == SENTINEL) and np.all(got[-1] == SENTINEL)
