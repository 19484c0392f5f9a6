"""Blend masks (aclhip_register_blend_mask, aclhip_decompress_poses_batch_masked) through the C ABI: the skeleton space blend with a
weight per (instance, clip, slot). The expected pose is built from the existing oracle bindings alone, as tests/test_gpu_skeleton_poses.py
builds it: the skeleton pose of every clip, the per slot weights from numpy float32 arithmetic in the order include/aclhip.h defines,
ob.oracle_blend_poses once per DISTINCT weight tuple of the instance over the slots that carry it (the blend is per transform: this is the
definition, not an approximation), then oracle_apply_additive_to_base and oracle_local_to_object_space. Compared bit for bit over the
whole sentinel filled buffer with its guard rows. Inputs keep one weight of every slot above 0 (weighted mode: clip 0's mask >= 0.25;
layered mode: e_0 == 1) and every test asserts that its expected poses are finite before it compares. Needs a GPU."""
import concurrent.futures
import itertools

import numpy as np
import pytest

from acl_amd import runtime, synth
from oracle import bindings as ob
import helpers
import test_gpu_skeleton_poses as sk

pytestmark = pytest.mark.gpu

DROPPED, SENTINEL = sk.DROPPED, sk.SENTINEL
NONE, RELATIVE, ADDITIVE0, ADDITIVE1 = sk.NONE, sk.RELATIVE, sk.ADDITIVE0, sk.ADDITIVE1
WEIGHTED, LAYERED = runtime.BLEND_WEIGHTED, runtime.BLEND_LAYERED
ONE = np.float32(1.0)


def slot_weights(weights, masks, mode, num_bones):
    """The definition: weights [K], masks K arrays [B] or None (the null handle) -> the weight of clip k at slot s, float32 [K, B]"""
    num_clips = len(weights)
    opacity = np.empty((num_clips, num_bones), dtype=np.float32)
    for k in range(num_clips):
        opacity[k] = np.float32(weights[k]) if masks[k] is None else np.float32(weights[k]) * np.asarray(masks[k], dtype=np.float32)
    if mode == WEIGHTED:
        return opacity
    layered = np.empty_like(opacity)
    for k in range(num_clips):
        rest = np.ones(num_bones, dtype=np.float32)
        for j in range(num_clips - 1, k, -1):
            rest = rest * (ONE - opacity[j])
        layered[k] = opacity[k] * rest
    assert layered.dtype == np.float32
    return layered


def masked_blend(poses, per_slot):
    """ob.oracle_blend_poses once per distinct weight tuple (by bits), over the slots that carry it"""
    columns = np.ascontiguousarray(per_slot.T).view(np.uint32)                      # [B, K]
    tuples, inverse = np.unique(columns, axis=0, return_inverse=True)
    inverse = np.asarray(inverse).reshape(-1)
    out = np.empty_like(poses[0])
    for index in range(tuples.shape[0]):
        slots = np.flatnonzero(inverse == index)
        out[slots] = ob.oracle_blend_poses([pose[slots] for pose in poses], np.ascontiguousarray(tuples[index]).view(np.float32))
    return out


def expected_masked_pose(skeleton, clips, weights, masks, mode, additive_format, base, object_space, rounding, looping):
    """sk.expected_pose with the masked blend in the place of the blend"""
    reference, parents = skeleton
    options = ob.default_options(looping_policy=looping)
    fill = reference if additive_format == NONE else sk.additive_identity(reference.shape[0], additive_format)
    poses = [sk.skeleton_pose(blob, time, table, fill, rounding, options) for blob, time, table in clips]
    pose = masked_blend(poses, slot_weights(weights, masks, mode, reference.shape[0]))
    if additive_format != NONE:
        base_pose = base if isinstance(base, np.ndarray) else sk.skeleton_pose(base[0], base[1], base[2], reference, rounding, options)
        pose = ob.oracle_apply_additive_to_base(additive_format, base_pose, pose)
    if object_space:
        pose = ob.oracle_local_to_object_space(parents, pose)
    return pose


class MaskedBatch(sk.Batch):
    """sk.Batch through aclhip_decompress_poses_batch_masked; launch_unmasked is the same batch through the mapped launch"""

    def __init__(self, ctx, num_instances, num_bones, pad_floats=4):
        super().__init__(ctx, num_instances, num_bones, pad_floats)
        self.masking = runtime.BlendMasking()

    def launch(self, clips, times, params=None, buffer=None):
        torch = self.torch
        if buffer is None:
            buffer = torch.full((self.n + 2, self.row_floats), float(SENTINEL), dtype=torch.float32, device=self.device)
        stream = torch.cuda.current_stream(self.device)
        self.ctx.decompress_poses_batch_masked(self.up(clips, np.uint32), self.up(times, np.float32), self.n, buffer[1].data_ptr(), self.row_floats * 4,
                                               self.consumers, self.mapping, self.masking, params=params, stream=stream.cuda_stream)
        self.buffer = buffer
        return self

    def launch_unmasked(self, clips, times, params=None):
        return sk.Batch.launch(self, clips, times, params=params)


def make_masks(rng, num_bones, count, floor=0.0):
    """random in [floor, 1] with an exact run of 1 (an "upper body" range) and, without a floor, an all-zero tail"""
    masks = []
    for index in range(count):
        mask = rng.uniform(floor, 1.0, size=num_bones).astype(np.float32)
        first = int(rng.integers(num_bones // 4, num_bones // 3))
        mask[first:first + num_bones // 3] = 1.0
        if floor == 0.0:
            mask[num_bones - num_bones // 8 - index:] = 0.0
            mask[int(rng.integers(0, first))] = 0.0
        masks.append(mask)
    return masks


def blend_weights(rng, mode, n, num_blend):
    if mode == WEIGHTED:
        return rng.dirichlet(np.ones(num_blend), size=n).astype(np.float32)            # (strictly positive: clip 0 carries every slot)
    weights = rng.uniform(0.0, 1.0, size=(n, num_blend)).astype(np.float32)
    weights[:, 0] = 1.0                                                                # e_0 == 1: the bottom layer is opaque
    weights[0, 1:] = 1.0                                                               # opaque layers above
    weights[1, 1:] = 0.0                                                               # transparent layers above
    return weights


@pytest.mark.parametrize("num_blend", [2, 3, 4])
@pytest.mark.parametrize("mode", [WEIGHTED, LAYERED])
def test_masked_blend_of_clips_with_different_track_counts(mode, num_blend):
    rng = np.random.default_rng(140 + 10 * mode + num_blend)
    num_bones = 128
    clips, tables = sk.blend_rig(rng, num_bones)
    reference, parents = sk.reference_pose(rng, num_bones), np.array(synth.humanoid_hierarchy(num_bones), dtype=np.uint32)
    # masks of the bottom clip: >= 0.25 everywhere in weighted mode, 1 everywhere in layered mode (or the null handle); the others are free
    bottom_masks = make_masks(rng, num_bones, 2, floor=0.25) if mode == WEIGHTED else [np.ones(num_bones, dtype=np.float32)]
    upper_masks = make_masks(rng, num_bones, 5)
    with runtime.Context(0) as ctx:
        handles = np.array([ctx.register_clip(c.blob) for c in clips], dtype=np.uint32)
        maps = np.array([ctx.register_track_map(t, num_bones) for t in tables], dtype=np.uint32)
        skeleton = ctx.register_skeleton(parents, reference)
        bottom_handles = [0] + [ctx.register_blend_mask(m) for m in bottom_masks]
        upper_handles = [0] + [ctx.register_blend_mask(m) for m in upper_masks]
        mask_of = {0: None}
        mask_of.update(zip(bottom_handles[1:], bottom_masks))
        mask_of.update(zip(upper_handles[1:], upper_masks))
        info = ctx.blend_mask_info(upper_handles[1])
        assert (info.num_slots, info.num_zero, info.num_one) == (num_bones, int((upper_masks[0] == 0).sum()), int((upper_masks[0] == 1).sum()))
        n = 23
        first = rng.integers(0, 4, size=n)
        others = rng.integers(0, 4, size=(n, num_blend - 1))
        times = np.array([rng.uniform(0.0, clips[c].duration) for c in first], dtype=np.float32)
        other_times = np.array([[rng.uniform(0.0, clips[c].duration) for c in row] for row in others], dtype=np.float32)
        weights = blend_weights(rng, mode, n, num_blend)
        instance_masks = np.empty((n, num_blend), dtype=np.uint32)                     # per instance handles, some of them null
        instance_masks[:, 0] = rng.choice(bottom_handles, size=n)
        instance_masks[:, 1:] = rng.choice(upper_handles, size=(n, num_blend - 1))
        instance_masks[2, 1:] = 0
        base = rng.integers(0, 4, size=n)
        base_times = np.array([rng.uniform(0.0, clips[c].duration) for c in base], dtype=np.float32)
        base_buffer = np.stack([sk.reference_pose(rng, num_bones) for _ in range(n)])
        combinations = [(NONE, False, False), (NONE, True, False)] + list(itertools.product((RELATIVE, ADDITIVE0, ADDITIVE1), (False, True), (False, True)))
        for index, (additive_format, object_space, base_as_buffer) in enumerate(combinations):
            rounding, looping = sk.POLICIES[(5 * index + num_blend + 3 * mode) % len(sk.POLICIES)]
            batch = MaskedBatch(ctx, n, num_bones, pad_floats=0 if index % 2 else 4)
            consumers, mapping = batch.consumers, batch.mapping
            consumers.additive_format, consumers.object_space, consumers.num_blend_clips = additive_format, int(object_space), num_blend
            consumers.blend_clips, consumers.blend_sample_times, consumers.blend_weights = batch.up(handles[others], np.uint32), batch.up(other_times, np.float32), batch.up(weights, np.float32)
            mapping.skeleton, mapping.instance_maps, mapping.blend_maps = skeleton, batch.up(maps[first], np.uint32), batch.up(maps[others], np.uint32)
            batch.masking.mode, batch.masking.instance_masks = mode, batch.up(instance_masks, np.uint32)
            if additive_format != NONE and base_as_buffer:
                consumers.base_poses, consumers.base_pose_stride_bytes = batch.up(base_buffer, np.float32), num_bones * 48
            elif additive_format != NONE:
                consumers.base_clips, consumers.base_sample_times, mapping.base_maps = batch.up(handles[base], np.uint32), batch.up(base_times, np.float32), batch.up(maps[base], np.uint32)
            got = batch.launch(handles[first], times, params=runtime.default_params(rounding_policy=rounding, looping_policy=looping)).result()
            rows = []
            for i in range(n):
                members = [(clips[first[i]].blob, times[i], tables[first[i]])] + [(clips[c].blob, t, tables[c]) for c, t in zip(others[i], other_times[i])]
                the_base = base_buffer[i] if base_as_buffer else (clips[base[i]].blob, base_times[i], tables[base[i]])
                rows.append(expected_masked_pose((reference, parents), members, weights[i], [mask_of[int(h)] for h in instance_masks[i]], mode,
                                                 additive_format, the_base, object_space, rounding, looping))
            assert np.isfinite(np.stack(rows)).all()
            assert helpers.exact(got, batch.expected(rows)), (mode, num_blend, rounding, looping, additive_format, object_space, base_as_buffer)
        assert ctx.rejected_instance_count() == 0


def test_nothing_changes_when_nothing_is_masked():
    rng = np.random.default_rng(151)
    num_bones = 128
    clips, tables = sk.blend_rig(rng, num_bones)
    reference, parents = sk.reference_pose(rng, num_bones), np.array(synth.humanoid_hierarchy(num_bones), dtype=np.uint32)
    with runtime.Context(0) as ctx:
        handles = np.array([ctx.register_clip(c.blob) for c in clips], dtype=np.uint32)
        maps = np.array([ctx.register_track_map(t, num_bones) for t in tables], dtype=np.uint32)
        skeleton = ctx.register_skeleton(parents, reference)
        n = 37

        def batch_of(num_blend, weights, object_space, additive_format=NONE):
            batch = MaskedBatch(ctx, n, num_bones)
            consumers, mapping = batch.consumers, batch.mapping
            consumers.object_space, consumers.num_blend_clips, consumers.additive_format = int(object_space), num_blend, additive_format
            consumers.blend_clips, consumers.blend_sample_times, consumers.blend_weights = batch.up(handles[others[:, :num_blend - 1]], np.uint32), batch.up(other_times[:, :num_blend - 1], np.float32), batch.up(weights, np.float32)
            mapping.skeleton, mapping.instance_maps, mapping.blend_maps = skeleton, batch.up(maps[first], np.uint32), batch.up(maps[others[:, :num_blend - 1]], np.uint32)
            if additive_format != NONE:
                consumers.base_clips, consumers.base_sample_times, mapping.base_maps = batch.up(handles[first], np.uint32), batch.up(times, np.float32), batch.up(maps[first], np.uint32)
            return batch

        first, others = rng.integers(0, 4, size=n), rng.integers(0, 4, size=(n, 3))
        times = np.array([rng.uniform(0.0, clips[c].duration) for c in first], dtype=np.float32)
        other_times = np.array([[rng.uniform(0.0, clips[c].duration) for c in row] for row in others], dtype=np.float32)
        ones = ctx.register_blend_mask(np.ones(num_bones, dtype=np.float32))
        # weighted mode, every handle 0 / a registered all-ones mask / a mix of both: the bits of the unmasked launch on the same batch
        for num_blend, object_space, additive_format in ((2, False, NONE), (3, True, NONE), (4, True, RELATIVE), (3, False, ADDITIVE1)):
            weights = rng.dirichlet(np.ones(num_blend), size=n).astype(np.float32)
            unmasked = batch_of(num_blend, weights, object_space, additive_format).launch_unmasked(handles[first], times).result()
            assert not np.all(unmasked[1:1 + n] == SENTINEL)
            for instance_masks in (np.zeros((n, num_blend)), np.full((n, num_blend), ones), rng.choice([0, ones], size=(n, num_blend))):
                batch = batch_of(num_blend, weights, object_space, additive_format)
                batch.masking.mode, batch.masking.instance_masks = WEIGHTED, batch.up(instance_masks, np.uint32)
                assert helpers.exact(batch.launch(handles[first], times).result(), unmasked), (num_blend, object_space, additive_format)
        # layered mode, local space, K = 2, mask 1: w = (1, 1) returns the top clip, w = (1, 0) the bottom clip -- BY VALUE, against that
        # clip's skeleton pose through the blend's final normalize (x * 0 added to the sum can flip the sign of a zero)
        options = ob.default_options()
        for top_weight, returned in ((1.0, 1), (0.0, 0)):
            weights = np.tile(np.array([1.0, top_weight], dtype=np.float32), (n, 1))
            for instance_masks in (np.full((n, 2), ones), np.zeros((n, 2))):
                batch = batch_of(2, weights, False)
                batch.masking.mode, batch.masking.instance_masks = LAYERED, batch.up(instance_masks, np.uint32)
                got = batch.launch(handles[first], times).result()
                rows = []
                for i in range(n):
                    member = (first[i], times[i]) if returned == 0 else (others[i, 0], other_times[i, 0])
                    rows.append(ob.oracle_blend_poses([sk.skeleton_pose(clips[member[0]].blob, member[1], tables[member[0]], reference, 0, options)], [1.0]))
                expected = batch.expected(rows)
                assert np.isfinite(np.stack(rows)).all()
                assert np.array_equal(got, expected), (top_weight, returned)              # == on the floats
        assert ctx.rejected_instance_count() == 0


def test_an_upper_body_layer_leaves_the_walking_legs_alone():
    """The use case: a walk (all bones) under an upper-body clip (maps to the upper half only), layered, w = (1, 1), the mask 1 on the upper
    half and 0 on the legs. The legs are the walk's; through the unmasked launch with the same clips and weights they are not."""
    rng = np.random.default_rng(152)
    num_bones = 100
    walk = synth.build_clip(seed=1001, num_tracks=100, num_samples=61)
    wave = synth.build_clip(seed=1002, num_tracks=50, num_samples=33)
    reference, parents = sk.reference_pose(rng, num_bones), np.array(synth.humanoid_hierarchy(num_bones), dtype=np.uint32)
    upper, legs = np.arange(0, 50), np.arange(50, 100)
    walk_table = np.arange(num_bones, dtype=np.uint32)
    wave_table = rng.permutation(upper).astype(np.uint32)                               # the upper-body clip's 50 tracks, all in the upper half
    mask = np.zeros(num_bones, dtype=np.float32)
    mask[upper] = 1.0
    with runtime.Context(0) as ctx:
        h_walk, h_wave = ctx.register_clip(walk.blob), ctx.register_clip(wave.blob)
        m_walk, m_wave = ctx.register_track_map(walk_table, num_bones), ctx.register_track_map(wave_table, num_bones)
        skeleton = ctx.register_skeleton(parents, reference)
        upper_body = ctx.register_blend_mask(mask)
        info = ctx.blend_mask_info(upper_body)
        assert (info.num_slots, info.num_zero, info.num_one) == (100, 50, 50)
        n = 33
        times = rng.uniform(0.0, walk.duration, size=n).astype(np.float32)
        wave_times = rng.uniform(0.0, wave.duration, size=n).astype(np.float32)
        weights = np.ones((n, 2), dtype=np.float32)
        batch = MaskedBatch(ctx, n, num_bones)
        consumers, mapping = batch.consumers, batch.mapping
        consumers.num_blend_clips = 2
        consumers.blend_clips, consumers.blend_sample_times, consumers.blend_weights = batch.up(np.full(n, h_wave), np.uint32), batch.up(wave_times, np.float32), batch.up(weights, np.float32)
        mapping.skeleton, mapping.map, mapping.blend_maps = skeleton, m_walk, batch.up(np.full(n, m_wave), np.uint32)
        batch.masking.mode, batch.masking.instance_masks = LAYERED, batch.up(np.tile(np.array([0, upper_body]), (n, 1)), np.uint32)
        got = batch.launch(np.full(n, h_walk), times).result()
        unmasked = batch.launch_unmasked(np.full(n, h_walk), times).result()
        options = ob.default_options()
        rows, walks = [], []
        for i in range(n):
            members = [(walk.blob, times[i], walk_table), (wave.blob, wave_times[i], wave_table)]
            rows.append(expected_masked_pose((reference, parents), members, weights[i], [None, mask], LAYERED, NONE, None, False, 0, 2))
            walks.append(ob.oracle_blend_poses([sk.skeleton_pose(walk.blob, times[i], walk_table, reference, 0, options)], [1.0]))
        assert np.isfinite(np.stack(rows)).all()
        assert helpers.exact(got, batch.expected(rows))
        poses = got[1:1 + n, : num_bones * 12].reshape(n, num_bones, 12)
        unmasked_poses = unmasked[1:1 + n, : num_bones * 12].reshape(n, num_bones, 12)
        walks = np.stack(walks)
        assert np.array_equal(poses[:, legs], walks[:, legs])                             # the legs walk (== on the floats)
        for i in range(n):
            assert not np.array_equal(unmasked_poses[i, legs], walks[i, legs]), i         # the defect: one weight per clip drags them to the fill
        assert not np.array_equal(poses[:, upper], walks[:, upper])                       # ... and the upper body is the upper-body clip's
        assert ctx.rejected_instance_count() == 0


def test_refusals_inside_an_otherwise_valid_batch_and_host_side_refusals():
    import torch
    rng = np.random.default_rng(153)
    num_bones = 48
    clip, other = synth.build_clip(seed=995, **sk.SHAPES["scaled_37"]), synth.build_clip(seed=996, **sk.SHAPES["small_12"])
    reference, parents = sk.reference_pose(rng, num_bones), sk.hierarchy(rng, num_bones)
    table, other_table = sk.make_map(rng, 37, num_bones, "permutation"), sk.make_map(rng, 12, num_bones, "ordered")
    good_mask, bottom_mask = make_masks(rng, num_bones, 1)[0], make_masks(rng, num_bones, 1, floor=0.25)[0]
    with runtime.Context(0) as ctx:
        h_clip, h_other = ctx.register_clip(clip.blob), ctx.register_clip(other.blob)
        m_clip, m_other = ctx.register_track_map(table, num_bones), ctx.register_track_map(other_table, num_bones)
        skeleton = ctx.register_skeleton(parents, reference)
        # before any mask was registered: the null handle serves, every other handle is refused
        n = 3
        times = rng.uniform(0.0, 0.3, size=n).astype(np.float32)
        weights = np.tile(np.array([0.25, 0.75], dtype=np.float32), (16, 1))

        def batch_of(count, instance_masks, mode=WEIGHTED):
            batch = MaskedBatch(ctx, count, num_bones)
            batch.consumers.num_blend_clips, batch.consumers.object_space = 2, 1
            batch.consumers.blend_clips, batch.consumers.blend_sample_times, batch.consumers.blend_weights = batch.up(np.full(count, h_other), np.uint32), batch.up(np.resize(times, count), np.float32), batch.up(weights[:count], np.float32)
            batch.mapping.skeleton, batch.mapping.map, batch.mapping.blend_maps = skeleton, m_clip, batch.up(np.full(count, m_other), np.uint32)
            batch.masking.mode, batch.masking.instance_masks = mode, batch.up(instance_masks, np.uint32)
            return batch

        def expected_row(time, masks, mode=WEIGHTED):
            row = expected_masked_pose((reference, parents), [(clip.blob, time, table), (other.blob, time, other_table)], weights[0], masks, mode, NONE, None, True, 0, 2)
            assert np.isfinite(row).all()
            return row

        before = ctx.rejected_instance_count()
        batch = batch_of(n, [[0, 0], [0, 1], [0, 0]])
        got = batch.launch(np.full(n, h_clip), times).result()
        assert helpers.exact(got, batch.expected([expected_row(times[0], [None, None]), None, expected_row(times[2], [None, None])]))
        assert ctx.rejected_instance_count() - before == 1

        good, bottom = ctx.register_blend_mask(good_mask), ctx.register_blend_mask(bottom_mask)
        other_size = ctx.register_blend_mask(np.ones(num_bones + 1, dtype=np.float32))        # a mask of another slot count
        smaller = ctx.register_blend_mask(np.ones(num_bones - 1, dtype=np.float32))
        ones = ctx.register_blend_mask(np.ones(num_bones, dtype=np.float32))
        retired = ctx.register_blend_mask(good_mask)                                       # (the last one registered: nothing below reuses its handle)
        ctx.unregister_blend_mask(retired)
        with pytest.raises(runtime.AclHipError):
            ctx.unregister_blend_mask(retired)
        with pytest.raises(runtime.AclHipError):
            ctx.blend_mask_info(retired)
        torch.cuda.synchronize()
        garbage = 0xFFFFFFFF
        #          masks of (clip 0, clip 1)   refused?
        cases = [((bottom, good), False), ((retired, good), True), ((bottom, retired), True), ((0, good), False), ((garbage, 0), True), ((0, garbage), True),
                 ((other_size, good), True), ((bottom, other_size), True), ((bottom, smaller), True), ((runtime.MAX_BLEND_MASKS, 0), True), ((0, runtime.MAX_BLEND_MASKS + 7), True),
                 ((bottom, 0), False), ((0, 0), False), ((bottom, good), False)]
        n = len(cases)
        mask_of = {0: None, good: good_mask, bottom: bottom_mask, ones: np.ones(num_bones, dtype=np.float32)}
        for mode in (WEIGHTED, LAYERED):
            if mode == LAYERED:
                weights[:, 0] = 1.0
                cases = [((ones if pair[0] == bottom else pair[0], pair[1]), refused) for pair, refused in cases]
            times = rng.uniform(0.0, 0.3, size=n).astype(np.float32)
            before = ctx.rejected_instance_count()
            batch = batch_of(n, [pair for pair, _ in cases], mode)
            got = batch.launch(np.full(n, h_clip), times).result()
            rows = [None if refused else expected_row(times[i], [mask_of[pair[0]], mask_of[pair[1]]], mode) for i, (pair, refused) in enumerate(cases)]
            assert helpers.exact(got, batch.expected(rows)), mode                           # refused rows keep the sentinel, the neighbours are bit exact
            assert ctx.rejected_instance_count() - before == sum(1 for _, refused in cases if refused)

        # host side refusals: ACLHIP_ERROR_INVALID_ARGUMENT, nothing launched
        before = ctx.rejected_instance_count()
        for spoil in ("masking", "mode", "reserved0", "reserved", "instance_masks", "no blend", "mapping", "blend_maps", "skeleton"):
            batch = batch_of(3, [[0, 0]] * 3)
            if spoil == "masking":
                batch.masking = None
            if spoil == "mode":
                batch.masking.mode = 2
            if spoil == "reserved0":
                batch.masking.reserved0 = 1
            if spoil == "reserved":
                batch.masking.reserved[1] = 1
            if spoil == "instance_masks":
                batch.masking.instance_masks = None
            if spoil == "no blend":
                batch.consumers.num_blend_clips = 1
            if spoil == "mapping":
                batch.mapping = None
            if spoil == "blend_maps":
                batch.mapping.blend_maps = None
            if spoil == "skeleton":
                batch.mapping.skeleton = 0
            with pytest.raises(runtime.AclHipError) as error:
                batch.launch(np.full(3, h_clip), times[:3])
            assert error.value.status == runtime.ERROR_INVALID_ARGUMENT, spoil
        batch = batch_of(3, [[0, 0]] * 3)
        batch.consumers.num_blend_clips = 0
        with pytest.raises(runtime.AclHipError):
            batch.launch(np.full(3, h_clip), times[:3])
        for bad in (np.array([0.5, np.nan, 0.5]), np.array([0.5, 1.5]), np.array([-0.25]), np.zeros(0)):
            with pytest.raises(runtime.AclHipError) as error:
                ctx.register_blend_mask(bad.astype(np.float32))
            assert error.value.status == runtime.ERROR_INVALID_ARGUMENT
        torch.cuda.synchronize()
        assert ctx.rejected_instance_count() == before


def test_lifetime_unregister_behind_a_launch_and_graph_replay():
    import torch
    rng = np.random.default_rng(154)
    num_bones = 128
    clips, tables = sk.blend_rig(rng, num_bones)
    reference, parents = sk.reference_pose(rng, num_bones), np.array(synth.humanoid_hierarchy(num_bones), dtype=np.uint32)
    bottom_mask, upper_mask = make_masks(rng, num_bones, 1, floor=0.25)[0], make_masks(rng, num_bones, 1)[0]
    with runtime.Context(0) as ctx:
        handles = np.array([ctx.register_clip(c.blob) for c in clips], dtype=np.uint32)
        maps = np.array([ctx.register_track_map(t, num_bones) for t in tables], dtype=np.uint32)
        skeleton = ctx.register_skeleton(parents, reference)
        n = 64
        first, others = rng.integers(0, 4, size=n), rng.integers(0, 4, size=(n, 2))
        times = np.array([rng.uniform(0.0, clips[c].duration) for c in first], dtype=np.float32)
        other_times = np.array([[rng.uniform(0.0, clips[c].duration) for c in row] for row in others], dtype=np.float32)
        weights = rng.dirichlet(np.ones(3), size=n).astype(np.float32)
        rows = []
        for i in range(n):
            members = [(clips[first[i]].blob, times[i], tables[first[i]])] + [(clips[c].blob, t, tables[c]) for c, t in zip(others[i], other_times[i])]
            rows.append(expected_masked_pose((reference, parents), members, weights[i], [bottom_mask, None, upper_mask], WEIGHTED, NONE, None, True, 0, 2))
        assert np.isfinite(np.stack(rows)).all()

        def batch_of(bottom, upper):
            batch = MaskedBatch(ctx, n, num_bones)
            consumers, mapping = batch.consumers, batch.mapping
            consumers.object_space, consumers.num_blend_clips = 1, 3
            consumers.blend_clips, consumers.blend_sample_times, consumers.blend_weights = batch.up(handles[others], np.uint32), batch.up(other_times, np.float32), batch.up(weights, np.float32)
            mapping.skeleton, mapping.instance_maps, mapping.blend_maps = skeleton, batch.up(maps[first], np.uint32), batch.up(maps[others], np.uint32)
            batch.masking.mode, batch.masking.instance_masks = WEIGHTED, batch.up(np.tile(np.array([bottom, 0, upper]), (n, 1)), np.uint32)
            return batch

        # unregistered right behind the enqueued launch: it still completes with the right bits; a later launch refuses the handles
        bottom, upper = ctx.register_blend_mask(bottom_mask), ctx.register_blend_mask(upper_mask)
        batch = batch_of(bottom, upper)
        batch.launch(handles[first], times)
        ctx.unregister_blend_mask(bottom)
        ctx.unregister_blend_mask(upper)
        assert helpers.exact(batch.result(), batch.expected(rows))
        assert ctx.rejected_instance_count() == 0
        later = batch_of(bottom, upper)
        assert helpers.exact(later.launch(handles[first], times).result(), later.expected([None] * n))
        assert ctx.rejected_instance_count() == n

        # a captured graph replays correctly after other masks came and went (the table never moves)
        bottom, upper = ctx.register_blend_mask(bottom_mask), ctx.register_blend_mask(upper_mask)
        batch = batch_of(bottom, upper)
        d_clips, d_times = batch.up(handles[first], np.uint32), batch.up(times, np.float32)
        buffer = torch.full((n + 2, batch.row_floats), float(SENTINEL), dtype=torch.float32, device=batch.device)
        side = torch.cuda.Stream(device=batch.device)
        side.wait_stream(torch.cuda.current_stream(batch.device))
        with torch.cuda.stream(side):
            ctx.decompress_poses_batch_masked(d_clips, d_times, n, buffer[1].data_ptr(), batch.row_floats * 4, batch.consumers, batch.mapping, batch.masking, stream=side.cuda_stream)   # warm-up
            side.synchronize()
            graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graph, stream=side):
                ctx.decompress_poses_batch_masked(d_clips, d_times, n, buffer[1].data_ptr(), batch.row_floats * 4, batch.consumers, batch.mapping, batch.masking, stream=side.cuda_stream)
        assert helpers.exact(buffer.cpu().numpy(), batch.expected(rows))
        coming_and_going = [ctx.register_blend_mask(rng.uniform(0.0, 1.0, size=20 + k).astype(np.float32)) for k in range(9)]
        for handle in coming_and_going[::2]:
            ctx.unregister_blend_mask(handle)
        more = [ctx.register_blend_mask(np.ones(num_bones, dtype=np.float32)) for _ in range(3)]
        assert bottom not in more and upper not in more
        buffer.fill_(float(SENTINEL))
        graph.replay()
        torch.cuda.synchronize()
        assert helpers.exact(buffer.cpu().numpy(), batch.expected(rows))
        assert ctx.rejected_instance_count() == n
        del graph


def test_full_size_three_layer_blend_in_object_space_every_instance():
    """65 536 instances, each three differently shaped clips layered in a 128-bone skeleton, object space: every pose against the oracle. The
    masks hold a few plateaus (0, 1 and values between) so that an instance has a handful of distinct weight tuples."""
    rng = np.random.default_rng(155)
    num_bones, n, num_blend = 128, 65536, 3
    clips, tables = sk.blend_rig(rng, num_bones, shapes=("characters_100", "scaled_37", "small_12"))
    reference, parents = sk.reference_pose(rng, num_bones), np.array(synth.humanoid_hierarchy(num_bones), dtype=np.uint32)
    masks = []
    for index in range(4):
        mask = np.zeros(num_bones, dtype=np.float32)
        edges = [0, 16 + 8 * index, 48 + 4 * index, 80, 112 - 8 * index, num_bones]
        for (begin, end), value in zip(zip(edges[:-1], edges[1:]), np.roll(np.array([0.0, 1.0, 0.375, 1.0, 0.0625 * (index + 1)], dtype=np.float32), index)):
            mask[begin:end] = value
        masks.append(mask)
    with runtime.Context(0) as ctx:
        handles = np.array([ctx.register_clip(c.blob) for c in clips], dtype=np.uint32)
        maps = np.array([ctx.register_track_map(t, num_bones) for t in tables], dtype=np.uint32)
        skeleton = ctx.register_skeleton(parents, reference)
        mask_handles = np.array([0] + [ctx.register_blend_mask(m) for m in masks], dtype=np.uint32)
        mask_table = np.stack([np.ones(num_bones, dtype=np.float32)] + masks)            # (row 0: the null handle, every slot 1 -- w * 1 is w)
        member = np.stack([rng.permutation(3) for _ in range(n)])
        times = np.stack([rng.uniform(0.0, clips[k].duration, size=n) for k in range(3)], axis=1).astype(np.float32)
        member_times = np.take_along_axis(times, member, axis=1)
        weights = rng.uniform(0.0, 1.0, size=(n, num_blend)).astype(np.float32)
        weights[:, 0] = 1.0
        which_mask = rng.integers(0, 5, size=(n, num_blend))
        which_mask[:, 0] = 0                                                             # e_0 == 1
        batch = MaskedBatch(ctx, n, num_bones, pad_floats=0)
        consumers, mapping = batch.consumers, batch.mapping
        consumers.object_space, consumers.num_blend_clips = 1, num_blend
        consumers.blend_clips, consumers.blend_sample_times, consumers.blend_weights = batch.up(handles[member[:, 1:]], np.uint32), batch.up(member_times[:, 1:], np.float32), batch.up(weights, np.float32)
        mapping.skeleton, mapping.instance_maps, mapping.blend_maps = skeleton, batch.up(maps[member[:, 0]], np.uint32), batch.up(maps[member[:, 1:]], np.uint32)
        batch.masking.mode, batch.masking.instance_masks = LAYERED, batch.up(mask_handles[which_mask], np.uint32)
        got = batch.launch(handles[member[:, 0]], member_times[:, 0]).result()
        assert ctx.rejected_instance_count() == 0

        skeleton_poses = np.empty((num_blend, n, num_bones, 12), dtype=np.float32)
        blobs = [c.blob for c in clips]
        for k in range(num_blend):
            decoded = ob.oracle_decompress_tracks_batch(blobs, member[:, k], member_times[:, k], 100, threads=16)
            skeleton_poses[k] = reference
            for c in range(3):
                rows_of_clip = np.flatnonzero(member[:, k] == c)
                mapped = tables[c] != DROPPED
                skeleton_poses[k][np.ix_(rows_of_clip, tables[c][mapped])] = decoded[rows_of_clip][:, np.flatnonzero(mapped)]
            del decoded

        def finish(i):
            per_slot = slot_weights(weights[i], [None if m == 0 else mask_table[m] for m in which_mask[i]], LAYERED, num_bones)
            local = masked_blend([skeleton_poses[k, i] for k in range(num_blend)], per_slot)
            return ob.oracle_local_to_object_space(parents, local)

        poses = got[1:1 + n].reshape(n, num_bones, 12)
        with concurrent.futures.ThreadPoolExecutor(max_workers=16) as pool:
            for i, expected in enumerate(pool.map(finish, range(n), chunksize=512)):
                assert np.isfinite(expected).all(), i
                assert helpers.exact(poses[i], expected), i
        assert np.all(got[0] == SENTINEL) and np.all(got[-1] == SENTINEL)


def test_a_mirrored_skeleton_in_object_space_is_counted_and_exact():
    rng = np.random.default_rng(156)
    num_bones = 64
    clip, partner = synth.build_clip(seed=993, **sk.SHAPES["scaled_37"]), synth.build_clip(seed=994, **sk.SHAPES["small_12"])
    reference, parents = sk.reference_pose(rng, num_bones), sk.hierarchy(rng, num_bones)
    table, partner_table = sk.make_map(rng, 37, num_bones, "permutation"), sk.make_map(rng, 12, num_bones, "ordered")
    unmapped = np.setdiff1d(np.arange(num_bones), np.concatenate([table, partner_table]))
    reference[unmapped[:5], 9] *= -1.0                                                   # mirrored bones no track overwrites
    bottom_mask, upper_mask = make_masks(rng, num_bones, 1, floor=0.25)[0], make_masks(rng, num_bones, 1)[0]
    with runtime.Context(0) as ctx:
        handle, h_partner = ctx.register_clip(clip.blob), ctx.register_clip(partner.blob)
        track_map, m_partner = ctx.register_track_map(table, num_bones), ctx.register_track_map(partner_table, num_bones)
        skeleton = ctx.register_skeleton(parents, reference)
        assert ctx.skeleton_info(skeleton).has_negative_scale == 1
        bottom, upper, ones = ctx.register_blend_mask(bottom_mask), ctx.register_blend_mask(upper_mask), ctx.register_blend_mask(np.ones(num_bones, dtype=np.float32))
        n = 19
        times = rng.uniform(0.0, clip.duration, size=n).astype(np.float32)
        partner_times = rng.uniform(0.0, partner.duration, size=n).astype(np.float32)
        for mode, bottom_handle, bottom_values in ((WEIGHTED, bottom, bottom_mask), (LAYERED, ones, None)):
            weights = rng.dirichlet(np.ones(2), size=n).astype(np.float32)
            if mode == LAYERED:
                weights[:, 0] = 1.0
            before = ctx.negative_scale_count()
            batch = MaskedBatch(ctx, n, num_bones)
            batch.consumers.object_space, batch.consumers.num_blend_clips = 1, 2
            batch.consumers.blend_clips, batch.consumers.blend_sample_times, batch.consumers.blend_weights = batch.up(np.full(n, h_partner), np.uint32), batch.up(partner_times, np.float32), batch.up(weights, np.float32)
            batch.mapping.skeleton, batch.mapping.map, batch.mapping.blend_maps = skeleton, track_map, batch.up(np.full(n, m_partner), np.uint32)
            batch.masking.mode, batch.masking.instance_masks = mode, batch.up(np.tile(np.array([bottom_handle, upper]), (n, 1)), np.uint32)
            got = batch.launch(np.full(n, handle), times).result()
            rows = [expected_masked_pose((reference, parents), [(clip.blob, times[i], table), (partner.blob, partner_times[i], partner_table)], weights[i],
                                         [bottom_values, upper_mask], mode, NONE, None, True, 0, 2) for i in range(n)]
            assert np.isfinite(np.stack(rows)).all()
            assert helpers.exact(got, batch.expected(rows)), mode
            assert ctx.negative_scale_count() > before
        assert ctx.rejected_instance_count() == 0
