"""Additive strength (aclhip_additive_layering, aclhip_decompress_poses_batch_additive_weighted) through the C ABI: the mapped launch with a
strength per (instance, slot) on the additive pose. The expected rows are built from the oracle's pieces in the order include/aclhip.h
defines: sk.skeleton_pose per clip, ob.oracle_blend_poses for K > 1, the two pose blend of the additive identity and the additive pose with
weights (1 - e, e) through test_gpu_blend_masks.masked_blend -- the rows where e == 1 taken from the additive pose --, then
oracle_apply_additive_to_base and oracle_local_to_object_space. Compared bit for bit over the whole sentinel filled buffer with its guard
rows. 37 instances (no multiple of a workgroup's 4 / 8); a 30 bone skeleton (90 quads: two lane passes) with two roots under a 17 track
additive clip in permuted order with a dropped track and a 22 track base clip; a 130 bone skeleton under a 120 track clip (two pose
windows). Needs a GPU."""
import functools

import numpy as np
import pytest

from acl_amd import runtime, synth
from oracle import bindings as ob
import helpers
import test_gpu_skeleton_poses as sk
import test_gpu_blend_masks as bm

pytestmark = pytest.mark.gpu

DROPPED, SENTINEL = sk.DROPPED, sk.SENTINEL
NONE, RELATIVE, ADDITIVE0, ADDITIVE1 = sk.NONE, sk.RELATIVE, sk.ADDITIVE0, sk.ADDITIVE1
ONE = np.float32(1.0)
N = 37
SUBNORMAL = np.float32(1.0e-40)


def strength_of(weight, mask, num_bones):
    """the definition's e: w, or w * mask[s]; float32 [B]"""
    if mask is None:
        return np.full(num_bones, np.float32(weight), dtype=np.float32)
    strength = np.float32(weight) * np.asarray(mask, dtype=np.float32)
    assert strength.dtype == np.float32
    return strength


def weighted_additive(additive_pose, strength, additive_format):
    """A -> A': the oracle's blend of (I, A) with weights (1 - e, e), A itself where e == 1"""
    identity = sk.additive_identity(additive_pose.shape[0], additive_format)
    out = bm.masked_blend([identity, additive_pose], np.stack([ONE - strength, strength]))
    full = strength == ONE
    out[full] = additive_pose[full]
    return out


def expected_row(skeleton, clips, blend_weights, strength, additive_format, base, object_space, rounding=0, looping=2):
    """sk.expected_pose with the strength on the additive pose. strength None: the mapped launch's row"""
    reference, parents = skeleton
    options = ob.default_options(looping_policy=looping)
    fill = sk.additive_identity(reference.shape[0], additive_format)
    poses = [sk.skeleton_pose(blob, time, table, fill, rounding, options) for blob, time, table in clips]
    pose = poses[0] if len(poses) == 1 else ob.oracle_blend_poses(poses, blend_weights)
    if strength is not None:
        pose = weighted_additive(pose, strength, additive_format)
    base_pose = base if isinstance(base, np.ndarray) else sk.skeleton_pose(base[0], base[1], base[2], reference, rounding, options)
    pose = ob.oracle_apply_additive_to_base(additive_format, base_pose, pose)
    if object_space:
        pose = ob.oracle_local_to_object_space(parents, pose)
    assert np.isfinite(pose).all()
    return pose


class WeightedBatch(sk.Batch):
    """sk.Batch through aclhip_decompress_poses_batch_additive_weighted; launch_mapped is the same batch through the mapped launch"""

    def __init__(self, ctx, num_instances, num_bones, pad_floats=4):
        super().__init__(ctx, num_instances, num_bones, pad_floats)
        self.layering = runtime.AdditiveLayering()

    def launch(self, clips, times, params=None, buffer=None):
        torch = self.torch
        if buffer is None:
            buffer = torch.full((self.n + 2, self.row_floats), float(SENTINEL), dtype=torch.float32, device=self.device)
        stream = torch.cuda.current_stream(self.device)
        self.ctx.decompress_poses_batch_additive_weighted(self.up(clips, np.uint32), self.up(times, np.float32), self.n, buffer[1].data_ptr(), self.row_floats * 4,
                                                          self.consumers, self.mapping, self.layering, params=params, stream=stream.cuda_stream)
        self.buffer = buffer
        return self

    def launch_mapped(self, clips, times, params=None):
        return sk.Batch.launch(self, clips, times, params=params)


@functools.lru_cache(maxsize=None)
def rig(num_bones=30, mirrored=False):
    """The small skeleton and its clips, built once: (reference, parents), additive clips and tables (17 tracks permuted with a dropped track;
    12 tracks, the blend partner), the base clip and its table (22 tracks), masks"""
    rng = np.random.default_rng(4100 + num_bones + int(mirrored))
    reference, parents = sk.reference_pose(rng, num_bones), sk.hierarchy(rng, num_bones)
    parents[num_bones // 3 + 1] = runtime.NO_PARENT                                       # a second root
    if num_bones == 30:
        additive = synth.build_clip(seed=4001, num_tracks=17, num_samples=33, has_scale=1, scale_default=0.3)
        base = synth.build_clip(seed=4003, num_tracks=22, num_samples=40, has_scale=1, scale_default=0.4)
    else:
        additive = synth.build_clip(seed=4004, num_tracks=120, num_samples=20, has_scale=1, scale_default=0.5)
        base = synth.build_clip(seed=4005, **sk.SHAPES["characters_100"])
    partner = synth.build_clip(seed=4002, **sk.SHAPES["small_12"])
    additive_table = sk.make_map(rng, additive.num_tracks, num_bones, "permutation")
    additive_table[int(np.flatnonzero(additive_table != DROPPED)[3])] = DROPPED             # one dropped track: its slot takes the identity
    partner_table = sk.make_map(rng, 12, num_bones, "ordered")
    base_table = sk.make_map(rng, base.num_tracks, num_bones, "permutation")
    if mirrored:
        unmapped = np.setdiff1d(np.arange(num_bones), base_table[base_table != DROPPED])
        assert unmapped.size >= 3
        reference[unmapped[:3], 9] *= -1.0                                               # mirrored bones the base clip leaves to the reference pose
    masks = bm.make_masks(rng, num_bones, 3)
    assert all((m == 1).any() and (m == 0).any() and ((m > 0) & (m < 1)).any() for m in masks)
    return (reference, parents), (additive, additive_table), (partner, partner_table), (base, base_table), masks


def instance_weights(rng, n=N):
    weights = rng.uniform(0.0, 1.0, size=n).astype(np.float32)
    weights[:6] = [0.0, 1.0, 0.37, SUBNORMAL, 1.0, 0.0]
    assert weights[3] != 0 and weights[3] < np.finfo(np.float32).tiny
    return weights


class Scene:
    """one context with the rig registered, a batch of N instances and their layering"""

    def __init__(self, ctx, num_bones=30, mirrored=False, seed=0):
        self.ctx, self.num_bones = ctx, num_bones
        self.skeleton_pose, (self.additive, self.additive_table), (self.partner, self.partner_table), (self.base, self.base_table), self.masks = rig(num_bones, mirrored)
        self.rng = rng = np.random.default_rng(4200 + seed)
        self.h_additive, self.h_partner, self.h_base = (ctx.register_clip(c.blob) for c in (self.additive, self.partner, self.base))
        self.m_additive, self.m_partner, self.m_base = (ctx.register_track_map(t, num_bones) for t in (self.additive_table, self.partner_table, self.base_table))
        self.skeleton = ctx.register_skeleton(self.skeleton_pose[1], self.skeleton_pose[0])
        self.mask_handles = [ctx.register_blend_mask(m) for m in self.masks]
        self.mask_of = {0: None}
        self.mask_of.update(zip(self.mask_handles, self.masks))
        self.times = rng.uniform(0.0, self.additive.duration, size=N).astype(np.float32)
        self.partner_times = rng.uniform(0.0, self.partner.duration, size=N).astype(np.float32)
        self.base_times = rng.uniform(0.0, self.base.duration, size=N).astype(np.float32)
        self.base_buffer = np.stack([sk.reference_pose(rng, num_bones) for _ in range(N)])
        self.blend_weights = rng.dirichlet(np.ones(2), size=N).astype(np.float32)
        self.weights = instance_weights(rng)
        self.handles = rng.choice([0] + self.mask_handles, size=N).astype(np.uint32)       # handle 0 mixed in
        self.handles[:6] = [0, self.mask_handles[0], 0, self.mask_handles[1], 0, self.mask_handles[2]]

    def batch(self, additive_format, base_as_buffer, object_space, num_blend=1, weights="own", handles="own", pad_floats=4):
        batch = WeightedBatch(self.ctx, N, self.num_bones, pad_floats)
        consumers, mapping = batch.consumers, batch.mapping
        consumers.additive_format, consumers.object_space = additive_format, int(object_space)
        mapping.skeleton, mapping.map = self.skeleton, self.m_additive
        if num_blend == 2:
            consumers.num_blend_clips = 2
            consumers.blend_clips, consumers.blend_sample_times, consumers.blend_weights = batch.up(np.full(N, self.h_partner), np.uint32), batch.up(self.partner_times, np.float32), batch.up(self.blend_weights, np.float32)
            mapping.blend_maps = batch.up(np.full(N, self.m_partner), np.uint32)
        if base_as_buffer:
            consumers.base_poses, consumers.base_pose_stride_bytes = batch.up(self.base_buffer, np.float32), self.num_bones * 48
        else:
            consumers.base_clips, consumers.base_sample_times, mapping.base_maps = batch.up(np.full(N, self.h_base), np.uint32), batch.up(self.base_times, np.float32), batch.up(np.full(N, self.m_base), np.uint32)
        weights = self.weights if isinstance(weights, str) else weights
        handles = self.handles if isinstance(handles, str) else handles
        batch.layering.instance_weights = batch.up(weights, np.float32) if weights is not None else None
        batch.layering.instance_masks = batch.up(handles, np.uint32) if handles is not None else None
        return batch

    def clips(self):
        return np.full(N, self.h_additive, dtype=np.uint32)

    def row(self, i, additive_format, base_as_buffer, object_space, num_blend=1, strength="own"):
        members = [(self.additive.blob, self.times[i], self.additive_table)]
        if num_blend == 2:
            members.append((self.partner.blob, self.partner_times[i], self.partner_table))
        if isinstance(strength, str):
            strength = strength_of(self.weights[i], self.mask_of[int(self.handles[i])], self.num_bones)
        base = self.base_buffer[i] if base_as_buffer else (self.base.blob, self.base_times[i], self.base_table)
        return expected_row(self.skeleton_pose, members, self.blend_weights[i], strength, additive_format, base, object_space)

    def rows(self, *args, **kwargs):
        return [self.row(i, *args, **kwargs) for i in range(N)]


@pytest.mark.parametrize("object_space", [False, True])
@pytest.mark.parametrize("base_as_buffer", [False, True])
@pytest.mark.parametrize("additive_format", [RELATIVE, ADDITIVE0, ADDITIVE1])
def test_every_additive_format_base_and_space(additive_format, base_as_buffer, object_space):
    with runtime.Context(0) as ctx:
        scene = Scene(ctx, seed=additive_format * 4 + base_as_buffer * 2 + object_space)
        batch = scene.batch(additive_format, base_as_buffer, object_space, pad_floats=0 if object_space else 4)
        got = batch.launch(scene.clips(), scene.times).result()
        assert helpers.exact(got, batch.expected(scene.rows(additive_format, base_as_buffer, object_space)))
        assert ctx.rejected_instance_count() == 0


@pytest.mark.parametrize("additive_format,base_as_buffer", [(ADDITIVE0, False), (RELATIVE, False), (RELATIVE, True)])
def test_a_blend_of_two_additive_clips_in_object_space(additive_format, base_as_buffer):
    with runtime.Context(0) as ctx:
        scene = Scene(ctx, seed=20 + additive_format + base_as_buffer)
        batch = scene.batch(additive_format, base_as_buffer, True, num_blend=2)
        got = batch.launch(scene.clips(), scene.times).result()
        assert helpers.exact(got, batch.expected(scene.rows(additive_format, base_as_buffer, True, num_blend=2)))
        assert ctx.rejected_instance_count() == 0


def test_a_130_bone_skeleton_under_a_120_track_clip():
    with runtime.Context(0) as ctx:
        scene = Scene(ctx, num_bones=130, seed=30)
        batch = scene.batch(ADDITIVE1, False, True)
        got = batch.launch(scene.clips(), scene.times).result()
        assert helpers.exact(got, batch.expected(scene.rows(ADDITIVE1, False, True)))
        assert ctx.rejected_instance_count() == 0


def test_full_strength_has_the_bits_of_the_mapped_launch():
    with runtime.Context(0) as ctx:
        scene = Scene(ctx, seed=40)
        ones_mask = ctx.register_blend_mask(np.ones(scene.num_bones, dtype=np.float32))
        ones = np.ones(N, dtype=np.float32)
        for additive_format, base_as_buffer, object_space, num_blend in ((ADDITIVE1, False, True, 1), (ADDITIVE0, False, False, 1), (RELATIVE, False, True, 1),
                                                                          (ADDITIVE0, True, False, 1), (RELATIVE, True, True, 2), (ADDITIVE1, False, True, 2)):
            mapped = scene.batch(additive_format, base_as_buffer, object_space, num_blend).launch_mapped(scene.clips(), scene.times).result()
            assert not np.all(mapped[1:1 + N] == SENTINEL)
            # weights all 1 with null masks (no array, handle 0) and with all-ones masks; the all-ones masks alone
            for weights, handles in ((ones, None), (ones, np.zeros(N)), (ones, np.full(N, ones_mask)), (None, np.full(N, ones_mask))):
                batch = scene.batch(additive_format, base_as_buffer, object_space, num_blend, weights=weights, handles=handles)
                assert helpers.exact(batch.launch(scene.clips(), scene.times).result(), mapped), (additive_format, base_as_buffer, object_space, num_blend)
        assert ctx.rejected_instance_count() == 0


def test_zero_strength_is_the_identity_and_an_upper_body_mask_leaves_the_legs_alone():
    with runtime.Context(0) as ctx:
        scene = Scene(ctx, seed=50)
        num_bones = scene.num_bones
        legs = np.arange(num_bones - 10, num_bones)
        animated = scene.additive_table[scene.additive_table != DROPPED]
        upper = np.setdiff1d(animated, legs)                                            # slots the additive clip animates, outside the legs
        assert np.intersect1d(animated, legs).size > 0 and upper.size > 0
        upper_body = np.ones(num_bones, dtype=np.float32)
        upper_body[legs] = 0.0
        mask = ctx.register_blend_mask(upper_body)
        weights = np.full(N, 0.4, dtype=np.float32)
        weights[0] = 0.0                                                                # ... and an instance at strength 0 without a mask
        handles = np.full(N, mask, dtype=np.uint32)
        handles[0] = 0
        for additive_format, base_as_buffer in ((ADDITIVE1, False), (RELATIVE, False), (ADDITIVE0, True)):
            batch = scene.batch(additive_format, base_as_buffer, False, weights=weights, handles=handles)
            got = batch.launch(scene.clips(), scene.times).result()
            strengths = [strength_of(weights[i], None if handles[i] == 0 else upper_body, num_bones) for i in range(N)]
            assert helpers.exact(got, batch.expected([scene.row(i, additive_format, base_as_buffer, False, strength=strengths[i]) for i in range(N)]))
            poses = got[1:1 + N, : num_bones * 12].reshape(N, num_bones, 12)
            zero = np.stack([scene.row(i, additive_format, base_as_buffer, False, strength=np.zeros(num_bones, dtype=np.float32)) for i in range(N)])
            full = np.stack([scene.row(i, additive_format, base_as_buffer, False, strength=None) for i in range(N)])
            identity = sk.additive_identity(num_bones, additive_format)
            options = ob.default_options()
            for i in range(N):
                base = scene.base_buffer[i] if base_as_buffer else sk.skeleton_pose(scene.base.blob, scene.base_times[i], scene.base_table, scene.skeleton_pose[0], 0, options)
                applied = ob.oracle_apply_additive_to_base(additive_format, base, identity)   # the oracle's apply of the identity additive
                assert helpers.exact(zero[i], applied), i
                assert helpers.exact(poses[i, legs], applied[legs]), i
                if i != 0:
                    assert not np.array_equal(poses[i, upper], full[i, upper]) and not np.array_equal(poses[i, upper], zero[i, upper]), i
            assert helpers.exact(poses[0], zero[0])
        assert ctx.rejected_instance_count() == 0


def test_a_mirrored_skeleton_with_the_relative_format_in_object_space_is_counted_and_exact():
    with runtime.Context(0) as ctx:
        scene = Scene(ctx, mirrored=True, seed=60)
        assert ctx.skeleton_info(scene.skeleton).has_negative_scale == 1
        before = ctx.negative_scale_count()
        batch = scene.batch(RELATIVE, False, True)
        got = batch.launch(scene.clips(), scene.times).result()
        assert helpers.exact(got, batch.expected(scene.rows(RELATIVE, False, True)))
        assert ctx.negative_scale_count() > before
        assert ctx.rejected_instance_count() == 0


def test_refusals_inside_an_otherwise_valid_batch():
    import torch
    with runtime.Context(0) as ctx:
        scene = Scene(ctx, seed=70)
        other_size = ctx.register_blend_mask(np.ones(scene.num_bones + 1, dtype=np.float32))
        retired = ctx.register_blend_mask(scene.masks[0])                                  # (the last one registered: nothing below reuses its handle)
        ctx.unregister_blend_mask(retired)
        torch.cuda.synchronize()
        refused = {5: 0xFFFFFFFF, 6: runtime.MAX_BLEND_MASKS, 11: retired, 12: other_size, 36: runtime.MAX_BLEND_MASKS + 9}
        for additive_format, base_as_buffer, object_space in ((ADDITIVE1, False, True), (RELATIVE, False, False), (ADDITIVE0, True, True)):
            handles = scene.handles.copy()
            for i, handle in refused.items():
                handles[i] = handle
            before = ctx.rejected_instance_count()
            batch = scene.batch(additive_format, base_as_buffer, object_space, handles=handles)
            got = batch.launch(scene.clips(), scene.times).result()
            rows = [None if i in refused else scene.row(i, additive_format, base_as_buffer, object_space) for i in range(N)]
            assert helpers.exact(got, batch.expected(rows))                                # refused rows and the guard rows keep the sentinel, the neighbours are bit exact
            assert ctx.rejected_instance_count() - before == len(refused)
        # host side: ACLHIP_ERROR_INVALID_ARGUMENT, nothing launched
        before = ctx.rejected_instance_count()
        for spoil in ("layering", "both arrays", "reserved", "no additive format", "mapping"):
            batch = scene.batch(ADDITIVE1, False, True)
            if spoil == "layering":
                batch.layering = None
            if spoil == "both arrays":
                batch.layering.instance_weights, batch.layering.instance_masks = None, None
            if spoil == "reserved":
                batch.layering.reserved[0] = 1
            if spoil == "no additive format":
                batch.consumers.additive_format = NONE
            if spoil == "mapping":
                batch.mapping = None
            with pytest.raises(runtime.AclHipError) as error:
                batch.launch(scene.clips(), scene.times)
            assert error.value.status == runtime.ERROR_INVALID_ARGUMENT, spoil
        torch.cuda.synchronize()
        assert ctx.rejected_instance_count() == before


def test_lifetime_unregister_behind_a_launch_and_graph_replay():
    import torch
    with runtime.Context(0) as ctx:
        scene = Scene(ctx, seed=80)
        rows = None

        def batch_of(mask):
            handles = np.full(N, mask, dtype=np.uint32)
            handles[::5] = 0
            return scene.batch(ADDITIVE1, False, True, handles=handles), handles

        # unregistered right behind the enqueued launch: it still decodes; a later launch refuses the handle
        mask = ctx.register_blend_mask(scene.masks[1])
        batch, handles = batch_of(mask)
        rows = [scene.row(i, ADDITIVE1, False, True, strength=strength_of(scene.weights[i], None if handles[i] == 0 else scene.masks[1], scene.num_bones)) for i in range(N)]
        batch.launch(scene.clips(), scene.times)
        ctx.unregister_blend_mask(mask)
        assert helpers.exact(batch.result(), batch.expected(rows))
        assert ctx.rejected_instance_count() == 0
        later, _ = batch_of(mask)
        gone = int((handles != 0).sum())
        assert helpers.exact(later.launch(scene.clips(), scene.times).result(), later.expected([rows[i] if handles[i] == 0 else None for i in range(N)]))
        assert ctx.rejected_instance_count() == gone

        # a captured graph: right while the mask lives, refused and counted once it is gone
        mask = ctx.register_blend_mask(scene.masks[1])
        batch, handles = batch_of(mask)
        d_clips, d_times = batch.up(scene.clips(), np.uint32), batch.up(scene.times, np.float32)
        buffer = torch.full((N + 2, batch.row_floats), float(SENTINEL), dtype=torch.float32, device=batch.device)
        side = torch.cuda.Stream(device=batch.device)
        side.wait_stream(torch.cuda.current_stream(batch.device))
        launch = lambda: ctx.decompress_poses_batch_additive_weighted(d_clips, d_times, N, buffer[1].data_ptr(), batch.row_floats * 4, batch.consumers, batch.mapping, batch.layering,
                                                                      stream=side.cuda_stream)
        with torch.cuda.stream(side):
            launch()                                                                    # warm-up
            side.synchronize()
            graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graph, stream=side):
                launch()
        buffer.fill_(float(SENTINEL))
        graph.replay()
        torch.cuda.synchronize()
        assert helpers.exact(buffer.cpu().numpy(), batch.expected(rows))
        assert ctx.rejected_instance_count() == gone
        ctx.unregister_blend_mask(mask)
        torch.cuda.synchronize()
        buffer.fill_(float(SENTINEL))
        graph.replay()
        torch.cuda.synchronize()
        assert helpers.exact(buffer.cpu().numpy(), batch.expected([rows[i] if handles[i] == 0 else None for i in range(N)]))
        assert ctx.rejected_instance_count() == 2 * gone
        del graph
