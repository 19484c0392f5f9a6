"""aclhip_blend_poses_batch through the C ABI: the masked blend of K pose buffers the caller filled, in local or object space.
The expected rows are built on the CPU from the oracle's pieces alone: the per slot weights restated in numpy float32 exactly as
include/aclhip.h states them (one operation at a time, the layered product from the top layer down), ob.oracle_blend_poses once per group
of slots with identical weight tuples (the blend is per transform: this is the definition, the method of tests/test_gpu_blend_masks.py),
then ob.oracle_local_to_object_space. Every comparison is on uint32 views, bit for bit, over whole sentinel filled buffers: a guard row
before and behind every buffer, pad floats behind every row, every input buffer a stride of its own. Inputs are finite records with
normalized rotations and NON-ZERO GARBAGE in both pads; some bones of buffer 1 carry the negated rotation of buffer 0. No slot's weights are
all 0 (weighted mode: buffer 0's weight and mask floor are above 0; layered mode: e_0 == 1): expected_local asserts it. Needs a GPU."""
import numpy as np
import pytest

from acl_amd import runtime, synth
from oracle import bindings as ob

pytestmark = pytest.mark.gpu

SENTINEL = np.float32(-7777.25)
WEIGHTED, LAYERED = runtime.BLEND_WEIGHTED, runtime.BLEND_LAYERED
ONE = np.float32(1.0)
INF = np.float32(np.inf)
BONES = [1, 21, 22, 100]     # 3, 63 (just under a pass of 64 quads), 66 (just over), 300 quads (five passes, the last partial; > 64 rotations)
COUNTS = [1, 9, 37]          # 9: one more than a workgroup's eight instances


def bits(array):
    return np.ascontiguousarray(array, dtype=np.float32).view(np.uint32)


def forest(rng, num_bones, root_chance=0.08):
    """a random forest, parents first: several roots, a parent up to nine bones back"""
    parents = np.zeros(num_bones, dtype=np.uint32)
    parents[0] = runtime.NO_PARENT
    for i in range(1, num_bones):
        parents[i] = runtime.NO_PARENT if rng.uniform() < root_chance else rng.integers(max(0, i - 9), i)
    return parents


def identity_pose(num_bones):
    pose = np.zeros((num_bones, 12), dtype=np.float32)
    pose[:, 3] = 1.0
    pose[:, 8:11] = 1.0
    return pose


def random_inputs(rng, num_buffers, n, num_bones, scale=(0.8, 1.25)):
    """K arrays float32 [n, B, 12]: unit rotations, translations within +-10, garbage in both pads; every third bone of buffer 1 is buffer
    0's rotation negated (the same orientation on the other side of the sphere: the sign bias decides)"""
    inputs = []
    for k in range(num_buffers):
        poses = np.zeros((n, num_bones, 12), dtype=np.float32)
        rotations = rng.normal(size=(n, num_bones, 4))
        poses[..., 0:4] = rotations / np.linalg.norm(rotations, axis=2, keepdims=True)
        poses[..., 4:7] = rng.uniform(-10.0, 10.0, size=(n, num_bones, 3))
        poses[..., 8:11] = rng.uniform(scale[0], scale[1], size=(n, num_bones, 3))
        poses[..., 7], poses[..., 11] = 5.5 + k, -6.5 - k
        inputs.append(poses)
    inputs[1][:, ::3, 0:4] = -inputs[0][:, ::3, 0:4]
    return inputs


def slot_weights(weights, masks, mode, num_bones):
    """The header's steps 1 and 2: weights [K], masks K arrays [B] or None (the null handle) -> the weight of buffer k at slot s, float32 [K, B]"""
    num_buffers = len(weights)
    opacity = np.empty((num_buffers, num_bones), dtype=np.float32)
    for k in range(num_buffers):
        opacity[k] = np.float32(weights[k]) if masks[k] is None else np.float32(weights[k]) * np.asarray(masks[k], dtype=np.float32)
    if mode == WEIGHTED:
        return opacity
    layered = np.empty_like(opacity)
    for k in range(num_buffers):
        rest = np.ones(num_bones, dtype=np.float32)
        for j in range(num_buffers - 1, k, -1):
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
        out[slots] = ob.oracle_blend_poses([np.ascontiguousarray(pose[slots]) for pose in poses], np.ascontiguousarray(tuples[index]).view(np.float32))
    return out


def expected_local(poses, weights, masks, mode):
    """poses: K arrays [B, 12] of one instance"""
    per_slot = slot_weights(weights, masks, mode, poses[0].shape[0])
    assert (per_slot != 0).any(axis=0).all()                 # the condition on the inputs: no slot whose weights are all 0
    row = masked_blend(poses, per_slot)
    assert np.isfinite(row).all()
    return row


def walked(parents, row):
    out = ob.oracle_local_to_object_space(parents, row)
    assert np.isfinite(out).all()
    return out


def make_masks(rng, num_bones, count, floor=0.0):
    """a few plateaus per mask -- 0 (without a floor), 1 and values between -- so that an instance has a handful of distinct weight tuples,
    plus single slots of their own"""
    masks = []
    for _ in range(count):
        mask = np.empty(num_bones, dtype=np.float32)
        edges = np.concatenate([[0], np.sort(rng.integers(0, num_bones + 1, size=4)), [num_bones]])
        values = rng.permutation(np.array([floor, 1.0, 0.375, 1.0, max(floor, 0.0625)], dtype=np.float32))
        for (begin, end), value in zip(zip(edges[:-1], edges[1:]), values):
            mask[begin:end] = value
        for slot in rng.integers(0, num_bones, size=min(3, num_bones)):
            mask[slot] = np.float32(rng.uniform(max(floor, 0.01), 1.0))
        masks.append(mask)
    return masks


def blend_weights(rng, mode, n, num_buffers):
    if mode == WEIGHTED:
        return (rng.dirichlet(np.ones(num_buffers), size=n) * 0.98 + 0.02 / num_buffers).astype(np.float32)    # (strictly positive: buffer 0 carries every slot)
    weights = rng.uniform(0.0, 1.0, size=(n, num_buffers)).astype(np.float32)
    weights[:, 0] = 1.0                                                                # e_0 == 1: the bottom layer is opaque
    weights[0, 1:] = 1.0                                                               # opaque layers above
    if n > 1:
        weights[1, 1:] = 0.0                                                           # transparent layers above
    return weights


class MaskSet:
    """the masks of one skeleton in one context: handle -> values (None for the null handle), and handles to draw from per layer"""

    def __init__(self, ctx, rng, num_bones, mode):
        bottom = make_masks(rng, num_bones, 2, floor=0.25) if mode == WEIGHTED else [np.ones(num_bones, dtype=np.float32)]
        upper = make_masks(rng, num_bones, 3)
        self.values = {0: None}
        self.bottom, self.upper = [0], [0]
        for group, masks in ((self.bottom, bottom), (self.upper, upper)):
            for mask in masks:
                handle = ctx.register_blend_mask(mask)
                group.append(handle)
                self.values[handle] = mask

    def draw(self, rng, n, num_buffers):
        """uint32 [n, K]: some null handles in every column; instance 2 of a larger batch has no mask above the bottom"""
        handles = np.empty((n, num_buffers), dtype=np.uint32)
        handles[:, 0] = rng.choice(self.bottom, size=n)
        handles[:, 1:] = rng.choice(self.upper, size=(n, num_buffers - 1))
        if n > 2:
            handles[2, 1:] = 0
        return handles


class Buffers:
    """The device buffers of one batch, each [n + 2, row floats], sentinel filled, with a guard row before and behind its n rows"""

    def __init__(self, n):
        import torch
        self.torch, self.n = torch, n
        self.device = torch.device("cuda:0")
        self.keep = []

    def host(self, row_floats, rows=None):
        """rows: per instance a pose [B_i, 12] or None (the row stays the sentinel)"""
        out = np.full((self.n + 2, row_floats), SENTINEL, dtype=np.float32)
        for i, pose in enumerate(rows if rows is not None else ()):
            if pose is not None:
                out[1 + i, : pose.size] = np.asarray(pose, dtype=np.float32).reshape(-1)
        return out

    def up(self, array):
        array = np.ascontiguousarray(array)
        tensor = self.torch.from_numpy(array.view(np.int32) if array.dtype == np.uint32 else array).to(self.device)
        self.keep.append(tensor)
        return tensor

    def stream(self):
        return self.torch.cuda.current_stream(self.device).cuda_stream

    def down(self, tensor):
        self.torch.cuda.current_stream(self.device).synchronize()
        return tensor.cpu().numpy()


class Launch:
    """One aclhip_blend_poses_batch. inputs: K lists (or arrays) of per instance poses [B_i, 12]. Buffer k's rows are row_bones[k] * 12 +
    4 * (k + 2) floats wide -- every buffer a stride of its own, each larger than B * 48 --, the output's row_bones * 12 + 4.
    in_place: None, or the buffer the output is. bounds_flags: "none" (no bounds), None (every bone counts) or uint8 flags."""

    def __init__(self, ctx, inputs, weights, mode, handles=None, skeleton=0, instance_skeletons=None, object_space=False, in_place=None, bounds_flags="none",
                 with_rows=True, row_bones=None, out_bones=None):
        num_buffers, n = len(inputs), len(inputs[0])
        largest = max(pose.shape[0] for pose in inputs[0])
        row_bones = row_bones if row_bones is not None else [largest] * num_buffers
        self.buffers = buffers = Buffers(n)
        self.n, self.in_place = n, in_place
        self.input_floats = [row_bones[k] * 12 + 4 * (k + 2) for k in range(num_buffers)]
        self.out_floats = self.input_floats[in_place] if in_place is not None else (out_bones if out_bones is not None else largest) * 12 + 4
        self.h_inputs = [buffers.host(self.input_floats[k], inputs[k]) for k in range(num_buffers)]
        self.d_inputs = [buffers.up(h) for h in self.h_inputs]
        self.d_out = self.d_inputs[in_place] if in_place is not None else buffers.up(buffers.host(self.out_floats))
        self.d_weights = buffers.up(np.ascontiguousarray(weights, dtype=np.float32))
        self.blend = blend = runtime.PoseBufferBlend()
        blend.skeleton, blend.num_buffers, blend.mode, blend.object_space = skeleton, num_buffers, mode, 1 if object_space else 0
        for k in range(num_buffers):
            blend.buffers[k], blend.buffer_stride_bytes[k] = self.d_inputs[k][1].data_ptr(), self.input_floats[k] * 4
        blend.weights = self.d_weights.data_ptr()
        if handles is not None:
            blend.instance_masks = buffers.up(np.ascontiguousarray(handles, dtype=np.uint32)).data_ptr()
        if instance_skeletons is not None:
            blend.instance_skeletons = buffers.up(np.asarray(instance_skeletons, dtype=np.uint32)).data_ptr()
        self.bounds, self.d_boxes = None, None
        if not isinstance(bounds_flags, str):
            self.bounds, self.d_boxes = runtime.PoseBounds(), buffers.up(np.full((n + 2, 8), SENTINEL, dtype=np.float32))
            self.bounds.bounds = self.d_boxes[1].data_ptr()
            self.bounds.bone_flags = buffers.up(np.asarray(bounds_flags, dtype=np.uint8)).data_ptr() if bounds_flags is not None else None
        self.poses_ptr = self.d_out[1].data_ptr() if with_rows else None
        self.ctx = ctx

    def enqueue(self, stream=None):
        self.ctx.blend_poses_batch(self.blend, self.n, self.poses_ptr, self.out_floats * 4, bounds=self.bounds, stream=stream if stream is not None else self.buffers.stream())
        return self

    def out(self):
        return self.buffers.down(self.d_out)

    def boxes(self):
        return self.buffers.down(self.d_boxes)

    def expected(self, rows):
        return self.buffers.host(self.out_floats, rows)

    def inputs_unchanged(self):
        return all(np.array_equal(bits(self.buffers.down(d)), bits(h)) for k, (d, h) in enumerate(zip(self.d_inputs, self.h_inputs)) if k != self.in_place)


def check(ctx, inputs, weights, mode, rows, **launch):
    """out of place: the output is `rows` over the whole guarded buffer (row tails and guard rows keep the prefill), every input is unchanged"""
    done = Launch(ctx, inputs, weights, mode, **launch).enqueue()
    out, want = done.out(), done.expected(rows)
    assert np.array_equal(bits(out), bits(want)), np.argwhere(bits(out) != bits(want))[:8]
    assert done.inputs_unchanged()
    return out


# ---- 1. parity ----------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("mode", [WEIGHTED, LAYERED])
@pytest.mark.parametrize("num_buffers", [2, 3, 4])
def test_parity_with_the_oracle(num_buffers, mode):
    """x {no masks, masks with some null handles} x {local, object space} over B in BONES and n in COUNTS; the rows of the 37 instance
    batch are computed once, and the smaller batches are its first instances"""
    rng = np.random.default_rng(7100 + 10 * num_buffers + mode)
    with runtime.Context(0) as ctx:
        for num_bones in BONES:
            parents = forest(rng, num_bones)
            skeleton = ctx.register_skeleton(parents, identity_pose(num_bones))
            masks = MaskSet(ctx, rng, num_bones, mode)
            largest = max(COUNTS)
            inputs = random_inputs(rng, num_buffers, largest, num_bones)
            weights = blend_weights(rng, mode, largest, num_buffers)
            for masked in (False, True):
                handles = masks.draw(rng, largest, num_buffers) if masked else None
                local = [expected_local([inputs[k][i] for k in range(num_buffers)], weights[i],
                                        [masks.values[int(h)] for h in handles[i]] if masked else [None] * num_buffers, mode) for i in range(largest)]
                assert all(np.all(row[:, [7, 11]] == 0.0) for row in local)          # the oracle's blend writes the pads 0
                object_rows = [walked(parents, row) for row in local]
                for n in COUNTS:
                    for object_space, rows in ((False, local), (True, object_rows)):
                        check(ctx, [buffer[:n] for buffer in inputs], weights[:n], mode, rows[:n], handles=handles[:n] if masked else None, skeleton=skeleton,
                              object_space=object_space)
        assert ctx.rejected_instance_count() == 0
        assert ctx.negative_scale_count() == 0


@pytest.mark.parametrize("object_space", [False, True])
def test_rows_beyond_the_default_limit_of_dynamic_lds(object_space):
    """rows of 1400 transforms: an image of 67 216 bytes, more dynamic LDS than a kernel gets without asking (65 408 bytes; BONES ends at
    100) -- one instance per workgroup, 22 passes of 64 quads and a partial one; two buffers, three instances"""
    rng = np.random.default_rng(7150 + int(object_space))
    num_bones, n, num_buffers = 1400, 3, 2
    parents = forest(rng, num_bones)
    inputs, weights = random_inputs(rng, num_buffers, n, num_bones), blend_weights(rng, WEIGHTED, n, num_buffers)
    rows = [expected_local([inputs[k][i] for k in range(num_buffers)], weights[i], [None] * num_buffers, WEIGHTED) for i in range(n)]
    if object_space:
        rows = [walked(parents, row) for row in rows]
    with runtime.Context(0) as ctx:
        skeleton = ctx.register_skeleton(parents, identity_pose(num_bones))
        check(ctx, inputs, weights, WEIGHTED, rows, skeleton=skeleton, object_space=object_space)
        assert ctx.rejected_instance_count() == 0
        assert ctx.negative_scale_count() == 0


# ---- 2. per instance skeletons ------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("mode", [WEIGHTED, LAYERED])
def test_skeletons_per_instance_mixed_inside_a_workgroup(mode):
    rng = np.random.default_rng(7201 + mode)
    small, large, num_buffers = 40, 100, 3
    parents = {small: forest(rng, small, root_chance=0.2), large: forest(rng, large)}
    which = [large, small, small, large, small, large, large, small, large]
    n = len(which)
    inputs = [[random_inputs(rng, 2, 1, bones)[k % 2][0] for bones in which] for k in range(num_buffers)]
    weights = blend_weights(rng, mode, n, num_buffers)
    with runtime.Context(0) as ctx:
        handles = {bones: ctx.register_skeleton(parents[bones], identity_pose(bones)) for bones in (small, large)}
        masks = {bones: MaskSet(ctx, rng, bones, mode) for bones in (small, large)}             # the masks are per skeleton
        mask_handles = np.stack([masks[bones].draw(rng, 4, num_buffers)[3] for bones in which])
        ids = [handles[bones] for bones in which]
        local = [expected_local([inputs[k][i] for k in range(num_buffers)], weights[i], [masks[which[i]].values[int(h)] for h in mask_handles[i]], mode) for i in range(n)]
        out = check(ctx, inputs, weights, mode, local, handles=mask_handles, instance_skeletons=ids)
        assert np.all(out[2, small * 12:] == SENTINEL)               # a row is written up to its own skeleton's B * 48
        rows = [walked(parents[which[i]], local[i]) for i in range(n)]
        check(ctx, inputs, weights, mode, rows, handles=mask_handles, instance_skeletons=ids, object_space=True)
        # a launch wide skeleton is ignored next to the list
        check(ctx, inputs, weights, mode, rows, handles=mask_handles, skeleton=handles[small], instance_skeletons=ids, object_space=True)
        assert ctx.rejected_instance_count() == 0


# ---- 3. in place --------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("object_space", [False, True])
@pytest.mark.parametrize("num_buffers", [2, 4])
def test_in_place_on_the_first_and_on_the_last_buffer(num_buffers, object_space):
    rng = np.random.default_rng(7300 + 2 * num_buffers + int(object_space))
    with runtime.Context(0) as ctx:
        for num_bones, n in ((22, 9), (100, 37)):
            parents = forest(rng, num_bones)
            skeleton = ctx.register_skeleton(parents, identity_pose(num_bones))
            masks = MaskSet(ctx, rng, num_bones, LAYERED)
            inputs, weights, handles = random_inputs(rng, num_buffers, n, num_bones), blend_weights(rng, LAYERED, n, num_buffers), masks.draw(rng, n, num_buffers)
            common = dict(handles=handles, skeleton=skeleton, object_space=object_space)
            apart = Launch(ctx, inputs, weights, LAYERED, **common).enqueue().out()
            assert not np.all(apart[1:1 + n] == SENTINEL)
            for target in (0, num_buffers - 1):
                done = Launch(ctx, inputs, weights, LAYERED, in_place=target, **common).enqueue()
                out = done.out()
                # the same rows, guard rows included (the in place buffer has its own stride: the records and the row tails apart)
                assert np.array_equal(bits(out[:, : num_bones * 12]), bits(apart[:, : num_bones * 12])), target
                assert np.all(out[:, num_bones * 12:] == SENTINEL)
                assert done.inputs_unchanged()                        # the other inputs
        assert ctx.rejected_instance_count() == 0


# ---- 4. agreement with the fused launch ---------------------------------------------------------------------------------------------

@pytest.mark.parametrize("mode", [WEIGHTED, LAYERED])
@pytest.mark.parametrize("num_buffers", [2, 4])
def test_the_blend_of_decoded_buffers_is_the_fused_masked_launch(num_buffers, mode):
    import torch
    rng = np.random.default_rng(7400 + 2 * num_buffers + mode)
    num_bones, n = 100, 37
    clips = [synth.build_clip(seed=7410 + k, num_tracks=num_bones, num_samples=30 + 7 * k, **(dict(has_scale=1, scale_default=0.3) if k == 1 else {})) for k in range(num_buffers)]
    parents = np.array(synth.humanoid_hierarchy(num_bones), dtype=np.uint32)
    reference = identity_pose(num_bones)
    with runtime.Context(0) as ctx:
        clip_handles = [ctx.register_clip(clip.blob) for clip in clips]
        identity_map = ctx.register_track_map(np.arange(num_bones, dtype=np.uint32), num_bones)
        skeleton = ctx.register_skeleton(parents, reference)
        masks = MaskSet(ctx, rng, num_bones, mode)
        handles, weights = masks.draw(rng, n, num_buffers), blend_weights(rng, mode, n, num_buffers)
        buffers = Buffers(n)
        device, stream = buffers.device, buffers.stream()
        times = [rng.uniform(0.0, clip.duration, size=n).astype(np.float32) for clip in clips]
        d_times = [buffers.up(t) for t in times]
        d_clips = [buffers.up(np.full(n, handle, dtype=np.uint32)) for handle in clip_handles]
        row_floats = num_bones * 12 + 4
        # the K buffers: aclhip_decompress_tracks_batch_mapped, one clip each
        decoded = [torch.full((n + 2, row_floats), float(SENTINEL), dtype=torch.float32, device=device) for _ in range(num_buffers)]
        for k in range(num_buffers):
            ctx.decompress_tracks_batch_mapped(d_clips[k], d_times[k], decoded[k][1:], row_floats * 4, track_map=identity_map, stream=stream)
        d_weights, d_handles = buffers.up(weights), buffers.up(handles)
        for object_space in (False, True):
            fused = torch.full((n + 2, row_floats), float(SENTINEL), dtype=torch.float32, device=device)
            consumers, mapping, masking = runtime.PoseConsumers(), runtime.PoseMapping(), runtime.BlendMasking()
            consumers.object_space, consumers.num_blend_clips = int(object_space), num_buffers
            d_partner_clips = buffers.up(np.tile(np.array(clip_handles[1:], dtype=np.uint32), (n, 1)))
            d_partner_times = buffers.up(np.stack(times[1:], axis=1))
            d_partner_maps = buffers.up(np.full((n, num_buffers - 1), identity_map, dtype=np.uint32))
            consumers.blend_clips, consumers.blend_sample_times, consumers.blend_weights = d_partner_clips.data_ptr(), d_partner_times.data_ptr(), d_weights.data_ptr()
            mapping.skeleton, mapping.map, mapping.blend_maps = skeleton, identity_map, d_partner_maps.data_ptr()
            masking.mode, masking.instance_masks = mode, d_handles.data_ptr()
            ctx.decompress_poses_batch_masked(d_clips[0].data_ptr(), d_times[0].data_ptr(), n, fused[1].data_ptr(), row_floats * 4, consumers, mapping, masking, stream=stream)
            blended = torch.full((n + 2, row_floats), float(SENTINEL), dtype=torch.float32, device=device)
            blend = runtime.PoseBufferBlend()
            blend.skeleton, blend.num_buffers, blend.mode, blend.object_space = skeleton, num_buffers, mode, int(object_space)
            for k in range(num_buffers):
                blend.buffers[k], blend.buffer_stride_bytes[k] = decoded[k][1].data_ptr(), row_floats * 4
            blend.weights, blend.instance_masks = d_weights.data_ptr(), d_handles.data_ptr()
            ctx.blend_poses_batch(blend, n, blended[1].data_ptr(), row_floats * 4, stream=stream)
            got, want = buffers.down(blended), buffers.down(fused)
            assert np.isfinite(want[1:1 + n, : num_bones * 12]).all() and not np.all(want[1:1 + n] == SENTINEL)
            assert np.array_equal(bits(got), bits(want)), (object_space, np.argwhere(bits(got) != bits(want))[:8])
        assert ctx.rejected_instance_count() == 0


# ---- 5. identity properties ---------------------------------------------------------------------------------------------------------

def test_a_weight_of_zero_returns_the_other_buffer_and_a_mask_of_ones_changes_nothing():
    rng = np.random.default_rng(7501)
    num_bones, n = 100, 9
    parents = forest(rng, num_bones)
    with runtime.Context(0) as ctx:
        skeleton = ctx.register_skeleton(parents, identity_pose(num_bones))
        inputs = random_inputs(rng, 2, n, num_bones)
        weights = np.tile(np.array([1.0, 0.0], dtype=np.float32), (n, 1))
        out = Launch(ctx, inputs, weights, WEIGHTED, skeleton=skeleton).enqueue().out()
        rows = out[1:1 + n, : num_bones * 12].reshape(n, num_bones, 12)
        for i in range(n):
            normalized = ob.oracle_blend_poses([inputs[0][i]], [1.0])                 # quat_normalize of buffer 0's rotation, per the oracle
            assert np.array_equal(bits(rows[i][:, 0:4]), bits(normalized[:, 0:4])), i
        assert np.array_equal(bits(rows[..., [4, 5, 6, 8, 9, 10]]), bits(inputs[0][..., [4, 5, 6, 8, 9, 10]]))
        assert np.all(rows[..., [7, 11]] == 0.0) and np.all(inputs[0][..., [7, 11]] != 0.0)
        # weighted mode: a mask that is 1 everywhere gives the bits of the launch without masks
        ones = ctx.register_blend_mask(np.ones(num_bones, dtype=np.float32))
        for num_buffers, object_space in ((2, False), (3, True), (4, True)):
            inputs, weights = random_inputs(rng, num_buffers, n, num_bones), blend_weights(rng, WEIGHTED, n, num_buffers)
            plain = Launch(ctx, inputs, weights, WEIGHTED, skeleton=skeleton, object_space=object_space).enqueue().out()
            assert not np.all(plain[1:1 + n] == SENTINEL)
            for handles in (np.full((n, num_buffers), ones), rng.choice([0, ones], size=(n, num_buffers)), np.zeros((n, num_buffers))):
                masked = Launch(ctx, inputs, weights, WEIGHTED, handles=handles, skeleton=skeleton, object_space=object_space).enqueue().out()
                assert np.array_equal(bits(masked), bits(plain)), (num_buffers, object_space)
        assert ctx.rejected_instance_count() == 0


# ---- 6. bounds ----------------------------------------------------------------------------------------------------------------------

def expected_boxes(rows, flags):
    """rows: float32 [n, B, 12] of the launch without bounds. [n + 2, 8] with the guards."""
    n = rows.shape[0]
    out = np.full((n + 2, 8), SENTINEL, dtype=np.float32)
    counted = np.ones(rows.shape[1], dtype=bool) if flags is None else flags != 0
    for i in range(n):
        box = np.zeros(8, dtype=np.float32)
        box[0:3], box[4:7] = INF, -INF
        if counted.any():
            translations = rows[i][counted, 4:7]
            box[0:3], box[4:7] = translations.min(axis=0), translations.max(axis=0)
        out[1 + i] = box
    return out


@pytest.mark.parametrize("num_bones", [22, 100])
def test_bounds_with_rows_and_alone(num_bones):
    rng = np.random.default_rng(7600 + num_bones)
    parents = forest(rng, num_bones)
    n, num_buffers = 9, 3
    with runtime.Context(0) as ctx:
        skeleton = ctx.register_skeleton(parents, identity_pose(num_bones))
        masks = MaskSet(ctx, rng, num_bones, WEIGHTED)
        inputs, weights, handles = random_inputs(rng, num_buffers, n, num_bones), blend_weights(rng, WEIGHTED, n, num_buffers), masks.draw(rng, n, num_buffers)
        common = dict(handles=handles, skeleton=skeleton, object_space=True)
        plain = Launch(ctx, inputs, weights, WEIGHTED, **common).enqueue().out()
        rows = plain[1:1 + n, : num_bones * 12].reshape(n, num_bones, 12)
        assert np.isfinite(rows).all()
        for index, flags in enumerate([None, (np.arange(num_bones) % 2 == 0).astype(np.uint8) * 255, (np.arange(num_bones) % 5 != 1).astype(np.uint8), np.zeros(num_bones, dtype=np.uint8)]):
            want = expected_boxes(rows, flags)
            done = Launch(ctx, inputs, weights, WEIGHTED, bounds_flags=flags, **common).enqueue()
            assert np.array_equal(bits(done.out()), bits(plain)), index                         # rows bit identical with and without bounds
            assert np.array_equal(bits(done.boxes()), bits(want)), (index, done.boxes(), want)
            alone = Launch(ctx, inputs, weights, WEIGHTED, bounds_flags=flags, with_rows=False, **common).enqueue()
            assert np.array_equal(bits(alone.boxes()), bits(want)), (index, "bounds alone")
            assert np.all(alone.out() == SENTINEL), index                                       # no row is written
            assert alone.inputs_unchanged()
        assert ctx.rejected_instance_count() == 0


# ---- 7. a mirrored skeleton ---------------------------------------------------------------------------------------------------------

def test_a_negative_scale_takes_the_matrix_route_and_is_counted():
    rng = np.random.default_rng(7701)
    num_bones, n, num_buffers = 100, 9, 2
    parents = forest(rng, num_bones)
    reference = identity_pose(num_bones)
    reference[5:9, 9] = -1.0
    inputs = random_inputs(rng, num_buffers, n, num_bones)
    flipped = rng.uniform(size=(n, num_bones)) < 0.15
    inputs[1][flipped, 8] *= -4.0                                                       # one input carries negative scales
    weights = blend_weights(rng, WEIGHTED, n, num_buffers)
    with runtime.Context(0) as ctx:
        skeleton = ctx.register_skeleton(parents, reference)
        assert ctx.skeleton_info(skeleton).has_negative_scale == 1
        masks = MaskSet(ctx, rng, num_bones, WEIGHTED)
        handles = masks.draw(rng, n, num_buffers)
        local = [expected_local([inputs[k][i] for k in range(num_buffers)], weights[i], [masks.values[int(h)] for h in handles[i]], WEIGHTED) for i in range(n)]
        assert (np.stack(local)[..., 8:11] < 0.0).any()
        rows = [walked(parents, row) for row in local]
        before = ctx.negative_scale_count()
        check(ctx, inputs, weights, WEIGHTED, rows, handles=handles, skeleton=skeleton, object_space=True)
        assert ctx.negative_scale_count() > before
        assert ctx.rejected_instance_count() == 0


# ---- 8. refusals --------------------------------------------------------------------------------------------------------------------

def test_refused_instances_are_counted_and_leave_row_and_box_alone():
    import torch
    rng = np.random.default_rng(7801)
    bones, more, num_buffers = 24, 32, 3
    parents, more_parents = forest(rng, bones), forest(rng, more)
    with runtime.Context(0) as ctx:
        good = ctx.register_skeleton(parents, identity_pose(bones))
        flat = ctx.register_skeleton(None, identity_pose(bones))                        # no hierarchy
        larger = ctx.register_skeleton(more_parents, identity_pose(more))
        retired = ctx.register_skeleton(parents, identity_pose(bones))
        ctx.unregister_skeleton(retired)
        masks = MaskSet(ctx, rng, bones, WEIGHTED)
        bottom, upper = masks.bottom[1], masks.upper[1]
        other_size = ctx.register_blend_mask(np.ones(bones + 1, dtype=np.float32))
        retired_mask = ctx.register_blend_mask(masks.values[upper])                     # (the last one registered: nothing below reuses its handle)
        ctx.unregister_blend_mask(retired_mask)
        torch.cuda.synchronize()
        #        skeleton     masks                           refused in object space?   in local space?
        cases = [(good, (bottom, upper, 0), False, False),
                 (0x00ABCDEF, (0, 0, 0), True, True),                                   # an unknown skeleton handle
                 (good, (0, 0, upper), False, False),
                 (retired, (0, 0, 0), True, True),                                      # a retired skeleton handle
                 (good, (bottom, other_size, 0), True, True),                           # a mask of another slot count
                 (good, (bottom, 0, retired_mask), True, True),                         # a retired mask
                 (good, (0, upper, upper), False, False),
                 (flat, (bottom, 0, 0), True, False),                                   # object space on a skeleton without a hierarchy
                 (0, (0, 0, 0), True, True),                                            # the null skeleton handle
                 (good, (0, 0xFFFFFFFF, 0), True, True),                                # an unknown mask handle
                 (good, (bottom, upper, upper), False, False)]
        n = len(cases)
        ids = [case[0] for case in cases]
        handles = np.array([case[1] for case in cases], dtype=np.uint32)
        inputs, weights = random_inputs(rng, num_buffers, n, bones), blend_weights(rng, WEIGHTED, n, num_buffers)
        local = [None if cases[i][3] else expected_local([inputs[k][i] for k in range(num_buffers)], weights[i], [masks.values[int(h)] for h in handles[i]], WEIGHTED)
                 for i in range(n)]
        rows = [None if cases[i][2] else walked(parents, local[i]) for i in range(n)]
        for object_space, want in ((True, rows), (False, local)):
            before = ctx.rejected_instance_count()
            check(ctx, inputs, weights, WEIGHTED, want, handles=handles, instance_skeletons=ids, object_space=object_space)
            assert ctx.rejected_instance_count() - before == sum(row is None for row in want)
        # with boxes: a refused record keeps the prefill, like the guard records
        before = ctx.rejected_instance_count()
        done = Launch(ctx, inputs, weights, WEIGHTED, handles=handles, instance_skeletons=ids, object_space=True, bounds_flags=None).enqueue()
        assert np.array_equal(bits(done.out()), bits(done.expected(rows)))
        assert ctx.rejected_instance_count() - before == sum(row is None for row in rows)
        boxes = done.boxes()
        for i in range(n):
            assert bool(np.all(boxes[1 + i] == SENTINEL)) == (rows[i] is None), i
        assert np.all(boxes[[0, n + 1]] == SENTINEL)
        # two skeletons mixed, ONE buffer's stride below B * 48 of the larger: its instances are refused for that stride alone
        which = [bones, more, bones, more, bones]
        ids = [good if b == bones else larger for b in which]
        mixed = [[random_inputs(rng, 2, 1, b)[k % 2][0] for b in which] for k in range(num_buffers)]
        narrow = [[pose[:bones] for pose in mixed[k]] if k == 1 else mixed[k] for k in range(num_buffers)]      # (what fits buffer 1's rows)
        weights = blend_weights(rng, WEIGHTED, len(which), num_buffers)
        local = [expected_local([mixed[k][i] for k in range(num_buffers)], weights[i], [None] * num_buffers, WEIGHTED) if which[i] == bones else None for i in range(len(which))]
        before = ctx.rejected_instance_count()
        check(ctx, narrow, weights, WEIGHTED, local, instance_skeletons=ids, row_bones=[more, bones, more], out_bones=more)
        assert ctx.rejected_instance_count() - before == 2
        # ... and with every stride wide enough the same batch is served whole
        local = [expected_local([mixed[k][i] for k in range(num_buffers)], weights[i], [None] * num_buffers, WEIGHTED) for i in range(len(which))]
        before = ctx.rejected_instance_count()
        check(ctx, mixed, weights, WEIGHTED, local, instance_skeletons=ids)
        assert ctx.rejected_instance_count() == before


def test_a_mask_handle_is_refused_in_a_context_that_never_registered_a_mask():
    """the context's mask table does not exist yet: the null handle serves, every other handle is refused in front of any record load"""
    rng = np.random.default_rng(7851)
    bones, num_buffers = 24, 3
    parents = forest(rng, bones)
    with runtime.Context(0) as ctx:
        skeleton = ctx.register_skeleton(parents, identity_pose(bones))
        handles = np.array([[0, 0, 0], [0, 1, 0], [0, 0, 0], [7, 0, 0], [0, 0, 0xFFFFFFFF], [0, 0, 0]], dtype=np.uint32)
        n = len(handles)
        refused = [bool(row.any()) for row in handles]
        inputs, weights = random_inputs(rng, num_buffers, n, bones), blend_weights(rng, LAYERED, n, num_buffers)
        local = [None if refused[i] else expected_local([inputs[k][i] for k in range(num_buffers)], weights[i], [None] * num_buffers, LAYERED) for i in range(n)]
        rows = [None if row is None else walked(parents, row) for row in local]
        for object_space, want in ((False, local), (True, rows)):
            before = ctx.rejected_instance_count()
            check(ctx, inputs, weights, LAYERED, want, handles=handles, skeleton=skeleton, object_space=object_space)
            assert ctx.rejected_instance_count() - before == sum(refused)


# ---- 9. lifetime --------------------------------------------------------------------------------------------------------------------

def test_unregister_behind_the_launch_and_a_graph_replay_with_new_weights():
    import torch
    rng = np.random.default_rng(7901)
    num_bones, n, num_buffers = 100, 37, 3
    parents = forest(rng, num_bones)
    inputs = random_inputs(rng, num_buffers, n, num_bones)
    bottom_mask, upper_mask = make_masks(rng, num_bones, 1, floor=0.25)[0], make_masks(rng, num_bones, 1)[0]
    mask_values = [bottom_mask, None, upper_mask]

    def rows_of(weights):
        return [walked(parents, expected_local([inputs[k][i] for k in range(num_buffers)], weights[i], mask_values, WEIGHTED)) for i in range(n)]

    weights, later_weights = blend_weights(rng, WEIGHTED, n, num_buffers), blend_weights(rng, WEIGHTED, n, num_buffers)
    rows, later_rows = rows_of(weights), rows_of(later_weights)
    assert not np.array_equal(bits(np.stack(rows)), bits(np.stack(later_rows)))
    with runtime.Context(0) as ctx:
        # unregistered right behind the enqueued launch: it is still served; a later launch refuses the handles
        skeleton = ctx.register_skeleton(parents, identity_pose(num_bones))
        bottom, upper = ctx.register_blend_mask(bottom_mask), ctx.register_blend_mask(upper_mask)
        handles = np.tile(np.array([bottom, 0, upper], dtype=np.uint32), (n, 1))
        done = Launch(ctx, inputs, weights, WEIGHTED, handles=handles, skeleton=skeleton, object_space=True).enqueue()
        ctx.unregister_skeleton(skeleton)
        ctx.unregister_blend_mask(upper)
        assert np.array_equal(bits(done.out()), bits(done.expected(rows)))
        assert ctx.rejected_instance_count() == 0
        later = Launch(ctx, inputs, weights, WEIGHTED, handles=handles, skeleton=skeleton, object_space=True).enqueue()
        assert np.all(later.out() == SENTINEL)
        assert ctx.rejected_instance_count() == n

        # one launch captured once, no parallel branches; replayed once after the weights changed on the device
        skeleton, upper = ctx.register_skeleton(parents, identity_pose(num_bones)), ctx.register_blend_mask(upper_mask)
        handles = np.tile(np.array([bottom, 0, upper], dtype=np.uint32), (n, 1))
        launch = Launch(ctx, inputs, weights, WEIGHTED, handles=handles, skeleton=skeleton, object_space=True)
        side = torch.cuda.Stream(device=launch.buffers.device)
        side.wait_stream(torch.cuda.current_stream(launch.buffers.device))
        with torch.cuda.stream(side):
            launch.enqueue(stream=side.cuda_stream)                                    # warm-up
            side.synchronize()
            graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graph, stream=side):
                launch.enqueue(stream=side.cuda_stream)
        assert np.array_equal(bits(launch.d_out.cpu().numpy()), bits(launch.expected(rows)))
        launch.d_weights.copy_(torch.from_numpy(later_weights))
        launch.d_out.fill_(float(SENTINEL))
        torch.cuda.synchronize()
        graph.replay()
        torch.cuda.synchronize()
        assert np.array_equal(bits(launch.d_out.cpu().numpy()), bits(launch.expected(later_rows)))
        del graph
        assert ctx.rejected_instance_count() == n
