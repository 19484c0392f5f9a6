"""Character bounds (aclhip_decompress_poses_batch_bounds) through the C ABI. min and max are exact and order independent, so the expected box
is always numpy's over the rows the EXISTING launch (aclhip_decompress_poses_batch, _mapped or _masked) writes for the same inputs:
rows[i, counted, 4:7].min(axis=0) / .max(axis=0) in float32, pads 0, compared with np.array_equal -- no tolerance. Every case runs the launch
three ways: without bounds (the reference rows), rows + bounds (rows byte identical, boxes as defined) and bounds alone (poses == NULL: the same
boxes, and the sentinel filled buffer that would have been the rows untouched), into a bounds buffer with a guard record before and behind.
Needs a GPU."""
import numpy as np
import pytest

from acl_amd import runtime, synth
import test_gpu_skeleton_poses as sk

pytestmark = pytest.mark.gpu

SENTINEL = sk.SENTINEL
NONE, RELATIVE, ADDITIVE0, ADDITIVE1 = sk.NONE, sk.RELATIVE, sk.ADDITIVE0, sk.ADDITIVE1
INF = np.float32(np.inf)


def flag_sets(num_bones):
    """NULL, all ones, one bone only, every other bone, all zero"""
    one = np.zeros(num_bones, dtype=np.uint8)
    one[num_bones // 2] = 7
    other = (np.arange(num_bones) % 2 == 0).astype(np.uint8) * 255
    return [None, np.ones(num_bones, dtype=np.uint8), one, other, np.zeros(num_bones, dtype=np.uint8)]


def expected_bounds(rows, pose_bones, flags, refused=()):
    """rows: float32 [n, B, 12] of the launch without bounds; pose_bones[i]: transforms of instance i's pose. [n + 2, 8] with the guards."""
    n = rows.shape[0]
    out = np.full((n + 2, 8), SENTINEL, dtype=np.float32)
    for i in range(n):
        if i in refused:
            continue
        counted = np.ones(pose_bones[i], dtype=bool) if flags is None else flags[:pose_bones[i]] != 0
        box = np.zeros(8, dtype=np.float32)
        box[0:3], box[4:7] = INF, -INF
        if counted.any():
            translations = rows[i, :pose_bones[i]][counted, 4:7]
            assert translations.dtype == np.float32 and not np.isnan(translations).any()
            box[0:3], box[4:7] = translations.min(axis=0), translations.max(axis=0)
        out[1 + i] = box
    return out


class Case:
    """One batch: device arrays, the consumers, and which of the three launches it goes through"""

    def __init__(self, ctx, num_bones, pad_floats=4):
        import torch
        self.torch, self.ctx, self.num_bones = torch, ctx, num_bones
        self.device = torch.device("cuda:0")
        self.row_floats = num_bones * 12 + pad_floats
        self.consumers, self.mapping, self.masking, self.params, self.keep = runtime.PoseConsumers(), None, None, None, []
        self.consumers.object_space = 1

    def up(self, array, dtype):
        array = np.ascontiguousarray(array, dtype=dtype)
        tensor = self.torch.from_numpy(array.view(np.int32) if dtype == np.uint32 else array).to(self.device)
        self.keep.append(tensor)
        return tensor.data_ptr()

    def sentinel(self, rows, floats):
        return self.torch.full((rows, floats), float(SENTINEL), dtype=self.torch.float32, device=self.device)

    def launch_plain(self, clips, times):
        n = len(clips)
        buffer = self.sentinel(n + 2, self.row_floats)
        stream = self.torch.cuda.current_stream(self.device).cuda_stream
        args = (self.up(clips, np.uint32), self.up(times, np.float32), n, buffer[1].data_ptr(), self.row_floats * 4, self.consumers)
        if self.masking is not None:
            self.ctx.decompress_poses_batch_masked(*args, self.mapping, self.masking, params=self.params, stream=stream)
        elif self.mapping is not None:
            self.ctx.decompress_poses_batch_mapped(*args, self.mapping, params=self.params, stream=stream)
        else:
            self.ctx.decompress_poses_batch(*args, params=self.params, stream=stream)
        self.torch.cuda.synchronize()
        return buffer.cpu().numpy()

    def launch_bounds(self, clips, times, flags, with_rows):
        """(the pose buffer, the bounds buffer with its guards) after the launch"""
        n = len(clips)
        buffer, boxes = self.sentinel(n + 2, self.row_floats), self.sentinel(n + 2, 8)
        bounds = runtime.PoseBounds()
        bounds.bounds = boxes[1].data_ptr()
        bounds.bone_flags = self.up(flags, np.uint8) if flags is not None else None
        self.ctx.decompress_poses_batch_bounds(self.up(clips, np.uint32), self.up(times, np.float32), n, bounds, buffer[1].data_ptr() if with_rows else None,
                                               self.row_floats * 4, self.consumers, self.mapping, self.masking, params=self.params,
                                               stream=self.torch.cuda.current_stream(self.device).cuda_stream)
        self.torch.cuda.synchronize()
        return buffer.cpu().numpy(), boxes.cpu().numpy()

    def check(self, clips, times, pose_bones, all_flags=(None,), refused=(), label=None):
        """Returns the rows of the launch without bounds ([n, B, 12])"""
        n = len(clips)
        plain = self.launch_plain(clips, times)
        rows = plain[1:1 + n, : self.num_bones * 12].reshape(n, self.num_bones, 12)
        untouched = np.full_like(plain, SENTINEL)
        for i in range(n):
            assert (i in refused or pose_bones[i] == 0) == bool(np.all(plain[1 + i] == SENTINEL)), (label, i)
        for index, flags in enumerate(all_flags):
            expected = expected_bounds(rows, pose_bones, flags, refused)
            with_rows, boxes = self.launch_bounds(clips, times, flags, True)
            assert np.array_equal(with_rows.view(np.uint32), plain.view(np.uint32)), (label, index)         # byte identical rows
            assert np.array_equal(boxes, expected), (label, index, boxes, expected)
            assert np.all(boxes[1:1 + n][:, [3, 7]][[i for i in range(n) if i not in refused]] == 0), (label, index)   # the pads
            no_rows, boxes = self.launch_bounds(clips, times, flags, False)
            assert np.array_equal(boxes, expected), (label, index, "bounds alone", boxes, expected)
            assert np.array_equal(no_rows, untouched), (label, index)
        return rows


@pytest.mark.parametrize("num_bones", [1, 63, 64, 65, 100, 129, 300, 1200])
def test_bone_and_instance_counts_through_both_image_layouts(num_bones):
    """Lane stride edges of the reduction (63 / 64 / 65, 129) and 4, 2 and 1 instances per workgroup (100 / 300 / 1200 bones), batches that
    end inside a workgroup (1, 3, 5, 9 instances). A registry of unit-scale clips alone takes the rotation | translation images; the same
    batches again once a scaled clip is registered take the qvv images."""
    rng = np.random.default_rng(900 + num_bones)
    clip = synth.build_clip(seed=700 + num_bones, num_tracks=num_bones, num_samples=12)
    parents = sk.hierarchy(rng, num_bones)
    with runtime.Context(0) as ctx:
        handle = ctx.register_clip(clip.blob)
        ctx.set_clip_hierarchy(handle, parents)
        batches = [(np.full(n, handle, dtype=np.uint32), rng.uniform(0.0, clip.duration, size=n).astype(np.float32)) for n in (1, 3, 5, 9)]
        unit_scale_rows = []
        for clips, times in batches:
            case = Case(ctx, num_bones, pad_floats=0 if len(clips) % 2 else 4)
            unit_scale_rows.append(case.check(clips, times, [num_bones] * len(clips), flag_sets(num_bones), label=("unit scale", len(clips))))
        scaled = ctx.register_clip(synth.build_clip(seed=699, num_tracks=5, num_samples=6, has_scale=1, scale_default=0.3).blob)
        assert ctx.clip_info(scaled).has_scale == 1
        for (clips, times), before in zip(batches, unit_scale_rows):
            case = Case(ctx, num_bones, pad_floats=0 if len(clips) % 2 else 4)
            rows = case.check(clips, times, [num_bones] * len(clips), flag_sets(num_bones), label=("qvv", len(clips)))
            assert np.array_equal(rows, before)
        assert ctx.rejected_instance_count() == 0


def test_a_negative_scale_takes_the_matrix_route_and_is_counted_alike():
    rng = np.random.default_rng(921)
    mirrored = synth.build_clip(seed=92, num_tracks=100, num_samples=45, has_scale=1, scale_default=0.3, scale_constant=0.3, mirrored_scale_fraction=0.3)
    parents = np.array(synth.humanoid_hierarchy(100), dtype=np.uint32)
    with runtime.Context(0) as ctx:
        handle = ctx.register_clip(mirrored.blob)
        ctx.set_clip_hierarchy(handle, parents)
        n = 9
        clips, times = np.full(n, handle, dtype=np.uint32), rng.uniform(0.0, mirrored.duration, size=n).astype(np.float32)
        case = Case(ctx, 100)
        counts = [ctx.negative_scale_count()]
        rows = case.launch_plain(clips, times)[1:1 + n, :1200].reshape(n, 100, 12)
        counts.append(ctx.negative_scale_count())
        assert (rows[..., 8:11] < 0.0).any() and counts[1] > counts[0]
        for with_rows in (True, False):
            _, boxes = case.launch_bounds(clips, times, None, with_rows)
            assert np.array_equal(boxes, expected_bounds(rows, [100] * n, None))
            counts.append(ctx.negative_scale_count())
        assert counts[2] - counts[1] == counts[3] - counts[2] == counts[1] - counts[0]       # moves as it does for the launch without bounds
        case.check(clips, times, [100] * n, flag_sets(100), label="mirrored")
        assert ctx.rejected_instance_count() == 0


def test_every_way_an_unmapped_image_gets_filled():
    """plain, additive0 onto a base clip (fused), relative onto a base clip (second wave), additive1 onto a base pose buffer, a 3-clip blend,
    ACLHIP_CONSUMERS_FAST -- once each, 100 bones with scale"""
    rng = np.random.default_rng(922)
    num_bones, n = 100, 7
    clips = [synth.build_clip(seed=710 + k, num_tracks=num_bones, num_samples=30 + k, has_scale=1, scale_default=0.3) for k in range(3)]
    parents = np.array(synth.humanoid_hierarchy(num_bones), dtype=np.uint32)
    with runtime.Context(0) as ctx:
        handles = np.array([ctx.register_clip(c.blob) for c in clips], dtype=np.uint32)
        for handle in handles:
            ctx.set_clip_hierarchy(handle, parents)
        first, others = rng.integers(0, 3, size=n), rng.integers(0, 3, size=(n, 2))
        times = np.array([rng.uniform(0.0, clips[c].duration) for c in first], dtype=np.float32)
        other_times = np.array([[rng.uniform(0.0, clips[c].duration) for c in row] for row in others], dtype=np.float32)
        base_buffer = np.stack([sk.reference_pose(rng, num_bones) for _ in range(n)])
        seen = []
        for name in ("plain", "additive0 fused", "relative second wave", "additive1 base buffer", "blend of three", "fast"):
            case = Case(ctx, num_bones)
            consumers = case.consumers
            if name == "additive0 fused":
                consumers.additive_format, consumers.base_clips, consumers.base_sample_times = ADDITIVE0, case.up(handles[others[:, 0]], np.uint32), case.up(other_times[:, 0], np.float32)
            if name == "relative second wave":
                consumers.additive_format, consumers.base_clips, consumers.base_sample_times = RELATIVE, case.up(handles[others[:, 0]], np.uint32), case.up(other_times[:, 0], np.float32)
            if name == "additive1 base buffer":
                consumers.additive_format, consumers.base_poses, consumers.base_pose_stride_bytes = ADDITIVE1, case.up(base_buffer, np.float32), num_bones * 48
            if name == "blend of three":
                consumers.num_blend_clips = 3
                consumers.blend_clips, consumers.blend_sample_times = case.up(handles[others], np.uint32), case.up(other_times, np.float32)
                consumers.blend_weights = case.up(rng.dirichlet(np.ones(3), size=n).astype(np.float32), np.float32)
            if name == "fast":
                consumers.flags = runtime.CONSUMERS_FAST
            rows = case.check(handles[first], times, [num_bones] * n, flag_sets(num_bones)[:4:3], label=name)
            assert np.isfinite(rows).all(), name
            assert name == "fast" or not any(np.array_equal(rows, other) for other in seen), name      # (different launches; FAST may round alike)
            seen.append(rows)
        assert ctx.rejected_instance_count() == 0


def test_skeleton_space_filled_slots_count_and_masked_layers():
    """_mapped into a skeleton with more slots than any clip has tracks (the reference pose fills the rest: those bones are in the box), then
    _masked, layered, over the same skeleton"""
    rng = np.random.default_rng(923)
    num_bones, n = 128, 9
    clips, tables = sk.blend_rig(rng, num_bones)
    reference, parents = sk.reference_pose(rng, num_bones), np.array(synth.humanoid_hierarchy(num_bones), dtype=np.uint32)
    reference[:, 4:7] *= 50.0                                                            # filled slots far out: they decide the box
    mask = rng.uniform(0.0, 1.0, size=num_bones).astype(np.float32)
    mask[40:80], mask[100:] = 1.0, 0.0
    with runtime.Context(0) as ctx:
        handles = np.array([ctx.register_clip(c.blob) for c in clips], dtype=np.uint32)
        maps = np.array([ctx.register_track_map(t, num_bones) for t in tables], dtype=np.uint32)
        skeleton = ctx.register_skeleton(parents, reference)
        upper = ctx.register_blend_mask(mask)
        first, others = rng.integers(0, 4, size=n), rng.integers(0, 4, size=(n, 1))
        times = np.array([rng.uniform(0.0, clips[c].duration) for c in first], dtype=np.float32)
        other_times = np.array([[rng.uniform(0.0, clips[c].duration) for c in row] for row in others], dtype=np.float32)

        case = Case(ctx, num_bones)
        case.mapping = runtime.PoseMapping()
        case.mapping.skeleton, case.mapping.instance_maps = skeleton, case.up(maps[first], np.uint32)
        rows = case.check(handles[first], times, [num_bones] * n, flag_sets(num_bones), label="mapped")
        unmapped_slots = np.setdiff1d(np.arange(num_bones), tables[first[0]][tables[first[0]] != sk.DROPPED])
        assert unmapped_slots.size > 0 and np.isfinite(rows).all()

        case = Case(ctx, num_bones, pad_floats=0)
        case.mapping, case.masking = runtime.PoseMapping(), runtime.BlendMasking()
        weights = np.ones((n, 2), dtype=np.float32)
        weights[:, 1] = rng.uniform(0.0, 1.0, size=n)
        case.consumers.num_blend_clips = 2
        case.consumers.blend_clips, case.consumers.blend_sample_times, case.consumers.blend_weights = case.up(handles[others], np.uint32), case.up(other_times, np.float32), case.up(weights, np.float32)
        case.mapping.skeleton, case.mapping.instance_maps, case.mapping.blend_maps = skeleton, case.up(maps[first], np.uint32), case.up(maps[others], np.uint32)
        case.masking.mode, case.masking.instance_masks = runtime.BLEND_LAYERED, case.up(np.tile(np.array([0, upper]), (n, 1)), np.uint32)
        masked_rows = case.check(handles[first], times, [num_bones] * n, flag_sets(num_bones), label="masked layered")
        assert np.isfinite(masked_rows).all() and not np.array_equal(masked_rows, rows)
        assert ctx.rejected_instance_count() == 0


def test_an_empty_pose_gets_the_empty_box():
    """a clip of zero tracks is served, not refused: +inf / -inf, no row; the same box as all-zero bone_flags give its neighbours"""
    rng = np.random.default_rng(924)
    clip, empty = synth.build_clip(seed=720, num_tracks=20, num_samples=10), synth.build_clip(seed=721, num_tracks=0, num_samples=10)
    with runtime.Context(0) as ctx:
        handle, h_empty = ctx.register_clip(clip.blob), ctx.register_clip(empty.blob)
        ctx.set_clip_hierarchy(handle, sk.hierarchy(rng, 20))
        ctx.set_clip_hierarchy(h_empty, np.zeros(0, dtype=np.uint32))
        clips = np.array([h_empty, handle, h_empty, handle, handle], dtype=np.uint32)
        times = rng.uniform(0.0, clip.duration, size=5).astype(np.float32)
        pose_bones = [0, 20, 0, 20, 20]
        for scaled in (False, True):
            if scaled:
                ctx.register_clip(synth.build_clip(seed=722, num_tracks=5, num_samples=6, has_scale=1, scale_default=0.3).blob)
            case = Case(ctx, 20)
            case.check(clips, times, pose_bones, flag_sets(20), label=scaled)
            _, boxes = case.launch_bounds(clips, times, None, False)
            assert np.array_equal(boxes[1], np.array([INF, INF, INF, 0, -INF, -INF, -INF, 0], dtype=np.float32)) and np.array_equal(boxes[1], boxes[3])
            _, zero_flags = case.launch_bounds(clips, times, np.zeros(20, dtype=np.uint8), True)
            assert all(np.array_equal(zero_flags[1 + i], boxes[1]) for i in range(5))
        assert ctx.rejected_instance_count() == 0


def test_refused_instances_leave_their_box_and_row_alone():
    """an unknown clip handle in the middle of five instances and a pose larger than pose_stride_bytes / 48 in another slot"""
    rng = np.random.default_rng(925)
    clip, larger = synth.build_clip(seed=730, num_tracks=20, num_samples=10), synth.build_clip(seed=731, num_tracks=30, num_samples=10)
    with runtime.Context(0) as ctx:
        handle, h_larger = ctx.register_clip(clip.blob), ctx.register_clip(larger.blob)
        ctx.set_clip_hierarchy(handle, sk.hierarchy(rng, 20))
        ctx.set_clip_hierarchy(h_larger, sk.hierarchy(rng, 30))
        clips = np.array([handle, handle, 0x00ABCDEF, h_larger, handle], dtype=np.uint32)
        times = rng.uniform(0.0, clip.duration, size=5).astype(np.float32)
        for scaled in (False, True):
            if scaled:
                ctx.register_clip(synth.build_clip(seed=732, num_tracks=5, num_samples=6, has_scale=1, scale_default=0.3).blob)
            case = Case(ctx, 20, pad_floats=0)
            before = ctx.rejected_instance_count()
            plain = case.launch_plain(clips, times)
            assert ctx.rejected_instance_count() - before == 2
            rows = plain[1:6].reshape(5, 20, 12)
            for with_rows in (True, False):
                before = ctx.rejected_instance_count()
                poses, boxes = case.launch_bounds(clips, times, None, with_rows)
                assert ctx.rejected_instance_count() - before == 2
                # the refused records and the guard records before and behind the bounds hold the sentinel, the neighbours are exact
                assert np.array_equal(boxes, expected_bounds(rows, [20] * 5, None, refused=(2, 3)))
                assert np.all(boxes[[0, 3, 4, 6]] == SENTINEL)
                assert np.array_equal(poses, plain if with_rows else np.full_like(plain, SENTINEL))
            case.check(clips, times, [20] * 5, flag_sets(20), refused=(2, 3), label=scaled)


def test_host_side_refusals_launch_nothing():
    import torch
    rng = np.random.default_rng(926)
    clip = synth.build_clip(seed=740, num_tracks=20, num_samples=10)
    with runtime.Context(0) as ctx:
        handle = ctx.register_clip(clip.blob)
        ctx.set_clip_hierarchy(handle, sk.hierarchy(rng, 20))
        case = Case(ctx, 20)
        clips, times = case.up(np.full(3, handle), np.uint32), case.up(np.zeros(3), np.float32)
        poses, boxes = case.sentinel(3, 240), case.sentinel(4, 8)
        stream = torch.cuda.current_stream().cuda_stream
        for spoil in ("bounds", "buffer", "alignment", "reserved", "local space", "masking alone", "stride", "params", "flags"):
            bounds, consumers, masking, params, stride = runtime.PoseBounds(), runtime.PoseConsumers(), None, None, 960
            bounds.bounds, consumers.object_space = boxes.data_ptr(), 1
            if spoil == "bounds":
                bounds = None
            if spoil == "buffer":
                bounds.bounds = None
            if spoil == "alignment":
                bounds.bounds = boxes.data_ptr() + 8
            if spoil == "reserved":
                bounds.reserved[0] = 1
            if spoil == "local space":
                consumers.object_space = 0
            if spoil == "masking alone":
                masking = runtime.BlendMasking()
            if spoil == "stride":
                stride = 968
            if spoil == "params":
                params = runtime.default_params(per_track_rounding=1)
            if spoil == "flags":
                consumers.flags = 0x80
            with pytest.raises(runtime.AclHipError) as error:
                ctx.decompress_poses_batch_bounds(clips, times, 3, bounds, poses.data_ptr(), stride, consumers, None, masking, params=params, stream=stream)
            assert error.value.status == runtime.ERROR_INVALID_ARGUMENT, spoil
        torch.cuda.synchronize()
        assert bool((poses == float(SENTINEL)).all()) and bool((boxes == float(SENTINEL)).all())
        assert ctx.rejected_instance_count() == 0
