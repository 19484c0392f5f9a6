"""aclhip_transform_poses_batch through the C ABI: apply_additive_to_base and local_to_object_space over pose buffers the caller filled.
The expected rows are the oracle's functions over the same arrays, oracle_apply_additive_to_base and oracle_local_to_object_space, compared
on bits (np.array_equal over uint32 views) over the whole sentinel filled buffers: a guard row before and behind every buffer, pad floats
behind every row. The kernels and the oracle run the same operation order, so there is no tolerance. Inputs are finite (a result that is
not a number has other bits on x86 than on the GPU): rotations are unit quaternions times a factor in [0.5, 2], translations lie within
+-10, scales in [0.5, 2] -- [0.9, 1.1] on the chain of depth 100, so that nothing overflows along it. Needs a GPU."""
import ctypes

import numpy as np
import pytest

from acl_amd import runtime, synth
from oracle import bindings as ob

pytestmark = pytest.mark.gpu

SENTINEL = np.float32(-7777.25)
NONE, RELATIVE, ADDITIVE0, ADDITIVE1 = runtime.ADDITIVE_NONE, runtime.ADDITIVE_RELATIVE, runtime.ADDITIVE_ADDITIVE0, runtime.ADDITIVE_ADDITIVE1
INF = np.float32(np.inf)


def bits(array):
    return np.ascontiguousarray(array, dtype=np.float32).view(np.uint32)


def forest(rng, num_bones, root_chance=0.08):
    """a random forest, parents first: several roots, a parent up to nine bones back"""
    parents = np.zeros(num_bones, dtype=np.uint32)
    parents[0] = runtime.NO_PARENT
    for i in range(1, num_bones):
        parents[i] = runtime.NO_PARENT if rng.uniform() < root_chance else rng.integers(max(0, i - 9), i)
    return parents


def chain(num_bones):
    parents = np.arange(num_bones, dtype=np.int64) - 1
    parents[0] = runtime.NO_PARENT
    return parents.astype(np.uint32)


def random_poses(rng, n, num_bones, scale=(0.5, 2.0)):
    """float32 [n, B, 12], the pads 0"""
    poses = np.zeros((n, num_bones, 12), dtype=np.float32)
    rotations = rng.normal(size=(n, num_bones, 4))
    rotations /= np.linalg.norm(rotations, axis=2, keepdims=True)
    poses[..., 0:4] = rotations * rng.uniform(0.5, 2.0, size=(n, num_bones, 1))
    poses[..., 4:7] = rng.uniform(-10.0, 10.0, size=(n, num_bones, 3))
    poses[..., 8:11] = rng.uniform(scale[0], scale[1], size=(n, num_bones, 3))
    return poses


def identity_pose(num_bones):
    pose = np.zeros((num_bones, 12), dtype=np.float32)
    pose[:, 3] = 1.0
    pose[:, 8:11] = 1.0
    return pose


def expected_rows(local, parents, additive_format=NONE, additive=None, object_space=True):
    """per instance: the oracle over the instance's arrays; parents: one hierarchy, or one per instance"""
    rows = []
    for i in range(len(local)):
        pose = local[i]
        if additive_format != NONE:
            pose = ob.oracle_apply_additive_to_base(additive_format, pose, additive[i])
        if object_space:
            pose = ob.oracle_local_to_object_space(parents[i] if isinstance(parents, list) else parents, pose)
        rows.append(pose)
    return rows


class Buffers:
    """The device buffers of one batch, each [n + 2, row floats], sentinel filled, with a guard row before and behind its n rows"""

    def __init__(self, n, row_floats):
        import torch
        self.torch, self.n, self.row_floats = torch, n, row_floats
        self.device = torch.device("cuda:0")
        self.keep = []

    def host(self, rows=None, row_floats=None):
        """rows: per instance a pose [B_i, 12] or None (the row stays the sentinel)"""
        out = np.full((self.n + 2, row_floats if row_floats is not None else self.row_floats), SENTINEL, dtype=np.float32)
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


def run(ctx, local, skeleton=0, instance_skeletons=None, object_space=True, additive_format=NONE, additive=None, pad_floats=4, in_place=False, bounds_flags="none",
        with_rows=True, row_bones=None, additive_row_bones=None):
    """One launch over `local` ([n, B, 12], or a list of per instance poses). Returns (output buffer, input buffer after the launch, input
    buffer as uploaded, boxes or None), all with their guard rows, on the host. bounds_flags: "none" (no bounds), None (every bone) or uint8 flags."""
    n = len(local)
    row_bones = row_bones if row_bones is not None else max(pose.shape[0] for pose in local)
    buffers = Buffers(n, row_bones * 12 + pad_floats)
    h_local = buffers.host(local)
    d_local = buffers.up(h_local)
    d_out = d_local if in_place else buffers.up(buffers.host())
    consumers = runtime.PoseBufferConsumers()
    consumers.skeleton, consumers.object_space, consumers.additive_format = skeleton, 1 if object_space else 0, additive_format
    if instance_skeletons is not None:
        consumers.instance_skeletons = buffers.up(np.asarray(instance_skeletons, dtype=np.uint32)).data_ptr()
    if additive_format != NONE:
        additive_floats = (additive_row_bones if additive_row_bones is not None else row_bones) * 12 + 8      # (a stride of its own)
        d_additive = buffers.up(buffers.host(additive, additive_floats))
        consumers.additive_poses, consumers.additive_pose_stride_bytes = d_additive[1].data_ptr(), additive_floats * 4
    bounds, d_boxes = None, None
    if not isinstance(bounds_flags, str):
        bounds, d_boxes = runtime.PoseBounds(), buffers.up(np.full((n + 2, 8), SENTINEL, dtype=np.float32))
        bounds.bounds = d_boxes[1].data_ptr()
        bounds.bone_flags = buffers.up(np.asarray(bounds_flags, dtype=np.uint8)).data_ptr() if bounds_flags is not None else None
    ctx.transform_poses_batch(d_local[1].data_ptr(), buffers.row_floats * 4, n, consumers, d_out[1].data_ptr() if with_rows else None, buffers.row_floats * 4,
                              bounds=bounds, stream=buffers.stream())
    out = buffers.down(d_out)
    if additive_format != NONE:
        assert np.array_equal(bits(buffers.down(d_additive)), bits(buffers.host(additive, additive_floats)))      # the additive buffer is only read
    return out, buffers.down(d_local), h_local, (buffers.down(d_boxes) if d_boxes is not None else None), buffers


def check(ctx, local, expected, **launch):
    """out of place: the output is `expected` over the whole guarded buffer, the input buffer is unchanged. Returns the output buffer."""
    out, local_after, local_before, _, buffers = run(ctx, local, **launch)
    assert np.array_equal(bits(local_after), bits(local_before))
    want = buffers.host(expected)
    assert np.array_equal(bits(out), bits(want)), np.argwhere(bits(out) != bits(want))[:8]
    return out


WALK_BONES = [1, 63, 64, 65, 100, 300, 1200]


@pytest.fixture(scope="module")
def walk_cases():
    """test 1's batches, shared with the in place test: B -> (parents, [(local poses, oracle rows) for n in 1, 3, 5, 9])"""
    cases = {}
    for num_bones in WALK_BONES:
        rng = np.random.default_rng(4100 + num_bones)
        parents = forest(rng, num_bones)
        batches = []
        for n in (1, 3, 5, 9):
            local = random_poses(rng, n, num_bones)
            batches.append((local, expected_rows(local, parents)))
        cases[num_bones] = (parents, batches)
    return cases


@pytest.mark.parametrize("num_bones", WALK_BONES)
def test_the_walk_is_the_oracles(walk_cases, num_bones):
    """lane stride edges (63 / 64 / 65), 4, 2 and 1 instances per workgroup (100 / 300 / 1200 bones), batches that end inside a workgroup"""
    parents, batches = walk_cases[num_bones]
    assert num_bones < 20 or int((parents == runtime.NO_PARENT).sum()) > 1        # several roots
    with runtime.Context(0) as ctx:
        skeleton = ctx.register_skeleton(parents, identity_pose(num_bones))
        for index, (local, rows) in enumerate(batches):
            assert np.isfinite(np.stack(rows)).all()
            check(ctx, local, rows, skeleton=skeleton, pad_floats=0 if index % 2 else 4)
        assert ctx.rejected_instance_count() == 0
        assert ctx.negative_scale_count() == 0


def test_a_chain_of_depth_100():
    rng = np.random.default_rng(4201)
    parents = chain(100)
    with runtime.Context(0) as ctx:
        skeleton = ctx.register_skeleton(parents, identity_pose(100))
        assert ctx.skeleton_info(skeleton).depth == 100
        for n in (1, 5):
            local = random_poses(rng, n, 100, scale=(0.9, 1.1))
            rows = expected_rows(local, parents)
            assert np.isfinite(np.stack(rows)).all()
            check(ctx, local, rows, skeleton=skeleton)
        assert ctx.rejected_instance_count() == 0


def test_a_root_keeps_its_bytes_and_every_walked_bone_gets_zero_pads():
    """the header's statement on pads: object space without an additive buffer copies a root whole; with one, every pad is 0"""
    rng = np.random.default_rng(4202)
    parents = forest(rng, 20, root_chance=0.2)
    roots = parents == runtime.NO_PARENT
    with runtime.Context(0) as ctx:
        skeleton = ctx.register_skeleton(parents, identity_pose(20))
        local = random_poses(rng, 3, 20)
        local[..., 7], local[..., 11] = 5.5, -6.5
        out, _, _, _, _ = run(ctx, local, skeleton=skeleton, pad_floats=0)
        rows = out[1:4].reshape(3, 20, 12)
        assert np.all(rows[:, roots][..., 7] == 5.5) and np.all(rows[:, roots][..., 11] == -6.5) and np.all(rows[:, ~roots][..., [7, 11]] == 0.0)
        expected = np.stack(expected_rows(local, parents))
        assert np.array_equal(bits(rows[..., [0, 1, 2, 3, 4, 5, 6, 8, 9, 10]]), bits(expected[..., [0, 1, 2, 3, 4, 5, 6, 8, 9, 10]]))
        additive = random_poses(rng, 3, 20)
        out, _, _, _, _ = run(ctx, local, skeleton=skeleton, pad_floats=0, additive_format=ADDITIVE0, additive=additive)
        assert np.array_equal(bits(out[1:4].reshape(3, 20, 12)), bits(np.stack(expected_rows(local, parents, ADDITIVE0, additive))))
        assert np.all(out[1:4].reshape(3, 20, 12)[..., [7, 11]] == 0.0)


@pytest.mark.parametrize("num_bones", [100, 65])
@pytest.mark.parametrize("object_space", [True, False])
@pytest.mark.parametrize("additive_format", [RELATIVE, ADDITIVE0, ADDITIVE1])
def test_additive_buffers(additive_format, object_space, num_bones):
    rng = np.random.default_rng(4300 + num_bones * 8 + additive_format * 2 + int(object_space))
    parents = forest(rng, num_bones)
    n = 5
    local, additive = random_poses(rng, n, num_bones), random_poses(rng, n, num_bones, scale=(0.5, 1.5))
    rows = expected_rows(local, parents, additive_format, additive, object_space)
    assert np.isfinite(np.stack(rows)).all()
    with runtime.Context(0) as ctx:
        # (local output needs no hierarchy: a skeleton registered without parents serves it)
        skeleton = ctx.register_skeleton(parents if object_space else None, identity_pose(num_bones))
        check(ctx, local, rows, skeleton=skeleton, object_space=object_space, additive_format=additive_format, additive=additive)
        assert ctx.rejected_instance_count() == 0


def test_negative_scales_take_the_matrix_route_and_are_counted():
    rng = np.random.default_rng(4401)
    num_bones, n = 100, 5
    parents = forest(rng, num_bones)
    local = random_poses(rng, n, num_bones, scale=(0.8, 1.25))
    flipped = rng.uniform(size=(n, num_bones, 3)) < 0.1
    local[..., 8:11][flipped] *= -1.0
    additive = random_poses(rng, n, num_bones, scale=(0.8, 1.25))
    additive[..., 8:11][rng.uniform(size=(n, num_bones, 3)) < 0.1] *= -1.0
    rows = expected_rows(local, parents)
    relative_rows = expected_rows(local, parents, RELATIVE, additive)
    assert np.isfinite(np.stack(rows)).all() and np.isfinite(np.stack(relative_rows)).all()      # (checked on the CPU first: the seed's outputs are numbers)
    assert (np.stack(rows)[..., 8:11] < 0.0).any()
    with runtime.Context(0) as ctx:
        skeleton = ctx.register_skeleton(parents, identity_pose(num_bones))
        before = ctx.negative_scale_count()
        check(ctx, local, rows, skeleton=skeleton)
        walked = ctx.negative_scale_count()
        assert walked > before
        check(ctx, local, relative_rows, skeleton=skeleton, additive_format=RELATIVE, additive=additive)
        assert ctx.negative_scale_count() > walked
        assert ctx.rejected_instance_count() == 0


@pytest.mark.parametrize("num_bones", [100, 1200])
def test_in_place_gives_the_bits_of_out_of_place(walk_cases, num_bones):
    parents, batches = walk_cases[num_bones]
    rng = np.random.default_rng(4500 + num_bones)
    with runtime.Context(0) as ctx:
        skeleton = ctx.register_skeleton(parents, identity_pose(num_bones))
        for local, rows in batches:
            apart = check(ctx, local, rows, skeleton=skeleton)
            out, local_after, _, _, _ = run(ctx, local, skeleton=skeleton, in_place=True)
            assert np.array_equal(bits(out), bits(apart)) and np.array_equal(bits(local_after), bits(apart))
        # with an additive buffer the tail reads the local rows from HBM while the image holds the additive ones
        local, _ = batches[3]
        additive = random_poses(rng, len(local), num_bones, scale=(0.8, 1.25))
        rows = expected_rows(local, parents, ADDITIVE1, additive)
        apart = check(ctx, local, rows, skeleton=skeleton, additive_format=ADDITIVE1, additive=additive)
        out, _, _, _, _ = run(ctx, local, skeleton=skeleton, additive_format=ADDITIVE1, additive=additive, in_place=True)
        assert np.array_equal(bits(out), bits(apart))
        assert ctx.rejected_instance_count() == 0


@pytest.mark.parametrize("scaled", [False, True])
def test_decode_then_walk_in_place_is_the_fused_object_space_launch(scaled):
    rng = np.random.default_rng(4600 + int(scaled))
    num_bones, n = 100, 9
    clip = synth.build_clip(seed=4610 + int(scaled), num_tracks=num_bones, num_samples=40, **(dict(has_scale=1, scale_default=0.3) if scaled else {}))
    parents = np.array(synth.humanoid_hierarchy(num_bones), dtype=np.uint32)
    with runtime.Context(0) as ctx:
        handle = ctx.register_clip(clip.blob)
        assert ctx.clip_info(handle).has_scale == int(scaled)
        ctx.set_clip_hierarchy(handle, parents)
        skeleton = ctx.register_skeleton(parents, identity_pose(num_bones))
        buffers = Buffers(n, num_bones * 12 + 4)
        d_clips, d_times = buffers.up(np.full(n, handle, dtype=np.uint32)), buffers.up(rng.uniform(0.0, clip.duration, size=n).astype(np.float32))
        fused, staged = buffers.up(buffers.host()), buffers.up(buffers.host())
        consumers = runtime.PoseConsumers()
        consumers.object_space = 1
        stride = buffers.row_floats * 4
        ctx.decompress_poses_batch(d_clips.data_ptr(), d_times.data_ptr(), n, fused[1].data_ptr(), stride, consumers, stream=buffers.stream())
        ctx.decompress_tracks_batch(d_clips.data_ptr(), d_times.data_ptr(), n, staged[1].data_ptr(), stride, stream=buffers.stream())
        local = buffers.down(staged).copy()
        on_buffers = runtime.PoseBufferConsumers()
        on_buffers.skeleton, on_buffers.object_space = skeleton, 1
        ctx.transform_poses_batch(staged[1].data_ptr(), stride, n, on_buffers, staged[1].data_ptr(), stride, stream=buffers.stream())
        walked, fused = buffers.down(staged), buffers.down(fused)
        assert np.array_equal(bits(walked), bits(fused))             # byte identical, guard rows and pad floats included
        assert not np.array_equal(bits(walked), bits(local))
        assert ctx.rejected_instance_count() == 0


def test_skeletons_per_instance_mixed_inside_a_workgroup():
    rng = np.random.default_rng(4701)
    small, large = 40, 100
    parents = {small: forest(rng, small, root_chance=0.2), large: forest(rng, large)}
    which = [large, small, small, large, small, large, large, small, large]
    local = [random_poses(rng, 1, bones)[0] for bones in which]
    additive = [random_poses(rng, 1, bones, scale=(0.8, 1.25))[0] for bones in which]
    with runtime.Context(0) as ctx:
        handles = {bones: ctx.register_skeleton(parents[bones], identity_pose(bones)) for bones in (small, large)}
        ids = [handles[bones] for bones in which]
        rows = expected_rows(local, [parents[bones] for bones in which])
        out = check(ctx, local, rows, instance_skeletons=ids, row_bones=large)
        assert np.all(out[2, small * 12:] == SENTINEL)               # a row is written up to its own skeleton's B * 48
        rows = expected_rows(local, [parents[bones] for bones in which], RELATIVE, additive)
        check(ctx, local, rows, instance_skeletons=ids, row_bones=large, additive_format=RELATIVE, additive=additive)
        # a launch wide skeleton is ignored next to the list
        check(ctx, local, rows, skeleton=handles[small], instance_skeletons=ids, row_bones=large, additive_format=RELATIVE, additive=additive)
        assert ctx.rejected_instance_count() == 0


def test_refused_instances_are_counted_and_leave_row_and_box_alone():
    import torch
    rng = np.random.default_rng(4801)
    bones = 24
    parents = forest(rng, bones)
    with runtime.Context(0) as ctx:
        good = ctx.register_skeleton(parents, identity_pose(bones))
        flat = ctx.register_skeleton(None, identity_pose(bones))                     # no hierarchy
        wide = ctx.register_skeleton(forest(rng, bones + 8), identity_pose(bones + 8))  # more bones than a row holds
        retired = ctx.register_skeleton(parents, identity_pose(bones))
        ctx.unregister_skeleton(retired)
        torch.cuda.synchronize()
        #      skeleton     refused under object space?
        ids = [good, 0, good, 0x00ABCDEF, retired, good, flat, wide, good]
        refused = [False, True, False, True, True, False, True, True, False]
        n = len(ids)
        local = [random_poses(rng, 1, bones)[0] for _ in range(n)]
        rows = [None if no else pose for no, pose in zip(refused, expected_rows(local, parents))]
        before = ctx.rejected_instance_count()
        check(ctx, local, rows, instance_skeletons=ids)
        assert ctx.rejected_instance_count() - before == sum(refused)
        # with boxes: a refused record keeps the sentinel, like the guard records
        before = ctx.rejected_instance_count()
        out, _, _, boxes, buffers = run(ctx, local, instance_skeletons=ids, bounds_flags=None)
        assert ctx.rejected_instance_count() - before == sum(refused)
        assert np.array_equal(bits(out), bits(buffers.host(rows)))
        for i in range(n):
            assert bool(np.all(boxes[1 + i] == SENTINEL)) == refused[i], i
        assert np.all(boxes[[0, n + 1]] == SENTINEL)
        # local output with an additive buffer: the skeleton without hierarchy is served, and a skeleton larger than the ADDITIVE stride is refused
        additive = [random_poses(rng, 1, bones, scale=(0.8, 1.25))[0] for _ in range(n)]
        ids_local = [good, flat, wide, good, 0]
        rows = expected_rows(local[:5], parents, ADDITIVE0, additive[:5], object_space=False)
        before = ctx.rejected_instance_count()
        check(ctx, local[:5], [rows[0], rows[1], None, rows[3], None], instance_skeletons=ids_local, object_space=False, additive_format=ADDITIVE0, additive=additive[:5])
        assert ctx.rejected_instance_count() - before == 2
        # rows wide enough for the larger skeleton, an additive stride that is not: refused for the additive stride alone
        wide_local = [random_poses(rng, 1, bones + 8)[0] for _ in range(3)]
        rows = expected_rows([pose[:bones] for pose in wide_local], parents, ADDITIVE0, additive[:3], object_space=False)
        before = ctx.rejected_instance_count()
        check(ctx, wide_local, [rows[0], None, rows[2]], instance_skeletons=[good, wide, good], object_space=False, additive_format=ADDITIVE0,
              additive=additive[:3], row_bones=bones + 8, additive_row_bones=bones)
        assert ctx.rejected_instance_count() - before == 1


def test_a_skeleton_unregistered_behind_the_launch_is_still_served():
    rng = np.random.default_rng(4802)
    bones, n = 100, 9
    parents = forest(rng, bones)
    local = random_poses(rng, n, bones)
    rows = expected_rows(local, parents)
    with runtime.Context(0) as ctx:
        skeleton = ctx.register_skeleton(parents, identity_pose(bones))
        buffers = Buffers(n, bones * 12 + 4)
        d_local, d_out = buffers.up(buffers.host(local)), buffers.up(buffers.host())
        consumers = runtime.PoseBufferConsumers()
        consumers.skeleton, consumers.object_space = skeleton, 1
        ctx.transform_poses_batch(d_local[1].data_ptr(), buffers.row_floats * 4, n, consumers, d_out[1].data_ptr(), buffers.row_floats * 4, stream=buffers.stream())
        ctx.unregister_skeleton(skeleton)                                # stream ordered: behind the launch
        assert np.array_equal(bits(buffers.down(d_out)), bits(buffers.host(rows)))
        assert ctx.rejected_instance_count() == 0


def flag_sets(num_bones):
    """NULL, every other bone, all zero"""
    return [None, (np.arange(num_bones) % 2 == 0).astype(np.uint8) * 255, np.zeros(num_bones, dtype=np.uint8)]


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


@pytest.mark.parametrize("num_bones", [64, 65, 300])
def test_bounds_with_rows_and_alone(num_bones):
    rng = np.random.default_rng(4900 + num_bones)
    parents = forest(rng, num_bones)
    n = 5
    local, additive = random_poses(rng, n, num_bones), random_poses(rng, n, num_bones, scale=(0.8, 1.25))
    with runtime.Context(0) as ctx:
        skeleton = ctx.register_skeleton(parents, identity_pose(num_bones))
        for launch in (dict(), dict(additive_format=ADDITIVE0, additive=additive)):
            plain = check(ctx, local, expected_rows(local, parents, launch.get("additive_format", NONE), additive), skeleton=skeleton, **launch)
            rows = plain[1:1 + n, : num_bones * 12].reshape(n, num_bones, 12)
            for index, flags in enumerate(flag_sets(num_bones)):
                want = expected_boxes(rows, flags)
                out, _, _, boxes, _ = run(ctx, local, skeleton=skeleton, bounds_flags=flags, **launch)
                assert np.array_equal(bits(out), bits(plain)), index                         # rows byte identical with and without bounds
                assert np.array_equal(bits(boxes), bits(want)), (index, boxes, want)
                out, _, _, boxes, _ = run(ctx, local, skeleton=skeleton, bounds_flags=flags, with_rows=False, **launch)
                assert np.array_equal(bits(boxes), bits(want)), (index, "bounds alone", boxes, want)
                assert np.all(out == SENTINEL), index                                       # the would-be row buffer is untouched
            empty = expected_boxes(rows, np.zeros(num_bones, dtype=np.uint8))
            assert np.array_equal(empty[1], np.array([INF, INF, INF, 0, -INF, -INF, -INF, 0], dtype=np.float32))
        assert ctx.rejected_instance_count() == 0


def test_a_captured_launch_replays_after_the_skeleton_table_changed():
    import torch
    rng = np.random.default_rng(5001)
    bones, n = 100, 9
    parents = forest(rng, bones)
    local = random_poses(rng, n, bones)
    rows = expected_rows(local, parents)
    with runtime.Context(0) as ctx:
        skeleton = ctx.register_skeleton(parents, identity_pose(bones))
        unrelated = ctx.register_skeleton(forest(rng, 30), identity_pose(30))
        buffers = Buffers(n, bones * 12 + 4)
        d_local, d_out = buffers.up(buffers.host(local)), buffers.up(buffers.host())
        consumers = runtime.PoseBufferConsumers()
        consumers.skeleton, consumers.object_space = skeleton, 1
        stride = buffers.row_floats * 4
        side = torch.cuda.Stream(device=buffers.device)
        side.wait_stream(torch.cuda.current_stream(buffers.device))
        with torch.cuda.stream(side):
            ctx.transform_poses_batch(d_local[1].data_ptr(), stride, n, consumers, d_out[1].data_ptr(), stride, stream=side.cuda_stream)       # warm-up
            side.synchronize()
            graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graph, stream=side):
                ctx.transform_poses_batch(d_local[1].data_ptr(), stride, n, consumers, d_out[1].data_ptr(), stride, stream=side.cuda_stream)
        first = d_out.cpu().numpy()
        assert np.array_equal(bits(first), bits(buffers.host(rows)))
        ctx.register_skeleton(forest(rng, 50), identity_pose(50))
        ctx.unregister_skeleton(unrelated)
        d_out.fill_(float(SENTINEL))
        graph.replay()
        torch.cuda.synchronize()
        assert np.array_equal(bits(d_out.cpu().numpy()), bits(first))
        del graph
        assert ctx.rejected_instance_count() == 0
