"""The launches that read poses or a reference pose from a CALLER, on inputs outside the range in which sqrt_rn_short / rcp_rn_short are
proven (aclhip_device.h): the counterpart of tests/test_gpu_exact_math.py for aclhip_transform_poses_batch, aclhip_blend_poses_batch,
aclhip_inverse_transform_poses_batch, the fused launches onto a caller's base_poses buffer and a registered skeleton's reference pose.
tests/test_caller_pose_ranges_oracle.py builds every input, every expected row (the oracle's functions, composed as the launches' own
test files compose them) and the conditions they meet -- finite rows, no normalize argument of 0, at least 500 normalizes per test with
an argument in (0, 2^-96) --; each test here fetches its cases from there BY ITS OWN NAME (GPU_TESTS). Every comparison is np.array_equal
over uint32 views of whole sentinel guarded buffers, no tolerance; 65 bones (two lane passes) and 100 bones (4 instances per workgroup),
9 instances (the batch ends inside a workgroup), out of place and in place where a launch has both.

The last three tests hand the pose buffer launches rows with NaN, +inf and an all-zero rotation in three of the nine instances, out
of place and in place: the other six and their boxes are bit identical to the launch over clean rows, a poisoned row has the oracle's
NaN mask and its bits elsewhere (NaN payloads differ between x86 and the device), and a box ignores a NaN coordinate (include/aclhip.h).

What these tests catch was measured once, on scratch builds that are not part of the repository, with one decision at a time switched
to the short forms (DESIGN 5 keeps the conclusion): transform_poses_kernel's walk fails test_transform_object_space_alone[gap], all six
test_transform_additive and test_transform_bounds; the inverse kernel's normalize fails test_inverse_to_local_space[gap] and the three
test_inverse_make_additive; blend_normalize_rotations fails the four test_blend and test_gap_reference_pose[masked]; the base buffer rule
of the unmapped, mapped and masked fused kernels fails the three test_fused_onto_a_gap_base_buffer of its launch each; a skeleton flag
that registration never clears fails test_gap_reference_pose[mapped], [masked_onto_base_clip] and [bone]. blend_poses_kernel's WALK with
the short forms fails nothing, and cannot: test_caller_pose_ranges_oracle.py::test_the_walk_behind_a_blend_never_meets_the_gap. Needs a GPU."""
import itertools

import numpy as np
import pytest

from acl_amd import runtime
import test_caller_pose_ranges_oracle as oc
import test_gpu_blend_masks as bm
import test_gpu_bone_object as bo
import test_gpu_pose_buffer_blend as bl
import test_gpu_pose_buffer_inverse as inv
import test_gpu_pose_buffers as pb
import test_gpu_skeleton_poses as sk
from test_gpu_pose_buffers import SENTINEL, bits, identity_pose

pytestmark = pytest.mark.gpu

NONE, RELATIVE, ADDITIVE0, ADDITIVE1 = oc.NONE, oc.RELATIVE, oc.ADDITIVE0, oc.ADDITIVE1
WEIGHTED, LAYERED = oc.WEIGHTED, oc.LAYERED
N, INF = oc.N, np.float32(np.inf)


def cases_of(request):
    """the cases of the running test, looked up by its name: the ones the CPU file asserts its conditions for; both shapes are among them"""
    cases = oc.GPU_TESTS[request.node.name][1]()
    assert {len(case.parents if hasattr(case, "parents") else case.rig.parents) for case in cases} == set(oc.SHAPES)
    return cases


# ---- a. aclhip_transform_poses_batch --------------------------------------------------------------------------------------------------

def check_transform(case):
    num_bones = len(case.parents)
    launch = dict(additive_format=case.additive_format, additive=case.additive) if case.additive_format != NONE else {}
    with runtime.Context(0) as ctx:
        skeleton = ctx.register_skeleton(case.parents, identity_pose(num_bones))
        apart = pb.check(ctx, case.local, case.rows, skeleton=skeleton, **launch)
        within, local_after, _, _, _ = pb.run(ctx, case.local, skeleton=skeleton, in_place=True, **launch)
        assert np.array_equal(bits(within), bits(apart)) and np.array_equal(bits(local_after), bits(apart)), num_bones
        assert ctx.rejected_instance_count() == 0 and ctx.negative_scale_count() == 0


@pytest.mark.parametrize("klass", ["gap", "large"])
def test_transform_object_space_alone(request, klass):
    for case in cases_of(request):
        check_transform(case)


@pytest.mark.parametrize("special_buffer,additive_format", list(itertools.product(("local", "additive"), oc.FORMATS)))
def test_transform_additive(request, special_buffer, additive_format):
    """RELATIVE / ADDITIVE0 / ADDITIVE1 with the gap class in the local buffer, and with it in the additive buffer"""
    for case in cases_of(request):
        check_transform(case)


@pytest.mark.parametrize("additive_format", oc.FORMATS)
def test_transform_additive_large(request, additive_format):
    for case in cases_of(request):
        check_transform(case)


def test_transform_bounds(request):
    """boxes bit equal to the minimum / maximum of the EXPECTED rows: next to the rows out of place and in place, and alone"""
    for case in cases_of(request):
        num_bones = len(case.parents)
        want_rows = np.stack(case.rows)
        with runtime.Context(0) as ctx:
            skeleton = ctx.register_skeleton(case.parents, identity_pose(num_bones))
            for index, flags in enumerate(pb.flag_sets(num_bones)):
                want = pb.expected_boxes(want_rows, flags)
                out, _, _, boxes, buffers = pb.run(ctx, case.local, skeleton=skeleton, bounds_flags=flags)
                assert np.array_equal(bits(out), bits(buffers.host(case.rows))), (num_bones, index)
                assert np.array_equal(bits(boxes), bits(want)), (num_bones, index, boxes, want)
                within, local_after, _, boxes, _ = pb.run(ctx, case.local, skeleton=skeleton, bounds_flags=flags, in_place=True)
                assert np.array_equal(bits(within), bits(out)) and np.array_equal(bits(local_after), bits(out)), (num_bones, index, "in place")
                assert np.array_equal(bits(boxes), bits(want)), (num_bones, index, "in place", boxes, want)
                out, _, _, boxes, _ = pb.run(ctx, case.local, skeleton=skeleton, bounds_flags=flags, with_rows=False)
                assert np.array_equal(bits(boxes), bits(want)), (num_bones, index, "bounds alone")
                assert np.all(out == SENTINEL)
            assert ctx.rejected_instance_count() == 0


# ---- b. aclhip_blend_poses_batch ------------------------------------------------------------------------------------------------------

def check_blend(case, num_buffers, mode):
    num_bones = len(case.parents)
    with runtime.Context(0) as ctx:
        skeleton = ctx.register_skeleton(case.parents, identity_pose(num_bones))
        registered = np.array([0] + [ctx.register_blend_mask(mask) for mask in case.masks], dtype=np.uint32)
        handles = registered[case.handles + 1]                          # -1: the null handle
        for object_space, rows in ((False, case.local), (True, case.object_rows)):
            common = dict(handles=handles, skeleton=skeleton, object_space=object_space)
            apart = bl.check(ctx, case.inputs, case.weights, mode, rows, **common)
            for target in (0, num_buffers - 1):
                done = bl.Launch(ctx, case.inputs, case.weights, mode, in_place=target, **common).enqueue()
                out = done.out()
                assert np.array_equal(bits(out[:, : num_bones * 12]), bits(apart[:, : num_bones * 12])), (num_bones, object_space, target)
                assert np.all(out[:, num_bones * 12:] == SENTINEL) and done.inputs_unchanged()
        assert ctx.rejected_instance_count() == 0 and ctx.negative_scale_count() == 0


@pytest.mark.parametrize("num_buffers,mode", list(itertools.product((2, 4), (WEIGHTED, LAYERED))))
def test_blend(request, num_buffers, mode):
    """one buffer of gap class rotations among in range ones, and every buffer gap class; local and object space"""
    for case in cases_of(request):
        check_blend(case, num_buffers, mode)


@pytest.mark.parametrize("num_buffers,mode", list(itertools.product((2, 4), (WEIGHTED, LAYERED))))
def test_blend_large(request, num_buffers, mode):
    for case in cases_of(request):
        check_blend(case, num_buffers, mode)


# ---- c. aclhip_inverse_transform_poses_batch ------------------------------------------------------------------------------------------

def check_inverse(case):
    num_bones = len(case.parents)
    launch = dict(additive_format=case.additive_format, base=case.base) if case.additive_format != NONE else {}
    with runtime.Context(0) as ctx:
        skeleton = ctx.register_skeleton(case.parents, identity_pose(num_bones))
        apart = inv.check(ctx, case.source, case.rows, skeleton=skeleton, **launch)
        within = inv.check(ctx, case.source, case.rows, skeleton=skeleton, in_place=True, **launch)
        assert np.array_equal(bits(within), bits(apart)), num_bones
        assert ctx.rejected_instance_count() == 0 and ctx.negative_scale_count() == 0


@pytest.mark.parametrize("klass", ["gap", "large"])
def test_inverse_to_local_space(request, klass):
    """every object space rotation 2^-35 .. 2^-26 long: the product with the parent's conjugate is what the gap holds"""
    for case in cases_of(request):
        check_inverse(case)


@pytest.mark.parametrize("additive_format", oc.FORMATS)
def test_inverse_make_additive(request, additive_format):
    for case in cases_of(request):
        check_inverse(case)


# ---- d. the fused launches onto a caller's base_poses buffer --------------------------------------------------------------------------

class UnmappedBatch(sk.Batch):
    """sk.Batch through aclhip_decompress_poses_batch"""

    def launch(self, clips, times):
        torch = self.torch
        self.buffer = torch.full((self.n + 2, self.row_floats), float(SENTINEL), dtype=torch.float32, device=self.device)
        self.ctx.decompress_poses_batch(self.up(clips, np.uint32), self.up(times, np.float32), self.n, self.buffer[1].data_ptr(), self.row_floats * 4, self.consumers,
                                        stream=torch.cuda.current_stream(self.device).cuda_stream)
        return self


def masked_batch(ctx, the, num_bones, skeleton, clip_handles, maps, masks):
    """the masked blend of the rig's first two clips, each with its own map, as oc.masked_members / oc.instance_masks_of describe it"""
    batch = bm.MaskedBatch(ctx, N, num_bones)
    consumers, mapping = batch.consumers, batch.mapping
    consumers.object_space, consumers.num_blend_clips = 1, 2
    consumers.blend_clips, consumers.blend_sample_times, consumers.blend_weights = batch.up(np.full((N, 1), clip_handles[1]), np.uint32), batch.up(the.times[1].reshape(N, 1), np.float32), batch.up(the.weights, np.float32)
    mapping.skeleton, mapping.map, mapping.blend_maps = skeleton, maps[0], batch.up(np.full((N, 1), maps[1]), np.uint32)
    batch.masking.mode, batch.masking.instance_masks = WEIGHTED, batch.up(masks[the.handles + 1], np.uint32)
    return batch


@pytest.mark.parametrize("launch,additive_format", list(itertools.product(("unmapped", "mapped", "masked"), oc.FORMATS)))
def test_fused_onto_a_gap_base_buffer(request, launch, additive_format):
    """the base buffer's non-root rotations are gap class: decode, oracle_apply_additive_to_base, oracle_local_to_object_space"""
    for case in cases_of(request):
        the = case.rig
        num_bones = len(the.parents)
        with runtime.Context(0) as ctx:
            if launch == "unmapped":
                handle = ctx.register_clip(the.whole.blob)
                ctx.set_clip_hierarchy(handle, the.parents)
                batch = UnmappedBatch(ctx, N, num_bones)
                clips, times = np.full(N, handle), the.times[3]
            else:
                clip_handles = [ctx.register_clip(clip.blob) for clip in the.clips]
                maps = [ctx.register_track_map(table, num_bones) for table in the.tables]
                skeleton = ctx.register_skeleton(the.parents, the.references["unit"])
                clips, times = np.full(N, clip_handles[0]), the.times[0]
                if launch == "mapped":
                    batch = sk.Batch(ctx, N, num_bones)
                    batch.mapping.skeleton, batch.mapping.map = skeleton, maps[0]
                else:
                    masks = np.array([0] + [ctx.register_blend_mask(mask) for mask in the.masks], dtype=np.uint32)
                    batch = masked_batch(ctx, the, num_bones, skeleton, clip_handles, maps, masks)
            batch.consumers.object_space, batch.consumers.additive_format = 1, additive_format
            batch.consumers.base_poses, batch.consumers.base_pose_stride_bytes = batch.up(the.base, np.float32), num_bones * 48
            got = batch.launch(clips, times).result()
            want = batch.expected(case.rows)
            assert np.array_equal(bits(got), bits(want)), (num_bones, np.argwhere(bits(got) != bits(want))[:8])
            assert ctx.rejected_instance_count() == 0 and ctx.negative_scale_count() == 0


# ---- e. a registered skeleton whose reference pose has gap class rotations ------------------------------------------------------------

@pytest.mark.parametrize("launch", ["mapped", "masked", "masked_onto_base_clip", "bone"])
def test_gap_reference_pose(request, launch):
    """aclhip_get_skeleton_info does not report the skeleton's short exact bit: the bit comparison is the assertion that registration
    cleared it. "dropped" maps: reference rotations fill slots and are walked. Each launch runs a second time over the otherwise equal
    skeleton with unit reference rotations (the short forms' side of the decision, covered elsewhere): a control."""
    for gap_case in cases_of(request):
        the = gap_case.rig
        num_bones = len(the.parents)
        for reference_class in ("gap", "unit"):
            case = oc.skeleton_case(num_bones, launch, reference_class)
            with runtime.Context(0) as ctx:
                clip_handles = [ctx.register_clip(clip.blob) for clip in the.clips]
                maps = [ctx.register_track_map(table, num_bones) for table in the.tables]
                skeleton = ctx.register_skeleton(the.parents, case.reference)
                clips, times = np.full(N, clip_handles[0], dtype=np.uint32), the.times[0]
                if launch == "bone":
                    # every slot once per instance time: the bones below a filled slot among them
                    slots = np.tile(np.arange(num_bones, dtype=np.uint32), N)
                    mapping = runtime.PoseMapping()
                    mapping.skeleton, mapping.map = skeleton, maps[0]
                    got = bo.launch_requests(ctx, np.repeat(clips, num_bones), np.repeat(times, num_bones), slots, mapping=mapping)
                    want = np.stack(case.rows).reshape(N * num_bones, 12)
                else:
                    if launch == "mapped":
                        batch = sk.Batch(ctx, N, num_bones)
                        batch.mapping.skeleton, batch.mapping.map = skeleton, maps[0]
                        batch.consumers.object_space = 1
                    else:
                        masks = np.array([0] + [ctx.register_blend_mask(mask) for mask in the.masks], dtype=np.uint32)
                        batch = masked_batch(ctx, the, num_bones, skeleton, clip_handles, maps, masks)
                        if launch == "masked_onto_base_clip":
                            batch.consumers.additive_format = ADDITIVE0
                            batch.consumers.base_clips, batch.consumers.base_sample_times = batch.up(np.full(N, clip_handles[2]), np.uint32), batch.up(the.times[2], np.float32)
                            batch.mapping.base_maps = batch.up(np.full(N, maps[2]), np.uint32)
                    got, want = batch.launch(clips, times).result(), batch.expected(case.rows)
                assert np.array_equal(bits(got), bits(want)), (num_bones, reference_class, np.argwhere(bits(got) != bits(want))[:8])
                assert ctx.rejected_instance_count() == 0 and ctx.negative_scale_count() == 0


# ---- f. non-finite rows: the pose buffer launches -------------------------------------------------------------------------------------

CLEAN = [i for i in range(N) if i not in oc.POISONED]


def assert_same_class(got, want, what):
    """NaN where the oracle's value is NaN, its bits everywhere else"""
    nan = np.isnan(want)
    assert np.array_equal(np.isnan(got), nan), (what, np.argwhere(np.isnan(got) != nan)[:8])
    assert np.array_equal(bits(got)[~nan], bits(want)[~nan]), (what, np.argwhere((bits(got) != bits(want)) & ~nan)[:8])


def boxes_ignoring_nan(written, flags):
    """written: the output buffer with its guard rows. Per component np.fmin / np.fmax over the counted translations, from +inf / -inf: a
    NaN coordinate is ignored, a component whose counted coordinates are all NaN keeps the empty value."""
    out = np.full((N + 2, 8), SENTINEL, dtype=np.float32)
    counted = np.ones(oc.POISON_BONES, dtype=bool) if flags is None else flags != 0
    for i in range(N):
        translations = written[1 + i, : oc.POISON_BONES * 12].reshape(oc.POISON_BONES, 12)[counted, 4:7]
        box = np.zeros(8, dtype=np.float32)
        box[0:3] = np.fmin.reduce(np.concatenate([np.full((1, 3), INF, dtype=np.float32), translations]), axis=0)
        box[4:7] = np.fmax.reduce(np.concatenate([np.full((1, 3), -INF, dtype=np.float32), translations]), axis=0)
        out[1 + i] = box
    return out


def check_poisoned_launch(case, launch_rows, launch_boxes, targets):
    """launch_rows(inputs, flags, target) -> (the records of the output buffer with its guard rows, [N + 2, B * 12], boxes): it asserts that
    everything behind the records kept the prefill; launch_boxes(inputs, flags) -> boxes of the launch without rows (which has no in place
    form). flags: "none" (no bounds), None (every bone counts) or uint8 flags. targets: None (out of place) first, then what the launch
    takes to run in place -- the row being rewritten is the poisoned one, or its clean neighbour's."""
    guards_and_clean = [0, N + 1] + [1 + i for i in CLEAN]
    want = np.full((N + 2, oc.POISON_BONES * 12), SENTINEL, dtype=np.float32)
    want[1:1 + N] = np.stack(case.rows).reshape(N, -1)
    plain = None
    for target in targets:
        rows, _ = launch_rows(case.poisoned, "none", target)
        assert_same_class(rows, want, ("rows", target))                                       # the guard rows included
        if plain is None:
            plain = rows
        assert np.array_equal(bits(rows), bits(plain)), target                                # in place: the bits of out of place
        clean_rows, _ = launch_rows(case.clean, "none", target)
        assert np.isfinite(clean_rows[1:1 + N]).all()
        assert np.array_equal(bits(rows[guards_and_clean]), bits(clean_rows[guards_and_clean])), target      # isolation
        for flags in (None, case.flags):
            out, boxes = launch_rows(case.poisoned, flags, target)
            assert np.array_equal(bits(out), bits(plain)), target                             # rows bit identical with and without bounds
            assert np.array_equal(bits(boxes), bits(boxes_ignoring_nan(out, flags))), (target, flags is None, boxes)
            _, clean_boxes = launch_rows(case.clean, flags, target)
            assert np.array_equal(bits(boxes[guards_and_clean]), bits(clean_boxes[guards_and_clean])), target   # isolation of the boxes
            if target is None:
                assert np.array_equal(bits(launch_boxes(case.poisoned, flags)), bits(boxes)), "bounds alone"
            if flags is not None:
                # the header's statement, seen on this input: the parent's rotation spreads instance 1's NaN over the three coordinates of
                # the poisoned bone, and its descendants add it to theirs -- every coordinate case.flags counts is NaN, the empty value stays
                assert np.array_equal(boxes[2], np.array([INF, INF, INF, 0, -INF, -INF, -INF, 0], dtype=np.float32))
                assert np.isfinite(boxes[[1 + i for i in CLEAN]]).all()


def test_poisoned_instances_leave_their_neighbours_alone_transform():
    case = oc.poison_case("transform")
    records = oc.POISON_BONES * 12
    with runtime.Context(0) as ctx:
        skeleton = ctx.register_skeleton(case.parents, identity_pose(oc.POISON_BONES))

        def launch_rows(local, flags, target):
            out, local_after, local_before, boxes, _ = pb.run(ctx, local, skeleton=skeleton, bounds_flags=flags, in_place=target is not None)
            assert np.array_equal(bits(local_after), bits(out if target is not None else local_before))
            assert np.all(out[:, records:] == SENTINEL)
            return out[:, :records], boxes

        def launch_boxes(local, flags):
            out, _, _, boxes, _ = pb.run(ctx, local, skeleton=skeleton, bounds_flags=flags, with_rows=False)
            assert np.all(out == SENTINEL)
            return boxes

        check_poisoned_launch(case, launch_rows, launch_boxes, [None, True])
        assert ctx.rejected_instance_count() == 0


def test_poisoned_instances_leave_their_neighbours_alone_blend():
    """in place on buffer 0, which holds the poison, and on buffer 1"""
    case = oc.poison_case("blend")
    records = oc.POISON_BONES * 12
    with runtime.Context(0) as ctx:
        skeleton = ctx.register_skeleton(case.parents, identity_pose(oc.POISON_BONES))

        def launch_rows(inputs, flags, target):
            done = bl.Launch(ctx, inputs, case.weights, WEIGHTED, skeleton=skeleton, object_space=True, bounds_flags=flags, in_place=target).enqueue()
            out = done.out()
            assert done.inputs_unchanged()                                                   # (every input but an in place target)
            assert np.all(out[:, records:] == SENTINEL)
            return out[:, :records], (done.boxes() if not isinstance(flags, str) else None)

        def launch_boxes(inputs, flags):
            done = bl.Launch(ctx, inputs, case.weights, WEIGHTED, skeleton=skeleton, object_space=True, bounds_flags=flags, with_rows=False).enqueue()
            assert np.all(done.out() == SENTINEL)
            return done.boxes()

        check_poisoned_launch(case, launch_rows, launch_boxes, [None, 0, 1])
        assert ctx.rejected_instance_count() == 0


def test_poisoned_instances_leave_their_neighbours_alone_inverse():
    """no boxes: isolation and the class comparison, out of place and in place"""
    case = oc.poison_case("inverse")
    guards_and_clean = [0, N + 1] + [1 + i for i in CLEAN]
    with runtime.Context(0) as ctx:
        skeleton = ctx.register_skeleton(case.parents, identity_pose(oc.POISON_BONES))
        for in_place in (False, True):
            out, untouched, _ = inv.run(ctx, case.poisoned, skeleton=skeleton, in_place=in_place)
            want = untouched.copy()
            want[1:1 + N, : oc.POISON_BONES * 12] = np.stack(case.rows).reshape(N, -1)
            assert_same_class(out, want, in_place)
            clean, _, _ = inv.run(ctx, case.clean, skeleton=skeleton, in_place=in_place)
            assert np.isfinite(clean[1:1 + N, : oc.POISON_BONES * 12]).all()
            assert np.array_equal(bits(out[guards_and_clean]), bits(clean[guards_and_clean]))
        assert ctx.rejected_instance_count() == 0
