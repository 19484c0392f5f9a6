"""aclhip_skinning_matrices_batch through the C ABI: skinning palettes of pose buffers the caller filled, in both layouts, over local rows
through the matrix walk and over rows taken as they are. The expected rows are the restatement of tests/test_skinning_matrices_oracle.py
(numpy float32 element operations in the header's order), compared on bits wherever the expectation is not a NaN; where it is one the
output must be one. The kernel and the restatement run the same operation order, so there is no tolerance anywhere. Every output buffer is
sentinel filled with a guard row before and behind its rows and strides wider than the rows, so the same comparison holds the bytes behind
the J records, the refused rows and the guards to the sentinel. Every launch has 17 instances: more than one workgroup, an odd count. The
input buffers are asserted unchanged. Needs a GPU."""
import numpy as np
import pytest

from acl_amd import runtime
from test_gpu_pose_buffers import SENTINEL, Buffers, bits, chain, identity_pose
from test_gpu_pose_error import signed_poses
from test_gpu_pose_matrices import batch_poses
from test_pose_error_oracle import forest
from test_pose_matrices_oracle import object_matrices
from test_skinning_matrices_oracle import RECORD_FLOATS, below, mixed_joint_list, palettes_of

pytestmark = pytest.mark.gpu

N = 17
WIDE, TRANSPOSED = runtime.PALETTE_3X4F_64, runtime.PALETTE_3X4F_TRANSPOSED_48
LAYOUTS = [WIDE, TRANSPOSED]
LAYOUT_IDS = {WIDE: "64", TRANSPOSED: "transposed48"}
LANE3_BITS = bits(np.array([0.0, 0.0, 0.0, 1.0], dtype=np.float32))


def random_bind(rng, num_joints):
    """finite inverse bind matrices in the 64 byte layout; lane 3 holds what a caller may have left there: it is ignored"""
    bind = rng.uniform(-2.0, 2.0, size=(num_joints, 4, 4)).astype(np.float32)
    bind[:, :, 3] = rng.normal(size=(num_joints, 4)).astype(np.float32)
    bind[num_joints // 2, 1, 3] = np.nan
    return bind


class Launched:
    pass


def launch(ctx, local, skin=0, skeleton=0, instance_skeletons=None, instance_skins=None, object_space=True, layout=WIDE, row_joints=None, pose_row_bones=None,
           exact_palette_stride=False, stream=None):
    """One launch over `local` ([n, B, 12], or a list of per instance poses) into rows of `row_joints` records; both strides are wider than
    their rows unless exact_palette_stride. Returns a Launched: palettes [n + 2, row floats] with its guard rows, on the host."""
    n = len(local)
    largest = max([pose.shape[0] for pose in local] + [1])
    pose_floats = (pose_row_bones if pose_row_bones is not None else largest) * 12 + 4
    palette_floats = row_joints * RECORD_FLOATS[layout] + (0 if exact_palette_stride else 8)
    buffers = Buffers(n, pose_floats)
    h_local = buffers.host(local, pose_floats)
    d_local = buffers.up(h_local)
    d_palettes = buffers.up(buffers.host(None, palette_floats))
    desc = runtime.SkinningDesc()
    desc.skeleton, desc.skin, desc.object_space, desc.layout = skeleton, skin, 1 if object_space else 0, layout
    if instance_skeletons is not None:
        desc.instance_skeletons = buffers.up(np.asarray(instance_skeletons, dtype=np.uint32)).data_ptr()
    if instance_skins is not None:
        desc.instance_skins = buffers.up(np.asarray(instance_skins, dtype=np.uint32)).data_ptr()
    out = Launched()
    out.buffers, out.tensor = buffers, d_palettes
    out.arguments = (d_local[1].data_ptr(), pose_floats * 4, n, desc, d_palettes[1].data_ptr(), palette_floats * 4)
    ctx.skinning_matrices_batch(*out.arguments, stream=stream if stream is not None else buffers.stream())
    if stream is not None:
        return out
    out.palettes = buffers.down(d_palettes)
    assert np.array_equal(bits(buffers.down(d_local)), bits(h_local))          # the input is only read
    return out


def check(palettes, rows, layout):
    """rows: per instance [J, 4, 4] / [J, 3, 4] or None (refused: the row stays the sentinel). On bits where the expectation is a number,
    a NaN where it is a NaN, the sentinel everywhere else; lane 3 of every 64 byte record is 0, 0, 0, 1."""
    want = np.full(palettes.shape, SENTINEL, dtype=np.float32)
    for i, row in enumerate(rows):
        if row is not None:
            assert row.shape[1:] == ((4, 4) if layout == WIDE else (3, 4))
            want[1 + i, : row.size] = row.reshape(-1)
            if layout == WIDE:
                lanes = bits(palettes[1 + i, : row.size]).reshape(-1, 4, 4)[:, :, 3]
                assert np.array_equal(lanes, np.broadcast_to(LANE3_BITS, lanes.shape)), i
    numbers = ~np.isnan(want)
    assert np.array_equal(bits(palettes)[numbers], bits(want)[numbers]), np.argwhere((bits(palettes) != bits(want)) & numbers)[:8]
    assert np.all(np.isnan(palettes[~numbers]))


SHAPES = [("forest", bones) for bones in (1, 63, 64, 65, 100, 300, 1200)] + [("chain", 200)]
NAN_INSTANCE = 3


@pytest.fixture(scope="module")
def cases():
    """(kind, B) -> (parents, local [N, B, 12], {object_space: object matrices [N, B, 4, 4]}, two skins (joint list or None, IB)), computed once"""
    out = {}
    for kind, num_bones in SHAPES:
        rng = np.random.default_rng(9300 + num_bones)
        parents = forest(rng, num_bones) if kind == "forest" else chain(num_bones)
        local = batch_poses(rng, N, num_bones)
        # one bone with a NaN, one with an infinite scale, a rotation of zeros, a negative zero: all reach the joints of the bone and of what hangs below it
        local[NAN_INSTANCE, num_bones // 2, 1] = np.nan
        local[8, num_bones // 3, 9] = np.inf
        local[11, num_bones - 1, 0:4] = 0.0
        local[12, 0, 10] = -0.0
        joints = mixed_joint_list(rng, num_bones)
        skins = [(None, random_bind(rng, num_bones)), (joints, random_bind(rng, len(joints)))]
        out[(kind, num_bones)] = (parents, local, {space: object_matrices(parents, local, space) for space in (True, False)}, skins)
    return out


@pytest.mark.parametrize("object_space", [True, False], ids=["object", "as-is"])
@pytest.mark.parametrize("layout", LAYOUTS, ids=LAYOUT_IDS.get)
@pytest.mark.parametrize("shape", SHAPES, ids=lambda shape: "%s-%d" % shape)
def test_the_rows_are_the_restatement(cases, shape, layout, object_space):
    """lane stride edges (63 / 64 / 65), 4, 2 and 1 images per workgroup (100 / 300 / 1200 bones), a batch that ends inside a workgroup,
    the deepest schedule (a chain of 200: one transform per step); scales of both signs, a NaN and an infinity; the identity list with
    random matrices, and a list that permutes, drops a quarter of the bones and repeats one"""
    parents, local, objects, skins = cases[shape]
    num_bones = shape[1]
    with runtime.Context(0) as ctx:
        skeleton = ctx.register_skeleton(parents, identity_pose(num_bones))
        before = ctx.negative_scale_count()
        for joints, bind in skins:
            want = palettes_of(objects[object_space], joints, bind, layout)
            # the NaN reaches exactly the joints whose bone hangs below it (in rows taken as they are: the bone's own joints)
            reached = below(parents, num_bones // 2) if object_space else np.arange(num_bones) == num_bones // 2
            bones_of_joints = np.arange(num_bones) if joints is None else joints
            assert np.array_equal(np.isnan(want[NAN_INSTANCE]).any(axis=(1, 2)), reached[bones_of_joints])
            assert not np.isnan(want[0]).any() and not np.isnan(want[4]).any()
            skin = ctx.register_skin(joints, bind, num_bones)
            info = ctx.skin_info(skin)
            assert (info.num_joints, info.num_bones, info.is_identity_joint_list, info.has_inverse_bind) == (len(bones_of_joints), num_bones, 1 if joints is None else 0, 1)
            out = launch(ctx, local, skin=skin, skeleton=skeleton, object_space=object_space, layout=layout, row_joints=len(bones_of_joints))
            check(out.palettes, list(want), layout)
            got = out.palettes[1 + NAN_INSTANCE, : want[NAN_INSTANCE].size].reshape(want[NAN_INSTANCE].shape)
            assert np.array_equal(np.isnan(got).any(axis=(1, 2)), reached[bones_of_joints])
        assert ctx.negative_scale_count() == before            # there is no qvv_mul here
        assert ctx.rejected_instance_count() == 0


@pytest.mark.parametrize("layout", LAYOUTS, ids=LAYOUT_IDS.get)
def test_output_quad_edges(cases, layout):
    """65 bones; 3 J and 4 J output quads on both sides of 64 and 128, one joint, and more joints than bones through duplicates; skins
    without matrices go through the product too"""
    parents, local, objects, _ = cases[("forest", 65)]
    rng = np.random.default_rng(9401)
    with runtime.Context(0) as ctx:
        skeleton = ctx.register_skeleton(parents, identity_pose(65))
        for num_joints in (1, 16, 17, 21, 22, 43, 65, 130):
            joints = rng.integers(0, 65, size=num_joints).astype(np.uint32)
            bind = random_bind(rng, num_joints) if num_joints != 43 else None
            skin = ctx.register_skin(joints, bind, 65)
            out = launch(ctx, local, skin=skin, skeleton=skeleton, layout=layout, row_joints=num_joints)
            check(out.palettes, list(palettes_of(objects[True], joints, bind, layout)), layout)
        # the identity list without matrices: every joint is its bone's object matrix
        skin = ctx.register_skin(None, None, 65)
        out = launch(ctx, local, skin=skin, skeleton=skeleton, layout=layout, row_joints=65)
        check(out.palettes, list(palettes_of(objects[True], None, None, layout)), layout)
        assert ctx.rejected_instance_count() == 0


def test_skeletons_and_skins_per_instance():
    """two bone counts and three joint counts inside one workgroup: a row is written up to its own J records"""
    rng = np.random.default_rng(9501)
    small, large = 40, 100
    parents = {small: forest(rng, small, root_chance=0.2), large: forest(rng, large)}
    skins = {"small": (small, rng.integers(0, small, size=25).astype(np.uint32)), "large": (large, None), "many": (large, rng.integers(0, large, size=130).astype(np.uint32))}
    binds = {name: random_bind(rng, bones if joints is None else len(joints)) for name, (bones, joints) in skins.items()}
    with runtime.Context(0) as ctx:
        skeletons = {bones: ctx.register_skeleton(parents[bones], identity_pose(bones)) for bones in (small, large)}
        handles = {name: ctx.register_skin(joints, binds[name], bones) for name, (bones, joints) in skins.items()}
        which = ["large", "small", "many", "large", "small", "many", "large", "small", "large", "small", "small", "many", "large", "large", "small", "many", "small"]
        assert len(which) == N
        local = [signed_poses(rng, 1, skins[name][0])[0] for name in which]
        for layout in LAYOUTS:
            for object_space in (True, False):
                # a launch wide skeleton and skin are ignored next to the lists
                out = launch(ctx, local, skin=handles["small"], skeleton=skeletons[small], instance_skeletons=[skeletons[skins[name][0]] for name in which],
                             instance_skins=[handles[name] for name in which], object_space=object_space, layout=layout, row_joints=130)
                rows = [palettes_of(object_matrices(parents[skins[name][0]], pose, object_space), skins[name][1], binds[name], layout) for name, pose in zip(which, local)]
                check(out.palettes, rows, layout)
                assert np.all(out.palettes[2, 25 * RECORD_FLOATS[layout]:] == SENTINEL)
        assert ctx.rejected_instance_count() == 0


@pytest.mark.parametrize("layout", LAYOUTS, ids=LAYOUT_IDS.get)
def test_refusals_leave_the_row_and_are_counted(layout):
    import torch
    rng = np.random.default_rng(9601)
    small, large = 40, 100
    parents = {small: forest(rng, small, root_chance=0.2), large: forest(rng, large)}
    record = RECORD_FLOATS[layout]
    with runtime.Context(0) as ctx:
        skeletons = {bones: ctx.register_skeleton(parents[bones], identity_pose(bones)) for bones in (small, large)}
        flat = ctx.register_skeleton(None, identity_pose(small))                        # no hierarchy
        joints = {small: rng.integers(0, small, size=30).astype(np.uint32), large: rng.integers(0, large, size=90).astype(np.uint32)}
        binds = {bones: random_bind(rng, len(joints[bones])) for bones in (small, large)}
        skins = {bones: ctx.register_skin(joints[bones], binds[bones], bones) for bones in (small, large)}
        retired = ctx.register_skin(joints[small], binds[small], small)
        ctx.unregister_skin(retired)
        torch.cuda.synchronize()

        def row(bones, pose, object_space=True):
            return palettes_of(object_matrices(parents[bones], pose, object_space), joints[bones], binds[bones], layout)

        # the null skin, an unknown one, a retired one, a skin made for another bone count; an unknown skeleton; object space without a hierarchy
        local = [signed_poses(rng, 1, small)[0] for _ in range(N)]
        skin_ids, skeleton_ids = [skins[small]] * N, [skeletons[small]] * N
        skin_ids[1], skin_ids[2], skin_ids[4], skin_ids[7], skin_ids[16] = 0, 0x00ABCDEF, retired, skins[large], 0xFFFFFFFF
        skeleton_ids[9], skeleton_ids[10], skeleton_ids[12] = 0, flat, 0x00ABCDEF
        refused = [skin != skins[small] or skeleton != skeletons[small] for skin, skeleton in zip(skin_ids, skeleton_ids)]
        before = ctx.rejected_instance_count()
        out = launch(ctx, local, instance_skeletons=skeleton_ids, instance_skins=skin_ids, layout=layout, row_joints=90)
        check(out.palettes, [None if no else row(small, pose) for no, pose in zip(refused, local)], layout)
        assert ctx.rejected_instance_count() - before == sum(refused) == 8
        # rows taken as they are need no hierarchy: the skeleton without one is served
        before = ctx.rejected_instance_count()
        out = launch(ctx, local, instance_skeletons=skeleton_ids, instance_skins=skin_ids, object_space=False, layout=layout, row_joints=90)
        check(out.palettes, [None if no and skeleton != flat else row(small, pose, False) for no, skeleton, pose in zip(refused, skeleton_ids, local)], layout)
        assert ctx.rejected_instance_count() - before == 7

        # a palette row one record too small for the larger skin, a pose row too small for the larger skeleton: refused, in front of any load
        which = [small, large] * 8 + [small]
        local = [signed_poses(rng, 1, bones)[0] for bones in which]
        skeleton_ids, skin_ids = [skeletons[bones] for bones in which], [skins[bones] for bones in which]
        rows = [None if bones == large else row(bones, pose) for bones, pose in zip(which, local)]
        before = ctx.rejected_instance_count()
        out = launch(ctx, local, instance_skeletons=skeleton_ids, instance_skins=skin_ids, layout=layout, row_joints=89, exact_palette_stride=True)
        assert out.palettes.shape[1] == 89 * record
        check(out.palettes, rows, layout)
        assert ctx.rejected_instance_count() - before == 8
        # (the stride that holds the last record serves them)
        out = launch(ctx, local, instance_skeletons=skeleton_ids, instance_skins=skin_ids, layout=layout, row_joints=90, exact_palette_stride=True)
        check(out.palettes, [row(bones, pose) for bones, pose in zip(which, local)], layout)
        assert ctx.rejected_instance_count() - before == 8
        before = ctx.rejected_instance_count()
        out = launch(ctx, [pose[:small] for pose in local], instance_skeletons=skeleton_ids, instance_skins=skin_ids, layout=layout, row_joints=90, pose_row_bones=small)
        check(out.palettes, rows, layout)
        assert ctx.rejected_instance_count() - before == 8

        # every instance refused
        before = ctx.rejected_instance_count()
        out = launch(ctx, local, skin=retired, instance_skeletons=skeleton_ids, layout=layout, row_joints=90)
        check(out.palettes, [None] * N, layout)
        assert ctx.rejected_instance_count() - before == N


def test_a_skin_retired_behind_a_launch_still_serves_it_and_its_handle_is_reused(cases):
    import torch
    parents, local, objects, skins = cases[("forest", 100)]
    joints, bind = skins[1]
    with runtime.Context(0) as ctx:
        skeleton = ctx.register_skeleton(parents, identity_pose(100))
        keeps = ctx.register_skin(None, None, 100)
        skin = ctx.register_skin(joints, bind, 100)
        stream = torch.cuda.current_stream(torch.device("cuda:0")).cuda_stream
        # enqueued, then retired without a wait in between: the launch is served
        served = launch(ctx, local, skin=skin, skeleton=skeleton, layout=TRANSPOSED, row_joints=len(joints), stream=stream)
        ctx.unregister_skin(skin)
        check(served.buffers.down(served.tensor), list(palettes_of(objects[True], joints, bind, TRANSPOSED)), TRANSPOSED)
        with pytest.raises(runtime.AclHipError):
            ctx.skin_info(skin)
        # the next launch refuses the handle
        before = ctx.rejected_instance_count()
        out = launch(ctx, local, skin=skin, skeleton=skeleton, layout=TRANSPOSED, row_joints=len(joints))
        check(out.palettes, [None] * N, TRANSPOSED)
        assert ctx.rejected_instance_count() - before == N
        # a registration reuses it, with its own content
        torch.cuda.synchronize()
        other_joints = joints[::-1].copy()
        again = ctx.register_skin(other_joints, None, 100)
        assert again == skin and again != keeps
        before = ctx.rejected_instance_count()
        out = launch(ctx, local, skin=again, skeleton=skeleton, layout=TRANSPOSED, row_joints=len(joints))
        check(out.palettes, list(palettes_of(objects[True], other_joints, None, TRANSPOSED)), TRANSPOSED)
        assert ctx.rejected_instance_count() == before


def test_a_captured_launch_replays_with_the_bytes_of_the_direct_one(cases):
    import torch
    parents, local, objects, skins = cases[("forest", 100)]
    joints, bind = skins[1]
    want = list(palettes_of(objects[True], joints, bind, TRANSPOSED))
    rng = np.random.default_rng(9701)
    with runtime.Context(0) as ctx:
        skeleton = ctx.register_skeleton(parents, identity_pose(100))
        skin = ctx.register_skin(joints, bind, 100)
        direct = launch(ctx, local, skin=skin, skeleton=skeleton, layout=TRANSPOSED, row_joints=len(joints))
        check(direct.palettes, want, TRANSPOSED)
        device = direct.buffers.device
        side = torch.cuda.Stream(device=device)
        side.wait_stream(torch.cuda.current_stream(device))
        with torch.cuda.stream(side):
            captured = launch(ctx, local, skin=skin, skeleton=skeleton, layout=TRANSPOSED, row_joints=len(joints), stream=side.cuda_stream)      # warm-up
            side.synchronize()
            captured.tensor.fill_(float(SENTINEL))
            side.synchronize()
            graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graph, stream=side):
                ctx.skinning_matrices_batch(*captured.arguments, stream=side.cuda_stream)
        # other skins come and go: the table does not move
        others = [ctx.register_skin(None, random_bind(rng, 100), 100) for _ in range(3)]
        ctx.unregister_skin(others[1])
        torch.cuda.synchronize()
        others.append(ctx.register_skin(rng.integers(0, 100, size=7).astype(np.uint32), None, 100))
        with torch.cuda.stream(side):
            graph.replay()
        torch.cuda.synchronize()
        replayed = captured.tensor.cpu().numpy()
        check(replayed, want, TRANSPOSED)
        assert np.array_equal(bits(replayed), bits(direct.palettes))
        del graph
        assert ctx.rejected_instance_count() == 0
