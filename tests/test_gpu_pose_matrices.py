"""aclhip_pose_matrices_batch through the C ABI: 3x4 matrices of pose buffers the caller filled, in local space and through the matrix walk.
The expected rows are the restatement of tests/test_pose_matrices_oracle.py (numpy float32 element operations in the header's order),
compared on bits wherever the expectation is not a NaN; where it is one the output must be one. The kernel and the restatement run the
same operation order, so there is no tolerance anywhere. Every output buffer is sentinel filled with a guard row before and behind its
rows and strides wider than the rows, so the same comparison holds the bytes behind 64 B, the refused rows and the guards to the sentinel.
Every launch has 17 instances: more than one workgroup, an odd count. The input buffers are asserted unchanged. Needs a GPU."""
import numpy as np
import pytest

from acl_amd import runtime
from test_gpu_pose_buffers import SENTINEL, Buffers, bits, chain, identity_pose
from test_gpu_pose_error import signed_poses
from test_pose_error_oracle import forest
from test_pose_matrices_oracle import object_matrices

pytestmark = pytest.mark.gpu

N = 17
LANE3_BITS = bits(np.array([0.0, 0.0, 0.0, 1.0], dtype=np.float32))


def batch_poses(rng, n, num_bones):
    """signed_poses; from 200 bones on the rotations have length 1 instead of [0.5, 2] and the scale magnitudes are drawn from
    2^U(-1/4, 1/4) instead of 2^U(-2, 2): along the deep hierarchies of these shapes the products of the matrices -- and the squares the
    error takes of them -- then stay finite in float32"""
    poses = signed_poses(rng, n, num_bones)
    if num_bones >= 200:
        poses[..., 0:4] /= np.linalg.norm(poses[..., 0:4], axis=2, keepdims=True)
        poses[..., 8:11] = np.copysign(np.abs(poses[..., 8:11]) ** np.float32(0.125), poses[..., 8:11])
    return poses


class Launched:
    pass


def launch(ctx, local, skeleton=0, instance_skeletons=None, object_space=True, local_row_bones=None, matrix_row_bones=None, stream=None):
    """One launch over `local` ([n, B, 12], or a list of per instance poses); both strides are wider than their rows. Returns a Launched:
    matrices [n + 2, row floats] with its guard rows, on the host."""
    n = len(local)
    largest = max([pose.shape[0] for pose in local] + [1])
    local_floats = (local_row_bones if local_row_bones is not None else largest) * 12 + 4
    matrix_floats = (matrix_row_bones if matrix_row_bones is not None else largest) * 16 + 8
    buffers = Buffers(n, local_floats)
    h_local = buffers.host(local, local_floats)
    d_local = buffers.up(h_local)
    d_matrices = buffers.up(buffers.host(None, matrix_floats))
    desc = runtime.PoseMatricesDesc()
    desc.skeleton, desc.object_space, desc.layout = skeleton, 1 if object_space else 0, runtime.MATRIX_3X4F_64
    if instance_skeletons is not None:
        desc.instance_skeletons = buffers.up(np.asarray(instance_skeletons, dtype=np.uint32)).data_ptr()
    out = Launched()
    out.buffers, out.tensor = buffers, d_matrices
    out.arguments = (d_local[1].data_ptr(), local_floats * 4, n, desc, d_matrices[1].data_ptr(), matrix_floats * 4)
    ctx.pose_matrices_batch(*out.arguments, stream=stream if stream is not None else buffers.stream())
    if stream is not None:
        return out
    out.matrices = buffers.down(d_matrices)
    assert np.array_equal(bits(buffers.down(d_local)), bits(h_local))          # the input is only read
    return out


def check(matrices, rows):
    """rows: per instance [B, 4, 4] or None (refused: the row stays the sentinel). On bits where the expectation is a number, a NaN where
    it is a NaN, the sentinel everywhere else; lane 3 of every record is 0, 0, 0, 1."""
    want = np.full(matrices.shape, SENTINEL, dtype=np.float32)
    for i, row in enumerate(rows):
        if row is not None:
            want[1 + i, : row.size] = row.reshape(-1)
            lanes = bits(matrices[1 + i, : row.size]).reshape(-1, 4, 4)[:, :, 3]
            assert np.array_equal(lanes, np.broadcast_to(LANE3_BITS, lanes.shape)), i
    numbers = ~np.isnan(want)
    assert np.array_equal(bits(matrices)[numbers], bits(want)[numbers]), np.argwhere((bits(matrices) != bits(want)) & numbers)[:8]
    assert np.all(np.isnan(matrices[~numbers]))


SHAPES = [("forest", bones) for bones in (1, 63, 64, 65, 100, 300, 1200)] + [("chain", 200)]


@pytest.fixture(scope="module")
def cases():
    """(kind, B) -> (parents, local [N, B, 12], {object_space: expected [N, B, 4, 4]}), computed once"""
    out = {}
    for kind, num_bones in SHAPES:
        rng = np.random.default_rng(9100 + num_bones)
        parents = forest(rng, num_bones) if kind == "forest" else chain(num_bones)
        local = batch_poses(rng, N, num_bones)
        # one bone with a NaN, one with an infinite scale, a rotation of zeros, a negative zero: all reach the bone and what hangs below it
        local[3, num_bones // 2, 1] = np.nan
        local[8, num_bones // 3, 9] = np.inf
        local[11, num_bones - 1, 0:4] = 0.0
        local[12, 0, 10] = -0.0
        out[(kind, num_bones)] = (parents, local, {space: object_matrices(parents, local, space) for space in (True, False)})
    return out


@pytest.mark.parametrize("object_space", [True, False])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda shape: "%s-%d" % shape)
def test_the_rows_are_the_restatement(cases, shape, object_space):
    """lane stride edges (63 / 64 / 65), 4, 2 and 1 images per workgroup (100 / 300 / 1200 bones), a batch that ends inside a workgroup,
    the deepest schedule (a chain of 200: one transform per step); scales of both signs, a NaN and an infinity"""
    parents, local, expected = cases[shape]
    num_bones = shape[1]
    want = expected[object_space]
    assert np.isnan(want[3]).any() and not np.isnan(want[0]).any() and not np.isnan(want[4]).any()
    with runtime.Context(0) as ctx:
        skeleton = ctx.register_skeleton(parents, identity_pose(num_bones))
        before = ctx.negative_scale_count()
        out = launch(ctx, local, skeleton=skeleton, object_space=object_space)
        check(out.matrices, list(want))
        assert ctx.negative_scale_count() == before            # there is no qvv_mul here
        assert ctx.rejected_instance_count() == 0


def test_object_space_differs_from_local_space_below_the_roots_only(cases):
    parents, _, expected = cases[("forest", 100)]
    roots = parents == runtime.NO_PARENT
    same = (bits(expected[True][0]) == bits(expected[False][0])).all(axis=(1, 2))
    assert same[roots].all() and not same[~roots].any()


def test_skeletons_per_instance_and_refusals():
    import torch
    rng = np.random.default_rng(9201)
    small, large = 40, 100
    parents = {small: forest(rng, small, root_chance=0.2), large: forest(rng, large)}
    with runtime.Context(0) as ctx:
        handles = {bones: ctx.register_skeleton(parents[bones], identity_pose(bones)) for bones in (small, large)}
        flat = ctx.register_skeleton(None, identity_pose(small))                        # no hierarchy
        retired = ctx.register_skeleton(parents[small], identity_pose(small))
        ctx.unregister_skeleton(retired)
        torch.cuda.synchronize()

        # different bone counts inside one workgroup: a row is written up to its own skeleton's 64 * B
        which = [large, small, small, large, small, large, large, small, large, small, small, large, large, large, small, large, small]
        assert len(which) == N
        local = [signed_poses(rng, 1, bones)[0] for bones in which]
        ids = [handles[bones] for bones in which]
        for object_space in (True, False):
            out = launch(ctx, local, skeleton=handles[small], instance_skeletons=ids, object_space=object_space)    # a launch wide skeleton is ignored next to the list
            check(out.matrices, [object_matrices(parents[bones], pose, object_space) for bones, pose in zip(which, local)])
            assert np.all(out.matrices[2, small * 16:] == SENTINEL)
        assert ctx.rejected_instance_count() == 0

        # handle 0, an unknown handle, a retired one, object space without a hierarchy: refused and counted, the row what it was
        local = [signed_poses(rng, 1, small)[0] for _ in range(N)]
        ids = [handles[small]] * N
        ids[1], ids[2], ids[4], ids[5], ids[16] = 0, 0x00ABCDEF, retired, flat, 0xFFFFFFFF
        refused = [handle != handles[small] for handle in ids]
        before = ctx.rejected_instance_count()
        out = launch(ctx, local, instance_skeletons=ids)
        check(out.matrices, [None if no else object_matrices(parents[small], pose) for no, pose in zip(refused, local)])
        assert ctx.rejected_instance_count() - before == sum(refused) == 5
        # in local space the skeleton without a hierarchy is served
        before = ctx.rejected_instance_count()
        out = launch(ctx, local, instance_skeletons=ids, object_space=False)
        check(out.matrices, [None if no and handle != flat else object_matrices(parents[small], pose, False) for no, handle, pose in zip(refused, ids, local)])
        assert ctx.rejected_instance_count() - before == 4

        # a row of either buffer that holds fewer bones than the skeleton: refused, in front of any load of it
        which = [small, large] * 8 + [small]
        local = [signed_poses(rng, 1, bones)[0] for bones in which]
        ids = [handles[bones] for bones in which]
        rows = [None if bones == large else object_matrices(parents[bones], pose) for bones, pose in zip(which, local)]
        for sizes in (dict(matrix_row_bones=small), dict(local_row_bones=small), dict(matrix_row_bones=large - 1)):
            cut = [pose[:small] for pose in local] if "local_row_bones" in sizes else local
            before = ctx.rejected_instance_count()
            out = launch(ctx, cut, instance_skeletons=ids, local_row_bones=sizes.get("local_row_bones", large), matrix_row_bones=sizes.get("matrix_row_bones", large))
            check(out.matrices, rows)
            assert ctx.rejected_instance_count() - before == 8, sizes

        # every instance refused
        before = ctx.rejected_instance_count()
        out = launch(ctx, local, skeleton=retired)
        check(out.matrices, [None] * N)
        assert ctx.rejected_instance_count() - before == N


def test_a_captured_launch_replays_with_the_bytes_of_the_direct_one(cases):
    import torch
    parents, local, expected = cases[("forest", 100)]
    with runtime.Context(0) as ctx:
        skeleton = ctx.register_skeleton(parents, identity_pose(100))
        direct = launch(ctx, local, skeleton=skeleton)
        check(direct.matrices, list(expected[True]))
        device = direct.buffers.device
        side = torch.cuda.Stream(device=device)
        side.wait_stream(torch.cuda.current_stream(device))
        with torch.cuda.stream(side):
            captured = launch(ctx, local, skeleton=skeleton, stream=side.cuda_stream)      # warm-up
            side.synchronize()
            captured.tensor.fill_(float(SENTINEL))
            side.synchronize()
            graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graph, stream=side):
                ctx.pose_matrices_batch(*captured.arguments, stream=side.cuda_stream)
        graph.replay()
        torch.cuda.synchronize()
        replayed = captured.tensor.cpu().numpy()
        check(replayed, list(expected[True]))
        assert np.array_equal(bits(replayed), bits(direct.matrices))
        del graph
        assert ctx.rejected_instance_count() == 0
