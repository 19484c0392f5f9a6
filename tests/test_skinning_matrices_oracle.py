"""What aclhip_skinning_matrices_batch computes, restated on the CPU as numpy float32 element operations in the header's operation order
(single, correctly rounded IEEE operations, nothing fused):

  steps 1, 2   object_matrices      of tests/test_pose_matrices_oracle.py: matrix_from_qvv per bone and the matrix walk
  step 3       skinning_matrices    S[j] = matrix_mul(IB[j], O[k[j]]), lhs first, and the record of the layout

tests/test_gpu_skinning_matrices.py compares the kernels with skinning_matrices on bits. The function takes a dtype: its float64 evaluation
over the same float32 inputs is what this file holds the float32 restatement to. A matrix is [4 axes, 4 lanes] as in that file; lane 3 of
an inverse bind matrix is ignored and lane 3 of a 64 byte record is the constant 0, 0, 0, 1. A transposed record is [3 rows, 4]: row k is
(x_axis[k], y_axis[k], z_axis[k], w_axis[k])."""
import numpy as np
import pytest

from test_pose_error_oracle import NO_PARENT, forest, rigid_pose
from test_pose_matrices_oracle import LANE3, SEEDED_HIERARCHIES, deviation, matrix_mul, object_matrices, scaled_poses

PALETTE_3X4F_64, PALETTE_3X4F_TRANSPOSED_48 = 0, 1
RECORD_FLOATS = {PALETTE_3X4F_64: 16, PALETTE_3X4F_TRANSPOSED_48: 12}


def skin_arrays(num_bones, joint_bones, inverse_bind, dtype=np.float32):
    """(k [J], IB [J, 4, 4] in dtype) of a skin as registration takes it: None is the identity list / identity matrices; lane 3 of a
    caller's matrices is ignored"""
    joints = np.arange(num_bones, dtype=np.int64) if joint_bones is None else np.asarray(joint_bones, dtype=np.int64)
    if inverse_bind is None:
        bind = np.broadcast_to(np.eye(4, dtype=dtype), (len(joints), 4, 4)).copy()
    else:
        bind = np.array(np.asarray(inverse_bind, dtype=np.float32).reshape(len(joints), 4, 4), dtype=dtype)
    bind[..., :, 3] = LANE3.astype(dtype)
    return joints, bind


def palettes_of(objects, joint_bones, inverse_bind, layout=PALETTE_3X4F_64):
    """step 3 over object matrices [..., B, 4, 4], in their dtype: [..., J, 4, 4] records of 64 bytes or [..., J, 3, 4] transposed ones"""
    joints, bind = skin_arrays(objects.shape[-3], joint_bones, inverse_bind, objects.dtype.type)
    product = matrix_mul(bind, objects[..., joints, :, :])
    return product if layout == PALETTE_3X4F_64 else np.ascontiguousarray(np.swapaxes(product[..., :, 0:3], -1, -2))


def skinning_matrices(parents, poses, joint_bones, inverse_bind, object_space=True, layout=PALETTE_3X4F_64, dtype=np.float32):
    """the header's definition over [..., B, 12] QVV48 rows"""
    return palettes_of(object_matrices(parents, poses, object_space, dtype), joint_bones, inverse_bind, layout)


def inverse_bind_of(parents, bind_pose):
    """the float64 inverse of a bind pose's object matrices, rounded to float32: [B, 4, 4] in the 64 byte layout"""
    objects = object_matrices(parents, bind_pose, dtype=np.float64)
    return np.linalg.inv(objects).astype(np.float32)


def mixed_joint_list(rng, num_bones):
    """a joint list that permutes the bones, drops about a quarter of them and repeats one"""
    order = rng.permutation(num_bones)
    kept = order[: max(1, num_bones - num_bones // 4)]
    return np.concatenate([kept, kept[:1]]).astype(np.uint32)


def below(parents, bone):
    """the bones that hang below `bone`, itself included"""
    out = np.zeros(len(parents), dtype=bool)
    out[bone] = True
    for b, parent in enumerate(parents):
        if parent != NO_PARENT and out[int(parent)]:
            out[b] = True
    return out


# ---- the properties ---------------------------------------------------------------------------------------------------------------

def test_the_restatement_is_the_float64_chain_to_float32_rounding():
    """the hierarchies and poses of the matrix walk's own test (unit rotations, translations within +-2, scale magnitudes 2^U(-2, 2) with a
    sixth negative), IB the float64 inverse of such a pose's object matrices rounded to float32: the largest deviation of the float32
    palette from the float64 chain over the same float32 IB, relative to the instance's largest palette entry, is 4.6e-6 over these seeds
    (printed); asserted below the 1e-4 of the walk. The product the other way round, matrix_mul(O, IB), is O(1) off."""
    worst = 0.0
    for index, (_, make) in enumerate(SEEDED_HIERARCHIES):
        rng = np.random.default_rng(8500 + index)
        parents = make(rng)
        bind = inverse_bind_of(parents, scaled_poses(rng, 1, len(parents))[0])
        poses = scaled_poses(rng, 24, len(parents))
        got, exact = skinning_matrices(parents, poses, None, bind), skinning_matrices(parents, poses, None, bind, dtype=np.float64)
        assert got.dtype == np.float32 and exact.dtype == np.float64
        worst = max(worst, float(deviation(got, exact).max()))
        swapped = matrix_mul(object_matrices(parents, poses), skin_arrays(len(parents), None, bind)[1])
        assert deviation(swapped, exact).max() > 0.1
    print("largest relative deviation of the float32 palette: %.3g" % worst)
    assert worst < 1.0e-4


BIND_POSE_DEVIATION = 3.2e-6      # measured over the seeded cases below (printed by the test); the assertion is 16 x this, capped at 1e-4
BIND_POSE_MARGIN = min(16.0 * BIND_POSE_DEVIATION, 1.0e-4)


def test_the_palette_of_a_rigid_bind_pose_is_the_identity():
    """unit rotations, scale exactly 1: IB[j] * O[j] of the bind pose itself is the identity to float32 rounding -- max |S - I| is
    3.2e-6 over these seeds (printed), asserted at 16 x that. SCALED bind poses are not asserted: the float32 product cancels
    catastrophically there (a stand-alone run gave 7e-3 up to 6e2 on a scaled chain of 32), which is a property of float32 inverse bind
    matrices, not of the operation order."""
    worst = 0.0
    for index, (_, make) in enumerate(SEEDED_HIERARCHIES):
        rng = np.random.default_rng(8600 + index)
        parents = make(rng)
        for _ in range(8):
            pose = rigid_pose(rng, len(parents))
            palette = skinning_matrices(parents, pose, None, inverse_bind_of(parents, pose))
            worst = max(worst, float(np.abs(palette.astype(np.float64) - np.eye(4)).max()))
    print("largest |S - I| of a rigid bind pose: %.3g" % worst)
    assert worst < BIND_POSE_MARGIN <= 1.0e-4


def test_a_skinned_point_goes_through_the_inverse_bind_and_then_the_bone():
    rng = np.random.default_rng(8701)
    parents = forest(rng, 100)
    joints = mixed_joint_list(rng, 100)
    bind = inverse_bind_of(parents, scaled_poses(rng, 1, 100)[0])[joints]
    bind[:, :, 3] = rng.normal(size=(len(joints), 4))                  # lane 3 of a caller's matrices is ignored
    poses = scaled_poses(rng, 3, 100)
    points = np.concatenate([rng.uniform(-2.0, 2.0, size=(len(joints), 3)), np.ones((len(joints), 1))], axis=1)

    # (p * IB[j]) * O[k[j]] is p * S[j], in float64
    palette = skinning_matrices(parents, poses, joints, bind, dtype=np.float64)
    objects = object_matrices(parents, poses, dtype=np.float64)[:, joints]
    in_bone_space = np.einsum("ja,jab->jb", points, skin_arrays(100, joints, bind, np.float64)[1])
    assert np.allclose(in_bone_space[:, 3], 1.0)
    through_both = np.einsum("ja,njab->njb", in_bone_space, objects)
    through_palette = np.einsum("ja,njab->njb", points, palette)
    assert np.allclose(through_palette, through_both, rtol=1.0e-10, atol=1.0e-10 * np.abs(through_both).max())

    # the transposed record read as three dot products gives the 64 byte record's point; lane 3 of the 64 byte record is 0, 0, 0, 1
    wide = skinning_matrices(parents, poses, joints, bind)
    transposed = skinning_matrices(parents, poses, joints, bind, layout=PALETTE_3X4F_TRANSPOSED_48)
    assert wide.shape == (3, len(joints), 4, 4) and transposed.shape == (3, len(joints), 3, 4) and transposed.dtype == np.float32
    assert np.array_equal(wide[..., 3].view(np.uint32), np.broadcast_to(LANE3.astype(np.float32).view(np.uint32), wide[..., 3].shape))
    for k in range(3):
        assert np.array_equal(transposed[..., k, :].view(np.uint32), wide[..., :, k].view(np.uint32))
    by_rows = np.einsum("njka,ja->njk", transposed.astype(np.float64), points)
    by_axes = np.einsum("ja,njab->njb", points, wide.astype(np.float64))[..., 0:3]
    assert np.allclose(by_rows, by_axes, rtol=1.0e-12, atol=0.0)


@pytest.mark.parametrize("object_space", [True, False])
def test_a_joint_list_gathers_the_bones_it_names(object_space):
    rng = np.random.default_rng(8801)
    parents = forest(rng, 80)
    joints = mixed_joint_list(rng, 80)
    assert len(joints) == 61 and len(set(joints.tolist())) == 60 and joints[-1] == joints[0] and not np.array_equal(joints[:-1], np.sort(joints[:-1]))
    bind = rng.uniform(-2.0, 2.0, size=(len(joints), 4, 4)).astype(np.float32)
    pose = scaled_poses(rng, 1, 80)[0]
    objects = object_matrices(parents, pose, object_space)
    palette = skinning_matrices(parents, pose, joints, bind, object_space)
    for j, bone in enumerate(joints):
        one = matrix_mul(skin_arrays(80, joints, bind)[1][j], objects[int(bone)])
        assert np.array_equal(palette[j].view(np.uint32), one.view(np.uint32)), j
    # with identity matrices a joint holds its bone's matrix (1 * x + 0 * y + 0 * z is x), and the identity list is every bone in order
    assert np.array_equal(skinning_matrices(parents, pose, joints, None, object_space), objects[joints])
    assert np.array_equal(skinning_matrices(parents, pose, None, None, object_space), objects)
    # a NaN in one bone reaches exactly the joints whose bone hangs below it -- through identity matrices too -- and lane 3 stays the constant
    bone = int(joints[3])
    broken = pose.copy()
    broken[bone, 9] = np.nan
    reached = below(parents, bone) if object_space else np.arange(80) == bone
    assert reached[joints].any() and not reached[joints].all()
    for matrices in (bind, None):
        palette = skinning_matrices(parents, broken, joints, matrices, object_space)
        assert np.array_equal(np.isnan(palette[..., 0:3]).any(axis=(1, 2)), reached[joints])
        assert np.array_equal(palette[..., 3], np.broadcast_to(LANE3.astype(np.float32), (len(joints), 4)))
