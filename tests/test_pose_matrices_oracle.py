"""What aclhip_pose_matrices_batch and aclhip_measure_pose_error_metric_batch (ACLHIP_METRIC_QVVF_MATRIX3X4F) compute, restated on the CPU
as numpy float32 element operations in the header's operation order (single, correctly rounded IEEE operations, nothing fused):

  step 1   matrices_of          rtm::matrix_from_qvv per bone                      (oracle/rtm_shim/rtm/matrix3x4f.h:11-20)
  step 2   walk_matrices        O[b] = matrix_mul(M[b], O[P[b]]), roots keep M     (transform_error_metrics.h:415-436)
  step 3   matrix_shell_errors  rtm::matrix_mul_point3 over the three shell points (transform_error_metrics.h:438-461)

They are the counterparts of shell_errors in tests/test_pose_error_oracle.py, whose forest, loose_poses, scan and scan_worst serve here too;
tests/test_gpu_pose_matrices.py and tests/test_gpu_pose_error_matrix.py compare the kernels with them on bits. Every function takes a
dtype: the float64 evaluation of the same chain is what this file holds the float32 restatement to. A matrix is [4 axes, 4 lanes]; lane 3
is the constant the launch writes (0, 0, 0, 1) and takes no part in any product."""
import numpy as np
import pytest

from oracle import bindings as ob
from test_pose_error_oracle import NO_BONE, NO_PARENT, as_distances, expected_measure, forest, rigid_pose, scan, shell_points

LANE3 = np.array([0.0, 0.0, 0.0, 1.0])


def matrices_of(poses, dtype=np.float32):
    """step 1 over [..., B, 12] QVV48 rows: [..., B, 4, 4]"""
    poses = np.asarray(poses, dtype=np.float32).astype(dtype)
    x, y, z, w = (poses[..., c] for c in range(4))
    sx, sy, sz = (poses[..., 8 + c] for c in range(3))
    one = dtype(1.0)
    out = np.empty(poses.shape[:-1] + (4, 4), dtype=dtype)
    with np.errstate(invalid="ignore", over="ignore"):
        x2, y2, z2 = x + x, y + y, z + z
        xx, xy, xz, yy, yz, zz, wx, wy, wz = x * x2, x * y2, x * z2, y * y2, y * z2, z * z2, w * x2, w * y2, w * z2
        out[..., 0, 0], out[..., 0, 1], out[..., 0, 2] = (one - (yy + zz)) * sx, (xy + wz) * sx, (xz - wy) * sx
        out[..., 1, 0], out[..., 1, 1], out[..., 1, 2] = (xy - wz) * sy, (one - (xx + zz)) * sy, (yz + wx) * sy
        out[..., 2, 0], out[..., 2, 1], out[..., 2, 2] = (xz + wy) * sz, (yz - wx) * sz, (one - (xx + yy)) * sz
    out[..., 3, 0:3] = poses[..., 4:7]
    out[..., :, 3] = LANE3.astype(dtype)
    return out


def matrix_mul(lhs, rhs):
    """rtm::matrix_mul over [..., 4, 4], lhs first: a row v of lhs becomes ((R.x_axis * v.x) + R.y_axis * v.y) + R.z_axis * v.z, the w row
    plus R.w_axis, added last"""
    out = np.empty(np.broadcast(lhs, rhs).shape, dtype=lhs.dtype)
    with np.errstate(invalid="ignore", over="ignore"):
        for row in range(4):
            v = lhs[..., row, :]
            value = ((rhs[..., 0, 0:3] * v[..., 0:1]) + (rhs[..., 1, 0:3] * v[..., 1:2])) + (rhs[..., 2, 0:3] * v[..., 2:3])
            out[..., row, 0:3] = value + rhs[..., 3, 0:3] if row == 3 else value
    out[..., :, 3] = LANE3.astype(lhs.dtype)
    return out


def walk_matrices(parents, matrices):
    """step 2 over [..., B, 4, 4], bones in ascending order (a parent comes before its children)"""
    out = np.array(matrices, copy=True)
    for bone, parent in enumerate(np.asarray(parents, dtype=np.uint32)):
        if parent != NO_PARENT:
            out[..., bone, :, :] = matrix_mul(matrices[..., bone, :, :], out[..., int(parent), :, :])
    return out


def object_matrices(parents, poses, object_space=True, dtype=np.float32):
    """steps 1 and 2 of [..., B, 12] rows"""
    matrices = matrices_of(poses, dtype)
    return walk_matrices(parents, matrices) if object_space and matrices.shape[-3] != 0 else matrices


def matrix_shell_errors(raw, lossy, shells):
    """step 3 over two [B, 4, 4] arrays: error[b], [B] in their dtype. All three products of a point are made, the zero ones too."""
    points = shell_points(as_distances(shells, raw.shape[0])).astype(raw.dtype)            # [B, 3 points, 3]

    def moved(matrices):
        m = matrices[:, None, :, 0:3]
        return (((m[:, :, 0] * points[..., 0:1]) + (m[:, :, 1] * points[..., 1:2])) + (m[:, :, 2] * points[..., 2:3])) + m[:, :, 3]

    with np.errstate(invalid="ignore", over="ignore"):
        d = moved(lossy) - moved(raw)
        e = np.sqrt(((d[..., 0] * d[..., 0]) + (d[..., 1] * d[..., 1])) + (d[..., 2] * d[..., 2]))
        first = np.where(e[:, 0] > e[:, 1], e[:, 0], e[:, 1])
        return np.where(first > e[:, 2], first, e[:, 2]).astype(raw.dtype)


def expected_matrix_measure(parents, raw, lossy, shells, object_space=True):
    """the header's definition of one instance under ACLHIP_METRIC_QVVF_MATRIX3X4F: (bone errors [B], (error, bone))"""
    raw, lossy = np.ascontiguousarray(raw, dtype=np.float32), np.ascontiguousarray(lossy, dtype=np.float32)
    if raw.shape[0] == 0:
        return np.zeros(0, dtype=np.float32), scan([])
    errors = matrix_shell_errors(object_matrices(parents, raw, object_space), object_matrices(parents, lossy, object_space), shells)
    return errors, scan(errors)


# ---- the properties ---------------------------------------------------------------------------------------------------------------

def chain(num_bones):
    parents = np.arange(num_bones, dtype=np.int64) - 1
    parents[0] = NO_PARENT
    return parents.astype(np.uint32)


def depth_of(parents):
    depths = np.zeros(len(parents), dtype=np.int64)
    for bone, parent in enumerate(parents):
        depths[bone] = 0 if parent == NO_PARENT else depths[int(parent)] + 1
    return int(depths.max())


def scaled_poses(rng, n, num_bones):
    """unit rotations, translations within +-2, scale magnitudes 2^U(-2, 2), a sixth of the components negative"""
    poses = np.zeros((n, num_bones, 12), dtype=np.float32)
    rotations = rng.normal(size=(n, num_bones, 4))
    poses[..., 0:4] = rotations / np.linalg.norm(rotations, axis=2, keepdims=True)
    poses[..., 4:7] = rng.uniform(-2.0, 2.0, size=(n, num_bones, 3))
    magnitudes = np.exp2(rng.uniform(-2.0, 2.0, size=(n, num_bones, 3)))
    poses[..., 8:11] = np.where(rng.uniform(size=magnitudes.shape) < 1.0 / 6.0, -magnitudes, magnitudes)
    return poses


def deviation(got, exact):
    """per instance: the largest deviation of [n, B, 4, 4] from the float64 chain, relative to the instance's largest entry"""
    got, exact = got[..., 0:3].astype(np.float64), exact[..., 0:3]
    return np.abs(got - exact).max(axis=(1, 2, 3)) / np.abs(exact).max(axis=(1, 2, 3))


SEEDED_HIERARCHIES = [("forest of 100", lambda rng: forest(rng, 100)), ("forest of 300", lambda rng: forest(rng, 300)), ("chain of 32", lambda rng: chain(32))]


def test_the_restatement_is_the_float64_chain_to_float32_rounding():
    """unit rotations, translations within +-2, scale magnitudes 2^U(-2, 2) with a sixth negative, depths up to 31: the largest deviation
    per instance, relative to the instance's largest entry, is 4.1e-6 over these seeds. A wrong operand order or a transposed product is
    O(1) off."""
    worst, deepest = 0.0, 0
    for index, (_, make) in enumerate(SEEDED_HIERARCHIES):
        rng = np.random.default_rng(8100 + index)
        parents = make(rng)
        deepest = max(deepest, depth_of(parents))
        poses = scaled_poses(rng, 24, len(parents))
        got, exact = object_matrices(parents, poses), object_matrices(parents, poses, dtype=np.float64)
        assert got.dtype == np.float32 and exact.dtype == np.float64
        worst = max(worst, float(deviation(got, exact).max()))
        # the operand order matters at this scale: the product the other way round is not the chain
        local = matrices_of(poses)
        swapped = np.array(local, copy=True)
        for bone, parent in enumerate(parents):
            if parent != NO_PARENT:
                swapped[:, bone] = matrix_mul(swapped[:, int(parent)], local[:, bone])
        assert deviation(swapped, exact).max() > 0.1
    print("largest relative deviation of the float32 restatement: %.3g" % worst)
    assert deepest == 31
    assert worst < 1.0e-4


RIGID_ORACLE_DEVIATION = 5.4e-7      # measured over the seeded cases below (printed by the test); the assertion is 16 x this
RIGID_MARGIN = min(16.0 * RIGID_ORACLE_DEVIATION, 1.0e-3)


def rigid_rows(rng, n, num_bones):
    return np.stack([rigid_pose(rng, num_bones) for _ in range(n)])


def test_on_rigid_rows_the_matrix_walk_and_the_qvv_oracle_meet_at_the_float64_chain():
    """unit rotations, scale exactly 1: matrix_from_qvv(oracle_local_to_object_space(...)) and the matrix walk are the same pose, and both
    are held to the float64 chain. The oracle's side deviates by 5.4e-7 of the instance's largest entry over these seeds (its walk
    renormalizes every rotation); it is asserted at 16 x that figure, the matrix walk at the 1e-4 of the test above."""
    oracle_worst, walk_worst = 0.0, 0.0
    for index, (_, make) in enumerate(SEEDED_HIERARCHIES):
        rng = np.random.default_rng(8200 + index)
        parents = make(rng)
        poses = rigid_rows(rng, 12, len(parents))
        exact = object_matrices(parents, poses, dtype=np.float64)
        by_oracle = matrices_of(np.stack([ob.oracle_local_to_object_space(parents, pose) for pose in poses]))
        oracle_worst = max(oracle_worst, float(deviation(by_oracle, exact).max()))
        walk_worst = max(walk_worst, float(deviation(object_matrices(parents, poses), exact).max()))
    print("largest relative deviation on rigid rows: oracle %.3g, matrix walk %.3g" % (oracle_worst, walk_worst))
    assert oracle_worst < RIGID_MARGIN <= 1.0e-3
    assert walk_worst < 1.0e-4


def quat_about_z(degrees):
    half = np.radians(degrees) / 2.0
    return np.array([0.0, 0.0, np.sin(half), np.cos(half)], dtype=np.float32)


def test_the_two_metrics_differ_under_shear_and_agree_on_rigid_rows():
    """a child rotated by 45 degrees under a parent scaled (3, 1, 1): the matrix product shears the child's axes, the QVV product keeps them
    orthogonal, so a rotation error of the child is measured differently -- by more than a tenth of the error here. Where every scale
    is 1 the two object space poses are the same pose, and the two errors agree to the margin of the test above, RIGID_MARGIN of the
    instance's largest entry L (8.6e-6 L): over the six seeded rows the largest |matrix error - qvv error| is 1.7e-6 to 3.2e-6, at most
    8.1e-7 L (printed by the test)."""
    parents = np.array([NO_PARENT, 0], dtype=np.uint32)
    raw = np.zeros((2, 12), dtype=np.float32)
    raw[:, 3], raw[:, 8:11] = 1.0, 1.0
    raw[0, 8:11] = (3.0, 1.0, 1.0)
    raw[1, 0:4], raw[1, 4:7] = quat_about_z(45.0), (1.0, 0.5, 0.0)
    lossy = raw.copy()
    lossy[1, 0:4] = quat_about_z(50.0)
    qvv_errors = expected_measure(parents, raw, lossy, 1.0)[0]
    matrix_errors, record = expected_matrix_measure(parents, raw, lossy, 1.0)
    assert qvv_errors[0] == 0.0 and matrix_errors[0] == 0.0 and record[1] == 1
    assert abs(float(matrix_errors[1]) - float(qvv_errors[1])) > 0.1 * float(qvv_errors[1]) > 0.0
    # in local space there is no product: the two metrics measure the same transform
    assert np.allclose(expected_matrix_measure(parents, raw, lossy, 1.0, False)[0], expected_measure(parents, raw, lossy, 1.0, False)[0], rtol=1.0e-5, atol=1.0e-6)

    rng = np.random.default_rng(8301)
    parents = forest(rng, 100)
    distance = 3.0
    for _ in range(6):
        raw = rigid_pose(rng, 100)
        lossy = raw.copy()
        lossy[:, 4:7] += rng.uniform(-0.01, 0.01, size=(100, 3)).astype(np.float32)
        twist = rng.normal(size=(100, 4)) * 0.01 + np.array([0.0, 0.0, 0.0, 1.0])
        twist = (twist / np.linalg.norm(twist, axis=1, keepdims=True)).astype(np.float32)
        lossy[:, 0:4] = [ob.oracle_quat_mul(twist[b], raw[b, 0:4]) for b in range(100)]
        lossy[:, 0:4] /= np.linalg.norm(lossy[:, 0:4], axis=1, keepdims=True)
        qvv_errors = expected_measure(parents, raw, lossy, distance)[0]
        matrix_errors = expected_matrix_measure(parents, raw, lossy, distance)[0]
        largest = float(np.abs(object_matrices(parents, raw, dtype=np.float64)[..., 0:3]).max())
        assert qvv_errors.max() > 1.0e-3
        difference = float(np.abs(matrix_errors.astype(np.float64) - qvv_errors).max())
        print("largest |matrix error - qvv error|: %.3g, %.3g of the largest entry %.3g" % (difference, difference / largest, largest))
        assert difference < RIGID_MARGIN * largest


@pytest.mark.parametrize("object_space", [True, False])
def test_identical_rows_give_zero_and_bone_zero_and_a_nan_stays_below_its_bone(object_space):
    rng = np.random.default_rng(8401)
    parents = forest(rng, 80)
    pose = scaled_poses(rng, 1, 80)[0]
    errors, record = expected_matrix_measure(parents, pose, pose.copy(), 3.0, object_space)
    assert np.all(errors.view(np.uint32) == 0) and record == (0.0, 0)
    assert expected_matrix_measure(parents[:0], pose[:0], pose[:0], 3.0, object_space)[1] == (-1.0, NO_BONE)
    # a NaN in one bone reaches the bone and its descendants and nowhere else; lane 3 stays the constant
    bone = 7
    broken = pose.copy()
    broken[bone, 9] = np.nan
    matrices = object_matrices(parents, broken, object_space)
    below = np.zeros(80, dtype=bool)
    below[bone] = True
    for b, parent in enumerate(parents):
        if parent != NO_PARENT and below[int(parent)]:
            below[b] = True
    touched = np.isnan(matrices[..., 0:3]).any(axis=(1, 2))
    assert np.array_equal(touched, below if object_space else np.arange(80) == bone)
    assert np.array_equal(matrices[..., 3], np.broadcast_to(LANE3.astype(np.float32), (80, 4)))
