"""What aclhip_measure_pose_error_batch computes, composed on the CPU from what oracle/bindings.py already offers plus numpy float32
element operations (single, correctly rounded IEEE operations: every operand below is float32, nothing is evaluated in float64):

  step 1   oracle_apply_additive_to_base(format, base = Bs, additive = R) and the same for Y      (track_error.impl.h:351-352)
  step 2   oracle_local_to_object_space(P, .) over both                                           (track_error.impl.h:354-355)
  step 3   point(p, t) = xyz of oracle_quat_mul(oracle_quat_mul(conj(t.rotation), (t.scale * p, 0)), t.rotation) + t.translation
           e_k = sqrt((dx * dx + dy * dy) + dz * dz), error[b] = max(max(e_0, e_1), e_2), max(a, b) = a > b ? a : b
           (qvvf_transform_error_metric::calculate_error, compression/transform_error_metrics.h:335-358)
  step 4   the scan of track_error.impl.h:358-375 from {-1, NO_BONE}: bone b is taken when error[b] > the record's error

Step 3 exists twice: bone by bone through oracle_quat_mul (shell_errors_by_oracle, the definition) and over whole arrays with the same
operations in the same order as numpy float32 arithmetic (shell_errors), which the first test here holds to the definition on bits;
tests/test_gpu_pose_error.py compares the kernel with it on bits. The rest of this file holds, without a device, the properties the
measure has to have."""
import numpy as np
import pytest

from oracle import bindings as ob

NO_PARENT = ob.INVALID_PARENT
NO_BONE = 0xFFFFFFFF
NONE, RELATIVE, ADDITIVE0, ADDITIVE1 = ob.ADDITIVE_NONE, ob.ADDITIVE_RELATIVE, ob.ADDITIVE_ADDITIVE0, ob.ADDITIVE_ADDITIVE1


def bits(array):
    return np.ascontiguousarray(array, dtype=np.float32).view(np.uint32)


def quat_mul_rows(lhs, rhs):
    """oracle_quat_mul over rows [..., 4]: its products, its sums and its signs in its order, every one a float32 operation"""
    lx, ly, lz, lw = (lhs[..., c] for c in range(4))
    rx, ry, rz, rw = (rhs[..., c] for c in range(4))
    out = np.empty(np.broadcast(lhs, rhs).shape, dtype=np.float32)
    out[..., 0] = ((rw * lx) + (rx * lw)) + ((ry * lz) + -(rz * ly))
    out[..., 1] = ((rw * ly) + -(rx * lz)) + ((ry * lw) + (rz * lx))
    out[..., 2] = ((rw * lz) + (rx * ly)) + (-(ry * lx) + (rz * lw))
    out[..., 3] = ((rw * lw) + -(rx * lx)) + (-(ry * ly) + -(rz * lz))
    return out


def conjugate(rotations):
    out = np.array(rotations, dtype=np.float32, copy=True)
    out[..., 0:3] = -out[..., 0:3]
    return out


def shell_points(distances):
    """[B, 3 points, 3]: (d, 0, 0), (0, d, 0), (0, 0, d) per bone"""
    distances = np.asarray(distances, dtype=np.float32)
    points = np.zeros((distances.size, 3, 3), dtype=np.float32)
    for k in range(3):
        points[:, k, k] = distances
    return points


def as_distances(shells, num_bones):
    return np.full(num_bones, shells, dtype=np.float32) if np.ndim(shells) == 0 else np.asarray(shells, dtype=np.float32)[:num_bones]


def moved_points(points, pose, quat_mul):
    """rtm::qvv_mul_point3 for the three points of every bone: [B, 3, 3]. All three components of scale * point are multiplied."""
    vectors = np.zeros(points.shape[:2] + (4,), dtype=np.float32)
    vectors[..., 0:3] = pose[:, None, 8:11] * points
    rotations = np.broadcast_to(pose[:, None, 0:4], vectors.shape)
    rotated = quat_mul(quat_mul(conjugate(rotations), vectors), rotations)
    return rotated[..., 0:3] + pose[:, None, 4:7]


def errors_of_points(raw_points, lossy_points):
    with np.errstate(invalid="ignore", over="ignore"):
        d = lossy_points - raw_points
        e = np.sqrt(((d[..., 0] * d[..., 0]) + (d[..., 1] * d[..., 1])) + (d[..., 2] * d[..., 2]))
        first = np.where(e[:, 0] > e[:, 1], e[:, 0], e[:, 1])
        return np.where(first > e[:, 2], first, e[:, 2]).astype(np.float32)


def shell_errors(raw, lossy, shells):
    """step 3 over whole arrays: error[b], float32 [B]"""
    raw, lossy = np.ascontiguousarray(raw, dtype=np.float32), np.ascontiguousarray(lossy, dtype=np.float32)
    points = shell_points(as_distances(shells, raw.shape[0]))
    with np.errstate(invalid="ignore", over="ignore"):
        return errors_of_points(moved_points(points, raw, quat_mul_rows), moved_points(points, lossy, quat_mul_rows))


def quat_mul_by_oracle(lhs, rhs):
    out = np.empty(lhs.shape, dtype=np.float32)
    for index in np.ndindex(lhs.shape[:-1]):
        out[index] = ob.oracle_quat_mul(lhs[index], rhs[index])
    return out


def shell_errors_by_oracle(raw, lossy, shells):
    """step 3 as the header states it: every quaternion product is oracle_quat_mul"""
    raw, lossy = np.ascontiguousarray(raw, dtype=np.float32), np.ascontiguousarray(lossy, dtype=np.float32)
    points = shell_points(as_distances(shells, raw.shape[0]))
    return errors_of_points(moved_points(points, raw, quat_mul_by_oracle), moved_points(points, lossy, quat_mul_by_oracle))


def takes_matrix_route(lhs, rhs):
    """rtm::qvv_mul leaves the quaternion path when a scale component of either side is negative; [B] bool"""
    return (np.minimum(lhs[:, 8:11], rhs[:, 8:11]) < 0).any(axis=1)


def measured_poses(parents, pose, object_space=True, additive_format=NONE, base=None):
    """steps 1 and 2 of one row: (pose as it is measured, matrix route products)"""
    pose, routed = np.ascontiguousarray(pose, dtype=np.float32), 0
    if additive_format != NONE:
        base = np.ascontiguousarray(base, dtype=np.float32)
        if additive_format == RELATIVE:
            routed += int(takes_matrix_route(pose, base).sum())
        pose = ob.oracle_apply_additive_to_base(additive_format, base, pose)
    if object_space and pose.shape[0] != 0:
        parents = np.asarray(parents, dtype=np.uint32)
        out = ob.oracle_local_to_object_space(parents, pose)
        children = np.flatnonzero(parents != NO_PARENT)
        children = children[children != 0]
        # (the walk multiplies the LOCAL child with the OBJECT parent)
        routed += int(takes_matrix_route(pose[children], out[parents[children]]).sum())
        pose = out
    return pose, routed


def scan(errors):
    """step 4: (error, bone), from (-1, NO_BONE); a NaN never compares greater"""
    record = (np.float32(-1.0), NO_BONE)
    for bone, error in enumerate(np.asarray(errors, dtype=np.float32)):
        if error > record[0]:
            record = (error, bone)
    return record


def expected_measure(parents, raw, lossy, shells, object_space=True, additive_format=NONE, base=None):
    """the header's definition of one instance: (bone errors [B], (error, bone), matrix route products)"""
    raw_measured, raw_routed = measured_poses(parents, raw, object_space, additive_format, base)
    lossy_measured, lossy_routed = measured_poses(parents, lossy, object_space, additive_format, base)
    errors = shell_errors(raw_measured, lossy_measured, shells) if raw_measured.shape[0] != 0 else np.zeros(0, dtype=np.float32)
    return errors, scan(errors), raw_routed + lossy_routed


def scan_worst(records):
    """step 6: (error, bone, instance) over the instances' records in ascending order"""
    worst = (np.float32(-1.0), NO_BONE, 0xFFFFFFFF)
    for instance, (error, bone) in enumerate(records):
        if error > worst[0]:
            worst = (error, bone, instance)
    return worst


# ---- the properties ---------------------------------------------------------------------------------------------------------------

def forest(rng, num_bones, root_chance=0.08):
    parents = np.zeros(num_bones, dtype=np.uint32)
    parents[0] = NO_PARENT
    for i in range(1, num_bones):
        parents[i] = NO_PARENT if rng.uniform() < root_chance else rng.integers(max(0, i - 9), i)
    return parents


def loose_poses(rng, n, num_bones, mirrored=False):
    """not only rigid: rotations of a length in [0.5, 2], scales per component in [0.25, 4] (a sixth negative when mirrored),
    translations within +-10; the pads 0"""
    poses = np.zeros((n, num_bones, 12), dtype=np.float32)
    rotations = rng.normal(size=(n, num_bones, 4))
    rotations /= np.linalg.norm(rotations, axis=2, keepdims=True)
    poses[..., 0:4] = rotations * rng.uniform(0.5, 2.0, size=(n, num_bones, 1))
    poses[..., 4:7] = rng.uniform(-10.0, 10.0, size=(n, num_bones, 3))
    scales = rng.uniform(0.25, 4.0, size=(n, num_bones, 3))
    if mirrored:
        scales = np.where(rng.uniform(size=scales.shape) < 1.0 / 6.0, -scales, scales)
    poses[..., 8:11] = scales
    return poses


def rigid_pose(rng, num_bones):
    pose = np.zeros((num_bones, 12), dtype=np.float32)
    rotations = rng.normal(size=(num_bones, 4))
    pose[:, 0:4] = rotations / np.linalg.norm(rotations, axis=1, keepdims=True)
    pose[:, 4:7] = rng.uniform(-1.0, 1.0, size=(num_bones, 3))
    pose[:, 8:11] = 1.0
    return pose


def test_the_array_form_is_the_oracle_quat_mul_form_on_bits():
    rng = np.random.default_rng(7001)
    raw, lossy = loose_poses(rng, 2, 150, mirrored=True), loose_poses(rng, 2, 150, mirrored=True)
    raw[0, 3, 0:4] = 0.0                    # a rotation of all zeros, a scale of zeros, a negative zero
    lossy[0, 5, 8:11] = 0.0
    lossy[1, 7, 9] = -0.0
    shells = rng.uniform(0.0, 3.0, size=150).astype(np.float32)
    shells[11] = 0.0
    for i in range(2):
        for distances in (shells, np.float32(1.0)):
            assert np.array_equal(bits(shell_errors(raw[i], lossy[i], distances)), bits(shell_errors_by_oracle(raw[i], lossy[i], distances)))
    lhs, rhs = rng.normal(size=(500, 4)).astype(np.float32), rng.normal(size=(500, 4)).astype(np.float32)
    assert np.array_equal(bits(quat_mul_rows(lhs, rhs)), bits(quat_mul_by_oracle(lhs, rhs)))


@pytest.mark.parametrize("object_space", [True, False])
def test_identical_poses_give_exactly_zero_and_bone_zero(object_space):
    rng = np.random.default_rng(7101)
    parents = forest(rng, 80)
    pose = loose_poses(rng, 1, 80, mirrored=True)[0]
    errors, record, _ = expected_measure(parents, pose, pose.copy(), 3.0, object_space)
    assert np.all(bits(errors) == 0)
    assert record == (0.0, 0) and np.signbit(record[0]) == False   # noqa: E712
    # no bones: the reference's invalid_track_error
    assert expected_measure(parents[:0], pose[:0], pose[:0], 3.0, object_space)[1] == (-1.0, NO_BONE)


@pytest.mark.parametrize("object_space", [True, False])
def test_a_translated_leaf_shows_its_float32_distance_and_nothing_else_moves(object_space):
    """the leaf's parent chain is the identity, so the leaf's object space translation is its local one and every shell point moves by
    exactly (0, t, 0): the three distances are |fl(y + t) - y| for the point's y, the largest of them is the error"""
    num_bones, leaf = 12, 11
    parents = np.arange(num_bones, dtype=np.int64) - 1
    parents[0] = NO_PARENT
    parents = parents.astype(np.uint32)
    raw = np.zeros((num_bones, 12), dtype=np.float32)
    raw[:, 3] = 1.0
    raw[:, 8:11] = 1.0
    lossy = raw.copy()
    t = np.float32(0.375)
    lossy[leaf, 5] = t
    errors, record, _ = expected_measure(parents, raw, lossy, 2.0, object_space)
    assert errors[leaf] == t and np.all(errors[:leaf] == 0.0)
    assert record == (t, leaf)
    # a t that is not a multiple of the point's ulp: the distance is what float32 leaves of it at (0, 2, 0)
    t = np.float32(0.1)
    lossy[leaf, 5] = t
    errors, record, _ = expected_measure(parents, raw, lossy, 2.0, object_space)
    at_origin, at_two = t, (np.float32(2.0) + t) - np.float32(2.0)
    assert errors[leaf] == max(at_origin, at_two) and record[1] == leaf and np.all(errors[:leaf] == 0.0)


def test_a_rotation_error_at_a_parent_shows_at_its_descendants_in_object_space_only():
    rng = np.random.default_rng(7301)
    num_bones, bent = 10, 3
    parents = np.arange(num_bones, dtype=np.int64) - 1
    parents[0] = NO_PARENT
    parents = parents.astype(np.uint32)
    raw = rigid_pose(rng, num_bones)
    lossy = raw.copy()
    half = np.float32(0.05)
    twist = np.array([np.sin(half), 0.0, 0.0, np.cos(half)], dtype=np.float32)
    lossy[bent, 0:4] = ob.oracle_quat_mul(twist, raw[bent, 0:4])
    local_errors, local_record, _ = expected_measure(parents, raw, lossy, 1.0, object_space=False)
    assert local_errors[bent] > 0.01 and np.all(np.delete(local_errors, bent) == 0.0) and local_record[1] == bent
    object_errors, _, _ = expected_measure(parents, raw, lossy, 1.0, object_space=True)
    assert np.all(object_errors[:bent] == 0.0)
    assert np.all(object_errors[bent:] > 0.01)


def test_the_error_of_a_bone_grows_with_its_shell_distance():
    rng = np.random.default_rng(7401)
    num_bones = 40
    parents = forest(rng, num_bones)
    raw = rigid_pose(rng, num_bones)
    lossy = raw.copy()
    half = rng.uniform(0.01, 0.1, size=num_bones).astype(np.float32)
    for b in range(num_bones):
        lossy[b, 0:4] = ob.oracle_quat_mul(np.array([0.0, np.sin(half[b]), 0.0, np.cos(half[b])], dtype=np.float32), raw[b, 0:4])
    previous = expected_measure(parents, raw, lossy, 0.0, object_space=False)[0]
    assert np.all(previous == 0.0)          # d = 0: every point is the bone's origin, which a rotation leaves where it is
    for distance in (0.5, 1.0, 2.0, 8.0):
        errors = expected_measure(parents, raw, lossy, distance, object_space=False)[0]
        assert np.all(errors > previous)
        previous = errors
    # a table: every bone by its own distance
    table = rng.uniform(0.5, 8.0, size=num_bones).astype(np.float32)
    by_table = expected_measure(parents, raw, lossy, table, object_space=False)[0]
    for b in (0, 17, 39):
        assert by_table[b] == expected_measure(parents, raw, lossy, table[b], object_space=False)[0][b]


def test_the_scan_ignores_a_nan_and_keeps_the_lowest_bone_among_equals():
    nan = np.float32(np.nan)
    assert scan([nan, 1.0, 2.0, nan, 2.0]) == (2.0, 2)
    assert scan([nan, nan]) == (-1.0, NO_BONE)
    assert scan([]) == (-1.0, NO_BONE)
    assert scan([0.0, 0.0]) == (0.0, 0)
    assert scan_worst([(np.float32(-1.0), NO_BONE), (np.float32(3.0), 4), (np.float32(3.0), 1)]) == (3.0, 4, 1)
    assert scan_worst([(np.float32(-1.0), NO_BONE)]) == (-1.0, NO_BONE, 0xFFFFFFFF)
    assert scan_worst([]) == (-1.0, NO_BONE, 0xFFFFFFFF)


@pytest.mark.parametrize("additive_format", [RELATIVE, ADDITIVE0, ADDITIVE1])
def test_the_same_base_under_both_poses(additive_format):
    """identical additive poses over a base give 0; a lossy additive pose gives an error that the base's scale carries into the measure"""
    rng = np.random.default_rng(7500 + additive_format)
    parents = forest(rng, 30)
    raw, base = loose_poses(rng, 1, 30)[0], loose_poses(rng, 1, 30)[0]
    errors, record, _ = expected_measure(parents, raw, raw.copy(), 1.0, True, additive_format, base)
    assert np.all(errors == 0.0) and record == (0.0, 0)
    lossy = raw.copy()
    lossy[:, 4:7] += np.float32(0.01)
    errors, record, _ = expected_measure(parents, raw, lossy, 1.0, True, additive_format, base)
    assert np.all(errors > 0.0) and np.isfinite(errors).all() and record[0] == errors.max()
