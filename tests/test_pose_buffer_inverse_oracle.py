"""What aclhip_inverse_transform_poses_batch computes, composed on the CPU from what oracle/bindings.py already offers plus numpy float32
element operations (single, correctly rounded IEEE operations: every operand below is float32, nothing is evaluated in float64):

  inverse(t)           rotation^-1 = sign flip of x, y, z; scale^-1 = float32(1) / scale; v = (scale^-1 * translation, 0);
                       translation^-1 = -xyz of oracle_quat_mul(oracle_quat_mul(conj(rotation^-1), v), rotation^-1)    (rtm::qvv_inverse)
  a non-root bone      oracle_local_to_object_space([NO_PARENT, 0], [inverse(X[parent]), X[bone]])[1]
                       = normalize(qvv_mul(X[bone], inverse(X[parent]))) with pads 0, rtm::qvv_mul's matrix route included
  convert_to_relative  oracle_apply_additive_to_base(RELATIVE, base = inverse(Bs[b]), additive = L[b]) = qvv_mul(L[b], inverse(Bs[b]))
  additive0 / 1        oracle_quat_mul for the rotation, float32 sub / div / mul / reciprocal for the rest (core/additive_utils.h:181-195)

tests/test_gpu_pose_buffer_inverse.py holds the kernel to these functions on bits. Here, without a device: the composition undoes the
oracle's forward steps, and the operand order of the reference's object_to_local_space text does not -- why include/aclhip.h deviates
from it. The bar, 2e-5 relative to max(1, |value|), is five times the worst case measured for this composition (4.1e-6): a bar on the
oracle-only composition, not on the code under test."""
import numpy as np
import pytest

from oracle import bindings as ob

NO_PARENT = ob.INVALID_PARENT
NONE, RELATIVE, ADDITIVE0, ADDITIVE1 = ob.ADDITIVE_NONE, ob.ADDITIVE_RELATIVE, ob.ADDITIVE_ADDITIVE0, ob.ADDITIVE_ADDITIVE1
ONE = np.float32(1.0)
BAR = 2.0e-5


def conjugate(rotations):
    out = np.array(rotations, dtype=np.float32, copy=True)
    out[..., 0:3] = -out[..., 0:3]
    return out


def inverse_pose(pose):
    """rtm::qvv_inverse per transform; pose float32 [B, 12]. The pads of the result are 0."""
    pose = np.ascontiguousarray(pose, dtype=np.float32)
    out = np.zeros_like(pose)
    out[:, 0:4] = conjugate(pose[:, 0:4])
    out[:, 8:11] = ONE / pose[:, 8:11]
    scaled = np.zeros((pose.shape[0], 4), dtype=np.float32)
    scaled[:, 0:3] = out[:, 8:11] * pose[:, 4:7]
    for b in range(pose.shape[0]):
        inverse_rotation = out[b, 0:4]
        rotated = ob.oracle_quat_mul(ob.oracle_quat_mul(conjugate(inverse_rotation), scaled[b]), inverse_rotation)
        out[b, 4:7] = -rotated[0:3]
    return out


def takes_matrix_route(lhs, rhs):
    """rtm::qvv_mul leaves the quaternion path when a scale component of either side is negative; [B] bool"""
    return (np.minimum(lhs[:, 8:11], rhs[:, 8:11]) < 0).any(axis=1)


def is_root(parents):
    roots = np.asarray(parents, dtype=np.uint32) == NO_PARENT
    roots[0] = True
    return roots


def pairs_through_the_walk(first, second):
    """normalize(qvv_mul(second[k], first[k])) per k, pads 0: every pair is a root and its one child under oracle_local_to_object_space"""
    count = first.shape[0]
    if count == 0:
        return np.zeros((0, 12), dtype=np.float32)
    pose = np.empty((2 * count, 12), dtype=np.float32)
    pose[0::2], pose[1::2] = first, second
    parents = np.full(2 * count, NO_PARENT, dtype=np.uint32)
    parents[1::2] = np.arange(count, dtype=np.uint32) * 2
    return ob.oracle_local_to_object_space(parents, pose)[1::2]


def object_to_local(parents, pose, reference_order=False):
    """(local pose, matrix route products). Roots keep their record whole, pads included; every other bone has pads 0.
    reference_order: the operand order of the reference's text, qvv_mul(inverse(object[parent]), object[bone])."""
    pose = np.ascontiguousarray(pose, dtype=np.float32)
    parents = np.asarray(parents, dtype=np.uint32)
    children = np.flatnonzero(~is_root(parents))
    inverses = inverse_pose(pose)[parents[children]]
    out = pose.copy()
    if reference_order:
        out[children] = pairs_through_the_walk(pose[children], inverses)
    else:
        out[children] = pairs_through_the_walk(inverses, pose[children])
    return out, int(takes_matrix_route(pose[children], inverses).sum())


def convert_to_additive(additive_format, base, pose):
    """(convert_to_relative / additive0 / additive1 of (base, transform = pose) per transform, matrix route products); pads 0"""
    base, pose = np.ascontiguousarray(base, dtype=np.float32), np.ascontiguousarray(pose, dtype=np.float32)
    if additive_format == RELATIVE:
        inverses = inverse_pose(base)
        return ob.oracle_apply_additive_to_base(RELATIVE, inverses, pose), int(takes_matrix_route(pose, inverses).sum())
    assert additive_format in (ADDITIVE0, ADDITIVE1)
    out = np.zeros_like(pose)
    base_conjugates = conjugate(base[:, 0:4])
    for b in range(pose.shape[0]):
        out[b, 0:4] = ob.oracle_quat_mul(pose[b, 0:4], base_conjugates[b])
    out[:, 4:7] = pose[:, 4:7] - base[:, 4:7]
    if additive_format == ADDITIVE0:
        out[:, 8:11] = pose[:, 8:11] / base[:, 8:11]
    else:
        out[:, 8:11] = (pose[:, 8:11] * (ONE / base[:, 8:11])) - ONE
    return out, 0


def expected_inverse_row(parents, pose, local_space=True, additive_format=NONE, base=None):
    """the header's definition of one row: (row, matrix route products)"""
    row, routed = np.ascontiguousarray(pose, dtype=np.float32), 0
    if local_space:
        row, routed = object_to_local(parents, row)
    if additive_format != NONE:
        row, more = convert_to_additive(additive_format, base, row)
        routed += more
    return row, routed


# ---- the properties ---------------------------------------------------------------------------------------------------------------

def forest(rng, num_bones, root_chance=0.08):
    parents = np.zeros(num_bones, dtype=np.uint32)
    parents[0] = NO_PARENT
    for i in range(1, num_bones):
        parents[i] = NO_PARENT if rng.uniform() < root_chance else rng.integers(max(0, i - 9), i)
    return parents


def rigid_poses(rng, n, num_bones, mirrored=True):
    """unit rotations, ONE scale per bone in [0.5, 2] (a sixth of the bones negated as (-s, -s, -s)), translations within +-10"""
    poses = np.zeros((n, num_bones, 12), dtype=np.float32)
    rotations = rng.normal(size=(n, num_bones, 4))
    poses[..., 0:4] = rotations / np.linalg.norm(rotations, axis=2, keepdims=True)
    poses[..., 4:7] = rng.uniform(-10.0, 10.0, size=(n, num_bones, 3))
    scales = rng.uniform(0.5, 2.0, size=(n, num_bones, 1))
    if mirrored:
        scales = np.where(rng.uniform(size=(n, num_bones, 1)) < 1.0 / 6.0, -scales, scales)
    poses[..., 8:11] = scales
    return poses


def relative_error(got, want):
    """max over the floats of |got - want| / max(1, |want|); a rotation is compared up to its sign (q and -q are one rotation, and
    rtm::quat_from_matrix on the matrix route picks the sign by its own rule)"""
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    flip = np.where((got[..., 0:4] * want[..., 0:4]).sum(axis=-1, keepdims=True) < 0.0, -1.0, 1.0)
    got = np.concatenate([got[..., 0:4] * flip, got[..., 4:]], axis=-1)
    return float((np.abs(got - want) / np.maximum(1.0, np.abs(want))).max())


def pushed_back(parents, object_pose, local_pose):
    """every composed local bone through the oracle's forward step with its parent's object transform: qvv_mul(local[b], object[parent])"""
    parents = np.asarray(parents, dtype=np.uint32)
    children = np.flatnonzero(~is_root(parents))
    out = local_pose.copy()
    out[children] = pairs_through_the_walk(object_pose[parents[children]], local_pose[children])
    return out


@pytest.fixture(scope="module")
def round_trip_cases():
    rng = np.random.default_rng(8101)
    parents = forest(rng, 300)
    return parents, rigid_poses(rng, 6, 300)


def test_the_composition_undoes_local_to_object_space(round_trip_cases):
    parents, poses = round_trip_cases
    worst, routed = 0.0, 0
    for pose in poses:
        local, count = object_to_local(parents, pose)
        routed += count
        assert np.isfinite(local).all()
        worst = max(worst, relative_error(pushed_back(parents, pose, local), pose))
    print(f"object -> local -> object: worst relative error {worst:.3e}, {routed} matrix route products")
    assert routed > 100                   # mirrored bones are part of the property
    assert worst <= BAR


def test_the_operand_order_of_the_reference_text_does_not(round_trip_cases):
    parents, poses = round_trip_cases
    worst = 0.0
    for pose in poses:
        local, _ = object_to_local(parents, pose, reference_order=True)
        worst = max(worst, relative_error(pushed_back(parents, pose, local), pose))
    print(f"the reference's operand order: worst relative error {worst:.3e}")
    assert worst > BAR


@pytest.mark.parametrize("additive_format", [RELATIVE, ADDITIVE0, ADDITIVE1])
def test_apply_additive_to_base_undoes_the_conversion(additive_format):
    rng = np.random.default_rng(8200 + additive_format)
    poses, bases = rigid_poses(rng, 6, 300), rigid_poses(rng, 6, 300)
    worst = 0.0
    for pose, base in zip(poses, bases):
        additive, _ = convert_to_additive(additive_format, base, pose)
        assert np.isfinite(additive).all() and np.all(additive[:, [7, 11]] == 0.0)
        worst = max(worst, relative_error(ob.oracle_apply_additive_to_base(additive_format, base, additive), pose))
    print(f"convert -> apply, format {additive_format}: worst relative error {worst:.3e}")
    assert worst <= BAR
