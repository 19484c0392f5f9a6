"""Poses and reference poses a CALLER hands over, outside the range in which the short exact forms are proven: the inputs of
tests/test_gpu_caller_pose_ranges.py and the conditions they have to meet, checked here with the oracle alone (no device).

sqrt_rn_short / rcp_rn_short (aclhip_device.h) give the bits of sqrtf / 1.0f / x for an argument of 0 or of at least 2^-96; the kernels
that read a caller's poses therefore normalize with the compiler's forms. Every other generator of the suite hands those launches
rotations of a squared length in [1/4, 4], where both forms agree, so nothing sees which one a kernel takes. The GAP: a normalize whose
float32 argument d -- x * x, then y * y + d, z * z + d, w * w + d, quat_normalize's order -- lies in 0 < d < 2^-96.

  gap_poses            rotations are unit quaternions times 2^e, e uniform in an exponent range; roots get e in [-1, 1] (the walk copies a
                       root as it is: a tiny root would send its children's products to 0 and the row to NaN); translations within +-10,
                       scales in [0.5, 2]
  GAP      [-70, -52]  non-root local, additive, blend, base and reference rotations: the walk's product with a normalized parent has a
                       squared length of 2^-140 .. 2^-104 (squares that are denormal: the device keeps IEEE denormals, as
                       tests/test_gpu_exact_math.py relies on)
  INVERSE  [-35, -26]  every object space rotation of the inverse launch, roots included: the product of TWO inputs is in the gap
  LARGE    [10, 30]    squares stay below 2^127; no role in the gap, it shows that nothing overflows early

A function per launch kind returns every normalize argument the launch meets, from oracle calls: the walk's is
oracle_quat_mul(local[b].rot, object[parent].rot) (aclo_qvv_mul: rotation = quat_mul(lhs.rot, rhs.rot) with lhs the local transform), the
inverse's the product with the parent's conjugate, the blend's the weighted sum (restated in numpy float32, one operation at a time, and
held to oracle_blend_poses through its normalize) and behind it the walk's. A case function per GPU test builds the inputs, the expected
rows and these arguments ONCE (functools.lru_cache); the GPU file calls the same functions with the same arguments, listed in GPU_TESTS.
The conditions, per GPU test: every expected row is finite, no argument is 0, and at least 500 normalizes lie in the gap (none in the
large class)."""
import functools
import types

import numpy as np
import pytest

from acl_amd import runtime, synth
from oracle import bindings as ob
import test_gpu_blend_masks as bm
import test_gpu_bone_object as bo
import test_gpu_pose_buffer_blend as bl
import test_gpu_pose_buffer_inverse as inv
import test_gpu_pose_buffers as pb
import test_gpu_skeleton_poses as sk
from test_pose_buffer_inverse_oracle import conjugate, is_root

NONE, RELATIVE, ADDITIVE0, ADDITIVE1 = pb.NONE, pb.RELATIVE, pb.ADDITIVE0, pb.ADDITIVE1
FORMATS = (RELATIVE, ADDITIVE0, ADDITIVE1)
WEIGHTED, LAYERED = bl.WEIGHTED, bl.LAYERED
DROPPED = sk.DROPPED
ONE = np.float32(1.0)
GAP_LIMIT = np.float32(2.0 ** -96)
GAP, INVERSE, LARGE = (-70.0, -52.0), (-35.0, -26.0), (10.0, 30.0)
RANGES = {"gap": GAP, "large": LARGE}
SHAPES = (65, 100)              # two lane passes; 4 instances per workgroup
N = 9                           # the batch ends inside a workgroup
MIN_GAP_NORMALIZES = 500


# ---- generators and arguments ---------------------------------------------------------------------------------------------------------

def gap_poses(rng, n, parents, exponent_range, root_exponent_range=(-1.0, 1.0)):
    """float32 [n, B, 12], the pads 0: unit quaternions times 2^e, e uniform in exponent_range (roots: root_exponent_range)"""
    num_bones = len(parents)
    poses = np.zeros((n, num_bones, 12), dtype=np.float32)
    rotations = rng.normal(size=(n, num_bones, 4))
    rotations /= np.linalg.norm(rotations, axis=2, keepdims=True)
    exponents = rng.uniform(exponent_range[0], exponent_range[1], size=(n, num_bones, 1))
    roots = is_root(parents)
    exponents[:, roots] = rng.uniform(root_exponent_range[0], root_exponent_range[1], size=(n, int(roots.sum()), 1))
    poses[..., 0:4] = rotations * np.exp2(exponents)
    poses[..., 4:7] = rng.uniform(-10.0, 10.0, size=(n, num_bones, 3))
    poses[..., 8:11] = rng.uniform(0.5, 2.0, size=(n, num_bones, 3))
    return poses


def normalize_argument(rotations):
    """quat_normalize's float32 argument, in its order; rotations [..., 4]"""
    q = np.asarray(rotations, dtype=np.float32)
    d = q[..., 0] * q[..., 0]
    d = (q[..., 1] * q[..., 1]) + d
    d = (q[..., 2] * q[..., 2]) + d
    d = (q[..., 3] * q[..., 3]) + d
    assert d.dtype == np.float32
    return d


def normalized(rotations):
    """quat_normalize itself: 1 / sqrt(d), then the four products (numpy's float32 sqrt and division are correctly rounded)"""
    q = np.asarray(rotations, dtype=np.float32)
    inv_len = ONE / np.sqrt(normalize_argument(q))
    return q * inv_len[..., None]


def in_gap(arguments):
    arguments = np.asarray(arguments, dtype=np.float32)
    return (arguments > 0) & (arguments < GAP_LIMIT)


def walk_arguments(parents, local):
    """(the object space pose, the argument of every non-root bone's normalize); local [B, 12]"""
    parents = np.asarray(parents, dtype=np.uint32)
    local = np.ascontiguousarray(local, dtype=np.float32)
    object_pose = ob.oracle_local_to_object_space(parents, local)
    children = np.flatnonzero(~is_root(parents))
    products = np.stack([ob.oracle_quat_mul(local[b, 0:4], object_pose[parents[b], 0:4]) for b in children]) if children.size else np.zeros((0, 4), dtype=np.float32)
    with np.errstate(all="ignore"):
        arguments = normalize_argument(products)
        # the product IS what the walk normalizes: its normalize gives the oracle's rotation (positive scales: no matrix route)
        finite = np.isfinite(object_pose[children]).all(axis=1)
        assert np.array_equal(pb.bits(normalized(products)[finite]), pb.bits(object_pose[children, 0:4][finite]))
    return object_pose, arguments


def inverse_arguments(parents, source):
    """the argument of every non-root bone's normalize in object -> local space: quat_mul(X[b].rot, conjugate(X[parent].rot))"""
    parents = np.asarray(parents, dtype=np.uint32)
    children = np.flatnonzero(~is_root(parents))
    conjugates = conjugate(source[:, 0:4])
    products = np.stack([ob.oracle_quat_mul(source[b, 0:4], conjugates[parents[b]]) for b in children])
    return normalize_argument(products)


def blend_arguments(poses, per_slot, blended):
    """the argument of every slot's normalize in a blend: the weighted sum of include/aclhip.h (aclo_blend_poses' accumulation restated in
    float32), held to the oracle's row `blended` through its normalize. poses: K arrays [B, 12]; per_slot: float32 [K, B]."""
    accumulated = poses[0][:, 0:4] * per_slot[0][:, None]
    for k in range(1, len(poses)):
        q = poses[k][:, 0:4]
        dot = accumulated[:, 0] * q[:, 0]
        dot = dot + (accumulated[:, 1] * q[:, 1])
        dot = dot + (accumulated[:, 2] * q[:, 2])
        dot = dot + (accumulated[:, 3] * q[:, 3])
        signed = np.where(dot < 0, -per_slot[k], per_slot[k]).astype(np.float32)
        accumulated = (q * signed[:, None]) + accumulated
    assert accumulated.dtype == np.float32
    assert np.array_equal(pb.bits(normalized(accumulated)), pb.bits(blended[:, 0:4]))
    return normalize_argument(accumulated)


def case_of(rows, arguments, **fields):
    """rows: the expected rows of the case's launches (a list of arrays); arguments: every normalize argument behind them"""
    return types.SimpleNamespace(rows=rows, arguments=np.concatenate([np.asarray(a, dtype=np.float32).reshape(-1) for a in arguments]), **fields)


def few_roots_forest(rng, num_bones):
    """pb.forest with fewer roots (more walked bones per pose), still several"""
    while True:
        parents = pb.forest(rng, num_bones, root_chance=0.04)
        if 2 <= int((parents == runtime.NO_PARENT).sum()) <= 5:
            return parents


# ---- a. aclhip_transform_poses_batch --------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def transform_case(num_bones, additive_format=NONE, special_buffer="local", klass="gap"):
    """the `klass` rotations in the local or in the additive buffer, in range ones (pb.random_poses) in the other; object space"""
    rng = np.random.default_rng(31000 + num_bones * 64 + additive_format * 8 + (4 if special_buffer == "additive" else 0) + (2 if klass == "large" else 0))
    parents = few_roots_forest(rng, num_bones)
    special, plain = gap_poses(rng, N, parents, RANGES[klass]), pb.random_poses(rng, N, num_bones, scale=(0.5, 1.5))
    local, additive = (special, plain) if special_buffer == "local" else (plain, special)
    additive = additive if additive_format != NONE else None
    rows = pb.expected_rows(local, parents, additive_format, additive)
    arguments = []
    for i in range(N):
        pose = local[i] if additive_format == NONE else ob.oracle_apply_additive_to_base(additive_format, local[i], additive[i])
        object_pose, walked = walk_arguments(parents, pose)
        assert np.array_equal(pb.bits(object_pose), pb.bits(rows[i]))
        arguments.append(walked)
    return case_of(rows, arguments, parents=parents, local=local, additive=additive, additive_format=additive_format)


# ---- b. aclhip_blend_poses_batch ------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def blend_case(num_bones, num_buffers, mode, which):
    """which: "one" -- one buffer of gap rotations among in range ones, weights and masks such that it carries some slots alone (layered:
    it is the top layer at weight 1 under a mask with plateaus of 1; weighted: it is buffer 0 and every other buffer has one mask with
    plateaus of 0) --, "all" or "large": every buffer of that class, drawn weights and masks.
    masks: host arrays; handles: int [N, K] into them, -1 the null handle."""
    rng = np.random.default_rng(32000 + num_bones * 64 + num_buffers * 8 + mode * 4 + {"one": 0, "all": 1, "large": 2}[which])
    parents = few_roots_forest(rng, num_bones)
    inputs = bl.random_inputs(rng, num_buffers, N, num_bones)
    special = [num_buffers - 1 if mode == LAYERED else 0] if which == "one" else list(range(num_buffers))
    for k in special:
        inputs[k][..., 0:4] = gap_poses(rng, N, parents, RANGES["large" if which == "large" else "gap"])[..., 0:4]
    if which != "one":
        inputs[1][:, ::3, 0:4] = -inputs[0][:, ::3, 0:4]               # the sign bias decides, as in bl.random_inputs
    weights = bl.blend_weights(rng, mode, N, num_buffers)
    if mode == WEIGHTED:
        # no weight below 0.6 / K, and buffer 0 always under the null handle: a weight of 2^-6 on a rotation of 2^-70 would leave a sum
        # whose squares are all below the smallest denormal -- an argument of 0, a row of NaN
        weights = (rng.dirichlet(np.ones(num_buffers), size=N) * 0.4 + 0.6 / num_buffers).astype(np.float32)
    handles = np.full((N, num_buffers), -1, dtype=np.int64)
    if which == "one":
        masks = bl.make_masks(rng, num_bones, 1)
        if mode == LAYERED:
            weights[:, num_buffers - 1] = 1.0
            handles[:, num_buffers - 1] = 0
        else:
            handles[:, 1:] = 0
    else:
        masks = [np.ones(num_bones, dtype=np.float32)] + bl.make_masks(rng, num_bones, 2)
        if mode == LAYERED:
            handles[:, 0] = rng.choice([-1, 0], size=N)
        handles[:, 1:] = rng.choice([-1, 1, 2], size=(N, num_buffers - 1))
    local, rows, arguments, behind_the_blend = [], [], [], []
    for i in range(N):
        poses = [inputs[k][i] for k in range(num_buffers)]
        instance_masks = [None if h < 0 else masks[h] for h in handles[i]]
        blended = bl.expected_local(poses, weights[i], instance_masks, mode)
        arguments.append(blend_arguments(poses, bl.slot_weights(weights[i], instance_masks, mode, num_bones), blended))
        object_pose, walked = walk_arguments(parents, blended)
        arguments.append(walked)
        behind_the_blend.append(walked)
        local.append(blended)
        rows.append(object_pose)
    return case_of(local + rows, arguments, parents=parents, inputs=inputs, weights=weights, masks=masks, handles=handles, local=local, object_rows=rows,
                   walk_arguments=np.concatenate(behind_the_blend))


# ---- c. aclhip_inverse_transform_poses_batch ------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def inverse_case(num_bones, additive_format=NONE, klass="gap"):
    """local_space over object space rotations of the INVERSE class (roots included) or the large one; the base, when there is one, in range"""
    rng = np.random.default_rng(33000 + num_bones * 64 + additive_format * 8 + (2 if klass == "large" else 0))
    parents = few_roots_forest(rng, num_bones)
    exponents = INVERSE if klass == "gap" else LARGE
    source = gap_poses(rng, N, parents, exponents, root_exponent_range=exponents)
    base = pb.random_poses(rng, N, num_bones) if additive_format != NONE else None
    rows, _ = inv.expected_rows(source, parents, True, additive_format, base)
    return case_of(rows, [inverse_arguments(parents, source[i]) for i in range(N)], parents=parents, source=source, base=base, additive_format=additive_format)


# ---- d. and e.: the fused launches ----------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def rig(num_bones):
    """what the fused cases of one shape share: a hierarchy, a clip of num_bones tracks for the unmapped launch, three clips of fewer
    tracks with "dropped" maps of their own (slots no track maps to are filled and walked), and a unit and a gap class reference pose that
    differ in their rotations alone"""
    rng = np.random.default_rng(34000 + num_bones)
    parents = few_roots_forest(rng, num_bones)
    whole = synth.build_clip(seed=34100 + num_bones, num_tracks=num_bones, num_samples=21)
    clips = [synth.build_clip(seed=34200 + num_bones + k, num_tracks=30 + 3 * k, num_samples=17 + 4 * k, **(dict(has_scale=1, scale_default=0.3) if k == 1 else {})) for k in range(3)]
    tables = [sk.make_map(rng, 30 + 3 * k, num_bones, "dropped") for k in range(3)]
    unit = sk.reference_pose(rng, num_bones)
    gap = unit.copy()
    gap[:, 0:4] = gap_poses(rng, 1, parents, GAP)[0, :, 0:4]
    times = rng.uniform(0.0, min(clip.duration for clip in clips + [whole]), size=(4, N)).astype(np.float32)
    base = gap_poses(rng, N, parents, GAP)
    # the masked blend's weights: clip 0 at 0.3 or more under the null handle (see blend_case), clip 1 under a mask with zeros or the null handle
    weights = (rng.dirichlet(np.ones(2), size=N) * 0.4 + 0.3).astype(np.float32)
    masks = bm.make_masks(rng, num_bones, 1)
    handles = np.stack([np.full(N, -1), rng.choice([-1, 0], size=N)], axis=1)
    return types.SimpleNamespace(parents=parents, whole=whole, clips=clips, tables=tables, references={"unit": unit, "gap": gap}, times=times, base=base, weights=weights,
                                 masks=masks, handles=handles)


def masked_members(the, i):
    return [(the.clips[0].blob, the.times[0, i], the.tables[0]), (the.clips[1].blob, the.times[1, i], the.tables[1])]


def instance_masks_of(the, i):
    return [None if h < 0 else the.masks[h] for h in the.handles[i]]


def masked_blend_arguments(the, reference, additive_format, i):
    """the fused masked blend's normalize arguments: the skeleton poses of instance i's two clips over the fill (the reference pose, or the
    additive identity under an additive format), their slot weights, the weighted sum -- held to bm.masked_blend of the same poses"""
    fill = reference if additive_format == NONE else sk.additive_identity(reference.shape[0], additive_format)
    poses = [sk.skeleton_pose(blob, time, table, fill, 0, ob.default_options(looping_policy=2)) for blob, time, table in masked_members(the, i)]
    per_slot = bm.slot_weights(the.weights[i], instance_masks_of(the, i), WEIGHTED, reference.shape[0])
    return blend_arguments(poses, per_slot, bm.masked_blend(poses, per_slot))


@functools.lru_cache(maxsize=None)
def fused_case(num_bones, launch, additive_format):
    """aclhip_decompress_poses_batch ("unmapped"), its mapped ("mapped") and its masked ("masked") form, in object space, onto a caller's
    base_poses buffer whose non-root rotations are gap class: decode, oracle_apply_additive_to_base, oracle_local_to_object_space"""
    the = rig(num_bones)
    skeleton = (the.references["unit"], the.parents)
    rows, arguments = [], []
    for i in range(N):
        if launch == "unmapped":
            pose = ob.oracle_apply_additive_to_base(additive_format, the.base[i], ob.oracle_decompress_tracks(the.whole.blob, float(the.times[3, i])))
            want = ob.oracle_local_to_object_space(the.parents, pose)
        elif launch == "mapped":
            members = [(the.clips[0].blob, the.times[0, i], the.tables[0])]
            pose = sk.expected_pose(skeleton, members, None, additive_format, the.base[i], False, 0, 2)
            want = sk.expected_pose(skeleton, members, None, additive_format, the.base[i], True, 0, 2)
        else:
            common = (skeleton, masked_members(the, i), the.weights[i], instance_masks_of(the, i), WEIGHTED, additive_format, the.base[i])
            pose = bm.expected_masked_pose(*common, False, 0, 2)
            want = bm.expected_masked_pose(*common, True, 0, 2)
            arguments.append(masked_blend_arguments(the, skeleton[0], additive_format, i))
        object_pose, walked = walk_arguments(the.parents, pose)
        assert np.array_equal(pb.bits(object_pose), pb.bits(want))
        arguments.append(walked)
        rows.append(want)
    return case_of(rows, arguments, rig=the, additive_format=additive_format)


@functools.lru_cache(maxsize=None)
def skeleton_case(num_bones, launch, reference_class):
    """a registered skeleton whose reference pose has gap class non-root rotations ("gap"), or the otherwise equal one with unit rotations
    ("unit", the control), behind "dropped" maps: the mapped pose launch ("mapped"), the masked blend of two clips ("masked"), that blend
    as an additive0 layer onto a base CLIP with a map of its own ("masked_onto_base_clip": the reference rotations that fill the base's
    slots reach the walk unnormalized) and the mapped single bone object launch ("bone": every slot, once per instance time), object space"""
    the = rig(num_bones)
    reference = the.references[reference_class]
    skeleton = (reference, the.parents)
    rows, arguments = [], []
    for i in range(N):
        if launch in ("mapped", "bone"):
            members = [(the.clips[0].blob, the.times[0, i], the.tables[0])]
            pose = sk.expected_pose(skeleton, members, None, NONE, None, False, 0, 2)
            want = sk.expected_pose(skeleton, members, None, NONE, None, True, 0, 2)
        else:
            additive_format = ADDITIVE0 if launch == "masked_onto_base_clip" else NONE
            base = (the.clips[2].blob, the.times[2, i], the.tables[2]) if additive_format != NONE else None
            common = (skeleton, masked_members(the, i), the.weights[i], instance_masks_of(the, i), WEIGHTED, additive_format, base)
            pose = bm.expected_masked_pose(*common, False, 0, 2)
            want = bm.expected_masked_pose(*common, True, 0, 2)
            arguments.append(masked_blend_arguments(the, reference, additive_format, i))
        object_pose, walked = walk_arguments(the.parents, pose)
        assert np.array_equal(pb.bits(object_pose), pb.bits(want))
        if launch == "bone":
            # a request walks its bone's chain: one normalize per non-root bone of it (the requested bone included)
            assert np.array_equal(pb.bits(want), pb.bits(bo.skeleton_object_pose(the.clips[0].blob, the.times[0, i], the.tables[0], reference, the.parents, 0, 2)))
            children = np.flatnonzero(~is_root(the.parents))
            argument_of = dict(zip(children.tolist(), walked.tolist()))
            for slot in range(num_bones):
                bone = slot
                while not is_root(the.parents)[bone]:
                    arguments.append([argument_of[bone]])
                    bone = int(the.parents[bone])
        else:
            arguments.append(walked)
        rows.append(want)
    return case_of(rows, arguments, rig=the, reference=reference)


# ---- f. non-finite rows ---------------------------------------------------------------------------------------------------------------

POISONED = (1, 2, 5)
POISON_BONES = 100
POISON_SEEDS = {"transform": 35001, "blend": 35002, "inverse": 35003}


def descendants(parents, bone):
    """bool [B]: the bones below `bone` (parents come first)"""
    below = np.zeros(len(parents), dtype=bool)
    for b in range(bone + 1, len(parents)):
        below[b] = parents[b] != runtime.NO_PARENT and (parents[b] == bone or below[parents[b]])
    return below


def mid_tree_bones(parents):
    """two non-root bones, neither below the other, each with two descendants or more and at most a third of the bones below it"""
    roots = is_root(parents)
    found = []
    for bone in range(1, len(parents)):
        below = descendants(parents, bone)
        if not roots[bone] and 2 <= below.sum() <= len(parents) // 3 and all(not descendants(parents, other)[bone] for other in found):
            found.append(bone)
            if len(found) == 2:
                return found
    raise AssertionError("the hierarchy has no two such bones")


def poison(poses, parents):
    """a copy of poses [n, B, 12] with instances 1, 2 and 5 poisoned, and the two bones: instance 1 a NaN translation component on the
    first bone; instance 2 a +inf translation component on it and an all-zero rotation on the second; instance 5 a NaN rotation
    component on the first. Scales stay what they were."""
    first, second = mid_tree_bones(parents)
    out = poses.copy()
    out[1, first, 5] = np.nan
    out[2, first, 4] = np.inf
    out[2, second, 0:4] = 0.0
    out[5, first, 2] = np.nan
    return out, first, second


@functools.lru_cache(maxsize=None)
def poison_case(launch):
    """"transform" (object space), "blend" (K = 2, weighted, no masks, object space; the poison sits in buffer 0, and the all-zero rotation
    in BOTH buffers, so that the weighted sum -- the blend's own normalize argument -- is 0 there) or "inverse" (local_space).
    clean / poisoned: the launch's input (K inputs for the blend); rows: the oracle over the poisoned input."""
    rng = np.random.default_rng(POISON_SEEDS[launch])
    parents = few_roots_forest(rng, POISON_BONES)
    with np.errstate(all="ignore"):
        if launch == "blend":
            clean = bl.random_inputs(rng, 2, N, POISON_BONES)
            spoiled, first, second = poison(clean[0], parents)
            zeroed = clean[1].copy()
            zeroed[2, second, 0:4] = 0.0
            poisoned = [spoiled, zeroed]
            weights = bl.blend_weights(rng, WEIGHTED, N, 2)
            rows = []
            for i in range(N):
                per_slot = bl.slot_weights(weights[i], [None, None], WEIGHTED, POISON_BONES)
                rows.append(ob.oracle_local_to_object_space(parents, bl.masked_blend([poisoned[0][i], poisoned[1][i]], per_slot)))
        else:
            clean, weights = pb.random_poses(rng, N, POISON_BONES), None
            poisoned, first, second = poison(clean, parents)
            rows = pb.expected_rows(poisoned, parents) if launch == "transform" else inv.expected_rows(poisoned, parents)[0]
    flags = descendants(parents, first)
    flags[first] = True
    return types.SimpleNamespace(parents=parents, clean=clean, poisoned=poisoned, weights=weights, rows=rows, first=first, second=second, flags=flags.astype(np.uint8))


# ---- the GPU file's tests and the cases each of them runs -----------------------------------------------------------------------------

def _both_shapes(build, *arguments):
    return lambda: [build(num_bones, *arguments) for num_bones in SHAPES]


GPU_TESTS = {}
for _klass in ("gap", "large"):
    GPU_TESTS[f"test_transform_object_space_alone[{_klass}]"] = (_klass, _both_shapes(transform_case, NONE, "local", _klass))
    GPU_TESTS[f"test_inverse_to_local_space[{_klass}]"] = (_klass, _both_shapes(inverse_case, NONE, _klass))
GPU_TESTS["test_transform_bounds"] = ("gap", _both_shapes(transform_case, NONE, "local", "gap"))
for _format in FORMATS:
    for _buffer in ("local", "additive"):
        GPU_TESTS[f"test_transform_additive[{_buffer}-{_format}]"] = ("gap", _both_shapes(transform_case, _format, _buffer, "gap"))
    GPU_TESTS[f"test_transform_additive_large[{_format}]"] = ("large", _both_shapes(transform_case, _format, "local", "large"))
    GPU_TESTS[f"test_inverse_make_additive[{_format}]"] = ("gap", _both_shapes(inverse_case, _format, "gap"))
    for _launch in ("unmapped", "mapped", "masked"):
        GPU_TESTS[f"test_fused_onto_a_gap_base_buffer[{_launch}-{_format}]"] = ("gap", _both_shapes(fused_case, _launch, _format))
for _buffers in (2, 4):
    for _mode in (WEIGHTED, LAYERED):
        GPU_TESTS[f"test_blend[{_buffers}-{_mode}]"] = ("gap", lambda buffers=_buffers, mode=_mode: [blend_case(b, buffers, mode, which) for b in SHAPES for which in ("one", "all")])
        GPU_TESTS[f"test_blend_large[{_buffers}-{_mode}]"] = ("large", _both_shapes(blend_case, _buffers, _mode, "large"))
for _launch in ("mapped", "masked", "masked_onto_base_clip", "bone"):
    GPU_TESTS[f"test_gap_reference_pose[{_launch}]"] = ("gap", _both_shapes(skeleton_case, _launch, "gap"))


@pytest.mark.parametrize("name", sorted(GPU_TESTS))
def test_the_conditions_of_every_gpu_test(name):
    klass, cases = GPU_TESTS[name]
    gap_normalizes = 0
    for case in cases():
        assert all(np.isfinite(row).all() for row in case.rows), name
        assert case.arguments.size > 0 and np.isfinite(case.arguments).all() and not (case.arguments == 0).any(), name
        gap_normalizes += int(in_gap(case.arguments).sum())
    print(f"{name}: {gap_normalizes} normalizes in the gap")
    if klass == "gap":
        assert gap_normalizes >= MIN_GAP_NORMALIZES
    else:
        assert gap_normalizes == 0


def test_the_walk_behind_a_blend_never_meets_the_gap():
    """The blend normalizes every rotation, roots included, in front of its walk: the walk's product of two of them has a squared length
    near 1 whatever the inputs were (0.978 .. 1.021 over these cases; the squares of a gap class sum are denormal, so its normalize is a
    few 2^-10 off). No finite input puts that argument below 2^-96, where the short forms differ -- exponents below -74 take the blend's
    own argument to 0 first. So the blend kernel's choice for its WALK (kernels_pose_buffers.inl: short_exact = 0 behind
    blend_normalize_rotations) cannot show in any output, and no test of the GPU file can depend on it; the blend's own normalize can."""
    for num_bones in SHAPES:
        for num_buffers in (2, 4):
            for mode in (WEIGHTED, LAYERED):
                for which in ("one", "all", "large"):
                    walked = blend_case(num_bones, num_buffers, mode, which).walk_arguments
                    assert walked.size > 0 and (walked >= 0.25).all() and (walked <= 4.0).all(), (num_bones, num_buffers, mode, which, walked.min(), walked.max())


def test_the_generator_meets_its_description():
    rng = np.random.default_rng(30001)
    parents = few_roots_forest(rng, 100)
    roots = is_root(parents)
    for exponents in (GAP, INVERSE, LARGE):
        poses = gap_poses(rng, N, parents, exponents)
        lengths = np.log2(np.linalg.norm(poses[..., 0:4].astype(np.float64), axis=2))
        assert (lengths[:, ~roots] >= exponents[0] - 1e-6).all() and (lengths[:, ~roots] <= exponents[1] + 1e-6).all()
        assert (np.abs(lengths[:, roots]) <= 1.0 + 1e-6).all()
        assert (np.abs(poses[..., 4:7]) <= 10.0).all() and (poses[..., 8:11] >= 0.5).all() and (poses[..., 8:11] <= 2.0).all()
        assert not poses[..., [7, 11]].any()
    # a gap class rotation alone is NOT in the gap's reach of the short forms' proof either way: its own squared length is below 2^-96
    assert in_gap(normalize_argument(gap_poses(rng, N, parents, GAP)[:, ~roots, 0:4])).all()
    assert not in_gap(normalize_argument(gap_poses(rng, N, parents, LARGE)[..., 0:4])).any()
    assert np.isfinite(normalize_argument(gap_poses(rng, N, parents, LARGE)[..., 0:4] * np.float32(2.0 ** 30))).all()      # the product of two: squares below 2^127


def test_the_control_skeleton_differs_in_its_rotations_alone():
    for num_bones in SHAPES:
        the = rig(num_bones)
        unit, gap = the.references["unit"], the.references["gap"]
        assert np.array_equal(unit[:, 4:], gap[:, 4:])
        roots = is_root(the.parents)
        assert in_gap(normalize_argument(gap[~roots, 0:4])).all() and not in_gap(normalize_argument(unit[:, 0:4])).any()
        # registration clears the short exact bit on a squared length outside [1/4, 4] (host_skeletons.inl): the gap reference has one
        assert (normalize_argument(gap[~roots, 0:4]) < 0.25).all()
        for table in the.tables:
            filled = np.setdiff1d(np.arange(num_bones), table[table != DROPPED])
            assert (~roots[filled]).sum() >= 20                                            # reference rotations fill slots that are walked
            assert np.isin(the.parents[~roots], filled).any()                              # and some bone sits below a filled slot


@pytest.mark.parametrize("launch", ["transform", "blend", "inverse"])
def test_the_poisoned_rows(launch):
    case = poison_case(launch)
    parents, first, second = case.parents, case.first, case.second
    roots = is_root(parents)
    assert not roots[first] and not roots[second]
    for bone in (first, second):
        below = descendants(parents, bone)
        assert below.any() and not below[np.arange(len(parents)) != bone].all()
    rows = np.stack(case.rows)
    clean = [i for i in range(N) if i not in POISONED]
    assert np.isfinite(rows[clean]).all()
    for i in POISONED:
        assert np.isnan(rows[i]).any() and not np.isnan(rows[i]).all()                     # the class comparison has both kinds to compare
    if launch == "blend":
        # the weighted sum of two all-zero rotations is 0: the blend's own normalize meets an argument of 0 and gives NaN
        assert not case.poisoned[0][2, second, 0:4].any() and not case.poisoned[1][2, second, 0:4].any()
        assert np.isnan(rows[2][second, 0:4]).all()
    if launch != "inverse":
        # the parent's rotation spreads the one NaN coordinate over all three, and every descendant adds it to its own: under case.flags
        # every counted coordinate of instance 1 is NaN, and every other bone's is a number
        assert np.isnan(rows[1][case.flags.astype(bool), 4:7]).all()
        assert np.isfinite(rows[1][~case.flags.astype(bool), 4:7]).all()
        assert np.isposinf(rows[2][..., 4:7]).any() or np.isnan(rows[2][..., 4:7]).any()
