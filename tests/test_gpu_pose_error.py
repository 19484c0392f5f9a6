"""aclhip_measure_pose_error_batch through the C ABI: the shell error of two pose buffers the caller filled. The expected records are
the composition of tests/test_pose_error_oracle.py (the oracle's functions plus numpy float32 element operations), compared on bits:
`errors` whole, `bone_errors` wherever the value is not a NaN (a NaN is a NaN there, of whatever payload), `worst` whole -- each inside a
sentinel filled buffer with guards before, behind and, for bone_errors, at the end of every row. The kernel and the composition run the
same operation order, so there is no tolerance anywhere. Every launch has 17 instances: more than one workgroup, an odd count. The
input buffers are asserted unchanged. Needs a GPU."""
import numpy as np
import pytest

from acl_amd import runtime, synth
from oracle import bindings as ob
from test_gpu_pose_buffers import SENTINEL, Buffers, bits, identity_pose
from test_pose_error_oracle import NO_BONE, expected_measure, forest, loose_poses, scan_worst

pytestmark = pytest.mark.gpu

NONE, RELATIVE, ADDITIVE0, ADDITIVE1 = runtime.ADDITIVE_NONE, runtime.ADDITIVE_RELATIVE, runtime.ADDITIVE_ADDITIVE0, runtime.ADDITIVE_ADDITIVE1
N = 17
SENTINEL_BITS = int(np.float32(SENTINEL).view(np.uint32))
NOT_MEASURED = (np.float32(-1.0), NO_BONE)


def signed_poses(rng, n, num_bones):
    """loose_poses with scale magnitudes spread evenly over the octaves of [0.25, 4] (their product along a chain stays finite) and a
    sixth of the scale components negative"""
    poses = loose_poses(rng, n, num_bones)
    magnitudes = np.exp2(rng.uniform(-2.0, 2.0, size=(n, num_bones, 3)))
    poses[..., 8:11] = np.where(rng.uniform(size=magnitudes.shape) < 1.0 / 6.0, -magnitudes, magnitudes)
    return poses


def expected_batch(parents, raw, lossy, shells, object_space=True, additive_format=NONE, base=None):
    """per instance (bone errors, record) and the batch's matrix route products; parents: one hierarchy, or one per instance"""
    rows, records, routed = [], [], 0
    for i in range(len(raw)):
        errors, record, count = expected_measure(parents[i] if isinstance(parents, list) else parents, raw[i], lossy[i], shells, object_space, additive_format,
                                                 base[i] if base is not None else None)
        rows.append(errors)
        records.append(record)
        routed += count
    return rows, records, routed


class Measured:
    pass


def launch(ctx, raw, lossy, skeleton=0, instance_skeletons=None, object_space=True, additive_format=NONE, base=None, shells=3.0, num_shells=None, with_bone_errors=True,
           with_worst=True, raw_row_bones=None, lossy_row_bones=None, base_row_bones=None, error_row_bones=None, same_buffer=False, n=None, stream=None):
    """One launch over `raw` and `lossy` ([n, B, 12], or lists of per instance poses); every buffer has a stride of its own. Returns a
    Measured: records [n] (error, bone), bone_errors [n + 2, row] float32 with its guards, worst (error, bone, instance, reserved)."""
    import torch
    n = len(raw) if n is None else n
    largest = max([pose.shape[0] for pose in raw] + [1])
    raw_floats = (raw_row_bones if raw_row_bones is not None else largest) * 12 + 4
    lossy_floats = raw_floats if same_buffer else (lossy_row_bones if lossy_row_bones is not None else largest) * 12 + 8
    error_floats = (error_row_bones if error_row_bones is not None else largest) + 3
    buffers = Buffers(len(raw), raw_floats)
    h_raw = buffers.host(raw, raw_floats)
    d_raw = buffers.up(h_raw)
    h_lossy = h_raw if same_buffer else buffers.host(lossy, lossy_floats)
    d_lossy = d_raw if same_buffer else buffers.up(h_lossy)
    d_errors = buffers.up(np.full((len(raw) + 2, 2), SENTINEL, dtype=np.float32))
    d_bone_errors = buffers.up(np.full((len(raw) + 2, error_floats), SENTINEL, dtype=np.float32))
    d_worst = buffers.up(np.full((3, 4), SENTINEL, dtype=np.float32))
    desc = runtime.PoseErrorDesc()
    desc.skeleton, desc.object_space, desc.additive_format = skeleton, 1 if object_space else 0, additive_format
    if instance_skeletons is not None:
        desc.instance_skeletons = buffers.up(np.asarray(instance_skeletons, dtype=np.uint32)).data_ptr()
    if additive_format != NONE:
        base_floats = (base_row_bones if base_row_bones is not None else largest) * 12 + 12
        h_base = buffers.host(base, base_floats)
        d_base = buffers.up(h_base)
        desc.base_poses, desc.base_pose_stride_bytes = d_base[1].data_ptr(), base_floats * 4
    if np.ndim(shells) == 0:
        desc.shell_distance = float(shells)
    else:
        d_shells = buffers.up(np.asarray(shells, dtype=np.float32))
        desc.shell_distances, desc.num_shell_distances = d_shells.data_ptr(), num_shells if num_shells is not None else d_shells.numel()
    if with_bone_errors:
        desc.bone_errors, desc.bone_error_stride_bytes = d_bone_errors[1].data_ptr(), error_floats * 4
    if with_worst:
        desc.worst = d_worst[1].data_ptr()
    arguments = (d_raw[1].data_ptr(), raw_floats * 4, d_lossy[1].data_ptr(), lossy_floats * 4, n, desc, d_errors[1].data_ptr())
    ctx.measure_pose_error(*arguments, stream=stream if stream is not None else buffers.stream())
    out = Measured()
    out.buffers, out.arguments, out.tensors = buffers, arguments, (d_errors, d_bone_errors, d_worst)
    if stream is not None:
        return out
    torch.cuda.synchronize()
    read_back(out)
    assert np.array_equal(bits(buffers.down(d_raw)), bits(h_raw)) and np.array_equal(bits(buffers.down(d_lossy)), bits(h_lossy))      # the inputs are only read
    if additive_format != NONE:
        assert np.array_equal(bits(buffers.down(d_base)), bits(h_base))
    return out


def read_back(out):
    d_errors, d_bone_errors, d_worst = out.tensors
    errors = d_errors.cpu().numpy()
    count = errors.shape[0] - 2
    assert np.all(bits(errors[[0, count + 1]]) == SENTINEL_BITS)                      # the guards around errors
    out.error_bits = bits(errors[1:1 + count]).copy()
    out.records = [(np.float32(error), int(bone)) for error, bone in zip(errors[1:1 + count, 0], bits(errors[1:1 + count, 1]))]
    out.bone_errors = d_bone_errors.cpu().numpy()
    worst = d_worst.cpu().numpy()
    assert np.all(bits(worst[[0, 2]]) == SENTINEL_BITS)                               # the guards around worst
    out.worst_written = not np.all(bits(worst[1]) == SENTINEL_BITS)
    words = bits(worst[1])
    out.worst = (np.float32(worst[1, 0]), int(words[1]), int(words[2]), int(words[3]))


def same_record(got, want):
    return bits(np.float32(got[0])) == bits(np.float32(want[0])) and got[1:] == tuple(want[1:])


def check(out, rows, records):
    """records on bits; bone_errors on bits wherever the expectation is not a NaN, a NaN there, the sentinel everywhere else (a row that
    is None stays untouched); worst against the host's scan of the expected records"""
    count = len(records)
    for i, (got, want) in enumerate(zip(out.records, records)):
        assert same_record(got, want), (i, got, want)
    assert len(out.records) >= count and np.all(out.error_bits[count:] == SENTINEL_BITS)          # (a launch of fewer instances than rows)
    want = np.full(out.bone_errors.shape, SENTINEL, dtype=np.float32)
    for i, row in enumerate(rows):
        if row is not None:
            want[1 + i, : row.size] = row
    numbers = ~np.isnan(want)
    assert np.array_equal(bits(out.bone_errors)[numbers], bits(want)[numbers]), np.argwhere((bits(out.bone_errors) != bits(want)) & numbers)[:8]
    assert np.all(np.isnan(out.bone_errors[~numbers]))
    if out.worst_written:
        assert same_record(out.worst, scan_worst(records) + (0,)), (out.worst, scan_worst(records))
    return out


FOREST_BONES = [1, 63, 64, 65, 100, 200, 300, 1200]


@pytest.fixture(scope="module")
def forest_cases():
    """B -> (parents, raw, lossy, {object_space: (rows, records, routed)}), computed once"""
    cases = {}
    for num_bones in FOREST_BONES:
        rng = np.random.default_rng(6100 + num_bones)
        parents = forest(rng, num_bones)
        raw, lossy = signed_poses(rng, N, num_bones), signed_poses(rng, N, num_bones)
        # half of the instances: a lossy pose close to the raw one, as a codec leaves it
        lossy[::2] = raw[::2] * (1.0 + rng.uniform(-1.0e-3, 1.0e-3, size=raw[::2].shape)).astype(np.float32)
        expected = {}
        for object_space in (True, False):
            expected[object_space] = expected_batch(parents, raw, lossy, 3.0, object_space)
            assert np.isfinite(np.stack(expected[object_space][0])).all()
        cases[num_bones] = (parents, raw, lossy, expected)
    return cases


@pytest.mark.parametrize("object_space", [True, False])
@pytest.mark.parametrize("num_bones", FOREST_BONES)
def test_random_forests_are_the_composition(forest_cases, num_bones, object_space):
    """lane stride edges (63 / 64 / 65: the second wave's first bone), 4, 2 and 1 image pairs per workgroup (100 / 200 / 300 and 1200
    bones), a batch that ends inside a workgroup; scales of both signs: the walk's matrix route and its counter"""
    parents, raw, lossy, expected = forest_cases[num_bones]
    rows, records, routed = expected[object_space]
    assert num_bones < 20 or int((parents == runtime.NO_PARENT).sum()) > 1        # several roots
    with runtime.Context(0) as ctx:
        skeleton = ctx.register_skeleton(parents, identity_pose(num_bones))
        before = ctx.negative_scale_count()
        out = check(launch(ctx, raw, lossy, skeleton=skeleton, object_space=object_space), rows, records)
        assert out.worst_written and out.worst[0] > 0.0
        assert ctx.negative_scale_count() - before == routed
        assert (routed > 0) == (object_space and num_bones > 1)
        # without the optional outputs: the same records, and neither of the two buffers is touched
        bare = launch(ctx, raw, lossy, skeleton=skeleton, object_space=object_space, with_bone_errors=False, with_worst=False)
        check(bare, [None] * N, records)
        assert not bare.worst_written
        assert ctx.rejected_instance_count() == 0


def test_mirrored_bones_take_the_matrix_route_and_are_counted():
    rng = np.random.default_rng(6201)
    num_bones = 100
    parents = forest(rng, num_bones)
    raw, lossy, base = signed_poses(rng, N, num_bones), signed_poses(rng, N, num_bones), signed_poses(rng, N, num_bones)
    plain = expected_batch(parents, raw, lossy, 2.0, True)
    relative = expected_batch(parents, raw, lossy, 2.0, True, RELATIVE, base)
    local = expected_batch(parents, raw, lossy, 2.0, False, RELATIVE, base)
    assert plain[2] > 500 and local[2] > 500 and relative[2] > local[2] + 500
    with runtime.Context(0) as ctx:
        skeleton = ctx.register_skeleton(parents, identity_pose(num_bones))
        for (rows, records, routed), options in ((plain, {}), (relative, dict(additive_format=RELATIVE, base=base)),
                                                 (local, dict(object_space=False, additive_format=RELATIVE, base=base))):
            before = ctx.negative_scale_count()
            check(launch(ctx, raw, lossy, skeleton=skeleton, shells=2.0, **options), rows, records)
            assert ctx.negative_scale_count() - before == routed
        # the two launches this one stands for move the counter by as much
        consumers = runtime.PoseBufferConsumers()
        consumers.skeleton, consumers.object_space = skeleton, 1
        buffers = Buffers(N, num_bones * 12)
        before = ctx.negative_scale_count()
        for poses in (raw, lossy):
            d_in, d_out = buffers.up(buffers.host(poses)), buffers.up(buffers.host())
            ctx.transform_poses_batch(d_in[1].data_ptr(), num_bones * 48, N, consumers, d_out[1].data_ptr(), num_bones * 48, stream=buffers.stream())
            buffers.down(d_out)
        assert ctx.negative_scale_count() - before == plain[2]
        assert ctx.rejected_instance_count() == 0


@pytest.mark.parametrize("num_bones", [65, 100])
@pytest.mark.parametrize("object_space", [True, False])
@pytest.mark.parametrize("additive_format", [RELATIVE, ADDITIVE0, ADDITIVE1])
def test_the_three_additive_formats(additive_format, object_space, num_bones):
    rng = np.random.default_rng(6300 + num_bones * 8 + additive_format * 2 + int(object_space))
    parents = forest(rng, num_bones)
    raw, lossy, base = loose_poses(rng, N, num_bones), loose_poses(rng, N, num_bones), loose_poses(rng, N, num_bones)
    rows, records, _ = expected_batch(parents, raw, lossy, 1.5, object_space, additive_format, base)
    assert np.isfinite(np.stack(rows)).all()
    with runtime.Context(0) as ctx:
        # (without object_space no hierarchy is needed: a skeleton registered without parents serves it)
        skeleton = ctx.register_skeleton(parents if object_space else None, identity_pose(num_bones))
        check(launch(ctx, raw, lossy, skeleton=skeleton, object_space=object_space, additive_format=additive_format, base=base, shells=1.5), rows, records)
        # the base may be one of the inputs: it is only read
        rows, records, _ = expected_batch(parents, raw, lossy, 1.5, object_space, additive_format, raw)
        check(launch(ctx, raw, lossy, skeleton=skeleton, object_space=object_space, additive_format=additive_format, base=raw, shells=1.5), rows, records)
        assert ctx.rejected_instance_count() == 0


def test_a_shell_table_against_the_uniform_value():
    rng = np.random.default_rng(6401)
    num_bones = 100
    parents = forest(rng, num_bones)
    raw, lossy = loose_poses(rng, N, num_bones), loose_poses(rng, N, num_bones)
    table = rng.uniform(0.0, 5.0, size=num_bones + 20).astype(np.float32)
    table[[0, 7, 64, 99]] = 0.0
    with runtime.Context(0) as ctx:
        skeleton = ctx.register_skeleton(parents, identity_pose(num_bones))
        by_table = check(launch(ctx, raw, lossy, skeleton=skeleton, shells=table), *expected_batch(parents, raw, lossy, table)[:2])
        # a table of one value is the uniform launch, bit for bit; d = 0 included: the distance of the two origins
        for distance in (2.5, 0.0):
            rows, records, _ = expected_batch(parents, raw, lossy, distance)
            uniform = check(launch(ctx, raw, lossy, skeleton=skeleton, shells=distance), rows, records)
            flat = check(launch(ctx, raw, lossy, skeleton=skeleton, shells=np.full(num_bones, distance, dtype=np.float32)), rows, records)
            assert np.array_equal(bits(uniform.bone_errors), bits(flat.bone_errors)) and np.array_equal(uniform.error_bits, flat.error_bits)
        zero_rows = expected_batch(parents, raw, lossy, 0.0)[0]
        for bone in (0, 7, 64, 99):
            assert np.array_equal(bits(by_table.bone_errors[1:1 + N, bone]), bits(np.stack(zero_rows)[:, bone]))
        assert ctx.rejected_instance_count() == 0


def test_ties_go_to_the_lowest_bone_and_the_lowest_instance():
    rng = np.random.default_rng(6501)
    num_bones = 150
    parents = forest(rng, num_bones)
    parents[[1, 3, 70, 140]] = runtime.NO_PARENT          # roots: nothing above them takes part in their error
    raw = loose_poses(rng, N, num_bones)
    lossy = raw.copy()
    # instance 0: bones 0 and 1, identical records in both buffers; instance 1: bones 3 and 70 (the first and the second wave); instance
    # 2: bones 70 and 140 (the second wave twice); instance 3: bones 1 and 3 (two lanes of one pass). Everything else does not move.
    pairs = {0: (0, 1), 1: (3, 70), 2: (70, 140), 3: (1, 3)}
    for instance, (low, high) in pairs.items():
        raw[instance, high] = raw[instance, low]
        lossy[instance, low, 4:7] += np.float32(0.5)
        lossy[instance, high] = lossy[instance, low]
    # instances 5 and 11: the same rows, the greatest error of the launch
    lossy[5, 9, 4:7] += np.float32(64.0)
    raw[11], lossy[11] = raw[5], lossy[5]
    rows, records, _ = expected_batch(parents, raw, lossy, 1.0, False)
    for instance, (low, high) in pairs.items():
        assert rows[instance][low] == rows[instance][high] > 0.0 and records[instance][1] == low
    assert records[5] == records[11] and scan_worst(records)[2] == 5
    with runtime.Context(0) as ctx:
        skeleton = ctx.register_skeleton(parents, identity_pose(num_bones))
        out = check(launch(ctx, raw, lossy, skeleton=skeleton, object_space=False, shells=1.0), rows, records)
        assert out.worst[1:3] == (9, 5)
        # and in object space, where the tied bones are roots
        rows, records, _ = expected_batch(parents, raw, lossy, 1.0, True)
        for instance, (low, high) in pairs.items():
            assert rows[instance][low] == rows[instance][high] > 0.0
        out = check(launch(ctx, raw, lossy, skeleton=skeleton, shells=1.0), rows, records)
        assert out.worst[2] == 5


def test_a_nan_never_wins():
    rng = np.random.default_rng(6601)
    num_bones = 100
    parents = forest(rng, num_bones)
    leaves = np.setdiff1d(np.arange(num_bones), parents)
    raw, lossy = loose_poses(rng, N, num_bones), loose_poses(rng, N, num_bones)
    nan = np.float32(np.nan)
    lossy[2, leaves[0], 5] = nan                 # one leaf
    raw[4, leaves[-1], 0] = nan                  # a leaf of the second wave
    lossy[6, 0, 9] = nan                         # a root: every bone below it
    lossy[8, :, 4] = nan                         # every bone
    raw[9, :, 0:4] = nan
    for object_space in (True, False):
        rows, records, _ = expected_batch(parents, raw, lossy, 1.0, object_space)
        assert np.isnan(rows[2][leaves[0]]) and int(np.isnan(rows[2]).sum()) == 1 and records[2][1] != leaves[0]
        assert np.isnan(rows[4][leaves[-1]]) and leaves[-1] >= 64
        assert np.isnan(rows[6][0]) and (int(np.isnan(rows[6]).sum()) > 1) == object_space
        assert records[8] == NOT_MEASURED and records[9] == NOT_MEASURED and np.isnan(rows[8]).all()
        with runtime.Context(0) as ctx:
            skeleton = ctx.register_skeleton(parents, identity_pose(num_bones))
            out = check(launch(ctx, raw, lossy, skeleton=skeleton, object_space=object_space, shells=1.0), rows, records)
            assert np.isnan(out.bone_errors[1 + 8, :num_bones]).all() and out.worst[2] not in (8, 9)
            assert ctx.rejected_instance_count() == 0


@pytest.mark.parametrize("object_space", [True, False])
def test_the_same_buffer_twice_gives_zero_and_bone_zero(object_space):
    rng = np.random.default_rng(6701)
    num_bones = 100
    parents = forest(rng, num_bones)
    raw = signed_poses(rng, N, num_bones)
    with runtime.Context(0) as ctx:
        skeleton = ctx.register_skeleton(parents, identity_pose(num_bones))
        out = launch(ctx, raw, raw, skeleton=skeleton, object_space=object_space, same_buffer=True)
        check(out, [np.zeros(num_bones, dtype=np.float32)] * N, [(np.float32(0.0), 0)] * N)
        assert out.worst == (0.0, 0, 0, 0)


def test_skeletons_per_instance_and_refusals():
    import torch
    rng = np.random.default_rng(6801)
    small, large = 40, 100
    parents = {small: forest(rng, small, root_chance=0.2), large: forest(rng, large)}
    with runtime.Context(0) as ctx:
        handles = {bones: ctx.register_skeleton(parents[bones], identity_pose(bones)) for bones in (small, large)}
        flat = ctx.register_skeleton(None, identity_pose(small))                        # no hierarchy
        retired = ctx.register_skeleton(parents[small], identity_pose(small))
        ctx.unregister_skeleton(retired)
        torch.cuda.synchronize()

        # different bone counts inside one workgroup: an error row is written up to its own skeleton's 4 * B
        which = [large, small, small, large, small, large, large, small, large, small, small, large, large, large, small, large, small]
        assert len(which) == N
        raw = [loose_poses(rng, 1, bones)[0] for bones in which]
        lossy = [loose_poses(rng, 1, bones)[0] for bones in which]
        base = [loose_poses(rng, 1, bones)[0] for bones in which]
        ids = [handles[bones] for bones in which]
        per_instance = [parents[bones] for bones in which]
        rows, records, _ = expected_batch(per_instance, raw, lossy, 3.0)
        out = check(launch(ctx, raw, lossy, instance_skeletons=ids), rows, records)
        assert np.all(out.bone_errors[2, small:] == SENTINEL)
        rows, records, _ = expected_batch(per_instance, raw, lossy, 3.0, True, ADDITIVE1, base)
        check(launch(ctx, raw, lossy, skeleton=handles[small], instance_skeletons=ids, additive_format=ADDITIVE1, base=base), rows, records)  # a launch wide skeleton is ignored next to the list
        assert ctx.rejected_instance_count() == 0

        # handle 0, an unknown handle, a retired one, object_space without a hierarchy: refused and counted, the record "not measured",
        # the error row what it was
        raw = [loose_poses(rng, 1, small)[0] for _ in range(N)]
        lossy = [loose_poses(rng, 1, small)[0] for _ in range(N)]
        ids = [handles[small]] * N
        ids[1], ids[2], ids[4], ids[5], ids[16] = 0, 0x00ABCDEF, retired, flat, 0xFFFFFFFF
        refused = [handle != handles[small] for handle in ids]
        rows, records, _ = expected_batch(parents[small], raw, lossy, 3.0)
        before = ctx.rejected_instance_count()
        check(launch(ctx, raw, lossy, instance_skeletons=ids), [None if no else row for no, row in zip(refused, rows)],
              [NOT_MEASURED if no else record for no, record in zip(refused, records)])
        assert ctx.rejected_instance_count() - before == sum(refused) == 5
        # in local space the skeleton without a hierarchy is served
        rows, records, _ = expected_batch(parents[small], raw, lossy, 3.0, False)
        before = ctx.rejected_instance_count()
        check(launch(ctx, raw, lossy, instance_skeletons=ids, object_space=False), [None if no and handle != flat else row for no, handle, row in zip(refused, ids, rows)],
              [NOT_MEASURED if no and handle != flat else record for no, handle, record in zip(refused, ids, records)])
        assert ctx.rejected_instance_count() - before == 4

        # B * 48 above each of the three strides in turn, 4 * B above the error stride, B above the shell table: every buffer but one
        # holds rows of `large` bones, that one rows of `small` bones (an input row too small for B is also an LDS image too small for B:
        # the images have min(raw, lossy stride) / 48 slots)
        which = [small, large] * 8 + [small]
        raw = [loose_poses(rng, 1, bones)[0] for bones in which]
        lossy = [loose_poses(rng, 1, bones)[0] for bones in which]
        base = [loose_poses(rng, 1, bones)[0] for bones in which]
        ids = [handles[bones] for bones in which]
        shells = rng.uniform(0.5, 2.0, size=large).astype(np.float32)
        rows, records, _ = expected_batch([parents[bones] for bones in which], raw, lossy, shells, True, ADDITIVE0, base)
        rows = [None if bones == large else row for bones, row in zip(which, rows)]
        records = [NOT_MEASURED if bones == large else record for bones, record in zip(which, records)]
        for short in ("raw_row_bones", "lossy_row_bones", "base_row_bones", "error_row_bones", "num_shells"):
            sizes = dict(raw_row_bones=large, lossy_row_bones=large, base_row_bones=large, error_row_bones=large, num_shells=large)
            sizes[short] = small
            cut = lambda poses, name: [pose[:small] for pose in poses] if short == name else poses      # noqa: E731
            before = ctx.rejected_instance_count()
            check(launch(ctx, cut(raw, "raw_row_bones"), cut(lossy, "lossy_row_bones"), instance_skeletons=ids, additive_format=ADDITIVE0, base=cut(base, "base_row_bones"),
                         shells=shells, **sizes), rows, records)
            assert ctx.rejected_instance_count() - before == 8, short

        # every instance refused: the records say so, and so does the worst record
        before = ctx.rejected_instance_count()
        out = check(launch(ctx, raw, lossy, skeleton=retired), [None] * N, [NOT_MEASURED] * N)
        assert out.worst == (-1.0, NO_BONE, 0xFFFFFFFF, 0)
        assert ctx.rejected_instance_count() - before == N


def test_the_worst_record_of_no_instances_and_of_a_part_of_the_rows():
    rng = np.random.default_rng(6901)
    num_bones = 30
    parents = forest(rng, num_bones)
    raw, lossy = loose_poses(rng, N, num_bones), loose_poses(rng, N, num_bones)
    rows, records, _ = expected_batch(parents, raw, lossy, 3.0)
    with runtime.Context(0) as ctx:
        skeleton = ctx.register_skeleton(parents, identity_pose(num_bones))
        # num_instances == 0: nothing but the worst record is written, and that says "none"
        out = check(launch(ctx, raw, lossy, skeleton=skeleton, n=0), [None] * N, [])
        assert out.worst_written and out.worst == (-1.0, NO_BONE, 0xFFFFFFFF, 0)
        out = check(launch(ctx, raw, lossy, skeleton=skeleton, n=0, with_worst=False), [None] * N, [])
        assert not out.worst_written
        # the first 5 and the first 9 of the rows: the records behind them stay what they were
        for count in (5, 9):
            out = check(launch(ctx, raw, lossy, skeleton=skeleton, n=count), rows[:count] + [None] * (N - count), records[:count])
            assert out.worst[2] == scan_worst(records[:count])[2]
        assert ctx.rejected_instance_count() == 0


def test_a_captured_launch_replays_with_the_bits_of_the_direct_one():
    import torch
    rng = np.random.default_rng(7001)
    num_bones = 100
    parents = forest(rng, num_bones)
    raw, lossy, base = loose_poses(rng, N, num_bones), loose_poses(rng, N, num_bones), loose_poses(rng, N, num_bones)
    rows, records, _ = expected_batch(parents, raw, lossy, 3.0, True, RELATIVE, base)
    with runtime.Context(0) as ctx:
        skeleton = ctx.register_skeleton(parents, identity_pose(num_bones))
        direct = check(launch(ctx, raw, lossy, skeleton=skeleton, additive_format=RELATIVE, base=base), rows, records)
        device = direct.buffers.device
        side = torch.cuda.Stream(device=device)
        side.wait_stream(torch.cuda.current_stream(device))
        with torch.cuda.stream(side):
            captured = launch(ctx, raw, lossy, skeleton=skeleton, additive_format=RELATIVE, base=base, stream=side.cuda_stream)      # warm-up
            side.synchronize()
            for tensor in captured.tensors:
                tensor.fill_(float(SENTINEL))
            side.synchronize()
            graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graph, stream=side):
                ctx.measure_pose_error(*captured.arguments, stream=side.cuda_stream)
        graph.replay()
        torch.cuda.synchronize()
        read_back(captured)
        check(captured, rows, records)
        assert np.array_equal(captured.error_bits, direct.error_bits) and captured.worst == direct.worst
        assert np.array_equal(bits(captured.bone_errors), bits(direct.bone_errors))
        del graph
        assert ctx.rejected_instance_count() == 0


def test_two_decodes_of_a_clip_end_to_end_and_clip_error():
    """one synthetic clip decoded twice at off-sample times, rounding none and rounding nearest: the measure over the two device buffers
    is the composition over the oracle's two decodes; clip_error is calculate_compression_error's loop over every sample on the host"""
    import torch
    num_bones = 100
    clip = synth.build_clip(seed=611, num_tracks=num_bones, num_samples=40, has_scale=1)
    other = synth.build_clip(seed=612, num_tracks=num_bones, num_samples=40, has_scale=1)
    parents = np.array(synth.humanoid_hierarchy(num_bones), dtype=np.uint32)
    shells = np.linspace(0.5, 3.0, num_bones).astype(np.float32)
    times = ((np.arange(N, dtype=np.float32) * 2.0 + 0.37) / np.float32(clip.sample_rate)).astype(np.float32)
    assert times.max() < clip.duration
    raw = [ob.oracle_decompress_tracks(clip.blob, float(t), ob.ROUND_NONE) for t in times]
    lossy = [ob.oracle_decompress_tracks(clip.blob, float(t), ob.ROUND_NEAREST) for t in times]
    rows, records, _ = expected_batch(parents, raw, lossy, shells)
    assert scan_worst(records)[0] > 0.0
    with runtime.Context(0) as ctx:
        handle, other_handle = ctx.register_clip(clip.blob), ctx.register_clip(other.blob)
        skeleton = ctx.register_skeleton(parents, identity_pose(num_bones))
        device = torch.device("cuda:0")
        stream = torch.cuda.current_stream(device).cuda_stream
        d_clips = torch.full((N,), handle, dtype=torch.int32, device=device)
        d_times = torch.from_numpy(times).to(device)
        d_poses = [torch.zeros((N, num_bones * 12), dtype=torch.float32, device=device) for _ in range(2)]
        for d_pose, rounding in zip(d_poses, (runtime.ROUND_NONE, runtime.ROUND_NEAREST)):
            ctx.decompress_tracks_batch(d_clips.data_ptr(), d_times.data_ptr(), N, d_pose.data_ptr(), num_bones * 48, params=runtime.default_params(rounding_policy=rounding), stream=stream)
        torch.cuda.synchronize()
        decoded = [d_pose.cpu().numpy().reshape(N, num_bones, 12) for d_pose in d_poses]
        out = check(launch(ctx, decoded[0], decoded[1], skeleton=skeleton, shells=shells), rows, records)
        assert out.worst[0] > 0.0

        # clip_error: every sample of the clip, min(i / rate, duration)
        sample_times = np.minimum(np.arange(clip.num_samples, dtype=np.float32) / np.float32(clip.sample_rate), np.float32(clip.duration)).astype(np.float32)
        host_records = [expected_measure(parents, ob.oracle_decompress_tracks(clip.blob, float(t)), ob.oracle_decompress_tracks(other.blob, float(t)), shells)[1]
                        for t in sample_times]
        error, bone, sample = scan_worst(host_records)
        got = runtime.clip_error(ctx, handle, other_handle, skeleton, shells)
        assert got[0] == bone and bits(np.float32(got[1])) == bits(error) and got[2] == float(sample_times[sample]) and error > 0.0
        # a clip against itself
        assert runtime.clip_error(ctx, handle, handle, skeleton, 3.0) == (0, 0.0, 0.0)
        # the object space flag and the decode parameters of either side reach the launches
        host_records = [expected_measure(parents, ob.oracle_decompress_tracks(clip.blob, float(t)), ob.oracle_decompress_tracks(other.blob, float(t), ob.ROUND_NEAREST), 2.0, False)[1]
                        for t in sample_times]
        error, bone, sample = scan_worst(host_records)
        got = runtime.clip_error(ctx, handle, other_handle, skeleton, 2.0, object_space=False, params_b=runtime.default_params(rounding_policy=runtime.ROUND_NEAREST))
        assert got[0] == bone and bits(np.float32(got[1])) == bits(error) and got[2] == float(sample_times[sample])
        assert ctx.rejected_instance_count() == 0
