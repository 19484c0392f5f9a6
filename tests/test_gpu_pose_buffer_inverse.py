"""aclhip_inverse_transform_poses_batch through the C ABI: object -> local space and make-additive over pose buffers the caller filled.
The expected rows are the composition of tests/test_pose_buffer_inverse_oracle.py (the oracle's functions plus numpy float32 element
operations), compared on bits (np.array_equal over uint32 views) over the whole sentinel filled buffers: a guard row before and behind
every buffer, pad floats behind every row; the kernel and the composition run the same operation order, so there is no tolerance. The
source and base buffers are asserted unchanged when the launch is out of place. Inputs are finite: rotations are unit quaternions times a
factor in [0.5, 2], translations lie within +-10, scales in [0.5, 2]. Needs a GPU."""
import numpy as np
import pytest

from acl_amd import runtime, synth
from test_gpu_pose_buffers import SENTINEL, Buffers, bits, chain, forest, identity_pose, random_poses
from test_pose_buffer_inverse_oracle import BAR, expected_inverse_row, relative_error, rigid_poses

pytestmark = pytest.mark.gpu

NONE, RELATIVE, ADDITIVE0, ADDITIVE1 = runtime.ADDITIVE_NONE, runtime.ADDITIVE_RELATIVE, runtime.ADDITIVE_ADDITIVE0, runtime.ADDITIVE_ADDITIVE1


def expected_rows(source, parents, local_space=True, additive_format=NONE, base=None):
    """(per instance rows, matrix route products of the whole batch); parents: one hierarchy, or one per instance"""
    rows, routed = [], 0
    for i in range(len(source)):
        row, count = expected_inverse_row(parents[i] if isinstance(parents, list) else parents, source[i], local_space, additive_format,
                                          base[i] if base is not None else None)
        rows.append(row)
        routed += count
    return rows, routed


def run(ctx, source, skeleton=0, instance_skeletons=None, local_space=True, additive_format=NONE, base=None, pad_floats=4, in_place=False,
        source_row_bones=None, out_row_bones=None, base_row_bones=None):
    """One launch over `source` ([n, B, 12], or a list of per instance poses). Every buffer has a stride of its own: *_row_bones * 12 floats
    plus pad floats (the base buffer 8 of them). Returns (output buffer, output buffer as it would be untouched, Buffers), on the host, with
    their guard rows; the source buffer (out of place) and the base buffer are asserted unchanged."""
    n = len(source)
    largest = max(pose.shape[0] for pose in source)
    source_floats = (source_row_bones if source_row_bones is not None else largest) * 12 + pad_floats
    out_floats = source_floats if in_place else (out_row_bones if out_row_bones is not None else largest) * 12 + pad_floats
    buffers = Buffers(n, out_floats)
    h_source = buffers.host(source, source_floats)
    d_source = buffers.up(h_source)
    d_out = d_source if in_place else buffers.up(buffers.host())
    inverse = runtime.PoseBufferInverse()
    inverse.skeleton, inverse.local_space, inverse.additive_format = skeleton, 1 if local_space else 0, additive_format
    if instance_skeletons is not None:
        inverse.instance_skeletons = buffers.up(np.asarray(instance_skeletons, dtype=np.uint32)).data_ptr()
    if additive_format != NONE:
        base_floats = (base_row_bones if base_row_bones is not None else largest) * 12 + 8
        h_base = buffers.host(base, base_floats)
        d_base = buffers.up(h_base)
        inverse.base_poses, inverse.base_pose_stride_bytes = d_base[1].data_ptr(), base_floats * 4
    ctx.inverse_transform_poses_batch(d_source[1].data_ptr(), source_floats * 4, n, inverse, d_out[1].data_ptr(), out_floats * 4, stream=buffers.stream())
    out = buffers.down(d_out)
    if not in_place:
        assert np.array_equal(bits(buffers.down(d_source)), bits(h_source))          # the source buffer is only read
    if additive_format != NONE:
        assert np.array_equal(bits(buffers.down(d_base)), bits(h_base))              # and so is the base buffer
    return out, (h_source if in_place else buffers.host()), buffers


def check(ctx, source, expected, **launch):
    """the output is `expected` over the whole guarded buffer (a row that is None stays what it was). Returns the output buffer."""
    out, untouched, buffers = run(ctx, source, **launch)
    want = untouched.copy()
    for i, row in enumerate(expected):
        if row is not None:
            want[1 + i, : row.size] = row.reshape(-1)
    assert np.array_equal(bits(out), bits(want)), np.argwhere(bits(out) != bits(want))[:8]
    return out


LOCAL_BONES = [1, 63, 64, 65, 100, 300, 1200, 1400]


@pytest.fixture(scope="module")
def local_cases():
    """test 1's batches: B -> (parents, [(object poses, composed rows) for n in 1, 3, 5, 9])"""
    cases = {}
    for num_bones in LOCAL_BONES:
        rng = np.random.default_rng(9100 + num_bones)
        parents = forest(rng, num_bones)
        batches = []
        for n in (1, 3, 5, 9):
            source = random_poses(rng, n, num_bones)
            batches.append((source, expected_rows(source, parents)[0]))
        cases[num_bones] = (parents, batches)
    return cases


@pytest.mark.parametrize("num_bones", LOCAL_BONES)
def test_to_local_space_is_the_composition(local_cases, num_bones):
    """lane stride edges (63 / 64 / 65), 4, 2 and 1 instances per workgroup (100 / 300 / 1200 bones), batches that end inside a workgroup;
    1400 bones: an image of 67 216 bytes, more dynamic LDS than a kernel gets without asking (65 408 bytes: the kernel has no walk
    schedule, 1200 bones stay below); out of place and in place"""
    parents, batches = local_cases[num_bones]
    assert num_bones < 20 or int((parents == runtime.NO_PARENT).sum()) > 1        # several roots
    with runtime.Context(0) as ctx:
        skeleton = ctx.register_skeleton(parents, identity_pose(num_bones))
        for index, (source, rows) in enumerate(batches):
            assert np.isfinite(np.stack(rows)).all()
            apart = check(ctx, source, rows, skeleton=skeleton, pad_floats=0 if index % 2 else 4)
            within = check(ctx, source, rows, skeleton=skeleton, pad_floats=0 if index % 2 else 4, in_place=True)
            assert np.array_equal(bits(within), bits(apart))
        assert ctx.rejected_instance_count() == 0
        assert ctx.negative_scale_count() == 0


@pytest.mark.parametrize("shape", ["chain65", "chain200", "star130"])
def test_the_descending_in_place_passes_at_their_deepest(shape):
    """chains: every bone's parent is the bone before it -- in the same pass of 64, or the first bone of a pass reads the last bone of the
    pass after it; a star: every pass reads bone 0, which the last pass holds"""
    num_bones = {"chain65": 65, "chain200": 200, "star130": 130}[shape]
    parents = chain(num_bones)
    if shape == "star130":
        parents[1:] = 0
    rng = np.random.default_rng(9200 + num_bones)
    source = random_poses(rng, 5, num_bones)
    rows, _ = expected_rows(source, parents)
    assert np.isfinite(np.stack(rows)).all()
    with runtime.Context(0) as ctx:
        skeleton = ctx.register_skeleton(parents, identity_pose(num_bones))
        check(ctx, source, rows, skeleton=skeleton)
        check(ctx, source, rows, skeleton=skeleton, in_place=True)
        assert ctx.rejected_instance_count() == 0


def test_mirrored_bones_take_the_matrix_route_and_are_counted():
    rng = np.random.default_rng(9301)
    num_bones, n = 100, 5
    parents = forest(rng, num_bones)
    source, base = random_poses(rng, n, num_bones), random_poses(rng, n, num_bones)
    for poses in (source, base):
        poses[..., 8:11][rng.uniform(size=(n, num_bones, 3)) < 1.0 / 6.0] *= -1.0
    rows, routed = expected_rows(source, parents)
    relative_rows, relative_routed = expected_rows(source, parents, True, RELATIVE, base)
    assert np.isfinite(np.stack(rows)).all() and np.isfinite(np.stack(relative_rows)).all()
    assert routed > 50 and relative_routed > routed + 50
    with runtime.Context(0) as ctx:
        skeleton = ctx.register_skeleton(parents, identity_pose(num_bones))
        before = ctx.negative_scale_count()
        check(ctx, source, rows, skeleton=skeleton)
        assert ctx.negative_scale_count() - before == routed
        before = ctx.negative_scale_count()
        check(ctx, source, relative_rows, skeleton=skeleton, additive_format=RELATIVE, base=base)
        assert ctx.negative_scale_count() - before == relative_routed
        # additive0 divides scale by scale: nothing beyond step 1's products is routed
        before = ctx.negative_scale_count()
        check(ctx, source, expected_rows(source, parents, True, ADDITIVE0, base)[0], skeleton=skeleton, additive_format=ADDITIVE0, base=base)
        assert ctx.negative_scale_count() - before == routed
        assert ctx.rejected_instance_count() == 0


@pytest.mark.parametrize("num_bones", [100, 65])
@pytest.mark.parametrize("local_space", [True, False])
@pytest.mark.parametrize("additive_format", [RELATIVE, ADDITIVE0, ADDITIVE1])
def test_the_three_additive_formats(additive_format, local_space, num_bones):
    """with and without local_space, the base buffer with a stride of its own (run), out of place and in place"""
    rng = np.random.default_rng(9400 + num_bones * 8 + additive_format * 2 + int(local_space))
    parents = forest(rng, num_bones)
    n = 5
    source, base = random_poses(rng, n, num_bones), random_poses(rng, n, num_bones)
    rows, _ = expected_rows(source, parents, local_space, additive_format, base)
    assert np.isfinite(np.stack(rows)).all()
    with runtime.Context(0) as ctx:
        # (without local_space no hierarchy is needed: a skeleton registered without parents serves it)
        skeleton = ctx.register_skeleton(parents if local_space else None, identity_pose(num_bones))
        check(ctx, source, rows, skeleton=skeleton, local_space=local_space, additive_format=additive_format, base=base)
        check(ctx, source, rows, skeleton=skeleton, local_space=local_space, additive_format=additive_format, base=base, in_place=True)
        assert ctx.rejected_instance_count() == 0


def test_a_root_keeps_its_bytes_and_everything_else_gets_zero_pads():
    rng = np.random.default_rng(9501)
    parents = forest(rng, 20, root_chance=0.2)
    roots = parents == runtime.NO_PARENT
    assert 1 < int(roots.sum()) < 20
    source, base = random_poses(rng, 3, 20), random_poses(rng, 3, 20)
    for poses in (source, base):
        poses[..., 7], poses[..., 11] = 5.5, -6.5
    with runtime.Context(0) as ctx:
        skeleton = ctx.register_skeleton(parents, identity_pose(20))
        out = check(ctx, source, expected_rows(source, parents)[0], skeleton=skeleton, pad_floats=0)
        rows = out[1:4].reshape(3, 20, 12)
        assert np.all(rows[:, roots][..., 7] == 5.5) and np.all(rows[:, roots][..., 11] == -6.5) and np.all(rows[:, ~roots][..., [7, 11]] == 0.0)
        assert np.array_equal(bits(rows[:, roots]), bits(source[:, roots]))
        for local_space in (True, False):
            out = check(ctx, source, expected_rows(source, parents, local_space, ADDITIVE1, base)[0], skeleton=skeleton, pad_floats=0, local_space=local_space,
                        additive_format=ADDITIVE1, base=base)
            assert np.all(out[1:4].reshape(3, 20, 12)[..., [7, 11]] == 0.0)


def test_skeletons_per_instance_and_refusals():
    import torch
    rng = np.random.default_rng(9601)
    small, large = 40, 100
    parents = {small: forest(rng, small, root_chance=0.2), large: forest(rng, large)}
    with runtime.Context(0) as ctx:
        handles = {bones: ctx.register_skeleton(parents[bones], identity_pose(bones)) for bones in (small, large)}
        flat = ctx.register_skeleton(None, identity_pose(small))                        # no hierarchy
        retired = ctx.register_skeleton(parents[small], identity_pose(small))
        ctx.unregister_skeleton(retired)
        torch.cuda.synchronize()

        # different bone counts inside one workgroup: a row is written up to its own skeleton's B * 48
        which = [large, small, small, large, small, large, large, small, large]
        source = [random_poses(rng, 1, bones)[0] for bones in which]
        base = [random_poses(rng, 1, bones)[0] for bones in which]
        ids = [handles[bones] for bones in which]
        per_instance = [parents[bones] for bones in which]
        out = check(ctx, source, expected_rows(source, per_instance)[0], instance_skeletons=ids)
        assert np.all(out[2, small * 12:] == SENTINEL)
        rows, _ = expected_rows(source, per_instance, True, RELATIVE, base)
        check(ctx, source, rows, instance_skeletons=ids, additive_format=RELATIVE, base=base)
        check(ctx, source, rows, skeleton=handles[small], instance_skeletons=ids, additive_format=RELATIVE, base=base, in_place=True)   # a launch wide skeleton is ignored next to the list
        assert ctx.rejected_instance_count() == 0

        # handle 0, an unknown handle, a retired one, local_space without a hierarchy: refused and counted, the row what it was
        source = [random_poses(rng, 1, small)[0] for _ in range(7)]
        ids = [handles[small], 0, 0x00ABCDEF, handles[small], retired, flat, handles[small]]
        refused = [False, True, True, False, True, True, False]
        rows = [None if no else row for no, row in zip(refused, expected_rows(source, parents[small])[0])]
        for in_place in (False, True):
            before = ctx.rejected_instance_count()
            check(ctx, source, rows, instance_skeletons=ids, in_place=in_place)
            assert ctx.rejected_instance_count() - before == sum(refused)
        # without local_space the skeleton without a hierarchy is served
        base = [random_poses(rng, 1, small)[0] for _ in range(7)]
        served = expected_rows(source, parents[small], False, ADDITIVE0, base)[0]
        before = ctx.rejected_instance_count()
        check(ctx, source, [None if no and handle != flat else row for no, handle, row in zip(refused, ids, served)], instance_skeletons=ids, local_space=False,
              additive_format=ADDITIVE0, base=base)
        assert ctx.rejected_instance_count() - before == sum(refused) - 1

        # B * 48 above each of the three strides in turn: every buffer but one holds rows of `large` bones, that one rows of `small` bones
        # (an output row too small for B is also an LDS image too small for B: the image has pose_stride_bytes / 48 slots)
        which = [small, large, small]
        source = [random_poses(rng, 1, bones)[0] for bones in which]
        base = [random_poses(rng, 1, bones)[0] for bones in which]
        ids = [handles[bones] for bones in which]
        rows, _ = expected_rows(source, [parents[bones] for bones in which], True, ADDITIVE1, base)
        for short in ("source_row_bones", "out_row_bones", "base_row_bones"):
            strides = dict(source_row_bones=large, out_row_bones=large, base_row_bones=large)
            strides[short] = small
            short_source = [pose[:small] for pose in source] if short == "source_row_bones" else source
            short_base = [pose[:small] for pose in base] if short == "base_row_bones" else base
            before = ctx.rejected_instance_count()
            check(ctx, short_source, [rows[0], None, rows[2]], instance_skeletons=ids, additive_format=ADDITIVE1, base=short_base, **strides)
            assert ctx.rejected_instance_count() - before == 1, short
        # in place: the one stride of source and output
        before = ctx.rejected_instance_count()
        check(ctx, [pose[:small] for pose in source], [rows[0], None, rows[2]], instance_skeletons=ids, additive_format=ADDITIVE1, base=base, in_place=True,
              source_row_bones=small, base_row_bones=large)
        assert ctx.rejected_instance_count() - before == 1


def test_transform_then_inverse_in_place_returns_the_local_pose():
    """decode-free round trip on the device: random local poses (unit rotations, one scale per bone, mirrored bones included) ->
    aclhip_transform_poses_batch(object_space) -> this launch, both in place. Held to the bar of the CPU composition, 2e-5 relative to
    max(1, |value|). The humanoid hierarchy keeps a chain to a dozen bones and the scales stay within [0.8, 1.25], so object space
    translations stay near a hundred units: the inverse's translation is a difference of two of them, and a value of 100 carries
    100 * 2^-24 = 6e-6 of absolute rounding per operation -- inside the bar next to local translations of up to 10; a deep chain with
    scales up to 2 would put object space translations in the thousands and the same rounding outside it."""
    rng = np.random.default_rng(9701)
    num_bones, n = 100, 9
    parents = np.array(synth.humanoid_hierarchy(num_bones), dtype=np.uint32)
    local = rigid_poses(rng, n, num_bones)
    magnitudes = rng.uniform(0.8, 1.25, size=(n, num_bones, 1)).astype(np.float32)
    local[..., 8:11] = np.sign(local[..., 8:11]) * magnitudes
    with runtime.Context(0) as ctx:
        skeleton = ctx.register_skeleton(parents, identity_pose(num_bones))
        buffers = Buffers(n, num_bones * 12 + 4)
        h_local = buffers.host(local)
        d_poses = buffers.up(h_local)
        stride = buffers.row_floats * 4
        forward = runtime.PoseBufferConsumers()
        forward.skeleton, forward.object_space = skeleton, 1
        back = runtime.PoseBufferInverse()
        back.skeleton, back.local_space = skeleton, 1
        ctx.transform_poses_batch(d_poses[1].data_ptr(), stride, n, forward, d_poses[1].data_ptr(), stride, stream=buffers.stream())
        in_object_space = buffers.down(d_poses).copy()
        ctx.inverse_transform_poses_batch(d_poses[1].data_ptr(), stride, n, back, d_poses[1].data_ptr(), stride, stream=buffers.stream())
        returned = buffers.down(d_poses)
        assert ctx.rejected_instance_count() == 0
    assert not np.array_equal(bits(in_object_space), bits(h_local))
    assert np.array_equal(bits(returned[[0, n + 1]]), bits(h_local[[0, n + 1]])) and np.array_equal(bits(returned[:, num_bones * 12:]), bits(h_local[:, num_bones * 12:]))
    worst = relative_error(returned[1:1 + n, : num_bones * 12].reshape(n, num_bones, 12), local)
    print(f"transform -> inverse transform on the device: worst relative error {worst:.3e}")
    assert worst <= BAR


def test_a_captured_launch_replays_with_the_bits_of_the_direct_one():
    import torch
    rng = np.random.default_rng(9801)
    bones, n = 100, 9
    parents = forest(rng, bones)
    source, base = random_poses(rng, n, bones), random_poses(rng, n, bones)
    rows, _ = expected_rows(source, parents, True, RELATIVE, base)
    with runtime.Context(0) as ctx:
        skeleton = ctx.register_skeleton(parents, identity_pose(bones))
        direct = check(ctx, source, rows, skeleton=skeleton, additive_format=RELATIVE, base=base)
        buffers = Buffers(n, bones * 12 + 4)
        d_source, d_base, d_out = buffers.up(buffers.host(source)), buffers.up(buffers.host(base)), buffers.up(buffers.host())
        inverse = runtime.PoseBufferInverse()
        inverse.skeleton, inverse.local_space, inverse.additive_format = skeleton, 1, RELATIVE
        stride = buffers.row_floats * 4
        inverse.base_poses, inverse.base_pose_stride_bytes = d_base[1].data_ptr(), stride
        side = torch.cuda.Stream(device=buffers.device)
        side.wait_stream(torch.cuda.current_stream(buffers.device))
        with torch.cuda.stream(side):
            ctx.inverse_transform_poses_batch(d_source[1].data_ptr(), stride, n, inverse, d_out[1].data_ptr(), stride, stream=side.cuda_stream)      # warm-up
            side.synchronize()
            d_out.fill_(float(SENTINEL))
            side.synchronize()
            graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graph, stream=side):
                ctx.inverse_transform_poses_batch(d_source[1].data_ptr(), stride, n, inverse, d_out[1].data_ptr(), stride, stream=side.cuda_stream)
        graph.replay()
        torch.cuda.synchronize()
        assert np.array_equal(bits(d_out.cpu().numpy()), bits(direct))
        del graph
        assert ctx.rejected_instance_count() == 0
