"""aclhip_measure_pose_error_metric_batch through the C ABI. ACLHIP_METRIC_QVVF is aclhip_measure_pose_error_batch itself: the two calls
over the same buffers leave identical bytes and move the counters alike. ACLHIP_METRIC_QVVF_MATRIX3X4F is compared on bits with the
restatement of tests/test_pose_matrices_oracle.py -- `errors` whole, `bone_errors` wherever the value is not a NaN, `worst` whole --
through the launch and check helpers of tests/test_gpu_pose_error.py, which keep every output inside sentinel filled guards and assert the
inputs unchanged. The kernel and the restatement run the same operation order, so there is no tolerance anywhere. Every launch has 17
instances: more than one workgroup, an odd count. Needs a GPU."""
import numpy as np
import pytest

from acl_amd import runtime, synth
from oracle import bindings as ob
from test_gpu_pose_buffers import bits, chain, identity_pose
from test_gpu_pose_error import N, NOT_MEASURED, RELATIVE, check, expected_batch, launch, signed_poses
from test_gpu_pose_matrices import batch_poses
from test_pose_error_oracle import NO_BONE, forest, loose_poses, scan_worst
from test_pose_matrices_oracle import expected_matrix_measure

pytestmark = pytest.mark.gpu

QVVF, MATRIX = runtime.ERROR_METRIC_QVVF, runtime.ERROR_METRIC_QVVF_MATRIX3X4F


class WithMetric:
    """a context whose measure_pose_error is the metric form with this metric: what test_gpu_pose_error.launch calls"""

    def __init__(self, ctx, metric):
        self.ctx, self.metric = ctx, metric

    def measure_pose_error(self, raw, raw_stride, lossy, lossy_stride, n, desc, errors, stream=None):
        self.ctx.measure_pose_error_metric(raw, raw_stride, lossy, lossy_stride, n, desc, self.metric, errors, stream=stream)


def expected_matrix_batch(parents, raw, lossy, shells, object_space=True):
    """per instance (bone errors, record); parents: one hierarchy, or one per instance"""
    rows, records = [], []
    for i in range(len(raw)):
        errors, record = expected_matrix_measure(parents[i] if isinstance(parents, list) else parents, raw[i], lossy[i], shells, object_space)
        rows.append(errors)
        records.append(record)
    return rows, records


@pytest.mark.parametrize("options", [dict(), dict(object_space=False), dict(additive_format=RELATIVE), dict(object_space=False, additive_format=RELATIVE)],
                         ids=["object", "local", "object-relative", "local-relative"])
def test_the_qvvf_metric_is_the_plain_call(options):
    rng = np.random.default_rng(9300)
    num_bones = 100
    parents = forest(rng, num_bones)
    raw, lossy, base = signed_poses(rng, N, num_bones), signed_poses(rng, N, num_bones), signed_poses(rng, N, num_bones)
    if "additive_format" in options:
        options = dict(options, base=base)
    rows, records, routed = expected_batch(parents, raw, lossy, 2.0, **options)
    assert (routed > 0) == (options.get("object_space", True) or "additive_format" in options)
    with runtime.Context(0) as ctx:
        skeleton = ctx.register_skeleton(parents, identity_pose(num_bones))
        before = ctx.negative_scale_count()
        plain = check(launch(ctx, raw, lossy, skeleton=skeleton, shells=2.0, **options), rows, records)
        moved = ctx.negative_scale_count() - before
        by_metric = check(launch(WithMetric(ctx, QVVF), raw, lossy, skeleton=skeleton, shells=2.0, **options), rows, records)
        assert ctx.negative_scale_count() - before == 2 * moved == 2 * routed
        assert np.array_equal(by_metric.error_bits, plain.error_bits)
        numbers = ~np.isnan(plain.bone_errors)
        assert np.array_equal(np.isnan(by_metric.bone_errors), ~numbers) and np.array_equal(bits(by_metric.bone_errors)[numbers], bits(plain.bone_errors)[numbers])
        assert by_metric.worst_written and bits(np.float32(by_metric.worst[0])) == bits(np.float32(plain.worst[0])) and by_metric.worst[1:] == plain.worst[1:]
        assert ctx.rejected_instance_count() == 0


SHAPES = [("forest", bones) for bones in (1, 63, 64, 65, 100, 300, 1200)] + [("chain", 200)]


@pytest.fixture(scope="module")
def matrix_cases():
    """(kind, B) -> (parents, raw, lossy, {object_space: (rows, records)}), computed once"""
    cases = {}
    for kind, num_bones in SHAPES:
        rng = np.random.default_rng(9400 + num_bones)
        parents = forest(rng, num_bones) if kind == "forest" else chain(num_bones)
        raw, lossy = batch_poses(rng, N, num_bones), batch_poses(rng, N, num_bones)
        # half of the instances: a lossy pose close to the raw one, as a codec leaves it
        lossy[::2] = raw[::2] * (1.0 + rng.uniform(-1.0e-3, 1.0e-3, size=raw[::2].shape)).astype(np.float32)
        # a NaN in one bone of one instance and an infinite scale in another: they never win the scan
        lossy[3, num_bones // 2, 5] = np.nan
        raw[7, num_bones // 3, 8] = np.inf
        cases[(kind, num_bones)] = (parents, raw, lossy, {space: expected_matrix_batch(parents, raw, lossy, 3.0, space) for space in (True, False)})
    return cases


@pytest.mark.parametrize("object_space", [True, False])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda shape: "%s-%d" % shape)
def test_the_matrix_metric_is_the_restatement(matrix_cases, shape, object_space):
    """lane stride edges (63 / 64 / 65: the second wave's first bone), 4, 2 and 1 image pairs per workgroup, a batch that ends inside a
    workgroup, the deepest schedule (a chain of 200); scales of both signs, and no counter moves: there is no qvv_mul"""
    parents, raw, lossy, expected = matrix_cases[shape]
    rows, records = expected[object_space]
    num_bones = shape[1]
    assert np.isnan(rows[3]).any() and np.isfinite(rows[0]).all()
    with runtime.Context(0) as ctx:
        skeleton = ctx.register_skeleton(parents, identity_pose(num_bones))
        before = ctx.negative_scale_count()
        out = check(launch(WithMetric(ctx, MATRIX), raw, lossy, skeleton=skeleton, object_space=object_space), rows, records)
        assert out.worst_written and out.worst[0] > 0.0
        assert ctx.negative_scale_count() == before
        # without the optional outputs: the same records, and neither of the two buffers is touched
        bare = launch(WithMetric(ctx, MATRIX), raw, lossy, skeleton=skeleton, object_space=object_space, with_bone_errors=False, with_worst=False)
        check(bare, [None] * N, records)
        assert not bare.worst_written
        assert ctx.rejected_instance_count() == 0


@pytest.mark.parametrize("object_space", [True, False])
def test_the_same_buffer_twice_gives_zero_and_bone_zero(object_space):
    rng = np.random.default_rng(9501)
    num_bones = 100
    parents = forest(rng, num_bones)
    raw = signed_poses(rng, N, num_bones)
    with runtime.Context(0) as ctx:
        skeleton = ctx.register_skeleton(parents, identity_pose(num_bones))
        out = launch(WithMetric(ctx, MATRIX), raw, raw, skeleton=skeleton, object_space=object_space, same_buffer=True)
        check(out, [np.zeros(num_bones, dtype=np.float32)] * N, [(np.float32(0.0), 0)] * N)
        assert out.worst == (0.0, 0, 0, 0)


def test_under_shear_the_two_metrics_leave_different_records():
    """every instance: a chain whose bones are rotated under parents scaled by up to 4 along one axis only -- the matrix product shears
    what the QVV product keeps orthogonal"""
    rng = np.random.default_rng(9601)
    num_bones = 20
    parents = chain(num_bones)
    raw = loose_poses(rng, N, num_bones)
    raw[..., 0:4] /= np.linalg.norm(raw[..., 0:4], axis=2, keepdims=True)
    raw[..., 8:11] = 1.0
    raw[..., 8] = rng.uniform(2.0, 4.0, size=(N, num_bones)).astype(np.float32)
    lossy = raw.copy()
    lossy[..., 0:4] += rng.uniform(-0.02, 0.02, size=(N, num_bones, 4)).astype(np.float32)
    lossy[..., 0:4] /= np.linalg.norm(lossy[..., 0:4], axis=2, keepdims=True)
    qvv_rows, qvv_records, _ = expected_batch(parents, raw, lossy, 1.0)
    matrix_rows, matrix_records = expected_matrix_batch(parents, raw, lossy, 1.0)
    relative = np.abs(np.stack(matrix_rows)[:, 1:] - np.stack(qvv_rows)[:, 1:]) / np.stack(qvv_rows)[:, 1:]
    assert np.median(relative) > 0.05                                      # not rounding: another pose
    assert np.allclose(np.stack(matrix_rows)[:, 0], np.stack(qvv_rows)[:, 0], rtol=1.0e-4)       # the root has no parent to shear it
    assert all(by_qvv[0] != by_matrix[0] for by_qvv, by_matrix in zip(qvv_records, matrix_records))
    with runtime.Context(0) as ctx:
        skeleton = ctx.register_skeleton(parents, identity_pose(num_bones))
        by_qvv = check(launch(WithMetric(ctx, QVVF), raw, lossy, skeleton=skeleton, shells=1.0), qvv_rows, qvv_records)
        by_matrix = check(launch(WithMetric(ctx, MATRIX), raw, lossy, skeleton=skeleton, shells=1.0), matrix_rows, matrix_records)
        assert not np.any(by_qvv.error_bits[:, 0] == by_matrix.error_bits[:, 0])          # (what check has just held to the two expectations)
        assert ctx.rejected_instance_count() == 0


def test_skeletons_per_instance_and_refusals():
    import torch
    rng = np.random.default_rng(9701)
    small, large = 40, 100
    parents = {small: forest(rng, small, root_chance=0.2), large: forest(rng, large)}
    with runtime.Context(0) as ctx:
        metric_ctx = WithMetric(ctx, MATRIX)
        handles = {bones: ctx.register_skeleton(parents[bones], identity_pose(bones)) for bones in (small, large)}
        flat = ctx.register_skeleton(None, identity_pose(small))                        # no hierarchy
        retired = ctx.register_skeleton(parents[small], identity_pose(small))
        ctx.unregister_skeleton(retired)
        torch.cuda.synchronize()

        # different bone counts inside one workgroup
        which = [large, small, small, large, small, large, large, small, large, small, small, large, large, large, small, large, small]
        raw = [signed_poses(rng, 1, bones)[0] for bones in which]
        lossy = [signed_poses(rng, 1, bones)[0] for bones in which]
        ids = [handles[bones] for bones in which]
        check(launch(metric_ctx, raw, lossy, instance_skeletons=ids), *expected_matrix_batch([parents[bones] for bones in which], raw, lossy, 3.0))
        assert ctx.rejected_instance_count() == 0

        # handle 0, an unknown handle, a retired one, object space without a hierarchy: refused and counted, the record "not measured"
        raw = [signed_poses(rng, 1, small)[0] for _ in range(N)]
        lossy = [signed_poses(rng, 1, small)[0] for _ in range(N)]
        ids = [handles[small]] * N
        ids[1], ids[2], ids[4], ids[5], ids[16] = 0, 0x00ABCDEF, retired, flat, 0xFFFFFFFF
        refused = [handle != handles[small] for handle in ids]
        rows, records = expected_matrix_batch(parents[small], raw, lossy, 3.0)
        before = ctx.rejected_instance_count()
        check(launch(metric_ctx, raw, lossy, instance_skeletons=ids), [None if no else row for no, row in zip(refused, rows)],
              [NOT_MEASURED if no else record for no, record in zip(refused, records)])
        assert ctx.rejected_instance_count() - before == sum(refused) == 5
        # in local space the skeleton without a hierarchy is served
        rows, records = expected_matrix_batch(parents[small], raw, lossy, 3.0, False)
        before = ctx.rejected_instance_count()
        check(launch(metric_ctx, raw, lossy, instance_skeletons=ids, object_space=False), [None if no and handle != flat else row for no, handle, row in zip(refused, ids, rows)],
              [NOT_MEASURED if no and handle != flat else record for no, handle, record in zip(refused, ids, records)])
        assert ctx.rejected_instance_count() - before == 4

        # B * 48 above either stride, 4 * B above the error stride, B above the shell table
        which = [small, large] * 8 + [small]
        raw = [signed_poses(rng, 1, bones)[0] for bones in which]
        lossy = [signed_poses(rng, 1, bones)[0] for bones in which]
        ids = [handles[bones] for bones in which]
        shells = rng.uniform(0.5, 2.0, size=large).astype(np.float32)
        rows, records = expected_matrix_batch([parents[bones] for bones in which], raw, lossy, shells)
        rows = [None if bones == large else row for bones, row in zip(which, rows)]
        records = [NOT_MEASURED if bones == large else record for bones, record in zip(which, records)]
        for short in ("raw_row_bones", "lossy_row_bones", "error_row_bones", "num_shells"):
            sizes = dict(raw_row_bones=large, lossy_row_bones=large, error_row_bones=large, num_shells=large)
            sizes[short] = small
            cut = lambda poses, name: [pose[:small] for pose in poses] if short == name else poses      # noqa: E731
            before = ctx.rejected_instance_count()
            check(launch(metric_ctx, cut(raw, "raw_row_bones"), cut(lossy, "lossy_row_bones"), instance_skeletons=ids, shells=shells, **sizes), rows, records)
            assert ctx.rejected_instance_count() - before == 8, short

        # every instance refused: the records say so, and so does the worst record
        before = ctx.rejected_instance_count()
        out = check(launch(metric_ctx, raw, lossy, skeleton=retired), [None] * N, [NOT_MEASURED] * N)
        assert out.worst == (-1.0, NO_BONE, 0xFFFFFFFF, 0)
        assert ctx.rejected_instance_count() - before == N


def test_clip_error_with_the_matrix_metric_is_the_host_loop_of_the_restatement():
    """two synthetic clips with scale, 40 samples x 20 bones: clip_error(..., metric=1) is calculate_compression_error's loop over every
    sample with the restatement in the place of the launch, over the oracle's decodes (which the device decode equals on bits); the
    default metric is untouched by the new argument"""
    num_bones = 20
    clip = synth.build_clip(seed=621, num_tracks=num_bones, num_samples=40, has_scale=1)
    other = synth.build_clip(seed=622, num_tracks=num_bones, num_samples=40, has_scale=1)
    parents = np.array(synth.humanoid_hierarchy(num_bones), dtype=np.uint32)
    shells = np.linspace(0.5, 3.0, num_bones).astype(np.float32)
    sample_times = np.minimum(np.arange(clip.num_samples, dtype=np.float32) / np.float32(clip.sample_rate), np.float32(clip.duration)).astype(np.float32)
    decoded = [(ob.oracle_decompress_tracks(clip.blob, float(t)), ob.oracle_decompress_tracks(other.blob, float(t))) for t in sample_times]
    with runtime.Context(0) as ctx:
        handle, other_handle = ctx.register_clip(clip.blob), ctx.register_clip(other.blob)
        skeleton = ctx.register_skeleton(parents, identity_pose(num_bones))
        for object_space in (True, False):
            error, bone, sample = scan_worst([expected_matrix_measure(parents, a, b, shells, object_space)[1] for a, b in decoded])
            got = runtime.clip_error(ctx, handle, other_handle, skeleton, shells, object_space=object_space, metric=MATRIX)
            assert got[0] == bone and bits(np.float32(got[1])) == bits(error) and got[2] == float(sample_times[sample]) and error > 0.0
        assert runtime.clip_error(ctx, handle, handle, skeleton, 3.0, metric=MATRIX) == (0, 0.0, 0.0)
        # metric 0 through the new argument is the call without it
        assert runtime.clip_error(ctx, handle, other_handle, skeleton, shells, metric=QVVF) == runtime.clip_error(ctx, handle, other_handle, skeleton, shells)
        assert ctx.rejected_instance_count() == 0
