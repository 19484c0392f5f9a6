"""What aclhip_compress_tracks_metric_batch, aclhip_compress_tracks_variable_metric_batch and aclhip_find_bit_rates_metric_batch compute:
the three existing restatements -- tests/lossy_rotation_compress_restatement.py, tests/variable_compress_restatement.py and
tests/bit_rate_search_restatement.py -- with the error metric as an argument. Nothing of them is copied: for the duration of a call
with ACLHIP_METRIC_QVVF_MATRIX3X4F their error functions are replaced, and put back behind it,

  shell_error   the looping vote and the compaction of constant and default sub-tracks: E_m(d, M(raw), M(lossy)), always
  error_of      S2 with has_scale: the same over QVV transforms (the local error) or over object matrices; without has_scale the
                qvvf restatement's own calculate_error_no_scale (the matrix metric inherits it)
  to_object     S2 with has_scale: O_0 = M(L_0), O_k = matrix_mul(M(L_k), O_k-1), lhs first, nothing normalized; without has_scale
                the qvvf restatement's own

with M = rtm::matrix_from_qvv and matrix_mul as tests/test_pose_matrices_oracle.py restates them (numpy float32 element operations,
one correctly rounded IEEE operation at a time, never fused) and E_m the metric's calculate_error (transform_error_metrics.h:438-461):
the three shell points through rtm::matrix_mul_point3 -- all three products of a point made, the zero ones too --, the largest of three
distances. With ACLHIP_METRIC_QVVF nothing is replaced: the functions below return what the existing restatements return.

A transform is the restatements' (rotation [..., 4], translation [..., 3], scale [..., 3]); an object transform under the matrix
metric is a float32 array [..., 4, 4] (lane 3 takes no part). A helper, not a test file: tests/test_matrix_metric_compress_oracle.py
holds it to the reference's compressor under its matrix metric, tests/test_gpu_matrix_metric_compress.py holds the kernels to it on
every byte."""
import contextlib

import numpy as np

import bit_rate_search_restatement as search
import lossy_rotation_compress_restatement as lossy
import variable_compress_restatement as variable
from lossy_rotation_compress_restatement import F32, OPTIMIZE_LOOPS, f32
from test_pose_matrices_oracle import matrices_of, matrix_mul

METRIC_QVVF, METRIC_MATRIX = 0, 1


def matrix_of(transform):
    """M(t) of a (rotation, translation, scale) whose leading shapes broadcast: float32 [..., 4, 4]; a matrix comes back as it is"""
    if isinstance(transform, np.ndarray):
        return transform
    rotation, translation, scale = (f32(part) for part in transform)
    rows = np.zeros(np.broadcast_shapes(rotation.shape[:-1], translation.shape[:-1], scale.shape[:-1]) + (12,), dtype=np.float32)
    rows[..., 0:4], rows[..., 4:7], rows[..., 8:11] = rotation, translation, scale
    return matrices_of(rows)


def matrix_shell_error(distance, raw, lossy_transform):
    """E_m(distance, M(raw), M(lossy)): both sides QVV transforms or matrices already"""
    raw, lossy_transform = matrix_of(raw), matrix_of(lossy_transform)
    errors = []
    with np.errstate(invalid="ignore", over="ignore"):
        for point in lossy.shell_points(distance):
            def moved(m):
                return (((m[..., 0, 0:3] * point[0]) + (m[..., 1, 0:3] * point[1])) + (m[..., 2, 0:3] * point[2])) + m[..., 3, 0:3]
            d = moved(lossy_transform) - moved(raw)
            errors.append(np.sqrt(((d[..., 0] * d[..., 0]) + (d[..., 1] * d[..., 1])) + (d[..., 2] * d[..., 2])))
        return f32(lossy.greater(lossy.greater(errors[0], errors[1]), errors[2]))


_qvvf_error_of, _qvvf_to_object = search.error_of, search.to_object


def error_of(distance, raw, lossy_transform, has_scale):
    if not has_scale:
        return _qvvf_error_of(distance, raw, lossy_transform, has_scale)
    return matrix_shell_error(distance, raw, lossy_transform)


def to_object(local, parent, has_scale):
    if not has_scale:
        return _qvvf_to_object(local, parent, has_scale)
    return matrix_mul(matrix_of(local), matrix_of(parent))


@contextlib.contextmanager
def arithmetic_of(metric):
    """the three restatements under `metric` while the block runs"""
    if metric not in (METRIC_QVVF, METRIC_MATRIX):
        raise ValueError("unknown error metric %r" % (metric,))
    if metric == METRIC_QVVF:
        yield
        return
    saved = lossy.shell_error, variable.shell_error, search.error_of, search.to_object
    lossy.shell_error = variable.shell_error = matrix_shell_error
    search.error_of, search.to_object = error_of, to_object
    try:
        yield
    finally:
        lossy.shell_error, variable.shell_error, search.error_of, search.to_object = saved


def compress_drop_w(samples, sample_rate, metric=METRIC_QVVF, **settings):
    """lossy_rotation_compress_restatement.compress under `metric`"""
    with arithmetic_of(metric):
        return lossy.compress(samples, sample_rate, **settings)


def compress_variable(samples, sample_rate, bit_rates, metric=METRIC_QVVF, **settings):
    """variable_compress_restatement.compress under `metric`"""
    with arithmetic_of(metric):
        return variable.compress(samples, sample_rate, bit_rates, **settings)


def find_bit_rates(samples, sample_rate, metric=METRIC_QVVF, **settings):
    """bit_rate_search_restatement.find_bit_rates under `metric`: its Search as it is, the record of visits included"""
    with arithmetic_of(metric):
        return search.find_bit_rates(samples, sample_rate, **settings)


def compress_with_search(samples, sample_rate, metric=METRIC_QVVF, **settings):
    """bit_rate_search_restatement.compress_with_search under `metric`: (the Search, the Compressed at its table)"""
    with arithmetic_of(metric):
        return search.compress_with_search(samples, sample_rate, **settings)


# ---- a decision that only the arithmetic decides ------------------------------------------------------------------------------------
# For one transform the two metrics agree up to rounding. A clip of ONE track whose precision is the qvvf error of the deciding sample
# itself makes `error > precision` false under the qvvf metric whatever the data; where the matrix arithmetic rounds that error up,
# it is true under the matrix metric: the two restatements then disagree on the decision, and only a kernel that switched the
# arithmetic of that very decision gives the matrix restatement's bytes.

def _one_track(seed, num_samples, close):
    rng = np.random.default_rng(9000 + seed)
    samples = np.zeros((num_samples, 1, 12), dtype=np.float32)
    axis = rng.normal(size=3)
    axis /= np.linalg.norm(axis)
    base = rng.normal(size=4)
    base /= np.linalg.norm(base)
    for s in range(num_samples):
        angle = 0.002 * s if not close else 0.3 * np.sin(s)
        turn = np.concatenate([axis * np.sin(angle / 2), [np.cos(angle / 2)]])
        samples[s, 0, 0:4] = lossy.quat_mul(f32(turn), f32(base))
    samples[:, 0, 4:7] = rng.uniform(-1.0, 1.0, size=(num_samples, 3)) if close else rng.uniform(-1.0, 1.0, size=3)
    samples[:, 0, 8:11] = rng.uniform(0.9, 1.1, size=(num_samples, 3)) if close else rng.uniform(0.9, 1.1, size=3)
    if close:       # the last sample a hair's breadth from the first: the vote has an error to weigh
        samples[-1] = samples[0]
        samples[-1, 0, 0:4] = lossy.quat_mul(f32(np.concatenate([axis * np.sin(0.0005), [np.cos(0.0005)]])), samples[0, 0, 0:4])
        samples[-1, 0, 4:7] += F32(0.001)
    return samples


def arithmetic_case(what, shell_distance=3.0, budget=400):
    """what: "constant" (the compaction of the rotation) or "vote". Returns (samples [S, 1, 12], precision float32, flags) of the first
    seeded candidate whose deciding error is at most the precision under the qvvf arithmetic and above it under the matrix one, or
    None when the budget ends first. The precision IS the qvvf error of the deciding sample."""
    for seed in range(budget):
        samples = _one_track(seed, 9, close=what == "vote")
        flags = OPTIMIZE_LOOPS if what == "vote" else 0
        probe = lossy.compress(samples, 32.0, flags=flags, precision=1.0e-4, shell_distance=shell_distance)
        errors = [error for kind, _, error, _ in probe.decisions if kind == what]
        if not errors or not errors[0] > 0.0:
            continue
        precision = F32(np.asarray(errors[0]).reshape(-1)[0])
        settings = dict(flags=flags, precision=precision, shell_distance=shell_distance)
        qvvf, matrix = compress_drop_w(samples, 32.0, METRIC_QVVF, **settings), compress_drop_w(samples, 32.0, METRIC_MATRIX, **settings)
        by_qvvf = [error > p for kind, _, error, p in qvvf.decisions if kind == what]
        by_matrix = [error > p for kind, _, error, p in matrix.decisions if kind == what]
        if by_qvvf and by_matrix and not by_qvvf[0] and by_matrix[0]:
            return samples, precision, flags
    return None
