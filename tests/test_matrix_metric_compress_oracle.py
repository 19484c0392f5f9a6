"""The restatement of tests/matrix_metric_compress_restatement.py -- the definition the three _metric entry points are held to by
tests/test_gpu_matrix_metric_compress.py under ACLHIP_METRIC_QVVF_MATRIX3X4F -- against the reference's own compress_track_list with
its qvvf_matrix3x4f_transform_error_metric (oracle/_ref/libaclref_compress.so, flag matrix_error_metric), on the input set of
tests/test_bit_rate_search_oracle.py: mixed_clip(k, S, T, offset=9k) with tree(k, T), k = 0 .. 3, its seven SHAPES, precision 0.01,
shell 3.0, 32 Hz, the levels lowest and medium (one search: the restatement runs it once per metric).

As there, exact equality cannot be demanded of the search (the reference normalizes rotations from the x86 reciprocal square root
estimate), and THE YARDSTICK IS THE REFERENCE AGAINST ITSELF under the matrix metric with every rotation component one ulp away
(test_bit_rate_search_oracle.one_ulp). Measured by test_the_yardstick_next_to_the_restatement, which prints it:

  the reference against itself    14 of 1 962 animated rates differ (0.71 %), 5 of 138 in the worst clip (3.6 %), at most by 2 rates; the
                                  stream bits of a clip by 0.16 % at most
  the caps, twice that rounded up 1.5 % overall, 8 % in any one clip, 0.4 % of a clip's stream bits; types and segment counts are equal
  the restatement                 5 of 1 962 (0.25 %), 3 of 120 in the worst clip (2.5 %), at most by 1 rate; stream bits within 0.10 %

and the test asserts that the caps still cover the yardstick. THE METRICS ARE TOLD APART: the reference differs from itself across
the two metrics by about 12 % of the rates of this set, and each restatement held to the OTHER metric's reference must miss the
overall cap by more than a factor of two. Without scale the matrix metric inherits the qvvf metric's _no_scale arithmetic: the table
and the blob of a clip whose scales are all default are the qvvf restatement's, byte for byte. The two writers are held to the matrix
reference under the comparison rules of tests/test_variable_compress_oracle.py and tests/test_lossy_rotation_compress_oracle.py, on
clips that close their loop, so that the vote is taken. Last, clips of one track whose precision is the qvvf error of the deciding
sample itself: the two restatements disagree there (no claim against the reference: its normalization differs in the last bit).

Tests 1 to 3 need no symbol of the new calls: they pass on a library without them and fail on a restatement that keeps the qvvf
arithmetic. No GPU."""
import os

import numpy as np
import pytest

from oracle import bindings as ob
import bit_rate_search_restatement as search
import lossy_rotation_compress_restatement as lossy
import matrix_metric_compress_restatement as metric_restatement
import variable_compress_restatement as restatement
import test_lossy_rotation_compress_oracle as drop_w_oracle
import test_variable_compress_oracle as variable_oracle
from matrix_metric_compress_restatement import METRIC_MATRIX, METRIC_QVVF
from test_bit_rate_search_oracle import PRECISION, RATE, SEEDS, SHAPES, SHELL, compare, one_ulp, report
from variable_compress_restatement import ANIMATED, CONSTANT, DEFAULT, IDENTITY, OPTIMIZE_LOOPS

# the reference under the matrix metric against itself, rotations one ulp apart, as measured (the test prints it again)
YARDSTICK_OVERALL, YARDSTICK_CLIP, YARDSTICK_BITS = 0.0071, 0.036, 0.0016
# twice that, rounded up
OVERALL_CAP, CLIP_CAP, BITS_CAP = 0.015, 0.08, 0.004
_reference, _restated = {}, {}


@pytest.fixture(autouse=True)
def reference_compressor():
    """(asked when a test runs: the session's build makes the library)"""
    if not os.path.exists(ob.REF_COMPRESS_PATH):
        pytest.skip("oracle/_ref/libaclref_compress.so not built (it is made from the reference's sources)")


def inputs(scales="mixed"):
    for num_tracks, num_samples in SHAPES:
        for seed in SEEDS:
            yield (num_tracks, num_samples, seed), restatement.mixed_clip(seed, num_samples, num_tracks, offset=9 * seed, scales=scales), restatement.tree(seed, num_tracks)


def reference_blob(samples, level, parents, metric, **switches):
    num_tracks = samples.shape[1]
    return np.asarray(ob.ref_compress_ex(samples, RATE, parents=np.asarray(parents, dtype=np.uint32).view(np.int32), bind_pose=np.tile(IDENTITY, (num_tracks, 1)), level=level,
                                         precision=PRECISION, shell_distance=SHELL, matrix_error_metric=metric == METRIC_MATRIX, **switches)).view(np.uint8)


def reference_rates(key, samples, level, parents, metric):
    """(the rates of the reference's blob, what its headers say), once per clip, level and metric"""
    if (key, level, metric) not in _reference:
        blob = reference_blob(samples, level, parents, metric)
        _reference[key, level, metric] = restatement.rates_of(blob), restatement.parse(blob)
    return _reference[key, level, metric]


def restated(key, samples, parents, metric):
    """the restatement's Search, once per clip and metric (lowest, low and medium run one search: tests/test_bit_rate_search_oracle.py)"""
    if (key, metric) not in _restated:
        _restated[key, metric] = metric_restatement.find_bit_rates(samples, RATE, metric, parents=parents, precision=PRECISION, shell_distance=SHELL, level="medium")
    return _restated[key, metric]


def measured(level, restatement_metric, reference_metric, scales="mixed", same_types=True):
    rows = []
    for key, samples, parents in inputs(scales):
        theirs, parsed = reference_rates((key, scales), samples, level, parents, reference_metric)
        mine = restated((key, scales), samples, parents, restatement_metric)
        kinds = 3 if parsed["has_scale"] else 2
        if same_types:
            assert restatement.decisions_are_clear(mine.base)
            assert parsed["num_segments"] == len(mine.base.segments) == mine.table.shape[0]
            assert np.array_equal(parsed["types"][:kinds], mine.base.types[:kinds])
            if kinds == 2:
                assert (mine.base.types[2] == DEFAULT).all()
        elif parsed["num_segments"] != mine.table.shape[0] or not np.array_equal(parsed["types"][:kinds], mine.base.types[:kinds]):
            continue            # (across metrics: a clip whose types differ has no rates to count)
        rows.append((key,) + compare(mine.table, theirs, mine.base.types, mine.base.segments))
    return rows


@pytest.mark.parametrize("level", ["lowest", "medium"])
def test_the_table_is_the_matrix_references_within_its_own_sensitivity(level):
    overall, clip, bits = report(measured(level, METRIC_MATRIX, METRIC_MATRIX), "matrix restatement against the matrix reference at %s" % level)
    assert overall <= OVERALL_CAP
    assert clip <= CLIP_CAP
    assert bits <= BITS_CAP


def test_the_yardstick_next_to_the_restatement():
    """the reference under the matrix metric against itself with every rotation component one ulp away, printed beside the
    restatement's figures; the caps are twice this sensitivity as it was measured, rounded up"""
    rows = []
    for key, samples, parents in inputs():
        theirs, parsed = reference_rates((key, "mixed"), samples, "medium", parents, METRIC_MATRIX)
        moved_blob = reference_blob(one_ulp(samples, key[2]), "medium", parents, METRIC_MATRIX)
        moved, parsed_moved = restatement.rates_of(moved_blob), restatement.parse(moved_blob)
        assert np.array_equal(parsed["types"], parsed_moved["types"]) and parsed["num_segments"] == parsed_moved["num_segments"]
        segments = list(zip([0] * parsed["num_segments"], restatement.split_samples_per_segment(parsed["num_samples"])))
        rows.append((key,) + compare(moved, theirs, parsed["types"], segments))
    yardstick = report(rows, "the matrix reference against itself, one ulp apart")
    mine = report(measured("medium", METRIC_MATRIX, METRIC_MATRIX), "matrix restatement against the matrix reference at medium")
    assert yardstick[0] <= OVERALL_CAP and yardstick[1] <= CLIP_CAP and yardstick[2] <= BITS_CAP, "the caps no longer cover the reference's own sensitivity"
    assert OVERALL_CAP >= 2.0 * YARDSTICK_OVERALL and CLIP_CAP >= 2.0 * YARDSTICK_CLIP and BITS_CAP >= 2.0 * YARDSTICK_BITS
    assert mine[0] <= OVERALL_CAP and mine[1] <= CLIP_CAP and mine[2] <= BITS_CAP


def test_the_inputs_tell_the_metrics_apart():
    """each restatement held to the OTHER metric's reference differs overall by more than twice the cap: a restatement (or a kernel
    held to it) that kept the qvvf arithmetic would not pass the test above"""
    qvvf_to_matrix = report(measured("medium", METRIC_QVVF, METRIC_MATRIX, same_types=False), "qvvf restatement against the matrix reference")
    matrix_to_qvvf = report(measured("medium", METRIC_MATRIX, METRIC_QVVF, same_types=False), "matrix restatement against the qvvf reference")
    assert qvvf_to_matrix[0] > 2.0 * OVERALL_CAP
    assert matrix_to_qvvf[0] > 2.0 * OVERALL_CAP


def test_metric_0_is_the_existing_restatements():
    samples, parents = restatement.mixed_clip(1, 33, 17, offset=9, close_loop=True), restatement.tree(1, 17)
    settings = dict(parents=parents, precision=PRECISION, shell_distance=SHELL, flags=OPTIMIZE_LOOPS)
    mine, theirs = metric_restatement.find_bit_rates(samples, RATE, METRIC_QVVF, **settings), search.find_bit_rates(samples, RATE, **settings)
    assert np.array_equal(mine.table, theirs.table) and np.array_equal(mine.errors, theirs.errors)
    assert np.array_equal(metric_restatement.compress_variable(samples, RATE, mine.table, METRIC_QVVF, **settings).blob, restatement.compress(samples, RATE, theirs.table, **settings).blob)
    assert np.array_equal(metric_restatement.compress_drop_w(samples, RATE, METRIC_QVVF, **settings).blob, lossy.compress(samples, RATE, **settings).blob)
    # and the functions are back in their places behind a matrix call
    metric_restatement.find_bit_rates(samples[:, :3], RATE, METRIC_MATRIX, precision=PRECISION, shell_distance=SHELL)
    assert np.array_equal(search.find_bit_rates(samples, RATE, **settings).table, theirs.table)
    with pytest.raises(ValueError):
        metric_restatement.find_bit_rates(samples, RATE, 2, **settings)


def test_without_scale_the_matrix_metric_is_the_qvvf_metric():
    """scales="default": has_scale is false, S2 is calculate_error_no_scale under either metric. The vote and the compaction still take
    the matrix route; where every decision is clear they fall as under qvvf, and table and blob are equal byte for byte"""
    compared = 0
    for key, samples, parents in inputs("default"):
        settings = dict(parents=parents, precision=PRECISION, shell_distance=SHELL)
        by_matrix, by_qvvf = restated((key, "default"), samples, parents, METRIC_MATRIX), restated((key, "default"), samples, parents, METRIC_QVVF)
        assert not (by_matrix.base.types[2] != DEFAULT).any()
        if not (restatement.decisions_are_clear(by_matrix.base) and restatement.decisions_are_clear(by_qvvf.base)):
            continue
        compared += 1
        assert np.array_equal(by_matrix.table, by_qvvf.table)
        assert np.array_equal(metric_restatement.compress_variable(samples, RATE, by_matrix.table, METRIC_MATRIX, **settings).blob,
                              metric_restatement.compress_variable(samples, RATE, by_qvvf.table, METRIC_QVVF, **settings).blob)
    assert compared >= len(SHAPES) * len(SEEDS) // 2
    overall, clip, bits = report(measured("medium", METRIC_MATRIX, METRIC_MATRIX, scales="default"), "matrix restatement against the matrix reference, no scale")
    assert overall <= OVERALL_CAP and clip <= CLIP_CAP and bits <= BITS_CAP


WRITER_SHAPES = [(t, s) for t in (3, 17) for s in (2, 33, 65)]


@pytest.mark.parametrize("num_tracks,num_samples", WRITER_SHAPES, ids=["%dx%d" % shape for shape in WRITER_SHAPES])
def test_the_variable_writer_at_the_matrix_references_rates_is_its_blob(num_tracks, num_samples, monkeypatch):
    """the rules of tests/test_variable_compress_oracle.py (its hold): equal on bits wherever no rotation normalization enters, the
    components within 1e-5 plus a quantization step elsewhere; a closing loop, both levels"""
    def matrix_reference(samples, level, default_pose=None, parents=None, flags=0):
        assert default_pose is None
        return reference_blob(samples, level, parents, METRIC_MATRIX, optimize_loops=bool(flags & OPTIMIZE_LOOPS))
    monkeypatch.setattr(variable_oracle, "reference", matrix_reference)
    for k, level in enumerate(("lowest", "medium")):
        samples = restatement.mixed_clip(k, num_samples, num_tracks, offset=9 * k, close_loop=num_samples > 2)
        with metric_restatement.arithmetic_of(METRIC_MATRIX):
            c = variable_oracle.hold(samples, level, parents=restatement.tree(k, num_tracks), flags=OPTIMIZE_LOOPS)
        votes = [d for d in c.decisions if d[0] == "vote"]
        assert len(votes) >= 1 and (num_samples == 2 or (c.wrap and c.num_samples == num_samples - 1))


@pytest.mark.parametrize("num_tracks,num_samples", WRITER_SHAPES, ids=["%dx%d" % shape for shape in WRITER_SHAPES])
def test_the_drop_w_writer_is_the_matrix_references_blob(num_tracks, num_samples):
    """the rules of tests/test_lossy_rotation_compress_oracle.py (its hold): every byte outside the rotation value words equal, those
    within 1e-5; full vectors, a closing loop"""
    for k in range(2):
        samples, parents = lossy.clip(k, num_samples, num_tracks, close_loop=num_samples > 2), lossy.tree(k, num_tracks)
        theirs = drop_w_oracle.reference(samples, parents=parents, flags=OPTIMIZE_LOOPS, matrix_error_metric=True)
        compressed = metric_restatement.compress_drop_w(samples, drop_w_oracle.RATE, METRIC_MATRIX, parents=parents, flags=OPTIMIZE_LOOPS, precision=PRECISION, shell_distance=SHELL)
        assert lossy.decisions_are_clear(compressed)
        drop_w_oracle.hold(compressed, theirs)
        assert any(d[0] == "vote" for d in compressed.decisions) and (num_samples == 2 or compressed.wrap)


@pytest.mark.parametrize("what", ["constant", "vote"])
def test_a_decision_that_only_the_arithmetic_decides(what):
    """one track, the precision the qvvf error of the deciding sample itself: `>` is false under the qvvf arithmetic; the candidate kept
    is one whose matrix arithmetic gives the other answer. The two restatements disagree on it: the rotation is constant or default
    under one metric and animated under the other; the vote removes the last sample under one and keeps it under the other"""
    case = metric_restatement.arithmetic_case(what)
    assert case is not None, "no candidate within the search budget"
    samples, precision, flags = case
    settings = dict(flags=flags, precision=precision, shell_distance=SHELL)
    for compress in (lambda metric: metric_restatement.compress_drop_w(samples, RATE, metric, **settings),
                     lambda metric: metric_restatement.compress_variable(samples, RATE, (12, 12, 12), metric, **settings)):
        by_qvvf, by_matrix = compress(METRIC_QVVF), compress(METRIC_MATRIX)
        if what == "constant":
            assert by_qvvf.types[0, 0] in (CONSTANT, DEFAULT) and by_matrix.types[0, 0] == ANIMATED
        else:
            assert by_qvvf.wrap and by_qvvf.num_samples == samples.shape[0] - 1 and not by_matrix.wrap and by_matrix.num_samples == samples.shape[0]
        assert not np.array_equal(by_qvvf.blob, by_matrix.blob)
