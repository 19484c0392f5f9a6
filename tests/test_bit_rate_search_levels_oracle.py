"""The restatement of tests/bit_rate_search_levels_restatement.py -- the definition aclhip_find_bit_rates_level_batch is held to by
tests/test_gpu_bit_rate_search_levels.py -- against the reference's own compress_track_list (oracle/_ref/libaclref_compress.so) at the
levels high and highest, under the matrix metric at highest, and at automatic.

Inputs: the shapes of tests/test_bit_rate_search_oracle.py plus (17, 33), seeds 0 to 3, mixed_clip(k, S, T, offset=9k) with tree(k, T):
32 TREE clips; and CHAINS of 9 and 17 bones by 33 samples, seeds 0 and 1, where the wider levels have the most arrangements to try.
Precision 0.01, shell 3.0, 32 Hz.

As in that file exact equality cannot be demanded of the search (the reference normalizes rotations from the x86 reciprocal square
root estimate; one last bit can flip a comparison on a threshold, and the search then takes another road), and THE YARDSTICK IS THE
REFERENCE AGAINST ITSELF at the same level with every rotation component one ulp away (test_bit_rate_search_oracle.one_ulp), run by
test_the_yardsticks_next_to_the_restatement, which prints it. A cap is twice the yardstick as measured, rounded up (cap_of); the test
asserts that the caps still cover the yardstick. One draw says little about a clip's stream bits or about four chain clips: at high
the reference puts the scale of one track of (65, 65, seed 1) at rate 20 in six of twelve draws and at rate 7 in the others, 0.56 % of
that clip's stream bits, which draw 0 happens not to show. So a yardstick is THE LARGEST OF THREE DRAWS (draw 0 is the draw of
tests/test_bit_rate_search_oracle.py). As measured (the share of the animated rates that differ overall, in the worst clip; the
largest difference of a clip's stream bits):

  tree clips, 2 076 rates    the reference against itself     the caps                the restatement against the reference
    high                     0.96 %, 3.2 %, bits 0.56 %       3 %, 10 %, 1.2 %        11 rates (0.53 %), 2.5 %, bits 0.56 %
    highest                  0.96 %, 2.9 %, bits 0.26 %       3 %, 10 %, 0.52 %        8 rates (0.39 %), 2.5 %, bits 0.10 %
    highest, matrix metric   0.58 %, 2.8 %, bits 0.26 %       3 %, 10 %, 0.52 %        5 rates (0.24 %), 2.5 %, bits 0.10 %
  chain clips, 80 rates
    high                     20 %, 44 %, bits 1.8 %           40 %, 89 %, 3.6 %        0 rates: equal tables
    highest                  12.5 %, 40 %, bits 1.3 %         25 %, 80 %, 2.6 %        0 rates
    highest, matrix metric   1.25 %, 2.8 %, bits 0.26 %       2.5 %, 5.6 %, 0.53 %     0 rates

(draw 0 alone on the tree clips: 16 rates at high, 13 at highest, 10 under the matrix metric; 3 % and 10 % are the caps of
tests/test_bit_rate_search_oracle.py and are twice the tree clips' yardsticks, rounded up, here too). A chain of 17 is where the
reference is most sensitive -- one flipped comparison near the root moves every bone below it -- and the rule gives caps there that
say little; what the restatement shows on the chains is equality with the reference in all twelve tables, and that is asserted.

What keeps this honest: the reference's high and highest each differ from its medium in more than the overall cap (8 % and 9 % of the
rates of the tree clips), and the restatement's three tables differ pairwise on (17, 33, seed 2), (65, 33, seed 1) and the 17-chains:
a restatement whose levels were one search would not pass.

AUTOMATIC: the reference at level 100 gives, byte for byte, its blob at the level automatic_level names, and not its blob at the
neighbouring level, for chains of 17 (highest), 18 and 24 (high) and 25 (medium) bones and for a clip of 501 samples (medium).

No symbol of the new call is needed: the file passes on a library without it. No GPU."""
import ctypes
import math
import os

import numpy as np
import pytest

from oracle import bindings as ob
import bit_rate_search_levels_restatement as levels
import variable_compress_restatement as restatement
from matrix_metric_compress_restatement import METRIC_MATRIX, METRIC_QVVF
from test_bit_rate_search_oracle import PRECISION, RATE, SEEDS, SHAPES, SHELL, compare, one_ulp, report
from variable_compress_restatement import DEFAULT, IDENTITY

TREE_SHAPES = SHAPES + ((17, 33),)
CHAINS = ((9, 33, 0), (9, 33, 1), (17, 33, 0), (17, 33, 1))
DRAWS = 3
# the reference against itself, one ulp apart, as measured: (input set, level, metric) -> the largest of DRAWS draws of (the share of
# the animated rates that differ overall, in the worst clip, the largest difference of a clip's stream bits)
YARDSTICKS = {("tree", "high", METRIC_QVVF): (0.00963, 0.03226, 0.00563), ("chain", "high", METRIC_QVVF): (0.20000, 0.44444, 0.01794),
              ("tree", "highest", METRIC_QVVF): (0.00963, 0.02917, 0.00257), ("chain", "highest", METRIC_QVVF): (0.12500, 0.40000, 0.01271),
              ("tree", "highest", METRIC_MATRIX): (0.00578, 0.02778, 0.00257), ("chain", "highest", METRIC_MATRIX): (0.01250, 0.02778, 0.00264)}
# the tree clips' caps on rates: those of tests/test_bit_rate_search_oracle.py, which are twice these yardsticks, rounded up, too
OVERALL_CAP, CLIP_CAP = 0.03, 0.10


def cap_of(measured):
    """twice the measured yardstick, rounded up to two significant digits; zero stays zero (tests/test_bit_rate_search_rate_range_oracle.py)"""
    if measured == 0.0:
        return 0.0
    digits = 1 - int(math.floor(math.log10(2.0 * measured)))
    return math.ceil(2.0 * measured * 10 ** digits - 1.0e-9) / 10 ** digits


_blobs, _restated = {}, {}


@pytest.fixture(autouse=True)
def reference_compressor():
    """(asked when a test runs: the session's build makes the library)"""
    if not os.path.exists(ob.REF_COMPRESS_PATH):
        pytest.skip("oracle/_ref/libaclref_compress.so not built (it is made from the reference's sources)")


def reference_blob(samples, level, parents, metric=METRIC_QVVF):
    """aclref_compress_ex with `level` as the number it is (oracle.bindings has no name for 100)"""
    lib = ctypes.CDLL(ob.REF_COMPRESS_PATH)
    call = lib.aclref_compress_ex
    call.argtypes = [ctypes.c_void_p, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_float, ctypes.c_void_p, ctypes.c_void_p, ctypes.POINTER(ob.RefCompressSettings),
                     ctypes.c_void_p, ctypes.c_uint32, ctypes.c_char_p, ctypes.c_uint32]
    call.restype = ctypes.c_uint32
    raw = np.ascontiguousarray(samples, dtype=np.float32)
    num_samples, num_tracks = raw.shape[0], raw.shape[1]
    table = np.ascontiguousarray(np.asarray(parents, dtype=np.uint32).view(np.int32))
    bind_pose = np.ascontiguousarray(np.tile(IDENTITY, (num_tracks, 1)), dtype=np.float32)
    settings = ob.RefCompressSettings(levels.LEVELS.get(level, level), ob.ROTATION_FORMATS["quatf_drop_w_variable"], ob.VECTOR_FORMATS["vector3f_variable"],
                                      ob.VECTOR_FORMATS["vector3f_variable"], ob.COMPRESS_FLAGS["matrix_error_metric"] if metric == METRIC_MATRIX else 0, 0.0, 0.0, PRECISION, SHELL)
    error = ctypes.create_string_buffer(256)
    arguments = [raw.ctypes.data, num_tracks, num_samples, ctypes.c_float(RATE), table.ctypes.data, bind_pose.ctypes.data, ctypes.byref(settings)]
    size = call(*arguments, None, 0, error, 256)
    assert size != 0, error.value.decode()
    blob = np.zeros(size, dtype=np.uint8)
    assert call(*arguments, blob.ctypes.data, size, error, 256) == size
    return blob


def tree_inputs():
    for num_tracks, num_samples in TREE_SHAPES:
        for seed in SEEDS:
            yield (num_tracks, num_samples, seed), restatement.mixed_clip(seed, num_samples, num_tracks, offset=9 * seed), restatement.tree(seed, num_tracks)


def chain_inputs():
    for num_tracks, num_samples, seed in CHAINS:
        yield ("chain", num_tracks, num_samples, seed), restatement.mixed_clip(seed, num_samples, num_tracks, offset=9 * seed), restatement.tree(seed, num_tracks, "chain")


def reference_rates(key, samples, level, parents, metric, draw=None):
    """(the rates of the reference's blob, what its headers say), once per clip, level and metric; with `draw` of the clip with every
    rotation component one ulp away: draw 0 is the draw of tests/test_bit_rate_search_oracle.py, the others are drawn anew"""
    if (key, level, metric, draw) not in _blobs:
        blob = reference_blob(samples if draw is None else one_ulp(samples, key[-1] + 1000 * draw), level, parents, metric)
        _blobs[key, level, metric, draw] = restatement.rates_of(blob), restatement.parse(blob)
    return _blobs[key, level, metric, draw]


def restated(key, samples, level, parents, metric):
    if (key, level, metric) not in _restated:
        _restated[key, level, metric] = levels.find_bit_rates_metric(samples, RATE, metric, level=level, parents=parents, precision=PRECISION, shell_distance=SHELL)
    return _restated[key, level, metric]


def measured(inputs, level, metric):
    """per clip the comparison of the restatement with the reference"""
    rows = []
    for key, samples, parents in inputs():
        theirs, parsed = reference_rates(key, samples, level, parents, metric)
        mine = restated(key, samples, level, parents, metric)
        assert restatement.decisions_are_clear(mine.base)
        assert parsed["num_segments"] == len(mine.base.segments) == mine.table.shape[0]
        kinds = 3 if parsed["has_scale"] else 2
        assert np.array_equal(parsed["types"][:kinds], mine.base.types[:kinds])
        if kinds == 2:
            assert (mine.base.types[2] == DEFAULT).all()
        rows.append((key,) + compare(mine.table, theirs, mine.base.types, mine.base.segments))
    return rows


def yardstick(inputs, level, metric, draw=0):
    """per clip the reference against itself, every rotation component one ulp away"""
    rows = []
    for key, samples, parents in inputs():
        theirs, parsed = reference_rates(key, samples, level, parents, metric)
        moved, parsed_moved = reference_rates(key, samples, level, parents, metric, draw)
        assert np.array_equal(parsed["types"], parsed_moved["types"]) and parsed["num_segments"] == parsed_moved["num_segments"]
        segments = list(zip([0] * parsed["num_segments"], restatement.split_samples_per_segment(parsed["num_samples"])))
        rows.append((key,) + compare(moved, theirs, parsed["types"], segments))
    return rows


CASES = [("high", METRIC_QVVF), ("highest", METRIC_QVVF), ("highest", METRIC_MATRIX)]
IDS = ["high", "highest", "highest-matrix"]
SETS = {"tree": tree_inputs, "chain": chain_inputs}


def caps_of(which, level, metric):
    """twice the yardstick as it was measured, rounded up; the tree clips' first two are the caps of tests/test_bit_rate_search_oracle.py,
    which already are that"""
    caps = tuple(cap_of(value) for value in YARDSTICKS[which, level, metric])
    return (OVERALL_CAP, CLIP_CAP, caps[2]) if which == "tree" else caps


@pytest.mark.parametrize("level,metric", CASES, ids=IDS)
@pytest.mark.parametrize("which", list(SETS))
def test_the_table_is_the_references_within_its_own_sensitivity(which, level, metric):
    rows = measured(SETS[which], level, metric)
    overall, clip, bits = report(rows, "restatement against the reference at %s, metric %d, %s clips" % (level, metric, which))
    caps = caps_of(which, level, metric)
    assert overall <= caps[0]
    assert clip <= caps[1]
    assert bits <= caps[2]
    if which == "chain":
        # the rule's caps say little on four chains; what the restatement shows there is asserted: every animated rate is the reference's
        assert [row[2] for row in rows] == [0] * len(CHAINS), rows


@pytest.mark.parametrize("level,metric", CASES, ids=IDS)
@pytest.mark.parametrize("which", list(SETS))
def test_the_yardsticks_next_to_the_restatement(which, level, metric):
    """the reference against itself, one ulp apart, the largest of DRAWS draws per figure, printed beside the restatement's figures;
    the caps are twice this sensitivity as it was measured, rounded up, and still cover it"""
    draws = [report(yardstick(SETS[which], level, metric, draw), "the reference against itself at %s, metric %d, %s clips, draw %d" % (level, metric, which, draw))
             for draw in range(DRAWS)]
    largest = tuple(max(draw[k] for draw in draws) for k in range(3))
    print("the largest of the draws: %.5f overall, %.5f in a clip, %.5f of a clip's stream bits; as stated: %s" % (largest + (YARDSTICKS[which, level, metric],)))
    mine = report(measured(SETS[which], level, metric), "restatement against the reference at %s, metric %d, %s clips" % (level, metric, which))
    caps = caps_of(which, level, metric)
    assert all(value <= cap for value, cap in zip(largest, caps)), "the caps no longer cover the reference's own sensitivity"
    assert all(cap >= 2.0 * value for value, cap in zip(YARDSTICKS[which, level, metric], caps))
    assert all(value <= cap for value, cap in zip(mine, caps))


def test_the_levels_are_told_apart():
    """the reference's high and highest each differ from its medium in more than the overall cap, and the restatement's three tables
    differ pairwise where the issue names them"""
    for level in ("high", "highest"):
        rows = []
        for key, samples, parents in tree_inputs():
            wide, parsed = reference_rates(key, samples, level, parents, METRIC_QVVF)
            medium, _ = reference_rates(key, samples, "medium", parents, METRIC_QVVF)
            segments = list(zip([0] * parsed["num_segments"], restatement.split_samples_per_segment(parsed["num_samples"])))
            rows.append((key,) + compare(wide, medium, parsed["types"], segments))
        overall, _, _ = report(rows, "the reference at %s against the reference at medium" % level)
        assert overall > OVERALL_CAP
    apart = [(key, samples, parents) for key, samples, parents in tree_inputs() if key in ((17, 33, 2), (65, 33, 1))]
    apart += [(key, samples, parents) for key, samples, parents in chain_inputs() if key[1] == 17]
    assert len(apart) == 4
    for key, samples, parents in apart:
        tables = [restated(key, samples, level, parents, METRIC_QVVF).table for level in ("medium", "high", "highest")]
        assert not np.array_equal(tables[0], tables[1]) and not np.array_equal(tables[0], tables[2]) and not np.array_equal(tables[1], tables[2]), key


def test_the_levels_below_high_are_the_existing_restatements():
    import bit_rate_search_restatement as search
    samples, parents = restatement.mixed_clip(1, 33, 17, offset=9), restatement.tree(1, 17)
    settings = dict(parents=parents, precision=PRECISION, shell_distance=SHELL)
    theirs = search.find_bit_rates(samples, RATE, **settings)
    for level in ("lowest", "low", "medium", 0, 1, 2):
        mine = levels.find_bit_rates(samples, RATE, level=level, **settings)
        assert np.array_equal(mine.table, theirs.table) and mine.level == levels.LEVELS.get(level, level)
    with pytest.raises(ValueError):
        levels.find_bit_rates(samples, RATE, level=5, **settings)


# (what the clip is, the level automatic_level must name, the neighbouring level whose blob must differ): the seeds are the first at
# which the reference's blob at the neighbouring level differs (most clips of 3 tracks give one blob at every level)
AUTOMATIC = [(("chain", 17, 17, 1), 4, 3), (("chain", 18, 17, 1), 3, 4), (("chain", 24, 17, 0), 3, 2), (("chain", 25, 17, 0), 2, 3), (("clip", 3, 501, 5), 2, 3)]


def automatic_input(key):
    what, num_tracks, num_samples, seed = key
    samples = restatement.mixed_clip(seed, num_samples, num_tracks, offset=9 * seed)
    return samples, restatement.tree(seed, num_tracks, "chain") if what == "chain" else restatement.tree(seed, num_tracks)


@pytest.mark.parametrize("key,level,neighbour", AUTOMATIC, ids=["%s-%dx%d" % key[0:3] for key, _, _ in AUTOMATIC])
def test_automatic_is_the_level_the_rule_names(key, level, neighbour):
    samples, parents = automatic_input(key)
    assert levels.automatic_level(samples.shape[0], parents, samples.shape[1]) == level
    automatic = reference_blob(samples, levels.AUTOMATIC, parents)
    assert np.array_equal(automatic, reference_blob(samples, level, parents))
    assert not np.array_equal(automatic, reference_blob(samples, neighbour, parents))
    # and the restatement at automatic is the restatement at that level
    mine = levels.find_bit_rates(samples, RATE, level="automatic", parents=parents, precision=PRECISION, shell_distance=SHELL)
    assert mine.level == level and np.array_equal(mine.table, levels.find_bit_rates(samples, RATE, level=level, parents=parents, precision=PRECISION, shell_distance=SHELL).table)


def test_automatic_counts_the_samples_as_registered_and_the_longest_chain():
    chain = restatement.tree(0, 30, "chain")
    assert [levels.automatic_level(17, chain, t) for t in (1, 17, 18, 24, 25, 30)] == [4, 4, 3, 3, 2, 2]
    assert levels.automatic_level(500, chain, 3) == 4 and levels.automatic_level(501, chain, 3) == 2
    assert levels.automatic_level(17, None, 65) == 4                                          # every track a root
    forked = np.array([0xFFFFFFFF] + list(range(0, 17)) + [3, 18, 19], dtype=np.uint32)        # a chain of 18 and a branch of 7 off bone 3
    assert levels.automatic_level(17, forked, 21) == 3 and levels.automatic_level(17, forked[:17], 17) == 4
