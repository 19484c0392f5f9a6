"""The restatement of tests/additive_compress_restatement.py -- the definition the _additive calls are held to by
tests/test_gpu_additive_compress.py -- against the reference's own compress_track_list WITH THE ADDITIVE BASE, the format and the
matching additive_qvvf_transform_error_metric<format>. oracle/ref_compress_bridge.cpp has no base argument, so this file compiles a
small bridge of its own, tests/c/ref_additive_compress_bridge.cpp, with the flags of oracle/Makefile's REF_FLAGS against
oracle/rtm_shim into a temporary directory; it skips where the reference's sources or the compiler are absent. Nothing compiled is kept.

Inputs: mixed_clip(seed, S, T, offset=9 seed) with tree(seed, T) over (5, 33), (17, 49), (4, 65) and (3, 31), seeds 1 to 3, and the
chain of 9 by 33 (seeds 2, 3); under ADDITIVE1 the scales moved by -1 with a default scale of 0. The base is mixed_clip of another seed
in three forms in turn: S_b = S, S_b = 1, S_b = 2 S - 1 at 19 Hz. Precision 0.01, shell 3.0, 32 Hz. The three formats; the levels medium
and highest. Every input's decisions are clear (decisions_are_clear: checked before the set was fixed, asserted here), so the exact
parts are demanded: sub-track types, segment counts and the header's default-scale bit are the reference's.

The rates are held under caps as in tests/test_bit_rate_search_levels_oracle.py: THE YARDSTICK IS THE REFERENCE AGAINST ITSELF with
every rotation component of clip AND base one ulp away (one_ulp), per format and level; a cap is twice the yardstick as measured,
rounded up (cap_of), and the test prints the yardstick and asserts that the caps still cover it. As measured (the share of the
animated rates that differ overall, in the worst clip; the largest difference of a clip's stream bits):

  14 clips, 233 rates      the reference against itself      the caps                 the restatement against the reference
    relative, medium       3.9 %, 30 %, bits 0.28 %          7.8 %, 60 %, 0.56 %      1 rate (0.43 %), 3.3 %, bits 0.56 %
    relative, highest      0, 0, 0                           0, 0, 0                  0 rates: equal tables
    additive0, medium      4.7 %, 37 %, bits 2.5 %           9.5 %, 74 %, 5.1 %       0 rates
    additive0, highest     2.6 %, 20 %, bits 1.1 %           5.2 %, 40 %, 2.2 %       0 rates
    additive1, medium      6.9 %, 53 %, bits 4.7 %           14 %, 110 %, 9.4 %       2 rates (0.86 %), 6.7 %, bits 0.77 %
    additive1, highest     1.7 %, 13 %, bits 0.79 %          3.5 %, 27 %, 1.6 %       1 rate (0.43 %), 3.3 %, bits 0.26 %

(a yardstick is the largest of three draws, as in that file; the test runs draw 0. The worst clip is the chain of 9, seed 2, in every
row: 30 animated rates, one flipped comparison near its root moves the bones below it. Where the reference is not sensitive at all --
relative at highest -- the cap is 0 and the restatement's table IS the reference's.)

THE ANCHOR: under ADDITIVE0 with an identity base the restatement's table and blob are the restatement's without a base, byte for byte
(the product with the identity is exact; no sign of a zero broke a byte). THE BASE MATTERS: under RELATIVE with base translations of
magnitude 50 the table is not the table without a base and spends more stream bits; and each format's restatement held to the
reference of ANOTHER format misses the overall cap wherever the two references are more than twice the cap apart (the other pairs
are printed).

No symbol of the new calls is needed: the file passes on a library without them. No GPU."""
import ctypes
import os
import shutil
import subprocess

import numpy as np
import pytest

import additive_compress_restatement as additive
import bit_rate_search_levels_restatement as levels
import bit_rate_search_restatement as search
import variable_compress_restatement as restatement
from additive_compress_restatement import ADDITIVE0, ADDITIVE1, NONE, RELATIVE
from test_bit_rate_search_levels_oracle import cap_of
from test_bit_rate_search_oracle import PRECISION, RATE, SHELL, compare, one_ulp, report
from variable_compress_restatement import DEFAULT, IDENTITY, OPTIMIZE_LOOPS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REFERENCE = os.environ.get("ACL_REFERENCE", "/root/reference")
SHAPES = ((5, 33), (17, 49), (4, 65), (3, 31))
SEEDS = (1, 2, 3)
CHAINS = ((9, 33, 2), (9, 33, 3))
BASE_RATE = 19.0
FORMATS = (RELATIVE, ADDITIVE0, ADDITIVE1)
LEVELS = ("medium", "highest")
ADDITIVE1_POSE = np.array([0, 0, 0, 1, 0, 0, 0, 0, 0, 0, 0, 0], dtype=np.float32)
# the reference against itself, clip and base one ulp apart, as measured: (format, level) -> (overall, worst clip, stream bits)
YARDSTICKS = {(RELATIVE, "medium"): (0.03863, 0.30000, 0.00279), (RELATIVE, "highest"): (0.00000, 0.00000, 0.00000),
              (ADDITIVE0, "medium"): (0.04721, 0.36667, 0.02530), (ADDITIVE0, "highest"): (0.02575, 0.20000, 0.01074),
              (ADDITIVE1, "medium"): (0.06867, 0.53333, 0.04669), (ADDITIVE1, "highest"): (0.01717, 0.13333, 0.00790)}
_blobs, _restated = {}, {}


@pytest.fixture(scope="session")
def bridge(tmp_path_factory):
    """tests/c/ref_additive_compress_bridge.cpp against the reference's headers, with oracle/Makefile's REF_FLAGS"""
    compiler = shutil.which("g++")
    if compiler is None or not os.path.isdir(os.path.join(REFERENCE, "includes", "acl")):
        pytest.skip("the reference's sources or g++ are absent")
    target = tmp_path_factory.mktemp("ref_additive") / "libaclref_additive.so"
    subprocess.run([compiler, "-std=c++17", "-O2", "-mavx2", "-mbmi", "-mlzcnt", "-mpopcnt", "-DACL_USE_POPCOUNT", "-ffp-contract=off", "-fPIC", "-shared", "-pthread",
                    "-I" + os.path.join(REFERENCE, "includes"), "-I" + os.path.join(ROOT, "oracle", "rtm_shim"), os.path.join(ROOT, "tests", "c", "ref_additive_compress_bridge.cpp"),
                    "-o", str(target)], check=True)
    lib = ctypes.CDLL(str(target))
    vp, u32, f32 = ctypes.c_void_p, ctypes.c_uint32, ctypes.c_float
    lib.aclref_compress_additive.argtypes = [vp, u32, u32, f32, vp, u32, u32, f32, u32, vp, vp, u32, u32, f32, f32, vp, u32, ctypes.c_char_p, u32]
    lib.aclref_compress_additive.restype = u32
    return lib


def reference_blob(lib, samples, base_samples, base_rate, additive_format, level, parents, default_pose=None, flags=0):
    raw, base = np.ascontiguousarray(samples, dtype=np.float32), np.ascontiguousarray(base_samples, dtype=np.float32)
    table = np.ascontiguousarray(np.asarray(parents, dtype=np.uint32).view(np.int32))
    pose = np.ascontiguousarray(np.tile(IDENTITY, (raw.shape[1], 1)) if default_pose is None else default_pose[:raw.shape[1]], dtype=np.float32)
    error = ctypes.create_string_buffer(256)
    arguments = [raw.ctypes.data, raw.shape[1], raw.shape[0], RATE, base.ctypes.data, base.shape[1], base.shape[0], base_rate, additive_format, table.ctypes.data, pose.ctypes.data,
                 levels.LEVELS.get(level, level), flags, PRECISION, SHELL]
    size = lib.aclref_compress_additive(*arguments, None, 0, error, 256)
    assert size != 0, error.value.decode()
    blob = np.zeros(size, dtype=np.uint8)
    assert lib.aclref_compress_additive(*arguments, blob.ctypes.data, size, error, 256) == size
    return blob


def clip_of(seed, num_samples, num_tracks, additive_format):
    samples = restatement.mixed_clip(seed, num_samples, num_tracks, offset=9 * seed)
    if additive_format == ADDITIVE1:
        samples[:, :, 8:11] = samples[:, :, 8:11] - np.float32(1.0)
    return samples


def base_of(seed, num_samples, num_tracks, form):
    count, rate = ((num_samples, RATE), (1, RATE), (2 * num_samples - 1, BASE_RATE))[form]
    return restatement.mixed_clip(50 + seed, count, num_tracks, offset=4 * seed + 2), rate


def inputs(additive_format):
    """(key, clip, parents, base samples, base rate, default pose): the base's three forms in turn"""
    shapes = [(t, s, seed, restatement.tree(seed, t)) for t, s in SHAPES for seed in SEEDS] + [(t, s, seed, restatement.tree(seed, t, "chain")) for t, s, seed in CHAINS]
    for index, (num_tracks, num_samples, seed, parents) in enumerate(shapes):
        base_samples, base_rate = base_of(seed, num_samples, num_tracks, index % 3)
        pose = np.tile(ADDITIVE1_POSE, (num_tracks, 1)) if additive_format == ADDITIVE1 else None
        yield (index, num_tracks, num_samples, seed), clip_of(seed, num_samples, num_tracks, additive_format), parents, base_samples, base_rate, pose


def reference_rates(lib, key, additive_format, level, samples, parents, base_samples, base_rate, pose, draw=None):
    if (key, additive_format, level, draw) not in _blobs:
        if draw is not None:
            samples, base_samples = one_ulp(samples, key[-1] + 1000 * draw), one_ulp(base_samples, key[-1] + 1000 * draw + 500)
        blob = reference_blob(lib, samples, base_samples, base_rate, additive_format, level, parents, pose)
        _blobs[key, additive_format, level, draw] = restatement.rates_of(blob), restatement.parse(blob), int(blob[28])
    return _blobs[key, additive_format, level, draw]


def restated(key, additive_format, level, samples, parents, base_samples, base_rate, pose):
    if (key, additive_format, level) not in _restated:
        settings = dict(parents=parents, precision=PRECISION, shell_distance=SHELL)
        if pose is not None:
            settings["default_pose"] = pose
        base = additive.Base(base_samples, base_rate, additive_format) if additive_format != NONE else None
        _restated[key, additive_format, level] = additive.find_bit_rates(samples, RATE, base, level=level, **settings)
    return _restated[key, additive_format, level]


def measured(lib, additive_format, level, against=None):
    """per clip the comparison of the restatement under `additive_format` with the reference under `against` (the same format when None)"""
    rows = []
    for key, samples, parents, base_samples, base_rate, pose in inputs(additive_format):
        theirs, parsed, misc = reference_rates(lib, key, additive_format if against is None else against, level, samples, parents, base_samples, base_rate, pose)
        mine = restated(key, additive_format, level, samples, parents, base_samples, base_rate, pose)
        if against is None:
            assert restatement.decisions_are_clear(mine.base), key
            assert parsed["num_segments"] == len(mine.base.segments) == mine.table.shape[0]
            kinds = 3 if parsed["has_scale"] else 2
            assert np.array_equal(parsed["types"][:kinds], mine.base.types[:kinds]), key
            if kinds == 2:
                assert (mine.base.types[2] == DEFAULT).all()
            assert (misc >> 1) & 1 == (0 if additive_format == ADDITIVE1 else 1) == (int(mine.base.blob[28]) >> 1) & 1       # the default-scale bit
        if np.array_equal(parsed["types"][:2], mine.base.types[:2]) and parsed["num_segments"] == mine.table.shape[0]:
            rows.append((key,) + compare(mine.table, theirs, mine.base.types, mine.base.segments))
    return rows


def yardstick(lib, additive_format, level, draw=0):
    rows = []
    for key, samples, parents, base_samples, base_rate, pose in inputs(additive_format):
        theirs, parsed, _ = reference_rates(lib, key, additive_format, level, samples, parents, base_samples, base_rate, pose)
        moved, parsed_moved, _ = reference_rates(lib, key, additive_format, level, samples, parents, base_samples, base_rate, pose, draw)
        assert np.array_equal(parsed["types"], parsed_moved["types"]) and parsed["num_segments"] == parsed_moved["num_segments"]
        segments = list(zip([0] * parsed["num_segments"], restatement.split_samples_per_segment(parsed["num_samples"])))
        rows.append((key,) + compare(moved, theirs, parsed["types"], segments))
    return rows


CASES = [(additive_format, level) for additive_format in FORMATS for level in LEVELS]
IDS = ["%s-%s" % (("relative", "additive0", "additive1")[additive_format - 1], level) for additive_format, level in CASES]


def caps_of(additive_format, level):
    return tuple(cap_of(value) for value in YARDSTICKS[additive_format, level])


@pytest.mark.parametrize("additive_format,level", CASES, ids=IDS)
def test_the_table_is_the_references_within_its_own_sensitivity(bridge, additive_format, level):
    """and the yardstick printed beside it: the caps are twice the reference's own sensitivity as measured, rounded up, and still cover it"""
    rows = measured(bridge, additive_format, level)
    mine = report(rows, "restatement against the reference, format %d at %s" % (additive_format, level))
    own = report(yardstick(bridge, additive_format, level), "the reference against itself, clip and base one ulp apart, format %d at %s" % (additive_format, level))
    print("as stated: %s" % (YARDSTICKS[additive_format, level],))
    caps = caps_of(additive_format, level)
    assert all(value <= cap for value, cap in zip(own, caps)), "the caps no longer cover the reference's own sensitivity"
    assert all(cap >= 2.0 * value for value, cap in zip(YARDSTICKS[additive_format, level], caps))
    assert all(value <= cap for value, cap in zip(mine, caps)), (mine, caps)


def test_the_anchor_an_identity_base_under_additive0():
    """the restatement's table and blob are the restatement's without a base, byte for byte"""
    for num_tracks, num_samples, seed, level in ((17, 49, 0, "medium"), (9, 33, 1, "highest"), (5, 33, 1, "medium")):
        samples, parents = restatement.mixed_clip(seed, num_samples, num_tracks, offset=9 * seed, close_loop=seed == 1), restatement.tree(seed, num_tracks)
        identity = np.tile(IDENTITY, (7, num_tracks + 1, 1))
        settings = dict(parents=parents, precision=PRECISION, shell_distance=SHELL, flags=OPTIMIZE_LOOPS)
        found, compressed = additive.compress_with_search(samples, RATE, additive.Base(identity, BASE_RATE, ADDITIVE0), level=level, **settings)
        plain_found, plain = levels.compress_with_search(samples, RATE, level=level, **settings)
        assert np.array_equal(found.table, plain_found.table) and np.array_equal(found.base.shells.view(np.uint32), plain_found.base.shells.view(np.uint32))
        assert np.array_equal(compressed.blob, plain.blob)
        by_drop_w = additive.compress_drop_w(samples, RATE, additive.Base(identity, BASE_RATE, ADDITIVE0), **settings)
        assert np.array_equal(by_drop_w.blob, additive.compress_drop_w(samples, RATE, None, **settings).blob)


def test_the_base_matters(bridge):
    """RELATIVE with base translations of magnitude 50: another table than without a base, and more stream bits; and a restatement held
    to the reference of another format misses the overall cap wherever the two references are more than twice the cap apart"""
    samples, parents = restatement.mixed_clip(2, 33, 17, offset=18), restatement.tree(2, 17)
    base_samples = restatement.mixed_clip(52, 33, 17, offset=10)
    directions = base_samples[:, :, 4:7].astype(np.float64) + 1.0e-3
    base_samples[:, :, 4:7] = (50.0 * directions / np.linalg.norm(directions, axis=-1, keepdims=True)).astype(np.float32)
    settings = dict(parents=parents, precision=PRECISION, shell_distance=SHELL)
    with_base = additive.find_bit_rates(samples, RATE, additive.Base(base_samples, RATE, RELATIVE), **settings)
    without = additive.find_bit_rates(samples, RATE, None, **settings)
    assert not np.array_equal(with_base.table, without.table)
    bits = [search.stream_bits(found.table, found.base.types, found.base.segments) for found in (with_base, without)]
    print("stream bits with the base %d, without %d" % tuple(bits))
    assert bits[0] > bits[1]

    asserted = 0
    for mine in FORMATS:
        for theirs in FORMATS:
            if mine == theirs or ADDITIVE1 in (mine, theirs):
                continue            # (ADDITIVE1's inputs are its own: their scales lie about 0)
            cap = caps_of(mine, "medium")[0]
            rows = []
            for key, clip, tree, base, base_rate, pose in inputs(mine):
                a, parsed, _ = reference_rates(bridge, key, mine, "medium", clip, tree, base, base_rate, pose)
                b, parsed_b, _ = reference_rates(bridge, key, theirs, "medium", clip, tree, base, base_rate, pose)
                if np.array_equal(parsed["types"], parsed_b["types"]):
                    segments = list(zip([0] * parsed["num_segments"], restatement.split_samples_per_segment(parsed["num_samples"])))
                    rows.append((key,) + compare(a, b, parsed["types"], segments))
            gap = report(rows, "the reference under format %d against the reference under format %d" % (mine, theirs))[0] if rows else 0.0
            crossed = measured(bridge, mine, "medium", against=theirs)
            missed = report(crossed, "restatement under format %d against the reference under format %d" % (mine, theirs))[0] if crossed else 1.0
            if gap > 2.0 * cap:
                asserted += 1
                assert missed > cap, (mine, theirs, missed, cap)
            else:
                print("formats %d and %d: the references are %.4f apart, not twice the cap %.4f: printed only" % (mine, theirs, gap, cap))
    print("%d pairs asserted" % asserted)
