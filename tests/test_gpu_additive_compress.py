"""aclhip_compress_tracks_additive_batch, aclhip_compress_tracks_variable_additive_batch and aclhip_find_bit_rates_additive_batch through
the C ABI: the expected tables, blobs, results and shells are the restatement's (tests/additive_compress_restatement.py, which
tests/test_additive_compress_oracle.py holds to the reference's compressor with the base), and every comparison is on BYTES: both
sides follow one definition, nothing has a tolerance.

The launches and the comparisons are the family's own (tests/compress_launches.py: a flat buffer of a sentinel byte between guards, one
comparison for every byte), at the three entries of the _additive front. The shapes are the smallest at which the kernels can go wrong: T in
1 (a root alone), 4 (one group of four rotations), 9 and 17 (the chains of the level tests; a group and a tail); S in 1 (no vote
possible), 2 (a vote), 17 (one segment), 33 and 48 (two) and 49 (three); bases of 1, 2, 7 and S samples and one of 2 S - 1 samples at another
rate, so that the nearest key lands on both sides of a half; clips with scale and without (the _no_scale route); ADDITIVE1 with a
default scale of 0 in the default pose; a loop that closes only ON the base; the levels medium, highest and automatic on the chain
of 9. Needs a GPU. Fails on a library without the calls."""
import numpy as np
import pytest

from acl_amd import runtime
import additive_compress_restatement as additive
import compress_launches as launches
import variable_compress_restatement as restatement
from additive_compress_restatement import ADDITIVE0, ADDITIVE1, NONE, RELATIVE
from compress_launches import PRECISION, RATE, SHELL, Entry, check_rows, check_table, ctx  # noqa: F401  (ctx: this module's fixture)
from variable_compress_restatement import ANIMATED, DEFAULT, IDENTITY, OPTIMIZE_LOOPS

pytestmark = pytest.mark.gpu

BASE_RATE = 19.0                        # the rate of a base that has another than the clips' (RATE, the launches' own)
# (48 samples are two segments of 24: split_samples_per_segment deals the last 16 out over the other two; 49 are 17 + 16 + 16)
TRACK_COUNTS, SAMPLE_COUNTS = (1, 4, 9, 17), (1, 2, 17, 33, 48, 49)
SHAPES = [(t, s) for t in TRACK_COUNTS for s in SAMPLE_COUNTS]
MAX_TRACKS, MAX_SAMPLES, MAX_SEGMENTS = 17, 49, 3
FORMATS = (RELATIVE, ADDITIVE0, ADDITIVE1)
MEDIUM, HIGHEST, AUTOMATIC = 2, 4, 100
REFUSED, NOT_FINITE = runtime.COMPRESS_REFUSED, runtime.COMPRESS_NOT_FINITE
ADDITIVE1_POSE = np.tile(np.array([0, 0, 0, 1, 0, 0, 0, 0, 0, 0, 0, 0], dtype=np.float32), (MAX_TRACKS, 1))     # a default scale of 0


def through(kind, bases, additive_format):
    """the _additive front of `kind` with `bases` (a handle for every instance, or one per instance; None: no handles at all)"""
    return Entry(kind, "additive", bases=bases, additive_format=additive_format)


def launch(ctx, entry, handles, **settings):
    settings.setdefault("max_tracks", MAX_TRACKS)
    settings.setdefault("max_samples", MAX_SAMPLES)
    return launches.launch(ctx, entry, handles, **settings)


class Case:
    """a clip, its base and what goes with them; the handles once registered"""


def clip_of(k, num_tracks, num_samples, additive_format, **keywords):
    """mixed_clip as an additive clip: under ADDITIVE1 its scales are about 0 where they were about 1 (x - 1 is exact there), default 0"""
    samples = restatement.mixed_clip(k, num_samples, num_tracks, offset=9 * k, **keywords)
    if additive_format == ADDITIVE1:
        samples[:, :, 8:11] = samples[:, :, 8:11] - np.float32(1.0)
    return samples


def base_of(k, num_tracks, num_samples, form):
    """a base of another seed in one of five forms: 1, 2, 7 or S samples at the clip's rate, or 2 S - 1 at another; two tracks more than
    the clip in every second one; translations up to 5 from the origin, so that a `relative` clip is levered"""
    count, rate = ((1, RATE), (2, RATE), (7, RATE), (num_samples, RATE), (2 * num_samples - 1, BASE_RATE))[form]
    samples = restatement.mixed_clip(100 + k, count, num_tracks + 2 * (k % 2), offset=5 * k + 3)
    samples[:, :, 4:7] *= np.float32(10.0)
    return samples, rate


def cases_of(additive_format):
    """every shape once: the base's form, a clip without scale and a closing loop each in turn"""
    cases = []
    for k, (num_tracks, num_samples) in enumerate(SHAPES):
        case = Case()
        case.format = additive_format
        case.samples = clip_of(k, num_tracks, num_samples, additive_format, scales="default" if k % 4 == 1 else "mixed", close_loop=k % 3 == 0 and num_samples > 2)
        case.base_samples, case.base_rate = base_of(k, num_tracks, num_samples, (k + k // 6) % 5)
        case.base = additive.Base(case.base_samples, case.base_rate, additive_format)
        cases.append(case)
    return cases


def settings_of(additive_format, parents, **settings):
    settings.setdefault("precision", PRECISION)
    settings.setdefault("shell_distance", SHELL)
    if additive_format == ADDITIVE1:
        settings.setdefault("default_pose", ADDITIVE1_POSE)
    return dict(settings, parents=parents)


def launch_settings(settings):
    """the restatement's settings as the launches' keywords"""
    return {key: value for key, value in settings.items() if key not in ("precision", "shell_distance")}


def register(ctx, cases):
    for case in cases:
        case.handle = ctx.register_raw_tracks(case.samples, RATE, runtime.LOOP_CLAMP)
        case.base_handle = ctx.register_raw_tracks(case.base_samples, case.base_rate, runtime.LOOP_CLAMP)


def unregister(ctx, cases):
    for case in cases:
        ctx.unregister_raw_tracks(case.handle)
        ctx.unregister_raw_tracks(case.base_handle)


def search(ctx, cases, additive_format, level=MEDIUM, **settings):
    return launch(ctx, through("search", [case.base_handle for case in cases], additive_format), [case.handle for case in cases], level=level, **settings)


def check_levels(launched, expected):
    check_table(launched, expected, levels=True)


@pytest.fixture(scope="module")
def sweep(ctx):
    """per format every shape registered once with its base, and the restatement's search at medium with tree(0, 17), loops on, and its
    two writers at that table -- computed once, shared and left unchanged"""
    parents = restatement.tree(0, MAX_TRACKS)
    by_format = {}
    for additive_format in FORMATS:
        cases = by_format[additive_format] = cases_of(additive_format)
        register(ctx, cases)
        settings = settings_of(additive_format, parents, flags=OPTIMIZE_LOOPS)
        for case in cases:
            case.found, case.variable = additive.compress_with_search(case.samples, RATE, case.base, level=MEDIUM, **settings)
            case.drop_w = additive.compress_drop_w(case.samples, RATE, case.base, **settings)
            if case.samples.shape[1] >= 9:
                case.found_without = additive.find_bit_rates(case.samples, RATE, None, level=MEDIUM, **settings)
    yield ctx, parents, by_format
    for cases in by_format.values():
        unregister(ctx, cases)


@pytest.mark.parametrize("additive_format", FORMATS)
def test_the_table_is_the_restatements(sweep, additive_format):
    """one launch mixes every shape, each instance with a base of its own: every byte of every row, the sentinel everywhere else, the
    results with the level, the shell metadata on bits"""
    ctx, parents, by_format = sweep
    cases = by_format[additive_format]
    settings = launch_settings(settings_of(additive_format, parents, flags=OPTIMIZE_LOOPS))
    check_levels(search(ctx, cases, additive_format, **settings), [case.found for case in cases])
    # the sweep is worth its name: the base decides, votes pass and fail, clips without scale, every segment count, the object phase at work
    assert sum(not np.array_equal(case.found.table, case.found_without.table) for case in cases if case.samples.shape[1] >= 9) >= 3
    assert {len(case.found.base.segments) for case in cases} == {1, 2, 3}
    assert any(case.found.base.wrap for case in cases) and any(not case.found.base.wrap and case.samples.shape[0] > 2 for case in cases)
    assert any(not (case.found.base.types[2] != DEFAULT).any() and (case.found.base.types[0:2] == ANIMATED).any() for case in cases)
    assert any(not np.array_equal(case.found.table, case.found.local_table) for case in cases)


@pytest.mark.parametrize("additive_format", FORMATS)
def test_the_two_writers_are_the_restatements(sweep, additive_format):
    """both writers on every byte, a sentinel behind `size`, the shell metadata on bits; the header's default-scale bit is 0 under
    ADDITIVE1 alone"""
    ctx, parents, by_format = sweep
    cases = by_format[additive_format]
    settings = launch_settings(settings_of(additive_format, parents, flags=OPTIMIZE_LOOPS))
    bases = [case.base_handle for case in cases]
    tables = np.zeros((len(cases), MAX_SEGMENTS, MAX_TRACKS, 4), dtype=np.uint8)
    for row, case in enumerate(cases):
        tables[row, :case.found.table.shape[0], :case.found.table.shape[1]] = case.found.table
    handles = [case.handle for case in cases]
    check_rows(launch(ctx, through("variable", bases, additive_format), handles, rates=tables, **settings), [case.variable for case in cases])
    check_rows(launch(ctx, through("tracks", bases, additive_format), handles, **settings), [case.drop_w for case in cases])
    for case in cases:
        for blob in (case.variable.blob, case.drop_w.blob):
            assert (int(blob[28]) >> 1) & 1 == (0 if additive_format == ADDITIVE1 else 1)


def test_the_levels_on_the_chain_of_nine(ctx):
    """medium, highest and automatic (a chain of 9 is below 18: highest) with a base, at every format"""
    parents = restatement.tree(0, 9, "chain")
    for additive_format in FORMATS:
        case = Case()
        case.samples = clip_of(31, 9, 33, additive_format)
        case.base_samples, case.base_rate = base_of(31, 9, 33, 2)
        case.base = additive.Base(case.base_samples, case.base_rate, additive_format)
        register(ctx, [case])
        try:
            settings = settings_of(additive_format, parents)
            found = {level: additive.find_bit_rates(case.samples, RATE, case.base, level=level, **settings) for level in (MEDIUM, HIGHEST)}
            for level, expected in ((MEDIUM, found[MEDIUM]), (HIGHEST, found[HIGHEST]), (AUTOMATIC, found[HIGHEST])):
                launched = search(ctx, [case, case], additive_format, level=level, max_tracks=9, max_samples=33, **launch_settings(settings))
                check_levels(launched, [expected] * 2)
        finally:
            unregister(ctx, [case])


def test_a_loop_that_closes_only_on_the_base(ctx):
    """ADDITIVE0: the clip's last sample is its first moved by what the base moves between ITS first and last sample, so the vote passes
    with A_first on the base's sample 0 and A_last on its last, and fails without a base"""
    num_tracks, num_samples = 4, 17
    parents = restatement.tree(0, num_tracks)
    case = Case()
    case.samples = clip_of(41, num_tracks, num_samples, ADDITIVE0)
    case.base_samples, case.base_rate = base_of(41, num_tracks, 7, 2)
    case.base_samples[:, :, 0:4] = case.base_samples[0:1, :, 0:4]                   # (the base turns nothing, and scales nothing, over its length)
    case.base_samples[:, :, 8:11] = case.base_samples[0:1, :, 8:11]
    case.base_samples[:, :, 4:7] = np.random.default_rng(41).uniform(-5.0, 5.0, size=case.base_samples[:, :, 4:7].shape)    # (and moves every track)
    case.samples[-1] = case.samples[0]
    case.samples[-1, :, 4:7] = case.samples[0, :, 4:7] + (case.base_samples[0, :num_tracks, 4:7] - case.base_samples[-1, :num_tracks, 4:7])
    case.base = additive.Base(case.base_samples, case.base_rate, ADDITIVE0)
    settings = settings_of(ADDITIVE0, parents, flags=OPTIMIZE_LOOPS)
    with_base = additive.compress_with_search(case.samples, RATE, case.base, **settings)
    without = additive.compress_with_search(case.samples, RATE, None, **settings)
    assert with_base[1].wrap and with_base[1].num_samples == num_samples - 1 and not without[1].wrap
    register(ctx, [case])
    try:
        keywords = dict(max_tracks=num_tracks, max_samples=num_samples, **launch_settings(settings))
        check_levels(search(ctx, [case], ADDITIVE0, **keywords), [with_base[0]])
        check_rows(launch(ctx, through("variable", [case.base_handle], ADDITIVE0), [case.handle], rates=with_base[0].table, **keywords), [with_base[1]])
        check_rows(launch(ctx, through("tracks", [case.base_handle], ADDITIVE0), [case.handle], **keywords), [additive.compress_drop_w(case.samples, RATE, case.base, **settings)])
    finally:
        unregister(ctx, [case])


def test_none_through_the_fronts_is_the_base_calls_bytes(sweep):
    """ACLHIP_ADDITIVE_NONE: table and blobs of the entry points without a base, byte for byte, sentinels included, with handles of live
    bases, with handles of nothing and with no handles at all"""
    ctx, parents, by_format = sweep
    cases = [case for case in by_format[RELATIVE] if case.samples.shape[1] in (9, 17)]
    handles = [case.handle for case in cases]
    settings = dict(flags=OPTIMIZE_LOOPS, parents=parents)
    for bases in ([case.base_handle for case in cases], [0xFFFFFF], None):
        for without, kind, arguments in ((Entry("search", "level", 0), "search", {"level": HIGHEST}), (Entry("variable"), "variable", {"rates": (9, 14, 7)}), (Entry("tracks"), "tracks", {})):
            base, front = (launch(ctx, entry, handles, **arguments, **settings) for entry in (without, through(kind, bases, NONE)))
            assert np.array_equal(base.flat, front.flat) and np.array_equal(base.results, front.results) and np.array_equal(base.metadata, front.metadata)
            assert (base.results[:, 0] == runtime.COMPRESS_OK).all() and base.rejected == front.rejected == 0


def test_refusals_and_a_base_that_is_not_finite_leave_their_rows(sweep):
    """a base with fewer tracks than the instance and a handle of nothing: ACLHIP_COMPRESS_REFUSED, counted; a base with a NaN in a
    track the instance does not even have: ACLHIP_COMPRESS_NOT_FINITE; each between served neighbours, its rows left to the sentinel"""
    ctx, parents, by_format = sweep
    cases = [case for case in by_format[ADDITIVE0] if case.samples.shape == (33, 9, 12) or case.samples.shape == (17, 4, 12)]
    nine, four = (next(case for case in cases if case.samples.shape[1] == t) for t in (9, 4))
    bad = nine.base_samples.copy()
    bad[-1, bad.shape[1] - 1, 9] = np.inf
    h_bad = ctx.register_raw_tracks(bad, nine.base_rate, runtime.LOOP_CLAMP)
    dead = ctx.register_raw_tracks(nine.base_samples, nine.base_rate, runtime.LOOP_CLAMP)
    ctx.unregister_raw_tracks(dead)
    try:
        handles = [nine.handle, nine.handle, four.handle, nine.handle, nine.handle, nine.handle]
        bases = [nine.base_handle, four.base_handle, four.base_handle, dead, h_bad, nine.base_handle]
        assert four.base_samples.shape[1] < 9
        settings = launch_settings(settings_of(ADDITIVE0, parents, flags=OPTIMIZE_LOOPS))
        launched = launch(ctx, through("search", bases, ADDITIVE0), handles, **settings)
        check_levels(launched, [nine.found, REFUSED, four.found, REFUSED, NOT_FINITE, nine.found])
        tables = np.zeros((len(handles), MAX_SEGMENTS, MAX_TRACKS, 4), dtype=np.uint8)
        for row, case in ((0, nine), (2, four), (5, nine)):
            tables[row, :case.found.table.shape[0], :case.found.table.shape[1]] = case.found.table
        out = launch(ctx, through("variable", bases, ADDITIVE0), handles, rates=tables, with_metadata=False, **settings)
        check_rows(out, [nine.variable.blob, REFUSED, four.variable.blob, REFUSED, NOT_FINITE, nine.variable.blob])
        out = launch(ctx, through("tracks", bases, ADDITIVE0), handles, with_metadata=False, **settings)
        check_rows(out, [nine.drop_w.blob, REFUSED, four.drop_w.blob, REFUSED, NOT_FINITE, nine.drop_w.blob])
        with pytest.raises(ValueError, match="ACLHIP_COMPRESS_REFUSED"):
            runtime.find_bit_rates(ctx, [nine.handle], parents=parents, precision=PRECISION, shell_distance=SHELL, additive_base=four.base_handle, additive_format=ADDITIVE0)
        with pytest.raises(RuntimeError, match="not finite"):
            runtime.compress_tracks(ctx, [nine.handle], parents=parents, precision=PRECISION, shell_distance=SHELL, additive_base=h_bad, additive_format=ADDITIVE0)
    finally:
        ctx.unregister_raw_tracks(h_bad)


def test_search_then_compress_end_to_end(sweep):
    """runtime.compress_tracks_variable(bit_rates="search", additive_base=, additive_format=) is the restatement's blob at the
    restatement's table; it registers and is graded by runtime.raw_clip_error with the same base. For a clip WITH scale the worst error
    is at most the precision wherever every track met its threshold in every segment; for a clip without scale the error is printed
    (the finding recorded in tests/test_bit_rate_search_rate_range_oracle.py: the search's _no_scale errors are not what the measure takes)"""
    ctx, parents, by_format = sweep
    all_met = 0
    for additive_format in FORMATS:
        cases = [case for case in by_format[additive_format] if case.samples.shape[0] >= 17 and case.samples.shape[1] >= 4]
        settings = {"parents": parents, "precision": PRECISION, "shell_distance": SHELL, "optimize_loops": True, "additive_format": additive_format,
                    "additive_base": [case.base_handle for case in cases]}
        if additive_format == ADDITIVE1:
            settings["default_pose"] = ADDITIVE1_POSE
        handles = [case.handle for case in cases]
        tables = runtime.find_bit_rates(ctx, handles, **settings)
        blobs, searched = runtime.compress_tracks_variable(ctx, handles, bit_rates="search", return_levels=True, **settings)
        assert searched.tolist() == [MEDIUM] * len(cases)
        for row, (case, blob) in enumerate(zip(cases, blobs)):
            want = np.zeros(tables.shape[1:], dtype=np.uint8)
            want[:case.found.table.shape[0], :case.found.table.shape[1]] = case.found.table
            assert np.array_equal(tables[row], want)
            assert np.array_equal(blob, case.variable.blob)
            status, message = runtime.check_clip(blob, check_hash=True)
            assert status == 0, message
            num_tracks = case.samples.shape[1]
            pose = (ADDITIVE1_POSE if additive_format == ADDITIVE1 else np.tile(IDENTITY, (MAX_TRACKS, 1)))[:num_tracks]
            clip = ctx.register_clip(blob)
            skeleton = ctx.register_skeleton(parents[:num_tracks], pose)
            try:
                bone, error, _ = runtime.raw_clip_error(ctx, case.handle, clip, skeleton, SHELL, additive_base=case.base_handle, additive_format=additive_format)
            finally:
                ctx.unregister_skeleton(skeleton)
                ctx.unregister_clip(clip)
            met = case.found.met.all(axis=0)
            has_scale = bool((case.found.base.types[2] != DEFAULT).any())
            print("format %d case %d (%d tracks, %d samples, scale %s): %d tracks met their threshold in every segment; worst error %.6f at bone %d"
                  % (additive_format, row, num_tracks, case.samples.shape[0], has_scale, int(met.sum()), error, bone))
            if has_scale and met.all():
                all_met += 1
                assert error <= PRECISION
    assert all_met >= 3
