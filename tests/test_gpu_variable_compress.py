"""aclhip_compress_tracks_variable_batch through the C ABI: compress_track_list with quatf_drop_w_variable / vector3f_variable /
vector3f_variable at GIVEN bit rates of registered raw track arrays. The expected blobs, results and shells are the restatement's
(tests/variable_compress_restatement.py, which tests/test_variable_compress_oracle.py holds to the reference's compressor), and every
comparison is on BYTES and BITS: both sides follow one definition, nothing has a tolerance.

The output region is the one of tests/compress_launches.py: a flat buffer of a sentinel byte, a guard, n rows, a guard;
one comparison holds [0, size) of every row to the blob and everything else to the sentinel. The shapes are T in 1, 3, 4, 5, 17, 65 (a
partial and a full group of four, a types word, a wave) and S in 1, 2, 31, 32, 33, 49, 65 (one segment; two; two dealt out 17 + 16;
three; and 32 closing on its first sample, voted down to one segment of 31). The sample rate is a power of two, so that the key times
i / rate are exact. Needs a GPU."""
import numpy as np
import pytest

from acl_amd import runtime
from oracle import bindings as ob
import compress_launches as launches
import variable_compress_restatement as restatement
from compress_launches import PRECISION, RATE, SHELL, Entry, Registered, check_rows, ctx, same  # noqa: F401  (ctx: this module's fixture)
from variable_compress_restatement import ANIMATED, LANES, OPTIMIZE_LOOPS, XYZ

pytestmark = pytest.mark.gpu

TRACK_COUNTS, SAMPLE_COUNTS = (1, 3, 4, 5, 17, 65), (1, 2, 31, 32, 33, 49, 65)
SHAPES = [(t, s) for t in TRACK_COUNTS for s in SAMPLE_COUNTS]
MAX_TRACKS, MAX_SAMPLES = 65, 65
MAX_SEGMENTS = 4
PARENTS, DESCRIPTIONS = restatement.INCLUDE_PARENT_TRACK_INDICES, restatement.INCLUDE_TRACK_DESCRIPTIONS


def launch(ctx, handles, rates, entry=Entry("variable"), max_tracks=MAX_TRACKS, max_samples=MAX_SAMPLES, **settings):
    """One launch over `handles` (tests/compress_launches.py). rates: three uniform rates, or a uint8 array whose last axes are [tracks, 4]"""
    return launches.launch(ctx, entry, handles, max_tracks, max_samples, rates=rates, **settings)


def compress(samples, rates, **settings):
    return restatement.compress(samples, RATE, rates, precision=PRECISION, shell_distance=SHELL, **settings)


def random_rates(seed, count):
    """[count, MAX_SEGMENTS, MAX_TRACKS, 4]: every rate 1 .. 24 about evenly"""
    rng = np.random.default_rng(70 + seed)
    rates = rng.integers(1, 25, size=(count, MAX_SEGMENTS, MAX_TRACKS, 4)).astype(np.uint8)
    rates[..., 3] = 0
    return rates


@pytest.fixture(scope="module")
def sweep(ctx):
    """every shape registered once, from variable_compress_restatement.mixed_clip: track b of array k has the (b + 9 k)-th of the 27
    (rotation, translation, scale) type triples, every seventh array no scale; every second array ends on its first sample, the S = 32 ones all do; the restatement at one uniform
    setting and at one table per instance, loops on -- computed once, shared and left unchanged"""
    with Registered(ctx) as arrays:
        clips = [restatement.mixed_clip(k, num_samples, num_tracks, offset=9 * k, scales="default" if k % 7 == 3 else "mixed", close_loop=k % 2 == 1 or num_samples == 32)
                 for k, (num_tracks, num_samples) in enumerate(SHAPES)]
        handles = [arrays.add(samples) for samples in clips]
        parents = restatement.tree(0, MAX_TRACKS)
        rates = random_rates(0, len(clips))
        for k, samples in enumerate(clips):
            closes = (k % 2 == 1 or samples.shape[0] == 32) and samples.shape[0] > 1           # (the vote takes the last sample)
            if restatement.num_segments(samples.shape[0] - (1 if closes else 0)) > 1:
                rates[k, 1::2, k % 3::3, 0:3] = 0            # rate 0 in some segments only, where segment ranges exist
                rates[k, :, k % 5::5, k % 3] = 0
        by_table = [compress(samples, rates[k], parents=parents, flags=OPTIMIZE_LOOPS) for k, samples in enumerate(clips)]
        uniform = [compress(samples, (9, 14, 7), parents=parents, flags=OPTIMIZE_LOOPS) for samples in clips]
        yield ctx, handles, clips, parents, rates, by_table, uniform


def test_uniform_rates_are_the_restatement(sweep):
    """mixed shapes and repeated handles in one launch: every byte of [0, size) with the hash, the sentinel behind, the results, the
    shell metadata on bits"""
    ctx, handles, clips, parents, _, _, uniform = sweep
    order = [(5 * i + 2) % len(handles) for i in range(len(handles) + 5)]
    check_rows(launch(ctx, [handles[k] for k in order], (9, 14, 7), flags=OPTIMIZE_LOOPS, parents=parents), [uniform[k] for k in order])
    by_shape = dict(zip(SHAPES, uniform))
    assert [len(by_shape[17, s].segments) for s in SAMPLE_COUNTS] == [1, 1, 1, 1, 2, 2, 4] and len(by_shape[65, 49].segments) == 3       # (17, 49) closes: 48 samples are two segments
    assert by_shape[17, 32].wrap and by_shape[17, 32].segments == [(0, 31)] and by_shape[17, 33].segments == [(0, 17), (17, 16)]
    # all 27 (rotation, translation, scale) triples, in one array of 65 tracks by itself
    assert len(restatement.triples_of(by_shape[65, 65])) == 27 and len(set().union(*(restatement.triples_of(c) for c in uniform))) == 27
    assert any(not (c.types[2] != restatement.DEFAULT).any() for c in uniform)                    # a clip without scale


def test_a_table_per_instance_and_segment_is_the_restatement(sweep):
    """every rate 0 .. 24 in one launch, 0 in some segments only; instance and segment strides from the table's shape"""
    ctx, handles, clips, parents, rates, by_table, _ = sweep
    check_rows(launch(ctx, handles, rates, flags=OPTIMIZE_LOOPS, parents=parents), by_table)
    used = set()
    for c in by_table:
        for kind in range(3):
            used |= set(c.rates[:, c.animated[kind], kind].reshape(-1).tolist())
    assert used == set(range(25))


def test_shared_rows_and_metadata(sweep):
    """a stride of 0 shares the rows: one [tracks, 4] row for every instance and segment, one [segments, tracks, 4] table for every
    instance; parent indices and descriptions behind a stream that ends on any byte; a default pose; no shell metadata asked for"""
    ctx, handles, clips, parents, rates, _, _ = sweep
    flags = PARENTS | DESCRIPTIONS | OPTIMIZE_LOOPS
    pose = restatement.lossy.raw_restatement.bind_pose(21, MAX_TRACKS)
    row = rates[3, 0]
    picked = list(range(0, len(handles), 3))
    want = [compress(clips[k], row, parents=parents, flags=flags, default_pose=pose) for k in picked]
    check_rows(launch(ctx, [handles[k] for k in picked], row, flags=flags, parents=parents, default_pose=pose), want)
    check_rows(launch(ctx, [handles[k] for k in picked], row, flags=flags, parents=parents, default_pose=pose, with_metadata=False), [c.blob for c in want])
    table = rates[3]
    want = [compress(clips[k], table, parents=parents, flags=PARENTS) for k in picked]
    check_rows(launch(ctx, [handles[k] for k in picked], table, flags=PARENTS, parents=parents), want)
    # the same table through explicit strides with room between the rows
    wide = np.zeros((len(picked), MAX_SEGMENTS + 1, MAX_TRACKS + 3, 4), dtype=np.uint8)
    wide[:, :MAX_SEGMENTS, :MAX_TRACKS] = rates[picked]
    want = [compress(clips[k], rates[k], parents=parents) for k in picked]
    check_rows(launch(ctx, [handles[k] for k in picked], wide, parents=parents), want)


def test_the_blobs_check_register_and_decode(sweep):
    """each blob of runtime.compress_tracks_variable passes aclhip_check_clip with the hash, registers, and decodes at every key time
    through the ordinary decode (ROUND_FLOOR, NORMALIZE_NEVER) to the bits oracle_decompress_tracks gives for the same blob, and in x, y, z
    of every sub-track to the values the restatement dequantizes"""
    ctx, handles, clips, parents, rates, by_table, _ = sweep
    picked = [k for k, shape in enumerate(SHAPES) if shape[0] in (5, 65) and shape[1] in (2, 32, 33, 65)]
    blobs = runtime.compress_tracks_variable(ctx, [handles[k] for k in picked], bit_rates=rates[picked], parents=parents, precision=PRECISION, shell_distance=SHELL, optimize_loops=True)
    options = ob.default_options(normalization=ob.NORMALIZE_NEVER)
    params = runtime.default_params(rounding_policy=runtime.ROUND_FLOOR, looping_policy=runtime.LOOP_AS_COMPRESSED, normalization=runtime.NORMALIZE_NEVER)
    for blob, k in zip(blobs, picked):
        want = by_table[k]
        assert blob.ctypes.data % 16 == 0 and np.array_equal(blob, want.blob)
        status, message = runtime.check_clip(blob, check_hash=True)
        assert status == 0, message
        clip = ctx.register_clip(blob)
        try:
            info = ctx.clip_info(clip)
            assert (info.num_tracks, info.num_samples) == (clips[k].shape[1], want.num_samples)
            times = (np.arange(want.num_samples) / RATE).astype(np.float32)
            poses = ctx.decompress_tracks(np.full(len(times), clip, dtype=np.uint32), times, params=params)
        finally:
            ctx.unregister_clip(clip)
        for key, time in enumerate(times):
            by_oracle = ob.oracle_decompress_tracks(blob, float(time), ob.ROUND_FLOOR, options=options)
            for lanes in LANES:
                assert np.array_equal(poses[key][:, lanes].view(np.uint32), by_oracle[:, lanes].view(np.uint32)), (k, key)
            for lanes in XYZ:
                assert np.array_equal(poses[key][:, lanes].view(np.uint32), want.decoded[key][:, lanes].view(np.uint32)), (k, key)


def test_a_zero_minimum_or_maximum_has_the_sign_of_the_last_zero_sample(ctx):
    """the analysis' pass of its own for a clip range that begins or ends on a zero of both signs"""
    clips = [restatement.signed_zeros(seed, num_samples, num_tracks) for seed, (num_tracks, num_samples) in enumerate(((3, 12), (5, 40), (5, 65)))]
    parents = restatement.tree(1, 5)
    with Registered(ctx) as arrays:
        handles = [arrays.add(samples) for samples in clips]
        want = [compress(samples, (11, 12, 13), parents=parents) for samples in clips]
        assert all(c.types[1, 0] == ANIMATED and c.clip_ranges[1, 0][0].view(np.uint32)[0] == 0x80000000 for c in want)
        check_rows(launch(ctx, handles, (11, 12, 13), max_tracks=5, parents=parents), want)


def test_segment_ranges_on_the_edges_of_the_fix_up(ctx):
    """minima and maxima of a segment that are k / 255 in its several float32 spellings, and their neighbours: the division, floorf, ceilf
    and both selects of the fix-up, and the quantization behind them at a low, a middle and the highest rate"""
    clips = [restatement.fixup_boundaries(num_tracks) for num_tracks in (5, 17, 65)]
    parents = restatement.tree(2, MAX_TRACKS)
    with Registered(ctx) as arrays:
        handles = [arrays.add(samples) for samples in clips]
        for rates in ((8, 3, 8), (12, 11, 12), (16, 23, 16)):
            check_rows(launch(ctx, handles, rates, parents=parents), [compress(samples, rates, parents=parents) for samples in clips])


def test_translation_and_scale_see_the_rotation_as_it_was_compacted(ctx):
    """a default rotation of length 2.2, used as given: the rotation becomes DEFAULT, and the scale is ANIMATED only under that default --
    under the registered rotation it stays within the precision of its first sample and of the default (variable_compress_restatement.long_default_rotation)"""
    samples, pose = restatement.long_default_rotation()
    with Registered(ctx) as arrays:
        handle = arrays.add(samples)
        want = restatement.compress(samples, RATE, (9, 9, 9), default_pose=pose, precision=84.0, shell_distance=SHELL)
        assert want.types[:, 0].tolist() == [restatement.DEFAULT, restatement.DEFAULT, ANIMATED]
        unit = restatement.compress(samples, RATE, (9, 9, 9), precision=84.0, shell_distance=SHELL)
        assert unit.types[:, 0].tolist() == [restatement.DEFAULT, restatement.DEFAULT, restatement.DEFAULT]
        check_rows(launch(ctx, [handle, handle], (9, 9, 9), max_tracks=1, max_samples=12, default_pose=pose, precision=84.0), [want, want])
        check_rows(launch(ctx, [handle], (9, 9, 9), max_tracks=1, max_samples=12, precision=84.0), [unit])


def test_refusals_leave_their_rows(ctx):
    """rate 25; rate 0 in a blob of one segment; more samples than max_samples; a stride too small; the drop-w call's refusals (a parent
    behind its child, handle 0) and not finite samples -- each next to served neighbours, its row untouched"""
    small, long = restatement.clip(0, 12, 5), restatement.clip(1, 40, 5)
    rng = np.random.default_rng(11)
    for samples in (small, long):                       # (something of every kind moves in both)
        samples[:, 1:4, 4:7] = rng.uniform(-0.5, 0.5, size=(samples.shape[0], 3, 3))
        samples[:, 2:4, 0:4] = restatement.lossy.raw_restatement.unit_quaternions(rng, (samples.shape[0], 2))
    parents = restatement.tree(4, 5)
    refused = runtime.COMPRESS_REFUSED
    with Registered(ctx) as arrays:
        h_small, h_long = arrays.add(small), arrays.add(long)
        bad = long.copy()
        bad[7, 2, 5] = np.nan
        h_bad = arrays.add(bad)
        rates = np.full((3, 3, 5, 4), 8, dtype=np.uint8)
        c_small, c_long = compress(small, rates[0], parents=parents), compress(long, rates[0], parents=parents)
        long_types = c_long.types
        moving = [[b for b in range(5) if c_small.types[kind, b] == ANIMATED and c_long.types[kind, b] == ANIMATED] for kind in range(3)]
        rates[1, 0, moving[1][0], 1] = 25               # one translation of one segment of instance 1
        rates[2, :, moving[0][0], 0] = 0                # every segment of a rotation of instance 2
        settings = {"max_tracks": 5, "max_samples": 40, "parents": parents}
        check_rows(launch(ctx, [h_small, h_long, 0, h_bad, h_small], (8, 8, 8), **settings), [c_small, c_long, refused, runtime.COMPRESS_NOT_FINITE, c_small])
        # (the shell of an instance the layout refuses was computed: its metadata is written; from here on only the rows are looked at)
        settings["with_metadata"] = False
        c_small, c_long = c_small.blob, c_long.blob
        check_rows(launch(ctx, [h_small, h_long, h_long], rates, **settings), [c_small, refused, compress(long, rates[2], parents=parents).blob])
        check_rows(launch(ctx, [h_long, h_small, h_small], rates, **settings), [c_long, refused, refused])
        check_rows(launch(ctx, [h_small, h_small], (0, 8, 8), **settings), [refused, refused])
        # a rate that no animated sub-track reads is not looked at
        ignored = rates[0].copy()
        for kind in range(3):
            ignored[:, long_types[kind] != ANIMATED, kind] = 77
        check_rows(launch(ctx, [h_long], ignored, **settings), [c_long])
        # max_samples 39: the array of 40 is refused, unless the vote takes one away
        check_rows(launch(ctx, [h_small, h_long, h_small], (8, 8, 8), max_tracks=5, max_samples=39, parents=parents, with_metadata=False), [c_small, refused, c_small])
        closed = long.copy()
        closed[-1] = closed[0]
        h_closed = arrays.add(closed)
        voted = compress(closed, (8, 8, 8), parents=parents, flags=OPTIMIZE_LOOPS)
        assert voted.num_samples == 39
        check_rows(launch(ctx, [h_closed, h_long], (8, 8, 8), max_tracks=5, max_samples=39, flags=OPTIMIZE_LOOPS, parents=parents, with_metadata=False), [voted.blob, refused])
        # a stride that holds the small blob and not the long one; and the largest stride that does not hold the small one
        stride = (c_small.size + 15) & ~15
        assert stride < c_long.size and c_small.size % 16 != 0
        check_rows(launch(ctx, [h_small, h_long, h_small], rates[0], stride=stride, **settings), [c_small, refused, c_small])
        check_rows(launch(ctx, [h_small, h_long], rates[0], stride=c_small.size & ~15, **settings), [refused, refused])
        check_rows(launch(ctx, [h_small, h_long], rates[0], max_tracks=5, max_samples=40, parents=np.array([0xFFFFFFFF, 0, 3, 0, 0], dtype=np.uint32)), [refused, refused])
        with pytest.raises(ValueError, match="ACLHIP_COMPRESS_REFUSED"):
            runtime.compress_tracks_variable(ctx, h_small, bit_rates=(0, 8, 8), parents=parents, precision=PRECISION, shell_distance=SHELL)


def test_two_runs_give_the_same_bytes_and_a_capture_replays_to_them(sweep):
    ctx, handles, clips, parents, rates, by_table, _ = sweep
    runs = [launch(ctx, handles, rates, flags=OPTIMIZE_LOOPS, parents=parents, graph=graph) for graph in (False, False, True)]
    assert same(runs[0], runs[1])
    assert same(runs[0], runs[2])           # the same launch captured into a graph and replayed


def test_compress_tracks_at_precision(ctx):
    """the blob that comes back is within the precision asked by raw_clip_error, and the rate below it is not"""
    samples = restatement.clip(2, 33, 17)
    parents = restatement.tree(2, 17)
    identity = np.tile(restatement.IDENTITY, (17, 1))
    precision = 0.01
    with Registered(ctx) as arrays:
        raw = arrays.add(samples)
        skeleton = ctx.register_skeleton(parents, identity)
        try:
            blob, rate = runtime.compress_tracks_at_precision(ctx, raw, skeleton, SHELL, precision, parents=parents, shell_distance=SHELL)
            assert rate is not None and 1 < rate <= 24

            def error_of(candidate):
                clip = ctx.register_clip(candidate)
                try:
                    return runtime.raw_clip_error(ctx, raw, clip, skeleton, SHELL)[1]
                finally:
                    ctx.unregister_clip(clip)
            assert error_of(blob) <= precision
            below = runtime.compress_tracks_variable(ctx, raw, bit_rates=(rate - 1,) * 3, parents=parents, precision=precision, shell_distance=SHELL)[0]
            assert error_of(below) > precision
            assert np.array_equal(blob, compress(samples, (rate,) * 3, parents=parents).blob)
        finally:
            ctx.unregister_skeleton(skeleton)
