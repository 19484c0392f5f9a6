"""aclhip_find_bit_rates_level_batch through the C ABI: find_optimal_bit_rates at the levels high and highest, and at automatic, of
registered raw track arrays. The expected tables are the restatement's (tests/bit_rate_search_levels_restatement.py, which
tests/test_bit_rate_search_levels_oracle.py holds to the reference's compressor), and every comparison is on BYTES, as in
tests/test_gpu_bit_rate_search.py, through the launch and check_table of tests/compress_launches.py: a table of sentinel bytes behind
guards, every byte of every row held to the restatement and everything else to the sentinel, the statuses, the refusal count, the
clip's shell as metadata, the workspace no larger than its size function says -- and here the second word of every result, the level
that was searched.

The shapes are the smallest at which each mechanism can still go wrong: T in 1, 2, 3, 5, 17, 65 by S in 2, 31, 33 under tree(0, 65);
chains of 2 links (the single {2,1} arrangement, no triple), of 3 (the one {1,1,1}), of 9 and of 17 (680 arrangements of {1,1,1}); and
for every edge the wider first loop has (bit_rate_search_levels_restatement.VISITS) an input whose restatement went over it, asserted
before the launch. Needs a GPU. Fails on a library without the call."""
import collections

import numpy as np
import pytest

from acl_amd import runtime
import bit_rate_search_levels_restatement as levels
import compress_launches as launches
import variable_compress_restatement as restatement
from compress_launches import PRECISION, RATE, SENTINEL, SHELL, Entry, Registered, check_table, ctx, same  # noqa: F401  (ctx: this module's fixture)
from matrix_metric_compress_restatement import METRIC_MATRIX, METRIC_QVVF
from variable_compress_restatement import IDENTITY, OPTIMIZE_LOOPS

pytestmark = pytest.mark.gpu

TRACK_COUNTS, SAMPLE_COUNTS = (1, 2, 3, 5, 17, 65), (2, 31, 33)
SHAPES = [(t, s) for t in TRACK_COUNTS for s in SAMPLE_COUNTS]
MAX_TRACKS, MAX_SAMPLES, MAX_SEGMENTS = 65, 33, 2
HIGH, HIGHEST, AUTOMATIC = 3, 4, 100
REFUSED, NOT_FINITE = runtime.COMPRESS_REFUSED, runtime.COMPRESS_NOT_FINITE
NEW_EDGES = tuple("shape_%s_won" % name for name in levels.SHAPES) + ("invalid_permutation_skipped", "early_exit_in_shape", "two_reached_raw", "three_reached_raw",
                                                                         "two_one_on_two_links")


def find(samples, level=HIGHEST, metric=METRIC_QVVF, **settings):
    settings.setdefault("precision", PRECISION)
    settings.setdefault("shell_distance", SHELL)
    return levels.find_bit_rates_metric(samples, RATE, metric, level=level, **settings)


def launch(ctx, handles, level=HIGHEST, metric=METRIC_QVVF, entry=None, max_tracks=MAX_TRACKS, max_samples=MAX_SAMPLES, **settings):
    """One launch of aclhip_find_bit_rates_level_batch at `metric` (or of `entry`) over `handles` (tests/compress_launches.py)"""
    return launches.launch(ctx, entry or Entry("search", "level", metric), handles, max_tracks, max_samples, level=level, **settings)


def check(launched, expected):
    """the table, and the level that was searched in the second word of every served instance's result"""
    check_table(launched, expected, levels=True)


def edges_of(found):
    total = collections.Counter()
    for f in found:
        total.update(f.visits)
    return total


@pytest.fixture(scope="module")
def sweep(ctx):
    """every shape registered once, from mixed_clip as tests/test_gpu_bit_rate_search.py draws it (every seventh array no scale, about
    every second closes its loop); the restatement's tables at high and highest with tree(0, 65), loops on -- computed once, shared and
    left unchanged"""
    with Registered(ctx) as arrays:
        clips = [restatement.mixed_clip(k, num_samples, num_tracks, offset=9 * k, scales="default" if k % 7 == 3 else "mixed", close_loop=(k // 4 + k) % 2 == 1 and num_samples > 2)
                 for k, (num_tracks, num_samples) in enumerate(SHAPES)]
        handles = [arrays.add(samples) for samples in clips]
        parents = restatement.tree(0, MAX_TRACKS)
        found = {level: [find(samples, level, parents=parents, flags=OPTIMIZE_LOOPS) for samples in clips] for level in (HIGH, HIGHEST)}
        yield ctx, handles, clips, parents, found


@pytest.mark.parametrize("level", [HIGH, HIGHEST])
def test_the_table_is_the_restatements(sweep, level):
    """mixed shapes and a repeated handle in one launch: every byte of every row, the sentinel everywhere else, the results with the level"""
    ctx, handles, clips, parents, found = sweep
    edges = edges_of(found[level])
    assert edges["shape_2_won"] and edges["invalid_permutation_skipped"] and edges["early_exit_in_shape"] and (level == HIGH or edges["two_one_on_two_links"])
    assert any(f.base.wrap and f.base.num_samples == clip.shape[0] - 1 for f, clip in zip(found[level], clips))            # a vote that removed a sample
    order = [(7 * i + 2) % len(handles) for i in range(len(handles) + 3)]
    check(launch(ctx, [handles[k] for k in order], level, flags=OPTIMIZE_LOOPS, parents=parents), [found[level][k] for k in order])


def test_under_the_matrix_metric(sweep):
    ctx, handles, clips, parents, found = sweep
    picked = [k for k, shape in enumerate(SHAPES) if shape in ((2, 31), (3, 33), (5, 33), (17, 33))]
    for level in (HIGH, HIGHEST):
        expected = [find(clips[k], level, METRIC_MATRIX, parents=parents, flags=OPTIMIZE_LOOPS) for k in picked]
        assert any(not np.array_equal(mine.table, found[level][k].table) for mine, k in zip(expected, picked))              # the metrics are told apart
        check(launch(ctx, [handles[k] for k in picked], level, METRIC_MATRIX, flags=OPTIMIZE_LOOPS, parents=parents), expected)


def test_the_levels_below_high_are_the_other_calls_bytes(sweep):
    ctx, handles, clips, parents, found = sweep
    picked = [k for k, shape in enumerate(SHAPES) if shape in ((17, 33), (5, 33), (65, 31), (1, 2))]
    for level in (0, 1, 2):
        for metric in (METRIC_QVVF, METRIC_MATRIX) if level == 2 else (METRIC_QVVF,):
            new = launch(ctx, [handles[k] for k in picked], level, metric, flags=OPTIMIZE_LOOPS, parents=parents)
            other = Entry("search") if metric == METRIC_QVVF else Entry("search", "metric", metric)
            old = launch(ctx, [handles[k] for k in picked], level, entry=other, flags=OPTIMIZE_LOOPS, parents=parents)
            assert np.array_equal(new.flat, old.flat) and np.array_equal(new.metadata, old.metadata)
            assert np.array_equal(new.results[:, 0], old.results[:, 0]) and (old.results[:, 1] == 0).all() and (new.results[:, 1] == level).all()
            assert (new.flat != SENTINEL).any()


def test_chains_of_two_three_nine_and_seventeen(ctx):
    """a chain of 2: {2,1} has one arrangement and there is no triple; of 3: the one {1,1,1}; of 9 and 17: the longest walks, 36 and 136
    pairs, 84 and 680 triples a round. Together the five shapes each win a round"""
    clips = {links: restatement.mixed_clip(seed, 33, links, offset=9 * seed) for links, seed in ((2, 2), (3, 2), (9, 1), (17, 0))}
    clips["17 no scale"] = restatement.mixed_clip(6, 33, 17, offset=18, scales="default")
    settings = {(3): {"precision": 0.001}}
    with Registered(ctx) as arrays:
        handles = {key: arrays.add(samples) for key, samples in clips.items()}
        edges = collections.Counter()
        for level in (HIGH, HIGHEST):
            for key, samples in clips.items():
                parents = restatement.tree(0, samples.shape[1], "chain")
                found = find(samples, level, parents=parents, **settings.get(key, {}))
                edges.update(found.visits)
                check(launch(ctx, [handles[key], handles[key]], level, max_tracks=samples.shape[1], parents=parents, **settings.get(key, {})), [found, found])
        parents = restatement.tree(0, 17, "chain")
        deep = find(clips[17], HIGHEST, METRIC_MATRIX, parents=parents)
        check(launch(ctx, [handles[17]], HIGHEST, METRIC_MATRIX, max_tracks=17, parents=parents), [deep])
        assert all(edges["shape_%s_won" % name] for name in ("2", "1_1", "3", "1_1_1")) and edges["two_one_on_two_links"], edges
        assert not (find(clips["17 no scale"], HIGHEST, parents=parents).base.types[2] != restatement.DEFAULT).any()


def test_every_edge_of_the_wider_loop(ctx):
    """the inputs that are here for an edge: a chain of 3 at precision 0.001 where {2,1} wins a round; a chain of 2 at precision 1e-5,
    where increases by 2 and by 3 run into rate 24 and both of {2,1}'s links may have nothing left to give. The other edges of
    NEW_EDGES are asserted where their inputs are: in the sweep's and in the chains' tests"""
    two_one = restatement.mixed_clip(2, 17, 3, offset=18)
    raw = restatement.mixed_clip(2, 17, 2, offset=18)
    with Registered(ctx) as arrays:
        h_two_one, h_raw = arrays.add(two_one), arrays.add(raw)
        f_two_one = find(two_one, HIGHEST, parents=restatement.tree(2, 3, "chain"), precision=0.001)
        f_raw = find(raw, HIGHEST, parents=restatement.tree(2, 2, "chain"), precision=1.0e-5)
        assert f_two_one.visits["shape_2_1_won"] and f_two_one.visits["early_exit_in_shape"] and f_two_one.visits["invalid_permutation_skipped"]
        assert f_raw.visits["two_reached_raw"] and f_raw.visits["three_reached_raw"] and f_raw.visits["two_one_on_two_links"] and f_raw.visits["invalid_permutation_skipped"]
        assert f_raw.evaluations < f_raw.evaluations_unmemoized                    # the memo had something to keep
        check(launch(ctx, [h_two_one], HIGHEST, max_tracks=3, max_samples=17, parents=restatement.tree(2, 3, "chain"), precision=0.001), [f_two_one])
        check(launch(ctx, [h_raw], HIGHEST, max_tracks=2, max_samples=17, parents=restatement.tree(2, 2, "chain"), precision=1.0e-5), [f_raw])
        for metric in (METRIC_QVVF, METRIC_MATRIX):
            f_high = find(raw, HIGH, metric, parents=restatement.tree(2, 2, "chain"), precision=1.0e-5)
            check(launch(ctx, [h_raw], HIGH, metric, max_tracks=2, max_samples=17, parents=restatement.tree(2, 2, "chain"), precision=1.0e-5), [f_high])


def test_precisions_and_shell_distances_per_track_and_a_default_pose(ctx):
    rng = np.random.default_rng(31)
    precisions = rng.choice(np.array([0.002, 0.01, 0.05], dtype=np.float32), size=17)
    distances = rng.choice(np.array([1.0, 3.0, 10.0], dtype=np.float32), size=17)
    pose = restatement.lossy.raw_restatement.bind_pose(21, 17)
    clips = [restatement.mixed_clip(7, 33, 17, offset=3, default_pose=pose), restatement.mixed_clip(8, 33, 5, offset=12, default_pose=pose)]
    parents = restatement.tree(3, 17)
    settings = {"parents": parents, "track_precisions": precisions, "track_shell_distances": distances, "default_pose": pose}
    with Registered(ctx) as arrays:
        handles = [arrays.add(samples) for samples in clips]
        found = [find(samples, HIGHEST, **settings) for samples in clips]
        assert len({float(p) for p in found[0].shells[:, :, 1].reshape(-1)}) > 1
        assert any(f.visits[name] for f in found for name in NEW_EDGES)
        check(launch(ctx, handles, HIGHEST, max_tracks=17, **settings), found)


def test_an_instance_that_ends_with_a_status_leaves_its_rows_and_its_level_word(ctx):
    """handle 0 (refused) and a sample that is not finite, each between served neighbours whose rows and levels are right"""
    small, long = restatement.mixed_clip(2, 12, 5, offset=20), restatement.mixed_clip(3, 33, 5, offset=20)
    parents = restatement.tree(4, 5)
    with Registered(ctx) as arrays:
        h_small, h_long = arrays.add(small), arrays.add(long)
        bad = long.copy()
        bad[7, 2, 5] = np.nan
        h_bad = arrays.add(bad)
        for level in (HIGHEST, AUTOMATIC):
            f_small, f_long = find(small, level, parents=parents), find(long, level, parents=parents)
            assert f_small.level == f_long.level == HIGHEST
            check(launch(ctx, [h_small, 0, h_long, h_bad, h_small], level, max_tracks=5, parents=parents), [f_small, REFUSED, f_long, NOT_FINITE, f_small])
        check(launch(ctx, [h_small, h_long, h_small], HIGH, max_tracks=5, max_samples=32, parents=parents), [find(small, HIGH, parents=parents), REFUSED, find(small, HIGH, parents=parents)])
        with pytest.raises(RuntimeError, match="not finite"):
            runtime.find_bit_rates(ctx, h_bad, level="highest", parents=parents, precision=PRECISION, shell_distance=SHELL)


def test_strides_larger_than_the_minimum(sweep):
    ctx, handles, clips, parents, found = sweep
    picked = [k for k, shape in enumerate(SHAPES) if shape in ((3, 33), (65, 33), (17, 31), (1, 2))]
    segment_stride = 4 * MAX_TRACKS + 12
    check(launch(ctx, [handles[k] for k in picked], HIGHEST, flags=OPTIMIZE_LOOPS, parents=parents, segment_stride=segment_stride, instance_stride=MAX_SEGMENTS * segment_stride + 8),
          [found[HIGHEST][k] for k in picked])


def test_two_runs_give_the_same_bytes_and_a_capture_replays_to_them(sweep):
    ctx, handles, clips, parents, found = sweep
    picked = [k for k, shape in enumerate(SHAPES) if shape[0] in (5, 17)]
    runs = [launch(ctx, [handles[k] for k in picked], HIGHEST, flags=OPTIMIZE_LOOPS, parents=parents, graph=graph) for graph in (False, False, True)]
    assert same(runs[0], runs[1])
    assert same(runs[0], runs[2]) and (runs[2].results[:, 1] == HIGHEST).all()           # the same launch captured into a graph and replayed


def test_automatic_decides_the_level_per_instance(ctx):
    """one launch mixing chains of 17, 18, 24 and 25 bones (17 samples) and a clip of 501 samples: highest, high, high, medium, medium --
    the level words and each table are the restatement's at that level"""
    chains = [restatement.mixed_clip(seed, 17, links, offset=9 * seed) for links, seed in ((17, 1), (18, 1), (24, 0), (25, 0))]
    long = restatement.mixed_clip(5, 501, 3, offset=45)
    parents = restatement.tree(0, 25, "chain")
    with Registered(ctx) as arrays:
        handles = [arrays.add(samples) for samples in chains + [long]]
        found = [find(samples, AUTOMATIC, parents=parents) for samples in chains + [long]]
        assert [f.level for f in found] == [4, 3, 3, 2, 2]
        assert found[4].base.num_samples == 501 and levels.automatic_level(500, parents, 3) == 4
        # the level matters to the first three: the table of the neighbouring level differs
        assert all(not np.array_equal(f.table, find(samples, neighbour, parents=parents).table) for f, samples, neighbour in zip(found[:3], chains[:3], (3, 4, 2)))
        order = [4, 0, 3, 1, 2, 0]
        check(launch(ctx, [handles[k] for k in order], AUTOMATIC, max_tracks=25, max_samples=501, parents=parents), [found[k] for k in order])
        tables, searched = runtime.find_bit_rates(ctx, handles[:4], level="automatic", parents=parents, precision=PRECISION, shell_distance=SHELL, return_levels=True)
        assert searched.tolist() == [4, 3, 3, 2] and np.array_equal(tables[1, 0, :18], found[1].table[0])


def test_search_then_compress_end_to_end(sweep):
    """compress_tracks_variable(bit_rates="search", level="highest") is the restatement's blob at the restatement's table in every byte,
    and the blob registers. The total blob bytes per level are printed, not ordered: the reference's own high is larger than its medium
    on some clips"""
    ctx, handles, clips, parents, found = sweep
    picked = [k for k, shape in enumerate(SHAPES) if shape in ((65, 33), (17, 33), (17, 31), (5, 33), (3, 31))]
    settings = {"parents": parents, "precision": PRECISION, "shell_distance": SHELL, "optimize_loops": True}
    totals = {}
    for level in ("medium", "high", "highest"):
        blobs, searched = runtime.compress_tracks_variable(ctx, [handles[k] for k in picked], bit_rates="search", level=level, return_levels=True, **settings)
        totals[level] = sum(int(blob.size) for blob in blobs)
        assert searched.tolist() == [runtime.COMPRESSION_LEVELS[level]] * len(picked)
        if level == "medium":
            continue
        for k, blob in zip(picked, blobs):
            mine = found[runtime.COMPRESSION_LEVELS[level]][k]
            expected = restatement.compress(clips[k], RATE, mine.table, parents=parents, flags=OPTIMIZE_LOOPS, precision=PRECISION, shell_distance=SHELL)
            assert np.array_equal(blob, expected.blob)
            status, message = runtime.check_clip(blob, check_hash=True)
            assert status == 0, message
            clip = ctx.register_clip(blob)
            skeleton = ctx.register_skeleton(parents[:clips[k].shape[1]], np.tile(IDENTITY, (clips[k].shape[1], 1)))
            try:
                bone, error, _ = runtime.raw_clip_error(ctx, handles[k], clip, skeleton, SHELL)
            finally:
                ctx.unregister_skeleton(skeleton)
                ctx.unregister_clip(clip)
            assert error <= PRECISION or not mine.met.all(axis=0)[bone]
    print("blob bytes of %d clips per level: %s" % (len(picked), totals))
