"""aclhip_find_bit_rates_batch and its _metric twin AT BOTH ENDS OF THE RATE TABLE. tests/test_gpu_bit_rate_search.py and
tests/test_gpu_matrix_metric_compress.py draw every input from mixed_clip, white noise, which at precision 0.01 lands in the rates 5 to 19
(and 1 in a clip of two samples): the rows of 2 to 4 bits and of the raw samples (rate 24) of the LDS value tables, a permutation list
walked to its end with nothing met, increment() arriving at 24, a link or a whole chain maxed out and the "rotation == translation, scale
already raw" bump with a real 24 were never run by a kernel under test. The inputs, each family in one launch per metric, mixed shapes
and a repeated handle in each (T in 1, 5, 17: one track has no parent, every object error a local one; S in 2, 31, 33 and 65):

  gentle         gentle_clip, mixed scales and every scale the default in turn: the rates 1 to 4
  far roots      far_roots_clip at 60 000 and at 250 000 in turn: the rates 23 and 24, the raw row picked by the local phase
  tight          mixed_clip searched at precision 1e-5: increment() reaches 24, chains maxed out, local phases that end with nothing met
  unreachable    mixed_clip with a precision of 1e-9 on a leaf, through track_precisions: the same exits, deterministically; the 5 x 2
                 clip alone in the first test of the file
  raw scale      raw_scale_clip: the bump with a real scale rate of 24, which no drawn input reaches (the branch is walked; on this clip
                 either order of raising ends on the same rates)
  chains of 17   gentle motion, and tight motion, where saturation climbs the longest chain

As in tests/test_gpu_bit_rate_search.py the expected tables are the restatement's and every comparison is on BYTES (the launch and
check_table of tests/compress_launches.py: every byte of every row, the sentinel everywhere else, the results, the shell metadata). Before a launch each test asserts on
the restatement's tables and Search.visits that its input goes where it is there to go: the comparison cannot pass on an input that
never went there. tests/test_bit_rate_search_rate_range_oracle.py holds the restatement to the reference's compressor on the gentle
and the far families; the tight and the unreachable inputs have no reference to be held to (the reference's own search is not stable
under one ulp there) and need none here. Then "search, then compress" end to end on the gentle and the far families. Tried once against
kernels changed on purpose: with an increment() that leaves a rate of 23 where it is, the tight, the unreachable and the chain tests
fail on bytes and every earlier test of the search passes; with the bump's scale comparison turned into `> 24` this file passes too.
Needs a GPU."""
import collections

import numpy as np
import pytest

from acl_amd import runtime
import compress_launches as launches
import matrix_metric_compress_restatement as metric_restatement
import variable_compress_restatement as restatement
from compress_launches import PRECISION, RATE, SHELL, Entry, Registered, check_table, ctx  # noqa: F401  (ctx: this module's fixture)
from matrix_metric_compress_restatement import METRIC_MATRIX, METRIC_QVVF
from variable_compress_restatement import ANIMATED, IDENTITY

pytestmark = pytest.mark.gpu

TIGHT = 1.0e-5
UNREACHABLE = 1.0e-9
TRACK_COUNTS, SAMPLE_COUNTS = (1, 5, 17), (2, 31, 33, 65)
SHAPES = [(t, s) for t in TRACK_COUNTS for s in SAMPLE_COUNTS]
MAX_TRACKS, MAX_SAMPLES, MAX_SEGMENTS = 17, 65, 4
METRICS = (METRIC_QVVF, METRIC_MATRIX)
PARENTS = restatement.tree(0, MAX_TRACKS)
CHAIN = restatement.tree(0, MAX_TRACKS, "chain")


def through(metric):
    """the entry point without a metric for the qvvf metric, the _metric front for the matrix metric"""
    return Entry("search") if metric == METRIC_QVVF else Entry("search", "metric", metric)


def find(samples, metric, **settings):
    settings.setdefault("precision", PRECISION)
    settings.setdefault("shell_distance", SHELL)
    return metric_restatement.find_bit_rates(samples, RATE, metric, **settings)


def offset_of(k, num_tracks):
    """where a clip's type triples start: 9 k as in the existing sweeps; one track alone has all three sub-tracks animated"""
    return 26 if num_tracks == 1 else 9 * k


def rates_of(found):
    """how often each rate occurs among the animated sub-tracks of a list of Search"""
    counts = collections.Counter()
    for f in found:
        for kind in range(3):
            counts.update(f.table[:, f.base.types[kind] == ANIMATED, kind].reshape(-1).tolist())
    return counts


def visits_of(found):
    total = collections.Counter()
    for f in found:
        total.update(f.visits)
    return total


def hold(ctx, clips, found, **settings):
    """one launch per metric over every clip in a mixed order with repeated handles, compared on every byte"""
    with Registered(ctx) as arrays:
        handles = [arrays.add(samples) for samples in clips]
        order = [(7 * i + 2) % len(handles) for i in range(len(handles) + 3)] if len(handles) > 1 else [0, 0]
        settings.setdefault("max_tracks", MAX_TRACKS)
        settings.setdefault("max_samples", MAX_SAMPLES)
        for metric in METRICS:
            launched = launches.launch(ctx, through(metric), [handles[k] for k in order], **settings)
            check_table(launched, [found[metric][k] for k in order])


def unreachable_precisions(*leaves):
    precisions = np.full(MAX_TRACKS, PRECISION, dtype=np.float32)
    precisions[list(leaves)] = UNREACHABLE
    return precisions


def test_the_unreachable_leaf_of_5_tracks_and_2_samples(ctx):
    """the smallest input that drives the object kernel's loops to their last exit: track 4, a leaf below 3 below 0, cannot be met; its
    chain is maxed out, link by link, and the pass ends there. Alone in its launch, first in the file"""
    samples = restatement.mixed_clip(0, 2, 5, offset=18)
    precisions = unreachable_precisions(4)
    settings = dict(parents=PARENTS, track_precisions=precisions)
    found = {metric: [find(samples, metric, **settings)] for metric in METRICS}
    for metric in METRICS:
        visits = found[metric][0].visits
        assert visits["chain_maxed_out"] >= 1 and visits["local_not_met"] >= 1 and visits["link_maxed_out"] >= 2 and visits["no_progress"] >= 1
        assert not found[metric][0].met[:, 4].any()
    hold(ctx, [samples], found, max_samples=2, **settings)


def test_gentle_motion_takes_the_rates_1_to_4(ctx):
    clips = [restatement.gentle_clip(k, num_samples, num_tracks, offset=offset_of(k, num_tracks), scales="default" if k % 2 else "mixed")
             for k, (num_tracks, num_samples) in enumerate(SHAPES)]
    found = {metric: [find(samples, metric, parents=PARENTS) for samples in clips] for metric in METRICS}
    for metric in METRICS:
        rates = rates_of(found[metric])
        assert all(rates[rate] >= 1 for rate in (1, 2, 3, 4)), sorted(rates.items())
        assert rates_of(f for f in found[metric] if len(f.base.segments) > 1)[2] >= 1          # and below 5 where a segment range is in play
        assert visits_of(found[metric])["ancestor_improved"] >= 1
        assert any(not (f.base.types[2] != restatement.DEFAULT).any() for f in found[metric]) and any((f.base.types[2] == ANIMATED).any() for f in found[metric])
    hold(ctx, clips, found, parents=PARENTS)


def far_clips():
    return [restatement.far_roots_clip(k, num_samples, num_tracks, 60000.0 if k % 2 else 250000.0, offset=offset_of(k, num_tracks), scales="default" if k % 4 == 1 else "mixed",
                                       parents=PARENTS[:num_tracks]) for k, (num_tracks, num_samples) in enumerate(SHAPES)]


def test_far_roots_take_the_rates_23_and_24(ctx):
    clips = far_clips()
    found = {metric: [find(samples, metric, parents=PARENTS) for samples in clips] for metric in METRICS}
    for metric in METRICS:
        rates = rates_of(found[metric])
        assert rates[24] >= 1 and rates[23] >= 1, sorted(rates.items())
        assert visits_of(found[metric])["local_picked_raw"] >= 1
        # the raw row is a root's translation, beside ordinary rates in the same table
        assert any((f.table[:, 0, 1] == 24).any() and min(rates_of([f])) < 20 for f in found[metric])
    hold(ctx, clips, found, parents=PARENTS)


def test_tight_precision_saturates_the_object_phase(ctx):
    clips = [restatement.mixed_clip(k, num_samples, num_tracks, offset=offset_of(k, num_tracks), scales="default" if k % 7 == 3 else "mixed")
             for k, (num_tracks, num_samples) in enumerate(SHAPES)]
    found = {metric: [find(samples, metric, parents=PARENTS, precision=TIGHT) for samples in clips] for metric in METRICS}
    for metric in METRICS:
        visits = visits_of(found[metric])
        for event in ("increment_reached_raw", "chain_maxed_out", "link_maxed_out", "local_not_met", "local_picked_raw", "no_progress", "ancestor_improved"):
            assert visits[event] >= 1, (event, dict(visits))
        assert rates_of(found[metric])[24] >= 1 and not all(f.met.all() for f in found[metric])
    hold(ctx, clips, found, parents=PARENTS, precision=TIGHT)


def test_an_unreachable_leaf_and_the_bump_with_a_raw_scale(ctx):
    """a precision of 1e-9 on track 4, the last leaf of the clips of 5 tracks, and on track 16, the last leaf of those of 17 (where
    track 4 is an inner track, as far out of reach as its leaf); and raw_scale_clip, whose two tracks and precisions go in a launch of
    their own"""
    shapes = [(5, 31), (5, 33), (17, 2), (17, 33), (17, 65), (5, 65)]
    clips = [restatement.mixed_clip(k, num_samples, num_tracks, offset=18) for k, (num_tracks, num_samples) in enumerate(shapes)]       # (from 18: the rotations of tracks 0 to 8 are animated)
    settings = dict(parents=PARENTS, track_precisions=unreachable_precisions(4, 16))
    assert 16 not in PARENTS.tolist() and 4 not in PARENTS[:5].tolist()
    found = {metric: [find(samples, metric, **settings) for samples in clips] for metric in METRICS}
    for metric in METRICS:
        for f in found[metric]:
            assert f.visits["chain_maxed_out"] >= 1 and f.visits["link_maxed_out"] >= 2, dict(f.visits)
            assert not f.met[:, f.table.shape[1] - 1].all()
        assert sum(f.visits["local_not_met"] >= 1 for f in found[metric]) >= len(clips) - 1        # (a local phase may find the raw row exact)
    hold(ctx, clips, found, **settings)

    made = [restatement.raw_scale_clip(seed, num_samples) for seed, num_samples in enumerate((5, 31, 33))]
    parents, precisions = made[0][1], made[0][2]
    clips = [samples for samples, _, _ in made]
    settings = dict(parents=parents, track_precisions=precisions)
    found = {metric: [find(samples, metric, **settings) for samples in clips] for metric in METRICS}
    for metric in METRICS:
        for f in found[metric]:
            assert f.visits["scale_raw_translation_bump"] >= len(f.base.segments) and (f.local_table[:, 0, 0:3] == (1, 1, 24)).all(), dict(f.visits)
    hold(ctx, clips, found, max_tracks=2, max_samples=33, **settings)


def test_chains_of_17_gentle_and_tight(ctx):
    """the longest walk: an increment kept on an ancestor under gentle motion; under tight motion every one of the 17 links maxed out"""
    gentle = [restatement.gentle_clip(6, 33, 17, offset=18), restatement.gentle_clip(7, 31, 17, offset=9, scales="default")]
    found = {metric: [find(samples, metric, parents=CHAIN) for samples in gentle] for metric in METRICS}
    for metric in METRICS:
        assert visits_of(found[metric])["ancestor_improved"] >= 1 and min(rates_of(found[metric])) <= 4
        assert any(not np.array_equal(f.table, f.local_table) for f in found[metric])
    hold(ctx, gentle, found, max_samples=33, parents=CHAIN)

    tight = [restatement.mixed_clip(6, 33, 17, offset=18), restatement.mixed_clip(7, 2, 17, offset=9, scales="default")]
    found = {metric: [find(samples, metric, parents=CHAIN, precision=TIGHT) for samples in tight] for metric in METRICS}
    for metric in METRICS:
        visits = visits_of(found[metric])
        assert visits["chain_maxed_out"] >= 1 and visits["link_maxed_out"] >= 17 and visits["increment_reached_raw"] >= 1 and visits["local_not_met"] >= 1, dict(visits)
        assert not found[metric][0].met[:, 16].any()            # the end of the chain was not met: the pass climbed all 17 links
    hold(ctx, tight, found, max_samples=33, parents=CHAIN, precision=TIGHT)


def test_search_then_compress_end_to_end_at_both_ends(ctx):
    """compress_tracks_variable(bit_rates="search") is the restatement's blob at the restatement's table in every byte, under both
    metrics; the blob passes check_clip with its hash and registers. On these clips every track met its threshold in every segment --
    asserted, so that the property is never vacuous --, so raw_clip_error, the clip's worst bone, is within the precision WHERE THE CLIP
    HAS SCALE. Where every scale is the default the search measures, as the reference's does, calculate_error_no_scale: the x and the y
    point of the shell (transform_error_metrics.h:360-378), while raw_clip_error, as the reference's calculate_compression_error
    (track_error.impl.h:240: has_scale = true), measures all three; a rotation error about an axis in the xy plane moves the z point
    furthest, and "met" bounds it no longer. The gentle clip of one track and 31 samples shows it: met at 0.009865 on two points, its
    blob 0.010991 on three (0.010991 as well by the restatement's decoded values on the CPU). Such clips are printed, not bounded: what
    holds them is the blob, equal in every byte to the restatement's at the restatement's table. The search, not a given table, puts
    the format byte of raw sub-tracks (31) and the rates 1 and 2 into these blobs"""
    picked = [k for k, shape in enumerate(SHAPES) if shape in ((17, 33), (17, 65), (5, 2), (1, 31), (5, 65))]
    gentle = [restatement.gentle_clip(k, SHAPES[k][1], SHAPES[k][0], offset=offset_of(k, SHAPES[k][0]), scales="default" if k % 2 else "mixed") for k in picked]
    far = [far_clips()[k] for k in picked]
    clips = gentle + far
    identity = np.tile(IDENTITY, (MAX_TRACKS, 1))
    formats, bounded = collections.Counter(), 0
    with Registered(ctx) as arrays:
        handles = [arrays.add(samples) for samples in clips]
        for metric in METRICS:
            settings = {"parents": PARENTS, "precision": PRECISION, "shell_distance": SHELL, "metric": metric}
            tables = runtime.find_bit_rates(ctx, handles, **settings)
            assert tables.shape == (len(clips), MAX_SEGMENTS, MAX_TRACKS, 4) and tables.dtype == np.uint8
            blobs = runtime.compress_tracks_variable(ctx, handles, bit_rates="search", **settings)
            for samples, handle, table, blob in zip(clips, handles, tables, blobs):
                found = find(samples, metric, parents=PARENTS)
                want = np.zeros((MAX_SEGMENTS, MAX_TRACKS, 4), dtype=np.uint8)
                want[:found.table.shape[0], :found.table.shape[1]] = found.table
                assert np.array_equal(table, want)
                expected = metric_restatement.compress_variable(samples, RATE, found.table, metric, parents=PARENTS, precision=PRECISION, shell_distance=SHELL)
                assert np.array_equal(blob, expected.blob)
                status, message = runtime.check_clip(blob, check_hash=True)
                assert status == 0, message
                for segment in restatement.parse(blob)["segments"]:
                    for kind in range(3):
                        formats.update(segment["formats"][kind].tolist())
                num_tracks = samples.shape[1]
                clip = ctx.register_clip(blob)
                skeleton = ctx.register_skeleton(PARENTS[:num_tracks], identity[:num_tracks])
                try:
                    bone, error, _ = runtime.raw_clip_error(ctx, handle, clip, skeleton, SHELL, metric=metric)
                finally:
                    ctx.unregister_skeleton(skeleton)
                    ctx.unregister_clip(clip)
                has_scale = bool((found.base.types[2] != restatement.DEFAULT).any())
                print("metric %d, %s, %s: worst error %.6f at bone %d" % (metric, samples.shape[0:2], "scale" if has_scale else "no scale", error, bone))
                assert found.met.all()
                if has_scale:
                    bounded += 1
                    assert error <= PRECISION
    assert bounded >= len(METRICS) * 6
    assert formats[restatement.RAW_FORMAT_BYTE] >= 1 and formats[1] >= 1 and formats[2] >= 1, sorted(formats.items())
