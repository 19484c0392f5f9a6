"""The restatement of tests/variable_compress_restatement.py -- the definition aclhip_compress_tracks_variable_batch is held to by
tests/test_gpu_variable_compress.py -- against the reference's own compress_track_list (oracle/_ref/libaclref_compress.so,
aclref_compress_ex) with quatf_drop_w_variable / vector3f_variable / vector3f_variable at the levels lowest and medium. The reference
SEARCHES its bit rates; the restatement takes them: each test reads the rates the reference chose out of its blob's format bytes (31
bits -> rate 24, otherwise the number of bits) and hands them over as the table.

  equal           size, all headers, start indices, segment headers, sub-track types, constant translations and scales, every
                  translation and scale byte of clip ranges, segment ranges and streams (on bits: fields are not byte aligned), format
                  bytes, padding, metadata
  reconstructed   what depends on a rotation's normalization (the reference starts from the x86 reciprocal square root estimate,
                  DESIGN.md 8): constant rotation words and the rotations' clip ranges within 1e-5; segment range bytes and bit fields
                  as the component they stand for, ((q / (2^bits - 1)) * segment extent + segment min) * clip extent + clip min, each
                  side with its own ranges, within 1e-5 + one quantization step of that sub-track in that segment (two correct
                  roundings of values an ulp apart may land on neighbouring codes). The worst difference is printed.
  the hash        recomputed over the restatement's own bytes, and through aclhip_check_clip with check_hash

Besides the sweep: clips whose later segments stand still (the reference answers with rate 0), segment minima and maxima on the edges
of fixup_range, clip ranges on a zero of both signs, metadata and a default pose.

Every constant / default / vote decision lies a factor 2 from its precision, asserted from the restatement's record. On these shapes the
reference never chooses rate 24 (it chose 0 to 21; the worst rotation difference seen is 0.919 of its bound, 1.2e-4
absolute: a field on the neighbouring code at a low rate); rate 24 and other tables it cannot produce are covered by the hand-built
tables below, decoded with the oracle's decoder: every key must give exactly the values the restatement dequantizes.

This file holds the DEFINITION to the reference: it runs the numpy restatement, the reference and the existing aclhip_check_clip, and but
for the bound's test it needs no symbol of the new call -- it passes on a library without it. The files that fail without the call are
tests/test_gpu_variable_compress.py and tests/test_variable_compress_arguments.py. No GPU."""
import os
import struct

import numpy as np
import pytest

from acl_amd import runtime
from oracle import bindings as ob
import variable_compress_restatement as restatement
from variable_compress_restatement import ANIMATED, IDENTITY, INV_255, NO_PARENT, OPTIMIZE_LOOPS, RAW_RATE, XYZ

RATE = 32.0
PRECISION, SHELL = 0.01, 3.0
TRACK_COUNTS, SAMPLE_COUNTS = (1, 3, 4, 5, 17, 65), (1, 2, 31, 32, 33, 49, 65)
SHAPES = [(t, s) for t in TRACK_COUNTS for s in SAMPLE_COUNTS]
TOLERANCE = 1.0e-5
worst_seen = [0.0, 0.0]         # in units of the bound; absolute
rates_seen = set()
SEEN_BY_THE_SWEEP = set()


@pytest.fixture(autouse=True)
def reference_compressor():
    """(asked when a test runs: the session's build makes the library)"""
    if not os.path.exists(ob.REF_COMPRESS_PATH):
        pytest.skip("oracle/_ref/libaclref_compress.so not built (it is made from the reference's sources)")


def reference(samples, level, default_pose=None, parents=None, flags=0):
    num_tracks = samples.shape[1]
    default_pose = np.tile(IDENTITY, (num_tracks, 1)) if default_pose is None else default_pose[:num_tracks]
    parents = np.full(num_tracks, NO_PARENT, dtype=np.uint32) if parents is None else parents[:num_tracks]
    names = {"optimize_loops": OPTIMIZE_LOOPS, "include_parent_track_indices": restatement.INCLUDE_PARENT_TRACK_INDICES, "include_track_descriptions": restatement.INCLUDE_TRACK_DESCRIPTIONS}
    switches = {name: True for name, bit in names.items() if flags & bit}
    return np.asarray(ob.ref_compress_ex(samples, RATE, parents=np.asarray(parents, dtype=np.uint32).view(np.int32), bind_pose=default_pose, level=level,
                                         precision=PRECISION, shell_distance=SHELL, **switches)).view(np.uint8)


def field(bits_of_blob, at, width):
    """`width` bits from bit `at`, most significant first"""
    value = 0
    for bit in bits_of_blob[at: at + width]:
        value = (value << 1) | int(bit)
    return value


def rotation_record(blob, c):
    """the rotation dependent content of a blob laid out as the restatement `c` lays its own: (bit mask over the blob, constant words,
    clip ranges {b: (min, extent)}, per (b, g) the segment range as floats (or None) and per (b, g, sample) the three stored codes)"""
    bits = np.unpackbits(blob)
    mask = np.zeros(bits.size, dtype=bool)
    mask[32:64] = True
    constants_at, constant_bytes = c.constant_rotations_at
    mask[8 * constants_at: 8 * (constants_at + constant_bytes)] = True
    constants = blob[constants_at: constants_at + constant_bytes].view("<f4")
    clip_at, clip_bytes = c.clip_rotations_at
    mask[8 * clip_at: 8 * (clip_at + clip_bytes)] = True
    clip_words = blob[clip_at: clip_at + clip_bytes].view("<f4")
    clip_ranges, segment_ranges, codes = {}, {}, {}
    for rank, b in enumerate(c.animated[0]):
        group, place = rank // 4, rank % 4
        group_size = min(4, len(c.animated[0]) - 4 * group)
        rows = clip_words[group * 24: group * 24 + 6 * group_size].reshape(6, group_size)[:, place]
        clip_ranges[b] = (rows[0:3].astype(np.float32), rows[3:6].astype(np.float32))
        for g in range(len(c.segments)):
            if len(c.segments) > 1:
                at = c.segment_range_at[g] + group * 24 + place
                mask[[8 * (at + 4 * row) + bit for row in range(6) for bit in range(8)]] = True
                rows8 = blob[[at + 4 * row for row in range(6)]].astype(np.uint32)
                if c.rates[g, b, 0] == 0:
                    codes[b, g, 0] = np.array([(rows8[0] << 8) | rows8[1], (rows8[2] << 8) | rows8[3], (rows8[4] << 8) | rows8[5]], dtype=np.uint32)
                else:
                    segment_ranges[b, g] = (rows8[0:3].astype(np.float32) * INV_255, rows8[3:6].astype(np.float32) * INV_255)
    for b, g, sample, at, width in c.fields:
        mask[at: at + 3 * width] = True
        codes[b, g, sample] = np.array([field(bits, at + k * width, width) for k in range(3)], dtype=np.uint32)
    return bits, mask, constants, clip_ranges, segment_ranges, codes


def reconstruct(code, rate, clip_range, segment_range):
    """the component a stored code stands for and the quantization step of its sub-track in its segment, in float64"""
    clip_min, clip_extent = (np.asarray(x, dtype=np.float64) for x in clip_range)
    if rate == RAW_RATE:
        return code.view(np.float32).astype(np.float64), np.zeros(3)
    if rate == 0:
        return code.astype(np.float64) / 65535.0 * clip_extent + clip_min, clip_extent / 65535.0
    value, step = code.astype(np.float64) / float((1 << rate) - 1), 1.0 / float((1 << rate) - 1)
    if segment_range is not None:
        value, step = value * segment_range[1].astype(np.float64) + segment_range[0].astype(np.float64), step * segment_range[1].astype(np.float64)
    return value * clip_extent + clip_min, step * clip_extent


def hold(samples, level, **settings):
    """the comparisons of the docstring for one array and one level; returns the restatement's Compressed"""
    theirs = reference(samples, level, **settings)
    rates = restatement.rates_of(theirs)
    c = restatement.compress(samples, RATE, rates, precision=PRECISION, shell_distance=SHELL, **settings)
    assert restatement.decisions_are_clear(c), [d for d in c.decisions if not (d[2] <= 0.5 * d[3] or d[2] >= 2.0 * d[3])]
    blob = c.blob
    assert blob.size == theirs.size, (blob.size, theirs.size)
    assert np.array_equal(restatement.parse(theirs)["types"][: 3 if c.types[2].any() else 2], c.types[: 3 if c.types[2].any() else 2])
    mine, theirs_record = rotation_record(blob, c), rotation_record(theirs, c)
    different = np.flatnonzero((mine[0] != theirs_record[0]) & ~mine[1])
    assert different.size == 0, (different[:8] // 8, blob[different[:8] // 8], theirs[different[:8] // 8])
    assert restatement.bound(*samples.shape[1::-1], settings.get("flags", 0)) >= blob.size

    def close(a, b, bound, what):
        if np.size(a) == 0:
            return
        difference = np.abs(np.asarray(a, dtype=np.float64) - np.asarray(b, dtype=np.float64))
        assert np.isfinite(difference).all()
        worst_seen[0] = max(worst_seen[0], float((difference / bound).max()))
        worst_seen[1] = max(worst_seen[1], float(difference.max()))
        assert (difference <= bound).all(), (what, float(difference.max()), bound)

    close(mine[2], theirs_record[2], TOLERANCE, "constant rotations")
    for b in c.animated[0]:
        close(mine[3][b][0], theirs_record[3][b][0], TOLERANCE, "clip min")
        close(mine[3][b][0].astype(np.float64) + mine[3][b][1], theirs_record[3][b][0].astype(np.float64) + theirs_record[3][b][1], TOLERANCE, "clip max")
        for g in range(len(c.segments)):
            rate = int(c.rates[g, b, 0])
            rates_seen.add(rate)
            if (b, g) in mine[4]:
                step = mine[3][b][1].astype(np.float64) / 255.0
                for part in (0, 1):         # the padded minimum, and the padded maximum, as components
                    ours_value = (mine[4][b, g][0] + part * mine[4][b, g][1]).astype(np.float64) * mine[3][b][1] + mine[3][b][0]
                    their_value = (theirs_record[4][b, g][0] + part * theirs_record[4][b, g][1]).astype(np.float64) * theirs_record[3][b][1] + theirs_record[3][b][0]
                    close(ours_value, their_value, TOLERANCE + step, "segment range")
    for key in mine[5]:
        b, g, _ = key
        rate = int(c.rates[g, b, 0])
        ours_value, step = reconstruct(mine[5][key], rate, mine[3][b], mine[4].get((b, g)))
        their_value, _ = reconstruct(theirs_record[5][key], rate, theirs_record[3][b], theirs_record[4].get((b, g)))
        close(ours_value, their_value, TOLERANCE + step, "rotation field")
    for kind in (1, 2):
        for b in c.animated[kind]:
            rates_seen.update(int(rate) for rate in c.rates[:, b, kind])
    print("worst rotation difference so far: %.3g of its bound, %.3g absolute; rates seen %s" % (worst_seen[0], worst_seen[1], sorted(rates_seen)))
    size, stored_hash = struct.unpack_from("<II", blob.tobytes(), 0)
    assert size == blob.size and stored_hash == restatement.fnv1a32(blob[8:])
    status, message = runtime.check_clip(aligned(blob), check_hash=True)
    assert status == 0, message
    return c


def aligned(blob):
    from acl_amd.synth import aligned_bytes
    out = aligned_bytes(blob.size)
    out[:] = blob
    return out


# ---- the sweep ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("num_tracks,num_samples", SHAPES, ids=["%dx%d" % shape for shape in SHAPES])
def test_the_sweep_is_the_reference(num_tracks, num_samples):
    """random trees; track b of clip k is DEFAULT, CONSTANT or ANIMATED in rotation, translation and scale as the (b + 9 k)-th of the 27
    triples says (variable_compress_restatement.mixed_clip): three clips of 9 tracks and more walk all 27, and every track's types are
    asserted to be the ones it was built for; a fourth clip has no scale; both levels; S = 32 closes its loop and is voted down to one
    segment of 31"""
    seen = set()
    for k in range(4):
        parents = restatement.tree(k, num_tracks)
        close_loop = num_samples == 32
        samples = restatement.mixed_clip(k, num_samples, num_tracks, offset=9 * k, scales="default" if k == 3 else "mixed", close_loop=close_loop)
        c = hold(samples, ("lowest", "medium")[k % 2], parents=parents, flags=OPTIMIZE_LOOPS if close_loop or k == 1 else 0)
        assert not close_loop or (c.wrap and c.segments == [(0, 31)])
        if c.wrap and not close_loop:       # (a clip of one track that stands still closes its loop by itself: one sample less)
            assert k == 1 and c.num_samples == num_samples - 1 and len(c.segments) == {1: 1, 30: 1, 32: 2, 48: 2, 64: 3}[c.num_samples]
        elif not close_loop:
            assert len(c.segments) == {1: 1, 2: 1, 31: 1, 33: 2, 49: 3, 65: 4}[num_samples]
            if num_samples == 33:
                assert c.segments == [(0, 17), (17, 16)]
        if k == 3:
            assert not (c.types[2] != restatement.DEFAULT).any() and not restatement.parse(c.blob)["has_scale"]
        elif num_samples > 1:
            assert [tuple(c.types[:, b]) for b in range(num_tracks)] == [restatement.triple_of(b, 9 * k) for b in range(num_tracks)]
            seen |= restatement.triples_of(c)
    assert len(seen) == (0 if num_samples == 1 else min(27, 3 * num_tracks) if num_tracks < 9 else 27)
    SEEN_BY_THE_SWEEP.update(seen)


def test_the_sweep_saw_all_27_mixes():
    """(behind the sweep in this file: every (rotation, translation, scale) triple was held to the reference, in every shape of 9 tracks
    and more by itself)"""
    if len(SEEN_BY_THE_SWEEP) == 0:
        pytest.skip("the sweep was not run in this session")
    assert len(SEEN_BY_THE_SWEEP) == 27


def half_frozen(seed, num_samples, num_tracks):
    """every sub-track moves in the first 16 samples and stands still behind them: constant in the later segments, animated in the clip"""
    samples = restatement.clip(seed, num_samples, num_tracks)
    rng = np.random.default_rng(seed)
    samples[:, :, 0:4] = restatement.lossy.raw_restatement.unit_quaternions(rng, (num_samples, num_tracks))
    samples[:, :, 4:7] = rng.uniform(-0.5, 0.5, size=(num_samples, num_tracks, 3))
    samples[16:] = samples[16]
    return samples


def test_the_reference_chooses_rate_0_in_a_segment_that_stands_still():
    seen = set()
    for seed, (num_tracks, num_samples) in enumerate(((5, 49), (17, 33), (4, 65))):
        c = hold(half_frozen(seed, num_samples, num_tracks), "medium", parents=restatement.tree(seed, num_tracks))
        for kind in range(3):
            seen |= set(c.rates[1:, c.animated[kind], kind].reshape(-1).tolist())
            assert (c.rates[0, c.animated[kind], kind] != 0).all()
    assert 0 in seen


def test_a_zero_minimum_or_maximum_has_the_sign_of_the_last_zero_sample():
    """rtm::vector_min and vector_max return their second operand on a tie: the clip range words are the reference's, sign bit included"""
    for seed, (num_tracks, num_samples) in enumerate(((3, 12), (5, 40))):
        samples = restatement.signed_zeros(seed, num_samples, num_tracks)
        c = hold(samples, "medium", parents=restatement.tree(seed, num_tracks))
        assert c.types[1, 0] == ANIMATED
        low, extent = c.clip_ranges[1, 0]
        assert low.view(np.uint32).tolist()[0:2] == [0x80000000, 0x00000000] and low[2] < 0 and extent[0] == 0 and extent[2] == -low[2]


def test_segment_ranges_on_the_edges_of_the_fix_up_are_the_reference_s():
    """minima and maxima that are k / 255 in its several float32 spellings, and their neighbours: floor, ceil and both selects of
    fixup_range, as written"""
    for num_tracks in (5, 17):
        samples = restatement.fixup_boundaries(num_tracks)
        c = hold(samples, "medium", parents=restatement.tree(2, num_tracks))
        assert (c.types[1] == ANIMATED).all() and len(c.segments) == 2
        for b in range(num_tracks):
            assert np.array_equal(c.clip_ranges[1, b][0], np.zeros(3, dtype=np.float32)) and np.array_equal(c.clip_ranges[1, b][1], np.ones(3, dtype=np.float32))
        padded = np.array([c.segment_ranges[1, b, 1] for b in range(num_tracks)])              # [T, 2, 3]
        low, high = samples[20:, :, 4:7].min(axis=0), samples[20:, :, 4:7].max(axis=0)
        assert (padded[:, 0] <= low).all() and (padded[:, 0] > low - 2.0 / 255.0).all()
        # (the reference compares the padded extent with the MAXIMUM, not with max - min: away from a minimum of 0 the select takes "one
        # higher" every time; the range is covered, by up to two steps more than it needs)
        assert (padded[:, 0] + padded[:, 1] >= high).all() and (padded[:, 1] <= high - padded[:, 0] + 2.5 / 255.0).all()
        assert (padded[:, 1] > high - padded[:, 0] + 0.5 / 255.0).any()


def test_metadata_and_a_default_pose():
    both = restatement.INCLUDE_PARENT_TRACK_INDICES | restatement.INCLUDE_TRACK_DESCRIPTIONS
    for num_tracks, num_samples in ((5, 33), (17, 9)):
        parents = restatement.tree(5, num_tracks)
        pose = restatement.lossy.raw_restatement.bind_pose(3, num_tracks)
        samples = restatement.clip(1, num_samples, num_tracks, default_pose=pose)
        for flags in (restatement.INCLUDE_PARENT_TRACK_INDICES, both | OPTIMIZE_LOOPS):
            hold(samples, "medium", default_pose=pose, parents=parents, flags=flags)


# ---- tables the reference cannot produce: decoded ----------------------------------------------------------------------------------------------
def decodes_to_its_own_values(c):
    blob = aligned(c.blob)
    status, message = runtime.check_clip(blob, check_hash=True)
    assert status == 0, message
    options = ob.default_options(normalization=ob.NORMALIZE_NEVER)
    for key in range(c.num_samples):
        decoded = ob.oracle_decompress_tracks(blob, key / RATE, ob.ROUND_FLOOR, options=options)
        for lanes in XYZ:
            assert np.array_equal(decoded[:, lanes].view(np.uint32), c.decoded[key][:, lanes].view(np.uint32)), key


@pytest.mark.parametrize("num_tracks,num_samples", [(5, 31), (17, 33), (4, 65), (65, 49)])
def test_hand_built_tables_decode_to_what_the_restatement_dequantizes(num_tracks, num_samples):
    samples = restatement.clip(1, num_samples, num_tracks, scales="default" if num_tracks > 17 else "mixed")
    parents = restatement.tree(1, num_tracks)
    settings = {"parents": parents, "precision": PRECISION, "shell_distance": SHELL}
    segments = restatement.num_segments(num_samples)
    for rate in (1, 3, 8, 19, 23, 24):
        c = restatement.compress(samples, RATE, (rate, rate, rate), **settings)
        assert restatement.bound(num_tracks, num_samples) >= c.blob.size
        decodes_to_its_own_values(c)
    rng = np.random.default_rng(num_tracks)
    mixed = rng.integers(1, 25, size=(segments, num_tracks, 4)).astype(np.uint8)         # per-track and per-segment mixes
    decodes_to_its_own_values(restatement.compress(samples, RATE, mixed, **settings))
    decodes_to_its_own_values(restatement.compress(samples, RATE, mixed[0], **settings))
    if segments > 1:
        mixed[1::2, ::2, 0:3] = 0                                                         # 0 in some segments only
        mixed[0, 1::3, 1] = 0
        c = restatement.compress(samples, RATE, mixed, **settings)
        assert any((c.rates[:, c.animated[kind], kind] == 0).any() for kind in range(3))
        decodes_to_its_own_values(c)
    else:
        with pytest.raises(restatement.Refused):
            restatement.compress(samples, RATE, (0, 8, 8), **settings)
    with pytest.raises(restatement.Refused):
        restatement.compress(samples, RATE, (25, 25, 25), **settings)


def test_the_bound_holds_with_rate_24_everywhere():
    rng = np.random.default_rng(3)
    for num_tracks, num_samples in SHAPES:
        samples = restatement.clip(0, num_samples, num_tracks)
        samples[:, :, 0:4] = restatement.lossy.raw_restatement.unit_quaternions(rng, (num_samples, num_tracks))
        samples[:, :, 4:7] = rng.uniform(-0.5, 0.5, size=(num_samples, num_tracks, 3))
        samples[:, :, 8:11] = rng.uniform(0.9, 1.1, size=(num_samples, num_tracks, 3))
        for flags in (0, restatement.INCLUDE_TRACK_DESCRIPTIONS):
            c = restatement.compress(samples, RATE, (24, 24, 24), flags=flags, precision=1.0e-4, shell_distance=SHELL)
            assert num_samples == 1 or (c.types == ANIMATED).all()
            assert c.blob.size <= restatement.bound(num_tracks, num_samples, flags) == runtime.variable_compress_bound(num_tracks, num_samples, flags)
            assert restatement.bound(num_tracks, num_samples, flags) - c.blob.size < 64 + 16 * len(c.segments) or num_samples == 1
