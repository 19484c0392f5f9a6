"""The restatement of tests/scalar_compress_restatement.py -- the definition aclhip_compress_raw_scalar_tracks_batch is held to by
tests/test_gpu_scalar_compress.py -- against the reference's own compress_track_list (oracle/_ref/libaclref_scalar.so,
aclref_scalar_compress) ON EVERY BYTE, hash included: all five track types, the sweep of shapes and precisions, the looping vote with a
last sample equal to the first, within 5e-5 of it and different, lists whose tracks span constant, every range of rates and raw, and the
values where the reference's operation order shows in the bytes (zeros of both signs as an extreme, extents near 0, values beyond the
start values of the range). No GPU."""
import numpy as np
import pytest

from oracle import bindings as ob
import scalar_compress_restatement as restatement
from scalar_compress_restatement import COMPONENTS, LAST_SAMPLES, PRECISIONS, SWEEP


@pytest.fixture(autouse=True)
def reference_compressor():
    """(asked when a test runs: the session's build makes the library)"""
    if not ob.have_ref_scalar():
        pytest.skip("oracle/_ref/libaclref_scalar.so not built (it is made from the reference's sources)")


RATE = 30.0
TYPES = (ob.TRACK_FLOAT1F, ob.TRACK_FLOAT2F, ob.TRACK_FLOAT3F, ob.TRACK_FLOAT4F, ob.TRACK_VECTOR4F)
TYPE_IDS = ("float1f", "float2f", "float3f", "float4f", "vector4f")


def same_bytes(samples, track_type, precision, optimize_loops=False):
    ours = restatement.compress(samples, track_type, RATE, precision=precision, optimize_loops=optimize_loops)
    theirs = np.asarray(ob.ref_scalar_compress(samples, track_type, RATE, precision=precision, optimize_loops=optimize_loops)).view(np.uint8)
    assert ours.size == theirs.size, (ours.size, theirs.size)
    different = np.flatnonzero(ours != theirs)
    assert different.size == 0, (different[:8], ours[different[:8]], theirs[different[:8]])
    return ours


def curves_of(track_type, num_samples, num_tracks):
    return restatement.curves(7300 + 1000 * track_type + 31 * num_tracks + num_samples, num_samples, num_tracks, COMPONENTS[track_type])


@pytest.mark.parametrize("num_samples,num_tracks", SWEEP, ids=["%dx%d" % shape for shape in SWEEP])
@pytest.mark.parametrize("track_type", TYPES, ids=TYPE_IDS)
def test_the_sweep_is_the_reference_on_every_byte(track_type, num_samples, num_tracks):
    samples = curves_of(track_type, num_samples, num_tracks)
    wrapped = []
    for precision in PRECISIONS:
        same_bytes(samples, track_type, precision)
        for how in LAST_SAMPLES:
            blob = same_bytes(restatement.with_last_sample(samples, how), track_type, precision, optimize_loops=True)
            wrapped.append((precision, how, restatement.parse(blob)["wrap"]))
    if num_samples > 1:
        # equal: always dropped; within 5e-5: dropped at 1e-4 and 1e-2 only
        for precision, how, wrap in wrapped:
            if how == "equal":
                assert wrap
            if how == "near":
                assert wrap == (precision >= 1.0e-4)
    else:
        assert not any(wrap for _, _, wrap in wrapped)


@pytest.mark.parametrize("track_type", TYPES, ids=TYPE_IDS)
def test_a_list_of_many_amplitudes_is_the_reference_on_every_byte(track_type):
    samples = restatement.amplitude_list(COMPONENTS[track_type])
    for precision in PRECISIONS:
        for loops in (False, True):
            same_bytes(samples, track_type, precision, loops)
    rates = restatement.parse(same_bytes(samples, track_type, 1.0e-4))["rates"]
    assert (rates == 0).any() and (rates == 24).any() and rates[rates > 0].min() <= 4 and rates[rates < 24].max() >= 21
    assert len(set(rates.tolist())) >= 10
    # precision 0: nothing is constant, not even the flat tracks, which end at rate 1
    rates = restatement.parse(same_bytes(samples, track_type, 0.0))["rates"]
    assert rates[0] == 1 and rates[12] == 1 and (rates != 0).all()


@pytest.mark.parametrize("track_type", TYPES, ids=TYPE_IDS)
def test_the_special_values_are_the_reference_on_every_byte(track_type):
    """exact low-bit values, an extent near 1e-30, minima and maxima made of +0 and -0, values beyond +-1e10"""
    c = COMPONENTS[track_type]
    samples = restatement.special_list(c)
    for precision in PRECISIONS:
        for loops in (False, True):
            same_bytes(samples, track_type, precision, loops)
    analysis = restatement.analyze(samples, np.zeros(samples.shape[1], dtype=np.float32))
    # the sign of a zero extreme is the LAST zero's; the start values take part
    zeros_low = samples[:, 2, 0][samples[:, 2, 0] == 0]
    assert np.signbit(zeros_low).any() and not np.signbit(zeros_low).all()
    assert np.signbit(analysis["min"][2, 0]) == np.signbit(zeros_low[-1])
    assert analysis["min"][4, 0] == np.float32(1.0e10) and (samples[:, 4] > 1.0e10).all()
    assert (analysis["extent"][5] == np.float32(-1.0e10) - analysis["min"][5]).all() and (samples[:, 5] < -1.0e10).all()
    # both orders of the zeros, so that neither sign can be right by accident
    same_bytes(samples[::-1].copy(), track_type, 0.0)
    flipped = restatement.analyze(samples[::-1].copy(), np.zeros(samples.shape[1], dtype=np.float32))
    assert np.signbit(flipped["min"][2, 0]) == np.signbit(zeros_low[0])


def test_the_search_ends_at_the_first_failing_rate():
    """values 0 .. 7 are exact at 3 bits, but 14 bits fail at 1e-4 before the search gets there: the reference stays at 15"""
    samples = restatement.special_list(1)[:, :1]
    rates = restatement.parse(same_bytes(samples, ob.TRACK_FLOAT1F, 1.0e-4))["rates"]
    assert rates[0] == 15


def test_a_sample_that_is_not_finite_raises_on_both_sides():
    for value in (np.nan, np.inf, -np.inf):
        samples = curves_of(ob.TRACK_FLOAT2F, 9, 4)
        samples[8, 2, 1] = value
        for loops in (False, True):
            with pytest.raises(ValueError, match=restatement.NOT_FINITE_MESSAGE):
                restatement.compress(samples, ob.TRACK_FLOAT2F, RATE, precision=1.0e-4, optimize_loops=loops)
            with pytest.raises(RuntimeError, match=restatement.NOT_FINITE_MESSAGE):
                ob.ref_scalar_compress(samples, ob.TRACK_FLOAT2F, RATE, precision=1.0e-4, optimize_loops=loops)


@pytest.mark.parametrize("track_type", TYPES, ids=TYPE_IDS)
def test_per_track_precisions_are_the_references_single_track_lists(track_type):
    """The bridge takes one precision per list. Without the vote a track's range, constant flag and rate depend on its own samples and
    precision alone: track b of a mixed list equals the reference's list of that one track at p_b."""
    samples = restatement.amplitude_list(COMPONENTS[track_type])
    num_tracks = samples.shape[1]
    table = np.array([1.0e-2, 0.0, 1.0e-5, 1.0e-3, 1.0e-4, 0.5, 3.0e-6] * 3, dtype=np.float32)
    mixed = restatement.parse(restatement.compress(samples, track_type, RATE, track_precisions=table))
    for b in range(num_tracks):
        single = restatement.parse(np.asarray(ob.ref_scalar_compress(samples[:, b:b + 1], track_type, RATE, precision=float(table[b]))).view(np.uint8))
        assert single["rates"][0] == mixed["rates"][b], b
        assert (0 in single["ranges"]) == (b in mixed["ranges"])
        if b in mixed["ranges"]:
            for ours, theirs in zip(mixed["ranges"][b], single["ranges"][0]):
                assert np.array_equal(ours.view(np.uint32), theirs.view(np.uint32))
    assert len(set(mixed["rates"].tolist())) >= 8
