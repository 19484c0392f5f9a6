"""runtime.raw_clip_error: acl::calculate_compression_error(raw_tracks, context, error_metric, additive_base_tracks)
(compression/impl/track_error.impl.h:581-689, loop :319-376) as launches -- the raw track array sampled, the clip decoded, an additive base
sampled at its own duration, the two buffers measured. The expectation is that loop on the host: the restatement's raw poses
(tests/test_raw_tracks_oracle.py), the oracle's decode, and the measure restatements of tests/test_pose_error_oracle.py and
tests/test_pose_matrices_oracle.py; the bone, the error's bits and the sample time all agree. The raw clip is a synthetic 20 bone x 40
sample clip with scale; its compressed form is the reference compressor's where that library is built, and a synthetic clip of the same
shape -- which differs from the raw data by construction -- everywhere. Needs a GPU."""
import numpy as np
import pytest

from acl_amd import runtime, synth
from oracle import bindings as ob
from test_gpu_pose_buffers import bits, identity_pose
from test_pose_error_oracle import expected_measure, scan_worst
from test_pose_matrices_oracle import expected_matrix_measure
from test_raw_tracks_oracle import CLAMP, NEAREST, NONE, finite_duration, sample_tracks

pytestmark = pytest.mark.gpu

BONES, SAMPLES, RATE = 20, 40, 30.0
ADDITIVE1 = runtime.ADDITIVE_ADDITIVE1


def smooth_clip(rng, num_samples, num_bones):
    """a clip that moves a little from key frame to key frame: rotations near a per bone rest rotation, translations and scales that drift"""
    clip = np.zeros((num_samples, num_bones, 12), dtype=np.float32)
    rest = rng.normal(size=(1, num_bones, 4))
    rotations = rest + np.cumsum(rng.normal(scale=0.03, size=(num_samples, num_bones, 4)), axis=0)
    clip[..., 0:4] = rotations / np.linalg.norm(rotations, axis=2, keepdims=True)
    clip[..., 4:7] = rng.uniform(-1.0, 1.0, size=(1, num_bones, 3)) + np.cumsum(rng.normal(scale=0.01, size=(num_samples, num_bones, 3)), axis=0)
    clip[..., 8:11] = 1.0 + np.cumsum(rng.normal(scale=0.004, size=(num_samples, num_bones, 3)), axis=0)
    return clip


@pytest.fixture(scope="module")
def case():
    rng = np.random.default_rng(7701)
    raw = smooth_clip(rng, SAMPLES, BONES)
    skeleton_parents = np.array(synth.humanoid_hierarchy(BONES), dtype=np.uint32)        # a spine of eight and twelve bones on the head
    parents = skeleton_parents.astype(np.int64)
    parents[skeleton_parents == runtime.NO_PARENT] = -1
    blobs = {"synth": synth.build_clip(seed=771, num_tracks=BONES, num_samples=SAMPLES, sample_rate=RATE, has_scale=1).blob}
    if ob.have_ref_compressor():
        blobs["compressed"] = ob.ref_compress(raw, RATE, parents=parents.astype(np.int32))
    bases = {7: smooth_clip(rng, 7, BONES), 1: smooth_clip(rng, 1, BONES)}
    shells = np.linspace(0.5, 3.0, BONES).astype(np.float32)
    return raw, skeleton_parents, blobs, bases, shells


def host_loop(raw, blob, parents, shells, rounding, object_space=True, metric=runtime.ERROR_METRIC_QVVF, base=None, base_rate=None, additive_format=runtime.ADDITIVE_NONE):
    """track_error.impl.h:319-376 over the restatements: (bone, error, sample_time)"""
    duration = finite_duration(raw.shape[0], RATE, CLAMP)
    sample_times = np.minimum(np.arange(raw.shape[0], dtype=np.float32) / np.float32(RATE), duration).astype(np.float32)
    records = []
    for t in sample_times:
        raw_pose = sample_tracks(raw, RATE, CLAMP, float(t), rounding)
        lossy_pose = ob.oracle_decompress_tracks(blob, float(t), rounding)
        if metric == runtime.ERROR_METRIC_QVVF_MATRIX3X4F:
            records.append(expected_matrix_measure(parents, raw_pose, lossy_pose, shells, object_space)[1])
            continue
        base_pose = None
        if base is not None:
            # :340-342: the base is sampled at the same share of its own duration, or at 0 when it has one sample
            base_duration = finite_duration(base.shape[0], base_rate, CLAMP)
            base_time = (np.float32(t) / duration) * base_duration if base.shape[0] > 1 else np.float32(0.0)
            base_pose = sample_tracks(base, base_rate, CLAMP, float(base_time), rounding)
        records.append(expected_measure(parents, raw_pose, lossy_pose, shells, object_space, additive_format, base_pose)[1])
    error, bone, instance = scan_worst(records)
    return bone, error, float(sample_times[instance])


def same(got, want):
    return got[0] == want[0] and bits(np.float32(got[1])) == bits(want[1]) and got[2] == want[2]


@pytest.mark.parametrize("source", ["compressed", "synth"])
def test_raw_clip_error_is_the_host_loop(case, source):
    raw, parents, blobs, bases, shells = case
    if source not in blobs:
        pytest.skip("the reference's compressor library is not built")
    blob = blobs[source]
    with runtime.Context(0) as ctx:
        raw_handle = ctx.register_raw_tracks(raw, RATE)
        clip = ctx.register_clip(blob)
        skeleton = ctx.register_skeleton(parents, identity_pose(BONES))
        info = ctx.clip_info(clip)
        assert (info.num_tracks, info.num_samples) == (BONES, SAMPLES) and not info.has_database and not info.has_stripped_keyframes

        # both metrics, with the reference's choice of rounding (nearest: the clip is whole), in object and in local space
        for metric in (runtime.ERROR_METRIC_QVVF, runtime.ERROR_METRIC_QVVF_MATRIX3X4F):
            for object_space in (True, False):
                want = host_loop(raw, blob, parents, shells, NEAREST, object_space, metric)
                got = runtime.raw_clip_error(ctx, raw_handle, clip, skeleton, shells, object_space=object_space, metric=metric)
                assert same(got, want), (metric, object_space, got, want)
                assert want[1] > 0.0
        # the rounding argument reaches both sides
        want = host_loop(raw, blob, parents, shells, NONE)
        assert same(runtime.raw_clip_error(ctx, raw_handle, clip, skeleton, shells, rounding=runtime.ROUND_NONE), want)
        # one shell distance for every bone
        want = host_loop(raw, blob, parents, 2.0, NEAREST)
        assert same(runtime.raw_clip_error(ctx, raw_handle, clip, skeleton, 2.0), want)

        # an additive base of another length and rate (7 samples, additive1), and a base of one sample: sampled at 0
        for base_samples, base_rate in ((7, 12.0), (1, 30.0)):
            base_handle = ctx.register_raw_tracks(bases[base_samples], base_rate)
            want = host_loop(raw, blob, parents, shells, NEAREST, base=bases[base_samples], base_rate=base_rate, additive_format=ADDITIVE1)
            got = runtime.raw_clip_error(ctx, raw_handle, clip, skeleton, shells, additive_base=base_handle, additive_format=ADDITIVE1)
            assert same(got, want), (base_samples, got, want)
        # the matrix metric takes no additive base: the measure refuses it
        with pytest.raises(runtime.AclHipError):
            runtime.raw_clip_error(ctx, raw_handle, clip, skeleton, shells, metric=runtime.ERROR_METRIC_QVVF_MATRIX3X4F, additive_base=base_handle, additive_format=ADDITIVE1)
        assert ctx.rejected_instance_count() == 0
