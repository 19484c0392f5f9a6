"""Non-finite STORED samples through every clip decode launch: the poisoned clips of nonfinite_clips.py (a NaN, an infinity, a
float whose square overflows or underflows, -0.0 in a stored animated sample or constant) against the CPU oracle, which
test_nonfinite_samples_oracle.py holds to the reference's own decoder. Needs a GPU.

Every launch alternates the poisoned clip with its clean original over the sample times around the poisoned key frames (about 34
instances) and is compared with nonfinite_clips.same_numbers_and_nans: equal bits where the oracle holds a number, a NaN where it holds a
NaN (NaN sign and payload differ between x86 and the GPU). So that this exemption hides nothing, every case first asserts on
the oracle's values alone that their NaN words lie in the poisoned sub-tracks (object space: in those bones and their descendants), that
every NaN-word poison shows, and that fewer than 5 % of the words are NaNs. The rows of the clean instances are bit identical to a launch
of the clean clip alone. The pose launches write into sentinel filled buffers with a guard row on both sides and rows wider than the pose.

What this file found when it was written: DESIGN 4.4, "non-finite stored samples"."""
import numpy as np
import pytest
import torch

from acl_amd import runtime
from oracle import bindings as ob
import helpers
import nonfinite_clips as nf
from test_gpu_layouts import launch as layout_launch, expected_through_layout, FILL
from test_gpu_bone_object import launch_requests

pytestmark = pytest.mark.gpu

CASES = nf.case_ids()
SENTINEL = np.float32(-7777.25)
PAD_FLOATS = 4
DEVICE = torch.device("cuda", 0)
FAST_TOLERANCE = helpers.FAST_ROTATION_TOLERANCE          # 2e-6, include/aclhip.h (ACLHIP_DECODE_FAST, ACLHIP_CONSUMERS_FAST)


@pytest.fixture(scope="module")
def context():
    ctx = runtime.Context(0)
    yield ctx
    assert ctx.rejected_instance_count() == 0
    ctx.close()


def up(array, dtype):
    array = np.ascontiguousarray(array, dtype=dtype)
    return torch.from_numpy(array.view(np.int32) if dtype == np.uint32 else array).to(DEVICE)


class Batch:
    """the poisoned clip and its clean original registered in `context`, the instances that alternate them over the clip's sample times"""

    def __init__(self, context, case, hierarchy=False, extra_times=()):
        self.context, self.clip = context, nf.poisoned_clip(case)
        self.blobs = [self.clip.blob, self.clip.clean]
        self.handles = [context.register_clip(blob, check_hash=False) for blob in self.blobs]
        if hierarchy:
            for handle in self.handles:
                context.set_clip_hierarchy(handle, self.clip.parents)
        times = np.concatenate([self.clip.times, np.asarray(extra_times, dtype=np.float32)])
        self.times = np.repeat(times, 2).astype(np.float32)
        self.which = np.tile(np.array([0, 1], dtype=np.uint32), times.size)
        self.ids = np.array([self.handles[w] for w in self.which], dtype=np.uint32)
        self.n, self.num_tracks = self.ids.size, self.clip.num_tracks
        self.poisoned = self.which == 0

    def close(self):
        for handle in self.handles:
            self.context.unregister_clip(handle)

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def clean_alone(self):
        """(ids, times) of the clean instances by themselves"""
        return self.ids[~self.poisoned], self.times[~self.poisoned]

    def oracle_tracks(self, rounding=ob.ROUND_NONE, options=None, prefill=None):
        out = None if prefill is None else np.broadcast_to(prefill, (self.n, self.num_tracks, 12)).astype(np.float32).copy()
        return ob.oracle_decompress_tracks_batch(self.blobs, self.which, self.times, self.num_tracks, rounding=rounding, options=options, out=out)


def guarded_launch(n, num_tracks, enqueue, prefill=None):
    """a pose launch into a sentinel filled [n + 2, num_tracks * 12 + PAD_FLOATS] buffer (enqueue(first row's address, stride in bytes)).
    The guard rows and the pad floats keep the sentinel. Returns the poses [n, num_tracks, 12]; prefill: what the pose floats hold before."""
    row_floats = num_tracks * 12 + PAD_FLOATS
    host = np.full((n + 2, row_floats), SENTINEL, dtype=np.float32)
    if prefill is not None:
        host[1:-1, : num_tracks * 12] = np.broadcast_to(prefill, (n, num_tracks, 12)).reshape(n, -1)
    buffer = torch.from_numpy(host).to(DEVICE)
    enqueue(buffer[1].data_ptr(), row_floats * 4)
    torch.cuda.synchronize(DEVICE)
    out = buffer.cpu().numpy()
    sentinel = nf.words(SENTINEL.reshape(1))[0]
    assert (nf.words(out[0]) == sentinel).all() and (nf.words(out[-1]) == sentinel).all(), "a guard row was written"
    assert (nf.words(out[1:-1, num_tracks * 12:]) == sentinel).all(), "the floats behind a pose were written"
    return out[1:-1, : num_tracks * 12].reshape(n, num_tracks, 12).copy()


def decode(context, ids, times, num_tracks, params=None, prefill=None, output=None):
    d_ids, d_times = up(ids, np.uint32), up(times, np.float32)
    stream = torch.cuda.current_stream(DEVICE).cuda_stream

    def enqueue(poses, stride):
        if output is not None:
            context.decompress_tracks_batch_out(d_ids.data_ptr(), d_times.data_ptr(), len(ids), poses, stride, output, params=params, stream=stream)
        else:
            context.decompress_tracks_batch(d_ids.data_ptr(), d_times.data_ptr(), len(ids), poses, stride, params=params, stream=stream)
    return guarded_launch(len(ids), num_tracks, enqueue, prefill)


def consume(context, ids, times, num_tracks, consumers, params=None):
    d_ids, d_times = up(ids, np.uint32), up(times, np.float32)
    stream = torch.cuda.current_stream(DEVICE).cuda_stream
    return guarded_launch(len(ids), num_tracks, lambda poses, stride: context.decompress_poses_batch(d_ids.data_ptr(), d_times.data_ptr(), len(ids), poses, stride, consumers,
                                                                                                    params=params, stream=stream))


def assert_same(got, want, what, never_normalized=False):
    same = nf.same_numbers_and_nans_never_normalized if never_normalized else nf.same_numbers_and_nans
    if not same(got, want):
        if never_normalized:
            free = nf.nan_sign_decided(want)
            got, want = np.where(free, np.float32(0.0), got), np.where(free, np.float32(0.0), want)
        raise AssertionError(f"{what}: {nf.describe_difference(got, want)}")


def assert_clean_rows(batch, got, alone, what):
    assert np.array_equal(nf.words(got[~batch.poisoned]), nf.words(alone)), f"{what}: the clean instances differ from a launch of the clean clip alone"


# ---- default settings -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("settings", [0, 1, 5])
@pytest.mark.parametrize("case", CASES)
def test_decompress_tracks(context, case, settings):
    """settings 0 (the default kernels), 1 (always-normalize and per track rounding: the any-settings kernel), 5 (never normalize) x
    rounding none / nearest / per track (settings 1; floor under the others, which refuse per track rounding); clips of one window and of two"""
    with Batch(context, case) as batch:
        clip = batch.clip
        rng = np.random.default_rng(len(case) + settings)
        track_rounding = rng.integers(0, 4, size=clip.num_tracks).astype(np.uint8)
        d_track_rounding = up(track_rounding, np.uint8)
        never = settings == 5
        # (per track rounding is refused unless the settings enable it: settings 1 does, and then every per track policy is met)
        for rounding in (ob.ROUND_NONE, ob.ROUND_NEAREST, ob.ROUND_PER_TRACK if settings == 1 else ob.ROUND_FLOOR):
            params = helpers.gpu_params(runtime, rounding, settings)
            params.track_rounding_policies = d_track_rounding.data_ptr()
            options = helpers.oracle_options(settings, 0, None, track_rounding)
            want = batch.oracle_tracks(rounding, options)
            nf.check_expectation(clip, want[batch.poisoned], need_every_nan=rounding == ob.ROUND_NONE, never_normalized=never)
            assert not nf.nan_mask(want[~batch.poisoned]).any()
            what = f"{case} settings {settings} rounding {rounding}"
            got = decode(context, batch.ids, batch.times, clip.num_tracks, params)
            assert_same(got, want, what, never_normalized=never)
            assert_clean_rows(batch, got, decode(context, *batch.clean_alone(), clip.num_tracks, params), what)


@pytest.mark.parametrize("case", [case for case in CASES if case.endswith("#0") or case.endswith("#1")])
def test_wrap_policy(context, case):
    """looping policy wrap: the interval behind the last sample interpolates towards the (poisoned) first one"""
    clip = nf.poisoned_clip(case)
    wrap_duration = ob.oracle().aclo_finite_duration(clip.blob.ctypes.data, ob.LOOP_WRAP)
    with Batch(context, case, extra_times=[wrap_duration, (clip.duration + wrap_duration) / 2]) as batch:
        for settings in (0, 1):
            params = helpers.gpu_params(runtime, 0, settings, looping=ob.LOOP_WRAP)
            want = batch.oracle_tracks(options=helpers.oracle_options(settings, looping=ob.LOOP_WRAP))
            nf.check_expectation(clip, want[batch.poisoned])
            got = decode(context, batch.ids, batch.times, clip.num_tracks, params)
            assert_same(got, want, f"{case} wrap, settings {settings}")


# ---- default sub-track modes: the launches that read markers out of the LDS image -------------------------------------------------------------
@pytest.mark.parametrize("default_mode", [0, 1, 2, 3])
@pytest.mark.parametrize("case", CASES)
def test_default_sub_track_modes(context, case, default_mode):
    """0: the track_writer's own (legacy scale), 1: skipped over a sentinel filled buffer -- where the oracle holds the NaN of an ANIMATED
    sub-track the sentinel must not survive --, 2 / 3: the caller's constant / per track values"""
    with Batch(context, case) as batch:
        clip = batch.clip
        rng = np.random.default_rng(default_mode)
        defaults = rng.uniform(-1, 1, size=(clip.num_tracks if default_mode == 3 else 1, 12)).astype(np.float32)
        d_defaults = up(defaults, np.float32)
        prefill = np.full((clip.num_tracks, 12), SENTINEL, dtype=np.float32)
        for settings in (0, 1):
            params = helpers.gpu_params(runtime, 0, settings, default_mode)
            if default_mode in (2, 3):
                params.default_values = d_defaults.data_ptr()
            want = batch.oracle_tracks(options=helpers.oracle_options(settings, default_mode, defaults), prefill=prefill)
            nf.check_expectation(clip, want[batch.poisoned])
            what = f"{case} default mode {default_mode} settings {settings}"
            got = decode(context, batch.ids, batch.times, clip.num_tracks, params, prefill=prefill)
            assert_same(got, want, what)
            assert_clean_rows(batch, got, decode(context, *batch.clean_alone(), clip.num_tracks, params, prefill=prefill), what)


# ---- compact layouts ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", CASES)
def test_compact_layouts(context, case):
    """qvv40 and qv32 with the default settings (the re-tiled stores) and through the default modes skipped / constant / variable with the
    caller's values (resolve_defaults per quad)"""
    with Batch(context, case) as batch:
        clip = batch.clip
        rng = np.random.default_rng(7)
        for default_mode in (0, 1, 2, 3):
            defaults = rng.uniform(-1, 1, size=(clip.num_tracks if default_mode == 3 else 1, 12)).astype(np.float32)
            d_defaults = up(defaults, np.float32)
            params = helpers.gpu_params(runtime, 0, 0, default_mode)
            if default_mode in (2, 3):
                params.default_values = d_defaults.data_ptr()
            want = batch.oracle_tracks(options=helpers.oracle_options(0, default_mode, defaults), prefill=np.full((clip.num_tracks, 12), FILL, dtype=np.float32))
            nf.check_expectation(clip, want[batch.poisoned])
            for layout in ("qvv40", "qv32"):
                what = f"{case} {layout}, default mode {default_mode}"
                got = layout_launch(context, batch.ids, batch.times, layout, max_tracks=clip.num_tracks, params=params)
                assert_same(got, expected_through_layout(want, layout, (0, 0, 0)), what)
                alone = layout_launch(context, *batch.clean_alone(), layout, max_tracks=clip.num_tracks, params=params)
                assert_clean_rows(batch, got, alone, what)


# ---- the bind pose default mode -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", [case for case in CASES if case.rsplit("#", 1)[0] in nf.CORPUS_SOURCES])
def test_bind_pose_default_mode(context, case):
    """ACLHIP_DEFAULT_BIND_POSE on the corpus clips: default sub-tracks take track_desc_transformf::default_value from the blob's metadata
    (the identity where the blob has none) == the oracle's variable mode over that table. QVV48 and one compact layout, both settings."""
    with Batch(context, case) as batch:
        clip = batch.clip
        spec = next(c["spec"] for c in helpers.load_corpus() if c["name"] == case.rsplit("#", 1)[0])
        if spec.get("include_track_descriptions"):
            table, _, _ = context.clip_track_descriptions(batch.handles[1])
            table = np.ascontiguousarray(table, dtype=np.float32)
        else:
            table = np.tile(np.array([0, 0, 0, 1, 0, 0, 0, 0, 1, 1, 1, 0], dtype=np.float32), (clip.num_tracks, 1))
        bind = runtime.DEFAULT_BIND_POSE
        prefill = np.full((clip.num_tracks, 12), SENTINEL, dtype=np.float32)
        for settings in (0, 1):
            normalization, per_track = helpers.settings_pair(settings)
            params = runtime.default_params(default_rotation_mode=bind, default_translation_mode=bind, default_scale_mode=bind, normalization=normalization,
                                            per_track_rounding=per_track)
            want = batch.oracle_tracks(options=helpers.oracle_options(settings, 3, table), prefill=prefill)
            nf.check_expectation(clip, want[batch.poisoned])
            what = f"{case} bind pose, settings {settings}"
            got = decode(context, batch.ids, batch.times, clip.num_tracks, params, prefill=prefill)
            assert_same(got, want, what)
            assert_clean_rows(batch, got, decode(context, *batch.clean_alone(), clip.num_tracks, params, prefill=prefill), what)
            compact = layout_launch(context, batch.ids, batch.times, "qvv40", max_tracks=clip.num_tracks, params=params)
            through = batch.oracle_tracks(options=helpers.oracle_options(settings, 3, table), prefill=np.full((clip.num_tracks, 12), FILL, dtype=np.float32))
            assert_same(compact, expected_through_layout(through, "qvv40", (0, 0, 0)), what + ", qvv40")


# ---- single tracks --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", CASES)
def test_single_tracks(context, case):
    """decompress_track for every poisoned track and its two neighbours at every time: the oracle's decompress_track and the row of
    the whole-pose launch"""
    with Batch(context, case) as batch:
        clip = batch.clip
        tracks = np.array(sorted({t for p in clip.tracks for t in (p - 1, p, p + 1) if 0 <= t < clip.num_tracks}), dtype=np.uint32)
        ids, times, which = np.repeat(batch.ids, tracks.size), np.repeat(batch.times, tracks.size), np.repeat(batch.which, tracks.size)
        track_of = np.tile(tracks, batch.n)
        for settings in (0, 1):
            params = helpers.gpu_params(runtime, 0, settings)
            options = helpers.oracle_options(settings)
            whole = decode(context, batch.ids, batch.times, clip.num_tracks, helpers.gpu_params(runtime, 0, settings)) if settings == 0 else None
            got = context.decompress_track(ids, times, track_of, params=params)
            want = np.stack([ob.oracle_decompress_track(batch.blobs[w], float(t), int(track), options=options) for w, t, track in zip(which, times, track_of)])
            assert_same(got, want, f"{case} settings {settings}")
            if settings == 0:
                # (under always-normalize decompress_track and decompress_tracks normalize in different places, in the reference as here:
                # only the default settings' single track is the whole pose's row)
                rows = whole[np.repeat(np.arange(batch.n), tracks.size), track_of]
                assert np.array_equal(nf.nan_mask(got), nf.nan_mask(rows)), f"{case}: NaNs of the whole pose"
                assert_same(got, rows, f"{case}: against the whole pose")


# ---- track maps -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", CASES)
def test_mapped_decode(context, case):
    """the decode through a permuting track map with dropped tracks, unmapped slots and a fill pose"""
    with Batch(context, case) as batch:
        clip = batch.clip
        rng = np.random.default_rng(len(case))
        num_slots = clip.num_tracks + 5
        slots = rng.permutation(num_slots)[: clip.num_tracks].astype(np.uint32)
        clean_tracks = np.array([t for t in range(clip.num_tracks) if t not in clip.tracks])
        slots[rng.choice(clean_tracks, size=3, replace=False)] = runtime.TRACK_DROPPED           # (every poisoned track stays mapped)
        track_map = context.register_track_map(slots, num_slots)
        fill = rng.uniform(-2, 2, size=(num_slots, 12)).astype(np.float32)
        d_fill = up(fill, np.float32)
        stream = torch.cuda.current_stream(DEVICE).cuda_stream

        def launch_mapped(ids, times):
            d_ids, d_times = up(ids, np.uint32), up(times, np.float32)
            return guarded_launch(len(ids), num_slots, lambda poses, stride: context.decompress_tracks_batch_mapped_at(
                d_ids.data_ptr(), d_times.data_ptr(), len(ids), poses, stride, track_map=track_map, fill_pose_ptr=d_fill.data_ptr(), stream=stream))
        got = launch_mapped(batch.ids, batch.times)
        decoded = batch.oracle_tracks()
        nf.check_expectation(clip, decoded[batch.poisoned])
        want = np.broadcast_to(fill, (batch.n, num_slots, 12)).copy()
        mapped = slots != runtime.TRACK_DROPPED
        want[:, slots[mapped]] = decoded[:, mapped]
        assert_same(got, want, f"{case} mapped")
        assert_clean_rows(batch, got, launch_mapped(*batch.clean_alone()), f"{case} mapped")
        context.unregister_track_map(track_map)


# ---- consumers ------------------------------------------------------------------------------------------------------------------------------
def oracle_consumers(batch, additive_format=0, object_space=False, base_which=None, base_times=None):
    return ob.oracle_decompress_poses_batch(batch.blobs, batch.which, batch.times, batch.num_tracks, additive_format=additive_format, base_clip_indices=base_which,
                                            base_sample_times=base_times, parent_indices=batch.clip.parents if object_space else None)


@pytest.mark.parametrize("case", CASES)
def test_object_space(context, case):
    with Batch(context, case, hierarchy=True) as batch:
        clip = batch.clip
        consumers = runtime.PoseConsumers()
        consumers.object_space = 1
        want = oracle_consumers(batch, object_space=True)
        nf.check_expectation(clip, want[batch.poisoned], object_space=True)
        assert not nf.nan_mask(want[~batch.poisoned]).any()
        got = consume(context, batch.ids, batch.times, clip.num_tracks, consumers)
        assert_same(got, want, f"{case} object space")
        assert_clean_rows(batch, got, consume(context, *batch.clean_alone(), clip.num_tracks, consumers), f"{case} object space")


def assert_fast(fast, exact, what, below=None):
    """NaN masks and infinities equal the bit exact kernel's; rotations within 2e-6 where both are numbers. below (object space: the bones
    that are poisoned or hang under one): translations and scales within 2e-6 of the pose's extent, which for the OTHER bones is taken
    over those bones alone (a stored 0x7F7FFFFF must not widen the bound for everyone).
    Without `below` (ACLHIP_DECODE_FAST) translations and scales are equal on bits."""
    assert np.array_equal(nf.nan_mask(fast), nf.nan_mask(exact)), f"{what}: NaN masks differ at {np.argwhere(nf.nan_mask(fast) != nf.nan_mask(exact))[:6].tolist()}"
    finite = np.isfinite(exact) & np.isfinite(fast)
    assert np.array_equal(np.isinf(fast), np.isinf(exact)), f"{what}: infinities differ"
    difference = np.where(finite, np.abs(np.where(finite, fast, 0).astype(np.float64) - np.where(finite, exact, 0)), 0.0)
    assert difference[..., 0:4].max() <= FAST_TOLERANCE, f"{what}: rotations differ by {difference[..., 0:4].max()}"
    if below is None:
        assert np.array_equal(nf.words(fast[..., helpers.FAST_VECTOR_LANES]), nf.words(exact[..., helpers.FAST_VECTOR_LANES])), f"{what}: translations / scales moved"
        return
    size = np.where(finite, np.abs(exact), 0.0).astype(np.float64)
    for lanes, name in ((slice(4, 7), "translations"), (slice(8, 11), "scales")):
        # per pose: the extent of the bones no poison reaches bounds them; a bone below a poison keeps the documented bound, the extent of
        # its whole pose, poisoned values included
        clean_extent = np.maximum(1.0, size[:, ~below, lanes].max(axis=(1, 2), initial=0.0))
        whole_extent = np.maximum(1.0, size[..., lanes].max(axis=(1, 2), initial=0.0))
        bound = np.empty(size[..., lanes].shape)
        bound[...] = FAST_TOLERANCE * clean_extent[:, None, None]
        bound[:, below] = FAST_TOLERANCE * whole_extent[:, None, None]
        worst = (difference[..., lanes] - bound).max()
        assert worst <= 0.0, f"{what}: {name} differ by {worst} more than 2e-6 of the pose's extent"


@pytest.mark.parametrize("additive_format", [1, 2, 3])
@pytest.mark.parametrize("case", CASES)
def test_additive(context, case, additive_format):
    """the base of instance i is the OTHER clip of the pair: the poisoned clip is the additive clip in half of the instances and the base in
    the other half; local space and object space"""
    with Batch(context, case, hierarchy=True) as batch:
        clip = batch.clip
        base_which = (1 - batch.which).astype(np.uint32)
        base_times = batch.times[::-1].copy()
        d_base = up(np.array([batch.handles[w] for w in base_which], dtype=np.uint32), np.uint32)
        d_base_times = up(base_times, np.float32)
        for object_space in (False, True):
            consumers = runtime.PoseConsumers()
            consumers.additive_format, consumers.object_space = additive_format, int(object_space)
            consumers.base_clips, consumers.base_sample_times = d_base.data_ptr(), d_base_times.data_ptr()
            want = oracle_consumers(batch, additive_format, object_space, base_which, base_times)
            nf.check_expectation(clip, want, object_space=True, need_every_nan=False)       # (NaNs stay within the poisoned bones and what hangs below them)
            got = consume(context, batch.ids, batch.times, clip.num_tracks, consumers)
            assert_same(got, want, f"{case} additive format {additive_format} object space {object_space}")


@pytest.mark.parametrize("case", CASES)
def test_blend_of_two_clips(context, case):
    """a two clip blend with the poisoned clip first (even instances) and second (odd instances)"""
    with Batch(context, case, hierarchy=True) as batch:
        clip = batch.clip
        rng = np.random.default_rng(len(case))
        other = (1 - batch.which).astype(np.uint32).reshape(-1, 1)
        other_times = batch.times[::-1].copy().reshape(-1, 1)
        weights = rng.uniform(0.2, 0.8, size=(batch.n, 2)).astype(np.float32)
        d_other = up(np.array([batch.handles[w] for w in other[:, 0]], dtype=np.uint32), np.uint32)
        d_other_times, d_weights = up(other_times, np.float32), up(weights, np.float32)
        for object_space in (False, True):
            consumers = runtime.PoseConsumers()
            consumers.object_space, consumers.num_blend_clips = int(object_space), 2
            consumers.blend_clips, consumers.blend_sample_times, consumers.blend_weights = d_other.data_ptr(), d_other_times.data_ptr(), d_weights.data_ptr()
            want = ob.oracle_decompress_blended_poses_batch(batch.blobs, batch.which, batch.times, other, other_times, weights, clip.num_tracks,
                                                            parent_indices=clip.parents if object_space else None)
            nf.check_expectation(clip, want, object_space=True, need_every_nan=False)
            got = consume(context, batch.ids, batch.times, clip.num_tracks, consumers)
            assert_same(got, want, f"{case} blend, object space {object_space}")


# ---- one case each ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["025_raw_33x33#1", "synthetic_140#0"])
def test_object_space_single_bone_requests(context, case):
    """a poisoned bone, a bone of the small subtree below one, and a clean bone"""
    with Batch(context, case, hierarchy=True) as batch:
        clip = batch.clip
        below = np.flatnonzero(clip.descendants())
        bones = sorted(set(below.tolist()) | {int(np.flatnonzero(~clip.descendants())[0])})
        assert len(below) > len(clip.tracks)                                          # (someone hangs below a poisoned bone)
        ids, times, which = np.repeat(batch.ids, len(bones)), np.repeat(batch.times, len(bones)), np.repeat(batch.which, len(bones))
        bone_of = np.tile(np.array(bones, dtype=np.uint32), batch.n)
        want = oracle_consumers(batch, object_space=True)
        nf.check_expectation(clip, want[batch.poisoned], object_space=True)
        got = launch_requests(context, ids, times, bone_of)
        assert_same(got, want[np.repeat(np.arange(batch.n), len(bones)), bone_of], f"{case} single bone requests")


def test_all_samples_of_the_small_poisoned_clip(context):
    clip = nf.poisoned_clip("025_raw_33x33#2")
    handle = context.register_clip(clip.blob, check_hash=False)
    info = context.clip_info(handle)
    scratch = torch.zeros(2 * info.num_samples, dtype=torch.int32, device=DEVICE)
    stream = torch.cuda.current_stream(DEVICE).cuda_stream
    got = guarded_launch(info.num_samples, info.num_tracks, lambda poses, stride: context.decompress_all_samples(handle, scratch.data_ptr(), poses, stride, stream=stream))
    times = np.minimum(np.arange(info.num_samples, dtype=np.float32) / np.float32(info.sample_rate), np.float32(info.duration)).astype(np.float32)
    want = np.stack([ob.oracle_decompress_tracks(clip.blob, float(t), ob.ROUND_NEAREST) for t in times])
    nf.check_expectation(clip, want)
    assert_same(got, want, "all samples")
    context.unregister_clip(handle)


@pytest.mark.parametrize("case", ["025_raw_33x33#3", "151_bones_105_raw#0"])
def test_skeleton_space(context, case):
    """the skeleton space launch over a registered skeleton and an identity track map: object space poses in skeleton order"""
    with Batch(context, case) as batch:
        clip = batch.clip
        reference_pose = np.zeros((clip.num_tracks, 12), dtype=np.float32)
        reference_pose[:, 3] = 1.0
        reference_pose[:, 8:11] = 1.0
        skeleton = context.register_skeleton(clip.parents, reference_pose)
        track_map = context.register_track_map(np.arange(clip.num_tracks, dtype=np.uint32), clip.num_tracks)
        got = context.decompress_poses_mapped(batch.ids, batch.times, skeleton, track_map, clip.num_tracks, object_space=True)
        want = oracle_consumers(batch, object_space=True)
        nf.check_expectation(clip, want[batch.poisoned], object_space=True)
        assert_same(got, want, f"{case} skeleton space")
        context.unregister_track_map(track_map)
        context.unregister_skeleton(skeleton)


# ---- opt-in fast arithmetic ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("base", ["none", "relative_clip", "additive0_clip", "additive1_clip", "additive0_buffer"])
@pytest.mark.parametrize("case", CASES)
def test_consumers_fast(context, case, base):
    """ACLHIP_CONSUMERS_FAST in object space: the NaN masks of the bit exact kernels, numbers within the 2e-6 include/aclhip.h states, for
    every way a fast kernel gets its local pose: no base, a base clip decoded by a second wave (relative), a base clip under the
    instance's own wave (additive0 / additive1), the caller's base poses. The base is the OTHER clip of the pair, so the poisoned clip
    is the additive clip in half of the instances and the base in the other half.

    Stored INFINITIES are what this holds (without a base 12 of 32 cases missed it when the test was written, 2 to 15 words each, every one
    on a bone whose poison is 0x7F800000 or 0xFF800000 in a translation, a scale or the x / y / z of a drop-W rotation): the fast kernels
    interpolated as fma(end, alpha, start * (1 - alpha)) and walk with two cross products, forms that reach inf - inf and 0 * inf in other
    places than the bit exact ones. They now interpolate in the stable form, fused (lerp_stable_fast), and a workgroup whose local poses
    hold a value that is not finite combines and walks with the bit exact forms (finish_consumer_poses)."""
    with Batch(context, case, hierarchy=True) as batch:
        consumers = runtime.PoseConsumers()
        consumers.object_space = 1
        keep = []
        if base != "none":
            consumers.additive_format = {"relative": 1, "additive0": 2, "additive1": 3}[base.split("_")[0]]
            base_which = (1 - batch.which).astype(np.uint32)
            base_times = batch.times[::-1].copy()
            if base.endswith("_clip"):
                keep += [up(np.array([batch.handles[w] for w in base_which], dtype=np.uint32), np.uint32), up(base_times, np.float32)]
                consumers.base_clips, consumers.base_sample_times = keep[0].data_ptr(), keep[1].data_ptr()
            else:
                poses = ob.oracle_decompress_tracks_batch(batch.blobs, base_which, base_times, batch.num_tracks)
                keep.append(up(poses, np.float32))
                consumers.base_poses, consumers.base_pose_stride_bytes = keep[0].data_ptr(), batch.num_tracks * 48
        exact = consume(context, batch.ids, batch.times, batch.num_tracks, consumers)
        consumers.flags = runtime.CONSUMERS_FAST
        fast = consume(context, batch.ids, batch.times, batch.num_tracks, consumers)
        assert nf.nan_mask(exact).any()
        assert_fast(fast, exact, f"{case} object space, base {base}, fast", below=batch.clip.descendants())


@pytest.mark.parametrize("case", CASES)
def test_decode_fast(context, case):
    """ACLHIP_DECODE_FAST: the NaN masks of the bit exact kernels, rotations within 2e-6, translations and scales on bits"""
    with Batch(context, case) as batch:
        for rounding in (ob.ROUND_NONE, ob.ROUND_NEAREST):
            exact = decode(context, batch.ids, batch.times, batch.num_tracks, runtime.default_params(rounding_policy=rounding))
            fast = decode(context, batch.ids, batch.times, batch.num_tracks, runtime.default_params(rounding_policy=rounding, flags=runtime.DECODE_FAST))
            assert_fast(fast, exact, f"{case} rounding {rounding}")
