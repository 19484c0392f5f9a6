"""What aclhip_compress_tracks_additive_batch, aclhip_compress_tracks_variable_additive_batch and aclhip_find_bit_rates_additive_batch
compute: the existing restatements -- tests/lossy_rotation_compress_restatement.py, tests/variable_compress_restatement.py,
tests/bit_rate_search_restatement.py and tests/bit_rate_search_levels_restatement.py -- with an additive base. Nothing of them is
copied: while a call with a base of a format other than NONE runs, their shell and their error functions are replaced, and put back
behind it,

  rigid_shell   step 2 and S0: the restatements' own walk over A(sample) in the place of the sample
  shell_error   the looping vote: A_first(first) against A_last(last), the base's sample 0 and its LAST sample; the compaction of
                constant and default sub-tracks: both sides through A with the sample's base(b, s)
  error_of      S2's local error, and the object error of a root: both sides through A (or its _no_scale twin), the base normalized
                once more
  to_object     S2 down the chain: the local transform of a link goes through A before it is multiplied onto its parent
  the header    the default-scale bit is 0 under ADDITIVE1

What is new is stated here once, in numpy float32 element operations (single, correctly rounded IEEE operations): base(b, s) with its
nearest key, A and its _no_scale twin, the base's refusals and its finite test.

HOW THE REPLACED FUNCTIONS KNOW THE TRACK AND THE SAMPLES. The restatements' functions are handed transforms, not where they come
from. Every call of them is made from a loop over the tracks whose variable is `b`, and in the search from a loop over the segments
whose variables are `start` and `count`: the replaced functions read those from the frames of their callers (sys._getframe), by
name. That is the one thing this module knows of the other restatements' text; a restatement that renames them fails here loudly
(KeyError), never silently.

A transform is the restatements' (rotation [..., 4], translation [..., 3], scale [..., 3]). A helper, not a test file:
tests/test_additive_compress_oracle.py holds it to the reference's compressor with the base, tests/test_gpu_additive_compress.py
holds the kernels to it on every byte."""
import contextlib
import sys

import numpy as np

import bit_rate_search_levels_restatement as levels
import bit_rate_search_restatement as search
import lossy_rotation_compress_restatement as lossy
import variable_compress_restatement as variable
from lossy_rotation_compress_restatement import F32, Refused, f32
from transform_compress_restatement import LANES, NOT_FINITE_MESSAGE

NONE, RELATIVE, ADDITIVE0, ADDITIVE1 = 0, 1, 2, 3       # acl::additive_clip_format8
ONES = np.ones(3, dtype=np.float32)


def finite_duration(num_samples, sample_rate, looping_wrap=False):
    """calculate_finite_duration of an array as it is registered: a wrapping one counts its first sample once more at the end"""
    count = num_samples + (1 if looping_wrap and num_samples else 0)
    return F32(0.0) if count <= 1 else F32(F32(count - 1) / F32(sample_rate))


class Base:
    """An additive base: samples float32 [S_b, T_b, 12] QVV48 as registered, its own sample rate, the format. Holds the samples with
    their rotations normalized once (step 1: the base goes through the same initialize_clip_context; never made of positive w)."""

    def __init__(self, samples, sample_rate, additive_format, looping_wrap=False):
        if additive_format not in (NONE, RELATIVE, ADDITIVE0, ADDITIVE1):
            raise ValueError("unknown additive format %r" % (additive_format,))
        self.format = additive_format
        self.sample_rate = F32(sample_rate)
        self.samples = f32(samples).copy()
        self.samples[:, :, 0:4] = lossy.normalize(self.samples[:, :, 0:4])
        self.num_samples, self.num_tracks = self.samples.shape[0], self.samples.shape[1]
        self.duration = finite_duration(self.num_samples, sample_rate, looping_wrap)

    def finite(self):
        """every used lane of every track and sample, the rotation as normalized"""
        return bool(np.isfinite(np.concatenate([self.samples[:, :, lanes] for lanes in LANES], axis=2)).all())


class _Clip:
    """what base(b, s) needs of the instance, as registered"""

    def __init__(self, num_samples, sample_rate, looping_wrap):
        self.sample_rate = F32(sample_rate)
        self.duration = finite_duration(num_samples, sample_rate, looping_wrap)


def base_keys(base, clip, sample_indices):
    """the base's key that goes with each sample index of the clip: get_uniform_sample_key (sample_streams.h:557-601) at
    ((min(s / rate, D) / D) * D_b) * rate_b -- nearest, never looping, never interpolated; with S = 1 the time is 0 / 0 and the key is
    min(1, S_b - 1) (include/aclhip.h says why)"""
    indices = np.asarray(sample_indices)
    if base.num_samples <= 1:
        return np.zeros(indices.shape, dtype=np.int64)
    last = base.num_samples - 1
    with np.errstate(all="ignore"):
        time = f32(indices.astype(np.float32) / clip.sample_rate)
        time = f32(np.where(time < clip.duration, time, clip.duration))
        x = f32(f32(f32(time / clip.duration) * base.duration) * base.sample_rate)
        is_nan = x != x
        key0 = np.minimum(np.where(is_nan, F32(0.0), x).astype(np.int64), last)
        key1 = np.minimum(key0 + 1, last)
        alpha = np.floor(f32(f32(x - key0.astype(np.float32)) + F32(0.5)))
    return np.where(is_nan, min(1, last), np.where(alpha == F32(0.0), key0, key1))


def base_at(base, b, keys, twice=False):
    """base(b, s) at keys: (rotation [n, 4], translation [n, 3], scale [n, 3]); twice: the rotation normalized once more (S2:
    sample_streams.h:611-625 normalizes what it reads)"""
    rows = base.samples[keys, b]
    rotation = rows[..., 0:4]
    return (lossy.normalize(rotation) if twice else rotation), rows[..., 4:7], rows[..., 8:11]


def apply_additive(additive_format, base_transform, transform, has_scale=True):
    """A(x) = apply_additive_to_base(format, base, x), or apply_additive_to_base_no_scale (core/additive_utils.h:128-174); relative is
    the quaternion route of qvv_mul / qvv_mul_no_scale"""
    base_rotation, base_translation, base_scale = (f32(part) for part in base_transform)
    rotation, translation, scale = (f32(part) for part in transform)
    with np.errstate(invalid="ignore", over="ignore"):
        out_rotation = lossy.quat_mul(rotation, base_rotation)
        if additive_format == RELATIVE:
            out_translation = f32(lossy.mul_point3(translation, base_rotation, base_translation, base_scale if has_scale else ONES))
        else:
            out_translation = f32(translation + base_translation)
        if not has_scale:
            out_scale = np.broadcast_to(ONES, out_translation.shape)
        elif additive_format == ADDITIVE1:
            out_scale = f32(f32(F32(1.0) + scale) * base_scale)
        else:
            out_scale = f32(scale * base_scale)
    return out_rotation, out_translation, out_scale


def _frame_with(name, function_names, depth=2):
    """the nearest caller's frame, from `depth` up, that runs one of `function_names` and has the local `name`"""
    frame = sys._getframe(depth)
    while frame is not None:
        if frame.f_code.co_name in function_names and name in frame.f_locals:
            return frame
        frame = frame.f_back
    raise KeyError("no caller among %s with a local %r: the restatements' text has changed" % (sorted(function_names), name))


_rigid_shell, _lossy_shell_error, _variable_shell_error, _error_of, _to_object = (lossy.rigid_shell, lossy.shell_error, variable.shell_error, search.error_of,
                                                                                   search.to_object)


@contextlib.contextmanager
def arithmetic_of(base, num_samples, sample_rate, looping_wrap=False):
    """the four restatements with `base` while the block runs; the clip is described as it is registered"""
    if base is None or base.format == NONE:
        yield
        return
    clip = _Clip(num_samples, sample_rate, looping_wrap)

    def on_base(b, sample_indices, transform, has_scale=True, twice=False):
        return apply_additive(base.format, base_at(base, b, base_keys(base, clip, sample_indices), twice), transform, has_scale)

    def rigid_shell(normalized, parents, precisions, distances):
        # step 2 (the clip from its sample 0) or S0 (the segment from `start`): the restatements' walk over A(sample)
        caller = sys._getframe(1)
        start = caller.f_locals["start"] if caller.f_code.co_name == "find_bit_rates" else 0
        applied = f32(normalized).copy()
        indices = start + np.arange(applied.shape[0])
        for b in range(applied.shape[1]):
            applied[:, b, 0:4], applied[:, b, 4:7], applied[:, b, 8:11] = on_base(b, indices, (applied[:, b, 0:4], applied[:, b, 4:7], applied[:, b, 8:11]))
        return _rigid_shell(applied, parents, precisions, distances)

    def shell_error_with(original):
        def shell_error(distance, raw, lossy_transform):
            caller = sys._getframe(1)
            if caller.f_code.co_name != "compress":
                return original(distance, raw, lossy_transform)         # (S2's: error_of has applied A where it is due)
            b = caller.f_locals["b"]
            if np.ndim(raw[0]) == 1:
                # the vote: the first sample on the base's sample 0, the last on the base's LAST sample
                first = apply_additive(base.format, base_at(base, b, 0), raw)
                last = apply_additive(base.format, base_at(base, b, base.num_samples - 1), lossy_transform)
                return original(distance, first, last)
            indices = np.arange(raw[0].shape[0])
            return original(distance, on_base(b, indices, raw), on_base(b, indices, lossy_transform))
        return shell_error

    def segment_of():
        frame = _frame_with("parent_of", ("find_bit_rates",), depth=3)
        return frame.f_locals["start"] + np.arange(frame.f_locals["count"]), frame.f_locals["parent_of"]

    def error_of(distance, raw, lossy_transform, has_scale):
        caller = sys._getframe(1)
        b = caller.f_locals["b"]
        indices, parent_of = segment_of()
        if caller.f_code.co_name == "find_bit_rates" or parent_of[b] < 0:
            # the local error, or the object error of a root, whose local transforms went through no to_object
            raw = on_base(b, indices, raw, has_scale, twice=True)
            lossy_transform = on_base(b, indices, lossy_transform, has_scale, twice=True)
        elif caller.f_code.co_name != "object_error":
            raise KeyError("error_of called from %s: the restatements' text has changed" % caller.f_code.co_name)
        return _error_of(distance, raw, lossy_transform, has_scale)

    def to_object(local, parent, has_scale):
        caller = sys._getframe(1)
        if caller.f_code.co_name not in ("raw_object_of", "object_of"):
            raise KeyError("to_object called from %s: the restatements' text has changed" % caller.f_code.co_name)
        b = caller.f_locals["b"]
        indices, parent_of = segment_of()
        local = on_base(b, indices, local, has_scale, twice=True)
        if parent_of[parent_of[b]] < 0:
            parent = on_base(parent_of[b], indices, parent, has_scale, twice=True)       # (a root is handed over as its local transform)
        return _to_object(local, parent, has_scale)

    saved = lossy.rigid_shell, lossy.shell_error, variable.shell_error, search.error_of, search.to_object, lossy.DEFAULT_SCALE_ONE, variable.DEFAULT_SCALE_ONE
    lossy.rigid_shell, lossy.shell_error, variable.shell_error = rigid_shell, shell_error_with(_lossy_shell_error), shell_error_with(_variable_shell_error)
    search.error_of, search.to_object = error_of, to_object
    if base.format == ADDITIVE1:
        lossy.DEFAULT_SCALE_ONE = variable.DEFAULT_SCALE_ONE = 0
    try:
        yield
    finally:
        lossy.rigid_shell, lossy.shell_error, variable.shell_error, search.error_of, search.to_object, lossy.DEFAULT_SCALE_ONE, variable.DEFAULT_SCALE_ONE = saved


def _checked(samples, base):
    """the per-instance refusals and the base's finite test, in front of everything"""
    if base is None or base.format == NONE:
        return
    if base.num_tracks < f32(samples).shape[1]:
        raise Refused("a base with fewer tracks than the instance")
    if not base.finite():
        raise ValueError(NOT_FINITE_MESSAGE)


def compress_drop_w(samples, sample_rate, base=None, **settings):
    """lossy_rotation_compress_restatement.compress against `base` (a Base or None)"""
    _checked(samples, base)
    with arithmetic_of(base, f32(samples).shape[0], sample_rate, settings.get("looping_wrap", False)):
        return lossy.compress(samples, sample_rate, **settings)


def compress_variable(samples, sample_rate, bit_rates, base=None, **settings):
    """variable_compress_restatement.compress against `base`"""
    _checked(samples, base)
    with arithmetic_of(base, f32(samples).shape[0], sample_rate, settings.get("looping_wrap", False)):
        return variable.compress(samples, sample_rate, bit_rates, **settings)


def find_bit_rates(samples, sample_rate, base=None, level="medium", **settings):
    """bit_rate_search_levels_restatement.find_bit_rates against `base`: its Search as it is"""
    _checked(samples, base)
    with arithmetic_of(base, f32(samples).shape[0], sample_rate, settings.get("looping_wrap", False)):
        return levels.find_bit_rates(samples, sample_rate, level=level, **settings)


def compress_with_search(samples, sample_rate, base=None, level="medium", **settings):
    """"search, then compress" against `base`: (the Search, the Compressed at its table)"""
    found = find_bit_rates(samples, sample_rate, base, level=level, **settings)
    return found, compress_variable(samples, sample_rate, found.table, base, **settings)
