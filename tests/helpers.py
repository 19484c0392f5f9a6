"""Shared helpers of the parity tests: maps a (settings, default mode) pair of the reference bridge onto oracle options and
C-ABI params, loads golden fixtures."""
import ctypes
import glob
import os

import numpy as np

from oracle import bindings as ob

GOLDEN_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")

# Components compared: W lanes of translation (7) and scale (11) are unspecified in the reference
# (animated_track_cache.transform.h:964); this framework defines them as 0.
XYZ_LANES = [0, 1, 2, 3, 4, 5, 6, 8, 9, 10]


def golden_cases():
    return sorted(os.path.splitext(os.path.basename(p))[0] for p in glob.glob(os.path.join(GOLDEN_DIR, "*.npz")))


def load_golden(name):
    data = np.load(os.path.join(GOLDEN_DIR, f"{name}.npz"))
    case = {key: data[key] for key in data.files}
    from acl_amd import synth
    blob = synth.aligned_bytes(case["blob"].size)
    blob[:] = case["blob"]
    case["blob"] = blob
    case["settings"] = int(case["settings"])
    case["default_mode"] = int(case["default_mode"])
    case["defaults"] = case["defaults"] if case["defaults"].size else None
    case["track_rounding"] = case["track_rounding"] if case["track_rounding"].size else None
    return case


def mode_triplet(default_mode):
    """reference bridge default_mode -> (rotation, translation, scale) default_sub_track_mode"""
    return {
        0: (ob.DEFAULT_CONSTANT, ob.DEFAULT_CONSTANT, ob.DEFAULT_LEGACY),
        1: (ob.DEFAULT_SKIPPED, ob.DEFAULT_SKIPPED, ob.DEFAULT_SKIPPED),
        2: (ob.DEFAULT_CONSTANT, ob.DEFAULT_CONSTANT, ob.DEFAULT_CONSTANT),
        3: (ob.DEFAULT_VARIABLE, ob.DEFAULT_VARIABLE, ob.DEFAULT_VARIABLE),
    }[default_mode]


def settings_pair(settings):
    """reference bridge settings id -> (normalization, per_track_rounding)"""
    return {0: (ob.NORMALIZE_LERP_ONLY, 0), 1: (ob.NORMALIZE_ALWAYS, 1), 2: (ob.NORMALIZE_LERP_ONLY, 1), 3: (ob.NORMALIZE_LERP_ONLY, 0),
            4: (ob.NORMALIZE_LERP_ONLY, 0), 5: (ob.NORMALIZE_NEVER, 0)}[settings]      # 4 / 5: default settings that take every packed format (ref_bridge.cpp)


def oracle_options(settings=0, default_mode=0, defaults=None, track_rounding=None, looping=ob.LOOP_AS_COMPRESSED):
    normalization, per_track = settings_pair(settings)
    rot, trans, scale = mode_triplet(default_mode)
    options = ob.default_options(looping_policy=looping, normalization=normalization, per_track_rounding=per_track,
                                 default_rotation_mode=rot, default_translation_mode=trans, default_scale_mode=scale)
    if defaults is not None and default_mode in (2, 3):
        options.default_values = defaults.ctypes.data
    if track_rounding is not None:
        options.track_rounding = track_rounding.ctypes.data
    return options


def gpu_params(runtime, rounding=0, settings=0, default_mode=0, looping=2):
    normalization, per_track = settings_pair(settings)
    rot, trans, scale = mode_triplet(default_mode)
    return runtime.default_params(rounding_policy=rounding, looping_policy=looping, normalization=normalization, per_track_rounding=per_track,
                                  default_rotation_mode=rot, default_translation_mode=trans, default_scale_mode=scale)


def max_abs_diff(a, b):
    if a.size == 0:
        return 0.0
    return float(np.abs(a[..., XYZ_LANES] - b[..., XYZ_LANES]).max())


def bit_equal(a, b):
    return np.array_equal(np.ascontiguousarray(a[..., XYZ_LANES]).view(np.uint32), np.ascontiguousarray(b[..., XYZ_LANES]).view(np.uint32))


# ACLHIP_DECODE_FAST's bound: rotation components within 2e-6 of the exact decode, translations and scales bit identical
FAST_ROTATION_TOLERANCE = 2.0e-6
FAST_VECTOR_LANES = [4, 5, 6, 8, 9, 10]


def assert_within_tolerance(fast, expected, what):
    """a fast decode against the exact one (or the oracle): returns the worst rotation difference"""
    worst = float(np.abs(fast[..., 0:4] - expected[..., 0:4]).max()) if fast.size else 0.0
    assert worst <= FAST_ROTATION_TOLERANCE, f"{what}: rotations differ by {worst}"
    assert np.array_equal(np.ascontiguousarray(fast[..., FAST_VECTOR_LANES]).view(np.uint32), np.ascontiguousarray(expected[..., FAST_VECTOR_LANES]).view(np.uint32)), f"{what}: translations / scales moved"
    return worst


def per_instance_looping_oracle(decode, policies):
    """decode(policy) -> values for every instance under that policy; picks every instance's own"""
    by_policy = [decode(policy) for policy in (ob.LOOP_CLAMP, ob.LOOP_WRAP, ob.LOOP_AS_COMPRESSED)]
    out = by_policy[0].copy()
    for policy in (1, 2):
        out[policies == policy] = by_policy[policy][policies == policy]
    return out


# ---- compressed_database fixtures (tests/golden/database/*.npz, see make_golden_database.py) ----
DATABASE_GOLDEN_DIR = os.path.join(GOLDEN_DIR, "database")


def database_golden_cases():
    return sorted(os.path.splitext(os.path.basename(p))[0] for p in glob.glob(os.path.join(DATABASE_GOLDEN_DIR, "*.npz")))


def load_database_golden(name):
    from acl_amd import synth

    def aligned(array):
        out = synth.aligned_bytes(max(array.size, 1))
        out[: array.size] = array
        return out[: array.size] if array.size else out[:0]

    data = np.load(os.path.join(DATABASE_GOLDEN_DIR, f"{name}.npz"))
    case = {key: data[key] for key in data.files}
    offsets = case["clip_offsets"]
    case["clips"] = [aligned(case["clips"][offsets[i]: offsets[i + 1]]) for i in range(offsets.size - 1)]
    for key in ("database", "database_inline", "bulk_medium", "bulk_low"):
        case[key] = aligned(case[key])
    return case


def load_bench_database():
    """tests/golden/bench/database_64_clips_100_bones.npz (make_bench_database.py): BASELINE.json configs[4] as written --
    64 clips bound to one database built by the reference's build_database with its default tier proportions."""
    from acl_amd import synth

    def aligned(array):
        out = synth.aligned_bytes(max(array.size, 1))
        out[: array.size] = array
        return out[: array.size] if array.size else out[:0]

    data = np.load(os.path.join(GOLDEN_DIR, "bench", "database_64_clips_100_bones.npz"))
    offsets = data["clip_offsets"]
    return {"clips": [aligned(data["clips"][offsets[i]: offsets[i + 1]]) for i in range(offsets.size - 1)],
            "database": aligned(data["database"]), "bulk_medium": aligned(data["bulk_medium"]), "bulk_low": aligned(data["bulk_low"])}


# ---- scalar track list fixtures (tests/golden/scalar/*.npz, see make_golden_scalar.py) ----
SCALAR_GOLDEN_DIR = os.path.join(GOLDEN_DIR, "scalar")

SCALAR_CLIP_SPECS = {
    "float1f_all_rates": dict(seed=101, track_type=0, num_tracks=48, num_samples=40),
    "float2f_v2_0_rates": dict(seed=102, track_type=1, num_tracks=19, num_samples=25, version=7),
    "float3f_wrap": dict(seed=103, track_type=2, num_tracks=33, num_samples=61, wrap=1),
    "float4f_mostly_raw": dict(seed=104, track_type=3, num_tracks=12, num_samples=17, raw_fraction=0.6, constant_fraction=0.1),
    "vector4f_low_bits": dict(seed=105, track_type=4, num_tracks=27, num_samples=33, min_bits=1, max_bits=6, raw_fraction=0.0),
    "float1f_one_sample": dict(seed=106, track_type=0, num_tracks=5, num_samples=1),
    "float3f_all_constant": dict(seed=107, track_type=2, num_tracks=9, num_samples=12, constant_fraction=1.0),
    "float1f_many_tracks": dict(seed=108, track_type=0, num_tracks=700, num_samples=9, version=8),
    "vector4f_two_samples_v2_0_wrap_flag_ignored": dict(seed=109, track_type=4, num_tracks=3, num_samples=2, version=7, wrap=1),
}


def scalar_golden_cases():
    return sorted(os.path.splitext(os.path.basename(p))[0] for p in glob.glob(os.path.join(SCALAR_GOLDEN_DIR, "*.npz")))


def load_scalar_golden(name):
    from acl_amd import synth
    data = np.load(os.path.join(SCALAR_GOLDEN_DIR, f"{name}.npz"))
    case = {key: data[key] for key in data.files}
    blob = synth.aligned_bytes(case["blob"].size)
    blob[:] = case["blob"]
    case["blob"] = blob
    return case


def exact(a, b):
    return np.array_equal(np.ascontiguousarray(a).view(np.uint32), np.ascontiguousarray(b).view(np.uint32))


# ---- pose consumer fixtures (tests/golden/consumers/*.npz, see make_golden_consumers.py) ----
CONSUMER_GOLDEN_DIR = os.path.join(GOLDEN_DIR, "consumers")


def consumer_golden_cases():
    return sorted(os.path.splitext(os.path.basename(p))[0] for p in glob.glob(os.path.join(CONSUMER_GOLDEN_DIR, "*.npz")))


def load_consumer_golden(name):
    from acl_amd import synth
    data = np.load(os.path.join(CONSUMER_GOLDEN_DIR, f"{name}.npz"))
    case = {key: data[key] for key in data.files}
    for key in ("additive_blob", "base_blob"):
        blob = synth.aligned_bytes(case[key].size)
        blob[:] = case[key]
        case[key] = blob
    return case


# ---- the real-compressor corpus (tests/golden/corpus/*.npz, see make_corpus.py) ----
CORPUS_DIR = os.path.join(GOLDEN_DIR, "corpus")
CORPUS_DATABASES = ("database", "database_4kb", "database_4kb_mixed", "database_mixed")
_corpus = {}


def _aligned_copy(array):
    from acl_amd import synth
    out = synth.aligned_bytes(max(array.size, 1))
    out[: array.size] = array
    return out[: array.size] if array.size else out[:0]


def load_corpus():
    """The transform clips the reference's compressor wrote for tests/golden/make_corpus.py: a list of dicts
    {name, spec, blob (16 byte aligned), parents (int32, -1 = root), bind_pose [num_tracks, 12], bind_is_default}"""
    import json
    if "transforms" not in _corpus:
        data = np.load(os.path.join(CORPUS_DIR, "transforms.npz"))
        specs = json.loads(str(data["specs"]))
        blobs, offsets, track_offsets = data["blobs"], data["offsets"], data["track_offsets"]
        parents, bind_poses, bind_is_default = data["parents"], data["bind_poses"], data["bind_is_default"]
        clips = []
        for index, spec in enumerate(specs):
            first, last = int(track_offsets[index]), int(track_offsets[index + 1])
            clips.append({"name": spec["name"], "spec": spec, "blob": _aligned_copy(blobs[offsets[index]: offsets[index + 1]]), "parents": parents[first:last].copy(),
                          "bind_pose": bind_poses[first:last].copy(), "bind_is_default": bool(bind_is_default[index])})
        _corpus["transforms"] = clips
    return _corpus["transforms"]


def load_corpus_database(name):
    """One of CORPUS_DATABASES: {clips: [blobs], database, bulk_medium, bulk_low, options}"""
    import json
    data = np.load(os.path.join(CORPUS_DIR, f"{name}.npz"))
    offsets = data["clip_offsets"]
    return {"clips": [_aligned_copy(data["clips"][offsets[i]: offsets[i + 1]]) for i in range(offsets.size - 1)], "database": _aligned_copy(data["database"]),
            "bulk_medium": _aligned_copy(data["bulk_medium"]), "bulk_low": _aligned_copy(data["bulk_low"]), "options": json.loads(str(data["options"]))}


def corpus_sample_times(blob):
    """validate_accuracy's sample times (tools/acl_compressor/sources/validate_tracks.cpp:125-129,217-219): min(i / rate, duration) for
    every sample of the clip, the repeating first sample of a wrapping clip included"""
    lib = ob.oracle()
    duration = lib.aclo_finite_duration(blob.ctypes.data, ob.LOOP_AS_COMPRESSED)
    rate = np.float32(lib.aclo_sample_rate(blob.ctypes.data))
    num_samples = lib.aclo_calculate_num_samples(ctypes.c_float(duration), ctypes.c_float(rate)) if lib.aclo_num_tracks(blob.ctypes.data) != 0 else 0
    times = np.minimum(np.arange(num_samples, dtype=np.float32) / rate, np.float32(duration)).astype(np.float32)
    return times, float(duration)
