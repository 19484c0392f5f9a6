"""What aclhip_compress_raw_tracks_batch computes -- acl::compress_track_list for a track_array_qvvf with the reference's RAW compression
settings (rotation_format = quatf_full, translation_format = scale_format = vector3f_full: get_raw_compression_settings();
compression/impl/compress.transform.impl.h:138-530 and the files it calls) -- restated on the CPU with numpy, in the order of the header's
definition. In that configuration nothing is searched: one segment, no range reduction, no looping vote, binary constant and default
tests, every animated sample stored as its own 32 bit words. What is left is the transform blob writer:

  step 1   the checks: every used lane finite, every rotation normalized by the reference's own test -- a rotation that fails it would be
           renormalized through the x86 reciprocal square root estimate, which no other device reproduces: such an array is refused
  step 2   looping: nothing is dropped; an array registered as wrapping is marked wrap optimized
  step 3   per sub-track: constant iff every sample == sample 0 in every used lane; default iff constant and sample 0 == the default value
  step 4   has_scale iff some scale sub-track is not default
  step 5   the blob: raw_buffer_header, tracks_header, transform_tracks_header, one segment_header, the packed sub-track types (2 bits
           each, 16 per word, first track in the top bits; rotations, translations, then scales when has_scale), sample 0 of the constant
           sub-tracks (rotations, translations, scales, each in track order), the animated stream (per sample: rotations xyzw,
           translations xyz, scales xyz, each in track order, every float as a 32 bit word most significant byte first)
  step 6   optional metadata: parent indices, track descriptions, the optional_metadata_header; or 15 zero bytes
  step 7   size, and the FNV-1a hash over [8, size)

A helper, not a test file: tests/test_transform_compress_oracle.py holds it to the reference's compressor on every byte,
tests/test_gpu_transform_compress.py holds the kernels to it on every byte."""
import struct

import numpy as np

F32 = np.float32
TAG_COMPRESSED_TRACKS = 0xAC11AC11
VERSION_LATEST = 10
TRACK_TYPE_QVVF = 12
HAS_SCALE, DEFAULT_SCALE_ONE, WRAP_OPTIMIZED, HAS_METADATA = 1, 2, 0x40000000, 0x80000000
INVALID_OFFSET = NO_PARENT = 0xFFFFFFFF
DEFAULT, CONSTANT, ANIMATED = 0, 1, 2
INCLUDE_PARENT_TRACK_INDICES, INCLUDE_TRACK_DESCRIPTIONS = 2, 4     # ACLHIP_COMPRESS_INCLUDE_*
NOT_FINITE_MESSAGE = "Some samples are not finite"
IDENTITY = np.array([0, 0, 0, 1, 0, 0, 0, 0, 1, 1, 1, 0], dtype=np.float32)       # QVV48 of qvv_identity (the fourth lanes are not read)
# the used lanes of a QVV48 record per sub-track type: rotation xyzw, translation xyz, scale xyz
LANES = (slice(0, 4), slice(4, 7), slice(8, 11))


class NotNormalized(ValueError):
    """ACLHIP_COMPRESS_NOT_NORMALIZED"""


def fnv1a32(data):
    acc = 2166136261
    for byte in bytes(data):
        acc = ((acc ^ byte) * 16777619) & 0xFFFFFFFF
    return acc


def rotations_normalized(rotations):
    """rtm::quat_is_normalized(q) (threshold 0.00001F) over float32 [..., 4]: fabs(dot - 1) < threshold with dot accumulated as
    (x * x + z * z) + (y * y + w * w), the lane order of vector_dot (oracle/rtm_shim/rtm/vector4f.h). True exactly when
    initialize_clip_context (clip_context.impl.h:147-153) keeps the rotation's bits."""
    q = np.asarray(rotations, dtype=np.float32)
    with np.errstate(all="ignore"):
        squares = (q * q).astype(np.float32)
        dot = ((squares[..., 0] + squares[..., 2]).astype(np.float32) + (squares[..., 1] + squares[..., 3]).astype(np.float32)).astype(np.float32)
        return np.abs((dot - F32(1.0)).astype(np.float32)) < F32(0.00001)


def bound(num_tracks, num_samples, flags=0):
    """aclhip_transform_compress_bound: headers, sub-track types, every sub-track animated (40 bytes per track and sample; a constant one
    takes its bytes once), metadata or the 15 byte tail, rounded up to 16"""
    size = 100 + 12 * ((num_tracks + 15) // 16) + 40 * num_tracks * num_samples
    if flags & (INCLUDE_PARENT_TRACK_INDICES | INCLUDE_TRACK_DESCRIPTIONS):
        size += 4 * num_tracks + (48 * num_tracks if flags & INCLUDE_TRACK_DESCRIPTIONS else 0) + 20
    else:
        size += 15
    return min((size + 15) & ~15, 0xFFFFFFFFFFFFFFF0)


def classify(samples, default_pose):
    """steps 3 and 4 over samples [S, T, 12]: types uint8 [3, T] (rotation, translation, scale rows) and has_scale"""
    num_tracks = samples.shape[1]
    types = np.zeros((3, num_tracks), dtype=np.uint8)
    for kind, lanes in enumerate(LANES):
        constant = (samples[:, :, lanes] == samples[:1, :, lanes]).all(axis=(0, 2))
        default = constant & (samples[0, :, lanes] == default_pose[:, lanes]).all(axis=1)
        types[kind] = np.where(default, DEFAULT, np.where(constant, CONSTANT, ANIMATED))
    return types, bool((types[2] != DEFAULT).any())


def pack_types(types):
    """one sub-track type row as its packed words: 16 per uint32, the first track in the top bits"""
    words = np.zeros((types.size + 15) // 16, dtype=np.uint32)
    for track, value in enumerate(types):
        words[track // 16] |= np.uint32(int(value) << ((15 - track % 16) * 2))
    return words.tobytes()


def compress(samples, sample_rate, default_pose=None, parents=None, flags=0, precision=1.0e-4, shell_distance=1.0, track_precisions=None,
             track_shell_distances=None, looping_wrap=False):
    """steps 1 - 7: the blob as a uint8 array. samples float32 [S, T, 12] QVV48; default_pose [>= T, 12] or None (the identity); parents
    uint32 [>= T] (0xFFFFFFFF: a root) or None (every track a root). Raises ValueError(NOT_FINITE_MESSAGE) or NotNormalized."""
    samples = np.ascontiguousarray(samples, dtype=np.float32)
    num_samples, num_tracks, _ = samples.shape
    default_pose = np.tile(IDENTITY, (num_tracks, 1)) if default_pose is None else np.ascontiguousarray(default_pose, dtype=np.float32)[:num_tracks]
    used = np.concatenate([samples[:, :, lanes] for lanes in LANES], axis=2)
    if not np.isfinite(used).all():
        raise ValueError(NOT_FINITE_MESSAGE)
    if not rotations_normalized(samples[:, :, 0:4]).all():
        raise NotNormalized("a rotation is not normalized")

    types, has_scale = classify(samples, default_pose)
    kinds = 3 if has_scale else 2
    packed_types = b"".join(pack_types(types[kind]) for kind in range(kinds))
    constants = b"".join(samples[0, b, LANES[kind]].tobytes() for kind in range(kinds) for b in range(num_tracks) if types[kind, b] == CONSTANT)
    animated = [[b for b in range(num_tracks) if types[kind, b] == ANIMATED] for kind in range(3)]
    pose = np.concatenate([samples[:, animated[kind], LANES[kind]].reshape(num_samples, -1) for kind in range(3)], axis=1)
    stream = np.ascontiguousarray(pose).view(np.uint32).astype(">u4").tobytes()        # most significant byte first
    pose_bits = 32 * pose.shape[1]

    if flags & INCLUDE_TRACK_DESCRIPTIONS:
        flags |= INCLUDE_PARENT_TRACK_INDICES
    metadata = b""
    types_offset = 52 + 16
    constants_offset = types_offset + len(packed_types)
    range_offset = constants_offset + len(constants)
    metadata_at = 32 + range_offset + len(stream)
    if flags & INCLUDE_PARENT_TRACK_INDICES:
        parents = np.full(num_tracks, NO_PARENT, dtype=np.uint32) if parents is None else np.asarray(parents).astype(np.uint32)[:num_tracks]
        parents = np.where(parents < num_tracks, parents, NO_PARENT).astype(np.uint32)      # write_parent_track_indices: find_output_index
        descriptions_at = INVALID_OFFSET
        metadata = parents.tobytes()
        if flags & INCLUDE_TRACK_DESCRIPTIONS:
            precisions = np.full(num_tracks, precision, dtype=np.float32) if track_precisions is None else np.asarray(track_precisions, dtype=np.float32)[:num_tracks]
            shells = np.full(num_tracks, shell_distance, dtype=np.float32) if track_shell_distances is None else np.asarray(track_shell_distances, dtype=np.float32)[:num_tracks]
            descriptions_at = metadata_at + len(metadata)
            rows = np.concatenate([precisions[:, None], shells[:, None], default_pose[:, 0:4], default_pose[:, 4:7], default_pose[:, 8:11]], axis=1).astype(np.float32)
            metadata += rows.tobytes()
        metadata += struct.pack("<5I", INVALID_OFFSET, INVALID_OFFSET, metadata_at, descriptions_at, INVALID_OFFSET)
    tail = metadata if metadata else b"\0" * 15

    misc = (HAS_SCALE if has_scale else 0) | DEFAULT_SCALE_ONE | (WRAP_OPTIMIZED if looping_wrap else 0) | (HAS_METADATA if metadata else 0)
    tracks_header = struct.pack("<IHBBIIfI", TAG_COMPRESSED_TRACKS, VERSION_LATEST, 0, TRACK_TYPE_QVVF, num_tracks, num_samples, F32(sample_rate), misc)
    counts = [int((types[kind] == ANIMATED).sum()) for kind in range(3)] + [int((types[kind] == CONSTANT).sum()) if kind < kinds else 0 for kind in range(3)]
    transform_header = struct.pack("<13I", 1, 0, *counts, INVALID_OFFSET, 52, types_offset, constants_offset, range_offset)
    segment_header = struct.pack("<4I", pose_bits, 128 * counts[0], 96 * counts[1], range_offset)
    body = tracks_header + transform_header + segment_header + packed_types + constants + stream + tail
    size = 8 + len(body)
    blob = struct.pack("<II", size, fnv1a32(body)) + body
    return np.frombuffer(blob, dtype=np.uint8).copy()


def parse(blob):
    """what the tests read back out of a blob"""
    raw = np.ascontiguousarray(blob, dtype=np.uint8).tobytes()
    size, _ = struct.unpack_from("<II", raw, 0)
    _, _, _, track_type, num_tracks, num_samples, _, misc = struct.unpack_from("<IHBBIIfI", raw, 8)
    header = struct.unpack_from("<13I", raw, 32)
    return {"size": size, "track_type": track_type, "num_tracks": num_tracks, "num_samples": num_samples, "has_scale": bool(misc & HAS_SCALE),
            "wrap": bool(misc & WRAP_OPTIMIZED), "has_metadata": bool(misc & HAS_METADATA), "misc": misc, "num_animated": header[2:5], "num_constant": header[5:8]}


# ---- the cases the CPU and the GPU tests share ----------------------------------------------------------------------------------------------
TRACK_COUNTS = (1, 3, 4, 5, 16, 17, 65)      # 4/5 crosses an animated group, 16/17 a sub-track type word, 64/65 a wave
SAMPLE_COUNTS = (1, 2, 7, 65)


def unit_quaternions(rng, shape):
    """normalized in float64 and rounded to float32: |len^2 - 1| is about 1e-7, far inside the reference's 1e-5"""
    q = rng.standard_normal(tuple(shape) + (4,))
    return (q / np.linalg.norm(q, axis=-1, keepdims=True)).astype(np.float32)


def bind_pose(seed, num_tracks):
    """a default pose that is not the identity"""
    rng = np.random.default_rng(seed)
    pose = np.zeros((num_tracks, 12), dtype=np.float32)
    pose[:, 0:4] = unit_quaternions(rng, (num_tracks,))
    pose[:, 4:7] = rng.uniform(-2.0, 2.0, size=(num_tracks, 3))
    pose[:, 8:11] = rng.uniform(0.5, 1.5, size=(num_tracks, 3))
    return pose


def clip(seed, num_samples, num_tracks, default_pose=None, scales="mixed"):
    """samples float32 [S, T, 12]: per track and sub-track type one of animated, constant, default -- (track + 3 * seed) walks all 27
    mixes. scales: "mixed", or "default" (every scale the default: no scale section). The fourth lanes hold garbage."""
    rng = np.random.default_rng(1000 + seed)
    default_pose = np.tile(IDENTITY, (num_tracks, 1)) if default_pose is None else default_pose
    samples = np.zeros((num_samples, num_tracks, 12), dtype=np.float32)
    samples[:, :, 0:4] = unit_quaternions(rng, (num_samples, num_tracks))
    samples[:, :, 4:7] = rng.uniform(-3.0, 3.0, size=(num_samples, num_tracks, 3))
    samples[:, :, 8:11] = rng.uniform(0.25, 2.0, size=(num_samples, num_tracks, 3))
    samples[:, :, 7] = rng.uniform(-9.0, 9.0, size=(num_samples, num_tracks))
    samples[:, :, 11] = rng.uniform(-9.0, 9.0, size=(num_samples, num_tracks))
    for track in range(num_tracks):
        mix = track + 3 * seed
        for kind, lanes in enumerate(LANES):
            how = (mix // 3 ** kind) % 3 if (kind < 2 or scales == "mixed") else DEFAULT
            if how == CONSTANT:
                samples[:, track, lanes] = samples[0, track, lanes]
            elif how == DEFAULT:
                samples[:, track, lanes] = default_pose[track, lanes]
    return samples


def chain_parents(num_tracks, seed=0):
    """a hierarchy: track 0 a root, every other track hangs below an earlier one; every fifth track a root as well"""
    rng = np.random.default_rng(77 + seed)
    parents = np.array([NO_PARENT] + [int(rng.integers(0, b)) for b in range(1, num_tracks)], dtype=np.uint32)
    parents[5::5] = NO_PARENT
    return parents
