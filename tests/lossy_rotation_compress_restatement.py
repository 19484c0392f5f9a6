"""What aclhip_compress_tracks_batch computes with rotation_format = quatf_drop_w_full (translation_format = scale_format =
vector3f_full) -- acl::compress_track_list once the rotation format is not quatf_full and nothing is variable
(compression/impl/compress.transform.impl.h:138-530) -- restated on the CPU with numpy float32 element operations (single, correctly
rounded IEEE operations; nothing is evaluated in float64), in the order of the header's definition:

  step 0   an instance with a parent index in [b, T) is refused
  step 1   every rotation normalized: q * (1 / sqrt((x * x + z * z) + (y * y + w * w))); then every used lane finite
  step 2   the rigid shell: tracks in descending order, { local shell distance, precision } handed to the parent
  step 3   the looping vote with the shell error at the shell
  step 4   rotations of positive w
  step 5   rotation sub-tracks constant / default by the shell error; translations and scales binary, as in the raw call
  step 6   the raw call's blob with three words per rotation

compress() returns the blob and, per decision (the vote per track, constant, default), the error and the precision it was compared
with. A helper, not a test file: tests/test_lossy_rotation_compress_oracle.py holds it to the reference's compressor,
tests/test_gpu_lossy_rotation_compress.py holds the kernels to it on every byte. Builds on tests/transform_compress_restatement.py."""
import struct

import numpy as np

import transform_compress_restatement as raw_restatement
from transform_compress_restatement import (ANIMATED, CONSTANT, DEFAULT, DEFAULT_SCALE_ONE, F32, HAS_METADATA, HAS_SCALE, IDENTITY, INCLUDE_PARENT_TRACK_INDICES,
                                            INCLUDE_TRACK_DESCRIPTIONS, INVALID_OFFSET, LANES, NO_PARENT, NOT_FINITE_MESSAGE, TAG_COMPRESSED_TRACKS, TRACK_TYPE_QVVF,
                                            VERSION_LATEST, WRAP_OPTIMIZED, fnv1a32, pack_types)

OPTIMIZE_LOOPS = 1                          # ACLHIP_COMPRESS_OPTIMIZE_LOOPS
QUATF_FULL, QUATF_DROP_W_FULL = 0, 2        # acl::rotation_format8
ROTATION_FORMAT_SHIFT = 4                   # in the packed word of the tracks_header


class Refused(ValueError):
    """ACLHIP_COMPRESS_REFUSED by step 0"""


class Compressed:
    """blob uint8; shells float32 [T, 2] { local shell distance, precision }; types uint8 [3, T]; num_samples behind the vote; wrap;
    decisions: a list of (what, track, error, precision) with what in "vote", "constant", "default"; rotation_bytes: a bool mask over
    the blob, True on the bytes of rotation VALUE words"""


def f32(array):
    return np.ascontiguousarray(array, dtype=np.float32)


def normalize(rotations):
    """step 1 over float32 [..., 4]"""
    q = f32(rotations)
    with np.errstate(all="ignore"):
        x, y, z, w = (q[..., c] for c in range(4))
        dot = ((x * x) + (z * z)) + ((y * y) + (w * w))
        inv_length = F32(1.0) / np.sqrt(dot)
        return f32(q * inv_length[..., None])


def positive_w(rotations):
    """step 4: the sign bit of w xored into all four lanes"""
    bits = f32(rotations).view(np.uint32)
    return (bits ^ (bits[..., 3:4] & np.uint32(0x80000000))).view(np.float32)


def quat_mul(lhs, rhs):
    """rtm::quat_mul, x86 form (aclhip_device.h: quat_mul_packed)"""
    lx, ly, lz, lw = (lhs[..., c] for c in range(4))
    rx, ry, rz, rw = (rhs[..., c] for c in range(4))
    out = np.empty(np.broadcast(lhs, rhs).shape, dtype=np.float32)
    out[..., 0] = ((rw * lx) + (rx * lw)) + ((ry * lz) + -(rz * ly))
    out[..., 1] = ((rw * ly) + -(rx * lz)) + ((ry * lw) + (rz * lx))
    out[..., 2] = ((rw * lz) + (rx * ly)) + (-(ry * lx) + (rz * lw))
    out[..., 3] = ((rw * lw) + -(rx * lx)) + (-(ry * ly) + -(rz * lz))
    return out


def mul_point3(point, rotation, translation, scale):
    """rtm::qvv_mul_point3: quat_mul_vector3(scale * point, rotation) + translation; all three components of scale * point are multiplied"""
    scaled = scale * point
    vector = np.zeros(np.broadcast(rotation[..., 0:3], scaled).shape[:-1] + (4,), dtype=np.float32)
    vector[..., 0:3] = scaled
    conjugate = np.array(np.broadcast_to(rotation, vector.shape), dtype=np.float32)
    conjugate[..., 0:3] = -conjugate[..., 0:3]
    rotated = quat_mul(quat_mul(conjugate, vector), np.broadcast_to(rotation, vector.shape))
    return rotated[..., 0:3] + translation


def shell_points(distance):
    points = np.zeros((3, 3), dtype=np.float32)
    points[0, 0] = points[1, 1] = points[2, 2] = F32(distance)
    return points


def greater(a, b):
    return np.where(a > b, a, b)


def shell_error(distance, raw, lossy):
    """qvvf_transform_error_metric::calculate_error: raw and lossy are (rotation [..., 4], translation [..., 3], scale [..., 3])"""
    errors = []
    with np.errstate(invalid="ignore", over="ignore"):
        for point in shell_points(distance):
            d = mul_point3(point, *lossy) - mul_point3(point, *raw)
            errors.append(np.sqrt(((d[..., 0] * d[..., 0]) + (d[..., 1] * d[..., 1])) + (d[..., 2] * d[..., 2])))
        return f32(greater(greater(errors[0], errors[1]), errors[2]))


def stretch_of(distance, rotation, translation, scale):
    """step 2's maximum over the samples [S, ...] and the three points, from 0.0F"""
    stretch = F32(0.0)
    with np.errstate(invalid="ignore", over="ignore"):
        for point in shell_points(distance):
            p = mul_point3(point, rotation, translation, scale)
            lengths = np.sqrt(((p[..., 0] * p[..., 0]) + (p[..., 1] * p[..., 1])) + (p[..., 2] * p[..., 2]))
            longest = lengths.max()         # (no length is a NaN inside the definition: the order of the comparisons does not show)
            stretch = longest if longest > stretch else stretch
    return F32(stretch)


def rigid_shell(normalized, parents, precisions, distances):
    """step 2 over samples [S, T, 12] with normalized rotations: float32 [T, 2] { local_b, sprec_b }"""
    num_tracks = normalized.shape[1]
    shells = np.stack([distances, precisions], axis=1).astype(np.float32)
    for b in range(num_tracks - 1, -1, -1):
        d = shells[b, 0]
        psd = stretch_of(d, normalized[:, b, 0:4], normalized[:, b, 4:7], normalized[:, b, 8:11])
        if d != distances[b]:
            psd = F32(psd + precisions[b])
        parent = int(parents[b])
        if parent < num_tracks and psd > shells[parent, 0]:
            shells[parent] = (psd, shells[b, 1])
    return shells


def compress(samples, sample_rate, default_pose=None, parents=None, flags=0, precision=1.0e-4, shell_distance=1.0, track_precisions=None,
             track_shell_distances=None, looping_wrap=False):
    """steps 0 - 6. samples float32 [S, T, 12] QVV48; default_pose [>= T, 12] or None (the identity); parents uint32 [>= T] (0xFFFFFFFF: a
    root) or None (every track a root); flags: OPTIMIZE_LOOPS and the two INCLUDE_* flags. Returns a Compressed. Raises Refused or
    ValueError(NOT_FINITE_MESSAGE)."""
    samples = f32(samples)
    num_samples, num_tracks, _ = samples.shape
    default_pose = np.tile(IDENTITY, (num_tracks, 1)) if default_pose is None else f32(default_pose)[:num_tracks]
    table_parents = np.full(num_tracks, NO_PARENT, dtype=np.uint32) if parents is None else np.asarray(parents).astype(np.uint32)[:num_tracks]
    precisions = np.full(num_tracks, precision, dtype=np.float32) if track_precisions is None else f32(track_precisions)[:num_tracks]
    distances = np.full(num_tracks, shell_distance, dtype=np.float32) if track_shell_distances is None else f32(track_shell_distances)[:num_tracks]
    out = Compressed()
    out.decisions = []

    # step 0
    if any(b <= int(parent) < num_tracks for b, parent in enumerate(table_parents)):
        raise Refused("a parent index at or behind its child")
    # step 1
    kept = samples.copy()
    kept[:, :, 0:4] = normalize(samples[:, :, 0:4])
    if not np.isfinite(np.concatenate([kept[:, :, lanes] for lanes in LANES], axis=2)).all():
        raise ValueError(NOT_FINITE_MESSAGE)
    # step 2
    shells = out.shells = rigid_shell(kept, table_parents, precisions, distances)
    # step 3
    wrap = bool(looping_wrap)
    if (flags & OPTIMIZE_LOOPS) and not looping_wrap and num_samples > 1:
        apart = False
        for b in range(num_tracks):
            error = shell_error(shells[b, 0], (kept[0, b, 0:4], kept[0, b, 4:7], kept[0, b, 8:11]), (kept[-1, b, 0:4], kept[-1, b, 4:7], kept[-1, b, 8:11]))
            out.decisions.append(("vote", b, F32(error), shells[b, 1]))
            apart = apart or bool(error > shells[b, 1])
        if not apart:
            kept, wrap = kept[:-1], True
            num_samples -= 1
    # step 4
    kept = kept.copy()
    kept[:, :, 0:4] = positive_w(kept[:, :, 0:4])
    # step 5
    types, has_scale = raw_restatement.classify(kept, default_pose)        # (translations and scales; the rotation row is replaced)
    for b in range(num_tracks):
        rotation, translation, scale = kept[:, b, 0:4], kept[:, b, 4:7], kept[:, b, 8:11]
        moved = shell_error(shells[b, 0], (rotation, translation, scale), (rotation[0], translation, scale)).max()
        out.decisions.append(("constant", b, F32(moved), shells[b, 1]))
        types[0, b] = ANIMATED
        if not moved > shells[b, 1]:
            off_default = shell_error(shells[b, 0], (rotation, translation, scale), (default_pose[b, 0:4], translation, scale)).max()
            out.decisions.append(("default", b, F32(off_default), shells[b, 1]))
            types[0, b] = CONSTANT if off_default > shells[b, 1] else DEFAULT
    out.types, out.num_samples, out.wrap = types, num_samples, wrap

    # step 6
    kinds = 3 if has_scale else 2
    widths = (slice(0, 3), LANES[1], LANES[2])          # a rotation is x, y, z
    packed_types = b"".join(pack_types(types[kind]) for kind in range(kinds))
    # (write_stream_data.h:213-267: groups of four constant rotations as xxxx yyyy zzzz, a last group of n as n, n and n)
    constant_tracks = [b for b in range(num_tracks) if types[0, b] == CONSTANT]
    constant_rotations = b"".join(np.ascontiguousarray(kept[0, constant_tracks[first: first + 4], 0:3].T).tobytes() for first in range(0, len(constant_tracks), 4))
    constants = constant_rotations + b"".join(kept[0, b, widths[kind]].tobytes() for kind in range(1, kinds) for b in range(num_tracks) if types[kind, b] == CONSTANT)
    animated = [[b for b in range(num_tracks) if types[kind, b] == ANIMATED] for kind in range(3)]
    pose = np.concatenate([kept[:, animated[kind], widths[kind]].reshape(num_samples, -1) for kind in range(3)], axis=1)
    stream = np.ascontiguousarray(pose).view(np.uint32).astype(">u4").tobytes()
    pose_bits = 32 * pose.shape[1]

    if flags & INCLUDE_TRACK_DESCRIPTIONS:
        flags |= INCLUDE_PARENT_TRACK_INDICES
    metadata = b""
    types_offset = 52 + 16
    constants_offset = types_offset + len(packed_types)
    range_offset = constants_offset + len(constants)
    metadata_at = 32 + range_offset + len(stream)
    if flags & INCLUDE_PARENT_TRACK_INDICES:
        written_parents = np.where(table_parents < num_tracks, table_parents, NO_PARENT).astype(np.uint32)
        descriptions_at = INVALID_OFFSET
        metadata = written_parents.tobytes()
        if flags & INCLUDE_TRACK_DESCRIPTIONS:
            descriptions_at = metadata_at + len(metadata)
            rows = np.concatenate([precisions[:, None], distances[:, None], default_pose[:, 0:4], default_pose[:, 4:7], default_pose[:, 8:11]], axis=1).astype(np.float32)
            metadata += rows.tobytes()
        metadata += struct.pack("<5I", INVALID_OFFSET, INVALID_OFFSET, metadata_at, descriptions_at, INVALID_OFFSET)
    tail = metadata if metadata else b"\0" * 15

    misc = ((HAS_SCALE if has_scale else 0) | DEFAULT_SCALE_ONE | (QUATF_DROP_W_FULL << ROTATION_FORMAT_SHIFT) | (WRAP_OPTIMIZED if wrap else 0)
            | (HAS_METADATA if metadata else 0))
    tracks_header = struct.pack("<IHBBIIfI", TAG_COMPRESSED_TRACKS, VERSION_LATEST, 0, TRACK_TYPE_QVVF, num_tracks, num_samples, F32(sample_rate), misc)
    counts = [len(animated[kind]) for kind in range(3)] + [int((types[kind] == CONSTANT).sum()) if kind < kinds else 0 for kind in range(3)]
    transform_header = struct.pack("<13I", 1, 0, *counts, INVALID_OFFSET, 52, types_offset, constants_offset, range_offset)
    segment_header = struct.pack("<4I", pose_bits, 96 * counts[0], 96 * counts[1], range_offset)
    body = tracks_header + transform_header + segment_header + packed_types + constants + stream + tail
    size = 8 + len(body)
    out.blob = np.frombuffer(struct.pack("<II", size, fnv1a32(body)) + body, dtype=np.uint8).copy()

    rotation_bytes = np.zeros(size, dtype=bool)
    constants_at = 32 + constants_offset
    rotation_bytes[constants_at: constants_at + len(constant_rotations)] = True
    stream_at = 32 + range_offset
    for sample in range(num_samples):
        rotation_bytes[stream_at + sample * pose_bits // 8: stream_at + sample * pose_bits // 8 + 12 * counts[0]] = True
    out.rotation_bytes = rotation_bytes
    return out


def rotation_bytes_of(blob):
    """the same mask read out of a blob's own headers"""
    raw = np.ascontiguousarray(blob, dtype=np.uint8).tobytes()
    num_samples = struct.unpack_from("<I", raw, 8 + 12)[0]
    header = struct.unpack_from("<13I", raw, 32)
    pose_bits = struct.unpack_from("<I", raw, 32 + 52)[0]
    mask = np.zeros(len(raw), dtype=bool)
    mask[32 + header[11]: 32 + header[11] + 12 * header[5]] = True
    for sample in range(num_samples):
        mask[32 + header[12] + sample * pose_bits // 8: 32 + header[12] + sample * pose_bits // 8 + 12 * header[2]] = True
    return mask


def rotation_values(blob, rotation_bytes):
    """the rotation value words of a blob as float32: the constant ones are little endian, the stream's most significant byte first"""
    raw = np.ascontiguousarray(blob, dtype=np.uint8)
    header = struct.unpack_from("<13I", raw.tobytes(), 32)
    stream_at = 32 + header[12]
    at = np.flatnonzero(rotation_bytes)
    constant = raw[at[at < stream_at]].view("<f4")
    streamed = raw[at[at >= stream_at]].view(">f4").astype(np.float32)
    return np.concatenate([constant, streamed])


# ---- the cases the CPU and the GPU tests share ------------------------------------------------------------------------------------------------
def tree(seed, num_tracks, shape="random"):
    """parents uint32 with parent < child: "random", "chain", "star" (every track below track 0) or "two_roots" (two stars)"""
    rng = np.random.default_rng(500 + seed)
    if shape == "chain":
        parents = [NO_PARENT] + list(range(num_tracks - 1))
    elif shape == "star":
        parents = [NO_PARENT] + [0] * (num_tracks - 1)
    elif shape == "two_roots":
        parents = [NO_PARENT, NO_PARENT] + [b % 2 for b in range(2, num_tracks)]
    else:
        parents = [NO_PARENT] + [int(rng.integers(-1, b)) for b in range(1, num_tracks)]
    return np.array(parents[:num_tracks], dtype=np.int64).astype(np.uint32)


def clip(seed, num_samples, num_tracks, default_pose=None, scales="mixed", close_loop=False):
    """samples float32 [S, T, 12] whose decisions are far from their precisions for precision 0.01 and shell distance 3: per track the
    rotation is one of freely animated, jittering by 1e-6 about a fixed rotation (constant), jittering by 1e-6 about the default (default)
    or fixed; translations small (|t| < 0.5) and scales within 10 % of 1, so that the shells of a shallow tree stay within
    a few units and a jitter of 1e-6 far below the precision; translations and scales are one of animated / constant / default each, or
    every scale is the default -- for a deep chain, whose shell would grow by a tenth at every level otherwise. close_loop: the last sample is the first."""
    rng = np.random.default_rng(9000 + seed)
    default_pose = np.tile(IDENTITY, (num_tracks, 1)) if default_pose is None else default_pose
    samples = np.zeros((num_samples, num_tracks, 12), dtype=np.float32)
    samples[:, :, 0:4] = raw_restatement.unit_quaternions(rng, (num_samples, num_tracks))
    samples[:, :, 4:7] = rng.uniform(-0.5, 0.5, size=(num_samples, num_tracks, 3))
    samples[:, :, 8:11] = rng.uniform(0.9, 1.1, size=(num_samples, num_tracks, 3))
    samples[:, :, 7] = rng.uniform(-9.0, 9.0, size=(num_samples, num_tracks))
    samples[:, :, 11] = rng.uniform(-9.0, 9.0, size=(num_samples, num_tracks))
    for track in range(num_tracks):
        mix = track + 3 * seed
        how = mix % 4
        if how != 0:
            about = default_pose[track, 0:4].astype(np.float64) if how == 2 else samples[0, track, 0:4].astype(np.float64)
            jitter = about + (rng.standard_normal((num_samples, 4)) * 1.0e-6 if how != 3 else 0.0)
            samples[:, track, 0:4] = (jitter / np.linalg.norm(jitter, axis=-1, keepdims=True)).astype(np.float32)
        for kind in (1, 2):
            how = ((mix // 4) % 3 if kind == 1 else (mix // 2 + 1) % 3) if (kind < 2 or scales == "mixed") else DEFAULT
            if how == CONSTANT:
                samples[:, track, LANES[kind]] = samples[0, track, LANES[kind]]
            elif how == DEFAULT:
                samples[:, track, LANES[kind]] = default_pose[track, LANES[kind]]
    if close_loop:
        samples[-1] = samples[0]
    return samples


def decisions_are_clear(compressed):
    """every decision's error is at most half or at least twice the precision it was compared with"""
    return all(error <= F32(0.5) * bound or error >= F32(2.0) * bound for _, _, error, bound in compressed.decisions)
