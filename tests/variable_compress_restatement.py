"""What aclhip_compress_tracks_variable_batch computes -- acl::compress_track_list with quatf_drop_w_variable / vector3f_variable /
vector3f_variable (compression/impl/compress.transform.impl.h:138-530) with the bit rates GIVEN instead of searched -- restated on the
CPU with numpy float32 element operations (single, correctly rounded IEEE operations; nothing is evaluated in float64), in the order of
the header's definition:

  steps 0 - 4  tests/lossy_rotation_compress_restatement.py: parent refusal, normalize and finite check, rigid shell, looping vote, positive w
  step 5       all three sub-track kinds constant / default by the shell error, each seeing the kinds compacted before it
  step 6       clip ranges and the clip-normalized samples
  step 7       split_samples_per_segment (ideal 16, at most 31)
  step 8       segment ranges with the 8 bit fix-up, the doubly normalized samples
  step 9       quantization at the entry's rate (0 .. 24)
  step 10      the segmented, bit packed blob

compress() returns the blob, what the drop-w restatement records (shells, types, decisions) and `decoded`: the values a decoder gives
at every key (the arithmetic of impl/decompression.transform.h: q * (1 / max), * extent + min of the segment, of the clip). A helper,
not a test file: tests/test_variable_compress_oracle.py holds it to the reference's compressor, tests/test_gpu_variable_compress.py holds
the kernels to it on every byte."""
import struct

import numpy as np

import lossy_rotation_compress_restatement as lossy
from lossy_rotation_compress_restatement import Compressed, Refused, OPTIMIZE_LOOPS, f32, shell_error, tree, clip, decisions_are_clear  # noqa: F401  (the cases the tests share)
from transform_compress_restatement import (ANIMATED, CONSTANT, DEFAULT, DEFAULT_SCALE_ONE, F32, HAS_METADATA, HAS_SCALE, IDENTITY, INCLUDE_PARENT_TRACK_INDICES,
                                            INCLUDE_TRACK_DESCRIPTIONS, INVALID_OFFSET, LANES, NO_PARENT, NOT_FINITE_MESSAGE, TAG_COMPRESSED_TRACKS, TRACK_TYPE_QVVF,
                                            VERSION_LATEST, WRAP_OPTIMIZED, fnv1a32, pack_types)

QUATF_DROP_W_VARIABLE, VECTOR3F_VARIABLE = 3, 1     # acl::rotation_format8, acl::vector_format8
RAW_RATE, RAW_FORMAT_BYTE = 24, 31                  # core/impl/variable_bit_rates.h:45; the number of bits a raw sub-track's format byte says
XYZ = (slice(0, 3), slice(4, 7), slice(8, 11))
INV_255 = F32(1.0) / F32(255.0)
INV_65535 = F32(1.0) / F32(65535.0)


def split_samples_per_segment(num_samples, ideal=16, most=31):
    """segment.transform.h:65-128"""
    if num_samples <= most:
        return [num_samples]
    estimated = (num_samples + ideal - 1) // ideal
    counts = [ideal] * estimated
    counts[-1] = ideal - (estimated * ideal - num_samples)
    if (estimated - 1) * (most - ideal) >= counts[-1]:
        while counts[-1] != 0:
            for i in range(estimated - 1):
                if counts[-1] == 0:
                    break
                counts[i] += 1
                counts[-1] -= 1
        counts.pop()
    return counts


def num_segments(num_samples):
    return len(split_samples_per_segment(num_samples))


def bound(num_tracks, num_samples, flags=0):
    """aclhip_variable_compress_bound: every sub-track animated at rate 24"""
    segments = num_segments(num_samples)
    padded = (num_tracks + 3) // 4 * 4
    size = 32 + 52 + (4 * (segments + 1) if segments > 1 else 0) + 16 * segments + 12 * ((num_tracks + 15) // 16) + 72 * num_tracks
    size += segments * ((padded + 2 * num_tracks + 1) + (6 * (padded + 2 * num_tracks) if segments > 1 else 0) + 3) + 36 * num_tracks * num_samples
    if flags & (INCLUDE_PARENT_TRACK_INDICES | INCLUDE_TRACK_DESCRIPTIONS):
        size += 3 + 4 * num_tracks + (48 * num_tracks if flags & INCLUDE_TRACK_DESCRIPTIONS else 0) + 20
    else:
        size += 15
    return (size + 15) & ~15


def value_range(values):
    """normalize.transform.h:51-76 over float32 [S, 3]: min and max from +-1e10, lane-wise. rtm::vector_min and vector_max return their
    second operand where the two compare equal: a zero that is the minimum or the maximum has the sign of the last sample that is a zero"""
    low, high = values.min(axis=0).astype(np.float32), values.max(axis=0).astype(np.float32)
    for c in range(values.shape[1]):
        zeros = np.flatnonzero(values[:, c] == 0)
        if zeros.size:
            low[c] = values[zeros[-1], c] if low[c] == 0 else low[c]
            high[c] = values[zeros[-1], c] if high[c] == 0 else high[c]
    return np.where(low < F32(1.0e10), low, F32(1.0e10)).astype(np.float32), np.where(high > F32(-1.0e10), high, F32(-1.0e10)).astype(np.float32)


def normalize_in(values, range_min, range_extent):
    """normalize.transform.h:200-262: min((v - min) / extent, 1), or 0 where extent < 1e-9"""
    with np.errstate(all="ignore"):
        normalized = np.minimum((values - range_min) / range_extent, F32(1.0)).astype(np.float32)
    return np.where(range_extent < F32(0.000000001), F32(0.0), normalized).astype(np.float32)


def fixup_range(range_min, range_max):
    """normalize.transform.h:133-171, as written: returns the padded min and the padded extent"""
    zero, one, most = F32(0.0), F32(1.0), F32(255.0)
    quantized_min0 = np.minimum(np.maximum(np.floor(range_min * most), zero), most)
    quantized_min1 = np.maximum(quantized_min0 - one, zero)
    padded_min0, padded_min1 = quantized_min0 * INV_255, quantized_min1 * INV_255
    padded_min = np.where(padded_min0 <= range_min, padded_min0, padded_min1).astype(np.float32)
    quantized_extent0 = np.minimum(np.maximum(np.ceil((range_max - padded_min) * most), zero), most)
    quantized_extent1 = np.minimum(quantized_extent0 + one, most)
    padded_extent0, padded_extent1 = quantized_extent0 * INV_255, quantized_extent1 * INV_255
    return padded_min, np.where(padded_extent0 >= range_max, padded_extent0, padded_extent1).astype(np.float32)


def pack_unsigned(values, bits):
    """math/scalar_packing.h:42-48: scalar_round_symmetric(input * float(2^bits - 1)) of an input that is not negative: floor(x + 0.5)"""
    return np.floor(f32(values) * F32((1 << bits) - 1) + F32(0.5)).astype(np.uint32)


def pack_bits(values, widths):
    """the fields back to back, each most significant bit first, zero bits up to a whole byte (core/memory_utils.h:295-335 on a zeroed buffer)"""
    if not values:
        return b""
    values, widths = np.asarray(values, dtype=np.uint64), np.asarray(widths, dtype=np.int64)
    ends = np.cumsum(widths)
    field = np.repeat(np.arange(values.size), widths)
    within = np.arange(int(ends[-1])) - np.repeat(ends - widths, widths)
    shifts = (np.repeat(widths, widths) - 1 - within).astype(np.uint64)
    return np.packbits(((values[field] >> shifts) & np.uint64(1)).astype(np.uint8)).tobytes()


def rate_table(bit_rates, num_rows, num_tracks):
    """uint8 [num_rows, T, 3] from three uniform rates, a [T, 4] table shared by the segments or a [G, T, 4] table of G >= num_rows rows"""
    rates = np.asarray(bit_rates, dtype=np.uint8)
    if rates.ndim == 1:
        return np.broadcast_to(rates[None, None, 0:3], (num_rows, num_tracks, 3))
    if rates.ndim == 2:
        rates = rates[None]
    if rates.shape[0] == 1:
        rates = np.broadcast_to(rates, (num_rows,) + rates.shape[1:])
    assert rates.shape[0] >= num_rows and rates.shape[1] >= num_tracks
    return rates[:num_rows, :num_tracks, 0:3]


def compress(samples, sample_rate, bit_rates, default_pose=None, parents=None, flags=0, precision=1.0e-4, shell_distance=1.0, track_precisions=None,
             track_shell_distances=None, looping_wrap=False, max_samples=None):
    """samples float32 [S, T, 12] QVV48; bit_rates: see rate_table; the rest as lossy_rotation_compress_restatement.compress. Returns a
    Compressed with, besides that one's fields, segments [(start, count)], rates uint8 [G, T, 3] and decoded float32 [S', T, 12]. Raises
    Refused or ValueError(NOT_FINITE_MESSAGE)."""
    samples = f32(samples)
    num_samples, num_tracks, _ = samples.shape
    default_pose = np.tile(IDENTITY, (num_tracks, 1)) if default_pose is None else f32(default_pose)[:num_tracks]
    table_parents = np.full(num_tracks, NO_PARENT, dtype=np.uint32) if parents is None else np.asarray(parents).astype(np.uint32)[:num_tracks]
    precisions = np.full(num_tracks, precision, dtype=np.float32) if track_precisions is None else f32(track_precisions)[:num_tracks]
    distances = np.full(num_tracks, shell_distance, dtype=np.float32) if track_shell_distances is None else f32(track_shell_distances)[:num_tracks]
    out = Compressed()
    out.decisions = []

    # steps 0 - 4
    if any(b <= int(parent) < num_tracks for b, parent in enumerate(table_parents)):
        raise Refused("a parent index at or behind its child")
    kept = samples.copy()
    kept[:, :, 0:4] = lossy.normalize(samples[:, :, 0:4])
    if not np.isfinite(np.concatenate([kept[:, :, lanes] for lanes in LANES], axis=2)).all():
        raise ValueError(NOT_FINITE_MESSAGE)
    shells = out.shells = lossy.rigid_shell(kept, table_parents, precisions, distances)
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
    if max_samples is not None and num_samples > max_samples:
        raise Refused("more samples than max_samples")
    kept = kept.copy()
    kept[:, :, 0:4] = lossy.positive_w(kept[:, :, 0:4])

    # step 5: per track rotation, translation, scale; a kind sees the kinds before it as they were compacted
    types = np.full((3, num_tracks), ANIMATED, dtype=np.uint8)
    for b in range(num_tracks):
        seen = [kept[:, b, 0:4].copy(), kept[:, b, 4:7].copy(), kept[:, b, 8:11].copy()]
        for kind in range(3):
            first = seen[kind][0].copy()
            lossy_transform = list(seen)
            lossy_transform[kind] = first
            moved = shell_error(shells[b, 0], tuple(seen), tuple(lossy_transform)).max()
            out.decisions.append(("constant", b, F32(moved), shells[b, 1]))
            if moved > shells[b, 1]:
                continue
            default_value = default_pose[b, LANES[kind]].copy()
            lossy_transform[kind] = default_value
            off_default = shell_error(shells[b, 0], tuple(seen), tuple(lossy_transform)).max()
            out.decisions.append(("default", b, F32(off_default), shells[b, 1]))
            types[kind, b] = CONSTANT if off_default > shells[b, 1] else DEFAULT
            seen[kind] = np.tile(first if types[kind, b] == CONSTANT else default_value, (num_samples, 1))
    has_scale = bool((types[2] != DEFAULT).any())
    out.types, out.num_samples, out.wrap = types, num_samples, wrap

    # steps 6 - 8
    counts = split_samples_per_segment(num_samples)
    starts = [sum(counts[:g]) for g in range(len(counts))]
    out.segments = list(zip(starts, counts))
    multiple = len(counts) > 1
    animated = [[b for b in range(num_tracks) if types[kind, b] == ANIMATED] for kind in range(3)]
    rates = out.rates = rate_table(bit_rates, len(counts), num_tracks)
    for kind in range(3):
        for b in animated[kind]:
            for g in range(len(counts)):
                if rates[g, b, kind] > RAW_RATE or (rates[g, b, kind] == 0 and not multiple):
                    raise Refused("a bit rate of %d" % rates[g, b, kind])
    clip_ranges, clip_normalized, segment_ranges, normalized = {}, {}, {}, {}
    for kind in range(3):
        for b in animated[kind]:
            values = kept[:, b, XYZ[kind]]
            low, high = value_range(values)
            clip_ranges[kind, b] = (low, f32(high - low))
            normalized[kind, b] = clip_normalized[kind, b] = normalize_in(values, *clip_ranges[kind, b])
            if multiple:
                normalized[kind, b] = clip_normalized[kind, b].copy()
                for g, (start, count) in enumerate(out.segments):
                    segment_ranges[kind, b, g] = fixup_range(*value_range(clip_normalized[kind, b][start: start + count]))
                    normalized[kind, b][start: start + count] = normalize_in(clip_normalized[kind, b][start: start + count], *segment_ranges[kind, b, g])

    # step 9 and the values a decoder gives
    decoded = out.decoded = np.zeros((num_samples, num_tracks, 12), dtype=np.float32)
    for kind in range(3):
        for b in range(num_tracks):
            decoded[:, b, XYZ[kind]] = default_pose[b, XYZ[kind]] if types[kind, b] == DEFAULT else kept[0, b, XYZ[kind]]
    quantized = {}
    for kind in range(3):
        for b in animated[kind]:
            clip_min, clip_extent = clip_ranges[kind, b]
            for g, (start, count) in enumerate(out.segments):
                rate = int(rates[g, b, kind])
                if rate == RAW_RATE:
                    quantized[kind, b, g] = kept[start: start + count, b, XYZ[kind]].view(np.uint32)
                    decoded[start: start + count, b, XYZ[kind]] = kept[start: start + count, b, XYZ[kind]]
                    continue
                if rate == 0:
                    quantized[kind, b, g] = pack_unsigned(clip_normalized[kind, b][start], 16)
                    value = np.tile(quantized[kind, b, g].astype(np.float32) * INV_65535, (count, 1))
                else:
                    quantized[kind, b, g] = pack_unsigned(normalized[kind, b][start: start + count], rate)
                    value = quantized[kind, b, g].astype(np.float32) * (F32(1.0) / F32((1 << rate) - 1))
                    if multiple:
                        low, extent = segment_ranges[kind, b, g]
                        low_byte, extent_byte = pack_unsigned(low, 8), pack_unsigned(extent, 8)
                        value = f32(f32(value * (extent_byte.astype(np.float32) * INV_255)) + low_byte.astype(np.float32) * INV_255)
                decoded[start: start + count, b, XYZ[kind]] = f32(f32(value * clip_extent) + clip_min)

    # step 10
    kinds = 3 if has_scale else 2
    packed_types = b"".join(pack_types(types[kind]) for kind in range(kinds))
    constant_tracks = [[b for b in range(num_tracks) if types[kind, b] == CONSTANT] for kind in range(3)]
    constants = b"".join(np.ascontiguousarray(kept[0, constant_tracks[0][first: first + 4], 0:3].T).tobytes() for first in range(0, len(constant_tracks[0]), 4))
    constant_rotation_bytes = len(constants)
    constants += b"".join(kept[0, b, XYZ[kind]].tobytes() for kind in (1, 2) for b in constant_tracks[kind])
    clip_range_data = b""
    for first in range(0, len(animated[0]), 4):
        group = animated[0][first: first + 4]
        clip_range_data += np.ascontiguousarray(np.stack([clip_ranges[0, b][0] for b in group]).T).tobytes() + np.ascontiguousarray(np.stack([clip_ranges[0, b][1] for b in group]).T).tobytes()
    clip_rotation_bytes = len(clip_range_data)
    clip_range_data += b"".join(clip_ranges[kind, b][0].tobytes() + clip_ranges[kind, b][1].tobytes() for kind in (1, 2) for b in animated[kind])

    padded_rotations = (len(animated[0]) + 3) // 4 * 4
    num_variable = padded_rotations + len(animated[1]) + len(animated[2])
    start_indices = struct.pack("<%dI" % (len(counts) + 1), *starts, 0xFFFFFFFF) if multiple else b""
    segment_headers_offset = 52 + len(start_indices)
    types_offset = segment_headers_offset + 16 * len(counts)
    constants_offset = types_offset + len(packed_types)
    range_offset = constants_offset + len(constants)
    cursor = 32 + range_offset + len(clip_range_data)
    rotation_bytes = {}             # absolute offset -> what lies there, for the comparisons of the oracle test
    segment_headers, segment_data = b"", b""
    out.fields = []                 # (kind, track, segment, sample in the segment, bit offset in the blob, bits) of every rotation bit field
    for g, (start, count) in enumerate(out.segments):
        data_offset = cursor - 32
        data = bytearray()
        for kind in range(3):
            data += bytes(RAW_FORMAT_BYTE if rates[g, b, kind] == RAW_RATE else int(rates[g, b, kind]) for b in animated[kind])
            if kind == 0:
                data += b"\0" * (padded_rotations - len(animated[0]))
        data += b"\0" * ((cursor + len(data)) % 2)
        if multiple:
            out.segment_range_at = getattr(out, "segment_range_at", {})
            out.segment_range_at[g] = cursor + len(data)
            rows = bytearray(6 * padded_rotations)
            for rank, b in enumerate(animated[0]):
                at = rank // 4 * 24 + rank % 4
                if rates[g, b, 0] == 0:
                    q = quantized[0, b, g]
                    values = [q[0] >> 8, q[0] & 255, q[1] >> 8, q[1] & 255, q[2] >> 8, q[2] & 255]
                else:
                    values = list(pack_unsigned(segment_ranges[0, b, g][0], 8)) + list(pack_unsigned(segment_ranges[0, b, g][1], 8))
                for row, value in enumerate(values):
                    rows[at + 4 * row] = int(value)
            data += rows
            for kind in (1, 2):
                for b in animated[kind]:
                    if rates[g, b, kind] == 0:
                        data += quantized[kind, b, g].astype("<u2").tobytes()
                    else:
                        data += pack_unsigned(segment_ranges[kind, b, g][0], 8).astype(np.uint8).tobytes() + pack_unsigned(segment_ranges[kind, b, g][1], 8).astype(np.uint8).tobytes()
        data += b"\0" * (-(cursor + len(data)) % 4)
        stream_at = cursor + len(data)
        values, value_widths, total_bits = [], [], 0
        widths = [[(32 if rates[g, b, kind] == RAW_RATE else int(rates[g, b, kind])) for b in animated[kind]] for kind in range(3)]
        for sample in range(count):
            for kind in range(3):
                for rank, b in enumerate(animated[kind]):
                    bits = widths[kind][rank]
                    if bits == 0:
                        continue
                    if kind == 0:
                        out.fields.append((b, g, sample, stream_at * 8 + total_bits, bits))
                    values.extend(quantized[kind, b, g][sample].tolist())
                    value_widths.extend((bits, bits, bits))
                    total_bits += 3 * bits
        pose_bits = [3 * sum(widths[kind]) for kind in range(3)]
        data += pack_bits(values, value_widths)
        segment_headers += struct.pack("<4I", sum(pose_bits), pose_bits[0], pose_bits[1], data_offset)
        segment_data += bytes(data)
        cursor += len(data)

    if flags & INCLUDE_TRACK_DESCRIPTIONS:
        flags |= INCLUDE_PARENT_TRACK_INDICES
    metadata = b""
    if flags & INCLUDE_PARENT_TRACK_INDICES:
        segment_data += b"\0" * (-cursor % 4)
        metadata_at = cursor + (-cursor % 4)
        written_parents = np.where(table_parents < num_tracks, table_parents, NO_PARENT).astype(np.uint32)
        descriptions_at = INVALID_OFFSET
        metadata = written_parents.tobytes()
        if flags & INCLUDE_TRACK_DESCRIPTIONS:
            descriptions_at = metadata_at + len(metadata)
            rows = np.concatenate([precisions[:, None], distances[:, None], default_pose[:, 0:4], default_pose[:, 4:7], default_pose[:, 8:11]], axis=1).astype(np.float32)
            metadata += rows.tobytes()
        metadata += struct.pack("<5I", INVALID_OFFSET, INVALID_OFFSET, metadata_at, descriptions_at, INVALID_OFFSET)
    tail = metadata if metadata else b"\0" * 15

    misc = ((HAS_SCALE if has_scale else 0) | DEFAULT_SCALE_ONE | (VECTOR3F_VARIABLE << 2) | (VECTOR3F_VARIABLE << 3) | (QUATF_DROP_W_VARIABLE << 4)
            | (WRAP_OPTIMIZED if wrap else 0) | (HAS_METADATA if metadata else 0))
    tracks_header = struct.pack("<IHBBIIfI", TAG_COMPRESSED_TRACKS, VERSION_LATEST, 0, TRACK_TYPE_QVVF, num_tracks, num_samples, F32(sample_rate), misc)
    sub_track_counts = [len(animated[kind]) for kind in range(3)] + [len(constant_tracks[kind]) if kind < kinds else 0 for kind in range(3)]
    transform_header = struct.pack("<13I", len(counts), num_variable, *sub_track_counts, INVALID_OFFSET, segment_headers_offset, types_offset, constants_offset, range_offset)
    body = tracks_header + transform_header + start_indices + segment_headers + packed_types + constants + clip_range_data + segment_data + tail
    size = 8 + len(body)
    out.blob = np.frombuffer(struct.pack("<II", size, fnv1a32(body)) + body, dtype=np.uint8).copy()
    out.animated, out.clip_ranges, out.segment_ranges = animated, clip_ranges, segment_ranges
    out.constant_rotations_at = (32 + constants_offset, constant_rotation_bytes)
    out.clip_rotations_at = (32 + range_offset, clip_rotation_bytes)
    return out


# ---- reading a blob back (the reference's, to take its rates and to compare by section) ---------------------------------------------------------
def parse(blob):
    """the sections of a variable blob from its own headers: a dict of counts, offsets (absolute) and per segment the format bytes, the
    range data offset and the stream offset"""
    raw = np.ascontiguousarray(blob, dtype=np.uint8).tobytes()
    num_tracks, num_samples = struct.unpack_from("<II", raw, 16)
    misc = struct.unpack_from("<I", raw, 28)[0]
    header = struct.unpack_from("<13I", raw, 32)
    parsed = {"num_tracks": num_tracks, "num_samples": num_samples, "misc": misc, "num_segments": header[0], "num_variable": header[1], "animated": header[2:5], "constant": header[5:8],
              "types_at": 32 + header[10], "constants_at": 32 + header[11], "clip_ranges_at": 32 + header[12], "has_scale": bool(misc & 1)}
    words = (num_tracks + 15) // 16
    types = np.zeros((3, num_tracks), dtype=np.uint8)
    for kind in range(3 if parsed["has_scale"] else 2):
        for b in range(num_tracks):
            word = struct.unpack_from("<I", raw, parsed["types_at"] + 4 * (kind * words + b // 16))[0]
            types[kind, b] = (word >> ((15 - b % 16) * 2)) & 3
    parsed["types"] = types
    padded = (header[2] + 3) // 4 * 4
    segments = []
    for g in range(header[0]):
        pose_bits, rotation_bits, translation_bits, data_offset = struct.unpack_from("<4I", raw, 32 + header[9] + 16 * g)
        formats_at = 32 + data_offset
        ranges_at = (formats_at + header[1] + 1) & ~1
        stream_at = (ranges_at + (6 * header[1] if header[0] > 1 else 0) + 3) & ~3
        formats = np.frombuffer(raw, dtype=np.uint8, count=header[1], offset=formats_at)
        segments.append({"pose_bits": pose_bits, "formats_at": formats_at, "ranges_at": ranges_at, "stream_at": stream_at,
                         "formats": (formats[:header[2]], formats[padded: padded + header[3]], formats[padded + header[3]:])})
    parsed["segments"] = segments
    return parsed


def rates_of(blob):
    """the rate table [G, T, 4] a blob was written with: 31 bits -> rate 24, otherwise the number of bits; sub-tracks that are not
    animated get 255 (never read)"""
    parsed = parse(blob)
    rates = np.full((parsed["num_segments"], parsed["num_tracks"], 4), 255, dtype=np.uint8)
    rates[:, :, 3] = 0
    for g, segment in enumerate(parsed["segments"]):
        for kind in range(3):
            tracks = np.flatnonzero(parsed["types"][kind] == ANIMATED)
            formats = segment["formats"][kind]
            rates[g, tracks, kind] = np.where(formats == RAW_FORMAT_BYTE, RAW_RATE, formats)
    return rates


def signed_zeros(seed, num_samples, num_tracks):
    """clip() with translations whose clip minimum or maximum is a zero that occurs with both signs: track 0's x is a zero throughout,
    its y lies in [0, 0.5] and its z in [-0.5, 0], each with zeros of both signs among its samples, the last of them -0, +0 and -0"""
    samples = clip(seed, num_samples, num_tracks)
    rng = np.random.default_rng(seed)
    samples[:, 0, 4:7] = rng.uniform(0.0, 0.5, size=(num_samples, 3)) * np.array([0.0, 1.0, -1.0])
    zeros = np.array([0.0, -0.0, 0.0, -0.0], dtype=np.float32)
    samples[1:9:2, 0, 4] = zeros[::-1]
    samples[-1, 0, 4] = -0.0
    samples[2:10:2, 0, 5] = zeros[::-1]
    samples[3:11:2, 0, 6] = zeros
    return samples


def fixup_boundaries(num_tracks, num_samples=40):
    """clip() of two segments whose translations sit on the edges of fixup_range: every component spans exactly [0, 1] in the first
    segment -- the clip range, so that a clip-normalized sample is the sample itself -- and in the second one runs between a minimum and a
    maximum that are k * (1.0F / 255.0F), its two float32 neighbours or k / 255.0F, for a k and a kind that walk with the component"""
    assert num_segments(num_samples) == 2
    start = split_samples_per_segment(num_samples)[0]
    samples = clip(1, num_samples, num_tracks)
    samples[:, :, 0:4] = lossy.raw_restatement.unit_quaternions(np.random.default_rng(num_tracks), (num_samples, num_tracks))

    def edge(k, kind):
        exact = F32(k) * INV_255
        return (exact, np.nextafter(exact, F32(0.0)), np.nextafter(exact, F32(1.0)), F32(k) / F32(255.0))[kind]
    for b in range(num_tracks):
        for c in range(3):
            index = 3 * b + c
            k_low = (7 * index) % 200 + 1
            low, high = edge(k_low, index % 4), edge(min(k_low + 1 + index % 50, 255), (index // 4) % 4)
            samples[:start, b, 4 + c] = np.linspace(0.0, 1.0, start).astype(np.float32)
            samples[start:, b, 4 + c] = np.where(np.arange(num_samples - start) % 3 == 0, low, np.where(np.arange(num_samples - start) % 3 == 1, high, F32(0.5) * (low + high)))
    return samples


def triple_of(track, offset):
    """the (rotation, translation, scale) types mixed_clip() gives a track: the 27 triples in turn, from `offset`"""
    index = (track + offset) % 27
    return index // 9, (index // 3) % 3, index % 3


def mixed_clip(seed, num_samples, num_tracks, offset=0, default_pose=None, scales="mixed", close_loop=False):
    """samples float32 [S, T, 12] in which track b's rotation, translation and scale are DEFAULT, CONSTANT or ANIMATED as triple_of(b, offset)
    says -- every one of the 27 triples within 27 tracks, or within three clips of 9 tracks and more whose offsets are 9 apart --, each
    decision far from its precision for precision 0.01 and shell distance 3: an animated rotation is free, an animated translation within
    0.5 and an animated scale within 10 % of 1; a constant one is a fixed value of its own (a rotation of an odd track jitters by 1e-6
    about it, a constant scale is at least 5 % from 1); a default one is the default pose's. scales="default": every scale is the
    default (a clip without scale). close_loop: the last sample is the first."""
    rng = np.random.default_rng(12000 + seed)
    default_pose = np.tile(IDENTITY, (num_tracks, 1)) if default_pose is None else default_pose
    samples = np.zeros((num_samples, num_tracks, 12), dtype=np.float32)
    samples[:, :, 0:4] = lossy.raw_restatement.unit_quaternions(rng, (num_samples, num_tracks))
    samples[:, :, 4:7] = rng.uniform(-0.5, 0.5, size=(num_samples, num_tracks, 3))
    samples[:, :, 8:11] = rng.uniform(0.9, 1.1, size=(num_samples, num_tracks, 3))
    samples[:, :, 7] = rng.uniform(-9.0, 9.0, size=(num_samples, num_tracks))
    samples[:, :, 11] = rng.uniform(-9.0, 9.0, size=(num_samples, num_tracks))
    for track in range(num_tracks):
        rotation, translation, scale = triple_of(track, offset)
        if rotation != ANIMATED:
            about = (default_pose[track, 0:4] if rotation == DEFAULT else samples[0, track, 0:4]).astype(np.float64)
            jitter = about + (rng.standard_normal((num_samples, 4)) * 1.0e-6 if track % 2 else 0.0)
            samples[:, track, 0:4] = (jitter / np.linalg.norm(jitter, axis=-1, keepdims=True)).astype(np.float32)
        if translation != ANIMATED:
            samples[:, track, 4:7] = default_pose[track, 4:7] if translation == DEFAULT else samples[0, track, 4:7]
        if scale == CONSTANT and scales == "mixed":
            samples[:, track, 8:11] = default_pose[track, 8:11] * np.where(rng.uniform(size=3) < 0.5, F32(0.93), F32(1.06))
        elif scale == DEFAULT or scales != "mixed":
            samples[:, track, 8:11] = default_pose[track, 8:11]
    if close_loop:
        samples[-1] = samples[0]
    return samples


def gentle_clip(seed, num_samples, num_tracks, offset=0, scales="mixed"):
    """mixed_clip() with every ANIMATED sub-track replaced by a smooth small motion about the track's first sample: the low end of the
    rate table (rates 1 to 4 at precision 0.01 and shell distance 3), where white noise never lands. With u(i) = sin(phi + 2 pi f i / S),
    phi uniform in [0, 2 pi) and f in [0.5, 2]: a rotation is the first sample's, pre-multiplied by a turn of a u(i) about one fixed
    random axis, a in [0.01, 0.05] rad; a translation component is the first sample's plus A u(i), A in [0.03, 0.15]; a scale component is
    1 + B u(i), B in [0.01, 0.03]; one amplitude for a sub-track, phi and f drawn per component of a translation or a scale. 2 to 15 precisions at the
    shell: every sub-track stays clearly ANIMATED. Computed in float64, rounded to float32 once."""
    samples = mixed_clip(seed, num_samples, num_tracks, offset, scales=scales)
    rng = np.random.default_rng(500 + seed)
    steps = np.arange(num_samples, dtype=np.float64)

    def wave():
        phase, frequency = rng.uniform(0.0, 2.0 * np.pi), rng.uniform(0.5, 2.0)
        return np.sin(phase + 2.0 * np.pi * frequency * steps / num_samples)
    for track in range(num_tracks):
        rotation, translation, scale = triple_of(track, offset)
        if rotation == ANIMATED:
            axis = rng.standard_normal(3)
            axis /= np.linalg.norm(axis)
            half = 0.5 * rng.uniform(0.01, 0.05) * wave()
            x, y, z = (axis[:, None] * np.sin(half)).astype(np.float64)
            w = np.cos(half)
            first = samples[0, track, 0:4].astype(np.float64)
            first /= np.linalg.norm(first)
            fx, fy, fz, fw = first
            turned = np.stack([w * fx + x * fw + y * fz - z * fy, w * fy - x * fz + y * fw + z * fx, w * fz + x * fy - y * fx + z * fw, w * fw - x * fx - y * fy - z * fz], axis=1)
            samples[:, track, 0:4] = (turned / np.linalg.norm(turned, axis=1, keepdims=True)).astype(np.float32)
        if translation == ANIMATED:
            waves = np.stack([wave() for _ in range(3)], axis=1)
            samples[:, track, 4:7] = (samples[0, track, 4:7].astype(np.float64) + rng.uniform(0.03, 0.15) * waves).astype(np.float32)
        if scale == ANIMATED and scales == "mixed":
            waves = np.stack([wave() for _ in range(3)], axis=1)
            samples[:, track, 8:11] = (1.0 + rng.uniform(0.01, 0.03) * waves).astype(np.float32)
    return samples


def far_roots_clip(seed, num_samples, num_tracks, factor, offset=0, scales="mixed", parents=None):
    """mixed_clip() with the translation of every track that has no parent in `parents` (tree(seed, T) when None) multiplied by
    float32(factor): at 60 000 and more a root's translation cannot be held to 0.01 by anything but the last rates of the table, the
    raw samples among them. A track that HAS a parent keeps its translation: a long lever below a rotating parent turns the parent's
    last bit into an error above the precision, and the reference's own search is no longer stable under one ulp."""
    samples = mixed_clip(seed, num_samples, num_tracks, offset, scales=scales)
    parents = tree(seed, num_tracks) if parents is None else np.asarray(parents).astype(np.uint32)[:num_tracks]
    roots = np.flatnonzero(parents >= num_tracks)
    samples[:, roots, 4:7] = (samples[:, roots, 4:7].astype(np.float64) * float(np.float32(factor))).astype(np.float32)
    return samples


def raw_scale_clip(seed, num_samples):
    """(samples [S, 2, 12], parents, track_precisions): a root and a leaf, built by hand for ONE event of the bit rate search that no drawn
    input reaches -- its last pass meeting a link whose rotation and translation rates are equal and below 24 while its scale rate is a
    real 24 (the pass raises the smallest rate first, so a scale it raised itself reaches 24 last). Both precisions are 1e-9.
    The root: every rotation is (0, 0, 0, 1) or (1, 0, 0, 0) and every translation component 0 or one value, which every rate gives
    back exactly; its scales are uniform in [0, 1), whose small values no rate below the raw one gives back to 1e-9: the local phase
    ends on (1, 1, 24) with an error of 0. The leaf: a free rotation, which dropping w alone moves by more than 1e-9, nothing else
    animated: it cannot be met, and the last pass walks up to the root. Needs more than two samples (two samples are exact at rate 1).
    What it holds is that the branch is WALKED and the table is still the restatement's: the root's rotation and translation are exact
    at every rate, so raising either first ends on the same rates, and a kernel that compared the scale with `> 24` gives these bytes too."""
    rng = np.random.default_rng(700 + seed)
    samples = np.tile(IDENTITY, (num_samples, 2, 1))
    pick = rng.integers(0, 2, size=num_samples)
    pick[0:2] = (0, 1)
    samples[:, 0, 0:4] = np.array([[0, 0, 0, 1], [1, 0, 0, 0]], dtype=np.float32)[pick]
    samples[:, 0, 4:7] = pick[:, None] * rng.uniform(0.1, 0.5, size=3).astype(np.float32)
    samples[:, 0, 8:11] = rng.uniform(0.0, 1.0, size=(num_samples, 3))
    samples[:, 1, 0:4] = lossy.raw_restatement.unit_quaternions(rng, (num_samples,))
    return samples, np.array([NO_PARENT, 0], dtype=np.uint32), np.full(2, 1.0e-9, dtype=np.float32)


def triples_of(compressed):
    """the set of (rotation, translation, scale) type triples of a Compressed"""
    return {tuple(int(kind) for kind in compressed.types[:, b]) for b in range(compressed.types.shape[1])}


def long_default_rotation(num_samples=12):
    """One track, for a precision of 84 at a shell of 3, that tells the rotation AFTER ITS COMPACTION from the registered one in the
    scale test. A translation is added behind the rotation and cancels in its own test, and any unit rotation keeps lengths, so with a
    unit default the scale test differs in rounding only; this call uses the default rotation as given (the reference refuses a
    description whose rotation is not normalized: no reference blob exists for this case; kernels and restatement follow one
    arithmetic, so no margin is needed). The default is (0, 0, 0, 2.2): rtm::quat_mul_vector3 with it multiplies every length by 4.84.
    The samples' rotation is the identity and the scale's x alternates between 1 and 7: the rotation is 3 * 3.84 * 7 = 80.6 from that
    default at the shell, under 84, and becomes DEFAULT; the scale moves 18 under the identity, within the precision (it would be constant, and default), and 87.1 under
    the default rotation: ANIMATED. Returns (samples [S, 1, 12], default pose [1, 12])."""
    pose = IDENTITY[None].copy()
    pose[0, 3] = 2.2
    samples = np.tile(IDENTITY, (num_samples, 1, 1))
    samples[1::2, 0, 8] = 7.0
    return samples, pose
