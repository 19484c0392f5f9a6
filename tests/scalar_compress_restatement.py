"""What aclhip_compress_raw_scalar_tracks_batch computes -- acl::compress_track_list for float1f .. vector4f
(compression/impl/compress.scalar.impl.h:65-269 and the files it calls) -- restated on the CPU as numpy float32 element operations
(every operand is float32, nothing is evaluated in float64, no multiply-add is fused), in the order of the header's definition:

  step 1   the finite check over every float of the array
  step 2   the looping vote: |v[0] - v[S-1]| <= p_b for every track and component drops the last sample   (optimize_looping.scalar.h)
  step 3   ranges: min from 1e10, max from -1e10, SEQUENTIALLY in ascending sample order, the second operand winning a tie
           (track_range_impl.h:44-63; SSE minps / maxps), extent = max - min
  step 4   constant tracks: |extent[c]| < p_b for every component, strictly
  step 5   n = min((x - min) / extent, 1), 0 where extent < 1e-9                                       (normalize.scalar.h:44-76)
  step 6   the rate search from 23 down to 1, ended by the first rate that fails                          (quantize.scalar.h:84-160)
  step 7   the blob: headers, one byte per track, constants, ranges, the bit stream (most significant bit first), 15 zero bytes, the
           FNV-1a hash over [8, size)                                        (compress.scalar.impl.h:93-251, write_track_data_impl.h)

A helper, not a test file: tests/test_scalar_compress_oracle.py holds it to the reference's compressor on every byte,
tests/test_gpu_scalar_compress.py holds the kernels to it on every byte."""
import struct

import numpy as np

F32 = np.float32
COMPONENTS = {0: 1, 1: 2, 2: 3, 3: 4, 4: 4}      # acl::track_type8 float1f .. float4f, vector4f
RAW_RATE = 24
TAG_COMPRESSED_TRACKS = 0xAC11AC11
VERSION_LATEST = 10
WRAP_OPTIMIZED = 0x40000000
NOT_FINITE_MESSAGE = "Some samples are not finite"


def num_bits_at(rate):
    return 32 if rate == RAW_RATE else int(rate)


def fnv1a32(data):
    acc = 2166136261
    for byte in bytes(data):
        acc = ((acc ^ byte) * 16777619) & 0xFFFFFFFF
    return acc


def align4(value):
    return (value + 3) & ~3


def bound(track_type, num_tracks, num_samples):
    """aclhip_scalar_compress_bound"""
    if track_type not in COMPONENTS:
        return 0
    c = COMPONENTS[track_type]
    return (52 + align4(num_tracks) + 8 * c * num_tracks + 4 * c * num_tracks * num_samples + 15 + 15) & ~15


def sequential_range(values):
    """step 3 over values [S, T, C]: (min, extent) float32 [T, C]; the loop is the reference's, the operations are elementwise"""
    lo = np.full(values.shape[1:], 1.0e10, dtype=np.float32)
    hi = np.full(values.shape[1:], -1.0e10, dtype=np.float32)
    for x in values:
        lo = np.where(lo < x, lo, x)
        hi = np.where(hi > x, hi, x)
    with np.errstate(all="ignore"):
        return lo.astype(np.float32), (hi - lo).astype(np.float32)


def normalize(values, lo, extent):
    """step 5 over values [S, T, C]"""
    with np.errstate(all="ignore"):
        n = ((values - lo[None]) / extent[None]).astype(np.float32)
    n = np.where(n < F32(1.0), n, F32(1.0)).astype(np.float32)
    return np.where((extent < F32(0.000000001))[None], F32(0.0), n).astype(np.float32)


def quantize(n, rate):
    """q = round_symmetric(n * max_value) for n >= 0: float32 [...], and (max_value, inv)"""
    max_value = F32((1 << num_bits_at(rate)) - 1)
    inv = F32(1.0) / max_value
    q = np.floor((n * max_value).astype(np.float32) + F32(0.5)).astype(np.float32)
    return q, max_value, F32(inv)


def analyze(samples, precisions, looping_wrap=False, optimize_loops=False):
    """steps 1 - 6 over samples [S, T, C] with one precision per track. Returns a dict: num_samples (after the vote), wrap, and per track
    min [T, C], extent [T, C], constant [T], rate [T] (0 for a constant track). Raises ValueError on a non-finite sample."""
    samples = np.ascontiguousarray(samples, dtype=np.float32)
    num_samples, num_tracks, _ = samples.shape
    precisions = np.asarray(precisions, dtype=np.float32)
    assert precisions.shape == (num_tracks,)
    if not np.isfinite(samples).all():
        raise ValueError(NOT_FINITE_MESSAGE)

    wrap = bool(looping_wrap)
    if optimize_loops and not wrap and num_samples > 1:
        with np.errstate(all="ignore"):
            near = np.abs((samples[0] - samples[-1]).astype(np.float32)) <= precisions[:, None]
        if near.all():
            num_samples -= 1
            wrap = True
    values = samples[:num_samples]

    lo, extent = sequential_range(values)
    with np.errstate(all="ignore"):
        constant = (np.abs(extent) < precisions[:, None]).all(axis=1)
    n = normalize(values, lo, extent)

    # the search of every track at once: a track leaves at its first failing rate, so `searching` only ever shrinks
    rates = np.where(constant, 0, RAW_RATE).astype(np.uint8)
    searching = ~constant
    for rate in range(RAW_RATE - 1, 0, -1):
        if not searching.any():
            break
        q, _, inv = quantize(n, rate)
        with np.errstate(all="ignore"):
            d = (((q * inv).astype(np.float32) * extent[None]).astype(np.float32) + lo[None]).astype(np.float32)
            passes = (np.abs((values - d).astype(np.float32)) <= precisions[None, :, None]).all(axis=(0, 2))
        searching = searching & passes
        rates[searching] = rate
    return {"num_samples": num_samples, "wrap": wrap, "min": lo, "extent": extent, "constant": constant, "rate": rates, "normalized": n, "values": values}


def compress(samples, track_type, sample_rate, precision=1.0e-5, track_precisions=None, looping_wrap=False, optimize_loops=False):
    """steps 1 - 7: the blob as a uint8 array. `track_precisions` (one per track, at least num_tracks of them) replaces `precision`."""
    samples = np.ascontiguousarray(samples, dtype=np.float32)
    if samples.ndim == 2:
        samples = samples[:, :, None]
    num_tracks, c = samples.shape[1], samples.shape[2]
    assert COMPONENTS[track_type] == c
    if track_precisions is None:
        precisions = np.full(num_tracks, precision, dtype=np.float32)
    else:
        precisions = np.asarray(track_precisions, dtype=np.float32)[:num_tracks]
    a = analyze(samples, precisions, looping_wrap, optimize_loops)
    num_samples, rates, values = a["num_samples"], a["rate"], a["values"]

    metadata = bytes(int(r) for r in rates) + b"\0" * (align4(num_tracks) - num_tracks)
    constants = b"".join(values[0, b].tobytes() for b in range(num_tracks) if rates[b] == 0)
    ranges = b"".join(a["min"][b].tobytes() + a["extent"][b].tobytes() for b in range(num_tracks) if 1 <= rates[b] < RAW_RATE)

    # the bit stream: per sample, per animated track, per component, num_bits(rate) bits, most significant bit first
    animated = [b for b in range(num_tracks) if rates[b] != 0]
    widths = np.array([num_bits_at(rates[b]) for b in animated for _ in range(c)], dtype=np.int64)
    num_bits_per_frame = int(widths.sum())
    stream = b""
    if animated and num_samples != 0:
        words = np.zeros((num_samples, len(animated) * c), dtype=np.uint64)
        for k, b in enumerate(animated):
            if rates[b] == RAW_RATE:
                words[:, k * c:(k + 1) * c] = values[:, b].view(np.uint32)
            else:
                q, _, _ = quantize(a["normalized"][:, b], rates[b])
                words[:, k * c:(k + 1) * c] = q.astype(np.uint32)
        # every column of the frame as its bits, most significant first: [S, num_bits_per_frame], frames back to back
        columns = [((words[:, k:k + 1] >> np.arange(int(w) - 1, -1, -1, dtype=np.uint64)) & np.uint64(1)).astype(np.uint8) for k, w in enumerate(widths)]
        stream = np.packbits(np.concatenate(columns, axis=1).reshape(-1)).tobytes()
    assert len(stream) == (num_bits_per_frame * num_samples + 7) // 8

    constants_offset = 20 + len(metadata)
    ranges_offset = constants_offset + len(constants)
    animated_offset = ranges_offset + len(ranges)
    scalar_header = struct.pack("<5I", num_bits_per_frame, 20, constants_offset, ranges_offset, animated_offset)
    tracks_header = struct.pack("<IHBBIIfI", TAG_COMPRESSED_TRACKS, VERSION_LATEST, 0, track_type, num_tracks, num_samples, F32(sample_rate),
                                WRAP_OPTIMIZED if a["wrap"] else 0)
    body = tracks_header + scalar_header + metadata + constants + ranges + stream + b"\0" * 15
    size = 8 + len(body)
    blob = struct.pack("<II", size, fnv1a32(body)) + body
    return np.frombuffer(blob, dtype=np.uint8).copy()


def parse(blob):
    """what the tests read back out of a scalar blob: rates [T], and per quantized track (min, extent)"""
    blob = np.ascontiguousarray(blob, dtype=np.uint8)
    raw = blob.tobytes()
    _, _, _, track_type, num_tracks, num_samples, _, misc = struct.unpack_from("<IHBBIIfI", raw, 8)
    bits_per_frame, metadata, constants, ranges, animated = struct.unpack_from("<5I", raw, 32)
    c = COMPONENTS[track_type]
    rates = np.frombuffer(raw, dtype=np.uint8, count=num_tracks, offset=32 + metadata).copy()
    range_values = {}
    offset = 32 + ranges
    for b in range(num_tracks):
        if 1 <= rates[b] < RAW_RATE:
            range_values[b] = (np.frombuffer(raw, dtype=np.float32, count=c, offset=offset).copy(), np.frombuffer(raw, dtype=np.float32, count=c, offset=offset + 4 * c).copy())
            offset += 8 * c
    return {"track_type": track_type, "num_tracks": num_tracks, "num_samples": num_samples, "wrap": bool(misc & WRAP_OPTIMIZED), "num_bits_per_frame": bits_per_frame,
            "rates": rates, "ranges": range_values, "constants_offset": 32 + constants, "animated_offset": 32 + animated}


# ---- the cases the CPU and the GPU tests share ----------------------------------------------------------------------------------------------
SWEEP = ((1, 1), (2, 1), (2, 5), (3, 70), (37, 12), (65, 65), (130, 3))      # (S, T)
PRECISIONS = (0.0, 1.0e-5, 1.0e-4, 1.0e-2)
LAST_SAMPLES = ("equal", "near", "different")


def curves(seed, num_samples, num_tracks, c):
    """smooth curves plus noise: amplitudes from 1e-5 to 1e3 around offsets in [-10, 10], one amplitude per track"""
    rng = np.random.default_rng(seed)
    amplitude = 10.0 ** rng.uniform(-5.0, 3.0, size=(1, num_tracks, 1))
    offset = rng.uniform(-10.0, 10.0, size=(1, num_tracks, c))
    phase = rng.uniform(0.0, 6.28, size=(1, num_tracks, c))
    t = np.arange(num_samples, dtype=np.float64)[:, None, None]
    return (offset + amplitude * (np.sin(0.37 * t + phase) + 0.1 * rng.standard_normal((num_samples, num_tracks, c)))).astype(np.float32)


def with_last_sample(samples, how):
    """the looping vote's three cases: the last sample equal to the first, within 5e-5 of it, or left as it is"""
    out = samples.copy()
    if samples.shape[0] > 1 and how == "equal":
        out[-1] = out[0]
    elif samples.shape[0] > 1 and how == "near":
        out[-1] = out[0] + np.float32(4.0e-5) * np.where(np.arange(out[0].size).reshape(out[0].shape) % 2 == 0, 1, -1).astype(np.float32)
    return out


def amplitude_list(c, num_samples=37):
    """tracks of amplitudes 0, 5e-5, 1e-3 ... 3e7 around offsets: constant tracks, rates from low to high and raw tracks in one blob"""
    amplitudes = np.array([0.0, 5.0e-5, 1.0e-3, 3.0e-3, 1.0e-2, 0.1, 1.0, 30.0, 1.0e3, 3.0e4, 1.0e6, 3.0e7, 0.0, 2.0e-2, 100.0, 300.0, 3.0], dtype=np.float64)
    rng = np.random.default_rng(4242 + c)
    t = np.arange(num_samples, dtype=np.float64)[:, None, None]
    offset = rng.uniform(-3.0, 3.0, size=(1, amplitudes.size, c))
    return (offset + amplitudes[None, :, None] * np.sin(0.29 * t + rng.uniform(0, 6.28, size=(1, amplitudes.size, c)))).astype(np.float32)


def special_list(c, num_samples=19):
    """exactly representable low-bit values; an extent near 1e-30; a minimum and a maximum made of +0 and -0 mixed; values beyond 1e10
    (the start values of the range take part), below -1e10, and a plain curve between them"""
    rng = np.random.default_rng(977 + c)
    s = np.arange(num_samples)
    tracks = []
    tracks.append(np.repeat(((s * 5) % 8).astype(np.float32)[:, None], c, axis=1))                              # 0 .. 7: exact at 3 bits
    tracks.append(np.repeat((np.float32(1.0e-30) * (1 + (s % 3)).astype(np.float32))[:, None], c, axis=1))      # extent 2e-30
    zeros = np.where(s % 2 == 0, np.float32(0.0), np.float32(-0.0)).astype(np.float32)
    low = np.where(s % 3 == 0, zeros, np.float32(1.5) + (s % 5).astype(np.float32)).astype(np.float32)          # minimum: zeros of both signs
    high = np.where(s % 3 == 1, zeros[::-1], np.float32(-2.5) - (s % 4).astype(np.float32)).astype(np.float32)  # maximum: zeros of both signs
    tracks.append(np.repeat(low[:, None], c, axis=1))
    tracks.append(np.repeat(high[:, None], c, axis=1))
    tracks.append(np.repeat((np.float32(3.0e10) + np.float32(1.0e9) * (s % 7).astype(np.float32))[:, None], c, axis=1))
    tracks.append(np.repeat((np.float32(-3.0e10) - np.float32(1.0e9) * (s % 7).astype(np.float32))[:, None], c, axis=1))
    tracks.append(rng.uniform(-1.0, 1.0, size=(num_samples, c)).astype(np.float32))
    out = np.stack(tracks, axis=1).astype(np.float32)
    if c > 1:
        out[:, 2, 1] = -out[:, 2, 1] * np.float32(0.5)      # the components of a track differ: another sign pattern in component 1
    return out
