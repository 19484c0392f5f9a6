"""Clips whose STORED samples are not finite: the poison builder of test_nonfinite_samples_oracle.py (oracle against the reference,
no GPU) and test_gpu_nonfinite_samples.py (every clip decode launch against the oracle).

A stored sample is found without layout arithmetic: the decoder returns a raw width sample unchanged at its exact key time under
never-normalize, so the big endian image of that value is searched for in the blob's bit string (np.unpackbits) and must occur exactly
once; constants are searched as the little endian floats the constant stream holds. One 32 bit word of the hit is then overwritten,
at whatever bit offset it lies. Every poisoned clip carries several poisons on different tracks: the first and the last located
ordinal of every pose window, the ordinals on both sides of a 64 lane decode pass, each sub-track kind, and constants.

NaN sign and payload differ between x86 and the GPU, so results are compared with same_numbers_and_nans: equal bits
where the expected word is a number, a NaN where it is a NaN. check_expectation asserts on the EXPECTED values alone that this
exemption stays small and lies where the poisons are."""
import numpy as np

from acl_amd import synth
from oracle import bindings as ob
import helpers

POISON_WORDS = [
    0x7FC00000, 0xFFC00000,     # the quiet NaNs
    0xFFC00001,                 # the "default sub-track, W = 1" marker of the LDS image
    0xFFE00003,                 # an "animated sub-track" marker
    0xFFFFFFFF,
    0x7F800001, 0xFF800001,     # signalling NaNs
    0x7F800000, 0xFF800000,     # infinities
    0x7F7FFFFF,                 # its square overflows
    0x00000001,                 # a denormal: its square underflows
    0x80000000,                 # -0.0
]
NO_PARENT = 0xFFFFFFFF
WINDOW_TRACKS = 104             # k_image_chunk_quads / 3
PASS_LANES = 64
NAN_WORD_CAP = 0.05
SKIP_FILL = np.float32(-7777.25)

# (name, corpus clip or synthetic spec, variants). A variant shifts which poison word goes to which placement.
CORPUS_SOURCES = ["025_raw_33x33", "151_bones_105_raw", "049_drop_w_full_33x33", "033_mixed_var_0_33x33", "206_metadata_raw"]     # (the last one: bind pose defaults in its metadata)
SYNTHETIC_SOURCES = {
    # variable formats with raw bit rate sub-tracks (width 32, at arbitrary bit offsets), scale, two pose windows
    "synthetic_105": dict(seed=32, num_tracks=105, num_samples=45, has_scale=1, raw_fraction=0.1),
    # mostly raw and animated, more than 64 animated sub-tracks in its first window; it wraps: the interval behind its last sample
    # interpolates towards the first one
    "synthetic_140": dict(seed=77, num_tracks=140, num_samples=40, has_scale=1, wrap=1, raw_fraction=0.6, rotation_default=0.05, rotation_constant=0.1,
                          translation_default=0.1, translation_constant=0.3, scale_default=0.3, scale_constant=0.2),
}
VARIANTS = {"025_raw_33x33": 12, "049_drop_w_full_33x33": 6, "033_mixed_var_0_33x33": 4, "151_bones_105_raw": 3, "206_metadata_raw": 1, "synthetic_105": 3, "synthetic_140": 4}


def is_nan_word(word):
    return (word & 0x7F800000) == 0x7F800000 and (word & 0x007FFFFF) != 0


def words(array):
    return np.ascontiguousarray(array, dtype=np.float32).view(np.uint32)


def nan_mask(array):
    return np.isnan(np.asarray(array, dtype=np.float32))


def same_numbers_and_nans(got, want):
    """where `want` is a number the bits are equal; where `want` is a NaN, `got` is a NaN (of any sign and payload)"""
    got, want = np.asarray(got, dtype=np.float32), np.asarray(want, dtype=np.float32)
    if got.shape != want.shape:
        return False
    nans = nan_mask(want)
    return bool(np.isnan(got[nans]).all() and np.array_equal(words(got)[~nans], words(want)[~nans]))


def nan_sign_decided(want):
    """[..., 12] mask of the words a NaN's SIGN decides under never-normalize: the number lanes of a rotation that has a NaN lane.
    quat_lerp_no_normalization flips its end key by the sign BIT of dot(start, end) (math/quatf.h:73,182), and that dot is a NaN here.
    Which sign a NaN comes out of a multiply-add chain with depends on the operand order the compiler picked, on x86 as on the GPU
    (DESIGN 4.4): the reference itself does not define these words. Every other setting normalizes such a rotation into four NaNs."""
    want = np.asarray(want, dtype=np.float32)
    decided = np.zeros(want.shape, dtype=bool)
    decided[..., 0:4] = nan_mask(want[..., 0:4]).any(axis=-1, keepdims=True) & ~nan_mask(want[..., 0:4])
    return decided


def same_numbers_and_nans_never_normalized(got, want):
    """same_numbers_and_nans over [..., 12] poses decoded with never-normalize: the words nan_sign_decided names are not compared"""
    got, want = np.asarray(got, dtype=np.float32), np.asarray(want, dtype=np.float32)
    if got.shape != want.shape:
        return False
    free = nan_sign_decided(want)
    return same_numbers_and_nans(np.where(free, np.float32(0.0), got), np.where(free, np.float32(0.0), want))


def describe_difference(got, want):
    got, want = np.asarray(got, dtype=np.float32), np.asarray(want, dtype=np.float32)
    nans = nan_mask(want)
    bad = np.where(nans, ~np.isnan(got), words(got) != words(want))
    where = np.argwhere(bad)
    first = tuple(where[0]) if where.size else None
    return f"{int(bad.sum())} words differ, first at {first}: got {got[first] if first else None!r} (0x{int(words(got)[first]) if first else 0:08X}), want {want[first] if first else None!r}"


# ---- locating and patching ------------------------------------------------------------------------------------------------------------
def blob_bits(blob):
    return np.unpackbits(blob).tobytes()


def find_all(haystack, needle):
    hits, at = [], haystack.find(needle)
    while at >= 0 and len(hits) < 3:
        hits.append(at)
        at = haystack.find(needle, at + 1)
    return hits


def locate_sample(bits, value, num_floats):
    """the bit offset of the big endian image of value[:num_floats], or None unless it occurs exactly once"""
    image = np.unpackbits(np.frombuffer(np.asarray(value[:num_floats], dtype=">f4").tobytes(), dtype=np.uint8)).tobytes()
    hits = find_all(bits, image)
    return hits[0] if len(hits) == 1 else None


def locate_constant(blob_bytes, value, num_floats):
    hits = find_all(blob_bytes, np.asarray(value[:num_floats], dtype="<f4").tobytes())
    return hits[0] * 8 if len(hits) == 1 else None


def write_word(blob, bit_offset, word, little_endian=False):
    """32 bits at ANY bit offset of the blob (most significant bit first, like the animated stream), or a little endian word of the constant stream"""
    if little_endian:
        assert bit_offset % 8 == 0
        blob[bit_offset // 8: bit_offset // 8 + 4] = np.frombuffer(np.array([word], dtype="<u4").tobytes(), dtype=np.uint8)
        return
    first_byte, last_byte = bit_offset // 8, (bit_offset + 32 + 7) // 8
    bits = np.unpackbits(blob[first_byte:last_byte])
    start = bit_offset - first_byte * 8
    bits[start: start + 32] = np.unpackbits(np.frombuffer(np.array([word], dtype=">u4").tobytes(), dtype=np.uint8))
    blob[first_byte:last_byte] = np.packbits(bits)


# ---- what a clip holds ----------------------------------------------------------------------------------------------------------------
def key_frames_of(blob, num_tracks):
    """(key times, duration, values [num key times, num_tracks, 12] at the exact key times under never-normalize with the defaults
    skipped over SKIP_FILL): a raw width sample comes back unchanged"""
    times, duration = helpers.corpus_sample_times(blob)
    options = helpers.oracle_options(5, 1)
    keys = np.stack([ob.oracle_decompress_tracks(blob, float(t), ob.ROUND_NONE, options, out=np.full((num_tracks, 12), SKIP_FILL, dtype=np.float32)) for t in times])
    return times, duration, keys


def classify(keys):
    """[num_tracks, 3] of "default" / "constant" / "animated" from the decoded key frames"""
    num_tracks = keys.shape[1]
    kinds = np.empty((num_tracks, 3), dtype=object)
    fill = words(SKIP_FILL.reshape(1))[0]
    for track in range(num_tracks):
        for kind in range(3):
            values = words(keys[:, track, kind * 4: kind * 4 + (4 if kind == 0 else 3)])
            if (values[:, :3] == fill).all():
                kinds[track, kind] = "default"
            elif (values == values[0]).all():
                kinds[track, kind] = "constant"
            else:
                kinds[track, kind] = "animated"
    return kinds


def animated_ordinals(kinds):
    """{(track, kind): (window, ordinal in the window)} as registration numbers the animated sub-tracks of a pose window: rotations
    first, then translations and scales in quad order (host_clips.inl, "animated sub-tracks in POSE order")"""
    out = {}
    num_tracks = kinds.shape[0]
    for window in range(-(-num_tracks // WINDOW_TRACKS)):
        tracks = range(window * WINDOW_TRACKS, min((window + 1) * WINDOW_TRACKS, num_tracks))
        ordered = [(t, 0) for t in tracks if kinds[t, 0] == "animated"] + [(t, k) for t in tracks for k in (1, 2) if kinds[t, k] == "animated"]
        for ordinal, sub_track in enumerate(ordered):
            out[sub_track] = (window, ordinal)
    return out


class Poison:
    def __init__(self, track, kind, lane, frames, word, constant):
        self.track, self.kind, self.lane, self.frames, self.word, self.constant = track, kind, lane, tuple(frames), word, constant
        self.window = self.ordinal = None

    @property
    def makes_nan(self):
        return is_nan_word(self.word)

    def __repr__(self):
        where = "constant" if self.constant else f"frames {self.frames} ordinal {self.window}:{self.ordinal}"
        return f"<0x{self.word:08X} track {self.track} kind {self.kind} lane {self.lane} {where}>"


class PoisonedClip:
    def __init__(self, name, clean, blob, poisons, times, duration, parents, wraps):
        self.name, self.clean, self.blob, self.poisons, self.times, self.duration, self.parents, self.wraps = name, clean, blob, poisons, times, duration, parents, wraps
        self.num_tracks = int(ob.oracle().aclo_num_tracks(blob.ctypes.data))
        self.sub_tracks = sorted({(p.track, p.kind) for p in poisons})
        self.tracks = sorted({p.track for p in poisons})

    def descendants(self, parents=None):
        """the poisoned tracks and every track below one, under `parents` (the clip's test hierarchy by default)"""
        parents = self.parents if parents is None else parents
        below = np.zeros(self.num_tracks, dtype=bool)
        below[self.tracks] = True
        for track in range(self.num_tracks):                # parents first
            if parents[track] != NO_PARENT and below[parents[track]]:
                below[track] = True
        return below

    def __repr__(self):
        return f"{self.name}: {self.poisons}"


def _interior_times(times, frames, duration):
    out = []
    last = len(times) - 1
    for k in frames:
        near = [np.float32(times[min(max(i, 0), last)]) for i in (k - 1, k, k + 1, k + 2)]
        out += near
        out += [np.float32((np.float64(near[0]) + np.float64(near[1])) / 2), np.float32((np.float64(near[1]) + np.float64(near[2])) / 2)]
    return out


def leaf_hierarchy(num_tracks, poisoned_tracks, seed):
    """A forest, parents first, in which every poisoned track is a leaf -- but the first, which gets a chain of two bones below it:
    a NaN then spreads to a small known subtree only. Returns (parents, the bone with the subtree)."""
    rng = np.random.default_rng(seed)
    poisoned = set(poisoned_tracks)
    parents = np.full(num_tracks, NO_PARENT, dtype=np.uint32)
    clean = []
    for track in range(num_tracks):
        if clean and rng.uniform() > 0.06:
            parents[track] = clean[int(rng.integers(max(0, len(clean) - 9), len(clean)))]
        if track not in poisoned:
            clean.append(track)
    with_subtree = None
    for track in poisoned_tracks:                           # (in the caller's order: it names animated poisons first)
        below = [t for t in range(track + 1, num_tracks) if t not in poisoned][:2]
        if len(below) == 2:
            parents[below[0]], parents[below[1]] = track, below[0]
            # (nothing else hangs off these two: re-parent their children to the root they came from)
            for t in range(below[0] + 1, num_tracks):
                if t != below[1] and parents[t] in (below[0], below[1]):
                    parents[t] = NO_PARENT
            with_subtree = track
            break
    return parents, with_subtree


def build_poisoned(name, clean, variant=0, looping=False):
    """One poisoned copy of `clean` (a 16 byte aligned blob). Raises if the clip holds nothing that can be located."""
    num_tracks = int(ob.oracle().aclo_num_tracks(clean.ctypes.data))
    times, duration, keys = key_frames_of(clean, num_tracks)
    num_stored = len(times) - (1 if looping else 0)        # a wrapping clip's last key time repeats its first sample
    kinds = classify(keys[:num_stored])
    ordinals = animated_ordinals(kinds)
    bits, blob_bytes = blob_bits(clean), clean.tobytes()
    interior = num_stored // 2
    frame_patterns = [(interior,), (interior, interior + 1), (0, num_stored - 1)]

    all_frames = sorted({k for pattern in frame_patterns for k in pattern})
    memo = {}

    def located(sub_track):
        """(bit offsets of the sub-track's sample in every frame of all_frames, the floats it stores), or None if one is not found exactly once"""
        if sub_track not in memo:
            track, kind = sub_track
            memo[sub_track] = None
            for num_floats in ((4, 3) if kind == 0 else (3,)):
                offsets = []
                for k in all_frames:
                    offsets.append(locate_sample(bits, keys[k, track, kind * 4: kind * 4 + 4], num_floats))
                    if offsets[-1] is None:
                        break
                if offsets[-1] is not None and len(set(offsets)) == len(offsets):
                    memo[sub_track] = (offsets, num_floats)
                    break
        return memo[sub_track]

    chosen = []                                             # (track, kind), in priority order; one sub-track per TRACK

    def take(candidates):
        for sub_track in candidates:
            if all(sub_track[0] != other[0] for other in chosen) and located(sub_track) is not None:
                chosen.append(sub_track)
                return

    by_window = {}
    for sub_track, (window, ordinal) in ordinals.items():
        by_window.setdefault(window, []).append((ordinal, sub_track))
    for window in sorted(by_window, reverse=True):          # (the second window first: its tracks are few)
        ordered = [sub_track for _, sub_track in sorted(by_window[window])]
        take(ordered)                                       # the first located ordinal of the window
        take(ordered[::-1])                                 # the last
        if len(ordered) > PASS_LANES:
            take(ordered[PASS_LANES - 1:: -1])              # ordinal 63, or the nearest located one below
            take(ordered[PASS_LANES:])                      # ordinal 64, or the nearest above
    every = [sub_track for _, sub_track in sorted((ordinals[s], s) for s in ordinals)]
    for kind in (0, 1, 2, 0):
        take([s for s in every[variant % 3:] if s[1] == kind])
    if not chosen:
        raise ValueError(f"{name}: no stored sample of a raw width found")
    budget = max(4, num_tracks // 10)               # about one poisoned sub-track per ten tracks (plus two constants)
    # a small clip keeps its first placement (the first ordinal: over the variants it meets every word); the variant rotates the others
    if len(chosen) > budget:
        rest = chosen[1:]
        shift = variant % len(rest)
        chosen = chosen[:1] + (rest[shift:] + rest[:shift])[:budget - 1]

    blob = synth.aligned_bytes(clean.size)
    blob[:] = clean
    poisons = []
    for slot, (track, kind) in enumerate(chosen):
        offsets, num_floats = located((track, kind))
        frames = frame_patterns[(slot + variant) % 3]
        if kind == 0:
            lane = (3 if track % 2 == 0 else 0) if num_floats == 4 else (slot + variant) % 3      # W or x of a quatf_full, else x, y or z
        else:
            lane = (slot + variant) % 3
        poison = Poison(track, kind, lane, frames, POISON_WORDS[(slot * 5 + variant) % len(POISON_WORDS)], constant=False)
        poison.window, poison.ordinal = ordinals[(track, kind)]
        for k in frames:
            write_word(blob, offsets[all_frames.index(k)] + 32 * lane, poison.word)
        poisons.append(poison)

    # constants: one rotation stored whole (quatf_full: its W is in the stream) and one translation
    taken_tracks = {p.track for p in poisons}
    for kind, num_floats, lane in ((0, 4, 3 if variant % 4 < 2 else 0), (1, 3, variant % 3)):
        if num_tracks < 100 and kind != variant % 2:       # (a constant is a NaN at every sample time: a small clip carries one of the two)
            continue
        for track in range(num_tracks):
            if kinds[track, kind] != "constant" or track in taken_tracks:
                continue
            offset = locate_constant(blob_bytes, keys[0, track, kind * 4: kind * 4 + 4], num_floats)
            if offset is None:
                continue
            poison = Poison(track, kind, lane, (), POISON_WORDS[(len(poisons) * 5 + variant) % len(POISON_WORDS)], constant=True)
            write_word(blob, offset + 32 * lane, poison.word, little_endian=True)
            poisons.append(poison)
            taken_tracks.add(track)
            break

    sample_times = [np.float32(0.0), np.float32(duration)]
    for pattern in frame_patterns:
        sample_times += _interior_times(times, pattern, duration)
    if looping:
        sample_times.append(np.float32((np.float64(times[num_stored - 1]) + np.float64(duration)) / 2))       # inside the wrap interval
    sample_times = np.unique(np.array(sample_times, dtype=np.float32))
    parents, _ = leaf_hierarchy(num_tracks, [p.track for p in poisons], seed=num_tracks + variant)
    return PoisonedClip(f"{name}#{variant}", clean, blob, poisons, sample_times, float(duration), parents, looping)


_cache = {}


def source_clips():
    """{name: (clean blob, looping)}"""
    if "sources" not in _cache:
        corpus = {clip["name"]: clip for clip in helpers.load_corpus()}
        sources = {name: (corpus[name]["blob"], False) for name in CORPUS_SOURCES}
        for name, spec in SYNTHETIC_SOURCES.items():
            sources[name] = (synth.build_clip(**spec).blob, bool(spec.get("wrap")))
        _cache["sources"] = sources
    return _cache["sources"]


def case_ids():
    return [f"{name}#{variant}" for name in CORPUS_SOURCES + sorted(SYNTHETIC_SOURCES) for variant in range(VARIANTS[name])]


def poisoned_clip(case_id):
    """the poisoned clip of one id of case_ids(), built once per process"""
    if case_id not in _cache:
        name, variant = case_id.rsplit("#", 1)
        clean, looping = source_clips()[name]
        _cache[case_id] = build_poisoned(name, clean, int(variant), looping)
    return _cache[case_id]


# ---- the expectation, on the expected values alone ------------------------------------------------------------------------------------
def check_expectation(clip, want, object_space=False, parents=None, extra_sub_tracks=(), need_every_nan=True, never_normalized=False):
    """want: [num times, num_tracks, 12] expected values of the poisoned clip over clip.times (or [..., num_tracks, 12] of any batch that
    covers them). Its NaN words lie only in the poisoned sub-tracks (object space: in the poisoned tracks and their descendants), every
    NaN-word poison shows as a NaN somewhere, and the NaN words (never_normalized: and the words nan_sign_decided exempts) stay below
    5 % of what is compared."""
    want = np.asarray(want, dtype=np.float32).reshape(-1, clip.num_tracks, 12)
    nans = nan_mask(want)
    allowed = np.zeros((clip.num_tracks, 12), dtype=bool)
    if object_space:
        allowed[clip.descendants(parents)] = True
    else:
        for track, kind in list(clip.sub_tracks) + list(extra_sub_tracks):
            allowed[track, kind * 4: kind * 4 + 4] = True
    stray = nans & ~allowed[None]
    assert not stray.any(), f"{clip.name}: NaN words outside the poisoned sub-tracks at {np.argwhere(stray)[:6].tolist()}"
    if need_every_nan:
        for poison in clip.poisons:
            if poison.makes_nan:
                lanes = slice(0, 12) if object_space else slice(poison.kind * 4, poison.kind * 4 + 4)
                assert nans[:, poison.track, lanes].any(), f"{clip.name}: {poison} shows in no expected value"
    if never_normalized:
        nans = nans | nan_sign_decided(want)                # (words that are not compared either: they count)
    fraction = nans[..., helpers.XYZ_LANES].mean() if nans.size else 0.0
    assert fraction < NAN_WORD_CAP, f"{clip.name}: {fraction:.3%} of the expected words are NaNs"
    return float(fraction)
