"""What aclhip_find_bit_rates_batch computes -- find_optimal_bit_rates (compression/impl/quantize.transform.h:1174-1523) at the levels
lowest, low and medium, for quatf_drop_w_variable / vector3f_variable / vector3f_variable and the qvvf error metric -- restated on the
CPU with numpy float32 element operations (single, correctly rounded IEEE operations; nothing is evaluated in float64), in the order of
the header's definition:

  steps 0 - 8  tests/variable_compress_restatement.py: everything up to the segment ranges
  S1           the sample a rate stands for: a pure function of (sub-track, sample, rate); no cache is rebuilt
  S2           the local and the object error at the track's rigid shell, with the two scan rules
  S3           the local phase over the permutation lists, generated here from their ordering rule
  S4           the object phase over the tracks in parent-first order

find_bit_rates() returns the table uint8 [G, T, 4] { rotation, translation, scale, 0 } (255 for a sub-track that is not animated) and,
per (segment, track), the object error over the whole segment at the final rates and whether it is below the track's precision.
The permutations and samples of a size class are evaluated at once; object transforms are kept per (track, rates of its chain).
A helper, not a test file: tests/test_bit_rate_search_oracle.py holds it to the reference's compressor,
tests/test_gpu_bit_rate_search.py holds the kernels to it on every byte."""
import collections
import itertools

import numpy as np

import variable_compress_restatement as variable
from variable_compress_restatement import ANIMATED, CONSTANT, DEFAULT, F32, IDENTITY, INV_65535, NO_PARENT, RAW_RATE, XYZ, f32, lossy  # noqa: F401

INVALID_RATE = 255
NUM_RATES = 25
BITS = np.array(list(range(24)) + [32], dtype=np.int64)       # core/impl/variable_bit_rates.h: the bits of a component at rate r
LEVELS = {"lowest": 0, "low": 1, "medium": 2, "high": 3, "highest": 4}
UNTIL_ERROR_TOO_HIGH, UNTIL_END_OF_SEGMENT = 0, 1
ONES = np.ones(3, dtype=np.float32)


def permutation_list(num_kinds):
    """The reference's k_local_bit_rate_permutations_{1,2,3}_dof from the rule its generator states: every tuple of `num_kinds` rates of
    0 .. 24, sorted by the bits of the transform (the sum of the three components of every kind), then by the rates themselves, the
    first kind first. Returns (uint8 [25 ** num_kinds, num_kinds], the bits of a component summed over the kinds)."""
    tuples = sorted((3 * int(BITS[list(rates)].sum()), rates) for rates in itertools.product(range(NUM_RATES), repeat=num_kinds))
    rates = np.array([entry[1] for entry in tuples], dtype=np.uint8)
    return rates, BITS[rates].sum(axis=1)


_PERMUTATIONS = {}


def permutations(num_kinds):
    if num_kinds not in _PERMUTATIONS:
        _PERMUTATIONS[num_kinds] = permutation_list(num_kinds)
    return _PERMUTATIONS[num_kinds]


def parent_first(parents, num_tracks):
    """sorted_transforms_parent_first (clip_context.impl.h:57-80): by parent index + 1 in 32 bits (no parent: 0), then by own index"""
    keys = [((int(parents[b]) + 1) & 0xFFFFFFFF if int(parents[b]) < num_tracks else 0, b) for b in range(num_tracks)]
    return [b for _, b in sorted(keys)]


def from_positive_w(xyz):
    """rtm::quat_from_positive_w then rtm::quat_normalize, over float32 [..., 3]"""
    x, y, z = xyz[..., 0], xyz[..., 1], xyz[..., 2]
    w = np.sqrt(np.abs(((F32(1.0) - x * x) - y * y) - z * z))
    return lossy.normalize(np.concatenate([xyz, w[..., None]], axis=-1).astype(np.float32))


def error_of(distance, raw, lossy_transform, has_scale):
    """calculate_error (three points) or calculate_error_no_scale (the x and y points, no scale: transform_error_metrics.h:360-378)"""
    if has_scale:
        return variable.shell_error(distance, raw, lossy_transform)
    errors = []
    with np.errstate(invalid="ignore", over="ignore"):
        for point in lossy.shell_points(distance)[0:2]:
            d = lossy.mul_point3(point, lossy_transform[0], lossy_transform[1], ONES) - lossy.mul_point3(point, raw[0], raw[1], ONES)
            errors.append(np.sqrt(((d[..., 0] * d[..., 0]) + (d[..., 1] * d[..., 1])) + (d[..., 2] * d[..., 2])))
    return f32(lossy.greater(errors[0], errors[1]))


def to_object(local, parent, has_scale):
    """qvv_normalize(qvv_mul(local, parent)) or its _no_scale twin, the quaternion path"""
    rotation = lossy.normalize(lossy.quat_mul(local[0], parent[0]))
    translation = f32(lossy.mul_point3(local[1], parent[0], parent[1], parent[2] if has_scale else ONES))
    return rotation, translation, f32(local[2] * parent[2]) if has_scale else np.broadcast_to(ONES, local[2].shape)


def scan(errors, threshold, stop):
    """the maximum a scan returns, from 0.0F: over all samples, or up to and including the first whose error is >= threshold.
    errors float32 [..., count]"""
    if stop == UNTIL_ERROR_TOO_HIGH:
        high = errors >= threshold
        first = np.where(high.any(axis=-1), high.argmax(axis=-1), errors.shape[-1] - 1)
        errors = np.where(np.arange(errors.shape[-1]) <= first[..., None], errors, F32(0.0))
    return np.maximum(errors.max(axis=-1), F32(0.0)).astype(np.float32)


# what Search.visits counts
VISITS = ("local_not_met",                  # S3 went through a track's whole permutation list and no entry was below the threshold
          "local_picked_raw",               # S3's winner holds a 24: the row of raw samples
          "increment_reached_raw",          # increment() took a real rate (one below 24) to 24; never the 255 of a sub-track that is not animated
          "link_maxed_out",                 # the last pass left a link that has an animated sub-track at three rates of 24 (or 255)
          "chain_maxed_out",                # ... and every link of the chain: the pass ends above the threshold
          "scale_raw_translation_bump",     # "rotation == translation, scale already raw" with a real scale rate of 24
          "ancestor_improved",              # the increment the first loop kept was on a link above the target
          "no_progress")                    # the first loop ended because no single increment lowered the error


class Search:
    """table uint8 [G, T, 4]; local_table: the same behind the local phase; errors float32 [G, T]; met bool [G, T]; base: the Compressed
    of variable_compress_restatement at the table; evaluations: how many object errors were measured; visits: a collections.Counter of
    the edges the search went over, by name (VISITS) -- a record beside the search: nothing is decided from it"""


def find_bit_rates(samples, sample_rate, default_pose=None, parents=None, flags=0, precision=1.0e-4, shell_distance=1.0, track_precisions=None,
                   track_shell_distances=None, looping_wrap=False, max_samples=None, level="medium"):
    """samples float32 [S, T, 12] QVV48; the settings as variable_compress_restatement.compress. Raises what that raises."""
    level = LEVELS.get(level, level)
    if level not in (0, 1, 2):
        raise ValueError("level %r is not built" % (level,))
    samples = f32(samples)
    num_tracks = samples.shape[1]
    settings = dict(default_pose=default_pose, parents=parents, flags=flags, precision=precision, shell_distance=shell_distance, track_precisions=track_precisions,
                    track_shell_distances=track_shell_distances, looping_wrap=looping_wrap, max_samples=max_samples)
    base = variable.compress(samples, sample_rate, (8, 8, 8), **settings)       # steps 0 - 8 (the rates do not enter them)
    default_pose = np.tile(IDENTITY, (num_tracks, 1)) if default_pose is None else f32(default_pose)[:num_tracks]
    table_parents = np.full(num_tracks, NO_PARENT, dtype=np.uint32) if parents is None else np.asarray(parents).astype(np.uint32)[:num_tracks]
    parent_of = [int(p) if int(p) < num_tracks else -1 for p in table_parents]
    kept = samples[:base.num_samples].copy()
    kept[:, :, 0:4] = lossy.positive_w(lossy.normalize(kept[:, :, 0:4]))
    types = base.types
    precisions = np.full(num_tracks, precision, dtype=np.float32) if track_precisions is None else f32(track_precisions)[:num_tracks]
    distances = np.full(num_tracks, shell_distance, dtype=np.float32) if track_shell_distances is None else f32(track_shell_distances)[:num_tracks]
    has_scale = bool((types[2] != DEFAULT).any())
    multiple = len(base.segments) > 1
    order = parent_first(table_parents, num_tracks)
    chains = []
    for b in range(num_tracks):
        chain = [b]
        while parent_of[chain[-1]] >= 0:
            chain.append(parent_of[chain[-1]])
        chains.append(chain[::-1])          # from the root to b

    out = Search()
    out.base = base
    out.table = np.full((len(base.segments), num_tracks, 4), INVALID_RATE, dtype=np.uint8)
    out.table[:, :, 3] = 0
    out.local_table = out.table.copy()
    out.errors = np.zeros((len(base.segments), num_tracks), dtype=np.float32)
    out.met = np.zeros((len(base.segments), num_tracks), dtype=bool)
    out.evaluations = 0
    visits = out.visits = collections.Counter()
    out.shells = np.zeros((len(base.segments), num_tracks, 2), dtype=np.float32)

    for g, (start, count) in enumerate(base.segments):
        rows = slice(start, start + count)
        # S1: per animated sub-track the value at every rate [25, count, 3 or 4]; the others once
        values = {}
        stored = np.zeros((count, num_tracks, 12), dtype=np.float32)       # what the segment's streams hold: S0
        for kind in range(3):
            for b in range(num_tracks):
                if types[kind, b] == DEFAULT:
                    fixed = default_pose[b, variable.LANES[kind]]
                    stored[:, b, XYZ[kind]] = default_pose[b, XYZ[kind]]
                elif types[kind, b] == CONSTANT:
                    fixed = lossy.normalize(kept[0, b, 0:4]) if kind == 0 else kept[0, b, XYZ[kind]]
                    stored[:, b, XYZ[kind]] = kept[0, b, XYZ[kind]]
                else:
                    clip_min, clip_extent = base.clip_ranges[kind, b]
                    clip_normalized = variable.normalize_in(kept[:, b, XYZ[kind]], clip_min, clip_extent)
                    normalized = clip_normalized[rows]
                    if multiple:
                        segment_min, segment_extent = base.segment_ranges[kind, b, g]
                        normalized = variable.normalize_in(normalized, segment_min, segment_extent)
                    stored[:, b, XYZ[kind]] = normalized
                    at_rates = np.zeros((NUM_RATES, count, 3), dtype=np.float32)
                    for rate in range(1, RAW_RATE):
                        most = F32((1 << rate) - 1)
                        decayed = f32(np.floor(normalized * most + F32(0.5)) * (F32(1.0) / most))
                        if multiple:
                            decayed = f32(f32(decayed * segment_extent) + segment_min)
                        at_rates[rate] = f32(f32(decayed * clip_extent) + clip_min)
                    decayed = f32(np.floor(clip_normalized[start] * F32(65535.0) + F32(0.5)) * INV_65535)
                    at_rates[0] = f32(f32(decayed * clip_extent) + clip_min)
                    at_rates[RAW_RATE] = kept[rows, b, XYZ[kind]]
                    values[kind, b] = from_positive_w(at_rates) if kind == 0 else at_rates
                    continue
                values[kind, b] = np.tile(f32(fixed), (count, 1))

        # S0: the shell of the segment, from what its streams hold
        stored[:, :, 0:4] = from_positive_w(stored[:, :, 0:3])
        shells = out.shells[g] = lossy.rigid_shell(stored, table_parents, precisions, distances)

        def local_of(b, rates):
            """the S1 transform of track b at its three rates: (rotation [count, 4], translation [count, 3], scale [count, 3])"""
            return tuple(values[kind, b][int(rates[kind])] if types[kind, b] == ANIMATED else values[kind, b] for kind in range(3))

        raw_local = [(lossy.normalize(kept[rows, b, 0:4]), kept[rows, b, 4:7], kept[rows, b, 8:11]) for b in range(num_tracks)]
        raw_object = {}

        def raw_object_of(b):
            if b not in raw_object:
                raw_object[b] = raw_local[b] if parent_of[b] < 0 else to_object(raw_local[b], raw_object_of(parent_of[b]), has_scale)
            return raw_object[b]

        # S3: the local phase
        rates = np.full((num_tracks, 3), INVALID_RATE, dtype=np.uint8)
        for b in range(num_tracks):
            kinds = [kind for kind in range(3) if types[kind, b] == ANIMATED]
            if not kinds:
                continue
            rates[b, kinds] = 0 if multiple else 1
            threshold = shells[b, 1]
            listed, sizes = permutations(len(kinds))
            best, best_error = rates[b].copy(), F32(1.0e10)
            boundaries = np.flatnonzero(np.diff(sizes)) + 1
            for first, last in zip(np.concatenate([[0], boundaries]), np.concatenate([boundaries, [len(sizes)]])):
                candidates = listed[first:last]
                if not multiple:
                    candidates = candidates[(candidates != 0).all(axis=1)]       # 0 bits need a segment range
                if len(candidates) == 0:
                    continue
                transform = []
                for kind in range(3):
                    if kind in kinds:
                        transform.append(values[kind, b][candidates[:, kinds.index(kind)]])
                    else:
                        transform.append(values[kind, b][None])
                errors = scan(error_of(shells[b, 0], tuple(part[None] for part in raw_local[b]), tuple(transform), has_scale), threshold, UNTIL_ERROR_TOO_HIGH)
                lowest = int(errors.argmin())           # the first of the smallest: what a sequence of strict < updates keeps
                if errors[lowest] < best_error:
                    best_error = errors[lowest]
                    best[kinds] = candidates[lowest]
                if best_error < threshold:
                    break                               # good enough: the sizes behind this one are not tried
            rates[b] = best
            visits["local_not_met"] += int(not best_error < threshold)
            visits["local_picked_raw"] += int((best[kinds] == RAW_RATE).any())
        out.local_table[g, :, 0:3] = rates

        # S2: the object error, S4: the object phase
        object_cache, error_cache = {}, {}

        def key_of(b, current):
            return tuple((a, int(current[a, 0]), int(current[a, 1]), int(current[a, 2])) for a in chains[b])

        def object_of(b, current, key):
            if key not in object_cache:
                local = local_of(b, current[b])
                object_cache[key] = local if parent_of[b] < 0 else to_object(local, object_of(parent_of[b], current, key[:-1]), has_scale)
            return object_cache[key]

        def object_error(b, current, stop):
            key = key_of(b, current)
            if (key, stop) not in error_cache:
                out.evaluations += 1
                errors = error_of(shells[b, 0], raw_object_of(b), object_of(b, current, key), has_scale)
                error_cache[key, stop] = F32(scan(errors, shells[b, 1], stop))
            return error_cache[key, stop]

        def increment(rate, by):
            visits["increment_reached_raw"] += int(rate < RAW_RATE <= rate + by)
            return rate if rate >= RAW_RATE else min(rate + by, RAW_RATE)

        def increase_bone_bit_rate(b, num_increments, old_error):
            """quantize.transform.h:997-1050, loop for loop; the error is measured AT b, the chain bone whose rate is being tried"""
            base_rates = rates[b].copy()
            best, best_error = base_rates.copy(), old_error
            for rotation_increment in range(num_increments + 1):
                rotation = increment(int(base_rates[0]), rotation_increment)
                for translation_increment in range(num_increments + 1):
                    translation = increment(int(base_rates[1]), translation_increment)
                    for scale_increment in range((num_increments if has_scale else 0) + 1):
                        scale = increment(int(base_rates[2]), scale_increment)
                        if rotation_increment + translation_increment + scale_increment != num_increments:
                            if scale >= RAW_RATE:
                                break
                            continue
                        rates[b] = (rotation, translation, scale)
                        error = object_error(b, rates, UNTIL_ERROR_TOO_HIGH)
                        if error < best_error:
                            best_error, best = error, rates[b].copy()
                        rates[b] = base_rates
                        if scale >= RAW_RATE:
                            break
                    if translation >= RAW_RATE:
                        break
                if rotation >= RAW_RATE:
                    break
            return best

        for b in order:
            threshold = shells[b, 1]
            chain = chains[b]
            error = object_error(b, rates, UNTIL_ERROR_TOO_HIGH)
            if not error < threshold:
                initial_error = error
                best_rates = None
                while error >= threshold:
                    original_error = best_error = error
                    # calculate_bone_permutation_error for the one permutation "one increment somewhere in the chain": own track first
                    found, found_error = None, original_error
                    for link in chain[::-1]:
                        tried = increase_bone_bit_rate(link, 1, original_error)
                        if (tried == rates[link]).all():
                            continue
                        saved = rates[link].copy()
                        rates[link] = tried
                        permutation_error = object_error(b, rates, UNTIL_ERROR_TOO_HIGH)
                        rates[link] = saved
                        if permutation_error < found_error:
                            found_error, found = permutation_error, (link, tried)
                            if permutation_error < threshold:
                                break
                    error = found_error
                    if error < best_error:
                        best_error, best_rates = error, found
                        if error < threshold:
                            visits["ancestor_improved"] += int(found[0] != b)
                            break
                    if best_error >= original_error:
                        visits["no_progress"] += 1
                        break                           # no progress
                    error = best_error
                    rates[best_rates[0]] = best_rates[1]
                    visits["ancestor_improved"] += int(best_rates[0] != b)
                if error < initial_error:
                    rates[best_rates[0]] = best_rates[1]

                # the error remains too high: from child to parent, increase indiscriminately and keep the best
                error = object_error(b, rates, UNTIL_END_OF_SEGMENT)
                while error >= threshold:
                    num_maxed_out = 0
                    for link in chain[::-1]:
                        best_link_rates, best_link_error = rates[link].copy(), error
                        while error >= threshold:
                            smallest = int(np.argmin(rates[link]))          # std::min_element: the first of the smallest
                            if rates[link, smallest] >= RAW_RATE:
                                num_maxed_out += 1
                                visits["link_maxed_out"] += int((types[:, link] == ANIMATED).any())
                                break
                            if rates[link, 0] == rates[link, 1] and rates[link, 1] < RAW_RATE and rates[link, 2] >= RAW_RATE:
                                visits["scale_raw_translation_bump"] += int(rates[link, 2] == RAW_RATE)
                                rates[link, 1] += 1
                            else:
                                rates[link, smallest] += 1
                            error = object_error(b, rates, UNTIL_END_OF_SEGMENT)
                            if error < best_link_error:
                                best_link_rates, best_link_error = rates[link].copy(), error
                        rates[link] = best_link_rates
                        error = best_link_error
                        if error < threshold:
                            break
                    if num_maxed_out == len(chain):
                        visits["chain_maxed_out"] += 1
                        break
                # (the max-out pass behind this is for quatf_full only: never here)
        out.table[g, :, 0:3] = rates
        for b in range(num_tracks):
            out.errors[g, b] = object_error(b, rates, UNTIL_END_OF_SEGMENT)
            out.met[g, b] = out.errors[g, b] < shells[b, 1]
    return out


def compress_with_search(samples, sample_rate, **settings):
    """"search, then compress": (the Search, variable_compress_restatement.compress at its table)"""
    level = settings.pop("level", "medium")
    found = find_bit_rates(samples, sample_rate, level=level, **settings)
    return found, variable.compress(samples, sample_rate, found.table, **settings)


def stream_bits(table, types, segments):
    """the bits of the animated streams a table gives: per segment its samples times the bits of a pose"""
    total = 0
    for g, (_, count) in enumerate(segments):
        for kind in range(3):
            tracks = np.flatnonzero(types[kind] == ANIMATED)
            total += count * 3 * int(BITS[np.minimum(table[g, tracks, kind], RAW_RATE)].sum())
    return total
