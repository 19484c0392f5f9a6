"""What aclhip_find_bit_rates_level_batch computes: find_optimal_bit_rates (compression/impl/quantize.transform.h:1174-1523) at all five
levels and at `automatic` (find_best_compression_level, compress.transform.impl.h:114-136), restated on the CPU on top of
tests/bit_rate_search_restatement.py. That one gives steps 0 - 8, the segment's shell (S0) and the local phase (S3) -- its
`local_table` and `shells` -- and, at lowest, low and medium, the whole answer; its arithmetic (error_of, to_object) is called through
the module, so tests/matrix_metric_compress_restatement.arithmetic_of swaps the metric here as it does there. Restated here: S1 as
that file states it, and the object phase S4 with the first loop of :1250-1377 loop for loop:

  a round's bar is original_error throughout; best_error is carried across the calls of the round
  medium      the chain increments {1}
  >= high     {2} on one link; with more than one link {1,1} on two
  >= highest  {3} on one link; with more than one link {2,1}; with more than two {1,1,1}
  after each call (calculate_bone_permutation_error): error < best_error keeps that permutation's rates; error < threshold leaves the round

The arrangements of a shape over the chain are std::next_permutation's over the chain array, root first (next_permutation below is the
algorithm itself, not a derived order). What to keep in mind:
  1. {2,1} starts at [..., 2, 1] -- parent + 2, own + 1 --, which is NOT the smallest arrangement: next_permutation runs from there to
     the end, so [..., 1, 2] is never tried and a chain of two links tries exactly one arrangement. Every other shape starts at its
     smallest arrangement and visits all.
  2. increase_bone_bit_rate(link, n) enumerates the (rotation, translation, scale) increments that sum to n with the reference's break
     and continue rules at rate 24 (:1005-1046; without scale the scale increment is 0). It measures AT THE CHAIN BONE whose rate is
     tried, not at the track under work, and its bar is old_error, the round's original_error.
  3. A permutation counts only if one of its links changed its rates (is_permutation_valid); an invalid one is skipped unmeasured.
  4. Inside one call a permutation below the threshold ends that call at once.
  5. A candidate is the table with up to three tracks' rates replaced.

Within a round neither the rates nor original_error change, so increase_bone_bit_rate(link, n) is a function of (link, n): the kernel
computes it once per round (a memo), the reference for every arrangement. No decision depends on that; `evaluations` counts the
object errors the kernel measures, `evaluations_unmemoized` those the reference's loops measure.
A helper, not a test file: tests/test_bit_rate_search_levels_oracle.py holds it to the reference's compressor,
tests/test_gpu_bit_rate_search_levels.py holds the kernels to it on every byte."""
import collections

import numpy as np

import bit_rate_search_restatement as search
import variable_compress_restatement as variable
from bit_rate_search_restatement import INVALID_RATE, NUM_RATES, UNTIL_END_OF_SEGMENT, UNTIL_ERROR_TOO_HIGH  # noqa: F401
from variable_compress_restatement import ANIMATED, CONSTANT, DEFAULT, F32, IDENTITY, INV_65535, NO_PARENT, RAW_RATE, XYZ, f32, lossy  # noqa: F401

AUTOMATIC = 100
LEVELS = dict(search.LEVELS, automatic=AUTOMATIC)
SHAPES = {"2": (2,), "1_1": (1, 1), "3": (3,), "2_1": (2, 1), "1_1_1": (1, 1, 1)}       # the increments, the own track's last

# what Search.visits counts besides bit_rate_search_restatement.VISITS
VISITS = search.VISITS + tuple("shape_%s_won" % name for name in SHAPES) + (     # a round ended with that shape's permutation as its best
    "shape_1_won",
    "invalid_permutation_skipped",    # no link of an arrangement changed its rates: not measured
    "early_exit_in_shape",            # a permutation below the threshold ended a call with arrangements left
    "two_reached_raw",                # increase_bone_bit_rate(link, 2) took a real rate to 24
    "three_reached_raw",              # ... (link, 3)
    "two_one_on_two_links")           # {2,1} on a chain of exactly two links: its one arrangement


def automatic_level(num_samples, parents, num_tracks):
    """find_best_compression_level: medium above 500 samples (the count as registered: the level is resolved at
    compress.transform.impl.h:217, the looping vote runs at :236); else by the longest chain, counted in bones from a root to a leaf
    (clip_context.impl.h:232-270: a leaf's chain holds the leaf and every ancestor): below 18 highest, below 25 high, else medium"""
    if num_samples > 500:
        return 2
    longest = 0
    for b in range(num_tracks):
        links, up = 1, b
        while parents is not None and int(parents[up]) < num_tracks:
            links, up = links + 1, int(parents[up])
        longest = max(longest, links)
    return 4 if longest < 18 else 3 if longest < 25 else 2


def next_permutation(a):
    """std::next_permutation over the list a, in place; False when it wrapped around to the sorted order"""
    i = len(a) - 1
    while i > 0 and a[i - 1] >= a[i]:
        i -= 1
    if i == 0:
        a.reverse()
        return False
    j = len(a) - 1
    while a[j] <= a[i - 1]:
        j -= 1
    a[i - 1], a[j] = a[j], a[i - 1]
    a[i:] = a[i:][::-1]
    return True


def find_bit_rates(samples, sample_rate, level="medium", **settings):
    """bit_rate_search_restatement.find_bit_rates with `level` one of LEVELS or its number. The Search has two more fields: level, the
    level that was searched (0 to 4), and evaluations_unmemoized."""
    level = LEVELS.get(level, level)
    if level not in LEVELS.values():
        raise ValueError("a level of %r" % (level,))
    samples = f32(samples)
    num_tracks = samples.shape[1]
    if level == AUTOMATIC:
        level = automatic_level(samples.shape[0], settings.get("parents"), num_tracks)
    out = search.find_bit_rates(samples, sample_rate, level="medium", **settings)
    out.level = level
    out.evaluations_unmemoized = out.evaluations
    if level < 3:
        return out

    base = out.base
    default_pose, parents = settings.get("default_pose"), settings.get("parents")
    default_pose = np.tile(IDENTITY, (num_tracks, 1)) if default_pose is None else f32(default_pose)[:num_tracks]
    table_parents = np.full(num_tracks, NO_PARENT, dtype=np.uint32) if parents is None else np.asarray(parents).astype(np.uint32)[:num_tracks]
    parent_of = [int(p) if int(p) < num_tracks else -1 for p in table_parents]
    kept = samples[:base.num_samples].copy()
    kept[:, :, 0:4] = lossy.positive_w(lossy.normalize(kept[:, :, 0:4]))
    types = base.types
    has_scale = bool((types[2] != DEFAULT).any())
    multiple = len(base.segments) > 1
    order = search.parent_first(table_parents, num_tracks)
    chains = []
    for b in range(num_tracks):
        chain = [b]
        while parent_of[chain[-1]] >= 0:
            chain.append(parent_of[chain[-1]])
        chains.append(chain[::-1])          # from the root to b
    out.evaluations = out.evaluations_unmemoized = 0
    visits = out.visits = collections.Counter({name: out.visits[name] for name in ("local_not_met", "local_picked_raw")})
    counts = {"memoized": 0, "unmemoized": 0}

    for g, (start, count) in enumerate(base.segments):
        rows = slice(start, start + count)
        shells = out.shells[g]
        # S1, as bit_rate_search_restatement states it
        values = {}
        for kind in range(3):
            for b in range(num_tracks):
                if types[kind, b] == DEFAULT:
                    values[kind, b] = np.tile(f32(default_pose[b, variable.LANES[kind]]), (count, 1))
                elif types[kind, b] == CONSTANT:
                    values[kind, b] = np.tile(f32(lossy.normalize(kept[0, b, 0:4]) if kind == 0 else kept[0, b, XYZ[kind]]), (count, 1))
                else:
                    clip_min, clip_extent = base.clip_ranges[kind, b]
                    clip_normalized = variable.normalize_in(kept[:, b, XYZ[kind]], clip_min, clip_extent)
                    normalized = clip_normalized[rows]
                    if multiple:
                        segment_min, segment_extent = base.segment_ranges[kind, b, g]
                        normalized = variable.normalize_in(normalized, segment_min, segment_extent)
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
                    values[kind, b] = search.from_positive_w(at_rates) if kind == 0 else at_rates

        def local_of(b, rates_of_b):
            return tuple(values[kind, b][int(rates_of_b[kind])] if types[kind, b] == ANIMATED else values[kind, b] for kind in range(3))

        raw_local = [(lossy.normalize(kept[rows, b, 0:4]), kept[rows, b, 4:7], kept[rows, b, 8:11]) for b in range(num_tracks)]
        raw_object, object_cache, error_cache = {}, {}, {}

        def raw_object_of(b):
            if b not in raw_object:
                raw_object[b] = raw_local[b] if parent_of[b] < 0 else search.to_object(raw_local[b], raw_object_of(parent_of[b]), has_scale)
            return raw_object[b]

        def object_of(b, current, key):
            if key not in object_cache:
                local = local_of(b, current[b])
                object_cache[key] = local if parent_of[b] < 0 else search.to_object(local, object_of(parent_of[b], current, key[:-1]), has_scale)
            return object_cache[key]

        def object_error(b, current, stop):
            """S2 (every call counts as one measured object error; equal ones are computed once)"""
            counts["memoized"] += 1
            counts["unmemoized"] += 1
            key = tuple((a, int(current[a, 0]), int(current[a, 1]), int(current[a, 2])) for a in chains[b])
            if (key, stop) not in error_cache:
                errors = search.error_of(shells[b, 0], raw_object_of(b), object_of(b, current, key), has_scale)
                error_cache[key, stop] = F32(search.scan(errors, shells[b, 1], stop))
            return error_cache[key, stop]

        rates = out.local_table[g, :, 0:3].copy()

        def increase_bone_bit_rate(b, num_increments, old_error):
            """quantize.transform.h:997-1050, loop for loop; the error is measured AT b, the chain bone whose rate is being tried"""
            def increment(rate, by):
                reached = int(rate < RAW_RATE <= rate + by)
                visits["increment_reached_raw"] += reached
                if num_increments > 1:
                    visits["two_reached_raw" if num_increments == 2 else "three_reached_raw"] += reached
                return rate if rate >= RAW_RATE else min(rate + by, RAW_RATE)
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
            links = len(chain)
            error = object_error(b, rates, UNTIL_ERROR_TOO_HIGH)
            if error < threshold:
                continue
            initial_error = error
            best_rates = None
            while error >= threshold:
                original_error = best_error = error
                memo = {}

                def increased(link, num_increments):
                    """increase_bone_bit_rate(link, n) of this round: measured once, counted for the reference every time"""
                    if (link, num_increments) not in memo:
                        before = counts["memoized"]
                        tried = increase_bone_bit_rate(link, num_increments, original_error)
                        memo[link, num_increments] = tried, counts["memoized"] - before
                    else:
                        counts["unmemoized"] += memo[link, num_increments][1]
                    return memo[link, num_increments][0]

                def calculate_bone_permutation_error(increments):
                    """:1052-1098 from the start arrangement: the increments on the last links of the chain, in the order given"""
                    permutation = [0] * links
                    permutation[links - len(increments):] = increments
                    found, found_error = None, original_error
                    while True:
                        changed, valid = [], False
                        for link, num_increments in zip(chain, permutation):
                            if num_increments != 0:
                                tried = increased(link, num_increments)
                                valid = valid or bool((tried != rates[link]).any())
                                changed.append((link, tried))
                        if valid:
                            saved = [rates[link].copy() for link, _ in changed]
                            for link, tried in changed:
                                rates[link] = tried
                            permutation_error = object_error(b, rates, UNTIL_ERROR_TOO_HIGH)
                            for (link, _), before in zip(changed, saved):
                                rates[link] = before
                            if permutation_error < found_error:
                                found_error, found = permutation_error, changed
                                if permutation_error < threshold:
                                    visits["early_exit_in_shape"] += int(next_permutation(list(permutation)))
                                    break
                        else:
                            visits["invalid_permutation_skipped"] += 1
                        if not next_permutation(permutation):
                            break
                    return found_error, found

                calls = [("1", (1,))]
                if level >= 3:
                    calls.append(("2", (2,)))
                    if links > 1:
                        calls.append(("1_1", (1, 1)))
                if level >= 4:
                    calls.append(("3", (3,)))
                    if links > 1:
                        calls.append(("2_1", (2, 1)))
                        visits["two_one_on_two_links"] += int(links == 2)
                        if links > 2:
                            calls.append(("1_1_1", (1, 1, 1)))
                met = False
                for name, increments in calls:
                    error, found = calculate_bone_permutation_error(list(increments))
                    if error < best_error:
                        best_error, best_rates, winner = error, found, name
                        if error < threshold:
                            met = True
                            break
                if met:
                    visits["shape_%s_won" % winner] += 1
                    visits["ancestor_improved"] += int(any(link != b for link, _ in best_rates))
                    break
                if best_error >= original_error:
                    visits["no_progress"] += 1
                    break                           # no progress
                error = best_error
                visits["shape_%s_won" % winner] += 1
                visits["ancestor_improved"] += int(any(link != b for link, _ in best_rates))
                for link, tried in best_rates:
                    rates[link] = tried
            if error < initial_error:
                for link, tried in best_rates:
                    rates[link] = tried

            # the error remains too high: from child to parent, increase indiscriminately and keep the best (unchanged by the level)
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
                if num_maxed_out == links:
                    visits["chain_maxed_out"] += 1
                    break
        out.table[g, :, 0:3] = rates
        out.evaluations, out.evaluations_unmemoized = counts["memoized"], counts["unmemoized"]
        for b in range(num_tracks):
            out.errors[g, b] = object_error(b, rates, UNTIL_END_OF_SEGMENT)
            out.met[g, b] = out.errors[g, b] < shells[b, 1]
    return out


def find_bit_rates_metric(samples, sample_rate, metric, level="medium", **settings):
    """find_bit_rates under the error metric `metric` (tests/matrix_metric_compress_restatement.py: its arithmetic while the search runs)"""
    import matrix_metric_compress_restatement as metric_restatement
    with metric_restatement.arithmetic_of(metric):
        return find_bit_rates(samples, sample_rate, level=level, **settings)


def compress_with_search(samples, sample_rate, metric=0, **settings):
    """"search, then compress": (the Search, variable_compress_restatement.compress at its table), both under `metric`"""
    import matrix_metric_compress_restatement as metric_restatement
    level = settings.pop("level", "medium")
    found = find_bit_rates_metric(samples, sample_rate, metric, level=level, **settings)
    return found, metric_restatement.compress_variable(samples, sample_rate, found.table, metric, **settings)
