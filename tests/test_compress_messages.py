"""The exact refusals of the compressors (aclhip_compress_raw_scalar_tracks_batch, aclhip_compress_raw_tracks_batch,
aclhip_compress_tracks_batch, aclhip_compress_tracks_variable_batch) and of the bit rate search (aclhip_find_bit_rates_batch), and the
exact values of their size functions, without a device: status, the whole text of aclhip_last_error_message, which refusal comes
first, and every size.

tests/golden/compress_messages.json is a recording, not an expectation written by hand. Per entry point it holds every call that
test_scalar_compress_arguments.py, test_transform_compress_arguments.py and test_compress_tracks_arguments.py make through a NULL
context (their refusals, their overlap cases and the calls that pass every check and end at "null context"; taken by wrapping the
library's functions while those tests ran), and calls in which two checks fail at once: one for every pair of neighbouring clauses of
the argument check that can fail together -- the pairs around the shell metadata alignment, the format refusals and the two overlap
passes of aclhip_compress_tracks_batch among them -- and pairs inside an overlap pass. `sizes` holds aclhip_scalar_compress_bound,
aclhip_scalar_compress_workspace_bytes, aclhip_transform_compress_bound, aclhip_transform_compress_workspace_bytes and
aclhip_compress_tracks_workspace_bytes over every combination of `grid` for their arguments, in itertools.product order; the grid
reaches the cap at the largest multiple of 16.

It was recorded from the library as it stood before the two transform compressors were given one host side -- commit 11942d1, "One
host front for the launches over a caller's pose rows" -- built in a directory of its own, where the recorder also asserted that each
half of a pair is refused on its own, with another message than the other half, and that the pair is refused as its first half. It
is replayed here against the library under test: a change to the host side that moves a clause, rewords a message, lets another
refusal win or changes a size shows as a difference. The layout of an entry point's group is that of pose_buffer_messages.json
(test_pose_buffer_messages.py, message_replay.py).

The groups of aclhip_compress_tracks_variable_batch and aclhip_find_bit_rates_batch and the sizes aclhip_variable_compress_num_segments,
aclhip_variable_compress_bound, aclhip_compress_variable_workspace_bytes and aclhip_find_bit_rates_workspace_bytes were recorded the
same way later, from the library as it stood before the host side stated its repeated parts once -- commit ff20f68, "Add
aclhip_find_bit_rates_batch: the variable formats' bit rate search" --: the calls of test_variable_compress_arguments.py and
test_bit_rate_search_arguments.py, and a pair for every two neighbouring clauses that can fail together, those behind the shared check
(max_samples, the level, the table's pointer, alignment, strides and the uniform rates) and the table's own overlap passes -- both of
the search's -- among them. Their sample count argument runs over `sample_grid`, which holds the counts at which the split into
segments changes shape (one segment up to 31, two at 32, the dealt-out last segment at 33, 47 and 48); their other arguments run over
`grid`."""
import itertools
import json
import os

import pytest

from acl_amd import runtime
from message_replay import arguments_of, replay

with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "compress_messages.json")) as file:
    FIXTURE = json.load(file)
STATUS = FIXTURE.pop("status")
SIZES = FIXTURE.pop("sizes")
FUNCTIONS = ("aclhip_compress_raw_scalar_tracks_batch", "aclhip_compress_raw_tracks_batch", "aclhip_compress_tracks_batch",
             "aclhip_compress_tracks_variable_batch", "aclhip_find_bit_rates_batch")
# the grid each argument runs over
G, S = "grid", "sample_grid"
SIZE_FUNCTIONS = {"aclhip_scalar_compress_bound": (G, G, G), "aclhip_scalar_compress_workspace_bytes": (G, G), "aclhip_transform_compress_bound": (G, G, G),
                  "aclhip_transform_compress_workspace_bytes": (G, G), "aclhip_compress_tracks_workspace_bytes": (G, G),
                  "aclhip_variable_compress_num_segments": (S,), "aclhip_variable_compress_bound": (G, S, G),
                  "aclhip_compress_variable_workspace_bytes": (G, G, S), "aclhip_find_bit_rates_workspace_bytes": (G, G, S)}
# the neighbouring clauses of each argument check that can fail together (the scalar call's check has 15 clauses; the variable call's
# 25, of which the strides and the uniform rates exclude each other; the search's 27, with three such exclusions)
PAIRS = {"aclhip_compress_raw_scalar_tracks_batch": 14, "aclhip_compress_raw_tracks_batch": 10, "aclhip_compress_tracks_batch": 10,
         "aclhip_compress_tracks_variable_batch": 24, "aclhip_find_bit_rates_batch": 27}


def test_the_recording_covers_every_entry_point_pairs_of_failing_checks_and_the_cap():
    assert set(FIXTURE) == set(FUNCTIONS) and set(SIZES["values"]) == set(SIZE_FUNCTIONS)
    for function, group in FIXTURE.items():
        assert group["base"][0] is None                             # a NULL context: no device
        assert len(group["recorded"]) >= 2 and "null context" in group["recorded"], function
        assert len(group["two_at_once"]) >= PAIRS[function], function
    assert {0, 1, 15, 16, 17, 0xFFFF, 1 << 31, (1 << 32) - 1} <= set(SIZES["grid"])
    assert {0, 1, 31, 32, 33, 47, 48, (1 << 32) - 1} <= set(SIZES["sample_grid"])
    for function, grids in SIZE_FUNCTIONS.items():
        assert len(SIZES["values"][function]) == len(list(itertools.product(*(SIZES[grid] for grid in grids))))
        if function not in ("aclhip_scalar_compress_bound", "aclhip_variable_compress_num_segments"):       # (64 bits wide and not capped; a count)
            assert 0xFFFFFFFFFFFFFFF0 in SIZES["values"][function], function


@pytest.mark.parametrize("function", FUNCTIONS)
def test_status_and_message_are_what_was_recorded(function):
    lib = runtime.load_library()
    group = FIXTURE[function]
    calls = [(changes, message) for message, recorded in group["recorded"].items() for changes in recorded] + list(map(tuple, group["two_at_once"].values()))
    for changes, message in calls:
        assert replay(lib, dict(function=function, arguments=arguments_of(group["base"], changes))) == (STATUS, message), changes


@pytest.mark.parametrize("function", sorted(SIZE_FUNCTIONS))
def test_every_size_is_what_was_recorded(function):
    size_of = getattr(runtime.load_library(), function)
    for arguments, size in zip(itertools.product(*(SIZES[grid] for grid in SIZE_FUNCTIONS[function])), SIZES["values"][function]):
        assert size_of(*arguments) == size, arguments
