"""The exact refusals of the three compressors (aclhip_compress_raw_scalar_tracks_batch, aclhip_compress_raw_tracks_batch,
aclhip_compress_tracks_batch) and the exact values of their size functions, without a device: status, the whole text of
aclhip_last_error_message, which refusal comes first, and every size.

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
(test_pose_buffer_messages.py, message_replay.py)."""
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
FUNCTIONS = ("aclhip_compress_raw_scalar_tracks_batch", "aclhip_compress_raw_tracks_batch", "aclhip_compress_tracks_batch")
SIZE_FUNCTIONS = {"aclhip_scalar_compress_bound": 3, "aclhip_scalar_compress_workspace_bytes": 2, "aclhip_transform_compress_bound": 3,
                  "aclhip_transform_compress_workspace_bytes": 2, "aclhip_compress_tracks_workspace_bytes": 2}
# the neighbouring clauses of each argument check that can fail together (the scalar call's check has 15 clauses)
PAIRS = {"aclhip_compress_raw_scalar_tracks_batch": 14, "aclhip_compress_raw_tracks_batch": 10, "aclhip_compress_tracks_batch": 10}


def test_the_recording_covers_every_entry_point_pairs_of_failing_checks_and_the_cap():
    assert set(FIXTURE) == set(FUNCTIONS) and set(SIZES["values"]) == set(SIZE_FUNCTIONS)
    for function, group in FIXTURE.items():
        assert group["base"][0] is None                             # a NULL context: no device
        assert len(group["recorded"]) >= 2 and "null context" in group["recorded"], function
        assert len(group["two_at_once"]) >= PAIRS[function], function
    assert {0, 1, 15, 16, 17, 0xFFFF, 1 << 31, (1 << 32) - 1} <= set(SIZES["grid"])
    for function, count in SIZE_FUNCTIONS.items():
        assert len(SIZES["values"][function]) == len(SIZES["grid"]) ** count
        if function != "aclhip_scalar_compress_bound":              # (64 bits wide and not capped)
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
    for arguments, size in zip(itertools.product(SIZES["grid"], repeat=SIZE_FUNCTIONS[function]), SIZES["values"][function]):
        assert size_of(*arguments) == size, arguments
