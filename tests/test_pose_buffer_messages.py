"""The exact refusals of the launches over a caller's pose rows (aclhip_transform_poses_batch, aclhip_blend_poses_batch,
aclhip_inverse_transform_poses_batch, aclhip_measure_pose_error_batch and its _metric form, aclhip_pose_matrices_batch,
aclhip_skinning_matrices_batch), without a device: status, the whole text of aclhip_last_error_message and which refusal comes first.

tests/golden/pose_buffer_messages.json is a recording, not an expectation written by hand: every call that the six argument test files of
these entry points make through a NULL context (their REFUSED tables, their overlap cases and the calls that pass every check and end at
"null context"), and calls in which two checks fail at once, one for nearly every pair of neighbouring clauses of each argument check.
It was recorded from the library as it stood before the host side of these entry points was given one front -- commit 6509a3d, "Add
aclhip_compress_tracks_batch" -- built in a directory of its own, and is replayed here against the library under test: a change to the
host side that moves a clause, rewords a message or lets another refusal win shows as a difference.

Per entry point the file holds `base`, the C arguments in order of a call that passes every check (the struct is an object of its fields
that are not 0, `bounds` in it an object of aclhip_pose_bounds' fields), and every call as its differences from them -- "<index>": a C
argument, "<name>": a field of the struct -- under the message it was refused with (`recorded`) or under the two checks that fail in it
(`two_at_once`: [differences, message]). Every status is `status`."""
import json
import os

import pytest

from acl_amd import runtime
from message_replay import arguments_of, replay

with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "pose_buffer_messages.json")) as file:
    FIXTURE = json.load(file)
STATUS = FIXTURE.pop("status")
FUNCTIONS = ("aclhip_transform_poses_batch", "aclhip_blend_poses_batch", "aclhip_inverse_transform_poses_batch", "aclhip_measure_pose_error_batch",
             "aclhip_measure_pose_error_metric_batch", "aclhip_pose_matrices_batch", "aclhip_skinning_matrices_batch")


def test_the_recording_covers_every_entry_point_and_pairs_of_failing_checks():
    assert set(FIXTURE) == set(FUNCTIONS)
    for function, group in FIXTURE.items():
        assert group["base"][0] is None                             # a NULL context: no device
        assert len(group["recorded"]) >= 2 and "null context" in group["recorded"], function
        if function != "aclhip_measure_pose_error_batch":           # (one check with its _metric form, which holds the pairs)
            assert len(group["two_at_once"]) >= 10, function


@pytest.mark.parametrize("function", FUNCTIONS)
def test_status_and_message_are_what_was_recorded(function):
    lib = runtime.load_library()
    group = FIXTURE[function]
    calls = [(changes, message) for message, recorded in group["recorded"].items() for changes in recorded] + list(map(tuple, group["two_at_once"].values()))
    for changes, message in calls:
        assert replay(lib, dict(function=function, arguments=arguments_of(group["base"], changes))) == (STATUS, message), changes
