"""aclhip_find_bit_rates_level_batch and its host-only size function without a device: the surface (header, library, binding), the
prototype from a C99 translation unit, the levels it takes and the message for every other, every refusal it shares with
aclhip_find_bit_rates_metric_batch under its own word ("bit rate level search"), both size functions against their formulas, and the
other two calls still refusing the levels 3 and 4. Every case is decided before any device call and works without a context. Fails on a
library without the call."""
import ctypes
import inspect
import os
import re
import subprocess

import pytest

from acl_amd import runtime
from test_bit_rate_search_arguments import (COUNT, INSTANCE_STRIDE, INVALID, MAX_SAMPLES, MAX_TRACKS, METADATA, RATES, RAWS, RESULTS, SEGMENT_STRIDE, SEGMENTS, TABLE, TABLES,
                                            WORKSPACE)
import test_bit_rate_search_arguments as base_arguments

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("aclhip_find_bit_rates_level_workspace_bytes", "aclhip_find_bit_rates_level_batch")
AUTOMATIC = 100
LEVEL_MESSAGE = "a level of %u: 0 (lowest), 1 (low), 2 (medium), 3 (high), 4 (highest) or 100 (automatic)"
CALL = ("aclhip_find_bit_rates_level_batch(gpu, d_raws, num_instances, &search, d_bit_rates, instance_stride, segment_stride, d_results, ACLHIP_METRIC_QVVF, "
        "(void*)hip_stream);")


def test_header_declares_library_exports_and_binding_binds_the_entry_points():
    header = open(os.path.join(ROOT, "include", "aclhip.h")).read()
    declared = set(re.findall(r"\b(aclhip_[a-z_0-9]+)\s*\(", re.sub(r"/\*.*?\*/", "", header, flags=re.S)))
    lib = runtime.load_library()
    for name in NAMES:
        assert name in declared and hasattr(lib, name) and name in runtime.EXPORTED_SYMBOLS, name
    assert re.search(r"#define\s+ACLHIP_LEVEL_AUTOMATIC\s+100u", header)
    assert hasattr(runtime.Context, "find_bit_rates_level_batch") and callable(runtime.find_bit_rates_level_workspace_bytes)
    assert lib.aclhip_abi_version() == runtime.ABI_VERSION == 6       # (added without a bump: no existing struct changed)
    assert runtime.COMPRESSION_LEVELS == {"lowest": 0, "low": 1, "medium": 2, "high": 3, "highest": 4, "automatic": AUTOMATIC} and runtime.LEVEL_AUTOMATIC == AUTOMATIC
    # the defaults stay medium, and the levels come back only where they are asked for
    for function in (runtime.find_bit_rates, runtime.compress_tracks_variable):
        parameters = inspect.signature(function).parameters
        assert parameters["level"].default == "medium" and parameters["return_levels"].default is False
    # the call that leaves the levels out says where they are
    comments = " ".join(" ".join(comment.replace("*", " ").split()) for comment in re.findall(r"/\*.*?\*/", header, flags=re.S))
    assert any("the levels high and highest" in text and "aclhip_find_bit_rates_level_batch" in text for text in re.findall(r"Left out[^.]*\.", comments))


def test_the_prototype_matches_a_c99_translation_unit(tmp_path):
    lib_dir = os.path.dirname(runtime.library_path())
    binary = tmp_path / "find_bit_rates_level_abi"
    source = os.path.join(ROOT, "tests", "c", "find_bit_rates_level_abi.c")
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-I", os.path.join(ROOT, "include"), source, "-L" + lib_dir, "-laclhip",
                    "-Wl,-rpath," + lib_dir, "-o", str(binary)], check=True)
    done = subprocess.run([str(binary)], stdout=subprocess.PIPE, text=True, timeout=120)
    assert done.returncode == 0, done.returncode        # (the program's own checks, INTEGRATION.md's call sequence among them)
    assert [int(word) for word in done.stdout.split()] == [AUTOMATIC]
    # the document shows the call the C file compiles
    assert CALL in open(os.path.join(ROOT, "INTEGRATION.md")).read() and CALL in open(source).read()


def search(raws=RAWS, rates=RATES, instance_stride=INSTANCE_STRIDE, segment_stride=SEGMENT_STRIDE, results=RESULTS, count=COUNT, no_desc=False, metric=0, **fields):
    lib = runtime.load_library()
    desc = runtime.FindBitRatesDesc()
    desc.precision, desc.shell_distance, desc.max_tracks, desc.max_samples, desc.workspace, desc.level = 1.0e-4, 1.0, MAX_TRACKS, MAX_SAMPLES, WORKSPACE, 4
    for name, value in fields.items():
        setattr(desc, name, value)
    status = lib.aclhip_find_bit_rates_level_batch(None, raws, count, None if no_desc else ctypes.byref(desc), rates, instance_stride, segment_stride, results, metric, None)
    message = lib.aclhip_last_error_message(None).decode()
    assert status == INVALID and message != ""
    return message


def test_the_levels_it_takes_and_the_message_for_any_other():
    for level in (0, 1, 2, 3, 4, AUTOMATIC):
        for metric in (0, 1):
            assert search(level=level, metric=metric) == "null context"          # what passes the checks ends at the missing context
    for level in (5, 6, 99, 101, 255, 0xFFFFFFFF):
        assert search(level=level) == LEVEL_MESSAGE % level
    # the other two calls as they were
    for level, name in ((3, "high"), (4, "highest")):
        assert base_arguments.search(level=level) == "level %u (%s) is not built: 0 (lowest), 1 (low) and 2 (medium) are" % (level, name)
    for level in (5, AUTOMATIC, 0xFFFFFFFF):
        assert base_arguments.search(level=level) == "a level of %u: 0 (lowest), 1 (low) or 2 (medium)" % level
    assert base_arguments.search(max_samples=0) == "a bit rate search desc of 0 max_samples"


def test_every_shared_refusal_under_this_calls_word():
    assert search(flags=7, precision=0.0, shell_distance=0.0, default_pose=TABLE, parent_indices=TABLE, track_precisions=TABLE, track_shell_distances=TABLE,
                  num_table_tracks=7, shell_metadata=METADATA) == "null context"
    assert search(count=0) == "null context"
    assert search(instance_stride=SEGMENTS * (SEGMENT_STRIDE + 8) + 4, segment_stride=SEGMENT_STRIDE + 8, rates=RATES * 16) == "null context"
    for metric in (2, 0xFFFFFFFF):
        assert search(metric=metric, raws=None) == "unknown error metric %u" % metric           # before any other argument is looked at
    assert search(raws=None) == "null raw track handles"
    assert search(no_desc=True) == "null bit rate level search desc"
    assert search(results=None) == "null compress results"
    assert search(workspace=None) == "null workspace"
    assert search(workspace=WORKSPACE + 8) == "the workspace must be 16 byte aligned"
    assert search(results=RESULTS + 4) == "compress results must be 8 byte aligned"
    assert search(default_pose=TABLE + 8, num_table_tracks=7) == "the default pose must be 16 byte aligned"
    for field in ("parent_indices", "track_precisions", "track_shell_distances"):
        assert search(num_table_tracks=7, **{field: TABLE + 2}) == "the track tables must be 4 byte aligned"
    assert search(shell_metadata=METADATA + 4) == "the shell metadata must be 8 byte aligned"
    for flags in (8, 9, 0x80000000):
        assert search(flags=flags) == "unknown compress flags 0x%x" % flags
    for fields in ({"reserved": (ctypes.c_uint64 * 2)(0, 1)}, {"reserved": (ctypes.c_uint64 * 2)(1 << 63, 0)}, {"reserved_word": 1 << 31}):
        assert search(**fields) == "the reserved fields of a bit rate level search desc are 0"
    for value, text in ((-1.0e-5, "-1e-05"), (float("nan"), "nan"), (float("inf"), "inf")):
        assert search(precision=value) == "a precision of %s: it must be finite and not negative" % text
        assert search(shell_distance=value) == "a shell distance of %s: it must be finite and not negative" % text
    for field, _, _ in TABLES:
        assert search(**{field: TABLE}) == "a track table with a count of 0"
    assert search(max_tracks=0) == "a bit rate level search desc of 0 max_tracks"
    assert search(max_samples=0) == "a bit rate level search desc of 0 max_samples"
    assert search(rates=None) == "null bit rate table"
    for rates in (RATES + 1, RATES + 2):
        assert search(rates=rates) == "the bit rate table must be 4 byte aligned"
    for strides in ({"instance_stride": INSTANCE_STRIDE + 2}, {"segment_stride": SEGMENT_STRIDE + 1}, {"instance_stride": 1 << 40, "segment_stride": 402}):
        assert search(**strides) == "the strides of the bit rate table are multiples of 4"
    for segment_stride in (0, 4, SEGMENT_STRIDE - 4):
        assert search(segment_stride=segment_stride) == "a segment stride of %u: a written row takes 4 * max_tracks = %u bytes" % (segment_stride, SEGMENT_STRIDE)
    for instance_stride in (0, SEGMENT_STRIDE, INSTANCE_STRIDE - 4):
        assert search(instance_stride=instance_stride) == "an instance stride of %u: the %u rows of an instance take %u segment strides" % (instance_stride, SEGMENTS, SEGMENTS)
    assert search(max_samples=31, instance_stride=SEGMENT_STRIDE) == "null context"


def test_the_table_is_on_the_written_side_of_the_overlap_check_and_the_workspace_is_this_calls():
    table_bytes = (COUNT - 1) * INSTANCE_STRIDE + (SEGMENTS - 1) * SEGMENT_STRIDE + 4 * MAX_TRACKS
    workspace_bytes = runtime.find_bit_rates_level_workspace_bytes(COUNT, MAX_TRACKS, MAX_SAMPLES)
    others = (("the compress results", RESULTS, COUNT * 8), ("the workspace", WORKSPACE, workspace_bytes), ("the shell metadata", METADATA, COUNT * MAX_TRACKS * 8),
              ("the raw track handles", RAWS, COUNT * 4))
    for what, base, size in others:
        assert search(shell_metadata=METADATA, rates=base + size - 4) == "the bit rate table overlap %s" % what
        assert search(shell_metadata=METADATA, rates=base - table_bytes + 4) == "the bit rate table overlap %s" % what
    assert search(shell_metadata=METADATA, rates=WORKSPACE + workspace_bytes) == "null context"
    for field, what, width in TABLES:
        assert search(num_table_tracks=7, rates=0x1000000, **{field: 0x1000000 + table_bytes - 16}) == "the bit rate table overlap %s" % what
        assert search(num_table_tracks=7, rates=0x1000000, **{field: 0x1000000 + table_bytes}) == "null context"
    # the workspace is the other call's and more: a buffer sized for that call is too small to stand in front of the results
    far = 0x4000000
    assert search(results=far, workspace=far - runtime.find_bit_rates_workspace_bytes(COUNT, MAX_TRACKS, MAX_SAMPLES)) == "the compress results overlap the workspace"
    assert search(results=far, workspace=far - workspace_bytes) == "null context"


def part(size):
    return (size + 15) & ~15


def segments_of(num_samples):
    if num_samples <= 31:
        return 1
    estimated = (num_samples + 15) // 16
    last = 16 - (estimated * 16 - num_samples)
    return estimated - 1 if (estimated - 1) * 15 >= last else estimated


def search_workspace(n, t, s):
    """aclhip_find_bit_rates_workspace_bytes, uncapped (tests/test_bit_rate_search_arguments.py)"""
    g = segments_of(max(s, 1))
    variable = part(n * 64) + part(n * t) + part(n * t * 6) + part(n * t * 8) + part(n * t * 72) + part(n * g * 32) + part(n * g * t * 12)
    return variable + part(n * g * 16) + part(n * g * t * 72) + part(n * g * t * 8) + part(n * g * t * 2)


@pytest.mark.parametrize("n", [0, 1, 2, 41, 4096])
def test_both_workspace_sizes_are_their_formulas_and_are_capped(n):
    cap = 0xFFFFFFFFFFFFFFF0
    for t in (1, 2, 65, 1000, 0xFFFF):
        for s in (1, 31, 32, 301, 65535):
            g = segments_of(s)
            old, new = runtime.find_bit_rates_workspace_bytes(n, t, s), runtime.find_bit_rates_level_workspace_bytes(n, t, s)
            assert old == min(search_workspace(n, t, s), cap)
            assert new == min(search_workspace(n, t, s) + part(n * g * t * 12), cap) and new % 16 == 0 and new >= old
    assert runtime.find_bit_rates_level_workspace_bytes(0xFFFFFFFF, 0xFFFFFFFF, 0xFFFFFFFF) == cap
    assert runtime.find_bit_rates_workspace_bytes(0xFFFFFFFF, 0xFFFFFFFF, 0xFFFFFFFF) == cap
