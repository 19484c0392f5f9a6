"""aclhip_find_bit_rates_batch and its host-only size function without a device: the surface (header, library, binding), the struct
layout against a C99 translation unit, every ACLHIP_ERROR_INVALID_ARGUMENT with its message -- each is decided before any device call
and works without a context --, the levels that are not built, the stride rules of a table that is WRITTEN, that table on the written
side of the overlap check, and the size function against its formula and at its cap. Fails on a library without the call."""
import ctypes
import os
import re
import subprocess

from acl_amd import runtime

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID = 1
NAMES = ("aclhip_find_bit_rates_workspace_bytes", "aclhip_find_bit_rates_batch")
# addresses nobody reads: every case returns before a device call
RAWS, RESULTS, WORKSPACE, TABLE, METADATA, RATES, COUNT, MAX_TRACKS, MAX_SAMPLES = 0x10000, 0x20000, 0x800000, 0x30000, 0x40000, 0x100000, 16, 100, 100
SEGMENTS = 6            # of MAX_SAMPLES
SEGMENT_STRIDE, INSTANCE_STRIDE = 4 * MAX_TRACKS, 4 * MAX_TRACKS * SEGMENTS
TABLES = (("default_pose", "the default pose", 48), ("parent_indices", "the parent indices", 4), ("track_precisions", "the track precisions", 4),
          ("track_shell_distances", "the track shell distances", 4))
FIELDS = ("flags", "max_tracks", "max_samples", "num_table_tracks", "default_pose", "parent_indices", "track_precisions", "track_shell_distances", "precision",
          "shell_distance", "workspace", "shell_metadata", "level", "reserved_word", "reserved")
OFFSETS = [0, 4, 8, 12, 16, 24, 32, 40, 48, 52, 56, 64, 72, 76, 80]
CALL = "aclhip_find_bit_rates_batch(gpu, d_raws, num_instances, &search, d_bit_rates, instance_stride, segment_stride, d_results, (void*)hip_stream);"


def test_header_declares_library_exports_and_binding_binds_the_entry_points():
    header = open(os.path.join(ROOT, "include", "aclhip.h")).read()
    declared = set(re.findall(r"\b(aclhip_[a-z_0-9]+)\s*\(", re.sub(r"/\*.*?\*/", "", header, flags=re.S)))
    lib = runtime.load_library()
    for name in NAMES:
        assert name in declared and hasattr(lib, name) and name in runtime.EXPORTED_SYMBOLS, name
    assert "aclhip_find_bit_rates_desc" in header
    assert hasattr(runtime.Context, "find_bit_rates_batch") and callable(runtime.find_bit_rates) and callable(runtime.find_bit_rates_workspace_bytes)
    assert lib.aclhip_abi_version() == runtime.ABI_VERSION == 6       # (added without a bump: no existing struct changed)
    assert runtime.variable_compress_num_segments(MAX_SAMPLES) == SEGMENTS
    # the two remarks that said the search was missing point to it now
    assert "the search does not" not in header and "Left out: the bit rate search and compression levels" not in header


def test_struct_size_and_offsets_match_a_c99_translation_unit(tmp_path):
    lib_dir = os.path.dirname(runtime.library_path())
    binary = tmp_path / "find_bit_rates_abi"
    source = os.path.join(ROOT, "tests", "c", "find_bit_rates_abi.c")
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-I", os.path.join(ROOT, "include"), source, "-L" + lib_dir, "-laclhip",
                    "-Wl,-rpath," + lib_dir, "-o", str(binary)], check=True)
    done = subprocess.run([str(binary)], stdout=subprocess.PIPE, text=True, timeout=120)
    assert done.returncode == 0, done.returncode        # (the program's own checks, INTEGRATION.md's call sequence among them)
    words = [int(word) for word in done.stdout.split()]
    desc = runtime.FindBitRatesDesc
    assert ctypes.sizeof(desc) == words[0] == 96
    assert [getattr(desc, name).offset for name in FIELDS] == words[1:] == OFFSETS
    # the document shows the call the C file compiles
    assert CALL in open(os.path.join(ROOT, "INTEGRATION.md")).read() and CALL in open(source).read()


def search(raws=RAWS, rates=RATES, instance_stride=INSTANCE_STRIDE, segment_stride=SEGMENT_STRIDE, results=RESULTS, count=COUNT, no_desc=False, **fields):
    lib = runtime.load_library()
    desc = runtime.FindBitRatesDesc()
    desc.precision, desc.shell_distance, desc.max_tracks, desc.max_samples, desc.workspace, desc.level = 1.0e-4, 1.0, MAX_TRACKS, MAX_SAMPLES, WORKSPACE, 2
    for name, value in fields.items():
        setattr(desc, name, value)
    status = lib.aclhip_find_bit_rates_batch(None, raws, count, None if no_desc else ctypes.byref(desc), rates, instance_stride, segment_stride, results, None)
    message = lib.aclhip_last_error_message(None).decode()
    assert status == INVALID and message != ""
    return message


def test_every_invalid_argument_has_its_message():
    # what passes the checks ends at the missing context
    assert search() == "null context"
    assert search(flags=7, precision=0.0, shell_distance=0.0, default_pose=TABLE, parent_indices=TABLE, track_precisions=TABLE, track_shell_distances=TABLE,
                  num_table_tracks=7, shell_metadata=METADATA) == "null context"
    assert search(count=0) == "null context"
    for level in (0, 1, 2):
        assert search(level=level) == "null context"
    assert search(instance_stride=SEGMENTS * (SEGMENT_STRIDE + 8) + 4, segment_stride=SEGMENT_STRIDE + 8, rates=RATES * 16) == "null context"      # (strides larger than the minimum)

    # the shared checks, with this call's word; it has no rows to refuse
    assert search(raws=None) == "null raw track handles"
    assert search(no_desc=True) == "null bit rate search desc"
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
        assert search(**fields) == "the reserved fields of a bit rate search desc are 0"
    for value, text in ((-1.0e-5, "-1e-05"), (float("nan"), "nan"), (float("inf"), "inf")):
        assert search(precision=value) == "a precision of %s: it must be finite and not negative" % text
        assert search(shell_distance=value) == "a shell distance of %s: it must be finite and not negative" % text
    for field, _, _ in TABLES:
        assert search(**{field: TABLE}) == "a track table with a count of 0"
    assert search(max_tracks=0) == "a bit rate search desc of 0 max_tracks"

    # its own
    assert search(max_samples=0) == "a bit rate search desc of 0 max_samples"
    assert search(level=3) == "level 3 (high) is not built: 0 (lowest), 1 (low) and 2 (medium) are"
    assert search(level=4) == "level 4 (highest) is not built: 0 (lowest), 1 (low) and 2 (medium) are"
    for level in (5, 255, 0xFFFFFFFF):
        assert search(level=level) == "a level of %u: 0 (lowest), 1 (low) or 2 (medium)" % level
    assert search(rates=None) == "null bit rate table"
    for rates in (RATES + 1, RATES + 2):
        assert search(rates=rates) == "the bit rate table must be 4 byte aligned"
    for strides in ({"instance_stride": INSTANCE_STRIDE + 2}, {"segment_stride": SEGMENT_STRIDE + 1}, {"instance_stride": 1 << 40, "segment_stride": 402}):
        assert search(**strides) == "the strides of the bit rate table are multiples of 4"


def test_the_strides_of_a_written_table_keep_its_writers_apart():
    for segment_stride in (0, 4, SEGMENT_STRIDE - 4):
        assert search(segment_stride=segment_stride) == "a segment stride of %u: a written row takes 4 * max_tracks = %u bytes" % (segment_stride, SEGMENT_STRIDE)
    for instance_stride in (0, SEGMENT_STRIDE, INSTANCE_STRIDE - 4):
        assert search(instance_stride=instance_stride) == "an instance stride of %u: the %u rows of an instance take %u segment strides" % (instance_stride, SEGMENTS, SEGMENTS)
    assert search(instance_stride=SEGMENTS * (SEGMENT_STRIDE + 4) - 4, segment_stride=SEGMENT_STRIDE + 4).startswith("an instance stride of")
    assert search(instance_stride=SEGMENTS * (SEGMENT_STRIDE + 4), segment_stride=SEGMENT_STRIDE + 4) == "null context"
    # one segment: an instance is one row
    assert search(max_samples=31, instance_stride=SEGMENT_STRIDE) == "null context"
    assert search(max_samples=31, instance_stride=SEGMENT_STRIDE - 4).startswith("an instance stride of")


def test_the_table_is_on_the_written_side_of_the_overlap_check():
    """the table -- (COUNT - 1) instance strides, (SEGMENTS - 1) segment strides and 4 * MAX_TRACKS bytes -- against everything else that
    is written and everything that is read: the first and the last byte of each range"""
    table_bytes = (COUNT - 1) * INSTANCE_STRIDE + (SEGMENTS - 1) * SEGMENT_STRIDE + 4 * MAX_TRACKS
    workspace_bytes = runtime.find_bit_rates_workspace_bytes(COUNT, MAX_TRACKS, MAX_SAMPLES)
    others = (("the compress results", RESULTS, COUNT * 8), ("the workspace", WORKSPACE, workspace_bytes), ("the shell metadata", METADATA, COUNT * MAX_TRACKS * 8),
              ("the raw track handles", RAWS, COUNT * 4))
    for what, base, size in others:
        assert search(shell_metadata=METADATA, rates=base + size - 4) == "the bit rate table overlap %s" % what
        assert search(shell_metadata=METADATA, rates=base - table_bytes + 4) == "the bit rate table overlap %s" % what
    assert search(shell_metadata=METADATA, rates=WORKSPACE + workspace_bytes) == "null context"
    for field, what, width in TABLES:
        assert search(num_table_tracks=7, rates=0x1000000, **{field: 0x1000000 + table_bytes - 16}) == "the bit rate table overlap %s" % what
        assert search(num_table_tracks=7, rates=0x1000000, **{field: 0x1000000 + table_bytes}) == "null context"
        assert search(num_table_tracks=7, rates=0x1000000, **{field: 0x1000000 - 7 * width}) == "null context"
    # the workspace is the variable call's and more: a buffer sized for that call is too small to stand in front of the results
    far = 0x4000000
    assert search(results=far, workspace=far - runtime.compress_variable_workspace_bytes(COUNT, MAX_TRACKS, MAX_SAMPLES)) == "the compress results overlap the workspace"
    assert search(results=far, workspace=far - workspace_bytes) == "null context"


def test_the_workspace_size_is_its_formula_and_is_capped():
    def part(size):
        return (size + 15) & ~15

    def segments_of(num_samples):
        if num_samples <= 31:
            return 1
        estimated = (num_samples + 15) // 16
        last = 16 - (estimated * 16 - num_samples)
        return estimated - 1 if (estimated - 1) * 15 >= last else estimated

    def workspace(n, t, s):
        g = segments_of(max(s, 1))
        variable = part(n * 64) + part(n * t) + part(n * t * 6) + part(n * t * 8) + part(n * t * 72) + part(n * g * 32) + part(n * g * t * 12)
        return min(variable + part(n * g * 16) + part(n * g * t * 72) + part(n * g * t * 8) + part(n * g * t * 2), 0xFFFFFFFFFFFFFFF0)
    for n in (0, 1, 2, 41, 4096):
        for t in (1, 2, 65, 1000, 0xFFFF):
            for s in (1, 31, 32, 301, 65535):
                size = runtime.find_bit_rates_workspace_bytes(n, t, s)
                assert size == workspace(n, t, s) and size % 16 == 0
                assert size >= runtime.compress_variable_workspace_bytes(n, t, s)
    assert runtime.find_bit_rates_workspace_bytes(0xFFFFFFFF, 0xFFFFFFFF, 0xFFFFFFFF) == 0xFFFFFFFFFFFFFFF0
