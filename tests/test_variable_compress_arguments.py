"""aclhip_compress_tracks_variable_batch and its three host-only functions without a device: the surface (header, library, binding), the
struct layout against a C99 translation unit, every ACLHIP_ERROR_INVALID_ARGUMENT with its message -- each is decided before any device
call and works without a context --, the two size functions at their caps, aclhip_variable_compress_num_segments against a Python
split_samples_per_segment and its monotonicity, and the bound against the restatement's
(tests/variable_compress_restatement.py)."""
import ctypes
import os
import re
import subprocess

from acl_amd import runtime
import variable_compress_restatement as restatement

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID = 1
NAMES = ("aclhip_variable_compress_num_segments", "aclhip_variable_compress_bound", "aclhip_compress_variable_workspace_bytes", "aclhip_compress_tracks_variable_batch")
# addresses nobody reads: every case returns before a device call
RAWS, BLOBS, RESULTS, WORKSPACE, TABLE, METADATA, RATES, STRIDE, COUNT, MAX_TRACKS, MAX_SAMPLES = 0x10000, 0x100000, 0x20000, 0x800000, 0x30000, 0x40000, 0x60000, 4096, 16, 100, 100
TABLES = (("default_pose", "the default pose", 48), ("parent_indices", "the parent indices", 4), ("track_precisions", "the track precisions", 4),
          ("track_shell_distances", "the track shell distances", 4))
FIELDS = ("flags", "max_tracks", "max_samples", "num_table_tracks", "default_pose", "parent_indices", "track_precisions", "track_shell_distances", "precision",
          "shell_distance", "workspace", "shell_metadata", "bit_rates", "bit_rate_instance_stride", "bit_rate_segment_stride", "rotation_bit_rate", "translation_bit_rate",
          "scale_bit_rate", "reserved_rate", "reserved_word", "reserved")
OFFSETS = [0, 4, 8, 12, 16, 24, 32, 40, 48, 52, 56, 64, 72, 80, 88, 96, 97, 98, 99, 100, 104]
CALL = "aclhip_compress_tracks_variable_batch(gpu, d_raws, num_instances, &desc, d_blobs, stride, d_results, (void*)hip_stream);"


def test_header_declares_library_exports_and_binding_binds_the_entry_points():
    header = open(os.path.join(ROOT, "include", "aclhip.h")).read()
    declared = set(re.findall(r"\b(aclhip_[a-z_0-9]+)\s*\(", re.sub(r"/\*.*?\*/", "", header, flags=re.S)))
    lib = runtime.load_library()
    for name in NAMES:
        assert name in declared and hasattr(lib, name) and name in runtime.EXPORTED_SYMBOLS, name
    assert "aclhip_compress_variable_desc" in header
    assert hasattr(runtime.Context, "compress_tracks_variable_batch") and callable(runtime.compress_tracks_variable) and callable(runtime.compress_tracks_at_precision)
    assert lib.aclhip_abi_version() == runtime.ABI_VERSION == 6       # (added without a bump: no existing struct changed)


def test_struct_size_and_offsets_match_a_c99_translation_unit(tmp_path):
    lib_dir = os.path.dirname(runtime.library_path())
    binary = tmp_path / "compress_variable_abi"
    source = os.path.join(ROOT, "tests", "c", "compress_variable_abi.c")
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-I", os.path.join(ROOT, "include"), source, "-L" + lib_dir, "-laclhip",
                    "-Wl,-rpath," + lib_dir, "-o", str(binary)], check=True)
    done = subprocess.run([str(binary)], stdout=subprocess.PIPE, text=True, timeout=120)
    assert done.returncode == 0, done.returncode        # (the program's own checks, INTEGRATION.md's call sequence among them)
    words = [int(word) for word in done.stdout.split()]
    desc = runtime.CompressVariableDesc
    assert ctypes.sizeof(desc) == words[0] == 120
    assert [getattr(desc, name).offset for name in FIELDS] == words[1:] == OFFSETS
    # the document shows the call the C file compiles
    assert CALL in open(os.path.join(ROOT, "INTEGRATION.md")).read() and CALL in open(source).read()


def compress(raws=RAWS, blobs=BLOBS, stride=STRIDE, results=RESULTS, count=COUNT, no_desc=False, **fields):
    lib = runtime.load_library()
    desc = runtime.CompressVariableDesc()
    desc.precision, desc.shell_distance, desc.max_tracks, desc.max_samples, desc.workspace = 1.0e-4, 1.0, MAX_TRACKS, MAX_SAMPLES, WORKSPACE
    desc.rotation_bit_rate = desc.translation_bit_rate = desc.scale_bit_rate = 16
    for name, value in fields.items():
        setattr(desc, name, value)
    status = lib.aclhip_compress_tracks_variable_batch(None, raws, count, None if no_desc else ctypes.byref(desc), blobs, stride, results, None)
    message = lib.aclhip_last_error_message(None).decode()
    assert status == INVALID and message != ""
    return message


def test_every_invalid_argument_has_its_message():
    # what passes the checks ends at the missing context
    assert compress() == "null context"
    assert compress(flags=7, precision=0.0, shell_distance=0.0, default_pose=TABLE, parent_indices=TABLE, track_precisions=TABLE, track_shell_distances=TABLE,
                    num_table_tracks=7, shell_metadata=METADATA, bit_rates=RATES, bit_rate_instance_stride=4 * MAX_TRACKS * 7, bit_rate_segment_stride=4 * MAX_TRACKS) == "null context"
    assert compress(count=0) == "null context"
    assert compress(rotation_bit_rate=0, translation_bit_rate=24, scale_bit_rate=1) == "null context"      # (0 is refused per instance, where it meets one segment)
    assert compress(bit_rates=RATES, rotation_bit_rate=200) == "null context"                                 # (with a table the uniform rates are not read)

    # the shared checks, with this call's word
    assert compress(raws=None) == "null raw track handles"
    assert compress(no_desc=True) == "null variable compress desc"
    assert compress(blobs=None) == "null blob buffer"
    assert compress(results=None) == "null compress results"
    assert compress(workspace=None) == "null workspace"
    assert compress(stride=0) == "a blob stride of 0"
    for arguments in ({"blobs": BLOBS + 8}, {"stride": STRIDE + 8}, {"stride": 1}):
        assert compress(**arguments) == "the blob buffer and its stride must be 16 byte aligned"
    assert compress(workspace=WORKSPACE + 8) == "the workspace must be 16 byte aligned"
    assert compress(results=RESULTS + 4) == "compress results must be 8 byte aligned"
    assert compress(default_pose=TABLE + 8, num_table_tracks=7) == "the default pose must be 16 byte aligned"
    for field in ("parent_indices", "track_precisions", "track_shell_distances"):
        assert compress(num_table_tracks=7, **{field: TABLE + 2}) == "the track tables must be 4 byte aligned"
    assert compress(shell_metadata=METADATA + 4) == "the shell metadata must be 8 byte aligned"
    for flags in (8, 9, 0x80000000):
        assert compress(flags=flags) == "unknown compress flags 0x%x" % flags
    for fields in ({"reserved": (ctypes.c_uint64 * 2)(0, 1)}, {"reserved": (ctypes.c_uint64 * 2)(1 << 63, 0)}, {"reserved_rate": 1}, {"reserved_word": 1 << 31}):
        assert compress(**fields) == "the reserved fields of a variable compress desc are 0"
    for value, text in ((-1.0e-5, "-1e-05"), (float("nan"), "nan"), (float("inf"), "inf")):
        assert compress(precision=value) == "a precision of %s: it must be finite and not negative" % text
        assert compress(shell_distance=value) == "a shell distance of %s: it must be finite and not negative" % text
    for field, _, _ in TABLES:
        assert compress(**{field: TABLE}) == "a track table with a count of 0"
    assert compress(max_tracks=0) == "a variable compress desc of 0 max_tracks"

    # its own
    assert compress(max_samples=0) == "a variable compress desc of 0 max_samples"
    for rates in (RATES + 1, RATES + 2):
        assert compress(bit_rates=rates) == "the bit rate table must be 4 byte aligned"
    for strides in ({"bit_rate_instance_stride": 6}, {"bit_rate_segment_stride": 401}, {"bit_rate_instance_stride": 1 << 40, "bit_rate_segment_stride": 2}):
        assert compress(bit_rates=RATES, **strides) == "the strides of the bit rate table are multiples of 4"
    assert compress(bit_rate_instance_stride=6) == "null context"           # (without a table the strides are not read)
    for rates in ((25, 16, 16), (16, 255, 16), (0, 0, 25)):
        assert compress(rotation_bit_rate=rates[0], translation_bit_rate=rates[1], scale_bit_rate=rates[2]) == "uniform bit rates of %u, %u and %u: 0 to 24" % rates


def test_every_overlap_of_the_rate_table_has_its_message():
    """the table -- (COUNT - 1) instance strides, (segments of MAX_SAMPLES - 1) segment strides and 4 * MAX_TRACKS bytes -- against
    everything that is written: the first and the last byte of each range. The other overlaps are the drop-w call's, by the same code."""
    segments = runtime.variable_compress_num_segments(MAX_SAMPLES)
    segment_stride, instance_stride = 4 * MAX_TRACKS, 4 * MAX_TRACKS * segments
    workspace_bytes = runtime.compress_variable_workspace_bytes(COUNT, MAX_TRACKS, MAX_SAMPLES)
    written = (("the blob rows", BLOBS, COUNT * STRIDE), ("the compress results", RESULTS, COUNT * 8), ("the workspace", WORKSPACE, workspace_bytes),
               ("the shell metadata", METADATA, COUNT * MAX_TRACKS * 8))
    for strides, table_bytes in (({}, 4 * MAX_TRACKS), ({"bit_rate_segment_stride": segment_stride}, segments * segment_stride),
                                 ({"bit_rate_segment_stride": segment_stride, "bit_rate_instance_stride": instance_stride}, COUNT * instance_stride)):
        for what, base, size in written:
            assert compress(shell_metadata=METADATA, bit_rates=base + size - 4, **strides) == "%s overlap the bit rate table" % what
            assert compress(shell_metadata=METADATA, bit_rates=base - table_bytes + 4, **strides) == "%s overlap the bit rate table" % what
            assert compress(shell_metadata=METADATA, bit_rates=base - table_bytes, **strides) == "null context"
    # the workspace is the drop-w call's and more: a buffer sized for that call is too small to stand in front of the rows
    assert compress(workspace=BLOBS - runtime.compress_tracks_workspace_bytes(COUNT, MAX_TRACKS)) == "the blob rows overlap the workspace"
    assert compress(workspace=BLOBS - workspace_bytes) == "null context"
    assert compress(raws=BLOBS + COUNT * STRIDE - 4) == "the blob rows overlap the raw track handles"


def python_num_segments(num_samples):
    return len(restatement.split_samples_per_segment(num_samples))


def test_num_segments_is_split_samples_per_segment_and_never_falls_with_one_sample_less():
    counts = [runtime.variable_compress_num_segments(s) for s in range(0, 4097)]
    assert counts[1:] == [python_num_segments(s) for s in range(1, 4097)] and counts[0] == 1
    # the looping vote can take one sample away after the caller sized its table: the count for S - 1 never exceeds the count for S
    assert all(counts[s - 1] <= counts[s] for s in range(1, 4097))
    assert [counts[s] for s in (1, 31, 32, 33, 47, 48, 49, 64, 65)] == [1, 1, 2, 2, 2, 2, 3, 3, 4]
    for s in (0xFFFFFFFF, 0xFFFFFFF0, 1 << 31):
        assert runtime.variable_compress_num_segments(s) == python_num_segments_closed(s)
    header = open(os.path.join(ROOT, "include", "aclhip.h")).read()
    assert "aclhip_variable_compress_num_segments(S) rows" in header


def python_num_segments_closed(num_samples):
    """the same split without the loop, for sample counts a list would not hold"""
    if num_samples <= 31:
        return 1
    estimated = (num_samples + 15) // 16
    last = 16 - (estimated * 16 - num_samples)
    return estimated - 1 if (estimated - 1) * 15 >= last else estimated


def test_the_sizes_are_their_formulas_and_are_capped():
    def part(size):
        return (size + 15) & ~15

    def workspace(n, t, s):
        g = python_num_segments_closed(max(s, 1))
        return min(part(n * 64) + part(n * t) + part(n * t * 6) + part(n * t * 8) + part(n * t * 72) + part(n * g * 32) + part(n * g * t * 12), 0xFFFFFFFFFFFFFFF0)
    for n in (0, 1, 2, 41, 4096):
        for t in (1, 2, 65, 1000, 0xFFFF):
            for s in (1, 31, 32, 301, 65535):
                size = runtime.compress_variable_workspace_bytes(n, t, s)
                assert size == workspace(n, t, s) and size % 16 == 0
                assert size >= runtime.compress_tracks_workspace_bytes(n, t)
    assert runtime.compress_variable_workspace_bytes(1, 1, 1) == 64 + 16 + 16 + 16 + 80 + 32 + 16
    assert runtime.compress_variable_workspace_bytes(0xFFFFFFFF, 0xFFFFFFFF, 0xFFFFFFFF) == 0xFFFFFFFFFFFFFFF0
    assert runtime.compress_variable_workspace_bytes(0xFFFFFFFF, 0x1000, 31) == workspace(0xFFFFFFFF, 0x1000, 31) < 0xFFFFFFFFFFFFFFF0
    # the bound: the restatement's formula over its shapes and both flag sets, a multiple of 16, capped
    for t in (0, 1, 3, 4, 5, 17, 65, 0xFFFF):
        for s in (1, 2, 31, 32, 33, 49, 65, 301):
            for flags in (0, restatement.OPTIMIZE_LOOPS, restatement.INCLUDE_PARENT_TRACK_INDICES, restatement.INCLUDE_TRACK_DESCRIPTIONS):
                assert runtime.variable_compress_bound(t, s, flags) == restatement.bound(t, s, flags)
    assert runtime.variable_compress_bound(0xFFFFFFFF, 0xFFFFFFFF, 4) == 0xFFFFFFFFFFFFFFF0
    assert runtime.variable_compress_bound(0x10000, 0x10000, 0) < 0xFFFFFFFFFFFFFFF0


def test_a_restatement_blob_is_never_above_the_bound():
    both = restatement.INCLUDE_PARENT_TRACK_INDICES | restatement.INCLUDE_TRACK_DESCRIPTIONS
    for num_tracks in (1, 3, 4, 5, 17, 65):
        for num_samples in (1, 2, 31, 32, 33, 49, 65):
            parents = restatement.tree(num_tracks, num_tracks)
            samples = restatement.clip(num_samples % 3, num_samples, num_tracks, scales="default" if num_tracks > 17 else "mixed")
            for flags in (0, both | restatement.OPTIMIZE_LOOPS):
                for rate in (1, 24):
                    blob = restatement.compress(samples, 30.0, (rate, rate, rate), parents=parents, flags=flags, precision=0.01, shell_distance=3.0).blob
                    assert blob.size <= runtime.variable_compress_bound(num_tracks, num_samples, flags)
