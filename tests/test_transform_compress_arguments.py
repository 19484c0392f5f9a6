"""aclhip_compress_raw_tracks_batch, aclhip_transform_compress_bound and aclhip_transform_compress_workspace_bytes without a device: the
surface (header, library, binding), the struct layout against a C99 translation unit, every ACLHIP_ERROR_INVALID_ARGUMENT with its
message -- each is decided before any device call and works without a context --, the bound against the restatement's blobs, and the
workspace size."""
import ctypes
import os
import re
import subprocess

import numpy as np

from acl_amd import runtime
import transform_compress_restatement as restatement
from transform_compress_restatement import SAMPLE_COUNTS, TRACK_COUNTS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID = 1
NAMES = ("aclhip_transform_compress_bound", "aclhip_transform_compress_workspace_bytes", "aclhip_compress_raw_tracks_batch")
# addresses nobody reads: every case returns before a device call
RAWS, BLOBS, RESULTS, WORKSPACE, TABLE, STRIDE, COUNT, MAX_TRACKS = 0x10000, 0x100000, 0x20000, 0x800000, 0x30000, 4096, 16, 100
TABLES = (("default_pose", "the default pose", 48), ("parent_indices", "the parent indices", 4), ("track_precisions", "the track precisions", 4),
          ("track_shell_distances", "the track shell distances", 4))


def test_header_declares_library_exports_and_binding_binds_the_entry_points():
    header = open(os.path.join(ROOT, "include", "aclhip.h")).read()
    declared = set(re.findall(r"\b(aclhip_[a-z_0-9]+)\s*\(", re.sub(r"/\*.*?\*/", "", header, flags=re.S)))
    lib = runtime.load_library()
    for name in NAMES:
        assert name in declared and hasattr(lib, name) and name in runtime.EXPORTED_SYMBOLS, name
    assert hasattr(runtime.Context, "compress_raw_tracks_batch") and callable(runtime.compress_raw_tracks)
    assert lib.aclhip_abi_version() == runtime.ABI_VERSION == 6       # (added without a bump: no existing struct changed)
    for name, value in (("ACLHIP_COMPRESS_INCLUDE_PARENT_TRACK_INDICES", runtime.COMPRESS_INCLUDE_PARENT_TRACK_INDICES),
                        ("ACLHIP_COMPRESS_INCLUDE_TRACK_DESCRIPTIONS", runtime.COMPRESS_INCLUDE_TRACK_DESCRIPTIONS),
                        ("ACLHIP_COMPRESS_NOT_NORMALIZED", runtime.COMPRESS_NOT_NORMALIZED)):
        assert int(re.search(r"#define\s+%s\s+(\d+)u" % name, header).group(1)) == value
    assert (runtime.COMPRESS_INCLUDE_PARENT_TRACK_INDICES, runtime.COMPRESS_INCLUDE_TRACK_DESCRIPTIONS) == (restatement.INCLUDE_PARENT_TRACK_INDICES, restatement.INCLUDE_TRACK_DESCRIPTIONS)


def test_struct_size_and_offsets_match_a_c99_translation_unit(tmp_path):
    lib_dir = os.path.dirname(runtime.library_path())
    binary = tmp_path / "transform_compress_abi"
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "c", "transform_compress_abi.c"),
                    "-L" + lib_dir, "-laclhip", "-Wl,-rpath," + lib_dir, "-o", str(binary)], check=True)
    done = subprocess.run([str(binary)], stdout=subprocess.PIPE, text=True, timeout=120)
    assert done.returncode == 0, done.returncode        # (the program's own checks)
    words = [int(word) for word in done.stdout.split()]
    desc = runtime.TransformCompressDesc
    assert ctypes.sizeof(desc) == words[0] == 80 and runtime.COMPRESS_RESULT_DTYPE.itemsize == words[1] == 8
    names = ("flags", "max_tracks", "default_pose", "parent_indices", "track_precisions", "track_shell_distances", "num_table_tracks", "precision", "shell_distance",
             "workspace", "reserved")
    assert [getattr(desc, name).offset for name in names] == words[2:13] == [0, 4, 8, 16, 24, 32, 40, 44, 48, 56, 64]
    assert words[13:17] == [runtime.COMPRESS_OPTIMIZE_LOOPS, runtime.COMPRESS_INCLUDE_PARENT_TRACK_INDICES, runtime.COMPRESS_INCLUDE_TRACK_DESCRIPTIONS, runtime.COMPRESS_NOT_NORMALIZED]


def compress(raws=RAWS, blobs=BLOBS, stride=STRIDE, results=RESULTS, count=COUNT, no_desc=False, **fields):
    lib = runtime.load_library()
    desc = runtime.TransformCompressDesc()
    desc.precision, desc.shell_distance, desc.max_tracks, desc.workspace = 1.0e-4, 1.0, MAX_TRACKS, WORKSPACE
    for name, value in fields.items():
        setattr(desc, name, value)
    status = lib.aclhip_compress_raw_tracks_batch(None, raws, count, None if no_desc else ctypes.byref(desc), blobs, stride, results, None)
    message = lib.aclhip_last_error_message(None).decode()
    assert status == INVALID and message != ""
    return message


def test_every_invalid_argument_has_its_message():
    # what passes the checks ends at the missing context
    assert compress() == "null context"
    assert compress(flags=7, precision=0.0, shell_distance=0.0, default_pose=TABLE, parent_indices=TABLE, track_precisions=TABLE, track_shell_distances=TABLE,
                    num_table_tracks=7) == "null context"
    assert compress(count=0) == "null context"

    assert compress(raws=None) == "null raw track handles"
    assert compress(no_desc=True) == "null transform compress desc"
    assert compress(blobs=None) == "null blob buffer"
    assert compress(results=None) == "null compress results"
    assert compress(workspace=None) == "null workspace"
    assert compress(stride=0) == "a blob stride of 0"
    for arguments in ({"blobs": BLOBS + 8}, {"blobs": BLOBS + 1}, {"stride": STRIDE + 8}, {"stride": STRIDE + 4}, {"stride": 1}):
        assert compress(**arguments) == "the blob buffer and its stride must be 16 byte aligned"
    for workspace in (WORKSPACE + 8, WORKSPACE + 1):
        assert compress(workspace=workspace) == "the workspace must be 16 byte aligned"
    for results in (RESULTS + 4, RESULTS + 1):
        assert compress(results=results) == "compress results must be 8 byte aligned"
    for default_pose in (TABLE + 8, TABLE + 4):
        assert compress(default_pose=default_pose, num_table_tracks=7) == "the default pose must be 16 byte aligned"
    for field in ("parent_indices", "track_precisions", "track_shell_distances"):
        assert compress(num_table_tracks=7, **{field: TABLE + 2}) == "the track tables must be 4 byte aligned"
    for flags in (8, 9, 0x80000000):
        assert compress(flags=flags) == "unknown compress flags 0x%x" % flags
    for reserved in ((0, 1), (1 << 63, 0)):
        assert compress(reserved=(ctypes.c_uint64 * 2)(*reserved)) == "the reserved fields of a transform compress desc are 0"
    for value, text in ((-1.0e-5, "-1e-05"), (float("nan"), "nan"), (float("inf"), "inf"), (float("-inf"), "-inf")):
        assert compress(precision=value) == "a precision of %s: it must be finite and not negative" % text
        assert compress(shell_distance=value) == "a shell distance of %s: it must be finite and not negative" % text
    for field, _, _ in TABLES:
        assert compress(**{field: TABLE}) == "a track table with a count of 0"
    assert compress(max_tracks=0) == "a transform compress desc of 0 max_tracks"


def test_every_overlap_has_its_message():
    """what is written -- COUNT rows of STRIDE bytes, COUNT results, the workspace -- against what is read and against each other: the
    first and the last byte of each range"""
    blob_bytes, result_bytes = COUNT * STRIDE, COUNT * 8
    workspace_bytes = runtime.transform_compress_workspace_bytes(COUNT, MAX_TRACKS)
    for name, base, size in (("the blob rows", BLOBS, blob_bytes), ("the workspace", WORKSPACE, workspace_bytes)):
        # an input that ends on the range's first byte, and one that starts on its last
        assert compress(raws=base - COUNT * 4 + 4) == "%s overlap the raw track handles" % name
        assert compress(raws=base + size - 4) == "%s overlap the raw track handles" % name
        assert compress(raws=base - COUNT * 4) == "null context" and compress(raws=base + size) == "null context"
        for field, what, width in TABLES:
            assert compress(num_table_tracks=16, **{field: base - 16 * width + 16}) == "%s overlap %s" % (name, what)
            assert compress(num_table_tracks=16, **{field: base + size - 16}) == "%s overlap %s" % (name, what)
            assert compress(num_table_tracks=16, **{field: base + size}) == "null context"
            assert compress(num_table_tracks=16, **{field: base - 16 * width}) == "null context"
    assert compress(raws=RESULTS + result_bytes - 4) == "the compress results overlap the raw track handles"
    for field, what, width in TABLES:
        assert compress(num_table_tracks=4, **{field: RESULTS - 4 * width + 16}) == "the compress results overlap %s" % what
    assert compress(results=BLOBS + blob_bytes - 8) == "the blob rows overlap the compress results"
    assert compress(results=BLOBS - result_bytes + 8) == "the blob rows overlap the compress results"
    assert compress(results=BLOBS + blob_bytes) == "null context"
    assert compress(workspace=BLOBS + blob_bytes - 16) == "the blob rows overlap the workspace"
    assert compress(workspace=BLOBS - workspace_bytes + 16) == "the blob rows overlap the workspace"
    assert compress(workspace=BLOBS - workspace_bytes) == "null context"
    assert compress(workspace=RESULTS + result_bytes - 16) == "the compress results overlap the workspace"
    assert compress(workspace=RESULTS + result_bytes) == "null context"


def test_the_bound_is_the_formula_and_never_below_a_blob():
    both = restatement.INCLUDE_PARENT_TRACK_INDICES | restatement.INCLUDE_TRACK_DESCRIPTIONS
    for num_tracks in TRACK_COUNTS:
        for num_samples in SAMPLE_COUNTS:
            for flags in (0, 1, restatement.INCLUDE_PARENT_TRACK_INDICES, restatement.INCLUDE_TRACK_DESCRIPTIONS, both):
                bound = runtime.transform_compress_bound(num_tracks, num_samples, flags)
                assert bound == restatement.bound(num_tracks, num_samples, flags) and bound % 16 == 0
                pose = restatement.bind_pose(3, num_tracks)
                for seed in range(3):
                    for default_pose in (None, pose):
                        for scales in ("mixed", "default"):
                            samples = restatement.clip(seed, num_samples, num_tracks, default_pose=default_pose, scales=scales)
                            assert restatement.compress(samples, 30.0, default_pose=default_pose, flags=flags).size <= bound
                # every sub-track animated (one sample: every sub-track constant, none default): the sections that make the bound
                rng = np.random.default_rng(num_tracks + num_samples)
                full = np.zeros((num_samples, num_tracks, 12), dtype=np.float32)
                full[:, :, 0:4] = restatement.unit_quaternions(rng, (num_samples, num_tracks))
                full[:, :, 4:7] = rng.uniform(1.0, 2.0, size=(num_samples, num_tracks, 3))
                full[:, :, 8:11] = rng.uniform(2.0, 3.0, size=(num_samples, num_tracks, 3))
                size = restatement.compress(full, 30.0, flags=flags).size
                assert bound - 16 - 12 < size <= bound
    # the largest array a registration takes, and counts no array has: nothing wraps
    assert runtime.transform_compress_bound(0xFFFF, 682, 0) == ((100 + 12 * 4096 + 40 * 0xFFFF * 682 + 15 + 15) & ~15)
    assert runtime.transform_compress_bound(0xFFFFFFFF, 0xFFFFFFFF, both) == 0xFFFFFFFFFFFFFFF0
    assert runtime.transform_compress_bound(0xFFFFFFFF, 1, both) == ((100 + 12 * (1 << 28) + 92 * 0xFFFFFFFF + 20 + 15) & ~15)
    assert runtime.transform_compress_bound(0, 0, 0) == 128


def test_the_workspace_size_is_monotone():
    sizes = np.array([[runtime.transform_compress_workspace_bytes(n, t) for t in (1, 2, 63, 64, 65, 1000, 0xFFFF)] for n in (0, 1, 2, 41, 4096, 1 << 20)], dtype=np.uint64)
    assert (sizes % 16 == 0).all() and (sizes[0] == 0).all()
    assert (np.diff(sizes.astype(np.float64), axis=0) > 0).all() and (np.diff(sizes.astype(np.float64), axis=1)[1:] >= 0).all()
    assert (np.diff(sizes.astype(np.float64), axis=1)[3:] > 0).all()
    assert runtime.transform_compress_workspace_bytes(1, 1) == 64 + 16 + 16
    assert runtime.transform_compress_workspace_bytes(1 << 20, 0xFFFF) == (1 << 20) * 64 + (1 << 20) * 0xFFFF + (1 << 20) * 0xFFFF * 6
    # what no address space holds does not wrap into a small number
    assert runtime.transform_compress_workspace_bytes(0xFFFFFFFF, 0xFFFFFFFF) == 0xFFFFFFFFFFFFFFF0
