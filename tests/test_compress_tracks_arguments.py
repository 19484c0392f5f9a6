"""aclhip_compress_tracks_batch and aclhip_compress_tracks_workspace_bytes without a device: the surface (header, library, binding), the
struct layout against a C99 translation unit, every ACLHIP_ERROR_INVALID_ARGUMENT with its message -- each is decided before any device
call and works without a context --, format values that are no format of the reference, the workspace size, and the restatement's blobs
(tests/lossy_rotation_compress_restatement.py) against aclhip_transform_compress_bound, which stays the bound."""
import ctypes
import os
import re
import subprocess

import numpy as np

from acl_amd import runtime
import lossy_rotation_compress_restatement as restatement

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID = 1
NAMES = ("aclhip_compress_tracks_workspace_bytes", "aclhip_compress_tracks_batch")
# addresses nobody reads: every case returns before a device call
RAWS, BLOBS, RESULTS, WORKSPACE, TABLE, METADATA, STRIDE, COUNT, MAX_TRACKS = 0x10000, 0x100000, 0x20000, 0x800000, 0x30000, 0x40000, 4096, 16, 100
TABLES = (("default_pose", "the default pose", 48), ("parent_indices", "the parent indices", 4), ("track_precisions", "the track precisions", 4),
          ("track_shell_distances", "the track shell distances", 4))
FIELDS = ("rotation_format", "translation_format", "scale_format", "flags", "max_tracks", "num_table_tracks", "default_pose", "parent_indices", "track_precisions",
          "track_shell_distances", "precision", "shell_distance", "workspace", "shell_metadata", "reserved")
OFFSETS = [0, 4, 8, 12, 16, 20, 24, 32, 40, 48, 56, 60, 64, 72, 80]


def test_header_declares_library_exports_and_binding_binds_the_entry_points():
    header = open(os.path.join(ROOT, "include", "aclhip.h")).read()
    declared = set(re.findall(r"\b(aclhip_[a-z_0-9]+)\s*\(", re.sub(r"/\*.*?\*/", "", header, flags=re.S)))
    lib = runtime.load_library()
    for name in NAMES:
        assert name in declared and hasattr(lib, name) and name in runtime.EXPORTED_SYMBOLS, name
    assert "aclhip_compress_tracks_desc" in header
    assert hasattr(runtime.Context, "compress_tracks_batch") and callable(runtime.compress_tracks)
    assert lib.aclhip_abi_version() == runtime.ABI_VERSION == 6       # (added without a bump: no existing struct changed)
    assert (runtime.ROTATION_QUATF_FULL, runtime.ROTATION_QUATF_DROP_W_FULL) == (restatement.QUATF_FULL, restatement.QUATF_DROP_W_FULL) == (0, 2)
    # the header says that the raw call's bound stays the bound
    assert re.search(r"aclhip_transform_compress_bound\(T, S, flags\) STAYS THE BOUND", header)


def test_struct_size_and_offsets_match_a_c99_translation_unit(tmp_path):
    lib_dir = os.path.dirname(runtime.library_path())
    binary = tmp_path / "compress_tracks_abi"
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "c", "compress_tracks_abi.c"),
                    "-L" + lib_dir, "-laclhip", "-Wl,-rpath," + lib_dir, "-o", str(binary)], check=True)
    done = subprocess.run([str(binary)], stdout=subprocess.PIPE, text=True, timeout=120)
    assert done.returncode == 0, done.returncode        # (the program's own checks, INTEGRATION.md's call sequence among them)
    words = [int(word) for word in done.stdout.split()]
    desc = runtime.CompressTracksDesc
    assert ctypes.sizeof(desc) == words[0] == 96
    assert [getattr(desc, name).offset for name in FIELDS] == words[1:16] == OFFSETS
    # the document shows the call the C file compiles
    integration = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert "aclhip_compress_tracks_batch(gpu, d_raws, num_instances, &desc, d_blobs, stride, d_results, (void*)hip_stream);" in integration
    assert "aclhip_compress_tracks_batch(gpu, d_raws, num_instances, &desc, d_blobs, stride, d_results, (void*)hip_stream);" in open(os.path.join(ROOT, "tests", "c", "compress_tracks_abi.c")).read()


def compress(raws=RAWS, blobs=BLOBS, stride=STRIDE, results=RESULTS, count=COUNT, no_desc=False, **fields):
    lib = runtime.load_library()
    desc = runtime.CompressTracksDesc()
    desc.rotation_format, desc.precision, desc.shell_distance, desc.max_tracks, desc.workspace = 2, 1.0e-4, 1.0, MAX_TRACKS, WORKSPACE
    for name, value in fields.items():
        setattr(desc, name, value)
    status = lib.aclhip_compress_tracks_batch(None, raws, count, None if no_desc else ctypes.byref(desc), blobs, stride, results, None)
    message = lib.aclhip_last_error_message(None).decode()
    assert status == INVALID and message != ""
    return message


def test_every_invalid_argument_has_its_message():
    # what passes the checks ends at the missing context
    assert compress() == "null context"
    assert compress(rotation_format=0) == "null context"
    assert compress(flags=7, precision=0.0, shell_distance=0.0, default_pose=TABLE, parent_indices=TABLE, track_precisions=TABLE, track_shell_distances=TABLE,
                    num_table_tracks=7, shell_metadata=METADATA) == "null context"
    assert compress(count=0) == "null context"

    assert compress(raws=None) == "null raw track handles"
    assert compress(no_desc=True) == "null tracks compress desc"
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
    for shell_metadata in (METADATA + 4, METADATA + 1):
        assert compress(shell_metadata=shell_metadata) == "the shell metadata must be 8 byte aligned"
    for flags in (8, 9, 0x80000000):
        assert compress(flags=flags) == "unknown compress flags 0x%x" % flags
    for reserved in ((0, 1), (1 << 63, 0)):
        assert compress(reserved=(ctypes.c_uint64 * 2)(*reserved)) == "the reserved fields of a tracks compress desc are 0"
    for value, text in ((-1.0e-5, "-1e-05"), (float("nan"), "nan"), (float("inf"), "inf"), (float("-inf"), "-inf")):
        assert compress(precision=value) == "a precision of %s: it must be finite and not negative" % text
        assert compress(shell_distance=value) == "a shell distance of %s: it must be finite and not negative" % text
    for field, _, _ in TABLES:
        assert compress(**{field: TABLE}) == "a track table with a count of 0"
    assert compress(max_tracks=0) == "a tracks compress desc of 0 max_tracks"


def test_values_that_are_no_format_of_the_reference():
    """acl::rotation_format8 has 0, 2 and 3, acl::vector_format8 0 and 1 (the reference's variable formats, 3 and 1, are refused as not
    built: no test pins that)"""
    for value in (1, 4, 5, 255, 0xFFFFFFFF):
        assert compress(rotation_format=value) == "a rotation format of %u: 0 (quatf_full) or 2 (quatf_drop_w_full)" % value
    for value in (2, 3, 255, 0xFFFFFFFF):
        assert compress(translation_format=value) == "a translation format of %u: 0 (vector3f_full)" % value
        assert compress(scale_format=value) == "a scale format of %u: 0 (vector3f_full)" % value
        assert compress(rotation_format=0, scale_format=value) == "a scale format of %u: 0 (vector3f_full)" % value


def test_every_overlap_has_its_message():
    """what is written -- COUNT rows of STRIDE bytes, COUNT results, the workspace, the shell metadata -- against what is read and against
    each other: the first and the last byte of each range"""
    blob_bytes, result_bytes, metadata_bytes = COUNT * STRIDE, COUNT * 8, COUNT * MAX_TRACKS * 8
    workspace_bytes = runtime.compress_tracks_workspace_bytes(COUNT, MAX_TRACKS)
    for name, base, size in (("the blob rows", BLOBS, blob_bytes), ("the workspace", WORKSPACE, workspace_bytes)):
        assert compress(raws=base - COUNT * 4 + 4) == "%s overlap the raw track handles" % name
        assert compress(raws=base + size - 4) == "%s overlap the raw track handles" % name
        assert compress(raws=base - COUNT * 4) == "null context" and compress(raws=base + size) == "null context"
        for field, what, width in TABLES:
            assert compress(num_table_tracks=16, **{field: base - 16 * width + 16}) == "%s overlap %s" % (name, what)
            assert compress(num_table_tracks=16, **{field: base + size - 16}) == "%s overlap %s" % (name, what)
            assert compress(num_table_tracks=16, **{field: base + size}) == "null context"
            assert compress(num_table_tracks=16, **{field: base - 16 * width}) == "null context"
    assert compress(raws=RESULTS + result_bytes - 4) == "the compress results overlap the raw track handles"
    assert compress(results=BLOBS + blob_bytes - 8) == "the blob rows overlap the compress results"
    assert compress(workspace=BLOBS + blob_bytes - 16) == "the blob rows overlap the workspace"
    assert compress(workspace=BLOBS - workspace_bytes + 16) == "the blob rows overlap the workspace"
    assert compress(workspace=BLOBS - workspace_bytes) == "null context"
    assert compress(workspace=RESULTS + result_bytes - 16) == "the compress results overlap the workspace"
    # the workspace is the raw call's and 8 bytes per instance and track: a buffer sized for the raw call is too small to stand in front of the rows
    assert compress(workspace=BLOBS - runtime.transform_compress_workspace_bytes(COUNT, MAX_TRACKS)) == "the blob rows overlap the workspace"
    # the shell metadata against everything else
    assert compress(shell_metadata=METADATA) == "null context"
    for what, base, size in (("the blob rows", BLOBS, blob_bytes), ("the compress results", RESULTS, result_bytes), ("the workspace", WORKSPACE, workspace_bytes),
                             ("the raw track handles", RAWS, COUNT * 4)):
        assert compress(shell_metadata=base + size - 8) == "the shell metadata overlap %s" % what
        assert compress(shell_metadata=base - metadata_bytes + 8) == "the shell metadata overlap %s" % what
        assert compress(shell_metadata=base + size + (-(base + size)) % 8) == "null context"
    for field, what, width in TABLES:
        assert compress(num_table_tracks=16, shell_metadata=METADATA, **{field: METADATA + metadata_bytes - 16}) == "the shell metadata overlap %s" % what
        assert compress(num_table_tracks=16, shell_metadata=METADATA, **{field: METADATA + metadata_bytes}) == "null context"


def test_the_workspace_size_is_the_formula():
    def formula(n, t):
        def part(size):
            return (size + 15) & ~15
        return min(part(n * 64) + part(n * t) + part(n * t * 6) + part(n * t * 8), 0xFFFFFFFFFFFFFFF0)
    for n in (0, 1, 2, 41, 4096, 1 << 20):
        for t in (1, 2, 63, 64, 65, 1000, 0xFFFF):
            size = runtime.compress_tracks_workspace_bytes(n, t)
            assert size == formula(n, t) and size % 16 == 0
            assert size >= runtime.transform_compress_workspace_bytes(n, t) + n * t * 8
    assert runtime.compress_tracks_workspace_bytes(1, 1) == 64 + 16 + 16 + 16
    # what no address space holds does not wrap into a small number: computed 128 bits wide and capped
    assert runtime.compress_tracks_workspace_bytes(0xFFFFFFFF, 0xFFFFFFFF) == 0xFFFFFFFFFFFFFFF0
    assert runtime.compress_tracks_workspace_bytes(0xFFFFFFFF, 0x10000000) == formula(0xFFFFFFFF, 0x10000000) < 0xFFFFFFFFFFFFFFF0
    assert runtime.compress_tracks_workspace_bytes(0xFFFFFFFF, 0x80000000) == 0xFFFFFFFFFFFFFFF0


def test_a_restatement_blob_is_never_above_the_raw_bound():
    both = restatement.INCLUDE_PARENT_TRACK_INDICES | restatement.INCLUDE_TRACK_DESCRIPTIONS
    for num_tracks in (1, 16, 17, 65):
        for num_samples in (1, 2, 65):
            parents = restatement.tree(num_tracks, num_tracks)
            for flags in (0, restatement.OPTIMIZE_LOOPS, restatement.INCLUDE_PARENT_TRACK_INDICES, both):
                bound = runtime.transform_compress_bound(num_tracks, num_samples, flags)
                for seed in range(2):
                    samples = restatement.clip(seed, num_samples, num_tracks)
                    assert restatement.compress(samples, 30.0, parents=parents, flags=flags, precision=0.01, shell_distance=3.0).blob.size <= bound
            # every sub-track animated: the drop-w blob is the raw one less 4 bytes per rotation and sample
            rng = np.random.default_rng(num_tracks + num_samples)
            full = np.zeros((num_samples, num_tracks, 12), dtype=np.float32)
            full[:, :, 0:4] = restatement.raw_restatement.unit_quaternions(rng, (num_samples, num_tracks))
            full[:, :, 4:7] = rng.uniform(1.0, 2.0, size=(num_samples, num_tracks, 3))
            full[:, :, 8:11] = rng.uniform(2.0, 3.0, size=(num_samples, num_tracks, 3))
            size = restatement.compress(full, 30.0, flags=both).blob.size
            assert size == restatement.raw_restatement.compress(full, 30.0, flags=both).size - 4 * num_tracks * num_samples <= runtime.transform_compress_bound(num_tracks, num_samples, both)
