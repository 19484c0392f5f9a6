"""aclhip_compress_raw_scalar_tracks_batch, aclhip_scalar_compress_bound and aclhip_scalar_compress_workspace_bytes without a device:
the surface (header, library, binding), the two struct layouts, every ACLHIP_ERROR_INVALID_ARGUMENT with its message -- each is decided
before any device call and works without a context --, the bound against the restatement's blobs, and the workspace size."""
import ctypes
import os
import re

import numpy as np

from acl_amd import runtime
import scalar_compress_restatement as restatement
from scalar_compress_restatement import COMPONENTS, PRECISIONS, SWEEP

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID = 1
NAMES = ("aclhip_scalar_compress_bound", "aclhip_scalar_compress_workspace_bytes", "aclhip_compress_raw_scalar_tracks_batch")
# addresses nobody reads: every case returns before a device call
RAWS, BLOBS, RESULTS, WORKSPACE, PRECISION_TABLE, STRIDE, COUNT, MAX_TRACKS = 0x10000, 0x100000, 0x20000, 0x800000, 0x30000, 4096, 16, 100


def test_header_declares_library_exports_and_binding_binds_the_entry_points():
    header = open(os.path.join(ROOT, "include", "aclhip.h")).read()
    declared = set(re.findall(r"\b(aclhip_[a-z_0-9]+)\s*\(", re.sub(r"/\*.*?\*/", "", header, flags=re.S)))
    lib = runtime.load_library()
    for name in NAMES:
        assert name in declared and hasattr(lib, name) and name in runtime.EXPORTED_SYMBOLS, name
    assert hasattr(runtime.Context, "compress_raw_scalar_tracks_batch") and callable(runtime.compress_scalar_tracks)
    assert lib.aclhip_abi_version() == runtime.ABI_VERSION == 6       # (added without a bump: no existing struct changed)
    for name, value in (("ACLHIP_COMPRESS_OPTIMIZE_LOOPS", runtime.COMPRESS_OPTIMIZE_LOOPS), ("ACLHIP_COMPRESS_OK", runtime.COMPRESS_OK),
                        ("ACLHIP_COMPRESS_NOT_FINITE", runtime.COMPRESS_NOT_FINITE), ("ACLHIP_COMPRESS_REFUSED", runtime.COMPRESS_REFUSED)):
        assert int(re.search(r"#define\s+%s\s+(\d+)u" % name, header).group(1)) == value


def test_struct_layouts():
    desc = runtime.ScalarCompressDesc
    assert ctypes.sizeof(desc) == 48
    names = ("precision", "flags", "track_precisions", "num_track_precisions", "max_tracks", "workspace", "reserved")
    assert [getattr(desc, name).offset for name in names] == [0, 4, 8, 16, 20, 24, 32]
    assert runtime.COMPRESS_RESULT_DTYPE.itemsize == 8 and runtime.COMPRESS_RESULT_DTYPE.fields["size"][1] == 4


def compress(raws=RAWS, blobs=BLOBS, stride=STRIDE, results=RESULTS, count=COUNT, no_desc=False, **fields):
    lib = runtime.load_library()
    desc = runtime.ScalarCompressDesc()
    desc.precision, desc.max_tracks, desc.workspace = 1.0e-4, MAX_TRACKS, WORKSPACE
    for name, value in fields.items():
        setattr(desc, name, value)
    status = lib.aclhip_compress_raw_scalar_tracks_batch(None, raws, count, None if no_desc else ctypes.byref(desc), blobs, stride, results, None)
    message = lib.aclhip_last_error_message(None).decode()
    assert status == INVALID and message != ""
    return message


def test_every_invalid_argument_has_its_message():
    # what passes the checks ends at the missing context
    assert compress() == "null context"
    assert compress(flags=runtime.COMPRESS_OPTIMIZE_LOOPS, precision=0.0, track_precisions=PRECISION_TABLE, num_track_precisions=7) == "null context"
    assert compress(count=0) == "null context"

    assert compress(raws=None) == "null raw scalar track handles"
    assert compress(no_desc=True) == "null scalar compress desc"
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
    for flags in (2, 3, 0x80000000):
        assert compress(flags=flags) == "unknown compress flags 0x%x" % flags
    for reserved in ((0, 1), (1 << 63, 0)):
        assert compress(reserved=(ctypes.c_uint64 * 2)(*reserved)) == "the reserved fields of a scalar compress desc are 0"
    for precision, text in ((-1.0e-5, "-1e-05"), (float("nan"), "nan"), (float("inf"), "inf"), (float("-inf"), "-inf")):
        assert compress(precision=precision) == "a precision of %s: it must be finite and not negative" % text
    assert compress(track_precisions=PRECISION_TABLE) == "track_precisions with a count of 0"
    assert compress(max_tracks=0) == "a scalar compress desc of 0 max_tracks"


def test_every_overlap_has_its_message():
    """what is written -- COUNT rows of STRIDE bytes, COUNT results, the workspace -- against what is read and against each other: the
    first and the last byte of each range"""
    blob_bytes, result_bytes = COUNT * STRIDE, COUNT * 8
    workspace_bytes = runtime.scalar_compress_workspace_bytes(COUNT, MAX_TRACKS)
    for name, base, size in (("the blob rows", BLOBS, blob_bytes), ("the workspace", WORKSPACE, workspace_bytes)):
        # an input that ends on the range's first byte, and one that starts on its last
        assert compress(raws=base - COUNT * 4 + 4) == "%s overlap the raw scalar track handles" % name
        assert compress(raws=base + size - 4) == "%s overlap the raw scalar track handles" % name
        assert compress(raws=base - COUNT * 4) == "null context" and compress(raws=base + size) == "null context"
        assert compress(track_precisions=base - 7 * 4 + 4, num_track_precisions=7) == "%s overlap the track precisions" % name
        assert compress(track_precisions=base + size - 4, num_track_precisions=7) == "%s overlap the track precisions" % name
        assert compress(track_precisions=base + size, num_track_precisions=7) == "null context"
    assert compress(raws=RESULTS + result_bytes - 4) == "the compress results overlap the raw scalar track handles"
    assert compress(track_precisions=RESULTS - 8, num_track_precisions=3) == "the compress results overlap the track precisions"
    assert compress(results=BLOBS + blob_bytes - 8) == "the blob rows overlap the compress results"
    assert compress(results=BLOBS - result_bytes + 8) == "the blob rows overlap the compress results"
    assert compress(results=BLOBS + blob_bytes) == "null context"
    assert compress(workspace=BLOBS + blob_bytes - 16) == "the blob rows overlap the workspace"
    assert compress(workspace=BLOBS - workspace_bytes + 16) == "the blob rows overlap the workspace"
    assert compress(workspace=BLOBS - workspace_bytes) == "null context"
    assert compress(workspace=RESULTS + result_bytes - 16) == "the compress results overlap the workspace"
    assert compress(workspace=RESULTS + result_bytes) == "null context"


def test_the_bound_is_the_formula_and_never_below_a_blob():
    for track_type, c in COMPONENTS.items():
        for num_samples, num_tracks in SWEEP:
            bound = runtime.scalar_compress_bound(track_type, num_tracks, num_samples)
            assert bound == restatement.bound(track_type, num_tracks, num_samples) and bound % 16 == 0
            samples = restatement.curves(9100 + 100 * track_type + num_tracks + num_samples, num_samples, num_tracks, c)
            for precision in PRECISIONS:
                for loops in (False, True):
                    assert restatement.compress(restatement.with_last_sample(samples, "equal"), track_type, 30.0, precision=precision, optimize_loops=loops).size <= bound
        # every track raw, and every track quantized at 23 bits with its range: the two sections that make the bound
        assert restatement.compress(restatement.special_list(c)[:, 4:6], track_type, 30.0, precision=0.0).size <= runtime.scalar_compress_bound(track_type, 2, 19)
    for track_type in (5, 11, 12, 13, 255, 0xFFFFFFFF):
        assert runtime.scalar_compress_bound(track_type, 10, 10) == 0
    # the largest array a registration takes: no 32 bit overflow
    assert runtime.scalar_compress_bound(4, 0xFFFF, 2047) == ((52 + 0x10000 + 8 * 4 * 0xFFFF + 4 * 4 * 0xFFFF * 2047 + 15 + 15) & ~15)


def test_the_workspace_size_is_monotone():
    sizes = np.array([[runtime.scalar_compress_workspace_bytes(n, t) for t in (1, 2, 63, 64, 65, 1000, 0xFFFF)] for n in (0, 1, 2, 41, 4096, 1 << 20)], dtype=np.uint64)
    assert (sizes % 16 == 0).all() and (sizes[0] == 0).all()
    assert (np.diff(sizes.astype(np.float64), axis=0) > 0).all() and (np.diff(sizes.astype(np.float64), axis=1)[1:] > 0).all()
    assert runtime.scalar_compress_workspace_bytes(1, 1) >= 64 + 56
    assert runtime.scalar_compress_workspace_bytes(1 << 20, 0xFFFF) == (((1 << 20) * (64 + 56 * 0xFFFF) + 15) & ~15)
    # what no address space holds does not wrap into a small number
    assert runtime.scalar_compress_workspace_bytes(0xFFFFFFFF, 0xFFFFFFFF) == 0xFFFFFFFFFFFFFFF0
