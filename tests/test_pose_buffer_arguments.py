"""aclhip_transform_poses_batch at the C ABI, without a device: declared, exported, bound; the binding's struct has the C compiler's size and
offsets; every ACLHIP_ERROR_INVALID_ARGUMENT case of the header is refused with a message through a NULL context -- the checks run before
any device call, so a call that passes all of them ends at "null context" -- and the three overlap cases of the in place rule."""
import ctypes
import os
import subprocess

import pytest

from acl_amd import runtime
from test_capi_symbols import declared_functions

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID = runtime.ERROR_INVALID_ARGUMENT
BASE = 0x10000000        # (addresses are compared and checked for alignment, never read: no context, no launch)
STRIDE, N = 4800, 8


def call(local=BASE, local_stride=STRIDE, n=N, consumers="default", poses=BASE + 0x100000, stride=STRIDE, **fields):
    """(status, message) of the call through a NULL context; consumers: object space with skeleton 1, changed by `fields`"""
    lib = runtime.load_library()
    if consumers == "default":
        consumers = runtime.PoseBufferConsumers()
        consumers.skeleton, consumers.object_space = 1, 1
        for name, value in fields.items():
            if name == "reserved":
                consumers.reserved[value] = 1
            else:
                setattr(consumers, name, value)
    status = lib.aclhip_transform_poses_batch(None, local, local_stride, n, ctypes.byref(consumers) if consumers is not None else None, poses, stride, None)
    return status, lib.aclhip_last_error_message(None).decode()


def test_header_declares_library_exports_and_binding_mirrors_the_struct(tmp_path):
    assert "aclhip_transform_poses_batch" in declared_functions()
    assert "aclhip_transform_poses_batch" in runtime.EXPORTED_SYMBOLS
    lib = runtime.load_library()
    assert hasattr(lib, "aclhip_transform_poses_batch")
    assert lib.aclhip_abi_version() == runtime.ABI_VERSION == 6       # (added without a bump: no existing struct changed)
    lib_dir = os.path.dirname(runtime.library_path())
    binary = tmp_path / "pose_buffer_abi"
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "c", "pose_buffer_abi.c"),
                    "-L" + lib_dir, "-laclhip", "-Wl,-rpath," + lib_dir, "-o", str(binary)], check=True)
    done = subprocess.run([str(binary)], stdout=subprocess.PIPE, text=True, timeout=120)
    assert done.returncode == 0, done.returncode
    words = [int(word) for word in done.stdout.split()]
    struct = runtime.PoseBufferConsumers
    assert ctypes.sizeof(struct) == words[0] == 64
    offsets = [getattr(struct, name).offset for name in ("skeleton", "instance_skeletons", "object_space", "additive_format", "additive_poses",
                                                         "additive_pose_stride_bytes", "bounds", "reserved")]
    assert offsets == words[1:9] == [0, 8, 16, 20, 24, 32, 40, 48]


def test_a_call_that_passes_every_check_ends_at_the_null_context():
    status, message = call()
    assert status == INVALID and message == "null context"
    bounds = runtime.PoseBounds()
    bounds.bounds = BASE + 0x800000
    for fields in (dict(bounds=ctypes.addressof(bounds)), dict(additive_format=runtime.ADDITIVE_RELATIVE, additive_poses=BASE + 0x400000, additive_pose_stride_bytes=STRIDE),
                   dict(object_space=0, additive_format=runtime.ADDITIVE_ADDITIVE1, additive_poses=BASE + 0x400000, additive_pose_stride_bytes=STRIDE),
                   dict(skeleton=0, instance_skeletons=BASE + 0x900000)):
        assert call(**fields) == (INVALID, "null context"), fields
    assert call(poses=None, stride=0, bounds=ctypes.addressof(bounds)) == (INVALID, "null context")      # the boxes alone
    assert call(n=0) == (INVALID, "null context")


BOUNDS_OK = runtime.PoseBounds()
BOUNDS_OK.bounds = BASE + 0x800000
BOUNDS_NO_BUFFER = runtime.PoseBounds()
BOUNDS_UNALIGNED = runtime.PoseBounds()
BOUNDS_UNALIGNED.bounds = BASE + 0x800008
BOUNDS_RESERVED = runtime.PoseBounds()
BOUNDS_RESERVED.bounds = BASE + 0x800000
BOUNDS_RESERVED.reserved[1] = 1
ADDITIVE = dict(additive_format=runtime.ADDITIVE_ADDITIVE0, additive_poses=BASE + 0x400000, additive_pose_stride_bytes=STRIDE)

REFUSED = {
    "null consumers": dict(consumers=None),
    "null local poses": dict(local=None),
    "no skeleton at all": dict(skeleton=0),
    "nothing to do": dict(object_space=0),
    "a format without additive poses": dict(additive_format=runtime.ADDITIVE_RELATIVE),
    "additive poses without a format": dict(additive_poses=BASE + 0x400000, additive_pose_stride_bytes=STRIDE),
    "an unknown format": dict(ADDITIVE, additive_format=4),
    "bounds without object space": dict(ADDITIVE, object_space=0, bounds=ctypes.addressof(BOUNDS_OK)),
    "no output without bounds": dict(poses=None),
    "unaligned local poses": dict(local=BASE + 8),
    "unaligned local stride": dict(local_stride=STRIDE + 8),
    "unaligned poses": dict(poses=BASE + 0x100004),
    "unaligned stride": dict(stride=STRIDE + 4),
    "unaligned additive poses": dict(ADDITIVE, additive_poses=BASE + 0x400008),
    "unaligned additive stride": dict(ADDITIVE, additive_pose_stride_bytes=STRIDE + 8),
    "reserved 0": dict(reserved=0),
    "reserved 1": dict(reserved=1),
    "bounds without a buffer": dict(bounds=ctypes.addressof(BOUNDS_NO_BUFFER)),
    "unaligned bounds": dict(bounds=ctypes.addressof(BOUNDS_UNALIGNED)),
    "bounds with a reserved field": dict(bounds=ctypes.addressof(BOUNDS_RESERVED)),
    "rows beyond 160 KiB of LDS": dict(stride=48 * 3500, poses=BASE + 0x1000000),
    "rows beyond 160 KiB of LDS, boxes alone": dict(local_stride=48 * 3500, poses=None, stride=0, bounds=ctypes.addressof(BOUNDS_OK)),
}


@pytest.mark.parametrize("name", sorted(REFUSED))
def test_invalid_arguments_are_refused_with_a_message_before_any_device_call(name):
    status, message = call(**REFUSED[name])
    assert status == INVALID, name
    assert message != "" and message != "null context", (name, message)


def test_the_largest_shape_that_fits_is_not_refused_for_its_size():
    # 3400 transforms: the pose consumers' stated end
    assert call(stride=48 * 3400, poses=BASE + 0x1000000) == (INVALID, "null context")


def test_in_place_is_the_one_overlap_allowed():
    # identical: accepted by the check
    assert call(poses=BASE) == (INVALID, "null context")
    assert call(poses=BASE, **ADDITIVE) == (INVALID, "null context")
    # the same pointer with another stride, shifted by one row (both ways), the last byte of the input range
    for poses, stride in ((BASE, STRIDE + 16), (BASE + STRIDE, STRIDE), (BASE - STRIDE, STRIDE), (BASE + STRIDE * N - 16, STRIDE), (BASE - STRIDE * N + 16, STRIDE)):
        status, message = call(poses=poses, stride=stride)
        assert status == INVALID and "overlap the local pose rows" in message, (hex(poses), stride, message)
    # ranges that touch do not overlap
    assert call(poses=BASE + STRIDE * N) == (INVALID, "null context")
    assert call(poses=BASE - STRIDE * N) == (INVALID, "null context")
    # an output that overlaps the additive buffer, identical included; in place over the local rows does not excuse it
    for poses in (BASE + 0x400000, BASE + 0x400000 + STRIDE, BASE + 0x400000 - STRIDE * (N - 1)):
        status, message = call(poses=poses, **ADDITIVE)
        assert status == INVALID and "overlap the additive pose rows" in message, (hex(poses), message)
    status, message = call(poses=BASE, **dict(ADDITIVE, additive_poses=BASE + STRIDE * (N - 1)))
    assert status == INVALID and "overlap the additive pose rows" in message, message
    # the boxes alone: no output range, nothing to overlap
    assert call(poses=None, stride=0, bounds=ctypes.addressof(BOUNDS_OK), **dict(ADDITIVE, additive_poses=BASE)) == (INVALID, "null context")
