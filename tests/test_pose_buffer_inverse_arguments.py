"""aclhip_inverse_transform_poses_batch at the C ABI, without a device: declared, exported, bound; the binding's struct has the C compiler's
size and offsets; every ACLHIP_ERROR_INVALID_ARGUMENT case of the header is refused with a message through a NULL context -- the checks run
before any device call, so a call that passes all of them ends at "null context" -- and the overlap cases of the in place rule."""
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


def call(source=BASE, source_stride=STRIDE, n=N, inverse="default", poses=BASE + 0x100000, stride=STRIDE, **fields):
    """(status, message) of the call through a NULL context; inverse: local space with skeleton 1, changed by `fields`"""
    lib = runtime.load_library()
    if inverse == "default":
        inverse = runtime.PoseBufferInverse()
        inverse.skeleton, inverse.local_space = 1, 1
        for name, value in fields.items():
            if name == "reserved":
                inverse.reserved[value] = 1
            else:
                setattr(inverse, name, value)
    status = lib.aclhip_inverse_transform_poses_batch(None, source, source_stride, n, ctypes.byref(inverse) if inverse is not None else None, poses, stride, None)
    return status, lib.aclhip_last_error_message(None).decode()


def test_header_declares_library_exports_and_binding_mirrors_the_struct(tmp_path):
    assert "aclhip_inverse_transform_poses_batch" in declared_functions()
    assert "aclhip_inverse_transform_poses_batch" in runtime.EXPORTED_SYMBOLS
    lib = runtime.load_library()
    assert hasattr(lib, "aclhip_inverse_transform_poses_batch")
    assert lib.aclhip_abi_version() == runtime.ABI_VERSION == 6       # (added without a bump: no existing struct changed)
    lib_dir = os.path.dirname(runtime.library_path())
    binary = tmp_path / "pose_buffer_inverse_abi"
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "c", "pose_buffer_inverse_abi.c"),
                    "-L" + lib_dir, "-laclhip", "-Wl,-rpath," + lib_dir, "-o", str(binary)], check=True)
    done = subprocess.run([str(binary)], stdout=subprocess.PIPE, text=True, timeout=120)
    assert done.returncode == 0, done.returncode
    words = [int(word) for word in done.stdout.split()]
    struct = runtime.PoseBufferInverse
    assert ctypes.sizeof(struct) == words[0] == 64
    offsets = [getattr(struct, name).offset for name in ("skeleton", "instance_skeletons", "local_space", "additive_format", "base_poses", "base_pose_stride_bytes", "reserved")]
    assert offsets == words[1:8] == [0, 8, 16, 20, 24, 32, 40]


WITH_BASE = dict(additive_format=runtime.ADDITIVE_ADDITIVE0, base_poses=BASE + 0x400000, base_pose_stride_bytes=STRIDE)


def test_a_call_that_passes_every_check_ends_at_the_null_context():
    assert call() == (INVALID, "null context")
    for fields in (dict(WITH_BASE, additive_format=runtime.ADDITIVE_RELATIVE), dict(WITH_BASE, local_space=0, additive_format=runtime.ADDITIVE_ADDITIVE1),
                   dict(WITH_BASE, base_pose_stride_bytes=STRIDE + 32), dict(skeleton=0, instance_skeletons=BASE + 0x900000)):
        assert call(**fields) == (INVALID, "null context"), fields
    assert call(n=0) == (INVALID, "null context")


REFUSED = {
    "null inverse": dict(inverse=None),
    "null source poses": dict(source=None),
    "null poses": dict(poses=None),
    "no skeleton at all": dict(skeleton=0),
    "nothing to do": dict(local_space=0),
    "a format without base poses": dict(additive_format=runtime.ADDITIVE_RELATIVE),
    "base poses without a format": dict(base_poses=BASE + 0x400000, base_pose_stride_bytes=STRIDE),
    "an unknown format": dict(WITH_BASE, additive_format=4),
    "unaligned source poses": dict(source=BASE + 8),
    "unaligned source stride": dict(source_stride=STRIDE + 8),
    "unaligned poses": dict(poses=BASE + 0x100004),
    "unaligned stride": dict(stride=STRIDE + 4),
    "unaligned base poses": dict(WITH_BASE, base_poses=BASE + 0x400008),
    "unaligned base stride": dict(WITH_BASE, base_pose_stride_bytes=STRIDE + 8),
    "reserved 0": dict(reserved=0),
    "reserved 1": dict(reserved=1),
    "reserved 2": dict(reserved=2),
    "rows beyond 160 KiB of LDS": dict(stride=48 * 3500, poses=BASE + 0x1000000),
}


@pytest.mark.parametrize("name", sorted(REFUSED))
def test_invalid_arguments_are_refused_with_a_message_before_any_device_call(name):
    status, message = call(**REFUSED[name])
    assert status == INVALID, name
    assert message != "" and message != "null context", (name, message)


def test_the_shape_comes_from_the_output_stride_alone():
    # 3400 transforms: the pose consumers' stated end; a source stride beyond it does not refuse the launch
    assert call(stride=48 * 3400, poses=BASE + 0x1000000) == (INVALID, "null context")
    assert call(source_stride=48 * 3500, poses=BASE + 0x10000000) == (INVALID, "null context")


def test_in_place_is_the_one_overlap_allowed():
    # identical: accepted by the check
    assert call(poses=BASE) == (INVALID, "null context")
    assert call(poses=BASE, **WITH_BASE) == (INVALID, "null context")
    # the same pointer with another stride, shifted by one row (both ways), the last byte of the source range
    for poses, stride in ((BASE, STRIDE + 16), (BASE + STRIDE, STRIDE), (BASE - STRIDE, STRIDE), (BASE + STRIDE * N - 16, STRIDE), (BASE - STRIDE * N + 16, STRIDE)):
        status, message = call(poses=poses, stride=stride)
        assert status == INVALID and "overlap the source pose rows" in message, (hex(poses), stride, message)
    # ranges that touch do not overlap
    assert call(poses=BASE + STRIDE * N) == (INVALID, "null context")
    assert call(poses=BASE - STRIDE * N) == (INVALID, "null context")
    # an output that overlaps the base buffer, identical included; in place over the source rows does not excuse it
    for poses in (BASE + 0x400000, BASE + 0x400000 + STRIDE, BASE + 0x400000 - STRIDE * (N - 1)):
        status, message = call(poses=poses, **WITH_BASE)
        assert status == INVALID and "overlap the base pose rows" in message, (hex(poses), message)
    status, message = call(poses=BASE, **dict(WITH_BASE, base_poses=BASE + STRIDE * (N - 1)))
    assert status == INVALID and "overlap the base pose rows" in message, message
    # the base is only read: it may be the source itself when the output is elsewhere
    assert call(**dict(WITH_BASE, base_poses=BASE)) == (INVALID, "null context")
