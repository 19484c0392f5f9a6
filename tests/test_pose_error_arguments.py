"""aclhip_measure_pose_error_batch at the C ABI, without a device: declared, exported, bound; the binding's structs have the C compiler's
sizes and offsets; every ACLHIP_ERROR_INVALID_ARGUMENT case of the header is refused with a message through a NULL context -- the checks
run before any device call, so a call that passes all of them ends at "null context" -- and the overlap rule: what is written overlaps
nothing that is read and no other output, what is read may overlap freely."""
import ctypes
import os
import subprocess

import pytest

from acl_amd import runtime
from test_capi_symbols import declared_functions

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID = runtime.ERROR_INVALID_ARGUMENT
RAW, LOSSY, BASE_POSES, ERRORS, BONE_ERRORS, WORST, SHELLS, SKELETONS = (0x10000000 + k * 0x1000000 for k in range(8))
# (addresses are compared and checked for alignment, never read: no context, no launch)
STRIDE, N, BONES = 4800, 8, 100


def call(raw=RAW, raw_stride=STRIDE, lossy=LOSSY, lossy_stride=STRIDE, n=N, desc="default", errors=ERRORS, **fields):
    """(status, message) of the call through a NULL context; desc: object space with skeleton 1 and shell distance 3, changed by `fields`"""
    lib = runtime.load_library()
    if desc == "default":
        desc = runtime.PoseErrorDesc()
        desc.skeleton, desc.object_space, desc.shell_distance = 1, 1, 3.0
        for name, value in fields.items():
            if name == "reserved":
                desc.reserved[value] = 1
            else:
                setattr(desc, name, value)
    status = lib.aclhip_measure_pose_error_batch(None, raw, raw_stride, lossy, lossy_stride, n, ctypes.byref(desc) if desc is not None else None, errors, None)
    return status, lib.aclhip_last_error_message(None).decode()


def test_header_declares_library_exports_and_binding_mirrors_the_structs(tmp_path):
    assert "aclhip_measure_pose_error_batch" in declared_functions()
    assert "aclhip_measure_pose_error_batch" in runtime.EXPORTED_SYMBOLS
    lib = runtime.load_library()
    assert hasattr(lib, "aclhip_measure_pose_error_batch")
    assert hasattr(runtime.Context, "measure_pose_error") and callable(runtime.clip_error)
    assert lib.aclhip_abi_version() == runtime.ABI_VERSION == 6       # (added without a bump: no existing struct changed)
    lib_dir = os.path.dirname(runtime.library_path())
    binary = tmp_path / "pose_error_abi"
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "c", "pose_error_abi.c"),
                    "-L" + lib_dir, "-laclhip", "-Wl,-rpath," + lib_dir, "-o", str(binary)], check=True)
    done = subprocess.run([str(binary)], stdout=subprocess.PIPE, text=True, timeout=120)
    assert done.returncode == 0, done.returncode
    words = [int(word) for word in done.stdout.split()]
    struct = runtime.PoseErrorDesc
    names = ("skeleton", "instance_skeletons", "object_space", "additive_format", "base_poses", "base_pose_stride_bytes", "shell_distances", "num_shell_distances",
             "shell_distance", "bone_errors", "bone_error_stride_bytes", "worst", "reserved")
    assert ctypes.sizeof(struct) == words[0] == 96
    assert [getattr(struct, name).offset for name in names] == words[1:14] == [0, 8, 16, 20, 24, 32, 40, 48, 52, 56, 64, 72, 80]
    assert [ctypes.sizeof(runtime.PoseError), runtime.PoseError.error.offset, runtime.PoseError.bone.offset] == words[14:17] == [8, 0, 4]
    worst = runtime.PoseErrorWorst
    assert [ctypes.sizeof(worst), worst.error.offset, worst.bone.offset, worst.instance.offset, worst.reserved.offset] == words[17:22] == [16, 0, 4, 8, 12]
    assert runtime.POSE_ERROR_DTYPE.itemsize == 8 and runtime.POSE_ERROR_WORST_DTYPE.itemsize == 16 and runtime.NO_BONE == 0xFFFFFFFF


WITH_BASE = dict(additive_format=runtime.ADDITIVE_ADDITIVE0, base_poses=BASE_POSES, base_pose_stride_bytes=STRIDE)
WITH_BONE_ERRORS = dict(bone_errors=BONE_ERRORS, bone_error_stride_bytes=BONES * 4)
WITH_SHELLS = dict(shell_distances=SHELLS, num_shell_distances=BONES)
EVERYTHING = dict(WITH_BASE, **WITH_BONE_ERRORS, **WITH_SHELLS, worst=WORST, instance_skeletons=SKELETONS)


def test_a_call_that_passes_every_check_ends_at_the_null_context():
    assert call() == (INVALID, "null context")
    for fields in (dict(object_space=0), dict(WITH_BASE, additive_format=runtime.ADDITIVE_RELATIVE), dict(WITH_BASE, object_space=0, additive_format=runtime.ADDITIVE_ADDITIVE1),
                   dict(WITH_BASE, base_pose_stride_bytes=STRIDE + 32), dict(skeleton=0, instance_skeletons=SKELETONS), WITH_BONE_ERRORS, WITH_SHELLS, dict(worst=WORST),
                   dict(WITH_BONE_ERRORS, bone_error_stride_bytes=4), dict(WITH_BONE_ERRORS, bone_errors=BONE_ERRORS + 4), dict(shell_distance=0.0), EVERYTHING):
        assert call(**fields) == (INVALID, "null context"), fields
    assert call(errors=ERRORS + 8) == (INVALID, "null context")
    assert call(lossy_stride=STRIDE * 2) == (INVALID, "null context")
    assert call(n=0) == (INVALID, "null context")
    assert call(n=0, worst=WORST) == (INVALID, "null context")


REFUSED = {
    "null desc": dict(desc=None),
    "null raw poses": dict(raw=None),
    "null lossy poses": dict(lossy=None),
    "null errors": dict(errors=None),
    "no skeleton at all": dict(skeleton=0),
    "a format without base poses": dict(additive_format=runtime.ADDITIVE_RELATIVE),
    "base poses without a format": dict(base_poses=BASE_POSES, base_pose_stride_bytes=STRIDE),
    "an unknown format": dict(WITH_BASE, additive_format=4),
    "a shell table of no entries": dict(shell_distances=SHELLS, num_shell_distances=0),
    "bone errors with stride 0": dict(WITH_BONE_ERRORS, bone_error_stride_bytes=0),
    "bone errors with a stride that is no multiple of 4": dict(WITH_BONE_ERRORS, bone_error_stride_bytes=BONES * 4 + 2),
    "unaligned raw poses": dict(raw=RAW + 8),
    "unaligned raw stride": dict(raw_stride=STRIDE + 8),
    "unaligned lossy poses": dict(lossy=LOSSY + 4),
    "unaligned lossy stride": dict(lossy_stride=STRIDE + 4),
    "unaligned base poses": dict(WITH_BASE, base_poses=BASE_POSES + 8),
    "unaligned base stride": dict(WITH_BASE, base_pose_stride_bytes=STRIDE + 8),
    "unaligned errors": dict(errors=ERRORS + 4),
    "unaligned worst": dict(worst=WORST + 8),
    "reserved 0": dict(reserved=0),
    "reserved 1": dict(reserved=1),
    "two rows beyond 160 KiB of LDS": dict(raw_stride=48 * 1750, lossy_stride=48 * 1750),
}


@pytest.mark.parametrize("name", sorted(REFUSED))
def test_invalid_arguments_are_refused_with_a_message_before_any_device_call(name):
    status, message = call(**REFUSED[name])
    assert status == INVALID, name
    assert message != "" and message != "null context", (name, message)


def test_the_shape_comes_from_the_smaller_input_stride():
    # 1700 transforms twice: 163 200 bytes of images and their pad, inside what a workgroup may ask for; one stride beyond it does not
    # refuse the launch while the other is small
    assert call(raw_stride=48 * 1700, lossy_stride=48 * 1700) == (INVALID, "null context")
    assert call(raw_stride=48 * 3500) == (INVALID, "null context")
    assert call(lossy_stride=48 * 3500) == (INVALID, "null context")


def test_what_is_read_may_overlap():
    assert call(lossy=RAW) == (INVALID, "null context")                       # the same buffer twice
    assert call(lossy=RAW + STRIDE) == (INVALID, "null context")
    assert call(**dict(WITH_BASE, base_poses=RAW)) == (INVALID, "null context")
    assert call(lossy=RAW, **dict(WITH_BASE, base_poses=RAW)) == (INVALID, "null context")


INPUTS = {
    "the raw pose rows": (RAW, STRIDE * N, {}),
    "the lossy pose rows": (LOSSY, STRIDE * N, {}),
    "the base pose rows": (BASE_POSES, STRIDE * N, WITH_BASE),
    "the skeleton list": (SKELETONS, 4 * N, dict(instance_skeletons=SKELETONS)),
    "the shell distances": (SHELLS, 4 * BONES, WITH_SHELLS),
}


@pytest.mark.parametrize("input_name", sorted(INPUTS))
def test_an_output_that_overlaps_an_input_is_refused(input_name):
    begin, size, fields = INPUTS[input_name]
    # the first byte, inside, the last byte; ranges that only touch do not overlap
    for errors in (begin, begin + 8, begin + size - 8, begin - 8 * N + 8):
        status, message = call(errors=errors, **fields)
        assert status == INVALID and "the pose error records overlap " + input_name in message, (hex(errors), message)
    assert call(errors=begin + (size + 7) // 8 * 8, **fields) == (INVALID, "null context")
    assert call(errors=begin - 8 * N, **fields) == (INVALID, "null context")
    row = BONES * 4
    for bone_errors in (begin, begin + size - 4, begin - row * N + 4):
        status, message = call(bone_errors=bone_errors, bone_error_stride_bytes=row, **fields)
        assert status == INVALID and "the bone errors overlap " + input_name in message, (hex(bone_errors), message)
    assert call(bone_errors=begin - row * N, bone_error_stride_bytes=row, **fields) == (INVALID, "null context")
    for worst in (begin, begin + (size - 1) // 16 * 16):
        status, message = call(worst=worst, **fields)
        assert status == INVALID and "the worst record overlap " + input_name in message, (hex(worst), message)
    assert call(worst=begin - 16, **fields) == (INVALID, "null context")


def test_outputs_that_overlap_each_other_are_refused():
    row = BONES * 4
    for bone_errors in (ERRORS, ERRORS + 8 * N - 4, ERRORS - row * N + 4):
        status, message = call(bone_errors=bone_errors, bone_error_stride_bytes=row)
        assert status == INVALID and "the pose error records overlap the bone errors" in message, message
    for worst in (ERRORS, ERRORS + 8 * N - 16):
        status, message = call(worst=worst)
        assert status == INVALID and "the pose error records overlap the worst record" in message, message
    for worst in (BONE_ERRORS, BONE_ERRORS + row * N - 16):
        status, message = call(worst=worst, **WITH_BONE_ERRORS)
        assert status == INVALID and "the bone errors overlap the worst record" in message, message
    # side by side is fine, and nothing is written for no instances but the worst record
    assert call(bone_errors=ERRORS + 8 * N, bone_error_stride_bytes=row, worst=ERRORS + 8 * N + row * N) == (INVALID, "null context")
    assert call(n=0, worst=ERRORS) == (INVALID, "null context")
    status, message = call(n=0, worst=RAW + 16, lossy=RAW)
    assert (status, message) == (INVALID, "null context")
