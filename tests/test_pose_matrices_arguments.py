"""aclhip_pose_matrices_batch and aclhip_measure_pose_error_metric_batch at the C ABI, without a device: declared, exported, bound; the
binding's struct has the C compiler's size and offsets; every ACLHIP_ERROR_INVALID_ARGUMENT case of the header is refused with a message
that names its cause through a NULL context -- the checks run before any device call, so a call that passes all of them ends at "null
context" -- and the overlap rule of the matrix launch: the output overlaps the input nowhere, in place included."""
import ctypes
import os
import subprocess

import pytest

from acl_amd import runtime
from test_capi_symbols import declared_functions
from test_pose_error_arguments import BASE_POSES, ERRORS, LOSSY, RAW, WITH_BASE
from test_pose_error_arguments import call as call_plain_measure

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID = runtime.ERROR_INVALID_ARGUMENT
LOCAL, MATRICES, SKELETONS = 0x10000000, 0x20000000, 0x30000000
# (addresses are compared and checked for alignment, never read: no context, no launch)
N, BONES = 8, 100
STRIDE, MATRIX_STRIDE = BONES * 48, BONES * 64
PASSES = (INVALID, "null context")


def call(local=LOCAL, local_stride=STRIDE, n=N, desc="default", matrices=MATRICES, matrix_stride=MATRIX_STRIDE, **fields):
    """(status, message) of aclhip_pose_matrices_batch through a NULL context; desc: object space with skeleton 1, changed by `fields`"""
    lib = runtime.load_library()
    if desc == "default":
        desc = runtime.PoseMatricesDesc()
        desc.skeleton, desc.object_space, desc.layout = 1, 1, runtime.MATRIX_3X4F_64
        for name, value in fields.items():
            if name == "reserved":
                desc.reserved[value] = 1
            else:
                setattr(desc, name, value)
    status = lib.aclhip_pose_matrices_batch(None, local, local_stride, n, ctypes.byref(desc) if desc is not None else None, matrices, matrix_stride, None)
    return status, lib.aclhip_last_error_message(None).decode()


def call_measure(metric, raw=RAW, lossy=LOSSY, stride=4800, n=N, errors=ERRORS, **fields):
    """(status, message) of aclhip_measure_pose_error_metric_batch through a NULL context, over the desc of test_pose_error_arguments.call"""
    lib = runtime.load_library()
    desc = runtime.PoseErrorDesc()
    desc.skeleton, desc.object_space, desc.shell_distance = 1, 1, 3.0
    for name, value in fields.items():
        if name == "reserved":
            desc.reserved[value] = 1
        else:
            setattr(desc, name, value)
    status = lib.aclhip_measure_pose_error_metric_batch(None, raw, stride, lossy, stride, n, ctypes.byref(desc), metric, errors, None)
    return status, lib.aclhip_last_error_message(None).decode()


def test_header_declares_library_exports_and_binding_mirrors_the_struct(tmp_path):
    for symbol in ("aclhip_pose_matrices_batch", "aclhip_measure_pose_error_metric_batch"):
        assert symbol in declared_functions()
        assert symbol in runtime.EXPORTED_SYMBOLS
        assert hasattr(runtime.load_library(), symbol)
    for method in ("pose_matrices_batch", "measure_pose_error_metric"):
        assert hasattr(runtime.Context, method)
    assert runtime.load_library().aclhip_abi_version() == runtime.ABI_VERSION == 6       # (added without a bump: no existing struct changed)
    lib_dir = os.path.dirname(runtime.library_path())
    binary = tmp_path / "pose_matrices_abi"
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "c", "pose_matrices_abi.c"),
                    "-L" + lib_dir, "-laclhip", "-Wl,-rpath," + lib_dir, "-o", str(binary)], check=True)
    done = subprocess.run([str(binary)], stdout=subprocess.PIPE, text=True, timeout=120)
    assert done.returncode == 0, done.returncode
    words = [int(word) for word in done.stdout.split()]
    struct = runtime.PoseMatricesDesc
    assert ctypes.sizeof(struct) == words[0] == 40
    assert [getattr(struct, name).offset for name in ("skeleton", "instance_skeletons", "object_space", "layout", "reserved")] == words[1:6] == [0, 8, 16, 20, 24]
    assert [runtime.MATRIX_3X4F_64, runtime.ERROR_METRIC_QVVF, runtime.ERROR_METRIC_QVVF_MATRIX3X4F] == words[6:9] == [0, 0, 1]


def test_a_call_that_passes_every_check_ends_at_the_null_context():
    assert call() == PASSES
    for fields in (dict(object_space=0), dict(skeleton=0, instance_skeletons=SKELETONS), dict(skeleton=7, instance_skeletons=SKELETONS)):
        assert call(**fields) == PASSES, fields
    assert call(local_stride=STRIDE + 32, matrix_stride=MATRIX_STRIDE + 48) == PASSES
    assert call(matrix_stride=64) == PASSES               # a row too small for a skeleton is the kernel's refusal, per instance
    assert call(n=0) == PASSES
    for metric in (runtime.ERROR_METRIC_QVVF, runtime.ERROR_METRIC_QVVF_MATRIX3X4F):
        assert call_measure(metric) == PASSES
        assert call_measure(metric, object_space=0) == PASSES
        assert call_measure(metric, lossy=RAW) == PASSES        # what is read may overlap
    assert call_measure(runtime.ERROR_METRIC_QVVF, **WITH_BASE) == PASSES


REFUSED = {
    "null desc": (dict(desc=None), "desc"),
    "null local poses": (dict(local=None), "local pose"),
    "null matrices": (dict(matrices=None), "matrix buffer"),
    "no skeleton at all": (dict(skeleton=0), "skeleton"),
    "an unknown layout": (dict(layout=1), "layout"),
    "unaligned local poses": (dict(local=LOCAL + 8), "local pose buffer and stride"),
    "unaligned local stride": (dict(local_stride=STRIDE + 8), "local pose buffer and stride"),
    "unaligned matrices": (dict(matrices=MATRICES + 4), "matrix buffer and stride"),
    "unaligned matrix stride": (dict(matrix_stride=MATRIX_STRIDE + 8), "matrix buffer and stride"),
    "reserved 0": (dict(reserved=0), "reserved"),
    "reserved 1": (dict(reserved=1), "reserved"),
    "a row beyond 160 KiB of LDS": (dict(local_stride=48 * 3500, matrix_stride=64 * 3500), "LDS"),
}


@pytest.mark.parametrize("name", sorted(REFUSED))
def test_invalid_arguments_are_refused_with_a_message_before_any_device_call(name):
    arguments, cause = REFUSED[name]
    status, message = call(**arguments)
    assert status == INVALID, name
    assert cause in message and message != "null context", (name, message)


def test_the_shape_comes_from_the_smaller_of_the_two_rows():
    # one row beyond the LDS does not refuse the launch while the other is small: min(local / 48, matrix / 64) slots per image
    assert call(local_stride=48 * 3500) == PASSES
    assert call(matrix_stride=64 * 3500) == PASSES
    assert call(local_stride=48 * 3300, matrix_stride=64 * 3300) == PASSES


def test_any_overlap_of_the_output_with_the_input_is_refused():
    size, out_size = STRIDE * N, MATRIX_STRIDE * N
    # in place, the first byte, inside, the last byte of the input; the last byte of the output on the first of the input
    for matrices in (LOCAL, LOCAL + 16, LOCAL + size - 16, LOCAL - out_size + 16):
        status, message = call(matrices=matrices)
        assert status == INVALID and "overlap the local pose rows" in message, (hex(matrices), message)
    status, message = call(matrices=LOCAL, matrix_stride=STRIDE)              # equal strides are no exception
    assert status == INVALID and "overlap the local pose rows" in message
    # ranges that only touch do not overlap
    assert call(matrices=LOCAL + size) == PASSES
    assert call(matrices=LOCAL - out_size) == PASSES
    # the skeleton list is read as well
    for matrices in (SKELETONS, SKELETONS - out_size + 16):
        status, message = call(matrices=matrices, instance_skeletons=SKELETONS)
        assert status == INVALID and "overlap the skeleton list" in message, (hex(matrices), message)
    assert call(matrices=SKELETONS - out_size, instance_skeletons=SKELETONS) == PASSES
    assert call(matrices=LOCAL, n=0) == PASSES                                # no instances: no bytes


def test_the_metric_form_checks_what_the_plain_form_checks_and_its_metric():
    status, message = call_measure(2)
    assert status == INVALID and "unknown error metric 2" in message
    status, message = call_measure(0xFFFFFFFF)
    assert status == INVALID and "unknown error metric" in message
    # the matrix metric takes no additive format, whichever it is
    for additive_format in (runtime.ADDITIVE_RELATIVE, runtime.ADDITIVE_ADDITIVE0, runtime.ADDITIVE_ADDITIVE1):
        status, message = call_measure(runtime.ERROR_METRIC_QVVF_MATRIX3X4F, **dict(WITH_BASE, additive_format=additive_format))
        assert status == INVALID and "matrix error metric takes no additive format" in message, message
    # every refusal of the plain form comes back from the metric form with the same message, for either metric
    cases = (dict(skeleton=0), dict(raw=None), dict(lossy=None), dict(errors=None), dict(raw=RAW + 8), dict(errors=ERRORS + 4), dict(reserved=0), dict(reserved=1),
             dict(additive_format=runtime.ADDITIVE_RELATIVE), dict(base_poses=BASE_POSES, base_pose_stride_bytes=4800), dict(errors=RAW), dict(stride=48 * 1750),
             dict(worst=ERRORS), dict(shell_distances=SKELETONS, num_shell_distances=0))
    for fields in cases:
        plain = dict(fields)
        if "stride" in plain:
            plain["raw_stride"] = plain["lossy_stride"] = plain.pop("stride")
        want = call_plain_measure(**plain)
        assert want[0] == INVALID and want[1] not in ("", "null context"), fields
        for metric in (runtime.ERROR_METRIC_QVVF, runtime.ERROR_METRIC_QVVF_MATRIX3X4F):
            assert call_measure(metric, **fields) == want, (metric, fields)
    lib = runtime.load_library()
    assert lib.aclhip_measure_pose_error_metric_batch(None, RAW, 4800, LOSSY, 4800, N, None, 1, ERRORS, None) == INVALID
    assert "desc" in lib.aclhip_last_error_message(None).decode()
