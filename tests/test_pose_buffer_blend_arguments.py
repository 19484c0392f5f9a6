"""aclhip_blend_poses_batch at the C ABI, without a device: declared, exported, bound; the binding's struct has the C compiler's size and
offsets; every ACLHIP_ERROR_INVALID_ARGUMENT case of the header is refused with a message through a NULL context -- the checks run before
any device call, so a call that passes all of them ends at "null context" -- and the overlap cases of the in place rule."""
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
SPACING = 0x100000       # between the input buffers
OUT = BASE + 0x800000
WEIGHTS, MASKS, BOXES = BASE + 0xA00000, BASE + 0xA10000, BASE + 0xA20000
WEIGHTED, LAYERED = runtime.BLEND_WEIGHTED, runtime.BLEND_LAYERED


def blend_of(k=2, mode=WEIGHTED, masks=False, object_space=1, strides=None, **fields):
    """K buffers SPACING apart, each of stride STRIDE (or strides[k]), skeleton 1, changed by `fields`: buffer<k> / stride<k> set one entry"""
    blend = runtime.PoseBufferBlend()
    blend.skeleton, blend.num_buffers, blend.mode, blend.object_space = 1, k, mode, object_space
    for index in range(min(k, 4)):
        blend.buffers[index] = BASE + index * SPACING
        blend.buffer_stride_bytes[index] = STRIDE if strides is None else strides[index]
    blend.weights = WEIGHTS
    blend.instance_masks = MASKS if masks else None
    for name, value in fields.items():
        if name == "reserved":
            blend.reserved[value] = 1
        elif name.startswith("buffer") and name[6:].isdigit():
            blend.buffers[int(name[6:])] = value
        elif name.startswith("stride") and name[6:].isdigit():
            blend.buffer_stride_bytes[int(name[6:])] = value
        else:
            setattr(blend, name, value)
    return blend


def call(blend="default", n=N, poses=OUT, stride=STRIDE, **fields):
    """(status, message) of the call through a NULL context"""
    lib = runtime.load_library()
    if blend == "default":
        blend = blend_of(**fields)
    status = lib.aclhip_blend_poses_batch(None, ctypes.byref(blend) if blend is not None else None, n, poses, stride, None)
    return status, lib.aclhip_last_error_message(None).decode()


FIELDS = ("skeleton", "instance_skeletons", "num_buffers", "mode", "buffers", "buffer_stride_bytes", "weights", "instance_masks", "object_space",
          "reserved0", "bounds", "reserved")


def test_header_declares_library_exports_and_binding_mirrors_the_struct(tmp_path):
    assert "aclhip_blend_poses_batch" in declared_functions()
    assert "aclhip_blend_poses_batch" in runtime.EXPORTED_SYMBOLS
    lib = runtime.load_library()
    assert hasattr(lib, "aclhip_blend_poses_batch")
    assert lib.aclhip_abi_version() == runtime.ABI_VERSION == 6       # (added without a bump: no existing struct changed)
    lib_dir = os.path.dirname(runtime.library_path())
    binary = tmp_path / "pose_buffer_blend_abi"
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "c", "pose_buffer_blend_abi.c"),
                    "-L" + lib_dir, "-laclhip", "-Wl,-rpath," + lib_dir, "-o", str(binary)], check=True)
    done = subprocess.run([str(binary)], stdout=subprocess.PIPE, text=True, timeout=120)
    assert done.returncode == 0, done.returncode
    words = [int(word) for word in done.stdout.split()]
    struct = runtime.PoseBufferBlend
    assert ctypes.sizeof(struct) == words[0] == 136
    offsets = [getattr(struct, name).offset for name in FIELDS]
    assert offsets == words[1:1 + len(FIELDS)] == [0, 8, 16, 20, 24, 56, 88, 96, 104, 108, 112, 120]
    assert len(words) == 1 + len(FIELDS)


BOUNDS_OK = runtime.PoseBounds()
BOUNDS_OK.bounds = BOXES
BOUNDS_NO_BUFFER = runtime.PoseBounds()
BOUNDS_UNALIGNED = runtime.PoseBounds()
BOUNDS_UNALIGNED.bounds = BOXES + 8
BOUNDS_RESERVED = runtime.PoseBounds()
BOUNDS_RESERVED.bounds = BOXES
BOUNDS_RESERVED.reserved[1] = 1


@pytest.mark.parametrize("masks", [False, True])
@pytest.mark.parametrize("mode", [WEIGHTED, LAYERED])
@pytest.mark.parametrize("k", [2, 3, 4])
def test_a_call_that_passes_every_check_ends_at_the_null_context(k, mode, masks):
    shape = dict(k=k, mode=mode, masks=masks)
    assert call(**shape) == (INVALID, "null context")
    assert call(object_space=0, **shape) == (INVALID, "null context")
    assert call(bounds=ctypes.addressof(BOUNDS_OK), **shape) == (INVALID, "null context")
    assert call(poses=None, stride=0, bounds=ctypes.addressof(BOUNDS_OK), **shape) == (INVALID, "null context")     # the boxes alone
    assert call(skeleton=0, instance_skeletons=BASE + 0xB00000, **shape) == (INVALID, "null context")
    assert call(n=0, **shape) == (INVALID, "null context")
    # in place on buffer 0 and on buffer K - 1
    assert call(poses=BASE, **shape) == (INVALID, "null context")
    assert call(poses=BASE + (k - 1) * SPACING, **shape) == (INVALID, "null context")
    # every buffer a stride of its own; in place takes the stride of its buffer
    strides = [STRIDE + 16 * index for index in range(4)]
    assert call(strides=strides, **shape) == (INVALID, "null context")
    assert call(strides=strides, poses=BASE + (k - 1) * SPACING, stride=strides[k - 1], **shape) == (INVALID, "null context")


REFUSED = {
    "null blend": dict(blend=None),
    "one buffer": dict(k=1),
    "no buffer": dict(k=0),
    "five buffers": dict(k=5),
    "an unknown mode": dict(mode=2),
    "a null buffer among the first K": dict(k=3, buffer1=None),
    "a null first buffer": dict(buffer0=None),
    "a buffer behind the blend": dict(k=2, buffer2=BASE + 2 * SPACING),
    "a last buffer behind the blend": dict(k=3, buffer3=BASE + 3 * SPACING),
    "null weights": dict(weights=None),
    "no skeleton at all": dict(skeleton=0),
    "bounds without object space": dict(object_space=0, bounds=ctypes.addressof(BOUNDS_OK)),
    "no output without bounds": dict(poses=None),
    "an unaligned buffer": dict(k=3, buffer2=BASE + 2 * SPACING + 8),
    "an unaligned buffer stride": dict(k=4, stride3=STRIDE + 8),
    "unaligned poses": dict(poses=OUT + 4),
    "unaligned stride": dict(stride=STRIDE + 4),
    "reserved0": dict(reserved0=1),
    "reserved 0": dict(reserved=0),
    "reserved 1": dict(reserved=1),
    "bounds without a buffer": dict(bounds=ctypes.addressof(BOUNDS_NO_BUFFER)),
    "unaligned bounds": dict(bounds=ctypes.addressof(BOUNDS_UNALIGNED)),
    "bounds with a reserved field": dict(bounds=ctypes.addressof(BOUNDS_RESERVED)),
    "rows beyond 160 KiB of LDS": dict(stride=48 * 3500, poses=BASE + 0x1000000),
    "rows beyond 160 KiB of LDS, boxes alone": dict(stride0=48 * 3500, poses=None, stride=0, bounds=ctypes.addressof(BOUNDS_OK)),
}


@pytest.mark.parametrize("name", sorted(REFUSED))
def test_invalid_arguments_are_refused_with_a_message_before_any_device_call(name):
    status, message = call(**REFUSED[name])
    assert status == INVALID, name
    assert message != "" and message != "null context", (name, message)


def test_the_largest_shape_that_fits_is_not_refused_for_its_size():
    # 3400 transforms: the pose consumers' stated end; the shape comes from the output rows, or from buffer 0's without them
    assert call(stride=48 * 3400, poses=BASE + 0x1000000) == (INVALID, "null context")
    assert call(stride0=48 * 3400, buffer0=BASE + 0x2000000, poses=None, stride=0, bounds=ctypes.addressof(BOUNDS_OK)) == (INVALID, "null context")


@pytest.mark.parametrize("k", [2, 4])
def test_in_place_on_one_input_is_the_one_overlap_allowed(k):
    for which in range(k):
        start = BASE + which * SPACING
        assert call(k=k, poses=start) == (INVALID, "null context")
        # the same pointer with another stride, shifted by one row (both ways), inside the input's range, its last byte
        for poses, stride in ((start, STRIDE + 16), (start, STRIDE - 16), (start + STRIDE, STRIDE), (start - STRIDE, STRIDE), (start + 3 * STRIDE + 16, 16),
                              (start + STRIDE * N - 16, STRIDE), (start - STRIDE * N + 16, STRIDE)):
            status, message = call(k=k, poses=poses, stride=stride)
            assert status == INVALID and "overlap the rows of pose buffer %u" % which in message, (which, hex(poses), stride, message)
        # ranges that touch do not overlap
        assert call(k=k, poses=start + STRIDE * N) == (INVALID, "null context")
        assert call(k=k, poses=start - STRIDE * N) == (INVALID, "null context")
    # in place on one input does not excuse an overlap with another
    status, message = call(k=k, poses=BASE, **{"buffer%u" % (k - 1): BASE + STRIDE})
    assert status == INVALID and "overlap the rows of pose buffer %u" % (k - 1) in message, message


def test_inputs_may_overlap_each_other():
    assert call(k=2, buffer1=BASE) == (INVALID, "null context")                        # the same buffer twice
    assert call(k=3, buffer1=BASE + STRIDE, buffer2=BASE + 16) == (INVALID, "null context")
    assert call(k=4, buffer1=BASE, buffer2=BASE, buffer3=BASE, stride3=STRIDE + 16) == (INVALID, "null context")
    # ... and the output may be all of them at once when they are the same rows
    assert call(k=2, buffer1=BASE, poses=BASE) == (INVALID, "null context")


def test_the_bounds_overlap_neither_an_input_nor_the_output():
    def bounds_at(address):
        bounds = runtime.PoseBounds()
        bounds.bounds = address
        return bounds

    for k in (2, 3):
        for which in range(k):
            for address in (BASE + which * SPACING, BASE + which * SPACING + STRIDE * N - 16, BASE + which * SPACING - 32 * N + 16):
                bounds = bounds_at(address)
                for launch in (dict(), dict(poses=None, stride=0)):
                    status, message = call(k=k, bounds=ctypes.addressof(bounds), **launch)
                    assert status == INVALID and "bounds overlap the rows of pose buffer %u" % which in message, (k, which, hex(address), message)
        bounds = bounds_at(OUT + STRIDE)
        status, message = call(k=k, bounds=ctypes.addressof(bounds))
        assert status == INVALID and "bounds overlap the output rows" in message, message
        # boxes that touch the end of a buffer, and boxes where the output would have been without one
        bounds = bounds_at(BASE + STRIDE * N)
        assert call(k=k, bounds=ctypes.addressof(bounds)) == (INVALID, "null context")
        bounds = bounds_at(OUT)
        assert call(k=k, poses=None, stride=0, bounds=ctypes.addressof(bounds)) == (INVALID, "null context")
