"""aclhip_skinning_matrices_batch at the C ABI, without a device: every ACLHIP_ERROR_INVALID_ARGUMENT case of the header is refused with a
message that names its cause through a NULL context -- the checks run before any device call, so a call that passes all of them ends at
"null context" -- and the overlap rule: the output overlaps nothing the launch reads, in place included."""
import ctypes

import pytest

from acl_amd import runtime

INVALID = runtime.ERROR_INVALID_ARGUMENT
POSES, PALETTES, SKELETONS, SKINS = 0x10000000, 0x20000000, 0x30000000, 0x40000000
# (addresses are compared and checked for alignment, never read: no context, no launch)
N, BONES, JOINTS = 8, 100, 100
STRIDE, PALETTE_STRIDE = BONES * 48, JOINTS * 64
PASSES = (INVALID, "null context")


def call(poses=POSES, pose_stride=STRIDE, n=N, desc="default", palettes=PALETTES, palette_stride=PALETTE_STRIDE, **fields):
    """(status, message) of aclhip_skinning_matrices_batch through a NULL context; desc: object space, skeleton 1, skin 1, 64 byte records,
    changed by `fields`"""
    lib = runtime.load_library()
    if desc == "default":
        desc = runtime.SkinningDesc()
        desc.skeleton, desc.skin, desc.object_space, desc.layout = 1, 1, 1, runtime.PALETTE_3X4F_64
        for name, value in fields.items():
            if name == "reserved":
                desc.reserved[value] = 1
            else:
                setattr(desc, name, value)
    status = lib.aclhip_skinning_matrices_batch(None, poses, pose_stride, n, ctypes.byref(desc) if desc is not None else None, palettes, palette_stride, None)
    return status, lib.aclhip_last_error_message(None).decode()


def test_a_call_that_passes_every_check_ends_at_the_null_context():
    assert call() == PASSES
    for fields in (dict(object_space=0), dict(layout=runtime.PALETTE_3X4F_TRANSPOSED_48), dict(skeleton=0, instance_skeletons=SKELETONS),
                   dict(skeleton=7, instance_skeletons=SKELETONS), dict(skin=0, instance_skins=SKINS), dict(skin=9, instance_skins=SKINS),
                   dict(skeleton=0, instance_skeletons=SKELETONS, skin=0, instance_skins=SKINS)):
        assert call(**fields) == PASSES, fields
    assert call(pose_stride=STRIDE + 32, palette_stride=PALETTE_STRIDE + 48) == PASSES
    assert call(palette_stride=JOINTS * 48, layout=runtime.PALETTE_3X4F_TRANSPOSED_48) == PASSES
    assert call(palette_stride=48) == PASSES              # a row too small for a skin is the kernel's refusal, per instance
    assert call(palette_stride=64 * 0xFFFF) == PASSES     # more joints than bones: the palette row says nothing about the shape
    assert call(n=0) == PASSES


REFUSED = {
    "null desc": (dict(desc=None), "desc"),
    "null poses": (dict(poses=None), "pose buffer"),
    "null palettes": (dict(palettes=None), "palette buffer"),
    "no skeleton at all": (dict(skeleton=0), "skeleton"),
    "no skin at all": (dict(skin=0), "skin or a list of skins"),
    "an unknown layout": (dict(layout=2), "layout 2"),
    "a layout far off": (dict(layout=0xFFFFFFFF), "layout"),
    "unaligned poses": (dict(poses=POSES + 8), "pose buffer and stride"),
    "unaligned pose stride": (dict(pose_stride=STRIDE + 8), "pose buffer and stride"),
    "unaligned palettes": (dict(palettes=PALETTES + 4), "palette buffer and stride"),
    "unaligned palette stride": (dict(palette_stride=PALETTE_STRIDE + 8), "palette buffer and stride"),
    "reserved 0": (dict(reserved=0), "reserved"),
    "reserved 1": (dict(reserved=1), "reserved"),
    "a row beyond 160 KiB of LDS": (dict(pose_stride=48 * 3500), "LDS"),
}


@pytest.mark.parametrize("name", sorted(REFUSED))
def test_invalid_arguments_are_refused_with_a_message_before_any_device_call(name):
    arguments, cause = REFUSED[name]
    status, message = call(**arguments)
    assert status == INVALID, name
    assert cause in message and message != "null context", (name, message)


def test_the_shape_comes_from_the_pose_rows_alone():
    assert call(pose_stride=48 * 3300, palette_stride=64) == PASSES
    status, message = call(pose_stride=48 * 3500, palette_stride=64)
    assert status == INVALID and "LDS" in message


def test_any_overlap_of_the_output_with_what_is_read_is_refused():
    size, out_size = STRIDE * N, PALETTE_STRIDE * N
    # in place, the first byte, inside, the last byte of the input; the last byte of the output on the first of the input
    for palettes in (POSES, POSES + 16, POSES + size - 16, POSES - out_size + 16):
        status, message = call(palettes=palettes)
        assert status == INVALID and "overlap the pose rows" in message, (hex(palettes), message)
    # equal strides are no exception: 100 bones and 100 transposed joints are rows of the same size
    status, message = call(palettes=POSES, palette_stride=STRIDE, layout=runtime.PALETTE_3X4F_TRANSPOSED_48)
    assert status == INVALID and "overlap the pose rows" in message
    # ranges that only touch do not overlap
    assert call(palettes=POSES + size) == PASSES
    assert call(palettes=POSES - out_size) == PASSES
    # the two lists are read as well
    for palettes in (SKELETONS, SKELETONS - out_size + 16):
        status, message = call(palettes=palettes, instance_skeletons=SKELETONS)
        assert status == INVALID and "overlap the skeleton list" in message, (hex(palettes), message)
    assert call(palettes=SKELETONS - out_size, instance_skeletons=SKELETONS) == PASSES
    assert call(palettes=SKELETONS + 4 * N, instance_skeletons=SKELETONS) == PASSES
    for palettes in (SKINS, SKINS - out_size + 16, SKINS + 16):
        status, message = call(palettes=palettes, instance_skins=SKINS)
        assert status == INVALID and "overlap the skin list" in message, (hex(palettes), message)
    assert call(palettes=SKINS - out_size, instance_skins=SKINS) == PASSES
    assert call(palettes=SKINS + 4 * N, instance_skins=SKINS) == PASSES
    assert call(palettes=POSES, n=0) == PASSES                                # no instances: no bytes
