"""The handle tables of track maps, skeletons and blend masks through the C ABI: which handle a registration gets, what a retired or a
refused one leaves behind, and what a full table says. No kernel is launched: the shapes are the smallest there are (a map of 4 tracks
into 6 slots, a skeleton of 3 bones with a hierarchy, a mask of 6 slots). One handle is retired at a time, so no order among several
retired handles is pinned. Needs a GPU (registration uploads to it)."""
import ctypes

import numpy as np
import pytest

from acl_amd import runtime

pytestmark = pytest.mark.gpu

INVALID_ARGUMENT, OUT_OF_MEMORY = 1, 5     # ACLHIP_ERROR_INVALID_ARGUMENT, ACLHIP_ERROR_OUT_OF_MEMORY
NO_PARENT, DROPPED = runtime.NO_PARENT, runtime.TRACK_DROPPED


def reference_pose(num_bones, offset):
    pose = np.zeros((num_bones, 12), dtype=np.float32)
    pose[:, 3] = 1.0                           # rotation: identity
    pose[:, 4] = offset + np.arange(num_bones)  # translation x
    pose[:, 8:11] = 1.0                        # scale
    return pose


class Kind:
    """One of the three registries: `valid[i]` are the arguments of four different valid objects, `refused` those of one registration refuses"""

    def __init__(self, noun, valid, refused, register, unregister, info, check):
        self.noun, self.valid, self.refused = noun, valid, refused
        self.register, self.unregister, self.info, self.check = register, unregister, info, check


KINDS = {
    "track_map": Kind(
        "track map",
        [([0, 2, 4, 5], 6), ([5, 4, DROPPED, 0], 6), ([0, 1, 2, 3], 6), ([DROPPED, 3, 1, DROPPED], 6)],
        ([0, 1, 1, 2], 6),                                   # a duplicate slot
        lambda ctx, args: ctx.register_track_map(*args), lambda ctx, handle: ctx.unregister_track_map(handle),
        lambda ctx, handle: ctx.track_map_info(handle), lambda args: runtime.check_track_map(*args)),
    "skeleton": Kind(
        "skeleton",
        [([NO_PARENT, 0, 1], reference_pose(3, 0.0)), ([NO_PARENT, 0, 0], reference_pose(3, 1.0)),
         ([NO_PARENT, NO_PARENT, 1], reference_pose(3, 2.0)), ([NO_PARENT, 0, 1], -reference_pose(3, 3.0))],
        ([NO_PARENT, 2, 0], reference_pose(3, 0.0)),          # bone 1 has parent 2
        lambda ctx, args: ctx.register_skeleton(*args), lambda ctx, handle: ctx.unregister_skeleton(handle),
        lambda ctx, handle: ctx.skeleton_info(handle), lambda args: runtime.check_skeleton(*args)),
    "blend_mask": Kind(
        "blend mask",
        [([0.0, 0.25, 0.5, 0.75, 1.0, 1.0],), ([1.0] * 6,), ([0.0] * 6,), ([0.5, 0.0, 0.0, 1.0, 0.125, 0.0],)],
        ([0.0, 0.25, 2.0, 0.75, 1.0, 1.0],),                   # a weight of 2.0
        lambda ctx, args: ctx.register_blend_mask(*args), lambda ctx, handle: ctx.unregister_blend_mask(handle),
        lambda ctx, handle: ctx.blend_mask_info(handle), lambda args: runtime.check_blend_mask(*args)),
}


def same_info(kind, ctx, handle, args):
    status, _, expected = kind.check(args)
    assert status == 0
    return bytes(kind.info(ctx, handle)) == bytes(expected)


def refused(call, status, text):
    with pytest.raises(runtime.AclHipError) as error:
        call()
    assert error.value.status == status, str(error.value)
    assert text in str(error.value), str(error.value)


@pytest.mark.parametrize("name", list(KINDS))
def test_handles_of_a_table(name):
    import torch

    kind = KINDS[name]
    with runtime.Context(0) as ctx:
        handles = [kind.register(ctx, args) for args in kind.valid[:3]]
        assert len(set(handles)) == 3 and min(handles) >= 1, handles
        for handle, args in zip(handles, kind.valid):
            assert same_info(kind, ctx, handle, args)

        # the middle one goes: unknown from then on, its neighbours intact
        middle = handles[1]
        kind.unregister(ctx, middle)
        unknown = "unknown %s handle %u" % (kind.noun, middle)
        refused(lambda: kind.info(ctx, middle), INVALID_ARGUMENT, unknown)
        refused(lambda: kind.unregister(ctx, middle), INVALID_ARGUMENT, unknown)
        for index in (0, 2):
            assert same_info(kind, ctx, handles[index], kind.valid[index])

        # its record is cleared behind the work in flight (none here): once that has happened the handle is the next one handed out
        torch.cuda.synchronize()
        fourth = kind.register(ctx, kind.valid[3])
        assert fourth == middle, (fourth, handles)
        assert same_info(kind, ctx, fourth, kind.valid[3])
        for index in (0, 2):
            assert same_info(kind, ctx, handles[index], kind.valid[index])

        # a refused registration consumes no handle
        status, message, _ = kind.check(kind.refused)
        assert status == INVALID_ARGUMENT and message
        refused(lambda: kind.register(ctx, kind.refused), INVALID_ARGUMENT, message)
        following = kind.register(ctx, kind.valid[1])
        assert following == max(handles) + 1, (following, handles)
        assert same_info(kind, ctx, following, kind.valid[1])
        refused(lambda: kind.info(ctx, following + 1), INVALID_ARGUMENT, "unknown %s handle %u" % (kind.noun, following + 1))
        refused(lambda: kind.info(ctx, 0), INVALID_ARGUMENT, "unknown %s handle 0" % kind.noun)


def test_a_full_table_refuses_and_recovers():
    """The smallest table (skeletons: ACLHIP_MAX_SKELETONS records, record 0 never handed out); the other two run the same code"""
    import torch

    pose = reference_pose(1, 0.0)
    with runtime.Context(0) as ctx:
        handles = []
        with pytest.raises(runtime.AclHipError) as error:
            for _ in range(runtime.MAX_SKELETONS + 1):
                handles.append(ctx.register_skeleton(None, pose))
        assert len(handles) == runtime.MAX_SKELETONS - 1 == 1023
        assert sorted(handles) == list(range(1, runtime.MAX_SKELETONS))
        assert error.value.status == OUT_OF_MEMORY, str(error.value)
        assert "the skeleton table holds 1023 skeletons" in str(error.value)

        ctx.unregister_skeleton(handles[500])
        torch.cuda.synchronize()
        assert ctx.register_skeleton(None, pose) == handles[500]
        refused(lambda: ctx.register_skeleton(None, pose), OUT_OF_MEMORY, "the skeleton table holds 1023 skeletons")
        assert ctx.skeleton_info(handles[-1]).num_bones == 1
