"""Skeletons at the C ABI (aclhip_register_skeleton, aclhip_decompress_poses_batch_mapped, ...): declared, exported, bound; the
binding's structs have the C compiler's sizes and offsets; the skeleton validation and the argument checks that need no device (no GPU)."""
import ctypes
import os
import subprocess

import numpy as np

from acl_amd import runtime, synth
from test_capi_symbols import declared_functions

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("aclhip_check_skeleton", "aclhip_register_skeleton", "aclhip_unregister_skeleton", "aclhip_get_skeleton_info", "aclhip_decompress_poses_batch_mapped")
NO_PARENT = 0xFFFFFFFF
INVALID = runtime.ERROR_INVALID_ARGUMENT


def identity_pose(num_bones):
    pose = np.zeros((num_bones, 12), dtype=np.float32)
    pose[:, 3] = 1.0
    pose[:, 8:11] = 1.0
    return pose


def test_header_declares_and_library_exports_the_entry_points():
    declared = declared_functions()
    lib = runtime.load_library()
    for name in NAMES:
        assert name in declared, name
        assert hasattr(lib, name), name
        assert name in runtime.EXPORTED_SYMBOLS, name
    assert lib.aclhip_abi_version() == runtime.ABI_VERSION == 6       # (added without a bump: no existing struct changed)


def test_struct_sizes_and_offsets_match_a_c99_translation_unit(tmp_path):
    lib_dir = os.path.dirname(runtime.library_path())
    binary = tmp_path / "skeleton_abi"
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "c", "skeleton_abi.c"),
                    "-L" + lib_dir, "-laclhip", "-Wl,-rpath," + lib_dir, "-o", str(binary)], check=True)
    done = subprocess.run([str(binary)], stdout=subprocess.PIPE, text=True, timeout=120)
    assert done.returncode == 0, done.returncode        # (the program's own argument and validation checks)
    words = [int(word) for word in done.stdout.split()]
    mapping, info = runtime.PoseMapping, runtime.SkeletonInfo
    assert ctypes.sizeof(mapping) == words[0] == 56
    assert ctypes.sizeof(info) == words[1] == 32
    assert [mapping.skeleton.offset, mapping.instance_skeletons.offset, mapping.map.offset, mapping.instance_maps.offset, mapping.blend_maps.offset,
            mapping.base_maps.offset] == words[2:8]
    assert [info.walk_steps.offset, info.has_negative_scale.offset] == words[8:10]
    assert runtime.MAX_SKELETONS == words[10]


def test_a_humanoid_hierarchy_is_accepted_and_reported_like_the_walk_plan():
    for num_bones in (100, 37, 128, 1):
        parents = synth.humanoid_hierarchy(num_bones)
        status, message, info = runtime.check_skeleton(parents, identity_pose(num_bones))
        assert status == 0, message
        steps = np.zeros(num_bones, dtype=np.uint32)
        num_steps = ctypes.c_uint32(0)
        assert runtime.load_library().aclhip_plan_hierarchy_walk(np.ascontiguousarray(parents, dtype=np.uint32).ctypes.data, num_bones, 16, steps.ctypes.data, ctypes.byref(num_steps)) == 0
        roots = [i for i in range(num_bones) if i == 0 or int(parents[i]) == NO_PARENT]
        depth = np.ones(num_bones, dtype=np.int64)
        for i in range(num_bones):
            if i not in roots:
                depth[i] = depth[int(parents[i])] + 1
        assert (info.num_bones, info.has_hierarchy, info.num_roots, info.depth, info.walk_steps, info.has_negative_scale) == (num_bones, 1, len(roots), int(depth.max()), num_steps.value, 0)
    # without parents: local space only
    status, _, info = runtime.check_skeleton(None, identity_pose(12))
    assert status == 0 and (info.num_bones, info.has_hierarchy, info.num_roots, info.depth, info.walk_steps) == (12, 0, 0, 0, 0)


def test_refusals_name_the_offending_bone():
    parents = np.array(synth.humanoid_hierarchy(40), dtype=np.uint32)
    pose = identity_pose(40)
    # a child before its parent
    broken = parents.copy()
    broken[17] = 23
    status, message, _ = runtime.check_skeleton(broken, pose)
    assert status == INVALID and "bone 17 " in message and "parent 23" in message, message
    # no bones, too many bones
    status, message, _ = runtime.check_skeleton(parents, pose, num_bones=0)
    assert status == INVALID and "0 bones" in message, message
    many = 0x10000
    status, message, _ = runtime.check_skeleton(np.full(many, NO_PARENT, dtype=np.uint32), identity_pose(many))
    assert status == INVALID and str(many) in message, message
    assert runtime.check_skeleton(np.full(0xFFFF, NO_PARENT, dtype=np.uint32), identity_pose(0xFFFF))[0] == 0
    # a NaN, an infinity in the reference pose
    for bone, component, value in ((29, 5, np.nan), (3, 0, np.inf), (39, 10, -np.inf)):
        bad = pose.copy()
        bad[bone, component] = value
        status, message, _ = runtime.check_skeleton(parents, bad)
        assert status == INVALID and ("bone %d:" % bone) in message, message
    # (the pads of translation and scale are not part of the pose)
    padded = pose.copy()
    padded[:, 7] = np.nan
    assert runtime.check_skeleton(parents, padded)[0] == 0
    # null pointers
    lib = runtime.load_library()
    info = runtime.SkeletonInfo()
    message = ctypes.create_string_buffer(64)
    assert lib.aclhip_check_skeleton(parents.ctypes.data, None, 40, ctypes.byref(info), message, 64) == INVALID and b"null" in message.value
    assert lib.aclhip_check_skeleton(parents.ctypes.data, pose.ctypes.data, 40, None, None, 0) == 0
    # a negative scale is accepted and reported
    mirrored = pose.copy()
    mirrored[7, 9] = -1.0
    status, _, info = runtime.check_skeleton(parents, mirrored)
    assert status == 0 and info.has_negative_scale == 1


def test_argument_checks_that_return_before_any_hip_call():
    lib = runtime.load_library()
    parents = np.array([NO_PARENT, 0, 1], dtype=np.uint32)
    pose = identity_pose(3)
    handle = ctypes.c_uint32(99)
    assert lib.aclhip_register_skeleton(None, parents.ctypes.data, pose.ctypes.data, 3, ctypes.byref(handle)) == INVALID
    assert lib.aclhip_unregister_skeleton(None, 1) == INVALID
    assert lib.aclhip_get_skeleton_info(None, 1, ctypes.byref(runtime.SkeletonInfo())) == INVALID
    params, consumers, mapping = runtime.default_params(), runtime.PoseConsumers(), runtime.PoseMapping()
    mapping.skeleton, mapping.map = 1, 1
    assert lib.aclhip_decompress_poses_batch_mapped(None, None, None, 4, ctypes.byref(params), ctypes.byref(consumers), ctypes.byref(mapping), None, 4800, None) == INVALID
    assert lib.aclhip_decompress_poses_batch_mapped(None, None, None, 0, ctypes.byref(params), ctypes.byref(consumers), None, None, 4800, None) == INVALID
