"""Skins at the C ABI (aclhip_check_skin, aclhip_register_skin, aclhip_unregister_skin, aclhip_get_skin_info,
aclhip_skinning_matrices_batch): declared, exported, bound; the binding's structs have the C compiler's sizes and offsets; the skin
validation -- every refusal with a message that names the joint -- and the argument checks that need no device (no GPU)."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

from acl_amd import runtime
from test_capi_symbols import declared_functions

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("aclhip_check_skin", "aclhip_register_skin", "aclhip_unregister_skin", "aclhip_get_skin_info", "aclhip_skinning_matrices_batch")
INVALID = runtime.ERROR_INVALID_ARGUMENT


def identity_matrices(num_joints):
    return np.broadcast_to(np.eye(4, dtype=np.float32), (num_joints, 4, 4)).copy()


def fields_of(info):
    return (info.num_joints, info.num_bones, info.is_identity_joint_list, info.has_inverse_bind, tuple(info.reserved))


def test_header_declares_library_exports_and_binding_binds_the_entry_points():
    declared = declared_functions()
    lib = runtime.load_library()
    for name in NAMES:
        assert name in declared, name
        assert hasattr(lib, name), name
        assert name in runtime.EXPORTED_SYMBOLS, name
    for method in ("register_skin", "unregister_skin", "skin_info", "skinning_matrices_batch"):
        assert hasattr(runtime.Context, method)
    assert callable(runtime.check_skin)
    assert lib.aclhip_abi_version() == runtime.ABI_VERSION == 6       # (added without a bump: no existing struct changed)


def test_struct_sizes_and_offsets_match_a_c99_translation_unit(tmp_path):
    lib_dir = os.path.dirname(runtime.library_path())
    binary = tmp_path / "skinning_abi"
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "c", "skinning_abi.c"),
                    "-L" + lib_dir, "-laclhip", "-Wl,-rpath," + lib_dir, "-o", str(binary)], check=True)
    done = subprocess.run([str(binary)], stdout=subprocess.PIPE, text=True, timeout=120)
    assert done.returncode == 0, done.returncode        # (the program's own argument and validation checks)
    words = [int(word) for word in done.stdout.split()]
    desc, info = runtime.SkinningDesc, runtime.SkinInfo
    assert ctypes.sizeof(desc) == words[0] == 56
    assert ctypes.sizeof(info) == words[1] == 32
    assert [getattr(desc, name).offset for name in ("skeleton", "instance_skeletons", "skin", "instance_skins", "object_space", "layout", "reserved")] == words[2:9] \
        == [0, 8, 16, 24, 32, 36, 40]
    assert [getattr(info, name).offset for name in ("num_joints", "num_bones", "is_identity_joint_list", "has_inverse_bind", "reserved")] == words[9:14] == [0, 4, 8, 12, 16]
    assert runtime.MAX_SKINS == words[14] == 4096
    assert [runtime.PALETTE_3X4F_64, runtime.PALETTE_3X4F_TRANSPOSED_48] == words[15:17] == [0, 1]
    assert words[17] == 4


def test_skins_that_pass_and_what_their_info_says():
    rng = np.random.default_rng(11)
    matrices = rng.uniform(-4.0, 4.0, size=(100, 4, 4)).astype(np.float32)
    matrices[:, :, 3] = np.nan                                      # lane 3 of every axis is ignored
    status, message, info = runtime.check_skin(None, matrices, 100)
    assert status == 0 and message == "", message
    assert fields_of(info) == (100, 100, 1, 1, (0, 0, 0, 0))
    status, message, info = runtime.check_skin(np.arange(100), None, 100)       # the identity list spelled out, no matrices
    assert status == 0 and fields_of(info) == (100, 100, 1, 0, (0, 0, 0, 0)), message
    joints = np.arange(100)[::-1].copy()
    status, message, info = runtime.check_skin(joints, matrices, 100)           # a permutation is not the identity list
    assert status == 0 and fields_of(info) == (100, 100, 0, 1, (0, 0, 0, 0)), message
    status, message, info = runtime.check_skin([4, 4, 0], None, 5)              # fewer joints than bones, a bone twice
    assert status == 0 and fields_of(info) == (3, 5, 0, 0, (0, 0, 0, 0)), message
    status, message, info = runtime.check_skin([0, 1, 1, 0, 1], identity_matrices(5), 2)        # more joints than bones
    assert status == 0 and fields_of(info) == (5, 2, 0, 1, (0, 0, 0, 0)), message
    status, message, info = runtime.check_skin([0, 1, 0], None, 3)              # as many joints as bones, but not in order
    assert status == 0 and info.is_identity_joint_list == 0, message
    for count in (1, 0xFFFF):
        status, message, info = runtime.check_skin(None, None, count)
        assert status == 0 and fields_of(info) == (count, count, 1, 0, (0, 0, 0, 0)), message
    status, message, info = runtime.check_skin(np.zeros(0xFFFF, dtype=np.uint32), None, 1)
    assert status == 0 and fields_of(info) == (0xFFFF, 1, 0, 0, (0, 0, 0, 0)), message
    # subnormals, -0 and the largest float are finite
    matrices = identity_matrices(3)
    matrices[1, 2, 0:3] = (1e-45, -0.0, np.finfo(np.float32).max)
    assert runtime.check_skin(None, matrices, 3)[0] == 0


def test_refusals_name_the_offending_joint():
    good_joints, good_matrices = np.arange(64, dtype=np.uint32), identity_matrices(64)
    # a joint bone outside the skeleton
    for joint, bone in ((0, 64), (17, 0xFFFFFFFF), (63, 65535)):
        bad = good_joints.copy()
        bad[joint] = bone
        status, message, _ = runtime.check_skin(bad, good_matrices, 64)
        assert status == INVALID and ("joint %d:" % joint) in message and str(bone) in message, (joint, message)
    # a matrix component of lanes 0-2 that is not finite
    for joint, axis, lane, value in ((5, 0, 0, np.nan), (0, 3, 2, np.inf), (63, 2, 1, -np.inf), (31, 1, 0, np.nan)):
        bad = good_matrices.copy()
        bad[joint, axis, lane] = value
        for joints in (good_joints, None):
            status, message, _ = runtime.check_skin(joints, bad, 64)
            assert status == INVALID and ("joint %d:" % joint) in message and "not finite" in message, (joint, message)
    # the FIRST offending joint is the one named, whichever of the two it offends with
    bad_joints, bad_matrices = good_joints.copy(), good_matrices.copy()
    bad_joints[40], bad_matrices[20, 1, 1] = 64, np.nan
    status, message, _ = runtime.check_skin(bad_joints, bad_matrices, 64)
    assert status == INVALID and "joint 20:" in message, message
    bad_joints[10] = 99
    status, message, _ = runtime.check_skin(bad_joints, bad_matrices, 64)
    assert status == INVALID and "joint 10:" in message, message
    # no joints, too many joints, no bones, too many bones
    status, message, _ = runtime.check_skin(good_joints, None, 64, num_joints=0)
    assert status == INVALID and "0 joints" in message, message
    status, message, _ = runtime.check_skin(np.zeros(0x10000, dtype=np.uint32), None, 64)
    assert status == INVALID and "65536 joints" in message, message
    status, message, _ = runtime.check_skin(good_joints, None, 0)
    assert status == INVALID and "0 bones" in message, message
    status, message, _ = runtime.check_skin(good_joints, None, 0x10000)
    assert status == INVALID and "65536 bones" in message, message
    # the identity list needs as many joints as bones
    for num_joints in (63, 65):
        status, message, _ = runtime.check_skin(None, None, 64, num_joints=num_joints)
        assert status == INVALID and "null joint bones" in message and str(num_joints) in message, message
    # the binding never hands the library a count beyond the arrays it passes along
    for arguments in ((good_joints, None, 64, 65), (None, good_matrices, 65, 65), (good_joints[:10], good_matrices, 64, 11)):
        with pytest.raises(ValueError):
            runtime.check_skin(arguments[0], arguments[1], arguments[2], num_joints=arguments[3])
    # out_info and message are optional; a refused skin leaves out_info alone
    lib = runtime.load_library()
    assert lib.aclhip_check_skin(good_joints.ctypes.data, good_matrices.ctypes.data, 64, 64, None, None, 0) == 0
    info = runtime.SkinInfo(7, 7, 7, 7)
    bad = good_joints.copy()
    bad[3] = 64
    assert lib.aclhip_check_skin(bad.ctypes.data, None, 64, 64, ctypes.byref(info), None, 0) == INVALID
    assert fields_of(info)[0:4] == (7, 7, 7, 7)
    short = ctypes.create_string_buffer(8)                          # a short message buffer is not overrun
    assert lib.aclhip_check_skin(bad.ctypes.data, None, 64, 64, None, short, 8) == INVALID and len(short.value) <= 7


def test_argument_checks_that_return_before_any_hip_call():
    lib = runtime.load_library()
    joints = np.arange(3, dtype=np.uint32)
    handle = ctypes.c_uint32(99)
    assert lib.aclhip_register_skin(None, joints.ctypes.data, None, 3, 3, ctypes.byref(handle)) == INVALID
    assert lib.aclhip_register_skin(None, joints.ctypes.data, None, 3, 3, None) == INVALID
    assert lib.aclhip_unregister_skin(None, 1) == INVALID
    assert lib.aclhip_get_skin_info(None, 1, ctypes.byref(runtime.SkinInfo())) == INVALID
    assert lib.aclhip_get_skin_info(None, 1, None) == INVALID
    desc = runtime.SkinningDesc()
    desc.skeleton, desc.skin = 1, 1
    assert lib.aclhip_skinning_matrices_batch(None, 0x1000, 4800, 4, ctypes.byref(desc), 0x100000, 4800, None) == INVALID
    assert lib.aclhip_last_error_message(None).decode() == "null context"
