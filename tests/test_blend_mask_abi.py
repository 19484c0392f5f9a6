"""Blend masks at the C ABI (aclhip_register_blend_mask, aclhip_decompress_poses_batch_masked, ...): declared, exported, bound; the
binding's structs have the C compiler's sizes and offsets; the mask validation and the argument checks that need no device (no GPU)."""
import ctypes
import os
import subprocess

import numpy as np

from acl_amd import runtime
from test_capi_symbols import declared_functions

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("aclhip_check_blend_mask", "aclhip_register_blend_mask", "aclhip_unregister_blend_mask", "aclhip_get_blend_mask_info", "aclhip_decompress_poses_batch_masked")
INVALID = runtime.ERROR_INVALID_ARGUMENT


def test_header_declares_and_library_exports_the_entry_points():
    declared = declared_functions()
    lib = runtime.load_library()
    for name in NAMES:
        assert name in declared, name
        assert hasattr(lib, name), name
        assert name in runtime.EXPORTED_SYMBOLS, name
    assert lib.aclhip_abi_version() == runtime.ABI_VERSION == 6       # (added without a bump: no existing struct changed)
    assert ctypes.sizeof(runtime.PoseMapping) == 56 and ctypes.sizeof(runtime.PoseConsumers) == 72


def test_struct_sizes_and_offsets_match_a_c99_translation_unit(tmp_path):
    lib_dir = os.path.dirname(runtime.library_path())
    binary = tmp_path / "blend_mask_abi"
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "c", "blend_mask_abi.c"),
                    "-L" + lib_dir, "-laclhip", "-Wl,-rpath," + lib_dir, "-o", str(binary)], check=True)
    done = subprocess.run([str(binary)], stdout=subprocess.PIPE, text=True, timeout=120)
    assert done.returncode == 0, done.returncode        # (the program's own argument and validation checks)
    words = [int(word) for word in done.stdout.split()]
    masking, info = runtime.BlendMasking, runtime.BlendMaskInfo
    assert ctypes.sizeof(masking) == words[0] == 32
    assert ctypes.sizeof(info) == words[1] == 16
    assert [masking.mode.offset, masking.reserved0.offset, masking.instance_masks.offset, masking.reserved.offset] == words[2:6] == [0, 4, 8, 16]
    assert [info.num_slots.offset, info.num_zero.offset, info.num_one.offset] == words[6:9]
    assert runtime.MAX_BLEND_MASKS == words[9]
    assert (runtime.BLEND_WEIGHTED, runtime.BLEND_LAYERED) == tuple(words[10:12]) == (0, 1)
    assert words[12] == 4


def test_masks_in_the_closed_unit_interval_are_accepted_and_counted():
    tiny = np.float32(1e-45)                                       # the smallest subnormal
    largest_subnormal = np.frombuffer(np.uint32(0x007FFFFF).tobytes(), dtype=np.float32)[0]
    below_one = np.nextafter(np.float32(1.0), np.float32(0.0))
    weights = np.array([0.0, 1.0, 0.5, tiny, largest_subnormal, below_one, 1.0, -0.0, 0.25, 1.0], dtype=np.float32)
    status, message, info = runtime.check_blend_mask(weights)
    assert status == 0, message
    assert message == ""
    assert (info.num_slots, info.num_zero, info.num_one, info.reserved) == (10, 2, 3, 0)
    for num_slots in (1, 100, 0xFFFF):
        status, message, info = runtime.check_blend_mask(np.ones(num_slots, dtype=np.float32))
        assert status == 0 and (info.num_slots, info.num_zero, info.num_one) == (num_slots, 0, num_slots), message
        status, message, info = runtime.check_blend_mask(np.zeros(num_slots, dtype=np.float32))
        assert status == 0 and (info.num_slots, info.num_zero, info.num_one) == (num_slots, num_slots, 0), message
    rng = np.random.default_rng(5)
    weights = rng.uniform(0.0, 1.0, size=300).astype(np.float32)
    weights[40:90], weights[250:] = 1.0, 0.0
    status, message, info = runtime.check_blend_mask(weights)
    assert status == 0 and (info.num_zero, info.num_one) == (int((weights == 0).sum()), int((weights == 1).sum())), message


def test_refusals_name_the_offending_slot():
    good = np.linspace(0.0, 1.0, 64, dtype=np.float32)
    for slot, value in ((17, np.nan), (0, np.inf), (63, -np.inf), (5, -0.25), (31, 1.0000001), (9, 2.0), (12, -1e-45)):
        bad = good.copy()
        bad[slot] = value
        assert not (0.0 <= bad[slot] <= 1.0)                      # (1.0000001 rounds to the float above 1, -1e-45 to the subnormal below 0)
        status, message, _ = runtime.check_blend_mask(bad)
        assert status == INVALID and ("slot %d:" % slot) in message, (slot, value, message)
    # the FIRST offending slot is the one named
    bad = good.copy()
    bad[20], bad[40] = 3.0, np.nan
    status, message, _ = runtime.check_blend_mask(bad)
    assert status == INVALID and "slot 20:" in message, message
    # no slots, too many slots, a null pointer
    status, message, _ = runtime.check_blend_mask(good, num_slots=0)
    assert status == INVALID and "0 slots" in message, message
    many = 0x10000
    status, message, _ = runtime.check_blend_mask(np.ones(many, dtype=np.float32))
    assert status == INVALID and str(many) in message, message
    status, message, _ = runtime.check_blend_mask(None, num_slots=8)
    assert status == INVALID and "null" in message, message
    # out_info and message are optional; a refused mask leaves out_info alone
    lib = runtime.load_library()
    assert lib.aclhip_check_blend_mask(good.ctypes.data, 64, None, None, 0) == 0
    info = runtime.BlendMaskInfo(7, 7, 7, 7)
    bad = good.copy()
    bad[3] = np.nan
    assert lib.aclhip_check_blend_mask(bad.ctypes.data, 64, ctypes.byref(info), None, 0) == INVALID
    assert (info.num_slots, info.num_zero, info.num_one, info.reserved) == (7, 7, 7, 7)
    short = ctypes.create_string_buffer(8)                          # a short message buffer is not overrun
    assert lib.aclhip_check_blend_mask(bad.ctypes.data, 64, None, short, 8) == INVALID and len(short.value) <= 7


def test_argument_checks_that_return_before_any_hip_call():
    lib = runtime.load_library()
    weights = np.ones(3, dtype=np.float32)
    handle = ctypes.c_uint32(99)
    assert lib.aclhip_register_blend_mask(None, weights.ctypes.data, 3, ctypes.byref(handle)) == INVALID
    assert lib.aclhip_register_blend_mask(None, weights.ctypes.data, 3, None) == INVALID
    assert lib.aclhip_unregister_blend_mask(None, 1) == INVALID
    assert lib.aclhip_get_blend_mask_info(None, 1, ctypes.byref(runtime.BlendMaskInfo())) == INVALID
    assert lib.aclhip_get_blend_mask_info(None, 1, None) == INVALID
    params, consumers, mapping, masking = runtime.default_params(), runtime.PoseConsumers(), runtime.PoseMapping(), runtime.BlendMasking()
    mapping.skeleton, mapping.map = 1, 1
    consumers.num_blend_clips = 2
    call = lib.aclhip_decompress_poses_batch_masked
    assert call(None, None, None, 4, ctypes.byref(params), ctypes.byref(consumers), ctypes.byref(mapping), ctypes.byref(masking), None, 4800, None) == INVALID
    assert call(None, None, None, 0, ctypes.byref(params), ctypes.byref(consumers), ctypes.byref(mapping), None, None, 4800, None) == INVALID
    assert call(None, None, None, 0, ctypes.byref(params), ctypes.byref(consumers), None, ctypes.byref(masking), None, 4800, None) == INVALID
    assert call(None, None, None, 0, ctypes.byref(params), None, ctypes.byref(mapping), ctypes.byref(masking), None, 4800, None) == INVALID
