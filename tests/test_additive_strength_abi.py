"""Additive strength at the C ABI (aclhip_additive_layering, aclhip_decompress_poses_batch_additive_weighted): declared, exported, bound; the
binding's struct has the C compiler's size and offsets; every ACLHIP_ERROR_INVALID_ARGUMENT case that is decided before a device call
returns it with a message that names the cause (no GPU)."""
import ctypes
import os
import subprocess

from acl_amd import runtime
from test_capi_symbols import declared_functions

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "aclhip_decompress_poses_batch_additive_weighted"
INVALID = runtime.ERROR_INVALID_ARGUMENT


def test_header_declares_and_library_exports_the_entry_point():
    lib = runtime.load_library()
    assert NAME in declared_functions()
    assert hasattr(lib, NAME)
    assert NAME in runtime.EXPORTED_SYMBOLS
    assert lib.aclhip_abi_version() == runtime.ABI_VERSION == 6       # (added without a bump: no existing struct changed)
    assert ctypes.sizeof(runtime.PoseConsumers) == 72 and ctypes.sizeof(runtime.PoseMapping) == 56 and ctypes.sizeof(runtime.BlendMasking) == 32
    assert ctypes.sizeof(runtime.PoseBounds) == 32


def test_struct_size_and_offsets_match_a_c99_translation_unit(tmp_path):
    lib_dir = os.path.dirname(runtime.library_path())
    binary = tmp_path / "additive_strength_abi"
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "c", "additive_strength_abi.c"),
                    "-L" + lib_dir, "-laclhip", "-Wl,-rpath," + lib_dir, "-o", str(binary)], check=True)
    done = subprocess.run([str(binary)], stdout=subprocess.PIPE, text=True, timeout=120)
    assert done.returncode == 0, done.returncode        # (the program's own argument checks)
    words = [int(word) for word in done.stdout.split()]
    layering = runtime.AdditiveLayering
    assert ctypes.sizeof(layering) == words[0] == 32
    assert [layering.instance_weights.offset, layering.instance_masks.offset, layering.reserved.offset] == words[1:4] == [0, 8, 16]
    assert words[4] == 6


def test_every_refusal_decided_before_a_device_call_has_a_message():
    lib = runtime.load_library()
    call = getattr(lib, NAME)
    box = (ctypes.c_float * 12)()
    aligned = (ctypes.addressof(box) + 15) & ~15                     # a HOST address: nothing below reaches a device call

    def attempt(spoil):
        params, consumers, mapping, layering = runtime.default_params(), runtime.PoseConsumers(), runtime.PoseMapping(), runtime.AdditiveLayering()
        consumers.additive_format, consumers.base_poses, consumers.base_pose_stride_bytes = runtime.ADDITIVE_ADDITIVE1, aligned, 4800
        mapping.skeleton, mapping.map = 1, 1
        layering.instance_weights, layering.instance_masks = aligned, aligned
        clips, times, poses, stride = aligned, aligned, aligned, 4800
        if spoil == "layering":
            layering = None
        if spoil == "both arrays":
            layering.instance_weights, layering.instance_masks = None, None
        if spoil in ("reserved0", "reserved1"):
            layering.reserved[int(spoil[-1])] = 1
        if spoil == "no additive format":
            consumers.additive_format = runtime.ADDITIVE_NONE
        if spoil == "consumers":
            consumers = None
        if spoil == "mapping":
            mapping = None
        if spoil == "no skeleton":
            mapping.skeleton = 0
        if spoil == "no map":
            mapping.map = 0
        if spoil == "no blend maps":
            consumers.num_blend_clips = 2
        if spoil == "no base maps":
            consumers.base_clips = aligned
        if spoil == "clips":
            clips = None
        if spoil == "times":
            times = None
        if spoil == "poses":
            poses = None
        if spoil == "stride":
            stride = 4808
        if spoil == "poses alignment":
            poses = aligned + 8
        ref = lambda value: ctypes.byref(value) if value is not None else None
        status = call(None, clips, times, 4, ctypes.byref(params), ref(consumers), ref(mapping), ref(layering), poses, stride, None)
        return status, lib.aclhip_last_error_message(None).decode()

    # one array alone is a layering: weights without masks, masks without weights pass the layering's own check (the null context is left)
    expected = {"layering": "null additive layering", "both arrays": "instance_weights or instance_masks", "reserved0": "reserved", "reserved1": "reserved",
                "no additive format": "additive_format is NONE", "consumers": "null consumers", "mapping": "null pose mapping", "no skeleton": "skeleton",
                "no map": "a map", "no blend maps": "blend_maps", "no base maps": "base_maps", "clips": "null instance list", "times": "null instance list",
                "poses": "output buffer", "stride": "16 byte aligned", "poses alignment": "16 byte aligned",
                "nothing (the null context is what is left)": "null context"}
    for spoil, words in expected.items():
        status, message = attempt(spoil)
        assert status == INVALID, spoil
        assert words in message, (spoil, message)
    for array in ("instance_weights", "instance_masks"):
        params, consumers, mapping, layering = runtime.default_params(), runtime.PoseConsumers(), runtime.PoseMapping(), runtime.AdditiveLayering()
        consumers.additive_format, consumers.base_poses, consumers.base_pose_stride_bytes = runtime.ADDITIVE_RELATIVE, aligned, 4800
        mapping.skeleton, mapping.map = 1, 1
        setattr(layering, array, aligned)
        assert call(None, aligned, aligned, 4, ctypes.byref(params), ctypes.byref(consumers), ctypes.byref(mapping), ctypes.byref(layering), aligned, 4800, None) == INVALID
        assert "null context" in lib.aclhip_last_error_message(None).decode(), array
