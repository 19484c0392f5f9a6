"""Character bounds at the C ABI (aclhip_pose_bounds, aclhip_decompress_poses_batch_bounds): declared, exported, bound; the binding's struct
has the C compiler's size and offsets; every ACLHIP_ERROR_INVALID_ARGUMENT case that is decided before a device call returns it with a
message (no GPU)."""
import ctypes
import os
import subprocess

from acl_amd import runtime
from test_capi_symbols import declared_functions

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "aclhip_decompress_poses_batch_bounds"
INVALID = runtime.ERROR_INVALID_ARGUMENT


def test_header_declares_and_library_exports_the_entry_point():
    lib = runtime.load_library()
    assert NAME in declared_functions()
    assert hasattr(lib, NAME)
    assert NAME in runtime.EXPORTED_SYMBOLS
    assert lib.aclhip_abi_version() == runtime.ABI_VERSION == 6       # (added without a bump: no existing struct changed)
    assert ctypes.sizeof(runtime.PoseConsumers) == 72 and ctypes.sizeof(runtime.PoseMapping) == 56 and ctypes.sizeof(runtime.BlendMasking) == 32


def test_struct_size_and_offsets_match_a_c99_translation_unit(tmp_path):
    lib_dir = os.path.dirname(runtime.library_path())
    binary = tmp_path / "pose_bounds_abi"
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "c", "pose_bounds_abi.c"),
                    "-L" + lib_dir, "-laclhip", "-Wl,-rpath," + lib_dir, "-o", str(binary)], check=True)
    done = subprocess.run([str(binary)], stdout=subprocess.PIPE, text=True, timeout=120)
    assert done.returncode == 0, done.returncode        # (the program's own argument checks)
    words = [int(word) for word in done.stdout.split()]
    bounds = runtime.PoseBounds
    assert ctypes.sizeof(bounds) == words[0] == 32
    assert [bounds.bounds.offset, bounds.bone_flags.offset, bounds.reserved.offset] == words[1:4] == [0, 8, 16]
    assert words[4] == 6


def test_every_refusal_decided_before_a_device_call_has_a_message():
    lib = runtime.load_library()
    call = lib.aclhip_decompress_poses_batch_bounds
    box = (ctypes.c_float * 12)()
    aligned = (ctypes.addressof(box) + 15) & ~15                     # a HOST address: nothing below reaches a device call

    def attempt(spoil):
        params, consumers, mapping, masking, bounds = runtime.default_params(), runtime.PoseConsumers(), None, None, runtime.PoseBounds()
        consumers.object_space, bounds.bounds = 1, aligned
        clips, times, poses, stride = aligned, aligned, None, 4800
        if spoil == "bounds":
            bounds = None
        if spoil == "buffer":
            bounds.bounds = None
        if spoil == "alignment":
            bounds.bounds = aligned + 4
        if spoil in ("reserved0", "reserved1"):
            bounds.reserved[int(spoil[-1])] = 1
        if spoil == "consumers":
            consumers = None
        if spoil == "local space":
            consumers.object_space = 0
        if spoil == "masking without mapping":
            masking = runtime.BlendMasking()
        if spoil == "clips":
            clips = None
        if spoil == "times":
            times = None
        if spoil == "stride":
            stride = 4808
        if spoil == "poses alignment":
            poses = aligned + 8
        if spoil in ("no skeleton", "no map", "no blend maps", "no base maps", "mode", "masking reserved", "no masks", "no blend"):
            mapping = runtime.PoseMapping()
            mapping.skeleton, mapping.map, mapping.blend_maps = 1, 1, aligned
        if spoil == "no skeleton":
            mapping.skeleton = 0
        if spoil == "no map":
            mapping.map = 0
        if spoil == "no blend maps":
            consumers.num_blend_clips, mapping.blend_maps = 2, None
        if spoil == "no base maps":
            consumers.additive_format, consumers.base_clips = runtime.ADDITIVE_ADDITIVE1, aligned
        if spoil in ("mode", "masking reserved", "no masks", "no blend"):
            masking = runtime.BlendMasking()
            masking.instance_masks, consumers.num_blend_clips = aligned, 2
        if spoil == "mode":
            masking.mode = 2
        if spoil == "masking reserved":
            masking.reserved[1] = 1
        if spoil == "no masks":
            masking.instance_masks = None
        if spoil == "no blend":
            consumers.num_blend_clips = 1
        ref = lambda value: ctypes.byref(value) if value is not None else None
        status = call(None, clips, times, 4, ctypes.byref(params), ref(consumers), ref(mapping), ref(masking), ref(bounds), poses, stride, None)
        return status, lib.aclhip_last_error_message(None).decode()

    expected = {"bounds": "null pose bounds", "buffer": "bounds buffer", "alignment": "16 byte aligned", "reserved0": "reserved", "reserved1": "reserved",
                "consumers": "null consumers", "local space": "object space", "masking without mapping": "pose mapping", "clips": "null instance list",
                "times": "null instance list", "stride": "16 byte aligned", "poses alignment": "16 byte aligned", "no skeleton": "skeleton", "no map": "a map",
                "no blend maps": "blend_maps", "no base maps": "base_maps", "mode": "blend mode", "masking reserved": "reserved", "no masks": "list of masks",
                "no blend": "num_blend_clips", "nothing (the null context is what is left)": "null context"}
    for spoil, words in expected.items():
        status, message = attempt(spoil)
        assert status == INVALID, spoil
        assert words in message, (spoil, message)
