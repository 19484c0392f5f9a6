"""Track maps at the C ABI (aclhip_register_track_map, aclhip_decompress_tracks_batch_mapped, ...): declared, exported, bound; the
binding's structs have the C compiler's sizes; argument checks and the map validation that need no device (no GPU)."""
import ctypes
import os
import subprocess

import numpy as np

from acl_amd import runtime
from test_capi_symbols import declared_functions

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("aclhip_check_track_map", "aclhip_register_track_map", "aclhip_unregister_track_map", "aclhip_get_track_map_info", "aclhip_decompress_tracks_batch_mapped")
DROPPED = 0xFFFFFFFF


def test_header_declares_and_library_exports_the_entry_points():
    declared = declared_functions()
    lib = runtime.load_library()
    for name in NAMES:
        assert name in declared, name
        assert hasattr(lib, name), name
        assert name in runtime.EXPORTED_SYMBOLS, name
    assert runtime.TRACK_DROPPED == DROPPED


def test_struct_sizes_match_a_c99_translation_unit(tmp_path):
    lib_dir = os.path.dirname(runtime.library_path())
    binary = tmp_path / "track_map_abi"
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "c", "track_map_abi.c"),
                    "-L" + lib_dir, "-laclhip", "-Wl,-rpath," + lib_dir, "-o", str(binary)], check=True)
    done = subprocess.run([str(binary)], stdout=subprocess.PIPE, text=True, timeout=120)
    assert done.returncode == 0, done.returncode        # (the program's own argument and validation checks)
    mapping_size, info_size, map_offset, instance_maps_offset, fill_pose_offset, fill_unmapped_offset = (int(word) for word in done.stdout.split())
    assert ctypes.sizeof(runtime.TrackMapping) == mapping_size == 32
    assert ctypes.sizeof(runtime.TrackMapInfo) == info_size == 32
    assert (runtime.TrackMapping.map.offset, runtime.TrackMapping.instance_maps.offset, runtime.TrackMapping.fill_pose.offset, runtime.TrackMapping.fill_unmapped.offset) \
        == (map_offset, instance_maps_offset, fill_pose_offset, fill_unmapped_offset)


def test_argument_checks_that_return_before_any_hip_call():
    lib = runtime.load_library()
    table = np.arange(4, dtype=np.uint32)
    handle = ctypes.c_uint32(99)
    invalid = runtime.ERROR_INVALID_ARGUMENT
    assert lib.aclhip_register_track_map(None, table.ctypes.data, 4, 4, ctypes.byref(handle)) == invalid
    assert lib.aclhip_unregister_track_map(None, 1) == invalid
    assert lib.aclhip_get_track_map_info(None, 1, ctypes.byref(runtime.TrackMapInfo())) == invalid
    params, mapping = runtime.default_params(), runtime.TrackMapping()
    assert lib.aclhip_decompress_tracks_batch_mapped(None, None, None, 4, ctypes.byref(params), None, ctypes.byref(mapping), None, 4800, None) == invalid
    assert lib.aclhip_decompress_tracks_batch_mapped(None, None, None, 0, ctypes.byref(params), None, None, None, 4800, None) == invalid
    # host only validation: null table, no tracks, no slots
    info = runtime.TrackMapInfo()
    assert lib.aclhip_check_track_map(None, 4, 4, ctypes.byref(info), None, 0) == invalid
    assert lib.aclhip_check_track_map(table.ctypes.data, 0, 4, ctypes.byref(info), None, 0) == invalid
    assert lib.aclhip_check_track_map(table.ctypes.data, 4, 0, ctypes.byref(info), None, 0) == invalid


def test_map_validation_names_the_first_offending_track():
    status, message, _ = runtime.check_track_map([0, 1, 2, 1, 2], 8)
    assert status == runtime.ERROR_INVALID_ARGUMENT and "track 3" in message and "slot 1" in message, message
    status, message, _ = runtime.check_track_map([0, 8, 9], 8)
    assert status == runtime.ERROR_INVALID_ARGUMENT and "track 1" in message and "slot 8" in message, message
    status, message, _ = runtime.check_track_map([3, DROPPED - 1], 8)       # (only 0xFFFFFFFF is "dropped")
    assert status == runtime.ERROR_INVALID_ARGUMENT and "track 1" in message, message
    status, _, info = runtime.check_track_map([DROPPED] * 5, 3)
    assert status == 0 and (info.num_mapped, info.num_dropped, info.num_unmapped_slots, info.is_identity, info.is_order_preserving) == (0, 5, 3, 0, 1)
    status, _, info = runtime.check_track_map(np.arange(7), 7)
    assert status == 0 and (info.num_mapped, info.num_dropped, info.num_unmapped_slots, info.is_identity, info.is_order_preserving) == (7, 0, 0, 1, 1)
    status, _, info = runtime.check_track_map(np.arange(7), 9)
    assert status == 0 and info.is_identity == 0 and info.is_order_preserving == 1 and info.num_unmapped_slots == 2


def restated_info(table, num_slots):
    """numpy restatement of aclhip_track_map_info"""
    table = np.asarray(table, dtype=np.uint64)
    mapped = table[table != DROPPED]
    return dict(num_tracks=table.size, num_slots=num_slots, num_mapped=mapped.size, num_dropped=table.size - mapped.size, num_unmapped_slots=num_slots - mapped.size,
                is_identity=int(table.size == num_slots and np.array_equal(table, np.arange(table.size))),
                is_order_preserving=int(bool(np.all(np.diff(mapped.astype(np.int64)) > 0))))


def test_info_fields_against_a_numpy_restatement_over_random_maps():
    rng = np.random.default_rng(2024)
    for case in range(400):
        num_tracks = int(rng.integers(1, 140))
        num_slots = int(rng.integers(1, 200))
        kind = case % 4
        keep = min(num_tracks, num_slots) if kind != 3 else int(rng.integers(0, min(num_tracks, num_slots) + 1))
        slots = rng.choice(num_slots, size=keep, replace=False)
        if kind in (0, 3):
            slots = np.sort(slots)
        table = np.full(num_tracks, DROPPED, dtype=np.uint32)
        table[np.sort(rng.choice(num_tracks, size=keep, replace=False))] = slots
        if kind == 2 and num_tracks == num_slots:
            table = np.arange(num_tracks, dtype=np.uint32)
        status, message, info = runtime.check_track_map(table, num_slots)
        assert status == 0, (case, message)
        expected = restated_info(table, num_slots)
        assert {name: getattr(info, name) for name in expected} == expected, (case, table, num_slots)
        # one broken entry: a duplicate, or a slot out of range
        mapped_tracks = np.flatnonzero(table != DROPPED)
        broken = table.copy()
        if mapped_tracks.size >= 2 and case % 2 == 0:
            first, second = np.sort(rng.choice(mapped_tracks, size=2, replace=False))
            broken[second] = broken[first]
            offender = second
        else:
            offender = int(rng.integers(0, num_tracks))
            broken[offender] = num_slots + int(rng.integers(0, 5))
        status, message, _ = runtime.check_track_map(broken, num_slots)
        assert status == runtime.ERROR_INVALID_ARGUMENT and ("track %d " % offender) in message, (case, message, offender)


def test_cpp_mirror_of_the_track_maps_compiles_warning_free(tmp_path):
    """aclhip.hpp: device::register_track_map takes a track_to_slot vector, decompress_tracks_mapped sits next to decompress_tracks"""
    source = tmp_path / "track_map_mirror.cpp"
    source.write_text(
        '#include "%s"\n'
        "int main()\n"
        "{\n"
        "\taclhip::device gpu(0);\n"
        "\tconst std::vector<uint32_t> track_to_slot{ 2, ACLHIP_TRACK_DROPPED, 0 };\n"
        "\tconst aclhip_track_map map = gpu.register_track_map(track_to_slot, 4);\n"
        "\tconst bool decoded = aclhip::decompress_tracks_mapped(gpu, nullptr, nullptr, 0, map, nullptr, nullptr, 0);\n"
        "\treturn gpu.unregister_track_map(map) && decoded ? 0 : 1;\n"
        "}\n" % os.path.join(ROOT, "acl_amd", "csrc", "aclhip.hpp"))
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fsyntax-only", str(source)], check=True)
