"""Raw track arrays at the C ABI (aclhip_check_raw_tracks, aclhip_register_raw_tracks, aclhip_unregister_raw_tracks,
aclhip_get_raw_tracks_info, aclhip_sample_raw_tracks_batch): declared, exported, bound; the binding's structs have the C compiler's sizes
and offsets; every refusal of the array check with its message, and every ACLHIP_ERROR_INVALID_ARGUMENT of the launch, which are decided
before any device call (no GPU)."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

from acl_amd import runtime
from oracle import bindings as ob
from test_capi_symbols import declared_functions

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("aclhip_check_raw_tracks", "aclhip_register_raw_tracks", "aclhip_unregister_raw_tracks", "aclhip_get_raw_tracks_info", "aclhip_sample_raw_tracks_batch")
INVALID = runtime.ERROR_INVALID_ARGUMENT
CLAMP, WRAP, AS_COMPRESSED = runtime.LOOP_CLAMP, runtime.LOOP_WRAP, runtime.LOOP_AS_COMPRESSED


def fields_of(info):
    return (info.num_tracks, info.num_samples, info.sample_rate, info.looping_policy, tuple(info.reserved))


def check(num_tracks, num_samples, sample_rate, looping, samples=0x1000):
    """the check through the library itself: it tests `samples` against NULL and reads nothing"""
    message, info = ctypes.create_string_buffer(256), runtime.RawTracksInfo()
    status = runtime.load_library().aclhip_check_raw_tracks(samples, num_tracks, num_samples, sample_rate, looping, ctypes.byref(info), message, 256)
    return status, message.value.decode(), info


def test_header_declares_library_exports_and_binding_binds_the_entry_points():
    declared = declared_functions()
    lib = runtime.load_library()
    for name in NAMES:
        assert name in declared, name
        assert hasattr(lib, name), name
        assert name in runtime.EXPORTED_SYMBOLS, name
    for method in ("register_raw_tracks", "unregister_raw_tracks", "raw_tracks_info", "sample_raw_tracks_batch"):
        assert hasattr(runtime.Context, method)
    assert callable(runtime.check_raw_tracks) and callable(runtime.raw_clip_error)
    assert lib.aclhip_abi_version() == runtime.ABI_VERSION == 6       # (added without a bump: no existing struct changed)


def test_struct_sizes_and_offsets_match_a_c99_translation_unit(tmp_path):
    lib_dir = os.path.dirname(runtime.library_path())
    binary = tmp_path / "raw_tracks_abi"
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "c", "raw_tracks_abi.c"),
                    "-L" + lib_dir, "-laclhip", "-Wl,-rpath," + lib_dir, "-o", str(binary)], check=True)
    done = subprocess.run([str(binary)], stdout=subprocess.PIPE, text=True, timeout=120)
    assert done.returncode == 0, done.returncode        # (the program's own argument and validation checks)
    words = [int(word) for word in done.stdout.split()]
    desc, info = runtime.RawSampleDesc, runtime.RawTracksInfo
    assert ctypes.sizeof(desc) == words[0] == 56
    assert ctypes.sizeof(info) == words[1] == 32
    names = ("rounding_policy", "reserved0", "instance_rounding_policies", "track_rounding_policies", "num_track_rounding_policies", "reserved1", "rows", "reserved")
    assert [getattr(desc, name).offset for name in names] == words[2:10] == [0, 1, 8, 16, 24, 28, 32, 40]
    names = ("num_tracks", "num_samples", "sample_rate", "duration", "looping_policy", "reserved")
    assert [getattr(info, name).offset for name in names] == words[10:16] == [0, 4, 8, 12, 16, 20]
    assert runtime.MAX_RAW_TRACKS == words[16] == 4096
    assert words[17] == 4


def test_arrays_that_pass_and_what_their_info_says():
    oracle = ob.oracle()
    for num_tracks, num_samples, rate, looping in ((1, 1, 30.0, CLAMP), (1, 1, 30.0, WRAP), (100, 301, 30.0, CLAMP), (0xFFFF, 2, 24.0, WRAP), (7, 31, 0.7, WRAP),
                                                   (1, (1 << 31) // 48, 1.0e-3, CLAMP), (3, 5, 3.0e38, CLAMP)):
        status, message, info = check(num_tracks, num_samples, rate, looping)
        assert status == 0 and message == "", message
        assert fields_of(info) == (num_tracks, num_samples, np.float32(rate), looping, (0, 0, 0))
        # track_array::get_finite_duration: calculate_finite_duration(num_samples + (wrap ? 1 : 0), sample_rate)
        want = oracle.aclo_calculate_finite_duration(num_samples + (1 if looping == WRAP else 0), ctypes.c_float(rate))
        assert np.float32(info.duration).view(np.uint32) == np.float32(want).view(np.uint32)
    # the values are not looked at: the binding's form takes an array of NaNs
    samples = np.full((3, 2, 12), np.nan, dtype=np.float32)
    status, message, info = runtime.check_raw_tracks(samples, 30.0, WRAP)
    assert status == 0 and fields_of(info) == (2, 3, 30.0, WRAP, (0, 0, 0)) and info.duration == np.float32(3.0) / np.float32(30.0)
    with pytest.raises(ValueError):
        runtime.check_raw_tracks(np.zeros((3, 2, 10), dtype=np.float32), 30.0)


def test_every_refusal_has_its_message():
    cases = [
        ((1, 2, 30.0, CLAMP, None), "null samples"),
        ((0, 2, 30.0, CLAMP), "0 tracks"),
        ((0x10000, 2, 30.0, CLAMP), "65536 tracks"),
        ((1, 0, 30.0, CLAMP), "0 samples"),
        ((1, (1 << 31) // 48 + 1, 30.0, CLAMP), "2^31 bytes"),
        ((0xFFFF, 683, 30.0, CLAMP), "2^31 bytes"),                 # 65535 * 683 * 48 is the first product past it
        ((100, 0xFFFFFFFF, 30.0, CLAMP), "2^31 bytes"),             # (no 32 bit product)
        ((1, 2, 0.0, CLAMP), "sample rate"),
        ((1, 2, -30.0, CLAMP), "sample rate"),
        ((1, 2, float("inf"), CLAMP), "sample rate"),
        ((1, 2, float("nan"), CLAMP), "sample rate"),
        ((1, 2, 30.0, AS_COMPRESSED), "ACLHIP_LOOP_AS_COMPRESSED"),
        ((1, 2, 30.0, 3), "unknown looping policy 3"),
        ((1, 2, 30.0, 0xFFFFFFFF), "unknown looping policy"),
    ]
    for arguments, text in cases:
        status, message, info = check(*arguments)
        assert status == INVALID and text in message, (arguments, message)
        assert fields_of(info) == (0, 0, 0.0, 0, (0, 0, 0))
    assert check(0xFFFF, 682, 30.0, CLAMP)[0] == 0                  # the last product below 2^31
    # out_info and message are optional; a refused array leaves out_info alone; a short message buffer is not overrun
    lib = runtime.load_library()
    assert lib.aclhip_check_raw_tracks(0x1000, 1, 2, 30.0, CLAMP, None, None, 0) == 0
    info = runtime.RawTracksInfo(7, 7, 7.0, 7.0, 7)
    assert lib.aclhip_check_raw_tracks(0x1000, 0, 2, 30.0, CLAMP, ctypes.byref(info), None, 0) == INVALID
    assert fields_of(info) == (7, 7, 7.0, 7, (0, 0, 0))
    short = ctypes.create_string_buffer(8)
    assert lib.aclhip_check_raw_tracks(0x1000, 0x10000, 2, 30.0, CLAMP, None, short, 8) == INVALID and len(short.value) <= 7


def test_registration_checks_that_return_before_any_hip_call():
    lib = runtime.load_library()
    samples = np.zeros((2, 3, 12), dtype=np.float32)
    handle = ctypes.c_uint32(99)
    # refused arrays are refused without a context too, with the check's message
    assert lib.aclhip_register_raw_tracks(None, samples.ctypes.data, 3, 2, 30.0, AS_COMPRESSED, ctypes.byref(handle)) == INVALID and handle.value == 0
    assert "ACLHIP_LOOP_AS_COMPRESSED" in lib.aclhip_last_error_message(None).decode()
    assert lib.aclhip_register_raw_tracks(None, None, 3, 2, 30.0, CLAMP, ctypes.byref(handle)) == INVALID
    assert lib.aclhip_last_error_message(None).decode() == "null samples"
    assert lib.aclhip_register_raw_tracks(None, samples.ctypes.data, 3, 2, 30.0, CLAMP, None) == INVALID
    assert lib.aclhip_last_error_message(None).decode() == "null out_raw"
    assert lib.aclhip_register_raw_tracks(None, samples.ctypes.data, 3, 2, 30.0, CLAMP, ctypes.byref(handle)) == INVALID
    assert lib.aclhip_last_error_message(None).decode() == "null context"
    assert lib.aclhip_unregister_raw_tracks(None, 1) == INVALID
    assert lib.aclhip_get_raw_tracks_info(None, 1, ctypes.byref(runtime.RawTracksInfo())) == INVALID
    assert lib.aclhip_get_raw_tracks_info(None, 1, None) == INVALID


RAWS, TIMES, POSES, STRIDE, COUNT = 0x10000, 0x20000, 0x100000, 4800, 16        # addresses nobody reads: every case returns before a device call


def sample(desc=None, raws=RAWS, times=TIMES, poses=POSES, stride=STRIDE, count=COUNT):
    lib = runtime.load_library()
    status = lib.aclhip_sample_raw_tracks_batch(None, raws, times, count, ctypes.byref(desc) if desc is not None else None, poses, stride, None)
    return status, lib.aclhip_last_error_message(None).decode()


def desc_with(**fields):
    desc = runtime.RawSampleDesc()
    for name, value in fields.items():
        setattr(desc, name, value)
    return desc


def test_every_invalid_argument_of_the_launch_has_its_message():
    # what passes the checks ends at the missing context, with or without a desc
    assert sample() == (INVALID, "null context")
    assert sample(desc_with(rounding_policy=runtime.ROUND_NEAREST, rows=0x30000, instance_rounding_policies=0x40000)) == (INVALID, "null context")
    assert sample(desc_with(rounding_policy=runtime.ROUND_PER_TRACK, track_rounding_policies=0x50000, num_track_rounding_policies=100)) == (INVALID, "null context")
    assert sample(desc_with(track_rounding_policies=0x50000, num_track_rounding_policies=1)) == (INVALID, "null context")

    assert sample(raws=None) == (INVALID, "null raw track handles")
    assert sample(times=None) == (INVALID, "null sample times")
    assert sample(poses=None) == (INVALID, "null pose buffer")
    for arguments in ({"poses": POSES + 8}, {"stride": STRIDE + 8}, {"poses": POSES + 4, "stride": STRIDE + 12}):
        assert sample(**arguments) == (INVALID, "pose buffer and stride must be 16 byte aligned")
    for policy in (5, 255):
        assert sample(desc_with(rounding_policy=policy)) == (INVALID, "unknown rounding policy %d" % policy)
    assert sample(desc_with(rounding_policy=runtime.ROUND_PER_TRACK)) == (INVALID, "ACLHIP_ROUND_PER_TRACK needs track_rounding_policies")
    assert sample(desc_with(track_rounding_policies=0x50000)) == (INVALID, "track_rounding_policies with a count of 0")
    reserved = [desc_with(reserved1=1), desc_with(reserved=(ctypes.c_uint64 * 2)(0, 1)), desc_with(reserved=(ctypes.c_uint64 * 2)(1 << 63, 0))]
    reserved += [desc_with(reserved0=(ctypes.c_uint8 * 7)(*[1 if k == byte else 0 for k in range(7)])) for byte in range(7)]
    for desc in reserved:
        assert sample(desc) == (INVALID, "the reserved fields of a raw sample desc are 0")

    # the output range -- COUNT rows of STRIDE bytes from POSES -- against every array the launch reads: its first and its last byte
    end = POSES + STRIDE * COUNT
    for raws in (POSES, end - 1, POSES - 4 * COUNT + 1):
        assert sample(raws=raws) == (INVALID, "the pose rows overlap the raw track handles")
    for times in (POSES + 4800, end - 4, POSES - 4 * COUNT + 4):
        assert sample(times=times) == (INVALID, "the pose rows overlap the sample times")
    for address in (POSES, end - 1, POSES - COUNT + 1):
        assert sample(desc_with(instance_rounding_policies=address)) == (INVALID, "the pose rows overlap the instance rounding policies")
    for address in (POSES + 16, end - 4, POSES - 4 * COUNT + 4):
        assert sample(desc_with(rows=address)) == (INVALID, "the pose rows overlap the row list")
    for address, count in ((POSES, 1), (end - 1, 1), (POSES - 99, 100)):
        assert sample(desc_with(track_rounding_policies=address, num_track_rounding_policies=count)) == (INVALID, "the pose rows overlap the track rounding policies")
    # arrays that end where the rows begin, or begin where they end, do not overlap
    assert sample(raws=POSES - 4 * COUNT, times=end) == (INVALID, "null context")
    assert sample(desc_with(rows=end, instance_rounding_policies=POSES - COUNT, track_rounding_policies=POSES - 100, num_track_rounding_policies=100)) == (INVALID, "null context")
    # no instances: nothing can overlap, and the launch would be a no-op
    assert sample(raws=POSES, count=0) == (INVALID, "null context")
    # a stride of 0 leaves the rows a point: inside the policy table it overlaps, at the table's end it does not
    assert sample(desc_with(track_rounding_policies=POSES - 50, num_track_rounding_policies=100), stride=0) == (INVALID, "the pose rows overlap the track rounding policies")
    assert sample(desc_with(track_rounding_policies=POSES - 100, num_track_rounding_policies=100), stride=0) == (INVALID, "null context")
