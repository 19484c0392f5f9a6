"""Raw scalar track arrays and the scalar track error at the C ABI (aclhip_check_raw_scalar_tracks, aclhip_register_raw_scalar_tracks,
aclhip_unregister_raw_scalar_tracks, aclhip_get_raw_scalar_tracks_info, aclhip_sample_raw_scalar_tracks_batch,
aclhip_sample_raw_scalar_track_batch, aclhip_measure_scalar_error_batch): declared, exported, bound; the binding's structs have the C
compiler's sizes and offsets; every refusal of the array check with its message, and every ACLHIP_ERROR_INVALID_ARGUMENT of the three
launches and the registration, which are decided before any device call and leave a message with a NULL context too (no GPU)."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

from acl_amd import runtime
from oracle import bindings as ob
from test_capi_symbols import declared_functions

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("aclhip_check_raw_scalar_tracks", "aclhip_register_raw_scalar_tracks", "aclhip_unregister_raw_scalar_tracks", "aclhip_get_raw_scalar_tracks_info",
         "aclhip_sample_raw_scalar_tracks_batch", "aclhip_sample_raw_scalar_track_batch", "aclhip_measure_scalar_error_batch")
INVALID = runtime.ERROR_INVALID_ARGUMENT
CLAMP, WRAP, AS_COMPRESSED = runtime.LOOP_CLAMP, runtime.LOOP_WRAP, runtime.LOOP_AS_COMPRESSED
COMPONENTS = {0: 1, 1: 2, 2: 3, 3: 4, 4: 4}


def fields_of(info):
    return (info.num_tracks, info.num_samples, info.sample_rate, info.looping_policy, info.track_type, info.num_components, info.reserved)


def check(track_type, num_tracks, num_samples, sample_rate, looping, samples=0x1000):
    """the check through the library itself: it tests `samples` against NULL and reads nothing"""
    message, info = ctypes.create_string_buffer(256), runtime.RawScalarTracksInfo()
    status = runtime.load_library().aclhip_check_raw_scalar_tracks(samples, track_type, num_tracks, num_samples, sample_rate, looping, ctypes.byref(info), message, 256)
    return status, message.value.decode(), info


def test_header_declares_library_exports_and_binding_binds_the_entry_points():
    declared = declared_functions()
    lib = runtime.load_library()
    for name in NAMES:
        assert name in declared, name
        assert hasattr(lib, name), name
        assert name in runtime.EXPORTED_SYMBOLS, name
    for method in ("register_raw_scalar_tracks", "unregister_raw_scalar_tracks", "raw_scalar_tracks_info", "sample_raw_scalar_tracks_batch", "sample_raw_scalar_track_batch",
                   "measure_scalar_error"):
        assert hasattr(runtime.Context, method)
    assert callable(runtime.check_raw_scalar_tracks) and callable(runtime.raw_scalar_clip_error) and callable(runtime.scalar_clip_error)
    assert lib.aclhip_abi_version() == runtime.ABI_VERSION == 6       # (added without a bump: no existing struct changed)
    assert runtime.NO_TRACK == runtime.NO_BONE == 0xFFFFFFFF


def test_struct_sizes_and_offsets_match_a_c99_translation_unit(tmp_path):
    lib_dir = os.path.dirname(runtime.library_path())
    binary = tmp_path / "raw_scalar_tracks_abi"
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "c", "raw_scalar_tracks_abi.c"),
                    "-L" + lib_dir, "-laclhip", "-Wl,-rpath," + lib_dir, "-o", str(binary)], check=True)
    done = subprocess.run([str(binary)], stdout=subprocess.PIPE, text=True, timeout=120)
    assert done.returncode == 0, done.returncode        # (the program's own argument and validation checks)
    words = [int(word) for word in done.stdout.split()]
    desc, info = runtime.ScalarErrorDesc, runtime.RawScalarTracksInfo
    assert ctypes.sizeof(desc) == words[0] == 48
    assert ctypes.sizeof(info) == words[1] == 32
    names = ("num_tracks", "num_components", "track_errors", "track_error_stride_bytes", "worst", "reserved")
    assert [getattr(desc, name).offset for name in names] == words[2:8] == [0, 4, 8, 16, 24, 32]
    names = ("num_tracks", "num_samples", "sample_rate", "duration", "looping_policy", "track_type", "num_components", "reserved")
    assert [getattr(info, name).offset for name in names] == words[8:16] == [0, 4, 8, 12, 16, 20, 24, 28]
    assert runtime.MAX_RAW_SCALAR_TRACKS == words[16] == 4096
    assert words[17:21] == [4, ctypes.sizeof(runtime.PoseError), ctypes.sizeof(runtime.PoseErrorWorst), 1] == [4, 8, 16, 1]
    assert runtime.TRACK_ERROR_DTYPE.itemsize == 8 and runtime.TRACK_ERROR_WORST_DTYPE.itemsize == 16


def test_arrays_that_pass_and_what_their_info_says():
    oracle = ob.oracle()
    for track_type, components in COMPONENTS.items():
        for num_tracks, num_samples, rate, looping in ((1, 1, 30.0, CLAMP), (1, 1, 30.0, WRAP), (100, 301, 30.0, CLAMP), (0xFFFF, 2, 24.0, WRAP), (7, 31, 0.7, WRAP),
                                                       (1, ((1 << 31) - 1) // (4 * components), 1.0e-3, CLAMP), (3, 5, 3.0e38, CLAMP)):
            status, message, info = check(track_type, num_tracks, num_samples, rate, looping)
            assert status == 0 and message == "", message
            assert fields_of(info) == (num_tracks, num_samples, np.float32(rate), looping, track_type, components, 0)
            # track_array::get_finite_duration: calculate_finite_duration(num_samples + (wrap ? 1 : 0), sample_rate)
            want = oracle.aclo_calculate_finite_duration(num_samples + (1 if looping == WRAP else 0), ctypes.c_float(rate))
            assert np.float32(info.duration).view(np.uint32) == np.float32(want).view(np.uint32)
    # the values are not looked at: the binding's form takes an array of NaNs, and [S, T] as float1f
    status, message, info = runtime.check_raw_scalar_tracks(np.full((3, 2, 3), np.nan, dtype=np.float32), runtime.TRACK_FLOAT3F, 30.0, WRAP)
    assert status == 0 and fields_of(info) == (2, 3, 30.0, WRAP, 2, 3, 0) and info.duration == np.float32(3.0) / np.float32(30.0)
    status, message, info = runtime.check_raw_scalar_tracks(np.zeros((3, 2), dtype=np.float32), runtime.TRACK_FLOAT1F, 30.0)
    assert status == 0 and fields_of(info) == (2, 3, 30.0, CLAMP, 0, 1, 0)
    with pytest.raises(ValueError):
        runtime.check_raw_scalar_tracks(np.zeros((3, 2, 3), dtype=np.float32), runtime.TRACK_VECTOR4F, 30.0)


def test_every_refusal_has_its_message():
    cases = [
        ((0, 1, 2, 30.0, CLAMP, None), "null samples"),
        ((0, 0, 2, 30.0, CLAMP), "0 tracks"),
        ((1, 0x10000, 2, 30.0, CLAMP), "65536 tracks"),
        ((2, 1, 0, 30.0, CLAMP), "0 samples"),
        ((0, 1, (1 << 31) // 4, 30.0, CLAMP), "2^31 bytes"),
        ((1, 1, (1 << 31) // 8, 30.0, CLAMP), "2^31 bytes"),
        ((2, 1, (1 << 31) // 12 + 1, 30.0, CLAMP), "2^31 bytes"),
        ((3, 1, (1 << 31) // 16, 30.0, CLAMP), "2^31 bytes"),
        ((4, 0xFFFF, 2049, 30.0, CLAMP), "2^31 bytes"),                 # 65535 * 2049 * 16 is the first product past it
        ((4, 100, 0xFFFFFFFF, 30.0, CLAMP), "2^31 bytes"),              # (no 32 bit product)
        ((0, 1, 2, 0.0, CLAMP), "sample rate"),
        ((0, 1, 2, -30.0, CLAMP), "sample rate"),
        ((0, 1, 2, float("inf"), CLAMP), "sample rate"),
        ((0, 1, 2, float("nan"), CLAMP), "sample rate"),
        ((0, 1, 2, 30.0, AS_COMPRESSED), "ACLHIP_LOOP_AS_COMPRESSED"),
        ((0, 1, 2, 30.0, 3), "unknown looping policy 3"),
        ((12, 1, 2, 30.0, CLAMP), "qvvf"),
        ((5, 1, 2, 30.0, CLAMP), "unknown track type 5"),
        ((11, 1, 2, 30.0, CLAMP), "unknown track type 11"),
        ((13, 1, 2, 30.0, CLAMP), "unknown track type 13"),
        ((0xFFFFFFFF, 1, 2, 30.0, CLAMP), "unknown track type"),
    ]
    for arguments, text in cases:
        status, message, info = check(*arguments)
        assert status == INVALID and text in message, (arguments, message)
        assert fields_of(info) == (0, 0, 0.0, 0, 0, 0, 0)
    assert check(4, 0xFFFF, 2048, 30.0, CLAMP)[0] == 0                  # the last product below 2^31
    assert check(2, 1, (1 << 31) // 12, 30.0, CLAMP)[0] == 0
    # out_info and message are optional; a refused array leaves out_info alone; a short message buffer is not overrun
    lib = runtime.load_library()
    assert lib.aclhip_check_raw_scalar_tracks(0x1000, 0, 1, 2, 30.0, CLAMP, None, None, 0) == 0
    info = runtime.RawScalarTracksInfo(7, 7, 7.0, 7.0, 7, 7, 7, 7)
    assert lib.aclhip_check_raw_scalar_tracks(0x1000, 0, 0, 2, 30.0, CLAMP, ctypes.byref(info), None, 0) == INVALID
    assert fields_of(info) == (7, 7, 7.0, 7, 7, 7, 7)
    short = ctypes.create_string_buffer(8)
    assert lib.aclhip_check_raw_scalar_tracks(0x1000, 12, 1, 2, 30.0, CLAMP, None, short, 8) == INVALID and len(short.value) <= 7


def test_registration_checks_that_return_before_any_hip_call():
    lib = runtime.load_library()
    samples = np.zeros((2, 3, 3), dtype=np.float32)
    handle = ctypes.c_uint32(99)

    def last():
        return lib.aclhip_last_error_message(None).decode()

    # refused arrays are refused without a context too, with the check's message
    for arguments, text in (((2, 3, 2, 30.0, AS_COMPRESSED), "ACLHIP_LOOP_AS_COMPRESSED"), ((12, 3, 2, 30.0, CLAMP), "qvvf"), ((7, 3, 2, 30.0, CLAMP), "unknown track type 7"),
                            ((2, 0, 2, 30.0, CLAMP), "0 tracks"), ((2, 3, 0, 30.0, CLAMP), "0 samples"), ((2, 3, 2, 0.0, CLAMP), "sample rate"),
                            ((4, 0xFFFF, 2049, 30.0, CLAMP), "2^31 bytes"), ((2, 0x10000, 2, 30.0, CLAMP), "65536 tracks"), ((2, 3, 2, 30.0, 9), "unknown looping policy 9")):
        handle.value = 99
        assert lib.aclhip_register_raw_scalar_tracks(None, samples.ctypes.data, *arguments, ctypes.byref(handle)) == INVALID and handle.value == 0
        assert text in last(), (arguments, last())
    assert lib.aclhip_register_raw_scalar_tracks(None, None, 2, 3, 2, 30.0, CLAMP, ctypes.byref(handle)) == INVALID
    assert last() == "null samples"
    assert lib.aclhip_register_raw_scalar_tracks(None, samples.ctypes.data, 2, 3, 2, 30.0, CLAMP, None) == INVALID
    assert last() == "null out_raw"
    assert lib.aclhip_register_raw_scalar_tracks(None, samples.ctypes.data, 2, 3, 2, 30.0, CLAMP, ctypes.byref(handle)) == INVALID
    assert last() == "null context"
    assert lib.aclhip_unregister_raw_scalar_tracks(None, 1) == INVALID
    assert lib.aclhip_get_raw_scalar_tracks_info(None, 1, ctypes.byref(runtime.RawScalarTracksInfo())) == INVALID
    assert lib.aclhip_get_raw_scalar_tracks_info(None, 1, None) == INVALID


RAWS, TIMES, TRACK_IDS, VALUES, STRIDE, COUNT = 0x10000, 0x20000, 0x28000, 0x100000, 268, 16      # addresses nobody reads: every case returns before a device call


def sample(desc=None, raws=RAWS, times=TIMES, tracks=None, values=VALUES, stride=STRIDE, count=COUNT, single=False):
    lib = runtime.load_library()
    desc = ctypes.byref(desc) if desc is not None else None
    if single:
        status = lib.aclhip_sample_raw_scalar_track_batch(None, raws, times, tracks, count, desc, values, stride, None)
    else:
        status = lib.aclhip_sample_raw_scalar_tracks_batch(None, raws, times, count, desc, values, stride, None)
    message = lib.aclhip_last_error_message(None).decode()
    assert status == INVALID and message != ""
    return message


def desc_with(**fields):
    desc = runtime.RawSampleDesc()
    for name, value in fields.items():
        setattr(desc, name, value)
    return desc


@pytest.mark.parametrize("single", [False, True], ids=["tracks", "track"])
def test_every_invalid_argument_of_the_sampling_launches_has_its_message(single):
    form = {"single": single, "tracks": TRACK_IDS if single else None}

    def refused(desc=None, **arguments):
        return sample(desc, **{**form, **arguments})

    # what passes the checks ends at the missing context, with or without a desc; a base and a stride that are only 4 byte aligned pass
    assert refused() == "null context"
    assert refused(values=VALUES + 4, stride=STRIDE + 4) == "null context"
    assert refused(desc_with(rounding_policy=runtime.ROUND_NEAREST, rows=0x30000, instance_rounding_policies=0x40000)) == "null context"
    assert refused(desc_with(rounding_policy=runtime.ROUND_PER_TRACK, track_rounding_policies=0x50000, num_track_rounding_policies=100)) == "null context"
    assert refused(desc_with(track_rounding_policies=0x50000, num_track_rounding_policies=1)) == "null context"

    assert refused(raws=None) == "null raw scalar track handles"
    assert refused(times=None) == "null sample times"
    assert refused(values=None) == "null value buffer"
    if single:
        assert refused(tracks=None) == "null track indices"
    for arguments in ({"values": VALUES + 2}, {"values": VALUES + 1}, {"stride": STRIDE + 2}, {"stride": STRIDE + 1}, {"stride": 0}):
        assert refused(**arguments) == "the value buffer and its stride must be 4 byte aligned, and the stride is not 0"
    for policy in (5, 255):
        assert refused(desc_with(rounding_policy=policy)) == "unknown rounding policy %d" % policy
    assert refused(desc_with(rounding_policy=runtime.ROUND_PER_TRACK)) == "ACLHIP_ROUND_PER_TRACK needs track_rounding_policies"
    assert refused(desc_with(track_rounding_policies=0x50000)) == "track_rounding_policies with a count of 0"
    reserved = [desc_with(reserved1=1), desc_with(reserved=(ctypes.c_uint64 * 2)(0, 1)), desc_with(reserved=(ctypes.c_uint64 * 2)(1 << 63, 0))]
    reserved += [desc_with(reserved0=(ctypes.c_uint8 * 7)(*[1 if k == byte else 0 for k in range(7)])) for byte in range(7)]
    for desc in reserved:
        assert refused(desc) == "the reserved fields of a raw sample desc are 0"

    # the output range -- COUNT rows of STRIDE bytes from VALUES -- against every array the launch reads: its first and its last byte
    end = VALUES + STRIDE * COUNT
    for raws in (VALUES, end - 1, VALUES - 4 * COUNT + 1):
        assert refused(raws=raws) == "the value rows overlap the raw scalar track handles"
    for times in (VALUES + 268, end - 4, VALUES - 4 * COUNT + 4):
        assert refused(times=times) == "the value rows overlap the sample times"
    if single:
        for tracks in (VALUES + 4, end - 4, VALUES - 4 * COUNT + 4):
            assert refused(tracks=tracks) == "the value rows overlap the track indices"
    for address in (VALUES, end - 1, VALUES - COUNT + 1):
        assert refused(desc_with(instance_rounding_policies=address)) == "the value rows overlap the instance rounding policies"
    for address in (VALUES + 16, end - 4, VALUES - 4 * COUNT + 4):
        assert refused(desc_with(rows=address)) == "the value rows overlap the row list"
    for address, count in ((VALUES, 1), (end - 1, 1), (VALUES - 99, 100)):
        assert refused(desc_with(track_rounding_policies=address, num_track_rounding_policies=count)) == "the value rows overlap the track rounding policies"
    # arrays that end where the rows begin, or begin where they end, do not overlap
    assert refused(raws=VALUES - 4 * COUNT, times=end) == "null context"
    assert refused(desc_with(rows=end, instance_rounding_policies=VALUES - COUNT, track_rounding_policies=VALUES - 100, num_track_rounding_policies=100)) == "null context"
    # no instances: nothing can overlap, and the launch would be a no-op
    assert refused(raws=VALUES, count=0) == "null context"


RAW_VALUES, LOSSY_VALUES, ERRORS, TRACK_ERRORS, WORST = 0x100000, 0x200000, 0x300000, 0x400000, 0x500000
T, C = 22, 3


def measure(raw=RAW_VALUES, raw_stride=STRIDE, lossy=LOSSY_VALUES, lossy_stride=STRIDE, count=COUNT, errors=ERRORS, no_desc=False, **fields):
    lib = runtime.load_library()
    desc = runtime.ScalarErrorDesc()
    desc.num_tracks, desc.num_components = T, C
    for name, value in fields.items():
        setattr(desc, name, value)
    status = lib.aclhip_measure_scalar_error_batch(None, raw, raw_stride, lossy, lossy_stride, count, None if no_desc else ctypes.byref(desc), errors, None)
    message = lib.aclhip_last_error_message(None).decode()
    assert status == INVALID and message != ""
    return message


def test_every_invalid_argument_of_the_measure_has_its_message():
    everything = {"track_errors": TRACK_ERRORS, "track_error_stride_bytes": 4 * T, "worst": WORST}
    assert measure() == "null context"
    assert measure(**everything) == "null context"
    assert measure(lossy=RAW_VALUES, **everything) == "null context"                                    # raw and lossy may be the same buffer
    assert measure(raw=RAW_VALUES + 4, raw_stride=4 * C * T, lossy_stride=4 * C * T + 4, errors=ERRORS + 8) == "null context"
    for components in (1, 2, 3, 4):
        assert measure(num_components=components, num_tracks=STRIDE // (4 * components)) == "null context"

    assert measure(no_desc=True) == "null scalar error desc"
    assert measure(raw=None) == "null raw value buffer"
    assert measure(lossy=None) == "null lossy value buffer"
    assert measure(errors=None) == "null track error records"
    assert measure(num_tracks=0) == "a scalar error desc of 0 tracks"
    for components in (0, 5, 0xFFFFFFFF):
        assert "components per track" in measure(num_components=components)
    assert "do not fit the value strides" in measure(raw_stride=4 * C * T - 4)
    assert "do not fit the value strides" in measure(lossy_stride=4 * C * T - 4)
    assert "do not fit the value strides" in measure(num_tracks=0xFFFFFFFF, num_components=4)          # (no 32 bit product)
    message = "track errors are 4 byte aligned and their stride is a multiple of 4 that holds every track"
    for fields in ({"track_error_stride_bytes": 0}, {"track_error_stride_bytes": 4 * T + 2}, {"track_error_stride_bytes": 4 * T - 4}, {"track_errors": TRACK_ERRORS + 2, "track_error_stride_bytes": 4 * T}):
        assert measure(**{"track_errors": TRACK_ERRORS, **fields}) == message
    assert measure(raw=RAW_VALUES + 2) == measure(raw_stride=STRIDE + 2) == "raw value buffer and stride must be 4 byte aligned"
    assert measure(lossy=LOSSY_VALUES + 1) == measure(lossy_stride=STRIDE + 1) == "lossy value buffer and stride must be 4 byte aligned"
    assert measure(errors=ERRORS + 4) == "track error records must be 8 byte aligned"
    assert measure(worst=WORST + 8) == "the worst track error record must be 16 byte aligned"
    for reserved in ((1, 0), (0, 1 << 63)):
        assert measure(reserved=(ctypes.c_uint64 * 2)(*reserved)) == "the reserved fields of a scalar error desc are 0"

    # every output range against every input and every other output: its first and its last byte
    raw_end, lossy_end = RAW_VALUES + STRIDE * COUNT, LOSSY_VALUES + STRIDE * COUNT
    for errors in (RAW_VALUES, raw_end - 8, RAW_VALUES - 8 * COUNT + 8):
        assert measure(errors=errors) == "the track error records overlap the raw value rows"
    assert measure(errors=lossy_end - 8) == "the track error records overlap the lossy value rows"
    assert measure(track_errors=RAW_VALUES + 4, track_error_stride_bytes=4 * T) == "the track errors overlap the raw value rows"
    assert measure(track_errors=lossy_end - 4, track_error_stride_bytes=4 * T) == "the track errors overlap the lossy value rows"
    assert measure(worst=RAW_VALUES + 16) == "the worst record overlap the raw value rows"
    assert measure(worst=LOSSY_VALUES) == "the worst record overlap the lossy value rows"
    assert measure(track_errors=ERRORS + 8 * COUNT - 4, track_error_stride_bytes=4 * T) == "the track error records overlap the track errors"
    assert measure(worst=ERRORS + 8 * COUNT - 16) == "the track error records overlap the worst record"
    assert measure(track_errors=TRACK_ERRORS, track_error_stride_bytes=4 * T + 8, worst=TRACK_ERRORS + (4 * T + 8) * COUNT - 16) == "the track errors overlap the worst record"
    # ranges that touch do not overlap; with no instances only the worst record is written
    assert measure(errors=raw_end, track_errors=raw_end + 8 * COUNT, track_error_stride_bytes=4 * T, worst=RAW_VALUES - 16) == "null context"
    assert measure(errors=RAW_VALUES, count=0) == "null context"
    assert measure(worst=RAW_VALUES, count=0) == "null context"
