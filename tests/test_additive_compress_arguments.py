"""aclhip_compress_tracks_additive_batch, aclhip_compress_tracks_variable_additive_batch and aclhip_find_bit_rates_additive_batch without
a device: the surface (header, library, binding), the prototypes against a C99 translation unit, every argument error of the
aclhip_additive_base with its message, and EVERY refusal of the three base calls through the _additive fronts at ACLHIP_ADDITIVE_NONE
with the base call's message. The last is not restated here: the argument tests of the base calls
(tests/test_compress_tracks_arguments.py, tests/test_variable_compress_arguments.py, tests/test_bit_rate_search_levels_arguments.py)
run again, case for case with the messages they assert, over a library whose three base entry points are the _additive fronts. Every
case is decided before any device call and works without a context. Fails on a library without the calls."""
import ctypes
import inspect
import os
import re
import subprocess

import pytest

from acl_amd import runtime
import test_bit_rate_search_levels_arguments as level_arguments
import test_compress_tracks_arguments as tracks_arguments
import test_variable_compress_arguments as variable_arguments

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID = 1
FRONTS = {"aclhip_compress_tracks_batch": "aclhip_compress_tracks_additive_batch", "aclhip_compress_tracks_variable_batch": "aclhip_compress_tracks_variable_additive_batch",
          "aclhip_find_bit_rates_level_batch": "aclhip_find_bit_rates_additive_batch"}
RAWS, BLOBS, RESULTS, WORKSPACE, RATES, BASES = 0x10000, 0x100000, 0x20000, 0x800000, 0x60000, 0x40000
COUNT, MAX_TRACKS, MAX_SAMPLES = 16, 100, 100


def record_of(additive_format=runtime.ADDITIVE_NONE, base_raws=None, **fields):
    record = runtime.AdditiveBase()
    record.additive_format, record.base_raws = additive_format, base_raws
    for field, value in fields.items():
        setattr(record, field, value)
    return record


class ThroughTheAdditiveFronts:
    """the library with its three base entry points replaced by the _additive fronts at ACLHIP_ADDITIVE_NONE: (arguments..., stream)
    becomes (arguments..., &base, stream); the level search hands its metric over first -- the fronts take none, so any metric but
    ACLHIP_METRIC_QVVF stays with the call it was made to"""
    def __init__(self, base_raws):
        self.lib, self.record = runtime.load_library(), record_of(base_raws=base_raws)

    def __getattr__(self, name):
        if name not in FRONTS:
            return getattr(self.lib, name)
        front = getattr(self.lib, FRONTS[name])
        if name == "aclhip_find_bit_rates_level_batch":
            original = getattr(self.lib, name)
            return lambda *arguments: front(*arguments[:-2], ctypes.byref(self.record), arguments[-1]) if arguments[-2] == 0 else original(*arguments)
        return lambda *arguments: front(*arguments[:-1], ctypes.byref(self.record), arguments[-1])


def test_header_declares_library_exports_and_binding_binds_the_entry_points():
    header = open(os.path.join(ROOT, "include", "aclhip.h")).read()
    declared = set(re.findall(r"\b(aclhip_[a-z_0-9]+)\s*\(", re.sub(r"/\*.*?\*/", "", header, flags=re.S)))
    lib = runtime.load_library()
    for name in FRONTS.values():
        assert name in declared and hasattr(lib, name) and name in runtime.EXPORTED_SYMBOLS, name
        assert hasattr(runtime.Context, name[len("aclhip_"):])
    assert lib.aclhip_abi_version() == runtime.ABI_VERSION == 6       # (added without a bump: no existing struct changed)
    assert ctypes.sizeof(runtime.AdditiveBase) == 32 and runtime.AdditiveBase.additive_format.offset == 8 and runtime.AdditiveBase.reserved.offset == 16
    assert "} aclhip_additive_base;" in header
    # the keywords are there, and their defaults are the calls as they were
    for function in (runtime.compress_tracks, runtime.compress_tracks_variable, runtime.find_bit_rates):
        parameters = inspect.signature(function).parameters
        assert parameters["additive_base"].default is None and parameters["additive_format"].default == runtime.ADDITIVE_NONE
    # the "Left out" lists of the family point here
    comments = " ".join(" ".join(comment.replace("*", " ").split()) for comment in re.findall(r"/\*.*?\*/", header, flags=re.S))
    left_out = re.findall(r"Left out[^.]*\.", comments)
    assert sum("additive bases" in text and "_additive_batch, below" in text for text in left_out) >= 4, [text for text in left_out if "additive" in text]
    assert any("a base under quatf_full" in text for text in left_out)


def test_the_prototypes_match_a_c99_translation_unit(tmp_path):
    lib_dir = os.path.dirname(runtime.library_path())
    binary = tmp_path / "compress_additive_abi"
    source = os.path.join(ROOT, "tests", "c", "compress_additive_abi.c")
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-I", os.path.join(ROOT, "include"), source, "-L" + lib_dir, "-laclhip",
                    "-Wl,-rpath," + lib_dir, "-o", str(binary)], check=True)
    done = subprocess.run([str(binary)], stdout=subprocess.PIPE, text=True, timeout=120)
    assert done.returncode == 0, done.returncode        # (the program's own checks: the struct's layout, two refusals, the missing context)
    assert done.stdout.split() == ["32", "16"]
    assert "aclhip_find_bit_rates_additive_batch(gpu, d_raws, num_instances, &search, d_bit_rates, instance_stride, segment_stride, d_results, &base, hip_stream)" in open(source).read()
    assert "aclhip_find_bit_rates_additive_batch(gpu, d_raws, num_instances, &search," in open(os.path.join(ROOT, "INTEGRATION.md")).read()


def call(name, record, results=RESULTS, blobs=BLOBS, rates=RATES, **fields):
    """one call of an _additive front with arguments that pass every check but what `record` and `fields` change; no context: the message"""
    lib = runtime.load_library()
    if name == "aclhip_compress_tracks_additive_batch":
        desc = runtime.CompressTracksDesc()
        desc.rotation_format = 2
    elif name == "aclhip_compress_tracks_variable_additive_batch":
        desc = runtime.CompressVariableDesc()
        desc.max_samples, desc.rotation_bit_rate, desc.translation_bit_rate, desc.scale_bit_rate = MAX_SAMPLES, 16, 16, 16
    else:
        desc = runtime.FindBitRatesDesc()
        desc.max_samples, desc.level = MAX_SAMPLES, 4
    desc.precision, desc.shell_distance, desc.max_tracks, desc.workspace = 1.0e-4, 1.0, MAX_TRACKS, WORKSPACE
    for field, value in fields.items():
        setattr(desc, field, value)
    base = ctypes.byref(record) if record is not None else None
    if name == "aclhip_find_bit_rates_additive_batch":
        status = getattr(lib, name)(None, RAWS, COUNT, ctypes.byref(desc), rates, 2800, 400, results, base, None)
    else:
        status = getattr(lib, name)(None, RAWS, COUNT, ctypes.byref(desc), blobs, 4096, results, base, None)
    assert status == INVALID
    return lib.aclhip_last_error_message(None).decode()


@pytest.mark.parametrize("name", sorted(FRONTS.values()))
def test_every_argument_error_of_the_additive_base_has_its_message(name):
    for additive_format in (runtime.ADDITIVE_RELATIVE, runtime.ADDITIVE_ADDITIVE0, runtime.ADDITIVE_ADDITIVE1):
        assert call(name, record_of(additive_format, BASES)) == "null context"          # (what passes every check ends at the missing context)
    for base_raws in (None, BASES, 3):
        assert call(name, record_of(runtime.ADDITIVE_NONE, base_raws)) == "null context"                # NONE: whatever base_raws is
    assert call(name, None) == "null additive base"
    assert call(name, None, max_tracks=0, workspace=None, flags=0x80000000) == "null additive base"        # in front of every other check
    for additive_format in (4, 255, 0xFFFFFFFF):
        assert call(name, record_of(additive_format, BASES)) == "unknown additive format %u" % additive_format
    for fields in ({"reserved_word": 1}, {"reserved": (ctypes.c_uint64 * 2)(0, 1)}, {"reserved": (ctypes.c_uint64 * 2)(1 << 63, 0)}):
        assert call(name, record_of(runtime.ADDITIVE_ADDITIVE0, BASES, **fields)) == "reserved fields of the additive base are not 0"
        assert call(name, record_of(runtime.ADDITIVE_NONE, None, **fields)) == "reserved fields of the additive base are not 0"
    for additive_format in (runtime.ADDITIVE_RELATIVE, runtime.ADDITIVE_ADDITIVE0, runtime.ADDITIVE_ADDITIVE1):
        assert call(name, record_of(additive_format, None)) == "additive format %u without base_raws" % additive_format
        assert call(name, record_of(additive_format, BASES + 2)) == "base_raws must be 4 byte aligned"


@pytest.mark.parametrize("name", sorted(FRONTS.values()))
def test_the_base_handles_overlap_nothing_that_is_written(name):
    with_rows = name != "aclhip_find_bit_rates_additive_batch"
    size = {"aclhip_compress_tracks_additive_batch": runtime.compress_tracks_workspace_bytes(COUNT, MAX_TRACKS),
            "aclhip_compress_tracks_variable_additive_batch": runtime.compress_variable_workspace_bytes(COUNT, MAX_TRACKS, MAX_SAMPLES),
            "aclhip_find_bit_rates_additive_batch": runtime.find_bit_rates_level_workspace_bytes(COUNT, MAX_TRACKS, MAX_SAMPLES)}[name]
    metadata = 0x2000000
    written = [("the compress results", RESULTS, COUNT * 8), ("the workspace", WORKSPACE, size), ("the shell metadata", metadata, COUNT * MAX_TRACKS * 8)]
    written.append(("the blob rows", BLOBS, COUNT * 4096) if with_rows else ("the bit rate table", RATES, (COUNT - 1) * 2800 + 5 * 400 + 4 * MAX_TRACKS))
    for what, start, extent in written:
        for base_raws in (start + extent - 4, start - COUNT * 4 + 4):
            assert call(name, record_of(runtime.ADDITIVE_RELATIVE, base_raws), shell_metadata=metadata) == "%s overlap the additive base handles" % what
        assert call(name, record_of(runtime.ADDITIVE_RELATIVE, start + extent), shell_metadata=metadata) == "null context"
        # NONE reads no handles: nothing can overlap
        assert call(name, record_of(runtime.ADDITIVE_NONE, start), shell_metadata=metadata) == "null context"


def test_the_raw_rotation_format_takes_no_base():
    name = "aclhip_compress_tracks_additive_batch"
    for additive_format in (runtime.ADDITIVE_RELATIVE, runtime.ADDITIVE_ADDITIVE0, runtime.ADDITIVE_ADDITIVE1):
        assert call(name, record_of(additive_format, BASES), rotation_format=0) == "rotation format quatf_full takes no additive base: the raw settings decide nothing by a metric"
    assert call(name, record_of(runtime.ADDITIVE_NONE, None), rotation_format=0) == "null context"
    assert call(name, record_of(runtime.ADDITIVE_NONE, None), rotation_format=0, scale_format=3) == "a scale format of 3: 0 (vector3f_full)"


@pytest.mark.parametrize("base_raws", [None, BASES], ids=["no_handles", "handles"])
@pytest.mark.parametrize("module,cases", [
    (tracks_arguments, ("test_every_invalid_argument_has_its_message", "test_values_that_are_no_format_of_the_reference", "test_every_overlap_has_its_message")),
    (variable_arguments, ("test_every_invalid_argument_has_its_message", "test_every_overlap_of_the_rate_table_has_its_message")),
    (level_arguments, ("test_the_levels_it_takes_and_the_message_for_any_other", "test_every_shared_refusal_under_this_calls_word",
                       "test_the_table_is_on_the_written_side_of_the_overlap_check_and_the_workspace_is_this_calls"))], ids=["drop_w", "variable", "search"])
def test_every_refusal_of_the_base_call_comes_back_through_the_front_at_none(module, cases, base_raws, monkeypatch):
    """the base call's own argument tests, every case with the message it asserts, over the _additive front at ACLHIP_ADDITIVE_NONE"""
    through = ThroughTheAdditiveFronts(base_raws)
    calls = []

    def counting_library():
        calls.append(1)
        return through
    monkeypatch.setattr(module.runtime, "load_library", counting_library)
    for case in cases:
        getattr(module, case)()
    assert len(calls) > 20 * len(cases) // 2        # (the cases did go through the replaced library)
