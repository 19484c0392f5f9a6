"""aclhip_compress_tracks_metric_batch, aclhip_compress_tracks_variable_metric_batch and aclhip_find_bit_rates_metric_batch without a
device: the surface (header, library, binding), the prototypes against a C99 translation unit, an unknown metric with its message, and
EVERY refusal of the three base calls through the _metric fronts with the base call's message. The last is not restated here: the
argument tests of the base calls (tests/test_compress_tracks_arguments.py, tests/test_variable_compress_arguments.py,
tests/test_bit_rate_search_arguments.py) run again, case for case with the messages they assert, over a library whose three base entry
points are the _metric fronts at a known metric. Every case is decided before any device call and works without a context. Fails on a
library without the calls."""
import ctypes
import os
import re
import subprocess

import pytest

from acl_amd import runtime
import test_bit_rate_search_arguments as search_arguments
import test_compress_tracks_arguments as tracks_arguments
import test_variable_compress_arguments as variable_arguments

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID = 1
FRONTS = {"aclhip_compress_tracks_batch": "aclhip_compress_tracks_metric_batch", "aclhip_compress_tracks_variable_batch": "aclhip_compress_tracks_variable_metric_batch",
          "aclhip_find_bit_rates_batch": "aclhip_find_bit_rates_metric_batch"}
UNKNOWN = (2, 255, 0xFFFFFFFF)


class ThroughTheMetricFronts:
    """the library with its three base entry points replaced by the _metric fronts at `metric`: (arguments..., stream) becomes
    (arguments..., metric, stream)"""
    def __init__(self, metric):
        self.lib, self.metric = runtime.load_library(), metric

    def __getattr__(self, name):
        if name not in FRONTS:
            return getattr(self.lib, name)
        front = getattr(self.lib, FRONTS[name])
        return lambda *arguments: front(*arguments[:-1], self.metric, arguments[-1])


def test_header_declares_library_exports_and_binding_binds_the_entry_points():
    header = open(os.path.join(ROOT, "include", "aclhip.h")).read()
    declared = set(re.findall(r"\b(aclhip_[a-z_0-9]+)\s*\(", re.sub(r"/\*.*?\*/", "", header, flags=re.S)))
    lib = runtime.load_library()
    for name in FRONTS.values():
        assert name in declared and hasattr(lib, name) and name in runtime.EXPORTED_SYMBOLS, name
        assert hasattr(runtime.Context, name[len("aclhip_"):])
    assert lib.aclhip_abi_version() == runtime.ABI_VERSION == 6       # (added without a bump: no existing struct changed)
    assert runtime.ERROR_METRIC_QVVF == 0 and runtime.ERROR_METRIC_QVVF_MATRIX3X4F == 1
    # the keyword is there, and its default is the call as it was
    import inspect
    for function in (runtime.compress_tracks, runtime.compress_tracks_variable, runtime.find_bit_rates, runtime.compress_tracks_at_precision):
        assert inspect.signature(function).parameters["metric"].default == runtime.ERROR_METRIC_QVVF
    # the "Left out" lists of the family no longer name the metric; the rest stays
    comments = " ".join(" ".join(comment.replace("*", " ").split()) for comment in re.findall(r"/\*.*?\*/", header, flags=re.S))
    left_out = re.findall(r"Left out[^.]*\.", comments)
    assert not any(re.search(r"(?<!\()the matrix error metric(?!:)", text) for text in left_out), [text for text in left_out if "matrix" in text]
    assert sum("additive bases" in text for text in left_out) >= 3 and any("the levels high and highest" in text for text in left_out)
    assert "ACLHIP_METRIC_QVVF_MATRIX3X4F follows the reference's CODE" in header


def test_the_prototypes_match_a_c99_translation_unit(tmp_path):
    lib_dir = os.path.dirname(runtime.library_path())
    binary = tmp_path / "compress_metric_abi"
    source = os.path.join(ROOT, "tests", "c", "compress_metric_abi.c")
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-I", os.path.join(ROOT, "include"), source, "-L" + lib_dir, "-laclhip",
                    "-Wl,-rpath," + lib_dir, "-o", str(binary)], check=True)
    done = subprocess.run([str(binary)], stdout=subprocess.PIPE, text=True, timeout=120)
    assert done.returncode == 0, done.returncode        # (the program's own checks: both metrics reach the missing context, a third is refused)


def call(name, metric, **fields):
    """one call of a _metric front with arguments that pass every check but what `fields` changes; no context: (status, message)"""
    lib = runtime.load_library()
    raws, blobs, results, workspace, rates = 0x10000, 0x100000, 0x20000, 0x800000, 0x60000
    if name == "aclhip_compress_tracks_metric_batch":
        desc = runtime.CompressTracksDesc()
        desc.rotation_format = 2
    elif name == "aclhip_compress_tracks_variable_metric_batch":
        desc = runtime.CompressVariableDesc()
        desc.max_samples, desc.rotation_bit_rate, desc.translation_bit_rate, desc.scale_bit_rate = 100, 16, 16, 16
    else:
        desc = runtime.FindBitRatesDesc()
        desc.max_samples, desc.level = 100, 2
    desc.precision, desc.shell_distance, desc.max_tracks, desc.workspace = 1.0e-4, 1.0, 100, workspace
    for field, value in fields.items():
        setattr(desc, field, value)
    if name == "aclhip_find_bit_rates_metric_batch":
        status = getattr(lib, name)(None, raws, 16, ctypes.byref(desc), rates, 2400, 400, results, metric, None)
    else:
        status = getattr(lib, name)(None, raws, 16, ctypes.byref(desc), blobs, 4096, results, metric, None)
    return status, lib.aclhip_last_error_message(None).decode()


@pytest.mark.parametrize("name", sorted(FRONTS.values()))
def test_an_unknown_metric_is_refused_with_its_message(name):
    for metric in (runtime.ERROR_METRIC_QVVF, runtime.ERROR_METRIC_QVVF_MATRIX3X4F):
        assert call(name, metric) == (INVALID, "null context")          # (what passes every check ends at the missing context)
    for metric in UNKNOWN:
        assert call(name, metric) == (INVALID, "unknown error metric %u" % metric)
        # in front of every other check: a desc with nothing right in it is not looked at
        assert call(name, metric, max_tracks=0, workspace=None, flags=0x80000000) == (INVALID, "unknown error metric %u" % metric)


def test_the_raw_format_takes_either_metric():
    """rotation_format == 0 uses no metric: a known one passes, its own refusals are the base call's, an unknown one is still refused"""
    for metric in (runtime.ERROR_METRIC_QVVF, runtime.ERROR_METRIC_QVVF_MATRIX3X4F):
        assert call("aclhip_compress_tracks_metric_batch", metric, rotation_format=0) == (INVALID, "null context")
        assert call("aclhip_compress_tracks_metric_batch", metric, rotation_format=0, scale_format=3) == (INVALID, "a scale format of 3: 0 (vector3f_full)")
    assert call("aclhip_compress_tracks_metric_batch", 2, rotation_format=0) == (INVALID, "unknown error metric 2")


@pytest.mark.parametrize("metric", [runtime.ERROR_METRIC_QVVF, runtime.ERROR_METRIC_QVVF_MATRIX3X4F])
@pytest.mark.parametrize("module,cases", [
    (tracks_arguments, ("test_every_invalid_argument_has_its_message", "test_values_that_are_no_format_of_the_reference", "test_every_overlap_has_its_message")),
    (variable_arguments, ("test_every_invalid_argument_has_its_message", "test_every_overlap_of_the_rate_table_has_its_message")),
    (search_arguments, ("test_every_invalid_argument_has_its_message", "test_the_strides_of_a_written_table_keep_its_writers_apart",
                        "test_the_table_is_on_the_written_side_of_the_overlap_check"))], ids=["drop_w", "variable", "search"])
def test_every_refusal_of_the_base_call_comes_back_through_the_front(module, cases, metric, monkeypatch):
    """the base call's own argument tests, every case with the message it asserts, over the _metric front at a known metric"""
    through = ThroughTheMetricFronts(metric)
    calls = []

    def counting_library():
        calls.append(1)
        return through
    monkeypatch.setattr(module.runtime, "load_library", counting_library)
    for case in cases:
        getattr(module, case)()
    assert len(calls) > 20 * len(cases) // 2        # (the cases did go through the replaced library)
