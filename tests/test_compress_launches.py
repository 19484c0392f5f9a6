"""tests/compress_launches.py and runtime.transform_compress_route without a device. The two comparisons of the harness are not vacuous:
a Launched built by hand passes, and each single byte or word that is changed in it raises. An Entry resolves to the Context method,
the desc struct and the workspace size function of its kind and front, for all eleven entry points (1 raw, 3 x 3, 1 level). The route of acl_amd.runtime picks,
for every combination of call, metric, level, bases and additive format, the method, the extra argument, the workspace size function
and with_levels that its docstring states; a stub context records what it is asked for."""
import collections
import copy
import ctypes

import numpy as np
import pytest

from acl_amd import runtime
from compress_launches import ENTRIES, GUARD, SENTINEL, Entry, Launched, check_rows, check_table

OK, NOT_FINITE, REFUSED = runtime.COMPRESS_OK, runtime.COMPRESS_NOT_FINITE, runtime.COMPRESS_REFUSED
Compressed = collections.namedtuple("Compressed", "blob shells")
Search = collections.namedtuple("Search", "table level base")
STRIDE, MAX_TRACKS = 64, 3
BLOBS = [np.arange(1, 21, dtype=np.uint8), np.arange(100, 133, dtype=np.uint8)]
SHELLS = np.array([[1.0, 0.01], [2.5, 0.01], [4.0, 0.02]], dtype=np.float32)
ROWS = [Compressed(BLOBS[0], SHELLS), Compressed(BLOBS[1], np.zeros((0, 2), dtype=np.float32))]
SEGMENT_STRIDE, INSTANCE_STRIDE = 4 * MAX_TRACKS + 4, 2 * (4 * MAX_TRACKS + 4) + 8           # both larger than the minimum
TABLES = [Search(np.arange(24, dtype=np.uint8).reshape(2, 3, 4), 4, Compressed(None, SHELLS)),
          Search(np.arange(50, 62, dtype=np.uint8).reshape(1, 3, 4), 3, Compressed(None, SHELLS[:2]))]          # one segment: the second row stays


def rows(second_refused=False):
    """two instances, rows of 64 bytes, blobs of 20 and 33 bytes, shells of the first"""
    flat = np.full(GUARD + 2 * STRIDE + GUARD, SENTINEL, dtype=np.uint8)
    metadata = np.full(GUARD + 2 * MAX_TRACKS * 8 + GUARD, SENTINEL, dtype=np.uint8)
    flat[GUARD: GUARD + 20] = BLOBS[0]
    metadata[GUARD: GUARD + 24] = SHELLS.view(np.uint8).reshape(-1)
    results = np.array([[OK, 20], [REFUSED, 0] if second_refused else [OK, 33]], dtype=np.uint32)
    if not second_refused:
        flat[GUARD + STRIDE: GUARD + STRIDE + 33] = BLOBS[1]
    return Launched(flat=flat, metadata=metadata, results=results, rejected=int(second_refused), n=2, stride=STRIDE, max_tracks=MAX_TRACKS)


def table():
    """two instances of two and of one segment, three tracks, strides with room between rows and between instances"""
    flat = np.full(GUARD + 2 * INSTANCE_STRIDE + GUARD, SENTINEL, dtype=np.uint8)
    metadata = np.full(GUARD + 2 * MAX_TRACKS * 8 + GUARD, SENTINEL, dtype=np.uint8)
    for i, found in enumerate(TABLES):
        for g in range(found.table.shape[0]):
            at = GUARD + i * INSTANCE_STRIDE + g * SEGMENT_STRIDE
            flat[at: at + 12] = found.table[g].reshape(-1)
        shells = found.base.shells.view(np.uint8).reshape(-1)
        metadata[GUARD + i * MAX_TRACKS * 8: GUARD + i * MAX_TRACKS * 8 + shells.size] = shells
    results = np.array([[OK, 4], [OK, 3]], dtype=np.uint32)
    return Launched(flat=flat, metadata=metadata, results=results, rejected=0, n=2, instance_stride=INSTANCE_STRIDE, segment_stride=SEGMENT_STRIDE, max_tracks=MAX_TRACKS)


def changed(launched, field, at=None, value=None):
    other = copy.deepcopy(launched)
    if field == "rejected":
        other.rejected += 1
    elif value is None:
        getattr(other, field)[at] ^= 0xFF
    else:
        getattr(other, field)[at] = value
    return other


def test_the_launched_objects_as_built_pass():
    check_rows(rows(), ROWS)
    check_rows(rows(), BLOBS)                                       # bare blobs: the same rows
    check_rows(rows(second_refused=True), [ROWS[0], REFUSED])
    check_table(table(), TABLES, levels=True)
    without_levels = table()
    without_levels.results[:, 1] = 0
    check_table(without_levels, TABLES)
    check_rows(changed(rows(), "metadata", GUARD + 5), BLOBS)       # and with bare blobs the metadata is not looked at


@pytest.mark.parametrize("field,at,value", [
    ("flat", 3, None), ("flat", GUARD + 2 * STRIDE + GUARD - 5, None), ("flat", GUARD + 20, None), ("results", (0, 1), 21), ("results", (1, 0), NOT_FINITE),
    ("metadata", GUARD + 5, None), ("metadata", 2, None), ("metadata", GUARD + 2 * MAX_TRACKS * 8 + 1, None), ("rejected", None, None)],
    ids=["leading_guard", "trailing_guard", "behind_a_blobs_size", "size_word", "status", "inside_the_shells", "metadata_leading_guard", "metadata_trailing_guard", "rejected_count"])
def test_one_change_to_the_rows_raises(field, at, value):
    with pytest.raises(AssertionError):
        check_rows(changed(rows(), field, at, value), ROWS)


def test_one_byte_in_a_refused_instances_row_raises():
    with pytest.raises(AssertionError):
        check_rows(changed(rows(second_refused=True), "flat", GUARD + STRIDE + 7), [ROWS[0], REFUSED])
    with pytest.raises(AssertionError):                              # and a refusal that was not counted
        check_rows(changed(rows(second_refused=True), "rejected", None, None), [ROWS[0], REFUSED])


@pytest.mark.parametrize("field,at,value", [
    ("flat", GUARD + 4 * MAX_TRACKS + 1, None), ("flat", GUARD + INSTANCE_STRIDE - 3, None), ("flat", GUARD + INSTANCE_STRIDE + SEGMENT_STRIDE + 1, None),
    ("results", (0, 1), 3), ("results", (1, 0), REFUSED), ("metadata", GUARD + MAX_TRACKS * 8 + 17, None), ("rejected", None, None)],
    ids=["between_the_rows", "between_the_instances", "a_segment_the_table_does_not_have", "level_word", "status", "a_shell_the_array_does_not_have", "rejected_count"])
def test_one_change_to_the_table_raises(field, at, value):
    with pytest.raises(AssertionError):
        check_table(changed(table(), field, at, value), TABLES, levels=True)


def test_the_checkers_leave_what_they_check():
    launched = table()
    before = copy.deepcopy(launched)
    check_table(launched, TABLES, levels=True)
    assert all(np.array_equal(getattr(launched, field), getattr(before, field)) for field in ("flat", "results", "metadata"))
    with pytest.raises(AssertionError):                              # without the option a level word is a wrong size word
        check_table(launched, TABLES)


METHODS = {
    ("raw", "base"): ("compress_raw_tracks_batch", "TransformCompressDesc", "transform_compress_workspace_bytes", "transform_compress_bound"),
    ("tracks", "base"): ("compress_tracks_batch", "CompressTracksDesc", "compress_tracks_workspace_bytes", "transform_compress_bound"),
    ("tracks", "metric"): ("compress_tracks_metric_batch", "CompressTracksDesc", "compress_tracks_workspace_bytes", "transform_compress_bound"),
    ("tracks", "additive"): ("compress_tracks_additive_batch", "CompressTracksDesc", "compress_tracks_workspace_bytes", "transform_compress_bound"),
    ("variable", "base"): ("compress_tracks_variable_batch", "CompressVariableDesc", "compress_variable_workspace_bytes", "variable_compress_bound"),
    ("variable", "metric"): ("compress_tracks_variable_metric_batch", "CompressVariableDesc", "compress_variable_workspace_bytes", "variable_compress_bound"),
    ("variable", "additive"): ("compress_tracks_variable_additive_batch", "CompressVariableDesc", "compress_variable_workspace_bytes", "variable_compress_bound"),
    ("search", "base"): ("find_bit_rates_batch", "FindBitRatesDesc", "find_bit_rates_workspace_bytes", None),
    ("search", "metric"): ("find_bit_rates_metric_batch", "FindBitRatesDesc", "find_bit_rates_workspace_bytes", None),
    ("search", "level"): ("find_bit_rates_level_batch", "FindBitRatesDesc", "find_bit_rates_level_workspace_bytes", None),
    ("search", "additive"): ("find_bit_rates_additive_batch", "FindBitRatesDesc", "find_bit_rates_level_workspace_bytes", None),
}


def test_every_entry_resolves_to_its_method_desc_and_size_function():
    assert sorted(ENTRIES) == sorted(METHODS) and len(ENTRIES) == 1 + 3 * 3 + 1
    for (kind, front), (method, desc, size_function, bound) in METHODS.items():
        entry = Entry(kind, front)
        assert (entry.method, entry.desc, entry.size_function, entry.bound) == (method, desc, size_function, bound), (kind, front)
        assert callable(getattr(runtime.Context, method)) and callable(getattr(runtime, size_function)) and issubclass(getattr(runtime, desc), ctypes.Structure)
        assert "aclhip_" + method in runtime.EXPORTED_SYMBOLS
    for kind, front in (("raw", "metric"), ("raw", "additive"), ("tracks", "level"), ("variable", "level"), ("search", "other")):
        with pytest.raises(AssertionError):
            Entry(kind, front)


class RecordingContext:
    """a context whose every _batch method records its name and keywords"""
    device_index = 0

    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        if not name.endswith("_batch"):
            raise AttributeError(name)
        return lambda *arguments, **keywords: self.calls.append((name, arguments, keywords))


ROUTES = {"tracks": ("compress_tracks", runtime.compress_tracks_workspace_bytes), "variable": ("compress_tracks_variable", runtime.compress_variable_workspace_bytes),
          "search": ("find_bit_rates", runtime.find_bit_rates_workspace_bytes)}
HANDLES = np.array([11, 12, 13], dtype=np.uint32)


@pytest.mark.parametrize("call", sorted(ROUTES))
def test_the_route_of_every_combination(call):
    stem, size_function = ROUTES[call]
    walked = 0
    for metric in (runtime.ERROR_METRIC_QVVF, runtime.ERROR_METRIC_QVVF_MATRIX3X4F):
        for level in (0, 1, 2, 3, 4, runtime.LEVEL_AUTOMATIC, "medium", "highest", "automatic"):
            for bases in (None, 7, [7], [7, 8, 9]):
                for additive_format in (runtime.ADDITIVE_NONE, runtime.ADDITIVE_ADDITIVE0):
                    context = RecordingContext()
                    settings = dict(metric=metric, level=level, additive_base=bases, additive_format=additive_format, device="cpu")
                    with_base = bases is not None or additive_format != runtime.ADDITIVE_NONE
                    if with_base and metric != runtime.ERROR_METRIC_QVVF:
                        with pytest.raises(ValueError, match="an additive base goes with the qvvf error metric: the reference has no additive matrix metric"):
                            runtime.transform_compress_route(context, call, HANDLES, **settings)
                        continue
                    launch, workspace_bytes, with_levels, alive = runtime.transform_compress_route(context, call, HANDLES, **settings)
                    launch(1, 2, 3, stream=5)
                    (name, arguments, keywords), = context.calls
                    assert arguments == (1, 2, 3) and keywords.pop("stream") == 5
                    above_medium = call == "search" and runtime.COMPRESSION_LEVELS.get(level, level) > 2
                    if with_base:
                        record = keywords.pop("additive_base")
                        assert name == stem + "_additive_batch" and isinstance(record, runtime.AdditiveBase) and record.additive_format == additive_format
                        assert alive[0] is record
                        if bases is None:
                            assert record.base_raws is None and alive[1] is None
                        else:
                            assert record.base_raws == alive[1].data_ptr()
                            assert alive[1].numpy().view(np.uint32).tolist() == ([7, 8, 9] if isinstance(bases, list) and len(bases) == 3 else [7, 7, 7])
                    elif above_medium:
                        assert name == "find_bit_rates_level_batch" and keywords.pop("metric") == metric
                    elif metric == runtime.ERROR_METRIC_QVVF:
                        assert name == stem + "_batch"
                    else:
                        assert name == stem + "_metric_batch" and keywords.pop("metric") == metric
                    assert keywords == {} and (with_base or alive is None)
                    assert with_levels == (call == "search" and (with_base or above_medium))
                    assert workspace_bytes is (runtime.find_bit_rates_level_workspace_bytes if with_levels else size_function)
                    walked += 1
    assert walked == 9 * (2 * 4 * 2 - 7)
    for count in (2, 4):
        with pytest.raises(ValueError, match="%d additive bases for 3 instances: one handle, or one per instance" % count):
            runtime.transform_compress_route(RecordingContext(), call, HANDLES, additive_base=list(range(1, count + 1)), additive_format=runtime.ADDITIVE_RELATIVE, device="cpu")
    with pytest.raises(KeyError):
        runtime.transform_compress_route(RecordingContext(), "raw", HANDLES)
