"""The launch harness of the transform compressor family's GPU tests: the eleven C entry points as values, one launch for all of them and
the two comparisons -- rows of blobs, a table of bit rates -- that hold every byte. Not a test file: tests/test_compress_launches.py
shows without a device that the comparisons are not vacuous.

An entry point is a KIND (what is written: raw, tracks, variable: rows of blobs; search: a table of bit rates) and a FRONT (which
extra argument the C call takes: base none, metric and level the error metric, additive an aclhip_additive_base). The front is always
named by the test: "metric 0 through the _metric front is the base call's bytes" is a statement about a C entry point.

The output region of every launch is one flat buffer filled with a sentinel byte: a guard, the n rows (or the n instances of the table),
a guard; the shell metadata likewise; the results are prefilled, the workspace carries a sentinel tail. One comparison holds what the
restatement says was written to its bytes and EVERYTHING ELSE to the sentinel. The sample rate is a power of two, so that the key times
i / rate are exact."""
import collections

import numpy as np
import pytest

from acl_amd import runtime

RATE = 32.0
SENTINEL = 0xA5
GUARD = 256
RESULT_FILL = 0x5A5A5A5A
PRECISION, SHELL = 0.01, 3.0

# per kind: the Context method without its front and "_batch", the desc struct, the workspace size function and the row bound, all of acl_amd.runtime
Kind = collections.namedtuple("Kind", "stem desc size_function bound")
KINDS = {"raw": Kind("compress_raw_tracks", "TransformCompressDesc", "transform_compress_workspace_bytes", "transform_compress_bound"),
         "tracks": Kind("compress_tracks", "CompressTracksDesc", "compress_tracks_workspace_bytes", "transform_compress_bound"),
         "variable": Kind("compress_tracks_variable", "CompressVariableDesc", "compress_variable_workspace_bytes", "variable_compress_bound"),
         "search": Kind("find_bit_rates", "FindBitRatesDesc", "find_bit_rates_workspace_bytes", None)}
FRONTS = {"base": "", "metric": "_metric", "level": "_level", "additive": "_additive"}


class Entry:
    """one C entry point: `metric` goes with the fronts metric and level; `bases` (one handle for all instances, one per instance, or
    None: no handles at all) and `additive_format` with the front additive"""
    def __init__(self, kind, front="base", metric=0, bases=None, additive_format=0):
        assert front in FRONTS and (kind != "raw" or front == "base") and (front != "level" or kind == "search"), (kind, front)
        self.kind, self.front, self.metric, self.bases, self.additive_format = kind, front, metric, bases, additive_format
        self.method = KINDS[kind].stem + FRONTS[front] + "_batch"
        self.desc, self.bound = KINDS[kind].desc, KINDS[kind].bound
        self.size_function = "find_bit_rates_level_workspace_bytes" if kind == "search" and front in ("level", "additive") else KINDS[kind].size_function


ENTRIES = [(kind, front) for kind in KINDS for front in FRONTS if (kind != "raw" or front == "base") and (front != "level" or kind == "search")]


class Launched:
    """what one launch left, on the host: flat (guard, rows or table, guard), results uint32 [n, 2], metadata (guard, n * max_tracks
    shells of 8 bytes, guard), rejected (the count's delta), n, max_tracks and the strides (stride; or instance_stride, segment_stride)"""
    def __init__(self, **fields):
        self.__dict__.update(fields)


@pytest.fixture(scope="module")
def ctx():
    context = runtime.Context(0)
    yield context
    context.close()


class Registered:
    """arrays registered with one context, unregistered together"""
    def __init__(self, ctx):
        self.ctx, self.handles = ctx, []

    def add(self, samples, looping=runtime.LOOP_CLAMP):
        handle = self.ctx.register_raw_tracks(samples, RATE, looping)
        self.handles.append(handle)
        return handle

    def __enter__(self):
        return self

    def __exit__(self, *args):
        for handle in self.handles:
            self.ctx.unregister_raw_tracks(handle)


def launch(ctx, entry, handles, max_tracks, max_samples=None, stride=None, flags=0, precision=PRECISION, shell_distance=SHELL, default_pose=None, parents=None,
           track_precisions=None, track_shell_distances=None, rotation_format=runtime.ROTATION_QUATF_DROP_W_FULL, rates=None, level=2, instance_stride=None,
           segment_stride=None, with_metadata=True, graph=False):
    """One launch of `entry` over `handles`. Rows are `stride` bytes (None: the kind's bound of (max_tracks, max_samples)); the table of a
    search has the two strides (None: 4 max_tracks, and that by the segments of max_samples). rates (variable): three uniform rates, or a
    uint8 array whose last axes are [tracks, 4]: the strides default to its own shape ([tracks, 4]: 0 and 0; [segments, tracks, 4]:
    shared by the instances; [instances, segments, tracks, 4]). graph: the call is captured on a side stream and replayed once into
    outputs filled anew -- what the capture itself may have left does not count."""
    import torch
    device = torch.device("cuda:0")
    n = len(handles)
    inputs = []

    def upload(host):
        """what the call only reads: compared with the host's bytes behind the launch"""
        host = np.ascontiguousarray(host)
        d_input = torch.from_numpy(host.view(np.uint8).reshape(-1)).to(device)
        inputs.append((host, d_input))
        return d_input.data_ptr()

    desc = getattr(runtime, entry.desc)()
    by_samples = hasattr(desc, "max_samples")
    if entry.kind == "search":
        segment_stride = 4 * max_tracks if segment_stride is None else segment_stride
        instance_stride = runtime.variable_compress_num_segments(max_samples) * segment_stride if instance_stride is None else instance_stride
        strides = (instance_stride, segment_stride)
        out = Launched(instance_stride=instance_stride, segment_stride=segment_stride)
    else:
        if stride is None:
            stride = getattr(runtime, entry.bound)(max_tracks, max_samples, flags)
        strides = (stride,)
        out = Launched(stride=stride)
    outputs = [(torch.full((GUARD + n * strides[0] + GUARD,), SENTINEL, dtype=torch.uint8, device=device), SENTINEL),
               (torch.full((n, 2), RESULT_FILL, dtype=torch.int32, device=device), RESULT_FILL),
               (torch.full((GUARD + n * max_tracks * 8 + GUARD,), SENTINEL, dtype=torch.uint8, device=device), SENTINEL)]
    (flat, _), (d_results, _), (d_metadata, _) = outputs
    assert (flat.data_ptr() + GUARD) % 16 == 0
    workspace_bytes = getattr(runtime, entry.size_function)(n, max_tracks, *([max_samples] if by_samples else []))
    d_workspace = torch.full((workspace_bytes + GUARD,), SENTINEL, dtype=torch.uint8, device=device)
    d_handles = upload(np.asarray(handles, dtype=np.uint32))

    desc.flags, desc.max_tracks, desc.precision, desc.shell_distance, desc.workspace = flags, max_tracks, precision, shell_distance, d_workspace.data_ptr()
    if by_samples:
        desc.max_samples = max_samples
    if hasattr(desc, "rotation_format"):
        desc.rotation_format = rotation_format
    if hasattr(desc, "level"):
        desc.level = level
    if hasattr(desc, "shell_metadata") and with_metadata:
        desc.shell_metadata = d_metadata.data_ptr() + GUARD
    for field, table, dtype in (("default_pose", default_pose, np.float32), ("parent_indices", parents, np.uint32), ("track_precisions", track_precisions, np.float32),
                                ("track_shell_distances", track_shell_distances, np.float32)):
        if table is not None:
            host = np.ascontiguousarray(table, dtype=dtype)
            setattr(desc, field, upload(host))
            desc.num_table_tracks = host.shape[0]
    if entry.kind == "variable":
        rates = np.ascontiguousarray(rates, dtype=np.uint8)
        if rates.ndim == 1:
            desc.rotation_bit_rate, desc.translation_bit_rate, desc.scale_bit_rate = (int(rate) for rate in rates)
        else:
            desc.bit_rates = upload(rates)
            desc.bit_rate_segment_stride = (rates.shape[-2] * 4 if rates.ndim >= 3 else 0) if segment_stride is None else segment_stride
            desc.bit_rate_instance_stride = (rates.shape[-3] * rates.shape[-2] * 4 if rates.ndim == 4 else 0) if instance_stride is None else instance_stride
    extra = {"metric": entry.metric} if entry.front in ("metric", "level") else {}
    if entry.front == "additive":
        record = runtime.AdditiveBase()             # (the record and its handles: alive until the stream is synchronized)
        record.additive_format = entry.additive_format
        if entry.bases is not None:
            bases = np.atleast_1d(np.asarray(entry.bases, dtype=np.uint32))
            bases = np.repeat(bases, n) if len(bases) == 1 else bases
            assert len(bases) == n
            record.base_raws = upload(bases)
        extra = {"additive_base": record}

    def call(stream):
        getattr(ctx, entry.method)(d_handles, n, desc, flat.data_ptr() + GUARD, *strides, d_results.data_ptr(), stream=stream.cuda_stream, **extra)

    rejected_before = ctx.rejected_instance_count()
    if graph:
        stream = torch.cuda.Stream(device)
        with torch.cuda.stream(stream):
            captured = torch.cuda.CUDAGraph()
            with torch.cuda.graph(captured, stream=stream):
                call(stream)
            for d_output, fill in outputs:
                d_output.fill_(fill)
            captured.replay()
    else:
        stream = torch.cuda.current_stream(device)
        call(stream)
    stream.synchronize()
    out.flat, out.n, out.max_tracks = flat.cpu().numpy(), n, max_tracks
    out.results = d_results.cpu().numpy().view(np.uint32).reshape(n, 2)
    out.metadata = d_metadata.cpu().numpy()
    out.rejected = ctx.rejected_instance_count() - rejected_before
    assert np.all(d_workspace[workspace_bytes:].cpu().numpy() == SENTINEL)                      # the workspace is as large as it says
    for host, d_input in inputs:
        assert np.array_equal(d_input.cpu().numpy(), host.view(np.uint8).reshape(-1))             # the inputs are only read
    return out


def same(one, other):
    """two launches left the same bytes everywhere: rows or table with the guards, results, metadata, the count"""
    return (np.array_equal(one.flat, other.flat) and np.array_equal(one.results, other.results) and np.array_equal(one.metadata, other.metadata)
            and one.rejected == other.rejected)


def check_rows(out, expected):
    """expected: per instance a Compressed (blob and shells), a blob alone (uint8: the shell metadata is not looked at), or the status
    of an instance that writes nothing"""
    want = np.full(out.flat.shape, SENTINEL, dtype=np.uint8)
    want_metadata = np.full(out.metadata.shape, SENTINEL, dtype=np.uint8)
    want_results = np.zeros((out.n, 2), dtype=np.uint32)
    with_shells = True
    for i, item in enumerate(expected):
        if isinstance(item, int):
            want_results[i] = (item, 0)
            continue
        blob = item if isinstance(item, np.ndarray) else item.blob
        want[GUARD + i * out.stride: GUARD + i * out.stride + blob.size] = blob
        want_results[i] = (runtime.COMPRESS_OK, blob.size)
        if isinstance(item, np.ndarray):
            with_shells = False
        else:
            shells = np.ascontiguousarray(item.shells, dtype=np.float32).view(np.uint8).reshape(-1)
            at = GUARD + i * out.max_tracks * 8
            want_metadata[at: at + shells.size] = shells
    assert np.array_equal(out.results, want_results), (out.results[:8], want_results[:8])
    different = np.flatnonzero(out.flat != want)
    assert different.size == 0, [(int(at - GUARD) // out.stride, int(at - GUARD) % out.stride, int(out.flat[at]), int(want[at])) for at in different[:8]]
    if with_shells:
        different = np.flatnonzero(out.metadata != want_metadata)
        assert different.size == 0, [(int(at - GUARD) // (out.max_tracks * 8), int(at - GUARD) % (out.max_tracks * 8) // 8, int(out.metadata[at]), int(want_metadata[at])) for at in different[:8]]
    assert out.rejected == sum(1 for item in expected if isinstance(item, int) and item == runtime.COMPRESS_REFUSED)


def check_table(launched, expected, levels=False):
    """expected: per instance a Search of the restatement, or the status of an instance that writes nothing. levels: the second word of
    a served instance's result is the level that was searched (the fronts level and additive); else it is 0"""
    want = np.full(launched.flat.shape, SENTINEL, dtype=np.uint8)
    metadata = np.full(launched.metadata.shape, SENTINEL, dtype=np.uint8)
    want_results = np.zeros((launched.n, 2), dtype=np.uint32)
    for i, found in enumerate(expected):
        if isinstance(found, int):
            want_results[i] = (found, 0)
            continue
        want_results[i] = (runtime.COMPRESS_OK, found.level if levels else 0)
        for g in range(found.table.shape[0]):
            at = GUARD + i * launched.instance_stride + g * launched.segment_stride
            want[at: at + 4 * found.table.shape[1]] = found.table[g].reshape(-1)
        at = GUARD + i * launched.max_tracks * 8
        metadata[at: at + 8 * found.base.shells.shape[0]] = found.base.shells.view(np.uint8).reshape(-1)
    different = np.flatnonzero(launched.flat != want)
    assert different.size == 0, (different.size, [(int(d - GUARD) // launched.instance_stride, int(d - GUARD) % launched.instance_stride // launched.segment_stride,
                                                   int(d - GUARD) % launched.segment_stride // 4, int(d - GUARD) % 4, int(launched.flat[d]), int(want[d])) for d in different[:12]])
    assert np.array_equal(launched.results, want_results), (launched.results[:8], want_results[:8])
    assert launched.rejected == sum(1 for found in expected if isinstance(found, int) and found == runtime.COMPRESS_REFUSED)
    if all(not isinstance(found, int) for found in expected):
        assert np.array_equal(launched.metadata, metadata)
