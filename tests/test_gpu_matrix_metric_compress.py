"""aclhip_compress_tracks_metric_batch, aclhip_compress_tracks_variable_metric_batch and aclhip_find_bit_rates_metric_batch through the C
ABI under ACLHIP_METRIC_QVVF_MATRIX3X4F: the expected tables, blobs, results and shells are the restatement's
(tests/matrix_metric_compress_restatement.py, which tests/test_matrix_metric_compress_oracle.py holds to the reference's compressor under
its matrix metric), and every comparison is on BYTES: both sides follow one definition, nothing has a tolerance.

The launches and the comparisons are the family's own (tests/compress_launches.py: a flat buffer of a sentinel byte between guards, one
comparison for every byte), at the three entries of the _metric front. The shapes are T in 1, 3, 5, 17 and S in 2 (the shortest scan), 31
(one segment), 33 (17 + 16) and 65 (four segments, three behind a vote); every (rotation, translation, scale) type triple; a chain of
17 whose scales are not uniform at any level -- the one place where two 3x4 matrices go down the chain and shear builds up --; the
clips of one track on which only the arithmetic decides the vote and the compaction. Metric 0 through the fronts is the base calls'
bytes. Needs a GPU. Fails on a library without the calls."""
import numpy as np
import pytest

from acl_amd import runtime
from oracle import bindings as ob
import compress_launches as launches
import matrix_metric_compress_restatement as metric_restatement
import variable_compress_restatement as restatement
from compress_launches import PRECISION, RATE, SENTINEL, SHELL, Entry, Registered, check_rows, check_table, ctx, same  # noqa: F401  (ctx: this module's fixture)
from matrix_metric_compress_restatement import METRIC_MATRIX, METRIC_QVVF
from variable_compress_restatement import ANIMATED, CONSTANT, DEFAULT, IDENTITY, LANES, OPTIMIZE_LOOPS

pytestmark = pytest.mark.gpu

TRACK_COUNTS, SAMPLE_COUNTS = (1, 3, 5, 17), (2, 31, 33, 65)
SHAPES = [(t, s) for t in TRACK_COUNTS for s in SAMPLE_COUNTS]
MAX_TRACKS, MAX_SAMPLES, MAX_SEGMENTS = 17, 65, 4
REFUSED, NOT_FINITE = runtime.COMPRESS_REFUSED, runtime.COMPRESS_NOT_FINITE


def find(samples, metric=METRIC_MATRIX, **settings):
    settings.setdefault("precision", PRECISION)
    settings.setdefault("shell_distance", SHELL)
    return metric_restatement.find_bit_rates(samples, RATE, metric, **settings)


def through(kind, metric=METRIC_MATRIX):
    """the _metric front of `kind` at `metric`"""
    return Entry(kind, "metric", metric)


def launch(ctx, entry, handles, **settings):
    settings.setdefault("max_tracks", MAX_TRACKS)
    settings.setdefault("max_samples", MAX_SAMPLES)
    return launches.launch(ctx, entry, handles, **settings)


def search(ctx, handles, metric=METRIC_MATRIX, **settings):
    return launch(ctx, through("search", metric), handles, **settings)


def scaled_chain(seed, num_samples, num_tracks):
    """every rotation and translation as mixed_clip makes them, every scale animated and not uniform, within 0.9 .. 1.1"""
    samples = restatement.mixed_clip(seed, num_samples, num_tracks, offset=18)
    samples[:, :, 8:11] = np.random.default_rng(40 + seed).uniform(0.9, 1.1, size=(num_samples, num_tracks, 3)).astype(np.float32)
    return samples


@pytest.fixture(scope="module")
def sweep(ctx):
    """every shape registered once, as the base search's sweep makes them: track b of array k has the (b + 9 k)-th of the 27 type triples,
    every seventh array no scale, about every second array of more than two samples ends on its first sample; and the chain of 17.
    The restatement's tables under BOTH metrics with tree(0, 17), loops on -- computed once, shared and left unchanged"""
    with Registered(ctx) as arrays:
        clips = [restatement.mixed_clip(k, num_samples, num_tracks, offset=9 * k, scales="default" if k % 7 == 3 else "mixed", close_loop=(k // 4 + k) % 2 == 1 and num_samples > 2)
                 for k, (num_tracks, num_samples) in enumerate(SHAPES)]
        handles = [arrays.add(samples) for samples in clips]
        parents = restatement.tree(0, MAX_TRACKS)
        found = {metric: [find(samples, metric, parents=parents, flags=OPTIMIZE_LOOPS) for samples in clips] for metric in (METRIC_QVVF, METRIC_MATRIX)}
        chain = scaled_chain(6, 33, 17)
        chain_parents = restatement.tree(0, 17, "chain")
        deep = {metric: find(chain, metric, parents=chain_parents) for metric in (METRIC_QVVF, METRIC_MATRIX)}
        yield ctx, handles, clips, parents, found, arrays.add(chain), chain, chain_parents, deep


def test_the_table_is_the_matrix_restatements(sweep):
    """mixed shapes, a repeated handle and refused instances in one launch, rows of a larger stride: every byte of every row, the sentinel
    everywhere else -- the rows the vote removed, the room between rows, the rows of the refused --, the results between served neighbours"""
    ctx, handles, clips, parents, found, *_ = sweep
    matrix = found[METRIC_MATRIX]
    order = [(7 * i + 2) % len(handles) for i in range(len(handles) + 3)]
    check_table(search(ctx, [handles[k] for k in order], flags=OPTIMIZE_LOOPS, parents=parents), [matrix[k] for k in order])
    picked = [k for k, shape in enumerate(SHAPES) if shape in ((3, 33), (17, 33), (17, 65), (1, 2), (5, 65))]
    segment_stride = 4 * MAX_TRACKS + 12
    with_refused = [handles[picked[0]], 0, handles[picked[1]], handles[picked[2]], 0xFFFFFF, handles[picked[3]], handles[picked[4]]]
    expected = [matrix[picked[0]], REFUSED, matrix[picked[1]], matrix[picked[2]], REFUSED, matrix[picked[3]], matrix[picked[4]]]
    check_table(search(ctx, with_refused, flags=OPTIMIZE_LOOPS, parents=parents, segment_stride=segment_stride, instance_stride=MAX_SEGMENTS * segment_stride + 8), expected)
    by_shape = dict(zip(SHAPES, matrix))
    assert [len(by_shape[17, s].base.segments) for s in SAMPLE_COUNTS] == [1, 1, 2, 4]
    assert any(f.base.wrap and f.base.num_samples == clip.shape[0] - 1 for f, clip in zip(matrix, clips))               # a vote that removed a sample
    assert len(set().union(*(restatement.triples_of(f.base) for f in matrix))) == 27
    assert any(not (f.base.types[2] != DEFAULT).any() and (f.base.types[0:2] == ANIMATED).any() for f in matrix)         # a clip without scale
    assert any(not np.array_equal(f.table, f.local_table) for f in matrix)                                               # the object phase had work to do
    # and the sweep itself tells the metrics apart: a kernel that kept the qvvf arithmetic would not give these bytes
    assert any(not np.array_equal(a.table, b.table) for a, b in zip(found[METRIC_QVVF], matrix))


def test_a_chain_of_17_with_scales_that_are_not_uniform(sweep):
    """two matrices down a chain of 17, shear at every level; the feature is observable: the table is not the qvvf search's"""
    ctx, _, _, _, _, h_chain, chain, chain_parents, deep = sweep
    assert (deep[METRIC_MATRIX].base.types[2] == ANIMATED).all()
    assert not np.array_equal(deep[METRIC_MATRIX].table, deep[METRIC_MATRIX].local_table)
    assert not np.array_equal(deep[METRIC_MATRIX].table, deep[METRIC_QVVF].table)
    by_matrix = search(ctx, [h_chain, h_chain], max_samples=33, parents=chain_parents)
    check_table(by_matrix, [deep[METRIC_MATRIX]] * 2)
    by_qvvf = search(ctx, [h_chain, h_chain], METRIC_QVVF, max_samples=33, parents=chain_parents)
    check_table(by_qvvf, [deep[METRIC_QVVF]] * 2)
    assert not np.array_equal(by_matrix.flat, by_qvvf.flat)


def test_all_roots_a_clip_without_scale_and_per_track_settings(ctx):
    """no parent table: every object error is a local one; every scale the default: the qvvf search's table; per-track precisions and
    shell distances with a default pose"""
    roots = restatement.mixed_clip(5, 33, 17, offset=9)
    plain = restatement.mixed_clip(6, 33, 17, offset=18, scales="default")
    chain_parents = restatement.tree(0, 17, "chain")
    rng = np.random.default_rng(31)
    precisions = rng.choice(np.array([0.002, 0.01, 0.05], dtype=np.float32), size=17)
    distances = rng.choice(np.array([1.0, 3.0, 10.0], dtype=np.float32), size=17)
    pose = restatement.lossy.raw_restatement.bind_pose(21, 17)
    posed = [restatement.mixed_clip(7, 33, 17, offset=3, default_pose=pose), restatement.mixed_clip(8, 65, 5, offset=12, default_pose=pose)]
    settings = {"parents": restatement.tree(3, 17), "track_precisions": precisions, "track_shell_distances": distances, "default_pose": pose}
    with Registered(ctx) as arrays:
        h_roots, h_plain = arrays.add(roots), arrays.add(plain)
        found = find(roots)
        assert np.array_equal(found.table, found.local_table)
        check_table(search(ctx, [h_roots], max_samples=33), [found])
        without_scale = find(plain, parents=chain_parents)
        assert not (without_scale.base.types[2] != DEFAULT).any() and np.array_equal(without_scale.table, find(plain, METRIC_QVVF, parents=chain_parents).table)
        check_table(search(ctx, [h_plain, h_plain], max_samples=33, parents=chain_parents), [without_scale] * 2)
        handles = [arrays.add(samples) for samples in posed]
        check_table(search(ctx, handles, **settings), [find(samples, **settings) for samples in posed])


def test_two_runs_give_the_same_bytes_and_a_capture_replays_to_them(sweep):
    ctx, handles, clips, parents, found, *_ = sweep
    picked = [k for k, shape in enumerate(SHAPES) if shape[0] in (5, 17)]
    runs = [search(ctx, [handles[k] for k in picked], flags=OPTIMIZE_LOOPS, parents=parents, graph=graph) for graph in (False, False, True)]
    assert same(runs[0], runs[1])
    assert same(runs[0], runs[2])           # the same launch captured into a graph and replayed


def arithmetic_cases():
    cases = {what: metric_restatement.arithmetic_case(what) for what in ("constant", "vote")}
    assert cases["constant"] is not None and cases["vote"] is not None
    return cases


def test_the_two_writers_are_the_matrix_restatements(sweep):
    """both writers at metric 1 on every byte, a sentinel behind `size`, the shell metadata on bits: closing loops (the vote), the chain,
    and the clips of one track on which only the arithmetic decides -- there the qvvf restatement gives other bytes, so these alone show
    that the vote and the compaction switched arithmetic"""
    ctx, handles, clips, parents, found, h_chain, chain, chain_parents, deep = sweep
    picked = [k for k, shape in enumerate(SHAPES) if shape in ((3, 33), (17, 33), (17, 65), (5, 2), (17, 31), (5, 65))]
    tables = np.zeros((len(picked), MAX_SEGMENTS, MAX_TRACKS, 4), dtype=np.uint8)
    expected = []
    for row, k in enumerate(picked):
        table = found[METRIC_MATRIX][k].table
        tables[row, :table.shape[0], :table.shape[1]] = table
        expected.append(metric_restatement.compress_variable(clips[k], RATE, table, METRIC_MATRIX, parents=parents, flags=OPTIMIZE_LOOPS, precision=PRECISION, shell_distance=SHELL))
    assert any(c.wrap for c in expected)
    check_rows(launch(ctx, through("variable"), [handles[k] for k in picked], rates=tables, flags=OPTIMIZE_LOOPS, parents=parents), expected)
    expected = [metric_restatement.compress_drop_w(clips[k], RATE, METRIC_MATRIX, parents=parents, flags=OPTIMIZE_LOOPS, precision=PRECISION, shell_distance=SHELL) for k in picked]
    check_rows(launch(ctx, through("tracks"), [handles[k] for k in picked], flags=OPTIMIZE_LOOPS, parents=parents), expected)
    # the chain under its own table
    want = metric_restatement.compress_variable(chain, RATE, deep[METRIC_MATRIX].table, METRIC_MATRIX, parents=chain_parents, precision=PRECISION, shell_distance=SHELL)
    check_rows(launch(ctx, through("variable"), [h_chain], rates=deep[METRIC_MATRIX].table, max_tracks=17, max_samples=33, parents=chain_parents), [want])

    with Registered(ctx) as arrays:
        for what, (samples, precision, flags) in arithmetic_cases().items():
            handle = arrays.add(samples)
            settings = dict(flags=flags, precision=precision, shell_distance=SHELL)
            for metric in (METRIC_MATRIX, METRIC_QVVF):
                by_variable = metric_restatement.compress_variable(samples, RATE, (12, 12, 12), metric, **settings)
                by_drop_w = metric_restatement.compress_drop_w(samples, RATE, metric, **settings)
                check_rows(launch(ctx, through("variable", metric), [handle], rates=(12, 12, 12), max_tracks=1, max_samples=9, flags=flags, precision=float(precision)), [by_variable])
                check_rows(launch(ctx, through("tracks", metric), [handle], max_tracks=1, max_samples=9, flags=flags, precision=float(precision)), [by_drop_w])
                f = find(samples, metric, flags=flags, precision=precision)
                check_table(search(ctx, [handle], metric, max_tracks=1, max_samples=9, flags=flags, precision=float(precision)), [f])
                if what == "constant":
                    assert (by_drop_w.types[0, 0] == ANIMATED) == (metric == METRIC_MATRIX) and (by_variable.types[0, 0] == ANIMATED) == (metric == METRIC_MATRIX)
                else:
                    assert by_drop_w.wrap == by_variable.wrap == f.base.wrap == (metric == METRIC_QVVF)


def test_metric_0_through_the_fronts_is_the_base_calls_bytes(sweep):
    """table and blobs: the entry points without a metric and the fronts at ACLHIP_METRIC_QVVF, byte for byte, sentinels included; and the
    raw format takes either metric and gives the raw format's bytes"""
    ctx, handles, clips, parents, found, h_chain, chain, chain_parents, deep = sweep
    picked = [handles[k] for k, shape in enumerate(SHAPES) if shape[0] in (5, 17)] + [h_chain]
    settings = dict(flags=OPTIMIZE_LOOPS, parents=parents)
    for kind, arguments in (("search", {}), ("variable", {"rates": (9, 14, 7)}), ("tracks", {})):
        base, front = (launch(ctx, entry, picked, **arguments, **settings) for entry in (Entry(kind), through(kind, METRIC_QVVF)))
        assert np.array_equal(base.flat, front.flat) and np.array_equal(base.results, front.results) and np.array_equal(base.metadata, front.metadata)
        assert (base.results[:, 0] == runtime.COMPRESS_OK).all() and base.rejected == front.rejected == 0
    raw_format = {"rotation_format": runtime.ROTATION_QUATF_FULL, "max_tracks": MAX_TRACKS, "max_samples": MAX_SAMPLES, "with_metadata": False}
    normalized = [k for k, shape in enumerate(SHAPES) if shape in ((5, 33), (17, 2))]
    rows = [launch(ctx, entry, [handles[k] for k in normalized], **raw_format) for entry in (Entry("tracks"), through("tracks", METRIC_QVVF), through("tracks"))]
    assert np.array_equal(rows[0].flat, rows[1].flat) and np.array_equal(rows[0].flat, rows[2].flat)
    assert np.array_equal(rows[0].results, rows[1].results) and np.array_equal(rows[0].results, rows[2].results) and (rows[0].results[:, 1] > 0).any()


def test_search_then_compress_end_to_end(sweep):
    """runtime.compress_tracks_variable(bit_rates="search", metric=1) is the restatement's blob at the restatement's table; it registers,
    decodes through the ordinary decode to the oracle decoder's bits, and is within the precision by raw_clip_error(..., metric=1)
    wherever the restatement's record says every track met its threshold in every segment"""
    ctx, handles, clips, parents, found, h_chain, chain, chain_parents, deep = sweep
    picked = [k for k, shape in enumerate(SHAPES) if shape in ((17, 33), (17, 65), (5, 65), (3, 31))]
    settings = {"parents": parents, "precision": PRECISION, "shell_distance": SHELL, "optimize_loops": True, "metric": runtime.ERROR_METRIC_QVVF_MATRIX3X4F}
    tables = runtime.find_bit_rates(ctx, [handles[k] for k in picked], **settings)
    assert tables.shape == (len(picked), MAX_SEGMENTS, MAX_TRACKS, 4) and tables.dtype == np.uint8
    blobs = runtime.compress_tracks_variable(ctx, [handles[k] for k in picked], bit_rates="search", **settings)
    chain_settings = dict(settings, parents=chain_parents, optimize_loops=False)
    blobs += runtime.compress_tracks_variable(ctx, [h_chain], bit_rates="search", **chain_settings)
    cases = [(clips[k], found[METRIC_MATRIX][k], handles[k], parents, OPTIMIZE_LOOPS) for k in picked] + [(chain, deep[METRIC_MATRIX], h_chain, chain_parents, 0)]
    options = ob.default_options(normalization=ob.NORMALIZE_NEVER)
    params = runtime.default_params(rounding_policy=runtime.ROUND_FLOOR, looping_policy=runtime.LOOP_AS_COMPRESSED, normalization=runtime.NORMALIZE_NEVER)
    identity = np.tile(IDENTITY, (MAX_TRACKS, 1))
    all_met = 0
    for row, ((samples, searched, handle, tree, flags), blob) in enumerate(zip(cases, blobs)):
        if row < len(picked):
            want = np.zeros((MAX_SEGMENTS, MAX_TRACKS, 4), dtype=np.uint8)
            want[:searched.table.shape[0], :searched.table.shape[1]] = searched.table
            assert np.array_equal(tables[row], want)
        num_tracks = samples.shape[1]
        expected = metric_restatement.compress_variable(samples, RATE, searched.table, METRIC_MATRIX, parents=tree, flags=flags, precision=PRECISION, shell_distance=SHELL)
        assert np.array_equal(blob, expected.blob)
        status, message = runtime.check_clip(blob, check_hash=True)
        assert status == 0, message
        clip = ctx.register_clip(blob)
        skeleton = ctx.register_skeleton(tree[:num_tracks], identity[:num_tracks])
        try:
            times = (np.arange(expected.num_samples) / RATE).astype(np.float32)
            poses = ctx.decompress_tracks(np.full(len(times), clip, dtype=np.uint32), times, params=params)
            bone, error, _ = runtime.raw_clip_error(ctx, handle, clip, skeleton, SHELL, metric=runtime.ERROR_METRIC_QVVF_MATRIX3X4F)
        finally:
            ctx.unregister_skeleton(skeleton)
            ctx.unregister_clip(clip)
        for key in (0, len(times) // 2, len(times) - 1):
            by_oracle = ob.oracle_decompress_tracks(blob, float(times[key]), ob.ROUND_FLOOR, options=options)
            for lanes in LANES:
                assert np.array_equal(poses[key][:, lanes].view(np.uint32), by_oracle[:, lanes].view(np.uint32)), (row, key)
        met = searched.met.all(axis=0)
        print("case %d: %d of %d tracks met their threshold in every segment; worst matrix error %.6f at bone %d" % (row, int(met.sum()), num_tracks, error, bone))
        if met.all():
            all_met += 1
            assert error <= PRECISION
        else:
            assert error <= PRECISION or not met[bone]
    assert all_met >= 3


def test_an_unknown_metric_and_a_refused_instance_write_nothing_they_should_not(sweep):
    """an unknown metric: ACLHIP_ERROR_INVALID_ARGUMENT with its message and not one byte of the table, the rows, the results or the
    metadata; a refused and a non-finite instance between served neighbours leave their rows to the sentinel under the matrix metric"""
    import torch
    ctx, handles, clips, parents, found, *_ = sweep
    device = torch.device("cuda:0")
    picked = [k for k, shape in enumerate(SHAPES) if shape in ((5, 33), (17, 31))]
    n = len(picked)
    d_handles = torch.from_numpy(np.asarray([handles[k] for k in picked], dtype=np.uint32).view(np.int32)).to(device)
    d_parents = torch.from_numpy(parents.view(np.int32)).to(device)
    stride = runtime.variable_compress_bound(MAX_TRACKS, MAX_SAMPLES, 0)
    flat = torch.full((n * max(stride, MAX_SEGMENTS * MAX_TRACKS * 4),), SENTINEL, dtype=torch.uint8, device=device)
    d_results = torch.full((n, 2), 0x5A5A5A5A, dtype=torch.int32, device=device)
    d_workspace = torch.full((runtime.find_bit_rates_workspace_bytes(n, MAX_TRACKS, MAX_SAMPLES),), SENTINEL, dtype=torch.uint8, device=device)
    stream = torch.cuda.current_stream(device)
    for metric in (2, 255, 0xFFFFFFFF):
        for desc, method, extra in ((runtime.FindBitRatesDesc(), ctx.find_bit_rates_metric_batch, (MAX_SEGMENTS * MAX_TRACKS * 4, MAX_TRACKS * 4)),
                                    (runtime.CompressVariableDesc(), ctx.compress_tracks_variable_metric_batch, (stride,)),
                                    (runtime.CompressTracksDesc(), ctx.compress_tracks_metric_batch, (stride,))):
            desc.max_tracks, desc.precision, desc.shell_distance, desc.workspace = MAX_TRACKS, PRECISION, SHELL, d_workspace.data_ptr()
            desc.parent_indices, desc.num_table_tracks = d_parents.data_ptr(), MAX_TRACKS
            if hasattr(desc, "max_samples"):
                desc.max_samples = MAX_SAMPLES
            if hasattr(desc, "rotation_format"):
                desc.rotation_format = runtime.ROTATION_QUATF_DROP_W_FULL
            if hasattr(desc, "rotation_bit_rate"):
                desc.rotation_bit_rate = desc.translation_bit_rate = desc.scale_bit_rate = 12
            rejected_before = ctx.rejected_instance_count()
            with pytest.raises(runtime.AclHipError, match="unknown error metric %d" % metric):
                method(d_handles.data_ptr(), n, desc, flat.data_ptr(), *extra, d_results.data_ptr(), metric, stream=stream.cuda_stream)
            stream.synchronize()
            assert ctx.rejected_instance_count() == rejected_before
            assert (flat.cpu().numpy() == SENTINEL).all() and (d_workspace.cpu().numpy() == SENTINEL).all() and (d_results.cpu().numpy() == 0x5A5A5A5A).all()
    small, long = restatement.mixed_clip(2, 12, 5, offset=20), restatement.mixed_clip(3, 40, 5, offset=20)
    tree = restatement.tree(4, 5)
    with Registered(ctx) as arrays:
        h_small, h_long = arrays.add(small), arrays.add(long)
        bad = long.copy()
        bad[7, 2, 5] = np.nan
        h_bad = arrays.add(bad)
        f_small, f_long = find(small, parents=tree), find(long, parents=tree)
        check_table(search(ctx, [h_small, 0, h_long, h_bad, h_small], max_tracks=5, max_samples=40, parents=tree), [f_small, REFUSED, f_long, NOT_FINITE, f_small])
        check_table(search(ctx, [h_small, h_long, h_small], max_tracks=5, max_samples=39, parents=tree), [f_small, REFUSED, f_small])
        c_small, c_long = (metric_restatement.compress_variable(samples, RATE, (12, 12, 12), METRIC_MATRIX, parents=tree, precision=PRECISION, shell_distance=SHELL) for samples in (small, long))
        out = launch(ctx, through("variable"), [h_small, 0, h_long, h_bad, h_small], rates=(12, 12, 12), max_tracks=5, max_samples=40, parents=tree, with_metadata=False)
        check_rows(out, [c_small.blob, REFUSED, c_long.blob, NOT_FINITE, c_small.blob])
        with pytest.raises(ValueError, match="ACLHIP_COMPRESS_REFUSED"):
            runtime.find_bit_rates(ctx, [h_small, h_long], parents=np.array([0xFFFFFFFF, 0, 3, 0, 0], dtype=np.uint32), precision=PRECISION, shell_distance=SHELL,
                                   metric=runtime.ERROR_METRIC_QVVF_MATRIX3X4F)
