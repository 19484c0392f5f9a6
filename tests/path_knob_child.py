"""One configuration of tests/test_gpu_path_knobs.py, in a process of its own (the library reads its path knobs once per process):
  python tests/path_knob_child.py CONFIG      with the knobs of CONFIGS[CONFIG] in the environment
Asserts the kernels the knobs select, then runs the configuration's matrix against the oracle, and prints one JSON line
{config, ok, kernels, checks, seconds}. Any failed check raises (non-zero exit)."""
import json
import os
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for path in (ROOT, HERE):
    if path not in sys.path:
        sys.path.insert(0, path)

import numpy as np
import torch     # before acl_amd.runtime: torch brings its own HIP runtime (conftest.py)

from acl_amd import runtime, synth
from oracle import bindings as ob
from oracle.database import OracleDatabase
import helpers
from conftest import CLIP_SPECS, sample_times_for
from test_gpu_path_knobs import CONFIGS

SENTINEL = 0x7FBADBAD                   # a NaN: no decode writes it
WINDOW_TRACKS = 104                     # k_image_chunk_quads / 3
WAVES_PER_BLOCK, NUM_XCDS = 4, 8
POLICIES = (ob.ROUND_NONE, ob.ROUND_FLOOR, ob.ROUND_CEIL, ob.ROUND_NEAREST)
DEVICE = torch.device("cuda", 0)

# window counts 1 .. 6 at rows of the clip's own width: (name, spec)
WINDOW_CLIPS = [
    ("cmu_100", CLIP_SPECS["cmu_100"]),
    ("tracks_104", dict(seed=31, num_tracks=104, num_samples=45, has_scale=1)),
    ("tracks_105", dict(seed=32, num_tracks=105, num_samples=45, has_scale=1, raw_fraction=0.1)),
    ("cinematic_300", CLIP_SPECS["cinematic_300"]),
    ("three_full_windows_320", CLIP_SPECS["three_full_windows_320"]),
    ("tracks_551", dict(seed=33, num_tracks=551, num_samples=30, has_scale=1, raw_fraction=0.05)),
    ("giant_2500_all_animated", CLIP_SPECS["giant_2500_all_animated"]),
    ("all_animated_65", CLIP_SPECS["all_animated_65"]),
    ("raw_and_constant_rates", CLIP_SPECS["raw_and_constant_rates"]),
    ("high_bits_23", CLIP_SPECS["high_bits_23"]),
    ("stripped_wrap_scale", CLIP_SPECS["stripped_wrap_scale"]),
    ("v2_0_low_bits", CLIP_SPECS["v2_0_low_bits"]),
]
SEVERAL_WINDOW_TRACKS = 300             # rows of 300 tracks: three windows, for the small clips too (windows 1, 2 of them empty)


class Checks:
    def __init__(self):
        self.count = 0

    def __call__(self, condition, what):
        if not condition:
            raise AssertionError(what)
        self.count += 1


check = Checks()


def stride_of(tracks):
    """a row of `tracks` tracks and 16 bytes more: the launch's shape is the same, the bytes past the tracks must keep the sentinel"""
    return tracks * 48 + 16


def windows_of(stride):
    return max(-(-(stride // 48) * 3 // (WINDOW_TRACKS * 3)), 1)


def turn_instances(n, windows, items, adjacent):
    """the instances a wave of window 0 takes in turn, per wave (lists), as host_launch.inl sizes the in-turn grid and
    kernels_pose.inl maps its items: consecutive instances (adjacent) or turn_blocks * 4 / W apart (the sweep)"""
    if items <= 1:
        return [[i] for i in range(n)]
    if adjacent:
        return [list(range(g * items, min(g * items + items, n))) for g in range(-(-n // items))]
    num_blocks = -(-n * windows // WAVES_PER_BLOCK)
    turn_blocks = -(-num_blocks // items)
    while (turn_blocks * WAVES_PER_BLOCK) % windows != 0 or turn_blocks % NUM_XCDS != 0:
        turn_blocks += 1
    spacing = turn_blocks * WAVES_PER_BLOCK // windows
    return [[first + t * spacing for t in range(items) if first + t * spacing < n] for first in range(min(spacing, n))]


def decode(context, handles, times, stride, params=None, output=None, rows=None):
    """one pose launch; returns the rows (n + 1 of them, the last one past the batch) as uint32 [n + 1, stride / 4]"""
    n = handles.size
    d_clips = torch.from_numpy(handles.astype(np.uint32).view(np.int32)).to(DEVICE)
    d_times = torch.from_numpy(np.ascontiguousarray(times, dtype=np.float32)).to(DEVICE)
    d_poses = torch.full((n + 1, stride // 4), SENTINEL, dtype=torch.int32, device=DEVICE)
    if output is not None:
        context.decompress_tracks_batch_out(d_clips.data_ptr(), d_times.data_ptr(), n, d_poses.data_ptr(), stride, output, params=params)
    else:
        context.decompress_tracks_batch(d_clips.data_ptr(), d_times.data_ptr(), n, d_poses.data_ptr(), stride, params=params)
    torch.cuda.synchronize(DEVICE)
    return d_poses.cpu().numpy().view(np.uint32)


def expected_rows(blobs, which, times, tracks_of, stride, rounding=ob.ROUND_NONE, options=None, valid=None):
    """the oracle's rows in the same form: tracks where the instance's clip has them, the sentinel everywhere else"""
    n = which.size
    widest = max(tracks_of)
    poses = np.full((n, widest, 12), SENTINEL, dtype=np.uint32).view(np.float32)
    ob.oracle_decompress_tracks_batch(blobs, which.astype(np.uint32), times, widest, rounding=rounding, options=options, out=poses)
    rows = np.full((n + 1, stride // 4), SENTINEL, dtype=np.uint32)
    rows[:n, : widest * 12] = poses.view(np.uint32).reshape(n, widest * 12)
    if valid is not None:
        rows[:n][~valid] = SENTINEL
    return rows


def as_poses(rows, tracks):
    return rows[:-1, : tracks * 12].view(np.float32).reshape(-1, tracks, 12)


def assert_rows(got, expected, what):
    if not np.array_equal(got, expected):
        bad = np.nonzero((got != expected).any(axis=1))[0]
        raise AssertionError(f"{what}: {bad.size} rows differ, first {bad[:8].tolist()}")
    check.count += 1


# ---------------------------------------------------------------------------------------------------------------------------------------
def check_kernels(context, config):
    """before anything is decoded: the knobs select the kernels the table names (a knob no longer read fails here)"""
    reached = []
    strides = {"one_window": 100 * 48, "several_windows": SEVERAL_WINDOW_TRACKS * 48}
    for kind, (exact, fast) in config["kernels"].items():
        for params, name in ((runtime.default_params(), exact), (runtime.default_params(flags=runtime.DECODE_FAST), fast)):
            got = context.tracks_kernel_name(params, pose_stride_bytes=strides[kind])
            check(got == name, f"{kind}: {got}, expected {name}")
            reached.append(got)
    for kind, name in config.get("other_kernels", {}).items():
        output, params = runtime.OutputDesc(), runtime.default_params()
        if kind in ("qv32", "qvv40"):
            output.layout = runtime.LAYOUT_QV32 if kind == "qv32" else runtime.LAYOUT_QVV40
        if kind in ("compact", "any_settings_compact"):
            output.skip_scales = 1
        if kind.startswith("any_settings"):
            params = helpers.gpu_params(runtime, settings=1)
        got = context.tracks_kernel_name(params, pose_stride_bytes=100 * 48, output=output)
        check(got == name, f"{kind}: {got}, expected {name}")
        reached.append(got)
    return reached


def window_counts(context, config, clips, handles, rng):
    """every clip of WINDOW_CLIPS at its own row width and at rows of three windows, all four rounding policies; the fast decode
    against the exact one and the oracle"""
    worst_fast = 0.0
    for (name, _), clip, handle in zip(WINDOW_CLIPS, clips, handles):
        times = sample_times_for(clip.duration, 40, rng)
        n = times.size
        ids = np.full(n, handle, dtype=np.uint32)
        which = np.zeros(n, dtype=np.uint32)
        for stride in sorted({stride_of(clip.num_tracks), stride_of(max(clip.num_tracks, SEVERAL_WINDOW_TRACKS))}):
            for policy in POLICIES:
                params = runtime.default_params(rounding_policy=policy)
                got = decode(context, ids, times, stride, params)
                expected = expected_rows([clip.blob], which, times, [clip.num_tracks], stride, rounding=policy)
                assert_rows(got, expected, f"{name}: {windows_of(stride)} windows, rounding {policy}")
                if config["fast_matrix"]:
                    fast = decode(context, ids, times, stride, runtime.default_params(rounding_policy=policy, flags=runtime.DECODE_FAST))
                    worst_fast = max(worst_fast, helpers.assert_within_tolerance(as_poses(fast, clip.num_tracks), as_poses(got, clip.num_tracks), name + " (fast)"))
                    helpers.assert_within_tolerance(as_poses(fast, clip.num_tracks)[::7], as_poses(expected, clip.num_tracks)[::7], name + " (fast, oracle)")
                    check(np.array_equal(fast[:, clip.num_tracks * 12:], got[:, clip.num_tracks * 12:]), f"{name} (fast): bytes past the tracks")
    if config["fast_matrix"]:
        check(worst_fast > 0.0, "ACLHIP_DECODE_FAST changed no rotation")


def tails_and_sequences(context, config, rng):
    """instance counts at the grid's tails, with the clip sequences A A B A, A B B A, A <invalid> A, A B A, A C A placed on one wave's
    turns and a random mix of A, B, C and invalid handles everywhere else"""
    specs = {"A": dict(seed=41, num_tracks=300, num_samples=36, has_scale=1, rotation_constant=0.3, translation_constant=0.4, scale_constant=0.3),
             "B": dict(seed=42, num_tracks=300, num_samples=52, has_scale=1, rotation_constant=0.25, translation_constant=0.35, scale_default=0.2, scale_constant=0.3, raw_fraction=0.05),
             "C": dict(seed=43, num_tracks=100, num_samples=40, rotation_constant=0.3, translation_constant=0.3)}
    clips = {key: synth.build_clip(**spec) for key, spec in specs.items()}
    handles = {key: context.register_clip(clip.blob) for key, clip in clips.items()}
    keys = ["A", "B", "C"]
    blobs = [clips[key].blob for key in keys]
    stride = stride_of(SEVERAL_WINDOW_TRACKS)
    windows = windows_of(stride)
    items = config["items"]
    sequences = ["AABA", "ABBA", "A-A", "ABA", "ACA"]
    for n in (1, 2, 3, 5, 1021, 4099, 4 * items * 8 - 1, 4 * items * 8 + 1):
        which = rng.choice(np.array([0, 0, 1, 1, 2, 3]), size=n)        # 3: an invalid handle
        waves = turn_instances(n, windows, items, config["adjacent"])
        taken = np.zeros(n, dtype=bool)
        placed = 0
        for sequence in sequences:
            for turns in waves:
                if len(turns) >= len(sequence) and not taken[turns[: len(sequence)]].any():
                    positions = turns[: len(sequence)]
                    which[positions] = ["ABC-".index(letter) for letter in sequence]
                    taken[positions] = True
                    placed += 1
                    break
        check(n < 1000 or items < 3 or placed >= 3, f"n {n}: only {placed} sequences placed")     # (small batches: few waves have turns)
        valid = which < 3
        ids = np.array([handles[keys[w]] if w < 3 else runtime.INVALID_HANDLE for w in which], dtype=np.uint32)
        durations = np.array([clips[keys[w]].duration if w < 3 else 1.0 for w in which], dtype=np.float32)
        times = (rng.uniform(-0.05, 1.05, size=n) * durations).astype(np.float32)
        for policy in (ob.ROUND_NONE, ob.ROUND_NEAREST):
            before = context.rejected_instance_count()
            got = decode(context, ids, times, stride, runtime.default_params(rounding_policy=policy))
            check(context.rejected_instance_count() - before == int((~valid).sum()), f"n {n}: rejected count")
            expected = expected_rows(blobs, np.where(valid, which, 0), times, [300, 300, 100], stride, rounding=policy, valid=valid)
            assert_rows(got, expected, f"n {n}: mixed clips, rounding {policy}")
        # one clip for the whole batch: every turn of every wave may reuse its image
        ids_a = np.full(n, handles["A"], dtype=np.uint32)
        got = decode(context, ids_a, times, stride)
        assert_rows(got, expected_rows(blobs, np.zeros(n, dtype=np.uint32), times, [300], stride), f"n {n}: clip A only")
        # and rows of one window
        ids_c = np.full(n, handles["C"], dtype=np.uint32)
        c_times = (rng.uniform(-0.05, 1.05, size=n) * clips["C"].duration).astype(np.float32)
        got = decode(context, ids_c, c_times, stride_of(100))
        assert_rows(got, expected_rows([clips["C"].blob], np.zeros(n, dtype=np.uint32), c_times, [100], stride_of(100)), f"n {n}: one window")
    return clips, handles


def per_instance_arrays(context, clips, handles, rng):
    """instance_rounding_policies, instance_looping_policies and output.instance_track_counts together, on poses of three windows"""
    keys = ["A", "B", "C"]
    n = 2000
    which = rng.integers(0, 3, size=n)
    ids = np.array([handles[keys[w]] for w in which], dtype=np.uint32)
    durations = np.array([clips[keys[w]].duration for w in which], dtype=np.float32)
    times = (rng.uniform(0.7, 1.3, size=n) * durations).astype(np.float32)
    rounding = rng.integers(0, 4, size=n).astype(np.uint8)
    looping = rng.integers(0, 3, size=n).astype(np.uint8)
    counts = rng.choice(np.array([300, 250, 104, 105, 60, 1]), size=n).astype(np.uint32)
    stride = stride_of(SEVERAL_WINDOW_TRACKS)
    blobs = [clips[key].blob for key in keys]
    expected = np.full((n + 1, stride // 4), SENTINEL, dtype=np.uint32)
    for policy in range(3):
        for round_policy in range(4):
            chosen = np.nonzero((looping == policy) & (rounding == round_policy))[0]
            if chosen.size:
                rows = expected_rows(blobs, which[chosen], times[chosen], [300, 300, 100], stride, rounding=round_policy, options=ob.default_options(looping_policy=policy))
                expected[chosen] = rows[:-1]
    for i in range(n):
        expected[i, counts[i] * 12:] = SENTINEL
    d_rounding, d_looping = torch.from_numpy(rounding).to(DEVICE), torch.from_numpy(looping).to(DEVICE)
    d_counts = torch.from_numpy(counts.view(np.int32)).to(DEVICE)
    params = runtime.default_params()
    params.instance_rounding_policies, params.instance_looping_policies = d_rounding.data_ptr(), d_looping.data_ptr()
    output = runtime.OutputDesc()
    output.instance_track_counts = d_counts.data_ptr()
    got = decode(context, ids, times, stride, params, output=output)
    assert_rows(got, expected, "per instance rounding, looping and track counts")


def database_clip(context, rng):
    """a database-bound clip of two windows: its keys come from database chunks through the wide reads, tiers out, in, out again"""
    case = helpers.load_database_golden("two_window_clip_130_bones")
    database = context.register_database(case["database"], case["bulk_medium"], case["bulk_low"])
    bound = [context.register_clip_with_database(blob, database) for blob in case["clips"]]
    oracle_db = OracleDatabase(case["database"], case["bulk_medium"], case["bulk_low"])
    blob = case["clips"][0]
    tracks = ob.oracle().aclo_num_tracks(blob.ctypes.data)
    check(tracks > WINDOW_TRACKS, "the database clip has one window")
    times, duration = helpers.corpus_sample_times(blob)
    times = np.concatenate([times, rng.uniform(0.0, duration, size=64).astype(np.float32)])
    n = times.size
    stride = stride_of(tracks)
    ids = np.full(n, bound[0], dtype=np.uint32)

    def compare(state):
        for policy in (ob.ROUND_NONE, ob.ROUND_NEAREST):
            got = decode(context, ids, times, stride, runtime.default_params(rounding_policy=policy))
            expected = np.full((n + 1, stride // 4), SENTINEL, dtype=np.uint32)
            for i in range(n):
                expected[i, : tracks * 12] = oracle_db.decompress_tracks(blob, float(times[i]), policy).view(np.uint32).ravel()
            assert_rows(got, expected, f"database clip, {state}, rounding {policy}")

    everything = 0xFFFFFFFF
    compare("tiers streamed out")
    for tier in (runtime.TIER_MEDIUM_IMPORTANCE, runtime.TIER_LOWEST_IMPORTANCE):
        check(context.database_stream_in(database, tier, everything) == oracle_db.stream_in(tier, everything), "stream in")
    torch.cuda.synchronize(DEVICE)
    compare("tiers streamed in")
    check(context.database_stream_out(database, runtime.TIER_LOWEST_IMPORTANCE, everything) == oracle_db.stream_out(runtime.TIER_LOWEST_IMPORTANCE, everything), "stream out")
    torch.cuda.synchronize(DEVICE)
    compare("low tier streamed out again")
    for handle in bound:
        context.unregister_clip(handle)
    context.unregister_database(database)


def pose_matrix(context, config, rng):
    clips = [synth.build_clip(**spec) for _, spec in WINDOW_CLIPS]
    handles = [context.register_clip(clip.blob) for clip in clips]
    reached = check_kernels(context, config)
    window_counts(context, config, clips, handles, rng)
    sequence_clips, sequence_handles = tails_and_sequences(context, config, rng)
    per_instance_arrays(context, sequence_clips, sequence_handles, rng)
    database_clip(context, rng)
    return reached


# ---------------------------------------------------------------------------------------------------------------------------------------
def short_exact_off(context, config, rng):
    """the compiler's square roots everywhere: every corpus clip (one window and several), every sample, whole poses and single tracks"""
    corpus = [clip for clip in helpers.load_corpus() if clip["spec"]["bones"] > 0]
    handles = [context.register_clip(clip["blob"]) for clip in corpus]
    reached = check_kernels(context, config)
    failures = []
    for clip, handle in zip(corpus, handles):
        bones = clip["spec"]["bones"]
        times, duration = helpers.corpus_sample_times(clip["blob"])
        rate = np.float32(clip["spec"]["rate"])
        # (and t = 0: a clip of one sample has no sample times of its own)
        times = np.concatenate([times, np.minimum(times + np.float32(0.37) / rate, np.float32(duration)), [0.0]]).astype(np.float32)
        ids = np.full(times.size, handle, dtype=np.uint32)
        for policy in (ob.ROUND_NONE, ob.ROUND_NEAREST):
            params = runtime.default_params(rounding_policy=policy)
            got = context.decompress_tracks(ids, times, params=params)
            expected = ob.oracle_decompress_tracks_batch([clip["blob"]], np.zeros(times.size, dtype=np.uint32), times, bones, rounding=policy)
            if not helpers.exact(got, expected):
                lanes = np.nonzero((got.view(np.uint32) != expected.view(np.uint32)).any(axis=(0, 1)))[0].tolist()
                failures.append(f"{clip['name']}: decompress_tracks, rounding {policy}: lanes {lanes}, xyz bit equal {helpers.bit_equal(got, expected)}, "
                                f"max diff {float(np.abs(got - expected).max())}, got {got.ravel()[:12].tolist()} expected {expected.ravel()[:12].tolist()}")
            count = min(times.size * bones, 4096)
            instance = rng.integers(0, times.size, size=count)
            track = rng.integers(0, bones, size=count).astype(np.uint32)
            single = context.decompress_track(ids[instance], times[instance], track, params=runtime.default_params(rounding_policy=policy))
            if not helpers.exact(single, expected[instance, track]):
                failures.append(f"{clip['name']}: decompress_track, rounding {policy}: xyz bit equal {helpers.bit_equal(single, expected[instance, track])}")
    check(not failures, "\n".join(failures))
    check(context.rejected_instance_count() == 0, "rejected instances")
    return reached


def no_slabs(context, config, rng):
    """one hipMalloc per clip and a fixed-size clip table: 1 500 clips registered, every other one unregistered, 500 more registered
    (free_clip_memory, recycled slots), then mixed batches, mixed single track requests and a scalar list clip"""
    check(context.lifetime_stats()["table_is_virtual"] == 0, "the clip table is virtual")
    live = {}
    for index in range(1500):
        spec = dict(seed=5000 + index, num_tracks=int(rng.integers(3, 301)), num_samples=int(rng.integers(2, 12)), has_scale=int(index % 3 == 0))
        clip = synth.build_clip(**spec)
        live[context.register_clip(clip.blob)] = clip
    for handle in list(live)[::2]:
        context.unregister_clip(handle)
        del live[handle]
    for index in range(500):
        clip = synth.build_clip(seed=7000 + index, num_tracks=int(rng.integers(3, 301)), num_samples=int(rng.integers(2, 12)))
        live[context.register_clip(clip.blob)] = clip
    stats = context.lifetime_stats()
    check(stats["table_is_virtual"] == 0 and stats["unregistered"] == 750 and stats["registered"] == 2000, f"lifetime stats {stats}")
    reached = check_kernels(context, config)
    handle_list = np.array(list(live), dtype=np.uint32)
    blobs = [live[int(h)].blob for h in handle_list]
    tracks = [live[int(h)].num_tracks for h in handle_list]
    n = 6000
    which = rng.integers(0, handle_list.size, size=n).astype(np.uint32)
    durations = np.array([live[int(h)].duration for h in handle_list], dtype=np.float32)
    times = (rng.uniform(-0.05, 1.05, size=n) * durations[which]).astype(np.float32)
    stride = stride_of(300)
    for policy in (ob.ROUND_NONE, ob.ROUND_NEAREST):
        got = decode(context, handle_list[which], times, stride, runtime.default_params(rounding_policy=policy))
        assert_rows(got, expected_rows(blobs, which, times, tracks, stride, rounding=policy), f"mixed batch, rounding {policy}")
    track_index = np.array([rng.integers(0, tracks[w]) for w in which], dtype=np.uint32)
    single = context.decompress_track(handle_list[which], times, track_index)
    expected = ob.oracle_decompress_tracks_batch(blobs, which, times, 300)
    check(helpers.exact(single, expected[np.arange(n), track_index]), "mixed single track requests")
    scalar = synth.build_scalar_clip(seed=9, track_type=2, num_tracks=21, num_samples=33)
    scalar_handle = context.register_clip(scalar.blob)
    scalar_times = sample_times_for(float(ob.oracle().aclo_finite_duration(scalar.blob.ctypes.data, ob.LOOP_AS_COMPRESSED)), 60, rng)
    values = context.decompress_scalar_tracks(np.full(scalar_times.size, scalar_handle, dtype=np.uint32), scalar_times)
    expected = ob.oracle_scalar_decompress_tracks_batch([scalar.blob], np.zeros(scalar_times.size, dtype=np.uint32), scalar_times, 21 * 3)
    check(helpers.exact(values.reshape(scalar_times.size, -1), expected.reshape(scalar_times.size, -1)), "scalar list clip")
    check(context.rejected_instance_count() == 0, "rejected instances")
    return reached


def order_3(context, config, rng):
    """the three launch form of aclhip_order_instances_device: a permutation bucketed by clip like the host's order, the decode
    through it, and one instance_list_update round"""
    from test_order_instances import check_order
    # (clip 0 is a 300-bone rig: the plain ordering call orders for rows of three windows, and the decode that follows has them)
    clips = [synth.build_clip(seed=8000 + i, num_tracks=300 if i == 0 else int(rng.integers(3, 101)), num_samples=int(rng.integers(2, 20))) for i in range(300)]
    handles = np.array([context.register_clip(clip.blob) for clip in clips], dtype=np.uint32)
    reached = check_kernels(context, config)
    stride = stride_of(300)
    windows = context.pose_windows_of_launch(stride)
    check(windows == 3, f"{windows} windows")
    n = 20000
    which = rng.integers(0, len(clips), size=n).astype(np.uint32)
    durations = np.array([clip.duration for clip in clips], dtype=np.float32)
    times = (rng.uniform(0.0, 1.0, size=n) * durations[which]).astype(np.float32)
    ids = handles[which]
    d_clips = torch.from_numpy(ids.view(np.int32)).to(DEVICE)
    d_times = torch.from_numpy(times).to(DEVICE)
    d_order = torch.full((n,), -1, dtype=torch.int32, device=DEVICE)
    d_out_clips = torch.full((n,), -1, dtype=torch.int32, device=DEVICE)
    d_out_times = torch.zeros((n,), dtype=torch.float32, device=DEVICE)
    context.order_instances_device(d_clips.data_ptr(), d_times.data_ptr(), n, d_order.data_ptr(), d_out_clips.data_ptr(), d_out_times.data_ptr())
    torch.cuda.synchronize(DEVICE)
    order = d_order.cpu().numpy().view(np.uint32)
    check_order(ids, order, windows, stable=False)
    check(np.array_equal(ids[order], ids[context.order_instances_for_locality(ids)]), "the device order's buckets are not the host order's")
    check(np.array_equal(d_out_clips.cpu().numpy().view(np.uint32), ids[order]), "ordered clips")
    check(np.array_equal(d_out_times.cpu().numpy().view(np.uint32), times[order].view(np.uint32)), "ordered times")
    got = decode(context, ids[order], times[order], stride)
    in_instance_order = np.empty_like(got)
    in_instance_order[order] = got[:-1]
    in_instance_order[-1] = got[-1]
    tracks = [clip.num_tracks for clip in clips]
    assert_rows(in_instance_order, expected_rows([clip.blob for clip in clips], which, times, tracks, stride), "decode through the device order")
    # an instance list: set, one update round, the decode in instance order
    instance_list = context.instance_list_create(n)
    context.instance_list_set_clips(instance_list, d_clips.data_ptr())
    changed = rng.choice(n, size=n // 20, replace=False).astype(np.int32)
    which[changed] = rng.integers(0, len(clips), size=changed.size).astype(np.uint32)
    d_changed = torch.from_numpy(changed).to(DEVICE)
    d_new = torch.from_numpy(handles[which[changed]].view(np.int32)).to(DEVICE)
    context.instance_list_update(instance_list, d_changed.data_ptr(), d_new.data_ptr(), changed.size)
    times = (rng.uniform(0.0, 1.0, size=n) * durations[which]).astype(np.float32)
    d_times.copy_(torch.from_numpy(times))
    d_rows = torch.full((n + 1, stride // 4), SENTINEL, dtype=torch.int32, device=DEVICE)
    torch.cuda.synchronize(DEVICE)
    context.decompress_tracks_list(instance_list, d_times.data_ptr(), d_rows.data_ptr(), stride, poses_in_instance_order=True)
    torch.cuda.synchronize(DEVICE)
    assert_rows(d_rows.cpu().numpy().view(np.uint32), expected_rows([clip.blob for clip in clips], which, times, tracks, stride), "instance list after an update")
    context.instance_list_destroy(instance_list)
    check(context.rejected_instance_count() == 0, "rejected instances")
    return reached


def main(name):
    start = time.time()
    config = CONFIGS[name]
    torch.cuda.init()
    rng = np.random.default_rng(sum(map(ord, name)))
    with runtime.Context(0) as context:
        run = {"pose": pose_matrix, "short_exact_off": short_exact_off, "no_slabs": no_slabs, "order_3": order_3}[config["child"]]
        reached = run(context, config, rng)
    print(json.dumps({"config": name, "ok": True, "kernels": sorted(set(reached)), "checks": check.count, "seconds": time.time() - start}))


if __name__ == "__main__":
    main(sys.argv[1])
