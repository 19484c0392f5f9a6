"""Track maps (aclhip_register_track_map, aclhip_decompress_tracks_batch_mapped): track t of a clip is stored in record map[t] of the
pose row -- the run time form of track_writer::write_rotation / _translation / _scale(track_index, value) (core/track_writer.h).

The expected buffer is always built in numpy from the ORACLE's pose of the unmapped decode: expected[row, map[t]] = oracle[row, t]
for what the writer of the launch takes; every other byte of the buffer -- untouched slots, skipped pieces, the bytes between
num_slots records and the stride, guard rows before and after -- keeps the sentinel it was filled with, filled slots hold fill_pose.
Compared on bits over the WHOLE buffer. Needs a GPU."""
import ctypes
import os
import threading

import numpy as np
import pytest
import torch

from acl_amd import runtime, synth
from oracle import bindings as ob
from oracle.database import OracleDatabase
import helpers
from conftest import CLIP_SPECS

pytestmark = pytest.mark.gpu

DROPPED = runtime.TRACK_DROPPED
SENTINEL = np.float32(-77.25)
FILL_SENTINELS = (np.float32(3.5), np.float32(-9.75))
GUARD_ROWS = 3
# floats of a QVV48 record a layout keeps, in the order it stores them
COLUMNS = {"qvv48": list(range(12)), "qvv40": [0, 1, 2, 3, 4, 5, 6, 8, 9, 10], "qv32": [0, 1, 2, 3, 4, 5, 6, 7]}
KIND_OF_FLOAT = np.repeat(np.arange(3), 4)


@pytest.fixture(scope="module", params=["common_case_kernel", "any_settings_kernel"])
def context(request):
    if request.param == "any_settings_kernel":
        os.environ["ACLHIP_FORCE_GENERIC_KERNEL"] = "1"
    try:
        ctx = runtime.Context(0)
    finally:
        os.environ.pop("ACLHIP_FORCE_GENERIC_KERNEL", None)
    yield ctx
    ctx.close()


# ---- maps ----
def order_preserving_map(num_tracks, num_slots, rng):
    return np.sort(rng.choice(num_slots, size=num_tracks, replace=False)).astype(np.uint32)


def permutation_map(num_tracks, num_slots, rng):
    return rng.choice(num_slots, size=num_tracks, replace=False).astype(np.uint32)


def dropping_map(num_tracks, num_slots, rng):
    table = permutation_map(num_tracks, num_slots, rng)
    table[rng.choice(num_tracks, size=num_tracks // 3, replace=False)] = DROPPED
    return table


def far_apart_map(num_tracks, num_slots):
    """neighbouring tracks go to slots a pose window (104 records) and more apart"""
    assert num_slots >= num_tracks
    stride = 105
    while np.gcd(stride, num_slots) != 1:
        stride += 1
    return ((np.arange(num_tracks, dtype=np.uint64) * stride) % num_slots).astype(np.uint32)


MAP_KINDS = {"order_preserving": order_preserving_map, "permutation": permutation_map, "dropping": dropping_map}


# ---- the oracle's side ----
def oracle_with_written_mask(blob, times, num_tracks, options=None, rounding=ob.ROUND_NONE):
    """(values, written) [n, tracks, 12]: the oracle's unmapped pose and which floats its writer wrote at all (skipped default sub-tracks
    leave theirs: decoded twice over two different backgrounds, what differs was not written)"""
    n = times.size
    outs = []
    for background in FILL_SENTINELS:
        out = np.full((n, num_tracks, 12), background, dtype=np.float32)
        ob.oracle_decompress_tracks_batch([blob], np.zeros(n, dtype=np.uint32), times, num_tracks, rounding=rounding, options=options, out=out)
        outs.append(out)
    return outs[0], outs[0].view(np.uint32) == outs[1].view(np.uint32)


def expected_buffer(layout, stride_floats, num_rows, values, written, tables, num_slots, rows=None, fill_pose=None, refused=()):
    """values / written: per instance [tracks_i, 12] arrays (lists: instances may differ in size); tables: per instance track_to_slot"""
    columns = COLUMNS[layout]
    width = len(columns)
    buffer = np.full((GUARD_ROWS + num_rows + GUARD_ROWS, stride_floats), SENTINEL, dtype=np.float32)
    for i in range(len(values)):
        if i in refused:
            continue
        row = buffer[GUARD_ROWS + (i if rows is None else int(rows[i]))]
        table = np.asarray(tables[i])
        records = row[: num_slots * width].reshape(num_slots, width)
        if fill_pose is not None:
            unmapped = np.setdiff1d(np.arange(num_slots), table[table != DROPPED])
            records[unmapped] = fill_pose.reshape(num_slots, width)[unmapped]
        mapped = np.flatnonzero(table != DROPPED)
        source, mask = values[i][mapped][:, columns], written[i][mapped][:, columns]
        target = records[table[mapped]]
        target[mask] = source[mask]
        records[table[mapped]] = target
    return buffer


class Launch:
    """one mapped launch into a guarded, sentinel filled buffer"""

    def __init__(self, context, layout, num_slots, num_rows, extra_stride_bytes=64):
        self.context, self.layout, self.num_slots, self.num_rows = context, layout, num_slots, num_rows
        self.layout_id, self.record_bytes = runtime.LAYOUTS[layout]
        self.stride = (num_slots * self.record_bytes + extra_stride_bytes + 63) // 64 * 64
        self.buffer = torch.full((GUARD_ROWS + num_rows + GUARD_ROWS, self.stride // 4), float(SENTINEL), dtype=torch.float32, device="cuda")
        self.keep = []

    def device(self, array, dtype):
        array = np.ascontiguousarray(array)
        if dtype == np.int32:       # (handles travel as their 32 bits: torch has no uint32 arithmetic to lose)
            array = array.astype(np.uint32).view(np.int32)
        self.keep.append(torch.from_numpy(array.astype(dtype)).cuda())
        return self.keep[-1]

    def fill_pose(self, rng):
        pose = rng.uniform(-4.0, 4.0, size=self.num_slots * self.record_bytes // 4).astype(np.float32)
        return pose, self.device(pose, np.float32)

    def run(self, handles, times, track_map=0, instance_maps=None, fill=None, output=None, params=None, stream=None):
        output = output if output is not None else runtime.OutputDesc()
        output.layout = self.layout_id
        poses = self.buffer[GUARD_ROWS:]
        self.context.decompress_tracks_batch_mapped(self.device(handles, np.int32), self.device(times, np.float32), poses, self.stride, track_map=track_map,
                                                    instance_maps=self.device(instance_maps, np.int32) if instance_maps is not None else None,
                                                    fill_pose=fill, output=output, params=params, stream=stream)

    def result(self):
        torch.cuda.synchronize()
        return self.buffer.cpu().numpy()


_rejections = {}


def assert_rejected(context, more=0):
    """the context's counter of refused instances runs on from test to test: it has grown by exactly `more` since it was last looked at"""
    _rejections[id(context)] = _rejections.get(id(context), 0) + more
    assert context.rejected_instance_count() == _rejections[id(context)]


def check(got, expected, what):
    same = got.view(np.uint32) == expected.view(np.uint32)
    if not same.all():
        rows, floats = np.nonzero(~same)
        raise AssertionError(f"{what}: {rows.size} floats differ, first at buffer row {rows[0]} float {floats[0]}: got {got[rows[0], floats[0]]!r}, expected {expected[rows[0], floats[0]]!r}")


# ---- 1. the identity map is the unmapped decode ----
@pytest.mark.parametrize("layout", ["qvv48", "qvv40", "qv32"])
@pytest.mark.parametrize("name", ["cmu_100", "cinematic_300", "two_samples_three_tracks"])
def test_identity_map_is_the_unmapped_decode(context, name, layout):
    clip = synth.build_clip(**CLIP_SPECS[name])
    handle = context.register_clip(clip.blob)
    tracks = clip.num_tracks
    track_map = context.register_track_map(np.arange(tracks), tracks)
    info = context.track_map_info(track_map)
    assert (info.is_identity, info.is_order_preserving, info.num_unmapped_slots, info.num_mapped) == (1, 1, 0, tracks)
    rng = np.random.default_rng(5)
    n = 130
    times = rng.uniform(0.0, clip.duration, size=n).astype(np.float32)
    handles = np.full(n, handle, dtype=np.uint32)
    mapped = Launch(context, layout, tracks, n)
    mapped.run(handles, times, track_map=track_map)
    plain = Launch(context, layout, tracks, n)
    output = runtime.OutputDesc()
    output.layout = plain.layout_id
    context.decompress_tracks_batch_out(plain.device(handles, np.int32).data_ptr(), plain.device(times, np.float32).data_ptr(), n, plain.buffer[GUARD_ROWS:].data_ptr(), plain.stride, output)
    check(mapped.result(), plain.result(), (name, layout))
    values, written = oracle_with_written_mask(clip.blob, times, tracks)
    check(mapped.result(), expected_buffer(layout, mapped.stride // 4, n, values, written, [np.arange(tracks)] * n, tracks), (name, layout, "oracle"))
    assert_rejected(context)
    context.unregister_track_map(track_map)
    context.unregister_clip(handle)


# ---- 2. 100 tracks into 128 slots ----
@pytest.mark.parametrize("layout", ["qvv48", "qvv40", "qv32"])
@pytest.mark.parametrize("fill", [0, 1])
@pytest.mark.parametrize("kind", sorted(MAP_KINDS))
def test_hundred_tracks_into_128_slots(context, kind, fill, layout):
    clip = synth.build_clip(**CLIP_SPECS["cmu_100"])
    handle = context.register_clip(clip.blob)
    rng = np.random.default_rng(len(kind) * 7 + fill * 3 + len(layout))
    table = MAP_KINDS[kind](100, 128, rng)
    track_map = context.register_track_map(table, 128)
    info = context.track_map_info(track_map)
    # (a seeded random permutation of 100 tracks is not sorted by chance; whoever shrinks the case must look again)
    assert info.num_unmapped_slots == 128 - np.count_nonzero(table != DROPPED) and info.is_order_preserving == int(kind == "order_preserving")
    n = 257
    times = rng.uniform(0.0, clip.duration, size=n).astype(np.float32)
    launch = Launch(context, layout, 128, n)
    fill_host, fill_device = launch.fill_pose(rng) if fill else (None, None)
    launch.run(np.full(n, handle, dtype=np.uint32), times, track_map=track_map, fill=fill_device)
    values, written = oracle_with_written_mask(clip.blob, times, 100)
    check(launch.result(), expected_buffer(layout, launch.stride // 4, n, values, written, [table] * n, 128, fill_pose=fill_host), (kind, fill, layout))
    assert_rejected(context)
    context.unregister_track_map(track_map)
    context.unregister_clip(handle)


# ---- 3. every setting that changes the store path, with a non-trivial map ----
def _setting_cases():
    constant, skipped, variable, legacy, bind = ob.DEFAULT_CONSTANT, ob.DEFAULT_SKIPPED, ob.DEFAULT_VARIABLE, ob.DEFAULT_LEGACY, runtime.DEFAULT_BIND_POSE
    cases = {
        "defaults_standard": dict(modes=(constant, constant, legacy)),
        "defaults_skipped": dict(modes=(skipped, skipped, skipped)),
        "defaults_constant_table": dict(modes=(constant, constant, constant), table="constant"),
        "defaults_variable_table": dict(modes=(variable, variable, variable), table="variable"),
        "defaults_bind_pose_mixed": dict(modes=(bind, skipped, bind)),
        "per_track_rounding": dict(per_track=1),
        "normalize_always": dict(normalization=ob.NORMALIZE_ALWAYS),
        "skip_rotations": dict(skip=(1, 0, 0)),
        "skip_translations_and_scales": dict(skip=(0, 1, 1)),
        "skip_tracks": dict(skip_tracks=True),
        "instance_masks": dict(instance_masks=True),
        "instance_track_counts": dict(track_counts=True),
        "rows": dict(rows=True),
    }
    return cases


@pytest.mark.parametrize("layout", ["qvv48", "qvv40", "qv32"])
@pytest.mark.parametrize("setting", sorted(_setting_cases()))
@pytest.mark.parametrize("name", ["raw_and_constant_rates", "cinematic_300"])
def test_settings_keep_their_meaning_per_track(context, name, setting, layout):
    case = _setting_cases()[setting]
    clip = synth.build_clip(**CLIP_SPECS[name])
    handle = context.register_clip(clip.blob)
    tracks = clip.num_tracks
    num_slots = tracks + 24
    rng = np.random.default_rng(len(name) + len(setting) * 5 + len(layout))
    table = dropping_map(tracks, num_slots, rng)
    track_map = context.register_track_map(table, num_slots)
    n = 150
    times = rng.uniform(0.0, clip.duration, size=n).astype(np.float32)
    launch = Launch(context, layout, num_slots, n + (37 if case.get("rows") else 0))
    fill_host, fill_device = launch.fill_pose(rng)

    modes = case.get("modes", (ob.DEFAULT_CONSTANT, ob.DEFAULT_CONSTANT, ob.DEFAULT_LEGACY))
    params = runtime.default_params(default_rotation_mode=modes[0], default_translation_mode=modes[1], default_scale_mode=modes[2],
                                    normalization=case.get("normalization", ob.NORMALIZE_LERP_ONLY), per_track_rounding=case.get("per_track", 0))
    oracle_modes = tuple(ob.DEFAULT_VARIABLE if mode == runtime.DEFAULT_BIND_POSE else mode for mode in modes)
    options = ob.default_options(default_rotation_mode=oracle_modes[0], default_translation_mode=oracle_modes[1], default_scale_mode=oracle_modes[2],
                                 normalization=case.get("normalization", ob.NORMALIZE_LERP_ONLY), per_track_rounding=case.get("per_track", 0))
    rounding = ob.ROUND_NONE
    host_table = None
    if case.get("table") is not None:
        host_table = rng.uniform(-2.0, 2.0, size=(tracks if case["table"] == "variable" else 1, 12)).astype(np.float32)
        host_table[:, [7, 11]] = 0.0
        params.default_values = launch.device(host_table, np.float32).data_ptr()
        options.default_values = host_table.ctypes.data
    if runtime.DEFAULT_BIND_POSE in modes:
        # synthetic clips carry no track descriptions: their bind pose is the identity transform (the variable mode fed that table by hand)
        host_table = np.tile(np.array([0, 0, 0, 1, 0, 0, 0, 0, 1, 1, 1, 0], dtype=np.float32), (tracks, 1))
        options.default_values = host_table.ctypes.data
    if case.get("per_track"):
        policies = rng.integers(0, 4, size=tracks).astype(np.uint8)        # none / floor / ceil / nearest
        params.rounding_policy = ob.ROUND_PER_TRACK
        params.track_rounding_policies = launch.device(policies, np.uint8).data_ptr()
        options.track_rounding = policies.ctypes.data
        rounding = ob.ROUND_PER_TRACK

    values, written = oracle_with_written_mask(clip.blob, times, tracks, options=options, rounding=rounding)
    written = written.copy()
    output = runtime.OutputDesc()
    if case.get("skip"):
        output.skip_rotations, output.skip_translations, output.skip_scales = case["skip"]
        for kind in range(3):
            if case["skip"][kind]:
                written[:, :, KIND_OF_FLOAT == kind] = False
    if case.get("skip_tracks"):
        masks = rng.integers(0, 8, size=tracks).astype(np.uint8)
        output.skip_tracks = launch.device(masks, np.uint8).data_ptr()
        for kind in range(3):
            written[:, ((masks >> kind) & 1) != 0, 4 * kind: 4 * kind + 4] = False
    if case.get("instance_masks"):
        mask_table = rng.integers(0, 8, size=(5, tracks + 3)).astype(np.uint8)
        which = rng.integers(0, 5, size=n).astype(np.uint8)
        output.mask_table = launch.device(mask_table, np.uint8).data_ptr()
        output.mask_stride = mask_table.shape[1]
        output.instance_masks = launch.device(which, np.uint8).data_ptr()
        for i in range(n):
            for kind in range(3):
                written[i, ((mask_table[which[i], :tracks] >> kind) & 1) != 0, 4 * kind: 4 * kind + 4] = False
    if case.get("track_counts"):
        # (counts that cut a pose window, end on one, and exceed the clip)
        counts = rng.choice(np.array([0, 1, tracks // 3, min(tracks, 104), min(tracks, 105), tracks - 1, tracks, tracks + 9]), size=n).astype(np.uint32)
        output.instance_track_counts = launch.device(counts, np.int32).data_ptr()
        for i in range(n):
            written[i, int(counts[i]):] = False
    rows = None
    if case.get("rows"):
        rows = rng.permutation(n + 37)[:n].astype(np.uint32)
        output.rows = launch.device(rows, np.int32).data_ptr()

    launch.run(np.full(n, handle, dtype=np.uint32), times, track_map=track_map, fill=fill_device, output=output, params=params)
    expected = expected_buffer(layout, launch.stride // 4, launch.num_rows, values, written, [table] * n, num_slots, rows=rows, fill_pose=fill_host)
    check(launch.result(), expected, (name, setting, layout))
    assert_rejected(context)
    context.unregister_track_map(track_map)
    context.unregister_clip(handle)


# ---- 4. several windows, grid tails ----
def _corpus_clip(bones):
    return next(clip for clip in helpers.load_corpus() if clip["name"] == f"{137 if bones == 300 else 138}_bones_{bones}")


@pytest.mark.parametrize("layout", ["qvv48", "qvv40", "qv32"])
@pytest.mark.parametrize("n", [1, 63, 64, 65, 3001])
@pytest.mark.parametrize("source", ["rig_300", "corpus_551"])
def test_poses_of_several_windows(context, source, n, layout):
    blob = synth.build_clip(**CLIP_SPECS["cinematic_300"]).blob if source == "rig_300" else _corpus_clip(551)["blob"]
    tracks = ob.oracle().aclo_num_tracks(blob.ctypes.data)
    duration = ob.oracle().aclo_finite_duration(blob.ctypes.data, ob.LOOP_AS_COMPRESSED)
    handle = context.register_clip(blob)
    num_slots = tracks + 117
    table = far_apart_map(tracks, num_slots)
    assert np.abs(np.diff(table.astype(np.int64))).min() >= 104
    track_map = context.register_track_map(table, num_slots)
    rng = np.random.default_rng(n + len(layout))
    times = rng.uniform(0.0, duration, size=n).astype(np.float32)
    launch = Launch(context, layout, num_slots, n)
    fill_host, fill_device = launch.fill_pose(rng)
    launch.run(np.full(n, handle, dtype=np.uint32), times, track_map=track_map, fill=fill_device)
    values, written = oracle_with_written_mask(blob, times, tracks)
    check(launch.result(), expected_buffer(layout, launch.stride // 4, n, values, written, [table] * n, num_slots, fill_pose=fill_host), (source, n, layout))
    assert_rejected(context)
    context.unregister_track_map(track_map)
    context.unregister_clip(handle)


def test_fill_is_complete_whatever_window_count_the_launch_has(context):
    """a 5-track clip in rows as wide as a 551-bone skeleton (six waves per instance, five of them without a window of the clip): every
    unmapped slot is still filled, once"""
    big = context.register_clip(_corpus_clip(551)["blob"])           # (the registry's largest clip: launches of wide rows take six windows)
    clip = synth.build_clip(seed=3, num_tracks=5, num_samples=20)
    handle = context.register_clip(clip.blob)
    num_slots = 600
    rng = np.random.default_rng(8)
    table = permutation_map(5, num_slots, rng)
    track_map = context.register_track_map(table, num_slots)
    n = 70
    times = rng.uniform(0.0, clip.duration, size=n).astype(np.float32)
    for layout in ("qvv48", "qvv40", "qv32"):
        launch = Launch(context, layout, num_slots, n)
        assert context.pose_windows_of_launch(launch.stride, launch.layout_id) == 6
        fill_host, fill_device = launch.fill_pose(rng)
        launch.run(np.full(n, handle, dtype=np.uint32), times, track_map=track_map, fill=fill_device)
        values, written = oracle_with_written_mask(clip.blob, times, 5)
        check(launch.result(), expected_buffer(layout, launch.stride // 4, n, values, written, [table] * n, num_slots, fill_pose=fill_host), layout)
    assert_rejected(context)
    context.unregister_track_map(track_map)
    context.unregister_clip(handle)
    context.unregister_clip(big)


# ---- 5. a mixed batch: a map per clip into one skeleton ----
@pytest.mark.parametrize("layout", ["qvv48", "qvv40", "qv32"])
def test_mixed_batch_with_a_map_per_instance(context, layout):
    case = helpers.load_database_golden("three_clips_4k_chunks")
    database = context.register_database(case["database"], case["bulk_medium"], case["bulk_low"])
    oracle_db = OracleDatabase(case["database"], case["bulk_medium"], case["bulk_low"])
    assert context.database_stream_in(database, 1, 1) == oracle_db.stream_in(1, 1)
    blobs = [synth.build_clip(seed=11, num_tracks=1, num_samples=9).blob, synth.build_clip(**CLIP_SPECS["cmu_70_default"]).blob, synth.build_clip(**CLIP_SPECS["cmu_100"]).blob,
             synth.build_clip(**CLIP_SPECS["cinematic_300"]).blob, synth.build_clip(**CLIP_SPECS["stripped_wrap_scale"]).blob, synth.build_clip(**CLIP_SPECS["stripped"]).blob]
    handles = [context.register_clip(blob) for blob in blobs]
    bound = [context.register_clip_with_database(blob, database) for blob in case["clips"]]
    blobs, handles = blobs + list(case["clips"]), handles + bound
    tracks = [ob.oracle().aclo_num_tracks(blob.ctypes.data) for blob in blobs]
    durations = np.array([ob.oracle().aclo_finite_duration(blob.ctypes.data, ob.LOOP_AS_COMPRESSED) for blob in blobs], dtype=np.float32)
    num_slots = 320
    rng = np.random.default_rng(len(layout))
    tables = [MAP_KINDS[sorted(MAP_KINDS)[index % 3]](tracks[index], num_slots, rng) for index in range(len(blobs))]
    maps = [context.register_track_map(table, num_slots) for table in tables]
    n = 700
    which = rng.integers(0, len(blobs), size=n)
    times = (rng.uniform(0.0, 1.0, size=n) * durations[which]).astype(np.float32)
    values, written = [], []
    for i in range(n):
        blob = blobs[which[i]]
        if which[i] >= len(blobs) - len(bound):
            pose = oracle_db.decompress_tracks(blob, float(times[i]))
        else:
            pose = ob.oracle_decompress_tracks(blob, float(times[i]))
        values.append(pose)
        written.append(np.ones(pose.shape, dtype=bool))
    launch = Launch(context, layout, num_slots, n)
    fill_host, fill_device = launch.fill_pose(rng)
    launch.run(np.array(handles, dtype=np.uint32)[which], times, instance_maps=np.array(maps)[which], fill=fill_device)
    check(launch.result(), expected_buffer(layout, launch.stride // 4, n, values, written, [tables[w] for w in which], num_slots, fill_pose=fill_host), layout)
    assert_rejected(context)
    for track_map in maps:
        context.unregister_track_map(track_map)
    for handle in handles:
        context.unregister_clip(handle)
    context.unregister_database(database)


# ---- 6. refusals ----
def test_refusals_are_counted_once_and_leave_the_row_untouched(context):
    clip = synth.build_clip(**CLIP_SPECS["cmu_100"])
    small = synth.build_clip(**CLIP_SPECS["cmu_70_default"])
    scalar = synth.build_scalar_clip(**helpers.SCALAR_CLIP_SPECS["float1f_all_rates"])
    handle, small_handle, scalar_handle = context.register_clip(clip.blob), context.register_clip(small.blob), context.register_clip(scalar.blob)
    scalar_tracks = context.clip_info(scalar_handle).num_tracks
    rng = np.random.default_rng(4)
    num_slots = 128
    table = order_preserving_map(100, num_slots, rng)
    good = context.register_track_map(table, num_slots)
    retired = context.register_track_map(permutation_map(100, num_slots, rng), num_slots)
    context.unregister_track_map(retired)
    torch.cuda.synchronize()
    for_70 = context.register_track_map(order_preserving_map(70, num_slots, rng), num_slots)
    for_scalar = context.register_track_map(np.arange(scalar_tracks), max(scalar_tracks, 1))
    too_wide = context.register_track_map(order_preserving_map(100, 4000, rng), 4000)            # 4000 records do not fit the stride
    n = 40
    handles = np.full(n, handle, dtype=np.uint32)
    maps = np.full(n, good, dtype=np.uint32)
    refused = {3: 0, 7: 0xFFFFFFFF, 11: runtime.MAX_TRACK_MAPS, 12: runtime.MAX_TRACK_MAPS - 1, 15: retired, 19: for_70, 23: too_wide, 31: for_scalar}
    for index, value in refused.items():
        maps[index] = value
    handles[31] = scalar_handle                                     # a scalar clip, with a map of its own track count
    handles[35], maps[35] = small_handle, good                      # the map of ANOTHER clip's track count
    refused[35] = good
    times = rng.uniform(0.0, small.duration, size=n).astype(np.float32)
    for layout in ("qvv48", "qvv40", "qv32"):
        launch = Launch(context, layout, num_slots, n)
        fill_host, fill_device = launch.fill_pose(rng)
        launch.run(handles, times, instance_maps=maps, fill=fill_device)
        values, written = oracle_with_written_mask(clip.blob, times, 100)
        expected = expected_buffer(layout, launch.stride // 4, n, values, written, [table] * n, num_slots, fill_pose=fill_host, refused=set(refused))
        check(launch.result(), expected, layout)
        assert_rejected(context, len(refused))
    # host side refusals
    launch = Launch(context, "qvv48", num_slots, n)
    d_handles, d_times = launch.device(handles, np.int32), launch.device(times, np.float32)
    lib, params = runtime.load_library(), runtime.default_params()
    call = lambda mapping: lib.aclhip_decompress_tracks_batch_mapped(context._handle, d_handles.data_ptr(), d_times.data_ptr(), n, ctypes.byref(params), None, mapping, launch.buffer[GUARD_ROWS:].data_ptr(), launch.stride, None)
    assert call(None) == runtime.ERROR_INVALID_ARGUMENT
    assert call(ctypes.byref(runtime.TrackMapping())) == runtime.ERROR_INVALID_ARGUMENT                       # a null map handle
    no_fill_pose = runtime.TrackMapping()
    no_fill_pose.map, no_fill_pose.fill_unmapped = good, 1
    assert call(ctypes.byref(no_fill_pose)) == runtime.ERROR_INVALID_ARGUMENT
    check(launch.result(), np.full_like(launch.result(), SENTINEL), "host side refusals write nothing")
    for track_map in (good, for_70, for_scalar, too_wide):
        context.unregister_track_map(track_map)
    with pytest.raises(runtime.AclHipError):
        context.unregister_track_map(good)
    for clip_handle in (handle, small_handle, scalar_handle):
        context.unregister_clip(clip_handle)


# ---- 7. lifetime ----
def test_unregistering_a_map_behind_an_enqueued_decode(context):
    clip = synth.build_clip(**CLIP_SPECS["cmu_100"])
    handle = context.register_clip(clip.blob)
    rng = np.random.default_rng(12)
    table = permutation_map(100, 128, rng)
    track_map = context.register_track_map(table, 128)
    n = 20000
    times = rng.uniform(0.0, clip.duration, size=n).astype(np.float32)
    handles = np.full(n, handle, dtype=np.uint32)
    first, second = Launch(context, "qvv48", 128, n), Launch(context, "qvv48", 128, n)
    d_handles, d_times = first.device(handles, np.int32), first.device(times, np.float32)
    torch.cuda.synchronize()
    stream = torch.cuda.current_stream().cuda_stream
    context.decompress_tracks_batch_mapped(d_handles, d_times, first.buffer[GUARD_ROWS:], first.stride, track_map=track_map, stream=stream)
    context.unregister_track_map(track_map)                     # the decode above is still enqueued or running
    values, written = oracle_with_written_mask(clip.blob, times, 100)
    check(first.result(), expected_buffer("qvv48", first.stride // 4, n, values, written, [table] * n, 128), "the decode enqueued before the unregistration")
    torch.cuda.synchronize()
    context.decompress_tracks_batch_mapped(d_handles, d_times, second.buffer[GUARD_ROWS:], second.stride, track_map=track_map, stream=stream)
    check(second.result(), np.full_like(second.result(), SENTINEL), "a decode after the unregistration")
    assert_rejected(context, n)
    context.unregister_clip(handle)


def test_maps_come_and_go_on_one_thread_while_another_decodes(context):
    clip = synth.build_clip(**CLIP_SPECS["cmu_100"])
    handle = context.register_clip(clip.blob)
    rng = np.random.default_rng(13)
    table = dropping_map(100, 128, rng)
    track_map = context.register_track_map(table, 128)
    n = 512
    times = rng.uniform(0.0, clip.duration, size=n).astype(np.float32)
    values, written = oracle_with_written_mask(clip.blob, times, 100)
    expected = expected_buffer("qvv48", (128 * 48 + 64) // 4, n, values, written, [table] * n, 128)
    stop, errors = threading.Event(), []

    def churn():
        try:
            local = np.random.default_rng(14)
            while not stop.is_set():
                handles = [context.register_track_map(permutation_map(60, 90, local), 90) for _ in range(8)]
                for other in handles:
                    context.unregister_track_map(other)
        except Exception as error:      # noqa: BLE001 (reported by the main thread)
            errors.append(error)

    thread = threading.Thread(target=churn)
    thread.start()
    try:
        stream = torch.cuda.Stream()
        with torch.cuda.stream(stream):
            for _ in range(40):
                launch = Launch(context, "qvv48", 128, n)
                launch.run(np.full(n, handle, dtype=np.uint32), times, track_map=track_map, stream=stream.cuda_stream)
                stream.synchronize()
                check(launch.result(), expected, "decode next to map churn")
    finally:
        stop.set()
        thread.join()
    assert not errors, errors
    assert_rejected(context)
    context.unregister_track_map(track_map)
    context.unregister_clip(handle)


def test_captured_graph_survives_other_maps_coming_and_going(context):
    clip = synth.build_clip(**CLIP_SPECS["cmu_100"])
    handle = context.register_clip(clip.blob)
    rng = np.random.default_rng(15)
    table = order_preserving_map(100, 128, rng)
    track_map = context.register_track_map(table, 128)
    n = 300
    times = rng.uniform(0.0, clip.duration, size=n).astype(np.float32)
    launch = Launch(context, "qvv40", 128, n)
    fill_host, fill_device = launch.fill_pose(rng)
    d_handles, d_times = launch.device(np.full(n, handle), np.int32), launch.device(times, np.float32)
    output = runtime.OutputDesc()
    output.layout = launch.layout_id
    stream = torch.cuda.Stream()
    graph = torch.cuda.CUDAGraph()
    torch.cuda.synchronize()
    with torch.cuda.graph(graph, stream=stream):
        context.decompress_tracks_batch_mapped(d_handles, d_times, launch.buffer[GUARD_ROWS:], launch.stride, track_map=track_map, fill_pose=fill_device, output=output,
                                               stream=torch.cuda.current_stream().cuda_stream)
    others = [context.register_track_map(permutation_map(100, 128, rng), 128) for _ in range(300)]
    for other in others[::2]:
        context.unregister_track_map(other)
    torch.cuda.synchronize()
    more = [context.register_track_map(permutation_map(33, 128, rng), 128) for _ in range(100)]
    values, written = oracle_with_written_mask(clip.blob, times, 100)
    expected = expected_buffer("qvv40", launch.stride // 4, n, values, written, [table] * n, 128, fill_pose=fill_host)
    for _ in range(2):
        launch.buffer.fill_(float(SENTINEL))
        graph.replay()
        check(launch.result(), expected, "replayed graph")
    assert_rejected(context)
    for other in others[1::2] + more + [track_map]:
        context.unregister_track_map(other)
    context.unregister_clip(handle)


# ---- 8. the real-compressor corpus, every sample x every bone, a random map per clip ----
def test_corpus_slice_through_random_maps(context):
    corpus = helpers.load_corpus()
    rng = np.random.default_rng(16)
    for index in range(0, len(corpus), 5):
        clip = corpus[index]
        blob = clip["blob"]
        tracks = ob.oracle().aclo_num_tracks(blob.ctypes.data)
        times, _ = helpers.corpus_sample_times(blob)
        handle = context.register_clip(blob)
        num_slots = tracks + int(rng.integers(0, 40))
        table = MAP_KINDS[sorted(MAP_KINDS)[index % 3]](tracks, num_slots, rng)
        track_map = context.register_track_map(table, num_slots)
        layout = ("qvv48", "qvv40", "qv32")[(index // 5) % 3]
        launch = Launch(context, layout, num_slots, times.size)
        fill_host, fill_device = launch.fill_pose(rng)
        launch.run(np.full(times.size, handle, dtype=np.uint32), times, track_map=track_map, fill=fill_device)
        values, written = oracle_with_written_mask(blob, times, tracks)
        check(launch.result(), expected_buffer(layout, launch.stride // 4, times.size, values, written, [table] * times.size, num_slots, fill_pose=fill_host), clip["name"])
        context.unregister_track_map(track_map)
        context.unregister_clip(handle)
    assert_rejected(context)
