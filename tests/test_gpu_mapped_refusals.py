"""What every skeleton space launch refuses, through the launches whose own tests only meet their mask handles: the clip / map / skeleton
case table of test_gpu_skeleton_poses.py::test_refusals_inside_an_otherwise_valid_batch -- good, garbage, zero and retired handles, a map
of another track count, a map into another slot count, a skeleton without a hierarchy, a skeleton larger than the row, a scalar clip --
through aclhip_decompress_poses_batch_masked (every mask handle 0), aclhip_decompress_poses_batch_additive_weighted (weights 1, null
handles: fused, second wave, base buffer with a blend) and aclhip_decompress_poses_batch_bounds (mapped, and mapped with a masking), with
instances whose blend partner's or base clip's map is wrong behind the table. Served rows and guard rows are the oracle's bits, refused
rows (and boxes) keep the sentinel, and the context's count of rejected instances rises by exactly the refused ones. Needs a GPU."""
import functools

import numpy as np
import pytest

from acl_amd import runtime, synth
import helpers
import test_gpu_skeleton_poses as sk
import test_gpu_blend_masks as bm
import test_gpu_additive_strength as ad
import test_gpu_pose_bounds as pb

pytestmark = pytest.mark.gpu

NONE, RELATIVE, ADDITIVE0, ADDITIVE1 = sk.NONE, sk.RELATIVE, sk.ADDITIVE0, sk.ADDITIVE1
NUM_BONES = 48
GARBAGE = 0xFFFFFFFF

#   clip        map        skeleton    refused: always, never, or in object space alone (no hierarchy to walk)
TABLE = [("clip", "clip", "skeleton", "never"), ("clip", "garbage", "skeleton", "always"), ("clip", "clip", "garbage", "always"), ("other", "other", "skeleton", "never"),
         ("clip", "retired", "skeleton", "always"), ("clip", "clip", "retired", "always"), ("clip", "other", "skeleton", "always"),     # a map of another track count
         ("clip", "small", "skeleton", "always"),                                                                              # a map into another slot count
         ("garbage", "clip", "skeleton", "always"), ("clip", "clip", "flat", "object space"),                                   # unknown clip; no hierarchy
         ("clip", "big", "big", "always"),                                                                                     # 48 B > stride
         ("clip", "zero", "skeleton", "always"), ("clip", "clip", "zero", "always"), ("other", "other", "skeleton", "never"),
         ("scalars", "other", "skeleton", "always"), ("clip", "clip", "skeleton", "never")]                                     # a scalar clip, and a last good neighbour
# behind the table: good instances whose second clip (a blend partner, a base clip) names a map of another track count, an unknown and a
# retired map, and a good neighbour (None: the second clip's own map)
SECOND_MAPS = [None] * len(TABLE) + ["other clip's", "garbage", "retired", None]
CASES = TABLE + [("clip", "clip", "skeleton", "never")] * 4
N = len(CASES)
assert len(TABLE) == 16 and len(SECOND_MAPS) == N


@functools.lru_cache(maxsize=None)
def rig():
    """host data, built once: the 37 track scaled clip, the 12 track clip, the scalar clip, their tables, the skeleton, the sample times"""
    rng = np.random.default_rng(95)
    clip, other = synth.build_clip(seed=995, **sk.SHAPES["scaled_37"]), synth.build_clip(seed=996, **sk.SHAPES["small_12"])
    scalars = synth.build_scalar_clip(seed=997, num_tracks=12, num_samples=25)
    reference, parents = sk.reference_pose(rng, NUM_BONES), sk.hierarchy(rng, NUM_BONES)
    table, other_table = sk.make_map(rng, 37, NUM_BONES, "permutation"), sk.make_map(rng, 12, NUM_BONES, "ordered")
    big = (sk.reference_pose(rng, NUM_BONES + 8), sk.hierarchy(rng, NUM_BONES + 8), sk.make_map(rng, 37, NUM_BONES + 8, "ordered"))
    times, second_times = rng.uniform(0.0, 0.3, size=N).astype(np.float32), rng.uniform(0.0, 0.3, size=N).astype(np.float32)
    weights = np.array([[0.25, 0.75]] * N, dtype=np.float32)
    base_buffer = np.stack([sk.reference_pose(rng, NUM_BONES) for _ in range(N)])
    return dict(clip=clip, other=other, scalars=scalars, reference=reference, parents=parents, table=table, other_table=other_table, big=big,
                times=times, second_times=second_times, weights=weights, base_buffer=base_buffer)


class Registry:
    """the rig registered with one context: handles by the names the case table uses"""

    def __init__(self, ctx):
        import torch
        r = rig()
        self.clips = {"clip": ctx.register_clip(r["clip"].blob), "other": ctx.register_clip(r["other"].blob), "scalars": ctx.register_clip(r["scalars"].blob), "garbage": GARBAGE}
        assert ctx.clip_info(self.clips["scalars"]).num_tracks == 12                      # a scalar track list with the track count of the "other" map
        big_reference, big_parents, big_table = r["big"]
        self.maps = {"clip": ctx.register_track_map(r["table"], NUM_BONES), "other": ctx.register_track_map(r["other_table"], NUM_BONES),
                     "small": ctx.register_track_map(np.arange(37, dtype=np.uint32), 40),  # made for a skeleton of 40 bones
                     "retired": ctx.register_track_map(r["table"], NUM_BONES), "big": ctx.register_track_map(big_table, NUM_BONES + 8), "garbage": GARBAGE, "zero": 0}
        self.skeletons = {"skeleton": ctx.register_skeleton(r["parents"], r["reference"]), "flat": ctx.register_skeleton(None, r["reference"]),
                          "big": ctx.register_skeleton(big_parents, big_reference), "retired": ctx.register_skeleton(r["parents"], r["reference"]), "garbage": GARBAGE, "zero": 0}
        ctx.unregister_track_map(self.maps["retired"])
        ctx.unregister_skeleton(self.skeletons["retired"])
        torch.cuda.synchronize()

    def fill(self, batch, second=None):
        """the table's per instance skeletons and maps into batch.mapping (sk.Batch or pb.Case); second: "blend" or "base" -- the second clip
        of every instance (the 12 track clip as a blend partner, the 37 track clip as a base clip) with its map, or SECOND_MAPS' wrong one.
        Returns the instances' clip handles."""
        r = rig()
        batch.mapping.instance_skeletons = batch.up([self.skeletons[c[2]] for c in CASES], np.uint32)
        batch.mapping.instance_maps = batch.up([self.maps[c[1]] for c in CASES], np.uint32)
        name = "other" if second == "blend" else "clip"
        own, wrong = self.maps[name], self.maps["clip" if second == "blend" else "other"]
        second_maps = [own if m is None else (wrong if m == "other clip's" else self.maps[m]) for m in SECOND_MAPS]
        if second == "blend":
            batch.consumers.num_blend_clips = 2
            batch.consumers.blend_clips, batch.consumers.blend_sample_times = batch.up(np.full(N, self.clips[name]), np.uint32), batch.up(r["second_times"], np.float32)
            batch.consumers.blend_weights, batch.mapping.blend_maps = batch.up(r["weights"], np.float32), batch.up(second_maps, np.uint32)
        if second == "base":
            batch.consumers.base_clips, batch.consumers.base_sample_times = batch.up(np.full(N, self.clips[name]), np.uint32), batch.up(r["second_times"], np.float32)
            batch.mapping.base_maps = batch.up(second_maps, np.uint32)
        return np.array([self.clips[c[0]] for c in CASES], dtype=np.uint32)


def refused(object_space, second):
    """per instance: does the launch refuse it?"""
    return [verdict == "always" or (verdict == "object space" and object_space) or (second is not None and SECOND_MAPS[i] is not None)
            for i, (_, _, _, verdict) in enumerate(CASES)]


@functools.lru_cache(maxsize=None)
def oracle_rows(additive_format, object_space, second, base_as_buffer=False):
    """the mapped launch's rows from the oracle, None for a refused instance; computed once per form and never written to"""
    r = rig()
    blobs, tables = {"clip": r["clip"].blob, "other": r["other"].blob}, {"clip": r["table"], "other": r["other_table"]}
    rows = []
    for i, ((clip, _, _, _), refuse) in enumerate(zip(CASES, refused(object_space, second))):
        if refuse:
            rows.append(None)
            continue
        members = [(blobs[clip], r["times"][i], tables[clip])] + ([(blobs["other"], r["second_times"][i], tables["other"])] if second == "blend" else [])
        base = r["base_buffer"][i] if base_as_buffer else (blobs["clip"], r["second_times"][i], tables["clip"])
        rows.append(sk.expected_pose((r["reference"], r["parents"]), members, r["weights"][i], additive_format, base, object_space, 0, 2))
    return tuple(rows)


def count(rows):
    return sum(1 for row in rows if row is None)


def test_the_table_is_what_it_says():
    assert count(oracle_rows(NONE, True, None)) == 12 and count(oracle_rows(NONE, True, "blend")) == 15 and count(oracle_rows(RELATIVE, False, "base")) == 14


def test_masked_launch_with_every_mask_handle_null():
    """K = 2, object space: served rows are the plain blend's bits"""
    with runtime.Context(0) as ctx:
        registry = Registry(ctx)
        batch = bm.MaskedBatch(ctx, N, NUM_BONES)
        batch.consumers.object_space = 1
        clips = registry.fill(batch, "blend")
        batch.masking.mode, batch.masking.instance_masks = runtime.BLEND_WEIGHTED, batch.up(np.zeros((N, 2)), np.uint32)
        rows = oracle_rows(NONE, True, "blend")
        before = ctx.rejected_instance_count()
        got = batch.launch(clips, rig()["times"]).result()
        assert helpers.exact(got, batch.expected(rows))
        assert ctx.rejected_instance_count() - before == count(rows)


@pytest.mark.parametrize("additive_format,object_space,second,base_as_buffer", [
    (ADDITIVE1, True, "base", False),       # onto a base clip, one wave: the fused instantiation
    (RELATIVE, False, "base", False),       # onto a base clip in local space: a second wave
    (ADDITIVE0, True, "blend", True),       # a blend of two onto a base pose buffer
])
def test_additive_weighted_launch_at_full_strength(additive_format, object_space, second, base_as_buffer):
    """weights 1, null handles: served rows are the mapped launch's oracle rows"""
    with runtime.Context(0) as ctx:
        registry = Registry(ctx)
        batch = ad.WeightedBatch(ctx, N, NUM_BONES)
        batch.consumers.additive_format, batch.consumers.object_space = additive_format, int(object_space)
        clips = registry.fill(batch, second)
        if base_as_buffer:
            batch.consumers.base_poses, batch.consumers.base_pose_stride_bytes = batch.up(rig()["base_buffer"], np.float32), NUM_BONES * 48
        batch.layering.instance_weights, batch.layering.instance_masks = batch.up(np.ones(N), np.float32), batch.up(np.zeros(N), np.uint32)
        rows = oracle_rows(additive_format, object_space, second, base_as_buffer)
        before = ctx.rejected_instance_count()
        got = batch.launch(clips, rig()["times"]).result()
        assert helpers.exact(got, batch.expected(rows))
        assert ctx.rejected_instance_count() - before == count(rows)


@pytest.mark.parametrize("masked", [False, True])
def test_bounds_launch_with_a_mapping(masked):
    """a refused instance leaves both its row and its box at the sentinel, with and without rows"""
    with runtime.Context(0) as ctx:
        registry = Registry(ctx)
        case = pb.Case(ctx, NUM_BONES)
        case.mapping = runtime.PoseMapping()
        clips = registry.fill(case, "blend" if masked else None)
        if masked:
            case.masking = runtime.BlendMasking()
            case.masking.mode, case.masking.instance_masks = runtime.BLEND_WEIGHTED, case.up(np.zeros((N, 2)), np.uint32)
        rows = oracle_rows(NONE, True, "blend" if masked else None)
        expected = np.full((N + 2, case.row_floats), sk.SENTINEL, dtype=np.float32)
        served = np.zeros((N, NUM_BONES, 12), dtype=np.float32)
        for i, row in enumerate(rows):
            if row is not None:
                expected[1 + i, : row.size], served[i] = row.reshape(-1), row
        boxes_expected = pb.expected_bounds(served, [NUM_BONES] * N, None, refused=[i for i, row in enumerate(rows) if row is None])
        for with_rows in (True, False):
            before = ctx.rejected_instance_count()
            poses, boxes = case.launch_bounds(clips, rig()["times"], None, with_rows)
            assert helpers.exact(poses, expected if with_rows else np.full_like(expected, sk.SENTINEL)), with_rows
            assert np.array_equal(boxes, boxes_expected), with_rows          # (compared as test_gpu_pose_bounds.py compares boxes)
            assert ctx.rejected_instance_count() - before == count(rows), with_rows
