"""aclhip_compress_tracks_batch through the C ABI: compress_track_list with quatf_drop_w_full rotations -- the rigid shell, the looping
vote, constant and default rotations by the error metric -- of registered raw track arrays. The expected blobs, results and shells are
the restatement's (tests/lossy_rotation_compress_restatement.py, which tests/test_lossy_rotation_compress_oracle.py holds to the
reference's compressor), and every comparison is on BYTES and BITS: both sides follow one definition, nothing has a tolerance.

The output region is one flat buffer filled with a sentinel byte: a guard, n rows of `stride` bytes, a guard. One comparison holds
[0, size) of every row to the blob and everything else -- the bytes behind `size`, refused rows, the guards -- to the sentinel; the
shell metadata likewise. The sample rate is a power of two, so that the key times i / rate are exact. Needs a GPU."""
import numpy as np
import pytest

from acl_amd import runtime
from oracle import bindings as ob
import compress_launches as launches
import lossy_rotation_compress_restatement as restatement
import transform_compress_restatement as raw_restatement
from compress_launches import GUARD, PRECISION, RATE, SENTINEL, SHELL, Entry, Registered, check_rows, ctx, same  # noqa: F401  (ctx: this module's fixture)
from lossy_rotation_compress_restatement import ANIMATED, CONSTANT, DEFAULT, IDENTITY, LANES, NO_PARENT, OPTIMIZE_LOOPS

pytestmark = pytest.mark.gpu

PARENTS, DESCRIPTIONS = restatement.INCLUDE_PARENT_TRACK_INDICES, restatement.INCLUDE_TRACK_DESCRIPTIONS
# T: the wave edges of the layout's passes of 64 tracks and the 16 tracks of a packed word; S: the wave edges of the sample reductions,
# and S' = 1 behind a vote
SHAPES = [(1, 1), (2, 2), (17, 3), (64, 64), (65, 65), (130, 129), (2, 129), (130, 2), (17, 64), (64, 3), (65, 1), (1, 65)]
MAX_TRACKS = 130
TREES = ("chain", "star", "two_roots")


def launch(ctx, handles, entry=Entry("tracks"), max_tracks=MAX_TRACKS, max_samples=129, **settings):
    """One launch over `handles` (tests/compress_launches.py); rows of the bound of (max_tracks, max_samples) unless `stride` says otherwise"""
    return launches.launch(ctx, entry, handles, max_tracks, max_samples, **settings)


def sweep_clips():
    """one array per shape; every second one ends on its first sample; an array of a deep chain keeps every scale the default"""
    return [restatement.clip(k % 3, num_samples, num_tracks, scales="default" if num_tracks > 17 else "mixed", close_loop=k % 2 == 1) for k, (num_tracks, num_samples) in enumerate(SHAPES)]


def sweep_expected(clips, shape, flags=0):
    parents = restatement.tree(0, MAX_TRACKS, shape)
    return parents, [restatement.compress(samples, RATE, parents=parents, flags=flags, precision=PRECISION, shell_distance=SHELL) for samples in clips]


@pytest.fixture(scope="module")
def sweep(ctx):
    """every shape registered once, and the restatement of every tree with the loops on -- computed once, shared and left unchanged"""
    with Registered(ctx) as arrays:
        clips = sweep_clips()
        handles = [arrays.add(samples) for samples in clips]
        expected = {shape: sweep_expected(clips, shape, OPTIMIZE_LOOPS) for shape in TREES}
        yield ctx, handles, clips, expected


@pytest.mark.parametrize("shape", TREES)
def test_the_blobs_results_and_shells_are_the_restatement(sweep, shape):
    """mixed shapes and repeated handles in one launch, the loops on: every byte of [0, size) with the hash, the sentinel behind, the
    results, the shell metadata on bits"""
    ctx, handles, clips, expected = sweep
    parents, compressed = expected[shape]
    order = [(5 * i + 2) % len(handles) for i in range(len(handles) + 7)]
    check_rows(launch(ctx, [handles[k] for k in order], flags=OPTIMIZE_LOOPS, parents=parents), [compressed[k] for k in order])
    if shape == "chain":
        assert any(c.wrap and c.num_samples == 1 for c in compressed) and any(not c.wrap for c in compressed)        # S' = 1 behind a vote
        kinds = np.concatenate([c.types[0] for c in compressed])
        assert {DEFAULT, CONSTANT, ANIMATED} == set(kinds.tolist())
        assert max(float(c.shells[:, 0].max()) for c in compressed) > 20.0                                             # the shell climbed the chain


def test_loops_off_metadata_and_tables(sweep):
    """without the flag nothing is voted; parent indices and descriptions in the blob; a default pose that is not the identity, per-track
    precisions and shell distances; no shell metadata asked for"""
    ctx, handles, clips, _ = sweep
    parents, compressed = sweep_expected(clips, "star")
    check_rows(launch(ctx, handles, parents=parents), compressed)
    assert not any(c.wrap for c in compressed)
    pose = raw_restatement.bind_pose(21, MAX_TRACKS)
    precisions = np.linspace(0.002, 0.05, MAX_TRACKS).astype(np.float32)
    shells = np.linspace(1.0, 5.0, MAX_TRACKS).astype(np.float32)
    parents = restatement.tree(3, MAX_TRACKS)
    flags = PARENTS | DESCRIPTIONS | OPTIMIZE_LOOPS
    compressed = [restatement.compress(samples, RATE, default_pose=pose, parents=parents, flags=flags, track_precisions=precisions, track_shell_distances=shells) for samples in clips]
    out = launch(ctx, handles, flags=flags, default_pose=pose, parents=parents, track_precisions=precisions, track_shell_distances=shells)
    check_rows(out, compressed)
    check_rows(launch(ctx, handles, flags=flags, default_pose=pose, parents=parents, track_precisions=precisions, track_shell_distances=shells, with_metadata=False),
          [c.blob for c in compressed])
    # no table at all: every track a root of its own shell
    check_rows(launch(ctx, handles[:4], flags=PARENTS), [restatement.compress(samples, RATE, flags=PARENTS, precision=PRECISION, shell_distance=SHELL) for samples in clips[:4]])


def test_rotation_format_0_is_the_raw_call(sweep):
    """quatf_full through the new call: aclhip_compress_raw_tracks_batch byte for byte on the same batch, its statuses included"""
    ctx, handles, clips, _ = sweep
    parents = restatement.tree(0, MAX_TRACKS, "chain")
    with Registered(ctx) as arrays:
        long = clips[2].copy()
        long[1, 3, 0:4] *= np.float32(1.5)              # ACLHIP_COMPRESS_NOT_NORMALIZED there, normalized here
        bad = clips[2].copy()
        bad[0, 1, 5] = np.inf
        batch = handles + [arrays.add(long), arrays.add(bad), 0, handles[0]]
        for flags in (0, OPTIMIZE_LOOPS | PARENTS | DESCRIPTIONS):
            new = launch(ctx, batch, rotation_format=runtime.ROTATION_QUATF_FULL, flags=flags, parents=parents)
            old = launch(ctx, batch, Entry("raw"), flags=flags, parents=parents)
            assert np.array_equal(new.flat, old.flat) and np.array_equal(new.results, old.results) and new.rejected == old.rejected == 1
            assert np.all(new.metadata == SENTINEL)
            assert new.results[len(handles)].tolist() == [runtime.COMPRESS_NOT_NORMALIZED, 0] and new.results[len(handles) + 1].tolist() == [runtime.COMPRESS_NOT_FINITE, 0]
            assert new.results[0, 0] == runtime.COMPRESS_OK and np.array_equal(new.flat[GUARD: GUARD + new.results[0, 1]], raw_restatement.compress(clips[0], RATE, parents=parents, flags=flags, precision=PRECISION, shell_distance=SHELL))
        # and the drop-w call takes the rotation of length 1.5
        expected = restatement.compress(long, RATE, parents=parents, precision=PRECISION, shell_distance=SHELL)
        assert np.array_equal(expected.blob, restatement.compress(clips[2], RATE, parents=parents, precision=PRECISION, shell_distance=SHELL).blob)
        check_rows(launch(ctx, [batch[len(handles)]], parents=parents), [expected])


def shell_error_of_poses(shells, registered, decoded):
    """the restatement's shell_error(local_b, registered sample, decoded sample) per track: float32 [T]"""
    return np.array([restatement.shell_error(shells[b, 0], (registered[b, 0:4], registered[b, 4:7], registered[b, 8:11]), (decoded[b, 0:4], decoded[b, 4:7], decoded[b, 8:11]))
                     for b in range(registered.shape[0])], dtype=np.float32)


def test_the_blobs_check_register_and_decode(sweep):
    """each blob of runtime.compress_tracks passes aclhip_check_clip with the hash, registers, and decodes at every key time with
    ROUND_FLOOR and NORMALIZE_NEVER to the bits oracle_decompress_tracks gives for the same blob; translations and scales are the
    registered key frames bit for bit; a rotation that became constant or default is within its shell's precision of the registered
    sample at its shell, by the restatement's shell_error"""
    ctx, handles, clips, expected = sweep
    parents, compressed = expected["chain"]
    blobs = runtime.compress_tracks(ctx, handles, parents=parents, precision=PRECISION, shell_distance=SHELL, optimize_loops=True)
    options = ob.default_options(normalization=ob.NORMALIZE_NEVER)
    params = runtime.default_params(rounding_policy=runtime.ROUND_FLOOR, looping_policy=runtime.LOOP_AS_COMPRESSED, normalization=runtime.NORMALIZE_NEVER)
    checked = 0
    for blob, want, samples in zip(blobs, compressed, clips):
        assert blob.ctypes.data % 16 == 0 and np.array_equal(blob, want.blob)
        assert restatement.decisions_are_clear(want)
        status, message = runtime.check_clip(blob, check_hash=True)
        assert status == 0, message
        clip = ctx.register_clip(blob)
        try:
            info = ctx.clip_info(clip)
            assert (info.num_tracks, info.num_samples) == (samples.shape[1], want.num_samples)
            times = (np.arange(want.num_samples) / RATE).astype(np.float32)
            poses = ctx.decompress_tracks(np.full(len(times), clip, dtype=np.uint32), times, params=params)
        finally:
            ctx.unregister_clip(clip)
        kept = want.types[0] != ANIMATED
        for key, time in enumerate(times):
            by_oracle = ob.oracle_decompress_tracks(blob, float(time), ob.ROUND_FLOOR, options=options)
            for lanes in LANES:
                assert np.array_equal(poses[key][:, lanes].view(np.uint32), by_oracle[:, lanes].view(np.uint32)), key
            for kind in (1, 2):
                stored = want.types[kind] != DEFAULT
                assert np.array_equal(poses[key][stored][:, LANES[kind]].view(np.uint32), samples[key][stored][:, LANES[kind]].view(np.uint32))
                assert (poses[key][~stored][:, LANES[kind]] == samples[key][~stored][:, LANES[kind]]).all()
            errors = shell_error_of_poses(want.shells, samples[key], poses[key])
            assert (errors[kept] <= want.shells[kept, 1]).all(), (key, errors[kept].max())
            checked += int(kept.sum())
    assert checked > 100


def test_the_vote_is_the_whole_list_or_nothing(ctx):
    """all tracks loop: the last sample goes; all loop but one, whose last sample is 0.05 away at its shell: it stays"""
    samples = restatement.clip(1, 9, 17, close_loop=True)
    apart = samples.copy()
    apart[-1, 11, 4] += np.float32(0.05)
    parents = restatement.tree(2, 17)
    with Registered(ctx) as arrays:
        handles = [arrays.add(samples), arrays.add(apart), arrays.add(samples, runtime.LOOP_WRAP)]
        expected = [restatement.compress(samples, RATE, parents=parents, flags=OPTIMIZE_LOOPS, precision=PRECISION, shell_distance=SHELL),
                    restatement.compress(apart, RATE, parents=parents, flags=OPTIMIZE_LOOPS, precision=PRECISION, shell_distance=SHELL),
                    restatement.compress(samples, RATE, parents=parents, flags=OPTIMIZE_LOOPS, precision=PRECISION, shell_distance=SHELL, looping_wrap=True)]
        assert [(c.wrap, c.num_samples) for c in expected] == [(True, 8), (False, 9), (True, 9)]
        check_rows(launch(ctx, handles, max_tracks=17, max_samples=9, flags=OPTIMIZE_LOOPS, parents=parents), expected)


def test_statuses_and_refusals_leave_their_rows(ctx):
    """not finite (a NaN lane, an infinity, a zero quaternion); a parent at or behind its child; an unknown handle, 0, a retired handle;
    more tracks than max_tracks; a table shorter than T; a stride one step too small -- each with its row and its shell metadata
    untouched, size 0, and one count where it is a refusal; the neighbours are served"""
    small, large = restatement.clip(0, 12, 4), restatement.clip(1, 12, 9)
    parents = restatement.tree(4, 9)
    settings = {"precision": PRECISION, "shell_distance": SHELL}
    refused, not_finite = runtime.COMPRESS_REFUSED, runtime.COMPRESS_NOT_FINITE
    with Registered(ctx) as arrays:
        h_small, h_large = arrays.add(small), arrays.add(large)
        c_small, c_large = restatement.compress(small, RATE, parents=parents, **settings), restatement.compress(large, RATE, parents=parents, **settings)
        bad = []
        for lane, value in ((0, np.nan), (3, np.inf), (4, -np.inf), (6, np.nan), (8, np.inf), (10, np.nan)):
            samples = large.copy()
            samples[11 if lane % 2 else 0, 8 if lane % 3 else 0, lane] = value
            bad.append(arrays.add(samples))
        samples = large.copy()
        samples[5, 7, 0:4] = 0.0                                # a zero quaternion: 0 * (1 / 0) is not finite
        bad.append(arrays.add(samples))
        handles = [h_small] + bad + [h_large]
        check_rows(launch(ctx, handles, max_tracks=9, max_samples=12, parents=parents), [c_small] + [not_finite] * len(bad) + [c_large])
        with pytest.raises(RuntimeError, match="Some samples are not finite"):
            runtime.compress_tracks(ctx, [h_small, bad[-1]], parents=parents)

        # a parent at its child, behind its child; a parent that is no track of the SMALL array is no parent there
        for forward in ([NO_PARENT, 0, 2, 0, 0, 1, 2, 3, 4], [NO_PARENT, 0, 1, 2, 3, 4, 5, 8, 0], [NO_PARENT, 0, 1, 2, 6, 0, 0, 0, 0]):
            table = np.array(forward, dtype=np.uint32)
            small_ok = not any(b <= p < 4 for b, p in enumerate(forward[:4]))
            check_rows(launch(ctx, [h_small, h_large, h_small], max_tracks=9, max_samples=12, parents=table),
                  [restatement.compress(small, RATE, parents=table, **settings) if small_ok else refused, refused,
                   restatement.compress(small, RATE, parents=table, **settings) if small_ok else refused])
        with pytest.raises(ValueError, match="ACLHIP_COMPRESS_REFUSED"):
            runtime.compress_tracks(ctx, h_large, parents=np.array([NO_PARENT, 0, 1, 2, 6, 0, 0, 0, 0], dtype=np.uint32))

        retired = ctx.register_raw_tracks(small, RATE)         # (behind every other registration: its slot is not handed out again here)
        ctx.unregister_raw_tracks(retired)
        handles = [h_small, 0, 4000, retired, 0xFFFFFFFF, h_large, h_small]
        check_rows(launch(ctx, handles, max_tracks=9, max_samples=12, parents=parents), [c_small, refused, refused, refused, refused, c_large, c_small])
        # max_tracks 4: the array of 9 tracks is refused
        check_rows(launch(ctx, handles, max_tracks=4, max_samples=12, parents=parents[:4]),
              [restatement.compress(small, RATE, parents=parents[:4], **settings), refused, refused, refused, refused, refused, restatement.compress(small, RATE, parents=parents[:4], **settings)])
        # tables of 4 entries, each kind alone
        roots = restatement.compress(small, RATE, **settings)
        short = {"default_pose": np.tile(IDENTITY, (4, 1)), "parents": np.full(4, NO_PARENT, dtype=np.uint32),
                 "track_precisions": np.full(4, PRECISION, dtype=np.float32), "track_shell_distances": np.full(4, SHELL, dtype=np.float32)}
        for name, table in short.items():
            check_rows(launch(ctx, handles, max_tracks=9, max_samples=12, **{name: table}), [roots, refused, refused, refused, refused, refused, roots])
        # a stride that holds the small blob and not the large one; and the largest stride that does not hold the small one
        assert c_small.blob.size < c_large.blob.size
        stride = (c_small.blob.size + 15) & ~15
        assert stride < c_large.blob.size
        # (the shell of an instance refused for its size was computed: its metadata is written; only the rows are looked at)
        check_rows(launch(ctx, handles, max_tracks=9, max_samples=12, parents=parents, stride=stride, with_metadata=False),
              [c_small.blob, refused, refused, refused, refused, refused, c_small.blob])
        assert c_small.blob.size % 16 != 0
        check_rows(launch(ctx, [h_small, h_large], max_tracks=9, max_samples=12, parents=parents, stride=c_small.blob.size & ~15, with_metadata=False), [refused, refused])


def test_two_runs_give_the_same_bytes_and_a_capture_replays_to_them(sweep):
    ctx, handles, clips, expected = sweep
    parents, compressed = expected["two_roots"]
    runs = [launch(ctx, handles + [0], flags=OPTIMIZE_LOOPS, parents=parents, graph=graph) for graph in (False, False, True)]
    assert same(runs[0], runs[1])
    assert same(runs[0], runs[2])           # the same launch captured into a graph and replayed
