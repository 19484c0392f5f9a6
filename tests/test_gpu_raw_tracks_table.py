"""The raw track table (aclhip_register_raw_tracks, aclhip_get_raw_tracks_info, aclhip_unregister_raw_tracks): a fifth handle table
with the lifetime of a skin's -- handles from 1, reused after a retirement, a table that never moves (a launch captured into a graph holds
its address and replays after dozens of registrations), unregistration ordered behind the launches already enqueued. Rows are compared on
bits with the restatement of tests/test_raw_tracks_oracle.py. Needs a GPU."""
import numpy as np
import pytest

from acl_amd import runtime
from test_gpu_pose_buffers import SENTINEL, bits
from test_gpu_raw_tracks import N, RATE, check, expected, launch
from test_raw_tracks_oracle import CLAMP, NEAREST, WRAP, finite_duration, random_clip

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def clips():
    rng = np.random.default_rng(7601)
    return [random_clip(rng, 2 + index % 5, 1 + (index * 7) % 23) for index in range(24)]


def test_register_info_unregister_and_handle_reuse(clips):
    import torch
    with runtime.Context(0) as ctx:
        with pytest.raises(runtime.AclHipError):
            ctx.raw_tracks_info(1)                                  # nothing was registered yet
        handles = [ctx.register_raw_tracks(clip, RATE + index, WRAP if index % 2 else CLAMP) for index, clip in enumerate(clips)]
        assert handles == list(range(1, len(clips) + 1))            # from 1: 0 is the null handle
        for index, (handle, clip) in enumerate(zip(handles, clips)):
            info = ctx.raw_tracks_info(handle)
            looping = WRAP if index % 2 else CLAMP
            assert (info.num_tracks, info.num_samples, info.sample_rate, info.looping_policy, tuple(info.reserved)) == (clip.shape[1], clip.shape[0], RATE + index, looping, (0, 0, 0))
            assert bits(np.float32(info.duration)) == bits(finite_duration(clip.shape[0], RATE + index, looping))
        for handle in (0, len(clips) + 1, 0xFFFFFFFF):
            with pytest.raises(runtime.AclHipError):
                ctx.raw_tracks_info(handle)
            with pytest.raises(runtime.AclHipError):
                ctx.unregister_raw_tracks(handle)
        # a refused array takes no handle
        with pytest.raises(runtime.AclHipError) as refused:
            ctx.register_raw_tracks(clips[0], 0.0)
        assert refused.value.status == runtime.ERROR_INVALID_ARGUMENT and "sample rate" in str(refused.value)
        # a retired handle is unknown at once, and the next registration behind its retirement reuses it, with its own content
        ctx.unregister_raw_tracks(handles[4])
        with pytest.raises(runtime.AclHipError):
            ctx.raw_tracks_info(handles[4])
        with pytest.raises(runtime.AclHipError):
            ctx.unregister_raw_tracks(handles[4])
        torch.cuda.synchronize()
        again = ctx.register_raw_tracks(clips[9], RATE, WRAP)
        assert again == handles[4]
        info = ctx.raw_tracks_info(again)
        assert (info.num_tracks, info.num_samples, info.sample_rate, info.looping_policy) == (clips[9].shape[1], clips[9].shape[0], RATE, WRAP)
        times = np.linspace(-0.01, 0.2, N).astype(np.float32)
        out = launch(ctx, [again] * N, times, clips[9].shape[1])
        check(out.poses, expected(clips[9], WRAP, times))
        assert ctx.rejected_instance_count() == 0


def test_the_caller_may_free_its_samples_when_registration_returns(clips):
    with runtime.Context(0) as ctx:
        mine = clips[3].copy()
        raw = ctx.register_raw_tracks(mine, RATE, CLAMP)
        want = expected(clips[3], CLAMP, np.linspace(0.0, 0.1, N).astype(np.float32), NEAREST)
        mine[:] = np.nan
        del mine
        out = launch(ctx, [raw] * N, np.linspace(0.0, 0.1, N).astype(np.float32), clips[3].shape[1], policy=NEAREST)
        check(out.poses, want)


def test_a_launch_enqueued_before_an_unregistration_still_samples(clips):
    import torch
    clip = clips[17]
    times = np.linspace(-0.02, 0.25, N).astype(np.float32)
    want = expected(clip, WRAP, times)
    with runtime.Context(0) as ctx:
        keeps = ctx.register_raw_tracks(clips[2], RATE, CLAMP)
        raw = ctx.register_raw_tracks(clip, RATE, WRAP)
        stream = torch.cuda.current_stream(torch.device("cuda:0")).cuda_stream
        # enqueued, then retired without a wait in between: the launch is served
        served = launch(ctx, [raw] * N, times, clip.shape[1], stream=stream)
        ctx.unregister_raw_tracks(raw)
        check(served.buffers.down(served.tensor), want)
        # the next launch refuses the handle
        before = ctx.rejected_instance_count()
        out = launch(ctx, [raw] * N, times, clip.shape[1])
        check(out.poses, [None] * N)
        assert ctx.rejected_instance_count() - before == N
        # the other array was never touched
        out = launch(ctx, [keeps] * N, times, clips[2].shape[1])
        check(out.poses, expected(clips[2], CLAMP, times))


def test_the_table_does_not_move_under_a_captured_launch(clips):
    import torch
    clip = clips[11]
    times = np.linspace(0.0, 0.2, N).astype(np.float32)
    want = expected(clip, CLAMP, times)
    with runtime.Context(0) as ctx:
        raw = ctx.register_raw_tracks(clip, RATE, CLAMP)             # the first registration makes the table
        device = torch.device("cuda:0")
        side = torch.cuda.Stream(device=device)
        side.wait_stream(torch.cuda.current_stream(device))
        with torch.cuda.stream(side):
            captured = launch(ctx, [raw] * N, times, clip.shape[1], stream=side.cuda_stream)       # warm-up
            side.synchronize()
            captured.tensor.fill_(float(SENTINEL))
            side.synchronize()
            graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graph, stream=side):
                ctx.sample_raw_tracks_batch(*captured.arguments, desc=captured.desc, stream=side.cuda_stream)
        # the graph holds the table's address: two dozen registrations and a few retirements later it still finds its array there
        others = [ctx.register_raw_tracks(other, RATE, CLAMP) for other in clips]
        for handle in others[::5]:
            ctx.unregister_raw_tracks(handle)
        torch.cuda.synchronize()
        with torch.cuda.stream(side):
            graph.replay()
        torch.cuda.synchronize()
        check(captured.tensor.cpu().numpy(), want)
        del graph
        assert ctx.rejected_instance_count() == 0
