"""The path knobs of INTEGRATION.md 7b, each held to the oracle. A shipped libaclhip.so reads them from the environment once per
process (static locals, at the first pose launch or registration), so a pytest process cannot reach the paths they select: every
configuration of CONFIGS runs in a fresh child process (tests/path_knob_child.py) that first asserts which kernels the knobs select
and then decodes its matrix -- window counts 1 .. 6, instance counts at the grid's tails, clip sequences on one wave's turns that a
stale LDS image would get wrong, per instance arrays, a database-bound clip of two windows, the fast decode -- bit for bit against the
oracle. One child at a time; a child that crashes or times out stops the rest. Needs a GPU."""
import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
CHILD = os.path.join(HERE, "path_knob_child.py")

# the kernel pose_kernel_of (host_launch.inl) picks for a plain QVV48 launch: (exact, ACLHIP_DECODE_FAST) per row width
DEFAULT_KERNELS = {
    "one_window": ("decompress_tracks_kernel", "decompress_tracks_fast_kernel"),
    "several_windows": ("decompress_tracks_in_turn_kernel", "decompress_tracks_in_turn_fast_kernel"),
}

# the kernels of output descriptors and non-default settings: no knob moves them (the control run checks their names)
OTHER_KERNELS = {
    "qv32": "decompress_tracks_qv32_kernel",
    "qvv40": "decompress_tracks_qvv40_kernel",
    "compact": "decompress_tracks_compact_kernel",
    "any_settings": "decompress_tracks_any_settings_kernel",
    "any_settings_compact": "decompress_tracks_any_settings_compact_kernel",
}

# name -> env: the knobs set for the child (nothing else), child: which matrix it runs, items / adjacent: the in-turn grid the knobs
# give poses of several windows, kernels: as DEFAULT_KERNELS, fast_matrix: the ACLHIP_DECODE_FAST comparisons run too
CONFIGS = {
    "default": dict(env={}, child="pose", items=4, adjacent=False, kernels=DEFAULT_KERNELS, fast_matrix=True, other_kernels=OTHER_KERNELS),
    "wide_on": dict(env={"ACLHIP_WIDE_KEY_LOADS": "1"}, child="pose", items=4, adjacent=False, fast_matrix=True, kernels={
        "one_window": ("decompress_tracks_wide_loads_kernel", "decompress_tracks_wide_loads_fast_kernel"),
        "several_windows": ("decompress_tracks_in_turn_kernel", "decompress_tracks_in_turn_fast_kernel")}),
    "wide_off": dict(env={"ACLHIP_WIDE_KEY_LOADS": "0"}, child="pose", items=1, adjacent=False, fast_matrix=True, kernels={
        "one_window": ("decompress_tracks_kernel", "decompress_tracks_fast_kernel"),
        "several_windows": ("decompress_tracks_kernel", "decompress_tracks_fast_kernel")}),
    "one_shot": dict(env={"ACLHIP_IN_TURN_ITEMS": "1"}, child="pose", items=1, adjacent=False, fast_matrix=True, kernels={
        "one_window": ("decompress_tracks_kernel", "decompress_tracks_fast_kernel"),
        "several_windows": ("decompress_tracks_wide_loads_kernel", "decompress_tracks_wide_loads_fast_kernel")}),
    "items_3": dict(env={"ACLHIP_IN_TURN_ITEMS": "3"}, child="pose", items=3, adjacent=False, kernels=DEFAULT_KERNELS, fast_matrix=False),
    "items_max": dict(env={"ACLHIP_IN_TURN_ITEMS": "300"}, child="pose", items=255, adjacent=False, kernels=DEFAULT_KERNELS, fast_matrix=False),
    "adjacent": dict(env={"ACLHIP_IN_TURN_ADJACENT": "1"}, child="pose", items=4, adjacent=True, fast_matrix=True, kernels={
        "one_window": ("decompress_tracks_kernel", "decompress_tracks_fast_kernel"),
        "several_windows": ("decompress_tracks_in_turn_adjacent_kernel", "decompress_tracks_in_turn_adjacent_fast_kernel")}),
    "adjacent_3": dict(env={"ACLHIP_IN_TURN_ADJACENT": "1", "ACLHIP_IN_TURN_ITEMS": "3"}, child="pose", items=3, adjacent=True, fast_matrix=False, kernels={
        "one_window": ("decompress_tracks_kernel", "decompress_tracks_fast_kernel"),
        "several_windows": ("decompress_tracks_in_turn_adjacent_kernel", "decompress_tracks_in_turn_adjacent_fast_kernel")}),
    "short_exact_off": dict(env={"ACLHIP_SHORT_EXACT_MATH": "0"}, child="short_exact_off", items=4, adjacent=False, kernels=DEFAULT_KERNELS, fast_matrix=False),
    "no_slabs": dict(env={"ACLHIP_CLIP_SLABS": "0", "ACLHIP_VIRTUAL_CLIP_TABLE": "0"}, child="no_slabs", items=4, adjacent=False, kernels=DEFAULT_KERNELS, fast_matrix=False),
    "order_3": dict(env={"ACLHIP_ORDER_LAUNCHES": "3"}, child="order_3", items=4, adjacent=False, kernels=DEFAULT_KERNELS, fast_matrix=False),
}

CHILD_TIMEOUT_S = 90
_crashed = []       # the config whose child ended by a signal or a timeout: no further child is started


@pytest.mark.parametrize("config", list(CONFIGS))
def test_knob_configuration_holds_to_the_oracle(config):
    if _crashed:
        pytest.fail(f"not run: an earlier child crashed ({_crashed[0]})")
    env = dict(os.environ, **CONFIGS[config]["env"])
    try:
        completed = subprocess.run([sys.executable, CHILD, config], cwd=os.path.dirname(HERE), env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                                   text=True, timeout=CHILD_TIMEOUT_S)
    except subprocess.TimeoutExpired:
        _crashed.append(config)
        pytest.fail(f"{config}: the child did not finish in {CHILD_TIMEOUT_S} s")
    if completed.returncode < 0 or completed.returncode in (134, 139):
        _crashed.append(config)
    lines = [line for line in completed.stdout.splitlines() if line.startswith("{")]
    assert completed.returncode == 0 and lines, f"{config}: exit {completed.returncode}\n{completed.stdout[-2000:]}\n{completed.stderr[-4000:]}"
    result = json.loads(lines[-1])
    assert result["config"] == config and result["ok"], result
    expected = {name for pair in CONFIGS[config]["kernels"].values() for name in pair} | set(CONFIGS[config].get("other_kernels", {}).values())
    assert set(result["kernels"]) == expected, result
    print(f"{config}: {result['seconds']:.1f} s, kernels {sorted(result['kernels'])}, checks {result['checks']}")
