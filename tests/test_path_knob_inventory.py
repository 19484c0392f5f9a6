"""Keeps tests/test_gpu_path_knobs.py level with the sources (no GPU needed): every path knob the library reads is set by one of its
configurations or named here with the test that reaches it, every kernel pose_kernel_of can pick is expected by one of its
configurations, and INTEGRATION.md 7b lists exactly the knobs the sources read."""
import glob
import os
import re

from test_gpu_path_knobs import CONFIGS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "acl_amd", "csrc")

# knobs whose paths another test file reaches (prefix match for the ordering barrier's test aids)
COVERED_ELSEWHERE = {
    "ACLHIP_FORCE_GENERIC_KERNEL": "test_gpu_parity.py",
    "ACLHIP_CONSUMER_KEEP_SCALE": "test_gpu_consumers.py",
    "ACLHIP_ORDER_TEST_": "test_gpu_order_device.py",
}


def _sources():
    return {path: open(path).read() for path in sorted(glob.glob(os.path.join(CSRC, "*")))}


def source_path_knobs():
    return {name for text in _sources().values() for name in re.findall(r'path_knob\("([A-Z0-9_]+)"\)', text)}


def pose_kernel_names():
    text = open(os.path.join(CSRC, "host_launch.inl")).read()
    body = re.search(r"pose_kernel pose_kernel_of\(.*?\n\t}\n", text, re.S).group(0)
    return set(re.findall(r'name = "([a-z0-9_]+)"', body))


def test_every_path_knob_is_reached_by_a_test():
    knobs = source_path_knobs()
    assert {"ACLHIP_WIDE_KEY_LOADS", "ACLHIP_IN_TURN_ITEMS", "ACLHIP_IN_TURN_ADJACENT"} <= knobs       # (the regex still finds them)
    configured = {name for config in CONFIGS.values() for name in config["env"]}
    for knob in sorted(knobs):
        if knob in configured:
            continue
        owners = [test for prefix, test in COVERED_ELSEWHERE.items() if knob.startswith(prefix)]
        assert owners, f"path knob {knob} is set by no configuration of test_gpu_path_knobs.py and covered by no other test"
        assert knob in open(os.path.join(ROOT, "tests", owners[0])).read(), f"{owners[0]} does not set {knob}"
    # the table names no knob the sources do not read
    assert configured <= knobs, configured - knobs


def test_every_pose_kernel_is_expected_by_a_configuration():
    names = pose_kernel_names()
    assert len(names) >= 13, names
    expected = set()
    for config in CONFIGS.values():
        expected |= {name for pair in config["kernels"].values() for name in pair}
        expected |= set(config.get("other_kernels", {}).values())
    assert names <= expected, f"kernels no configuration expects: {sorted(names - expected)}"
    assert expected <= names, f"kernels pose_kernel_of no longer picks: {sorted(expected - names)}"


def test_integration_lists_exactly_the_path_knobs():
    text = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    section = text[text.index("## 7b."):]
    table = section[section.index("| path knob |"):]
    table = table[: table.index("\n\n")]
    listed = set(re.findall(r"ACLHIP_[A-Z0-9_]+", table))
    assert listed == source_path_knobs(), (sorted(listed - source_path_knobs()), sorted(source_path_knobs() - listed))
