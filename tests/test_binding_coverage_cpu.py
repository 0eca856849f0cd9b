"""Every function csrc/bindings.cpp exports is called from some test, or is on a short allow-list with a reason.

Kernel launchers must not be on the list: a launcher that only whole-network steps reach is checked at network-level
tolerances, where a kernel wrong in every small-magnitude channel passes (the gap tests/test_bn_chain_gpu.py,
test_state_kernels_gpu.py and test_small_kernels_gpu.py closed).
"""
import glob
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# name -> why no test calls it directly; queries, aliases and probes only
ALLOWED_UNCALLED = {
    "conv_m_tiles": "query: the M-tile count of a conv plan, read by the executor's planner",
    "gconv_slice": "query: the grouped-conv channel-slice constant",
    "wgrad_3x3c64_supported": "query: shape predicate of the 3x3 C=64 wgrad kernel",
    "conv_dgrad_persistent": "query: which dgrad shapes take the persistent kernel",
    "stem_fwd_supported": "query: shape predicate of the window-mode stem",
    "bw_probe": "probe: streaming-bandwidth experiment behind tools/bw_probe.py, not on any training path",
}


def _exported():
    src = open(os.path.join(ROOT, "csrc", "bindings.cpp")).read()
    names = re.findall(r'\bm\.def\(\s*"([A-Za-z0-9_]+)"', src)
    assert len(names) > 80 and len(set(names)) == len(names), "m.def parsing broke"
    return names


def _test_sources():
    me = os.path.abspath(__file__)
    return {p: open(p).read() for p in sorted(glob.glob(os.path.join(ROOT, "tests", "*.py"))) if os.path.abspath(p) != me}


def test_every_exported_binding_is_called_from_a_test():
    srcs = _test_sources()
    uncalled = [n for n in _exported()
                if not any(re.search(r"\." + re.escape(n) + r"\(", s) for s in srcs.values())]
    unexpected = sorted(set(uncalled) - set(ALLOWED_UNCALLED))
    assert not unexpected, (f"bindings exported by csrc/bindings.cpp that no test calls: {unexpected}; add a direct test "
                            "(a kernel launcher may not be allow-listed)")


def test_allow_list_is_short_and_current():
    exported = set(_exported())
    stale = sorted(set(ALLOWED_UNCALLED) - exported)
    assert not stale, f"allow-listed names that are no longer exported: {stale}"
    srcs = _test_sources()
    now_called = sorted(n for n in ALLOWED_UNCALLED
                        if any(re.search(r"\." + re.escape(n) + r"\(", s) for s in srcs.values()))
    assert not now_called, f"allow-listed names that a test calls now (remove them from the list): {now_called}"
    assert len(ALLOWED_UNCALLED) <= 8
    for name, reason in ALLOWED_UNCALLED.items():
        assert reason.split(":")[0] in ("query", "alias", "probe"), f"{name}: only queries, aliases and probes"
