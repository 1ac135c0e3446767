"""The ray loop of the two static run kernels lies contiguously in the built
code object (no GPU, no compile: tools/hot_layout.py on librwrt.so).

The rarely taken branches of the loop carry their weight (RARE / UNLIKELY in
csrc/rwrt.hip), so their bodies lie behind the loop and the loop's span -- the
backward branch that encloses the six 24-load cell-cache refills -- is the
common path with its refills.  The limit is tools/hot_layout.py's SPAN_LIMIT,
48 KiB: the ~40 KB common path, the inline refills and a margin, below a
64 KB instruction cache that two CUs running the same loop share.  (Without
the weights the spans are 107 796 and 108 984 bytes,
profiles/layout/static_gate.txt.)
"""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import hot_layout as HL   # noqa: E402

LIB = os.path.join(HL.PKG, "librwrt.so")


@pytest.fixture(scope="module")
def layouts():
    if not HL.tools_present():
        pytest.skip("clang-offload-bundler / llvm-objdump / llvm-objcopy not found under " + HL.LLVM)
    if not os.path.exists(LIB):
        pytest.skip("librwrt.so is not built")
    return {r["kernel"]: r for r in HL.layouts(LIB, HL.GATED)}


@pytest.mark.parametrize("kernel", HL.GATED)
def test_ray_loop_span(layouts, kernel):
    r = layouts[kernel]
    loop = r["ray_loop"]
    assert loop is not None, "no loop with six 24-load refills in " + HL.KERNELS[kernel]
    print(f"{kernel}: kernel {r['size']} B, ray loop +0x{loop['start']:x}..+0x{loop['end']:x}, "
          f"span {loop['span']} B, {loop['instructions']} instructions, refills {loop['refills']}")
    assert HL.SPAN_LIMIT == 48 * 1024
    assert loop["span"] <= HL.SPAN_LIMIT
    assert len(loop["refills"]) == 6 and loop["refill_loads"] == [HL.REFILL_LOADS] * 6
    # every load of every refill inside the span (first and last load of each)
    for first, last in zip(loop["refills"], loop["refill_last"]):
        assert loop["start"] <= first <= last < loop["end"]
    # the six refills in stage order, none shared with a latency-mode loop
    assert loop["refills"] == sorted(loop["refills"])
    for q in r["quad_loops"]:
        assert q["end"] < loop["start"] or loop["end"] < q["start"]
