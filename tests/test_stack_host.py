"""Member stacks, host side (no GPU): csrc/stack_image.h in a stand-alone
program under the sanitizers against a Python restatement, the per-member
outcomes (``ensemble.member_outcomes``) on hand-made tensors, and the slot
layout and ``by`` channels of ``EnsembleWR``."""
import os
import shutil
import subprocess
import types

import numpy as np
import pytest
import torch

from ensemble import EnsembleWR, member_outcomes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TILE, REACH, LIMIT = 6 * 1024, 8 * 1024, 1 << 32


# ---- the Python restatement of csrc/stack_image.h
def image_bytes(npts):
    return (npts + 63) // 64 * TILE


def point_offset(p):
    # chunk 0 of point p: tile p // 64, 16 B per point inside the tile's first KiB
    return (p // 64) * TILE + (p % 64) * 16


def fits(npts, nmember):
    return nmember >= 1 and npts >= 1 and nmember * image_bytes(npts) + REACH <= LIMIT


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("c++")
    if cxx is None:
        pytest.skip("no host C++ compiler")
    exe = str(tmp_path_factory.mktemp("stack") / "stack_image_main")
    cmd = [cxx, "-O1", "-g", "-std=c++17", "-Wall", "-fsanitize=undefined,address", "-fno-sanitize-recover=all",
           "-fno-omit-frame-pointer", "-I" + os.path.join(ROOT, "rossby-wave-ray-tracing_amd", "csrc"),
           "-o", exe, os.path.join(ROOT, "tests", "host", "stack_image_main.cpp")]
    b = subprocess.run(cmd, capture_output=True, text=True)
    if b.returncode != 0 and "sanitize" in b.stderr and "stack_image" not in b.stderr:
        pytest.skip("this toolchain has no sanitizer runtime: " + b.stderr[-300:])
    assert b.returncode == 0, b.stderr[-3000:]

    def ask(lines):
        r = subprocess.run([exe], input="\n".join(lines) + "\n", capture_output=True, text=True)
        assert r.returncode == 0, r.stderr[-3000:]
        return [int(x) for x in r.stdout.split()]
    return ask


GRIDS = (145 * 73, 1441 * 721, 64, 65, 2 * 2, (1 << 24) - 1)


def test_offsets_match_the_restatement(program):
    rng = np.random.default_rng(7)
    q, want = [], []
    for npts in GRIDS:
        q.append(f"bytes {npts}")
        want.append(image_bytes(npts))
        pts = sorted({0, 1, 63, 64, 65, npts - 1, npts // 2} | set(int(x) for x in rng.integers(0, npts, 6)))
        for p in (p for p in pts if 0 <= p < npts):
            q.append(f"point {p}")
            want.append(point_offset(p))
            # every chunk of every point lies inside its member's image
            assert point_offset(p) + 5 * 1024 + 16 <= image_bytes(npts)
            for m in (0, 1, 2, 41):
                q.append(f"off {npts} {m} {p}")
                want.append(m * image_bytes(npts) + point_offset(p))
    assert program(q) == want


def test_one_member_is_the_static_image(program):
    """nmember = 1: offset 0, and the image size is the static cache image's
    (6 KiB per 64 points)."""
    for npts in GRIDS:
        size, m0, last = program([f"bytes {npts}", f"off {npts} 0 0", f"off {npts} 0 {npts - 1}"])
        assert size == (npts + 63) // 64 * 6144 and m0 == 0
        assert last == ((npts - 1) >> 6) * 5120 + (npts - 1) * 16   # rwrt.hip img_offset, restated
        assert program([f"fits {npts} 1"]) == [1]


def test_limit_edges(program):
    # exactly at the limit, one byte over
    assert program([f"bytesfit {LIMIT - REACH}", f"bytesfit {LIMIT - REACH + 1}", "bytesfit 0",
                    f"bytesfit {LIMIT}"]) == [1, 0, 1, 0]
    # images come in 6 KiB tiles: the last count of tiles that fits, and the next
    tiles = (LIMIT - REACH) // TILE
    assert tiles * TILE + REACH <= LIMIT < (tiles + 1) * TILE + REACH
    assert program([f"fits {tiles * 64} 1", f"fits {tiles * 64 + 1} 1"]) == [1, 0]
    # 0.25 degrees: 43 members fit, 44 and 64 do not; 2.5 degrees: thousands
    big, small = 1441 * 721, 145 * 73
    assert program([f"fits {big} 43", f"fits {big} 44", f"fits {big} 64"]) == [1, 0, 0]
    n = (LIMIT - REACH) // image_bytes(small)
    assert n > 4000 and program([f"fits {small} {n}", f"fits {small} {n + 1}"]) == [1, 0]
    q = [(npts, m) for npts in GRIDS for m in (1, 2, 43, 44, 4000, 5000, 1 << 20, (1 << 31) - 1)]
    assert program([f"fits {a} {b}" for a, b in q]) == [int(fits(a, b)) for a, b in q]
    assert program(["fits 0 1", "fits 64 0", "fits 64 -1", f"fits {1 << 40} 1"]) == [0, 0, 0, 0]


def test_member_index_is_clamped(program):
    assert program(["clamp -1 3", "clamp 0 3", "clamp 2 3", "clamp 3 3", "clamp 2147483647 3",
                    "clamp -2147483648 1"]) == [0, 0, 2, 2, 2, 0]


# ---- the per-member outcomes
def test_member_outcomes_failed_broken_and_empty_members():
    nt, nan = 20, float("nan")
    #            m0: fine      m1: failed        m2: breaks at 7   (m3: no ray)   m4: dead slots only
    member = torch.tensor([0, 0, 0, 1, 1, 1, 2, 2, 2, 4, 4])
    live = torch.tensor([1, 1, 0, 1, 1, 0, 1, 1, 0, 0, 0], dtype=torch.int32)
    h_abs = torch.tensor([5.0, nan, nan, nan, nan, 3.0, 1.0, 2.0, nan, nan, 4.0])
    nanrow = torch.tensor([nt, 4, 1, nt, nt, 1, 7, 3, 1, 1, 1], dtype=torch.int32)
    failed, brk = member_outcomes(member, live, h_abs, nanrow, 5, nt)
    # m1: live rays, none with a finite h_abs (the finite one belongs to a dead slot)
    assert failed == [False, True, False, False, False]
    # m0 has a ray that never breaks; m2's last ray breaks at 7; m4: every slot NaN from row 1
    assert brk == [None, 1, 7, None, 1]
    # the same from arrays, in another ray order
    perm = np.random.default_rng(1).permutation(len(member))
    f2, b2 = member_outcomes(member.numpy()[perm], live.numpy()[perm], h_abs.numpy()[perm], nanrow.numpy()[perm], 5, nt)
    assert (f2, b2) == (failed, brk)
    # an inf step is not NaN: rkf45.py:423-425 tests isnan
    failed, _ = member_outcomes([0], [1], [float("inf")], [nt], 1, nt)
    assert failed == [False]


# ---- the slot layout and the channels, without a device
def _ensemble(nmember=3, nsource=4, nzwn=5):
    return EnsembleWR(types.SimpleNamespace(nlev=nmember), nzwn, nsource, 7200.0, 180 * 7200.0)


def test_slot_layout_and_channels():
    ew = _ensemble()
    assert ew.nt == 181 and ew.nray == 3 * 3 * 4 * 5 and ew.slot_shape == (3, 3, 4, 5)
    idx = np.arange(ew.nray).reshape(ew.slot_shape)
    for m, r, s, z in ((0, 0, 0, 0), (2, 2, 3, 4), (1, 0, 3, 2), (2, 1, 0, 4)):
        assert ew.slot(m, r, s, z) == idx[m, r, s, z] == ((m * 3 + r) * 4 + s) * 5 + z
    assert ew.channels(None) == (None, 1)
    for by, ax, n in (("member", 0, 3), ("root", 1, 3), ("zwn", 3, 5)):
        chan, nchan = ew.channels(by)
        assert nchan == n and chan.dtype == np.int32 and chan.shape == (ew.nray,)
        assert np.array_equal(chan.reshape(ew.slot_shape), np.indices(ew.slot_shape)[ax])
    assert np.array_equal(ew.members(), np.repeat(np.arange(3), 3 * 4 * 5))
    with pytest.raises(ValueError):
        ew.channels("source")
    # member m's block of slots is a WR's slot order
    assert np.array_equal(idx[1].reshape(-1) - idx[1, 0, 0, 0], np.arange(3 * 4 * 5))


def test_sources_and_wavenumbers_are_wr_s():
    from wr import WR
    ew = _ensemble(nsource=6, nzwn=2)
    w = WR(2, 6, 7200.0, 180 * 7200.0, nx=144, ny=73)
    for o in (ew, w):
        o.set_zwn([3, 5])
        o.set_source_matrix(350.0, -10.0, 25.0, 12.5, 3, 2)
    assert np.array_equal(ew.zwn, w.zwn) and np.array_equal(ew.source_lon, w.source_lon)
    assert np.array_equal(ew.source_lat, w.source_lat) and ew.nt == w.nt
    assert np.array_equal(ew.cut_off, w.cut_off)
    with pytest.raises(ValueError):
        ew.set_zwn([1, 2, 3])
