"""rwrt_rk45_init_stack / rwrt_rk45_run_stack (member stacks, include/rwrt.h)
validate their arguments before the first HIP call (no GPU needed):
RWRT_ERR_ARG with a message; an empty batch is a no-op."""
import ctypes

import _hip as H
from support.abi import A, ENTRIES, NPTS, NROW, grid, stack

run, init = ENTRIES["rwrt_rk45_run_stack"], ENTRIES["rwrt_rk45_init_stack"]   # (keyword callers, valid-looking defaults)


def refused(lib, st, word):
    assert st == H.RWRT_ERR_ARG, st
    assert word in lib.rwrt_last_error(), lib.rwrt_last_error()


def test_stack_struct_is_32_bytes():
    assert ctypes.sizeof(H.Stack) == 32
    assert H.Stack.member_stride.offset == 16 and H.Stack.d_member.offset == 24


def test_null_grid_stack_and_member_arrays():
    lib = H.load()
    for call in (run, init):
        refused(lib, call(lib, g=None), b"grid is NULL")
        refused(lib, call(lib, s=None), b"stack is NULL")
        refused(lib, call(lib, s=stack(packed=None)), b"d_packed is NULL")
        refused(lib, call(lib, s=stack(member=None)), b"d_member is NULL")
        refused(lib, call(lib, s=stack(packed=A + 8)), b"16-byte aligned")


def test_member_count_and_stride():
    lib = H.load()
    for call in (run, init):
        for n in (0, -2):
            refused(lib, call(lib, s=stack(nmember=n)), b"nmember >= 1")
        refused(lib, call(lib, s=stack(stride=NPTS * 12 - 2)), b"member_stride")
        refused(lib, call(lib, s=stack(stride=0)), b"member_stride")
        refused(lib, call(lib, s=stack(stride=NPTS * 12 + 1)), b"member_stride")   # (odd: members lose 16-B alignment)


def test_image_limit():
    """nmember * cache_image_bytes + 8 KiB <= 2^32: 64 members at 0.25 degrees
    (1441 x 721) are refused, 43 pass this check (and fail a later one)."""
    lib = H.load()
    ncol, nrow = 1441, 721
    image = (ncol * nrow + 63) // 64 * 6144
    assert 43 * image + 8192 <= 2 ** 32 < 44 * image + 8192
    for call in (run, init):
        refused(lib, call(lib, g=grid(ncol, nrow), s=stack(nmember=64, stride=ncol * nrow * 12)), b"32-bit")
        refused(lib, call(lib, g=grid(ncol, nrow), s=stack(nmember=44, stride=ncol * nrow * 12)), b"32-bit")
        # 43 members fit: the next check speaks (params)
        refused(lib, call(lib, g=grid(ncol, nrow), s=stack(nmember=43, stride=ncol * nrow * 12), p=None), b"params")


def test_run_keeps_every_check_of_the_static_entry():
    lib = H.load()
    refused(lib, run(lib, ctx=None), b"rwrt_ctx is NULL")
    refused(lib, run(lib, p=None), b"params is NULL")
    for nray in (-1, 1 << 31):
        refused(lib, run(lib, nray=nray), b"nray out of range")
    for i0, i1 in ((0, 5), (5, 5), (1, 182)):
        refused(lib, run(lib, i0=i0, i1=i1), b"it_begin")
    for name in ("tbound", "work", "state", "count", "nanrow", "out"):
        refused(lib, run(lib, **{name: None}), b"NULL buffer")
    refused(lib, run(lib, out=A + 8), b"16-byte aligned")
    refused(lib, run(lib, tail_from=A), b"tails need both")
    refused(lib, run(lib, tail_row=A), b"tails need both")
    refused(lib, run(lib, tail_from=A, tail_row=A + 8), b"16-byte aligned")
    # slots without tails
    refused(lib, run(lib, slot=A), b"row slots need tails")
    refused(lib, run(lib, g=grid(1, NROW), s=stack(stride=NROW * 12)), b"at least 2x2")


def test_init_keeps_every_check_of_the_static_entry():
    lib = H.load()
    refused(lib, init(lib, p=None), b"params is NULL")
    refused(lib, init(lib, nray=-1), b"nray out of range")
    for name in ("y0", "state", "count", "nanrow", "live", "summary"):
        refused(lib, init(lib, **{name: None}), b"NULL buffer")


def test_empty_batch_is_a_noop():
    """nray == 0: nothing is launched and no per-ray buffer is needed (the
    member arrays of the stack included)."""
    lib = H.load()
    s = stack(packed=None, member=None)
    assert run(lib, nray=0, s=s, state=None, count=None, nanrow=None, out=None) == H.RWRT_OK
    assert run(lib, nray=0, tail_from=A, tail_row=A, slot=A, state=None, count=None, nanrow=None, out=None) == H.RWRT_OK
    # (the checks that need no ray still speak)
    refused(lib, run(lib, nray=0, s=stack(nmember=0)), b"nmember >= 1")
    refused(lib, run(lib, nray=0, ctx=None), b"rwrt_ctx is NULL")
