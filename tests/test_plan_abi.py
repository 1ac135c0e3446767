"""rwrt_launch_plan / rwrt_launch_plan_bytes validate their arguments before
the first HIP call (no GPU needed): RWRT_ERR_ARG with a message."""
import ctypes

import _hip as H

A = 4096          # an aligned, non-NULL "device pointer": never dereferenced by a refused call
N = 16


def call(lib, nray=N, policy=H.PLAN_SINCE, state=A, count=A, prev=A, work=A, order=A, slot=A, nslot=A,
         nlive=True, scratch=A, nbytes=1 << 20):
    h = ctypes.c_int64(-7)
    st = lib.rwrt_launch_plan(nray, policy, state, count, prev, work, order, slot, nslot,
                              ctypes.byref(h) if nlive else None, scratch, nbytes, None)
    return st, h.value


def test_launch_plan_refuses_bad_shapes_and_policies():
    lib = H.load()
    for nray in (-1, 1 << 31):
        st, h = call(lib, nray=nray)
        assert st == H.RWRT_ERR_ARG and b"nray" in lib.rwrt_last_error() and h == -7
    for policy in (-1, 2, 7):
        st, _ = call(lib, policy=policy)
        assert st == H.RWRT_ERR_ARG and b"policy" in lib.rwrt_last_error()


def test_launch_plan_refuses_null_buffers():
    lib = H.load()
    for name in ("state", "count", "prev", "work", "order", "slot", "nslot", "scratch"):
        st, _ = call(lib, **{name: None})
        assert st == H.RWRT_ERR_ARG and b"NULL" in lib.rwrt_last_error(), name
    st, _ = call(lib, nlive=False)
    assert st == H.RWRT_ERR_ARG and b"NULL" in lib.rwrt_last_error()
    # (no ray: the per-ray buffers may be NULL, the two counts may not)
    st, _ = call(lib, nray=0, nslot=None)
    assert st == H.RWRT_ERR_ARG and b"NULL" in lib.rwrt_last_error()


def test_launch_plan_refuses_misaligned_buffers():
    lib = H.load()
    for name in ("state", "count", "prev", "work", "order", "nslot"):
        st, _ = call(lib, **{name: A + 4})
        assert st == H.RWRT_ERR_ARG and b"misaligned" in lib.rwrt_last_error(), name
    st, _ = call(lib, slot=A + 2)
    assert st == H.RWRT_ERR_ARG and b"misaligned" in lib.rwrt_last_error()
    st, _ = call(lib, scratch=A + 128)
    assert st == H.RWRT_ERR_ARG and b"misaligned" in lib.rwrt_last_error()


def test_launch_plan_bytes_refuses_bad_arguments():
    lib = H.load()
    b = ctypes.c_int64(0)
    assert lib.rwrt_launch_plan_bytes(-1, ctypes.byref(b)) == H.RWRT_ERR_ARG
    assert b"nray" in lib.rwrt_last_error()
    assert lib.rwrt_launch_plan_bytes(1 << 31, ctypes.byref(b)) == H.RWRT_ERR_ARG
    assert lib.rwrt_launch_plan_bytes(N, None) == H.RWRT_ERR_ARG
    assert b"NULL" in lib.rwrt_last_error()
