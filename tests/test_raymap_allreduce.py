"""The table-driven reduction of the map products (raymap.allreduce_tensors,
behind every ``DeviceMap.allreduce``) on the CPU: world size 2 over gloo
(127.0.0.1), plain tensors -- the map classes themselves need a GPU
(tests/test_gpu_multirank.py)."""
import os

import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from support.dist import free_port

INT32_MAX = 2 ** 31 - 1


def _tensors(rank):
    """What rank ``rank`` holds: an arrival-like ``first`` (MIN, INT32_MAX:
    none), ``last`` (MAX, -1: none), an int64 ``count`` and an fp64 ``wsum``
    (SUM), and an array the product does not have (None)."""
    first = torch.tensor([[3, INT32_MAX, 7], [INT32_MAX, INT32_MAX, 2]], dtype=torch.int32)
    last = torch.tensor([[5, -1, 9], [-1, -1, 2]], dtype=torch.int32)
    count = torch.tensor([2 ** 40 + 1, 0, 5], dtype=torch.int64)
    wsum = torch.tensor([0.5, -1.25, 0.0], dtype=torch.float64)
    if rank == 1:
        first = torch.tensor([[4, 1, INT32_MAX], [INT32_MAX, 8, 2]], dtype=torch.int32)
        last = torch.tensor([[4, 6, -1], [-1, 8, 11]], dtype=torch.int32)
        count = torch.tensor([2 ** 40, 3, 0], dtype=torch.int64)
        wsum = torch.tensor([0.25, 1.25, 2.0 ** -60], dtype=torch.float64)
    return first, last, count, wsum


def _worker(rank, world, port, q):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        import raymap
        first, last, count, wsum = _tensors(rank)
        raymap.allreduce_tensors([(first, "MIN"), (last, "MAX"), (None, "SUM"), (count, "SUM"), (wsum, "SUM")])
        q.put(("ok", rank, first.tolist(), last.tolist(), count.tolist(), wsum.tolist()))
    except Exception as e:  # pragma: no cover
        q.put(("err", rank, repr(e)))
        raise
    finally:
        dist.destroy_process_group()


def test_world2_gloo_min_max_sum_and_none():
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = free_port()
    procs = [ctx.Process(target=_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    res = [q.get(timeout=120) for _ in procs]
    for p in procs:
        p.join(timeout=60)
    assert sorted(r[1] for r in res) == [0, 1] and all(r[0] == "ok" for r in res), res
    for r in res:                                   # the same, reduced arrays on both ranks, in place
        assert r[2] == [[3, 1, 7], [INT32_MAX, 8, 2]]
        assert r[3] == [[5, 6, 9], [-1, 8, 11]]
        assert r[4] == [2 ** 41 + 1, 3, 5]
        assert r[5] == [0.75, 0.0, 2.0 ** -60]
