"""TEST INFRASTRUCTURE shared by tests/test_inbatch_dp_host.py and tests/test_gpu_inbatch_dp.py: starting the ranks of a two-rank
in-batch step so that one rank's failure ends the test at once, and the rows both modules step over.  Never imported by the
product."""
import datetime
import os
import queue
import socket
import time
import traceback

import torch
import torch.multiprocessing as mp

NAMES = ("all", "other_class", "multi_positive")
GROUP_TIMEOUT = datetime.timedelta(seconds=60)      # a collective whose peer is gone raises instead of waiting for ever

# Global index rows of 6 items over a pool of 12; rank r takes items [3r, 3r + 3) of a row (tests/test_gpu_dp2.py: _tables).
# With SyntheticTripletPool(12, seed=3) (gt = 4 3 1 2 3 4 2 0 0 0 2 1, sn = 3 0 0 1 4 1 0 3 2 2 1 3) rank 1's anchors of row 0
# (classes 2 3 4) meet their classes among rank 0's candidates (4 3 1 | 3 0 0), and no two of the four (rank, row) class
# vectors are equal -- the tests assert it on the tables.
ITEMS = [list(range(0, 6)), list(range(11, 5, -1))]


def free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def init_group(rank, world, port):
    import torch.distributed as dist
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world, timeout=GROUP_TIMEOUT)


def report(out, rank, body, *args):
    """The whole of a rank's entry function: put (rank, True, body(*args)) on the queue, or the exception as text, so that the
    parent never waits for a rank that has failed; the group is destroyed either way."""
    import torch.distributed as dist
    try:
        out.put((rank, True, body(*args)))
    except BaseException:                                        # noqa: B902 -- reported, then the process ends with a failure
        out.put((rank, False, traceback.format_exc()))
        raise
    finally:
        if dist.is_initialized():
            dist.destroy_process_group()


class Ranks:
    """`world` spawned processes of worker(rank, world, port, queue, *args) (a module-level function that ends in report()), as a
    context: collect() returns their reports in rank order, and the first rank that reports an exception or dies fails the test
    there and then; whatever is still alive when the context ends is terminated.  Between entering and collect() the parent may
    do work of its own."""

    def __init__(self, worker, args=(), world=2, wait=300):
        ctx = mp.get_context("spawn")
        self.q, self.world, self.wait = ctx.Queue(), world, wait
        port = free_port()
        self.procs = [ctx.Process(target=worker, args=(r, world, port, self.q) + tuple(args)) for r in range(world)]

    def __enter__(self):
        for p in self.procs:
            p.start()
        return self

    def collect(self):
        got, deadline = {}, time.monotonic() + self.wait
        while len(got) < self.world:
            try:
                rank, ok, payload = self.q.get(timeout=1)
            except queue.Empty:
                dead = [(r, p.exitcode) for r, p in enumerate(self.procs) if p.exitcode not in (None, 0)]
                assert not dead, f"rank(s) ended without a report: (rank, exit code) {dead}"
                assert time.monotonic() < deadline, f"no report from every rank within {self.wait} s"
                continue
            assert ok, f"rank {rank} raised:\n{payload}"
            got[rank] = payload
        for p in self.procs:
            p.join(timeout=60)
            assert p.exitcode == 0
        return [got[r] for r in range(self.world)]

    def __exit__(self, *exc):
        for p in self.procs:
            if p.is_alive():
                p.terminate()
                p.join(timeout=10)


def run_ranks(worker, args=(), world=2, wait=300):
    with Ranks(worker, args, world, wait) as ranks:
        return ranks.collect()


def rank_items(items, rank, world=2):
    n = len(items) // world
    return items[rank * n:(rank + 1) * n]


def candidate_classes(gt_tab, sn_tab, items, world=2):
    """[gt_0 ; sn_0 ; gt_1 ; sn_1 ; ...] of a global row: the classes in the ranks' candidate order (int32 tensor)."""
    parts = []
    for r in range(world):
        i = torch.as_tensor(rank_items(items, r, world), device=gt_tab.device)
        parts += [gt_tab[i], sn_tab[i]]
    return torch.cat(parts).to(torch.int32)


def assert_classes_differ(gt_tab, sn_tab, rows=ITEMS, world=2):
    """The rows tell a stale or misplaced class vector from the right one: every (rank, row) has its own [gt ; sn], so the ranks
    differ within a step and a rank differs between consecutive steps."""
    seen = [tuple(candidate_classes(gt_tab, sn_tab, rank_items(items, r, world), 1).tolist()) for items in rows for r in range(world)]
    assert len(set(seen)) == len(seen), seen
