"""Spawned rank groups for the data-parallel tests: joined under a time limit of their own, never retried."""
import time

import torch.multiprocessing as mp


def spawn_joined(fn, args, nprocs: int, limit: float = 300.0):
    """``mp.spawn(fn, args, nprocs)`` whose join ends after ``limit`` seconds at the latest: the children still alive then are
    killed and the caller fails with ``TimeoutError``.  A rank that raises ends the group at once (``ProcessRaisedException``,
    the other ranks are terminated by torch) -- nothing is started again."""
    ctx = mp.start_processes(fn, args=args, nprocs=nprocs, join=False, start_method="spawn")
    deadline = time.monotonic() + limit
    try:
        while not ctx.join(timeout=max(0.0, min(5.0, deadline - time.monotonic()))):      # (returns as soon as a rank ends)
            if time.monotonic() >= deadline:
                raise TimeoutError(f"{nprocs} spawned ranks of {fn.__name__} still running after {limit:.0f} s: killed")
    finally:
        for p in ctx.processes:
            if p.is_alive():
                p.kill()
        for p in ctx.processes:
            p.join(10)
