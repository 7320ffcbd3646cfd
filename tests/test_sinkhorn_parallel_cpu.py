"""The Sinkhorn potentials across ranks, in the manner of tests/test_parallel_cpu.py: a world-2 gloo group whose ranks hold 10 and
14 rows of one recorded [24, 1000] case (kernels under the CPU SIMT executor in every rank) must arrive at the potentials one process
computes from all 24 rows - the column sums are all-reduced under a shift the ranks agree on, and the reference's B cancels."""
import os
import sys

import numpy as np
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SPLIT = (10, 14)


def _case():
    for p in (ROOT, os.path.join(ROOT, "tests")):
        if p not in sys.path:
            sys.path.insert(0, p)
    import sinkhorn_np as R
    name, c = [(n, c) for n, c in R.load_cases(os.path.join(ROOT, "tests", "golden")) if c["t"].shape == (24, 1000)][0]
    return R, c


def _single_process(c):
    from backends import Backend
    from ccd_amd import ops
    with Backend("sim"):
        return ops.sinkhorn_potentials(torch.from_numpy(c["t"]), torch.tensor([24], dtype=torch.int32), c["temp"], c["n"], rows_mul=1).numpy()


def _worker(rank, world, port, single):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world))
    R, c = _case()
    torch.set_num_threads(2)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    from backends import Backend
    from ccd_amd import ops
    with Backend("sim"):
        first = sum(SPLIT[:rank])
        mine = c["t"][first:first + SPLIT[rank]]
        t = torch.full((16, 1000), float("nan"))                     # the launch is sized for 16 rows, the device-side count says fewer
        t[:len(mine)] = torch.from_numpy(mine)
        got = ops.sinkhorn_potentials(t, torch.tensor([len(mine)], dtype=torch.int32), c["temp"], c["n"], rows_mul=1).numpy()
    want = R.potentials(c["t"], c["temp"], c["n"])
    print(f"rank {rank}: |c - single process| {np.abs(got - single).max():.2e}, |c - float64| {np.abs(got - want).max():.2e}, max |c| {np.abs(got).max():.3f}")
    assert np.abs(got).max() <= 1.0 and abs(float(got.astype(np.float64).mean())) <= 1e-6
    assert np.abs(got - single).max() <= 1e-6, np.abs(got - single).max()
    assert np.abs(got - want).max() <= 1e-6, np.abs(got - want).max()
    both = [torch.zeros(1000) for _ in range(world)]
    dist.all_gather(both, torch.from_numpy(got))
    assert torch.equal(both[0], both[1]), "the ranks disagree about the potentials"
    dist.destroy_process_group()


def test_sinkhorn_potentials_world2():
    _, c = _case()
    single = _single_process(c)
    mp.spawn(_worker, args=(2, 29631, single), nprocs=2, join=True)
