"""GPU: device memory over the life of a handle.  Handles are created, given scenes, used through the host-pointer entry
points and closed, over and over; the free device memory must not shrink and the results must not move.

What this can see: a leaked SCENE buffer.  With 128^3 voxels the smallest buffer a scene owns (a uint8 distance field) is
2 MiB, so losing one of them per cycle costs 40 MiB over the 20 cycles between the two readings, twice the bound.
What it cannot see: buffers of a few kilobytes (the robot tables, the staging slots of a small batch, the pinned words).
Twenty of those vanish in the allocator's granularity.  For them the type is the guarantee: every allocation of
gto_api.hip outside DepthPool lives in an owner (csrc/gto_owned.h, tested by tests/owned_buffer_main.cpp) that frees it
when the handle, the scene entry, the observation or the grid goes away.  tools/leak_check.py is the longer manual soak."""
import numpy as np
import pytest

from grasptrajopt_amd import synthetic as syn
from helpers import Problem

pytestmark = pytest.mark.gpu

CYCLES, FIRST_READING = 25, 5
# A condition, not a measurement: half of what one leaked 2 MiB buffer per cycle adds between the two readings.
BOUND_MIB = 20.0


def test_handle_cycles_return_their_device_memory(oracle_mod):
    import torch
    import __graft_entry__ as gr
    gr.build()
    from grasptrajopt_amd import _capi

    B = 2
    prob = Problem("panda", B=B, scene_seed=1, n=128, res=0.0175)
    big = prob.scene
    small = syn.make_scene(1, n=96, res=0.0175 * 128 / 96)  # the same box at a coarser pitch: its buffers fit no spare
    assert big.c_all.size == 128 ** 3 and small.c_all.size == 96 ** 3
    opts = oracle_mod.reference_opts(max_iter=2)
    ee, gripper = prob.cfg["link_ee"], prob.cfg["link_gripper"]
    torch.cuda.init()

    def cycle(i):
        h = _capi.SolverHandle(prob.desc, ee, gripper, opts, device=0)
        if i == 0:
            prob.finish(h.eval_fk)
        h.set_scene(0, big.c_all, big.c_obs, big.shape, big.origin, big.res)
        h.set_scene(0, big.c_all, big.c_obs, big.shape, big.origin, big.res)  # takes the first one's buffers as spares
        h.set_scene(0, small.c_all, small.c_obs, small.shape, small.origin, small.res)  # the spares do not fit: freed
        h.set_scene(1, big.c_all, big.c_obs, big.shape, big.origin, big.res, values_only=True)
        h2 = _capi.SolverHandle(prob.desc, ee, gripper, opts, device=0)
        h2.share_scene(0, h)
        borrowed = h2.solve_batch(*prob.solve_args())
        h2.close()
        solved = h.solve_batch(*prob.solve_args())
        ik = h.solve_ik_batch(0, prob.qc, prob.goals[:, 0], prob.base, max_iter=2)
        cost = h.plan_cost(0, solved[0], prob.base[0])
        pts = h.eval_points(1, prob.qc, prob.base)
        rt = h.retime_batch(solved[0], 2.0, 5.0)
        base = h.solve_base_batch(prob.qc, prob.goals, max_iter=2)
        h.drop_scene(0)
        h.close()
        return [*borrowed, *solved, *ik, *cost, *pts, *(rt[k] for k in sorted(rt)), *base]

    free = {}
    for i in range(CYCLES):
        out = cycle(i)
        if i == 0:
            first = out
        if i + 1 in (FIRST_READING, CYCLES):
            torch.cuda.synchronize()
            free[i + 1] = torch.cuda.mem_get_info()[0] / 2 ** 20
    lost = free[FIRST_READING] - free[CYCLES]
    print(f"free device memory after cycle {FIRST_READING}: {free[FIRST_READING]:.1f} MiB, after cycle {CYCLES}: "
          f"{free[CYCLES]:.1f} MiB, not returned: {lost:.1f} MiB")
    assert lost < BOUND_MIB
    assert len(out) == len(first)
    for a, b in zip(first, out):
        assert a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()
