"""Child process of test_gpu_step_tclass.py: every case of CASES solved once under the GTO_STEP_TCLASS of this process's
environment, the outputs (Q, dQ, cost, iterations, status) of all of them into one .npz.

usage: python step_tclass_child.py OUT.npz

The small Panda, a 48^3 synthetic scene and max_iter = 12, as smoke(); every case on a handle of its own, created under the
case's knobs (the library reads them in gto_create)."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for p in (ROOT, HERE):
    if p not in sys.path:
        sys.path.insert(0, p)

T_CLASSES = (4, 30, 49, 50, 51, 96)  # the smallest T gto_create accepts; 50 | 51: the class boundary; 96: GTO_MAX_T
FULL = {"GTO_FEW_INSTANCES": "0"}    # six instances are a full round: the one-candidate kernel with its broad-phase tail
FEW = {}                             # the default: the eight-wave kernel with candidates
KNOBS = ("GTO_FEW_INSTANCES", "GTO_SLOTS")
NAN_INSTANCE = 2


def cases():
    """name -> (T, B, knobs, max_iter, poison the seed of NAN_INSTANCE)"""
    out = {}
    for kind, env in (("full", FULL), ("few", FEW)):
        for T in T_CLASSES:
            out[f"T{T}_{kind}"] = (T, 6, env, 12, False)
        # ten instances on four slots: six finishing workgroups hand their slot over (the exit block's second half)
        out[f"handover_{kind}"] = (50, 10, dict(env, GTO_SLOTS="4"), 12, False)
        out[f"cap1_{kind}"] = (50, 6, env, 1, False)  # the iteration cap: the exit in P1
        out[f"cap2_{kind}"] = (50, 6, env, 2, False)
        out[f"nan_{kind}"] = (50, 6, env, 12, True)   # a seed without a finite objective: GTO_STATUS_NUMERICAL, 0 iterations
    return out


def solve(capi, oracle, T, B, env, max_iter, poison):
    from helpers import Problem
    for k in KNOBS:
        os.environ.pop(k, None)
    os.environ.update(env)
    prob = Problem("panda", B=B, scene_seed=3, n=48, res=0.0467, T=T)
    opts = oracle.reference_opts(max_iter=max_iter, T=T, standoff_offset=-max(1, T // 5))
    h = capi.SolverHandle(prob.desc, prob.cfg["link_ee"], prob.cfg["link_gripper"], opts, device=0)
    prob.finish(h.eval_fk)
    h.set_scene(*prob.scene_args())
    args = list(prob.solve_args())
    if poison:
        Q0 = args[-1].copy()
        Q0[NAN_INSTANCE, prob.desc.opt_index[1], T // 2] = np.nan
        args[-1] = Q0
    out = h.solve_batch(*args)
    h.close()
    return out


def main():
    from grasptrajopt_amd import _capi
    from oracle import oracle
    res = {}
    for name, (T, B, env, max_iter, poison) in cases().items():
        for key, a in zip(("Q", "dQ", "cost", "iterations", "status"), solve(_capi, oracle, T, B, env, max_iter, poison)):
            res[f"{name}.{key}"] = np.asarray(a)
    np.savez(sys.argv[1], **res)


if __name__ == "__main__":
    main()
