"""Child process of test_gpu_step_texact.py: every case of cases() solved once under the GTO_STEP_TEXACT of this process's
environment, the outputs (Q, dQ, cost, iterations, status) of all of them into one .npz; then the cases of COUNTED once more
under GTO_DEBUG_TIMING, whose stderr report says how many of a call's narrow step launches were k_lm_step_t50's (their
counts go into the same .npz as NAME.exact and NAME.other; their outputs are not kept: the stamps are a different path).

usage: python step_texact_child.py OUT.npz

The small Panda, a 48^3 synthetic scene and max_iter = 12, as smoke(); every case on a handle of its own, created under the
case's knobs (the library reads them in gto_create).  Modelled on step_tclass_child.py."""
import os
import re
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for p in (ROOT, HERE):
    if p not in sys.path:
        sys.path.insert(0, p)

T_CASES = (49, 50, 51)               # the exact length and its two neighbours, which must take the kernels they took
FULL = {"GTO_FEW_INSTANCES": "0"}    # six instances are a full round: the one-candidate kernel with its broad-phase tail
FEW = {}                             # the default: the eight-wave kernel with candidates
KNOBS = ("GTO_FEW_INSTANCES", "GTO_SLOTS", "GTO_PREBROAD", "GTO_DEBUG_TIMING")
COUNTED = tuple(f"T{T}_{kind}" for T in T_CASES for kind in ("full", "few"))
LINE = re.compile(r"narrow step launches of the call: (\d+) of k_lm_step_t50 \(T = 50 a constant\), (\d+) of the others")


def cases():
    """name -> (T, B, knobs, option overrides)"""
    out = {}
    for kind, env in (("full", FULL), ("few", FEW)):
        for T in T_CASES:
            out[f"T{T}_{kind}"] = (T, 6, env, {})
        # the exit block's three entrances, at T = 50:
        # ten instances on four slots and the iteration cap: the exit in P1, with and without a slot to hand over
        out[f"handover_{kind}"] = (50, 10, dict(env, GTO_SLOTS="4"), {})
        out[f"cap1_{kind}"] = (50, 6, env, {"max_iter": 1})
        # no velocity term: a waypoint in free space has a zero block, its pivot is not positive, and the instance leaves
        # behind the meeting block with GTO_STATUS_NUMERICAL
        out[f"wvel0_{kind}"] = (50, 6, env, {"w_vel": 0.0})
        # a step tolerance no step exceeds: the first trial point ends the solve in P4 with GTO_STATUS_CONVERGED
        out[f"tolstep_{kind}"] = (50, 6, env, {"tol_step": 1e3})
    # the tail's item lists against an obstacle launch that looks at every group
    out["T50_full_nopb"] = (50, 6, dict(FULL, GTO_PREBROAD="0"), {})
    return out


def solve(capi, oracle, T, B, env, over):
    from helpers import Problem
    for k in KNOBS:
        os.environ.pop(k, None)
    os.environ.update(env)
    prob = Problem("panda", B=B, scene_seed=3, n=48, res=0.0467, T=T)
    opts = oracle.reference_opts(**dict(dict(max_iter=12, T=T, standoff_offset=-max(1, T // 5)), **over))
    h = capi.SolverHandle(prob.desc, prob.cfg["link_ee"], prob.cfg["link_gripper"], opts, device=0)
    prob.finish(h.eval_fk)
    h.set_scene(*prob.scene_args())
    out = h.solve_batch(*prob.solve_args())
    h.close()
    return out


def counted(capi, oracle, T, B, env):
    """(launches of k_lm_step_t50, of the other narrow step kernels) of one solve call, read from the library's stderr"""
    sys.stderr.flush()
    keep = os.dup(2)
    with tempfile.TemporaryFile() as tf:
        os.dup2(tf.fileno(), 2)
        try:
            solve(capi, oracle, T, B, dict(env, GTO_DEBUG_TIMING="1"), {})
        finally:
            os.dup2(keep, 2)
            os.close(keep)
        tf.seek(0)
        text = tf.read().decode(errors="replace")
    hits = LINE.findall(text)
    assert hits, "no launch count in the GTO_DEBUG_TIMING report:\n" + text[-2000:]
    return sum(int(a) for a, _ in hits), sum(int(b) for _, b in hits)


def main():
    from grasptrajopt_amd import _capi
    from oracle import oracle
    res = {}
    all_cases = cases()
    for name, (T, B, env, over) in all_cases.items():
        for key, a in zip(("Q", "dQ", "cost", "iterations", "status"), solve(_capi, oracle, T, B, env, over)):
            res[f"{name}.{key}"] = np.asarray(a)
    for name in COUNTED:
        T, B, env, _ = all_cases[name]
        ex, ot = counted(_capi, oracle, T, B, env)
        res[f"{name}.exact"], res[f"{name}.other"] = np.int64(ex), np.int64(ot)
    np.savez(sys.argv[1], **res)


if __name__ == "__main__":
    main()
