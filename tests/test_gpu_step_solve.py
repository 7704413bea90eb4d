"""GPU: the block solve inside the step kernels at every shape of its block pattern.  tests/step_solve_cases.py chooses the
pattern of each case (the length of the leading diagonal stretch, the meeting block, the active set) and
tests/test_step_solve_cpu.py vets the cases, the FP64 oracle and the dense numpy restatement tests/step_solve_ref.py against
each other first.  Here:

  lock step     solve_batch capped at 1, 2, 3 iterations (6 where the active set changes at later iterates) against the
                oracle: iterations and status exact, Q / dQ / f at the capped-solve tolerances of
                tests/test_gpu_solver_opts.py (atol 1e-9, atol 1e-8, rtol 1e-9); the first evaluation also against the
                restatement's trial point.  Every iterate inside the limits; a variable the restatement freezes at iterate
                k keeps its bits at iterate k + 1.
  families      narrow cases again on a fresh handle with GTO_FEW_INSTANCES=0 and under the deepest candidate lists:
                bit-identical, k_lm_step<8,4> in the default and k_lm_step<4,1> in the full-GPU rounds
  mixed batch   all cases of one (robot, T) in one call, at most eight a call: s_dense and mid are per workgroup, so the
                loop trip counts of neighbouring workgroups differ; every instance gives the bits of a call of its own

Run the file under a time limit and stop at the first fault: timeout -k 10 600 pytest -x tests/test_gpu_step_solve.py."""
import numpy as np
import pytest

import step_solve_cases as sc

pytestmark = pytest.mark.gpu

GROUPS = list(sc.GROUPS)
GROUP_IDS = ["-".join(str(x) for x in (g[0], f"T{g[1]}", f"off{g[2]}") + tuple(f"{k}{v}" for k, v in g[3])) for g in GROUPS]
NARROW = [g for g in GROUPS if sc.robot(g[0])[0].n_opt <= 8]
NARROW_IDS = [GROUP_IDS[GROUPS.index(g)] for g in NARROW]
MAX_B = 8
# the deepest candidate lists (SPECULATION of tests/test_gpu_solver_opts.py)
SPECULATION = dict(GTO_SPEC_ACC="4", GTO_SPEC_DEEP="100000", GTO_SPEC_JOBS="100000", GTO_SPEC_STREAK="0", GTO_SPEC_REJ="3")


@pytest.fixture(scope="module")
def capi():
    import __graft_entry__ as g
    g.build()
    from grasptrajopt_amd import _capi
    return _capi


def make_handle(capi, group):
    """A handle of a group with the field of its i-th case as scene i."""
    names = sc.GROUPS[group]
    p = sc.problem(names[0])
    h = capi.SolverHandle(p.desc, p.ee, p.gr, p.opts, device=0, n_gripper_points=p.ngp)
    h.set_mode(0)
    for i, nm in enumerate(names):
        h.set_scene(i, *sc.problem(nm).scene)
    return h


@pytest.fixture(scope="module")
def handles(capi):
    """One handle per group, made on first use and kept for the module; solo results per (case, cap) with them."""
    made = {}

    def get(group):
        if group not in made:
            made[group] = make_handle(capi, group)
        return made[group]
    get.solo = {}
    yield get
    for h in made.values():
        h.close()


def batch_args(group, names):
    all_names = sc.GROUPS[group]
    ps = [sc.problem(nm) for nm in names]
    return (np.array([all_names.index(nm) for nm in names], dtype=np.int32), np.stack([p.qc for p in ps]),
            np.stack([p.goals for p in ps]), 1, ps[0].S, np.stack([p.base for p in ps]), np.stack([p.Q0 for p in ps]))


def caps_run(case):
    """The caps a case is solved at: the compared ones, and every one below the largest for the frozen-variable check."""
    return tuple(range(1, max(case.caps) + 1))


def solo(handles, name, cap):
    """(Q, dQ, f, iterations, status) of a case in a call of its own on the group's handle."""
    if (name, cap) not in handles.solo:
        group = sc.CASES[name].group
        h = handles(group)
        h.set_opts(max_iter=cap)
        handles.solo[name, cap] = h.solve_batch(*batch_args(group, [name]))
    return handles.solo[name, cap]


def same(a, b):
    return all(np.ascontiguousarray(x).tobytes() == np.ascontiguousarray(y).tobytes() for x, y in zip(a, b))


def ran(h, args):
    """Launch counts per kernel variant of a profiled repeat of the last solve."""
    h.set_profiling(True)
    h.solve_batch(*args)
    prof = h.last_kernel_profile()
    h.set_profiling(False)
    return {k: v[1] for k, v in prof.items()}


# ------------------------------------------------------------------------------------------------------------ 1. lock step
@pytest.mark.parametrize("group", GROUPS, ids=GROUP_IDS)
def test_lock_step_with_oracle_and_restatement(capi, oracle_mod, handles, group):
    for name in sc.GROUPS[group]:
        case, p = sc.CASES[name], sc.problem(name)
        d, oi = p.desc, p.desc.opt_index
        tr = sc.trace(name)[4]
        got = {cap: solo(handles, name, cap) for cap in caps_run(case)}
        for cap in case.caps:
            assert sc.decided(name, cap)
            Qo, dQo, fo, ito, sto, _ = sc.oracle_run(name, cap)
            Qg, dQg, fg, itg, stg = (x[0] for x in got[cap])
            print(f"{name:20s} cap {cap} iters {itg} status {stg} max|Q - oracle| {np.abs(Qg - Qo).max():.3e} "
                  f"max|dQ - oracle| {np.abs(dQg - dQo).max():.3e} rel |f - oracle| {abs(fg - fo) / abs(fo):.3e}")
            assert (itg, stg) == (ito, sto), (name, cap)
            np.testing.assert_allclose(Qg, Qo, rtol=0, atol=1e-9, err_msg=f"{name} cap {cap}")
            np.testing.assert_allclose(dQg, dQo, rtol=0, atol=1e-8, err_msg=f"{name} cap {cap}")
            np.testing.assert_allclose(fg, fo, rtol=1e-9, err_msg=f"{name} cap {cap}")
        # the first evaluation against the restatement: its trial point where it accepts, the seed where it rejects
        want = tr[0]["trial"] if tr[0]["accepted"] else p.Q0
        print(f"{name:20s} cap 1 max|Q - restatement| {np.abs(got[1][0][0] - want).max():.3e}")
        np.testing.assert_allclose(got[1][0][0], want, rtol=0, atol=1e-9, err_msg=name)
        # limits, and frozen variables: the step from the iterate after k evaluations leaves them where they are
        prev = p.Q0
        for cap in caps_run(case):
            Qg = got[cap][0][0]
            assert (Qg[oi] >= d.lower[oi][:, None]).all() and (Qg[oi] <= d.upper[oi][:, None]).all(), (name, cap)
            np.testing.assert_array_equal(Qg[d.param_index], p.Q0[d.param_index])
            np.testing.assert_array_equal(Qg[oi, :2], p.Q0[oi, :2])
            if cap - 1 < len(tr):
                fz = tr[cap - 1]["act"].T                                    # (n, m)
                assert Qg[oi, 2:][fz].tobytes() == prev[oi, 2:][fz].tobytes(), (name, cap)
            prev = Qg
    # which step kernel ran
    names = sc.GROUPS[group][:MAX_B]
    h = handles(group)
    h.set_opts(max_iter=max(sc.CAPS))
    launches = ran(h, batch_args(group, names))
    print(f"{GROUP_IDS[GROUPS.index(group)]}: launches {launches}")
    if sc.robot(group[0])[0].n_opt > 8:
        assert launches["k_lm_step_wide<16>"] > 0, launches
    else:
        assert launches["k_lm_step<8,4>"] > 0 and launches["k_lm_step<4,1>"] == 0, launches


# ------------------------------------------------------------------------------------------------------------ 2. both launch families
@pytest.mark.parametrize("group", NARROW, ids=NARROW_IDS)
def test_both_launch_families_and_deepest_candidate_lists(capi, oracle_mod, handles, monkeypatch, group):
    names = sc.GROUPS[group]
    want = {(nm, cap): solo(handles, nm, cap) for nm in names for cap in sc.CASES[nm].caps}
    monkeypatch.setenv("GTO_FEW_INSTANCES", "0")
    h = make_handle(capi, group)
    for (nm, cap), w in want.items():
        h.set_opts(max_iter=cap)
        got = h.solve_batch(*batch_args(group, [nm]))
        assert same(got, w), (nm, cap, "GTO_FEW_INSTANCES=0", [float(np.abs(a - b).max()) for a, b in zip(got, w)])
    launches = ran(h, batch_args(group, names[:1]))
    h.close()
    assert launches["k_lm_step<4,1>"] > 0 and launches["k_lm_step<8,4>"] == 0, launches
    monkeypatch.delenv("GTO_FEW_INSTANCES")
    for k, v in SPECULATION.items():
        monkeypatch.setenv(k, v)
    h = make_handle(capi, group)
    for (nm, cap), w in want.items():
        h.set_opts(max_iter=cap)
        got = h.solve_batch(*batch_args(group, [nm]))
        assert same(got, w), (nm, cap, "speculation", [float(np.abs(a - b).max()) for a, b in zip(got, w)])
    h.close()


# ------------------------------------------------------------------------------------------------------------ 3. mixed batch
@pytest.mark.parametrize("group", [g for g in GROUPS if len(sc.GROUPS[g]) > 1], ids=[i for g, i in zip(GROUPS, GROUP_IDS) if len(sc.GROUPS[g]) > 1])
def test_mixed_batch_gives_each_instance_its_own_bits(capi, oracle_mod, handles, group):
    names = sc.GROUPS[group]
    h = handles(group)
    for lo in range(0, len(names), MAX_B):
        part = names[lo:lo + MAX_B]
        if len(part) == 1:          # (a lone last case joins the one before it)
            part = names[lo - 1:lo + 1]
        for cap in sc.CAPS:
            h.set_opts(max_iter=cap)
            got = h.solve_batch(*batch_args(group, part))
            for i, nm in enumerate(part):
                w = solo(handles, nm, cap)
                assert same([x[i:i + 1] for x in got], w), (nm, cap, [float(np.abs(a[i] - b[0]).max()) for a, b in zip(got, w)])
