"""GPU: the narrow step kernels compiled for one trajectory length (k_lm_step_t50<4,1> and <8,4>: lm_step_body with
T = GTO_STEP_T_EXACT = 50 a constant), launched at exactly that T.

The constant changes no floating-point expression, reduction order, LDS layout or list protocol, so every output of a call
is the same bits with the exact kernels (GTO_STEP_TEXACT=1) and without them (0): numpy.array_equal on Q, dQ, cost,
iterations and status.  Each setting runs in a fresh child process (step_texact_child.py: all cases once, one .npz),
started once per module.

Cases (the small Panda, a 48^3 scene, max_iter = 12, as smoke()):
  T in {49, 50, 51}, B = 6, each once with GTO_FEW_INSTANCES=0 (the one-candidate kernel with its broad-phase tail) and once
      with the default (the eight-wave kernel with candidates).  Under GTO_DEBUG_TIMING the library reports how many narrow
      step launches of a call were k_lm_step_t50's: all of them at T = 50 under setting 1, none at 49, at 51 or under 0;
  the exit block through its three entrances, at T = 50: the iteration cap and a slot hand-over (B = 10 on GTO_SLOTS=4) in
      P1, a pivot that is not positive behind the meeting block (w_vel = 0: GTO_STATUS_NUMERICAL), and a step below the step
      tolerance in P4 (tol_step = 1e3: GTO_STATUS_CONVERGED);
  the tail's item lists at T = 50 against GTO_PREBROAD=0, where the obstacle launch looks at every group."""
import os
import subprocess
import sys

import numpy as np
import pytest

import step_texact_child as child

pytestmark = pytest.mark.gpu

KEYS = ("Q", "dQ", "cost", "iterations", "status")
CASES = child.cases()


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    """{setting: the child's .npz} for GTO_STEP_TEXACT = 1 and 0"""
    import __graft_entry__ as g
    g.build()
    d = tmp_path_factory.mktemp("step_texact")
    out = {}
    for setting in ("1", "0"):
        path = str(d / f"texact{setting}.npz")
        env = dict(os.environ, GTO_STEP_TEXACT=setting)
        res = subprocess.run([sys.executable, child.__file__, path], env=env, capture_output=True, text=True, timeout=300)
        assert res.returncode == 0, res.stderr[-4000:]
        with np.load(path) as z:
            out[setting] = {k: z[k] for k in z.files}
    return out


@pytest.mark.parametrize("name", sorted(CASES))
def test_same_bits_with_and_without_the_exact_kernels(runs, name):
    T, B, _, _ = CASES[name]
    for key in KEYS:
        a, b = runs["1"][f"{name}.{key}"], runs["0"][f"{name}.{key}"]
        assert a.shape == b.shape and a.shape[0] == B, (name, key, a.shape, b.shape)
        assert np.array_equal(a, b, equal_nan=True), (name, key, np.argwhere(~((a == b) | ((a != a) & (b != b))))[:4].tolist())


@pytest.mark.parametrize("name", child.COUNTED)
def test_exact_kernels_run_at_their_length_and_nowhere_else(runs, name):
    T = CASES[name][0]
    on = int(runs["1"][f"{name}.exact"]), int(runs["1"][f"{name}.other"])
    off = int(runs["0"][f"{name}.exact"]), int(runs["0"][f"{name}.other"])
    print(name, "GTO_STEP_TEXACT=1 (exact, other):", on, " =0:", off)
    assert off[0] == 0 and off[1] >= 1, (name, off)
    if T == 50:
        assert on[0] >= 1 and on[1] == 0, (name, on)
    else:
        assert on[0] == 0 and on[1] >= 1, (name, on)


@pytest.mark.parametrize("name", sorted(n for n in CASES if n.startswith("T") or n.startswith("handover")))
def test_the_clean_cases_do_solve(runs, name):
    """Nothing above would notice two runs that both did nothing: the clean cases move their seeds and end in a known status."""
    from grasptrajopt_amd import _capi
    r = runs["1"]
    assert np.isfinite(r[f"{name}.Q"]).all() and np.isfinite(r[f"{name}.cost"]).all()
    assert (r[f"{name}.iterations"] >= 1).all(), r[f"{name}.iterations"].tolist()
    assert (np.abs(r[f"{name}.dQ"]).max(axis=(1, 2)) > 0).all()
    assert (r[f"{name}.status"] != _capi.GTO_STATUS_NUMERICAL).all()


@pytest.mark.parametrize("kind", ["full", "few"])
def test_the_three_entrances_of_the_exit_block(runs, kind):
    from grasptrajopt_amd import _capi
    for setting in ("1", "0"):
        r = runs[setting]
        it, st = r[f"cap1_{kind}.iterations"], r[f"cap1_{kind}.status"]  # P1: the iteration cap
        assert (it <= 1).all() and (st == _capi.GTO_STATUS_MAX_ITER).any() and (it[st == _capi.GTO_STATUS_MAX_ITER] == 1).all(), (setting, it.tolist(), st.tolist())
        st = r[f"wvel0_{kind}.status"]  # behind the meeting block: a pivot that is not positive
        assert (st == _capi.GTO_STATUS_NUMERICAL).any(), (setting, st.tolist())
        st = r[f"tolstep_{kind}.status"]  # P4: the first trial point lies within the step tolerance
        assert (st == _capi.GTO_STATUS_CONVERGED).all(), (setting, st.tolist())
        assert (r[f"tolstep_{kind}.iterations"] <= 1).all(), (setting, r[f"tolstep_{kind}.iterations"].tolist())


def test_item_lists_of_the_exact_tail_against_every_group_looked_at(runs):
    """GTO_PREBROAD=0 gives every (job, group) an obstacle workgroup; the tail of k_lm_step_t50<4,1> settles the groups no
    sphere of which reaches a non-zero voxel and lists the rest.  What it settles contributes nothing: the same bits."""
    for setting in ("1", "0"):
        r = runs[setting]
        for key in KEYS:
            assert np.array_equal(r[f"T50_full.{key}"], r[f"T50_full_nopb.{key}"]), (setting, key)
