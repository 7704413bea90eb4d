"""GPU: the narrow step kernels by class of trajectory length (k_lm_step_short for T <= GTO_STEP_T_SHORT = 50, k_lm_step
beyond) and their single exit block.

The short instantiation runs the same arithmetic in the same order on the same LDS layout with half the unrolled bodies, so
every output of a call is the same bits with it (GTO_STEP_TCLASS=1, the default) and with the general instantiation at every T
(GTO_STEP_TCLASS=0): numpy.array_equal on Q, dQ, cost, iterations and status.  Each setting runs in a fresh child process
(step_tclass_child.py: all cases once, one .npz), started once per module.

Cases (the small Panda, a 48^3 scene, max_iter = 12, as smoke()):
  T in {4, 30, 49, 50, 51, 96}, B = 6: 4 is the smallest T gto_create accepts, 50 and 51 straddle the class boundary, 51 and 96
      take the general kernel under either setting;
  each once with GTO_FEW_INSTANCES=0 (the one-candidate kernel with its broad-phase tail) and once with the default (the
      eight-wave kernel with candidates);
  the exit block: B = 10 on GTO_SLOTS=4 (finishing workgroups hand their slot over), max_iter 1 and 2 (the cap's exit) and an
      instance whose seed holds a NaN (GTO_STATUS_NUMERICAL with 0 iterations, as test_gpu_parity.py states it)."""
import os
import subprocess
import sys

import numpy as np
import pytest

import step_tclass_child as child

pytestmark = pytest.mark.gpu

KEYS = ("Q", "dQ", "cost", "iterations", "status")
CASES = child.cases()


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    """{setting: the child's .npz} for GTO_STEP_TCLASS = 1 and 0"""
    import __graft_entry__ as g
    g.build()
    d = tmp_path_factory.mktemp("step_tclass")
    out = {}
    for setting in ("1", "0"):
        path = str(d / f"tclass{setting}.npz")
        env = dict(os.environ, GTO_STEP_TCLASS=setting)
        res = subprocess.run([sys.executable, child.__file__, path], env=env, capture_output=True, text=True, timeout=300)
        assert res.returncode == 0, res.stderr[-4000:]
        with np.load(path) as z:
            out[setting] = {k: z[k] for k in z.files}
    return out


@pytest.mark.parametrize("name", sorted(CASES))
def test_same_bits_with_and_without_the_short_instantiation(runs, name):
    T, B, _, max_iter, _ = CASES[name]
    for key in KEYS:
        a, b = runs["1"][f"{name}.{key}"], runs["0"][f"{name}.{key}"]
        assert a.shape == b.shape and a.shape[0] == B, (name, key, a.shape, b.shape)
        assert np.array_equal(a, b, equal_nan=True), (name, key, np.argwhere(~((a == b) | ((a != a) & (b != b))))[:4].tolist())
    it = runs["1"][f"{name}.iterations"]
    assert (it <= max_iter).all(), (name, it.tolist())


@pytest.mark.parametrize("name", sorted(n for n in CASES if n.startswith("T") or n.startswith("handover")))
def test_the_cases_do_solve(runs, name):
    """Nothing above would notice two runs that both did nothing: the clean cases move their seeds and end in a known status."""
    from grasptrajopt_amd import _capi
    r = runs["1"]
    assert np.isfinite(r[f"{name}.Q"]).all() and np.isfinite(r[f"{name}.cost"]).all()
    assert (r[f"{name}.iterations"] >= 1).all(), r[f"{name}.iterations"].tolist()
    assert (np.abs(r[f"{name}.dQ"]).max(axis=(1, 2)) > 0).all()
    assert (r[f"{name}.status"] != _capi.GTO_STATUS_NUMERICAL).all()


@pytest.mark.parametrize("kind", ["full", "few"])
def test_iteration_cap_leaves_through_the_exit_block(runs, kind):
    from grasptrajopt_amd import _capi
    for setting in ("1", "0"):
        for cap in (1, 2):
            it, st = runs[setting][f"cap{cap}_{kind}.iterations"], runs[setting][f"cap{cap}_{kind}.status"]
            assert (it <= cap).all() and (it[st == _capi.GTO_STATUS_MAX_ITER] == cap).all(), (setting, cap, it.tolist(), st.tolist())
            assert (st == _capi.GTO_STATUS_MAX_ITER).any(), (setting, cap, st.tolist())


@pytest.mark.parametrize("kind", ["full", "few"])
def test_nan_seed_ends_in_status_numerical(runs, kind):
    """... with 0 iterations, for exactly that instance; its neighbours get the bits of the clean batch (T50 of the same kind)."""
    from grasptrajopt_amd import _capi
    for setting in ("1", "0"):
        r = runs[setting]
        st, it = r[f"nan_{kind}.status"], r[f"nan_{kind}.iterations"]
        bad = child.NAN_INSTANCE
        assert st[bad] == _capi.GTO_STATUS_NUMERICAL and it[bad] == 0, (setting, st.tolist(), it.tolist())
        ok = np.setdiff1d(np.arange(len(st)), [bad])
        assert (st[ok] != _capi.GTO_STATUS_NUMERICAL).all()
        for key in KEYS:
            assert np.array_equal(r[f"nan_{kind}.{key}"][ok], r[f"T50_{kind}.{key}"][ok]), (setting, key)
