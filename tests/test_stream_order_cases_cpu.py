"""CPU: the case builders of the stream-order tests (tests/stream_order_cases.py).  A decoy has to be a valid problem, or a
read that races would be an invalid access instead of a wrong answer, and it has to differ from the true inputs in every
array, or a race on that array could not be seen."""
import numpy as np
import pytest

import stream_order_cases as soc

CHECK_REGROW = sorted({e for run in soc.REGROW_RUNS.values() for e in run})
ALL_ENTRIES = soc.ENTRIES + [e for e in CHECK_REGROW if e not in soc.ENTRIES]


def _all_cases():
    for entry in soc.ENTRIES:
        for B in soc.BS:
            yield entry, B
    for entry in CHECK_REGROW:
        for B in soc.REGROW_BS:
            yield entry, B


@pytest.mark.parametrize("entry", ALL_ENTRIES)
def test_true_inputs_and_decoys_are_valid_problems(entry):
    for e, B in _all_cases():
        if e != entry:
            continue
        for decoy in (False, True):
            case = soc.inputs(e, B, decoy=decoy)
            assert soc.valid(case) == [], (e, B, decoy)
            for name in ("n_goals", "n_grasps"):
                for part in (case.dev, case.host):
                    if name in part:
                        assert part[name].dtype == np.int32 and part[name].min() >= 1 and part[name].max() <= soc.N_MAX


@pytest.mark.parametrize("entry", ALL_ENTRIES)
def test_decoys_have_the_shapes_of_the_true_inputs_and_differ_in_every_array(entry):
    for e, B in _all_cases():
        if e != entry:
            continue
        true, decoy = soc.inputs(e, B), soc.inputs(e, B, decoy=True)
        assert true.outs == decoy.outs
        for part in ("dev", "host"):
            a, b = getattr(true, part), getattr(decoy, part)
            assert list(a) == list(b)
            for name in a:
                assert a[name].shape == b[name].shape and a[name].dtype == b[name].dtype, (e, B, name)
                assert not np.array_equal(a[name], b[name]), (e, B, name)
                assert not a[name].flags.writeable  # shared between tests: nobody changes a case


def test_valid_notices_what_it_is_there_for():
    case = soc.inputs("solve", 3)
    broken = lambda **kw: soc.SimpleNamespace(**{**vars(case), "dev": {**case.dev, **kw}})
    assert any("n_goals" in r for r in soc.valid(broken(n_goals=np.array([1, 0, 2], np.int32))))
    assert any("n_goals" in r for r in soc.valid(broken(n_goals=np.array([1, soc.N_MAX + 1, 2], np.int32))))
    assert any("scene_id" in r for r in soc.valid(broken(scene_id=np.array([0, 2, 1], np.int32))))
    qc = case.dev["qc"].copy()
    qc[1, 3] = 0.5  # the Panda's fourth joint ends at -0.0698
    assert any("qc" in r for r in soc.valid(broken(qc=qc)))
    goals = case.dev["goals"].copy()
    goals[0, 0, 5] = np.nan
    assert any("goals" in r for r in soc.valid(broken(goals=goals)))


def test_the_rig_is_the_one_the_tests_state():
    desc, cfg = soc.robot()
    assert desc.n_opt <= 8 and soc.T + soc.STANDOFF_OFFSET >= 2
    assert soc.T + soc.STANDOFF_OFFSET - 10 < 0 <= soc.T_REVERSE + soc.STANDOFF_OFFSET - 10  # why the reverse path has its own horizon
    depth, K, cam = soc.depth_observation()
    assert depth.shape == (12, 16) and depth.dtype == np.float32
    pts, nrm = soc.cloud_observation()
    assert pts.shape == nrm.shape == (65, 3) and np.allclose(np.linalg.norm(nrm, axis=1), 1.0)
    assert soc.FILTER_OBS == (0, 1, 1, 0)
    assert len(soc.REGROW_BS) > 4  # more calls in flight than pinned slots
    from grasptrajopt_amd import _capi
    assert soc.CONVEX_MAX_NEWTON == _capi.RETIME_MAX_NEWTON and soc.CONVEX_GAP_TOL == 1e-8
    assert "retime_paths_convex" in soc.NO_HOST_SYNC
    assert soc.REGROW_RUNS["retime"] == ("retime_paths", "retime_paths_convex", "retime_paths_torque")
    for B in soc.BS + soc.REGROW_BS:  # the convex call: the greedy call's arrays and an iteration count per path
        a, b = soc.inputs("retime_paths", B), soc.inputs("retime_paths_convex", B)
        assert list(a.dev) == list(b.dev) and list(a.host) == list(b.host) == ["vmax", "amax"]
        assert b.outs == {**a.outs, "iters": ((B,), np.dtype(np.int32))} and b.dev["n_cols"].min() >= 3
    sc = soc.scenes()
    assert len(sc) == 2 and tuple(sc[0].shape) == (32, 32, 32) and not np.array_equal(sc[0].c_obs, sc[1].c_obs)


def test_the_torque_retime_and_the_rollout_are_entries_with_their_host_arrays():
    """Both new entries run in the four modes of the common rig and must return under the hold; their HOST arrays are the ones
    include/gto_solver.h marks HOST, the payloads are device arrays, and the rig's Panda carries link inertials."""
    desc, _ = soc.robot()
    assert desc.has_inertials and np.isfinite(desc.effort).all() and (desc.effort > 0).all()
    for e in ("retime_paths_torque", "track_rollout"):
        assert e in soc.ENTRIES and e in soc.NO_HOST_SYNC
    for B in soc.BS + soc.REGROW_BS:
        a, b = soc.inputs("retime_paths_convex", B), soc.inputs("retime_paths_torque", B)
        assert list(b.host) == ["vmax", "amax", "tau_max"] and list(b.dev) == list(a.dev) + ["payload_mass", "payload_com", "payload_inertia"]
        assert b.outs == {**a.outs, "tau": ((B, soc.M_SAMPLES, desc.ndof), np.dtype(np.float64))}
        assert (b.host["tau_max"] >= 1.2 * desc.effort).all() and b.dev["payload_inertia"].shape == (B, 6)
    for B in soc.BS:
        for decoy in (False, True):
            c = soc.inputs("track_rollout", B, decoy=decoy)
            assert list(c.host) == ["kp", "kd", "tau_max", "locked"] and c.host["locked"].dtype == np.int32
            assert c.host["locked"][desc.param_index].all() and c.host["locked"][desc.opt_index].sum() == 1
            assert list(c.dev) == ["duration", "q_ref", "qd_ref", "qdd_ref", "model_mass", "plant_mass", "plant_com", "plant_inertia"]
            assert c.dev["q_ref"].shape == (B, soc.TRACK_M, desc.ndof) and c.outs["q"][0] == (B, soc.TRACK_MO, desc.ndof)
            steps = np.ceil((c.dev["duration"] + soc.TRACK_SETTLE) / soc.TRACK_DT)
            assert (soc.TRACK_M, soc.TRACK_MO) == (5, 4) and steps.min() >= 4 and steps.max() <= 10
        assert not np.array_equal(soc.inputs("track_rollout", B).host["locked"], soc.inputs("track_rollout", B, decoy=True).host["locked"])
