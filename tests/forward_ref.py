"""Forward dynamics and the tracking rollout in numpy FP64: the yardstick of gto_forward_dynamics and gto_track_rollout (no
GPU here), built on tests/dynamics_ref.py.

forward_dynamics takes the mass matrix from the JACOBIAN SUM (mass_matrix of tests/test_dynamics_cpu.py: sum over the bodies
of m Jv^T Jv + Jw^T R I R^T Jw), not from unit-acceleration passes as the kernel does (csrc/gto_forward.h), the bias from
dynamics_ref.inverse_dynamics, and solves with numpy's LAPACK.  rollout is the contract of include/gto_solver.h written
plainly, one path at a time.  columns=True builds M from ID(q, 0, e_j) - g columns instead (symmetrised): the other ordering
of the same sums, used only to measure how far round-off alone moves a rollout (tests/test_gpu_forward.py's tolerance).
tests/test_forward_cpu.py holds all of it against physics.
"""
import math

import numpy as np

import dynamics_ref as dr
from test_dynamics_cpu import mass_matrix, potential

CONVERGED, NUMERICAL = 0, 2
MAX_STEPS = 1 << 20


def free_joints(desc, locked=None):
    """(ndof,) bool: the joints some actuated frame names and `locked` does not mark; locked=None locks every joint that is
    not optimised."""
    named = np.zeros(desc.ndof, dtype=bool)
    for f in range(desc.n_frames):
        if desc.joint_type[f] != 0 and desc.q_index[f] >= 0:
            named[desc.q_index[f]] = True
    if locked is None:
        lk = np.ones(desc.ndof, dtype=bool)
        lk[np.asarray(desc.opt_index, dtype=int)] = False
    else:
        lk = np.asarray(locked) != 0
    return named & ~lk


def named_joints(desc):
    return free_joints(desc, np.zeros(desc.ndof))


def mass_matrix_columns(desc, q, ee, payload):
    """M from unit accelerations, symmetrised: the kernel's formulation."""
    zero = np.zeros(desc.ndof)
    g = dr.inverse_dynamics(desc, q, zero, zero, ee, payload)
    M = np.stack([dr.inverse_dynamics(desc, q, zero, e, ee, payload) - g for e in np.eye(desc.ndof)], axis=1)
    return 0.5 * (M + M.T)


def forward_dynamics(desc, q, qd, tau, ee=None, payload=None, locked=None, columns=False):
    """(qdd (ndof,), M (ndof, ndof)) at one state: M_ff qdd_f = (tau - ID(q, qd, 0))_f on the free joints, 0 elsewhere; a NaN
    qdd where M_ff is not positive definite or an input is not finite."""
    q, qd, tau = (np.asarray(x, dtype=np.float64) for x in (q, qd, tau))
    fr = free_joints(desc, locked)
    if not (np.isfinite(q).all() and np.isfinite(qd).all() and np.isfinite(tau).all()):
        return np.full(desc.ndof, np.nan), np.full((desc.ndof, desc.ndof), np.nan)
    M = mass_matrix_columns(desc, q, ee, payload) if columns else mass_matrix(desc, q, ee, payload)
    c = dr.inverse_dynamics(desc, q, qd, np.zeros(desc.ndof), ee, payload)
    qdd = np.zeros(desc.ndof)
    if fr.any():
        Mff = M[np.ix_(fr, fr)]
        try:
            if not (np.diag(Mff) > 0).all():
                raise np.linalg.LinAlgError
            np.linalg.cholesky(Mff)
            qdd[fr] = np.linalg.solve(Mff, (tau - c)[fr])
        except np.linalg.LinAlgError:
            qdd[:] = np.nan
    return qdd, M


def reference_at(t, duration, q_ref, qd_ref, qdd_ref):
    """(q, qd, qdd) (ndof,) of the reference at time t: cubic Hermite in (q_m, qd_m), its derivative, qdd_m joined by lines;
    the last sample at rest from t = duration on."""
    M = q_ref.shape[0]
    if not t < duration:
        return q_ref[-1].copy(), np.zeros(q_ref.shape[1]), np.zeros(q_ref.shape[1])
    h = duration / (M - 1)
    s = t / duration * (M - 1)
    i = min(int(s), M - 2)
    u = s - i
    u2, u3 = u * u, u * u * u
    q0, q1, v0, v1 = q_ref[i], q_ref[i + 1], qd_ref[i], qd_ref[i + 1]
    q = (2 * u3 - 3 * u2 + 1) * q0 + (u3 - 2 * u2 + u) * (h * v0) + (3 * u2 - 2 * u3) * q1 + (u3 - u2) * (h * v1)
    qd = (6 * u2 - 6 * u) * (q0 - q1) / h + (3 * u2 - 4 * u + 1) * v0 + (3 * u2 - 2 * u) * v1
    return q, qd, (1 - u) * qdd_ref[i] + u * qdd_ref[i + 1]


def energy(desc, q, qd, ee=None, payload=None):
    """T + V of the state, T from the Jacobian mass matrix."""
    return 0.5 * qd @ mass_matrix(desc, q, ee, payload) @ qd + potential(desc, q, ee, payload)


def rollout(desc, ee, duration, q_ref, qd_ref, qdd_ref, kp, kd, tau_max, dt=1e-3, settle=0.0, n_samples=100, feedforward=2,
            model_payload=None, plant_payload=None, locked=None, columns=False):
    """One path.  Returns a dict q, qd (n_samples, ndof), t (n_samples,), err_max, err_end, sat_steps, steps, status and, for
    the tests' own use, clip_margin: the smallest | |tau_raw| - tau_max | / tau_max over the steps and the free joints with
    a finite limit (inf without one): how close the run came to a clip decision."""
    nd, Mo = desc.ndof, int(n_samples)
    q_ref, qd_ref, qdd_ref = (np.asarray(x, dtype=np.float64) for x in (q_ref, qd_ref, qdd_ref))
    kp, kd, tau_max = (np.broadcast_to(np.asarray(x, dtype=np.float64), (nd,)) for x in (kp, kd, tau_max))
    fr = free_joints(desc, locked)
    bad = dict(q=np.full((Mo, nd), np.nan), qd=np.full((Mo, nd), np.nan), t=np.full(Mo, np.nan), err_max=np.nan, err_end=np.nan,
               sat_steps=0, steps=0, status=NUMERICAL, clip_margin=np.inf)
    if not (np.isfinite(duration) and duration >= 0):
        return bad
    Kd = math.ceil((duration + settle) / dt)
    if not 1 <= Kd <= MAX_STEPS:
        return bad
    if not (np.isfinite(q_ref[:, fr]).all() and np.isfinite(qd_ref[:, fr]).all() and np.isfinite(qdd_ref[:, fr]).all()
            and np.isfinite(q_ref[0]).all()):
        return bad
    K = int(Kd)
    q0 = q_ref[0].copy()

    def ref(t):
        a, b, c = reference_at(t, duration, q_ref, qd_ref, qdd_ref)
        return np.where(fr, a, q0), np.where(fr, b, 0.0), np.where(fr, c, 0.0)

    def fd(q, qd, tau):
        return forward_dynamics(desc, q, qd, tau, ee, plant_payload, ~fr, columns)[0]

    q, qd = q0.copy(), np.where(fr, qd_ref[0], 0.0)
    km = [m * K // (Mo - 1) for m in range(Mo)]
    out = dict(q=np.zeros((Mo, nd)), qd=np.zeros((Mo, nd)), t=np.zeros(Mo), clip_margin=np.inf)

    def emit(k):
        for m in range(Mo):
            if km[m] == k:
                out["q"][m], out["qd"][m], out["t"][m] = q, qd, k * dt

    emit(0)
    zero = np.zeros(nd)
    err_max = err_end = 0.0
    sat = 0
    rq, rqd, rqdd = ref(0.0)
    for k in range(K):
        if feedforward == 0:
            ff = zero
        elif feedforward == 1:
            ff = dr.inverse_dynamics(desc, rq, zero, zero, ee, model_payload)
        else:
            ff = dr.inverse_dynamics(desc, rq, rqd, rqdd, ee, model_payload)
        raw = np.where(fr, ff + kp * (rq - q) + kd * (rqd - qd), 0.0)
        tau = np.where(fr, np.clip(raw, -tau_max, tau_max), 0.0)
        sat += int((tau != raw).any())
        lim = fr & np.isfinite(tau_max)
        if lim.any():
            out["clip_margin"] = min(out["clip_margin"], np.min(np.abs(np.abs(raw[lim]) - tau_max[lim]) / tau_max[lim]))
        k1q, k1v = qd, fd(q, qd, tau)
        k2q, k2v = qd + 0.5 * dt * k1v, fd(q + 0.5 * dt * k1q, qd + 0.5 * dt * k1v, tau)
        k3q, k3v = qd + 0.5 * dt * k2v, fd(q + 0.5 * dt * k2q, qd + 0.5 * dt * k2v, tau)
        k4q, k4v = qd + dt * k3v, fd(q + dt * k3q, qd + dt * k3v, tau)
        q = np.where(fr, q + dt / 6.0 * (k1q + 2.0 * k2q + 2.0 * k3q + k4q), q)
        qd = np.where(fr, qd + dt / 6.0 * (k1v + 2.0 * k2v + 2.0 * k3v + k4v), 0.0)
        if not (np.isfinite(q).all() and np.isfinite(qd).all()):
            return bad
        rq, rqd, rqdd = ref((k + 1) * dt)
        err_end = float(np.abs(q - rq)[fr].max()) if fr.any() else 0.0
        err_max = max(err_max, err_end)
        emit(k + 1)
    out.update(err_max=err_max, err_end=err_end, sat_steps=sat, steps=K, status=CONVERGED)
    return out


def rollout_batch(desc, ee, duration, q_ref, qd_ref, qdd_ref, kp, kd, tau_max, model_payload=None, plant_payload=None, **kw):
    """rollout over the paths of a batch; payloads as (mass (B,), com (B, 3) or None, inertia (B, 6) or None) or None.  The
    dict's entries are stacked."""
    def row(pl, b):
        return None if pl is None else (pl[0][b], None if pl[1] is None else pl[1][b], None if pl[2] is None else pl[2][b])

    res = [rollout(desc, ee, duration[b], q_ref[b], qd_ref[b], qdd_ref[b], kp, kd, tau_max, model_payload=row(model_payload, b),
                   plant_payload=row(plant_payload, b), **kw) for b in range(len(duration))]
    return {k: np.stack([np.asarray(r[k]) for r in res]) for k in res[0]}
