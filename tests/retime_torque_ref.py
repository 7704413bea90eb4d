"""FP64 numpy restatement of gto_retime_paths_torque (include/gto_solver.h), independent of the HIP code: the program of
tests/retime_convex_ref.py with, for every gridpoint i <= N-2 and every joint j with a finite tau_max_j, the two rows

    -tau_max_j <= a_ij c (x_{i+1} - x_i) + b_ij x_i + g_ij <= tau_max_j,        c = (N-1)/2,
    g_i = ID(q_i, 0, 0),   a_i = ID(q_i, 0, p1_i) - g_i,   b_i = ID(q_i, p1_i, p2_i) - g_i,

appended to retime_convex_ref.rows and solved by retime_convex_ref.solve, which takes any A x <= b.  ID is
tests/dynamics_ref.py's inverse dynamics (Newton-Euler in the base frame with full matrices: another formulation than the
kernel's), q / p1 / p2 come from scipy's spline as in tests/retime_ref.py.  A row whose coefficients on the interior
variables are both zero is left out.  The INFEASIBLE rule, the samples and the joint forces at the samples are here too."""
import numpy as np

import dynamics_ref as dr
import retime_convex_ref as cr
import retime_ref as rr

GTO_STATUS_INFEASIBLE = 3
GTO_STATUS_NUMERICAL = cr.GTO_STATUS_NUMERICAL


def payload_of(payload, b):
    """Path b's (mass, com or None, inertia six or None) of a per-path payload (mass (B,), com (B, 3) | None, inertia
    (B, 6) | None), or None."""
    if payload is None:
        return None
    return payload[0][b], None if payload[1] is None else payload[1][b], None if payload[2] is None else payload[2][b]


def coefficients(desc, ee_frame, q, p1, p2, payload=None):
    """(a, b, g), each (N, ndof), at the gridpoints: tau = a u + b x + g along the path."""
    ID = lambda qd, qdd: np.array([dr.inverse_dynamics(desc, q[i], qd[i], qdd[i], ee_frame, payload) for i in range(len(q))])
    zero = np.zeros_like(q)
    g = ID(zero, zero)
    return ID(zero, p1) - g, ID(p1, p2) - g, g


def path_points(plan, subdiv):
    """(q, p1, p2, moving) at the gridpoints of one path (ndof, C), C >= 2, with p1 = p2 = 0 on the joints that do not move."""
    moving = np.any(plan != plan[:, :1], axis=1)
    sp, s, p1, p2 = rr.path_derivatives(plan, subdiv)
    p1[:, ~moving] = 0.0
    p2[:, ~moving] = 0.0
    q = sp(s)
    q[:, ~moving] = plan[~moving, 0]
    return q, p1, p2, moving


def torque_rows(a, b, g, tau_max):
    """The torque rows over the interior variables x_1 .. x_{N-2} as A x <= rhs, and (gridpoint, joint, sign) of each."""
    N = a.shape[0]
    n, c = N - 2, 0.5 * (N - 1)
    A, rhs, who = [], [], []
    for i in range(N - 1):
        for j in np.nonzero(np.isfinite(tau_max))[0]:
            r = np.zeros(n)
            if i + 1 <= N - 2:
                r[i] = a[i, j] * c                     # x_{i+1}
            if i >= 1:
                r[i - 1] = b[i, j] - a[i, j] * c       # x_i
            if not r.any():
                continue
            A.append(r), rhs.append(tau_max[j] - g[i, j]), who.append((i, j, 1))
            A.append(-r), rhs.append(tau_max[j] + g[i, j]), who.append((i, j, -1))
    return np.array(A).reshape(-1, n), np.array(rhs), who


def infeasible(g, tau_max):
    """The rule of the contract: some joint cannot hold the path at rest at some gridpoint 0 .. N-1."""
    return bool(np.any(np.abs(g) >= tau_max))


def program(desc, ee_frame, plan, vmax, amax, tau_max, payload, subdiv):
    """(A, rhs, n_convex_rows, who, (a, b, g)) of a moving path with N >= 3."""
    q, p1, p2, moving = path_points(plan, subdiv)
    A0, b0 = cr.rows(p1, p2, vmax, amax, moving)
    a, b, g = coefficients(desc, ee_frame, q, p1, p2, payload)
    A1, b1, who = torque_rows(a, b, g, tau_max)
    return np.concatenate([A0, A1]), np.concatenate([b0, b1]), len(b0), who, (a, b, g)


def tau_at(desc, ee_frame, q, qd, qdd, payload):
    return np.array([dr.inverse_dynamics(desc, q[i], qd[i], qdd[i], ee_frame, payload) for i in range(len(q))])


def retime_one(desc, ee_frame, plan, vmax, amax, tau_max, payload=None, subdiv=2, M=100, gap_tol=1e-8, max_newton=cr.MAX_NEWTON):
    """dict(duration, t_grid, sd_grid, q, qd, qdd, tau, status, iters) of one path (ndof, C), C >= 1."""
    plan = np.asarray(plan, dtype=np.float64)
    vmax, amax, tau_max = (np.asarray(v, float) for v in (vmax, amax, tau_max))
    ndof, C = plan.shape
    N = subdiv * (C - 1) + 1
    nan = np.full((M, ndof), np.nan)
    none = lambda status: dict(duration=np.nan, t_grid=np.full(N, np.nan), sd_grid=np.full(N, np.nan), q=nan, qd=nan, qdd=nan,
                               tau=nan, status=status, iters=0)
    if not np.all(np.isfinite(plan)):
        return none(GTO_STATUS_NUMERICAL)
    if C == 1:
        g = dr.inverse_dynamics(desc, plan[:, 0], np.zeros(ndof), np.zeros(ndof), ee_frame, payload)
        if not np.all(np.isfinite(g)):
            return none(GTO_STATUS_NUMERICAL)
        if infeasible(g, tau_max):
            return none(GTO_STATUS_INFEASIBLE)
        return dict(duration=0.0, t_grid=np.zeros(1), sd_grid=np.zeros(1), q=np.tile(plan[:, 0], (M, 1)), qd=np.zeros((M, ndof)),
                    qdd=np.zeros((M, ndof)), tau=np.tile(g, (M, 1)), status=0, iters=0)
    q, p1, p2, moving = path_points(plan, subdiv)
    a, b, g = coefficients(desc, ee_frame, q, p1, p2, payload)
    if not (np.all(np.isfinite(a)) and np.all(np.isfinite(b)) and np.all(np.isfinite(g))):
        return none(GTO_STATUS_NUMERICAL)
    if infeasible(g, tau_max):
        return none(GTO_STATUS_INFEASIBLE)
    if not moving.any() or N == 2:  # nothing to solve: the convex call's rules
        r = cr.retime_one(plan, vmax, amax, subdiv, M, gap_tol, max_newton)
        tau = nan if r["status"] == GTO_STATUS_NUMERICAL else tau_at(desc, ee_frame, r["q"], r["qd"], r["qdd"], payload)
        return dict(r, tau=tau)
    A0, b0 = cr.rows(p1, p2, vmax, amax, moving)
    A1, b1, _ = torque_rows(a, b, g, tau_max)
    xi, status, iters = cr.solve(np.concatenate([A0, A1]), np.concatenate([b0, b1]), gap_tol, max_newton)
    if status == GTO_STATUS_NUMERICAL:
        return dict(none(status), iters=iters)
    r = cr.sample(plan, np.concatenate([[0.0], xi, [0.0]]), subdiv, M)
    return dict(r, tau=tau_at(desc, ee_frame, r["q"], r["qd"], r["qdd"], payload), status=status, iters=iters)


def retime_paths_torque_ref(desc, ee_frame, paths, n_cols, vmax, amax, tau_max, payload=None, subdiv=2, M=100, gap_tol=1e-8,
                            max_newton=cr.MAX_NEWTON):
    """The arrays of gto_retime_paths_torque; payload = (mass (B,), com (B, 3) | None, inertia (B, 6) | None) or None."""
    paths = np.asarray(paths, dtype=np.float64)
    nB, ndof, Tp = paths.shape
    Nmax = subdiv * (Tp - 1) + 1
    cols = np.full(nB, Tp) if n_cols is None else np.asarray(n_cols)
    out = dict(duration=np.full(nB, np.nan), t_grid=np.full((nB, Nmax), np.nan), sd_grid=np.full((nB, Nmax), np.nan),
               q=np.full((nB, M, ndof), np.nan), qd=np.full((nB, M, ndof), np.nan), qdd=np.full((nB, M, ndof), np.nan),
               tau=np.full((nB, M, ndof), np.nan), status=np.full(nB, GTO_STATUS_NUMERICAL, dtype=np.int32),
               iters=np.zeros(nB, dtype=np.int32))
    for b in range(nB):
        C = int(cols[b])
        if C < 1 or C > Tp:
            continue
        r = retime_one(desc, ee_frame, paths[b][:, :C], vmax, amax, tau_max, payload_of(payload, b), subdiv, M, gap_tol, max_newton)
        N = subdiv * (C - 1) + 1
        out["duration"][b], out["status"][b], out["iters"][b] = r["duration"], r["status"], r["iters"]
        if r["status"] in (GTO_STATUS_INFEASIBLE,) or np.isnan(r["duration"]):
            continue  # NaN over all Nmax grid entries
        out["t_grid"][b, :N], out["sd_grid"][b, :N] = r["t_grid"], r["sd_grid"]
        out["t_grid"][b, N:], out["sd_grid"][b, N:] = r["duration"], 0.0
        for k in ("q", "qd", "qdd", "tau"):
            out[k][b] = r[k]
    return out
