"""FP64 numpy restatement of gto_retime_paths_convex (include/gto_solver.h), independent of the HIP code: the time-optimal
profile on the fixed grid as a convex program,

    minimise  T(x) = sum_i 2 Delta / (sqrt x_i + sqrt x_{i+1}),   x_0 = x_{N-1} = 0,
    subject to 0 <= x_i <= xcap_i and -alpha + beta x_i <= (x_{i+1} - x_i) (N-1)/2 <= alpha + beta x_i for every line,

with the rows of tests/retime_ref.py (path_derivatives, _lines, x_bounds) and a log-barrier Newton method of its own: dense
rows, numpy's solver for the Newton system.  The samples are retime_ref.retime_one's, on the new x."""
import numpy as np

import retime_ref as rr

GTO_STATUS_MAX_ITER = 1
GTO_STATUS_NUMERICAL = rr.GTO_STATUS_NUMERICAL
MAX_NEWTON = 400       # the default of the Python layers
SHRINK = 0.1           # barrier weight per outer round
CENTRED = 0.25         # Newton decrement below which an iterate counts as centred


def rows(p1, p2, vmax, amax, moving):
    """The constraints on the interior variables x_1 .. x_{N-2} as A x <= b (dense), every row strictly satisfiable."""
    N = p1.shape[0]
    n = N - 2
    c = 0.5 * (N - 1)
    cap = rr.x_bounds(p1, p2, vmax, amax, moving)
    mv = np.nonzero(moving)[0]
    A, b = [], []

    def unit(i, s):  # s x_i as a row over the interior variables (x_0 and x_{N-1} are 0)
        r = np.zeros(n)
        if 1 <= i <= N - 2:
            r[i - 1] = s
        return r

    for i in range(1, N - 1):
        A.append(unit(i, -1.0)), b.append(0.0)
        if np.isfinite(cap[i]):
            A.append(unit(i, 1.0)), b.append(cap[i])
    for i in range(N - 1):
        al, be = rr._lines(p1[i, mv], p2[i, mv], amax[mv])
        for a_, b_ in zip(al, be):
            r = unit(i + 1, c) + unit(i, -c - b_)   # u_i - beta x_i
            A.append(r), b.append(a_)
            A.append(-r), b.append(a_)
    return np.array(A).reshape(-1, n), np.array(b)


def total_time(x):
    """T of the interior variables x (x_0 = x_{N-1} = 0 appended)."""
    sd = np.sqrt(np.concatenate([[0.0], x, [0.0]]))
    return float(np.sum((2.0 / (len(sd) - 1)) / (sd[:-1] + sd[1:])))


def time_derivatives(x):
    """Gradient (n,) and Hessian (n, n, tridiagonal) of T at the interior variables x."""
    n = len(x)
    N = n + 2
    w = 2.0 / (N - 1)
    sd = np.sqrt(np.concatenate([[0.0], x, [0.0]]))
    g, H = np.zeros(n), np.zeros((n, n))
    for i in range(N - 1):  # f = 1 / (p + q), p = sqrt x_i, q = sqrt x_{i+1}
        p, q = sd[i], sd[i + 1]
        S = p + q
        if i >= 1:
            g[i - 1] += -w / (2 * p * S ** 2)
            H[i - 1, i - 1] += w * (1 / (4 * p ** 3 * S ** 2) + 1 / (2 * p ** 2 * S ** 3))
        if i + 1 <= N - 2:
            g[i] += -w / (2 * q * S ** 2)
            H[i, i] += w * (1 / (4 * q ** 3 * S ** 2) + 1 / (2 * q ** 2 * S ** 3))
        if i >= 1 and i + 1 <= N - 2:
            H[i - 1, i] += w / (2 * p * q * S ** 3)
            H[i, i - 1] += w / (2 * p * q * S ** 3)
    return g, H


def solve(A, b, gap_tol=1e-8, max_newton=MAX_NEWTON):
    """(x, status, Newton steps): log-barrier path following on F = T + mu * -sum log(b - A x).  Stops at an iterate whose
    Newton decrement lam is below CENTRED and whose gap bound mu (m + (lam + sqrt m) lam / (1 - lam)) is at most
    gap_tol * T(x) (m mu at the centre itself)."""
    m, n = A.shape
    with np.errstate(divide="ignore"):
        eps = 0.5 * np.min(np.where(A.sum(axis=1) > 0, b / np.where(A.sum(axis=1) > 0, A.sum(axis=1), 1.0), np.inf))
    x = np.full(n, eps)
    mu = total_time(x) / m

    def F(y, mu):
        s = b - A @ y
        if np.any(s <= 0) or np.any(y <= 0):
            return np.inf
        return total_time(y) - mu * np.sum(np.log(s))

    it = 0
    while True:
        s = b - A @ x
        gT, HT = time_derivatives(x)
        g = gT + mu * (A.T @ (1.0 / s))
        H = HT + mu * (A.T * (1.0 / s ** 2)) @ A
        dx = -np.linalg.solve(H, g)
        if not np.all(np.isfinite(dx)):
            return x, GTO_STATUS_NUMERICAL, it
        lam = np.sqrt(max(-(g @ dx), 0.0) / mu)
        if lam < CENTRED:
            if mu * (m + (lam + np.sqrt(m)) * lam / (1 - lam)) <= gap_tol * total_time(x):
                return x, 0, it
            mu *= SHRINK  # the next weight, from the same x: not a Newton step
            continue
        if it == max_newton:
            return x, GTO_STATUS_MAX_ITER, it
        ds = -(A @ dx)
        with np.errstate(divide="ignore", invalid="ignore"):
            eta = min(1.0, 0.99 * np.min(np.where(ds < 0, s / np.where(ds < 0, -ds, 1.0), np.inf)))
        F0, slope = F(x, mu), g @ dx
        for _ in range(60):  # backtracking; differences below the round-off of F count as a decrease
            if F(x + eta * dx, mu) <= F0 + 1e-4 * eta * slope + 4e-16 * abs(F0):
                x = x + eta * dx
                break
            eta *= 0.5
        it += 1


def retime_one(plan, vmax, amax, subdiv=2, M=100, gap_tol=1e-8, max_newton=MAX_NEWTON):
    """dict(duration, t_grid, sd_grid, q, qd, qdd, status, iters) of one path (ndof, C), C >= 2."""
    plan = np.asarray(plan, dtype=np.float64)
    vmax, amax = np.asarray(vmax, float), np.asarray(amax, float)
    ndof, C = plan.shape
    N = subdiv * (C - 1) + 1
    nan = np.full((M, ndof), np.nan)
    if not np.all(np.isfinite(plan)):
        return dict(duration=np.nan, t_grid=np.full(N, np.nan), sd_grid=np.full(N, np.nan), q=nan, qd=nan, qdd=nan,
                    status=GTO_STATUS_NUMERICAL, iters=0)
    moving = np.any(plan != plan[:, :1], axis=1)
    if not moving.any():
        r = rr.retime_one(plan, vmax, amax, subdiv, M)
        return dict(r, iters=0)
    if N == 2:  # no variable: both ends rest
        return dict(duration=np.inf, t_grid=np.array([0.0, np.inf]), sd_grid=np.zeros(2), q=nan, qd=nan, qdd=nan,
                    status=GTO_STATUS_NUMERICAL, iters=0)
    sp, s, p1, p2 = rr.path_derivatives(plan, subdiv)
    p1[:, ~moving] = 0.0
    p2[:, ~moving] = 0.0
    A, b = rows(p1, p2, vmax, amax, moving)
    xi, status, iters = solve(A, b, gap_tol, max_newton)
    x = np.concatenate([[0.0], xi, [0.0]])
    if status == GTO_STATUS_NUMERICAL:
        return dict(duration=np.nan, t_grid=np.full(N, np.nan), sd_grid=np.full(N, np.nan), q=nan, qd=nan, qdd=nan,
                    status=status, iters=iters)
    r = sample(plan, x, subdiv, M)
    return dict(r, status=status, iters=iters)


def sample(plan, x, subdiv, M):
    """Times and samples of profile x (N,) on the path: retime_ref.retime_one's code from its profile on, with x given."""
    keep = rr.profile, rr.STALL
    rr.profile, rr.STALL = (lambda *a: (x, None)), -1.0  # the stall rule is the greedy pass's: not applied here
    try:
        r = rr.retime_one(plan, np.full(plan.shape[0], np.inf), np.ones(plan.shape[0]), subdiv, M)
    finally:
        rr.profile, rr.STALL = keep
    return r


def retime_paths_convex_ref(paths, n_cols, vmax, amax, subdiv=2, M=100, gap_tol=1e-8, max_newton=MAX_NEWTON):
    """The arrays of gto_retime_paths_convex: those of retime_paths_ref.retime_paths_ref, and iters (B,)."""
    paths = np.asarray(paths, dtype=np.float64)
    nB, ndof, Tp = paths.shape
    Nmax = subdiv * (Tp - 1) + 1
    cols = np.full(nB, Tp) if n_cols is None else np.asarray(n_cols)
    out = dict(duration=np.full(nB, np.nan), t_grid=np.full((nB, Nmax), np.nan), sd_grid=np.full((nB, Nmax), np.nan),
               q=np.full((nB, M, ndof), np.nan), qd=np.full((nB, M, ndof), np.nan), qdd=np.full((nB, M, ndof), np.nan),
               status=np.full(nB, GTO_STATUS_NUMERICAL, dtype=np.int32), iters=np.zeros(nB, dtype=np.int32))
    for b in range(nB):
        C = int(cols[b])
        if C < 1 or C > Tp or not np.all(np.isfinite(paths[b][:, :C])):
            continue
        if C == 1:
            r = dict(duration=0.0, t_grid=np.zeros(1), sd_grid=np.zeros(1), q=np.tile(paths[b][:, 0], (M, 1)),
                     qd=np.zeros((M, ndof)), qdd=np.zeros((M, ndof)), status=0, iters=0)
        else:
            r = retime_one(paths[b][:, :C], vmax, amax, subdiv, M, gap_tol, max_newton)
        N = subdiv * (C - 1) + 1
        out["duration"][b], out["status"][b], out["iters"][b] = r["duration"], r["status"], r["iters"]
        out["t_grid"][b, :N], out["sd_grid"][b, :N] = r["t_grid"], r["sd_grid"]
        out["t_grid"][b, N:], out["sd_grid"][b, N:] = r["duration"], 0.0
        for k in ("q", "qd", "qdd"):
            out[k][b] = r[k]
    return out
