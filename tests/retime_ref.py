"""FP64 numpy restatement of the retiming contract (include/gto_solver.h gto_retime_batch), independent of the HIP code:
the path comes from scipy's CubicSpline, each stage LP is solved by enumerating the vertices of its bounds, and the
grid constraints are also written out as LPs (grid_lp, controllable_lp) that scipy's HiGHS solves independently."""
import numpy as np
from scipy.interpolate import CubicSpline

GTO_STATUS_NUMERICAL = 2
STALL = 1e-6  # a segment with x <= STALL * max x at both ends: the profile rests there, status GTO_STATUS_NUMERICAL


def random_plans(desc, B, T, seed):
    """B smooth random plans (B, ndof, T) inside the joint limits; parameter rows constant, as in a solved plan."""
    rng = np.random.default_rng(seed)
    lo, hi = np.maximum(desc.lower, -3.0), np.minimum(desc.upper, 3.0)
    s = np.linspace(0.0, 1.0, T)
    a = lo + (hi - lo) * rng.uniform(0.2, 0.8, (B, desc.ndof))
    b = lo + (hi - lo) * rng.uniform(0.2, 0.8, (B, desc.ndof))
    P = a[..., None] + (b - a)[..., None] * (3 * s ** 2 - 2 * s ** 3)
    P += 0.05 * np.sin(2 * np.pi * rng.uniform(0.5, 2.0, (B, desc.ndof, 1)) * s + rng.uniform(0, 6, (B, desc.ndof, 1)))
    P[:, desc.param_index] = P[:, desc.param_index, :1]
    return P


def path_derivatives(plan, subdiv):
    """(spline, s grid (N,), p1 (N, ndof), p2 (N, ndof)) of one plan (ndof, T)."""
    T = plan.shape[1]
    sp = CubicSpline(np.linspace(0.0, 1.0, T), plan.T, bc_type="not-a-knot")
    s = np.linspace(0.0, 1.0, subdiv * (T - 1) + 1)
    return sp, s, sp(s, 1), sp(s, 2)


def _has_line(a, b, amax):
    """Joints whose acceleration limit bounds u: p1 != 0 and neither amax/|p1| nor p2/p1 overflows."""
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        return np.isfinite(amax / np.abs(a)) & np.isfinite(b / a)


def _lines(a, b, amax):
    """Upper bounds u <= alpha + beta x and lower bounds u >= -alpha + beta x of the joints that have one."""
    nz = _has_line(a, b, amax)
    return amax[nz] / np.abs(a[nz]), -b[nz] / a[nz]


def x_bounds(p1, p2, vmax, amax, moving):
    """The cap on x at every gridpoint that does not involve u."""
    N = p1.shape[0]
    cap = np.full(N, np.inf)
    for i in range(N):
        for j in np.nonzero(moving)[0]:
            if p1[i, j] != 0 and np.isfinite(vmax[j]):
                cap[i] = min(cap[i], (vmax[j] / abs(p1[i, j])) ** 2)
            if not _has_line(p1[i, j], p2[i, j], amax[j]) and p2[i, j] != 0 and i < N - 1:
                cap[i] = min(cap[i], amax[j] / abs(p2[i, j]))
    return cap


def profile(p1, p2, vmax, amax, moving):
    """x = sdot^2 at the N gridpoints: controllable sets backward, greedy forward.  Returns (x, xmax)."""
    N = p1.shape[0]
    c = 0.5 * (N - 1)
    cap = x_bounds(p1, p2, vmax, amax, moving)
    mv = np.nonzero(moving)[0]
    xmax = np.zeros(N)
    for i in range(N - 2, -1, -1):
        al, be = _lines(p1[i, mv], p2[i, mv], amax[mv])
        au = np.append(al, xmax[i + 1] * c)   # upper lines: the joints, then the link to K_{i+1}
        bu = np.append(be, -c)
        alo = np.append(-al, 0.0)             # lower lines
        db = np.append(be, -c)[None, :] - bu[:, None]
        with np.errstate(invalid="ignore", divide="ignore"):
            r = np.where(db > 0, (au[:, None] - alo[None, :]) / np.where(db > 0, db, 1.0), np.inf)
        xmax[i] = max(0.0, min(cap[i], r.min()))
    x = np.zeros(N)
    for i in range(N - 1):
        al, be = _lines(p1[i, mv], p2[i, mv], amax[mv])
        u = min(np.min(al + be * x[i], initial=np.inf), (xmax[i + 1] - x[i]) * c)
        x[i + 1] = min(max(x[i] + u / c, 0.0), xmax[i + 1])
    return x, xmax


def retime_one(plan, vmax, amax, subdiv=2, M=100):
    """dict(duration, t_grid, sd_grid, q, qd, qdd, status) of one plan (ndof, T)."""
    plan = np.asarray(plan, dtype=np.float64)
    ndof, T = plan.shape
    N = subdiv * (T - 1) + 1
    if not np.all(np.isfinite(plan)):
        nan = np.full((M, ndof), np.nan)
        return dict(duration=np.nan, t_grid=np.full(N, np.nan), sd_grid=np.full(N, np.nan), q=nan, qd=nan, qdd=nan,
                    status=GTO_STATUS_NUMERICAL)
    moving = np.any(plan != plan[:, :1], axis=1)
    sp, s, p1, p2 = path_derivatives(plan, subdiv)
    p1[:, ~moving] = 0.0
    p2[:, ~moving] = 0.0
    x = profile(p1, p2, np.asarray(vmax, float), np.asarray(amax, float), moving)[0] if moving.any() else np.zeros(N)
    sd = np.sqrt(x)
    t = np.zeros(N)
    if moving.any():
        t[1:] = np.cumsum((2.0 / (N - 1)) / (sd[:-1] + sd[1:]))
    dur = t[-1]
    if moving.any() and (not np.isfinite(dur) or np.maximum(x[:-1], x[1:]).min() <= STALL * x.max()):
        nan = np.full((M, ndof), np.nan)
        return dict(duration=dur, t_grid=t, sd_grid=sd, q=nan, qd=nan, qdd=nan, status=GTO_STATUS_NUMERICAL)
    ts = np.linspace(0.0, dur, M)
    i = np.clip(np.searchsorted(t, ts, side="right") - 1, 0, N - 2)
    u = (x[i + 1] - x[i]) * 0.5 * (N - 1)
    tau = ts - t[i]
    sdot = sd[i] + u * tau
    ss = np.clip(s[i] + tau * (sd[i] + 0.5 * u * tau), 0.0, 1.0)
    q1, q2 = sp(ss, 1), sp(ss, 2)
    q1[:, ~moving] = 0.0
    q2[:, ~moving] = 0.0
    return dict(duration=dur, t_grid=t, sd_grid=sd, q=sp(ss), qd=q1 * sdot[:, None],
                qdd=q1 * u[:, None] + q2 * (sdot ** 2)[:, None], status=0)


def retime(plans, vmax, amax, subdiv=2, M=100):
    """The batch: the arrays of gto_retime_batch."""
    rs = [retime_one(p, vmax, amax, subdiv, M) for p in np.asarray(plans, dtype=np.float64)]
    return {k: np.array([r[k] for r in rs]) for k in rs[0]}


def step_lp(p1, p2, vmax, amax, i, x_i, xmax_next):
    """The largest x_{i+1} reachable from x_i in one segment that stays inside [0, xmax_next], by scipy's HiGHS over u_i:
    what the greedy forward pass picks."""
    from scipy.optimize import linprog
    N = p1.shape[0]
    d2 = 2.0 / (N - 1)
    A = np.concatenate([p1[i], -p1[i]])[:, None]
    b = np.concatenate([amax - p2[i] * x_i, amax + p2[i] * x_i])
    res = linprog([-1.0], A_ub=A, b_ub=b, bounds=[(-x_i / d2, (xmax_next - x_i) / d2)], method="highs")
    assert res.status == 0, res.message
    return x_i + d2 * res.x[0]


def controllable_lp(p1, p2, vmax, amax, i):
    """The largest x_i from which the end can still be reached at rest, by one LP over the grid constraints of gridpoints
    i..N-1 (x_i free in [0, cap]): the controllable set K_i = [0, xmax_i] of the backward pass, found without it."""
    return grid_lp(p1[i:], p2[i:], vmax, amax, delta=1.0 / (p1.shape[0] - 1), free_start=True)[0]


def grid_lp(p1, p2, vmax, amax, delta=None, free_start=False):
    """max sum x (free_start: max x_0) over the grid constraints with scipy.optimize.linprog (HiGHS): variables
    x_0..x_{N-1}, u_0..u_{N-2}.  Returns the optimal x."""
    from scipy.optimize import linprog
    from scipy.sparse import lil_matrix
    N, nd = p1.shape
    if delta is None:
        delta = 1.0 / (N - 1)
    nv = N + N - 1
    d2 = 2.0 * delta
    A = lil_matrix((2 * nd * (N - 1), nv))
    bub = np.zeros(2 * nd * (N - 1))
    r = 0
    for i in range(N - 1):
        for j in range(nd):
            for sg in (1.0, -1.0):   # sg (p1 u + p2 x) <= amax
                A[r, N + i] = sg * p1[i, j]
                A[r, i] = sg * p2[i, j]
                bub[r] = amax[j]
                r += 1
    Aeq = lil_matrix((N - 1, nv))
    for i in range(N - 1):  # x_{i+1} - x_i - 2 Delta u_i = 0
        Aeq[i, i + 1], Aeq[i, i], Aeq[i, N + i] = 1.0, -1.0, -d2
    xcap = np.full(N, np.inf)
    for j in range(nd):
        with np.errstate(divide="ignore"):
            v = np.where((p1[:, j] != 0) & np.isfinite(vmax[j]), (vmax[j] / np.abs(p1[:, j])) ** 2, np.inf)
        xcap = np.minimum(xcap, v)
    fixed = (N - 1,) if free_start else (0, N - 1)
    bounds = [(0.0, 0.0) if i in fixed else (0.0, None if not np.isfinite(xcap[i]) else xcap[i]) for i in range(N)]
    bounds += [(None, None)] * (N - 1)
    cost = np.concatenate([-np.ones(N), np.zeros(N - 1)])
    if free_start:
        cost[1:N] = 0.0
    res = linprog(cost, A_ub=A.tocsr(), b_ub=bub, A_eq=Aeq.tocsr(), b_eq=np.zeros(N - 1), bounds=bounds, method="highs",
                  options=dict(primal_feasibility_tolerance=1e-10, dual_feasibility_tolerance=1e-10))
    assert res.status == 0, res.message
    return res.x[:N]
