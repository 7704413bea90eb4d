"""A plain numpy restatement of one Levenberg-Marquardt step of the trajectory solve, for tests/test_step_solve_cpu.py and
tests/test_gpu_step_solve.py.  Imports without a GPU.

It shares no code with block_tridiag_solve of oracle/gto_oracle.c and none with the step kernels: from the blocks
Oracle.eval_normal_eq reports at an iterate it writes the whole damped system of the m = T - 2 free waypoints as ONE dense
(m n) x (m n) matrix and hands it to numpy.linalg.solve.

  undamped model   A = blockdiag(w_obstacle JtJ_obs[t] + goal block at T - 1 + standoff block at ts + velocity 2 alpha I
                   (alpha I at T - 1)) with - alpha I between neighbouring waypoints;  b = w_obstacle Jtr_obs[t] + goal
                   terms + alpha (q_t - q_{t-1}) - alpha (q_{t+1} - q_t);  alpha = w_vel / dt^2, dt = Tmax / (T - 1)
  active set       variable (t, i) is frozen when it sits on a bound and - b points outward
  damped system    the diagonal of A times (1 + lambda) (Marquardt scaling); the rows and columns of frozen variables
                   replaced by the identity (which also removes their coupling, from either side), their right-hand side 0
  step             x = M^-1 (- b), one step of iterative refinement with the residual formed in numpy.longdouble;
                   trial = clip(Q + x, lower, upper), s = trial - Q, predicted decrease - (2 b.s + s.A.s)

lm() wraps the step in the accept / reject rule of solve_instance (gain-ratio update of lambda, doubling on a reject), with the
objective taken from Oracle.eval_objective, so that iterates beyond the first can be restated too.
"""
import numpy as np

STATUS_CONVERGED, STATUS_MAX_ITER, STATUS_NUMERICAL = 0, 1, 2


def alpha_of(opts):
    dt = opts.Tmax / (opts.T - 1)
    return opts.w_vel / (dt * dt)


def pinned(desc, qc, Q0):
    """The seed as the solvers take it: waypoints 0 and 1 of the optimised joints at qc, the others clipped into the bounds."""
    Q = np.array(Q0, dtype=np.float64)
    oi = desc.opt_index
    Q[oi, :2] = np.asarray(qc)[oi][:, None]
    Q[oi, 2:] = np.clip(Q[oi, 2:], desc.lower[oi][:, None], desc.upper[oi][:, None])
    return Q


def system(o, prob, sid, Q, lam):
    """The dense system at iterate Q (ndof, T) under damping lam.  prob has desc, goals (n_goals, 16), n_goals, S (or
    None), base (3,); o is the Oracle (its opts are the options).  Returns a dict: A, b (undamped), M, rhs (damped, frozen
    rows the identity), act (m, n) bool, obs (T,) bool: waypoints with a non-zero obstacle block."""
    d, opts = prob.desc, o.opts
    T, n = int(opts.T), d.n_opt
    m, oi = T - 2, d.opt_index
    ts = T + int(opts.standoff_offset)
    alpha = alpha_of(opts)
    JtJ, Jtr, _, Hg, gg = o.eval_normal_eq(sid, prob.goals[None], prob.n_goals, prob.S, prob.base, Q[None])
    JtJ, Jtr, Hg, gg = JtJ[0], Jtr[0], Hg[0], gg[0]
    N = m * n
    A, b = np.zeros((N, N)), np.zeros(N)
    q = Q[oi]                                                   # (n, T)
    for s in range(m):
        t, sl = s + 2, slice(s * n, (s + 1) * n)
        A[sl, sl] = opts.w_obstacle * JtJ[t]
        b[sl] = opts.w_obstacle * Jtr[t]
        if t == T - 1:
            A[sl, sl] += Hg[0]
            b[sl] += gg[0]
        if prob.S is not None and t == ts:
            A[sl, sl] += Hg[1]
            b[sl] += gg[1]
        A[sl, sl] += alpha * np.eye(n)
        b[sl] += alpha * (q[:, t] - q[:, t - 1])
        if t < T - 1:
            A[sl, sl] += alpha * np.eye(n)
            b[sl] -= alpha * (q[:, t + 1] - q[:, t])
            nx = slice((s + 1) * n, (s + 2) * n)
            A[sl, nx] = A[nx, sl] = -alpha * np.eye(n)
    lo, hi = d.lower[oi], d.upper[oi]
    qf = q[:, 2:].T.reshape(-1)                                 # variable (s, i) at s n + i
    act = ((qf <= np.tile(lo, m)) & (b > 0.0)) | ((qf >= np.tile(hi, m)) & (b < 0.0))
    M = A.copy()
    M[np.diag_indices(N)] *= 1.0 + lam
    rhs = -b
    fz = np.flatnonzero(act)
    M[fz, :] = 0.0
    M[:, fz] = 0.0
    M[fz, fz] = 1.0
    rhs[fz] = 0.0
    obs = np.array([bool(np.any(JtJ[t] != 0.0)) for t in range(T)])
    return dict(A=A, b=b, M=M, rhs=rhs, act=act.reshape(m, n), obs=obs, alpha=alpha, m=m, n=n)


def solve_dense(M, rhs):
    x = np.linalg.solve(M, rhs)
    r = (rhs.astype(np.longdouble) - M.astype(np.longdouble) @ x.astype(np.longdouble)).astype(np.float64)
    return x + np.linalg.solve(M, r)


def step(prob, Q, sysd, M=None):
    """(trial (ndof, T), s (m n,), predicted decrease, largest |s|) of the system sysd at Q; M: another damped matrix in
    place of sysd's (the teeth of the CPU test)."""
    d = prob.desc
    oi, m, n = d.opt_index, sysd["m"], sysd["n"]
    x = solve_dense(sysd["M"] if M is None else M, sysd["rhs"])
    trial = Q.copy()
    v = np.clip(Q[oi, 2:] + x.reshape(m, n).T, d.lower[oi][:, None], d.upper[oi][:, None])
    trial[oi, 2:] = v
    s = (v - Q[oi, 2:]).T.reshape(-1)
    pred = -(2.0 * sysd["b"] @ s + s @ sysd["A"] @ s)
    return trial, s, float(pred), float(np.abs(s).max())


def lm(o, prob, sid, Q0, max_iter):
    """The solve of solve_instance with the step above.  Returns (Q, f, iterations, status, trace); trace[k] is the record of
    evaluation k >= 1: dict(Q: the iterate the step left from, lam, act, trial, s, pred, accepted)."""
    d, opts = prob.desc, o.opts
    f_of = lambda Qx: float(sum(x[0] for x in o.eval_objective(sid, prob.goals[None], prob.n_goals, prob.S, prob.base, Qx[None])[:3]))
    Q = pinned(d, prob.qc, Q0)
    f = f_of(Q)
    lam, nu, k, trace = float(opts.lambda0), 2.0, 0, []
    if not np.isfinite(f):
        return Q, f, 0, STATUS_NUMERICAL, trace
    while True:
        if k >= max_iter:
            return Q, f, k, STATUS_MAX_ITER, trace
        sysd = system(o, prob, sid, Q, lam)
        trial, s, pred, big = step(prob, Q, sysd)
        if big < opts.tol_step:
            return Q, f, k, STATUS_CONVERGED, trace
        rec = dict(Q=Q, lam=lam, act=sysd["act"], obs=sysd["obs"], trial=trial, s=s, pred=pred)
        trace.append(rec)
        k += 1
        f_try = f_of(trial)
        rec["accepted"] = bool(f_try < f and pred > 0.0)
        if rec["accepted"]:
            df, rho = f - f_try, (f - f_try) / pred
            Q, f = trial, f_try
            lam = max(lam * max(1.0 - (2.0 * rho - 1.0) ** 3, 1.0 / 3.0), 1e-12)
            nu = 2.0
            if df <= opts.tol_rel_f * (1.0 + f):
                return Q, f, k, STATUS_CONVERGED, trace
        else:
            lam *= nu
            nu *= 2.0
            if lam > 1e15:
                return Q, f, k, STATUS_CONVERGED, trace
