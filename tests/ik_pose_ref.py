"""CPU restatement (numpy) of the orientation-goal IK of gto_solve_ik_pose_batch: the pose terms of
gto/ik_solver_quaternion.py:50-55 and gto/ik_solver_rpy.py:53-58 in Gauss-Newton form, and the projected
Levenberg-Marquardt rules of k_ik_solve (those of the oracle's solve_ik_instance: seed clip, accept / reject, lambda
and nu update, active set, iteration cap).  Kinematics come from the oracle's eval_fk; everything else is here.

Convention of the kernel: f = sum r^2, b = J^T r (half the gradient), A = J^T J.
"""
import numpy as np

GTO_IK_GOAL_POINTS, GTO_IK_GOAL_QUATERNION, GTO_IK_GOAL_RPY = 0, 1, 2
GTO_STATUS_CONVERGED, GTO_STATUS_MAX_ITER, GTO_STATUS_NUMERICAL = 0, 1, 2
REVOLUTE, PRISMATIC = 1, 2
PAIRS = [(0, 1), (0, 2), (0, 3), (1, 2), (1, 3), (2, 3)]


def quat_of(R):
    """Unit quaternion (x, y, z, w) of a rotation matrix, Shepperd's branches (the kernel's)."""
    R00, R01, R02 = R[0]
    R10, R11, R12 = R[1]
    R20, R21, R22 = R[2]
    tr = R00 + R11 + R22
    if tr >= R00 and tr >= R11 and tr >= R22:
        w = 0.5 * np.sqrt(1.0 + tr)
        s = 0.25 / w
        return np.array([(R21 - R12) * s, (R02 - R20) * s, (R10 - R01) * s, w])
    if R00 >= R11 and R00 >= R22:
        x = 0.5 * np.sqrt(1.0 + R00 - R11 - R22)
        s = 0.25 / x
        return np.array([x, (R01 + R10) * s, (R02 + R20) * s, (R21 - R12) * s])
    if R11 >= R22:
        y = 0.5 * np.sqrt(1.0 - R00 + R11 - R22)
        s = 0.25 / y
        return np.array([(R01 + R10) * s, y, (R12 + R21) * s, (R02 - R20) * s])
    z = 0.5 * np.sqrt(1.0 - R00 - R11 + R22)
    s = 0.25 / z
    return np.array([(R02 + R20) * s, (R12 + R21) * s, z, (R10 - R01) * s])


def shepperd_branch(R):
    """The pivot quat_of takes: 0 for w, 1, 2, 3 for x, y, z."""
    tr = R[0, 0] + R[1, 1] + R[2, 2]
    if tr >= R[0, 0] and tr >= R[1, 1] and tr >= R[2, 2]:
        return 0
    if R[0, 0] >= R[1, 1] and R[0, 0] >= R[2, 2]:
        return 1
    return 2 if R[1, 1] >= R[2, 2] else 3


def shepperd_margin(R):
    """How far the pivot's quantity (the largest of tr, R00, R11, R22) lies above the runner-up."""
    v = np.sort([R[0, 0] + R[1, 1] + R[2, 2], R[0, 0], R[1, 1], R[2, 2]])
    return float(v[3] - v[2])


def small_rotations(eta):
    """The six rotations by +-eta about the world axes."""
    out = []
    for a in range(3):
        for s in (eta, -eta):
            K = np.zeros((3, 3))
            i, j = (a + 1) % 3, (a + 2) % 3
            K[j, i], K[i, j] = 1.0, -1.0
            out.append(np.eye(3) + np.sin(s) * K + (1.0 - np.cos(s)) * K @ K)  # Rodrigues
    return out


def rpy_of(R):
    """optas Quaternion.getrpy in matrix entries: pitch +pi/2 whenever |R20| >= 1 (-1 included)."""
    pitch = np.pi / 2.0 if abs(R[2, 0]) >= 1.0 else np.arcsin(-R[2, 0])
    return np.array([np.arctan2(R[2, 1], R[2, 2]), pitch, np.arctan2(R[1, 0], R[0, 0])])


def residual(kind, T, g):
    """(residual r, constant c) with pose term f = c + |r|^2."""
    p, R = T[:3, 3], T[:3, :3]
    rt = p - g[:3]
    if kind == GTO_IK_GOAL_QUATERNION:
        q, gq = quat_of(R), np.asarray(g[3:7], dtype=np.float64)
        rq = np.array([q[i] * gq[k] - q[k] * gq[i] for i, k in PAIRS])
        return np.concatenate([rt, rq]), 1.0 - float(gq @ gq)
    if kind == GTO_IK_GOAL_RPY:
        return np.concatenate([rt, (rpy_of(R) - g[3:6]) / np.pi]), 0.0
    raise ValueError(kind)


def pose_term(kind, T, g):
    """The pose term's value, summed in the kernel's order."""
    r, c = residual(kind, T, g)
    f = r[0] * r[0] + r[1] * r[1] + r[2] * r[2]
    rest = 0.0
    for v in r[3:]:
        rest += v * v
    return f + (c + rest) if kind == GTO_IK_GOAL_QUATERNION else f + rest


def reference_pose_term(kind, T, g):
    """The reference's own formula on the true quaternion / angles: 1 - (quat . g)^2 resp. |(rpy - g) / pi|^2."""
    p = T[:3, 3]
    ft = float(np.sum((p - g[:3]) ** 2))
    if kind == GTO_IK_GOAL_QUATERNION:
        return ft + 1.0 - float(quat_of(T[:3, :3]) @ g[3:7]) ** 2
    return ft + float(np.sum(((rpy_of(T[:3, :3]) - g[3:6]) / np.pi) ** 2))


def screws(desc, frames, fe):
    """World screws (w; v) of the optimised joints that move frame fe, (n, 6); zero rows for the others."""
    n = len(desc.opt_index)
    S = np.zeros((n, 6))
    chain, i = set(), fe
    while i >= 0:
        chain.add(i)
        i = int(desc.parent[i])
    for j, dof in enumerate(desc.opt_index):
        fr = [i for i in range(desc.n_frames) if desc.q_index[i] == dof and desc.joint_type[i] != 0]
        if not fr or fr[0] not in chain:
            continue
        i = fr[0]
        F = frames[i]
        u = desc.axis[i] / np.linalg.norm(desc.axis[i])
        a = F[:3, :3] @ u
        if desc.joint_type[i] == PRISMATIC:
            S[j, 3:] = a
        else:
            S[j, :3] = a
            S[j, 3:] = np.cross(F[:3, 3], a)
    return S


def jacobian(kind, T, g, S):
    """Rows of the residual's Jacobian, (m, n), from the screws."""
    p, R = T[:3, 3], T[:3, :3]
    n = S.shape[0]
    m = 9 if kind == GTO_IK_GOAL_QUATERNION else 6
    J = np.zeros((m, n))
    q = quat_of(R)
    gq = np.asarray(g[3:7], dtype=np.float64) if kind == GTO_IK_GOAL_QUATERNION else None
    for j in range(n):
        w, v = S[j, :3], S[j, 3:]
        J[:3, j] = np.cross(w, p) + v
        if kind == GTO_IK_GOAL_QUATERNION:
            dq = np.concatenate([0.5 * (q[3] * w + np.cross(w, q[:3])), [-0.5 * float(w @ q[:3])]])
            J[3:, j] = [dq[i] * gq[k] - dq[k] * gq[i] for i, k in PAIRS]
        else:
            dR = np.cross(w[:, None], R, axis=0)  # [w]x R
            dr = R[2, 1] ** 2 + R[2, 2] ** 2
            dy = R[1, 0] ** 2 + R[0, 0] ** 2
            J[3, j] = (R[2, 2] * dR[2, 1] - R[2, 1] * dR[2, 2]) / dr / np.pi if dr > 0 else 0.0
            J[4, j] = 0.0 if abs(R[2, 0]) >= 1.0 else -dR[2, 0] / np.sqrt(1.0 - R[2, 0] ** 2) / np.pi
            J[5, j] = (R[0, 0] * dR[1, 0] - R[1, 0] * dR[0, 0]) / dy / np.pi if dy > 0 else 0.0
    return J


class PoseProblem:
    """f(x), b(x), A(x) of one instance (no collision term) as functions of the optimised joints."""

    def __init__(self, oracle_obj, desc, link_ee, kind, q_full, g, rot=None):
        self.o, self.d, self.kind, self.rot = oracle_obj, desc, kind, rot  # rot: a 3x3 turned onto link_ee's rotation
        self.fe = desc.frame_index(link_ee)
        self.q_full = np.array(q_full, dtype=np.float64)
        self.g = np.asarray(g, dtype=np.float64)
        self.oi = desc.opt_index

    def full(self, x):
        q = self.q_full.copy()
        q[self.oi] = x
        return q

    def frames(self, X):
        Q = np.repeat(self.q_full[None], len(X), 0)
        Q[:, self.oi] = X
        fr = self.o.eval_fk(Q)
        if self.rot is not None:
            fr[:, self.fe, :3, :3] = self.rot @ fr[:, self.fe, :3, :3]
        return fr

    def f(self, X):
        fr = self.frames(np.atleast_2d(X))
        return np.array([pose_term(self.kind, F[self.fe], self.g) for F in fr])

    def eval(self, x):
        fr = self.frames(np.atleast_2d(x))[0]
        T = fr[self.fe]
        r, _ = residual(self.kind, T, self.g)
        J = jacobian(self.kind, T, self.g, screws(self.d, fr, self.fe))
        return pose_term(self.kind, T, self.g), J.T @ r, J.T @ J


def solve(prob, q0_full, opts, max_iter):
    """k_ik_solve's projected Levenberg-Marquardt loop on prob -> (q_full, f, iters, status)."""
    d = prob.d
    lo, hi = d.lower[prob.oi], d.upper[prob.oi]
    n = len(prob.oi)
    xt = np.clip(np.asarray(q0_full, dtype=np.float64)[prob.oi], lo, hi)
    x = xt.copy()
    lam, nu, f, pred = float(opts.lambda0), 2.0, np.inf, 0.0
    first, status, k = True, GTO_STATUS_MAX_ITER, 0
    A = b = None
    while True:
        f_try, b_try, A_try = prob.eval(xt)
        done = False
        if first:
            first = False
            f, x, A, b = f_try, xt.copy(), A_try, b_try
            if not np.isfinite(f):
                status = GTO_STATUS_NUMERICAL
                break
        elif f_try < f and pred > 0.0:
            df = f - f_try
            rho = df / pred
            f, x, A, b = f_try, xt.copy(), A_try, b_try
            sg = 2.0 * rho - 1.0
            lam = max(lam * max(1.0 - sg * sg * sg, 1.0 / 3.0), 1e-12)
            nu = 2.0
            if df <= opts.tol_rel_f * (1.0 + f):
                status, done = GTO_STATUS_CONVERGED, True
        else:
            lam *= nu
            nu *= 2.0
            if lam > 1e15:
                status, done = GTO_STATUS_CONVERGED, True
        if done:
            break
        if k >= max_iter:
            status = GTO_STATUS_MAX_ITER
            break
        act = (x <= lo) & (b > 0.0) | (x >= hi) & (b < 0.0)
        S = A * (1.0 + lam * np.eye(n))
        S[np.diag(A) == 0.0, np.diag(A) == 0.0] = lam  # a joint no residual depends on: lambda itself damps it
        S[act, :] = 0.0
        S[:, act] = 0.0
        S[act, act] = 1.0
        try:
            np.linalg.cholesky(S)
        except np.linalg.LinAlgError:
            status = GTO_STATUS_NUMERICAL
            break
        dx = np.linalg.solve(S, np.where(act, 0.0, -b))
        xt = np.clip(x + dx, lo, hi)
        s = xt - x
        pred = -(s @ A @ s + 2.0 * b @ s)
        if np.abs(s).max() < opts.tol_step:
            status = GTO_STATUS_CONVERGED
            break
        k += 1
    return prob.full(x), f, k, status
