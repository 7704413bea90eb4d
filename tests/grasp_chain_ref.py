"""numpy restatement of the steps between IK and the trajectory solve that gto_ik_report_device and
gto_seed_goalsets_device run on the GPU: the report of an IK solution (gto/ik_solver.py:88-97), the driver's acceptance
test and order-preserving selection (examples/pybullet_gto_planning.py:262-269), the seed candidates
(gto/gto_planner.py:197-206), the choice np.lexsort((dist, cost))[0] written out, and the q_solutions=None branch."""
import numpy as np


def report(T_ee, RT, cost, pos_tol, rot_tol_deg, cost_tol):
    """err_pos, err_rot (degrees), accept for frames T_ee (B, 4, 4) against goals RT (B, 4, 4) and costs (B,)."""
    T_ee, RT = np.asarray(T_ee, dtype=np.float64), np.asarray(RT, dtype=np.float64)
    err_pos = np.linalg.norm(RT[:, :3, 3] - T_ee[:, :3, 3], axis=1)
    cosang = (np.einsum("bij,bij->b", RT[:, :3, :3], T_ee[:, :3, :3]) - 1.0) / 2.0
    err_rot = np.degrees(np.arccos(np.clip(cosang, -1.0, 1.0)))
    with np.errstate(invalid="ignore"):
        accept = (err_pos < pos_tol) & (err_rot < rot_tol_deg) & (np.asarray(cost) < cost_tol)  # NaN compares false
    return err_pos, err_rot, accept


def clamp_count(n, n_max):
    return int(min(max(int(n), 1), n_max))


def accepted_rows(n_goals, n_max, accept):
    """Rows of the accepted solutions among the first n_goals (clamped to [1, n_max]), in their order."""
    nb = clamp_count(n_goals, n_max)
    if accept is None:
        return np.arange(nb)
    return np.flatnonzero(np.asarray(accept[:nb]).astype(bool))


def candidates(qc, q_solutions, T, param_index, f32=False):
    """(n, ndof, T): clamped cubic from qc to every solution at s = (t + 1) / (T + 1), parameter rows qc's."""
    qc = np.asarray(qc, dtype=np.float64)
    qs = np.asarray(q_solutions, dtype=np.float64).reshape(-1, qc.shape[0])
    if f32:
        with np.errstate(over="ignore", invalid="ignore"):
            qs = qs.astype(np.float32).astype(np.float64)
    out = np.empty((qs.shape[0], qc.shape[0], T))
    for t in range(T):
        s = float(t + 1) / float(T + 1)
        h = s * s * (3.0 - 2.0 * s)
        out[:, :, t] = qc[None, :] + (qs - qc[None, :]) * h
    out[:, np.asarray(param_index, dtype=np.int64), :] = qc[np.asarray(param_index, dtype=np.int64)][None, :, None]
    return out


def key_less(a, b):
    """numpy's order of floating-point sort keys: a NaN after every number, NaNs equal among themselves."""
    return bool(a < b or (b != b and a == a))


def before(c1, d1, p1, c2, d2, p2):
    if key_less(c1, c2):
        return True
    if key_less(c2, c1):
        return False
    if key_less(d1, d2):
        return True
    if key_less(d2, d1):
        return False
    return p1 < p2


def choose(cost, dist):
    """np.lexsort((dist, cost))[0] written out: lowest cost, then lowest distance, then lowest position."""
    best = 0
    for p in range(1, len(cost)):
        if before(cost[p], dist[p], p, cost[best], dist[best], best):
            best = p
    return best


def distance(plans):
    d = plans[:, :, 0] - plans[:, :, -1]
    out = np.zeros(plans.shape[0])
    for j in range(plans.shape[1]):  # joint order, squares and sums apart
        out = out + d[:, j] * d[:, j]
    return np.sqrt(out)


def seed_from(qc, cand, interpolate, T, standoff_offset):
    if interpolate:
        return cand.copy()
    Q0 = np.tile(np.asarray(qc, dtype=np.float64)[:, None], (1, T))
    Q0[:, T + standoff_offset:] = cand[:, T - 1:T]
    return Q0


def seed_goalsets(qc, goals, n_goals, q_solutions, accept, T, standoff_offset, param_index, interpolate, f32, score):
    """One instance.  goals (n_max, 16), q_solutions (n_max, ndof), accept (n_max,) or None; score(plans (n, ndof, T)) ->
    cost (n,) (the obstacle cost of every candidate).  Returns a dict of goals_out (count, 16), n_goals_out, n_accepted,
    Q0 (ndof, T), seed_index, seed_cost, seed_dist (n_accepted,), plans."""
    goals = np.asarray(goals, dtype=np.float64).reshape(-1, 16)
    n_max = goals.shape[0]
    rows = accepted_rows(n_goals, n_max, accept)
    qc = np.asarray(qc, dtype=np.float64)
    if len(rows) == 0:
        nb = clamp_count(n_goals, n_max)
        return dict(goals_out=goals[:nb].copy(), n_goals_out=nb, n_accepted=0, Q0=np.tile(qc[:, None], (1, T)), seed_index=-1,
                    seed_cost=np.empty(0), seed_dist=np.empty(0), plans=np.empty((0, qc.shape[0], T)))
    plans = candidates(qc, np.asarray(q_solutions)[rows], T, param_index, f32)
    cost, dist = np.asarray(score(plans), dtype=np.float64), distance(plans)
    k = choose(cost, dist)
    return dict(goals_out=goals[rows].copy(), n_goals_out=len(rows), n_accepted=len(rows),
                Q0=seed_from(qc, plans[k], interpolate, T, standoff_offset), seed_index=k, seed_cost=cost, seed_dist=dist, plans=plans)
