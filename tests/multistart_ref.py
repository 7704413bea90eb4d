"""numpy restatement of what gto_seed_goalsets_multi_device and gto_select_plans_device add to the chain restated in
tests/grasp_chain_ref.py: the first k entries of np.lexsort((dist, cost)) written out, the slots of an instance, the class of
a slot's plan and the choice among an object's slots."""
import numpy as np

import grasp_chain_ref as ref

STATUS_NUMERICAL = 2  # GTO_STATUS_NUMERICAL
NAN = float("nan")

# slots that hit every class: status, cost, err_pos, err_rot, counts (three waypoints), class at pos_tol = 0.01,
# rot_tol_deg = 5, max_points = 5
CLASS_TABLE = [
    (0, 3.0, 0.005, 1.0, [0, 5, 0], 0),
    (1, 2.0, 0.02, 1.0, [0, 0, 0], 1),      # too far
    (0, 2.5, 0.005, 5.0, [0, 0, 0], 1),     # the tolerance itself is not within it
    (0, 1.0, 0.005, 1.0, [0, 6, 0], 2),     # one waypoint above max_points
    (0, 1.5, 0.001, 0.1, [0, -1, 0], 2),    # a waypoint that could not be checked is not free
    (0, 0.5, NAN, 1.0, [9, 0, 0], 3),       # NaN: not reached
    (2, 0.1, 0.0, 0.0, [0, 0, 0], 4),       # GTO_STATUS_NUMERICAL
    (0, NAN, 0.0, 0.0, [0, 0, 0], 4),
    (0, float("inf"), 0.0, 0.0, [0, 0, 0], 4),
    (0, 3.0, 0.005, 1.0, [0, 0, 0], 0),     # ties row 0 in class and cost
]


def class_table(rows):
    """(status, cost, err_pos, err_rot, counts (k, 3)) of the listed rows of CLASS_TABLE as slots, and their classes."""
    cols = list(zip(*[CLASS_TABLE[i] for i in rows]))
    return (np.array(cols[0], np.int32), np.array(cols[1]), np.array(cols[2]), np.array(cols[3]), np.array(cols[4], np.int32)), list(cols[5])


def choose_ranked(cost, dist, k):
    """np.lexsort((dist, cost))[:k] written out: rank after rank, the first by ref.before among the positions not chosen yet."""
    left, out = list(range(len(cost))), []
    while left and len(out) < k:
        best = left[0]
        for p in left[1:]:
            if ref.before(cost[p], dist[p], p, cost[best], dist[best], best):
                best = p
        out.append(best)
        left.remove(best)
    return out


def seed_slots(qc, goals, n_goals, q_solutions, accept, T, standoff_offset, param_index, interpolate, f32, score, k):
    """One instance of gto_seed_goalsets_multi_device with k slots, on ref.seed_goalsets (which yields the compaction, the
    candidates and their scores).  Returns its dict plus rows (the original row of every compacted position), seed_index
    (k,) and Q0 (k, ndof, T): slot r < n_accepted the r-th ranked candidate; a slot behind them -1 and slot 0's seed; without
    an accepted solution the constant seed in every slot."""
    r = ref.seed_goalsets(qc, goals, n_goals, q_solutions, accept, T, standoff_offset, param_index, interpolate, f32, score)
    n_max = np.asarray(goals).reshape(-1, 16).shape[0]
    r["rows"] = ref.accepted_rows(n_goals, n_max, accept)
    if r["n_accepted"] == 0:
        r["seed_index"], r["Q0"] = np.full(k, -1), np.tile(r["Q0"][None], (k, 1, 1))
        return r
    order = choose_ranked(r["seed_cost"], r["seed_dist"], k)
    assert order[0] == r["seed_index"]
    Q0 = [ref.seed_from(qc, r["plans"][p], interpolate, T, standoff_offset) for p in order]
    r["seed_index"] = np.array(order + [-1] * (k - len(order)))
    r["Q0"] = np.stack(Q0 + [Q0[0]] * (k - len(order)))
    return r


def slot_class(status, cost, err_pos, err_rot, counts, pos_tol, rot_tol_deg, max_points):
    """0 valid, free and reached; 1 valid and free; 2 valid and reached; 3 valid; 4 not valid.  counts (T,) or None."""
    if status == STATUS_NUMERICAL or not np.isfinite(cost):
        return 4
    free = counts is None or all(0 <= int(c) <= max_points for c in counts)
    reached = bool(err_pos < pos_tol and err_rot < rot_tol_deg)  # false on NaN
    return (0 if free else 2) + (0 if reached else 1)


def slot_before(c1, f1, s1, c2, f2, s2):
    """(class, cost, slot) of one slot in front of another's: class, then cost in numpy's order of keys, then slot."""
    if c1 != c2:
        return c1 < c2
    if ref.key_less(f1, f2):
        return True
    if ref.key_less(f2, f1):
        return False
    return s1 < s2


def select(status, cost, err_pos, err_rot, counts, pos_tol, rot_tol_deg, max_points):
    """One object: per-slot arrays (k,), counts (k, T) or None.  Returns (best slot, its class, every slot's class)."""
    k = len(cost)
    cls = [slot_class(status[s], cost[s], err_pos[s], err_rot[s], None if counts is None else counts[s], pos_tol, rot_tol_deg,
                      max_points) for s in range(k)]
    best = 0
    for s in range(1, k):
        if slot_before(cls[s], cost[s], s, cls[best], cost[best], best):
            best = s
    return best, cls[best], cls
