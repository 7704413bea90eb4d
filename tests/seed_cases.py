"""Goal sets wider than one wave for gto_seed_goalsets_device: plain numpy, no GPU.  k_seed_score and k_seed_select walk a
goal set 64 rows at a time; the twelve instances below put the accepted rows, the ties, the NaNs and the cheapest row where
the arithmetic that crosses a chunk (rows seen so far, row of the j-th accepted solution, a lane's best of several rows, the
fold over all 64 lanes) decides the result."""
import numpy as np

WIDE_B = 12


def wide_rows(n_max):
    """The rows the instance list names, and the nearest valid form of those that need a row a small set does not have:
      first    instance 2: rows before it rejected, every row from it on accepted: 64, or n_max // 2 if there is no row 64
      full     instance 3: rows 0 .. full-1 accepted, none behind: 64, or n_max if the set is no longer than a chunk
      pair     instance 5: the only accepted rows: (63, 64), or the last two rows if there is no row 64
      ties3    instances 6, 7: (3, 67, n_max - 1), with n_max // 2 for 67 if row 67 is not in front of the last row
      ties2    instances 6, 7: (64, 65), or (n_max - 3, n_max - 2) if row 65 is not in front of the last row
      far      instance 8: where the cheapest row goes: n_max - 2 if that is a row >= 128, else the last but one row of the
               last chunk (the last row if the chunk has one row)
      nans     instance 9: (1, 70), or (1, n_max - 1) if there is no row 70
      cut      instance 10: n_goals: 70, or n_max - 3 if that still cuts the second chunk (n_max >= 67), else n_max // 2
      lo11     instance 11: lower end of the random n_goals: 65, or n_max // 2 if there is no row 64"""
    assert n_max >= 8
    return dict(first=64 if n_max > 64 else n_max // 2,
                full=min(64, n_max),
                pair=(63, 64) if n_max > 64 else (n_max - 2, n_max - 1),
                ties3=(3, 67 if n_max > 68 else n_max // 2, n_max - 1),
                ties2=(64, 65) if n_max > 66 else (n_max - 3, n_max - 2),
                far=max(64 * ((n_max - 1) // 64), n_max - 2),
                nans=(1, 70 if n_max > 70 else n_max - 1),
                cut=70 if n_max >= 72 else (n_max - 3 if n_max >= 67 else n_max // 2),
                lo11=65 if n_max > 64 else n_max // 2)


def distance_to_qc(b, qc, qs):
    """The stand-in for `lowest` where no oracle is at hand: the row nearest to qc."""
    return int(np.argmin(np.linalg.norm(np.nan_to_num(qs - qc[None, :], nan=1e9), axis=1)))


def seed_case_wide(desc, qc0, rng, n_max, lowest=distance_to_qc, instances=None):
    """qc, qs, goals, n_goals, accept, sid, base of WIDE_B = 12 instances (or of the listed ones, in that order).
    lowest(b, qc (ndof,), qs (n, ndof)) -> the row among qs that the scorer (the FP64 oracle in the GPU tests) puts first;
    it is asked for instances 7 (every row) and 8 (the accepted rows).  Every joint of a solution is random within the limits
    (cut to +-2.5), the parameter joints too: a candidate keeps qc's value there whatever the solution says.

      0  every row accepted, n_goals = n_max
      1  nothing accepted
      2  rows 0 .. first-1 rejected, every row from `first` on accepted
      3  exactly rows 0 .. full-1 accepted, n_goals = n_max
      4  only row n_max - 1 accepted
      5  only the rows `pair` accepted
      6  every row accepted; the rows `ties3` hold one solution and the rows `ties2` another: bit-equal ties across chunks
         and across lanes
      7  as 6, and the solution in `ties3` is a copy of the row that `lowest` names: the lowest position wins
      8  a random mask (0.8) in which the accepted row that `lowest` names changes places with row `far`
      9  every row accepted, a NaN solution in each of the rows `nans`
     10  n_goals = cut, in the middle of a chunk, with accepted rows behind it that do not count
     11  a random mask (0.5), n_goals random in [lo11, n_max]"""
    B, R = WIDE_B, wide_rows(n_max)
    oi = np.asarray(desc.opt_index)
    qc = np.tile(np.asarray(qc0, dtype=np.float64), (B, 1))
    qc[:, oi] += rng.uniform(-0.05, 0.05, (B, len(oi)))
    qs = rng.uniform(np.maximum(desc.lower, -2.5), np.minimum(desc.upper, 2.5), (B, n_max, desc.ndof))
    goals = rng.standard_normal((B, n_max, 16))
    n_goals = np.full(B, n_max, np.int32)
    accept = np.ones((B, n_max), np.uint8)
    sid = (np.arange(B) % 2).astype(np.int32)
    base = rng.uniform(-0.03, 0.03, (B, 3))
    accept[1] = 0
    n_goals[1] = rng.integers(1, n_max + 1)
    accept[2, :R["first"]] = 0
    accept[3, R["full"]:] = 0
    accept[4, :n_max - 1] = 0
    accept[5] = 0
    accept[5, list(R["pair"])] = 1
    for b in (6, 7):
        qs[b, R["ties3"][1]] = qs[b, R["ties3"][2]] = qs[b, R["ties3"][0]]
        qs[b, R["ties2"][1]] = qs[b, R["ties2"][0]]
    qs[7, list(R["ties3"])] = qs[7, lowest(7, qc[7], qs[7])]
    accept[8] = rng.random(n_max) < 0.8
    accept[8, R["far"]] = 1
    rows8 = np.flatnonzero(accept[8])
    low8 = int(rows8[lowest(8, qc[8], qs[8, rows8])])
    qs[8, [low8, R["far"]]] = qs[8, [R["far"], low8]]
    qs[9, list(R["nans"]), oi[min(2, len(oi) - 1)]] = np.nan
    accept[10] = rng.random(n_max) < 0.7
    accept[10, R["cut"] - 1:R["cut"] + 2] = 1
    n_goals[10] = R["cut"]
    accept[11] = rng.random(n_max) < 0.5
    n_goals[11] = rng.integers(R["lo11"], n_max + 1)
    out = (qc, qs, goals, n_goals, accept, sid, base)
    return out if instances is None else tuple(x[list(instances)].copy() for x in out)
