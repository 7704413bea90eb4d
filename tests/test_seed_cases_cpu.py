"""CPU: the wide goal-set generator of the GPU seed tests (tests/seed_cases.py) builds the masks its instance list promises,
read back through grasp_chain_ref.accepted_rows, at every size tests/test_gpu_seed_waves.py runs; and the written-out choice
(grasp_chain_ref.choose) is np.lexsort((dist, cost))[0] on the generator's tie and NaN patterns."""
import numpy as np
import pytest

import grasp_chain_ref as ref
from grasptrajopt_amd.robot_desc import load_builtin
from seed_cases import WIDE_B, seed_case_wide, wide_rows

SIZES = [63, 64, 65, 70, 128, 130, 200]


def rows_of(case, b, n_max):
    return ref.accepted_rows(case[3][b], n_max, case[4][b])


@pytest.mark.parametrize("n_max", SIZES)
def test_masks_have_the_listed_properties(n_max):
    desc = load_builtin("panda")
    qc0 = np.linspace(-0.4, 0.4, desc.ndof)
    calls = []

    def lowest(b, qc, qs):
        calls.append((b, len(qs)))
        return int(np.argmin(np.abs(qs[:, desc.opt_index[0]])))
    case = seed_case_wide(desc, qc0, np.random.default_rng(n_max), n_max, lowest)
    qc, qs, goals, n_goals, accept, sid, base = case
    assert qc.shape == (WIDE_B, desc.ndof) and qs.shape == (WIDE_B, n_max, desc.ndof) and goals.shape == (WIDE_B, n_max, 16)
    assert accept.dtype == np.uint8 and n_goals.dtype == np.int32 and sid.tolist() == [b % 2 for b in range(WIDE_B)]
    assert np.abs(base).max() <= 0.03 and ((n_goals >= 1) & (n_goals <= n_max)).all()
    wide = n_max > 64           # there is a row 64
    all_rows = list(range(n_max))
    assert rows_of(case, 0, n_max).tolist() == all_rows
    assert rows_of(case, 1, n_max).tolist() == []
    r2 = rows_of(case, 2, n_max)
    assert r2.tolist() == list(range(64 if wide else n_max // 2, n_max)) and len(r2) > 0
    assert rows_of(case, 3, n_max).tolist() == list(range(min(64, n_max))) and n_goals[3] == n_max
    assert rows_of(case, 4, n_max).tolist() == [n_max - 1]
    assert rows_of(case, 5, n_max).tolist() == ([63, 64] if wide else [n_max - 2, n_max - 1])
    R = wide_rows(n_max)
    if n_max > 68:
        assert R["ties3"] == (3, 67, n_max - 1) and R["ties2"] == (64, 65)
    for b in (6, 7):
        assert rows_of(case, b, n_max).tolist() == all_rows
        t3, t2 = list(R["ties3"]), list(R["ties2"])
        assert len(set(t3 + t2)) == 5 and max(t3 + t2) < n_max
        assert (qs[b, t3] == qs[b, t3[0]]).all() and (qs[b, t2] == qs[b, t2[0]]).all()
        assert t3[0] // 64 != t3[2] // 64 or not wide          # a tie across chunks ...
        assert t2[0] % 64 != t2[1] % 64                          # ... and one across lanes
        other = np.delete(qs[b], t3 + t2, axis=0)
        # no further duplicate, but the row that 7 copied
        assert n_max - 3 - (b == 7) <= len(np.unique(np.concatenate([other, qs[b, [t3[0], t2[0]]]]), axis=0)) <= n_max - 3
    # 7: the tied solution is the one the scorer puts first
    assert lowest(7, qc[7], qs[7]) == 3
    # 8: the accepted row the scorer puts first sits at `far`
    r8 = rows_of(case, 8, n_max)
    far = int(r8[lowest(8, qc[8], qs[8, r8])])
    assert far == R["far"] and (far >= 128 if n_max > 128 else far // 64 == (n_max - 1) // 64)
    assert 0 < len(r8) < n_max or accept[8].all()
    assert calls[:2] == [(7, n_max), (8, len(r8))]
    # 9
    assert rows_of(case, 9, n_max).tolist() == all_rows
    nan_rows = np.flatnonzero(np.isnan(qs[9]).any(axis=1)).tolist()
    assert nan_rows == ([1, 70] if n_max > 70 else [1, n_max - 1])
    assert not np.isnan(np.delete(qs, 9, axis=0)).any() and not np.isnan(qc).any()
    # 10: the cut falls inside a chunk, accepted rows stand on both sides of it
    cut = int(n_goals[10])
    assert cut == (70 if n_max >= 72 else R["cut"]) and cut % 64 != 0 and cut < n_max
    assert (cut > 64) == (n_max >= 67)
    r10 = rows_of(case, 10, n_max)
    assert r10.max() == cut - 1 and accept[10, cut:].sum() >= 2 and np.array_equal(r10, np.flatnonzero(accept[10, :cut]))
    # 11
    assert (65 if wide else n_max // 2) <= n_goals[11] <= n_max
    r11 = rows_of(case, 11, n_max)
    assert 0.25 * n_goals[11] < len(r11) < 0.75 * n_goals[11]
    # a subset keeps the instances as they are
    sub = seed_case_wide(desc, qc0, np.random.default_rng(n_max), n_max, lowest, instances=(0, 1, 2, 6, 9, 10))
    for a, c in zip(sub, case):
        assert a.tobytes() == c[[0, 1, 2, 6, 9, 10]].tobytes()


@pytest.mark.parametrize("n_max", SIZES)
def test_choice_is_first_of_lexsort_on_the_tie_and_nan_patterns(n_max):
    """A synthetic score on the generator's solutions: a function of the solution alone (so duplicated rows tie in cost and
    distance), coarse (so other rows tie in cost alone), NaN where the solution is."""
    desc = load_builtin("panda")
    oi = desc.opt_index
    case = seed_case_wide(desc, np.zeros(desc.ndof), np.random.default_rng(5), n_max)
    qc, qs, goals, n_goals, accept, sid, base = case
    R = wide_rows(n_max)
    for b in range(WIDE_B):
        rows = rows_of(case, b, n_max)
        if len(rows) == 0:
            continue
        x = qs[b, rows]
        for cost, dist in ((np.round(np.abs(x[:, oi[0]]) * 4.0), np.round(np.abs(x[:, oi[1]]) * 8.0)),      # many ties
                           (np.abs(x[:, oi[2]]), np.abs(x[:, oi[1]])),                                       # NaN costs in 9
                           (np.zeros(len(rows)), np.abs(x[:, oi[2]])),                                       # NaN distances
                           (np.zeros(len(rows)), np.zeros(len(rows)))):                                      # all tied
            assert ref.choose(cost, dist) == int(np.lexsort((dist, cost))[0]), (b, n_max)
    # the patterns are there: the ties of 6 share a key, the NaNs of 9 sort behind every number and tie among themselves
    x = qs[6]
    cost, dist = np.abs(x[:, oi[2]]), np.abs(x[:, oi[1]])
    cost[list(R["ties3"])] = -1.0   # the tied solution the cheapest: the lowest of its positions
    assert ref.choose(cost, dist) == 3 == int(np.lexsort((dist, cost))[0])
    cost = np.abs(qs[9][:, oi[2]])
    assert np.isnan(cost[list(R["nans"])]).all() and ref.choose(cost, cost) not in R["nans"]
    only = np.full(n_max, np.nan)
    assert ref.choose(only, only) == 0 == int(np.lexsort((only, only))[0])
    order = np.lexsort((cost, cost))
    assert order[-2:].tolist() == list(R["nans"])
