"""CPU: the rule by which a solve call runs its init pass once per run of equal start states (k_init_heads, gto_kernels.h),
restated in numpy.

What the init pass of instance b reads is its key: scene_id[b], base_pos[b] and the joint value of every frame at the two
pinned waypoints (rows 0 and 1 of the solver's qf table: an optimised joint's value is qc's at both, any other actuated
joint's is the seed's own, a fixed frame's is 0).  b is a head when it is the first of its block of BLOCK instances or its key
differs from that of b - 1 IN ANY BIT (so -0.0 and +0.0 differ and a NaN equals only its own bits), and rep[b] is the nearest
head at or before b in its block.  Only the heads run the init pass; the others take their representative's four numbers.
The rule may miss duplicates (keys that are equal but not neighbours, or sit in two blocks); it may never merge two keys
that differ.  tests/test_gpu_init_dedup.py builds its cases with these functions and checks the kernel through the results."""
import numpy as np

BLOCK = 64  # GTO_HEAD_BLOCK: one wavefront, one ballot


def start_rows(desc, qc, Q0):
    """[B][2][F]: rows 0 and 1 of qf as k_lm_init writes them for a solve call."""
    qc, Q0 = np.asarray(qc, dtype=np.float64), np.asarray(Q0, dtype=np.float64)
    B, F = len(qc), desc.n_frames
    opt = set(int(j) for j in desc.opt_index)
    rows = np.zeros((B, 2, F))
    for i in range(F):
        dq = int(desc.q_index[i])
        if dq < 0:
            continue
        rows[:, :, i] = qc[:, dq, None] if dq in opt else Q0[:, dq, :2]
    return rows


def keys(scene_id, base_pos, rows):
    """[B][1 + 3 + 2 F] unsigned 64-bit words: the bits the init pass reads."""
    B = len(rows)
    sid = np.broadcast_to(np.asarray(scene_id, dtype=np.int32), (B,)).astype(np.uint32).astype(np.uint64)
    base = np.ascontiguousarray(np.broadcast_to(np.asarray(base_pos, dtype=np.float64), (B, 3)))
    return np.concatenate([sid[:, None], base.view(np.uint64), np.ascontiguousarray(rows, dtype=np.float64).reshape(B, -1).view(np.uint64)], axis=1)


def init_heads(key, block=BLOCK):
    """rep[b] for the keys [B][words]."""
    B = len(key)
    head = np.ones(B, dtype=bool)
    head[1:] = (key[1:] != key[:-1]).any(axis=1)
    head[::block] = True
    return np.maximum.accumulate(np.where(head, np.arange(B), 0)).astype(np.int32)


def _rows(B, F=3, value=0.25):
    return np.full((B, 2, F), value)


def test_equal_keys_share_the_first_of_each_block():
    for B in (1, 2, 63, 64, 65, 130):
        rep = init_heads(keys(0, (0.0, 0.0, 0.0), _rows(B)))
        np.testing.assert_array_equal(rep, (np.arange(B) // BLOCK) * BLOCK)


def test_equal_keys_that_are_not_neighbours_are_computed_again():
    rows = _rows(3)
    rows[1, 0, 1] = 0.5
    np.testing.assert_array_equal(init_heads(keys(0, (0.0, 0.0, 0.0), rows)), [0, 1, 2])


def test_every_part_of_the_key_counts_down_to_one_bit():
    B = 6
    base = np.zeros((B, 3))
    base[1:, 2] = np.nextafter(0.5, 1.0)          # the last bit of base_pos[2]: 1 differs from 0
    base[0, 2] = 0.5
    rows = _rows(B)
    rows[3:, 1, 2] = np.nextafter(0.25, 1.0)      # one joint value of waypoint 1: 3 differs from 2
    sid = np.array([0, 0, 0, 0, 0, 1])            # the scene: 5 differs from 4
    np.testing.assert_array_equal(init_heads(keys(sid, base, rows)), [0, 1, 1, 3, 3, 5])


def test_signed_zero_and_nan_compare_as_bits():
    base = np.zeros((4, 3))
    base[1, 0] = -0.0
    np.testing.assert_array_equal(init_heads(keys(0, base, _rows(4))), [0, 1, 2, 2])
    rows = _rows(5)
    rows[1:3, 0, 0] = np.nan                      # two NaNs of the same bits are one key; a NaN is no key of its neighbours
    np.testing.assert_array_equal(init_heads(keys(0, (0.0, 0.0, 0.0), rows)), [0, 1, 1, 3, 3])
    quiet = rows.copy()
    quiet.view(np.uint64)[2, 0, 0] ^= np.uint64(1)  # another payload: another key
    assert np.isnan(quiet[2, 0, 0])
    np.testing.assert_array_equal(init_heads(keys(0, (0.0, 0.0, 0.0), quiet)), [0, 1, 2, 3, 3])


def test_a_run_never_crosses_a_block():
    B = 130
    rows = _rows(B)
    rows[BLOCK - 1:, 0, 0] = 0.75                 # the run changes at the last instance of block 0
    rep = init_heads(keys(0, (0.0, 0.0, 0.0), rows))
    want = np.zeros(B, dtype=np.int32)
    want[BLOCK - 1] = BLOCK - 1
    want[BLOCK:2 * BLOCK] = BLOCK
    want[2 * BLOCK:] = 2 * BLOCK
    np.testing.assert_array_equal(rep, want)
    assert (rep <= np.arange(B)).all() and (rep // BLOCK == np.arange(B) // BLOCK).all() and (rep[rep] == rep).all()


def test_start_rows_follow_qc_for_optimised_joints_and_the_seed_for_the_others():
    from grasptrajopt_amd.robot_desc import load_builtin
    d = load_builtin("panda")
    rng = np.random.default_rng(0)
    B, T = 3, 6
    qc, Q0 = rng.standard_normal((B, d.ndof)), rng.standard_normal((B, d.ndof, T))
    rows = start_rows(d, qc, Q0)
    assert rows.shape == (B, 2, d.n_frames)
    opt = set(int(j) for j in d.opt_index)
    for i in range(d.n_frames):
        dq = int(d.q_index[i])
        if dq < 0:
            assert (rows[:, :, i] == 0.0).all()
        elif dq in opt:
            np.testing.assert_array_equal(rows[:, 0, i], qc[:, dq])
            np.testing.assert_array_equal(rows[:, 1, i], qc[:, dq])
        else:
            np.testing.assert_array_equal(rows[:, :, i], Q0[:, dq, :2])
