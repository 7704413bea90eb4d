"""CPU: the cases of tests/held_ref.py (the held object's points along the motion after the grasp, gto_check_held_paths) are
what its text claims, decided by a margin the GPU's kinematics cannot cross, and the new entry points are declared, bound
and exported alike."""
import ctypes as C

import numpy as np
import pytest

import held_ref as hr


@pytest.mark.parametrize("name", hr.ROBOTS)
def test_every_case_is_decided_by_a_margin(oracle_mod, name):
    """gto_eval_fk is held to the oracle to 1e-13; a decision at least 1e-9 m (1e-9 px) from turning is the GPU's too, so its
    counts must be equal.  A case that misses changes its seed in held_ref.SEEDS."""
    for frame in ("world", "object"):
        for kind in hr.KINDS:
            counts, m1, m2 = hr.expected(oracle_mod, name, kind, frame)
            print(name, frame, kind, "margins", m1, m2)
            if kind.startswith("cloud"):
                assert m1 >= hr.TOL and m2 == 0, (name, frame, kind, m1, m2)
            else:
                assert m1 >= hr.TOL and m2 >= hr.TOL, (name, frame, kind, m1, m2)
            assert (counts >= 0).all() and (counts <= np.array(hr.N_HELD)[:, None]).all()
    for kind in ("depth", "labels", "cloud11"):
        counts, m1, m2 = hr.expected(oracle_mod, name, kind, nan_point=True)
        assert m1 >= hr.TOL and (m2 == 0 if kind.startswith("cloud") else m2 >= hr.TOL)


@pytest.mark.parametrize("name", hr.ROBOTS)
def test_the_counts_span_nothing_some_and_all(oracle_mod, name):
    seen = set()
    for kind in hr.KINDS:
        counts = hr.expected(oracle_mod, name, kind)[0]
        for b, n in enumerate(hr.N_HELD):
            if n >= 63:
                seen |= {"none"} if (counts[b] == 0).any() else set()
                seen |= {"some"} if ((counts[b] > 0) & (counts[b] < n)).any() else set()
                seen |= {"all"} if (counts[b] == n).any() else set()
    assert seen == {"none", "some", "all"}, seen
    for kind in ("cloud1", "cloud11"):  # the box is felt
        assert (hr.expected(oracle_mod, name, kind)[0] > 0).any()


@pytest.mark.parametrize("name", hr.ROBOTS)
def test_the_label_rule_decides_the_grasp_column(oracle_mod, name):
    plain, ruled = hr.expected(oracle_mod, name, "depth")[0], hr.expected(oracle_mod, name, "labels")[0]
    held = np.array(hr.N_HELD) > 0
    assert (plain[held, 0] > 0).all() and (plain[:, 0] == hr.N_HELD).all()  # on or behind the object's own seen surface
    assert (ruled[:, 0] == 0).all()                                          # what was behind the held object was never seen
    assert (plain != ruled).any() and (ruled <= plain).all()
    assert (ruled > 0).any()                                                 # the neighbour's pixels still count


@pytest.mark.parametrize("name", hr.ROBOTS)
def test_object_frame_points_are_the_world_points(oracle_mod, name):
    s = hr.case(oracle_mod, name)
    for b, n in enumerate(hr.N_HELD):
        np.testing.assert_allclose(hr.place(s.held_obj[b, :n], s.pose[b]), s.held[b, :n], rtol=0, atol=1e-14)
    for kind in hr.KINDS:  # the margin is far above the rounding of the placement: the same counts
        np.testing.assert_array_equal(hr.expected(oracle_mod, name, kind, "object")[0], hr.expected(oracle_mod, name, kind)[0])


def test_a_nan_point_is_one_point_less(oracle_mod):
    b, i = hr.NAN_POINT
    assert i < hr.N_HELD[b]
    for kind in ("depth", "labels", "cloud11"):
        clean, dirty = hr.expected(oracle_mod, "panda", kind)[0], hr.expected(oracle_mod, "panda", kind, nan_point=True)[0]
        rows = np.arange(hr.B) != b
        np.testing.assert_array_equal(dirty[rows], clean[rows])
        assert ((clean[b] - dirty[b]) >= 0).all() and ((clean[b] - dirty[b]) <= 1).all()
    clean, dirty = hr.expected(oracle_mod, "panda", "depth")[0], hr.expected(oracle_mod, "panda", "depth", nan_point=True)[0]
    assert dirty[b, 0] == clean[b, 0] - 1  # at the grasp column every point counts


def test_the_restatement_carries_points_rigidly(oracle_mod):
    """Against plain matrix algebra: X_t = E_t E_a^-1 (x - base) + base, to rounding."""
    s = hr.case(oracle_mod, "panda")
    b = 6
    X = hr.held_world(s.frames[b], s.frames[b, 0], s.base, s.held[b])
    for t in range(hr.TP_FULL):
        M = s.frames[b, t] @ np.linalg.inv(s.frames[b, 0])
        want = (s.held[b] - s.base) @ M[:3, :3].T + M[:3, 3] + s.base
        np.testing.assert_allclose(X[t], want, rtol=0, atol=1e-13)
    np.testing.assert_allclose(X[0], s.held[b], rtol=0, atol=1e-14)  # column 0 is the grasp
    assert np.abs(X[-1] - X[0]).max() > 0.02                         # and the motion moves them


def test_the_second_chain_instance(oracle_mod):
    c = hr.chunk_instance(oracle_mod)
    assert c.paths.shape == (64, c.desc.ndof, 65) and c.held.shape == (64, 4096, 3) and c.n_held[63] == 4096
    assert 64 * 65 * 4096 > 1 << 24 >= 63 * 65 * 4096
    assert (c.counts > 0).any() and (c.counts[63] != c.counts[61]).any()  # plan 63's own count of points shows


def test_new_entry_points_agree_in_header_binding_and_library():
    import __graft_entry__ as g
    g.build()
    from grasptrajopt_amd import _capi
    from test_capi_cpu import header_prototypes, table_type
    hdr, lib = header_prototypes(), _capi.load_library()
    for name in ("gto_check_held_paths", "gto_check_held_paths_device"):
        assert name in hdr and name in _capi.PROTOTYPES and name in _capi.EXPORTED_SYMBOLS
        ret, args = hdr[name]
        restype, argtypes = _capi.PROTOTYPES[name]
        assert restype is table_type(_capi, ret) and len(argtypes) == len(args)
        for k, (a, t) in enumerate(zip(args, argtypes)):
            untyped = t is C.c_void_p and a.endswith("*") and not a.endswith("**")
            assert t is table_type(_capi, a) or untyped, (name, k, a, t)
        fn = getattr(lib, name)  # exported, and called with the table's types
        assert fn.restype is restype and list(fn.argtypes) == list(argtypes)
    names = list(hdr)
    assert names.index("gto_check_held_paths") == names.index("gto_check_paths_device") + 1
    # the host variant differs from the device variant by the stream alone
    assert len(hdr["gto_check_held_paths_device"][1]) == len(hdr["gto_check_held_paths"][1]) + 1
