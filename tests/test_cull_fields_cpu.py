"""CPU: the promises of tests/cull_fields.py, the field builder of the broad-phase culling tests (tests/test_gpu_culling.py).

A designed edge voxel is exactly R (Chebyshev index steps) from its chunk's centre voxel, so that margin 0 keeps the chunk and
margin -1 would cull it; a near-miss voxel leaves every touched record exactly zero; the numpy distance transform equals its
definition."""
import numpy as np
import pytest

import cull_fields as cf
from grasptrajopt_amd import synthetic as syn
from grasptrajopt_amd.robot_desc import load_builtin
from helpers import cfg_of


@pytest.mark.parametrize("shape,density,cap", [((5, 7, 3), 0.05, 48), ((1, 9, 6), 0.04, 48), ((11, 2, 13), 0.02, 3),
                                               ((6, 6, 6), 0.0, 48), ((4, 12, 1), 0.1, 2), ((9, 9, 9), 0.003, 5)])
def test_chebyshev_transform_equals_its_definition(shape, density, cap):
    rng = np.random.default_rng(sum(shape) + cap)
    mask = rng.random(shape) < density
    if density > 0 and not mask.any():
        mask[tuple(s // 2 for s in shape)] = True
    np.testing.assert_array_equal(cf.chebyshev(mask, cap), cf.chebyshev_brute(mask, cap))


def test_chebyshev_transform_against_scipy():
    nd = pytest.importorskip("scipy.ndimage")
    rng = np.random.default_rng(3)
    mask = rng.random((17, 9, 23)) < 0.01
    ref = nd.distance_transform_cdt(~mask, metric="chessboard")
    np.testing.assert_array_equal(cf.chebyshev(mask, 48), np.minimum(ref, 48))


def test_records_follow_the_clipped_differences():
    shape = (4, 1, 5)
    c = np.zeros(shape, np.float32)
    c[0, 0, 2] = 0.03  # on the low x face, y axis of length one
    nz = cf.records_nonzero(c, shape)
    want = {(0, 0, 2), (1, 0, 2), (0, 0, 1), (0, 0, 3)}  # the voxel, its clipped x difference (x = 0 and 1), z neighbours
    assert set(map(tuple, np.argwhere(nz))) == want


def _panda_geometry(res, shape=None, origin=(-1.1, -1.1, -0.4), T=12, B=3, seed=0):
    from oracle import oracle as om
    desc = cf.thin_robot(load_builtin("panda"))
    cfg = cfg_of("panda")
    o = om.Oracle(desc, cfg["link_ee"], cfg["link_gripper"], om.reference_opts(T=T, standoff_offset=-3))
    rng = np.random.default_rng(seed)
    qc = np.tile(np.array(cfg["default_pose"]), (B, 1))
    qg = rng.uniform(0.6 * desc.lower, 0.6 * desc.upper, (B, desc.ndof))
    qg[:, desc.param_index] = qc[:, desc.param_index]
    Q0 = np.stack([syn.make_seed(qc[b], qg[b], T, desc.param_index) for b in range(B)])
    n = int(np.ceil(2.2 / res))
    shape = shape or (n, n, n)

    def make(shift):
        return cf.Geometry(o, desc, Q0, np.zeros((B, 3)), cf.Grid(shape, tuple(np.asarray(origin) + shift * res), res))
    return make, T - 3


@pytest.mark.parametrize("res,shape,kind", [(r, s, k) for r, s in [(0.04, None), (0.1, None), (0.3, None), (0.05, (1, 40, 33)), (0.05, (64, 2, 5))]
                                            for k in ("edge", "gradient", "near") if not (k == "edge" and s is not None)])
def test_designs_sit_on_the_edge_of_the_culling_rule(oracle_mod, res, shape, kind):
    make, ts = _panda_geometry(res, shape)
    fb = cf.search(make, ts, [dict(kind=kind), dict(kind=kind)], seed=1)
    g = fb.geo.grid
    for d in fb.designs:
        c = fb.fields[d.field]
        assert np.count_nonzero(fb.fields["all"]) + np.count_nonzero(fb.fields["obs"]) == len(fb.designs)
        dist = cf.chebyshev(cf.records_nonzero(c, g.shape))
        D = int(dist[d.centre])
        nzrec = cf.records_nonzero(c, g.shape)
        pv = tuple(int(x) for x in fb.geo.pv[d.b, d.t, d.point])
        R = int(cf.cull_radius(fb.geo.radius[d.link], g.res))
        assert d.R == R
        if kind in ("edge", "gradient"):
            assert D == R                    # kept at margin 0 (D <= R) ...
            assert D > int(cf.cull_radius(fb.geo.radius[d.link], g.res, margin=-1))  # ... culled at margin -1
            assert nzrec[pv]                 # and the point's record is non-zero: something to be found
            vv = np.asarray(c).reshape(g.shape)[pv]
            assert (vv != 0) == (kind == "edge")  # gradient-only: c = 0 at the touched voxel, a non-zero difference
            assert np.abs(np.asarray(pv) - np.asarray(d.centre)).max() == R
        else:
            assert D <= R                    # the chunk survives the broad phase ...
            touched = fb.geo.touched()
            assert not any(nzrec.reshape(-1)[f] for f in touched)  # ... and every record it touches is exactly zero


def test_cap_designs_reach_the_saturation(oracle_mod):
    """A resolution that makes R = 47 for one chunk: the nearest record is its farthest point's distance away (up to 47),
    and the field saturates at the cap elsewhere."""
    desc = cf.thin_robot(load_builtin("panda"))
    _, rad = cf.chunk_spheres(desc)
    l = int(np.argmax(rad))
    res = rad[l] / 46.5
    make, ts = _panda_geometry(res, shape=(120, 120, 120), origin=(-0.1, -0.3, 0.25))
    fb = cf.search(make, ts, [dict(kind="farthest", links=[l], bs=[0], ts=[5])], seed=2)
    d = fb.designs[0]
    dist = cf.chebyshev(cf.records_nonzero(fb.fields[d.field], fb.geo.grid.shape))
    assert d.R == 47 and dist[d.centre] == d.dist and 30 <= d.dist <= 47
    np.testing.assert_array_equal(dist[::7, ::7, ::7], cf.chebyshev_brute(cf.records_nonzero(fb.fields[d.field], fb.geo.grid.shape))[::7, ::7, ::7])
    assert dist.max() == cf.CAP  # some voxels saturate
