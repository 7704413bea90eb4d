"""Trajectory problems with a CHOSEN block pattern, for the block-tridiagonal solve inside the step kernels (k_lm_step<4,1>,
k_lm_step<8,4>, k_lm_step_wide<16>).  Shared by tests/test_step_solve_cpu.py and tests/test_gpu_step_solve.py; imports
without a GPU.

Which loops of that solve run depends on the input: the length of the leading diagonal stretch (waypoints without an
obstacle block or goal term), the meeting block `mid` of the twisted factorisation, the active set.  A case fixes them:

  robot    panda / fetch_mobile thinned to 24 points a link (n = 7 / 10), chain_1 and chain_9_short of tests/small_robots.py
           (n = 1 / 9), chain16 of tests/depth_cases.py (n = 16)
  T, offset  the horizon and the standoff offset (None: no standoff term)
  D        the waypoints that carry an obstacle block at the seed: the field is zero but for one voxel per t in D, an axis
           neighbour of the voxel of one surface point at waypoint t (that point's record then has a gradient and no value),
           chosen so that no point of another waypoint touches the voxel's seven-record stencil.  A `push` waypoint also
           gets a value in the point's own voxel, so that the block has a gradient term J^T r.
  design   a bound design (below), or none
  opts     solver options away from the reference's

RECORD is the certificate: per case the picks (waypoint, surface point, voxels and values) and the bound design's joint /
corner that `PYTHONPATH=. python tests/step_solve_cases.py` found; the CPU test re-derives every pattern from Oracle.eval_normal_eq.

Bound designs (a free-space waypoint cannot be frozen at the seed: its only gradient is the velocity term):
  goal_part      one joint's seed ends on its limit and the goal lies beyond it: the goal block is partly frozen
  goal_all       the seed ends in a corner of the box and the goal lies beyond every limit: the goal block is the identity
  push_first     a joint rides on its limit along the whole seed (its velocity gradient is exactly zero) and the obstacle
  push_mid       block at the first dense waypoint / at the meeting block / at two neighbouring waypoints pushes it outward
  push_adjacent
  late           the seed ends 0.02 rad inside a limit with the goal beyond it: the projection puts the joint on the limit at
                 the first iterate and the active set freezes it afterwards (compared to cap 6)

census() names what an iterate visits; it repeats the kernels' `mid` formula for that only, nothing is compared against it.
"""
import dataclasses
import functools

import numpy as np

import cull_fields as cf
import small_robots as sr
import step_solve_ref as ref
from grasptrajopt_amd import synthetic as syn
from grasptrajopt_amd.robot_desc import load_builtin
from helpers import cfg_of

PAD, PER_LINK = 4, 24
# voxel pitch per robot (the small chains move a few millimetres a waypoint); no axis gets more than MAX_SIDE voxels
RES = {"panda": 0.02, "fetch_mobile": 0.02, "chain_1": 0.003, "chain_9_short": 0.005, "chain16": 0.01}
MAX_SIDE = 110
VAL, VAL_OWN = 0.2, 0.05          # the neighbour voxel's value (the record's gradient), the own voxel's (its value)
CAPS, LATE_CAP = (1, 2, 3), 6
EPS, Q_STABLE = 1e-13, 1e-9       # solver_opts_cases.traj_decided's rule
TEETH = 1e-6                      # a dropped coupling must move the first step by this much: 1000 x the GPU tolerance on Q
ROBOTS = ("panda", "chain_1", "fetch_mobile", "chain_9_short", "chain16")
PUSH = ("push_first", "push_mid", "push_adjacent")


@dataclasses.dataclass(frozen=True)
class Case:
    name: str
    robot: str
    T: int
    offset: object = None       # standoff_offset, None: no standoff term
    D: tuple = ()
    design: str = ""
    opts: tuple = ()            # ((field, value), ...)
    push: tuple = ()            # waypoints of D whose block pushes the design's joint outward
    res: object = None          # a voxel pitch of the case's own: the grid then holds only the last moving link at D's waypoints

    @property
    def caps(self):
        return CAPS + ((LATE_CAP,) if self.design == "late" else ())

    @property
    def group(self):
        """Cases of one group are solved by one handle in one call."""
        return (self.robot, self.T, self.offset, self.opts)


def _cases():
    c = []
    P, W = "panda", "fetch_mobile"
    for T in (4, 5, 6, 7, 50):                                   # s_dense = 0 at m = 2, 3, 4, 5, 48
        c.append(Case(f"p{T}_D2", P, T, None, (2,)))
    for k in (1, 2, 3, 4, 5, 7, 8, 9):                           # nd = k: remainder only, whole batches, both
        c.append(Case(f"p24_nd{k}", P, 24, None, (k + 2,)))
    c += [Case("p24_D19", P, 24, None, (19,)),                    # one dense block between the stretch and mid
          Case("p24_D20", P, 24, None, (20,)),                    # s_dense == mid
          Case("p24_D22", P, 24, None, (22,)),                    # s_dense == mid + 1
          Case("p24_goal_only", P, 24, None, ()),                 # s_dense = m - 1 > mid + 1
          Case("p96_D50", P, 96, None, (50,)),                    # a stretch of 48, twenty dense blocks up to mid
          Case("p50_D44", P, 50, None, (44,)),                    # a stretch of 42 that ends at mid
          Case("p50_D5_26", P, 50, -10, (5, 26)),
          Case("p24_so_first", P, 24, -10, (18,)),                # the standoff slot is the first dense block
          Case("p24_so_after_obs", P, 24, -10, (5,)),             # an obstacle block before the standoff slot
          Case("p12_damping_small", P, 12, None, (5,), opts=(("lambda0", 1e-6),)),
          Case("p12_damping_large", P, 12, -3, (4, 8), opts=(("lambda0", 10.0),))]
    for T, off in ((6, None), (9, None), (12, -3), (13, -3), (24, None)):   # n = 1: no block is dense, s_dense = m
        c.append(Case(f"c1_{T}", "chain_1", T, off, (3,)))
    for s in (0, 1, 62, 63, 64, 65, 92):                          # the wide kernel's masks nz0 / nz1 around bit 64
        c.append(Case(f"w96_s{s}", W, 96, None, (s + 2,), res=0.002 if s == 92 else None))  # (4 mm a waypoint at the seed's slow end)
    c += [Case("w96_none", W, 96, None, ()),
          Case("w50_so_first", W, 50, -10, (45,)),                # standoff slot 38 before the first obstacle slot 43
          Case("w50_D5_26", W, 50, None, (5, 26)),
          Case("w8_D4", W, 8, -3, (4,)),
          Case("c9_4", "chain_9_short", 4, -1, (2,)),
          Case("c9_5", "chain_9_short", 5, None, (3,)),
          Case("c9_12", "chain_9_short", 12, None, (5, 6, 7)),
          Case("c16_8", "chain16", 8, -3, (5,)),
          Case("c16_50", "chain16", 50, None, (30,))]
    for tag, robot in (("p", P), ("w", W)):                       # the bound designs, on both widths
        c += [Case(f"{tag}12_goal_part", robot, 12, None, (5,), "goal_part"),
              Case(f"{tag}12_goal_all", robot, 12, None, (), "goal_all"),
              Case(f"{tag}12_push_first", robot, 12, None, (5,), "push_first", push=(5,)),
              Case(f"{tag}12_push_mid", robot, 12, None, (3, 6), "push_mid", push=(6,)),
              Case(f"{tag}12_push_adjacent", robot, 12, None, (5, 6), "push_adjacent", push=(5, 6)),
              Case(f"{tag}12_late", robot, 12, None, (5,), "late")]
    return c


CASES = {c.name: c for c in _cases()}
NAMES = list(CASES)
GROUPS = {}
for _c in CASES.values():
    GROUPS.setdefault(_c.group, []).append(_c.name)

# ---------------------------------------------------------------------------------------------------------------- certificate
# name -> dict(picks=((t, point, ((voxel, value), ...)), ...), joint=, side=, corner=): written by `PYTHONPATH=. python tests/step_solve_cases.py`
RECORD = {
    'p4_D2': {'picks': ((2, 287, (((16, 12, 38), 0.2),)),)},
    'p5_D2': {'picks': ((2, 287, (((29, 18, 35), 0.2),)),)},
    'p6_D2': {'picks': ((2, 287, (((28, 15, 38), 0.2),)),)},
    'p7_D2': {'picks': ((2, 287, (((31, 22, 36), 0.2),)),)},
    'p50_D2': {'picks': ((2, 193, (((28, 37, 37), 0.2),)),)},
    'p24_nd1': {'picks': ((3, 281, (((34, 36, 39), 0.2),)),)},
    'p24_nd2': {'picks': ((4, 282, (((34, 33, 38), 0.2),)),)},
    'p24_nd3': {'picks': ((5, 286, (((34, 32, 38), 0.2),)),)},
    'p24_nd4': {'picks': ((6, 286, (((34, 30, 38), 0.2),)),)},
    'p24_nd5': {'picks': ((7, 285, (((33, 26, 38), 0.2),)),)},
    'p24_nd7': {'picks': ((9, 286, (((30, 21, 37), 0.2),)),)},
    'p24_nd8': {'picks': ((10, 287, (((29, 17, 37), 0.2),)),)},
    'p24_nd9': {'picks': ((11, 279, (((27, 15, 37), 0.2),)),)},
    'p24_D19': {'picks': ((19, 227, (((11, 18, 43), 0.2),)),)},
    'p24_D20': {'picks': ((20, 199, (((12, 13, 43), 0.2),)),)},
    'p24_D22': {'picks': ((22, 208, (((14, 13, 46), 0.2),)),)},
    'p24_goal_only': {'picks': ()},
    'p96_D50': {'picks': ((50, 207, (((18, 8, 38), 0.2),)),)},
    'p50_D44': {'picks': ((44, 171, (((7, 10, 39), 0.2),)),)},
    'p50_D5_26': {'picks': ((5, 209, (((28, 34, 38), 0.2),)), (26, 279, (((22, 15, 33), 0.2),)))},
    'p24_so_first': {'picks': ((18, 256, (((13, 19, 41), 0.2),)),)},
    'p24_so_after_obs': {'picks': ((5, 286, (((34, 32, 38), 0.2),)),)},
    'p12_damping_small': {'picks': ((5, 287, (((31, 22, 35), 0.2),)),)},
    'p12_damping_large': {'picks': ((4, 287, (((34, 26, 36), 0.2),)), (8, 283, (((21, 17, 32), 0.2),)))},
    'c1_6': {'picks': ((3, 10, (((17, 40, 45), 0.2),)),)},
    'c1_9': {'picks': ((3, 10, (((16, 41, 47), 0.2),)),)},
    'c1_12': {'picks': ((3, 10, (((15, 42, 50), 0.2),)),)},
    'c1_13': {'picks': ((3, 10, (((15, 42, 50), 0.2),)),)},
    'c1_24': {'picks': ((3, 8, (((14, 32, 43), 0.2),)),)},
    'w96_s0': {'picks': ((2, 101, (((71, 88, 16), 0.2),)),)},
    'w96_s1': {'picks': ((3, 72, (((68, 87, 5), 0.2),)),)},
    'w96_s62': {'picks': ((64, 239, (((46, 6, 25), 0.2),)),)},
    'w96_s63': {'picks': ((65, 239, (((44, 6, 26), 0.2),)),)},
    'w96_s64': {'picks': ((66, 239, (((40, 6, 26), 0.2),)),)},
    'w96_s65': {'picks': ((67, 239, (((36, 8, 26), 0.2),)),)},
    'w96_s92': {'picks': ((94, 239, (((20, 11, 13), 0.2),)),)},
    'w96_none': {'picks': ()},
    'w50_so_first': {'picks': ((45, 238, (((8, 13, 37), 0.2),)),)},
    'w50_D5_26': {'picks': ((5, 203, (((46, 93, 39), 0.2),)), (26, 239, (((86, 53, 25), 0.2),)))},
    'w8_D4': {'picks': ((4, 239, (((94, 37, 27), 0.2),)),)},
    'c9_4': {'picks': ((2, 63, (((29, 76, 82), 0.2),)),)},
    'c9_5': {'picks': ((3, 63, (((28, 56, 64), 0.2),)),)},
    'c9_12': {'picks': ((5, 63, (((64, 83, 65), 0.2),)), (6, 63, (((48, 78, 74), 0.2),)), (7, 63, (((34, 68, 81), 0.2),)))},
    'c16_8': {'picks': ((5, 767, (((68, 30, 35), 0.2),)),)},
    'c16_50': {'picks': ((30, 766, (((62, 41, 66), 0.2),)),)},
    'p12_goal_part': {'joint': 0, 'side': 1, 'seed': 0, 'picks': ((5, 287, (((52, 27, 35), 0.2),)),)},
    'p12_goal_all': {'joint': 0, 'side': 1, 'seed': 0, 'corner': (-1, 1, 1, -1, -1, -1, 1), 'picks': ()},
    'p12_push_first': {'joint': 0, 'side': 1, 'seed': 0, 'picks': ((5, 271, (((19, 28, 35), 0.2), ((20, 28, 35), 0.05))),)},
    'p12_push_mid': {'joint': 0, 'side': 1, 'seed': 0, 'picks': ((3, 286, (((19, 21, 37), 0.2),)), (6, 262, (((24, 32, 33), 0.2), ((23, 32, 33), 0.05))))},
    'p12_push_adjacent': {'joint': 0, 'side': 1, 'seed': 0, 'picks': ((5, 271, (((19, 28, 35), 0.2), ((20, 28, 35), 0.05))), (6, 262, (((24, 32, 33), 0.2), ((23, 32, 33), 0.05))))},
    'p12_late': {'joint': 0, 'side': 1, 'seed': 0, 'picks': ((5, 287, (((51, 27, 35), 0.2),)),)},
    'w12_goal_part': {'joint': 0, 'side': 1, 'seed': 0, 'picks': ((5, 239, (((80, 66, 26), 0.2),)),)},
    'w12_goal_all': {'joint': 0, 'side': 1, 'seed': 2, 'corner': (1, -1, -1, -1, -1, -1, -1, 1, -1, -1), 'picks': ()},
    'w12_push_first': {'joint': 0, 'side': 1, 'seed': 0, 'picks': ((5, 239, (((89, 66, 26), 0.2), ((90, 66, 26), 0.05))),)},
    'w12_push_mid': {'joint': 0, 'side': 1, 'seed': 0, 'picks': ((3, 239, (((66, 94, 35), 0.2),)), (6, 239, (((87, 38, 24), 0.2), ((88, 38, 24), 0.05))))},
    'w12_push_adjacent': {'joint': 0, 'side': 1, 'seed': 0, 'picks': ((5, 239, (((89, 66, 26), 0.2), ((90, 66, 26), 0.05))), (6, 239, (((87, 38, 24), 0.2), ((88, 38, 24), 0.05))))},
    'w12_late': {'joint': 0, 'side': 1, 'seed': 0, 'picks': ((5, 239, (((80, 66, 26), 0.2),)),)},
}


# -------------------------------------------------------------------------------------------------------------------- robots
@functools.lru_cache(maxsize=None)
def oracle_mod():
    from oracle import oracle
    oracle.build()
    return oracle


@functools.lru_cache(maxsize=None)
def robot(name):
    """(desc, link_ee, link_gripper, n_gripper_points, qc)."""
    rng = np.random.default_rng(40 + ROBOTS.index(name))
    if name in ("panda", "fetch_mobile"):
        cfg, desc = cfg_of(name), cf.thin_robot(load_builtin(name), per_link=PER_LINK)
        pose = np.array(cfg["default_pose"], dtype=np.float64)
        return desc, cfg["link_ee"], cfg["link_gripper"], None, np.concatenate([np.zeros(desc.ndof - len(pose)), pose])
    if name == "chain16":
        import depth_cases as dc
        desc, ee, gr, ngp = dc.plan_robot("chain16")
        desc = cf.thin_robot(desc, per_link=PER_LINK)
    else:
        r = sr.Robot(name)
        desc, ee, gr, ngp = r.desc, r.ee, r.gripper, r.n_gripper_points
    mid, half = 0.5 * (desc.lower + desc.upper), 0.5 * (desc.upper - desc.lower)
    return desc, ee, gr, ngp, mid + 0.3 * half * rng.uniform(-1, 1, desc.ndof)


class Problem:
    """One instance: qc, a goal, a seed (syn.make_seed towards a configuration 0.15 rad off the goal's, so that the goal
    term pulls), the design's changes to them, a grid around the seed's swept volume, and the field of the case's picks."""

    def __init__(self, case, record=None):
        om = oracle_mod()
        self.case = case
        rec = self.record = RECORD.get(case.name, {}) if record is None else record
        d, self.ee, self.gr, self.ngp, qc = robot(case.robot)
        self.desc = d
        oi = d.opt_index
        rng = np.random.default_rng([ROBOTS.index(case.robot), case.T, rec.get("seed", 0)])
        lo, hi = np.maximum(d.lower, -2.5), np.minimum(d.upper, 2.5)
        mid, half = 0.5 * (lo + hi), 0.5 * (hi - lo)
        qc = qc.copy()
        # the seed's far end: on the other side of each joint's range, so that every waypoint moves every link
        qg = mid - np.where(qc >= mid, 1.0, -1.0) * half * rng.uniform(0.3, 0.6, d.ndof)
        qt = qg.copy()
        qt[oi] += 0.15 * rng.uniform(-1, 1, len(oi))               # the goal's configuration
        j, side = rec.get("joint", 0), rec.get("side", 1)
        bound = lambda i, s: (d.upper if s > 0 else d.lower)[oi[i]]
        if case.design == "goal_part":
            qg[oi[j]], qt[oi[j]] = bound(j, side), bound(j, side) + 0.4 * side
        elif case.design == "goal_all":
            corner = np.asarray(rec.get("corner", np.ones(len(oi))))
            for i in range(len(oi)):
                qg[oi[i]] = bound(i, corner[i])
                qt[oi[i]] = qg[oi[i]] + 0.3 * corner[i]
        elif case.design in PUSH:
            qc[oi[j]] = qg[oi[j]] = qt[oi[j]] = bound(j, side)
        elif case.design == "late":
            qg[oi[j]], qt[oi[j]] = bound(j, side) - 0.02 * side, bound(j, side) + 0.4 * side
        qg[d.param_index] = qt[d.param_index] = qc[d.param_index]
        self.opts = om.reference_opts(T=case.T, standoff_offset=case.offset if case.offset is not None else -1,
                                      max_iter=max(case.caps), **dict(case.opts))
        self.o = om.Oracle(d, self.ee, self.gr, self.opts, n_gripper_points=self.ngp)
        self.qc, self.base, self.n_goals = qc, np.zeros(3), 1
        self.goals = self.o.eval_fk(qt)[0, d.frame_index(self.ee)].reshape(1, 16)
        axis = cfg_of(case.robot)["axis_standoff"] if case.robot in ("panda", "fetch_mobile") else "z"
        self.S = syn.standoff_pose(-0.05, axis) if case.offset is not None else None
        Q0 = syn.make_seed(qc, qg, case.T, d.param_index)
        Q0[oi, -1] = qg[oi]                                         # (make_seed stops one sample short of qg)
        self.Q0 = ref.pinned(d, qc, Q0)
        self._geo = None
        self.set_picks(rec.get("picks", ()))

    # the grid: a box around every surface point of the seed, PAD voxels wider
    @property
    def geo(self):
        if self._geo is None:
            om = oracle_mod()
            g = om.Oracle(self.desc, self.ee, self.gr, self.opts, n_gripper_points=self.ngp)
            xyz = g.eval_points(0, np.ascontiguousarray(self.Q0.T), self.base, want_field=False)[0]
            if self.case.res is None:
                xyz = xyz.reshape(-1, 3)
                ext = float((xyz.max(axis=0) - xyz.min(axis=0)).max())
                res = max(RES[self.case.robot], round(ext / (MAX_SIDE - 2 * PAD - 2), 3))
            else:  # (points outside the grid read its border voxels, which stay zero)
                last = int(np.flatnonzero(self.desc.link_is_moving())[-1])
                ts = sorted({min(max(t + k, 0), self.case.T - 1) for t in self.case.D for k in (-1, 0, 1)})
                xyz, res = xyz[ts][:, self.desc.point_link == last].reshape(-1, 3), self.case.res
            lo = np.floor(xyz.min(axis=0) / res) * res - PAD * res - 0.37 * res
            shape = tuple(int(x) for x in np.ceil((xyz.max(axis=0) - lo) / res) + PAD)
            self._geo = cf.Geometry(g, self.desc, self.Q0[None], self.base[None], cf.Grid(shape, tuple(lo), res))
        return self._geo

    def set_picks(self, picks):
        self.picks = tuple(picks)
        grid = self.geo.grid
        c = np.zeros(grid.nvox, np.float32)
        for _, _, cells in self.picks:
            for v, val in cells:
                c[grid.flat(v)] = val
        self.scene = (c, c, grid.shape, grid.origin, grid.res)
        self.o.set_scene(0, *self.scene)

    def solve_args(self, Q0=None):
        return (0, self.qc[None], self.goals[None], 1, self.S, self.base[None], (self.Q0 if Q0 is None else Q0)[None])


@functools.lru_cache(maxsize=None)
def problem(name):
    return Problem(CASES[name])


# -------------------------------------------------------------------------------------------------------------------- census
def _mid(m, sd, w):
    """The kernels' balance formula (w = 10 narrow, 20 wide), repeated to NAME what a case visits."""
    sd = sd if sd < m else m - 1
    m2, m1 = (w * (m - 1) + (w - 1) * sd) // (2 * w), (w * (m - 1)) // (w + 1)
    mid = m2 if m2 >= sd else (m1 if m1 < sd else sd)
    return min(max(mid, 0), m - 1)


def census(case, Q, lam):
    """What the step solve at iterate Q (ndof, T) under damping lam visits: dict(m, n, offdiag: slots whose damped block has
    an off-diagonal entry once frozen rows are the identity, obs: slots with an obstacle block, s_dense_narrow, s_dense_wide,
    s_dense / mid / nd by the rule of the case's width, act (m, n), features: set of names)."""
    p = problem(case.name) if isinstance(case, Case) else case
    case = p.case
    sysd = ref.system(p.o, p, 0, Q, lam)
    m, n, T, act, M = sysd["m"], sysd["n"], case.T, sysd["act"], sysd["M"]
    off = []
    for s in range(m):
        blk = M[s * n:(s + 1) * n, s * n:(s + 1) * n]
        if np.any(blk - np.diag(np.diag(blk)) != 0.0):
            off.append(s)
    obs = [t - 2 for t in range(2, T) if sysd["obs"][t]]
    so = case.offset is not None
    st = T + case.offset - 2 if so else None
    sdn = off[0] if off else m
    sdw = min(obs[0] if obs else m, min(st, T - 3) if so else T - 3)
    wide = n > 8
    sd = sdw if wide else sdn
    mid = _mid(m, sd, 20 if wide else 10)
    nd = min(sd, mid)
    f = set()
    if not wide:
        if sd == 0:
            f.add(f"sdense0_m{m}")
        f.add(f"nd{nd}")
        if nd >= 40:
            f.add("stretch40")
        if mid - nd >= 1:
            f.add("dense_between_1")
        if mid - nd >= 3:
            f.add("dense_between_3")
        if sd < m:
            f.add("sdense_eq_mid" if sd == mid else ("sdense_eq_mid1" if sd == mid + 1 else ("sdense_gt_mid1" if sd > mid + 1 else "sdense_lt_mid")))
        if sd == m - 1 and not obs and not so:
            f.add("goal_only")
        if so and sd == st and obs and obs[0] > st:
            f.add("standoff_first")
        if so and obs and obs[0] < st:
            f.add("obs_before_standoff")
        if sd == m:
            f.add(f"sdense_m_T{T}")
    else:
        if T == 96 and obs:
            f.add(f"first_obs_{obs[0]}")
            if obs[0] == m - 2:
                f.add("first_obs_m2")
        if not obs:
            f.add("no_obs")
        if so and obs and st < obs[0]:
            f.add("standoff_before_obs")
        f.update((f"T{T}", f"n{n}"))
    g = set()
    if 0 < act[m - 1].sum() < n:
        g.add("goal_part")
    if act[m - 1].all():
        g.add("goal_all")
    if sd < m and sd in obs and act[sd].any():
        g.add("push_first")
    if mid in obs and act[mid].any():
        g.add("push_mid")
    if any(s + 1 in obs and (act[s] & act[s + 1]).any() for s in obs):
        g.add("push_adjacent")
    pre = "wide:" if wide else "narrow:"
    f = {pre + x for x in f | g}
    return dict(m=m, n=n, offdiag=off, obs=obs, s_dense_narrow=sdn, s_dense_wide=sdw, s_dense=sd, mid=mid, nd=nd, act=act,
                wide=wide, features=f, sysd=sysd)


REQUIRED = (["narrow:" + x for x in
             [f"sdense0_m{m}" for m in (2, 3, 4, 5, 48)] + [f"nd{k}" for k in (1, 2, 3, 4, 5, 7, 8, 9)]
             + ["stretch40", "dense_between_1", "dense_between_3", "sdense_eq_mid", "sdense_eq_mid1", "sdense_gt_mid1", "goal_only",
                "standoff_first", "obs_before_standoff"] + [f"sdense_m_T{T}" for T in (6, 9, 12, 13, 24)]]
            + ["wide:" + x for x in
               [f"first_obs_{s}" for s in (0, 1, 62, 63, 64, 65)] + ["first_obs_m2", "no_obs", "standoff_before_obs"]
               + [f"T{T}" for T in (4, 5, 8, 50, 96)] + [f"n{n}" for n in (9, 10, 16)]]
            + [w + x for w in ("narrow:", "wide:")
               for x in ("goal_part", "goal_all", "push_first", "push_mid", "push_adjacent", "frozen_later", "reject_then_accept")])


# ------------------------------------------------------------------------------------------------- the oracle and the restatement
@functools.lru_cache(maxsize=None)
def trace(name):
    """step_solve_ref.lm on the case to its largest cap: (Q, f, iterations, status, trace)."""
    p = problem(name)
    return ref.lm(p.o, p, 0, p.Q0, max(p.case.caps))


def _run(p, cap, Q0=None):
    """The oracle capped at `cap`, and its accept / reject sequence: evaluation k was accepted where the answer capped at k
    differs from the answer capped at k - 1 (the objective trace alone does not tell: a step is also rejected when the
    model predicts no decrease)."""
    acc, prev = [], None
    for k in range(1, cap + 1):
        p.o.set_opts(max_iter=k)
        Q, dQ, f, it, st = p.o.solve_batch(*p.solve_args(Q0))
        if it[0] < k:
            break
        acc.append(bool(np.any(Q[0] != (p.Q0 if Q0 is None else ref.pinned(p.desc, p.qc, Q0)) if prev is None else Q[0] != prev)))
        prev = Q[0]
    return Q[0], dQ[0], float(f[0]), int(it[0]), int(st[0]), acc


@functools.lru_cache(maxsize=None)
def oracle_run(name, cap):
    """(Q, dQ, f, iterations, status, accept sequence) of the oracle capped at `cap`."""
    return _run(problem(name), cap)


@functools.lru_cache(maxsize=None)
def decided(name, cap):
    """solver_opts_cases.traj_decided's rule on one case: with the seed's free entries moved by +-1e-13 the oracle gives
    the same iterations, status and accept / reject sequence and an answer within 1e-9.  An entry that sits on a bound
    stays there: the solvers clip an outward move away, and an inward one changes the active set, which is another
    problem and not a rounding."""
    p = problem(name)
    d = p.desc
    oi = d.opt_index
    Q, _, _, it, st, acc = oracle_run(name, cap)
    for e in (EPS, -EPS):
        Q0 = p.Q0.copy()
        free = (Q0[oi, 2:] > d.lower[oi][:, None]) & (Q0[oi, 2:] < d.upper[oi][:, None])
        Q0[oi, 2:] += e * free
        Q2, _, _, it2, st2, acc2 = _run(p, cap, Q0)
        if (it2, st2, acc2) != (it, st, acc) or not np.abs(Q2 - Q).max() <= Q_STABLE:
            return False
    return True


def features(name):
    """The census of every iterate the case's capped solves step from, and what the sequence itself shows."""
    p = problem(name)
    tr = trace(name)[4]
    out, first = set(), None
    for k, rec in enumerate(tr):
        c = census(p, rec["Q"], rec["lam"])
        first = c if k == 0 else first
        out |= c["features"]
        pre = "wide:" if c["wide"] else "narrow:"
        if k >= 1 and (rec["act"] & ~tr[0]["act"]).any():
            out.add(pre + "frozen_later")
        if k >= 1 and rec["accepted"] and not tr[k - 1]["accepted"]:
            out.add(pre + "reject_then_accept")
    return out, first


def teeth_slots(c):
    """The structural slots of the coupling e: 0, nd - 1, nd, mid - 1, mid, m - 2, where they exist."""
    return sorted({s for s in (0, c["nd"] - 1, c["nd"], c["mid"] - 1, c["mid"], c["m"] - 2) if 0 <= s <= c["m"] - 2})


def teeth(name):
    """{slot: largest move of the first step when the coupling between slot and slot + 1 is dropped from the damped matrix},
    for the structural slots whose coupling the active set has left in place."""
    p = problem(name)
    c = census(p, p.Q0, float(p.opts.lambda0))
    sysd, n = c["sysd"], c["n"]
    base = ref.step(p, p.Q0, sysd)[0]
    out = {}
    for s in teeth_slots(c):
        M = sysd["M"].copy()
        if not np.any(M[s * n:(s + 1) * n, (s + 1) * n:(s + 2) * n] != 0.0):
            continue  # (every variable on one side is frozen: the active set has dropped this coupling already)
        M[s * n:(s + 1) * n, (s + 1) * n:(s + 2) * n] = 0.0
        M[(s + 1) * n:(s + 2) * n, s * n:(s + 1) * n] = 0.0
        out[s] = float(np.abs(ref.step(p, p.Q0, sysd, M=M)[0] - base).max())
    return out


# ------------------------------------------------------------------------------------------------------------------- builder
def _owners(geo):
    """flat voxel -> set of the waypoints with a point in it."""
    g, own = geo.grid, {}
    f = geo.pv[0, :, :, 2] + g.shape[2] * (geo.pv[0, :, :, 1] + g.shape[1] * geo.pv[0, :, :, 0])
    for t in range(f.shape[0]):
        for x in np.unique(f[t]).tolist():
            own.setdefault(x, set()).add(t)
    return own


def find_picks(p):
    """Picks for p.case.D, first fit: for each t the first (point, axis neighbour) whose stencils no other waypoint touches
    and which the oracle confirms: blocks exactly at the waypoints picked so far, the new one with an off-diagonal entry
    (n > 1), a push block with J^T r pointing outward for the design's joint."""
    case, geo, d = p.case, p.geo, p.desc
    g, own = geo.grid, _owners(geo)
    n, oi = d.n_opt, d.opt_index
    j, side = p.record.get("joint", 0), p.record.get("side", 1)
    moving = d.link_is_moving()
    pts = [i for i in range(d.n_points - 1, -1, -1) if moving[d.point_link[i]]]
    picks, used = [], []
    for t in case.D:
        found = None
        for i in pts:
            if not geo.fine[0, t, d.point_link[i]]:
                continue
            o = geo.pv[0, t, i]
            for a in range(3):
                for sg in (1, -1):
                    v = o.copy()
                    v[a] += sg
                    if not all(2 <= v[x] < g.shape[x] - 2 for x in range(3)):
                        continue
                    cells = [(tuple(int(x) for x in v), VAL)] + ([(tuple(int(x) for x in o), VAL_OWN)] if t in case.push else [])
                    sten = {g.flat(w) for cv, _ in cells for w in cf._stencil(cv, g)}
                    if any(own.get(w, set()) - {t} for w in sten) or any(np.abs(np.array(cv) - np.array(u)).max() <= 3 for cv, _ in cells for u in used):
                        continue
                    p.set_picks(picks + [(t, i, tuple(cells))])
                    JtJ, Jtr, _, _, _ = p.o.eval_normal_eq(0, p.goals[None], 1, p.S, p.base, p.Q0[None])
                    nzb = [tt for tt in range(case.T) if np.any(JtJ[0, tt] != 0.0)]
                    if nzb != sorted(x[0] for x in picks) + [t]:
                        continue
                    B = JtJ[0, t]
                    if n > 1 and not np.any(B - np.diag(np.diag(B)) != 0.0):
                        continue
                    if t in case.push and not Jtr[0, t, j] * side < 0.0:
                        continue
                    found = (t, i, tuple(cells))
                    break
                if found:
                    break
            if found:
                break
        if found is None:
            raise RuntimeError(f"{case.name}: no pick for waypoint {t}")
        picks.append(found)
        used += [cv for cv, _ in found[2]]
    p.set_picks(picks)
    return tuple(picks)


def build(name):
    """The RECORD entry of a case: tries design parameters (joint, side, corner, seed) until the census shows the design."""
    case = CASES[name]
    n = robot(case.robot)[0].n_opt
    want = {"goal_part": "goal_part", "goal_all": "goal_all", "late": "frozen_later"}
    want.update({k: k for k in PUSH})

    def shows(p):
        feats = set()
        if case.design == "late":
            tr = ref.lm(p.o, p, 0, p.Q0, LATE_CAP)[4]
            return len(tr) > 1 and any((r["act"] & ~tr[0]["act"]).any() for r in tr[1:])
        feats = census(p, p.Q0, float(p.opts.lambda0))["features"]
        return any(x.endswith(":" + want[case.design]) for x in feats)

    if not case.design:
        p = Problem(case, {})
        return dict(picks=find_picks(p))
    for seed in range(4):
        for j in range(n):
            for side in (1, -1):
                rec = dict(joint=j, side=side, seed=seed)
                if case.design == "goal_all":
                    if j or side < 0:
                        continue
                    corner = np.random.default_rng(seed).choice([-1, 1], n)
                    for _ in range(40):   # flip the joints whose gradient points inward until none does
                        p = Problem(case, dict(rec, corner=tuple(int(x) for x in corner)))
                        sysd = ref.system(p.o, p, 0, p.Q0, 1e-3)
                        bad = ~sysd["act"][-1]
                        if not bad.any():
                            break
                        corner = np.where(bad, -corner, corner)
                    rec["corner"] = tuple(int(x) for x in corner)
                try:
                    p = Problem(case, rec)
                    rec["picks"] = find_picks(p)
                    p = Problem(case, rec)
                except RuntimeError:
                    continue
                if shows(p):
                    return rec
    raise RuntimeError(f"{name}: no design found")


if __name__ == "__main__":
    import sys
    for nm in (sys.argv[1:] or NAMES):
        print(f"    {nm!r}: {build(nm)!r},", flush=True)
