"""GPU: WHEN the stream-ordered entry points read and write, not what they compute.

Every other GPU test that passes a stream synchronises the device first: its call starts on an idle device with finished
inputs, and there a missing dependency, a hidden use of another stream or a host array read too late cannot change a bit.
Here the stream is held busy by one bounded kernel (tests/held_stream.py) while the call is enqueued, which makes each of
these deterministic.  Per entry point (tests/stream_order_cases.py builds true inputs and a valid decoy of the same shapes):

  idle pass         synchronise, call, synchronise -- what today's tests do -- twice: the expected outputs (both runs agree
                    bit for bit, or no comparison below would mean anything), the decoy's outputs, which must differ from
                    them in every compared array at one of the entry's B at least (or the scenario could not see a race on
                    that array; SAME_FOR_DECOY names the arrays that cannot differ), and the host time t_host of the enqueue.
  held pass         hold = min(500 ms, max(30 ms, 20 x t_host)), then
    late inputs       the device inputs hold the decoy; behind the hold the true inputs are copied into them on the stream,
                      then the call: it must see the true inputs
    early consumers   behind the call, on the stream, the outputs are copied away and then overwritten with the sentinel:
                      the copies must hold the results, so whatever the call ran on streams of its own is joined back
    host arrays       every HOST array of the call is overwritten with the decoy's values as soon as the call returns; once
                      with the arrays in pageable memory, once in page-locked memory (which a copy reads when it RUNS)
  six calls in flight with B = 1, 3, 65, 7, 130, 2 on a fresh handle: more calls than pinned slots, every buffer regrown
                    while earlier calls are queued
  the whole chain   eleven calls behind one hold with late inputs at the head, against the chain run call by call

All comparisons are bit for bit (a NaN equals a NaN).  A scenario that was not ENTERED under a live hold fails as vacuous.
An entry point whose header says that it enqueues "without a host synchronisation" must also RETURN while the hold is live
(gto_solve_batch_device is exempt: it throttles on the GPU's progress).  DESIGN.md 7r
holds the table of what was observed.  Nothing here provokes a fault: decoys are valid problems, pointers stay live
(held_stream.Scenario), holds end by themselves.  Run the file under a time limit (timeout -k 10 300 pytest ...)."""
import time

import numpy as np
import pytest

import held_stream as hs
import stream_order_cases as soc

pytestmark = pytest.mark.gpu

MODES = ("late", "early", "host", "host_pinned")  # host_pinned: the caller's host arrays live in page-locked memory
# Outputs that cannot tell the decoy from the true inputs, per entry: left out of "the decoy's outputs differ" by name (they
# are still compared with the idle pass).
#   iters, status of the solvers   max_iter = 3 ends every solve of the rig at the cap: 3 iterations and GTO_STATUS_MAX_ITER
#                                  for any valid input (the lift: for every step)
#   status of the retime calls     GTO_STATUS_CONVERGED for every finite plan that moves (the convex call's iters DO differ
#                                  with the inputs and are compared like every other output); the torque call's limits
#                                  lie above the Panda's own, so no path of the rig is INFEASIBLE
#   status, steps of the rollout   every path of the rig is followed to its end; steps = ceil((duration + settle) / dt) is one
#                                  of 4 .. 10 and may come out the same for a few paths
_SOLVER = ("iters", "status")
SAME_FOR_DECOY = {"solve": _SOLVER, "ik_pose": _SOLVER, "retrieve_lift": _SOLVER, "solve_base": _SOLVER, "retime_batch": ("status",),
                  "retime_paths": ("status",), "retime_paths_convex": ("status",), "retime_paths_torque": ("status",),
                  "track_rollout": ("status", "steps"), "chain": ("ik_iters", "ik_status", "iters", "status", "rt_status", "rp_status")}


def torch_dtype(dt):
    import torch
    return {np.dtype(np.float64): torch.float64, np.dtype(np.int32): torch.int32, np.dtype(np.uint8): torch.uint8}[np.dtype(dt)]


def cu(a):
    import torch
    return torch.from_numpy(np.array(a, order="C")).to("cuda:0")  # (a copy: the cases' arrays are read-only)


def same(a, b):
    """Bit for bit; a NaN equals a NaN (the payload of a NaN an operation makes is the processor's choice)."""
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    if a.dtype != b.dtype or a.shape != b.shape:
        return False
    if a.dtype == np.float64:
        return bool(((a.view(np.uint64) == b.view(np.uint64)) | (np.isnan(a) & np.isnan(b))).all())
    return bool((a == b).all())


def differing(want, got):
    return [k for k in want if not same(want[k], got[k])]


class Rig:
    def __init__(self, capi, oracle_mod):
        import torch
        from grasptrajopt_amd.observation import Observation
        from grasptrajopt_amd.occupancy import OccupancyGrid
        self.capi, self.oracle_mod = capi, oracle_mod
        self.desc, self.cfg = soc.robot()
        self._handles, self._fresh, self._override = {}, [], None
        depth, K, cam = soc.depth_observation()
        self.depth = Observation.from_depth(depth, K, cam, None, 1.5)
        self.cloud = Observation.from_cloud(*soc.cloud_observation(), soc.CLOUD_K)
        self.occ = OccupancyGrid.from_points(soc.occupancy_points(), margin=0.4, resolution=0.05, epsilon=0.05)
        self.stream = torch.cuda.Stream(device="cuda:0")
        self.idle_cache, self.observed, self.blind, self.dead = {}, {}, {}, False

    def _new(self, T, scenes):
        opts = self.oracle_mod.reference_opts(T=T, standoff_offset=soc.STANDOFF_OFFSET, max_iter=soc.MAX_ITER)
        h = self.capi.SolverHandle(self.desc, self.cfg["link_ee"], self.cfg["link_gripper"], opts, device=0)
        if scenes:
            for k, sc in enumerate(soc.scenes()):
                h.set_scene(k, sc.c_all, sc.c_obs, sc.shape, sc.origin, sc.res)
        return h

    def handle(self, T):
        if self._override is not None:
            return self._override
        if T not in self._handles:
            self._handles[T] = self._new(T, True)
        return self._handles[T]

    def fresh_handle(self):
        """A handle whose buffers have never grown (no scene: the entries of the regrowth runs need none)."""
        self._fresh.append(self._new(soc.T, False))
        return self._fresh[-1]

    def observation(self, entry):
        return self.depth if entry.endswith("depth") else self.cloud

    def obs_pointers(self, kinds):
        return np.array([(self.depth, self.cloud)[k]._ptr().value for k in kinds], dtype=np.int64)

    def close(self):
        import torch
        torch.cuda.synchronize()
        for h in list(self._handles.values()) + self._fresh:
            h.close()
        self.depth.close()
        self.cloud.close()
        self.occ.close()


@pytest.fixture(scope="module")
def rig(oracle_mod):
    import __graft_entry__ as g
    g.build()
    from grasptrajopt_amd import _capi
    r = Rig(_capi, oracle_mod)
    yield r
    r.close()
    rows = [f"{k[0]:>20} {k[1]:>6}  returned while held: {v[0]!s:>5}  t_host {1e3 * v[1]:7.3f} ms  hold {v[2]:5.0f} ms" for k, v in sorted(r.observed.items())]
    print("\nobserved (" + hs.method() + f", {hs.cycles_per_ms()} cycles per ms):\n" + "\n".join(rows))


@pytest.fixture(autouse=True)
def stop_after_a_gpu_error(rig):
    """After a HIP error nothing more is started on the GPU: the tests that follow fail without touching it."""
    import torch
    if rig.dead:
        pytest.fail("an earlier test of this file met a HIP error: nothing more runs on the GPU")
    yield
    try:
        torch.cuda.synchronize()
    except Exception:
        rig.dead = True
        raise


class Buffers:
    """The caller's side of one call: device inputs, host arrays of its own, outputs filled with the sentinel."""

    def __init__(self, rig, sc, case, dev_from=None, pinned=False):
        import torch
        src = case if dev_from is None else dev_from
        self.dev = {k: sc.keep(cu(v)) for k, v in src.dev.items()}
        self.host = self.host_arrays(rig, case)
        if pinned:  # the caller's host arrays in page-locked memory: a copy straight from them is a DMA that reads them LATE
            self.host = {k: sc.keep(torch.from_numpy(v).pin_memory()).numpy() for k, v in self.host.items()}
        self.out = {k: sc.keep(torch.full(s, soc.SENTINEL[t], dtype=torch_dtype(t), device="cuda:0")) for k, (s, t) in case.outs.items()}
        self.d = {k: v.data_ptr() for k, v in self.dev.items()}
        self.o = {k: v.data_ptr() for k, v in self.out.items()}

    @staticmethod
    def host_arrays(rig, case):
        return {k: (rig.obs_pointers(v) if k == "obs" else v.copy()) for k, v in case.host.items()}

    def scribble(self, rig, decoy):
        for k, v in self.host_arrays(rig, decoy).items():
            self.host[k][...] = v

    def results(self, outs=None):
        return {k: v.cpu().numpy() for k, v in (self.out if outs is None else outs).items()}


def call_of(entry):
    if entry == "chain":
        return lambda rig, case, buf, stream: soc.enqueue_chain(rig, case, buf.d, buf.host, buf.o, stream)
    return lambda rig, case, buf, stream: soc.enqueue(rig, entry, case, buf.d, buf.host, buf.o, stream)


def case_of(entry, B, decoy=False):
    return soc.chain_inputs(decoy) if entry == "chain" else soc.inputs(entry, B, decoy=decoy)


def idle(rig, entry, B, tag=""):
    """(expected outputs, t_host) of the call on an idle device, the second of two runs; asserts that the two runs agree and
    that the decoy's outputs differ from them in every compared array."""
    import torch
    key = (entry, B, tag)
    if key not in rig.idle_cache:
        runs = []
        for decoy in (False, False, True):
            case = case_of(entry, B, decoy)
            with hs.Scenario() as sc:
                buf = Buffers(rig, sc, case)
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                call_of(entry)(rig, case, buf, rig.stream.cuda_stream)
                t_host = time.perf_counter() - t0
                rig.stream.synchronize()
                runs.append((buf.results(), t_host))
        (first, _), (want, t_host), (other, _) = runs
        assert differing(first, want) == [], f"{entry}, B = {B}: two idle runs disagree: nothing can be compared bit for bit"
        untouched = [k for k, v in want.items() if (v == soc.SENTINEL[v.dtype]).all()]
        assert untouched == [], f"{entry}, B = {B}: the call wrote nothing into {untouched}"
        rig.blind.setdefault((entry, tag), {})[B] = {k for k in want if same(want[k], other[k])}
        rig.idle_cache[key] = (want, t_host)
    return rig.idle_cache[key]


def assert_not_blind(rig, entry, tag=""):
    """Every compared array of `entry` differs between the true inputs and the decoy at one of the B that were run, at least:
    the scenario over these B can see a race on it.  (Per B a count or a flag of a few items may come out the same by chance:
    n_accepted of one goal set is 1, 2 or 3.)"""
    per_B = rig.blind[(entry, tag)]
    never = sorted(set.intersection(*per_B.values()) - set(SAME_FOR_DECOY.get(entry, ())))
    assert never == [], (f"{entry}: the decoy gives the true inputs' {never} at every B of {sorted(per_B)}: a race on them could not be "
                         f"seen (per B: { {B: sorted(v) for B, v in per_B.items()} })")


def held(rig, entry, B, mode, tag="", pinned=False):
    """One held pass; returns (entered under the hold, returned under the hold, the arrays that differ from the idle pass)."""
    import torch
    want, t_host = idle(rig, entry, B, tag)
    true, decoy = case_of(entry, B), case_of(entry, B, True)
    ms = hs.hold_ms(t_host)
    with hs.Scenario() as sc:
        buf = Buffers(rig, sc, true, dev_from=decoy if mode == "late" else None, pinned=pinned)
        src = {k: sc.keep(cu(v)) for k, v in true.dev.items()} if mode == "late" else {}
        copies = {k: sc.keep(torch.full_like(v, soc.SENTINEL[true.outs[k][1]])) for k, v in buf.out.items()} if mode == "early" else None
        torch.cuda.synchronize()
        event = hs.hold(rig.stream, ms)
        with torch.cuda.stream(rig.stream):
            for k, v in src.items():
                buf.dev[k].copy_(v, non_blocking=True)
        entered = hs.still_held(event)
        call_of(entry)(rig, true, buf, rig.stream.cuda_stream)
        returned = hs.still_held(event)
        if mode == "host":
            buf.scribble(rig, decoy)
        if mode == "early":
            with torch.cuda.stream(rig.stream):
                for k, v in buf.out.items():
                    copies[k].copy_(v, non_blocking=True)
                    v.fill_(soc.SENTINEL[true.outs[k][1]])
        rig.stream.synchronize()
        got = buf.results(copies)
    rig.observed[(entry + tag, mode + ("_pinned" if pinned else ""))] = (returned, t_host, ms)
    return entered, returned, differing(want, got)


def judge(entry, B, mode, entered, returned, wrong, no_host_sync):
    assert entered, (f"{entry}, B = {B}, {mode}: the hold had ended before the call was entered: the scenario was vacuous "
                     "(nothing was tested; a longer hold or a shorter sequence is needed)")
    assert wrong == [], f"{entry}, B = {B}, {mode}: {wrong} differ from the idle pass: the call is not ordered on its stream"
    if no_host_sync:
        assert returned, (f"{entry}, B = {B}, {mode}: the call returned only after the hold had ended: it waits for the stream, "
                          "although its header says that it enqueues without a host synchronisation")


# ---------------------------------------------------------------------------------------------- 0. the hold itself
def test_a_hold_holds_its_stream_and_ends_by_itself(rig):
    import torch
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    event = hs.hold(rig.stream, 30.0)
    assert hs.still_held(event), "a hold of 30 ms had ended when hold() returned: the calibration is off"
    event.synchronize()
    took = 1e3 * (time.perf_counter() - t0)
    print(f"a hold of 30 ms took {took:.1f} ms ({hs.method()}, {hs.cycles_per_ms()} cycles per ms)")
    assert 15.0 <= took <= 2.0 * hs.MAX_HOLD_MS
    assert hs.hold_ms(0.0) == 30.0 and hs.hold_ms(0.004) == 80.0 and hs.hold_ms(10.0) == hs.MAX_HOLD_MS


# ---------------------------------------------------------------------------------------------- 1. one call behind a hold
@pytest.mark.parametrize("entry,mode", [(e, m) for e in soc.ENTRIES if e != "solve" for m in MODES
                                        if not m.startswith("host") or soc.inputs(e, 1).host])  # (host: the entries that take a HOST array)
def test_a_call_behind_a_busy_stream(rig, entry, mode):
    mode, pinned = mode.split("_")[0], mode.endswith("_pinned")
    for B in ((4,) if entry == "filter_grasps" else soc.BS):
        judge(entry, B, mode, *held(rig, entry, B, mode, pinned=pinned), no_host_sync=entry in soc.NO_HOST_SYNC)
    assert_not_blind(rig, entry)


@pytest.mark.parametrize("mode", ("late", "early"))
@pytest.mark.parametrize("lanes", [(1, 1, 0), (4, 1, 2)], ids=["one_lane", "four_lanes_handed_over"])
def test_a_solve_behind_a_busy_stream(rig, lanes, mode):
    """With (4, 1, 2) and B = 5 the lanes run on streams of their own, forked from and joined to the caller's by events, and
    lanes that are left with at most two instances hand them to lane 0 and are skipped at the join."""
    h = rig.handle(soc.T)
    h.set_lanes(*lanes)
    try:
        for B in soc.BS:
            judge("solve", B, mode, *held(rig, "solve", B, mode, tag=f"_lanes{lanes[0]}"), no_host_sync=False)
        assert_not_blind(rig, "solve", f"_lanes{lanes[0]}")
    finally:
        h.set_lanes(1, 256, 0)


# ---------------------------------------------------------------------------------------------- 2. six calls in flight
@pytest.mark.parametrize("memory", ["pageable", "pinned"])
@pytest.mark.parametrize("run", list(soc.REGROW_RUNS))
def test_more_calls_in_flight_than_pinned_slots_with_regrowth(rig, run, memory):
    """Six calls (twelve for the base pair, eighteen for the three retime calls, whose greedy, convex and torque calls take
    turns on the rt_* workspace they share, of which k_retime_convex rewrites rt_P1 / rt_P2 in place and to which the torque
    call adds rt_TA / rt_TB / rt_TG: the torque call at B = 65 is still queued when the greedy call at B = 130 regrows the
    workspace) of one fresh handle on one stream behind
    a hold, each with host arrays and outputs
    of its own, the host arrays overwritten as soon as their call returns.  Past four calls the pinned ring is reused, which is
    safe only behind the slot's event; B = 65 and 130 regrow bs_ng / ck_base / the held, filter and retime workspaces by free and
    allocate while earlier calls are queued, which is safe only because hipFree waits for the device (so does the first retime
    call of a handle, which uploads its factor table).  That wait also ends
    the hold, so the stream is held again in front of the next call: every call is entered under a live hold."""
    import torch
    seq = [(e, B) for B in soc.REGROW_BS for e in soc.REGROW_RUNS[run]]
    rig._override = rig.fresh_handle()
    try:
        want, t_host = [], 0.0
        for e, B in seq:  # the idle pass: the same sequence on a handle of its own, a synchronise around every call
            case = soc.inputs(e, B)
            with hs.Scenario() as sc:
                buf = Buffers(rig, sc, case)
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                soc.enqueue(rig, e, case, buf.d, buf.host, buf.o, rig.stream.cuda_stream)
                t_host += time.perf_counter() - t0
                rig.stream.synchronize()
                want.append(buf.results())
        ms = hs.hold_ms(t_host)
        rig._override = rig.fresh_handle()
        with hs.Scenario() as sc:
            bufs = [Buffers(rig, sc, soc.inputs(e, B), pinned=memory == "pinned") for e, B in seq]
            torch.cuda.synchronize()
            event, holds, entered = hs.hold(rig.stream, ms), 1, []
            for (e, B), buf in zip(seq, bufs):
                if not hs.still_held(event):
                    event, holds = hs.hold(rig.stream, ms), holds + 1
                entered.append(hs.still_held(event))
                soc.enqueue(rig, e, soc.inputs(e, B), buf.d, buf.host, buf.o, rig.stream.cuda_stream)
                buf.scribble(rig, soc.inputs(e, B, decoy=True))
            rig.stream.synchronize()
            got = [buf.results() for buf in bufs]
    finally:
        rig._override = None
    print(f"{run}: {len(seq)} calls, t_host {1e3 * t_host:.2f} ms, hold {ms:.0f} ms, held {holds} times")
    rig.observed[("six_calls_" + run, "host" + ("_pinned" if memory == "pinned" else ""))] = (holds == 1, t_host, ms)
    assert all(entered), f"{run}: calls {[i for i, x in enumerate(entered) if not x]} were entered after their hold had ended: vacuous"
    wrong = [(e, B, differing(w, g)) for (e, B), w, g in zip(seq, want, got) if differing(w, g)]
    assert wrong == [], f"{run}: calls whose outputs differ from their idle pass: {wrong}"


# ---------------------------------------------------------------------------------------------- 3. the whole chain
def test_the_whole_chain_behind_a_hold(rig):
    """From grasp poses to the retimed retrieve path: eleven calls on one stream with late inputs at the head and ONE
    synchronise at the end, against the same chain with a device synchronise after every call."""
    import torch
    true, decoy = soc.chain_inputs(), soc.chain_inputs(True)
    passes = []
    for case in (true, true, decoy):  # (the first run also pays the handle's first retime call, which synchronises)
        with hs.Scenario() as sc:
            buf = Buffers(rig, sc, case)
            torch.cuda.synchronize()
            soc.enqueue_chain(rig, case, buf.d, buf.host, buf.o, rig.stream.cuda_stream, between=lambda step: torch.cuda.synchronize())
            passes.append(buf.results())
    first, want, other = passes
    assert differing(first, want) == [], "two call-by-call runs of the chain disagree"
    blind = [k for k in want if same(want[k], other[k]) and k not in SAME_FOR_DECOY.get("chain", ())]
    assert blind == [], f"the decoy gives the true inputs' {blind}: a race on them could not be seen"
    with hs.Scenario() as sc:  # t_host of the chain without synchronises in between
        buf = Buffers(rig, sc, true)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        soc.enqueue_chain(rig, true, buf.d, buf.host, buf.o, rig.stream.cuda_stream)
        t_host = time.perf_counter() - t0
        rig.stream.synchronize()
        assert differing(want, buf.results()) == [], "the chain with one synchronise at its end, on an idle device"
    rig.idle_cache[("chain", soc.CHAIN_B, "")] = (want, t_host)
    entered, returned, wrong = held(rig, "chain", soc.CHAIN_B, "late")
    judge("chain", soc.CHAIN_B, "late", entered, returned, wrong, no_host_sync=False)  # (it contains gto_solve_batch_device)
