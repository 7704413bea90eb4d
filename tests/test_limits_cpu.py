"""CPU: gto_create accepts every robot within the capacity include/gto_solver.h advertises, at every T up to 96, and
refuses one past each limit with that limit's own message.

gto_create validates the descriptor, builds its tables and sizes every kernel's LDS before it looks for a device: without
a GPU an accepted robot ends in GTO_ERR_NO_DEVICE (-3), a refused one in GTO_ERR_UNSUPPORTED (-4) or GTO_ERR_INVALID_ARG
(-1).  With a GPU the accepted robots are created and closed."""
import copy
import re

import numpy as np
import pytest

from helpers import limit_robot


@pytest.fixture(scope="module")
def capi():
    import __graft_entry__ as g
    g.build()
    from grasptrajopt_amd import _capi
    return _capi


def _create(capi, desc, ee, T=50, off=-10):
    """'accepted' or the error text of gto_create."""
    opts = capi.default_opts()
    opts.T, opts.standoff_offset = T, off
    try:
        h = capi.SolverHandle(desc, ee, ee, opts, device=0)
    except capi.GTOError as e:
        if "(-3): no HIP device" in str(e):
            return "accepted"
        return str(e)
    h.close()
    return "accepted"


@pytest.mark.parametrize("kind", ["chain", "bushy", "forked"])
@pytest.mark.parametrize("ppl", [64, 512])
def test_every_n_opt_is_accepted_at_32_frames_and_32_links(capi, kind, ppl):
    """1 to 16 optimised joints on 32 frames and 32 collision links, with 64 points per link (2048) and with 512 (the 16384
    maximum): the 8-wide robots (n_opt <= 8) were refused with 26 or more such links ("robot too large for the obstacle
    kernel's LDS") while the same trees with nine optimised joints were created."""
    for n_opt in range(1, 17):
        desc, ee = limit_robot(kind, n_opt=n_opt, points_per_link=ppl, seed=n_opt)
        assert (desc.n_frames, desc.n_links, desc.n_opt, desc.n_points) == (32, 32, n_opt, 32 * ppl)
        for T, off in ((4, -1), (50, -10), (96, -10)):
            assert _create(capi, desc, ee, T, off) == "accepted", (kind, ppl, n_opt, T)


@pytest.mark.parametrize("n_links", [24, 26, 28, 32])
@pytest.mark.parametrize("n_opt", [1, 7, 8, 9, 16])
def test_links_of_the_issue_probe_are_accepted(capi, n_links, n_opt):
    """The serial chain of 32 frames with a link of 64 points on each of its last L frames, and 28 frames with 28 links."""
    desc, ee = limit_robot("chain", n_links=n_links, n_opt=n_opt)
    assert _create(capi, desc, ee, 96, -10) == "accepted"
    desc, ee = limit_robot("chain", n_frames=28, n_links=28, n_opt=n_opt)
    assert _create(capi, desc, ee, 96, -10) == "accepted"


@pytest.mark.parametrize("ppl", [1, 65, [1, 65, 64, 63, 129, 2, 128, 300] * 4])
def test_point_counts_at_chunk_edges_are_accepted(capi, ppl):
    for kind, n_opt in (("chain", 8), ("bushy", 16)):
        desc, ee = limit_robot(kind, n_opt=n_opt, points_per_link=ppl)
        assert _create(capi, desc, ee, 96, -10) == "accepted"


def _edit(desc, **kw):
    d = copy.deepcopy(desc)
    for k, v in kw.items():
        setattr(d, k, v)
    return d


def test_one_past_each_limit_is_refused_with_its_own_message(capi):
    desc, ee = limit_robot("chain", n_opt=8)
    assert _create(capi, desc, ee) == "accepted"
    msg = lambda code, text: rf"^gto_create failed \({code}\): {re.escape(text)}$"
    # 33 frames (a 33rd frame, fixed, under the end effector)
    d = _edit(desc, frame_names=desc.frame_names + ["f32"], parent=np.append(desc.parent, 31).astype(np.int32),
              joint_type=np.append(desc.joint_type, 0).astype(np.int32), q_index=np.append(desc.q_index, -1).astype(np.int32),
              origin_xyz=np.vstack([desc.origin_xyz, [0, 0, 0.05]]), origin_rpy=np.vstack([desc.origin_rpy, np.zeros(3)]),
              axis=np.vstack([desc.axis, [0, 0, 1.0]]))
    assert re.match(msg(-4, "n_frames out of range (max 32)"), _create(capi, d, ee))
    # 33 collision links on 32 frames is refused for the count, before any frame is looked at twice
    d = _edit(desc, link_names=desc.link_names + ["extra"], link_frame=np.append(desc.link_frame, 0).astype(np.int32),
              visual_xyz=np.vstack([desc.visual_xyz, np.zeros(3)]), visual_rpy=np.vstack([desc.visual_rpy, np.zeros(3)]))
    assert re.match(msg(-4, "n_links out of range (max 32)"), _create(capi, d, ee))
    # 17 optimised joints (of the chain's 31)
    d17, _ = limit_robot("chain", n_opt=16)
    extra = [k for k in d17.param_index.tolist()][0]
    d = _edit(d17, opt_index=np.array(sorted(d17.opt_index.tolist() + [extra]), dtype=np.int32),
              param_index=d17.param_index[1:].astype(np.int32))
    assert re.match(msg(-4, "n_opt out of range (max 16)"), _create(capi, d, ee))
    # 33 actuated joints (a 33rd joint value no frame reads)
    d = _edit(desc, actuated_joint_names=desc.actuated_joint_names + ["j31", "j32"], lower=np.append(desc.lower, [-1, -1]),
              upper=np.append(desc.upper, [1, 1]), param_index=np.append(desc.param_index, [31, 32]).astype(np.int32))
    assert d.ndof == 33
    assert re.match(msg(-4, "ndof out of range (max 32)"), _create(capi, d, ee))
    d = _edit(d, actuated_joint_names=d.actuated_joint_names[:32], lower=d.lower[:32], upper=d.upper[:32],
              param_index=d.param_index[:-1])
    assert d.ndof == 32 and _create(capi, d, ee) == "accepted"
    # 16385 surface points (one link of 513), and 279 runs of 64 in fewer than 16384 points
    too_many = "too many surface points (max 16384, in at most 256 runs of up to 64 points of one link)"
    for ppl in ([512] * 31 + [513], [513] * 31 + [1]):
        d, _ = limit_robot("chain", n_opt=8, points_per_link=ppl)
        assert re.match(msg(-4, too_many), _create(capi, d, ee)), (sum(ppl), _create(capi, d, ee))
    d, _ = limit_robot("chain", n_opt=8, points_per_link=[512] * 31 + [511])
    assert _create(capi, d, ee) == "accepted"
    # T = 97
    assert re.match(msg(-1, "T must be <= 96 (GTO_MAX_T)"), _create(capi, desc, ee, 97, -10))
