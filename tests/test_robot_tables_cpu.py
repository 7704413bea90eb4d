"""CPU: the robot tables gto_create uploads (csrc/gto_robot.h), built by a stand-alone host program under AddressSanitizer
and UBSan (tests/robot_tables_main.cpp): no HIP, nothing loaded into this process.

Every descriptor is written as the bytes the library would see (the counts, then the arrays _capi.pack_robot_desc keeps
alive, in struct order).  The program refuses or accepts it, holds the accepted tables to their invariants and prints a
digest of each.  Asserted here: status 0 and no sanitizer report for every run, the code and message of every refusal, one
refused descriptor per message the header can give, and equal output from two runs.  No digest is kept in the repository:
the origins go through the host's sin and cos."""
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import ROOT
from helpers import cfg_of, limit_robot, random_robot

CSRC = os.path.join(ROOT, "grasptrajopt_amd", "csrc")
SCALARS = ("n_frames", "ndof", "n_opt", "n_links", "n_points", "frame_ee", "frame_gripper", "n_gripper_points")
ARRAYS = ("parent", "joint_type", "q_index", "origin_xyz", "origin_rpy", "axis", "opt_index", "lower", "upper", "link_frame",
          "visual_xyz", "visual_rpy", "points", "point_link", "gripper_points")
PB_MERGE = (1, 4, 7)
CHUNK_EDGES = [1, 65, [1, 65, 64, 63, 129, 2, 128, 300] * 4]   # tests/test_limits_cpu.py
TOO_MANY = "too many surface points (max 16384, in at most 256 runs of up to 64 points of one link)"


def packed(desc, ee, gripper, ngp=None):
    """The descriptor's fields by name: the struct's counts, and copies of the arrays it points to."""
    from grasptrajopt_amd import _capi
    c, keep = _capi.pack_robot_desc(desc, ee, gripper, ngp)
    assert len(keep) == len(ARRAYS)
    f = {k: int(getattr(c, k)) for k in SCALARS}
    f.update({k: a.copy() for k, a in zip(ARRAYS, keep)})
    return f


def write(path, f):
    with open(path, "wb") as fh:
        fh.write(np.array([f[k] for k in SCALARS], dtype="<i4").tobytes())
        for k in ARRAYS:
            fh.write(np.ascontiguousarray(f[k], dtype="<i4" if f[k].dtype.kind == "i" else "<f8").tobytes())


def edited(f, **kw):
    """A copy of the fields with some replaced; name=(index, value) sets one element of an array."""
    g = {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in f.items()}
    for k, v in kw.items():
        if isinstance(v, tuple):
            g[k][v[0]] = v[1]
        else:
            g[k] = v
    return g


def grown(a, row):
    return np.concatenate([a, np.asarray([row], dtype=a.dtype).reshape((1,) + a.shape[1:])])


def accepted_corpus():
    from grasptrajopt_amd.robot_desc import load_builtin
    import renumbered_robots as rr
    import small_robots as sr
    out = {}
    for name in ("panda", "fetch", "panda_5k"):
        cfg = cfg_of(name)
        out[name] = packed(load_builtin(name), cfg["link_ee"], cfg["link_gripper"])
    order = np.random.default_rng(0).permutation(out["panda"]["n_points"])   # every other robot lists its points link by link
    out["panda_shuffled"] = edited(out["panda"], points=out["panda"]["points"][order], point_link=out["panda"]["point_link"][order])
    for kind in sr.KINDS:
        r = sr.Robot(kind)
        out[f"small_{kind}"] = packed(r.desc, r.ee, r.gripper, r.n_gripper_points)
    for kind in ("chain", "bushy", "forked"):
        for n_opt in (1, 8, 9, 16):
            d, ee = limit_robot(kind, n_opt=n_opt, points_per_link=64, seed=n_opt)
            out[f"limit_{kind}_{n_opt}"] = packed(d, ee, ee)
        for n_opt in (8, 16):
            for k, ppl in enumerate(CHUNK_EDGES + [512]):
                d, ee = limit_robot(kind, n_opt=n_opt, points_per_link=ppl)
                out[f"limit_{kind}_{n_opt}_{'edges%d' % k if k < 3 else 'full'}"] = packed(d, ee, ee)
    for name, (robot, _, _, pi) in rr.CASES.items():
        if robot == "panda":
            cfg = cfg_of("panda")
            d, ee, gripper, ngp = load_builtin("panda"), cfg["link_ee"], cfg["link_gripper"], None
        else:
            d, ee = random_robot(*robot)
            gripper, ngp = ee, 40
        out[f"renumbered_{name}_original"] = packed(d, ee, gripper, ngp)
        for variant in rr.VARIANTS:
            out[f"renumbered_{name}_{variant}"] = packed(rr.renumber(d, pi, variant == "sorted"), ee, gripper, ngp)
    return out


def refused_corpus(ok):
    """name -> (fields, code, message): one-field edits of accepted robots (an array grows with the count that is edited)."""
    panda, chain, chain16 = ok["panda"], ok["limit_chain_8"], ok["limit_chain_16"]
    act = int(np.flatnonzero(panda["joint_type"] != 0)[0])   # a frame with an actuated joint
    spare = [j for j in range(chain16["ndof"]) if j not in chain16["opt_index"].tolist()][0]
    out = {
        # tests/test_capi_cpu.py::test_create_validates_and_has_no_cpu_fallback
        "parent_after_child": (edited(panda, parent=(1, 2)), -1, "frames must list parents before children"),
        "two_links_one_frame": (edited(panda, link_frame=(1, panda["link_frame"][0])), -1, "two collision links on one frame"),
        "point_link_range": (edited(panda, point_link=(0, panda["n_links"])), -1, "point_link out of range"),
        "lower_above_upper": (edited(panda, lower=(0, panda["upper"][0] + 1.0)), -1, "lower > upper"),
        # the refusals no other test reaches
        "opt_index_range": (edited(panda, opt_index=(0, panda["ndof"])), -1, "opt_index out of range"),
        "opt_index_negative": (edited(panda, opt_index=(0, -1)), -1, "opt_index out of range"),
        "opt_index_twice": (edited(panda, opt_index=(1, panda["opt_index"][0])), -1, "opt_index names a joint twice"),
        "joint_type": (edited(panda, joint_type=(act, 3)), -4, "joint type not supported (optas/models.py:865-866)"),
        "q_index_range": (edited(panda, q_index=(act, panda["ndof"])), -1, "q_index out of range for an actuated joint"),
        "zero_axis": (edited(panda, axis=(act, 0.0)), -1, "zero joint axis"),
        "link_frame_range": (edited(panda, link_frame=(0, panda["n_frames"])), -1, "link_frame out of range"),
        "link_frame_negative": (edited(panda, link_frame=(0, -1)), -1, "link_frame out of range"),
        # one past each count (tests/test_limits_cpu.py)
        "33_frames": (edited(chain, n_frames=33, parent=grown(chain["parent"], 31), joint_type=grown(chain["joint_type"], 0),
                             q_index=grown(chain["q_index"], -1), origin_xyz=grown(chain["origin_xyz"], [0, 0, 0.05]),
                             origin_rpy=grown(chain["origin_rpy"], [0, 0, 0]), axis=grown(chain["axis"], [0, 0, 1.0])),
                      -4, "n_frames out of range (max 32)"),
        "33_links": (edited(chain, n_links=33, link_frame=grown(chain["link_frame"], 0), visual_xyz=grown(chain["visual_xyz"], [0, 0, 0]),
                            visual_rpy=grown(chain["visual_rpy"], [0, 0, 0])), -4, "n_links out of range (max 32)"),
        "17_opt": (edited(chain16, n_opt=17, opt_index=grown(chain16["opt_index"], spare), lower=grown(chain16["lower"], -1.0),
                          upper=grown(chain16["upper"], 1.0)), -4, "n_opt out of range (max 16)"),
        "ndof_33": (edited(chain, ndof=33), -4, "ndof out of range (max 32)"),
        "ndof_below_n_opt": (edited(chain, ndof=chain["n_opt"] - 1), -4, "ndof out of range (max 32)"),
        "no_points": (edited(panda, n_points=0, points=panda["points"][:0], point_link=panda["point_link"][:0]), -1,
                      "robot has no surface points"),
        "no_gripper_points": (edited(panda, n_gripper_points=0, gripper_points=panda["gripper_points"][:0]), -1,
                              "robot has no gripper points"),
        "frame_ee_range": (edited(panda, frame_ee=panda["n_frames"]), -1, "frame_ee / frame_gripper out of range"),
        "frame_gripper_negative": (edited(panda, frame_gripper=-1), -1, "frame_ee / frame_gripper out of range"),
    }
    for k, ppl in enumerate(([512] * 31 + [513], [513] * 31 + [1])):   # 16385 points, and 279 runs in fewer than 16384
        d, ee = limit_robot("chain", n_opt=8, points_per_link=ppl)
        out[f"too_many_{k}"] = (packed(d, ee, ee), -4, TOO_MANY)
    return out


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    """pb_merge -> the program's output lines by descriptor name, from two runs that had to agree."""
    tmp = tmp_path_factory.mktemp("robot_tables")
    exe = tmp / "robot_tables"
    subprocess.check_call(["g++", "-std=c++17", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include", "-Wno-unknown-pragmas",
                           "-I", CSRC, os.path.join(ROOT, "tests", "robot_tables_main.cpp"), "-o", str(exe)])
    ok = accepted_corpus()
    bad = refused_corpus(ok)
    files = []
    for name, f in list(ok.items()) + [(k, v[0]) for k, v in bad.items()]:
        files.append(str(tmp / name))
        write(files[-1], f)
    out = {}
    for m in PB_MERGE:
        texts = []
        for _ in range(2):
            res = subprocess.run([str(exe), str(m)] + files, capture_output=True, text=True, timeout=300)
            assert res.returncode == 0 and res.stderr == "", res.stdout[-2000:] + res.stderr[-4000:]
            texts.append(res.stdout)
        assert texts[0] == texts[1]   # the same digests from the same input
        lines = dict(line.split(" ", 1) for line in texts[0].splitlines())
        assert list(lines) == list(ok) + list(bad)
        out[m] = lines
    return dict(out=out, ok=ok, bad=bad)


ACCEPTED = re.compile(r"rc=0 n_chunks=(\d+) pb_C=(\d+) n_cframes=(\d+) n_xst=(\d+) fk_rounds=(\d+) fk_rounds_c=(\d+)"
                      r"( (rb|px|py|pz|plink|perm|chunks|pbchunks)=[0-9a-f]{16}){8} why=$")


def test_accepted_descriptors_pass_their_invariants_under_the_sanitizers(runs):
    """The program has checked each table's invariants (it leaves with status 1 otherwise); the counts it prints are the
    ones the descriptor gives without any table."""
    for m in PB_MERGE:
        for name, f in runs["ok"].items():
            got = ACCEPTED.match(runs["out"][m][name])
            assert got, (m, name, runs["out"][m][name])
            n_chunks, pb_C, n_cframes, n_xst = (int(x) for x in got.groups()[:4])
            per_link = np.bincount(f["point_link"], minlength=f["n_links"])
            assert n_chunks == int((-(-per_link // 64)).sum()), (m, name)
            assert pb_C <= n_chunks and (m > 1 or pb_C == n_chunks - _static_chunks(f)), (m, name)
            assert n_cframes <= f["n_frames"] and n_xst <= f["n_frames"]
    for name in runs["ok"]:   # pb_merge changes the merged spheres and nothing else
        rest = [re.sub(r" pb_C=\d+| pbchunks=\w+", "", runs["out"][m][name]) for m in PB_MERGE]
        assert rest[0] == rest[1] == rest[2], name


def _static_chunks(f):
    """Chunks of the links that no optimised joint moves."""
    opt = set(f["opt_index"].tolist())
    moved = np.zeros(f["n_frames"], dtype=bool)
    for i in range(f["n_frames"]):
        p = f["parent"][i]
        moved[i] = (p >= 0 and moved[p]) or (f["joint_type"][i] != 0 and int(f["q_index"][i]) in opt)
    per_link = np.bincount(f["point_link"], minlength=f["n_links"])
    return int((-(-per_link // 64))[~moved[f["link_frame"]]].sum())


def test_refused_descriptors_get_their_code_and_message(runs):
    for m in PB_MERGE:
        for name, (_, code, why) in runs["bad"].items():
            assert runs["out"][m][name] == f"rc={code} why={why}", (m, name)


def test_every_refusal_of_the_header_has_a_descriptor(runs):
    src = open(os.path.join(CSRC, "gto_robot.h")).read()
    messages = set(re.findall(r'bad\(GTO_\w+, "([^"]+)"\)', src)) | set(re.findall(r'why = "([^"]+)"', src))
    assert len(messages) == 18 and messages == {why for _, _, why in runs["bad"].values()}
