"""The ordering of the inner iterations (slam-tricks_amd/csrc/inner_plan.hpp, what stba_ba_set_inner_iterations runs) without a
device: tests/cpp/inner_plan_driver.cpp, compiled with g++, reads one case and prints the plan or the refusal.

Expected plans come from inner_iterations_ref.ordering_lists -- the reference's ordering() flattened, with the mask rule of its
sweep() -- and are compared exactly.  The refusals are compared in full against the sentences stba_ba_set_inner_iterations has
always produced behind its own name (tests/ba_refusal_cases.py, test_gpu_inner_iterations.py assert them on the device); a
dependent group names the first offending observation in the order the observations are given.  Every deliberate mistake of
inner_iterations_ref.ORDERING_MUTATIONS makes the reference disagree with the driver on some case: the cases can tell them apart.
The driver is also built with the address + undefined-behaviour sanitizers and must run without a report and print the same."""
import os
import re
import subprocess
from types import SimpleNamespace

import numpy as np
import pytest

import inner_iterations_ref as I

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "slam-tricks_amd", "csrc", "inner_plan.hpp")
SANITIZERS = {"plain": [], "asan_ubsan": ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-g"]}

# three cameras, four landmarks, nine observations (camera, landmark); every camera sees three landmarks
OBS = [(0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (1, 3), (2, 0), (2, 3), (2, 2)]
ALL6 = 63


def case(nc=3, npt=4, obs=OBS, cam_fixed=None, pt_fixed=None, rot=None, pos=None, pt=None, error=None):
    """cam_fixed: per camera the mask of constant dofs (bit a = dof a), pt_fixed: per landmark 0 / 1; None: a null pointer"""
    assert 2 <= nc <= 4 and 3 <= npt <= 6 and len(obs) <= 12
    return dict(nc=nc, np=npt, obs=obs, cam_fixed=cam_fixed, pt_fixed=pt_fixed, rot=rot, pos=pos, pt=pt, error=error)


CASES = {
    "default_nothing_constant": case(),
    "default_constant_camera_and_landmark": case(cam_fixed=[0, ALL6, 0], pt_fixed=[0, 0, 1, 0]),
    "three_groups": case(rot=[0, 0, 0], pos=[1, 1, 1], pt=[2, 2, 2, 2]),
    "rotation_and_position_share_an_id": case(rot=[0, 0, 0], pos=[0, 0, 0], pt=[1, 1, 1, 1]),
    "landmarks_in_the_lowest_id": case(rot=[1, 1, 1], pos=[2, 2, 2], pt=[0, 0, 0, 0]),
    "only_pt_group": case(pt=[0, 0, 1, 1]),
    "ids_9_2_5": case(rot=[9, 9, 9], pos=[2, 2, 2], pt=[5, 5, 5, 5]),
    "minus_one_mixed_in": case(rot=[0, -1, 0], pos=[-1, 1, 1], pt=[2, -1, 2, 3]),
    "one_constant_rotation_dof": case(cam_fixed=[2, 0, 0], rot=[0, 0, 0], pos=[1, 1, 1], pt=[2, 2, 2, 2]),
    # camera 1's rotation shares id 0 with the landmarks it observes, but all of it is constant: ignored, the group is independent
    "constant_rotation_is_ignored": case(cam_fixed=[0, 7, 0], pt_fixed=[0, 0, 0, 0], rot=[-1, 0, -1], pos=[1, 1, 1], pt=[0, 0, 0, 0]),
    "camera_without_observation": case(nc=4, rot=[0, 0, 0, 0], pos=[1, 1, 1, 1], pt=[2, 2, 2, 2]),
    "camera_without_observation_default": case(nc=4),
    "everything_constant": case(cam_fixed=[ALL6] * 3, pt_fixed=[1] * 4, rot=[0, 0, 0], pos=[1, 1, 1], pt=[2, 2, 2, 2]),
    "everything_constant_default": case(cam_fixed=[ALL6] * 3, pt_fixed=[1] * 4),
    # ---- the refusals
    "camera_id_minus_2": case(rot=[0, -2, 0], pos=[0, 0, 0], pt=[1, 1, 1, 1], error="camera 1: a group id below -1"),
    "camera_position_id_minus_2": case(pos=[0, 0, -2], error="camera 2: a group id below -1"),
    "landmark_id_minus_2": case(rot=[0, 0, 0], pos=[0, 0, 0], pt=[1, 1, 1, -2], error="landmark 3: a group id below -1"),
    # landmark 3 shares id 0 with every rotation: the first observation of it in the order given is (1, 3) ...
    "dependent_group": case(rot=[0, 0, 0], pt=[1, 1, 1, 0],
                            error="group 0 is not an independent set: camera 1 and landmark 3 share a residual"),
    # ... and, with the same observations the other way round, (2, 3)
    "dependent_group_reversed_observations": case(obs=OBS[::-1], rot=[0, 0, 0], pt=[1, 1, 1, 0],
                                                  error="group 0 is not an independent set: camera 2 and landmark 3 share a residual"),
    "dependent_group_by_position": case(pos=[4, 4, 4], pt=[4, -1, -1, -1],
                                        error="group 4 is not an independent set: camera 0 and landmark 0 share a residual"),
}
PLANS = sorted(k for k, c in CASES.items() if c["error"] is None)
REFUSALS = sorted(k for k, c in CASES.items() if c["error"] is not None)


def stdin_of(c):
    opt = lambda v: "0" if v is None else "1 " + " ".join(str(int(x)) for x in v)
    return "\n".join([f"{c['nc']} {c['np']} {len(c['obs'])}", opt(c["cam_fixed"]), opt(c["pt_fixed"]), opt(c["rot"]), opt(c["pos"]), opt(c["pt"]),
                      " ".join(str(o[0]) for o in c["obs"]), " ".join(str(o[1]) for o in c["obs"])]) + "\n"


def parse(stdout):
    """("error", why) or ("plan", the five arrays as inner_iterations_ref.ordering_lists returns them)"""
    lines = stdout.splitlines()
    if lines[0].startswith("error: "):
        assert len(lines) == 1
        return "error", lines[0][len("error: "):]
    n = int(lines[0].split()[1])
    assert lines[0].split()[0] == "groups" and len(lines) == 1 + n + 4
    groups = []
    for l in lines[1:1 + n]:
        t = l.split()
        assert t[0] == "range" and len(t) == 5
        groups.append(tuple(int(v) for v in t[1:]))
    out = dict(groups=groups)
    for name, l in zip(("cam", "pt", "mask", "kind"), lines[1 + n:]):
        t = l.split()
        assert t[0] == name
        out[name] = [int(v) for v in t[1:]]
    return "plan", out


def problem(c):
    """what inner_iterations_ref.ordering reads of a BAProblem"""
    nc, npt = c["nc"], c["np"]
    m = np.array(c["cam_fixed"] if c["cam_fixed"] is not None else [0] * nc)
    cam_fixed = ((m[:, None] >> np.arange(6)[None, :]) & 1).astype(bool)
    pt_fixed = np.array(c["pt_fixed"] if c["pt_fixed"] is not None else [0] * npt).astype(bool)
    return SimpleNamespace(nc=nc, np_=npt, oc=np.array([o[0] for o in c["obs"]]), op=np.array([o[1] for o in c["obs"]]), cam_fixed=cam_fixed,
                           pt_fixed=pt_fixed, rot_active=~cam_fixed[:, :3].all(1), pos_active=~cam_fixed[:, 3:].all(1))


def reference(c, mut=frozenset()):
    """the reference's answer in parse()'s form.  It has no rule about ids below -1 (the Python wrapper refuses them before the
    library is reached): those cases keep their sentence"""
    if c["error"] is not None and "a group id below -1" in c["error"]:
        return "error", c["error"]
    try:
        return "plan", I.ordering_lists(problem(c), c["rot"], c["pos"], c["pt"], frozenset(mut))
    except ValueError as e:
        return "error", str(e) + " share a residual"


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    """kind -> {case: the driver's stdout}; every kind is built once"""
    base = tmp_path_factory.mktemp("inner_plan")
    out = {}
    for kind, flags in SANITIZERS.items():
        exe = str(base / f"driver_{kind}")
        subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", *flags, os.path.join(ROOT, "tests", "cpp", "inner_plan_driver.cpp"), "-o", exe])
        out[kind] = {}
        for name, c in CASES.items():
            p = subprocess.run([exe], input=stdin_of(c), capture_output=True, text=True, timeout=60)
            assert p.returncode == 0 and p.stderr == "", (kind, name, p.returncode, p.stderr[-2000:])
            out[kind][name] = p.stdout
    return out


def test_the_header_is_host_only():
    includes = re.findall(r"^\s*#\s*include\s*(\S+)", open(HEADER).read(), re.M)
    assert includes and all(i.startswith("<") and "hip" not in i for i in includes), includes


@pytest.mark.parametrize("name", PLANS)
def test_plan_equals_the_reference(runs, name):
    got, want = parse(runs["plain"][name]), reference(CASES[name])
    assert want[0] == "plan" and got == want, (name, got, want)
    p = got[1]
    assert len(p["cam"]) == len(p["mask"]) == len(p["kind"])
    assert all(lo <= hi for g in p["groups"] for lo, hi in (g[:2], g[2:]))


def test_the_plan_cases_reach_their_branches(runs):
    plan = lambda name: parse(runs["plain"][name])[1]
    d = plan("default_nothing_constant")
    assert d == dict(groups=[(0, 3, 0, 0), (3, 3, 0, 4)], cam=[0, 1, 2], pt=[0, 1, 2, 3], mask=[ALL6] * 3, kind=[3] * 3)
    d = plan("default_constant_camera_and_landmark")
    assert d["cam"] == [0, 2] and d["pt"] == [0, 1, 3]
    assert plan("rotation_and_position_share_an_id")["kind"] == [3, 3, 3] and len(plan("rotation_and_position_share_an_id")["groups"]) == 2
    assert plan("three_groups")["kind"] == [1, 1, 1, 2, 2, 2] and plan("three_groups")["mask"] == [7, 7, 7, 56, 56, 56]
    assert plan("landmarks_in_the_lowest_id")["groups"][0] == (0, 0, 0, 4)
    assert plan("only_pt_group") == dict(groups=[(0, 0, 0, 2), (0, 0, 2, 4)], cam=[], pt=[0, 1, 2, 3], mask=[], kind=[])
    d = plan("ids_9_2_5")           # ascending: positions (2), landmarks (5), rotations (9)
    assert d["groups"] == [(0, 3, 0, 0), (3, 3, 0, 4), (3, 6, 4, 4)] and d["kind"] == [2, 2, 2, 1, 1, 1]
    d = plan("minus_one_mixed_in")
    assert d["cam"] == [0, 2, 1, 2] and d["pt"] == [0, 2, 3] and d["groups"] == [(0, 2, 0, 0), (2, 4, 0, 0), (4, 4, 0, 2), (4, 4, 2, 3)]
    assert plan("one_constant_rotation_dof")["mask"][0] == 5 != 7
    d = plan("constant_rotation_is_ignored")
    assert d["groups"][0] == (0, 0, 0, 4) and d["cam"] == [0, 1, 2] and d["kind"] == [2, 2, 2]
    assert plan("camera_without_observation")["cam"] == [0, 1, 2, 3, 0, 1, 2, 3] and plan("camera_without_observation_default")["cam"] == [0, 1, 2, 3]
    empty = dict(groups=[], cam=[], pt=[], mask=[], kind=[])
    assert plan("everything_constant") == empty and plan("everything_constant_default") == empty


@pytest.mark.parametrize("name", REFUSALS)
def test_refusals_are_the_sentences_of_the_entry_point(runs, name):
    c = CASES[name]
    assert parse(runs["plain"][name]) == ("error", c["error"]) == reference(c), name


def test_a_dependent_group_names_the_first_observation_in_the_order_given(runs):
    a, b = CASES["dependent_group"], CASES["dependent_group_reversed_observations"]
    assert sorted(a["obs"]) == sorted(b["obs"]) and a["obs"] != b["obs"] and {k: a[k] for k in ("rot", "pos", "pt")} == {k: b[k] for k in ("rot", "pos", "pt")}
    assert "camera 1 and landmark 3" in parse(runs["plain"]["dependent_group"])[1]
    assert "camera 2 and landmark 3" in parse(runs["plain"]["dependent_group_reversed_observations"])[1]


def test_every_mutation_is_caught(runs):
    caught = {m: [name for name, c in CASES.items() if reference(c, (m,)) != parse(runs["plain"][name])] for m in I.ORDERING_MUTATIONS}
    for m, names in caught.items():
        print(f"MUTATION {m}: caught by {names}")
    assert all(caught.values()), caught
    assert all(reference(c) == parse(runs["plain"][name]) for name, c in CASES.items()), "without a mutation nothing differs"


def test_sanitized_driver_runs_clean(runs):
    """(the fixture asserts exit code 0 and an empty stderr: a sanitizer report is neither)"""
    assert runs["asan_ubsan"] == runs["plain"]
