"""The step loop of fps_kernel (psg_geometry.hip; reference: farthest_point_sample, PointNet/models/pointnet_util.py:63-84)
through runtime.fps, bit for bit against oracle.pn2.fps: one shape and its ragged neighbour per launch path (64 x 1, 64 x 4,
256 x 4, 512 x 8 - up to 256 problems -, 256 x 16 with the centroid from global memory - above 256 problems, the probe's
crossover -, 1024 x 8 threads x points), clouds of exact ties inside a lane,
between lanes and between waves (lowest index wins), a start at the last point, S = N, S = 1, non-finite coordinates
against the numpy restatement of the documented rule (tests/fps_step_ref.py; tests/test_fps_step_host.py pins the
expectations on the host), and every launch shape PSG_FPS_CFG adds for measurements against the default in a child process."""
import os
import subprocess
import sys
import tempfile

import numpy as np
import pytest
import torch

import fps_step_ref as ref

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def run(xyz, s, start):
    from pointsecguard_amd import runtime
    return runtime.fps(torch.from_numpy(xyz).cuda(), s, torch.from_numpy(start).cuda()).cpu().numpy()


def check(case, problems=None):
    from oracle import pn2
    name, xyz, s, start = case
    got = run(xyz, s, start)
    assert got.shape == (xyz.shape[0], s) and got.dtype == np.int32
    for p in (range(xyz.shape[0]) if problems is None else problems):
        want = pn2.fps(xyz[p], s, start[p])
        assert np.array_equal(got[p], want), (name, p, np.nonzero(got[p] != want)[0][:4])
    return got


@pytest.mark.parametrize("case", ref.path_cases(), ids=lambda c: c[0])
def test_every_launch_path_equals_oracle(case):
    check(case)


@pytest.mark.parametrize("case", ref.tie_cases(), ids=lambda c: c[0])
def test_ties_resolve_to_the_lowest_index(case):
    name, xyz, s, start = case
    got = check(case)
    if name.startswith("twins"):
        n = xyz.shape[1]
        assert (got[:, 1:] < n // 2).all() and (got[:, 1:] % 16 != 1).all()


def test_lattice_past_its_positions_returns_index_zero():
    (_, xyz, _, start), = [c for c in ref.tie_cases() if c[0] == "lattice_256"]
    got = check(("lattice_256_s80", xyz, 80, start))
    assert (got[:, 64:] == 0).all()                   # at most 64 positions: every key is 0 from there on


@pytest.mark.parametrize("case", ref.edge_cases(), ids=lambda c: c[0])
def test_edges_equal_oracle(case):
    name, xyz, s, start = case
    got = check(case)
    if name.startswith("all_taken"):
        assert (np.sort(got, axis=1) == np.arange(s)).all()


def test_non_finite_coordinates_follow_the_documented_rule():
    xyz, start = ref.non_finite(9)
    only_inf = xyz.copy()
    only_inf[:, 77, 1] = 0.25
    neg = xyz.copy()
    neg[:, 200, 0] = -np.inf
    for cloud in (xyz, only_inf, neg):
        got = run(cloud, 16, start)
        for p in range(cloud.shape[0]):
            assert np.array_equal(got[p], ref.fps_rule(cloud[p], 16, start[p])), p


CHILD = """
import sys
import numpy as np, torch
sys.path.insert(0, %r)
sys.path.insert(0, %r)
import fps_step_ref as ref
from pointsecguard_amd import runtime
out = [runtime.fps(torch.from_numpy(xyz).cuda(), s, torch.from_numpy(start).cuda()).cpu().numpy().reshape(-1)
       for _, xyz, s, start in ref.switch_cases()]
np.save(sys.argv[1], np.concatenate(out))
""" % (os.path.join(ROOT, "tests"), ROOT)


@pytest.fixture(scope="module")
def default_outputs():
    assert not os.environ.get("PSG_FPS_CFG"), "the default launch table is what the switch values are compared with"
    cases = ref.switch_cases()
    out = []
    for case in cases:
        # the oracle on every problem of the small cases, on a few of the 256-problem ones
        out.append(check(case, None if case[1].shape[0] <= 3 else (0, 1, 255)).reshape(-1))
    return np.concatenate(out)


@pytest.mark.parametrize("cfg", ["3", "4", "5"])
def test_switch_value_equals_default(cfg, default_outputs):
    """PSG_FPS_CFG = 4 / 5 (256 x 16 / 512 x 8 without the cloud in LDS: the centroid comes from global memory) and 3 (256 x 16
    with it, which no problem count selects by default) in a fresh child process: byte-equal outputs on the random, tie and
    edge clouds at N = 4096 and 4000."""
    with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, "cfg.npy")
        env = dict(os.environ)
        env["PSG_FPS_CFG"] = cfg
        r = subprocess.run([sys.executable, "-c", CHILD, path], env=env, capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stderr[-2000:]
        got = np.load(path)
    assert got.dtype == default_outputs.dtype and got.tobytes() == default_outputs.tobytes()
