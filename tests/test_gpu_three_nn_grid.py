"""The grid 3-NN (three_nn_grid_kernel, psg_geometry.hip; reference: the 3-NN interpolation of PointNet/models/
pointnet_util.py:301-307) writes what the scan kernel writes - idx and w, byte for byte - on the shapes where pruning by cells
could go wrong (tests/three_nn_grid_ref.py: cases), on a fine cloud shared by several problems, on both workgroup shapes and on
one level-0 problem; and what the oracle's 3-NN computes.  PSG_THREE_NN is read once per process, so the two kernels run in
two fresh child processes (=grid: the grid kernel at every shape, =scan), once for the whole module."""
import os
import subprocess
import sys
import tempfile

import numpy as np
import pytest
import torch

import three_nn_grid_ref as R

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

CHILD = """
import sys
import numpy as np, torch
sys.path.insert(0, %r)
from pointsecguard_amd import _lib, runtime
inp = np.load(sys.argv[1])
names = sorted(set(k[:-5] for k in inp.files if k.endswith(".fine")))
ctx = runtime.context(torch.device("cuda:0"))
out = {}
for name in names:
    fine, coarse = torch.from_numpy(inp[name + ".fine"]).cuda(), torch.from_numpy(inp[name + ".crse"]).cuda()
    P, S = coarse.shape[:2]
    N = fine.shape[1]
    idx = torch.full((P, N, 3), -1, dtype=torch.int32, device="cuda")
    w = torch.full((P, N, 3), -1.0, dtype=torch.float32, device="cuda")
    _lib.call("psg_three_nn", ctx, runtime.ptr(fine), fine.shape[0], runtime.ptr(coarse), P, N, S, runtime.ptr(idx), runtime.ptr(w),
              runtime.stream())
    torch.cuda.synchronize()
    out[name + ".idx"], out[name + ".w"] = idx.cpu().numpy(), w.cpu().numpy().view(np.uint32)
np.savez(sys.argv[2], **out)
""" % ROOT


def level0_problem():
    from pointsecguard_amd import runtime
    from pointsecguard_amd.synthetic import make_rooms
    fine = torch.from_numpy(np.ascontiguousarray(make_rooms(1, 29)[:, :, :3])).cuda()
    sel = runtime.fps(fine, 1024, torch.tensor([5], dtype=torch.int32, device="cuda"))
    coarse = runtime.gather_points(fine, sel)
    return fine.cpu().numpy(), coarse.cpu().numpy()


@pytest.fixture(scope="module")
def runs():
    """name -> (fine [C, N, 3], coarse [P, S, 3]) and the outputs of both kernels."""
    rng = np.random.default_rng(7)
    inputs = {k: (f[None], c[None]) for k, (f, c) in R.cases().items()}
    # the fine cloud of problem p is cloud p % n_clouds1
    inputs["shared"] = (rng.random((2, 300, 3), dtype=np.float32), rng.random((6, 40, 3), dtype=np.float32))
    # enough problems for the workgroup shape that serves 4096 queries: a second workgroup per problem with a ragged tail
    inputs["many"] = (rng.random((3, 4100, 3), dtype=np.float32), rng.random((420, 6, 3), dtype=np.float32))
    inputs["level0"] = level0_problem()
    # a plan's worth of level-0 problems on one shared fine cloud: the size from which the dispatch takes the grid kernel by itself
    shift = (np.arange(320, dtype=np.float32) * np.float32(1e-4))[:, None, None]
    inputs["plan320"] = (inputs["level0"][0], (inputs["level0"][1] + shift).astype(np.float32))
    res = {}
    with tempfile.TemporaryDirectory() as tmp:
        src = os.path.join(tmp, "in.npz")
        np.savez(src, **{k + ".fine": f for k, (f, c) in inputs.items()}, **{k + ".crse": c for k, (f, c) in inputs.items()})
        for mode in ("grid", "scan"):
            env = dict(os.environ, PSG_THREE_NN=mode)
            dst = os.path.join(tmp, mode + ".npz")
            r = subprocess.run([sys.executable, "-c", CHILD, src, dst], env=env, capture_output=True, text=True, timeout=300)
            assert r.returncode == 0, r.stderr[-2000:]
            res[mode] = dict(np.load(dst))
    return inputs, res


NAMES = sorted(R.cases()) + ["shared", "many", "level0", "plan320"]


@pytest.mark.parametrize("name", NAMES)
def test_grid_kernel_equals_scan_kernel(runs, name):
    inputs, res = runs
    for part in (".idx", ".w"):
        g, s = res["grid"][name + part], res["scan"][name + part]
        assert g.shape == s.shape and np.array_equal(g, s), (name, part, np.argwhere(g != s)[:6])


@pytest.mark.parametrize("name", [n for n in NAMES if n not in ("outside", "inf_coarse")])
def test_grid_kernel_equals_oracle(runs, name):
    from oracle import pn2
    inputs, res = runs
    fine, coarse = inputs[name]
    P = coarse.shape[0]
    for p in sorted({0, P // 2, P - 1}):
        oi, ow = pn2.three_nn(fine[p % fine.shape[0]], coarse[p])
        assert np.array_equal(res["grid"][name + ".idx"][p], oi), (name, p)
        assert np.array_equal(res["grid"][name + ".w"][p], ow.view(np.uint32)), (name, p)


def test_expected_rows(runs):
    inputs, res = runs
    assert (res["grid"]["identical.idx"] == np.array([0, 1, 2])).all()                 # every d ties
    assert (res["grid"]["cube.idx"][0, 0] == np.array([0, 1, 2])).all()               # the centre of the cube
    assert 0 in res["grid"]["lattice_tie.idx"][0, 0]                                   # the tie from beyond the first block
    assert (res["grid"]["outside.idx"][0, 52:58] == 0).all()                           # overflow and non-finite queries: nothing passes `<`


def test_default_dispatch_gives_the_scan_bytes(runs):
    """No switch set (this process): 320 level-0 problems, the shape and count at which psg_three_nn picks the grid kernel."""
    from pointsecguard_amd import _lib, runtime
    inputs, res = runs
    fine, coarse = (torch.from_numpy(a).cuda() for a in inputs["plan320"])
    P, S = coarse.shape[:2]
    N = fine.shape[1]
    idx = torch.full((P, N, 3), -1, dtype=torch.int32, device="cuda")
    w = torch.full((P, N, 3), -1.0, dtype=torch.float32, device="cuda")
    _lib.call("psg_three_nn", runtime.context(fine.device), runtime.ptr(fine), 1, runtime.ptr(coarse), P, N, S, runtime.ptr(idx),
              runtime.ptr(w), runtime.stream())
    torch.cuda.synchronize()
    assert np.array_equal(idx.cpu().numpy(), res["scan"]["plan320.idx"])
    assert np.array_equal(w.cpu().numpy().view(np.uint32), res["scan"]["plan320.w"])
