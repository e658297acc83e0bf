"""Grid sub-sampling and sub-cloud projection on the device (psg_grid.hip through randla/grid.py) against the numpy float32
restatement (tests/grid_ref.py, itself pinned to the reference's native code by tests/test_grid_host.py) and, for the
projection, against psg_knn_points.  Everything is compared bit for bit: no tolerance anywhere in this file."""
import os
import time

import numpy as np
import pytest

import grid_ref

pytestmark = pytest.mark.gpu

GOLD = os.path.join(os.path.dirname(__file__), "golden", "grid_sub.npz")
NAMES = ("room", "neg", "tiny")
F = np.float32


@pytest.fixture(scope="module")
def fx():
    return dict(np.load(GOLD))


@pytest.fixture(scope="module")
def subs(fx):
    """name -> (raw points, sub-cloud of the restatement, dl): computed once, never written to."""
    out = {}
    for name in NAMES:
        p, dl = fx[name + "_points"], float(fx[name + "_dl"])
        sub = grid_ref.grid_sub_sampling(p, None, None, dl)["sub_points"]
        sub.setflags(write=False)
        out[name] = (p, sub, dl)
    return out


def dev(a):
    import torch
    return None if a is None else torch.from_numpy(np.array(a, copy=True, order="C")).cuda()


def host(t):
    return None if t is None else t.cpu().numpy()


def run_device(p, f, lab, dl):
    from pointsecguard_amd.randla.grid import grid_sub_sampling_device
    return [host(t) for t in grid_sub_sampling_device(dev(p), dev(f), dev(lab), dl, return_index=True)]


def check_a(p, f=None, lab=None, dl=0.1):
    """Device against restatement: sub_points, sub_features, sub_labels, voxel_of_point, all exact."""
    want = grid_ref.grid_sub_sampling(p, f, lab, dl)
    sp, sf, sl, vox = run_device(p, f, lab, dl)
    assert sp.dtype == F and grid_ref.same_bits(sp, want["sub_points"])
    assert vox.dtype == np.int32 and np.array_equal(vox, want["voxel_of_point"])
    if f is None:
        assert sf is None
    else:
        assert sf.dtype == F and grid_ref.same_bits(sf, want["sub_features"])
    if lab is None:
        assert sl is None
    else:
        assert sl.dtype == np.int32 and sl.ndim == 2 and np.array_equal(sl, want["sub_labels"])
    return want


def cloud(n, seed, box=1.0, d=3, l=1):
    rng = np.random.default_rng(seed)
    p = (rng.random((n, 3), dtype=F) * F(box)).astype(F)
    f = None if d == 0 else rng.integers(0, 256, (n, d)).astype(F)
    lab = None if l == 0 else rng.integers(0, 13, (n, l) if l > 1 else n).astype(np.int32)
    return p, f, lab


# ------------------------------------------------------------------------------------------------ A
@pytest.mark.parametrize("name", NAMES)
def test_fixtures(fx, name):
    want = check_a(fx[name + "_points"], fx[name + "_colors"], fx[name + "_labels"], float(fx[name + "_dl"]))
    assert len(want["count"]) == len(fx[name + "_sub_points"])


@pytest.mark.parametrize("n", (1, 2, 63, 64, 65, 257, 4097))
def test_sizes(n):
    check_a(*cloud(n, n), dl=0.11)


def test_one_voxel():
    p, f, lab = cloud(4096, 1, box=0.03)
    want = check_a(p + F(0.005), f, lab, dl=0.04)
    assert len(want["count"]) == 1


def test_every_point_its_own_voxel():
    g = np.stack(np.meshgrid(np.arange(16), np.arange(15), np.arange(9), indexing="ij"), -1).reshape(-1, 3)
    rng = np.random.default_rng(3)
    p = ((g[rng.permutation(len(g))] + F(0.5)) * F(0.25)).astype(F)
    want = check_a(p, *cloud(len(p), 4)[1:], dl=0.25)
    assert len(want["count"]) == len(p)


def test_long_segment_among_singletons():
    """One voxel of 4096 points among 4096 voxels of one point, interleaved in input order: the long segment of the sorted
    order spans sixteen workgroups of the per-position kernels."""
    rng = np.random.default_rng(5)
    g = np.stack(np.meshgrid(np.arange(1, 17), np.arange(16), np.arange(16), indexing="ij"), -1).reshape(-1, 3)
    single = ((g + F(0.5)) * F(0.1)).astype(F)
    crowd = (rng.random((4096, 3), dtype=F) * F(0.09) + F(0.005)).astype(F)
    p = np.empty((8192, 3), F)
    p[0::2], p[1::2] = single, crowd
    _, f, lab = cloud(8192, 6)
    want = check_a(p, f, lab, dl=0.1)
    assert sorted(want["count"])[-2:] == [1, 4096] and len(want["count"]) == 4097


def test_points_on_cell_faces():
    """Coordinates exactly k * dl in float32, both signs - among them minima whose cell index is -1 in the reference's formula
    (tests/test_grid_host.py::test_negative_cell_index_is_clamped)."""
    dl = F(0.04)
    k = np.arange(-400, 400, dtype=np.int64)
    rng = np.random.default_rng(8)
    for lo in (-400, -396, -37, 0):
        ks = k[k >= lo]
        p = np.stack([rng.choice(ks, 3000).astype(F) * dl, rng.choice(ks[:40], 3000).astype(F) * dl, rng.choice(ks[:9], 3000).astype(F) * dl], 1)
        p[0] = F(lo) * dl
        check_a(p.astype(F), *cloud(3000, 9)[1:], dl=dl)
    x = np.nextafter(F(-396) * dl, F(-np.inf))
    p = np.array([[x, 0, 0], [x, 0.01, 0], [x + F(0.03), 0, 0], [0, 0, 0]], F)
    origin, _, _ = grid_ref.grid_of(p, dl)
    assert origin[0] > x                                  # the clamped case itself
    check_a(p, None, np.array([3, 4, 4, 5], np.int32), dl=dl)


def test_duplicated_points():
    p, f, lab = cloud(3000, 10)
    p[1000:2000] = p[:1000]
    p[2000:2500] = p[7]
    check_a(p, f, lab, dl=0.07)


@pytest.mark.parametrize("d", (0, 1, 3, 6))
@pytest.mark.parametrize("l", (0, 1, 2))
def test_feature_and_label_widths(d, l):
    p, f, lab = cloud(2500, 11 + d + 10 * l, d=d, l=l)
    check_a(p, f, lab, dl=0.12)


def test_label_values_span_int32():
    p, f, _ = cloud(4000, 12, d=1)
    rng = np.random.default_rng(13)
    vals = np.array([-2 ** 31, -2 ** 31 + 1, -70000, -1, 0, 1, 255, 65536, 2 ** 31 - 2, 2 ** 31 - 1], np.int64)
    lab = vals[rng.integers(0, len(vals), (4000, 2))].astype(np.int32)
    want = check_a(p, f, lab, dl=0.2)
    assert want["tied"].any() and (want["sub_labels"] < 0).any() and (want["sub_labels"] > 65536).any()


def test_vote_is_not_quadratic():
    """4096 points of one voxel with 1000 distinct labels: exact, and within the seconds a test has."""
    import torch
    p = (np.random.default_rng(14).random((4096, 3), dtype=F) * F(0.03) + F(0.005)).astype(F)
    lab = (np.arange(4096) % 1000).astype(np.int32) * 7 - 3000
    lab[4000:] = 77                                       # the unique maximum, 96 votes (77 is not of the form 7 k - 3000)
    lab = lab[np.random.default_rng(15).permutation(4096)]
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    want = check_a(p, None, lab, dl=0.04)
    assert time.perf_counter() - t0 < 5.0
    assert want["sub_labels"].tolist() == [[77]]


def test_two_runs_are_byte_identical(fx):
    a = run_device(fx["room_points"], fx["room_colors"], fx["room_labels"], 0.04)
    b = run_device(fx["room_points"], fx["room_colors"], fx["room_labels"], 0.04)
    for x, y in zip(a, b):
        assert x.tobytes() == y.tobytes()


def test_non_default_stream(fx, subs):
    import torch
    from pointsecguard_amd.randla.grid import nearest_sub_point
    p, sub, dl = subs["neg"]
    st = torch.cuda.Stream()
    with torch.cuda.stream(st):
        check_a(p, fx["neg_colors"], fx["neg_labels"], dl)
        got = host(nearest_sub_point(dev(sub), dev(p), dl))
    st.synchronize()
    assert np.array_equal(got, grid_ref.nearest_sub_point(sub, p))


def test_reference_api_tuples(fx):
    from pointsecguard_amd.randla.helper_tool import DP
    p, col, lab = fx["tiny_points"], fx["tiny_colors"], fx["tiny_labels"]
    want = grid_ref.grid_sub_sampling(p, col, lab, 0.05)
    m = len(want["count"])
    a = DP.grid_sub_sampling(p.astype(np.float64), grid_size=0.05)
    assert isinstance(a, np.ndarray) and a.dtype == F and a.shape == (m, 3) and grid_ref.same_bits(a, want["sub_points"])
    b = DP.grid_sub_sampling(p, features=col.astype(np.uint8), grid_size=0.05)
    assert isinstance(b, tuple) and len(b) == 2 and b[1].dtype == F and grid_ref.same_bits(b[1], want["sub_features"])
    c = DP.grid_sub_sampling(p, labels=lab.astype(np.int64), grid_size=0.05)
    assert len(c) == 2 and c[1].dtype == np.int32 and c[1].shape == (m, 1) and np.array_equal(c[1], want["sub_labels"])
    e = DP.grid_sub_sampling(p, col, lab, 0.05, verbose=0)
    assert len(e) == 3 and [x.shape for x in e] == [(m, 3), (m, 3), (m, 1)] and [x.dtype for x in e] == [F, F, np.int32]


# ------------------------------------------------------------------------------------------------ B
def check_b(sub, q, dl):
    from pointsecguard_amd.randla.grid import nearest_sub_point
    from pointsecguard_amd.randla.helper_tool import knn_points
    got = host(nearest_sub_point(dev(sub), dev(q), dl))
    assert got.dtype == np.int32 and got.shape == (len(q),)
    knn = host(knn_points(dev(sub[None]), dev(q[None]), 1))[0, :, 0]
    assert np.array_equal(got, knn)
    assert np.array_equal(got, grid_ref.nearest_sub_point(sub, q))
    return got


@pytest.mark.parametrize("name", NAMES)
def test_projection_of_raw_points(subs, name):
    p, sub, dl = subs[name]
    check_b(sub, p, dl)


@pytest.mark.parametrize("name,scale", [(n, s) for n in NAMES for s in (1.0, 3.0, 1000.0)])
def test_projection_of_random_queries(subs, name, scale):
    """4097 queries inside the cloud's box, in a box three times as large around it, and 1000 box sizes away (there the
    float32 distances tie in runs and the lower index must win over the whole cloud)."""
    _, sub, dl = subs[name]
    lo, hi = sub.min(0), sub.max(0)
    rng = np.random.default_rng(int(scale) + len(sub))
    u = rng.random((4097, 3), dtype=F)
    if scale < 100:
        mid, half = (lo + hi) / 2, (hi - lo) / 2 * F(scale)
        q = mid - half + u * 2 * half
    else:
        q = hi + (hi - lo) * F(scale) * (F(0.5) + u) * np.array([1, -1, 1], F)
    check_b(sub, q.astype(F), dl)


@pytest.mark.parametrize("m", (1, 2, 26, 27))
def test_projection_small_sub_clouds(m):
    rng = np.random.default_rng(20 + m)
    sub = rng.random((m, 3), dtype=F)
    q = (rng.random((1000, 3), dtype=F) * 3 - 1).astype(F)
    for dl in (0.04, 0.5, 7.0):
        check_b(sub, q, dl)


@pytest.mark.parametrize("dl", (1e-3, 1e-5))
def test_projection_sparse_sub_cloud_with_small_cells(dl):
    """50 sub-points in a 100 m box under cells of 1 mm and of 0.01 mm (10^5 and 10^7 cells along an axis): the table doubles its
    cell until the grid has at most 64 cells per sub-point, so the queries neither walk an empty grid nor are refused."""
    rng = np.random.default_rng(31)
    sub = (rng.random((50, 3), dtype=F) * 100).astype(F)
    q = (rng.random((2000, 3), dtype=F) * 140 - 20).astype(F)
    check_b(sub, q, dl)


def test_projection_exact_hits_and_ties(subs):
    _, sub, dl = subs["tiny"]
    got = check_b(sub, sub.copy(), dl)                               # a query exactly at a sub-point
    assert np.array_equal(got, np.arange(len(sub)))
    # two sub-points equidistant from the query, far enough apart to lie in different cells; the lower index is listed second
    sub2 = np.array([[5, 5, 5], [0.75, 0.25, 0.25], [-0.25, 0.25, 0.25], [0.25, 0.25, 0.75], [0.25, -0.25, 0.25]], F)
    q = np.array([[0.25, 0.25, 0.25]], F)
    for dl in (0.1, 0.25, 0.3, 2.0):
        assert check_b(sub2, q, dl).tolist() == [1]
        assert check_b(sub2[::-1].copy(), q, dl).tolist() == [0]


# ------------------------------------------------------------------------------------------------ refusals
def test_device_refusals():
    import torch
    from pointsecguard_amd import _lib
    from pointsecguard_amd.randla.grid import grid_sub_sampling_device, nearest_sub_point
    p = dev(cloud(100, 30)[0])
    for bad in (float("nan"), float("inf"), -float("inf")):
        q = p.clone()
        q[57, 1] = bad
        with pytest.raises(_lib.PsgError, match="non-finite"):
            grid_sub_sampling_device(q, grid_size=0.1)
        with pytest.raises(_lib.PsgError, match="non-finite"):
            nearest_sub_point(q, p, 0.1)
    wide = p.clone()
    wide[3, 2] = 2.0 ** 20 * 0.1 + 5.0
    with pytest.raises(_lib.PsgError, match=r"more than 2\^20 cells"):
        grid_sub_sampling_device(wide, grid_size=0.1)
    with pytest.raises(_lib.PsgError, match=r"more than 2\^20 cells"):
        grid_sub_sampling_device(p, grid_size=1e-30)
    with pytest.raises(ValueError):
        grid_sub_sampling_device(p, grid_size=0.0)
    with pytest.raises(ValueError):
        grid_sub_sampling_device(p, features=torch.zeros(99, 3, device="cuda"), grid_size=0.1)
    with pytest.raises(ValueError):
        grid_sub_sampling_device(p[:, :2].contiguous(), grid_size=0.1)
    sp, _, _ = grid_sub_sampling_device(p, grid_size=0.1)            # the handle still works after the refusals
    assert grid_ref.same_bits(host(sp), grid_ref.grid_sub_sampling(host(p), None, None, 0.1)["sub_points"])
