"""Farthest-point sampling: the numpy float32 restatement of the rule fps_kernel (psg_geometry.hip) documents, and the
clouds of tests/test_fps_step_host.py and tests/test_gpu_fps_step.py.

The rule: distances start at 1e10f; a step computes d = ((dx*dx) + (dy*dy)) + (dz*dz) in float32 in that order against the
last pick, keeps d where `d < dist` (so a NaN or +inf d keeps the old distance), and picks the arg-max of the distances'
BIT PATTERNS (they are non-negative floats: the same order), the lowest index among equals."""
import numpy as np

F = np.float32


def fps_rule(xyz, npoint, start):
    x = np.ascontiguousarray(xyz, F)
    dist = np.full(x.shape[0], F(1e10))
    out = np.empty(npoint, np.int32)
    far = int(start)
    with np.errstate(all="ignore"):
        for s in range(npoint):
            out[s] = far
            dx, dy, dz = x[:, 0] - x[far, 0], x[:, 1] - x[far, 1], x[:, 2] - x[far, 2]
            d = ((dx * dx) + (dy * dy)) + (dz * dz)
            assert d.dtype == F
            dist = np.where(d < dist, d, dist)
            far = int(np.argmax(dist.view(np.uint32)))      # numpy's argmax returns the first maximum
    return out


def uniform(P, n, seed):
    """uniform in [0, 1)^3, z stretched by 3 (test_unit_geometry_vs_oracle's clouds), random starts"""
    rng = np.random.default_rng(seed)
    xyz = rng.random((P, n, 3), dtype=F)
    xyz[..., 2] *= 3
    return xyz, rng.integers(0, n, P).astype(np.int32)


def lattice(P, n, seed):
    """integer lattice {0, 1, 2, 3}^3: 64 positions for n points, exact duplicates and equal distances everywhere"""
    rng = np.random.default_rng(seed)
    return rng.integers(0, 4, (P, n, 3)).astype(F), rng.integers(0, n, P).astype(np.int32)


def twins(P, seed, n=4096):
    """points 16k and 16k + 1 are equal (two keys of one lane at 16 points per thread), and point i equals point i + n/2
    (the same key in two waves)"""
    rng = np.random.default_rng(seed)
    xyz = rng.random((P, n, 3), dtype=F)
    xyz[..., 2] *= 3
    xyz[:, 1:n // 2:16] = xyz[:, 0:n // 2:16]
    xyz[:, n // 2:] = xyz[:, :n // 2]
    return xyz, rng.integers(0, n, P).astype(np.int32)


def non_finite(seed, n=256):
    """one NaN and one +inf coordinate, at points that are not the start"""
    xyz, start = uniform(2, n, seed)
    xyz[:, 77, 1] = np.nan
    xyz[:, 200, 0] = np.inf
    start[:] = (5, n - 1)
    return xyz, start


def path_cases():
    """item 1: one shape per launch path and its ragged neighbour; (name, xyz [P,N,3], S, start [P])"""
    out = []
    for n in (64, 37, 256, 130, 1024, 1000, 1001, 4096, 4000, 4003, 5000):
        xyz, start = uniform(3, n, 100 + n)
        out.append(("uniform_%d" % n, xyz, 16, start))
    for n in (4096, 4001):                                  # one problem per CU: the last count that takes 512 x 8
        xyz, start = uniform(256, n, 200 + n)
        out.append(("uniform_%d_p256" % n, xyz, 48, start))
    for n in (4096, 4001):                                  # more: 256 threads x 16 points, centroid from global memory
        xyz, start = uniform(320, n, 250 + n)
        out.append(("uniform_%d_p320" % n, xyz, 48, start))
    return out


def tie_cases():
    xyz, start = lattice(3, 256, 7)
    tw, tws = twins(256, 8)
    tw2, tws2 = twins(320, 9)
    return [("lattice_256", xyz, 64, start), ("twins_4096_p256", tw, 32, tws), ("twins_4096_p320", tw2, 32, tws2)]


def edge_cases(sizes=(64, 130)):
    out = []
    for n in sizes:
        xyz, start = uniform(3, n, 300 + n)
        out.append(("all_taken_%d" % n, xyz, n, start))                                  # S = N: then every key is 0
        out.append(("last_start_%d" % n, xyz, min(n, 16), np.full(3, n - 1, np.int32)))
        out.append(("one_sample_%d" % n, xyz, 1, start))
    return out


def switch_cases():
    """item 5: what a PSG_FPS_CFG value is compared on, at N = 4096 and 4000"""
    out = []
    for n in (4096, 4000):
        xyz, start = uniform(3, n, 400 + n)
        out.append(("uniform_%d" % n, xyz, 16, start))
        xyz, start = uniform(256, n, 500 + n)
        out.append(("uniform_%d_p256" % n, xyz, 48, start))
        lat, ls = lattice(3, n, 600 + n)
        out.append(("lattice_%d" % n, lat, 80, ls))                                      # 64 positions: keys all 0 from step 64
    tw, tws = twins(256, 8)
    out.append(("twins_4096_p256", tw, 32, tws))
    return out + edge_cases((4096, 4000))
