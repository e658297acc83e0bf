"""Level 0 of a many-forward geometry plan takes its groups from a per-room ball table (psg_pn2.hip: ball_table_route,
group_from_table_kernel): a level-0 centroid is a point of the room, so its ball query - the first K indices in index order
with sqdist <= r^2 - is a function of that point alone, and the table holds it for every point of the room, built once per
psg_pn2_plan_build.  The result is integers: equal to the direct query or wrong.

Through the C ABI: psg_pn2_plan_build, level-0 FPS and groups read back with psg_pn2_plan_ptr, and the stand-alone
psg_ball_query on the centroids gathered from the room by those FPS indices; all P x 1024 x K indices must be equal, for SSG
(r = 0.1, K = 32) and both MSG scales (r = 0.05, K = 16; r = 0.1, K = 32).

  * B = 2 (p % n_clouds and the room stride of the table), N = 4096; plans of 7 forwards (just below the threshold
    n_forward x 1024 >= 2 N: the direct query), 8 (just at it: the table) and 40 (the attack's plan), all in this process;
    which route ran is read from psg_pn2_prof_read: the table route is one launch more under the ball-query tag per scale
    (with PSG_PN2_BALL_TABLE=0 set for the whole suite every plan must report the direct route, and the equalities still hold);
  * rooms: a seeded synthetic one; one where 64 points are exact copies of others (ties at distance 0, index order); one with
    a point farther than r from every other (its group: itself K times); one with a clump of 100 points inside one ball,
    scattered over the index range (the stop at K, index order);
  * a second plan on the same workspace with other rooms follows the new rooms (the table is rebuilt, nothing stale);
  * the coordinate attack rebuilds one-forward plans: it stays on the direct route on a workspace that owns a table."""

import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
B, N, S0 = 2, 4096, 1024
F_MAX = 40
TABLE_FROM = 8          # BALL_TABLE_C = 2 (psg_pn2.hip): the table route from n_forward * 1024 >= 2 * N
ISO, CLUMP_N = 1234, 100
SWITCH = os.environ.get("PSG_PN2_BALL_TABLE", "1")   # 0: the direct query for every plan; 2: the table for every plan
SCALES = {0: ((0.1, 32),), 1: ((0.05, 16), (0.1, 32))}     # runtime.ARCH_SSG / ARCH_MSG: (radius, nsample) of level 0


def dev(a, dt=None):
    t = torch.from_numpy(np.ascontiguousarray(a))
    return (t.to(dt) if dt is not None else t).cuda().contiguous()


def rooms_pair(kind):
    """float32 [2][4096][9]"""
    from pointsecguard_amd.synthetic import make_rooms
    if kind == "seeded_dup":
        r = make_rooms(2, 4242)
        rng = np.random.default_rng(7)
        src = rng.permutation(N)[:128]
        r[1, src[64:]] = r[1, src[:64]]                         # 64 exact duplicates (whole rows), at scattered indices
        return r
    r = make_rooms(2, 99)
    r[0, ISO, 0:3] = (1.5, 1.5, 4.0)                            # room 0: more than 0.1 from every other point
    rng = np.random.default_rng(8)
    idx = np.sort(rng.permutation(N)[:CLUMP_N])                 # room 1: 100 points within 0.02 of one place
    r[1, idx, 0:3] = np.array([0.1, -0.2, 1.0], np.float32) + rng.uniform(-0.01, 0.01, (CLUMP_N, 3)).astype(np.float32)
    return r


def clump_of(rooms):
    return np.nonzero(np.abs(rooms[1, :, 0:3] - np.array([0.1, -0.2, 1.0], np.float32)).max(-1) <= 0.0101)[0]


def table_route(n_forward):
    return SWITCH == "2" or (SWITCH != "0" and n_forward >= TABLE_FROM)


def starts_for(n_forward, seed, room1_start=None):
    """[n_forward][4][B] FPS start draws; room1_start: the level-0 start of room 1 in every forward"""
    rng = np.random.default_rng(seed)
    st = np.stack([rng.integers(0, n, (n_forward, B)) for n in (N, 1024, 256, 64)], axis=1).astype(np.int32)
    if room1_start is not None:
        st[:, 0, 1] = room1_start
    return st


@pytest.fixture(scope="module")
def workspaces():
    from pointsecguard_amd import runtime
    return {arch: runtime.PN2Workspace(B, N, F_MAX, arch=arch) for arch in (runtime.ARCH_SSG, runtime.ARCH_MSG)}


def plan_block(ws, what, n_forward, k):
    """[n_forward * B][1024](, k) int32: slots 0 .. n_forward - 1 of a level-0 plan table, contiguous from slot 0, room 0"""
    from pointsecguard_amd import _lib, runtime
    src = _lib.load().psg_pn2_plan_ptr(ws.handle, what, 0, 0, 0)
    assert src
    out = torch.empty((n_forward * B, S0) + ((k,) if k else ()), dtype=torch.int32, device=ws.device)
    runtime._hip_memcpy_d2d(out.data_ptr(), src, out.numel() * 4)
    return out


def build_and_check(ws, arch, rooms, n_forward, seed, room1_start=None):
    """-> (fps, [groups per scale]) as numpy, after the equality check against the stand-alone query and the route check"""
    from pointsecguard_amd import _lib, runtime
    x0 = dev(rooms)
    ws.prof_enable(True)
    ws.plan_build(x0, dev(starts_for(n_forward, seed, room1_start)), n_forward)
    launches = ws.prof_read()["ball_query"][1]
    ws.prof_enable(False)
    ns = len(SCALES[arch])
    assert launches == (5 if table_route(n_forward) else 4) * ns, (n_forward, launches)
    P = n_forward * B
    fps = plan_block(ws, 0, n_forward, 0)
    xyz = x0[:, :, 0:3].contiguous()
    room_of = torch.arange(P, device=xyz.device) % B
    new_xyz = xyz[room_of[:, None], fps.long()].contiguous()                # [P][1024][3]: xyz0[p % B][fps[p][s]]
    groups = []
    for sc, (radius, k) in enumerate(SCALES[arch]):
        got = plan_block(ws, 1 if sc == 0 else 5, n_forward, k)
        want = torch.empty_like(got)
        r2 = float(np.float32(radius ** 2))
        _lib.call("psg_ball_query", runtime.context(xyz.device), runtime.ptr(xyz), B, runtime.ptr(new_xyz), P, N, S0, r2, k,
                  runtime.ptr(want), runtime.stream())
        torch.cuda.synchronize()
        g, w = got.cpu().numpy(), want.cpu().numpy()
        assert g.tobytes() == w.tobytes(), (arch, sc, n_forward, int((g != w).any(-1).sum()))
        assert g.min() >= 0 and g.max() < N                                 # every centroid finds at least itself
        groups.append(g)
    return fps.cpu().numpy(), groups


@pytest.mark.parametrize("n_forward", [TABLE_FROM - 1, TABLE_FROM, F_MAX])
@pytest.mark.parametrize("kind", ["seeded_dup", "iso_clump"])
@pytest.mark.parametrize("arch", [0, 1])
def test_plan_groups_equal_the_standalone_query(workspaces, arch, kind, n_forward):
    rooms = rooms_pair(kind)
    # (FPS spaces its 1024 samples ~0.14 apart: room 1 starts inside the 0.02 clump, so that a clump point is a centroid)
    start1 = int(clump_of(rooms)[-1]) if kind == "iso_clump" else None
    fps, groups = build_and_check(workspaces[arch], arch, rooms, n_forward, 100 * n_forward + arch, start1)
    if kind != "iso_clump":
        return
    clump = clump_of(rooms)
    assert len(clump) >= CLUMP_N
    for sc, (radius, k) in enumerate(SCALES[arch]):
        g = groups[sc]
        # the isolated point is the farthest from everything: FPS takes it in every forward, and its group is itself K times
        p, s = np.nonzero(fps[0::B] == ISO)
        assert len(p) == n_forward
        assert (g[0::B][p, s] == ISO).all()
        # a centroid inside the clump (every clump point is within 0.035 of it: inside the ball of either scale): K distinct
        # indices, ascending, no padding, and none beyond the K-th clump point - the scan stopped at K of >= 100 candidates
        p, s = np.nonzero(np.isin(fps[1::B], clump))
        assert len(p) >= n_forward
        rows = g[1::B][p, s]
        assert (np.diff(rows, axis=-1) > 0).all() and rows.max() <= clump[k - 1]


@pytest.mark.parametrize("arch", [0, 1])
def test_second_plan_on_the_workspace_follows_the_new_rooms(workspaces, arch):
    ws = workspaces[arch]
    _, a = build_and_check(ws, arch, rooms_pair("seeded_dup"), TABLE_FROM, 5)
    _, b = build_and_check(ws, arch, rooms_pair("iso_clump"), TABLE_FROM, 5)        # same starts, other rooms
    assert any(x.tobytes() != y.tobytes() for x, y in zip(a, b))
    _, a2 = build_and_check(ws, arch, rooms_pair("seeded_dup"), TABLE_FROM, 5)
    assert all(x.tobytes() == y.tobytes() for x, y in zip(a, a2))


def test_coordinate_attack_plans_take_the_direct_route(workspaces, gpu_model):
    """field = "coord" moves xyz, so every iteration rebuilds a one-forward plan: 1024 centroids per room, below the threshold
    on a workspace whose capacity (40 forwards) gave it a table - four ball-query launches per iteration, none for a table."""
    from pointsecguard_amd.synthetic import rule_labels
    ws, iters = workspaces[0], 2
    rooms = rooms_pair("seeded_dup")
    images = dev(rooms.transpose(0, 2, 1))
    labels = dev(rule_labels(rooms).astype(np.int32))
    ws.prof_enable(True)
    adv = ws.field_attack(gpu_model, images, labels, dev(starts_for(iters, 3)), 0.05, 2 / 255, iters, "coord")
    torch.cuda.synchronize()
    launches = ws.prof_read()["ball_query"][1]
    ws.prof_enable(False)
    assert launches == (5 if table_route(1) else 4) * iters
    assert not torch.equal(adv[:, 0:3], images[:, 0:3]) and torch.equal(adv[:, 3:], images[:, 3:])
