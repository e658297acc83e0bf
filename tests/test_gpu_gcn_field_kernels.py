"""The two new kernels of the ResGCN coordinate-field attacks alone, in the style of
tests/test_gpu_nu_field_kernels.py: every case runs twice from fresh buffers and must repeat bit for bit except the atomically
accumulated sums; outputs whose contract is "left untouched" are compared byte for byte with what was put there.

psg_smooth_knn_xyz_sym_rooms: its lists are pass 1's contract replayed in fp32 numpy (ascending (distance, index) on the direct
distance) EXACTLY, and float64's sets except at near ties (listed, re-decided, capped at 0.1 %); the two-sided gradient lies
within the derived bound of tests/gcn_field_ref64.py on the chosen lists and sums to zero over the room within that bound.
psg_nu_coord_adam_step_rooms_w: psg_nu_coord_adam_step_rooms bit for bit when the two weights agree, attack_ref64's error
model when they differ.  (Its device-row constants exist only inside a window: tests/test_gpu_gcn_field.py compares windows
that read them with hand-driven steps that pass the same constants by value, bit for bit.)"""
import numpy as np
import pytest
import torch

import gcn_field_ref64 as G
import nu_field_ref64 as R
from test_attack_kernels import ADAM_EPS, BETA1, BETA2, F, LR, assert_bits, check64, dev, f32, host, lib, nanf, twice
from test_gpu_nu_field_kernels import point_cases

pytestmark = pytest.mark.gpu

SHAPES = ((1, 1, 5), (1, 7, 10), (3, 333, 10), (2, 1024, 5), (1, 2049, 16))       # (G, N, nb); 2049 crosses the pass-2 tile


def rooms_for(k):
    """per shape: (xyz [G][N][3], active [G] or None, what each room is)"""
    Gr, N, nb = SHAPES[k]
    if k == 2:
        dup = G.sym_points(N, 0.0, room=1).copy()
        src = np.random.default_rng(53).permutation(N)[:60]
        dup[(src + 1) % N] = dup[src]                                  # exact duplicates: decided by index
        return np.stack([G.sym_points(N, 1e-2), G.sym_points(N, 1e-4), dup]), np.array([1, 0, 1], np.uint8), ("moved", "inactive", "duplicates")
    if k == 3:
        same = np.broadcast_to(G.sym_points(N, 0.0)[17], (N, 3)).copy()
        return np.stack([G.sym_points(N, 1e-4), same]), None, ("moved", "coincident")
    return np.stack([G.sym_points(N, 1e-2 if k == 4 else 0.0)]), None, ("moved" if k == 4 else "clean",)


def run_sym(xyz, nb, active=None, lists=True):
    _lib, P, st = lib()
    Gr, N, _ = xyz.shape
    x0 = np.full((Gr, N, 9), 7.0, F)
    x0[:, :, 0:3] = xyz
    x0, act = dev(x0), dev(active)
    total = torch.full((Gr,), 0.25, device="cuda")
    grad = nanf(Gr, N, 3)
    nn = torch.full((Gr, N, nb), -1, dtype=torch.int32, device="cuda")
    _lib.call("psg_smooth_knn_xyz_sym_rooms", P(x0), 9, N * 9, Gr, N, nb, P(total), P(grad), P(act), P(nn) if lists else None, st())
    return dict(total=host(total), grad=host(grad), nn=host(nn), x0=host(x0))


@pytest.mark.parametrize("k", range(len(SHAPES)))
def test_smooth_xyz_sym(k):
    Gr, N, nb = SHAPES[k]
    xyz, active, kinds = rooms_for(k)
    got = twice(lambda: run_sym(xyz, nb, active), skip=("total",))
    assert (got["x0"][:, :, 3:] == 7.0).all() and np.array_equal(got["x0"][:, :, 0:3], xyz)
    held = min(nb, N)
    listed = 0
    for b in range(Gr):
        nn, g, total = got["nn"][b], got["grad"][b], float(got["total"][b])
        if kinds[b] == "inactive":
            assert np.isnan(g).all() and (nn == -1).all()
            assert_bits(got["total"][b:b + 1], np.array([0.25], F), "sum slot of the inactive room")
            continue
        # the lists: pass 1's contract, replayed exactly; ranks nobody holds (N < nb) stay as they were
        d32 = np.sqrt(G.d2_direct_fp32(xyz[b])).astype(F)
        want = G.pass1_lists(d32, nb)
        assert np.array_equal(nn[:, :held], want), "%s room %d: lists differ from the (distance, index) order" % (SHAPES[k], b)
        assert (nn[:, held:] == -1).all()
        # .. and float64's sets away from near ties
        ref = G.sym_smooth(xyz[b], nb)
        same = (np.sort(nn[:, :held], 1) == np.sort(ref["idx"], 1)).all(1)
        tie = R.near_tie(ref, nb)
        assert not (~same & ~tie).any(), "room %d: %d queries away from any near tie chose another set" % (b, int((~same & ~tie).sum()))
        assert tie.mean() <= G.TIE_SHARE_CAP
        for q in np.nonzero(~same)[0]:
            d_q = R.dist64(xyz[b][q:q + 1], xyz[b])[0]
            kth, slack = ref["d"][q, -1], 2 * R.dist_bound(ref["next_d"][q])
            print("LISTED %s room %d query %d" % (SHAPES[k], b, q))
            assert len(set(nn[q])) == nb and (d_q[nn[q]] <= kth + slack).all()
            assert set(np.nonzero(d_q < kth - slack)[0]) <= set(nn[q])
        listed += int((~same).sum())
        # the two-sided gradient on the CHOSEN lists, and the sum of the distances
        g64, gb, d_chosen = G.grad_on_lists(xyz[b], nn[:, :held])
        gerr = np.abs(g.astype(np.float64) - g64)
        print("RATIO %-28s grad room %d (%s) %.4f" % (SHAPES[k], b, kinds[b], float((gerr / gb).max())))
        assert np.isfinite(g).all() and (gerr <= gb).all(), "room %d: gradient outside the derived bound, worst %.3g x" % (b, float((gerr / gb).max()))
        tb = R.sum_bound(np.append(d_chosen.reshape(-1), 0.25))
        assert abs(total - 0.25 - d_chosen.sum()) <= tb
        # every pair term enters once with each sign: the room's gradients add up to zero within their bounds
        assert (np.abs(g.astype(np.float64).sum(0)) <= gb.sum(0)).all()
        assert (nn[:, 0] == np.arange(N)).all() or kinds[b] in ("duplicates", "coincident")       # itself first, at distance 0
        if kinds[b] == "coincident":
            assert_bits(g, np.zeros((N, 3), F), "coincident points: every term is exactly zero")
            assert_bits(got["total"][b:b + 1], np.array([0.25], F), "coincident points: sum of zero distances")
            assert (nn == np.arange(nb)[None]).all()
        if kinds[b] == "duplicates":
            assert (d_chosen[:, 1] == 0).any()                              # a duplicate at rank 1, at distance exactly 0
    assert listed <= G.TIE_SHARE_CAP * Gr * N


def test_smooth_xyz_sym_without_a_list_buffer_and_with_every_room_active():
    xyz, active, _ = rooms_for(2)
    with_lists, without = run_sym(xyz, 10, active), run_sym(xyz, 10, active, lists=False)
    for b in (0, 2):
        assert_bits(without["grad"][b], with_lists["grad"][b], "scratch lists, room %d" % b)
    assert np.isnan(without["grad"][1]).all() and (without["nn"] == -1).all()
    full = run_sym(xyz, 10, None)
    for b in (0, 2):
        assert_bits(full["grad"][b], with_lists["grad"][b], "room %d beside an active room 1" % b)
    assert np.isfinite(full["grad"][1]).all()


def test_smooth_xyz_sym_refusals():
    _lib, P, st = lib()
    t, s = nanf(1, 64, 3), nanf(1)
    for N, nb, total in ((64, 17, s), (64, 0, s), (8193, 5, s), (64, 5, None)):
        with pytest.raises(_lib.PsgError):
            _lib.call("psg_smooth_knn_xyz_sym_rooms", P(t), 3, 0, 1, N, nb, P(total), P(t), None, None, st())


def run_adam(c, name, *weights):
    _lib, P, st = lib()
    B, N = c["B"], c["N"]
    d, m, v = dev(c["delta"]), dev(c["m"]), dev(c["v"])
    mk, dx0, sg, act = dev(c["mask"]), dev(c["dx0"]), dev(c["sg"]), dev(c["active"])
    l2 = torch.zeros(B, device="cuda")
    if B > 1:
        l2[1] = 0.5                                               # the inactive room's sum: not to be touched
    _lib.call(name, P(d), P(m), P(v), P(mk), P(dx0), P(sg), *weights, LR, BETA1, BETA2, ADAM_EPS, c["step"], B, N, P(act), P(l2), st())
    return dict(delta=host(d), m=host(m), v=host(v), l2=host(l2))


def test_coord_adam_step_with_two_weights():
    _lib, P, st = lib()
    for c in point_cases():
        B, N = c["B"], c["N"]
        # equal weights: the one-weight entry point, bit for bit
        one = run_adam(c, "psg_nu_coord_adam_step_rooms", c["c"])
        two = twice(lambda: run_adam(c, "psg_nu_coord_adam_step_rooms_w", c["c"], c["c"]), skip=("l2",))
        for k in ("delta", "m", "v"):
            assert_bits(two[k], one[k], c["name"] + ": equal weights, " + k)
        # different weights: float64 autograd + torch's Adam within the error model
        cs, cl = f32(1e-4), f32(0.3)
        got = run_adam(c, "psg_nu_coord_adam_step_rooms_w", cs, cl)
        d2, m2, v2, l2, de, me, ve, l2e = G.coord_adam_step_w(c["delta"], c["m"], c["v"], c["mask"], c["dx0"], c["sg"], cs, cl, f32(LR),
                                                              f32(BETA1), f32(BETA2), f32(ADAM_EPS), c["step"], c["active"])
        check64(c["name"] + " w delta", got["delta"], d2, de)
        check64(c["name"] + " w m", got["m"], m2, me)
        check64(c["name"] + " w v", got["v"], v2, ve)
        live = c["active"].astype(bool)
        check64(c["name"] + " w l2", got["l2"][live], l2[live], l2e[:, live])
        on = (np.ones((B, N), bool) if c["mask"] is None else c["mask"].astype(bool)) & live[:, None]
        for k in ("delta", "m", "v"):
            assert_bits(got[k][~on], c[k][~on], c["name"] + ": untouched " + k)
        if B > 1:
            assert_bits(got["l2"][1:2], np.array([0.5], F), c["name"] + ": L2 slot of the inactive room")
    with pytest.raises(_lib.PsgError):
        t = nanf(1, 64, 9)
        _lib.call("psg_nu_coord_adam_step_rooms_w", P(t), P(t), P(t), None, P(t), None, 0.0, 0.0, LR, BETA1, BETA2, ADAM_EPS, 0, 1, 64, None,
                  None, st())
