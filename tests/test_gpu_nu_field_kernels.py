"""The three kernels of csrc/psg_nu_field.cuh alone, in the style of tests/test_attack_kernels.py: every
case runs twice from fresh buffers and must repeat bit for bit except the atomically accumulated sums; outputs whose
contract is "left untouched" are compared byte for byte with what was put there.

psg_nu_coord_apply_rooms is exact (one fp32 addition); psg_nu_coord_adam_step_rooms lies within attack_ref64's error model
(V / bound) of float64 autograd + torch's Adam; psg_smooth_knn_xyz_rooms lies within the DERIVED bounds of
tests/nu_field_ref64.py (|d_fp32 - d| <= 4 * 2^-24 d, propagated to sums and gradients) and picks float64's neighbour sets
- except at queries whose float64 ranks nb and nb + 1 lie closer than twice that bound: those are listed, re-decided (every
index chosen must lie within the bound of the nb-th distance, every clearly nearer one must be chosen) and capped at 0.1 %."""
import numpy as np
import pytest
import torch

import nu_field_ref64 as R
from test_attack_kernels import ADAM_EPS, BETA1, BETA2, F, LR, POINT_SHAPES, assert_bits, check64, dev, f32, host, lib, nanf, seeded, twice

pytestmark = pytest.mark.gpu


def point_cases():
    out = []
    for k, (B, N) in enumerate(POINT_SHAPES):
        for use_mask in (False, True):
            for step in (1, 7):
                rng = seeded(61, k, int(use_mask), step)
                x0 = rng.random((B, N, 9)).astype(F)
                ori = (rng.random((B, N, 3)) * np.array([1, 1, 3]) - np.array([0.5, 0.5, 0])).astype(F)
                first = step == 1
                delta = np.zeros((B, N, 3), F) if first else (rng.standard_normal((B, N, 3)) * 10.0 ** rng.uniform(-5, -2, (B, N, 3))).astype(F)
                m = np.zeros_like(delta) if first else (rng.standard_normal(delta.shape) * 1e-3).astype(F)
                v = np.zeros_like(delta) if first else (rng.random(delta.shape) * 1e-5 + 1e-12).astype(F)
                dx0 = (rng.standard_normal((B, N, 9)) * 10.0 ** rng.uniform(-6, -1, (B, N, 9))).astype(F)
                dx0[:, ::5, 0] = (F(0), F(-0.0))[k % 2]
                sg = rng.standard_normal((B, N, 3)).astype(F)
                mask = (rng.random((B, N)) < 0.6).astype(np.uint8)
                mask[0, 0], mask[-1, -1] = (0, 1) if N > 1 else (1, 1)
                active = np.ones(B, np.uint8)
                if B > 1:
                    active[1] = 0
                out.append(dict(B=B, N=N, step=step, x0=x0, ori=ori, delta=delta, m=m, v=v, dx0=dx0, sg=sg if (k + step) % 2 else None,
                                mask=mask if use_mask else None, active=active, c=f32(1e-4),
                                name="coord B=%d N=%d step=%d mask=%d" % (B, N, step, use_mask)))
    return out


def test_coord_apply():
    _lib, P, st = lib()
    for c in point_cases():
        B, N = c["B"], c["N"]

        def run():
            # (every buffer is held in a name until the launch is enqueued: a temporary's block would be handed to the next one)
            x0, delta, ori, mk, act = dev(c["x0"]), dev(c["delta"]), dev(c["ori"]), dev(c["mask"]), dev(c["active"])
            _lib.call("psg_nu_coord_apply_rooms", P(delta), P(ori), P(mk), B, N, P(act), P(x0), st())
            return dict(x0=host(x0))
        got = twice(run)["x0"]
        assert_bits(got, R.coord_apply(c["x0"], c["delta"], c["ori"], c["mask"], c["active"]), c["name"] + " apply")
        on = np.ones((B, N), bool) if c["mask"] is None else c["mask"].astype(bool)
        on = on & c["active"].astype(bool)[:, None]
        assert_bits(got[~on], c["x0"][~on], c["name"] + ": masked-out points and the inactive room")
        assert_bits(got[:, :, 3:], c["x0"][:, :, 3:], c["name"] + ": channels 3:9")
    with pytest.raises(_lib.PsgError):
        _lib.call("psg_nu_coord_apply_rooms", None, None, None, 1, 4, None, None, st())


def test_coord_adam_step():
    _lib, P, st = lib()
    for c in point_cases():
        B, N = c["B"], c["N"]

        def run():
            d, m, v = dev(c["delta"]), dev(c["m"]), dev(c["v"])
            mk, dx0, sg, act = dev(c["mask"]), dev(c["dx0"]), dev(c["sg"]), dev(c["active"])
            l2 = torch.zeros(B, device="cuda")
            if B > 1:
                l2[1] = 0.5                                               # the inactive room's sum: not to be touched
            _lib.call("psg_nu_coord_adam_step_rooms", P(d), P(m), P(v), P(mk), P(dx0), P(sg), c["c"], LR, BETA1, BETA2, ADAM_EPS,
                      c["step"], B, N, P(act), P(l2), st())
            return dict(delta=host(d), m=host(m), v=host(v), l2=host(l2))
        got = twice(run, skip=("l2",))
        d2, m2, v2, l2, de, me, ve, l2e = R.coord_adam_step(c["delta"], c["m"], c["v"], c["mask"], c["dx0"], c["sg"], c["c"], f32(LR),
                                                            f32(BETA1), f32(BETA2), f32(ADAM_EPS), c["step"], c["active"])
        check64(c["name"] + " delta", got["delta"], d2, de)
        check64(c["name"] + " m", got["m"], m2, me)
        check64(c["name"] + " v", got["v"], v2, ve)
        live = c["active"].astype(bool)
        check64(c["name"] + " l2", got["l2"][live], l2[live], l2e[:, live])
        on = np.ones((B, N), bool) if c["mask"] is None else c["mask"].astype(bool)
        on = on & live[:, None]
        for k in ("delta", "m", "v"):
            assert_bits(got[k][~on], c[k][~on], c["name"] + ": untouched " + k)
        if B > 1:
            assert_bits(got["l2"][1:2], np.array([0.5], F), c["name"] + ": L2 slot of the inactive room")
    with pytest.raises(_lib.PsgError):
        t = nanf(1, 64, 9)
        _lib.call("psg_nu_coord_adam_step_rooms", P(t), P(t), P(t), None, P(t), None, 0.0, LR, BETA1, BETA2, ADAM_EPS, 0, 1, 64, None, None, st())


def run_smooth(c, active=None, nb=None):
    _lib, P, st = lib()
    B, N, nb = c["B"], c["N"], nb or c["nb"]
    # adversarial points as channels 0:3 of nine-channel rows, the references compact - the strides the attack uses
    x0 = np.full((B, N, 9), 7.0, F)
    x0[:, :, 0:3] = c["adv"]
    x0, ref, act = dev(x0), dev(c["ref"]), dev(active)
    total = torch.full((B,), 0.25, device="cuda")
    grad = nanf(B, N, 3)
    nn = torch.full((B, N, nb), -1, dtype=torch.int32, device="cuda")
    _lib.call("psg_smooth_knn_xyz_rooms", P(x0), 9, N * 9, P(ref), 3, N * 3, B, N, nb, P(total), P(grad), P(act), P(nn), st())
    return dict(total=host(total), grad=host(grad), nn=host(nn))


@pytest.mark.parametrize("k", range(len(R.SMOOTH_SHAPES)))
def test_smooth_xyz(k):
    c = R.smooth_cases()[k]
    B, N, nb = c["B"], c["N"], c["nb"]
    got = twice(lambda: run_smooth(c), skip=("total",))
    listed = 0
    for b in range(B):
        ref = c["refs"][b]
        nn, g = got["nn"][b], got["grad"][b]
        assert (nn >= 0).all() and (nn < N).all()
        same = (np.sort(nn, 1) == np.sort(ref["idx"], 1)).all(1)
        tie = R.near_tie(ref, nb)
        assert not (~same & ~tie).any(), "%s room %d: %d queries away from any near tie chose another neighbour set" % (
            c["name"], b, int((~same & ~tie).sum()))
        # the listed queries, re-decided: what was chosen lies within the bound of the nb-th distance, what is clearly nearer was chosen
        for q in np.nonzero(~same)[0]:
            d_q = R.dist64(c["adv"][b][q:q + 1], c["ref"][b])[0]
            kth = ref["d"][q, -1]
            slack = 2 * R.dist_bound(ref["next_d"][q])
            print("LISTED %s room %d query %d: float64 ranks %d / %d at %.9e / %.9e, chose %s" % (
                c["name"], b, q, nb, nb + 1, kth, ref["next_d"][q], sorted(set(nn[q]) - set(ref["idx"][q]))))
            assert len(set(nn[q])) == nb and (d_q[nn[q]] <= kth + slack).all()
            assert set(np.nonzero(d_q < kth - slack)[0]) <= set(nn[q])
        listed += int((~same).sum())
        assert tie.mean() <= R.TIE_SHARE_CAP
        # distances, in the kernel's own rank order, through the gradient and the sum on the CHOSEN sets
        g64, abs_terms = R.grad_on(c["adv"][b], c["ref"][b], nn.astype(np.int64))
        gerr = np.abs(g.astype(np.float64) - g64)
        gb = R.grad_bound(abs_terms, nb)
        print("RATIO %-40s grad room %d  %.4f" % (c["name"], b, float((gerr / gb).max())))
        assert (gerr <= gb).all(), "%s room %d: gradient outside the derived bound, worst %.3g x" % (c["name"], b, float((gerr / gb).max()))
        d_chosen = np.take_along_axis(R.dist64(c["adv"][b], c["ref"][b]), nn.astype(np.int64), 1)
        # rank order: ascending distances up to the bound, the lower index first at exact ties
        assert (np.diff(d_chosen, axis=1) >= -2 * R.dist_bound(d_chosen[:, 1:])).all()
        eq = np.diff(d_chosen, axis=1) == 0
        assert (np.diff(nn, axis=1)[eq] > 0).all()
        terr = abs(float(got["total"][b]) - 0.25 - d_chosen.sum())
        # (the sum is ADDED to the 0.25 the slot held: one more term of the any-order sum model)
        tb = R.sum_bound(np.append(d_chosen.reshape(-1), 0.25))
        print("RATIO %-40s total room %d %.4f" % (c["name"], b, terr / tb))
        assert terr <= tb
        if c["perts"][b] == 0.0:
            # unmoved points: the self neighbour is rank 0 at distance exactly 0 and adds exactly nothing
            assert (nn[:, 0] == np.arange(N)).all()
            g_wo_self, _ = R.grad_on(c["adv"][b], c["ref"][b], nn[:, 1:].astype(np.int64))
            assert (np.abs(g - g_wo_self) <= gb).all()
    print("%s: %d listed queries of %d" % (c["name"], listed, B * N))
    assert listed <= R.TIE_SHARE_CAP * B * N


def test_smooth_xyz_one_neighbour_of_unmoved_points_is_exactly_zero():
    c = R.smooth_cases()[0]
    got = twice(lambda: run_smooth(c, nb=1), skip=())
    assert_bits(got["total"], np.array([0.25], F), "sum of zero distances")
    assert_bits(got["grad"], np.zeros((1, c["N"], 3), F), "gradient of the self neighbour")
    assert (got["nn"][0, :, 0] == np.arange(c["N"])).all()


def test_smooth_xyz_inactive_room_is_untouched():
    c = R.smooth_cases()[1]
    active = np.array([1, 0, 1], np.uint8)
    full, part = run_smooth(c), twice(lambda: run_smooth(c, active=active), skip=("total",))
    for b in (0, 2):
        assert_bits(part["grad"][b], full["grad"][b], "active room %d gradient" % b)
        assert_bits(part["nn"][b], full["nn"][b], "active room %d lists" % b)
    assert_bits(part["total"][1:2], np.array([0.25], F), "sum slot of the inactive room")
    assert np.isnan(part["grad"][1]).all() and (part["nn"][1] == -1).all()


def test_smooth_xyz_refusals():
    _lib, P, st = lib()
    t, r = nanf(1, 64, 3), nanf(1, 64, 3)
    for N, nb in ((64, 17), (64, 0), (8193, 5)):
        with pytest.raises(_lib.PsgError):
            _lib.call("psg_smooth_knn_xyz_rooms", P(t), 3, 0, P(r), 3, 0, 1, N, nb, None, P(t), None, None, st())
