"""RandLA-Net's position-branch gradient on the CPU: the float64 stages of tests/rla_coord_ref64.py ARE float64 autograd of
the network for a leaf on the point positions (indices constant, the distance column contributing zero where it is zero), each
transpose is the adjoint of its forward stage, a float32 evaluation passes every bound, every mutant fails at its own stage,
and the feature path alone - what psg_rla_backward returns - fails the end-to-end bars the GPU tests set
(tests/test_gpu_rla_coord.py): SIGN_BAR / FLIP_BAR of DESIGN.md section 5k."""
import numpy as np
import pytest

from oracle import randla_net
from pointsecguard_amd.synthetic import randla_params
import randla_ref64 as R
import rla_coord_ref64 as C
from test_randla_stages import cpu_case, failing, knn_tree, make_cloud  # noqa: F401  (cpu_case: a module-scoped fixture)

SIGN_BAR, FLIP_BAR = 0.999, 1e-3


@pytest.fixture(scope="module")
def xyz_case(cpu_case):
    """per cloud: the float32 emulation of the position-branch stages on the float32 emulation of the network, and the
    float64 stages on the SAME forward state and decisions"""
    P, cases = cpu_case
    out = {}
    for n, c in cases.items():
        emu, _ = C.walk_xyz(P, c["fwd"], c["bwd"], c["geo"], dt=np.float32)
        bwd64, _ = R.walk_backward(P, c["fwd"], c["dl"], c["geo"])
        ref, _ = C.walk_xyz(P, c["fwd"], bwd64, c["geo"])
        out[n] = dict(emu=emu, bwd64=bwd64, ref=ref)
    return out


class _ZeroSafeOracle(randla_net.RandLAOracle):
    """the oracle with a distance column that is differentiable at zero: d sqrt(|rel|^2) = 0 where rel = 0"""

    @staticmethod
    def relative_pos_encoding(xyz, neigh):
        import torch
        nb = xyz[neigh]
        tile = xyz[:, None, :].expand_as(nb)
        rel = tile - nb
        sq = (rel * rel).sum(-1, keepdim=True)
        pos = sq > 0
        dis = torch.where(pos, torch.sqrt(torch.where(pos, sq, torch.ones_like(sq))), torch.zeros_like(sq))
        return torch.cat([dis, rel, tile, nb], dim=-1)


def autograd_xyz(params, c, through_features):
    """d colper loss / d positions in float64 autograd: the positions feed every level's relpos (level l + 1 = the first
    n / ratio rows of level l) and, when through_features, columns 0:3 of the features"""
    import torch
    o = _ZeroSafeOracle(params, dtype=torch.float64)
    _, neigh, pools, ups = c["pyr"]
    x = torch.from_numpy(c["xyz"]).double().requires_grad_(True)
    levels = [x]
    for i in range(4):
        levels.append(levels[-1][:levels[-1].shape[0] // R.RATIO[i]])
    lng = lambda a: torch.from_numpy(np.ascontiguousarray(a)).long()          # noqa: E731
    feats = torch.cat([x if through_features else x.detach(), torch.from_numpy(c["rgb"]).double()], -1)
    logits = o.forward(feats, levels, [lng(a) for a in neigh], [lng(a) for a in pools], [lng(a) for a in ups])
    randla_net.colper_loss(logits, lng(c["labels"])).backward()
    assert torch.isfinite(x.grad).all()
    return x.grad.numpy()


@pytest.mark.parametrize("n", [8192, 8704])
def test_float64_stages_compose_to_autograd(cpu_case, monkeypatch, n):
    """exact fold, the oracle's slope: geometric part alone and the sum with dfeatures[:, 0:3], to 1e-12 of the maximum"""
    monkeypatch.setattr(R, "SLOPE", 0.2)
    _, cases = cpu_case
    c = cases[n]
    params = randla_params(3)
    P = R.fold_all(params, rounded=False)
    fwd, _ = R.walk_forward(P, c["feats"], c["geo"])
    bwd, _ = R.walk_backward(P, fwd, R.colper_dlogits(fwd[("logits", 0)], c["labels"]), c["geo"])
    got, _ = C.walk_xyz(P, fwd, bwd, c["geo"])
    geo_only = autograd_xyz(params, c, False)
    both = autograd_xyz(params, c, True)
    assert np.abs(geo_only).max() > 0
    assert np.abs(got[("dxyz", 0)] - geo_only).max() <= 1e-12 * np.abs(geo_only).max()
    assert np.abs(got[("dxyz", 0)] + bwd[("dfeatures", 0)][:, :3] - both).max() <= 1e-12 * np.abs(both).max()


def test_transposes_are_adjoint():
    """<J v, u> = <v, J^T u> to 1e-12 for every new transpose, on random vectors"""
    import torch
    rng = np.random.default_rng(7)
    n, h, n_sub = 60, 8, 15
    d = 2 * h
    nb = rng.integers(0, n, (n, 16))
    nb[:, 0] = np.arange(n)                                     # self edges: dist == 0
    rel = lambda a, b: abs(a - b) <= 1e-12 * max(abs(a), abs(b))          # noqa: E731
    # attentive pooling w.r.t. the position half
    W = (rng.standard_normal((d, d)), None)
    f, fxyz, v, u = rng.standard_normal((n, h)), rng.standard_normal((n * 16, h)), rng.standard_normal((n * 16, h)), rng.standard_normal((n, d))
    tn, tW, tf = torch.from_numpy(nb), torch.from_numpy(W[0]), torch.from_numpy(f)

    def pool(tx):
        cat = torch.cat([tf[tn], tx.reshape(n, 16, h)], -1)
        return (cat * torch.softmax(cat @ tW.T, 1)).sum(1)
    _, jv = torch.autograd.functional.jvp(pool, torch.from_numpy(fxyz), torch.from_numpy(v))
    assert rel(float((jv.numpy() * u).sum()), float((v * C.att_pool_T_xyz(f, fxyz, nb, W, u)[0]).sum()))
    # relpos of two chained levels (level 1 = the first n_sub rows of level 0) w.r.t. the positions
    x, vx = rng.standard_normal((n, 3)), rng.standard_normal((n, 3))
    nb1 = rng.integers(0, n_sub, (n_sub, 16))
    nb1[:, 0] = np.arange(n_sub)
    u0, u1 = rng.standard_normal((n * 16, 10)), rng.standard_normal((n_sub * 16, 10))
    t0, t1 = torch.from_numpy(nb), torch.from_numpy(nb1)

    def enc(tx):
        a = _ZeroSafeOracle.relative_pos_encoding(tx, t0).reshape(-1, 10)
        b = _ZeroSafeOracle.relative_pos_encoding(tx[:n_sub], t1).reshape(-1, 10)
        return a, b
    (r0, r1), (j0, j1) = torch.autograd.functional.jvp(enc, torch.from_numpy(x), torch.from_numpy(vx))
    assert np.abs(r0.numpy() - R.relpos(x.astype(np.float32), nb)).max() < 1e-6        # (R.relpos rounds the points to float32)
    si, _, sj, _ = C.relpos_T(r1.numpy(), u1)
    g1, _ = C.point_sum(si, sj, nb1, None, None)
    si, _, sj, _ = C.relpos_T(r0.numpy(), u0)
    g0, _ = C.point_sum(si, sj, nb, g1, np.arange(n_sub))
    assert rel(float((j0.numpy() * u0).sum() + (j1.numpy() * u1).sum()), float((vx * g0).sum()))
    assert np.abs(C.relpos_fwd(r0.numpy()[:, 1:4]) - r0.numpy()[:, 0]).max() <= 1e-12


@pytest.mark.parametrize("n", [8192, 8704])
def test_float32_emulation_passes_every_new_stage(cpu_case, xyz_case, n):
    P, cases = cpu_case
    c, x = cases[n], xyz_case[n]
    _, rep = C.walk_xyz(P, c["fwd"], c["bwd"], c["geo"], taps=x["emu"])
    for k in sorted(rep.ratio, key=str):
        print("%-16s error / bound %.3f" % (k, rep.ratio[k]))
    assert not rep.fail, rep.fail
    assert len(rep.stages) == 31


STAGES = lambda *names: sorted("('%s', %d)" % (k, i) for k in names for i in range(5))          # noqa: E731
MUTANT_FAILS = {"no_in_edges": STAGES("gxyz"), "no_dist": STAGES("side_i", "side_j"), "flip_j": STAGES("side_j"),
                "no_chain": STAGES("gxyz")[:4], "swap_masks": STAGES("G1", "G2"), "no_direct": STAGES("G1", "G2")}


@pytest.mark.parametrize("mutant", C.MUTANTS)
def test_mutants_fail_at_their_own_stage(cpu_case, mutant):
    """a snapshot of a network with one of the bugs (in-edge side dropped, distance column dropped, sign of the j side
    flipped, level chain dropped, sign words of fxyz1 and fxyz2 swapped, direct pooling term dropped) fails, at the stages
    that bug touches and nowhere else"""
    P, cases = cpu_case
    c = cases[8704]
    wrong, _ = C.walk_xyz(P, c["fwd"], c["bwd"], c["geo"], dt=np.float32, mutant=mutant)
    _, rep = C.walk_xyz(P, c["fwd"], c["bwd"], c["geo"], taps=wrong)
    assert failing(rep) == MUTANT_FAILS[mutant], rep.fail


def test_zero_distance_adds_exactly_zero():
    """self edges (every point is its own first neighbour) and the duplicated points of the batch's second cloud: the distance
    column's gradient, however large, leaves no trace - side_i / side_j are what the other nine columns give, bit for bit"""
    xyz, _, _ = make_cloud(8192, 2, 12)
    cloud = xyz[8192:]
    nb = knn_tree(cloud[None], cloud[None], 16)[0].astype(np.int64)
    rp = R.relpos(cloud, nb, np.float32)
    zero = rp[:, 0] == 0
    assert int((nb == np.arange(8192)[:, None]).sum()) == 8192 and int(zero.sum()) == 8192 + 512
    rng = np.random.default_rng(3)
    g = rng.standard_normal((len(rp), 10)).astype(np.float32)
    big = g.copy()
    big[:, 0] = np.float32(3e38)
    for dt in (np.float32, np.float64):
        si, _, sj, _ = C.relpos_T(rp, big, dt)
        assert np.isfinite(si[zero]).all() and np.isfinite(sj[zero]).all()
        assert np.array_equal(si[zero, :3], (g[zero, 1:4].astype(dt) + g[zero, 4:7].astype(dt)))
        assert np.array_equal(sj[zero, :3], (g[zero, 7:10].astype(dt) - g[zero, 1:4].astype(dt)))
        ref_i = C.relpos_T(rp, g, dt, dist_col=False)[0]
        assert np.array_equal(C.relpos_T(rp, g, dt)[0][zero], ref_i[zero])


@pytest.mark.parametrize("n", [8192, 8704])
def test_end_to_end_bars(cpu_case, xyz_case, n):
    """the premise of the GPU tests' end-to-end bars - a float32 evaluation against the float64 stages ON ITS OWN DECISIONS is
    inside them - and that the feature path alone, what the library returned before, is far outside"""
    _, cases = cpu_case
    c, x = cases[n], xyz_case[n]
    ref = x["ref"][("dxyz", 0)] + x["bwd64"][("dfeatures", 0)][:, :3]
    emu = x["emu"][("dxyz", 0)].astype(np.float64) + c["bwd"][("dfeatures", 0)][:, :3].astype(np.float64)
    agree, flip = C.sign_bars(emu, ref)
    err = np.abs(emu - ref).max() / np.abs(ref).max()
    print("n=%d float32 emulation vs float64 on its decisions: sign agreement %.6f, largest flipped %.3e, max err / max mag %.3e"
          % (n, agree, flip, err))
    assert agree >= SIGN_BAR and flip <= FLIP_BAR
    feat_only = x["bwd64"][("dfeatures", 0)][:, :3]
    agree, flip = C.sign_bars(feat_only, ref)
    missing = np.abs(feat_only - ref).max() / np.abs(ref).max()
    print("n=%d feature path alone: sign agreement %.4f, largest flipped %.3e, misses %.3f of the largest magnitude" % (n, agree, flip, missing))
    assert agree < SIGN_BAR and flip > FLIP_BAR
    assert 0.70 < agree < 0.85


@pytest.mark.parametrize("metric", ["l_inf", "l_2"])
def test_field_step_restatement(metric):
    """rla_coord_ref64.field_step is the oracle's BIM update (bim.py:84-98) without a box, and its l_2 form lies inside the
    float64 error model; the step never leaves the eps ball"""
    rng = np.random.default_rng(11)
    n, eps, alpha = 1000, 0.05, 0.02
    ori = (rng.random((n, 3)) * 4).astype(np.float32)
    g = rng.standard_normal((n, 3)).astype(np.float32)
    g[::7] = 0.0
    adv = ori.copy()
    for _ in range(4):
        new = C.field_step(adv, g, ori, eps, alpha, metric)
        want = randla_net.bim_step(ori.reshape(-1), adv.reshape(-1), g.reshape(-1), eps, alpha, metric, x_min=-np.inf, x_max=np.inf).reshape(n, 3)
        if metric == "l_inf":
            assert np.array_equal(new, want)
            e32 = np.float64(np.float32(eps))                   # (the ball's edge ori +- eps is itself rounded once)
            assert (np.abs(new.astype(np.float64) - ori) <= e32 + R.U * (np.abs(ori) + e32)).all()
        else:
            ref, b = C.field_step_l2_bound(adv, g, ori, eps, alpha)
            assert (np.abs(new - ref) <= b).all() and (np.abs(want - ref) <= b).all()
            assert np.sqrt(((new.astype(np.float64) - ori) ** 2).sum()) <= eps * (1 + 1e-6)
        adv = new
        g = rng.standard_normal((n, 3)).astype(np.float32)
