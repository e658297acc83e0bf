"""Host tests of RandLA-Net's NU attacks on the coordinate field: the float64 restatement of the two
update kernels with its counted bounds against their float32 emulation and five mutants, the gradient that enters Adam against
float64 autograd through the oracle, the lockstep control flow against a plain per-cloud loop on scripted networks with three
mutants, the C ABI of the new entry points and the refusals of the classes that need no device."""
import ctypes

import numpy as np
import pytest

from oracle import randla_net
from pointsecguard_amd.synthetic import randla_params
import randla_ref64 as R64
import rla_coord_ref64 as C
import rla_nu_field_ref as F
import rla_nu_ref as R
from test_randla_stages import cpu_case  # noqa: F401  (a module-scoped fixture)
from test_rla_coord_host import _ZeroSafeOracle


# ---------------------------------------------------------------------------------------------------- the two kernels
def kernel_case(n, masked, moved, seed=0, G=3):
    """state of an attack on G clouds: `moved` False is the zero-delta first step (dist2 = 0 exactly)"""
    rng = np.random.default_rng(seed + n)
    ori = (rng.random((G, n, 3), dtype=np.float32) * np.array([4, 3, 3], np.float32)).astype(np.float32)
    mask = (rng.random((G, n)) < 0.4) if masked else None
    if masked:
        mask[:, 0] = True
    delta = (0.01 * rng.standard_normal((G, n, 3))).astype(np.float32) if moved else np.zeros((G, n, 3), np.float32)
    m = (0.1 * rng.standard_normal((G, n, 3))).astype(np.float32) if moved else np.zeros((G, n, 3), np.float32)
    v = (0.01 * rng.random((G, n, 3))).astype(np.float32) if moved else np.zeros((G, n, 3), np.float32)
    dfeat3 = rng.standard_normal((G, n, 3)).astype(np.float32)
    dxyz = rng.standard_normal((G, n, 3)).astype(np.float32)
    return ori, delta, m, v, dfeat3, dxyz, mask


@pytest.mark.parametrize("masked", [False, True])
@pytest.mark.parametrize("n", [1, 63, 1000])
def test_float32_emulation_is_inside_the_counted_bounds(n, masked):
    c, lr = 0.5, 0.01
    for moved, t in ((False, 1), (True, 3), (True, 7)):
        ori, delta, m, v, dfeat3, dxyz, mask = kernel_case(n, masked, moved)
        xyz, dist2 = F.apply32(ori, delta, mask)
        ref, b = F.apply64(ori, delta, mask)
        assert (np.abs(xyz - ref) <= b).all()
        if masked:
            assert np.array_equal(xyz[~mask].view(np.uint32), ori[~mask].view(np.uint32))
        d2, b2 = F.dist2_64(xyz, ori)
        assert (np.abs(dist2.astype(np.float64) - d2) <= b2).all()
        assert moved or (dist2 == 0).all()
        got = F.coord_adam32(ori, delta, m, v, xyz, dfeat3, dxyz, dist2, c, lr, t, mask)
        want, bound = F.coord_adam64(ori, delta, m, v, xyz, dfeat3, dxyz, dist2, c, lr, t, mask)
        for name, g, w, e in zip(("delta", "m", "v"), got, want, bound):
            err = np.abs(g.astype(np.float64) - w)
            assert np.isfinite(g).all() and (err <= e).all(), (name, t, float((err / np.maximum(e, 1e-300)).max()))
        if masked:      # a point off the mask: no gradient, the moments only decay, delta stays where it is when m is zero
            off = ~mask
            assert np.array_equal(want[1][off], np.float64(R.B1) * m[off]) and np.array_equal(want[2][off], np.float64(R.B2) * v[off])
            if not moved:
                assert not got[0][off].any()


@pytest.mark.parametrize("mutant", F.ADAM_MUTANTS)
def test_adam_mutants_fail_their_own_check(mutant):
    """Each of the five bugs, as a float32 evaluation, leaves the bound of the specification somewhere - on the inputs that
    expose it: the guard on the zero-delta first step (0 / 0), the bias correction at t = 1 where lr_t = 0.316 lr, the mask on a
    masked case, the two dropped terms on a moved state."""
    c, lr = 0.5, 0.01
    masked = mutant == "mask_ignored"
    moved, t = (False, 1) if mutant == "no_guard" else (True, 1 if mutant == "no_bias_correction" else 3)
    ori, delta, m, v, dfeat3, dxyz, mask = kernel_case(1000, masked, moved)
    xyz, dist2 = F.apply32(ori, delta, mask)
    args = (ori, delta, m, v, xyz, dfeat3, dxyz, dist2, c, lr, t, mask)
    want, bound = F.coord_adam64(*args)
    good = F.coord_adam32(*args)
    assert all((np.abs(g.astype(np.float64) - w) <= e).all() for g, w, e in zip(good, want, bound))
    with np.errstate(invalid="ignore"):
        bad = F.coord_adam32(*args, mutant=mutant)
        out = [not (np.abs(g.astype(np.float64) - w) <= e).all() for g, w, e in zip(bad, want, bound)]
    assert any(out), mutant
    if mutant == "no_guard":
        assert np.isnan(bad[0]).all() and np.isfinite(good[0]).all()
    if mutant == "no_bias_correction":
        assert out == [True, False, False]              # the moments do not see the step size


# ---------------------------------------------------------------------------------------------------- gradient == autograd
def autograd_field(params, c, ori, delta, ys, mask, cs):
    """d (|delta|_2 + cs * hinge) / d delta in float64 autograd: xyz = ori + mask * delta feeds every level's relpos and the
    features' columns 0:3; the indices are the case's, constant"""
    import torch
    o = _ZeroSafeOracle(params, dtype=torch.float64)
    _, neigh, pools, ups = c["pyr"]
    d = torch.from_numpy(delta.astype(np.float64)).requires_grad_(True)
    mk = torch.ones(len(ori), 1, dtype=torch.float64) if mask is None else torch.from_numpy(mask.astype(np.float64))[:, None]
    x = torch.from_numpy(ori.astype(np.float64)) + mk * d
    levels = [x]
    for i in range(4):
        levels.append(levels[-1][:levels[-1].shape[0] // R64.RATIO[i]])
    lng = lambda a: torch.from_numpy(np.ascontiguousarray(a)).long()          # noqa: E731
    feats = torch.cat([x, torch.from_numpy(c["rgb"]).double()], -1)
    logits = o.forward(feats, levels, [lng(a) for a in neigh], [lng(a) for a in pools], [lng(a) for a in ups])
    score = randla_net.colper_loss_masked(logits, lng(ys), None if mask is None else torch.from_numpy(mask.astype(np.float64)))
    dist = torch.sqrt(((x - torch.from_numpy(ori.astype(np.float64))) ** 2).sum())
    (dist + cs * score).backward()
    return d.grad.numpy()


@pytest.mark.parametrize("masked", [False, True])
def test_gradient_into_adam_is_float64_autograd(cpu_case, monkeypatch, masked):
    """At a moved state (delta != 0) of the 8192-point cloud: coord_grad64 fed by the float64 stages (feature path +
    position branch, rla_coord_ref64's composition) IS autograd of |xyz - ori|_2 + cs * hinge w.r.t. delta, to 1e-12 of the
    maximum; the feature path alone fails the same assertion."""
    monkeypatch.setattr(R64, "SLOPE", 0.2)
    _, cases = cpu_case
    c = cases[8192]
    n, cs, ori_cls, target = 8192, 100.0, 3, 9
    params = randla_params(3)
    P = R64.fold_all(params, rounded=False)
    labels = np.asarray(c["labels"])
    mask = (labels == ori_cls) if masked else None
    ys = np.where(labels == ori_cls, target, labels) if masked else labels
    ori = c["xyz"]
    delta = (0.01 * np.random.default_rng(4).standard_normal((n, 3))).astype(np.float32)
    xyz, dist2 = F.apply32(ori, delta, mask)                 # float32 positions: exact inputs of both sides
    delta_eff = (xyz.astype(np.float64) - ori.astype(np.float64))
    geo = R64.geometry(xyz, c["geo"]["neigh"], c["geo"]["up"])
    fwd, _ = R64.walk_forward(P, np.concatenate([xyz, c["rgb"]], 1), geo)
    dl = R64.colper_dlogits(fwd[("logits", 0)], ys)
    if masked:
        dl = dl * mask[:, None]
    bwd, _ = R64.walk_backward(P, fwd, dl, geo)
    taps, _ = C.walk_xyz(P, fwd, bwd, geo)
    dfeat3, dxyz = bwd[("dfeatures", 0)][:, :3], taps[("dxyz", 0)]
    d2 = (delta_eff ** 2).sum()
    got, _ = F.coord_grad64(ori, xyz, dfeat3, dxyz, d2, cs, mask)
    # autograd w.r.t. delta at the point where ori + mask * delta = xyz exactly (delta_eff is a sum of two floats)
    want = autograd_field(params, dict(c, xyz=xyz), ori, delta_eff, ys, mask, cs)
    top = np.abs(want).max()
    assert top > 0 and np.abs(got - want).max() <= 1e-12 * top
    if masked:
        assert not got[~mask].any() and not want[~mask].any()
    feat_only, _ = F.coord_grad64(ori, xyz, dfeat3, dxyz, d2, cs, mask, mutant="no_dxyz")
    assert not np.abs(feat_only - want).max() <= 1e-12 * top


# ---------------------------------------------------------------------------------------------------- lockstep control flow
def scripted(G, n, mode, exits, seed=5):
    """Scripted networks.  Cloud g's prediction is "nothing fires" before evaluation exits[g] and "fires" from it on (None:
    never); the gradients depend on the evaluation index, the cloud and the positions they are taken at."""
    rng = np.random.default_rng(seed)
    labels = rng.integers(0, 13, (G, n)).astype(np.int32)
    if mode == 1:
        labels[:, :40] = 3
        mask = labels == 3
        ys = np.where(mask, 9, labels).astype(np.int32)
    else:
        mask, ys = None, labels
    feat0 = rng.random((G, n, 6), dtype=np.float32)

    def pred_fn(e, g, feat_g):
        fires = exits[g] is not None and e >= exits[g]
        if mode == 0:
            return ((labels[g] + 1) % 13 if fires else labels[g]).astype(np.int32)
        return (ys[g] if fires else labels[g]).astype(np.int32)

    def grad_fn(e, g, feat_g):
        s = np.sin(37.0 * feat_g[:, 0:3].astype(np.float64) + e + 3 * g)
        dfeat = np.zeros((n, 6), np.float32)
        dfeat[:, 0:3] = (0.01 * s).astype(np.float32)
        return dfeat, (0.02 * np.cos(11.0 * feat_g[:, 0:3].astype(np.float64) - e)).astype(np.float32)

    return feat0, labels, ys, mask, pred_fn, grad_fn


# cap 12 in windows of 5: [1..5] latches evaluations 0..4, [6..10] 5..9, [11..12] 10, 11 and the tail 12
EXITS = [1, 3, 4, 5, 12, None]          # evaluation 1, mid-window, a window's last step, the next window's first, the tail, never


@pytest.mark.parametrize("mode", [0, 1])
def test_lockstep_equals_the_plain_per_cloud_loop(mode):
    G, n, cap, chunk, cs, lr = len(EXITS), 130, 12, 5, 0.5, 0.01
    num, den = (1, 13) if mode == 0 else (19, 20)
    feat0, labels, ys, mask, pred_fn, grad_fn = scripted(G, n, mode, EXITS)
    st, hist, (delta, m, v), steps = F.lockstep(feat0, pred_fn, grad_fn, labels, ys, mask, mode, num, den, cap, cs, lr, chunk)
    assert st["exit_step"].tolist() == [-1 if e is None else e for e in EXITS]
    assert steps.tolist() == [cap if e is None else e for e in EXITS]
    assert len(hist) == cap + 1
    for g in range(G):
        p = F.plain_loop(g, feat0[g], pred_fn, grad_fn, labels[g], ys[g], None if mask is None else mask[g], mode, cap, cs, lr)
        assert p["exit_step"] == st["exit_step"][g], g
        last = p["exit_step"] if p["exit_step"] >= 0 else cap
        same = lambda a, b: np.array_equal(np.ascontiguousarray(a).view(np.uint32), np.ascontiguousarray(b).view(np.uint32))    # noqa: E731
        assert same(st["out_adv_xyz"][g], p["xyz"]) and np.array_equal(st["out_pred"][g], p["pred"]), g
        assert same(st["out_stats"][g], p["rows"][last]), g
        assert same(st["out_adv"][g], feat0[g][:, 3:6])
        for e in range(1, last + 1):                       # the rows of the evaluations the plain loop makes
            assert same(hist[e][g], p["rows"][e]), (g, e)
        assert np.isnan(hist[last + 1:, g]).all()          # frozen afterwards: no row is written
        for name, a, b in (("delta", delta[g], p["delta"]), ("m", m[g], p["m"]), ("v", v[g], p["v"])):
            assert same(a, b), (g, name)
        if mask is not None:
            assert same(st["out_adv_xyz"][g][~mask[g]], feat0[g][:, 0:3][~mask[g]])


@pytest.mark.parametrize("mutant", F.LOCKSTEP_MUTANTS)
def test_lockstep_mutants_are_caught(mutant):
    G, n, cap, chunk, cs, lr = len(EXITS), 130, 12, 5, 0.5, 0.01
    feat0, labels, ys, mask, pred_fn, grad_fn = scripted(G, n, 0, EXITS)
    spec = F.lockstep(feat0, pred_fn, grad_fn, labels, ys, mask, 0, 1, 13, cap, cs, lr, chunk)
    mut = F.lockstep(feat0, pred_fn, grad_fn, labels, ys, mask, 0, 1, 13, cap, cs, lr, chunk, mutant=mutant)
    if mutant == "eval_off_by_one":
        assert mut[0]["exit_step"].tolist() != spec[0]["exit_step"].tolist()
    elif mutant == "frozen_still_steps":
        assert mut[0]["exit_step"].tolist() == spec[0]["exit_step"].tolist()
        assert not np.array_equal(mut[2][0][0], spec[2][0][0])                 # cloud 0 left at evaluation 1 and went on moving
        assert np.array_equal(mut[2][0][5], spec[2][0][5])                     # the cloud that never leaves is the same
    else:
        assert mut[0]["exit_step"][4] == -1 and spec[0]["exit_step"][4] == cap
        assert not mut[0]["out_adv_xyz"][5].any() and spec[0]["out_adv_xyz"][5].any()      # no snapshot at the cap


def test_latch_rows_and_position_snapshot():
    """the 4-column row and the position snapshot on top of rla_nu_ref.latch; dist2_rgb None (the "coord" field) is 0"""
    G, n = 2, 26
    labels = np.tile(np.arange(n) % 13, (G, 1)).astype(np.int32)
    pred = (labels + 1) % 13
    pred[0, :2] = labels[0, :2]
    pred[1, :1] = labels[1, :1]
    z = np.zeros((G, n, 13), np.float32)
    np.put_along_axis(z, pred[..., None].astype(np.int64), 1.0, -1)
    feat = np.random.default_rng(0).random((G, n, 6), dtype=np.float32)
    d_xyz, d_rgb = np.array([0.25, 0.5], np.float32), np.array([2.0, 3.0], np.float32)
    st, row = F.new_state(G, n), np.zeros((G, 4), np.float32)
    F.latch(st, row, z, labels, labels, None, None, feat, None, d_xyz, 0, 1, 13, 1, 1, 0)
    assert row.tolist() == [[2, 0, 0, 0.25], [1, 0, 0, 0.5]] and st["exit_step"].tolist() == [-1, 1]
    assert np.array_equal(st["out_adv_xyz"][1], feat[1][:, 0:3]) and np.array_equal(st["out_adv"][1], feat[1][:, 3:6])
    assert not st["out_adv_xyz"][0].any() and st["out_stats"].tolist() == [[0, 0, 0, 0], [1, 0, 0, 0.5]]
    row2 = np.full((G, 4), -7.0, np.float32)
    F.latch(st, row2, z, labels, labels, None, None, feat + 1, d_rgb, d_xyz, 0, 1, 13, 2, 1, 1)
    assert row2.tolist() == [[2, 0, 2.0, 0.25], [-7, -7, -7, -7]]                    # the frozen cloud gets no row
    assert np.array_equal(st["out_adv_xyz"][0], feat[0][:, 0:3] + 1) and np.array_equal(st["out_adv_xyz"][1], feat[1][:, 0:3])


# ---------------------------------------------------------------------------------------------------- ABI and classes
NEW_SYMBOLS = ("psg_rla_nu_coord_apply_clouds", "psg_rla_nu_coord_adam_clouds", "psg_rla_nu_field_latch_clouds", "psg_rla_nu_field_window")


def test_abi_of_the_new_entry_points():
    from pointsecguard_amd import _lib
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name in NEW_SYMBOLS:
        assert name in _lib.SIGNATURES, name
        assert hasattr(lib, name), name
    # the argument block mirrors psg_rla_nu_field_window_args: 2 handles, 9 ints, 3 floats, 31 pointers, no padding
    A = _lib.RlaNuFieldWindowArgs
    assert ctypes.sizeof(A) == 2 * 8 + 9 * 4 + 3 * 4 + 31 * 8
    assert A.field.offset == 48 and A.cs.offset == 52 and A.xs.offset == 64 and A.exit_step.offset == 64 + 30 * 8
    assert _lib.SIGNATURES["psg_rla_nu_field_window"][1] == [_lib.vp, _lib.vp]          # no graph handle


def test_classes_and_their_host_side_contract():
    from pointsecguard_amd.randla import attack, nu_field
    assert issubclass(nu_field.NUattackField, attack.NUattack) and issubclass(nu_field.tar_NUattackField, attack.tar_NUattack)
    assert nu_field.NUattackField.EXIT_RATIO == (1, 13) and nu_field.tar_NUattackField.EXIT_RATIO == (19, 20)
    assert nu_field.NUattackField.EXIT_MODE == 0 and nu_field.tar_NUattackField.EXIT_MODE == 1
    assert nu_field._FIELD_CODE == {"coord": 1, "both": 2}
    # a bad field is refused before the model is looked at
    for cls in (nu_field.NUattackField, nu_field.tar_NUattackField):
        with pytest.raises(ValueError, match="field"):
            cls(None, field="xyz")
        with pytest.raises(TypeError):
            cls(None)
    # the parents' refusal text names the new classes and still says batch_attack
    assert "batch_attack" in attack._FIELD_ONLY and "nu_field" in attack._FIELD_ONLY
