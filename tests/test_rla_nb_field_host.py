"""Host tests of the lockstep BIM family of RandLA-Net on the coordinate field: the numpy restatement of the lockstep field loop
(tests/rla_nb_field_ref.py) against a plain per-cloud loop with TBIM.batch_attack's field control flow on scripted networks, the
mutants that restatement must tell apart, mode 0 against plain field steps, a float32 emulation of the batched l_2 step against
the float64 bound of the one-cloud step, and the new module and C ABI."""
import ctypes

import numpy as np
import pytest

import rla_coord_ref64 as C
import rla_nb_field_ref as F
import rla_tbim_ref as R

N, NM, TARGET, ORI = 20, 10, 7, 2        # 10 masked points: 9 hits are ON 9/10, 10 are above


def scripted(hits, iteration, seed=0):
    """G = len(hits) clouds; hits[g][it] of cloud g's 10 origin points are predicted as the target in iteration it.  The
    gradients of iteration it are fixed random fields (so every update moves positions and colours and differs from every
    other), dxyz as large as dfeat's position columns: dropping it changes every step."""
    G = len(hits)
    rng = np.random.default_rng(seed)
    labels = np.tile(np.r_[np.full(NM, ORI), 3 + np.arange(N - NM) % 3].astype(np.int32), (G, 1))
    mask = (labels == ORI).astype(np.uint8)
    hit_ys = np.where(mask.astype(bool), TARGET, labels).astype(np.int32)
    feat0 = (0.25 + 0.5 * rng.random((G, N, 6))).astype(np.float32)
    grads = rng.standard_normal((iteration + 1, G, N, 6)).astype(np.float32)
    gxyz = rng.standard_normal((iteration + 1, G, N, 3)).astype(np.float32)

    def pred_fn(it, feat):
        p = labels.copy()
        for g in range(G):
            p[g, :hits[g][it]] = TARGET
        return p

    def grad_fn(it, feat):
        return grads[it], gxyz[it]

    return dict(feat0=feat0, pred_fn=pred_fn, grad_fn=grad_fn, labels=labels, hit_ys=hit_ys, mask=mask, iteration=iteration)


def per_cloud(case, g, **kw):
    def grad_g(it, f):
        dfeat, dxyz = case["grad_fn"](it, None)
        return dfeat[g], dxyz[g]
    return F.host_loop(case["feat0"][g], lambda it, f: case["pred_fn"](it, None)[g], grad_g, case["hit_ys"][g], case["mask"][g],
                       case["iteration"], **kw)


def agrees(case, **mut):
    """Does the (possibly mutated) lockstep loop give every cloud what the per-cloud loop gives it alone: the snapshot's
    prediction, positions and colours, the steps, and the features it is left with?"""
    kw = {k: mut.pop(k) for k in ("l2_metric", "chunk", "field") if k in mut}
    st, hist, feat, steps = F.lockstep(**case, **kw, **mut)
    ok = True
    for g in range(case["labels"].shape[0]):
        pred, xyz, rgb, n_steps = per_cloud(case, g, **{k: v for k, v in kw.items() if k != "chunk"})
        ok &= np.array_equal(st["out_pred"][g], pred) and np.array_equal(st["out_adv_xyz"][g], xyz) and steps[g] == n_steps
        ok &= np.array_equal(st["out_adv"][g], rgb) and np.array_equal(feat[g][:, 0:3], xyz) and np.array_equal(feat[g][:, 3:6], rgb)
    return bool(ok), st, hist, steps


CAP = 5
SCENARIOS = {
    "exit at it = 1": [[0, 10, 10, 10, 10, 10]],
    "a would-be exit at it = 0": [[10, 4, 5, 10, 10, 10]],
    "exit exactly at the cap": [[0, 1, 2, 3, 9, 10]],
    "no exit": [[0, 1, 2, 3, 9, 9]],
    "on the threshold, then above": [[0, 9, 9, 10, 10, 10]],
    "clouds leaving at different iterations": [[0, 3, 10, 0, 0, 0], [0, 10, 0, 0, 0, 0], [10, 9, 9, 9, 10, 10], [0, 0, 0, 0, 0, 0]],
}
WANT_EXIT = {"exit at it = 1": [1], "a would-be exit at it = 0": [3], "exit exactly at the cap": [5], "no exit": [-1],
             "on the threshold, then above": [3], "clouds leaving at different iterations": [2, 1, 4, -1]}


@pytest.mark.parametrize("field", ["coord", "both"])
@pytest.mark.parametrize("l2_metric", [0, 1])
@pytest.mark.parametrize("chunk", [1, 2, 10])
@pytest.mark.parametrize("name", list(SCENARIOS))
def test_lockstep_reproduces_the_per_cloud_loop(name, chunk, l2_metric, field):
    case = scripted(SCENARIOS[name], CAP)
    ok, st, hist, steps = agrees(case, chunk=chunk, l2_metric=l2_metric, field=field)
    assert ok, name
    assert st["exit_step"].tolist() == WANT_EXIT[name]
    assert steps.tolist() == [e + 1 if e >= 0 else CAP + 1 for e in WANT_EXIT[name]]
    assert not st["active"].any() and not st["leaving"].any()
    for g, h in enumerate(SCENARIOS[name]):
        for it in range(hist.shape[0]):                  # the rows of the forward before each update; a retired cloud's stay zero
            assert hist[it, g, 1] == (h[it] if it < steps[g] else 0), (g, it)
        assert st["out_stats"][g, 1] == h[steps[g] - 1]
        moved = not np.array_equal(st["out_adv"][g], case["feat0"][g][:, 3:6])
        assert moved == (field == "both")               # colours keep their bytes under "coord"
        assert not np.array_equal(st["out_adv_xyz"][g], case["feat0"][g][:, 0:3])


MUTANTS = {"positions snapshot before the update": dict(snapshot_xyz="before"),
           "update withheld from the leaving cloud": dict(update_leaving=False),
           "a retired cloud still stepping": dict(freeze_retired=False),
           "dxyz dropped from the gradient": dict(use_dxyz=False)}
MADE_FOR = {"positions snapshot before the update": "exit at it = 1", "update withheld from the leaving cloud": "exit at it = 1",
            "a retired cloud still stepping": "clouds leaving at different iterations", "dxyz dropped from the gradient": "no exit"}


@pytest.mark.parametrize("l2_metric", [0, 1])
@pytest.mark.parametrize("mutant", list(MUTANTS))
def test_mutants_are_caught(mutant, l2_metric):
    caught = [name for name in SCENARIOS if not agrees(scripted(SCENARIOS[name], CAP), l2_metric=l2_metric, **MUTANTS[mutant])[0]]
    print(mutant, "caught by", caught)
    assert MADE_FOR[mutant] in caught, mutant


@pytest.mark.parametrize("field", ["coord", "both"])
@pytest.mark.parametrize("l2_metric", [0, 1])
@pytest.mark.parametrize("chunk", [1, 2, 10])
def test_mode_0_is_iteration_plus_one_plain_steps(chunk, l2_metric, field):
    case = scripted(SCENARIOS["clouds leaving at different iterations"], CAP)
    xyz, rgb, active = F.lockstep_bim(case["feat0"], case["grad_fn"], CAP, field=field, l2_metric=l2_metric, chunk=chunk)
    feat0 = case["feat0"]
    for g in range(feat0.shape[0]):
        f = feat0[g].copy()
        for it in range(CAP + 1):
            dfeat, dxyz = case["grad_fn"](it, None)
            f[:, 0:3] = C.field_step(f[:, 0:3], dfeat[g][:, 0:3] + dxyz[g], feat0[g][:, 0:3], 0.3, 0.02, F.METRIC[l2_metric])
            if field == "both":
                R.bim_step(f[None], dfeat[g][None], feat0[g][None, :, 3:6], None, 0.5, 0.01, l2_metric)
        assert np.array_equal(xyz[g], f[:, 0:3]) and np.array_equal(rgb[g], f[:, 3:6]), g
        assert not np.array_equal(xyz[g], feat0[g][:, 0:3])
    assert not active.any()


@pytest.mark.parametrize("n", [1, 63, 1000])
def test_batched_l2_step_uses_each_clouds_own_norms(n):
    """Three clouds with gradients a factor of ten apart each (their norms differ by as much), one inside the eps ball, one an
    all-zero gradient half an eps out, one clipped: the float32 emulation of the batched step lies within
    rla_coord_ref64.field_step_l2_bound of the float64 step of every cloud alone; with cloud 0's norms for all it does not."""
    G, eps, alpha = 3, 0.05, 0.01
    rng = np.random.default_rng(n)
    ori = (rng.random((G, n, 3)) * 4).astype(np.float32)
    adv = ori.copy()
    adv[1] += np.float32(0.5 * eps / np.sqrt(3 * n))
    adv[2] += np.float32(2.0 * eps / np.sqrt(3 * n))
    g = (rng.standard_normal((G, n, 3)) * np.array([1.0, 0.0, 100.0])[:, None, None]).astype(np.float32)
    got, norms = F.field_step_l2_f32(adv, g, ori, eps, alpha)
    mutant, _ = F.field_step_l2_f32(adv, g, ori, eps, alpha, shared_norms=True)
    assert norms[0][1] == 0.0 and np.sqrt(norms[1][0]) < eps and np.sqrt(norms[1][1]) < eps and np.sqrt(norms[1][2]) > eps
    off = False
    for c in range(G):
        ref, bound = C.field_step_l2_bound(adv[c], g[c], ori[c], np.float64(np.float32(eps)), np.float64(np.float32(alpha)))
        err = np.abs(got[c].astype(np.float64) - ref)
        print("n", n, "cloud", c, "largest error / bound", float((err / np.maximum(bound, 1e-300)).max()))
        assert (err <= bound).all(), c
        # the one-cloud float32 step states the same arithmetic
        assert np.array_equal(got[c], C.field_step(adv[c], g[c], ori[c], eps, alpha, "l_2")), c
        off |= bool((np.abs(mutant[c].astype(np.float64) - ref) > bound).any())
    assert off


NEW_SYMBOLS = ("psg_rla_bim_step_field_clouds", "psg_rla_tbim_retire_field_clouds", "psg_rla_bim_field_window")


def test_abi_of_the_new_entry_points():
    from pointsecguard_amd import _lib
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name in NEW_SYMBOLS:
        assert name in _lib.SIGNATURES, name
        assert hasattr(lib, name), name
    # the argument block mirrors psg_rla_bim_field_window_args: 2 handles, 10 ints, 5 floats, 4 bytes of padding, 26 pointers
    A = _lib.RlaBimFieldWindowArgs
    assert ctypes.sizeof(A) == 2 * 8 + 10 * 4 + 5 * 4 + 4 + 26 * 8
    assert A.eps.offset == 56 and A.ori.offset == 80 and A.out_adv_xyz.offset == 80 + 25 * 8
    assert _lib.SIGNATURES["psg_rla_bim_field_window"][1] == [_lib.vp, _lib.vp]          # no graph handle


def test_module_and_classes():
    from pointsecguard_amd.randla import attack, nb_field
    for cls, parent in ((nb_field.BIMField, attack.BIM), (nb_field.NBattackField, attack.NBattack), (nb_field.TBIMField, attack.TBIM),
                        (nb_field.tar_NBattackField, attack.tar_NBattack)):
        assert issubclass(cls, parent) and callable(cls.batch_attack_clouds)
        assert cls.batch_attack is parent.batch_attack                   # the one-cloud host loop, inherited untouched
        assert cls.chunk == attack.CHUNK and cls.window_hook is None
    assert nb_field.TBIMField.EXIT_RATIO == (9, 10)
    assert nb_field.TBIMField.batch_attack_clouds is not attack.TBIM.batch_attack_clouds
