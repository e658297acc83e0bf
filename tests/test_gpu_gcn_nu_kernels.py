"""The two kernels of the lockstep ResGCN NU loop on their own: psg_gcn_f_loss_grad_rooms against G one-room calls (bit for
bit) and attack_ref64's error model (sums); psg_smooth_knn_sym_rooms against the numpy restatement of tests/gcn_nu_ref.py
(exact inputs: bit for bit; real inputs: lists equal, gradient within the summation bound of the terms both kernels add)
and against the one-room psg_smooth_knn."""
import numpy as np
import pytest
import torch

import attack_ref64 as A
import gcn_nu_ref as R

pytestmark = pytest.mark.gpu
F = np.float32
U = 2.0 ** -24


def lib():
    from pointsecguard_amd import _lib, runtime
    return _lib, runtime.ptr, runtime.stream


def dev(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()


def bits(a):
    return np.ascontiguousarray(a).view(np.uint8)


# ======================================================================================================== f-loss rooms
def _logits(G, N, seed):
    rng = np.random.default_rng(seed)
    z = rng.standard_normal((G, N, 13)).astype(F)
    labels = rng.integers(0, 13, (G, N)).astype(np.int32)
    for g in range(G):
        # rows whose maxima are exact zeros: all classes <= 0 with a 0 in slot 0 / in a slot before the true class / the
        # true class itself at 0 in slot 0 and elsewhere (torch.max's first maximum decides who takes the gradient)
        z[g, 0] = -np.abs(z[g, 0]); z[g, 0, 0] = 0; labels[g, 0] = 5
        z[g, 1] = -np.abs(z[g, 1]); z[g, 1, 3] = 0; labels[g, 1] = 7
        z[g, 2] = -np.abs(z[g, 2]); z[g, 2, 0] = 0; labels[g, 2] = 0
        z[g, 3] = -np.abs(z[g, 3]); z[g, 3, 9] = 0; labels[g, 3] = 9
    masks = rng.random((G, N)) < 0.6
    masks[:, :4] = True
    return z, labels, masks


@pytest.mark.parametrize("mode", [0, 1, 2])
@pytest.mark.parametrize("G,N", [(1, 64), (3, 64), (1, 192), (3, 192)])
def test_f_loss_rooms_equals_one_room_calls(mode, G, N):
    _lib, P, st = lib()
    z, labels, masks = _logits(G, N, 10 * G + N + mode)
    target, kappa, tsign, scale = 4, 0.25, 1.0, 0.37
    for use_mask in ((False, True) if mode == 0 else (True,)):
        mk = masks.astype(np.uint8) if use_mask else None
        zd, ld, md = dev(z), dev(labels), dev(mk)
        dz = torch.full((G, N, 13), float("nan"), device="cuda")
        pred = torch.full((G, N), -1, dtype=torch.int32, device="cuda")
        fs = torch.zeros(G, device="cuda")
        _lib.call("psg_gcn_f_loss_grad_rooms", P(zd), P(ld), target, P(md), mode, G, N, 13, kappa, tsign, scale, P(dz), P(fs), P(pred), st())
        for g in range(G):
            dz1 = torch.full((N, 13), float("nan"), device="cuda")
            p1 = torch.full((N,), -1, dtype=torch.int32, device="cuda")
            f1 = torch.zeros(1, device="cuda")
            _lib.call("psg_gcn_f_loss_grad", P(zd[g]), P(ld[g]), target, P(md[g]) if use_mask else None, mode, N, N, 13, kappa, tsign,
                      scale, P(dz1), P(f1), P(p1), st())
            assert np.array_equal(bits(dz[g].cpu().numpy()), bits(dz1.cpu().numpy())), (mode, g)
            assert np.array_equal(pred[g].cpu().numpy(), p1.cpu().numpy()), (mode, g)
        _, f_ref, pred_ref, _, fe = R.f_loss_rooms(z, labels, target, masks if use_mask else None, mode, kappa, tsign, scale)
        got = fs.cpu().numpy().astype(np.float64)
        print("f sums", got, f_ref, "error / bound", np.abs(got - f_ref) / A.bound(fe))
        assert (np.abs(got - f_ref) <= A.bound(fe)).all()
        assert np.array_equal(pred.cpu().numpy(), pred_ref)


def test_f_loss_rooms_refusals():
    _lib, P, st = lib()
    t, i = torch.zeros(2, 64, 33, device="cuda"), torch.zeros(2, 64, dtype=torch.int32, device="cuda")
    for args in ((3, 13), (0, 33), (0, 1)):                                # mode, n_cls
        with pytest.raises(_lib.PsgError):
            _lib.call("psg_gcn_f_loss_grad_rooms", P(t), P(i), 0, None, args[0], 2, 64, args[1], 0.0, 1.0, 1.0, P(t), P(t), None, st())


# ================================================================================================= symmetric Smooth term
def _sym(col_rooms, nb, active=None, stride=9, nn=True):
    """psg_smooth_knn_sym_rooms on colours [G, N, 3] placed at channel 3 of rows of `stride` floats; NaN / -7 canaries"""
    _lib, P, st = lib()
    from pointsecguard_amd.attacks.torchattacks.attacks.nu import ctypes_off
    G, N, _ = col_rooms.shape
    x0 = np.full((G, N, stride), 0.5, F)
    x0[:, :, 3:6] = col_rooms
    x0 = dev(x0)
    grad = torch.full((G, N, 3), float("nan"), device="cuda")
    dsum = torch.full((G,), float("nan"), device="cuda") if active is not None else torch.zeros(G, device="cuda")
    if active is not None:
        dsum[torch.from_numpy(np.asarray(active, bool)).cuda()] = 0
    nn_out = torch.full((G, N, nb), -7, dtype=torch.int32, device="cuda") if nn else None
    _lib.call("psg_smooth_knn_sym_rooms", ctypes_off(x0, 3), stride, N * stride, G, N, nb, P(dsum), P(grad),
              P(dev(np.asarray(active, np.uint8))) if active is not None else None, P(nn_out), st())
    return grad.cpu().numpy(), dsum.cpu().numpy(), nn_out.cpu().numpy() if nn else None


def _one_room(col, nb):
    """the one-room entry point in symmetric mode (float atomics: the order of a sum is whatever the run gave)"""
    _lib, P, st = lib()
    c = dev(np.ascontiguousarray(col, F))
    grad, dsum = torch.empty(len(col), 3, device="cuda"), torch.zeros(1, device="cuda")
    _lib.call("psg_smooth_knn", P(c), 3, P(c), 3, len(col), nb, P(dsum), P(grad), st())
    return grad.cpu().numpy(), float(dsum.item())


def _line(ks):
    """colours on a line: x = k / 64, y and z constant dyadic values - every product, d^2, root and u = +-1 is exact"""
    col = np.empty((len(ks), 3), F)
    col[:, 0] = np.asarray(ks, F) / F(64)
    col[:, 1], col[:, 2] = F(0.25), F(0.5)
    return col


@pytest.mark.parametrize("nb", [5, 10])
def test_sym_smooth_exact_on_a_line(nb):
    rng = np.random.default_rng(nb)
    ks = np.concatenate([np.arange(0, 40), [3, 3, 17, 39, 39], rng.choice(np.arange(41, 64), 11, replace=False)])   # equal spacings, duplicates
    ks = ks[rng.permutation(len(ks))]
    col = _line(ks)
    nn_ref, g_ref, s_ref, u = R.smooth_sym(col, nb)
    assert np.array_equal(g_ref, np.round(g_ref)) and set(np.unique(np.abs(u))) <= {0.0, 1.0}            # integers: the exact case
    # the selection from exact integers: |k - k'| then the index
    want = np.array([sorted(range(len(ks)), key=lambda j: (abs(int(ks[i]) - int(ks[j])), j))[:nb] for i in range(len(ks))])
    assert np.array_equal(nn_ref, want)
    assert (np.abs(ks[want][:, :-1] - ks[:, None]) == np.abs(ks[want][:, 1:] - ks[:, None])).any()      # distance ties are in the lists
    grad, dsum, nn = _sym(col[None], nb)
    assert np.array_equal(nn[0], want)
    assert np.array_equal(bits(grad[0]), bits(g_ref))
    assert float(dsum[0]) == s_ref                                              # sixty-fourths: every partial sum is exact
    # (the one-room kernel can order references at exactly the same distance differently inside a lane's list - see
    # smooth_knn_kernel; sums of +-1 do not depend on the order)
    g1, s1 = _one_room(col, nb)
    assert np.array_equal(bits(grad[0]), bits(g1)) and s1 == s_ref
    dup = np.array([(ks == k).sum() > 1 for k in ks])
    zero_terms = (np.take_along_axis(R.dist2(col), want, 1) == 0)
    assert zero_terms[dup].sum() > dup.sum() and (u[zero_terms] == 0).all()    # duplicates are neighbours at d = 0: exactly zero


@pytest.mark.parametrize("N,nb,G", [(100, 5, 1), (100, 10, 3), (100, 16, 3), (1024, 5, 3), (1024, 10, 1), (1024, 16, 1), (3, 5, 3),
                                    (3, 16, 1)])
def test_sym_smooth_real_inputs(N, nb, G):
    rng = np.random.default_rng(1000 * G + N + nb)
    col = rng.random((G, N, 3)).astype(F)
    grad, dsum, nn = _sym(col, nb)
    grad2, _, _ = _sym(col, nb)
    assert np.array_equal(bits(grad), bits(grad2))                              # no atomics on the gradient: run to run
    cnt = min(nb, N)
    for g in range(G):
        nn_ref, g_ref, s_ref, u = R.smooth_sym(col[g], nb)
        assert np.array_equal(nn[g][:, :cnt], nn_ref) and (nn[g][:, cnt:] == -7).all()
        assert np.array_equal(bits(grad[g]), bits(g_ref))                       # the restatement's order is the kernel's
        g1, s1 = _one_room(col[g], nb)
        n_i, s_abs = R.in_degree_terms(nn_ref, u)
        bound = 2 * (n_i - 1)[:, None] * U * s_abs
        err = np.abs(grad[g].astype(np.float64) - g1.astype(np.float64))
        print("N %d nb %d room %d: worst |diff| / bound %.3f" % (N, nb, g, float((err / np.maximum(bound, 1e-300)).max())))
        assert (err <= bound).all()
        assert abs(float(dsum[g]) - s_ref) <= 2 * (N * nb - 1) * U * s_ref
    if G > 1:                                                                   # a room inside the launch = the room alone
        alone, s_alone, nn_alone = _sym(col[1:2], nb)
        assert np.array_equal(bits(alone[0]), bits(grad[1])) and np.array_equal(nn_alone[0], nn[1])


def test_sym_smooth_without_lists_and_on_plain_rows():
    col = np.random.default_rng(5).random((2, 200, 3)).astype(F)
    a, sa, _ = _sym(col, 10)
    b, sb, none = _sym(col, 10, nn=False)
    assert none is None and np.array_equal(bits(a), bits(b))
    _lib, P, st = lib()
    c = dev(col)
    grad, dsum = torch.empty(2, 200, 3, device="cuda"), torch.zeros(2, device="cuda")
    _lib.call("psg_smooth_knn_sym_rooms", P(c), 3, 600, 2, 200, 10, P(dsum), P(grad), None, None, st())
    assert np.array_equal(bits(grad.cpu().numpy()), bits(a))


def test_sym_smooth_inactive_room_is_untouched():
    col = np.random.default_rng(6).random((3, 130, 3)).astype(F)
    grad, dsum, nn = _sym(col, 5, active=[1, 0, 1])
    assert np.isnan(grad[1]).all() and np.isnan(dsum[1]) and (nn[1] == -7).all()
    ref, sref, nref = _sym(col, 5)
    for g in (0, 2):
        assert np.array_equal(bits(grad[g]), bits(ref[g])) and np.array_equal(nn[g], nref[g])
        assert abs(dsum[g] - sref[g]) <= 2 * (130 * 5 - 1) * U * sref[g]


def test_sym_smooth_refusals():
    _lib, P, st = lib()
    t = torch.zeros(8193 * 3, device="cuda")
    for N, nb in ((64, 0), (64, 17), (8193, 5)):
        with pytest.raises(_lib.PsgError):
            _lib.call("psg_smooth_knn_sym_rooms", P(t), 3, N * 3, 1, N, nb, P(t), P(t), None, None, st())
