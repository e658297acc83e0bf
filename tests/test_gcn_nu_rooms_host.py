"""CPU side of the lockstep ResGCN NU attacks: the numpy restatement of the symmetric Smooth term (tests/gcn_nu_ref.py)
pinned to float64 autograd, its teeth, the per-room f-loss reference, and the refusals of forward_rooms (no GPU)."""
import numpy as np
import pytest
import torch

import attack_ref64 as A
import gcn_nu_ref as R

F = np.float32
U = 2.0 ** -24


def _separated_colours(N, nb, seed):
    """random colours whose ranks nb and nb + 1 are further apart than the expansion's noise (asserted)"""
    col = np.random.default_rng(seed).random((N, 3)).astype(F)
    c = col.astype(np.float64)
    d2 = ((c[:, None] - c[None]) ** 2).sum(-1)
    srt = np.sort(d2, 1)
    q = (c ** 2).sum(1)
    # five float32 operations on partial results no larger than 2 (|a|^2 + |r|^2)
    noise = 10 * U * (q[:, None] + q[None]).max()
    assert (srt[:, nb] - srt[:, nb - 1] > 4 * noise).all() and (srt[:, 1] > 4 * noise).all()
    return col, noise


def _autograd64(col, nb):
    """sum of the nb smallest sqrt distances of adv against itself, both sides differentiable (the self pair is the
    constant 0: its root has no gradient)"""
    a = torch.from_numpy(col.astype(np.float64)).requires_grad_(True)
    d2 = ((a[:, None] - a[None]) ** 2).sum(-1)
    idx = torch.topk(d2.detach(), nb, dim=1, largest=False).indices
    sel = torch.gather(d2, 1, idx)
    pair = idx != torch.arange(len(col))[:, None]
    loss = torch.sqrt(sel[pair]).sum()
    loss.backward()
    return idx.numpy(), a.grad.numpy(), float(loss.detach())


@pytest.mark.parametrize("N,nb", [(60, 5), (40, 10)])
def test_restatement_against_float64_autograd(N, nb):
    col, noise = _separated_colours(N, nb, N + nb)
    nn, grad, total, u = R.smooth_sym(col, nb)
    idx64, g64, loss64 = _autograd64(col, nb)
    assert np.array_equal(np.sort(nn, 1), np.sort(idx64, 1))
    # a term u = (a - r) / d: d comes from d^2 with the expansion's absolute noise, the difference and the quotient add 2 u
    d2 = np.take_along_axis(R.dist2(col).astype(np.float64), nn.astype(np.int64), 1)
    with np.errstate(divide="ignore"):
        rel = np.where(d2 > 0, noise / (2 * d2) + 4 * U, 0.0)
    term_err = np.abs(u).astype(np.float64) * rel[:, :, None]
    n_i, s_abs = R.in_degree_terms(nn, u)
    bound = term_err.sum(1)
    for k in range(N):
        bound[nn[k]] += term_err[k]
    bound += n_i[:, None] * U * s_abs
    err = np.abs(grad.astype(np.float64) - g64)
    print("worst error / bound %.3f" % float((err / bound).max()))
    assert (err <= bound).all()
    assert abs(total - loss64) <= (np.sqrt(d2) * rel).sum() + N * nb * U * loss64
    for mutant in ("one_sided",):
        _, gm, _, _ = R.smooth_sym(col, nb, mutant=mutant)
        assert (np.abs(gm.astype(np.float64) - g64) > bound).any(), mutant


def test_tie_order_mutant_fails_on_a_line():
    ks = np.arange(24)
    col = np.stack([ks.astype(F) / F(64), np.full(24, 0.25, F), np.full(24, 0.5, F)], 1)
    want = np.array([sorted(range(24), key=lambda j: (abs(i - j), j))[:4] for i in range(24)])
    nn, grad, _, _ = R.smooth_sym(col, 4)
    assert np.array_equal(nn, want)
    nn_m, grad_m, _, _ = R.smooth_sym(col, 4, mutant="tie_high")
    assert not np.array_equal(nn_m, want) and not np.array_equal(grad_m, grad)
    # an interior point's pulls cancel; the lower index wins rank 3, so the pull towards i - 2 is the unpaired one
    assert np.array_equal(grad, np.round(grad))


def test_f_loss_rooms_reference_is_the_one_room_reference_per_room():
    rng = np.random.default_rng(0)
    z = rng.standard_normal((3, 70, 13)).astype(F)
    labels = rng.integers(0, 13, (3, 70))
    masks = rng.random((3, 70)) < 0.5
    dz, f, pred, e, fe = R.f_loss_rooms(z, labels, 4, masks, 1, 0.0, 1.0, 0.5)
    one = A.gcn_f_loss_grad(z[1], labels[1], 4, masks[1], 1, 70, 0.0, 1.0, 0.5)
    assert np.array_equal(dz[1], one[0]) and f[1] == one[1] and np.array_equal(pred[1], one[2])
    assert (dz[1][~masks[1]] == 0).all() and fe.shape[1] == 3


class _FakeGCN(torch.nn.Module):
    """passes attacks.colper._gcn without a GPU: forward_rooms must refuse before it touches the device"""
    n_blocks = 5

    def __init__(self):
        super().__init__()
        self.p = torch.nn.Parameter(torch.zeros(1))

    def _packed(self):
        raise AssertionError("the refusal must come before the model is packed")


def test_forward_rooms_refusals():
    from pointsecguard_amd.resgcn.sem_seg_dense.attacks import torchattacks
    x, y = torch.zeros(2, 9, 64, 1), torch.zeros(2, 64, dtype=torch.int64)
    with pytest.raises(TypeError):
        torchattacks.NU_attack(torch.nn.Linear(2, 2)).forward_rooms(x, y)
    with pytest.raises(TypeError):
        torchattacks.tar_NU_attack(torch.nn.Linear(2, 2), target=3).forward_rooms(x, y, np.ones((2, 64), bool))
    atk = torchattacks.tar_NU_attack(_FakeGCN(), target=3, lr=0.25)
    with pytest.raises(ValueError):
        atk.forward_rooms(x, y, None)
    for bad in (np.ones(64, bool), np.ones((1, 64), bool), np.ones((2, 63), bool)):
        with pytest.raises(ValueError):
            atk.forward_rooms(x, y, bad)
    empty = np.ones((2, 64), bool)
    empty[1] = False
    with pytest.raises(ZeroDivisionError):
        atk.forward_rooms(x, y, empty)
    with pytest.raises(ValueError):
        torchattacks.NU_attack(_FakeGCN()).forward_rooms(torch.zeros(2, 9, 64), y)
    assert atk.lr == 0.25
