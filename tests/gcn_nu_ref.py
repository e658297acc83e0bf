"""Plain references for the lockstep ResGCN NU kernels (psg_smooth_knn_sym_rooms, psg_gcn_f_loss_grad_rooms).

TEST INFRASTRUCTURE ONLY: no GPU, no oracle import.

smooth_sym: a numpy float32 restatement of smooth(adv, adv) (colper.py:115-120) with the kernel's expression, one IEEE
operation per line, and the kernel's fixed summation order:
  d^2(k, i) = max((fma(-2 z_k, z_i, fma(-2 y_k, y_i, (-2 x_k) x_i)) + |a_k|^2) + |a_i|^2, 0),  |a|^2 = (x x + y y) + z z
  neighbours of k: the nb smallest by (d^2, index);  u(k, j) = (a_k - a_j) / sqrt(d^2), exactly zero where d == 0
  grad[i] = ((0 + u(i, j_0)) + u(i, j_1)) + ..   own terms in ascending rank
            - u(k_0, i) - u(k_1, i) - ..          then the terms received as a neighbour, in ascending k
The fused multiply-add is evaluated in the platform's extended precision (64-bit mantissa: the 48-bit product is exact, the
sum is rounded once to 64 bits and once more to 24: the two roundings differ from one only when the 64-bit sum lies within
2^-40 of a float32 tie).
"""
import numpy as np

import attack_ref64

F = np.float32
LD = np.longdouble
assert np.finfo(LD).nmant >= 63, "gcn_nu_ref needs an extended-precision long double for its fma"


def fma32(a, b, c):
    return (a.astype(LD) * b.astype(LD) + c.astype(LD)).astype(F)


def sq_norm(col):
    x, y, z = col[:, 0], col[:, 1], col[:, 2]
    return (x * x + y * y) + z * z


def dist2(col):
    """d^2[k, i] with k in the query's role (the expansion is not symmetric in float32)"""
    col = np.ascontiguousarray(col, F)
    q = sq_norm(col)
    m2 = F(-2.0) * col
    x, y, z = col[:, 0][None], col[:, 1][None], col[:, 2][None]
    d2 = fma32(m2[:, 2:3], z, fma32(m2[:, 1:2], y, m2[:, 0:1] * x))
    d2 = (d2 + q[:, None]) + q[None]
    return np.maximum(d2, F(0))


def smooth_sym(col, nb, mutant=None):
    """(nn [N, min(nb, N)] int32, grad [N, 3] float32, sum of the selected distances float64, terms u [N, cnt, 3] float32)"""
    col = np.ascontiguousarray(col, F)
    N = len(col)
    cnt = min(nb, N)
    d2 = dist2(col)
    if mutant == "tie_high":                    # equal distances resolved to the HIGHER index
        nn = (N - 1 - np.argsort(d2[:, ::-1], axis=1, kind="stable")[:, :cnt]).astype(np.int32)
    else:
        nn = np.argsort(d2, axis=1, kind="stable")[:, :cnt].astype(np.int32)
    d = np.sqrt(np.take_along_axis(d2, nn.astype(np.int64), 1))
    with np.errstate(divide="ignore", invalid="ignore"):
        u = (col[:, None, :] - col[nn]) / d[:, :, None]
    u = np.where(d[:, :, None] > 0, u, F(0)).astype(F)
    grad = np.zeros((N, 3), F)
    for t in range(cnt):
        grad = grad + u[:, t]
    if mutant != "one_sided":
        for k in range(N):                      # ascending source index; the neighbours of one k are distinct
            grad[nn[k]] = grad[nn[k]] - u[k]
    return nn, grad, float(d.astype(np.float64).sum()), u


def in_degree_terms(nn, u):
    """per colour and component: n_i = own non-zero terms + in-degree (every k that holds i), and sum |t| over those terms"""
    N = len(nn)
    n = (np.abs(u).max(2) > 0).sum(1).astype(np.int64)
    s = np.abs(u).astype(np.float64).sum(1)
    for k in range(N):
        n[nn[k]] += 1
        s[nn[k]] += np.abs(u[k]).astype(np.float64)
    return n, s


def f_loss_rooms(z, labels, target, masks, mode, kappa, tsign, scale):
    """attack_ref64.gcn_f_loss_grad room by room: z [G, N, C] -> (dz [G, N, C], f [G], pred [G, N], dz error parts, f error parts [G])"""
    outs = [attack_ref64.gcn_f_loss_grad(z[g], None if labels is None else labels[g], target, None if masks is None else masks[g],
                                         mode, z.shape[1], kappa, tsign, scale) for g in range(len(z))]
    return (np.stack([o[0] for o in outs]), np.array([o[1] for o in outs]), np.stack([o[2] for o in outs]),
            np.stack([o[3] for o in outs], 1), np.stack([o[4] for o in outs], 1))
