"""Float64 restatement of the reference's PointNet++ SSG sem-seg forward (PointNet/models/pointnet2_sem_seg.py:22-40 with
pointnet_util.py:110-143, :181-207, :281-320) with the INDEX TABLES GIVEN (FPS, ball query, 3-NN) and everything else
differentiable: relative coordinates (xyz[idx] - xyz[fps_idx]), square_distance -> inverse-distance weights, the shared
layers, the max-pool.  That is the function the reference's autograd differentiates for a leaf on the whole [B, 9, N]
input (its index selections carry no gradient), so autograd through this file is the yardstick of the coordinate
gradient; tests/test_pn2_fullgrad_host.py pins it to the reference's recorded gradient
(tests/golden/pn2_fullgrad.npz).  The reference itself does not exist where the GPU tests run."""
import numpy as np
import torch
import torch.nn.functional as F

EPS = 1e-5
GROUPS = ((0, 3), (3, 6), (6, 9))   # channel groups of the input: xyz, colour, normalised xyz


def _t(sd, k):
    v = sd[k]
    if not isinstance(v, torch.Tensor):
        v = torch.from_numpy(np.asarray(v))
    return v.detach().to(torch.float64)


def _layer(sd, name, i, x):
    """Conv -> BatchNorm(eval) -> ReLU over channel-last rows x [..., cin]."""
    w = _t(sd, "%s.mlp_convs.%d.weight" % (name, i))
    w = w.reshape(w.shape[0], -1)
    y = x @ w.T + _t(sd, "%s.mlp_convs.%d.bias" % (name, i))
    bn = "%s.mlp_bns.%d" % (name, i)
    y = (y - _t(sd, bn + ".running_mean")) / torch.sqrt(_t(sd, bn + ".running_var") + EPS) * _t(sd, bn + ".weight") + _t(sd, bn + ".bias")
    return F.relu(y)


def _index(points, idx):
    """index_points: points [B, N, C], idx [B, ...] -> [B, ..., C]."""
    B = points.shape[0]
    flat = idx.reshape(B, -1).long()
    out = torch.gather(points, 1, flat[:, :, None].expand(-1, -1, points.shape[2]))
    return out.reshape(tuple(idx.shape) + (points.shape[2],))


def tables_from(npz_like, batch=None):
    """{'fps0'.., 'group0'.., 'nn_idx0'..} -> int64 tensors ([B, ...])."""
    out = {}
    for l in range(4):
        for k in ("fps%d", "group%d", "nn_idx%d"):
            a = np.asarray(npz_like[k % l]).astype(np.int64)
            out[k % l] = torch.from_numpy(a if batch is None else a[batch])
    return out


def forward(sd, x, tables, xyz_from=None):
    """x [B, 9, N] float64 (may require grad), tables: see tables_from -> log-probs [B, N, 13].  xyz_from (optional,
    [B, 9, N]): the tensor l0_xyz is sliced from instead of x - a detached copy of x gives the feature path alone."""
    x = x.to(torch.float64)
    pts = x.transpose(1, 2)                  # l0_points: all nine channels
    xyz = (pts if xyz_from is None else xyz_from.to(torch.float64).transpose(1, 2))[:, :, :3]      # l0_xyz
    lv_xyz, lv_pts = [xyz], [pts]
    for l, name in enumerate(("sa1", "sa2", "sa3", "sa4")):
        new_xyz = _index(lv_xyz[l], tables["fps%d" % l])                          # [B, S, 3]
        gi = tables["group%d" % l]
        rel = _index(lv_xyz[l], gi) - new_xyz[:, :, None, :]                     # grouped_xyz_norm
        h = torch.cat([rel, _index(lv_pts[l], gi)], dim=-1)                      # [B, S, K, 3 + D]
        for i in range(3):
            h = _layer(sd, name, i, h)
        lv_xyz.append(new_xyz)
        lv_pts.append(torch.max(h, 2)[0])
    up = lv_pts[4]
    for l, name, nl in ((3, "fp4", 2), (2, "fp3", 2), (1, "fp2", 2), (0, "fp1", 3)):
        x1, x2 = lv_xyz[l], lv_xyz[l + 1]
        idx = tables["nn_idx%d" % l]
        nb = _index(x2, idx)                                                     # [B, N, 3, 3]
        # square_distance: -2 x.y + |x|^2 + |y|^2 for the three neighbours the sort kept
        d = -2.0 * (x1[:, :, None, :] * nb).sum(-1) + (x1 ** 2).sum(-1)[:, :, None] + (nb ** 2).sum(-1)
        r = 1.0 / (d + 1e-8)
        w = r / r.sum(dim=2, keepdim=True)
        h = (_index(up, idx) * w[:, :, :, None]).sum(dim=2)
        if l > 0:
            h = torch.cat([lv_pts[l], h], dim=-1)
        for i in range(nl):
            h = _layer(sd, name, i, h)
        up = h
    h = up @ _t(sd, "conv1.weight").reshape(128, 128).T + _t(sd, "conv1.bias")
    h = (h - _t(sd, "bn1.running_mean")) / torch.sqrt(_t(sd, "bn1.running_var") + EPS) * _t(sd, "bn1.weight") + _t(sd, "bn1.bias")
    h = F.relu(h)
    h = h @ _t(sd, "conv2.weight").reshape(13, 128).T + _t(sd, "conv2.bias")
    return F.log_softmax(h, dim=-1)


def nb_cost(logp, labels):
    """The NB attack's cost (nontarget.py:26,34): CrossEntropyLoss(sum) ON the log-probs, over all rooms, / N."""
    return F.cross_entropy(logp.reshape(-1, logp.shape[-1]), labels.reshape(-1).long(), reduction="sum") / logp.shape[1]


def tar_cost(logp, target):
    """tar_NB's cost (target.py:27,36-39): CrossEntropyLoss(mean) of batch row 0 against the target class."""
    y = torch.full((logp.shape[1],), int(target), dtype=torch.long)
    return F.cross_entropy(logp[0], y)


def input_grad(sd, x_np, tables, labels=None, target=None):
    """d cost / d x for x [B, 9, N] (numpy), float64 [B, 9, N]; also returns the log-probs."""
    x = torch.from_numpy(np.asarray(x_np, np.float64)).clone().requires_grad_(True)
    logp = forward(sd, x, tables)
    cost = nb_cost(logp, torch.from_numpy(np.asarray(labels))) if target is None else tar_cost(logp, target)
    cost.backward()
    return x.grad.numpy(), logp.detach().numpy()


def grad_error(got, ref):
    """Per channel group of [B, 9, N] gradients: (max |got - ref| / max |ref|, share of entries whose signs agree,
    largest |ref| among the disagreeing entries / max |ref|)."""
    out = []
    for lo, hi in GROUPS:
        g, r = np.asarray(got[:, lo:hi], np.float64), np.asarray(ref[:, lo:hi], np.float64)
        top = np.abs(r).max()
        agree = np.sign(g) == np.sign(r)
        out.append((float(np.abs(g - r).max() / top), float(agree.mean()),
                    float(np.abs(r[~agree]).max() / top) if not agree.all() else 0.0))
    return out


def median_rel(got, ref):
    """Per channel group: the median over the non-zero entries of |got - ref| / |ref| (the third clause of check_grad,
    tests/test_gpu_parity.py)."""
    out = []
    for lo, hi in GROUPS:
        g, r = np.asarray(got[:, lo:hi], np.float64), np.asarray(ref[:, lo:hi], np.float64)
        nz = r != 0
        out.append(float(np.median(np.abs(g - r)[nz] / np.abs(r[nz]))))
    return out
