"""Float64 restatement of the reference's vanilla PointNet sem-seg forward (PointNet/models/pointnet.py:10-130,
pointnet_sem_seg.py:26-49) for arbitrary inputs, from a state dict with the reference's keys: the yardstick of the GPU
parity tests (the reference itself does not exist where those run).  Autograd through it gives the reference's input
gradients; tests/test_pointnet_host.py pins it to the reference's recorded outputs (tests/golden/pointnet_room.npz).

Also the split / fold identities the gfx950 path relies on, stated on host in float64."""
import numpy as np
import torch
import torch.nn.functional as F

EPS = 1e-5


def _t(sd, k):
    v = sd[k]
    if not isinstance(v, torch.Tensor):
        v = torch.from_numpy(np.asarray(v))
    return v.detach().to(torch.float64)


def _bn(sd, name, x):
    return F.batch_norm(x, _t(sd, name + ".running_mean"), _t(sd, name + ".running_var"), _t(sd, name + ".weight"),
                        _t(sd, name + ".bias"), False, 0.0, EPS)


def _conv(sd, name, x):
    return F.conv1d(x, _t(sd, name + ".weight"), _t(sd, name + ".bias"))


def _fc(sd, name, x):
    return F.linear(x, _t(sd, name + ".weight"), _t(sd, name + ".bias"))


def _stn(sd, p, x, k):
    x = F.relu(_bn(sd, p + ".bn1", _conv(sd, p + ".conv1", x)))
    x = F.relu(_bn(sd, p + ".bn2", _conv(sd, p + ".conv2", x)))
    x = F.relu(_bn(sd, p + ".bn3", _conv(sd, p + ".conv3", x)))
    g, arg = torch.max(x, 2)
    x = F.relu(_bn(sd, p + ".bn4", _fc(sd, p + ".fc1", g)))
    x = F.relu(_bn(sd, p + ".bn5", _fc(sd, p + ".fc2", x)))
    x = _fc(sd, p + ".fc3", x) + torch.eye(k, dtype=torch.float64).reshape(1, k * k)
    return x.view(-1, k, k), g, arg


def forward(sd, x, extras=False):
    """x [B,9,N] float64 -> (log_probs [B,N,13], trans_feat [B,64,64]); extras=True adds a dict with trans, the three
    pooled vectors 'g_stn', 'g_fstn', 'g_feat' [B,1024] and their arg-max sets 'arg_*' [B,1024]."""
    B, _, N = x.shape
    x = x[:, :6, :]
    trans, g_stn, arg_stn = _stn(sd, "feat.stn", x, 3)
    xt = x.transpose(2, 1)
    xyz, feat = xt.split(3, dim=2)
    xt = torch.cat([torch.bmm(xyz, trans), feat], dim=2).transpose(2, 1)
    h = F.relu(_bn(sd, "feat.bn1", _conv(sd, "feat.conv1", xt)))
    trans_feat, g_fstn, arg_fstn = _stn(sd, "feat.fstn", h, 64)
    pf = torch.bmm(h.transpose(2, 1), trans_feat).transpose(2, 1)
    e = F.relu(_bn(sd, "feat.bn2", _conv(sd, "feat.conv2", pf)))
    e = _bn(sd, "feat.bn3", _conv(sd, "feat.conv3", e))
    g, arg = torch.max(e, 2)
    z = torch.cat([g[:, :, None].expand(B, 1024, N), pf], 1)
    z = F.relu(_bn(sd, "bn1", _conv(sd, "conv1", z)))
    z = F.relu(_bn(sd, "bn2", _conv(sd, "conv2", z)))
    z = F.relu(_bn(sd, "bn3", _conv(sd, "conv3", z)))
    z = _conv(sd, "conv4", z).transpose(2, 1).contiguous()
    logp = F.log_softmax(z.view(-1, 13), dim=-1).view(B, N, 13)
    if not extras:
        return logp, trans_feat
    return logp, trans_feat, dict(trans=trans, g_stn=g_stn, g_fstn=g_fstn, g_feat=g, arg_stn=arg_stn, arg_fstn=arg_fstn,
                                  arg_feat=arg, h=h)


def regulariser(trans):
    d = trans.size()[1]
    eye = torch.eye(d, dtype=trans.dtype)[None]
    return torch.mean(torch.norm(torch.bmm(trans, trans.transpose(2, 1) - eye), dim=(1, 2)))


def grads(sd, x, labels, with_reg=False, weight=None):
    """d NLL / d x (and, with_reg, d get_loss / d x: NLL + 0.001 * regulariser) for x [B,9,N] float64, labels [B,N]."""
    x = x.detach().clone().requires_grad_(True)
    logp, tf = forward(sd, x)
    loss = F.nll_loss(logp.reshape(-1, 13), labels.reshape(-1), weight=weight)
    if with_reg:
        loss = loss + regulariser(tf) * 0.001
    loss.backward()
    return x.grad


def folded_forward(folded, x):
    """The executed forward of the gfx950 path, in float64 from the folded layers (runtime.fold_pointnet_state_dict order):
    per-room transforms folded into the next layer's weights, the head's global columns as a per-room bias.
    Returns (log_probs, trans_feat)."""
    W = [torch.from_numpy(np.asarray(w, np.float64)) for w, _ in folded]
    b = [torch.from_numpy(np.asarray(v, np.float64)) for _, v in folded]
    B, _, N = x.shape
    p = x[:, :6, :].transpose(1, 2)                               # [B,N,6]

    def lin(i, a, relu=True):
        y = a @ W[i].T + b[i]
        return F.relu(y) if relu else y

    def stn(a, first, k):
        y = lin(first + 2, lin(first + 1, lin(first, a)))
        g = y.max(1)[0]
        return lin(first + 5, lin(first + 4, lin(first + 3, g)), relu=False).view(B, k, k)

    trans = stn(p, 0, 3)
    w1f = torch.cat([W[6][:, :3] @ trans.transpose(1, 2), W[6][:, 3:6].expand(B, 64, 3)], 2)   # W[:, :3] trans^T per room
    h = F.relu(torch.bmm(p, w1f.transpose(1, 2)) + b[6])
    tf = stn(h, 7, 64)
    c2f = W[13] @ tf.transpose(1, 2)                                # [B,128,64]
    e = F.relu(torch.bmm(h, c2f.transpose(1, 2)) + b[13])
    g = (e @ W[14].T + b[14]).max(1)[0]
    gb = g @ W[15][:, :1024].T + b[15]                              # per-room bias
    h1pf = W[15][:, 1024:] @ tf.transpose(1, 2)
    z = F.relu(torch.bmm(h, h1pf.transpose(1, 2)) + gb[:, None, :])
    z = lin(18, lin(17, lin(16, z)), relu=False)
    return F.log_softmax(z, -1), tf
