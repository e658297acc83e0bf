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


def _relu(x, dec, key):
    """ReLU, or - with prescribed decisions - the product with the given 0 / 1 gate of x's shape"""
    return F.relu(x) if dec is None else x * dec[key]


def _stn(sd, p, x, k, dec=None):
    x = _relu(_bn(sd, p + ".bn1", _conv(sd, p + ".conv1", x)), dec, p + ".1")
    x = _relu(_bn(sd, p + ".bn2", _conv(sd, p + ".conv2", x)), dec, p + ".2")
    x = _bn(sd, p + ".bn3", _conv(sd, p + ".conv3", x))
    if dec is None:
        g, arg = torch.max(F.relu(x), 2)
    else:                                   # the pooled layer's ReLU acts on the pooled value: gate [B,1024]
        arg = dec[p + ".arg"]
        g = torch.gather(x, 2, arg[:, :, None])[:, :, 0] * dec[p + ".pool"]
    x = _relu(_bn(sd, p + ".bn4", _fc(sd, p + ".fc1", g)), dec, p + ".4")
    x = _relu(_bn(sd, p + ".bn5", _fc(sd, p + ".fc2", x)), dec, p + ".5")
    x = _fc(sd, p + ".fc3", x) + torch.eye(k, dtype=torch.float64).reshape(1, k * k)
    return x.view(-1, k, k), g, arg


def forward(sd, x, extras=False, decide=None):
    """x [B,9,N] float64 -> (log_probs [B,N,13], trans_feat [B,64,64]); extras=True adds a dict with trans, the three
    pooled vectors 'g_stn', 'g_fstn', 'g_feat' [B,1024] and their arg-max sets 'arg_*' [B,1024].
    decide: the network's discrete decisions PRESCRIBED instead of taken (device_decisions builds them from a workspace
    snapshot): float64 0 / 1 gates in the layout of the tensor they multiply - 'feat.stn.1', '.2' [B,C,N], '.4', '.5' [B,C]
    and '.pool' [B,1024] (likewise 'feat.fstn.*'), 'h', 'e2', 'z1', 'z2', 'z3' [B,C,N] - and the int64 arg-max sets
    'feat.stn.arg', 'feat.fstn.arg', 'arg' [B,1024].  The result is then a smooth function of x around the decisions."""
    B, _, N = x.shape
    x = x[:, :6, :]
    dec = decide
    trans, g_stn, arg_stn = _stn(sd, "feat.stn", x, 3, dec)
    xt = x.transpose(2, 1)
    xyz, feat = xt.split(3, dim=2)
    xt = torch.cat([torch.bmm(xyz, trans), feat], dim=2).transpose(2, 1)
    h = _relu(_bn(sd, "feat.bn1", _conv(sd, "feat.conv1", xt)), dec, "h")
    trans_feat, g_fstn, arg_fstn = _stn(sd, "feat.fstn", h, 64, dec)
    pf = torch.bmm(h.transpose(2, 1), trans_feat).transpose(2, 1)
    e = _relu(_bn(sd, "feat.bn2", _conv(sd, "feat.conv2", pf)), dec, "e2")
    e = _bn(sd, "feat.bn3", _conv(sd, "feat.conv3", e))
    if dec is None:
        g, arg = torch.max(e, 2)
    else:
        arg = dec["arg"]
        g = torch.gather(e, 2, arg[:, :, None])[:, :, 0]
    z = torch.cat([g[:, :, None].expand(B, 1024, N), pf], 1)
    z = _relu(_bn(sd, "bn1", _conv(sd, "conv1", z)), dec, "z1")
    z = _relu(_bn(sd, "bn2", _conv(sd, "conv2", z)), dec, "z2")
    z = _relu(_bn(sd, "bn3", _conv(sd, "conv3", z)), dec, "z3")
    z = _conv(sd, "conv4", z).transpose(2, 1).contiguous()
    logp = F.log_softmax(z.view(-1, 13), dim=-1).view(B, N, 13)
    if not extras:
        return logp, trans_feat
    return logp, trans_feat, dict(trans=trans, g_stn=g_stn, g_fstn=g_fstn, g_feat=g, arg_stn=arg_stn, arg_fstn=arg_fstn,
                                  arg_feat=arg, h=h)


def device_decisions(snap, B, N):
    """`decide` of forward() from a workspace snapshot (tap names; bit words unpacked to [rows, M] bool)"""
    def pts(a):                                                  # [B*N, C] -> [B, C, N]
        return torch.from_numpy(np.asarray(a).reshape(B, N, -1).transpose(0, 2, 1).astype(np.float64))

    def room(a):
        return torch.from_numpy(np.asarray(a).astype(np.float64))
    pool, pidx = np.asarray(snap["pool"]), np.asarray(snap["pidx"]).astype(np.int64)
    dec = {"h": pts(snap["mh"]), "e2": pts(np.asarray(snap["e2"]) > 0), "z1": pts(snap["m1"]), "z2": pts(snap["m2"]), "z3": pts(snap["m3"]),
           "arg": torch.from_numpy(pidx[:, 2048:])}
    for p, k, a1, a2, m1, m2 in (("feat.stn", 0, "a1", "a2", "mf1", "mf2"), ("feat.fstn", 1, "k1", "k2", "mfk1", "mfk2")):
        dec[p + ".1"], dec[p + ".2"] = pts(np.asarray(snap[a1]) > 0), pts(np.asarray(snap[a2]) > 0)
        dec[p + ".4"], dec[p + ".5"] = room(snap[m1]), room(snap[m2])
        dec[p + ".pool"] = room(pool[:, k * 1024:(k + 1) * 1024] > 0)
        dec[p + ".arg"] = torch.from_numpy(pidx[:, k * 1024:(k + 1) * 1024])
    return dec


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
