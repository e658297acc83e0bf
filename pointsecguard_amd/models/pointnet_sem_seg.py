"""Vanilla PointNet semantic-segmentation network behind the reference's module API.

Drop-in for the reference's PointNet/models/pointnet_sem_seg.py (get_model :8-38, get_loss :40-49): same class names,
constructor arguments and parameter names (reference checkpoints load with load_state_dict unchanged), and the forward
contract x [B,9,N] -> (log_softmax [B,N,13], trans_feat [B,64,64]).  The computation is ONE call into libpsg.so
(psg_pointnet_forward, hand-written gfx950 kernels); autograd sees a single Function whose backward is the HIP
input-gradient pass, differentiable in both outputs (trans_feat feeds get_loss's regulariser).

Eval mode, 13 classes and with_rgb=True only (the colour attacks need colours).  Like the reference, the network draws
nothing from torch's random number generators.
"""
import torch
import torch.nn as nn
import torch.nn.functional as F

try:  # the reference imports `pointnet` with models/ on sys.path
    from .pointnet import PointNetEncoder, feature_transform_reguliarzer
except ImportError:  # pragma: no cover - flat import (`sys.path.append('models')`) like the reference harness
    from pointnet import PointNetEncoder, feature_transform_reguliarzer

from pointsecguard_amd import _lib, runtime


class _PointNetFunction(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, module):
        B, C, N = x.shape
        model = module._packed()
        ws = module._workspace(B, N)
        xin = x.detach().contiguous().float()
        x0 = torch.empty(B, N, C, device=x.device, dtype=torch.float32)
        _lib.call("psg_to_point_major", runtime.ptr(xin), B, C, N, runtime.ptr(x0), runtime.stream())
        logp, trans_feat = ws.forward(model, x0)
        module._generation += 1
        ctx.module, ctx.model, ctx.ws, ctx.generation = module, model, ws, module._generation
        return logp, trans_feat

    @staticmethod
    def backward(ctx, dlogp, dtrans_feat):
        if ctx.generation != ctx.module._generation:
            raise RuntimeError("the activations of this forward were overwritten by a later forward of the same "
                               "module; only the most recent forward can be back-propagated")
        ws = ctx.ws
        B, N = ws.batch, ws.n_point
        if dlogp is None:
            dlogp = torch.zeros(B, N, runtime.NUM_CLASSES, device=dtrans_feat.device, dtype=torch.float32)
        dtf = None if dtrans_feat is None else dtrans_feat.contiguous().float()
        dx0 = ws.backward(ctx.model, dlogp.contiguous().float(), dtf)
        dx = torch.empty(B, 9, N, device=dx0.device, dtype=torch.float32)
        _lib.call("psg_to_channel_major", runtime.ptr(dx0), B, 9, N, runtime.ptr(dx), runtime.stream())
        return dx, None


class get_model(nn.Module):
    PSG_NETWORK = "pointnet"   # what the attacks dispatch on (the harness may import this file a second time by name)

    def __init__(self, num_class, with_rgb=True):
        super(get_model, self).__init__()
        if num_class != runtime.NUM_CLASSES:
            raise ValueError("the gfx950 kernels are specialised for the %d S3DIS classes" % runtime.NUM_CLASSES)
        if not with_rgb:
            raise NotImplementedError("with_rgb=False is out of scope: the colour attacks need the colour channels")
        channel = 6
        self.k = num_class
        self.feat = PointNetEncoder(global_feat=False, feature_transform=True, channel=channel)
        self.conv1 = torch.nn.Conv1d(1088, 512, 1)
        self.conv2 = torch.nn.Conv1d(512, 256, 1)
        self.conv3 = torch.nn.Conv1d(256, 128, 1)
        self.conv4 = torch.nn.Conv1d(128, self.k, 1)
        self.bn1 = nn.BatchNorm1d(512)
        self.bn2 = nn.BatchNorm1d(256)
        self.bn3 = nn.BatchNorm1d(128)
        self._psg_model = None
        self._psg_key = None
        self._psg_ws = {}
        self._generation = 0

    # ---- libpsg plumbing
    def _packed(self):
        """BN-folded weights on the device; rebuilt when a parameter / buffer changed."""
        tensors = list(self.parameters()) + list(self.buffers())
        key = tuple((t.data_ptr(), t._version) for t in tensors)
        if self._psg_model is None or key != self._psg_key:
            sd = {k: v.detach().cpu() for k, v in self.state_dict().items()}
            self._psg_model = runtime.PointNetModel(runtime.fold_pointnet_state_dict(sd))
            self._psg_key = key
        return self._psg_model

    def _workspace(self, batch, n_point):
        key = (batch, n_point)
        ws = self._psg_ws.get(key)
        if ws is None:
            ws = runtime.PointNetWorkspace(batch, n_point)
            self._psg_ws[key] = ws
        return ws

    def forward(self, x):
        if self.training:
            raise NotImplementedError("pointsecguard_amd implements the eval-mode attack path only; call .eval() "
                                      "(training-mode BatchNorm is out of scope)")
        runtime.require_cuda(x, "x")
        if x.dim() != 3 or x.shape[1] != 9:
            raise ValueError("expected input [B, 9, N], got %s" % (tuple(x.shape),))
        if x.shape[2] % runtime.POINTNET_POINT_TILE:
            raise _lib.PsgError("N=%d is not a multiple of the point tile %d" % (x.shape[2], runtime.POINTNET_POINT_TILE))
        return _PointNetFunction.apply(x, self)


class get_loss(torch.nn.Module):
    def __init__(self, mat_diff_loss_scale=0.001):
        super(get_loss, self).__init__()
        self.mat_diff_loss_scale = mat_diff_loss_scale

    def forward(self, pred, target, trans_feat, weight):
        loss = F.nll_loss(pred, target, weight=weight)
        mat_diff_loss = feature_transform_reguliarzer(trans_feat)
        total_loss = loss + mat_diff_loss * self.mat_diff_loss_scale
        return total_loss
