"""Sub-modules of the vanilla PointNet behind the reference's module API (PointNet/models/pointnet.py:10-130): STN3d,
STNkd, PointNetEncoder and feature_transform_reguliarzer, with the reference's constructor arguments and parameter names,
so that a checkpoint of pointnet_sem_seg.get_model loads with load_state_dict.

They hold parameters only: the network runs as ONE call into libpsg.so from pointnet_sem_seg.get_model (the transforms
are folded into the next layers per room and the three max-pools are fused into their GEMMs), so a sub-module's own
forward raises instead of computing elsewhere.
"""
import torch
import torch.nn as nn


def _whole_network_only(module):
    raise NotImplementedError("pointsecguard_amd runs %s only as part of pointnet_sem_seg.get_model (one fused gfx950 "
                              "forward); there is no per-module path" % type(module).__name__)


class STN3d(nn.Module):
    def __init__(self, channel):
        super(STN3d, self).__init__()
        self.conv1 = torch.nn.Conv1d(channel, 64, 1)
        self.conv2 = torch.nn.Conv1d(64, 128, 1)
        self.conv3 = torch.nn.Conv1d(128, 1024, 1)
        self.fc1 = nn.Linear(1024, 512)
        self.fc2 = nn.Linear(512, 256)
        self.fc3 = nn.Linear(256, 9)
        self.relu = nn.ReLU()
        self.bn1 = nn.BatchNorm1d(64)
        self.bn2 = nn.BatchNorm1d(128)
        self.bn3 = nn.BatchNorm1d(1024)
        self.bn4 = nn.BatchNorm1d(512)
        self.bn5 = nn.BatchNorm1d(256)

    def forward(self, x):
        _whole_network_only(self)


class STNkd(nn.Module):
    def __init__(self, k=64):
        super(STNkd, self).__init__()
        self.conv1 = torch.nn.Conv1d(k, 64, 1)
        self.conv2 = torch.nn.Conv1d(64, 128, 1)
        self.conv3 = torch.nn.Conv1d(128, 1024, 1)
        self.fc1 = nn.Linear(1024, 512)
        self.fc2 = nn.Linear(512, 256)
        self.fc3 = nn.Linear(256, k * k)
        self.relu = nn.ReLU()
        self.bn1 = nn.BatchNorm1d(64)
        self.bn2 = nn.BatchNorm1d(128)
        self.bn3 = nn.BatchNorm1d(1024)
        self.bn4 = nn.BatchNorm1d(512)
        self.bn5 = nn.BatchNorm1d(256)
        self.k = k

    def forward(self, x):
        _whole_network_only(self)


class PointNetEncoder(nn.Module):
    def __init__(self, global_feat=True, feature_transform=False, channel=3):
        super(PointNetEncoder, self).__init__()
        self.stn = STN3d(channel)
        self.conv1 = torch.nn.Conv1d(channel, 64, 1)
        self.conv2 = torch.nn.Conv1d(64, 128, 1)
        self.conv3 = torch.nn.Conv1d(128, 1024, 1)
        self.bn1 = nn.BatchNorm1d(64)
        self.bn2 = nn.BatchNorm1d(128)
        self.bn3 = nn.BatchNorm1d(1024)
        self.global_feat = global_feat
        self.feature_transform = feature_transform
        if self.feature_transform:
            self.fstn = STNkd(k=64)

    def forward(self, x):
        _whole_network_only(self)


def feature_transform_reguliarzer(trans):
    """pointnet.py:125-130 as written there: mean over rooms of ||T (T^T - I)||_F (the reference's bracket, kept, so that
    get_loss and its gradient are the reference's).  Loss glue on a [B,64,64] tensor, differentiable by autograd."""
    d = trans.size()[1]
    eye = torch.eye(d, device=trans.device, dtype=trans.dtype)[None, :, :]
    return torch.mean(torch.norm(torch.bmm(trans, trans.transpose(2, 1) - eye), dim=(1, 2)))
