"""Targeted colour attacks with the reference's constructor signatures
(PointNet/attacks/torchattacks/attacks/target.py: tar_NB_attack :7-45, tar_NU_attack :52-175)."""
import torch

from pointsecguard_amd.models.pointnet2_sem_seg import draw_fps_starts, upload

from ..attack import Attack
from ._common import check_field, mask_to_device, psg_model
from .pointnet import is_pointnet, nb_attack as pointnet_nb_attack


class tar_NB_attack(Attack):
    """Targeted norm-bounded attack: only colours under `mask` move (on every batch row), descent on
    CE(mean) of batch row 0 towards `target` (target.py:26,36-43: labels[0] / outputs[0] only)."""

    def __init__(self, model, eps=0.3, alpha=2 / 255, iters=40, target=None, mask=None, field="color", coord_eps=None,
                 coord_alpha=None):
        super(tar_NB_attack, self).__init__("tar_NB_attack", model)
        self.model = model
        self.eps = eps
        self.alpha = alpha
        self.iters = iters
        self.target = target
        self.mask = mask
        self.field = check_field(field)      # extension of the reference API: see NB_attack
        self.coord_eps = coord_eps
        self.coord_alpha = coord_alpha

    def forward(self, images, labels):
        if is_pointnet(self.model):
            if self.field != "color":
                raise NotImplementedError("field=%r is implemented for the PointNet++ SSG network" % self.field)
            if self.target is None or self.mask is None:
                raise ValueError("tar_NB_attack needs target and mask")
            return pointnet_nb_attack(self, images, None, mask=self.mask, target=self.target)
        net = psg_model(self.model)
        if self.target is None or self.mask is None:
            raise ValueError("tar_NB_attack needs target and mask")
        images = images.detach().to(self.device).float().contiguous()
        B, C, N = images.shape
        mask = mask_to_device(self.mask, N, self.device)
        starts = upload(draw_fps_starts(B, N, self.iters, pinned=True), self.device, pin=True)
        ws = net._workspace(B, N, self.iters if self.field == "color" else 1)   # (the coordinate fields rebuild plan slot 0)
        net._generation += 1
        if self.field != "color":
            return ws.field_attack(net._packed(), images, None, starts, self.eps, self.alpha, self.iters, self.field,
                                   coord_eps=self.coord_eps, coord_alpha=self.coord_alpha, mask=mask, target=int(self.target))
        return ws.nb_attack(net._packed(), images, None, starts, self.eps, self.alpha, self.iters, mask=mask,
                            target=int(self.target))


class tar_NU_attack(Attack):
    """Targeted norm-unbounded attack.  `field` / `coord_c` / `coord_lr` are an extension of the reference API, see NU_attack:
    "color" (default) runs exactly the code path it always ran.  With field != "color" (PointNet++ SSG, one room per call or
    `forward_rooms`) the learning-rate halving with a fresh optimiser every 50 steps stays - both learning rates halve, all
    moments are zeroed - but the restart of target.py:127-132 is NOT applied: it is uniform [0, 1] noise followed by a clamp
    of all nine channels to the colour box, which has no coordinate counterpart and would wipe the perturbation."""

    def __init__(self, model, c=1e-4, kappa=0, steps=1000, lr=0.01, target=None, mask=None, field="color", coord_c=None,
                 coord_lr=None):
        super(tar_NU_attack, self).__init__("tar_NU_attack", model)
        self.c = c
        self.kappa = kappa
        self.steps = steps
        self.lr = lr
        self.target = target
        self.mask = mask
        self.field = check_field(field)
        self.coord_c = coord_c
        self.coord_lr = coord_lr

    def forward(self, images, labels):
        if self.field != "color":
            from .nu_field import nu_field_attack
            return nu_field_attack(self, images, labels, mask=self.mask, target=self.target, neighbour=5, targeted_variant=True)
        if is_pointnet(self.model):
            from .pointnet import nu_attack as pointnet_nu_attack
            return pointnet_nu_attack(self, images, labels, mask=self.mask, target=self.target, neighbour=5,
                                      targeted_variant=True)
        from .nu import nu_attack
        return nu_attack(self, images, labels, mask=self.mask, target=self.target, neighbour=5, targeted_variant=True)

    def forward_rooms(self, images, labels, masks):
        """Extension of the reference API: the attack applied to every room of `images` [R, 9, N] on its own (what R calls
        with batches of one and `mask = masks[r]` compute), all rooms advanced in lockstep with one launch per operation.
        Returns (adversarial images [R, 9, N], optimiser steps run per room); see nu.nu_attack_rooms for the two
        bookkeeping differences from R sequential calls (order of RNG consumption; at most 50 steps)."""
        if self.field != "color":
            from .nu_field import nu_field_attack_rooms
            return nu_field_attack_rooms(self, images, labels, masks, self.target, neighbour=5, targeted_variant=True)
        from .nu import nu_attack_rooms
        return nu_attack_rooms(self, images, labels, masks, self.target, neighbour=5, targeted_variant=True)
