"""Non-targeted colour attacks with the reference's constructor signatures
(PointNet/attacks/torchattacks/attacks/nontarget.py: NB_attack :10-42, NU_attack :44-135)."""
import torch

from pointsecguard_amd.models.pointnet2_sem_seg import draw_fps_starts, upload

from ..attack import Attack
from ._common import check_field, labels_to_device, psg_model
from .pointnet import is_pointnet, nb_attack as pointnet_nb_attack


class NB_attack(Attack):
    """Norm-bounded (PGD-style) attack on the colour channels 3:6.

    One fused, stream-ordered libpsg call: geometry of all `iters` forwards built up front, then
    iters x (forward, CE-on-log-probs gradient, input-gradient backward, sign step + L-inf
    projection).  Like the reference, the returned colours are the UN-projected last step
    (nontarget.py:37-41: the projection lands in `color`, which is not written back)."""

    def __init__(self, model, eps=0.3, alpha=2 / 255, iters=40, field="color", coord_eps=None, coord_alpha=None):
        super(NB_attack, self).__init__("NB_attack", model)
        self.model = model
        self.eps = eps
        self.alpha = alpha
        self.iters = iters
        # extension of the reference API: which field moves.  "color" (default): the reference's attack, the fused call.
        # "coord": channels 0:3 with the same loop body (sign step, eta clamped to +-coord_eps, no [0, 1] clamp), geometry
        # rebuilt from the moved points every iteration; "both": the two fields together.  PointNet++ SSG only.
        self.field = check_field(field)
        self.coord_eps = coord_eps
        self.coord_alpha = coord_alpha

    def forward(self, images, labels):
        if is_pointnet(self.model):
            if self.field != "color":
                raise NotImplementedError("field=%r is implemented for the PointNet++ SSG network" % self.field)
            return pointnet_nb_attack(self, images, labels)
        net = psg_model(self.model)
        images = images.detach().to(self.device).float().contiguous()
        B, C, N = images.shape
        labels = labels_to_device(labels, self.device, pin=True)
        starts = upload(draw_fps_starts(B, N, self.iters, pinned=True), self.device, pin=True)
        ws = net._workspace(B, N, self.iters if self.field == "color" else 1)   # (the coordinate fields rebuild plan slot 0)
        net._generation += 1  # the workspace activations no longer belong to an earlier autograd forward
        if self.field != "color":
            return ws.field_attack(net._packed(), images, labels, starts, self.eps, self.alpha, self.iters, self.field,
                                   coord_eps=self.coord_eps, coord_alpha=self.coord_alpha)
        return ws.nb_attack(net._packed(), images, labels, starts, self.eps, self.alpha, self.iters)


class NU_attack(Attack):
    """Norm-unbounded attack (Adam on f + c (Smooth + L2)).  `field` is an extension of the reference API, like NB_attack's:
    "color" (default) is the reference's attack on channels 3:6 and runs exactly the code path it always ran; "coord" moves
    channels 0:3 (delta in metres optimised directly, cost f + coord_c (Smooth_xyz + L2_xyz), step size coord_lr), "both"
    the two fields together - PointNet++ SSG only, one room per call or `forward_rooms` (nu_field.py).  coord_c / coord_lr
    default to c / lr."""

    def __init__(self, model, c=1e-4, kappa=0, steps=1000, lr=0.01, field="color", coord_c=None, coord_lr=None):
        super(NU_attack, self).__init__("NU_attack", model)
        self.c = c
        self.kappa = kappa
        self.steps = steps
        self.lr = lr
        self.field = check_field(field)
        self.coord_c = coord_c
        self.coord_lr = coord_lr

    def forward(self, images, labels):
        if self.field != "color":
            from .nu_field import nu_field_attack
            return nu_field_attack(self, images, labels, mask=None, target=None, neighbour=10)
        if is_pointnet(self.model):
            from .pointnet import nu_attack as pointnet_nu_attack
            return pointnet_nu_attack(self, images, labels, mask=None, target=None, neighbour=10)
        from .nu import nu_attack
        return nu_attack(self, images, labels, mask=None, target=None, neighbour=10)

    def forward_rooms(self, images, labels):
        """Extension of the reference API: the attack applied to every room of `images` [R, 9, N] on its own (R calls with
        batches of one), all rooms advanced in lockstep; returns (adversarial images, optimiser steps run per room)."""
        if self.field != "color":             # (one room and more; the colour path keeps its R >= 2 rule)
            from .nu_field import nu_field_attack_rooms
            return nu_field_attack_rooms(self, images, labels, None, None, neighbour=10)
        from .nu import nu_attack_rooms
        return nu_attack_rooms(self, images, labels, None, None, neighbour=10)
