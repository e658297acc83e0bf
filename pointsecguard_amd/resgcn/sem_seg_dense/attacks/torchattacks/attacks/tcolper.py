"""Targeted attack on DenseDeepGCN (reference: .../attacks/tcolper.py: tar_NB_attack :7-46): only points under `mask`
move, CrossEntropyLoss (mean over ALL rows) towards `target`, early exit when more than 90 % of the masked points are
classified as the target, the projected field written back at the end.  `field` ("color" | "coord" | "both") is an extension
of the reference API, as in colper.py."""
import numpy as np
import torch

from pointsecguard_amd import _lib, runtime
from pointsecguard_amd.attacks.torchattacks.attacks._common import check_field

from ..attack import Attack
from .colper import _gcn


class tar_NB_attack(Attack):
    def __init__(self, model, eps=0.3, alpha=2 / 255, iters=40, target=None, mask=None, field="color", coord_eps=None,
                 coord_alpha=None):
        super(tar_NB_attack, self).__init__("tar_NB_attack", model)
        self.model, self.eps, self.alpha, self.iters, self.target, self.mask = model, eps, alpha, iters, target, mask
        self.field = check_field(field)
        self.coord_eps = eps if coord_eps is None else coord_eps
        self.coord_alpha = alpha if coord_alpha is None else coord_alpha

    def forward(self, images, labels):
        net = _gcn(self.model)
        images = images.detach().to(self.device).float()
        B, C, N, _ = images.shape
        mask_np = self.mask.detach().cpu().numpy() if isinstance(self.mask, torch.Tensor) else np.asarray(self.mask)
        mask_d = torch.from_numpy(mask_np.astype(np.uint8)).to(self.device)
        mask_b = mask_d.bool()
        model, ws = net._packed(), net._workspace(B, N)
        net._generation += 1
        st = runtime.stream
        x0 = torch.empty(B, N, 9, device=self.device, dtype=torch.float32)
        _lib.call("psg_to_point_major", runtime.ptr(images[:, :, :, 0].contiguous()), B, 9, N, runtime.ptr(x0), st())
        ori = x0[:, :, 3:6].contiguous()
        ori_xyz = x0[:, :, 0:3].contiguous() if self.field != "color" else None
        dl = torch.empty(B, N, 13, device=self.device, dtype=torch.float32)
        out = torch.empty(B, 9, N, device=self.device, dtype=torch.float32)

        def snapshot():
            _lib.call("psg_to_channel_major", runtime.ptr(x0), B, 9, N, runtime.ptr(out), st())
            return out.unsqueeze(-1)

        for i in range(self.iters):
            net.consume_rng(1)
            logits = ws.forward(model, x0)          # (every forward rebuilds the head's xyz graph: the points may have moved)
            pred = logits.argmax(dim=2)
            target_acc = pred[:, mask_b].eq(int(self.target)).sum().item() / float(mask_b.sum().item())
            if target_acc > 0.9:                                    # tcolper.py:37-38
                return snapshot()
            _lib.call("psg_ce_logp_grad", runtime.ptr(logits), None, int(self.target), B * N, B * N, 13, 1.0 / (B * N),
                      runtime.ptr(dl), None, st())
            dx0 = ws.backward(model, dl)
            # descent, the projected field kept in x0 (the reference writes the projected colour back, :45)
            if self.field == "color":
                _lib.call("psg_pgd_step", runtime.ptr(x0), runtime.ptr(dx0), runtime.ptr(ori), runtime.ptr(mask_d), B, N,
                          float(self.alpha), float(self.eps), -1.0, 0, st())
                continue
            _lib.call("psg_pgd_step_field", runtime.ptr(x0), runtime.ptr(dx0), runtime.ptr(ori_xyz), runtime.ptr(mask_d), B, N, 0,
                      float(self.coord_alpha), float(self.coord_eps), -1.0, 0, st())
            if self.field == "both":
                _lib.call("psg_pgd_step_field", runtime.ptr(x0), runtime.ptr(dx0), runtime.ptr(ori), runtime.ptr(mask_d), B, N, 3,
                          float(self.alpha), float(self.eps), -1.0, 0, st())
        return snapshot()


class tar_NU_attack(Attack):
    """Targeted norm-unbounded attack (tcolper.py:51-170): masked colours, cost = f + 1e-4*Smooth + c*L2, learning
    rate halved with a fresh optimiser every 50 steps, restart check every 10 steps.  field "coord" / "both" (nu_field.py):
    Adam on delta in metres with step size coord_lr (default lr), cost f + 1e-4*Smooth_xyz + coord_c*L2_xyz (coord_c
    defaults to c; + the colour terms with "both"), both learning rates halved every 50 steps, NO restart."""

    def __init__(self, model, c=1e-4, kappa=0, steps=1000, lr=0.01, target=None, mask=None, field="color", coord_c=None,
                 coord_lr=None):
        super(tar_NU_attack, self).__init__("tar_NU_attack", model)
        self.c, self.kappa, self.steps, self.lr, self.target, self.mask = c, kappa, steps, lr, target, mask
        self.field, self.coord_c, self.coord_lr = check_field(field), coord_c, coord_lr

    def forward(self, images, labels):
        if self.field != "color":
            from .nu_field import gcn_nu_field_attack
            return gcn_nu_field_attack(self, images, labels, mask=self.mask, target=self.target, neighbour=5, targeted_variant=True)
        from .nu import gcn_nu_attack
        return gcn_nu_attack(self, images, labels, mask=self.mask, target=self.target, neighbour=5, targeted_variant=True)

    def forward_rooms(self, images, labels, masks):
        """R >= 1 one-room attacks in lockstep (nu.gcn_nu_attack_rooms), room r under masks[r]: images [R, 9, N, 1], labels
        [R, N], masks [R, N] bool -> (adv [R, 9, N, 1], steps_run [R]).  Every room starts from this object's lr, which is
        put back on return (R fresh attack objects, as the reference's harness builds them)."""
        if self.field != "color":
            from .nu_field import gcn_nu_field_attack_rooms
            return gcn_nu_field_attack_rooms(self, images, labels, masks=masks, target=self.target, neighbour=5,
                                             targeted_variant=True)
        from .nu import gcn_nu_attack_rooms
        return gcn_nu_attack_rooms(self, images, labels, masks=masks, target=self.target, neighbour=5, targeted_variant=True)
