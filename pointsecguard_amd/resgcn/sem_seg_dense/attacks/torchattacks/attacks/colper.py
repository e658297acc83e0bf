"""Non-targeted attacks on DenseDeepGCN with the reference's signatures
(ResGCN/sem_seg_dense/attacks/torchattacks/attacks/colper.py: NB_attack :9-39).  `field` ("color" | "coord" | "both") is an
extension of the reference API: which three-channel field of the room the attack moves."""
import torch

from pointsecguard_amd.attacks.torchattacks.attacks._common import check_field

from ..attack import Attack

FIELD_CODES = {"coord": 1, "both": 2}          # PSG_NU_FIELD_COORD / PSG_NU_FIELD_BOTH of include/psg.h
ATYPES = {"Color": "color", "Coord": "coord", "Both": "both"}


def _gcn(model):
    if not hasattr(model, "_packed") or not hasattr(model, "n_blocks"):
        raise TypeError("pointsecguard_amd ResGCN attacks drive pointsecguard_amd.resgcn...DenseDeepGCN; got %s"
                        % type(model).__name__)
    return model


def resolve_field(field, atype):
    """The field one NB_attack.forward call moves: atype "Color" (the default of the reference's signature) means "use the
    constructor's field"; "Coord" / "Both" select that field, and must not contradict a non-colour constructor field."""
    if atype not in ATYPES:
        raise NotImplementedError("atype must be one of %s, got %r" % (sorted(ATYPES), atype))
    field = check_field(field)
    asked = ATYPES[atype]
    if asked == "color":
        return field
    if field != "color" and field != asked:
        raise ValueError("atype=%r contradicts the attack's field=%r" % (atype, field))
    return asked


class NB_attack(Attack):
    """PGD: CrossEntropyLoss() (mean) on the logits, sign ascent, L-inf projection; one fused libpsg call.  Returns the
    un-projected last step like the reference (colper.py:35-39).  field "color" (default): the reference's attack on
    channels 3:6.  "coord": the same loop body on channels 0:3 with (coord_eps, coord_alpha) - defaults eps, alpha - and no
    [0, 1] clamp, the head's xyz graph rebuilt from the moved points by every forward; "both": the two together."""

    def __init__(self, model, eps=0.3, alpha=2 / 255, iters=40, field="color", coord_eps=None, coord_alpha=None):
        super(NB_attack, self).__init__("NB_attack", model)
        self.model, self.eps, self.alpha, self.iters = model, eps, alpha, iters
        self.field = check_field(field)
        self.coord_eps = eps if coord_eps is None else coord_eps
        self.coord_alpha = alpha if coord_alpha is None else coord_alpha

    def forward(self, images, labels, atype="Color"):
        field = resolve_field(self.field, atype)
        net = _gcn(self.model)
        images = images.detach().to(self.device).float()
        B, C, N, _ = images.shape
        x = images[:, :, :, 0].contiguous()
        labels = labels.detach().to(self.device).to(torch.int32).contiguous()
        net.consume_rng(self.iters)                  # RNG parity: one draw per stochastic DenseDilated.forward
        net._generation += 1
        if field == "color":
            adv = net._workspace(B, N).nb_attack(net._packed(), x, labels, self.eps, self.alpha, self.iters)
        else:
            adv = net._workspace(B, N).nb_attack_field(net._packed(), x, labels, FIELD_CODES[field], self.eps, self.alpha,
                                                       self.coord_eps, self.coord_alpha, self.iters)
        return adv.unsqueeze(-1)


class NU_attack(Attack):
    """Norm-unbounded attack (colper.py:42-120): Adam on w (tanh space), cost = c*f + 1e-4*Smooth + L2.  field "coord" /
    "both" (nu_field.py): Adam on delta [N, 3] in metres with step size coord_lr (default lr), cost c*f + 1e-4*Smooth_xyz +
    L2_xyz (+ the colour terms with "both"); one room per `forward` call, or `forward_rooms`."""

    def __init__(self, model, c=1e-4, kappa=0, steps=1000, lr=0.01, target=None, ori=None, field="color", coord_lr=None):
        super(NU_attack, self).__init__("NU_attack", model)
        self.c, self.kappa, self.steps, self.lr, self.target, self.ori = c, kappa, steps, lr, target, ori
        self.field, self.coord_lr = check_field(field), coord_lr

    def forward(self, images, labels):
        if self.field != "color":
            from .nu_field import gcn_nu_field_attack
            return gcn_nu_field_attack(self, images, labels, neighbour=10)
        from .nu import gcn_nu_attack
        return gcn_nu_attack(self, images, labels, neighbour=10)

    def forward_rooms(self, images, labels):
        """R >= 1 one-room attacks in lockstep (nu.gcn_nu_attack_rooms): images [R, 9, N, 1], labels [R, N] ->
        (adv [R, 9, N, 1], steps_run [R]); per room what `forward` computes on that room alone."""
        if self.field != "color":
            from .nu_field import gcn_nu_field_attack_rooms
            return gcn_nu_field_attack_rooms(self, images, labels, neighbour=10)
        from .nu import gcn_nu_attack_rooms
        return gcn_nu_attack_rooms(self, images, labels, neighbour=10)
