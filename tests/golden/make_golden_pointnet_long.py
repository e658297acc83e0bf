"""Generate tests/golden/pointnet_tarnu_long.npz by running the REFERENCE tar_NU_attack itself past its step-50 learning-rate
halving (build container only; never runs on the GPU box).

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_pointnet_long.py

Weights and rooms are NOT stored (pointsecguard_amd.synthetic.pointnet_state_dict(PN_SEED), make_rooms(2, ROOM_SEED), as in
make_golden_pointnet.py).  The unmodified reference tar_NU_attack(c=0, kappa=1, lr=3, STEPS steps, target=4, mask = every
fourth point) on room 0 with labels = the clean prediction, single thread.  Recorded, numbers only:
  costs            the scalar every .backward() was called on, one per optimiser step
  restart_steps    the steps after which the reference drew its restart noise (target.py:127-132), seen as its uniform_ call
  restart_margins  cost[s] - cost[s - 10] at every restart test s = 20, 30, ..: how far each decision is from a tie
  lr_after, n_steps_run    the attack object's lr after the call (halved after step 50) and the optimiser steps it ran
  s<t>_*           for the steps LONG_KEEP (around the first restart and around the halving): w before, gradient, w / m / v
                   after, lr and Adam's step counter (make_golden.py's Instrument), for teacher forcing
The restart noise lands on the masked colours, which tanh_space(w) overwrites in the next step: the trajectory does not
depend on it, only on the clamp of all channels that comes with it.  So there is no seed to choose; the script refuses to
write a fixture in which a restart decision is closer to a tie than the fp32 cost bar of the tests (1e-4 |cost| + 0.02),
in which no restart happens or which does not cross step 50.
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
REF = "/root/reference/PointNet"
sys.path[:0] = [ROOT, REF, REF + "/models", REF + "/attacks"]
sys.dont_write_bytecode = True

from pointsecguard_amd.synthetic import make_rooms, pointnet_state_dict  # noqa: E402

import pointnet_sem_seg as ref  # noqa: E402  (reference)
import torchattacks  # noqa: E402  (reference)

sys.path.insert(0, HERE)
from make_golden import Instrument, _pack_adam  # noqa: E402

PN_SEED, ROOM_SEED = 3, 5
STEPS = 62
LONG_KEEP = (19, 20, 21, 49, 50, 51, 52)


def main():
    torch.set_num_threads(1)
    m = ref.get_model(13)
    m.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in pointnet_state_dict(PN_SEED).items()}, strict=True)
    m.eval()
    rooms = make_rooms(2, ROOM_SEED)
    x1 = torch.from_numpy(np.ascontiguousarray(rooms.transpose(0, 2, 1)))[:1]
    with torch.no_grad():
        pred = m(x1)[0].argmax(-1).numpy()
    mask = np.zeros(4096, bool)
    mask[::4] = True
    restarts = []
    torch.manual_seed(2)
    with Instrument() as inst:
        uniform_ = torch.Tensor.uniform_

        def counted(t, *a, **k):
            restarts.append(len(inst.adam) - 1)          # the step whose optimiser update has just been made
            return uniform_(t, *a, **k)

        torch.Tensor.uniform_ = counted
        try:
            atk = torchattacks.tar_NU_attack(m, c=0, kappa=1, steps=STEPS, lr=3.0, target=4, mask=mask)
            adv = atk(x1.clone(), pred.astype(np.float64)).detach()
        finally:
            torch.Tensor.uniform_ = uniform_
    costs = np.array(inst.costs, np.float64)
    n_run = len(inst.adam)
    tests = [s for s in range(20, n_run, 10)]
    margins = np.array([costs[s] - costs[s - 10] for s in tests])
    print("steps run", n_run, "lr after", atk.lr, "restarts after steps", restarts)
    print("restart tests", tests, "margins", margins.round(3).tolist())
    bar = 1e-4 * np.abs(costs[tests]) + 0.02
    assert restarts and n_run > 51, "the run must restart at least once and cross step 50"
    assert (np.abs(margins) > bar).all(), "a restart decision is a near-tie: %s against %s" % (margins, bar)
    assert [s for s, d in zip(tests, margins) if d >= 0] == restarts
    out = {"labels": pred.astype(np.int16), "mask": mask, "c": 0, "kappa": 1, "lr": 3.0, "steps": STEPS, "target": 4,
           "n_steps_run": n_run, "lr_after": float(atk.lr), "restart_steps": np.array(restarts, np.int32),
           "restart_tests": np.array(tests, np.int32), "restart_margins": margins,
           "adv_geometry": adv.numpy()[:, [0, 1, 2, 6, 7, 8]], "keep": np.array(LONG_KEEP)}
    _pack_adam(out, inst, LONG_KEEP)
    path = os.path.join(HERE, "pointnet_tarnu_long.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
