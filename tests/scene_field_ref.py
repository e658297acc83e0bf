"""Plain references for the coordinate field of the whole-scene NB attack (csrc/psg_scene.hip: psg_scene_delta_to_blocks,
psg_scene_field_step).

TEST INFRASTRUCTURE ONLY: no GPU, no oracle import.  numpy float32, one IEEE operation per line, compared bit for bit.  The
variable is delta [n_scene][3] (metres): a slot e holds x[e][0:3] = fl32(x_clean[e][0:3] + delta[point_idx[e]])."""
import numpy as np

import scene_ref

F = np.float32

MUTANTS = ("descending", "drop_last", "sum_of_signs", "no_clamp", "box", "last_proj")
SUM_MUTANTS = ("descending", "drop_last", "sum_of_signs")


def delta_to_blocks(delta, point_idx, x_clean, x, mutant=None):
    """x [rows][9] with channels 0:3 of every slot replaced by the CLEAN coordinate plus its point's displacement; the other
    six channels keep the bytes of x.  mutant "onto_moved": the displacement is added onto x's own (already moved) channels."""
    assert mutant in (None, "onto_moved")
    out = x.copy()
    base = (x if mutant == "onto_moved" else x_clean).reshape(-1, 9)[:, 0:3].astype(F)
    moved = (base + delta[np.asarray(point_idx).reshape(-1)].astype(F)).astype(F)
    out.reshape(-1, 9)[:, 0:3] = moved
    return out


def grad_sum(dx0, occ_off, occ_ent, scene_mask=None, mutant=None):
    """g [n_scene][3] = ((0 + d[e_0]) + d[e_1]) + ... with d = dx0[e][0:3]: scene_ref.grad_sum's walk (it reads channels
    3:6) on a copy that carries the coordinate channels there."""
    shifted = np.zeros((dx0.reshape(-1, 9).shape[0], 9), F)
    shifted[:, 3:6] = dx0.reshape(-1, 9)[:, 0:3]
    return scene_ref.grad_sum(shifted, occ_off, occ_ent, scene_mask, mutant)


def field_step(delta, dx0, occ_off, occ_ent, scene_mask, alpha, eps, direction, last, mutant=None):
    """(delta after one step, g): points under the mask with at least one slot take
    delta = last ? delta + step * sign(g) : clamp(delta + step * sign(g), -eps, +eps); every other point keeps its bytes."""
    assert mutant is None or mutant in MUTANTS
    g = grad_sum(dx0, occ_off, occ_ent, scene_mask, mutant if mutant in SUM_MUTANTS else None)
    moves = (occ_off[1:] - occ_off[:-1]) > 0
    if scene_mask is not None:
        moves = moves & np.asarray(scene_mask, bool)
    step = F(F(direction) * F(alpha))
    eps = F(eps)
    sg = np.where(g > 0, F(1), np.where(g < 0, F(-1), F(0))).astype(F)
    move = (step * sg).astype(F)
    stepped = (delta.astype(F) + move).astype(F)
    low = np.maximum(stepped, -eps)
    clamped = np.minimum(low, eps)
    if mutant == "no_clamp":
        clamped = stepped
    if mutant == "box":
        clamped = np.minimum(np.maximum(clamped, F(0)), F(1))
    new = stepped if (last and mutant != "last_proj") else clamped
    out = delta.astype(F).copy()
    out[moves] = new[moves]
    return out, g


# ------------------------------------------------------------------------------------------------ shared test inputs
def field_case(seed, point_idx, n_scene, eps=0.1):
    """(delta, dx0 [rows][9], mask): scene_ref.step_case's gradients (exact zeros, a cancelling pair, a NaN, the
    order-sensitive triple 1, 1e8, -1e8) carried to channels 0:3, with other random numbers left in 3:9; displacements at
    0 and at both faces of the eps ball, so that a step pushes past either face and a [0, 1] box would cut the negative ones."""
    _, _, dx0_c, mask = scene_ref.step_case(seed, point_idx, n_scene, eps=eps)
    rng = np.random.default_rng(seed + 100)
    dx0 = rng.standard_normal(dx0_c.shape).astype(F)
    dx0[:, 0:3] = dx0_c[:, 3:6]
    delta = rng.choice(np.array([-eps, 0, eps], F), (n_scene, 3)).astype(F)
    return delta, dx0, mask
