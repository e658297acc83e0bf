"""Plain references for the whole-scene NB attack kernels of csrc/psg_scene.hip.

TEST INFRASTRUCTURE ONLY: no GPU, no oracle import.  numpy float32, one IEEE operation per line, compared bit for bit.
A "slot" is a block row e = b * block_points + i; point_idx[e] names its scene point."""
import numpy as np

import attack_ref64

F = np.float32

MUTANTS = ("descending", "drop_last", "sum_of_signs", "box_first", "last_proj")


def occ_lists(point_idx, n_scene):
    """(occ_off [n_scene + 1], occ_ent [rows]): the slots of point p are occ_ent[occ_off[p] : occ_off[p + 1]], ascending."""
    idx = np.asarray(point_idx).reshape(-1).astype(np.int64)
    ent = np.argsort(idx, kind="stable").astype(np.int32)
    off = np.zeros(n_scene + 1, np.int32)
    off[1:] = np.cumsum(np.bincount(idx, minlength=n_scene))
    return off, ent


def colour_to_blocks(scene_rgb, point_idx, x):
    """x [rows][9] with channels 3:6 of every slot replaced by its point's colour"""
    x = x.copy()
    x.reshape(-1, 9)[:, 3:6] = scene_rgb[np.asarray(point_idx).reshape(-1)]
    return x


def rows_mask(dlogp, point_idx, scene_mask):
    """dlogp [rows][n_cls] with the rows of slots whose point is not under the mask set to +0.0"""
    out = dlogp.copy()
    off = ~np.asarray(scene_mask, bool)[np.asarray(point_idx).reshape(-1)]
    out.reshape(off.size, -1)[off] = F(0)
    return out


def grad_sum(dx0, occ_off, occ_ent, scene_mask=None, mutant=None):
    """g [n_scene][3] = ((0 + d[e_0]) + d[e_1]) + ... over the slots of every point in list order, d = dx0[e][3:6];
    +0 for a point outside the mask or without a slot.  One float32 addition per line (the loop runs over the position in
    the list; the points that still have an entry at that position advance together)."""
    d = np.ascontiguousarray(dx0.reshape(-1, 9)[:, 3:6]).astype(F)
    n_scene = occ_off.size - 1
    length = (occ_off[1:] - occ_off[:-1]).astype(np.int64)
    if mutant == "drop_last":
        length = np.maximum(length - 1, 0)
    on = np.ones(n_scene, bool) if scene_mask is None else np.asarray(scene_mask, bool)
    g = np.zeros((n_scene, 3), F)
    live = np.nonzero(on & (length > 0))[0]
    j = 0
    with np.errstate(invalid="ignore", over="ignore"):
        while live.size:
            pos = occ_off[live] + (length[live] - 1 - j if mutant == "descending" else j)
            term = d[occ_ent[pos]]
            if mutant == "sum_of_signs":
                term = np.where(term > 0, F(1), np.where(term < 0, F(-1), F(0))).astype(F)
            g[live] = (g[live] + term).astype(F)
            j += 1
            live = live[length[live] > j]
    return g


def scene_step(c, c0, dx0, occ_off, occ_ent, scene_mask, alpha, eps, direction, last, mutant=None):
    """(c after one step, g): the ordered float32 sum, then attack_ref64.pgd_step_field at c0 = 3 on the points that are
    under the mask and have at least one slot; every other point keeps its bytes."""
    assert mutant is None or mutant in MUTANTS
    g = grad_sum(dx0, occ_off, occ_ent, scene_mask, mutant if mutant in ("descending", "drop_last", "sum_of_signs") else None)
    n_scene = c.shape[0]
    moves = (occ_off[1:] - occ_off[:-1]) > 0
    if scene_mask is not None:
        moves = moves & np.asarray(scene_mask, bool)
    x = np.zeros((1, n_scene, 9), F)
    x[0, :, 3:6] = c
    grad = np.zeros((1, n_scene, 9), F)
    grad[0, :, 3:6] = g
    out = attack_ref64.pgd_step_field(x, grad, c0[None].astype(F), moves, 3, F(alpha), F(eps), F(direction), last,
                                      mutant=mutant if mutant in ("box_first", "last_proj") else None)
    return np.ascontiguousarray(out[0, :, 3:6]), g


# ------------------------------------------------------------------------------------------------ shared test inputs
def hand_made_index(seed=0, n_scene=700, rows=5003):
    """point_idx [rows] (rows no multiple of 64) over n_scene points: point 5 never occurs, point 9 occurs 3000 times, the
    rest 0 to a handful of times, all shuffled."""
    rng = np.random.default_rng(seed)
    others = np.array([p for p in range(n_scene) if p not in (5, 9)])
    idx = np.concatenate([np.full(3000, 9), rng.choice(others, rows - 3000, replace=True)])
    rng.shuffle(idx)
    assert idx.size == rows and rows % 64
    return idx.astype(np.int32), n_scene


def step_case(seed, point_idx, n_scene, eps=0.1):
    """(c, c0, dx0 [rows][9], mask) for psg_scene_pgd_step: gradients with exact zeros, pairs that cancel to zero, a NaN,
    an order-sensitive triple (1, 1e8, -1e8 in slot order: the float32 sum is 0 ascending and 1 descending), colours at the
    faces of the eps ball and of [0, 1] so that the step pushes past both."""
    rng = np.random.default_rng(seed)
    rows = point_idx.size
    off, ent = occ_lists(point_idx, n_scene)
    dx0 = rng.standard_normal((rows, 9)).astype(F)
    length = off[1:] - off[:-1]
    singles = np.nonzero(length == 1)[0]
    pairs = np.nonzero(length == 2)[0]
    triples = np.nonzero(length == 3)[0]
    assert singles.size >= 4 and pairs.size >= 2 and triples.size >= 1
    dx0[ent[off[singles[0]]], 3:6] = F(0)                                   # exact zero: the point gets sign 0
    dx0[ent[off[singles[1]]], 3:6] = F(-0.0)
    dx0[ent[off[singles[2]]], 4] = F(np.nan)                                # NaN: sign 0 as well
    a = ent[off[pairs[0]]: off[pairs[0]] + 2]
    dx0[a[1], 3:6] = -dx0[a[0], 3:6]                                        # a pair that cancels exactly
    t = ent[off[triples[0]]: off[triples[0]] + 3]
    dx0[t[0], 3:6], dx0[t[1], 3:6], dx0[t[2], 3:6] = F(1), F(1e8), F(-1e8)  # ascending: 0; descending: +1
    c0 = rng.random((n_scene, 3)).astype(F)
    c0[::7] = F(0)
    c0[3::7] = F(1)                                                         # at the faces of the box
    # clean values OUTSIDE the box (no scene has them, the arithmetic takes them): with the clean value inside [0, 1] "box
    # before ball" is the same real number as "ball before box"; these tell the two apart
    c0[1::7, 0] = F(1.2)
    c0[2::7, 1] = F(-0.2)
    c =np.clip(c0 + rng.choice(np.array([-eps, 0, eps], F), (n_scene, 3)), 0, 1).astype(F)     # and of the eps ball
    mask = rng.random(n_scene) < 0.5
    mask[[singles[0], singles[2], pairs[0], triples[0]]] = True
    return c, c0, dx0, mask
