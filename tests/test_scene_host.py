"""CPU tests of the whole-scene NB attack: the plain references of tests/scene_ref.py against brute
force and against attack_ref64, the mutants each of them must catch, the slicer premises the GPU tests rest on, and the
argument checks that need no device."""
import numpy as np
import pytest
import torch

import attack_ref64
import scene_ref
from test_gpu_harness import synth_scene

F = np.float32


def bits(a):
    return np.ascontiguousarray(a, F).view(np.uint32)


def slice_scene(scene, seed=3, block_points=1024):
    from pointsecguard_amd import harness
    ds = harness.ScannetDatasetWholeScene(None, block_points=block_points, scenes={"Area_5_a.npy": scene})
    np.random.seed(seed)
    return ds, ds[0]


def test_occ_lists_vs_brute_force():
    idx, n_scene = scene_ref.hand_made_index()
    off, ent = scene_ref.occ_lists(idx, n_scene)
    lists = {}
    for e, p in enumerate(idx.tolist()):
        lists.setdefault(p, []).append(e)
    assert 5 not in lists and len(lists[9]) == 3000 and len(lists[9]) > 2000
    assert off[0] == 0 and off[-1] == idx.size
    for p in range(n_scene):
        assert ent[off[p]:off[p + 1]].tolist() == lists.get(p, []), p
    assert off[6] == off[5]                                     # the empty point


def test_scene_step_equals_pgd_step_where_nothing_overlaps():
    rng = np.random.default_rng(4)
    n = 777
    idx = rng.permutation(n).astype(np.int32)                   # every point exactly once, in some block order
    off, ent = scene_ref.occ_lists(idx, n)
    dx0 = rng.standard_normal((n, 9)).astype(F)
    dx0[::11, 3:6] = 0
    c0 = rng.random((n, 3)).astype(F)
    c = np.clip(c0 + F(0.1) * rng.choice(np.array([-1, 0, 1], F), (n, 3)), 0, 1).astype(F)
    for last in (False, True):
        for direction in (1.0, -1.0):
            for mask in (None, rng.random(n) < 0.5):
                got, g = scene_ref.scene_step(c, c0, dx0, off, ent, mask, 0.05, 0.1, direction, last)
                # the same step in block order: x, grad, ori are the scene's rows gathered into the slots
                x = np.zeros((1, n, 9), F)
                x[0, :, 3:6] = c[idx]
                want = attack_ref64.pgd_step(x, dx0[None], c0[idx][None], None if mask is None else mask[idx], F(0.05), F(0.1),
                                             F(direction), last)
                assert np.array_equal(bits(got[idx]), bits(want[0, :, 3:6]))
                on = np.ones(n, bool) if mask is None else mask
                assert np.array_equal(g[idx][on[idx]] == 0, dx0[:, 3:6][on[idx]] == 0)
                assert np.array_equal(g[idx][on[idx]], dx0[:, 3:6][on[idx]])


def test_scene_step_mutants_are_caught():
    idx, n_scene = scene_ref.hand_made_index()
    off, ent = scene_ref.occ_lists(idx, n_scene)
    c, c0, dx0, mask = scene_ref.step_case(7, idx, n_scene, eps=0.1)
    for m in (None, mask):
        good = {last: scene_ref.scene_step(c, c0, dx0, off, ent, m, 0.05, 0.1, 1.0, last)[0] for last in (False, True)}
        for mutant in scene_ref.MUTANTS:
            caught = False
            for last in (False, True):
                bad, _ = scene_ref.scene_step(c, c0, dx0, off, ent, m, 0.05, 0.1, 1.0, last, mutant=mutant)
                caught = caught or not np.array_equal(bits(bad), bits(good[last]))
            assert caught, mutant
    # the descending order is caught by the SIGN of the order-sensitive triple alone (1 + 1e8 - 1e8 in float32)
    length = off[1:] - off[:-1]
    p = np.nonzero(length == 3)[0][0]
    g_up = scene_ref.grad_sum(dx0, off, ent)[p]
    g_down = scene_ref.grad_sum(dx0, off, ent, mutant="descending")[p]
    assert (g_up == 0).all() and (g_down == 1).all()
    # a point without a slot keeps its bytes; so does a point outside the mask
    out, g = scene_ref.scene_step(c, c0, dx0, off, ent, mask, 0.05, 0.1, -1.0, False)
    assert np.array_equal(bits(out[5]), bits(c[5])) and np.array_equal(bits(out[~mask]), bits(c[~mask]))
    assert (g[~mask] == 0).all() and (g[5] == 0).all()


def test_rows_mask_and_colour_to_blocks_vs_plain_loops():
    rng = np.random.default_rng(3)
    n_scene = 90
    idx = rng.integers(0, n_scene, 333).astype(np.int32)
    dlogp = rng.standard_normal((idx.size, 13)).astype(F)
    mask = rng.random(n_scene) < 0.4
    want = dlogp.copy()
    for e in range(idx.size):
        if not mask[idx[e]]:
            for k in range(13):
                want[e, k] = F(0)
    got = scene_ref.rows_mask(dlogp, idx, mask)
    assert np.array_equal(bits(got), bits(want)) and not np.signbit(got[~mask[idx]]).any()
    rgb = rng.random((n_scene, 3)).astype(F)
    x = rng.standard_normal((idx.size, 9)).astype(F)
    want = x.copy()
    for e in range(idx.size):
        for k in range(3):
            want[e, 3 + k] = rgb[idx[e], k]
    assert np.array_equal(bits(scene_ref.colour_to_blocks(rgb, idx, x)), bits(want))


def test_slicer_premises_of_the_gpu_tests():
    # a room smaller than one block: one window, 2048 points -> 2 blocks, every point exactly once
    scene = synth_scene(21, 2048, 0.9, 0.9)
    _, (data, _, _, index) = slice_scene(scene)
    assert data.shape == (2, 1024, 9)
    assert np.array_equal(np.bincount(index.reshape(-1), minlength=2048), np.ones(2048, np.int64))
    # the overlapping room of test_whole_scene_loop_end_to_end
    scene = synth_scene(11, 5000, 1.6, 1.2)
    _, (data, _, _, index) = slice_scene(scene)
    assert data.shape == (18, 1024, 9)
    counts = np.bincount(index.reshape(-1), minlength=5000)
    assert counts.min() >= 1
    assert abs(float((counts > 1).mean()) - 0.9038) < 5e-5
    assert abs(float(counts.mean()) - 3.69) < 5e-3 and counts.max() == 11
    # the scene's clean colours are the bits the slicer puts into channels 3:6 of every slot
    c0 = (scene[:, 3:6] / 255.0).astype(F)
    assert np.array_equal(bits(c0[index.reshape(-1)]), bits(data.reshape(-1, 9)[:, 3:6].astype(F)))


def test_argument_checks_without_a_device(tmp_path):
    from pointsecguard_amd import _lib, harness
    from pointsecguard_amd.attacks.scene import SceneNBAttack
    from pointsecguard_amd.models import pointnet2_sem_seg, pointnet_sem_seg
    ds, (data, label, _, index) = slice_scene(synth_scene(21, 2048, 0.9, 0.9))
    pn2 = pointnet2_sem_seg.get_model(13).eval()                 # on the CPU: there is no CPU path
    with pytest.raises(_lib.PsgError):
        harness.evaluate_whole_scene_consistent(pn2, ds, lambda m: SceneNBAttack(m, 0.1, 0.05, 1), log=lambda *_: None)
    atk = SceneNBAttack(pn2, 0.1, 0.05, 1)
    with pytest.raises(_lib.PsgError):
        atk(torch.from_numpy(data.astype(F)), torch.from_numpy(index.astype(np.int32)), torch.from_numpy(label.astype(np.int32)),
            ds.scene_points_list[0][:, 3:6], ds.semantic_labels_list[0])
    vanilla = pointnet_sem_seg.get_model(13).eval()
    with pytest.raises(NotImplementedError):
        SceneNBAttack(vanilla, 0.1, 0.05, 1)
    with pytest.raises(NotImplementedError):
        harness.evaluate_whole_scene_consistent(vanilla, ds, lambda m: SceneNBAttack(m, 0.1, 0.05, 1), log=lambda *_: None)
    with pytest.raises(ValueError):
        SceneNBAttack(pn2, 0.1, 0.05, 1, target=3)               # targeted needs the origin class as well
