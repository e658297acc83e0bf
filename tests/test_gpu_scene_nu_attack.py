"""GPU tests of the whole-scene NU attack (attacks/scene.py: SceneNUAttack): bit-equivalence with the
existing NU entry points driven block-wise where no blocks overlap; on an overlapping scene one colour per point, the block
gradients of stand-alone calls, every step teacher-forced through tests/scene_nu_ref.py; the integer exit; the targeted
variant; the MSG network; the evaluation loop around it.

Every scene is sliced at block_points = 1024 under np.random.seed(3), as in tests/test_gpu_scene_attack.py."""
import ctypes

import numpy as np
import pytest
import torch

import scene_nu_ref as ref
import scene_ref
from test_gpu_scene_attack import (Sliced, bits, check_one_colour_per_point, copies_disagree, dev, flat, msg_net, net,  # noqa: F401
                                   overlap, two_scene_dataset)

pytestmark = pytest.mark.gpu
F = np.float32
NEVER = (0, 1)                       # exit_below that cannot fire
KEYS = ("dx0", "sgrad", "pred", "w_before", "w_after", "m_after", "v_after", "c", "gsum_f", "gsum_s")


def run_nu(model, s, seed, steps=3, batch_size=4, record=False, **kw):
    from pointsecguard_amd.attacks.scene import SceneNUAttack
    trace_rows = []

    def trace(d):
        row = {k: (None if d[k] is None else d[k].cpu().numpy()) for k in KEYS}
        row.update(s=d["s"], active=d["active"], starts=[x.cpu().numpy() for x in d["starts"]])
        trace_rows.append(row)

    kw.setdefault("exit_below", NEVER)
    atk = SceneNUAttack(model, steps=steps, batch_size=batch_size, trace=trace if record else None, **kw)
    torch.manual_seed(seed)
    adv_rgb, adv_blocks = atk(s.data, s.index, s.label, s.rgb, s.labels)
    torch.cuda.synchronize()
    return adv_rgb.cpu().numpy(), adv_blocks.cpu().numpy(), trace_rows, atk


def off3(t):
    return ctypes.c_void_p(t.data_ptr() + 12)


def block_gradients(model_net, x0, x_clean, starts, labels, target, neighbour, tsign, slot_mask=None):
    """the per-step pieces of ONE batch through the existing entry points, stand-alone: (dx0, sgrad, pred) numpy"""
    from pointsecguard_amd import _lib, runtime
    b, n = x0.shape[0], x0.shape[1]
    ws = runtime.PN2Workspace(b, n, 1, arch=getattr(model_net, "ARCH", runtime.ARCH_SSG))
    model = model_net._packed()
    ws.plan_build(x0, starts, 1)
    logp = ws.forward(model, 0, x0, lean=True)
    dlogp, f_sum = torch.empty_like(logp), torch.zeros(b, dtype=torch.float32, device="cuda")
    pred = torch.empty(b, n, dtype=torch.int32, device="cuda")
    _lib.call("psg_nu_f_loss_grad_rooms", runtime.ptr(logp), runtime.ptr(labels), int(target), b, n, 13, 0.0, tsign,
              runtime.ptr(dlogp), runtime.ptr(f_sum), runtime.ptr(pred), runtime.stream())
    if slot_mask is not None:
        dlogp[~slot_mask] = 0.0
    dx0 = ws.backward(model, 0, dlogp, colour_only=True)
    sgrad = torch.empty(b, n, 3, dtype=torch.float32, device="cuda")
    nn = torch.empty(b, n, neighbour, dtype=torch.int32, device="cuda")
    _lib.call("psg_smooth_knn_rooms", off3(x0), 9, n * 9, off3(x_clean), 9, n * 9, b, n, neighbour, None, runtime.ptr(sgrad),
              runtime.ptr(nn), 0, runtime.stream())
    return dx0.cpu().numpy(), sgrad.cpu().numpy(), pred.cpu().numpy()


# ------------------------------------------------------------------------------------ where nothing overlaps
@pytest.mark.parametrize("seed", [5, 6])
def test_equals_the_block_wise_nu_entry_points_where_nothing_overlaps(net, flat, seed):
    """2 blocks in one batch, every scene point in exactly one slot: a one-entry list adds 0 + x, so w / m / v after every step
    and the returned blocks are, bit for bit, psg_nu_inverse_tanh, psg_nu_tanh_color_rooms, plan, forward_lean,
    psg_nu_f_loss_grad_rooms, colour backward, psg_smooth_knn_rooms, psg_nu_adam_step_rooms under the same seed."""
    from pointsecguard_amd import _lib, runtime
    from pointsecguard_amd.models.pointnet2_sem_seg import draw_fps_starts
    s, steps, n = flat, 3, 1024
    _, adv_blocks, rows, atk = run_nu(net, s, seed, steps=steps, batch_size=2, record=True)
    assert atk.last_exit_step == -1 and len(rows) == steps
    model = net._packed()
    x0 = dev(s.blocks)
    ori = x0[:, :, 3:6].contiguous()
    labels = dev(s.label.astype(np.int32))
    f32 = lambda *shape: torch.zeros(*shape, dtype=torch.float32, device="cuda")       # noqa: E731
    w, m, v, sgrad, f_sum = f32(2, n, 3), f32(2, n, 3), f32(2, n, 3), f32(2, n, 3), f32(2)
    dlogp, pred = f32(2, n, 13), torch.zeros(2, n, dtype=torch.int32, device="cuda")
    nn = torch.zeros(2, n, 10, dtype=torch.int32, device="cuda")
    ws = runtime.PN2Workspace(2, n, 1)
    st = runtime.stream
    _lib.call("psg_nu_inverse_tanh", runtime.ptr(x0), 2, n, runtime.ptr(w), st())
    flat_idx = s.index.reshape(-1)
    torch.manual_seed(seed)
    for t in range(steps):
        _lib.call("psg_nu_tanh_color_rooms", runtime.ptr(w), None, 2, n, runtime.ptr(x0), st())
        ws.plan_build(x0, draw_fps_starts(2, n, 1).cuda(), 1)
        logp = ws.forward(model, 0, x0, lean=True)
        _lib.call("psg_nu_f_loss_grad_rooms", runtime.ptr(logp), runtime.ptr(labels), 0, 2, n, 13, 0.0, 1.0, runtime.ptr(dlogp),
                  runtime.ptr(f_sum), runtime.ptr(pred), st())
        dx0 = ws.backward(model, 0, dlogp, colour_only=True)
        _lib.call("psg_smooth_knn_rooms", off3(x0), 9, n * 9, runtime.ptr(ori), 3, n * 3, 2, n, 10, None, runtime.ptr(sgrad),
                  runtime.ptr(nn), 1 if t > 0 else 0, st())
        if t < steps - 1:
            _lib.call("psg_nu_adam_step_rooms", runtime.ptr(w), runtime.ptr(m), runtime.ptr(v), None, runtime.ptr(dx0),
                      runtime.ptr(x0), runtime.ptr(ori), runtime.ptr(sgrad), 1e-4, 1e-4, 0.01, 0.9, 0.999, 1e-8, t + 1, 2, n, None,
                      None, st())
        row = rows[t]
        assert np.array_equal(bits(row["dx0"].reshape(-1, 9)[:, 3:6]), bits(dx0.cpu().numpy().reshape(-1, 9)[:, 3:6])), t
        assert np.array_equal(bits(row["sgrad"]), bits(sgrad.cpu().numpy())) and np.array_equal(row["pred"], pred.cpu().numpy()), t
        for name, mine in (("w_after", w), ("m_after", m), ("v_after", v)):
            same = float((bits(row[name][flat_idx]) == bits(mine.cpu().numpy().reshape(-1, 3))).mean())
            print("step %d %s: bit-equal share %.6f" % (t, name, same))
            assert same == 1.0, (t, name)
    pieces = x0.cpu().numpy()
    assert not np.array_equal(bits(pieces[:, :, 3:6]), bits(s.blocks[:, :, 3:6]))
    same = float((bits(adv_blocks) == bits(pieces)).mean())
    print("scene NU attack vs block-wise pieces: bit-equal share %.6f" % same)
    assert same == 1.0
    assert (bits(rows[1]["w_after"]) != bits(rows[0]["w_before"])).mean() > 0.9


# ------------------------------------------------------------------------------------ on the overlapping scene
@pytest.fixture(scope="module")
def overlap_run(net, overlap):
    return run_nu(net, overlap, 7, record=True)


def check_step0_blocks(model_net, s, row, batch_size, labels, target, neighbour, tsign, mask=None):
    """step 0: the recorded slice of every batch is a stand-alone call on the blocks that carry the step's colours"""
    nb = s.blocks.shape[0]
    x_all = scene_ref.colour_to_blocks(row["c"], s.index, s.blocks)
    batches = [(lo, min(lo + batch_size, nb)) for lo in range(0, nb, batch_size)]
    assert len(row["starts"]) == len(batches)
    for k, (lo, hi) in enumerate(batches):
        slot_mask = None if mask is None else dev(mask[s.index[lo:hi]])
        dx0, sgrad, pred = block_gradients(model_net, dev(x_all[lo:hi]), dev(s.blocks[lo:hi]), dev(row["starts"][k]),
                                           None if labels is None else dev(labels[lo:hi].astype(np.int32)), target, neighbour, tsign,
                                           slot_mask)
        assert np.abs(dx0[:, :, 3:6]).max() > 0 and np.abs(sgrad).max() > 0
        assert np.array_equal(bits(dx0[:, :, 3:6]), bits(row["dx0"][lo:hi][:, :, 3:6])), k
        assert np.array_equal(bits(sgrad), bits(row["sgrad"][lo:hi])), k
        assert np.array_equal(pred, row["pred"][lo:hi]), k


def check_teacher_forced(s, rows, mask, cw=1e-4, lr=0.01):
    """every step from its recorded inputs: the ordered sums bit for bit, w / m / v and the colours within the bound"""
    n = s.n_scene
    on = ref.moves(s.off, mask)
    w0, e0 = ref.init64(s.c0)
    assert ref.within(rows[0]["w_before"], w0, e0).all()
    m_before, v_before = np.zeros((n, 3), F), np.zeros((n, 3), F)
    worst = dict(w=0.0, m=0.0, v=0.0, c=0.0)
    for t, row in enumerate(rows):
        assert row["s"] == t
        if t:
            assert np.array_equal(bits(row["w_before"]), bits(rows[t - 1]["w_after"]))
        c64, ce, written = ref.colour64(row["w_before"], s.c0, s.off, mask)
        assert np.array_equal(written, on) and ref.within(row["c"][on], c64[on], ce[:, on]).all()
        assert np.array_equal(bits(row["c"][~on]), bits(s.c0[~on]))
        worst["c"] = max(worst["c"], ref.ratio(row["c"][on], c64[on], ce[:, on]))
        if row["gsum_f"] is None:                                  # the last step: no optimiser step follows it
            assert t == len(rows) - 1 and np.array_equal(bits(row["w_after"]), bits(row["w_before"]))
            assert np.array_equal(bits(row["m_after"]), bits(m_before)) and np.array_equal(bits(row["v_after"]), bits(v_before))
            continue
        dx0, sgrad = row["dx0"].reshape(-1, 9), row["sgrad"].reshape(-1, 3)
        w64, m64, v64, we, me, ve, gf, gs = ref.step64(row["w_before"], m_before, v_before, row["c"], s.c0, dx0, sgrad, s.off, s.ent,
                                                       mask, cw, lr, t + 1)
        assert np.array_equal(bits(row["gsum_f"]), bits(gf)) and np.array_equal(bits(row["gsum_s"]), bits(gs)), t
        for name, got, want, e in (("w", row["w_after"], w64, we), ("m", row["m_after"], m64, me), ("v", row["v_after"], v64, ve)):
            worst[name] = max(worst[name], ref.ratio(got[on], want[on], e[:, on]))
            assert ref.within(got[on], want[on], e[:, on]).all(), (t, name)
            assert np.array_equal(bits(got[~on]), bits((row["w_before"] if name == "w" else m_before if name == "m" else v_before)[~on]))
        m_before, v_before = row["m_after"], row["v_after"]
    print("teacher-forced steps: largest error / first-order bound %s" % worst)


def test_one_colour_per_point_and_clean_channels(overlap, overlap_run):
    adv_rgb, adv_blocks, rows, atk = overlap_run
    check_one_colour_per_point(overlap, adv_rgb, adv_blocks)
    assert not np.array_equal(bits(adv_rgb), bits(overlap.c0)) and adv_rgb.min() >= 0.0 and adv_rgb.max() <= 1.0
    assert atk.last_exit_step == -1 and atk.last_history.shape == (3, 2) and atk.last_history.dtype == np.int64
    assert (atk.last_history[:, 1] == 18 * 1024).all() and atk.last_w.is_cuda
    assert np.array_equal(bits(adv_rgb), bits(rows[-1]["c"]))      # the colours of the last forward
    for row in rows:                                               # the recorded counts are the recorded predictions'
        assert tuple(atk.last_history[row["s"]]) == ref.latch_counts(row["pred"], overlap.label, 0, overlap.index, None)


def test_first_step_gradients_are_the_block_gradients(net, overlap, overlap_run):
    check_step0_blocks(net, overlap, overlap_run[2][0], 4, overlap.label, 0, 10, 1.0)


def test_every_step_is_the_restated_step(overlap, overlap_run):
    rows = overlap_run[2]
    assert [r["s"] for r in rows] == [0, 1, 2] and all(r["active"] == 1 for r in rows)
    check_teacher_forced(overlap, rows, None)


def test_seeded_runs_return_the_same_bytes(net, overlap, overlap_run):
    adv_rgb, adv_blocks, _, _ = run_nu(net, overlap, 7)            # and tracing changes nothing
    assert np.array_equal(bits(adv_rgb), bits(overlap_run[0])) and np.array_equal(bits(adv_blocks), bits(overlap_run[1]))


def test_the_block_attack_recolours_a_point_per_block(net, overlap, overlap_run):
    """teeth: NU_attack.forward_rooms over the same blocks in groups of 4 leaves the copies of one point with different colours.
    Its exit (correct / 4096 < 1 / 13, the reference's literal) is kept from firing by attacking the network's own clean
    predictions: 1024 correct points per block at step 0."""
    from pointsecguard_amd.attacks import torchattacks
    s = overlap
    torch.manual_seed(7)
    out = np.empty_like(s.blocks)
    for lo in range(0, 18, 4):
        hi = min(lo + 4, 18)
        images = dev(np.ascontiguousarray(s.blocks[lo:hi].transpose(0, 2, 1)))
        labels = net(images)[0].argmax(dim=2).cpu().numpy()
        adv, steps_run = torchattacks.NU_attack(net, steps=3).forward_rooms(images, labels)
        assert (np.asarray(steps_run) == 3).all()
        out[lo:hi] = adv.cpu().numpy().transpose(0, 2, 1)
    share_blocks, share_scene = copies_disagree(s, out), copies_disagree(s, overlap_run[1])
    print("multi-occurrence points whose copies disagree: per-block NU attack %.4f, scene NU attack %.4f" % (share_blocks, share_scene))
    assert share_blocks > 0.5 and share_scene == 0.0


# ------------------------------------------------------------------------------------ the exit latch
def test_exit_at_the_step_the_integer_rule_gives(net, overlap):
    s = overlap
    _, _, rows, atk = run_nu(net, s, 13, steps=4, record=True)
    hist = atk.last_history
    assert hist.shape == (4, 2) and atk.last_exit_step == -1 and (hist[:, 1] == 18 * 1024).all()
    hits, n = hist[:, 0].tolist(), int(hist[0, 1])
    later = [t for t in range(1, 4) if hits[t] < min(hits[:t])]
    at = later[0] if later else 0
    num, den = hits[at] + 1, n                                     # fires where n_hits <= hits[at]: first at step `at`
    want = ref.first_exit(hist, num, den, False)
    print("recorded n_hits %s of %d -> exit_below = (%d, %d), exit expected at step %d" % (hits, n, num, den, want))
    assert want == at
    runs = {ce: run_nu(net, s, 13, steps=4, exit_below=(num, den), check_every=ce) for ce in (1, 10)}
    for ce, (adv_rgb, adv_blocks, _, a) in runs.items():
        assert a.last_exit_step == want, ce
        assert np.array_equal(a.last_history, hist[:want + 1]), ce
        assert np.array_equal(bits(adv_rgb), bits(rows[want]["c"])), ce
        check_one_colour_per_point(s, adv_rgb, adv_blocks)
    assert np.array_equal(bits(runs[1][1]), bits(runs[10][1]))
    # traced, the loop stops at the exit step and hands over the same bytes
    adv_rgb, _, traced, a = run_nu(net, s, 13, steps=4, exit_below=(num, den), record=True)
    assert a.last_exit_step == want and [r["active"] for r in traced] == [1] * want + [0]
    assert np.array_equal(bits(adv_rgb), bits(rows[want]["c"])) and traced[-1]["gsum_f"] is None
    assert np.array_equal(bits(traced[-1]["w_after"]), bits(traced[-1]["w_before"]))


# ------------------------------------------------------------------------------------ targeted
def test_targeted_moves_points_of_the_origin_class_only(net, overlap):
    s = overlap
    origin = int(np.bincount(s.labels.astype(np.int64)).argmax())
    target = (origin + 1) % 13
    adv_rgb, adv_blocks, rows, atk = run_nu(net, s, 9, record=True, target=target, origin=origin, exit_above=(1, 1))
    mask = s.labels == origin
    assert 0 < mask.sum() < s.n_scene and atk.neighbour == 5 and atk.last_exit_step == -1
    assert np.array_equal(bits(adv_rgb[~mask]), bits(s.c0[~mask]))
    assert (bits(adv_rgb[mask]) != bits(s.c0[mask])).any()
    check_one_colour_per_point(s, adv_rgb, adv_blocks)
    check_step0_blocks(net, s, rows[0], 4, None, target, 5, -1.0, mask=mask)
    check_teacher_forced(s, rows, mask)
    for row in rows:
        assert tuple(atk.last_history[row["s"]]) == ref.latch_counts(row["pred"], None, target, s.index, mask)
    # a scene without a slot of the origin class is refused before the loop
    elsewhere = np.where(s.labels == origin, target, s.labels)
    from pointsecguard_amd.attacks.scene import SceneNUAttack
    with pytest.raises(ValueError):
        SceneNUAttack(net, steps=1, target=target, origin=origin)(s.data, s.index, s.label, s.rgb, elsewhere)


# ------------------------------------------------------------------------------------ MSG
def test_msg_network(msg_net, overlap):
    adv_rgb, adv_blocks, rows, atk = run_nu(msg_net, overlap, 11, steps=2, record=True)
    check_one_colour_per_point(overlap, adv_rgb, adv_blocks)
    assert not np.array_equal(bits(adv_rgb), bits(overlap.c0)) and atk.last_exit_step == -1
    check_step0_blocks(msg_net, overlap, rows[0], 4, overlap.label, 0, 10, 1.0)


# ------------------------------------------------------------------------------------ the evaluation loop, refusals
def test_consistent_whole_scene_loop_with_the_nu_attack(net):
    from pointsecguard_amd import harness
    from pointsecguard_amd.attacks.scene import SceneNUAttack
    ds = two_scene_dataset()
    handed = []
    np.random.seed(3)
    torch.manual_seed(3)
    res = harness.evaluate_whole_scene_consistent(net, ds, lambda m: SceneNUAttack(m, steps=2, exit_below=NEVER), batch_size=4,
                                                  log=lambda *_: None, on_scene=lambda name, rgb: handed.append((name, rgb)))
    assert [name for name, _ in handed] == ["Area_5_a", "Area_5_b"]
    for si, (_, rgb) in enumerate(handed):
        c0 = (ds.scene_points_list[si][:, 3:6] / 255.0).astype(F)
        assert rgb.shape == c0.shape and rgb.dtype == np.float32 and not np.array_equal(rgb, c0)
        assert rgb.min() >= 0.0 and rgb.max() <= 1.0
    np.random.seed(3)
    torch.manual_seed(3)
    clean = harness.evaluate_whole_scene(net, ds, None, batch_size=4, log=lambda *_: None)
    assert np.array_equal(clean["counters"][0], res["counters"][0])
    assert res["counters"][1][0].sum() == 8000


def test_refusals(net, flat):
    from pointsecguard_amd.attacks.scene import SceneNUAttack
    from pointsecguard_amd.models import pointnet_sem_seg
    with pytest.raises(NotImplementedError):
        SceneNUAttack(pointnet_sem_seg.get_model(13).cuda().eval())
    broken = flat.index.copy()
    broken[1, 7] = flat.n_scene
    with pytest.raises(IndexError):
        SceneNUAttack(net, steps=1, batch_size=2)(flat.data, broken, flat.label, flat.rgb, flat.labels)
