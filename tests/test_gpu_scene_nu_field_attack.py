"""GPU tests of the whole-scene NU attack on the coordinate field (attacks/scene.py: SceneNUAttack(field="coord" | "both");
DESIGN.md section 5z): Adam on ONE displacement per scene point.  Bit-equivalence with the coordinate-field NU entry points
driven block-wise where no blocks overlap; on an overlapping scene the slots, the block gradients of stand-alone calls, every
step teacher-forced through tests/scene_nu_field_ref.py; the integer exit; the targeted variant; both fields; the premise;
one batch against float64; the MSG refusal; the evaluation loop around it.

Every scene is sliced at block_points = 1024 under np.random.seed(3), as in tests/test_gpu_scene_attack.py; steps = 3,
batch_size = 4 and exit_below = (0, 1) unless a test says otherwise."""
import numpy as np
import pytest
import torch

import pn2_ref64
import scene_field_ref
import scene_nu_field_ref as ref
import scene_nu_ref
import scene_ref
from test_gpu_nu_field import f_loss64
from test_gpu_pn2_fullgrad import FLIP_BAR, MEDIAN_BAR, SIGN_BAR, coord_bars, plan_tables
from test_gpu_scene_attack import Sliced, bits, dev, flat, msg_net, net, overlap, two_scene_dataset  # noqa: F401
from test_gpu_scene_field_attack import copies_displaced_differently
from test_gpu_scene_nu_attack import KEYS, NEVER, off3, run_nu

pytestmark = pytest.mark.gpu
F = np.float32
FIELD_KEYS = ("delta_before", "delta_after", "mx_after", "vx_after", "sgrad_xyz", "gsum_x", "gsum_sx")
BATCHES = [(lo, min(lo + 4, 18)) for lo in range(0, 18, 4)]
CC, CLR = 1e-4, 0.01                  # coord_c / coord_lr: the fall-backs to c / lr


def run_field(model, s, seed, field="coord", steps=3, batch_size=4, record=False, **kw):
    """-> dict(rgb, blocks, delta, rows, atk): the attack's two results, last_delta and (record) every step's trace as numpy"""
    from pointsecguard_amd.attacks.scene import SceneNUAttack
    rows = []

    def trace(d):
        assert sorted(d) == sorted(KEYS + FIELD_KEYS + ("s", "active", "starts"))
        row = {k: (None if d[k] is None else d[k].cpu().numpy()) for k in KEYS + FIELD_KEYS}
        row.update(s=d["s"], active=d["active"], starts=[x.cpu().numpy() for x in d["starts"]])
        rows.append(row)

    kw.setdefault("exit_below", NEVER)
    atk = SceneNUAttack(model, steps=steps, batch_size=batch_size, trace=trace if record else None, field=field, **kw)
    torch.manual_seed(seed)
    adv_rgb, adv_blocks = atk(s.data, s.index, s.label, s.rgb, s.labels)
    torch.cuda.synchronize()
    for t in (atk.last_delta, atk.last_mx, atk.last_vx):
        assert t.is_cuda and tuple(t.shape) == (s.n_scene, 3) and t.dtype == torch.float32
    return dict(rgb=adv_rgb.cpu().numpy(), blocks=adv_blocks.cpu().numpy(), delta=atk.last_delta.cpu().numpy(), rows=rows, atk=atk)


@pytest.fixture(scope="module")
def coord_run(net, overlap):
    return run_field(net, overlap, 7, record=True)


@pytest.fixture(scope="module")
def both_run(net, overlap):
    return run_field(net, overlap, 7, field="both", record=True)


def moved_blocks(s, delta, rgb=None):
    """the slots of the clean blocks with delta added (and, for both fields, the scene's colours written): the restatement of
    psg_scene_delta_to_blocks (and psg_scene_colour_to_blocks)"""
    clean = s.blocks.reshape(-1, 9)
    x = scene_field_ref.delta_to_blocks(delta, s.index, clean, clean).reshape(s.blocks.shape)
    return x if rgb is None else scene_ref.colour_to_blocks(rgb, s.index, x)


def check_slots_agree_with_the_scene(s, run, colours_clean):
    flat_adv, clean = run["blocks"].reshape(-1, 9), s.blocks.reshape(-1, 9)
    want = (clean[:, 0:3] + run["delta"][s.index.reshape(-1)]).astype(F)
    assert np.array_equal(bits(flat_adv[:, 0:3]), bits(want))
    assert np.array_equal(bits(flat_adv[:, 6:9]), bits(clean[:, 6:9]))
    if colours_clean:
        assert np.array_equal(bits(flat_adv[:, 3:6]), bits(clean[:, 3:6])) and np.array_equal(bits(run["rgb"]), bits(s.c0))
    else:
        assert np.array_equal(bits(flat_adv[:, 3:6]), bits(run["rgb"][s.index.reshape(-1)]))


def block_pieces(model_net, x0, x_clean, starts, labels, target, neighbour, tsign, slot_mask=None, full=True, colour=False):
    """the per-step pieces of ONE batch through the existing entry points, stand-alone: dict(dx0, sgrad_xyz, pred, tables[,
    sgrad]) as numpy.  full=False: psg_pn2_backward (the feature path alone) in the place of psg_pn2_backward_full."""
    from pointsecguard_amd import _lib, runtime
    b, n = x0.shape[0], x0.shape[1]
    ws = runtime.PN2Workspace(b, n, 1)
    model = model_net._packed()
    ws.plan_build(x0, starts, 1)
    logp = ws.forward(model, 0, x0, lean=True)
    dlogp, f_sum = torch.empty_like(logp), torch.zeros(b, dtype=torch.float32, device="cuda")
    pred = torch.empty(b, n, dtype=torch.int32, device="cuda")
    _lib.call("psg_nu_f_loss_grad_rooms", runtime.ptr(logp), runtime.ptr(labels), int(target), b, n, 13, 0.0, tsign,
              runtime.ptr(dlogp), runtime.ptr(f_sum), runtime.ptr(pred), runtime.stream())
    if slot_mask is not None:
        dlogp[~slot_mask] = 0.0
    dx0 = ws.backward(model, 0, dlogp, full=True) if full else ws.backward(model, 0, dlogp)
    sgrad_xyz = torch.empty(b, n, 3, dtype=torch.float32, device="cuda")
    _lib.call("psg_smooth_knn_xyz_rooms", runtime.ptr(x0), 9, n * 9, runtime.ptr(x_clean), 9, n * 9, b, n, neighbour, None,
              runtime.ptr(sgrad_xyz), None, None, runtime.stream())
    out = dict(dx0=dx0.cpu().numpy(), sgrad_xyz=sgrad_xyz.cpu().numpy(), pred=pred.cpu().numpy(), tables=plan_tables(ws, b))
    if colour:
        sgrad = torch.empty(b, n, 3, dtype=torch.float32, device="cuda")
        nn = torch.empty(b, n, neighbour, dtype=torch.int32, device="cuda")
        _lib.call("psg_smooth_knn_rooms", off3(x0), 9, n * 9, off3(x_clean), 9, n * 9, b, n, neighbour, None, runtime.ptr(sgrad),
                  runtime.ptr(nn), 0, runtime.stream())
        out["sgrad"] = sgrad.cpu().numpy()
    return out


def check_blocks_of_every_step(model_net, s, rows, labels, target, neighbour, tsign, mask=None, both=False):
    """at every step the recorded slice of every batch - dx0 (all nine channels), sgrad_xyz, pred - is a stand-alone call on
    the blocks that carry the step's displacements (and colours) with the traced starts"""
    for row in rows:
        x_all = moved_blocks(s, row["delta_before"], row["c"] if both else None)
        if row["s"] == 0:
            assert np.array_equal(bits(x_all[:, :, 0:3]), bits(s.blocks[:, :, 0:3]))
        else:
            assert not np.array_equal(bits(x_all[:, :, 0:3]), bits(s.blocks[:, :, 0:3]))
        assert len(row["starts"]) == len(BATCHES)
        for k, (lo, hi) in enumerate(BATCHES):
            slot_mask = None if mask is None else dev(mask[s.index[lo:hi]])
            got = block_pieces(model_net, dev(x_all[lo:hi]), dev(s.blocks[lo:hi]), dev(row["starts"][k]),
                               None if labels is None else dev(labels[lo:hi].astype(np.int32)), target, neighbour, tsign, slot_mask,
                               colour=both and row["s"] == 0)
            assert np.abs(got["dx0"][:, :, 0:3]).max() > 0
            assert np.array_equal(bits(got["dx0"]), bits(row["dx0"][lo:hi])), (row["s"], k)
            assert np.array_equal(bits(got["sgrad_xyz"]), bits(row["sgrad_xyz"][lo:hi])), (row["s"], k)
            assert np.array_equal(got["pred"], row["pred"][lo:hi]), (row["s"], k)
            if "sgrad" in got:                                     # (later steps warm-start the colour Smooth term's lists)
                assert np.array_equal(bits(got["sgrad"]), bits(row["sgrad"][lo:hi])), (row["s"], k)


def check_teacher_forced(s, rows, mask, cc=CC, clr=CLR):
    """every step from its recorded inputs: the ordered sums bit for bit, delta / mx / vx within the bound"""
    n = s.n_scene
    on = ref.moves(s.off, mask)
    assert (bits(rows[0]["delta_before"]) == 0).all()
    m_before, v_before = np.zeros((n, 3), F), np.zeros((n, 3), F)
    worst = dict(delta=0.0, mx=0.0, vx=0.0)
    for t, row in enumerate(rows):
        assert row["s"] == t
        if t:
            assert np.array_equal(bits(row["delta_before"]), bits(rows[t - 1]["delta_after"]))
        if row["gsum_x"] is None:                                  # the last step: no optimiser step follows it
            assert t == len(rows) - 1 and np.array_equal(bits(row["delta_after"]), bits(row["delta_before"]))
            assert np.array_equal(bits(row["mx_after"]), bits(m_before)) and np.array_equal(bits(row["vx_after"]), bits(v_before))
            continue
        dx0, sg = row["dx0"].reshape(-1, 9), row["sgrad_xyz"].reshape(-1, 3)
        d64, m64, v64, de, me, ve, gx, gs = ref.step64(row["delta_before"], m_before, v_before, dx0, sg, s.off, s.ent, mask, cc, clr, t + 1)
        assert np.array_equal(bits(row["gsum_x"]), bits(gx)) and np.array_equal(bits(row["gsum_sx"]), bits(gs)), t
        for name, got, want, e, before in (("delta", row["delta_after"], d64, de, row["delta_before"]), ("mx", row["mx_after"], m64, me, m_before),
                                           ("vx", row["vx_after"], v64, ve, v_before)):
            worst[name] = max(worst[name], ref.ratio(got[on], want[on], e[:, on]))
            assert ref.within(got[on], want[on], e[:, on]).all(), (t, name)
            assert np.array_equal(bits(got[~on]), bits(before[~on]))
        m_before, v_before = row["mx_after"], row["vx_after"]
    print("teacher-forced coordinate steps: largest error / first-order bound %s" % worst)


# ------------------------------------------------------------------------------------ the colour path is untouched
def test_field_color_returns_the_bytes_of_a_call_without_the_argument(net, overlap):
    from pointsecguard_amd.attacks.scene import SceneNUAttack
    plain = run_nu(net, overlap, 7, record=True)
    named = run_nu(net, overlap, 7, record=True, field="color")
    assert np.array_equal(bits(plain[0]), bits(named[0])) and np.array_equal(bits(plain[1]), bits(named[1]))
    assert not np.array_equal(bits(plain[0]), bits(overlap.c0))
    assert named[3].last_delta is None and named[3].last_mx is None and named[3].last_vx is None
    seen = []
    SceneNUAttack(net, steps=1, batch_size=4, exit_below=NEVER, trace=seen.append, field="color")(
        overlap.data, overlap.index, overlap.label, overlap.rgb, overlap.labels)
    assert sorted(seen[0]) == sorted(KEYS + ("s", "active", "starts"))     # exactly the colour attack's keys
    atk = SceneNUAttack(net, steps=1, batch_size=4, field="coord", exit_below=NEVER)
    atk(overlap.data, overlap.index, overlap.label, overlap.rgb, overlap.labels)
    assert atk.last_delta is not None and atk.last_w is None
    atk.field = "color"                                  # a colour run leaves no displacement behind
    atk(overlap.data, overlap.index, overlap.label, overlap.rgb, overlap.labels)
    assert atk.last_delta is None and atk.last_w is not None


# ------------------------------------------------------------------------------------ where nothing overlaps
@pytest.mark.parametrize("seed", [5, 6])
def test_equals_the_block_wise_coordinate_entry_points_where_nothing_overlaps(net, flat, seed):
    """2 blocks in one batch, every scene point in exactly one slot: a one-entry list adds 0 + x, so delta / mx / vx after every
    step and the returned blocks are, bit for bit, psg_nu_coord_apply_rooms, plan, forward_lean, psg_nu_f_loss_grad_rooms,
    psg_pn2_backward_full, psg_smooth_knn_xyz_rooms, psg_nu_coord_adam_step_rooms under the same seed."""
    from pointsecguard_amd import _lib, runtime
    from pointsecguard_amd.models.pointnet2_sem_seg import draw_fps_starts
    s, steps, n = flat, 3, 1024
    run = run_field(net, s, seed, steps=steps, batch_size=2, record=True)
    rows = run["rows"]
    assert run["atk"].last_exit_step == -1 and len(rows) == steps
    model = net._packed()
    x0 = dev(s.blocks)
    ori_xyz = x0[:, :, 0:3].contiguous()
    labels = dev(s.label.astype(np.int32))
    f32 = lambda *shape: torch.zeros(*shape, dtype=torch.float32, device="cuda")       # noqa: E731
    delta, m, v, sgrad, f_sum = f32(2, n, 3), f32(2, n, 3), f32(2, n, 3), f32(2, n, 3), f32(2)
    dlogp, pred = f32(2, n, 13), torch.zeros(2, n, dtype=torch.int32, device="cuda")
    ws = runtime.PN2Workspace(2, n, 1)
    st, P = runtime.stream, runtime.ptr
    flat_idx = s.index.reshape(-1)
    torch.manual_seed(seed)
    for t in range(steps):
        _lib.call("psg_nu_coord_apply_rooms", P(delta), P(ori_xyz), None, 2, n, None, P(x0), st())
        ws.plan_build(x0, draw_fps_starts(2, n, 1).cuda(), 1)
        logp = ws.forward(model, 0, x0, lean=True)
        _lib.call("psg_nu_f_loss_grad_rooms", P(logp), P(labels), 0, 2, n, 13, 0.0, 1.0, P(dlogp), P(f_sum), P(pred), st())
        dx0 = ws.backward(model, 0, dlogp, full=True)
        _lib.call("psg_smooth_knn_xyz_rooms", P(x0), 9, n * 9, P(ori_xyz), 3, n * 3, 2, n, 10, None, P(sgrad), None, None, st())
        if t < steps - 1:
            _lib.call("psg_nu_coord_adam_step_rooms", P(delta), P(m), P(v), None, P(dx0), P(sgrad), CC, CLR, 0.9, 0.999, 1e-8, t + 1,
                      2, n, None, None, st())
        row = rows[t]
        assert np.array_equal(bits(row["dx0"]), bits(dx0.cpu().numpy())), t
        assert np.array_equal(bits(row["sgrad_xyz"]), bits(sgrad.cpu().numpy())) and np.array_equal(row["pred"], pred.cpu().numpy()), t
        for name, mine in (("delta_after", delta), ("mx_after", m), ("vx_after", v)):
            same = float((bits(row[name][flat_idx]) == bits(mine.cpu().numpy().reshape(-1, 3))).mean())
            print("step %d %s: bit-equal share %.6f" % (t, name, same))
            assert same == 1.0, (t, name)
    pieces = x0.cpu().numpy()
    assert not np.array_equal(bits(pieces[:, :, 0:3]), bits(s.blocks[:, :, 0:3]))
    same = float((bits(run["blocks"]) == bits(pieces)).mean())
    print("scene NU coordinate attack vs block-wise pieces: bit-equal share %.6f" % same)
    assert same == 1.0
    assert (bits(rows[1]["delta_after"]) != bits(rows[0]["delta_before"])).mean() > 0.9


# ------------------------------------------------------------------------------------ on the overlapping scene
def test_slots_agree_with_the_scene(overlap, coord_run):
    check_slots_agree_with_the_scene(overlap, coord_run, colours_clean=True)
    atk, rows = coord_run["atk"], coord_run["rows"]
    assert (coord_run["delta"] != 0).any() and atk.last_w is None
    assert atk.last_exit_step == -1 and atk.last_history.shape == (3, 2) and (atk.last_history[:, 1] == 18 * 1024).all()
    assert np.array_equal(bits(coord_run["delta"]), bits(rows[-1]["delta_after"]))
    for row in rows:                                               # the colour state does not exist; the colours are the clean ones
        assert all(row[k] is None for k in ("w_before", "w_after", "m_after", "v_after", "sgrad", "gsum_f", "gsum_s"))
        assert np.array_equal(bits(row["c"]), bits(overlap.c0))
        assert tuple(atk.last_history[row["s"]]) == scene_nu_ref.latch_counts(row["pred"], overlap.label, 0, overlap.index, None)


def test_gradients_of_every_step_are_the_block_gradients(net, overlap, coord_run):
    assert [hi - lo for lo, hi in BATCHES] == [4, 4, 4, 4, 2]
    check_blocks_of_every_step(net, overlap, coord_run["rows"], overlap.label, 0, 10, 1.0)


def test_every_step_is_the_restated_step(overlap, coord_run):
    rows = coord_run["rows"]
    assert [r["s"] for r in rows] == [0, 1, 2] and all(r["active"] == 1 for r in rows)
    check_teacher_forced(overlap, rows, None)


def test_seeded_runs_return_the_same_bytes(net, overlap, coord_run):
    again = run_field(net, overlap, 7)                             # and tracing changes nothing
    for k in ("rgb", "blocks", "delta"):
        assert np.array_equal(bits(again[k]), bits(coord_run[k])), k
    other = run_field(net, overlap, 8)
    assert not np.array_equal(bits(other["delta"]), bits(coord_run["delta"]))


# ------------------------------------------------------------------------------------ the exit latch
def test_exit_leaves_the_displacement_of_the_firing_steps_forward(net, overlap):
    s = overlap
    never = run_field(net, s, 13, steps=4, record=True)
    rows, hist = never["rows"], never["atk"].last_history
    assert hist.shape == (4, 2) and never["atk"].last_exit_step == -1 and (hist[:, 1] == 18 * 1024).all()
    hits, n = hist[:, 0].tolist(), int(hist[0, 1])
    later = [t for t in range(1, 4) if hits[t] < min(hits[:t])]
    print("recorded n_hits %s of %d" % (hits, n))
    assert later, "the recorded history never falls below its first count: no exit at a step >= 1 can be placed"
    at = later[0]
    num, den = hits[at] + 1, n                                     # fires where n_hits <= hits[at]: first at step `at`
    want = scene_nu_ref.first_exit(hist, num, den, False)
    print("exit_below = (%d, %d), exit expected at step %d" % (num, den, want))
    assert want == at >= 1
    runs = {ce: run_field(net, s, 13, steps=4, exit_below=(num, den), check_every=ce) for ce in (1, 10)}
    for ce, run in runs.items():
        assert run["atk"].last_exit_step == want, ce
        assert np.array_equal(run["atk"].last_history, hist[:want + 1]), ce
        assert np.array_equal(bits(run["delta"]), bits(rows[want]["delta_before"])), ce
        assert (run["delta"] != 0).any()
        check_slots_agree_with_the_scene(s, run, colours_clean=True)
    assert np.array_equal(bits(runs[1]["blocks"]), bits(runs[10]["blocks"])) and np.array_equal(bits(runs[1]["delta"]), bits(runs[10]["delta"]))
    # traced, the loop stops at the exit step and hands over the same bytes
    traced = run_field(net, s, 13, steps=4, exit_below=(num, den), record=True)
    assert traced["atk"].last_exit_step == want and [r["active"] for r in traced["rows"]] == [1] * want + [0]
    assert np.array_equal(bits(traced["delta"]), bits(rows[want]["delta_before"])) and traced["rows"][-1]["gsum_x"] is None
    assert np.array_equal(bits(traced["rows"][-1]["delta_after"]), bits(traced["rows"][-1]["delta_before"]))


# ------------------------------------------------------------------------------------ targeted
def test_targeted_moves_points_of_the_origin_class_only(net, overlap):
    s = overlap
    origin = int(np.bincount(s.labels.astype(np.int64)).argmax())
    target = (origin + 1) % 13
    run = run_field(net, s, 9, record=True, target=target, origin=origin, exit_above=(1, 1))
    mask = s.labels == origin
    assert 0 < mask.sum() < s.n_scene and run["atk"].neighbour == 5 and run["atk"].last_exit_step == -1
    assert (bits(run["delta"][~mask]) == 0).all() and (run["delta"][mask] != 0).any()
    check_slots_agree_with_the_scene(s, run, colours_clean=True)
    check_blocks_of_every_step(net, s, run["rows"][:1], None, target, 5, -1.0, mask=mask)
    check_teacher_forced(s, run["rows"], mask)
    for row in run["rows"]:
        assert tuple(run["atk"].last_history[row["s"]]) == scene_nu_ref.latch_counts(row["pred"], None, target, s.index, mask)


# ------------------------------------------------------------------------------------ both fields
def test_both_moves_coordinates_and_colours_only(net, overlap, both_run):
    s, run = overlap, both_run
    check_slots_agree_with_the_scene(s, run, colours_clean=False)
    assert (run["delta"] != 0).any() and not np.array_equal(bits(run["rgb"]), bits(s.c0))
    assert run["rgb"].min() >= 0.0 and run["rgb"].max() <= 1.0 and run["atk"].last_w.is_cuda
    rows = run["rows"]
    assert np.array_equal(bits(run["rgb"]), bits(rows[-1]["c"]))
    check_blocks_of_every_step(net, s, rows[:2], s.label, 0, 10, 1.0, both=True)
    check_teacher_forced(s, rows, None)
    # the colour half: section 5w's step on channels 3:6 of the same gradients - the restatement's sums bit for bit, w / m / v
    # within the bound of its float64 reference
    on = scene_nu_ref.moves(s.off, None)
    m_before, v_before = np.zeros((s.n_scene, 3), F), np.zeros((s.n_scene, 3), F)
    for t, row in enumerate(rows[:-1]):
        dx0, sgrad = row["dx0"].reshape(-1, 9), row["sgrad"].reshape(-1, 3)
        w32, m32, v32, gf, gs = scene_nu_ref.step32(row["w_before"], m_before, v_before, row["c"], s.c0, dx0, sgrad, s.off, s.ent, None,
                                                    1e-4, 0.01, t + 1)
        assert np.array_equal(bits(row["gsum_f"]), bits(gf)) and np.array_equal(bits(row["gsum_s"]), bits(gs)), t
        w64, m64, v64, we, me, ve, _, _ = scene_nu_ref.step64(row["w_before"], m_before, v_before, row["c"], s.c0, dx0, sgrad, s.off,
                                                              s.ent, None, 1e-4, 0.01, t + 1)
        for name, got, r32, want, e in (("w", row["w_after"], w32, w64, we), ("m", row["m_after"], m32, m64, me), ("v", row["v_after"], v32, v64, ve)):
            assert scene_nu_ref.within(got[on], want[on], e[:, on]).all(), (t, name)
            assert scene_nu_ref.within(r32[on], want[on], e[:, on]).all(), (t, name)
        m_before, v_before = row["m_after"], row["v_after"]
    # (no bit-equality with the "coord" run is claimed, not even at step 0: the colours of the first forward have been
    # through tanh space once and differ from the clean ones in the last place)


# ------------------------------------------------------------------------------------ the premise
def test_the_block_attack_displaces_a_point_per_block(net, overlap, coord_run):
    """The premise: NU_attack(field="coord").forward_rooms over the same blocks in groups of 4 puts one physical point in
    several places.  Its exit is kept from firing by attacking the network's own clean predictions."""
    from pointsecguard_amd.attacks import torchattacks
    s = overlap
    torch.manual_seed(7)
    out = np.empty_like(s.blocks)
    for lo, hi in BATCHES:
        images = dev(np.ascontiguousarray(s.blocks[lo:hi].transpose(0, 2, 1)))
        labels = net(images)[0].argmax(dim=2).cpu().numpy()
        adv, steps_run = torchattacks.NU_attack(net, steps=3, field="coord").forward_rooms(images, labels)
        assert (np.asarray(steps_run) == 3).all()
        out[lo:hi] = adv.cpu().numpy().transpose(0, 2, 1)
    assert np.array_equal(bits(out[:, :, 3:]), bits(s.blocks[:, :, 3:]))
    share_blocks, share_scene = copies_displaced_differently(s, out), copies_displaced_differently(s, coord_run["blocks"])
    print("multi-slot points whose copies sit more than 1e-4 m apart: per-block NU attack %.4f, scene NU attack %.4f"
          % (share_blocks, share_scene))
    assert share_blocks > 0.5 and share_scene == 0.0


# ------------------------------------------------------------------------------------ float64
def test_traced_gradient_of_a_moved_batch_vs_float64(net, overlap, coord_run, weights_sd):
    """Channels 0:3 of one batch at step 1 - the geometry has moved - against tests/pn2_ref64.py plus the float64 f-loss on the
    plan's own tables: the three clauses of check_grad (sign agreement >= 99.9 %, every flip below 1e-3 of the largest
    magnitude, median relative error < 1e-4).  The largest error is printed, not bounded: no reference figure exists at this
    shape.  psg_pn2_backward (the feature path alone) in its place does not meet the clauses."""
    s, row = overlap, coord_run["rows"][1]
    assert (row["delta_before"] != 0).any()
    x_t = moved_blocks(s, row["delta_before"])
    # the batch: the last one that holds a block padded with copies of its own points, so that level-0 FPS names a point more
    # than once and the gradient comes down through a table that is not injective (section 5v)
    distinct = np.array([np.unique(blk[:, 0:3], axis=0).shape[0] for blk in x_t])
    k = max(i for i, (lo, hi) in enumerate(BATCHES) if (distinct[lo:hi] < 1024).any())
    lo, hi = BATCHES[k]
    args = (net, dev(x_t[lo:hi]), dev(s.blocks[lo:hi]), dev(row["starts"][k]), dev(s.label[lo:hi].astype(np.int32)), 0, 10, 1.0)
    alone = block_pieces(*args)
    x = torch.from_numpy(x_t[lo:hi].transpose(0, 2, 1).astype(np.float64)).clone().requires_grad_(True)
    f_loss64(pn2_ref64.forward(weights_sd, x, pn2_ref64.tables_from(alone["tables"])), s.label[lo:hi], None).backward()
    yard = x.grad.numpy()[:, :3]
    figures = {}
    for what, got in (("backward_full (traced)", row["dx0"][lo:hi].transpose(0, 2, 1)[:, :3]),
                      ("psg_pn2_backward", block_pieces(*args, full=False)["dx0"].transpose(0, 2, 1)[:, :3])):
        agree, flip = coord_bars(got, yard)
        nz = yard != 0
        median = float(np.median(np.abs(got - yard)[nz] / np.abs(yard[nz])))
        err = float(np.abs(got - yard).max() / np.abs(yard).max())
        print("%s 0:3 vs float64 at step 1 (batch %d): sign agreement %.6f (bar %.3f), largest flipped %.3e (bar %.0e), median "
              "relative error %.3e (bar %.0e), max abs / max mag %.3e (not bounded)" % (what, k, agree, SIGN_BAR, flip, FLIP_BAR, median,
                                                                                         MEDIAN_BAR, err))
        figures[what] = (agree, flip, median)
    agree, flip, median = figures["backward_full (traced)"]
    assert agree >= SIGN_BAR
    assert flip <= FLIP_BAR
    assert median < MEDIAN_BAR
    agree, flip, median = figures["psg_pn2_backward"]
    assert not (agree >= SIGN_BAR and flip <= FLIP_BAR and median < MEDIAN_BAR)


# ------------------------------------------------------------------------------------ MSG, the evaluation loop
def test_msg_network_is_refused(msg_net):
    from pointsecguard_amd.attacks.scene import SceneNUAttack
    for field in ("coord", "both"):
        with pytest.raises(NotImplementedError, match="psg_pn2_backward_full refuses MSG"):
            SceneNUAttack(msg_net, steps=1, field=field)


def test_consistent_whole_scene_loop_with_the_coordinate_field(net):
    from pointsecguard_amd import harness
    from pointsecguard_amd.attacks.scene import SceneNUAttack
    ds = two_scene_dataset()
    made, handed = [], []

    def make(m):
        made.append(SceneNUAttack(m, steps=3, exit_below=NEVER, field="coord"))
        return made[-1]

    np.random.seed(3)
    torch.manual_seed(3)
    res = harness.evaluate_whole_scene_consistent(
        net, ds, make, batch_size=4, log=lambda *_: None,
        on_scene_field=lambda name, rgb, xyz: handed.append((name, rgb, xyz, made[-1].last_delta.cpu().numpy())))
    assert [h[0] for h in handed] == ["Area_5_a", "Area_5_b"]
    for si, (_, rgb, xyz, delta) in enumerate(handed):
        pts = ds.scene_points_list[si]
        assert rgb.dtype == np.float32 and np.array_equal(bits(rgb), bits((pts[:, 3:6] / 255.0).astype(F)))
        assert xyz.dtype == np.float64 and xyz.shape == (pts.shape[0], 3) and (delta != 0).any()
        assert np.array_equal(xyz, pts[:, 0:3].astype(np.float64) + delta.astype(np.float64))
    np.random.seed(3)
    torch.manual_seed(3)
    clean = harness.evaluate_whole_scene(net, ds, None, batch_size=4, log=lambda *_: None, streams=1)
    assert np.array_equal(clean["counters"][0], res["counters"][0])
    assert res["counters"][1][0].sum() == 8000
