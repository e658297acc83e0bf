"""GPU tests of the whole-scene NB attack on the coordinate field (attacks/scene.py: SceneNBAttack(field="coord" | "both"),
harness.evaluate_whole_scene_consistent(on_scene_field=...)): one displacement per scene point.

Scenes, slicing (block_points = 1024 under np.random.seed(3)) and the network are those of tests/test_gpu_scene_attack.py:
`flat` (2 blocks, nothing overlaps) and `overlap` (18 x 1024, 90 % of the points in more than one slot); iters = 3 and
batch_size = 4 unless a test says otherwise.  The coordinate field runs with its own (coord_eps, coord_alpha) = (0.06,
0.025): three steps reach 0.075, so the clamp of the last projected step works."""
import numpy as np
import pytest
import torch

import pn2_ref64
import scene_field_ref
import scene_ref
from test_gpu_pn2_fullgrad import FLIP_BAR, MEDIAN_BAR, SIGN_BAR, coord_bars, plan_tables
from test_gpu_scene_attack import ALPHA, EPS, Sliced, bits, dev, run_scene_attack, two_scene_dataset
from test_gpu_harness import synth_scene

pytestmark = pytest.mark.gpu
F = np.float32
CEPS, CALPHA = 0.06, 0.025
BATCHES = [(lo, min(lo + 4, 18)) for lo in range(0, 18, 4)]


@pytest.fixture(scope="module")
def net(weights_sd):
    from pointsecguard_amd.models.pointnet2_sem_seg import get_model
    m = get_model(13).cuda().eval()
    m.load_state_dict({k: torch.from_numpy(v) for k, v in weights_sd.items()})
    return m


@pytest.fixture(scope="module")
def flat():
    return Sliced(synth_scene(21, 2048, 0.9, 0.9))


@pytest.fixture(scope="module")
def overlap():
    s = Sliced(synth_scene(11, 5000, 1.6, 1.2))
    assert s.blocks.shape == (18, 1024, 9)
    return s


def run_field_attack(model, s, seed, field="coord", iters=3, batch_size=4, record=False, coord_eps=CEPS, coord_alpha=CALPHA, **kw):
    """-> dict(rgb, blocks, delta, steps): the attack's two results, last_delta and (record) every iteration's trace as numpy"""
    from pointsecguard_amd.attacks.scene import SceneNBAttack
    steps = []

    def trace_field(d):
        assert sorted(d) == ["c_after", "c_before", "delta_after", "delta_before", "dlogp", "dx0", "starts", "t"]
        steps.append({k: ([x.cpu().numpy() for x in v] if k == "starts" else (v.cpu().numpy() if torch.is_tensor(v) else v))
                      for k, v in d.items()})

    atk = SceneNBAttack(model, EPS, ALPHA, iters, batch_size=batch_size, field=field, coord_eps=coord_eps, coord_alpha=coord_alpha,
                        trace_field=trace_field if record else None, **kw)
    torch.manual_seed(seed)
    adv_rgb, adv_blocks = atk(s.data, s.index, s.label, s.rgb, s.labels)
    torch.cuda.synchronize()
    assert atk.last_delta.is_cuda and tuple(atk.last_delta.shape) == (s.n_scene, 3) and atk.last_delta.dtype == torch.float32
    return dict(rgb=adv_rgb.cpu().numpy(), blocks=adv_blocks.cpu().numpy(), delta=atk.last_delta.cpu().numpy(), steps=steps)


@pytest.fixture(scope="module")
def coord_run(net, overlap):
    return run_field_attack(net, overlap, 7, record=True)


@pytest.fixture(scope="module")
def both_run(net, overlap):
    return run_field_attack(net, overlap, 7, field="both", record=True)


def moved_blocks(s, delta):
    """the slots of the clean blocks with delta added: the restatement of psg_scene_delta_to_blocks"""
    clean = s.blocks.reshape(-1, 9)
    return scene_field_ref.delta_to_blocks(delta, s.index, clean, clean).reshape(s.blocks.shape)


def check_slots_agree_with_the_scene(s, run, colours_clean):
    flat_adv, clean = run["blocks"].reshape(-1, 9), s.blocks.reshape(-1, 9)
    want = (clean[:, 0:3] + run["delta"][s.index.reshape(-1)]).astype(F)
    assert np.array_equal(bits(flat_adv[:, 0:3]), bits(want))
    assert np.array_equal(bits(flat_adv[:, 6:9]), bits(clean[:, 6:9]))
    if colours_clean:
        assert np.array_equal(bits(flat_adv[:, 3:6]), bits(clean[:, 3:6])) and np.array_equal(bits(run["rgb"]), bits(s.c0))
    else:
        assert np.array_equal(bits(flat_adv[:, 3:6]), bits(run["rgb"][s.index.reshape(-1)]))


# ------------------------------------------------------------------------------------ 1: the colour path is untouched
def test_field_color_returns_the_bytes_of_a_call_without_the_argument(net, overlap):
    from pointsecguard_amd.attacks.scene import SceneNBAttack
    plain = run_scene_attack(net, overlap, 7)
    named = run_scene_attack(net, overlap, 7, field="color")
    assert np.array_equal(bits(plain[0]), bits(named[0])) and np.array_equal(bits(plain[1]), bits(named[1]))
    assert not np.array_equal(bits(plain[0]), bits(overlap.c0))
    atk = SceneNBAttack(net, EPS, ALPHA, 1, batch_size=4, field="coord")
    atk(overlap.data, overlap.index, overlap.label, overlap.rgb, overlap.labels)
    assert atk.last_delta is not None
    atk.field = "color"                                  # a colour run leaves no displacement behind
    atk(overlap.data, overlap.index, overlap.label, overlap.rgb, overlap.labels)
    assert atk.last_delta is None


# ------------------------------------------------------------------------------------ 2, 3: slots and bounds
def test_slots_agree_with_the_scene(overlap, coord_run):
    check_slots_agree_with_the_scene(overlap, coord_run, colours_clean=True)
    assert (coord_run["delta"] != 0).any()


def test_bounds(net, overlap, coord_run):
    assert np.abs(coord_run["delta"]).max() <= F(CEPS)                        # project_last = True: exactly
    assert np.abs(coord_run["delta"]).max() == F(CEPS)                        # (and the clamp was reached: 3 x 0.025 > 0.06)
    free = run_field_attack(net, overlap, 7, project_last=False)
    top = np.abs(free["delta"]).max()
    print("project_last=False: largest |delta| %.9g (coord_eps %.9g, coord_alpha %.9g)" % (top, F(CEPS), F(CALPHA)))
    assert top <= F(F(CEPS) + F(CALPHA))                                      # the float32 sum: fl is monotone
    assert top > F(CEPS)
    check_slots_agree_with_the_scene(overlap, free, colours_clean=True)
    # coord_eps / coord_alpha fall back to eps / alpha
    fallback = run_field_attack(net, overlap, 7, iters=1, coord_eps=None, coord_alpha=None)
    assert set(np.unique(np.abs(fallback["delta"])).tolist()) <= {0.0, float(F(ALPHA))}


# ------------------------------------------------------------------------------------ 4: teacher-forced steps
def test_every_step_is_the_ordered_sum_step(overlap, coord_run):
    s, steps = overlap, coord_run["steps"]
    assert [st["t"] for st in steps] == [0, 1, 2]
    assert (bits(steps[0]["delta_before"]) == 0).all()
    for k, st in enumerate(steps):
        want, _ = scene_field_ref.field_step(st["delta_before"], st["dx0"].reshape(-1, 9), s.off, s.ent, None, CALPHA, CEPS, 1.0, False)
        assert np.array_equal(bits(st["delta_after"]), bits(want)), st["t"]
        assert st["c_before"] is None and st["c_after"] is None
        if k:
            assert np.array_equal(bits(st["delta_before"]), bits(steps[k - 1]["delta_after"]))
    assert np.array_equal(bits(coord_run["delta"]), bits(steps[-1]["delta_after"]))


# ------------------------------------------------------------------------------------ 5: traced gradients
def standalone_gradients(net, s, x_blocks, starts, lo, hi, full=True):
    """plan_build -> forward_lean -> psg_ce_logp_grad -> backward_full (full=False: psg_pn2_backward) of one batch on its own
    workspace; returns (dx0, dlogp, the plan's tables)"""
    from pointsecguard_amd import _lib, runtime
    model, b = net._packed(), hi - lo
    ws = runtime.PN2Workspace(b, 1024, 1)
    x0 = dev(x_blocks[lo:hi])
    ws.plan_build(x0, dev(starts), 1)
    logp = ws.forward(model, 0, x0, lean=True)
    dlogp = torch.empty_like(logp)
    _lib.call("psg_ce_logp_grad", runtime.ptr(logp), runtime.ptr(dev(s.label[lo:hi].astype(np.int32))), 0, b * 1024, b * 1024, 13,
              1.0 / 1024, runtime.ptr(dlogp), None, runtime.stream())
    dx0 = ws.backward(model, 0, dlogp, full=True) if full else ws.backward(model, 0, dlogp)
    torch.cuda.synchronize()
    return dx0.cpu().numpy(), dlogp.cpu().numpy(), plan_tables(ws, b)


def test_traced_gradients_are_the_block_gradients(net, overlap, coord_run):
    s = overlap
    assert [hi - lo for lo, hi in BATCHES] == [4, 4, 4, 4, 2]
    for st in coord_run["steps"]:
        assert len(st["starts"]) == 5
        x_t = moved_blocks(s, st["delta_before"])
        if st["t"] == 0:
            assert np.array_equal(bits(x_t), bits(s.blocks))
        for k, (lo, hi) in enumerate(BATCHES):
            dx0, dlogp, _ = standalone_gradients(net, s, x_t, st["starts"][k], lo, hi)
            assert np.abs(dx0[:, :, 0:3]).max() > 0
            assert np.array_equal(bits(dx0), bits(st["dx0"][lo:hi])), (st["t"], k)
            assert np.array_equal(bits(dlogp), bits(st["dlogp"][lo:hi])), (st["t"], k)


def test_traced_gradient_of_a_moved_batch_vs_float64(net, overlap, coord_run, weights_sd):
    """Channels 0:3 of one batch at iteration 1 - the geometry has moved - against tests/pn2_ref64.py on the
    plan's own tables: the three clauses of check_grad (sign agreement >= 99.9 %, every flip below 1e-3 of the largest
    magnitude, median relative error < 1e-4).  The largest error is printed, not bounded: no reference figure exists at this
    shape.  psg_pn2_backward (the feature path alone) in its place does not meet the clauses."""
    s, st = overlap, coord_run["steps"][1]
    assert (st["delta_before"] != 0).any()
    x_t = moved_blocks(s, st["delta_before"])
    # the batch: the last one that holds a block padded with copies of its own points (sampling with replacement).  Such a
    # block has fewer distinct positions than level 0 samples (S = N = 1024), so FPS names one point more than once and the
    # gradient of the coarse level comes down through a table that is NOT injective: the sum over the repeats is checked here
    distinct = np.array([np.unique(blk[:, 0:3], axis=0).shape[0] for blk in x_t])
    k = max(i for i, (lo, hi) in enumerate(BATCHES) if (distinct[lo:hi] < 1024).any())
    lo, hi = BATCHES[k]
    _, _, tables = standalone_gradients(net, s, x_t, st["starts"][k], lo, hi)
    repeats = [1024 - np.unique(row).size for row in tables["fps0"]]
    print("batch %d (blocks %d:%d): distinct positions %s, repeated level-0 FPS picks %s" % (k, lo, hi, distinct[lo:hi].tolist(), repeats))
    assert max(repeats) > 0
    yard, _ = pn2_ref64.input_grad(weights_sd, x_t[lo:hi].transpose(0, 2, 1), pn2_ref64.tables_from(tables), labels=s.label[lo:hi])
    ref = yard[:, :3]
    ours = st["dx0"][lo:hi].transpose(0, 2, 1)[:, :3]
    figures = {}
    for what, got in (("backward_full (traced)", ours),
                      ("psg_pn2_backward", standalone_gradients(net, s, x_t, st["starts"][k], lo, hi, full=False)[0]
                       .transpose(0, 2, 1)[:, :3])):
        agree, flip = coord_bars(got, ref)
        nz = ref != 0
        median = float(np.median(np.abs(got - ref)[nz] / np.abs(ref[nz])))
        err = float(np.abs(got - ref).max() / np.abs(ref).max())
        print("%s 0:3 vs float64 at t = 1: sign agreement %.6f (bar %.3f), largest flipped %.3e (bar %.0e), median relative error "
              "%.3e (bar %.0e), max abs / max mag %.3e (not bounded)" % (what, agree, SIGN_BAR, flip, FLIP_BAR, median, MEDIAN_BAR, err))
        figures[what] = (agree, flip, median)
    agree, flip, median = figures["backward_full (traced)"]
    assert agree >= SIGN_BAR
    assert flip <= FLIP_BAR
    assert median < MEDIAN_BAR
    agree, flip, median = figures["psg_pn2_backward"]
    assert not (agree >= SIGN_BAR and flip <= FLIP_BAR and median < MEDIAN_BAR)


# ------------------------------------------------------------------------------------ 6: where nothing overlaps
@pytest.mark.parametrize("seed", [5, 6])
def test_one_step_is_the_block_attacks_step_where_nothing_overlaps(net, flat, seed):
    """iters = 1, both blocks in one batch: the same gradient, so the same signs.  Bit-equality is not claimed - the per-block
    step rounds x + step - ori -: the blocks agree to one ulp of the coordinate."""
    from pointsecguard_amd.attacks import torchattacks
    s = flat
    run = run_field_attack(net, s, seed, iters=1, batch_size=2, project_last=False)
    torch.manual_seed(seed)
    images = dev(np.ascontiguousarray(s.blocks.transpose(0, 2, 1)))
    adv = torchattacks.NB_attack(net, eps=EPS, alpha=ALPHA, iters=1, field="coord", coord_eps=CEPS, coord_alpha=CALPHA)(images, s.label)
    adv = adv.cpu().numpy().transpose(0, 2, 1).reshape(-1, 9)
    ori = s.blocks.reshape(-1, 9)
    idx = s.index.reshape(-1)
    sign_block = np.sign(adv[:, 0:3].astype(np.float64) - ori[:, 0:3].astype(np.float64))
    assert (sign_block != 0).any()
    assert np.array_equal(np.sign(run["delta"])[idx], sign_block)
    ours = run["blocks"].reshape(-1, 9)
    ulp = np.spacing(np.maximum(np.abs(ours[:, 0:3]), np.abs(adv[:, 0:3])).astype(F))
    gap = np.abs(ours[:, 0:3].astype(np.float64) - adv[:, 0:3].astype(np.float64))
    print("flat scene, one step: largest gap to the per-block attack %.3e, in ulps of the coordinate %.3f"
          % (gap.max(), (gap / ulp).max()))
    assert (gap <= ulp).all()
    assert np.array_equal(bits(ours[:, 3:]), bits(adv[:, 3:]))


# ------------------------------------------------------------------------------------ 7: seeded runs
def test_seeded_runs_return_the_same_bytes(net, overlap, coord_run):
    again = run_field_attack(net, overlap, 7)                                 # and tracing changes nothing
    for k in ("rgb", "blocks", "delta"):
        assert np.array_equal(bits(again[k]), bits(coord_run[k])), k
    other = run_field_attack(net, overlap, 8)
    assert not np.array_equal(bits(other["delta"]), bits(coord_run["delta"]))


# ------------------------------------------------------------------------------------ 8: targeted
@pytest.mark.parametrize("field", ["coord", "both"])
def test_targeted_moves_masked_points_only(net, overlap, field):
    s = overlap
    origin = int(np.bincount(s.labels.astype(np.int64)).argmax())
    target = (origin + 1) % 13
    run = run_field_attack(net, s, 9, field=field, record=True, target=target, origin=origin)
    mask = s.labels == origin
    assert 0 < mask.sum() < s.n_scene
    assert (bits(run["delta"][~mask]) == 0).all()
    assert (run["delta"][mask] != 0).any()
    assert np.abs(run["delta"]).max() <= F(CEPS)
    check_slots_agree_with_the_scene(s, run, colours_clean=field == "coord")
    if field == "both":
        assert np.array_equal(bits(run["rgb"][~mask]), bits(s.c0[~mask])) and (bits(run["rgb"][mask]) != bits(s.c0[mask])).any()
    slot_masked = mask[s.index.reshape(-1)]
    for st in run["steps"]:
        want, _ = scene_field_ref.field_step(st["delta_before"], st["dx0"].reshape(-1, 9), s.off, s.ent, mask, CALPHA, CEPS, -1.0, False)
        assert np.array_equal(bits(st["delta_after"]), bits(want)), st["t"]
        rows = st["dlogp"].reshape(-1, 13)
        assert (bits(rows[~slot_masked]) == 0).all() and (rows[slot_masked] != 0).any()


# ------------------------------------------------------------------------------------ 9: both fields
def test_both_moves_coordinates_and_colours_only(overlap, both_run, coord_run):
    s, run = overlap, both_run
    check_slots_agree_with_the_scene(s, run, colours_clean=False)
    assert (run["delta"] != 0).any() and not np.array_equal(bits(run["rgb"]), bits(s.c0))
    assert np.abs(run["delta"]).max() <= F(CEPS)
    assert np.abs(run["rgb"].astype(np.float64) - s.c0.astype(np.float64)).max() <= float(F(EPS)) + 2.0 ** -23
    assert run["rgb"].min() >= 0.0 and run["rgb"].max() <= 1.0
    steps = run["steps"]
    assert np.array_equal(bits(steps[0]["c_before"]), bits(s.c0)) and (bits(steps[0]["delta_before"]) == 0).all()
    for k, st in enumerate(steps):
        want_d, _ = scene_field_ref.field_step(st["delta_before"], st["dx0"].reshape(-1, 9), s.off, s.ent, None, CALPHA, CEPS, 1.0, False)
        want_c, _ = scene_ref.scene_step(st["c_before"], s.c0, st["dx0"].reshape(-1, 9), s.off, s.ent, None, ALPHA, EPS, 1.0, False)
        assert np.array_equal(bits(st["delta_after"]), bits(want_d)), st["t"]
        assert np.array_equal(bits(st["c_after"]), bits(want_c)), st["t"]
        if k:
            assert np.array_equal(bits(st["c_before"]), bits(steps[k - 1]["c_after"]))
    assert np.array_equal(bits(run["rgb"]), bits(steps[-1]["c_after"])) and np.array_equal(bits(run["delta"]), bits(steps[-1]["delta_after"]))
    # the first iteration sees the clean scene under either field: the same coordinate step
    assert np.array_equal(bits(steps[0]["delta_after"]), bits(coord_run["steps"][0]["delta_after"]))


# ------------------------------------------------------------------------------------ 10: the premise
def copies_displaced_differently(s, adv_blocks):
    """share of the multi-slot scene points whose copies do not all carry the same displacement: adv - clean per slot in
    float64, compared with the point's first slot; 1e-4 m is far above the rounding of a coordinate of a few metres (half
    an ulp: 2.4e-7) and far below a step"""
    d = adv_blocks.reshape(-1, 9)[:, 0:3].astype(np.float64) - s.blocks.reshape(-1, 9)[:, 0:3].astype(np.float64)
    idx = s.index.reshape(-1)
    first = d[s.ent[s.off[:-1].clip(max=s.ent.size - 1)]]
    differs = np.zeros(s.n_scene, bool)
    np.logical_or.at(differs, idx, (np.abs(d - first[idx]) > 1e-4).any(axis=1))
    multi = (s.off[1:] - s.off[:-1]) > 1
    return float(differs[multi].mean())


def test_the_block_attack_displaces_a_point_per_block(net, overlap, coord_run):
    """The premise: the per-block NB_attack(field="coord") under evaluate_whole_scene puts one physical point in several places."""
    from pointsecguard_amd import harness
    from pointsecguard_amd.attacks import torchattacks
    s = overlap
    seen = []

    class Recording:
        def __init__(self, m):
            self.atk = torchattacks.NB_attack(m, eps=EPS, alpha=ALPHA, iters=3, field="coord", coord_eps=CEPS, coord_alpha=CALPHA)

        def __call__(self, images, labels):
            adv = self.atk(images, labels)
            seen.append(adv.detach().cpu().numpy().transpose(0, 2, 1))
            return adv

    ds = harness.ScannetDatasetWholeScene(None, block_points=1024, scenes={"Area_5_a.npy": synth_scene(11, 5000, 1.6, 1.2)})
    np.random.seed(3)
    torch.manual_seed(7)
    harness.evaluate_whole_scene(net, ds, Recording, batch_size=4, log=lambda *_: None, streams=1)
    out = np.concatenate(seen)
    assert out.shape == s.blocks.shape and np.array_equal(bits(out[:, :, 3:]), bits(s.blocks[:, :, 3:]))      # the same slicing
    share_blocks, share_scene = copies_displaced_differently(s, out), copies_displaced_differently(s, coord_run["blocks"])
    print("multi-slot points whose copies are displaced differently: per-block attack %.4f, scene attack %.4f"
          % (share_blocks, share_scene))
    assert share_blocks > 0.0 and share_scene == 0.0


# ------------------------------------------------------------------------------------ 11: the evaluation loop
def test_consistent_whole_scene_loop_with_the_coordinate_field(tmp_path, net):
    from pointsecguard_amd import harness
    from pointsecguard_amd.attacks.scene import SceneNBAttack
    ds = two_scene_dataset()
    made, handed, handed_rgb = [], [], []

    def make(m):
        made.append(SceneNBAttack(m, EPS, ALPHA, 3, field="coord", coord_eps=CEPS, coord_alpha=CALPHA))
        return made[-1]

    def on_scene_field(name, rgb, xyz):
        handed.append((name, rgb, xyz, made[-1].last_delta.cpu().numpy()))

    np.random.seed(3)
    torch.manual_seed(3)
    path = tmp_path / "log.txt"
    res = harness.evaluate_whole_scene_consistent(net, ds, make, batch_size=4, log_path=str(path), log=lambda *_: None,
                                                  on_scene=lambda name, rgb: handed_rgb.append((name, rgb)),
                                                  on_scene_field=on_scene_field)
    state_after = torch.get_rng_state()
    rows = path.read_text().splitlines()
    assert rows[0] == "index\tL2_dis\tadv_acc\tacc\tadv_miou\tmiou"
    np.random.seed(3)
    n_batches = [-(-ds[i][0].shape[0] // 4) for i in range(2)]
    assert len(rows) == 1 + sum(n_batches)
    for r in rows[1:]:
        f = r.split("\t")
        assert len(f) == 7 and float(f[1]) > 0.0 and 0.0 <= float(f[2]) <= 1.0 and 0.0 <= float(f[3]) <= 1.0
    c = res["counters"]
    assert c[0][0].sum() == 8000 and c[1][0].sum() == 8000
    assert [h[0] for h in handed] == ["Area_5_a", "Area_5_b"] == [h[0] for h in handed_rgb]
    for si, (_, rgb, xyz, delta) in enumerate(handed):
        pts = ds.scene_points_list[si]
        c0 = (pts[:, 3:6] / 255.0).astype(F)
        assert rgb.dtype == np.float32 and np.array_equal(bits(rgb), bits(c0)) and np.array_equal(bits(handed_rgb[si][1]), bits(c0))
        assert xyz.dtype == np.float64 and xyz.shape == (pts.shape[0], 3)
        assert (delta != 0).any() and np.abs(delta).max() <= F(CEPS)
        assert np.array_equal(xyz, pts[:, 0:3].astype(np.float64) + delta.astype(np.float64))
    # the clean side is the clean evaluation's, and the generator stands where the clean forwards left it
    np.random.seed(3)
    torch.manual_seed(3)
    clean = harness.evaluate_whole_scene(net, ds, None, batch_size=4, log=lambda *_: None, streams=1)
    assert np.array_equal(clean["counters"][0], c[0])
    assert torch.equal(torch.get_rng_state(), state_after)
    # a scene that is not attacked hands over the clean arrays
    a, b = synth_scene(31, 5000, 1.6, 1.2), synth_scene(12, 3000, 1.0, 1.4)
    origin = int(np.bincount(a[:, 6].astype(np.int64)).argmax())
    target = (origin + 1) % 13
    b[b[:, 6] == origin, 6] = target
    ds2 = harness.ScannetDatasetWholeScene(None, block_points=1024, scenes={"Area_5_a.npy": a, "Area_5_b.npy": b})
    np.random.seed(5)
    torch.manual_seed(5)
    got = []
    harness.evaluate_whole_scene_consistent(
        net, ds2, lambda m: SceneNBAttack(m, EPS, ALPHA, 2, target=target, origin=origin, field="coord"), batch_size=4,
        log=lambda *_: None, targeted=dict(origin=origin, target=target), on_scene_field=lambda *args: got.append(args))
    assert [g[0] for g in got] == ["Area_5_a", "Area_5_b"]
    assert not np.array_equal(got[0][2], a[:, 0:3]) and np.array_equal(got[1][2], b[:, 0:3].astype(np.float64))
    assert np.array_equal(bits(got[1][1]), bits((b[:, 3:6] / 255.0).astype(F)))
