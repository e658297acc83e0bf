"""RandLA-Net on the GPU: the position-branch gradient (psg_rla_backward_full on a psg_rla_ws_create_full workspace), stage by
stage against tests/rla_coord_ref64.py on the GPU's own inputs and decisions, and the coordinate-field BIM attacks built on it.

Shapes: those of tests/test_randla_stages.py (8192; 8704 = 17 x 512, ragged last tiles at every level; 2 x 8192 with 256
duplicated points).  One forward and one backward_full per shape, every tap copied back; then
  * every new buffer (G2, G1, g_rp, side_i, side_j, gxyz per level, and dxyz) inside its stage bound on EVERY entry: 31 stages;
    the sign words of fxyz1 / fxyz2 as the other sign words are checked;
  * the existing forward and backward walks of randla_ref64 on the full workspace (level 0 on the unfused chain);
  * dfeatures byte-equal to psg_rla_backward's after a second identical forward; two runs bit-equal; backward_full(2 g) =
    2 backward_full(g) exactly (every stage is linear in g and a factor 2 is exact);
  * end to end, dxyz + dfeatures[:, 0:3] against the float64 stages composed on the GPU's own forward state and decisions:
    sign agreement >= SIGN_BAR = 99.9 %, every disagreeing entry below FLIP_BAR = 1e-3 of the largest magnitude (DESIGN.md
    section 5k); dfeatures[:, 0:3] alone - what the library returned before - fails both.
The same stage checks under PSG_RLA_NO_SPLIT=1 (the level-0 chain at every level) in a fresh child process, 8704 points.
Largest error / bound per stage, as printed on the MI355X, stands in DESIGN.md section 5q.

Attacks (8192 points, at most 4 iterations): see the tests' docstrings."""
import os
import subprocess
import sys

import numpy as np
import pytest

from pointsecguard_amd.synthetic import randla_params
import randla_ref64 as R
import rla_coord_ref64 as C
from test_randla_stages import BWD_LEVEL, BWD_NET, FWD_DEC, FWD_LEVEL, FWD_NET, SHAPES, knn_tree, make_cloud, mask_list, snapshot

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIGN_BAR, FLIP_BAR = 0.999, 1e-3
PSG_ERR_ARG = -1                     # include/psg.h
XYZ_LEVEL = ["G2", "G1", "g_rp", "side_i", "side_j", "gxyz"]


def dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def full_run(name):
    import torch
    from pointsecguard_amd.randla import network
    n, batch = SHAPES[name]
    xyz, rgb, labels = make_cloud(n, batch, 12)
    params = randla_params(3)
    P = R.fold_all(params)
    model, ws = network.RandLAModel(params), network.RandLAWorkspace(n, batch=batch, full=True)
    ws.set_cloud(dev(xyz))
    geo = R.geometry(xyz, [ws.index(0, l).cpu().numpy() for l in range(5)], [ws.index(1, l).cpu().numpy() for l in range(5)], batch)
    feats = np.concatenate([xyz, rgb], 1)
    f_dev = dev(feats)
    logits = ws.forward(model, f_dev)
    xyz_masks = [(k, i, d // 2) for i, d in enumerate(R.D_OUT) for k in ("m_fxyz1", "m_fxyz2")]
    fwd = snapshot(ws, FWD_NET, FWD_DEC, FWD_LEVEL, mask_list() + xyz_masks)
    _, dl = network.colper_grad(logits, dev(labels.astype(np.int32)))
    dfeat, dxyz = ws.backward(model, dl, full=True)
    bwd = snapshot(ws, BWD_NET, ["d_dec_out"], BWD_LEVEL + XYZ_LEVEL, [])
    bwd[("dfeatures", 0)], bwd[("dxyz", 0)] = dfeat.cpu().numpy(), dxyz.cpu().numpy()
    # a second identical forward, then the feature-path backward; a second full run; a run on 2 g
    ws.forward(model, f_dev)
    dfeat_plain = ws.backward(model, dl).cpu().numpy()
    ws.forward(model, f_dev)
    again = [t.cpu().numpy() for t in ws.backward(model, dl, full=True)]
    ws.forward(model, f_dev)
    twice = [t.cpu().numpy() for t in ws.backward(model, 2 * dl, full=True)]
    torch.cuda.synchronize()
    dl = dl.cpu().numpy()
    _, rep_f = R.walk_forward(P, feats, geo, taps=fwd)
    C.check_fxyz_masks(P, fwd, rep_f)
    _, rep_b = R.walk_backward(P, fwd, dl, geo, taps=bwd)
    _, rep_x = C.walk_xyz(P, fwd, bwd, geo, taps=bwd)
    for k in sorted(rep_x.ratio, key=str):
        print("%s %-16s error / bound %.3f" % (name, k, rep_x.ratio[k]))
    print("%s softmax transposes of the existing walk: largest error / first-order bound %.3f" % (name, rep_b.softmax_ratio()))
    # the float64 stages, free-running from the GPU's forward state and decisions
    bwd64, _ = R.walk_backward(P, fwd, dl, geo)
    x64, _ = C.walk_xyz(P, fwd, bwd64, geo)
    ref = x64[("dxyz", 0)] + bwd64[("dfeatures", 0)][:, :3]
    return dict(name=name, n=n, batch=batch, ws=ws, model=model, fwd=fwd, bwd=bwd, rep_f=rep_f, rep_b=rep_b, rep_x=rep_x, ref=ref,
                dfeat_plain=dfeat_plain, again=again, twice=twice)


@pytest.fixture(scope="module")
def runs():
    cache = {}

    def get(name):
        if name not in cache:
            cache[name] = full_run(name)
        return cache[name]
    return get


@pytest.mark.parametrize("shape", list(SHAPES))
def test_gpu_position_branch_stages(runs, shape):
    """every new buffer at every level inside its stage bound on every entry"""
    rep = runs(shape)["rep_x"]
    assert not rep.fail, "\n".join(rep.fail)
    assert len(rep.stages) == 31


@pytest.mark.parametrize("shape", list(SHAPES))
def test_gpu_existing_walks_on_the_full_workspace(runs, shape):
    """psg_rla_forward / psg_rla_backward_full's feature path on a full workspace: the stages of tests/test_randla_stages.py,
    plus the sign words of fxyz1 / fxyz2"""
    run = runs(shape)
    assert not run["rep_f"].fail, "\n".join(run["rep_f"].fail)
    assert not run["rep_b"].fail, "\n".join(run["rep_b"].fail)
    assert len(run["rep_f"].stages) == 80 and len(run["rep_f"].flips) == 39 and len(run["rep_b"].stages) == 45


@pytest.mark.parametrize("shape", list(SHAPES))
def test_gpu_dfeatures_bytes_and_reproducibility(runs, shape):
    run = runs(shape)
    dfeat, dxyz = run["bwd"][("dfeatures", 0)], run["bwd"][("dxyz", 0)]
    same = lambda a, b: np.array_equal(a.view(np.uint32), b.view(np.uint32))          # noqa: E731
    assert same(dfeat, run["dfeat_plain"])                       # psg_rla_backward on the same workspace, byte for byte
    assert same(dfeat, run["again"][0]) and same(dxyz, run["again"][1])
    assert np.abs(dxyz).max() > 0 and np.isfinite(dxyz).all()
    assert same(np.float32(2) * dfeat, run["twice"][0]) and same(np.float32(2) * dxyz, run["twice"][1])


@pytest.mark.parametrize("shape", list(SHAPES))
def test_gpu_end_to_end_bars(runs, shape):
    run = runs(shape)
    ref = run["ref"]
    feat_only = run["bwd"][("dfeatures", 0)][:, :3].astype(np.float64)
    full = feat_only + run["bwd"][("dxyz", 0)].astype(np.float64)
    agree, flip = C.sign_bars(full, ref)
    a0, f0 = C.sign_bars(feat_only, ref)
    print("%s dxyz + dfeatures[:, 0:3] vs float64 on the GPU's decisions: sign agreement %.6f (bar %.3f), largest flipped %.3e (bar %.0e), "
          "max err / max mag %.3e; dfeatures[:, 0:3] alone: %.4f, %.3e" % (shape, agree, SIGN_BAR, flip, FLIP_BAR,
                                                                          np.abs(full - ref).max() / np.abs(ref).max(), a0, f0))
    assert agree >= SIGN_BAR
    assert flip <= FLIP_BAR
    assert a0 < SIGN_BAR and f0 > FLIP_BAR


def test_gpu_duplicates_occurred(runs):
    """the batch's second cloud: 8192 self edges per cloud and 512 edges between distinct coincident points at level 0, where
    the distance column adds exactly zero (checked entry by entry in the side_i / side_j stages; here: that the case occurred
    and left finite values)"""
    run = runs("b2x8192")
    rp = run["fwd"][("relpos", 0)]
    assert int((rp[:, 0] == 0).sum()) == 2 * 8192 + 512
    zero = rp[:, 0] == 0
    g, si = run["bwd"][("g_rp", 0)], run["bwd"][("side_i", 0)]
    assert np.array_equal(si[zero, :3], g[zero, 1:4] + g[zero, 4:7]) and np.isfinite(run["bwd"][("gxyz", 0)]).all()


def test_gpu_refusals(runs):
    import torch
    from pointsecguard_amd import _lib, runtime
    from pointsecguard_amd.randla import network
    run = runs("n8192")
    lib, ws, model = _lib.load(), run["ws"], run["model"]
    n = run["n"]
    plain = network.RandLAWorkspace(n)
    plain.set_cloud(dev(make_cloud(n, 1, 12)[0]))
    logits = plain.forward(model, dev(np.zeros((n, 6), np.float32)))
    dl, df, dx = torch.zeros_like(logits), torch.zeros(n, 6, device="cuda"), torch.zeros(n, 3, device="cuda")
    args = lambda h, *p: (model.handle, h) + tuple(None if t is None else runtime.ptr(t) for t in p) + (runtime.stream(),)  # noqa: E731
    assert lib.psg_rla_backward_full(*args(plain.handle, dl, df, dx)) == PSG_ERR_ARG and b"psg_rla_ws_create_full" in lib.psg_last_error()
    for bad in ((None, df, dx), (dl, None, dx), (dl, df, None)):
        assert lib.psg_rla_backward_full(*args(ws.handle, *bad)) == PSG_ERR_ARG and b"null argument" in lib.psg_last_error()
    assert plain.backward(model, dl).shape == (n, 6)             # the refused calls consumed nothing
    for what, level in ((70, 0), (75, 4)):                       # the new taps exist on a full workspace only
        assert not lib.psg_rla_debug_ptr(plain.handle, what, level, None, None)
        assert b"psg_rla_ws_create_full" in lib.psg_last_error()
    for what, level in ((99, 0), (7, 0), (78, 0), (69, 0), (72, 5), (72, -1)):
        assert not lib.psg_rla_debug_ptr(ws.handle, what, level, None, None)
        assert b"psg_rla_debug_ptr" in lib.psg_last_error()
    assert tuple(ws.debug("g_rp", 4).shape) == (n // 256 * 16, 10)
    feat, nr, dt = torch.zeros(n, 6, device="cuda"), torch.zeros(2, device="cuda"), torch.zeros(n, 3, device="cuda")
    step = lambda *p: lib.psg_rla_bim_step_field(*[None if t is None else runtime.ptr(t) for t in p[:4]], n, 0.1, 0.01, p[4],  # noqa: E731
                                                 *[None if t is None else runtime.ptr(t) for t in p[5:]], runtime.stream())
    assert step(None, df, dx, dx, 0, nr, dt) != 0 and b"psg_rla_bim_step_field" in lib.psg_last_error()
    assert step(feat, df, dx, dx, 1, None, dt) != 0
    # PSG_RLA_ATOMICS=1 builds no inverse lists: a full workspace is refused (a fresh child: the switch is read at creation)
    code = ("import ctypes\nfrom pointsecguard_amd import _lib, runtime\nh = ctypes.c_void_p()\n"
            "rc = _lib.load().psg_rla_ws_create_full(runtime.context(None), 8192, 1, ctypes.byref(h))\n"
            "assert rc != 0 and b'PSG_RLA_ATOMICS' in _lib.load().psg_last_error(), rc\nprint('refused')\n")
    out = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, PSG_RLA_ATOMICS="1"), cwd=ROOT, capture_output=True,
                         text=True, timeout=300)
    assert out.returncode == 0 and "refused" in out.stdout, out.stdout[-2000:] + out.stderr[-2000:]


def test_gpu_stages_without_the_split_path():
    """PSG_RLA_NO_SPLIT=1: the level-0 chain (gather + per-edge score GEMM) at every level, whose transpose leaves the whole
    per-edge gradient of the concatenation in scratch; the same stage checks, 8704 points, in a fresh child process"""
    env = dict(os.environ, PSG_RLA_NO_SPLIT="1")
    for k in ("PSG_RLA_ATOMICS", "PSG_RLA_NO_DIRECT", "PSG_TRACE_SYNC"):
        env.pop(k, None)
    out = subprocess.run([sys.executable, "-m", "pytest", os.path.abspath(__file__), "-x", "-q", "-m", "gpu", "-k",
                          "(position_branch_stages or existing_walks or end_to_end_bars or dfeatures_bytes) and n8704", "-s", "-p",
                          "no:cacheprovider"], env=env, cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stdout[-4000:]
    assert "4 passed" in out.stdout and "skipped" not in out.stdout.splitlines()[-1]


# ------------------------------------------------------------------------------------------------ the attacks
N_ATK, EPS, ALPHA = 8192, 0.05, 0.02


@pytest.fixture(scope="module")
def atk_case():
    from pointsecguard_amd.randla import network
    xyz, rgb, labels = make_cloud(N_ATK, 1, 12)
    model = network.RandLAModel(randla_params(3))
    return dict(model=model, feats=np.concatenate([xyz, rgb], 1), labels=labels.astype(np.int32), ws=network.RandLAWorkspace(N_ATK, full=True))


def own_gradient(case, feats):
    """forward + hinge gradient + backward_full on a workspace of the test's own: -> (loss, dfeat, dxyz) as numpy"""
    from pointsecguard_amd.randla import network
    ws, f = case["ws"], dev(feats)
    ws.set_cloud(f[:, 0:3].contiguous())
    logits = ws.forward(case["model"], f)
    loss, dl = network.colper_grad(logits, dev(case["labels"]))
    dfeat, dxyz = ws.backward(case["model"], dl, full=True)
    return float(loss), dfeat.cpu().numpy(), dxyz.cpu().numpy()


def make(cls, case, metric, field, iteration, **cfg):
    atk = cls(case["model"], distance_metric=metric, field=field)
    atk.config(magnitude=EPS, alpha=ALPHA, iteration=iteration, **cfg)
    return atk


@pytest.mark.parametrize("metric", ["l_inf", "l_2"])
def test_gpu_one_coordinate_step_is_the_numpy_step(atk_case, metric):
    """iteration = 0 is the one update before the loop: on the clean cloud, the GPU's own gradient g = dfeat[:, 0:3] + dxyz
    (one float32 add) through the numpy field step - bit for bit for l_inf, inside the float64 error model for l_2; the
    colours are untouched"""
    from pointsecguard_amd.randla import attack
    feats = atk_case["feats"]
    _, dfeat, dxyz = own_gradient(atk_case, feats)
    atk = make(attack.NBattack, atk_case, metric, "coord", 0, coord_magnitude=0.03, coord_alpha=0.01)
    rgb = atk.batch_attack(feats, atk_case["labels"]).cpu().numpy()
    got = atk.last_adv_xyz.cpu().numpy()
    g = dfeat[:, :3] + dxyz
    assert np.array_equal(rgb, feats[:, 3:])
    if metric == "l_inf":
        assert np.array_equal(got, C.field_step(feats[:, :3], g, feats[:, :3], 0.03, 0.01, metric))
        assert (got != feats[:, :3]).mean() > 0.9
    else:
        ref, b = C.field_step_l2_bound(feats[:, :3], g, feats[:, :3], 0.03, 0.01)
        assert (np.abs(got - ref) <= b).all()
        assert abs(float(atk.last_dist_xyz) - 0.01) < 1e-5       # one normalised step of length coord_alpha < coord_magnitude


@pytest.mark.parametrize("metric", ["l_inf", "l_2"])
@pytest.mark.parametrize("field", ["coord", "both"])
def test_gpu_field_attack(atk_case, metric, field):
    """4 updates: the positions stay inside the eps ball at every iteration, the colours are untouched under "coord" and move
    (inside their own ball and box) under "both", the workspace is left on the moved positions (its level-0 neighbour table is
    their kNN), and the non-targeted loss rises"""
    from pointsecguard_amd.randla import attack
    feats, labels = atk_case["feats"], atk_case["labels"]
    atk = make(attack.NBattack, atk_case, metric, field, 3)
    seen = []
    atk.step_hook = lambda it, f: seen.append(f.clone())
    rgb = atk.batch_attack(feats, labels).cpu().numpy()
    assert len(seen) == 4
    e32 = np.float64(np.float32(EPS))
    for f in seen:
        d = f.cpu().numpy().astype(np.float64) - feats
        if metric == "l_inf":
            assert (np.abs(d[:, :3]) <= e32 + R.U * (np.abs(feats[:, :3]) + e32)).all()
            assert (np.abs(d[:, 3:]) <= e32 + 2 * R.U).all()
        else:
            assert np.sqrt((d[:, :3] ** 2).sum()) <= EPS * (1 + 1e-5) and np.sqrt((d[:, 3:] ** 2).sum()) <= EPS * (1 + 1e-5)
        assert (d[:, :3] != 0).any()
    adv_xyz = atk.last_adv_xyz.cpu().numpy()
    assert np.array_equal(adv_xyz, seen[-1].cpu().numpy()[:, :3])
    assert abs(float(atk.last_dist_xyz) - np.sqrt(((adv_xyz.astype(np.float64) - feats[:, :3]) ** 2).sum())) < 1e-4
    if field == "coord":
        assert np.array_equal(rgb, feats[:, 3:])
    else:
        assert (rgb != feats[:, 3:]).mean() > 0.5 and rgb.min() >= 0 and rgb.max() <= 1
    table = atk._ws[("field", N_ATK)].ws.index(0, 0).cpu().numpy()
    assert np.array_equal(table, knn_tree(adv_xyz[None], adv_xyz[None], 16)[0])
    assert not np.array_equal(table, knn_tree(feats[None, :, :3], feats[None, :, :3], 16)[0])
    loss0 = own_gradient(atk_case, feats)[0]
    loss1 = own_gradient(atk_case, np.concatenate([adv_xyz, rgb], 1))[0]
    print("%s %s: colper loss %.3f -> %.3f" % (metric, field, loss0, loss1))
    assert loss1 > loss0


def test_gpu_color_field_is_the_default_object(atk_case):
    from pointsecguard_amd.randla import attack
    feats, labels = atk_case["feats"], atk_case["labels"]
    outs = []
    for kw in ({}, {"field": "color"}):
        atk = attack.NBattack(atk_case["model"], **kw)
        atk.config(magnitude=EPS, alpha=ALPHA, iteration=2)
        outs.append(atk.batch_attack(feats, labels).cpu().numpy())
        assert atk.last_adv_xyz is None
    assert np.array_equal(outs[0].view(np.uint32), outs[1].view(np.uint32))
    lab = np.where(np.arange(N_ATK) < 2000, 2, labels).astype(np.int32)
    outs = []
    for kw in ({}, {"field": "color"}):
        atk = attack.tar_NBattack(atk_case["model"], **kw)
        atk.config(magnitude=EPS, alpha=ALPHA, iteration=1)
        outs.append((atk.batch_attack(feats, lab, target=5, ori=2), atk.last_adv.cpu().numpy()))
    assert outs[0][0] == outs[1][0] and np.array_equal(outs[0][1].view(np.uint32), outs[1][1].view(np.uint32))


def test_gpu_not_implemented_cases(atk_case):
    from pointsecguard_amd.randla import attack
    model = atk_case["model"]
    for make_it in (lambda: attack.NBattack(model, batch_size=2, field="coord"), lambda: attack.BIM(model, batch_size=2, field="both"),
                    lambda: attack.NUattack(model, field="coord"), lambda: attack.tar_NUattack(model, field="both")):
        with pytest.raises(NotImplementedError, match="batch_attack"):
            make_it()
    atk = make(attack.tar_NBattack, atk_case, "l_2", "coord", 1)
    with pytest.raises(NotImplementedError, match="batch_attack"):
        atk.batch_attack_clouds(atk_case["feats"][None], atk_case["labels"][None], target=5, ori=2)
    with pytest.raises(ValueError):
        attack.NBattack(model, field="xyz")


def test_gpu_targeted_coordinate_attack_tuple(atk_case):
    """tar_NBattack(field="coord"): the seven-field tuple; sr is the share of the MASKED points predicted as the target by the
    forward the last update stepped from - recomputed here on a workspace of the test's own from the positions before it"""
    from pointsecguard_amd.randla import attack
    feats = atk_case["feats"]
    lab = np.where(np.arange(N_ATK) < 2000, 2, atk_case["labels"]).astype(np.int32)
    atk = make(attack.tar_NBattack, atk_case, "l_2", "coord", 2)
    seen = []
    atk.step_hook = lambda it, f: seen.append(f.clone())
    out = atk.batch_attack(feats, lab, target=5, ori=2)
    assert len(out) == 7 and out[0] == float((lab == 2).sum()) and 1 <= len(seen) <= 3
    before = feats if len(seen) == 1 else seen[-2].cpu().numpy()
    ws, f = atk_case["ws"], dev(before)
    ws.set_cloud(f[:, 0:3].contiguous())
    pred = ws.forward(atk_case["model"], f).argmax(1).cpu().numpy()
    mask = lab == 2
    assert out[1] == float(np.sum(pred[mask] == 5) / mask.sum())
    assert np.array_equal(atk.last_adv.cpu().numpy(), feats[:, 3:]) and out[4] == 0.0
    assert float(atk.last_dist_xyz) > 0 and np.array_equal(atk.last_adv_xyz.cpu().numpy(), seen[-1].cpu().numpy()[:, :3])
