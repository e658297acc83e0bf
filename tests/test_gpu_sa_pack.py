"""The packed SA forward of PointNet++ SSG (psg_pn2_kernels.cuh: sa_pack_plan_kernel, sa_fwd_packed_kernel): the three layers
and the max-pool run on the VALID rows of a ball-query group only - the rows behind them are copies of member 0, never win the
pool and get no gradient.  PSG_PN2_PACK=0 keeps the unpacked kernels.  Every valid row goes through the k-loops it had unpacked,
so the two paths must agree BYTE for byte, not to a tolerance.  The switch is read once per process: each value runs in a fresh
child interpreter (this file run as a script).

Per room kind of tests/sa_pack_rooms.py - uniform, structured, with duplicated points, shrunk to 0.25 (every level-0 ball full:
nothing to skip), one dense clump plus isolated points (groups of 1 next to groups of 32) - with B = 3, N = 4096 and a plan of
two forwards with different FPS starts, a child computes: the log-probs of both forwards, the pooled outputs and arg-max bytes
of all four levels, the colour-only gradient, the 9-channel psg_pn2_backward, psg_pn2_backward_full, and a 3-iteration
psg_pn2_nb_attack; for the golden room (B = 3) the log-probs, module outputs and gradient the fixtures pin.

Checked: packed == unpacked byte for byte; two packed children byte-identical; both paths inside the bars of
tests/test_gpu_parity.py against the reference-generated fixtures; the plan's count and segmentation tables equal their numpy
restatement on the group tables read back from the same plan; the switch selected other launches."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
LOGP_TOL = 1e-4     # tests/test_gpu_parity.py
B, N, ITERS = 3, 4096, 3
N_SRC = (4096, 1024, 256, 64)


def check_grad(ours, ref):      # tests/test_gpu_parity.py, clause for clause
    nz = ref != 0
    assert np.array_equal(ours != 0, nz), "zero pattern of the colour gradient differs"
    agree = np.sign(ours[nz]) == np.sign(ref[nz])
    assert agree.mean() >= 0.999
    if not agree.all():
        assert np.abs(ref[nz][~agree]).max() <= 1e-3 * np.abs(ref).max()
    rel = np.abs(ours - ref)[nz] / np.abs(ref[nz])
    assert np.median(rel) < 1e-4


def _child_main(out_path):
    import torch
    sys.path.insert(0, ROOT)
    import sa_pack_rooms as spr
    from pointsecguard_amd import _lib, runtime
    from pointsecguard_amd.synthetic import rule_labels

    def dev(a, dt=None):
        t = torch.from_numpy(np.ascontiguousarray(a))
        return (t.to(dt) if dt is not None else t).cuda().contiguous()

    def ce_grad(logp, labels):
        dlogp = torch.empty_like(logp)
        _lib.call("psg_ce_logp_grad", runtime.ptr(logp), runtime.ptr(labels), 0, B * N, B * N, 13, 1.0 / N,
                  runtime.ptr(dlogp), None, runtime.stream())
        return dlogp

    packed = os.environ.get("PSG_PN2_PACK", "1") != "0"
    out = {}
    model = runtime.PN2Model(runtime.fold_state_dict(dict(np.load(os.path.join(GOLDEN, "pn2_weights.npz")))))
    ws = runtime.PN2Workspace(B, N, ITERS)
    for ki, kind in enumerate(spr.ROOM_KINDS):
        rooms = spr.rooms_of(kind, B, 1000 + ki)
        labels = dev(rule_labels(rooms).astype(np.int32))
        x0 = dev(rooms)
        rng = np.random.default_rng(50 + ki)
        starts = np.stack([rng.integers(0, n, (ITERS, B)) for n in N_SRC], axis=1).astype(np.int32)   # [ITERS][4][B]
        ws.plan_build(x0, dev(starts[:2]), 2)
        for lvl in range(4):
            for f in range(2):
                for b in range(B):
                    key = "%s_f%d_b%d_l%d" % (kind, f, b, lvl)
                    out["gidx_" + key] = ws.plan_tensor(1, lvl, f, b).cpu().numpy()
                    if packed:
                        out["cnt_" + key] = ws.plan_tensor(6, lvl, f, b).cpu().numpy()
                        out["seg_" + key] = ws.plan_tensor(7, lvl, f, b).cpu().numpy()
                        out["dsc_" + key] = ws.plan_tensor(9, lvl, f, b).cpu().numpy()
        for f in (1, 0):                                           # (slot 0 last: the backward passes below use it)
            logp = ws.forward(model, f, x0)
            out["%s_logp%d" % (kind, f)] = logp.cpu().numpy()
            for lvl in range(4):
                out["%s_pool%d_l%d" % (kind, f, lvl)] = ws.activation(lvl).cpu().numpy()
                out["%s_arg%d_l%d" % (kind, f, lvl)] = np.stack([ws.plan_tensor(8, lvl, 0, b).cpu().numpy() for b in range(B)])
        dlogp = ce_grad(logp, labels)
        out[kind + "_dcolour"] = ws.backward(model, 0, dlogp, colour_only=True).cpu().numpy()
        out[kind + "_dx0"] = ws.backward(model, 0, dlogp).cpu().numpy()
        out[kind + "_dx0_full"] = ws.backward(model, 0, dlogp, full=True).cpu().numpy()
        images = dev(rooms.transpose(0, 2, 1))
        out[kind + "_adv"] = ws.nb_attack(model, images, labels, dev(starts), 0.05, 2 / 255, ITERS).cpu().numpy()
    # the golden room three times (an odd workgroup count), against the reference-generated fixture
    g = dict(np.load(os.path.join(GOLDEN, "pn2_room.npz")))
    x0 = dev(np.repeat(g["room"][None], B, axis=0))
    ws.plan_build(x0, dev(np.repeat(g["starts"].reshape(1, 4, 1), B, axis=2), torch.int32), 1)
    logp = ws.forward(model, 0, x0)
    out["golden_logp"] = logp.cpu().numpy()
    for w in range(7):
        out["golden_act%d" % w] = ws.activation(w).cpu().numpy()
    dlogp = ce_grad(logp, dev(np.repeat(g["labels"].astype(np.int32)[None], B, axis=0)))
    out["golden_dx0"] = ws.backward(model, 0, dlogp).cpu().numpy()
    torch.cuda.synchronize()
    np.savez(out_path, **out)


def _child(tmp_path, tag, value):
    env = dict(os.environ)
    env["PSG_PN2_PACK"] = value
    env["PSG_TRACE_SYNC"] = "1"
    out = str(tmp_path / ("%s.npz" % tag))
    r = subprocess.run([sys.executable, os.path.abspath(__file__), out], env=env, cwd=ROOT, capture_output=True, text=True,
                       timeout=600)
    assert r.returncode == 0, (r.stdout + r.stderr)[-3000:]
    sites = set(re.findall(r"\[psg trace\] launch \d+ at (\S+) issued", r.stderr + r.stdout))
    return dict(np.load(out)), sites


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("sa_pack")
    return {"off": _child(tmp, "off", "0"), "on": _child(tmp, "on", "1"), "on2": _child(tmp, "on2", "1")}


def _results(d):
    return sorted(k for k in d if not k.startswith(("cnt_", "seg_", "dsc_")))


@pytest.mark.gpu
def test_packed_is_byte_equal_to_unpacked_and_reproducible(runs):
    (off, off_sites), (on, on_sites), (on2, _) = runs["off"], runs["on"], runs["on2"]
    assert _results(on) == _results(off) and sorted(on) == sorted(on2)
    for k in _results(on):
        assert on[k].tobytes() == on2[k].tobytes(), "%s: two runs of the packed path differ" % k
        assert on[k].tobytes() == off[k].tobytes(), "%s: packed and unpacked paths differ" % k
    assert any("#packed" in s for s in on_sites), sorted(on_sites)
    assert not any("#packed" in s for s in off_sites), sorted(off_sites)


@pytest.mark.gpu
def test_plan_tables_equal_their_numpy_restatement(runs):
    import sa_pack_rooms as spr
    on = runs["on"][0]
    keys = [k[4:] for k in on if k.startswith("cnt_")]
    assert len(keys) == len(spr.ROOM_KINDS) * 2 * B * 4
    skipped = total = 0
    for key in keys:
        lvl = int(key[-1])
        gidx = on["gidx_" + key]
        cnt = spr.valid_counts(gidx, N_SRC[lvl])
        assert np.array_equal(on["cnt_" + key], cnt), key
        seg = spr.segmentation(cnt, spr.SA_P[lvl])
        n = int(seg[0])
        assert np.array_equal(on["seg_" + key][:n + 2], seg[:n + 2]), key      # (entries behind the last one are not written)
        assert np.array_equal(on["dsc_" + key], spr.descriptors(cnt, seg, spr.SA_P[lvl])), key
        if key.startswith("shrunk") and lvl == 0:
            assert n == 1024 // 4, "a room of full balls keeps the unpacked segmentation"
        skipped += gidx.size - int(cnt.sum())
        total += gidx.size
    assert skipped > total // 2, "these rooms pad most of their rows"


@pytest.mark.gpu
@pytest.mark.parametrize("path", ["on", "off"])
def test_golden_room_vs_reference(runs, golden_room, path):
    r, g = runs[path][0], golden_room
    for b in range(B):
        for which, name in enumerate(("sa1", "sa2", "sa3", "sa4", "fp4", "fp3", "fp2")):
            assert np.abs(r["golden_act%d" % which][b] - g["act_" + name]).max() <= LOGP_TOL, (b, name)
        assert np.abs(r["golden_logp"][b] - g["logp"]).max() <= LOGP_TOL, b
        check_grad(r["golden_dx0"][b, :, 3:6], g["dcolor"])


if __name__ == "__main__":
    _child_main(sys.argv[1])
