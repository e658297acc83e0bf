"""The packed SA backward of PointNet++ SSG (psg_pn2_kernels.cuh: sa_bwd_packed_kernel) and the ReLU masks keyed by packed
workgroup that go with it: where a level's backward runs packed (level 0 is what is built), its transposed layers run over the
valid rows of the forward's packed workgroups only, and the forward stores its mask words where that backward looks for them.
Every valid row goes through the k-loops it had unpacked, so all gradients must agree BYTE for byte with the unpacked backward
(PSG_PN2_PACK_BWD=0: today's kernels and mask layout) and with PSG_PN2_PACK=0 (nothing packed).  The switches are read once per
process: each value runs in a fresh child interpreter (this file run as a script), with PSG_TRACE_SYNC=1.

Per room kind of tests/sa_pack_bwd_rooms.py - the five of tests/sa_pack_rooms.py, a lattice (every level-0 group one row, 16
groups per workgroup) and clusters (workgroups of P - 1 rows, aligned and unaligned workgroups of full groups, groups across a
32-row block) - with B = 2, N = 4096 (the network's level sizes are fixed: its smallest shape) and a plan of two forwards with
different FPS starts, a child computes the colour-only gradient, the 9-channel psg_pn2_backward, psg_pn2_backward_full and a
3-iteration psg_pn2_nb_attack; for the golden room the gradient the fixtures pin.

Checked: the four children (default, default again, PSG_PN2_PACK_BWD=0, PSG_PN2_PACK=0) are byte-equal on every array; launch
sites ending in #bwd#packed appear in the default children only; the golden room's gradient stays inside the bars of
tests/test_gpu_parity.py on every path.  (No level with a packed backward kernel is kept unpacked by default, so the default IS
the all-levels setting.)"""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
B, N, ITERS = 2, 4096, 3
N_SRC = (4096, 1024, 256, 64)
CHILDREN = (("on", {}), ("on2", {}), ("bwd_off", {"PSG_PN2_PACK_BWD": "0"}), ("off", {"PSG_PN2_PACK": "0"}))


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
    import sa_pack_bwd_rooms as sbr
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

    out = {}
    model = runtime.PN2Model(runtime.fold_state_dict(dict(np.load(os.path.join(GOLDEN, "pn2_weights.npz")))))
    ws = runtime.PN2Workspace(B, N, ITERS)
    for ki, kind in enumerate(sbr.ROOM_KINDS):
        rooms = sbr.rooms_of(kind, B, 1000 + ki)
        labels = dev(rule_labels(rooms).astype(np.int32))
        x0 = dev(rooms)
        rng = np.random.default_rng(50 + ki)
        starts = np.stack([rng.integers(0, n, (ITERS, B)) for n in N_SRC], axis=1).astype(np.int32)   # [ITERS][4][B]
        if kind == "clusters":
            starts[0, 0, 0] = sbr.CLUSTERS_START0          # the room and start whose segmentation the host test states
        ws.plan_build(x0, dev(starts[:2]), 2)
        ws.forward(model, 1, x0)
        logp = ws.forward(model, 0, x0)                    # (slot 0 last: the backward passes below use it)
        dlogp = ce_grad(logp, labels)
        out[kind + "_logp"] = logp.cpu().numpy()
        out[kind + "_dcolour"] = ws.backward(model, 0, dlogp, colour_only=True).cpu().numpy()
        out[kind + "_dx0"] = ws.backward(model, 0, dlogp).cpu().numpy()
        out[kind + "_dx0_full"] = ws.backward(model, 0, dlogp, full=True).cpu().numpy()
        images = dev(rooms.transpose(0, 2, 1))
        out[kind + "_adv"] = ws.nb_attack(model, images, labels, dev(starts), 0.05, 2 / 255, ITERS).cpu().numpy()
    g = dict(np.load(os.path.join(GOLDEN, "pn2_room.npz")))
    x0 = dev(np.repeat(g["room"][None], B, axis=0))
    ws.plan_build(x0, dev(np.repeat(g["starts"].reshape(1, 4, 1), B, axis=2), torch.int32), 1)
    logp = ws.forward(model, 0, x0)
    dlogp = ce_grad(logp, dev(np.repeat(g["labels"].astype(np.int32)[None], B, axis=0)))
    out["golden_dx0"] = ws.backward(model, 0, dlogp).cpu().numpy()
    torch.cuda.synchronize()
    np.savez(out_path, **out)


def _child(tmp_path, tag, switches):
    env = {k: v for k, v in os.environ.items() if k not in ("PSG_PN2_PACK", "PSG_PN2_PACK_BWD")}
    env.update(switches)
    env["PSG_TRACE_SYNC"] = "1"
    out = str(tmp_path / ("%s.npz" % tag))
    r = subprocess.run([sys.executable, os.path.abspath(__file__), out], env=env, cwd=ROOT, capture_output=True, text=True,
                       timeout=600)
    assert r.returncode == 0, (r.stdout + r.stderr)[-3000:]
    sites = set(re.findall(r"\[psg trace\] launch \d+ at (\S+) issued", r.stderr + r.stdout))
    return dict(np.load(out)), sites


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("sa_pack_bwd")
    return {tag: _child(tmp, tag, switches) for tag, switches in CHILDREN}


@pytest.mark.gpu
def test_all_paths_byte_equal(runs):
    import sa_pack_bwd_rooms as sbr
    on = runs["on"][0]
    assert len(on) == 5 * len(sbr.ROOM_KINDS) + 1
    for tag, _ in CHILDREN[1:]:
        other = runs[tag][0]
        assert sorted(other) == sorted(on)
        for k in sorted(on):
            assert on[k].tobytes() == other[k].tobytes(), "%s: default and %s differ" % (k, tag)
    for kind in sbr.ROOM_KINDS:
        assert np.abs(on[kind + "_dcolour"]).max() > 0 and np.abs(on[kind + "_dx0_full"][..., 0:3]).max() > 0, kind


@pytest.mark.gpu
def test_packed_backward_sites_in_the_default_children_only(runs):
    for tag, _ in CHILDREN:
        sites = runs[tag][1]
        bwd = sorted(s for s in sites if s.endswith("#bwd#packed"))
        if tag in ("on", "on2"):
            assert any("#colour" in s for s in bwd) and any("#colour" not in s for s in bwd), sorted(sites)
        else:
            assert not bwd, bwd
        assert any(s.endswith("#packed") for s in sites) == (tag != "off"), sorted(sites)


@pytest.mark.gpu
@pytest.mark.parametrize("path", [tag for tag, _ in CHILDREN])
def test_golden_room_gradient_vs_reference(runs, golden_room, path):
    r = runs[path][0]
    for b in range(B):
        check_grad(r["golden_dx0"][b, :, 3:6], golden_room["dcolor"])


if __name__ == "__main__":
    _child_main(sys.argv[1])
