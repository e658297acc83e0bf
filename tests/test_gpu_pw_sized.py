"""The right-sized per-point launches of the split SA levels (psg_pn2.hip: run_pw_fwd / run_pw_bwd; psg_pn2_kernels.cuh:
pw_fwd_kernel, pw_bwd_kernel<32, 4>).  PSG_PN2_PW_SIZED=0 keeps the launches as they were: the forward product on the borrowed
fp_fwd_kernel<32, 8>, its gradient on eight waves whatever the layer's width.

Both paths run every output tile through the same k-loop over the whole K, so they must agree BYTE for byte, not to a
tolerance.  The switch is read once per process: each value runs in a fresh child interpreter (this file run as a script) that
computes, with the launch tracer on,

  * SSG, B = 1 and B = 3 (the golden room three times: an odd workgroup count, so the XCD tile order takes its fallback and the
    wave rotation every phase), N = 4096 - the split levels then have 1024 / 256 / 64 points per room, i.e. 32 / 8 / 2 point
    tiles, and level 3 runs two workgroups per tile: log-probs and the seven module outputs, and the input gradient;
  * MSG, B = 1 (96 / 256 / 512 feature channels: a 3-tile transposed layer on the 4-wave kernel, the 16-tile one stays on
    eight waves): log-probs and the input gradient.

Checked: sized == unsized byte for byte, two sized children byte-identical, every room of either path inside the bars of
tests/test_gpu_parity.py / tests/test_gpu_msg.py against the reference-generated fixtures (1e-4 on log-probs, check_grad's
clauses on the colour gradient, unchanged), and the two children's launch sites differ (the switch selected other kernels)."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
LOGP_TOL = 1e-4     # tests/test_gpu_parity.py


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
    from pointsecguard_amd import _lib, runtime
    from pointsecguard_amd.synthetic import msg_state_dict

    def dev(a, dt=None):
        t = torch.from_numpy(np.ascontiguousarray(a))
        return (t.to(dt) if dt is not None else t).cuda().contiguous()

    def run(model, g, B, arch=None):
        kw = {} if arch is None else {"arch": arch}
        ws = runtime.PN2Workspace(B, 4096, 2, **kw)
        x0 = dev(np.repeat(g["room"][None], B, axis=0))
        starts = dev(np.repeat(g["starts"].reshape(1, 4, 1), B, axis=2), torch.int32)
        ws.plan_build(x0, starts, 1)
        logp = ws.forward(model, 0, x0)
        acts = [ws.activation(w).cpu().numpy() for w in range(7)]
        labels = dev(np.repeat(g["labels"].astype(np.int32)[None], B, axis=0))
        dlogp = torch.empty_like(logp)
        _lib.call("psg_ce_logp_grad", runtime.ptr(logp), runtime.ptr(labels), 0, B * 4096, B * 4096, 13, 1.0 / 4096,
                  runtime.ptr(dlogp), None, runtime.stream())
        dx0 = ws.backward(model, 0, dlogp)
        torch.cuda.synchronize()
        return logp.cpu().numpy(), acts, dx0.cpu().numpy()

    out = {}
    ssg = runtime.PN2Model(runtime.fold_state_dict(dict(np.load(os.path.join(GOLDEN, "pn2_weights.npz")))))
    g = dict(np.load(os.path.join(GOLDEN, "pn2_room.npz")))
    for B in (1, 3):
        logp, acts, dx0 = run(ssg, g, B)
        out["ssg%d_logp" % B] = logp
        out["ssg%d_dx0" % B] = dx0
        for w, a in enumerate(acts):
            out["ssg%d_act%d" % (B, w)] = a
    gm = dict(np.load(os.path.join(GOLDEN, "pn2msg_room.npz")))
    msg = runtime.PN2Model(runtime.fold_state_dict(msg_state_dict(int(gm["msg_seed"])), msg=True), arch=runtime.ARCH_MSG)
    logp, _, dx0 = run(msg, gm, 1, runtime.ARCH_MSG)
    out["msg1_logp"] = logp
    out["msg1_dx0"] = dx0
    np.savez(out_path, **out)


def _child(tmp_path, tag, value):
    env = dict(os.environ)
    env["PSG_PN2_PW_SIZED"] = value
    env["PSG_TRACE_SYNC"] = "1"
    out = str(tmp_path / ("%s.npz" % tag))
    r = subprocess.run([sys.executable, os.path.abspath(__file__), out], env=env, cwd=ROOT, capture_output=True, text=True,
                       timeout=600)
    assert r.returncode == 0, (r.stdout + r.stderr)[-3000:]
    sites = set(re.findall(r"\[psg trace\] launch \d+ at (\S+) issued", r.stderr + r.stdout))
    return dict(np.load(out)), sites


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("pw_sized")
    return {"off": _child(tmp, "off", "0"), "on": _child(tmp, "on", "1"), "on2": _child(tmp, "on2", "1")}


@pytest.mark.gpu
def test_sized_is_byte_equal_to_unsized_and_reproducible(runs):
    (off, off_sites), (on, on_sites), (on2, _) = runs["off"], runs["on"], runs["on2"]
    assert sorted(on) == sorted(off)
    for k in sorted(on):
        assert on[k].tobytes() == on2[k].tobytes(), "%s: two runs of the sized path differ" % k
        assert on[k].tobytes() == off[k].tobytes(), "%s: sized and unsized paths differ" % k
    # the switch selected other launches: the #nw2 / #nw4 sites exist with it on only
    assert any("#nw2" in s for s in on_sites) and any("#nw4" in s for s in on_sites), sorted(on_sites)
    assert not any("#nw" in s for s in off_sites), sorted(off_sites)


@pytest.mark.gpu
@pytest.mark.parametrize("path", ["on", "off"])
@pytest.mark.parametrize("B", [1, 3])
def test_ssg_rooms_vs_reference(runs, golden_room, path, B):
    r, g = runs[path][0], golden_room
    for b in range(B):
        for which, name in enumerate(("sa1", "sa2", "sa3", "sa4", "fp4", "fp3", "fp2")):
            assert np.abs(r["ssg%d_act%d" % (B, which)][b] - g["act_" + name]).max() <= LOGP_TOL, (b, name)
        assert np.abs(r["ssg%d_logp" % B][b] - g["logp"]).max() <= LOGP_TOL, b
        check_grad(r["ssg%d_dx0" % B][b, :, 3:6], g["dcolor"])


@pytest.mark.gpu
@pytest.mark.parametrize("path", ["on", "off"])
def test_msg_room_vs_reference(runs, path):
    r = runs[path][0]
    g = dict(np.load(os.path.join(GOLDEN, "pn2msg_room.npz")))
    assert np.abs(r["msg1_logp"][0] - g["logp"]).max() <= LOGP_TOL
    check_grad(r["msg1_dx0"][0, :, 3:6], g["dcolor"])


if __name__ == "__main__":
    _child_main(sys.argv[1])
