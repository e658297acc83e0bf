"""The packed SA backward of PointNet++ SSG levels 1 - 3 (psg_pn2_kernels.cuh: sa_bwd_packed_kernel with SPV > 0): the level's
sparse max-pool transpose runs in batches over the groups of a packed workgroup, the mask pass, the transposed second layer and
the stores over its valid rows only, and the level's forward keys its ReLU masks by packed workgroup.  Every valid row keeps its
fmaf chain and its k-loops, so all gradients must agree BYTE for byte whichever levels run packed.  PSG_PN2_PACK_BWD is read
once per process: each value runs in a fresh child interpreter (this file run as a script), with PSG_TRACE_SYNC=1.

The scheme of tests/test_gpu_sa_pack_bwd.py: per room kind of tests/sa_pack_bwd_levels_rooms.py (that test's seven, with its
seeds and starts, and "twofull": an unaligned workgroup of two full groups at level 1; what the rooms hold at levels 1 - 3 is
stated on the CPU by tests/test_sa_pack_bwd_levels_host.py), with B = 2, N = 4096 (the network's smallest shape) and a plan of two
forwards, a child computes the colour-only gradient, psg_pn2_backward, psg_pn2_backward_full and a 3-iteration
psg_pn2_nb_attack; for the golden room the gradient the fixtures pin.

Checked: the children (unset, L0, L01, L02, L03, L0123, PSG_PN2_PACK_BWD=0, PSG_PN2_PACK=0) are byte-equal on every array;
launch sites ending in #bwd#packed appear exactly for the levels a child names (levels 1 - 3 carry #sa2 / #sa3 / #sa4; the
unset child runs the default set, level 0 among it); the golden room's gradient stays inside the bars of
tests/test_gpu_parity.py on every child."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
CHILDREN = (("unset", {}, None), ("L0", {"PSG_PN2_PACK_BWD": "L0"}, {0}), ("L01", {"PSG_PN2_PACK_BWD": "L01"}, {0, 1}),
            ("L02", {"PSG_PN2_PACK_BWD": "L02"}, {0, 2}), ("L03", {"PSG_PN2_PACK_BWD": "L03"}, {0, 3}),
            ("L0123", {"PSG_PN2_PACK_BWD": "L0123"}, {0, 1, 2, 3}), ("bwd_off", {"PSG_PN2_PACK_BWD": "0"}, set()),
            ("off", {"PSG_PN2_PACK": "0"}, set()))


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
    import sa_pack_bwd_levels_rooms as lr
    from pointsecguard_amd import _lib, runtime
    from pointsecguard_amd.synthetic import rule_labels
    B, N, ITERS = lr.B, lr.N, lr.ITERS

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
    for ki, kind in enumerate(lr.ROOM_KINDS):
        rooms, starts = lr.rooms_and_starts(ki, kind)
        labels = dev(rule_labels(rooms).astype(np.int32))
        x0 = dev(rooms)
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
    tmp = tmp_path_factory.mktemp("sa_pack_bwd_levels")
    return {tag: _child(tmp, tag, switches) for tag, switches, _ in CHILDREN}


def packed_levels(sites):
    """the SA levels whose backward launched packed: levels 1 - 3 carry their module's tag, level 0 none"""
    levels = set()
    for s in sites:
        if s.endswith("#bwd#packed"):
            m = re.search(r"#sa([234])#bwd#packed$", s)
            levels.add(int(m.group(1)) - 1 if m else 0)
    return levels


@pytest.mark.gpu
def test_all_children_byte_equal(runs):
    import sa_pack_bwd_levels_rooms as lr
    ref = runs["bwd_off"][0]
    assert len(ref) == 5 * len(lr.ROOM_KINDS) + 1
    for tag, _, _ in CHILDREN:
        other = runs[tag][0]
        assert sorted(other) == sorted(ref)
        for k in sorted(ref):
            assert ref[k].tobytes() == other[k].tobytes(), "%s: PSG_PN2_PACK_BWD=0 and %s differ" % (k, tag)
    for kind in lr.ROOM_KINDS:
        assert np.abs(ref[kind + "_dcolour"]).max() > 0 and np.abs(ref[kind + "_dx0_full"][..., 0:3]).max() > 0, kind


@pytest.mark.gpu
def test_packed_backward_sites_exactly_for_the_named_levels(runs):
    for tag, _, named in CHILDREN:
        levels = packed_levels(runs[tag][1])
        if named is None:
            assert 0 in levels, sorted(runs[tag][1])          # the default set: level 0 and the levels enabled on measured merit
        else:
            assert levels == named, (tag, sorted(runs[tag][1]))


@pytest.mark.gpu
@pytest.mark.parametrize("path", [tag for tag, _, _ in CHILDREN])
def test_golden_room_gradient_vs_reference(runs, golden_room, path):
    import sa_pack_bwd_levels_rooms as lr
    r = runs[path][0]
    for b in range(lr.B):
        check_grad(r["golden_dx0"][b, :, 3:6], golden_room["dcolor"])


if __name__ == "__main__":
    _child_main(sys.argv[1])
