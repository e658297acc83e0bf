"""The NB loop's fused fp1 + head launch (psg_pn2_kernels.cuh: fp1_loop_kernel - fp1 + head forward, CE gradient and fp1 + head
backward of a 64-point tile in one workgroup) against the three launches it replaces (PSG_PN2_FP1_LOOP=0: fp_fwd_kernel<64, 4>,
ce_logp_grad_kernel, fp_bwd_kernel<64, 4, 2>).  Every tile runs the same k-loops and the same row arithmetic, so the two paths
must agree BYTE for byte.  The switch is read once per process: each value runs in a fresh child interpreter (this file run as a
script) with PSG_TRACE_SYNC=1, the second child only after the first returned 0.

A child computes
  * psg_pn2_nb_attack on seeded synthetic rooms with explicit FPS starts:
      ssg_b1    SSG, B = 1, N = 1024 (the smallest workspace: 16 workgroups of the fused kernel), 3 iterations
      ssg_b3    SSG, B = 3, N = 4096, 2 iterations (rooms above 0; 192 workgroups in xcd_tile's order)
      msg_b1    MSG, B = 1, N = 1024, 2 iterations
      tar_b3    SSG targeted, B = 3, N = 1024 (rooms 1 and 2 are rows beyond rows_active), 2 iterations
      mask_b1   SSG with a point mask, 2 iterations
  * teacher-forced: psg_pn2_nb_step twice (plan slots 0 and 1, the second as the attack's last step) against the sequence
    psg_pn2_forward_lean -> psg_ce_logp_grad -> psg_pn2_backward_colour_pgd on the same inputs: the updated rooms and fp1's dZ1
    rows (psg_pn2_fp1_grad_ptr) after each step; SSG at B = 1, N = 1024, and SSG and MSG at B = 2, N = 4096 (real interpolation
    weights, unsaturated log-probs: where a differently rounded sum shows).
Weights: tests/golden/pn2_weights.npz (SSG), msg_state_dict(seed of tests/golden/pn2msg_room.npz) (MSG)."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
EPS, ALPHA = 0.05, 2 / 255
MARK_STEP = "[fp1_loop child] teacher-forced steps"


def _starts(rng, iters, batch, n_point):
    n_src = (n_point, 1024, 256, 64)
    return np.stack([rng.integers(0, n, (iters, batch)) for n in n_src], axis=1).astype(np.int32)   # [iters][4][B]


def _child_main(out_path):
    import torch
    sys.path.insert(0, ROOT)
    from pointsecguard_amd import _lib, runtime
    from pointsecguard_amd.synthetic import make_rooms, msg_state_dict, rule_labels

    def dev(a, dt=None):
        t = torch.from_numpy(np.ascontiguousarray(a))
        return (t.to(dt) if dt is not None else t).cuda().contiguous()

    ssg = runtime.PN2Model(runtime.fold_state_dict(dict(np.load(os.path.join(GOLDEN, "pn2_weights.npz")))))
    seed = int(np.load(os.path.join(GOLDEN, "pn2msg_room.npz"))["msg_seed"])
    msg = runtime.PN2Model(runtime.fold_state_dict(msg_state_dict(seed), msg=True), arch=runtime.ARCH_MSG)
    out = {}

    def attack(name, model, arch, batch, n_point, iters, seed, target=None, mask=None):
        rooms = make_rooms(batch, seed, num_point=n_point)
        rooms = rooms.numpy() if hasattr(rooms, "numpy") else np.asarray(rooms)
        labels = None if target is not None else dev(rule_labels(rooms).astype(np.int32))
        starts = dev(_starts(np.random.default_rng(seed + 1), iters, batch, n_point))
        ws = runtime.PN2Workspace(batch, n_point, iters, arch=arch)
        images = dev(rooms.transpose(0, 2, 1))
        adv = ws.nb_attack(model, images, labels, starts, EPS, ALPHA, iters, mask=mask, target=target)
        out[name] = adv.cpu().numpy()
        assert not np.array_equal(out[name], images.cpu().numpy()), name     # (the attack moved the colours)

    attack("ssg_b1", ssg, runtime.ARCH_SSG, 1, 1024, 3, 11)
    attack("ssg_b3", ssg, runtime.ARCH_SSG, 3, 4096, 2, 12)
    attack("msg_b1", msg, runtime.ARCH_MSG, 1, 1024, 2, 13)
    attack("tar_b3", ssg, runtime.ARCH_SSG, 3, 1024, 2, 14, target=5)
    attack("mask_b1", ssg, runtime.ARCH_SSG, 1, 1024, 2, 15, mask=dev((np.random.default_rng(16).random(1024) < 0.6).astype(np.uint8)))
    torch.cuda.synchronize()
    sys.stderr.write(MARK_STEP + "\n")
    sys.stderr.flush()

    # teacher-forced: the exported step against the launches one at a time
    def steps(tag, model, arch, B, N, seed):
        rooms = make_rooms(B, seed, num_point=N)
        rooms = rooms.numpy() if hasattr(rooms, "numpy") else np.asarray(rooms)
        labels = dev(rule_labels(rooms).astype(np.int32))
        starts = dev(_starts(np.random.default_rng(seed + 1), 2, B, N))
        ws = runtime.PN2Workspace(B, N, 2, arch=arch)
        x_step, x_seq = dev(rooms), dev(rooms)
        ori = x_step[:, :, 3:6].contiguous()
        ws.plan_build(x_step, starts, 2)
        for slot in (0, 1):
            ws.nb_step(model, slot, x_step, ori, labels, ALPHA, EPS, last=slot == 1)
            out["%s_step_x%d" % (tag, slot)] = x_step.cpu().numpy()
            out["%s_step_dz%d" % (tag, slot)] = ws.fp1_grad().cpu().numpy()
            logp = ws.forward(model, slot, x_seq, lean=True)
            dlogp = torch.empty_like(logp)
            _lib.call("psg_ce_logp_grad", runtime.ptr(logp), runtime.ptr(labels), 0, B * N, B * N, 13, 1.0 / N, runtime.ptr(dlogp),
                      None, runtime.stream())
            ws.backward_pgd(model, slot, dlogp, x_seq, ori, ALPHA, EPS, last=slot == 1)
            out["%s_seq_x%d" % (tag, slot)] = x_seq.cpu().numpy()
            out["%s_seq_dz%d" % (tag, slot)] = ws.fp1_grad().cpu().numpy()

    steps("ssg1024", ssg, runtime.ARCH_SSG, 1, 1024, 21)
    # (at N = 1024 every point is its own nearest coarse point: interpolation weights 1, 0, 0.  N = 4096 has real weights, and
    # the MSG network's unfitted weights give unsaturated log-probs: the rounding of the gather's sums and of the CE row's log
    # shows there and not in the first case)
    steps("ssg4096", ssg, runtime.ARCH_SSG, 2, 4096, 23)
    steps("msg4096", msg, runtime.ARCH_MSG, 2, 4096, 25)
    torch.cuda.synchronize()
    np.savez(out_path, **out)


def _child(tmp, tag, value):
    env = dict(os.environ)
    for name in ("PSG_PN2_FP1_LOOP", "PSG_FP1_WAVE", "PSG_PN2_FPSPLIT", "PSG_PN2_PGD_FUSE", "PSG_PN2_GRAPH"):
        env.pop(name, None)
    if value is not None:
        env["PSG_PN2_FP1_LOOP"] = value
    env["PSG_TRACE_SYNC"] = "1"
    out = str(tmp / ("%s.npz" % tag))
    r = subprocess.run([sys.executable, os.path.abspath(__file__), out], env=env, cwd=ROOT, capture_output=True, text=True,
                       timeout=300)
    assert r.returncode == 0, (r.stdout + r.stderr)[-3000:]
    attack_log, _, step_log = r.stderr.partition(MARK_STEP)
    sites = [set(re.findall(r"\[psg trace\] launch \d+ at (\S+) issued", part)) for part in (attack_log, step_log)]
    return dict(np.load(out)), sites[0], sites[1]


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("fp1_loop")
    fused = _child(tmp, "fused", None)           # (an assertion inside ends the fixture: the second child is not started then)
    return {"fused": fused, "split": _child(tmp, "split", "0")}


@pytest.mark.gpu
@pytest.mark.parametrize("case", ["ssg_b1", "ssg_b3", "msg_b1", "tar_b3", "mask_b1"])
def test_attack_is_byte_identical_to_the_three_launches(runs, case):
    fused, split = runs["fused"][0][case], runs["split"][0][case]
    assert fused.shape == split.shape and fused.dtype == np.float32
    assert np.isfinite(fused).all()
    assert fused.tobytes() == split.tobytes(), "%d of %d floats differ" % ((fused != split).sum(), fused.size)


@pytest.mark.gpu
@pytest.mark.parametrize("tag", ["ssg1024", "ssg4096", "msg4096"])
def test_teacher_forced_step_matches_the_launch_sequence(runs, tag):
    fused, split = runs["fused"][0], runs["split"][0]
    for slot in (0, 1):
        for what in ("x", "dz"):
            step, seq = fused["%s_step_%s%d" % (tag, what, slot)], fused["%s_seq_%s%d" % (tag, what, slot)]
            assert np.isfinite(step).all()
            # the fused step against the separate launches in the SAME process, and against the other process's step
            assert step.tobytes() == seq.tobytes(), (what, slot, int((step != seq).sum()))
            assert step.tobytes() == split["%s_step_%s%d" % (tag, what, slot)].tobytes(), (what, slot)
        assert np.abs(fused["%s_step_dz%d" % (tag, slot)]).max() > 0
    assert not np.array_equal(fused[tag + "_step_x0"], fused[tag + "_step_x1"])


def _ce_site():
    """file:line of psg_ce_logp_grad's launch check, as the tracer prints it"""
    src = open(os.path.join(ROOT, "pointsecguard_amd", "csrc", "psg_attack.hip")).read().split("\n")
    at = next(i for i, line in enumerate(src) if "hipLaunchKernelGGL(ce_logp_grad_kernel" in line)
    chk = next(i for i in range(at, len(src)) if "PSG_LAUNCH_CHECK()" in src[i])
    return "psg_attack.hip:%d" % (chk + 1)


@pytest.mark.gpu
def test_switch_selects_other_kernels(runs):
    (_, fused_attack, fused_step), (_, split_attack, _) = runs["fused"], runs["split"]
    ce = _ce_site()
    assert fused_attack and split_attack and fused_attack != split_attack, sorted(fused_attack ^ split_attack)
    assert ce in split_attack, (ce, sorted(split_attack))
    assert ce not in fused_attack                   # no CE launch between forward and backward
    assert ce in fused_step                         # (the site is spelled right: the teacher-forced sequence launches it)
    only_fused, only_split = fused_attack - split_attack, split_attack - fused_attack
    # the fused launch for the CE launch and fp1 + head's 64-point backward (its forward shares fp2 - fp4's launch line)
    assert len(only_fused) == 1 and next(iter(only_fused)).startswith("psg_pn2.hip:"), sorted(only_fused)
    assert ce in only_split and any(s.startswith("psg_pn2.hip:") for s in only_split), sorted(only_split)


if __name__ == "__main__":
    _child_main(sys.argv[1])
