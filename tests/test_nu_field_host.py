"""CPU side of the coordinate-field NU attacks: the float64 references of tests/nu_field_ref64.py pinned
to torch, the reason the new Smooth kernel exists shown in fp32 numpy, the teeth of the references, the static checks of the
new symbols and kernels (pattern of tests/test_pointnet_nu_static.py), and the host refusals."""
import os
import re
import shutil
import subprocess
import sys

import numpy as np
import pytest
import torch

import attack_ref64 as A
import nu_field_ref64 as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "pointsecguard_amd", "csrc")
NEW = ("psg_smooth_knn_xyz_rooms", "psg_nu_coord_apply_rooms", "psg_nu_coord_adam_step_rooms", "psg_pn2_nu_field_step")
KERNELS = ("smooth_knn_xyz_kernel", "nu_coord_apply_kernel", "nu_coord_adam_kernel")
BETA1, BETA2, ADAM_EPS, LR = 0.9, 0.999, 1e-8, 0.01
F = np.float32

needs_hipcc = pytest.mark.skipif(shutil.which("hipcc") is None and not os.path.exists("/opt/rocm/bin/hipcc"), reason="needs hipcc")


# ================================================================================================ the references pinned
def test_adam_on_delta_is_torch_adam_float64():
    rng = np.random.default_rng(70)
    B, N, c = 2, 9, 1e-4
    d0 = np.zeros((B, N, 3))
    p = torch.nn.Parameter(torch.from_numpy(d0.copy()))
    opt = torch.optim.Adam([p], lr=LR, betas=(BETA1, BETA2), eps=ADAM_EPS)
    d, m, v = d0.copy(), np.zeros_like(d0), np.zeros_like(d0)
    for t in (1, 2, 3, 4):
        dx0 = rng.standard_normal((B, N, 9)) * 10.0 ** rng.uniform(-6, -1, (B, N, 9))
        sg = rng.standard_normal((B, N, 3))
        opt.zero_grad()
        loss = (torch.from_numpy(dx0[:, :, 0:3]) * p).sum() + c * (p * p).sum() + c * (torch.from_numpy(sg) * p).sum()
        loss.backward()
        opt.step()
        d, m, v = R.coord_adam_step(d, m, v, None, dx0, sg, c, LR, BETA1, BETA2, ADAM_EPS, t)[:3]
        assert np.abs(d - p.detach().numpy()).max() <= 1e-12
    assert np.abs(d).max() > 1e-3


def test_smooth_reference_is_torch_cdist_topk_float64():
    for c in R.smooth_cases()[:2]:
        for b in range(c["B"]):
            ref = c["refs"][b]
            total, grad, idx = R.smooth_xyz_torch(c["adv"][b], c["ref"][b], c["nb"])
            assert abs(total - ref["total"]) <= 1e-12 * max(1.0, abs(total))
            # (at zero perturbation autograd's sqrt backward gives NaN at the self distance of 0; the reference's rule there
            # - that neighbour adds exactly zero - is what nan_to_num of a 0 / 0 stands for, and is pinned by the mutant below)
            assert np.abs(np.nan_to_num(grad) - ref["grad"]).max() <= 1e-9 or c["perts"][b] == 0.0
            if c["perts"][b] != 0.0:
                assert (np.sort(idx, 1) == np.sort(ref["idx"], 1)).all()
                assert np.abs(grad - ref["grad"]).max() <= 1e-9


def test_near_ties_of_the_float64_reference_stay_under_the_cap():
    """The only queries whose neighbour set fp32 may decide differently are rarer than 0.1 % on the chosen inputs."""
    for c in R.smooth_cases():
        for b in range(c["B"]):
            share = float(R.near_tie(c["refs"][b], c["nb"]).mean())
            print("%s room %d: near-tie share %.6f (cap %.4f)" % (c["name"], b, share, R.TIE_SHARE_CAP))
            assert share <= R.TIE_SHARE_CAP


# ================================================================================================ why the kernel exists
def test_expansion_distance_leaves_the_bound_the_direct_form_meets():
    """make_rooms(2, 5) room 0, channels 0:3, zero perturbation: the colour kernel's |a|^2 + |r|^2 - 2 a.r in fp32 misses the
    per-distance bound 4 * 2^-24 d by orders of magnitude and picks other neighbour sets; direct differences meet it."""
    from pointsecguard_amd.synthetic import make_rooms
    xyz = np.ascontiguousarray(make_rooms(2, 5)[0, :, 0:3])
    d64 = R.dist64(xyz, xyz)
    bound = R.dist_bound(d64)
    err_direct = np.abs(R.dist_direct_fp32(xyz, xyz).astype(np.float64) - d64)
    err_exp = np.abs(R.dist_expansion_fp32(xyz, xyz).astype(np.float64) - d64)
    k = 10
    top64 = np.sort(np.argsort(d64, 1, kind="stable")[:, :k], 1)
    differ = lambda d: float((np.sort(np.argsort(d, 1, kind="stable")[:, :k], 1) != top64).any(1).mean())     # noqa: E731
    share_exp, share_direct = differ(R.dist_expansion_fp32(xyz, xyz)), differ(R.dist_direct_fp32(xyz, xyz))
    print("expansion: largest distance error %.3e m, rows with another neighbour set %.4f %%" % (err_exp.max(), 100 * share_exp))
    print("direct:    largest distance error %.3e m, rows with another neighbour set %.4f %%; largest error / bound %.3f"
          % (err_direct.max(), 100 * share_direct, float((err_direct / bound).max())))
    assert (err_direct <= bound).all()
    assert share_direct == 0.0
    assert (err_exp > bound).any() and err_exp.max() > 1e3 * err_direct.max()
    assert share_exp > 0.0


# ================================================================================================ teeth of the references
def _adam_case(step):
    rng = np.random.default_rng([71, step])
    B, N = 2, 300
    delta = (rng.standard_normal((B, N, 3)) * 1e-3).astype(F)
    m = np.zeros_like(delta) if step == 1 else (rng.standard_normal(delta.shape) * 1e-3).astype(F)
    v = np.zeros_like(delta) if step == 1 else (rng.random(delta.shape) * 1e-5 + 1e-12).astype(F)
    dx0 = (rng.standard_normal((B, N, 9)) * 10.0 ** rng.uniform(-6, -3, (B, N, 9))).astype(F)
    sg = rng.standard_normal((B, N, 3)).astype(F)
    return lambda c, mutant=None: R.coord_adam_step(delta, m, v, None, dx0, sg, F(c), F(LR), F(BETA1), F(BETA2), F(ADAM_EPS), step,
                                                     mutant=mutant)


def _outside(mut, ref, e):
    return bool((~((mut == ref) | (np.abs(mut - ref) <= A.bound(e)))).any())


def test_adam_without_bias_correction_leaves_the_bound():
    run = _adam_case(7)
    ref, mut = run(1e-4), run(1e-4, "no_bias")
    assert _outside(mut[0], ref[0], ref[4])


def test_dropping_the_l2_gradient_leaves_the_bound():
    run = _adam_case(7)
    ref, mut = run(1.0), run(1.0, "no_l2_grad")           # coord_c = 1: the term is of the gradient's own size
    assert _outside(mut[1], ref[1], ref[5]) and _outside(mut[0], ref[0], ref[4])


def test_zero_distance_neighbour_with_a_unit_gradient_leaves_the_bound():
    c = R.smooth_cases()[0]                               # zero perturbation: every point's rank 0 is itself at distance 0
    ref = c["refs"][0]
    mut = R.smooth_xyz(c["adv"][0], c["ref"][0], c["nb"], mutant="zero_unit")
    assert (np.abs(mut["grad"] - ref["grad"]) > R.grad_bound(ref["abs_terms"], c["nb"])).any()


def test_tie_resolved_to_the_higher_index_breaks_equality():
    c = R.smooth_cases()[2]                               # room 0 holds exactly duplicated points
    ref = c["refs"][0]
    mut = R.smooth_xyz(c["adv"][0], c["ref"][0], c["nb"], mutant="tie_high")
    assert (np.sort(mut["idx"], 1) != np.sort(ref["idx"], 1)).any()
    assert (mut["idx"] != ref["idx"]).any()


# ================================================================================================ static checks
def test_new_symbols_are_declared_bound_and_exported():
    from pointsecguard_amd import _lib
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "psg.h")).read(), flags=re.S)
    exported = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    for name in NEW:
        assert re.search(r"\b%s\s*\(" % name, header), name
        assert name in _lib.SIGNATURES, name
        assert re.search(r" T %s$" % name, exported, flags=re.M), name
        proto = re.search(r"\b%s\s*\((.*?)\)\s*;" % name, header, flags=re.S).group(1)
        assert len(proto.split(",")) == len(_lib.SIGNATURES[name][1]), name
    body = re.search(r"typedef struct psg_nu_field_args \{(.*?)\} psg_nu_field_args;", header, flags=re.S).group(1)
    fields = []
    for decl in body.split(";"):
        decl = decl.strip()
        if decl:
            fields += [f.strip().lstrip("*") for f in re.sub(r"^(const\s+)?\w+\s+", "", decl).split(",")]
    assert fields == [n for n, _ in _lib.NuFieldArgs._fields_]


@needs_hipcc
def test_new_kernels_use_no_scratch_and_pass_the_hazard_lint(tmp_path):
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import check_asm_hazards
    cmd = subprocess.run(["make", "-n", "-B", "psg_attack.o"], cwd=CSRC, capture_output=True, text=True, check=True).stdout
    line = next(l for l in cmd.splitlines() if "hipcc" in l and " -c " in l)
    path = os.path.join(str(tmp_path), "psg_attack.s")
    line = line.replace(" -c ", " -S --cuda-device-only -c ").replace("-o psg_attack.o", "-o " + path)
    subprocess.run(line, shell=True, cwd=CSRC, check=True, capture_output=True)
    text = open(path).read()
    for kernel in KERNELS:
        found = list(re.finditer(r"^(_Z\w*%s\w*):.*?^\s*s_endpgm.*?; ScratchSize: (\d+)" % kernel, text, flags=re.S | re.M))
        assert found, kernel
        for m in found:                                    # (every instantiation of the templated one)
            assert int(m.group(2)) == 0, m.group(1)
            body = m.group(0)
            assert not re.search(r"\bscratch_(load|store)", body)
            assert "ASMSTART" not in body                  # no inline assembly in the new kernels
            desc = re.search(r"\.amdhsa_kernel %s\n(.*?)\.end_amdhsa_kernel" % re.escape(m.group(1)), text, flags=re.S).group(1)
            assert re.search(r"\.amdhsa_private_segment_fixed_size 0\b", desc)
    assert len(re.findall(r"^_Z\w*smooth_knn_xyz_kernel\w*:", text, flags=re.M)) == 3
    assert check_asm_hazards.scan(path) == []


# ================================================================================================ host refusals
def _ssg():
    from pointsecguard_amd.models.pointnet2_sem_seg import get_model
    return get_model(13).eval()


def test_unknown_field_raises():
    from pointsecguard_amd.attacks import torchattacks
    net = _ssg()
    for cls in (torchattacks.NU_attack, torchattacks.tar_NU_attack):
        with pytest.raises(ValueError):
            cls(net, field="normals")
        atk = cls(net)
        assert atk.field == "color" and atk.coord_c is None and atk.coord_lr is None


def test_more_than_one_room_through_forward_raises_and_names_forward_rooms():
    from pointsecguard_amd.attacks import torchattacks
    net = _ssg()
    images, labels = torch.zeros(2, 9, 128), np.zeros((2, 128))
    for atk in (torchattacks.NU_attack(net, field="coord"),
                torchattacks.tar_NU_attack(net, field="both", target=1, mask=np.ones(128, bool))):
        with pytest.raises(ValueError, match="forward_rooms"):
            atk(images, labels)


def test_pointnet_and_msg_raise_not_implemented():
    from pointsecguard_amd.attacks import torchattacks
    from pointsecguard_amd.models import pointnet2_sem_seg_msg, pointnet_sem_seg
    images, labels = torch.zeros(1, 9, 128), np.zeros((1, 128))
    for net in (pointnet_sem_seg.get_model(13).eval(), pointnet2_sem_seg_msg.get_model(13).eval()):
        for field in ("coord", "both"):
            with pytest.raises(NotImplementedError):
                torchattacks.NU_attack(net, field=field)(images, labels)
            with pytest.raises(NotImplementedError):
                torchattacks.tar_NU_attack(net, field=field, target=1, mask=np.ones(128, bool)).forward_rooms(images, labels, np.ones((1, 128), bool))
