"""CPU side of the ResGCN coordinate-field attacks: the float64 references of tests/gcn_field_ref64.py
pinned to torch, the membership rule of the Smooth kernel's second pass replayed in fp32 numpy with its mutants, the static
checks of the new symbols and kernels, and the field / atype mapping of the four attacks."""
import os
import re
import shutil
import subprocess
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import attack_ref64 as A
import gcn_field_ref64 as G
import nu_field_ref64 as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "pointsecguard_amd", "csrc")
NEW = ("psg_smooth_knn_xyz_sym_rooms", "psg_nu_coord_adam_step_rooms_w", "psg_gcn_nb_attack_field", "psg_gcn_nu_field_window")
KERNELS = ("smooth_xyz_sym_incoming_kernel", "nu_coord_adam_w_kernel")
BETA1, BETA2, ADAM_EPS, LR = 0.9, 0.999, 1e-8, 0.01
F = np.float32

needs_hipcc = pytest.mark.skipif(shutil.which("hipcc") is None and not os.path.exists("/opt/rocm/bin/hipcc"), reason="needs hipcc")


# ================================================================================================ the references pinned
@pytest.mark.parametrize("n,sigma,nb", [(333, 0.0, 10), (333, 1e-2, 5), (1024, 1e-4, 16)])
def test_sym_smooth_reference_is_torch_autograd_float64(n, sigma, nb):
    xyz = G.sym_points(n, sigma)
    ref = G.sym_smooth(xyz, nb)
    total, grad = G.sym_smooth_torch(xyz, nb)
    assert abs(total - ref["total"]) <= 1e-12 * max(1.0, abs(total))
    assert np.abs(grad - ref["grad"]).max() <= 1e-9
    assert (ref["idx"][:, 0] == np.arange(n)).all() and (ref["d"][:, 0] == 0).all()       # itself, at distance 0, adds nothing
    assert ref["indeg"].sum() == n * nb and ref["indeg"].min() >= 1


def test_sym_smooth_gradient_sums_to_zero_in_float64():
    """every pair term enters once with each sign"""
    ref = G.sym_smooth(G.sym_points(1024, 1e-2), 10)
    assert np.abs(ref["grad"].sum(0)).max() <= 1e-10


@pytest.mark.parametrize("n", G.SYM_N)
def test_near_ties_of_the_float64_reference_stay_under_the_cap(n):
    """The only queries whose neighbour set fp32 may decide differently: float64 ranks nb and nb + 1 closer than twice the
    distance bound.  On the chosen inputs there is none, and no exact tie either."""
    for sigma in G.SYM_SIGMA:
        xyz = G.sym_points(n, sigma)
        d = R.dist64(xyz, xyz)
        s = np.sort(np.partition(d, 17, axis=1)[:, :18], axis=1)
        for nb in G.SYM_NB:
            gap = s[:, nb] - s[:, nb - 1]
            near = (gap > 0) & (gap < 2 * R.dist_bound(s[:, nb]))
            print("N=%d sigma=%g nb=%d: near ties %d, exact ties %d" % (n, sigma, nb, int(near.sum()), int((gap == 0).sum())))
            assert near.mean() <= G.TIE_SHARE_CAP
            assert (gap > 0).all()


def test_adam_with_two_weights_is_torch_adam_and_the_one_weight_reference():
    rng = np.random.default_rng(72)
    B, N, cs, cl = 2, 9, 1e-4, 0.7
    d0 = np.zeros((B, N, 3))
    p = torch.nn.Parameter(torch.from_numpy(d0.copy()))
    opt = torch.optim.Adam([p], lr=LR, betas=(BETA1, BETA2), eps=ADAM_EPS)
    d, m, v = d0.copy(), np.zeros_like(d0), np.zeros_like(d0)
    for t in (1, 2, 3, 4):
        dx0 = rng.standard_normal((B, N, 9)) * 10.0 ** rng.uniform(-6, -1, (B, N, 9))
        sg = rng.standard_normal((B, N, 3))
        opt.zero_grad()
        ((torch.from_numpy(dx0[:, :, 0:3]) * p).sum() + cl * (p * p).sum() + cs * (torch.from_numpy(sg) * p).sum()).backward()
        opt.step()
        d, m, v = G.coord_adam_step_w(d, m, v, None, dx0, sg, cs, cl, LR, BETA1, BETA2, ADAM_EPS, t)[:3]
        assert np.abs(d - p.detach().numpy()).max() <= 1e-12
    assert np.abs(d).max() > 1e-3
    # one weight for both terms: nu_field_ref64's reference, values and error model
    delta = (rng.standard_normal((B, N, 3)) * 1e-3).astype(F)
    mm, vv = (rng.standard_normal(delta.shape) * 1e-3).astype(F), (rng.random(delta.shape) * 1e-5).astype(F)
    dx0, sg = rng.standard_normal((B, N, 9)).astype(F), rng.standard_normal((B, N, 3)).astype(F)
    a = G.coord_adam_step_w(delta, mm, vv, None, dx0, sg, F(1e-4), F(1e-4), F(LR), F(BETA1), F(BETA2), F(ADAM_EPS), 7)
    b = R.coord_adam_step(delta, mm, vv, None, dx0, sg, F(1e-4), F(LR), F(BETA1), F(BETA2), F(ADAM_EPS), 7)
    for x, y in zip(a, b):
        assert np.array_equal(x, y)
    # teeth: the Smooth weight in the L2 term's place leaves the error model's bound
    c = G.coord_adam_step_w(delta, mm, vv, None, dx0, sg, F(1e-4), F(0.7), F(LR), F(BETA1), F(BETA2), F(ADAM_EPS), 7)
    assert (np.abs(a[1] - c[1]) > A.bound(c[5])).any()


# ================================================================================================ the two passes in fp32
def _inputs():
    return [("rooms", G.sym_points(1024, 1e-2)), ("clean", G.sym_points(333, 0.0)), ("duplicates", G.dup_points(1024)),
            ("few", G.sym_points(7, 0.0)), ("circle", G.circle_points())]


def test_direct_distance_is_bit_symmetric_in_fp32():
    for name, xyz in _inputs():
        d2 = G.d2_direct_fp32(xyz)
        assert np.array_equal(d2.view(np.uint32), d2.T.copy().view(np.uint32)), name
        d = np.sqrt(d2).astype(F)
        assert np.array_equal(d, R.dist_direct_fp32(xyz, xyz)) and (np.diag(d) == 0).all(), name


@pytest.mark.parametrize("nb", [5, 10, 16])
def test_membership_rule_of_the_second_pass_reproduces_the_lists(nb):
    """member(k, i) <=> (d(k, i), i) <= (d(k, j*), j*), j* the last neighbour k actually holds - on rooms, exact duplicates,
    fewer points than neighbours, and distances that collide after the root"""
    for name, xyz in _inputs():
        d2 = G.d2_direct_fp32(xyz)
        d = np.sqrt(d2).astype(F)
        lists = G.pass1_lists(d, nb)
        assert lists.shape[1] == min(nb, len(xyz))
        want = G.members_of_lists(lists, len(xyz))
        assert np.array_equal(G.pass2_members(d, lists), want), name


def test_comparing_squares_or_dropping_the_index_is_caught():
    xyz = G.circle_points()
    d2 = G.d2_direct_fp32(xyz)
    d = np.sqrt(d2).astype(F)
    ring = d[0, 1:]
    assert len(np.unique(d2[0, 1:])) > len(np.unique(ring))              # different d^2, one d
    caught = {"d2": 0, "no_index": 0}
    for nb in range(2, 17):
        lists = G.pass1_lists(d, nb)
        want = G.members_of_lists(lists, len(xyz))
        assert np.array_equal(G.pass2_members(d, lists), want)
        for rule in caught:
            caught[rule] += int(not np.array_equal(G.pass2_members(d, lists, rule, d2), want))
    print("mutants caught at", caught, "of 15 neighbour counts")
    assert caught["d2"] > 0 and caught["no_index"] > 0
    # exact duplicates: the index clause alone decides
    xyz = G.dup_points(1024)
    d = np.sqrt(G.d2_direct_fp32(xyz)).astype(F)
    lists = G.pass1_lists(d, 5)
    assert not np.array_equal(G.pass2_members(d, lists, "no_index"), G.members_of_lists(lists, 1024))


def test_fp32_lists_equal_float64_lists_and_duplicates_are_decided_by_index():
    for name, xyz in _inputs()[:3]:
        d = np.sqrt(G.d2_direct_fp32(xyz)).astype(F)
        for nb in (5, 10):
            ref = G.sym_smooth(xyz, nb)
            assert np.array_equal(G.pass1_lists(d, nb), ref["idx"]), (name, nb)


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
    body = re.search(r"typedef struct psg_gcn_nu_field_window_args \{(.*?)\} psg_gcn_nu_field_window_args;", header, flags=re.S).group(1)
    fields = []
    for decl in body.split(";"):
        decl = decl.strip()
        if decl:
            fields += [f.strip().lstrip("*") for f in re.sub(r"^(const\s+)?\w+\s+", "", decl).split(",")]
    assert fields == [n for n, _ in _lib.GcnNuFieldWindowArgs._fields_]


@needs_hipcc
def test_new_kernels_use_no_scratch_and_no_inline_assembly(tmp_path):
    cmd = subprocess.run(["make", "-n", "-B", "psg_attack.o"], cwd=CSRC, capture_output=True, text=True, check=True).stdout
    line = next(l for l in cmd.splitlines() if "hipcc" in l and " -c " in l)
    path = os.path.join(str(tmp_path), "psg_attack.s")
    line = line.replace(" -c ", " -S --cuda-device-only -c ").replace("-o psg_attack.o", "-o " + path)
    subprocess.run(line, shell=True, cwd=CSRC, check=True, capture_output=True)
    text = open(path).read()
    for kernel in KERNELS:
        found = list(re.finditer(r"^(_Z\w*%s\w*):.*?^\s*s_endpgm.*?; ScratchSize: (\d+)" % kernel, text, flags=re.S | re.M))
        assert len(found) == 1, kernel
        m = found[0]
        assert int(m.group(2)) == 0, m.group(1)
        assert not re.search(r"\bscratch_(load|store)", m.group(0))
        assert "ASMSTART" not in m.group(0)
        desc = re.search(r"\.amdhsa_kernel %s\n(.*?)\.end_amdhsa_kernel" % re.escape(m.group(1)), text, flags=re.S).group(1)
        assert re.search(r"\.amdhsa_private_segment_fixed_size 0\b", desc)
        print(kernel, re.search(r"; NumVgprs: (\d+)", text[m.end():m.end() + 2000]))


# ================================================================================================ field / atype mapping
def _net():
    from pointsecguard_amd.resgcn.sem_seg_dense.architecture import DenseDeepGCN
    opt = SimpleNamespace(n_filters=64, k=16, act="relu", norm="batch", bias=True, epsilon=0.0, stochastic=True,
                          conv="edge", n_blocks=5, block="res", in_channels=9, dropout=0.0, n_classes=13)
    return DenseDeepGCN(opt).eval()


def test_field_argument_of_the_four_attacks():
    from pointsecguard_amd.resgcn.sem_seg_dense.attacks import torchattacks as ta
    net = _net()
    for cls in (ta.NB_attack, ta.tar_NB_attack, ta.NU_attack, ta.tar_NU_attack):
        assert cls(net).field == "color"
        for field in ("coord", "both"):
            assert cls(net, field=field).field == field
        with pytest.raises(ValueError):
            cls(net, field="normals")
    nb = ta.NB_attack(net, eps=0.1, alpha=0.01)
    assert (nb.coord_eps, nb.coord_alpha) == (0.1, 0.01)
    nb = ta.tar_NB_attack(net, eps=0.1, alpha=0.01, coord_eps=0.02, coord_alpha=0.005)
    assert (nb.coord_eps, nb.coord_alpha) == (0.02, 0.005)
    assert ta.NU_attack(net).coord_lr is None
    t = ta.tar_NU_attack(net, coord_c=0.3, coord_lr=0.02)
    assert (t.coord_c, t.coord_lr) == (0.3, 0.02)


def test_atype_selects_the_field_and_must_not_contradict_it():
    from pointsecguard_amd.resgcn.sem_seg_dense.attacks.torchattacks.attacks.colper import resolve_field
    assert resolve_field("color", "Color") == "color"
    assert resolve_field("coord", "Color") == "coord" and resolve_field("both", "Color") == "both"
    assert resolve_field("color", "Coord") == "coord" and resolve_field("color", "Both") == "both"
    assert resolve_field("coord", "Coord") == "coord" and resolve_field("both", "Both") == "both"
    for field, atype in (("coord", "Both"), ("both", "Coord")):
        with pytest.raises(ValueError):
            resolve_field(field, atype)
    with pytest.raises(ValueError):
        resolve_field("normals", "Color")


def test_nb_attack_refuses_a_contradicting_or_unknown_atype_before_any_device_work():
    from pointsecguard_amd.resgcn.sem_seg_dense.attacks import torchattacks as ta
    net = _net()
    with pytest.raises(ValueError):
        ta.NB_attack(net, field="both").forward(torch.zeros(1, 9, 128, 1), torch.zeros(1, 128), atype="Coord")
    with pytest.raises(NotImplementedError):
        ta.NB_attack(net, field="coord").forward(torch.zeros(1, 9, 128, 1), torch.zeros(1, 128), atype="Normal")


def test_more_than_one_room_through_forward_raises_and_names_forward_rooms():
    from pointsecguard_amd.resgcn.sem_seg_dense.attacks import torchattacks as ta
    net = _net()
    images, labels = torch.zeros(2, 9, 128, 1), torch.zeros(2, 128)
    for atk in (ta.NU_attack(net, field="coord"), ta.tar_NU_attack(net, field="both", target=1, mask=np.ones(128, bool))):
        with pytest.raises(ValueError, match="forward_rooms"):
            atk.forward(images, labels)
