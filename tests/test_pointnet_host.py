"""CPU tests of the vanilla PointNet path: the module's parameter layout against the reference's state_dict list, the
BatchNorm fold and the split / fold identities of the gfx950 forward in float64 against the reference's recorded
activations, and static checks of the psg_pointnet translation unit (asm hazards, no scratch)."""
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CSRC = os.path.join(ROOT, "pointsecguard_amd", "csrc")
sys.path.insert(0, HERE)
import pointnet_ref64 as ref64  # noqa: E402

PN_SEED, ROOM_SEED = 3, 5


def _golden(name):
    return np.load(os.path.join(HERE, "golden", name))


def test_state_dict_layout_is_the_references():
    from pointsecguard_amd import synthetic
    from pointsecguard_amd.models.pointnet_sem_seg import get_model
    want = [(k, tuple(s)) for k, s in json.load(open(os.path.join(HERE, "golden", "pointnet_keys.json")))]
    got = [(k, tuple(v.shape)) for k, v in get_model(13).state_dict().items()]
    assert got == want
    sd = synthetic.pointnet_state_dict(PN_SEED)
    assert sorted((k, tuple(np.shape(v))) for k, v in sd.items()) == sorted(want)
    m = get_model(13)
    m.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in sd.items()}, strict=True)


def test_module_contract_on_host():
    from pointsecguard_amd.models import pointnet_sem_seg
    with pytest.raises(NotImplementedError):
        pointnet_sem_seg.get_model(13, with_rgb=False)
    with pytest.raises(ValueError):
        pointnet_sem_seg.get_model(40)
    m = pointnet_sem_seg.get_model(13).eval()
    from pointsecguard_amd import _lib
    with pytest.raises(_lib.PsgError):
        m(torch.zeros(1, 9, 128))        # no CPU path


def _room_x():
    from pointsecguard_amd import synthetic
    return torch.from_numpy(np.ascontiguousarray(synthetic.make_rooms(2, ROOM_SEED).transpose(0, 2, 1))).double()


def test_restatement_reproduces_the_reference():
    from pointsecguard_amd import synthetic
    g = _golden("pointnet_room.npz")
    sd = synthetic.pointnet_state_dict(PN_SEED)
    logp, tf, ex = ref64.forward(sd, _room_x(), extras=True)
    assert np.abs(logp.numpy() - g["logp"]).max() <= 1e-4
    assert np.abs(tf.numpy() - g["trans_feat"]).max() <= 1e-6
    assert np.abs(ex["trans"].numpy() - g["trans"]).max() <= 1e-6
    # the fixture weights keep both transforms near the identity (the parity bars stay meaningful)
    assert np.abs(g["trans"] - np.eye(3)).max() < 0.1 and np.abs(g["trans_feat"] - np.eye(64)).max() < 0.15
    for name in ("stn", "fstn", "feat"):
        assert np.abs(ex["g_" + name].numpy() - g["g_" + name]).max() <= 1e-4
        decided = g["gap_" + name] > 1e-4
        assert np.array_equal(ex["arg_" + name].numpy()[decided], g["arg_" + name][decided])


def test_fold_identities_in_float64():
    """BN fold + identity-in-bias + per-room transform folds + global columns as a per-room bias, in float64, give the
    unfolded network's activations within 1e-6"""
    from pointsecguard_amd import runtime, synthetic
    sd = synthetic.pointnet_state_dict(PN_SEED)
    x = _room_x()
    logp, tf = ref64.forward(sd, x)
    f64 = [(np.asarray(w, np.float64), np.asarray(b, np.float64)) for w, b in runtime.fold_pointnet_state_dict(sd)]
    assert [w.shape for w, _ in f64] == [(64, 6), (128, 64), (1024, 128), (512, 1024), (256, 512), (9, 256), (64, 6),
                                        (64, 64), (128, 64), (1024, 128), (512, 1024), (256, 512), (4096, 256),
                                        (128, 64), (1024, 128), (512, 1088), (256, 512), (128, 256), (13, 128)]
    lp2, tf2 = ref64.folded_forward(f64, x)
    g = _golden("pointnet_room.npz")
    assert np.abs(tf2.numpy() - tf.numpy()).max() <= 1e-6
    assert np.abs(tf2.numpy() - g["trans_feat"]).max() <= 1e-6
    # the identities themselves, on the fold before its fp32 rounding: 1e-6 on every output
    f64x = runtime.fold_pointnet_state_dict(sd, dtype=np.float64)
    lp3, tf3 = ref64.folded_forward(f64x, x)
    assert np.abs(lp3.numpy() - logp.numpy()).max() <= 1e-6
    assert np.abs(tf3.numpy() - tf.numpy()).max() <= 1e-6


def test_flat_import_model_dispatches_to_the_pointnet_attacks():
    """INTEGRATION section 1 imports the model module by file name: a second class object, which the attacks must still
    recognise (they dispatch on a class marker, not on class identity)"""
    import importlib
    import pointsecguard_amd
    from pointsecguard_amd.attacks.torchattacks.attacks.pointnet import is_pointnet
    from pointsecguard_amd.models.pointnet2_sem_seg import get_model as pn2_model
    pkg = os.path.dirname(pointsecguard_amd.__file__)
    saved_path, saved_mods = list(sys.path), dict(sys.modules)
    try:
        sys.path.insert(0, os.path.join(pkg, "models"))
        flat = importlib.import_module("pointnet_sem_seg")
        from pointsecguard_amd.models.pointnet_sem_seg import get_model
        assert flat.get_model is not get_model
        assert is_pointnet(flat.get_model(13)) and is_pointnet(get_model(13))
        assert not is_pointnet(pn2_model(13))
    finally:
        sys.path[:] = saved_path
        for k in list(sys.modules):
            if k not in saved_mods:
                del sys.modules[k]


def _make_line(unit):
    cmd = subprocess.run(["make", "-n", "-B", unit + ".o"], cwd=CSRC, capture_output=True, text=True, check=True).stdout
    return next(l for l in cmd.splitlines() if "hipcc" in l and " -c " in l)


@pytest.mark.skipif(not os.path.exists("/opt/rocm/bin/hipcc"), reason="needs hipcc")
def test_pointnet_unit_has_no_asm_hazards(tmp_path):
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import check_asm_hazards
    out = str(tmp_path / "psg_pointnet.s")
    line = _make_line("psg_pointnet").replace(" -c ", " -S --cuda-device-only -c ").replace("-o psg_pointnet.o", "-o " + out)
    subprocess.run(line, shell=True, cwd=CSRC, check=True, capture_output=True)
    text = open(out).read()
    assert "pn_max_gemm_kernel" in text and "v_mfma_f32_32x32x2" in text
    assert check_asm_hazards.scan(out) == []


@pytest.mark.skipif(not os.path.exists("/opt/rocm/bin/hipcc"), reason="needs hipcc")
def test_pointnet_kernels_use_no_scratch(tmp_path):
    line = _make_line("psg_pointnet").replace(" -c ", " --cuda-device-only -Rpass-analysis=kernel-resource-usage -c ")
    line = line.replace("-o psg_pointnet.o", "-o " + str(tmp_path / "x.o"))
    r = subprocess.run(line, shell=True, cwd=CSRC, check=True, capture_output=True, text=True)
    names = re.findall(r"remark: [^\n]*Function Name: (\S+)", r.stderr)
    scratch = [int(v) for v in re.findall(r"ScratchSize \[bytes/lane\]: (\d+)", r.stderr)]
    assert len(names) >= 8 and len(scratch) == len(names)
    assert all(s == 0 for s in scratch), list(zip(names, scratch))
