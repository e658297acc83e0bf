"""CPU tests of the shared launch plumbing: the dynamic-LDS opt-in has one home in the HIP sources, the per-path copies of
the launch helper and the private PointNet++ profiler stay gone, and the BatchNorm folds of runtime.py, now on one shared
helper, return the bits of the implementation they replaced (kept below as the yardstick)."""
import os

import numpy as np
import pytest
import torch

from pointsecguard_amd import runtime, synthetic

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "pointsecguard_amd", "csrc")
GOLDEN = os.path.join(ROOT, "tests", "golden")


def csrc_sources():
    return {f: open(os.path.join(CSRC, f)).read() for f in sorted(os.listdir(CSRC)) if f.endswith((".hip", ".cuh", ".h"))}


def test_lds_opt_in_has_one_home():
    """Launch paths call psg::allow_big_lds (psg_api.hip: memoised per kernel, thread-safe); none reaches the driver itself."""
    users = [f for f, src in csrc_sources().items() if "hipFuncSetAttribute" in src]
    assert users == ["psg_api.hip"], users
    assert csrc_sources()["psg_api.hip"].count("hipFuncSetAttribute(") == 1


@pytest.mark.parametrize("name", ["launch_lds_colour", "launch_lds_fp_split", "ProfScope"])
def test_duplicated_plumbing_stays_gone(name):
    """One launch_lds that takes the caller's trace site, and psg_common.h's EvLog / EvScope as the only event profiler."""
    assert [f for f, src in csrc_sources().items() if name in src] == []


PN2_SWITCHES = ["PSG_PN2_SPLIT", "PSG_PN2_FPSPLIT", "PSG_FP1_WAVE", "PSG_PN2_PACK", "PSG_PN2_PACK_BWD", "PSG_PN2_POOLT_ORDER",
                "PSG_PN2_POOLT_SPARSE", "PSG_PN2_L1T_COLOUR", "PSG_PN2_PW_SIZED", "PSG_PN2_BALL_TABLE", "PSG_PN2_FP1_LOOP",
                "PSG_PN2_PGD_FUSE", "PSG_PN2_GRAPH", "PSG_DIAG"]


@pytest.mark.parametrize("name", PN2_SWITCHES)
def test_every_pn2_switch_is_read_in_one_place(name):
    """One env_int / env_str call per PointNet++ switch in csrc/: the switch set of psg_pn2_paths.h (Pn2Switches), which
    psg_pn2.hip fills once per process; nothing reads the environment on its own."""
    import re
    reads = [(f, m.group(0)) for f, src in csrc_sources().items() for m in re.finditer(r'env_(?:int|str)\(\s*"%s"' % re.escape(name), src)]
    assert len(reads) == 1 and reads[0][0] == "psg_pn2_paths.h", reads
    assert csrc_sources()["psg_pn2.hip"].count("read_switches(") == 1
    assert not any("getenv(" in src for f, src in csrc_sources().items() if f.startswith("psg_pn2"))


@pytest.mark.parametrize("kernel", ["sa_fwd_kernel<", "sa_fwd_packed_kernel<", "sa_bwd_kernel<", "sa_bwd_sparse_kernel<", "sa_bwd_packed_kernel<"])
def test_sa_kernels_are_named_by_the_table_visitor_alone(kernel):
    """psg_pn2.hip names each SA kernel with template arguments at most twice (run_sa_fwd / run_sa_bwd, from the row of the
    kernel table in psg_pn2_paths.h); the per-configuration switch tables and their key macro stay gone."""
    src = csrc_sources()["psg_pn2.hip"]
    assert 1 <= src.count(kernel) <= 2, src.count(kernel)
    assert "PSG_CFG_KEY" not in src


# ---- the folds as they were before runtime._as_f64 / runtime._fold_conv_bn (this project's own earlier code, verbatim)
def old_fold_state_dict(sd, eps=1e-5, msg=False):
    def arr(k):
        v = sd[k]
        if isinstance(v, torch.Tensor):
            v = v.detach().cpu().numpy()
        return np.asarray(v, np.float64)

    def fold(conv, bn):
        w = arr(conv + ".weight")
        w = w.reshape(w.shape[0], -1)
        b = arr(conv + ".bias")
        if bn is not None:
            s = arr(bn + ".weight") / np.sqrt(arr(bn + ".running_var") + eps)
            w = w * s[:, None]
            b = (b - arr(bn + ".running_mean")) * s + arr(bn + ".bias")
        return np.ascontiguousarray(w, np.float32), np.ascontiguousarray(b, np.float32)

    out = []
    if msg:
        for l in range(1, 5):
            for i in range(2):
                for j in range(3):
                    out.append(fold("sa%d.conv_blocks.%d.%d" % (l, i, j), "sa%d.bn_blocks.%d.%d" % (l, i, j)))
    else:
        for name in ("sa1", "sa2", "sa3", "sa4"):
            for i in range(3):
                out.append(fold("%s.mlp_convs.%d" % (name, i), "%s.mlp_bns.%d" % (name, i)))
    for name, nl in (("fp4", 2), ("fp3", 2), ("fp2", 2), ("fp1", 3)):
        for i in range(nl):
            out.append(fold("%s.mlp_convs.%d" % (name, i), "%s.mlp_bns.%d" % (name, i)))
    out.append(fold("conv1", "bn1"))
    out.append(fold("conv2", None))
    return out


def old_fold_pointnet_state_dict(sd, eps=1e-5, dtype=np.float32):
    def arr(k):
        v = sd[k]
        if isinstance(v, torch.Tensor):
            v = v.detach().cpu().numpy()
        return np.asarray(v, np.float64)

    out = []
    for layer, bn, iden in runtime.POINTNET_LAYERS:
        w = arr(layer + ".weight")
        w = w.reshape(w.shape[0], -1)
        b = arr(layer + ".bias")
        if bn is not None:
            s = arr(bn + ".weight") / np.sqrt(arr(bn + ".running_var") + eps)
            w = w * s[:, None]
            b = (b - arr(bn + ".running_mean")) * s + arr(bn + ".bias")
        if iden:
            b = b + np.eye(iden).reshape(-1)
        out.append((np.ascontiguousarray(w, dtype), np.ascontiguousarray(b, dtype)))
    return out


def assert_same_bits(got, want, n_layers):
    assert len(got) == len(want) == n_layers
    for i, ((w, b), (w0, b0)) in enumerate(zip(got, want)):
        for x, x0 in ((w, w0), (b, b0)):
            assert x.dtype == x0.dtype and x.shape == x0.shape and x.flags["C_CONTIGUOUS"], i
            assert x.tobytes() == x0.tobytes(), "layer %d" % i


def as_tensors(sd):
    return {k: torch.from_numpy(np.array(v)) for k, v in sd.items()}


def test_fold_state_dict_bits_ssg():
    sd = dict(np.load(os.path.join(GOLDEN, "pn2_weights.npz")))
    want = old_fold_state_dict(sd)
    assert_same_bits(runtime.fold_state_dict(sd), want, runtime.ARCH_LAYERS[runtime.ARCH_SSG])
    assert_same_bits(runtime.fold_state_dict(as_tensors(sd)), want, runtime.ARCH_LAYERS[runtime.ARCH_SSG])     # state_dict of tensors
    assert_same_bits(runtime.fold_state_dict(sd, eps=1e-3), old_fold_state_dict(sd, eps=1e-3), runtime.ARCH_LAYERS[runtime.ARCH_SSG])


def test_fold_state_dict_bits_msg():
    sd = synthetic.msg_state_dict(int(np.load(os.path.join(GOLDEN, "pn2msg_room.npz"))["msg_seed"]))     # (tests/test_oracle_msg.py)
    assert_same_bits(runtime.fold_state_dict(sd, msg=True), old_fold_state_dict(sd, msg=True), runtime.ARCH_LAYERS[runtime.ARCH_MSG])


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_fold_pointnet_state_dict_bits(dtype):
    sd = synthetic.pointnet_state_dict(3)     # (PN_SEED of tests/test_pointnet_host.py)
    want = old_fold_pointnet_state_dict(sd, dtype=dtype)
    assert_same_bits(runtime.fold_pointnet_state_dict(sd, dtype=dtype), want, len(runtime.POINTNET_LAYERS))
    assert_same_bits(runtime.fold_pointnet_state_dict(as_tensors(sd), dtype=dtype), want, len(runtime.POINTNET_LAYERS))
    assert want[0][0].dtype == dtype


def test_gcn_tensor_list_keeps_fp32():
    """gcn_tensor_list shares only the tensor -> ndarray step: fp32 throughout, conv weights flattened to two dimensions."""
    sd = dict(np.load(os.path.join(GOLDEN, "gcn_weights.npz")))
    n_blocks = 1 + len({k.split(".")[1] for k in sd if k.startswith("backbone.")})
    for got, t in zip(runtime.gcn_tensor_list(sd, n_blocks), runtime.gcn_tensor_list(as_tensors(sd), n_blocks)):
        assert got.dtype == np.float32 and got.ndim <= 2 and got.tobytes() == t.tobytes()
