"""The sparse max-pool transpose of the SA backward (psg_pn2_kernels.cuh: sa_pool_t_sparse, sa_bwd_sparse_kernel; selected per
level by run_sa_bwd, PSG_PN2_POOLT_SPARSE=0 keeps the dense transposed layer).

GPU: the switch is read once per process, so each value runs in a fresh child interpreter (this file run as a script) that
computes the SSG forward + full input-gradient backward of the golden room and a 40-iteration fused NB attack on the golden
NB rooms.  Sparse against dense: the input gradients agree to 1e-5 of their largest magnitude with >= 99.9 % equal signs (the
dense layer adds two k-products per MFMA step, the stream one per fmaf, so the bits may differ); two sparse children are
byte-identical, gradients and attack outputs alike.
CPU: the sparse instantiations in hipcc's device assembly run without scratch, at 5 waves per SIMD like the dense ones they
replace, and the asm-boundary hazard lint finds nothing in them."""
import os
import re
import shutil
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
SPARSE = [r"sa_bwd_sparse_kernelILi64ELi4ELi2ELi1E", r"sa_bwd_sparse_kernelILi32ELi4ELi2ELi2E",
          r"sa_bwd_sparse_kernelILi32ELi8ELi2ELi4E"]

needs_hipcc = pytest.mark.skipif(shutil.which("hipcc") is None and not os.path.exists("/opt/rocm/bin/hipcc"),
                                 reason="needs hipcc")


def _child_main(out_path):
    import torch
    sys.path.insert(0, ROOT)
    from pointsecguard_amd import _lib, runtime

    def dev(a, dt=None):
        t = torch.from_numpy(np.ascontiguousarray(a))
        return (t.to(dt) if dt is not None else t).cuda().contiguous()

    model = runtime.PN2Model(runtime.fold_state_dict(dict(np.load(os.path.join(GOLDEN, "pn2_weights.npz")))))
    g = dict(np.load(os.path.join(GOLDEN, "pn2_room.npz")))
    ws = runtime.PN2Workspace(1, 4096, 2)
    x0 = dev(g["room"][None])
    ws.plan_build(x0, dev(g["starts"].reshape(1, 4, 1), torch.int32), 1)
    logp = ws.forward(model, 0, x0)
    labels = dev(g["labels"].astype(np.int32)[None])
    dlogp = torch.empty_like(logp)
    _lib.call("psg_ce_logp_grad", runtime.ptr(logp), runtime.ptr(labels), 0, 4096, 4096, 13, 1.0 / 4096,
              runtime.ptr(dlogp), None, runtime.stream())
    dx0 = ws.backward(model, 0, dlogp)
    nb = dict(np.load(os.path.join(GOLDEN, "pn2_nb.npz")))
    rooms, iters = nb["rooms"], 40
    images = dev(np.ascontiguousarray(rooms.transpose(0, 2, 1)))
    wsn = runtime.PN2Workspace(rooms.shape[0], 4096, iters)
    adv = wsn.nb_attack(model, images, dev(nb["labels"].astype(np.int32)), dev(nb["starts"][1:1 + iters], torch.int32),
                        float(nb["eps"]), float(nb["alpha"]), iters)
    torch.cuda.synchronize()
    np.savez(out_path, dx0=dx0.cpu().numpy(), adv=adv.cpu().numpy())


def _child(tmp_path, tag, value):
    env = dict(os.environ)
    env["PSG_PN2_POOLT_SPARSE"] = value
    out = str(tmp_path / ("%s.npz" % tag))
    r = subprocess.run([sys.executable, os.path.abspath(__file__), out], env=env, cwd=ROOT, capture_output=True, text=True,
                       timeout=600)
    assert r.returncode == 0, (r.stdout + r.stderr)[-3000:]
    return dict(np.load(out))


@pytest.mark.gpu
def test_sparse_matches_dense_and_is_deterministic(tmp_path):
    dense = _child(tmp_path, "dense", "0")
    sp1 = _child(tmp_path, "sparse1", "1")
    sp2 = _child(tmp_path, "sparse2", "1")
    for k in ("dx0", "adv"):
        assert sp1[k].tobytes() == sp2[k].tobytes(), k
    a, b = sp1["dx0"], dense["dx0"]
    scale = np.abs(b).max()
    assert scale > 0
    assert np.abs(a - b).max() <= 1e-5 * scale, np.abs(a - b).max() / scale
    nz = (a != 0) | (b != 0)
    assert (np.sign(a[nz]) == np.sign(b[nz])).mean() >= 0.999


def _asm(out_dir):
    csrc = os.path.join(ROOT, "pointsecguard_amd", "csrc")
    cmd = subprocess.run(["make", "-n", "-B", "psg_pn2.o"], cwd=csrc, capture_output=True, text=True, check=True).stdout
    line = next(l for l in cmd.splitlines() if "hipcc" in l and " -c " in l)
    out = os.path.join(out_dir, "psg_pn2.s")
    line = line.replace(" -c ", " -S --cuda-device-only -c ").replace("-o psg_pn2.o", "-o " + out)
    subprocess.run(line, shell=True, cwd=csrc, check=True, capture_output=True)
    return out


@needs_hipcc
def test_sparse_instantiations(tmp_path):
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import check_asm_hazards
    import mlp_asm_table
    path = _asm(str(tmp_path))
    table = mlp_asm_table.scan(path, "sa_bwd_(sparse_)?kernel")
    dense_occ = min(r["occ"] for n, r in table.items() if "sparse" not in n)
    for pat in SPARSE:
        names = [n for n in table if re.search(pat, n)]
        assert names, pat
        for n in names:
            assert table[n]["scratch"] == 0, "%s: scratch %d bytes" % (n, table[n]["scratch"])
            assert table[n]["occ"] >= dense_occ, "%s: %d waves per SIMD" % (n, table[n]["occ"])
            assert table[n]["vgpr"] <= 96, "%s: %d VGPRs" % (n, table[n]["vgpr"])
    bad = check_asm_hazards.scan(path)
    assert not bad, bad[:5]


if __name__ == "__main__":
    _child_main(sys.argv[1])
