"""CPU side of the PointNet NU windows: the new entry points are declared, bound and exported, and hipcc's gfx950 device
assembly of the two new kernels (pn_nu_head_kernel in psg_pointnet.hip, nu_restart_rooms_kernel in psg_attack.hip) runs
without scratch and passes the asm-boundary hazard lint.  hipcc cross-compiles without a GPU; ~40 s."""
import os
import re
import shutil
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "pointsecguard_amd", "csrc")
NEW = ("psg_pointnet_nu_window", "psg_pointnet_nu_head", "psg_nu_restart_rooms")

needs_hipcc = pytest.mark.skipif(shutil.which("hipcc") is None and not os.path.exists("/opt/rocm/bin/hipcc"), reason="needs hipcc")


def test_new_symbols_are_declared_bound_and_exported():
    from pointsecguard_amd import _lib
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "psg.h")).read(), flags=re.S)
    exported = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    for name in NEW:
        assert re.search(r"\b%s\s*\(" % name, header), name
        assert name in _lib.SIGNATURES, name
        assert re.search(r" T %s$" % name, exported, flags=re.M), name
    # the ctypes struct mirrors the header's field order
    body = re.search(r"typedef struct psg_pointnet_nu_window_args \{(.*?)\} psg_pointnet_nu_window_args;", header, flags=re.S).group(1)
    fields = []
    for decl in body.split(";"):
        decl = decl.strip()
        if decl:
            fields += [f.strip().lstrip("*") for f in re.sub(r"^(const\s+)?\w+\s+", "", decl).split(",")]
    assert fields == [n for n, _ in _lib.PointnetNuWindowArgs._fields_]


def _asm_of(unit, out_dir):
    cmd = subprocess.run(["make", "-n", "-B", unit + ".o"], cwd=CSRC, capture_output=True, text=True, check=True).stdout
    line = next(l for l in cmd.splitlines() if "hipcc" in l and " -c " in l)
    out = os.path.join(out_dir, unit + ".s")
    line = line.replace(" -c ", " -S --cuda-device-only -c ").replace("-o %s.o" % unit, "-o " + out)
    subprocess.run(line, shell=True, cwd=CSRC, check=True, capture_output=True)
    return out


@needs_hipcc
@pytest.mark.parametrize("unit,kernel", [("psg_pointnet", "pn_nu_head_kernel"), ("psg_attack", "nu_restart_rooms_kernel")])
def test_new_kernels_use_no_scratch_and_pass_the_hazard_lint(tmp_path, unit, kernel):
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import check_asm_hazards
    path = _asm_of(unit, str(tmp_path))
    text = open(path).read()
    m = re.search(r"^(_Z\w*%s\w*):.*?^\s*s_endpgm.*?; ScratchSize: (\d+)" % kernel, text, flags=re.S | re.M)
    assert m, kernel
    assert int(m.group(2)) == 0
    body = m.group(0)
    assert not re.search(r"\bscratch_(load|store)", body)
    assert "ASMSTART" not in body                          # no inline assembly in the new kernels
    desc = re.search(r"\.amdhsa_kernel %s\n(.*?)\.end_amdhsa_kernel" % re.escape(m.group(1)), text, flags=re.S).group(1)
    assert re.search(r"\.amdhsa_private_segment_fixed_size 0\b", desc)
    assert check_asm_hazards.scan(path) == []
