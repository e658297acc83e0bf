"""Static side of the FPS step loop (psg_geometry.hip): hipcc's device assembly of the geometry unit through
tools/fps_isa_count.py.  The loop is vector-issue-bound at the benchmark's problem count, so its vector-instruction count is
what the kernel costs: every instantiation stays at or below the count it had before the bookkeeping was rewritten (unsigned
min on the distance bits, no padding guard, keys-only arg-max with a scalar pick, one-instruction DPP stages), 256 x 16 at
or below 0.70 of it, nothing spills, every DPP stage of the reductions is one v_max_u32_dpp, and the unit has no finding of
the asm-boundary hazard lint.  CPU test: hipcc cross-compiles gfx950 without a GPU; ~15 s."""
import os
import re
import shutil
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

pytestmark = pytest.mark.skipif(shutil.which("hipcc") is None and not os.path.exists("/opt/rocm/bin/hipcc"), reason="needs hipcc")

# vector-ALU instructions of the step loop before the rewrite (the same tool on the parent's source), by (threads, points)
BEFORE = {(64, 1): 35, (64, 4): 61, (256, 4): 79, (1024, 4): 79, (512, 8): 119, (1024, 8): 119, (256, 16): 199}


@pytest.fixture(scope="module")
def listing():
    import fps_isa_count
    asm = fps_isa_count.compile_asm(os.path.join(fps_isa_count.CSRC, "psg_geometry.hip"))
    yield asm, fps_isa_count.table(asm)
    os.remove(asm)


def test_step_loops_issue_fewer_vector_instructions(listing):
    _, rows = listing
    seen = set()
    for name, c, vgpr, scratch in rows:
        nt, ppt = map(int, re.match(r"fps_kernel<(\d+), (\d+)", name).groups())
        seen.add((nt, ppt))
        assert c is not None, name
        print(name, c, vgpr, scratch)
        assert c["valu"] <= BEFORE[(nt, ppt)], (name, c)
        assert scratch == 0 and vgpr <= 128, (name, vgpr, scratch)
        if (nt, ppt) == (256, 16):
            assert c["valu"] <= 0.70 * BEFORE[(256, 16)], (name, c)
    assert seen == set(BEFORE)


def test_dpp_stages_fold_and_the_unit_passes_the_hazard_lint(listing):
    import check_asm_hazards
    import fps_isa_count
    asm, _ = listing
    body, _ = fps_isa_count.functions(asm)
    for name, lines in body.items():
        ops = [l.split(";")[0].split()[0] for l in lines if l.split(";")[0].strip() and not l.split(";")[0].strip().endswith(":")]
        waves = int(re.search(r"fps_kernelILi(\d+)E", name).group(1)) // 64
        assert ops.count("v_max_u32_dpp") == (6 if waves == 1 else 10), name      # wave max: 6 stages; + 4 over the wave partials
        assert "v_mov_b32_dpp" not in ops, name
    assert check_asm_hazards.scan(asm) == []
