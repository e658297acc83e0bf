"""The opt-in alternative kernels keep the same parity bars as the default ones.

  PSG_FP1_WAVE=1     wave-private fp1 + head chain (psg_chain.cuh) instead of the workgroup-cooperative kernels
  PSG_RLA_ATOMICS=1  RandLA-Net backward scatters with float atomics instead of the inverse-list gathers
  PSG_RLA_NO_FUSE16=1  RandLA-Net level 0: the unfused gather / score GEMM / softmax chain instead of lfa16_fwd / _bwd_kernel
  PSG_RLA_NO_SPLIT=1   RandLA-Net levels 1-4: gather + per-edge score GEMM instead of att_pool_split_fwd / _bwd_kernel
  PSG_RLA_NO_DIRECT=1  RandLA-Net: the narrow layers (<= 64 output channels) on the LDS-tiled GEMM / the row-per-thread vector
                     kernel (rounds 1-4) instead of the barrier-free direct MFMA kernel (round 5)
  PSG_GCN_PQ_FUSION=1  ResGCN: a block's edge pass also computes the next block's per-vertex [P | Q] product
  PSG_PN2_SPLIT=0    PointNet++ SSG: whole first layers at SA levels 1-3 (rounds 1-4) instead of the split per-point product +
                     per-row xyz chunk (round 5)
  PSG_PN2_FPSPLIT=0  PointNet++: whole first layers in fp1 - fp3 instead of the interpolated-part product per coarse point inside
                     the coarser module's kernels (round 5)
  PSG_PN2_L1T_COLOUR=0  PointNet++ attack loop: the first SA layer's transpose on the matrix pipe (rounds 1-4) instead of its three
                     colour columns on the vector pipe (round 5)
  PSG_PN2_PGD_FUSE=0  PointNet++ attack loop: the PGD step as a launch of its own behind the gradient's last gather (rounds 1-4)
  PSG_GCN_EDGE_BWD=atomic  ResGCN: the EdgeConv max-pass backward scatters with float atomics (rounds 1-3) instead of the
                     inverse-graph gather
  PSG_GEMM_SMALL_BELOW=0  every GEMM on its wide workgroup tiles (<2,2>, <4,1>) instead of 64 x 64 tiles for small grids: the
                     tile shape must not change the k order, so where the launch sites coincide with the default's the results
                     must be bit-equal (the stage tests print a hash of logits and, for conv = edge, dx0)

The switches are read once per process, so each case runs the relevant parity tests in ONE child interpreter with the
switch set and the launch tracer on (PSG_TRACE_SYNC=1 prints the site of every launch - the source line where the launch is
written, or, for a launch helper, its CALLER's line with an optional #variant; the child runs with -s so the library's
stderr reaches this process): the child must pass, and
its set of launch sites must differ from the default child's - the switch really selected other kernels."""
import os
import re
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def child(test_file, keyword, extra_env):
    env = dict(os.environ)
    env.pop("PSG_FP1_WAVE", None)
    env.pop("PSG_RLA_ATOMICS", None)
    env.pop("PSG_GCN_PQ_FUSION", None)
    env.pop("PSG_GCN_EDGE_BWD", None)
    env.pop("PSG_GEMM_SMALL_BELOW", None)
    env.pop("PSG_PN2_SPLIT", None)
    env.pop("PSG_RLA_NO_DIRECT", None)
    env.pop("PSG_RLA_NO_FUSE16", None)
    env.pop("PSG_RLA_NO_SPLIT", None)
    env.pop("PSG_PN2_FPSPLIT", None)
    env.pop("PSG_PN2_L1T_COLOUR", None)
    env.pop("PSG_PN2_PGD_FUSE", None)
    env.update(extra_env)
    env["PSG_TRACE_SYNC"] = "1"
    out = subprocess.run([sys.executable, "-m", "pytest", os.path.join(ROOT, "tests", test_file), "-x", "-q", "-m", "gpu",
                          "-k", keyword, "-s", "-p", "no:cacheprovider"], env=env, cwd=ROOT, capture_output=True, text=True,
                         timeout=900)
    sites = set(re.findall(r"\[psg trace\] launch \d+ at (\S+) issued", out.stderr + out.stdout))
    return out, sites


_BASE = {}


@pytest.mark.parametrize("test_file,keyword,switch", [
    ("test_gpu_parity.py", "forward_vs_reference or backward_vs_reference or forward_backward_vs_oracle_batch", "PSG_FP1_WAVE"),
    ("test_randla_net.py", "forward_backward_vs_oracle or bim_attack_vs_oracle", "PSG_RLA_ATOMICS"),
    ("test_randla_net.py", "forward_backward_vs_oracle or bim_attack_vs_oracle", "PSG_RLA_NO_DIRECT"),
    # the stage-by-stage float64 checks (ragged 8704-point cloud: every row count off its tile) on each RandLA path
    ("test_randla_stages.py", "(forward_stages or backward_stages) and n8704", "PSG_RLA_NO_FUSE16"),
    ("test_randla_stages.py", "(forward_stages or backward_stages) and n8704", "PSG_RLA_NO_SPLIT"),
    ("test_randla_stages.py", "(forward_stages or backward_stages) and n8704", "PSG_RLA_ATOMICS"),
    ("test_randla_stages.py", "(forward_stages or backward_stages) and n8704", "PSG_RLA_NO_DIRECT"),
    ("test_gpu_resgcn28.py", "not knn_on_reference_features", "PSG_GCN_PQ_FUSION"),
    ("test_gpu_resgcn.py", "forward_backward or nb_attack", "PSG_GCN_EDGE_BWD=atomic"),
    # the ResGCN stage-by-stage float64 checks at ragged, multi-room shapes (288 and 400 rows, all six configurations)
    ("test_gpu_gcn_stages.py", "every_stage and (b3n96 or b2n200)", "PSG_GCN_PQ_FUSION"),
    ("test_gpu_gcn_stages.py", "every_stage and (b3n96 or b2n200)", "PSG_GCN_EDGE_BWD=atomic"),
    ("test_gpu_gcn_stages.py", "every_stage and (b3n96 or b2n200)", "PSG_GEMM_SMALL_BELOW=0"),
    ("test_gpu_parity.py", "forward_vs_reference or backward_vs_reference or forward_backward_vs_oracle_batch or nb_attack_steps_vs_reference",
     "PSG_PN2_SPLIT=0"),
    ("test_gpu_parity.py", "forward_vs_reference or backward_vs_reference or forward_backward_vs_oracle_batch or nb_attack_steps_vs_reference",
     "PSG_PN2_FPSPLIT=0"),
    ("test_gpu_msg.py", "forward_vs_reference or backward_vs_reference", "PSG_PN2_FPSPLIT=0"),
    # (round 6: the "timed" parametrisations of the step tests and the fused first-iterations test are the ones that run the
    # colour-only backward / the fused call, i.e. the tests in which these two switches act; round 5 pointed them at the
    # general entry points, where PSG_PN2_L1T_COLOUR cannot act)
    ("test_gpu_parity.py", "(nb_attack_steps_vs_reference or tar_nb_attack_steps or nb_b8_steps) and timed or fused_nb_attack_first_iterations",
     "PSG_PN2_L1T_COLOUR=0"),
    ("test_gpu_parity.py", "fused_nb_attack_first_iterations or nb_attack_free_run_vs_reference or nb_b8_statistical_parity",
     "PSG_PN2_PGD_FUSE=0"),
])
def test_switch_selects_other_kernels_with_the_same_parity(test_file, keyword, switch):
    if (test_file, keyword) not in _BASE:                       # the default child of a (file, keyword) runs once
        _BASE[test_file, keyword] = child(test_file, keyword, {})
    base, base_sites = _BASE[test_file, keyword]
    assert base.returncode == 0, base.stdout[-3000:]
    name, _, value = switch.partition("=")
    alt, alt_sites = child(test_file, keyword, {name: value or "1"})
    assert alt.returncode == 0, alt.stdout[-3000:]
    assert " passed" in alt.stdout and "skipped" not in alt.stdout.splitlines()[-1]
    if name == "PSG_GEMM_SMALL_BELOW" and base_sites and alt_sites == base_sites:
        # the same launch sites with other tile shapes: the k order is the same, so the results are bit-equal
        hashes = [re.findall(r"hash (\S+ \S+ [0-9a-f]{16})", o.stdout) for o in (base, alt)]
        print("\n".join(hashes[1]))
        assert len(hashes[0]) >= 12 and hashes[0] == hashes[1], (hashes[0], hashes[1])
        return
    assert base_sites and alt_sites and alt_sites != base_sites, (switch, sorted(alt_sites ^ base_sites))


@pytest.mark.parametrize("arch", ["ssg", "msg"])
def test_traced_forward_backward_completes(arch):
    """Round 5's stale wave-uniform trip count (a v_readfirstlane one instruction behind the VALU write of its source, inside
    inline assembly: the k-loop ran off its weights, a memory fault) was found with the launch tracer: one plan + forward +
    backward with a synchronisation and an error check after every launch (tools/fp_split_probe.py).  Pinned here so that
    one run shows a regression of that class launch by launch (round-5 advisor); the static side of the same class is
    tools/check_asm_hazards.py over the compiler's assembly."""
    env = dict(os.environ)
    env["PSG_TRACE_SYNC"] = "1"
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "fp_split_probe.py"), arch], env=env, cwd=ROOT,
                         capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, (out.stdout + out.stderr)[-3000:]
    assert "forward ok" in out.stdout and "backward ok" in out.stdout
    issued = re.findall(r"\[psg trace\] launch (\d+) at (\S+) issued", out.stderr + out.stdout)
    assert len(issued) >= 40, len(issued)


def test_knn_prefilter_with_two_sample_tiles_per_wave():
    """PSG_KNN_SAMPLE2_KK: the prefilter kernel's second sample tile per wave (rows of 1.45 KK instead of 1.7 KK entries) was
    the default from KK = 311 in rounds 4-5 and starts at KK = 430 since round 6 (psg_knn.hip: one tile is faster once the
    finalists no longer limit the rows), i.e. no dilation of the 28-block network takes it by default any more.  The path
    stays a switch and keeps its parity: the kNN tests that reach d >= 21 run in a child with the round-5 setting."""
    out, _ = child("test_gpu_knn_bf16.py", "default_split or adversarial or spatially_sorted", {"PSG_KNN_SAMPLE2_KK": "311"})
    assert out.returncode == 0, out.stdout[-3000:]
    assert " passed" in out.stdout and "skipped" not in out.stdout.splitlines()[-1]
