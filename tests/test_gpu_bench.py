"""bench.py without --full: one headline line, and --dump-outputs writes what the last timed step returned."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.gpu
def test_plain_bench_line_and_dumped_outputs(tmp_path):
    from pointsecguard_amd.synthetic import make_rooms
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_PORT")}
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1",
                        "--dump-outputs", str(tmp_path)], env=env, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-3000:]
    line = json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][-1])
    assert line["steps"] == 3 and line["unit"] == "rooms/s" and line["higher_is_better"] is True and line["dtype"] == "f32"
    assert line["value"] > 0 and abs(line["value"] * line["ms_per_step"] - 8e3) <= 1e-6 * 8e3     # 8 rooms per step
    assert not {"roofline", "cpu_baseline", "secondary", "parity"} & set(line)                       # --full's parts
    adv = np.load(tmp_path / "adv_images.npy")
    assert adv.dtype == np.float32 and adv.shape == (8, 9, 4096)
    # --steps 3 --warmup 1: one warm-up and one timed launch of 3 steps; the timed one attacks make_rooms(24, 1001), and its
    # last step is the last 8 rooms.  The attack moves colour only, by at most eps + alpha (the un-projected last step).
    clean = make_rooms(24, 1001)[-8:].transpose(0, 2, 1)
    assert np.array_equal(adv[:, :3], clean[:, :3]) and np.array_equal(adv[:, 6:], clean[:, 6:])
    moved = np.abs(adv[:, 3:6] - clean[:, 3:6])
    assert moved.max() <= 0.05 + 2 / 255 + 1e-6 and moved.mean() > 0.01
