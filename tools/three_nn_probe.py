"""GPU box: time psg_three_nn per launch, scan kernel against grid kernel (PSG_THREE_NN=scan | grid, one fresh child process
each: the switch is read once per process), at the plan's shapes (N, S) = (4096, 1024), (1024, 256), (256, 64) for 2560, 320
and 8 problems, on synthetic rooms with FPS-sampled coarse points (level 0 shares the rooms' clouds, as in a plan):
    python tools/three_nn_probe.py
HIP events around 10 launches after 2 warm-up launches, three repetitions per row (all three are printed)."""
import os, subprocess, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def child():
    import numpy as np, torch
    sys.path.insert(0, ROOT)
    from pointsecguard_amd import _lib, runtime
    from pointsecguard_amd.synthetic import make_rooms
    mode = os.environ["PSG_THREE_NN"]
    ctx = runtime.context(torch.device("cuda:0"))
    for P in (2560, 320, 8):
        B = min(64, P)
        cur = torch.from_numpy(np.ascontiguousarray(make_rooms(B, 5)[:, :, :3])).cuda()
        rng = np.random.default_rng(0)
        for n, s in ((4096, 1024), (1024, 256), (256, 64)):
            ncl = cur.shape[0]
            full = cur if ncl == P else cur.repeat(P // ncl, 1, 1)
            start = torch.from_numpy(rng.integers(0, n, P).astype(np.int32)).cuda()
            new = runtime.gather_points(full, runtime.fps(full, s, start))
            del full
            idx = torch.empty(P, n, 3, dtype=torch.int32, device="cuda")
            w = torch.empty(P, n, 3, dtype=torch.float32, device="cuda")
            def call():
                _lib.call("psg_three_nn", ctx, runtime.ptr(cur), ncl, runtime.ptr(new), P, n, s, runtime.ptr(idx), runtime.ptr(w), runtime.stream())
            call(); call(); torch.cuda.synchronize()
            ms = []
            for _ in range(3):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(10): call()
                e1.record(); torch.cuda.synchronize()
                ms.append(e0.elapsed_time(e1) / 10)
            print("%-4s P=%4d N=%4d S=%4d: %s ms per launch (checksum %d)" % (mode, P, n, s, " ".join("%.4f" % m for m in ms), int(idx.sum())), flush=True)
            cur = new


if __name__ == "__main__":
    if len(sys.argv) > 1 and sys.argv[1] == "--child":
        child()
    else:
        for mode in ("scan", "grid"):
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child"], env=dict(os.environ, PSG_THREE_NN=mode), timeout=240)
            if r.returncode != 0:
                sys.exit("three_nn_probe: the %s child ended with status %d" % (mode, r.returncode))
