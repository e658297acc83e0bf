"""GPU box: level-0 ball query of psg_pn2_plan_build per plan size, direct route (PSG_PN2_BALL_TABLE=0) or table route for
every plan (=2): python tools/ball_table_probe.py ROOMS [n_forward ...]   (default 1 4 8 10 40; SSG, N = 4096)

Prints the ball-query tag of psg_pn2_prof_read per plan (HIP events: every level's query, the table build and expansion, and
the inverse group lists); run under `rocprofv3 --kernel-trace` the launches are told apart by grid
(tools/kernel_trace_by_grid.py): ball_query_grid_kernel 1 x (n_forward * ROOMS) is the direct level-0 query, 4 x ROOMS the
table build, group_from_table_kernel 32 * n_forward * ROOMS workgroups the expansion."""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from pointsecguard_amd import runtime
from pointsecguard_amd.synthetic import make_rooms

B = int(sys.argv[1])
plans = [int(a) for a in sys.argv[2:]] or [1, 4, 8, 10, 40]
REPS = 3
x0 = torch.from_numpy(make_rooms(B, 5)).cuda()
rng = np.random.default_rng(0)
ws = runtime.PN2Workspace(B, 4096, max(plans))
for nf in plans:
    starts = torch.from_numpy(np.stack([rng.integers(0, n, (nf, B)) for n in (4096, 1024, 256, 64)], axis=1).astype(np.int32)).cuda()
    ws.plan_build(x0, starts, nf)
    torch.cuda.synchronize()
    ws.prof_enable(True)
    for _ in range(REPS):
        ws.plan_build(x0, starts, nf)
    torch.cuda.synchronize()
    ms, cnt = ws.prof_read()["ball_query"]
    ws.prof_enable(False)
    print("PSG_PN2_BALL_TABLE=%s rooms=%d n_forward=%d: ball_query tag %.3f ms per plan (%d launches)" % (
        os.environ.get("PSG_PN2_BALL_TABLE", "default"), B, nf, ms / REPS, cnt // REPS), flush=True)
