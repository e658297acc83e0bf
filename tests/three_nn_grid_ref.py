"""A numpy float32 restatement of the grid 3-NN (three_nn_grid_kernel, psg_geometry.hip): the uniform grid over the coarse
cloud, the shell walk of one query, the stop rule with its error term, and the (d, j) candidate order - next to the plain
scan it has to equal.  The squared distances themselves are an INPUT (the [N, S] matrix of the oracle's square_distance,
which is the kernels' expansion with its fused multiply-adds: numpy has no fma), so what is restated here is only what the
grid adds: which candidates a query looks at, in which order it ranks them, and when it stops.

The three switches turn the walk into the mutants the host test has to tell apart from the real thing:
    stop_ge   stop when L^2 - err >= third best (a tie with a lower j in the next shell is skipped)
    zero_err  err = 0 (the rounding of the expansion is ignored: wrong far from the origin)
    d_only    candidates ranked by d alone, first met stays (the grid meets them in cell order, not in j order)
"""
import numpy as np

F = np.float32
PPC = F(2.0)         # coarse points per cell the edge aims at (NNG_PPC)
MAX_CELLS = 1024      # NNG_CELLS
ERR_REL = F(1e-5)     # expansion rounding: below 3e-6 max|coordinate|^2, taken as 1e-5 (the ball grid's factor)
SLACK_REL = F(4e-6)   # rounding of the cell index and of the face position, relative to max|coordinate|


def scan_three_nn(d):
    """The scan: candidates j = 0 .. S-1 in order, strict `<` against the best three, slots start as (inf, 0).
    d: [N, S] float32.  Returns idx [N, 3] int32, dist [N, 3] float32."""
    n, s = d.shape
    with np.errstate(invalid="ignore"):
        eff = np.where(d < np.inf, d, np.inf).astype(F)          # NaN and +inf never pass `d < best`
    order = np.argsort(eff, axis=1, kind="stable")[:, :3]         # ascending d, ties by ascending j
    dist = np.take_along_axis(eff, order, axis=1)
    idx = np.where(dist < np.inf, order, 0).astype(np.int32)
    return idx, dist


class Grid:
    """The grid of one coarse cloud [S, 3] (float32 arithmetic throughout)."""

    def __init__(self, coarse, ppc=PPC, max_cells=MAX_CELLS):
        c = np.ascontiguousarray(coarse, dtype=F)
        self.S = c.shape[0]
        self.finite = bool(np.all(np.abs(c) < F(1e18)))           # false for NaN and infinities
        if not self.finite:
            return
        self.lo, self.hi = c.min(axis=0), c.max(axis=0)
        self.maxabs = F(max(np.abs(self.lo).max(), np.abs(self.hi).max()))
        ext = (self.hi - self.lo).astype(F)
        emax = F(ext.max())
        if emax > 0:
            e = np.maximum(ext, emax * F(1.0 / 64.0))
            edge = F(np.cbrt(F(F(F(e[0] * e[1]) * e[2]) * F(ppc / F(self.S)))))
            while True:
                dim = (ext / edge).astype(np.int64) + 1
                if dim.prod() <= max_cells:
                    break
                edge = F(edge * F(1.25))
        else:
            edge, dim = F(1.0), np.ones(3, np.int64)
        self.edge, self.inv, self.dim = edge, F(F(1.0) / edge), dim
        cell = self.cells(c)
        lin = (cell[:, 2] * dim[1] + cell[:, 1]) * dim[0] + cell[:, 0]
        self.sorted = np.argsort(lin, kind="stable")              # (the kernel's order inside a cell is arbitrary)
        self.start = np.searchsorted(lin[self.sorted], np.arange(dim.prod() + 1))
        self.span = F(F(dim.max()) * edge)

    def cells(self, pts):
        t = ((pts - self.lo).astype(F) * self.inv).astype(F)
        t = np.fmin(np.fmax(t, F(0)), (self.dim - 1).astype(F))   # clamped in float (NaN -> 0), then truncated
        return t.astype(np.int64)

    def face(self, axis, m):
        return F(self.lo[axis] + F(F(m) * self.edge))


def walk(grid, q, drow, stop_ge=False, zero_err=False, d_only=False, order=None, box=None):
    """One query q [3] against the grid; drow [S] are its squared distances.  Returns (idx [3], dist [3], visited, shells);
    shells = 0 for the fallback (all S candidates in ascending j through the scan's compare chain)."""
    best_d, best_j = [F(np.inf)] * 3, [0, 0, 0]

    def insert(d, j):
        def before(k):
            return d < best_d[k] or (not d_only and d == best_d[k] and j < best_j[k])
        if before(2):
            if before(1):
                best_d[2], best_j[2] = best_d[1], best_j[1]
                if before(0):
                    best_d[1], best_j[1] = best_d[0], best_j[0]
                    best_d[0], best_j[0] = d, j
                else:
                    best_d[1], best_j[1] = d, j
            else:
                best_d[2], best_j[2] = d, j

    q = np.asarray(q, dtype=F)
    if is_far(grid, q):                   # (a NaN coordinate is far)
        for j in range(grid.S):
            if drow[j] < best_d[2]:
                insert(drow[j], j)            # in ascending j the key order and the strict chain are the same thing
        return np.array(best_j, np.int32), np.array(best_d, F), grid.S, 0
    maxabs = F(max(grid.maxabs, np.abs(q).max()))
    err = F(0) if zero_err else F(ERR_REL * F(maxabs * maxabs))
    slack = F(SLACK_REL * maxabs)
    c = grid.cells(q[None])[0]
    nx, ny, nz = (int(v) for v in grid.dim)
    visited = 0

    def run(z, y, x0, x1):
        nonlocal visited
        x0, x1 = max(x0, 0), min(x1, nx - 1)
        if x0 > x1:
            return
        lin = (z * ny + y) * nx
        members = grid.sorted[grid.start[lin + x0]:grid.start[lin + x1 + 1]]
        if order is not None:
            members = order(members)
        for j in members:
            insert(drow[j], int(j))
        visited += len(members)

    def done(k):
        L = F(np.inf)                         # distance to the nearest face of what has not been visited (box borders: nothing beyond)
        for a in range(3):
            if c[a] - k > 0:
                L = min(L, F(q[a] - grid.face(a, c[a] - k)))
            if c[a] + k < grid.dim[a] - 1:
                L = min(L, F(grid.face(a, c[a] + k + 1) - q[a]))
        if L == np.inf:
            return True
        Ls = F(L - slack)
        if Ls > 0:
            bound = F(F(Ls * Ls) - err)
            return bool(bound >= best_d[2]) if stop_ge else bool(bound > best_d[2])
        return False

    if box is not None:
        # the kernel's first step: every cell of a box that holds this query's own 3 x 3 x 3 block (the box around the blocks
        # of the 64 queries its wave serves); if that is not enough the lane starts over and walks by itself
        lo, hi = box
        assert all(lo[a] <= max(c[a] - 1, 0) and hi[a] >= min(c[a] + 1, grid.dim[a] - 1) for a in range(3))
        for z in range(lo[2], hi[2] + 1):
            for y in range(lo[1], hi[1] + 1):
                run(z, y, lo[0], hi[0])
        if done(1):
            return np.array(best_j, np.int32), np.array(best_d, F), visited, 1
        best_d[:], best_j[:] = [F(np.inf)] * 3, [0, 0, 0]
    k = 1
    while True:
        for z in range(max(c[2] - k, 0), min(c[2] + k, nz - 1) + 1):
            for y in range(max(c[1] - k, 0), min(c[1] + k, ny - 1) + 1):
                if k == 1 or abs(z - c[2]) == k or abs(y - c[1]) == k:
                    run(z, y, c[0] - k, c[0] + k)
                else:
                    run(z, y, c[0] - k, c[0] - k)
                    run(z, y, c[0] + k, c[0] + k)
        if done(k):
            break
        k += 1
    return np.array(best_j, np.int32), np.array(best_d, F), visited, k


def is_far(grid, q):
    if not grid.finite:
        return True
    with np.errstate(invalid="ignore"):
        return not bool(np.all((q >= grid.lo - grid.span) & (q <= grid.hi + grid.span)))


def grid_three_nn(fine, coarse, d, waves=False, **kw):
    """All queries of one problem.  Returns idx [N, 3], dist [N, 3], visited [N], shells [N].  waves=True is the kernel's
    schedule: queries in cell order, 64 to a wave, a wave's box first (walk: box)."""
    g = Grid(coarse)
    n = len(fine)
    boxes = [None] * n
    if waves and g.finite:
        qc = g.cells(fine)
        order = np.argsort((qc[:, 2] * g.dim[1] + qc[:, 1]) * g.dim[0] + qc[:, 0], kind="stable")
        for w in range(0, n, 64):
            members = [i for i in order[w:w + 64] if not is_far(g, fine[i])]
            if members:
                lo = np.maximum(qc[members].min(axis=0) - 1, 0)
                hi = np.minimum(qc[members].max(axis=0) + 1, g.dim - 1)
                for i in members:
                    boxes[i] = (lo, hi)
    out = [walk(g, fine[i], d[i], box=boxes[i], **kw) for i in range(n)]
    return (np.stack([o[0] for o in out]), np.stack([o[1] for o in out]), np.array([o[2] for o in out]),
            np.array([o[3] for o in out]))


# ---------------------------------------------------------------------------------------------------------------------
# The inputs both test files use: name -> (fine [N, 3], coarse [S, 3]), the smallest at which the walk can still go wrong.
# ---------------------------------------------------------------------------------------------------------------------
def lattice_tie_case():
    """Coarse points on a 1/16 lattice, queries on the half lattice (all coordinates dyadic: the expansion is exact, so equal
    true distances are equal computed distances).  Query 0 is one whose third-best distance is shared by a point OUTSIDE its
    3 x 3 x 3 block of cells; that point is then given j = 0, the lowest index of the tie: a walk that stops after the block,
    or ranks by d alone, returns another index.  Returns (fine, coarse, block) with block = mask [S] of the coarse points in
    query 0's first block."""
    for seed in range(1000):
        rng = np.random.default_rng(seed)
        sites = rng.choice(16 ** 3, 160, replace=False)
        coarse = (np.stack([sites % 16, sites // 16 % 16, sites // 256], axis=1).astype(F) / F(16)).astype(F)
        fine = ((2 * rng.integers(0, 16, (64, 3)) + 1).astype(F) / F(32)).astype(F)
        g = Grid(coarse)
        cc = g.cells(coarse)
        for i in range(len(fine)):
            diff = (coarse - fine[i]).astype(F)
            d = (diff * diff).sum(axis=1, dtype=F)                   # exact on these coordinates
            block = (np.abs(cc - g.cells(fine[i][None])[0]) <= 1).all(axis=1)
            third = np.sort(d)[2]
            out = np.nonzero((d == third) & ~block)[0]
            if len(out) and (d[block] == third).any() and (d < third).sum() <= 2:
                j = out[0]
                coarse[[0, j]] = coarse[[j, 0]]
                block[[0, j]] = block[[j, 0]]
                fine[[0, i]] = fine[[i, 0]]
                return fine, coarse, block
    raise AssertionError("no lattice with a tie across the first block found")


def cases():
    rng = np.random.default_rng(29)
    out = {}
    u = lambda n, scale=1.0: (rng.random((n, 3), dtype=F) * F(scale)).astype(F)
    out["min"] = (u(1), u(3))                                            # S = 3, N = 1: one cell, minimum S
    out["ragged"] = (u(257), u(5))                                       # ragged against 64 and 256
    out["identical"] = (u(64), np.tile(u(1), (8, 1)))                    # every d ties: j = 0, 1, 2
    corners = np.array([[x, y, z] for z in (0, 1) for y in (0, 1) for x in (0, 1)], F)[[5, 2, 7, 0, 3, 6, 1, 4]]
    out["cube"] = (np.concatenate([np.full((1, 3), 0.5, F), u(4)]), corners)   # ties met out of j order
    lt = lattice_tie_case()
    out["lattice_tie"] = (lt[0], lt[1])
    off = np.array([50, -48, 52], F)
    out["offset"] = (u(300) + off, u(256) + off)                         # err ~ 0.03: the walk widens by shells
    out["dense_offset"] = (u(128, 0.1) + off, u(512, 0.1) + off)         # spacing^2 far below the expansion's rounding
    blob = np.concatenate([u(61, 0.01) + F(0.3), np.array([[10, 0.3, 0.3], [0.3, -10, 0.3], [0.3, 0.3, 10]], F)])
    out["one_cell_far"] = (np.concatenate([u(40, 0.01) + F(0.3), u(40, 10.0), u(20, 20.0) - F(10)]), blob[rng.permutation(64)])
    coarse = u(100)
    far = np.concatenate([u(30) + F(1.5), u(10) * F(-40), u(6) + F(1e3), u(6) - F(3e6), np.array(
        [[1e20, 0, 0], [0.5, -1e20, 0.5], [3e38, 3e38, 3e38], [np.nan, 0.5, 0.5], [0.5, np.inf, 0.5], [0.1, 0.2, -np.inf]], F), u(6)])
    out["outside"] = (far.astype(F), coarse)                             # queries outside the box, non-finite queries
    bad = u(50)
    bad[17, 1] = np.inf
    out["inf_coarse"] = (u(70), bad)                                     # no grid: every query is the scan
    return {k: (np.ascontiguousarray(f, dtype=F), np.ascontiguousarray(c, dtype=F)) for k, (f, c) in out.items()}
