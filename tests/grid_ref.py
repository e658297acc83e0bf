"""numpy float32 restatement of the reference's grid sub-sampling (grid_subsampling.cpp:5-106) and of the 1-NN projection
onto the sub-cloud, for tests/test_grid_host.py and tests/test_gpu_grid.py.

grid_sub_sampling: every step in float32, in the reference's order - origin = floor(min * (1 / dl)) * dl with 1 / dl
rounded first, cell index floor((p - origin) / dl) (clamped at 0: the reference's cast of -1 is undefined), key =
iX + NX * iY + NX * NY * iZ, a STABLE sort by key so that a cell's members stay in input order, per-cell sums as sequential
float32 additions in that order, barycentre = sum * float32(1.0 / count), mean feature = sum / float32(count), label =
the most frequent value per dimension.  Ours: output rows ascend by key, label ties go to the smallest value.

The keyword switches turn single steps into the mutants that tests/test_grid_host.py must catch."""
import numpy as np

F = np.float32


def grid_of(points, dl, origin_floor=True):
    """(origin [3] f32, n [3] int, cell [N,3] int64) of the reference's grid over points [N,3] f32."""
    p = np.ascontiguousarray(points, F)
    dl = F(dl)
    inv = F(1) / dl
    mn, mx = p.min(0), p.max(0)
    origin = (np.floor(mn * inv) * dl).astype(F) if origin_floor else mn.copy()
    n = np.maximum(np.floor((mx - origin) / dl), 0).astype(np.int64) + 1
    cell = np.maximum(np.floor((p - origin) / dl), 0).astype(np.int64)
    return origin, n, cell


def cell_keys(points, dl, origin_floor=True):
    _, n, cell = grid_of(points, dl, origin_floor)
    return cell[:, 0] + n[0] * cell[:, 1] + n[0] * n[1] * cell[:, 2]


def _sequential_sums(values, order, start, count, reverse):
    """sum over each segment of values[order], as float32 additions in segment order (vectorised over the segments)."""
    acc = np.zeros((len(start),) + values.shape[1:], F)
    for r in range(int(count.max())):
        live = np.nonzero(count > r)[0]
        pos = start[live] + (count[live] - 1 - r if reverse else r)
        acc[live] = acc[live] + values[order[pos]]
    return acc


def grid_sub_sampling(points, features=None, labels=None, dl=0.1, reverse=False, origin_floor=True, bary_div=False,
                      ties_largest=False):
    """-> dict(sub_points [M,3] f32, sub_features [M,d] f32 | None, sub_labels [M,l] i32 | None, voxel_of_point [N] i32,
    tied [M,l] bool | None, count [M])."""
    p = np.ascontiguousarray(points, F)
    key = cell_keys(p, dl, origin_floor)
    order = np.argsort(key, kind="stable")
    ks = key[order]
    head = np.r_[True, ks[1:] != ks[:-1]]
    start = np.nonzero(head)[0]
    count = np.diff(np.r_[start, len(ks)])
    rank = np.cumsum(head) - 1
    vox = np.empty(len(p), np.int32)
    vox[order] = rank
    cf = count.astype(F)
    sp = _sequential_sums(p, order, start, count, reverse)
    out = {"voxel_of_point": vox, "count": count, "sub_features": None, "sub_labels": None, "tied": None}
    out["sub_points"] = (sp / cf[:, None]).astype(F) if bary_div else (sp * (1.0 / count.astype(np.float64)).astype(F)[:, None]).astype(F)
    if features is not None:
        f = np.ascontiguousarray(features, F)
        out["sub_features"] = (_sequential_sums(f, order, start, count, reverse) / cf[:, None]).astype(F)
    if labels is not None:
        lab = np.ascontiguousarray(labels, np.int32).reshape(len(p), -1)
        M, L = len(start), lab.shape[1]
        sub = np.empty((M, L), np.int32)
        tied = np.zeros((M, L), bool)
        for c in range(L):
            o2 = np.lexsort((lab[:, c], vox))                    # by (cell, label)
            v2, l2 = vox[o2], lab[o2, c]
            rh = np.r_[True, (v2[1:] != v2[:-1]) | (l2[1:] != l2[:-1])]
            rs = np.nonzero(rh)[0]
            rlen = np.diff(np.r_[rs, len(v2)])
            rv, rl = v2[rs], l2[rs]
            best = np.zeros(M, np.int64)
            np.maximum.at(best, rv, rlen)
            top = rlen == best[rv]                               # the runs that reach their cell's maximum, label ascending
            tied[:, c] = np.bincount(rv[top], minlength=M) > 1
            if ties_largest:
                sub[rv[top], c] = rl[top]                        # the last assignment per cell wins: the largest label
            else:
                sub[rv[top][::-1], c] = rl[top][::-1]            # ... the smallest
        out["sub_labels"], out["tied"] = sub, tied
    return out


def sq_dist(q, s):
    """float32 ((dx*dx) + dy*dy) + dz*dz of q [Q,3] against s [M,3] -> [Q,M]."""
    q, s = q.astype(F), s.astype(F)
    d = q[:, None, 0] - s[None, :, 0]
    acc = d * d
    d = q[:, None, 1] - s[None, :, 1]
    acc += d * d                                             # one rounding of the product, one of the sum: no contraction in numpy
    d = q[:, None, 2] - s[None, :, 2]
    acc += d * d
    return acc


def nearest_sub_point(sub, query, chunk=1024):
    """Index of the nearest sub-point of every query, brute force in the float32 formula, ties to the lower index."""
    sub, query = np.ascontiguousarray(sub, F), np.ascontiguousarray(query, F)
    out = np.empty(len(query), np.int32)
    for a in range(0, len(query), chunk):
        out[a:a + chunk] = np.argmin(sq_dist(query[a:a + chunk], sub), axis=1)
    return out


def canonical(points, features=None, labels=None):
    """Rows sorted lexicographically by (x, y, z): the order-free form of a sub-cloud."""
    o = np.lexsort((points[:, 2], points[:, 1], points[:, 0]))
    return (points[o], None if features is None else features[o], None if labels is None else labels.reshape(len(points), -1)[o], o)


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a.view(np.uint32), b.view(np.uint32))
