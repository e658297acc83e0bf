// The occurrence lists of the whole-scene attacks (psg_scene.hip builds them, psg_scene.hip and psg_scene_nu.hip read them):
// occ_off [n_scene + 1] and occ_ent [rows], the slot numbers of every scene point in ascending order.  One walk for every
// reader, so that the order of a point's gradient sum - which decides bits - is written down once.
#pragma once
#include <climits>
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace {

inline unsigned blocks_for(size_t n) { return (unsigned)((n + 255) / 256); }

// the rows of [rows][9] are addressed through int32 slot numbers (the lists hold them): rows * 9 floats must stay below 2^31
inline bool rows_ok(int rows) { return rows > 0 && rows <= INT_MAX / 9; }

// slot(e) for every slot e of scene point p, in list order; returns whether there was one.  The list's bounds are clamped
// to [0, rows] and entries outside [0, rows) are passed over (psg_scene_occ_build leaves -1 where a row's index was bad), so
// no caller indexes with anything else.
template <typename F>
__device__ __forceinline__ bool for_each_slot(const int32_t *__restrict__ occ_off, const int32_t *__restrict__ occ_ent, size_t p,
                                              int rows, F slot)
{
    const int lo = max(occ_off[p], 0), hi = min(occ_off[p + 1], rows);
    bool any = false;
    for (int i = lo; i < hi; ++i) {
        const int e = occ_ent[i];
        if (e < 0 || e >= rows) continue;
        slot(e);
        any = true;
    }
    return any;
}

}  // namespace
