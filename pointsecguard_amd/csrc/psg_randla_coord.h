// Internal (not part of the C ABI): the kernels of RandLA-Net's coordinate gradient that are compiled with
// -ffp-contract=off (psg_randla_coord.hip), launched from psg_rla_backward_full (psg_randla_net.hip).
#pragma once
#include "psg_common.h"

namespace psg {

// transpose of relative_pos_encoding per edge e = (i, k), j = neigh[e]: relpos [E][10] (the forward's own values), g_rp [E][10]
// -> side_i [E] = what point i receives, side_j [E] = what point j receives (x, y, z, 0)
int rla_relpos_bwd(const float *relpos, const float *g_rp, size_t edges, float4 *side_i, float4 *side_j, hipStream_t st);

// gxyz [n][3] of one level: a point's own 16 edges (ascending k), its in-edges through inv_off / inv_ent (ascending), and - for a
// row among its cloud's first nc_sub - the next level's complete gradient g_next [n / nc * nc_sub][3] (null at the last level)
int rla_point_sum(const float4 *side_i, const float4 *side_j, const int32_t *inv_off, const int32_t *inv_ent, const float *g_next,
                  int nc, int nc_sub, size_t n, float *gxyz, hipStream_t st);

}  // namespace psg
