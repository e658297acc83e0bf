// One row of the CE-on-log-probs gradient (nontarget.py:34 / target.py:36-39: CrossEntropyLoss applied to the network's
// log-probs, i.e. a second log_softmax), shared by ce_logp_grad_kernel (psg_attack.hip, one launch over all rows) and
// fp1_loop_kernel (psg_pn2_kernels.cuh, the row inside the fused fp1 + head launch of the NB loop).  The two units are compiled
// with different contraction settings (psg_attack.o: -ffp-contract=off, psg_pn2.o: the compiler's default), and the fused
// launch must give the bits of the separate one: the arithmetic lives here, once, with contraction off in the function itself.
// Plain C++ apart from the qualifiers, so that tests/test_ce_row_host.py can compile it for the host.
#pragma once
#include <math.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define PSG_CE_ROW_FN __host__ __device__ __forceinline__
#else
#define PSG_CE_ROW_FN inline
#endif

namespace psg {

constexpr int CE_ROW_MAXC = 32;

// g[c] = (softmax(lp)[c] - [c == y]) * scale for the n_cls (<= CE_ROW_MAXC) entries of one row, classes walked 0 .. n_cls - 1 in
// every loop; an inactive row (beyond rows_active: the targeted attack's rooms 1 ..) gets zeros.  Returns the row's loss term
// -log_softmax(lp)[y] * scale (0 for an inactive row or a y outside the classes).
PSG_CE_ROW_FN float ce_row_grad(const float *lp, int n_cls, int y, float scale, bool active, float *g)
{
#pragma clang fp contract(off)
    if (!active) {
        for (int c = 0; c < n_cls; ++c) g[c] = 0.0f;
        return 0.0f;
    }
    // exp and log as the BUILTINS, not through the header's expf / logf: the wrappers are functions of their own, compiled with
    // the unit's contraction setting whatever the pragma above says, and the device expansion of a log whose call may contract
    // fuses its last multiply-add (one ulp apart from ce_logp_grad_kernel's on one row in ten)
    float z[CE_ROW_MAXC];
    float m = -INFINITY;
    for (int c = 0; c < n_cls; ++c) { z[c] = lp[c]; m = fmaxf(m, z[c]); }
    float s = 0.0f;
    for (int c = 0; c < n_cls; ++c) s += __builtin_expf(z[c] - m);
    const float lse = __builtin_logf(s);
    float term = 0.0f;
    for (int c = 0; c < n_cls; ++c) {
        const float lp2 = (z[c] - m) - lse;  // second log_softmax (CrossEntropyLoss applied to log-probs)
        const float p = __builtin_expf(lp2);
        g[c] = (p - (c == y ? 1.0f : 0.0f)) * scale;
        if (c == y) term = -lp2 * scale;
    }
    return term;
}

}  // namespace psg
