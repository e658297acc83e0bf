// One row of the ResGCN f-loss (gcn_f_loss_grad_kernel, psg_attack.hip), included as TEXT by that kernel and by
// gcn_f_loss_grad_rooms_kernel, which runs it per room on pointers moved to the room: the one-room kernel keeps the
// instructions it had.  Names it expects in scope: r, rows, N, z, dz, pred, labels, mask, target, mode, n_cls, kappa, tsign,
// scale and the result fval.
    if (r < rows) {
        const float *zr = z + (size_t)r * n_cls;
        float v[MAXC];
        float m = -INFINITY;
        int am = 0;
        for (int c = 0; c < n_cls; ++c) {
            v[c] = zr[c];
            if (v[c] > m) { m = v[c]; am = c; }
        }
        if (pred) pred[r] = am;
        float *g = dz + (size_t)r * n_cls;
        for (int c = 0; c < n_cls; ++c) g[c] = 0.0f;
        const bool counted = mode == 0 || (r < N && (!mask || mask[r]));
        if (counted) {
            const int y = (mode == 2 || !labels) ? target : labels[r];
            // the zeroed slot of the true class takes part in the max, and torch.max returns its FIRST maximum: a class
            // at exactly 0 (all others <= 0) takes the gradient when it stands before the true class, not after it
            float oth = -INFINITY;
            int oi = -1;
            for (int c = 0; c < n_cls; ++c) {
                const float s = c == y ? 0.0f : v[c];
                if (s > oth) { oth = s; oi = c == y ? -1 : c; }
            }
            float own = v[y];
            bool own_live = true;
            // mode 0: max(onehot * z) - the other slots hold 0; a true-class logit of exactly 0 is the first maximum only in slot 0
            if (mode == 0 && !(own > 0.0f)) { own_live = own == 0.0f && y == 0; own = 0.0f; }
            const float jv = mode == 2 ? oth : own, iv = mode == 2 ? own : oth;
            const float val = tsign * (jv - iv);
            const bool pass = val >= -kappa;
            fval = pass ? val : -kappa;
            if (pass) {
                const float gs = tsign * scale;
                if (mode == 2) {
                    if (oi >= 0) g[oi] += gs;
                    g[y] -= gs;
                } else {
                    if (own_live) g[y] += gs;
                    if (oi >= 0) g[oi] -= gs;
                }
            }
        }
    }
