// The attack loops of ResGCN: the NB loop (colours, and the coordinate field) and the NU windows.  They reach the network
// only through psg_gcn_forward / psg_gcn_backward and the handles of psg_resgcn.h; this unit has no kernel of its own.
// Reference (paths relative to its ResGCN directory): sem_seg_dense/attacks/torchattacks/attacks/colper.py:17-39 NB_attack,
// :62-95 NU_attack, tcolper.py:85-132 tar_NU_attack.
#include <cmath>
#include <cstring>
#include <type_traits>

#include "psg_resgcn.h"

using namespace psg;
using namespace psg_gcn;

// ====================================================================================== NB attack
// colper.NB_attack: CrossEntropyLoss() (mean over all B*N points) on the logits, sign ascent, L-inf projection; the returned
// values are the un-projected last step (the projection is not written back after the loop).  field = colour: the colour
// channels through psg_pgd_step.  field = coord | both, an extension of the reference API (colper.py:17-37
// branches on `atype` and ships the colour branch only): psg_pgd_step_field on channels 0:3 - sign step, eta clamped to
// +-coord_eps, no [0, 1] clamp - and, both, on 3:6.  The kNN graphs are constants of the derivative (topk under no_grad), so
// psg_gcn_backward's dx0[0:3] IS the coordinate gradient.
static int gcn_nb_loop(psg_gcn_model *m, psg_gcn_ws *ws, const float *images, const int32_t *labels, int field, float eps,
                       float alpha, float coord_eps, float coord_alpha, int iters, float *adv_out, hipStream_t st)
{
    const int B = ws->B, N = ws->N;
    const size_t R = (size_t)B * N;
    const bool colour = field == kGcnFieldColour, both = field == PSG_NU_FIELD_BOTH;
    int rc;
    if ((rc = psg_to_point_major(images, B, 9, N, ws->x0, st))) return rc;
    if ((rc = gcn_extract_clean(ws, !colour, st))) return rc;
    PSG_CHECK_HIP(hipMemcpyAsync(ws->nb_labels, labels, R * sizeof(int32_t), hipMemcpyDeviceToDevice, st));
    // colours only: the head's kNN graph on xyz (architecture.py:59) is the same in every iteration, so the first forward
    // builds it and the later ones keep it.  Where the points move, every forward rebuilds it: it is never frozen.
    struct Unfreeze { psg_gcn_ws *w; ~Unfreeze() { w->head_graph_frozen = false; } } unfreeze{ws};
    ws->head_graph_frozen = false;
    auto iteration = [&](bool last) -> int {
        int r;
        if ((r = psg_gcn_forward(m, ws, ws->x0, ws->logits, st))) return r;
        ws->head_graph_frozen = colour;
        if ((r = psg_ce_logp_grad(ws->logits, ws->nb_labels, 0, (int)R, (int)R, NCLS, 1.0f / (float)R, ws->dlogits, nullptr, st)))
            return r;
        if ((r = psg_gcn_backward(m, ws, ws->dlogits, ws->dx0, st))) return r;
        if (colour) return psg_pgd_step(ws->x0, ws->dx0, ws->ori, nullptr, B, N, alpha, eps, 1.0f, last ? 1 : 0, st);
        if ((r = psg_pgd_step_field(ws->x0, ws->dx0, ws->ori_xyz, nullptr, B, N, 0, coord_alpha, coord_eps, 1.0f, last ? 1 : 0, st)))
            return r;
        return both ? psg_pgd_step_field(ws->x0, ws->dx0, ws->ori, nullptr, B, N, 3, alpha, eps, 1.0f, last ? 1 : 0, st) : PSG_OK;
    };
    // The first iteration runs eagerly (it also sets kernel attributes outside any capture).  The interior iterations 1 .. iters-2
    // enqueue exactly the same ~300 short launches with the same arguments (a single chain on `st`): where at least two are left they
    // are captured once into the field's holder, kept in the workspace with the key it is valid for, and replayed, which removes
    // most of the per-launch cost that bounds a single-room iteration; a capture that fails - it is not possible on the legacy
    // default stream - leaves them eager, counted.  The last iteration differs (it returns the un-projected step): eager again.
    // Under PSG_GCN_NO_GRAPH, under the launch tracer (it synchronises after every launch), while the workspace is profiling
    // and - the field loop only, which refuses the capture the colour loop lets fail - on the null stream all stay eager.
    const bool use_graph = !gcn_switches().no_graph && !trace_sync_enabled() && !ws->prof.on && (colour || st);
    const NbKey key{m->gen, field, eps, alpha, coord_eps, coord_alpha, ws->fixed_graphs};
    NbGraph &g = colour ? ws->nb : ws->nbf;
    if ((rc = iteration(iters == 1))) return rc;
    int it = 1;
    if (use_graph && iters - 1 - it >= 2) {
        if (!(g.key == key)) PSG_CHECK_HIP(g.slot.forget(st));
        if (!g.slot.exec && !g.slot.capture_failed) {
            g.slot.capture(st, [&] { return iteration(false); });
            g.key = key;
        }
        if (g.slot.exec) {
            PSG_CHECK_HIP(g.slot.replay(st, iters - 1 - it));
            it = iters - 1;
        } else {
            g.slot.note_eager(iters - 1 - it);
        }
    }
    for (; it < iters; ++it)
        if ((rc = iteration(it == iters - 1))) return rc;
    return psg_to_channel_major(ws->x0, B, 9, N, adv_out, st);
}

extern "C" int psg_gcn_nb_attack(psg_gcn_model *m, psg_gcn_ws *ws, const float *images, const int32_t *labels,
                                 float eps, float alpha, int iters, float *adv_out, psg_stream stream)
{
    PSG_REQUIRE(m && ws && images && labels && adv_out, "psg_gcn_nb_attack: null argument");
    PSG_REQUIRE(iters > 0, "psg_gcn_nb_attack: iters must be positive");
    if (int rc = gcn_keep_refuses(ws, "psg_gcn_nb_attack")) return rc;
    return gcn_nb_loop(m, ws, images, labels, kGcnFieldColour, eps, alpha, 0.f, 0.f, iters, adv_out, (hipStream_t)stream);
}

extern "C" int psg_gcn_nb_attack_field(psg_gcn_model *m, psg_gcn_ws *ws, const float *images, const int32_t *labels, int field,
                                       float eps, float alpha, float coord_eps, float coord_alpha, int iters, float *adv_out,
                                       psg_stream stream)
{
    PSG_REQUIRE(m && ws && images && labels && adv_out, "psg_gcn_nb_attack_field: null argument");
    PSG_REQUIRE(iters > 0, "psg_gcn_nb_attack_field: iters must be positive");
    PSG_REQUIRE(field == PSG_NU_FIELD_COORD || field == PSG_NU_FIELD_BOTH,
                "psg_gcn_nb_attack_field: field %d is neither coord (%d) nor both (%d); colours alone are psg_gcn_nb_attack", field,
                PSG_NU_FIELD_COORD, PSG_NU_FIELD_BOTH);
    PSG_REQUIRE(gcn_same_cfg(m, ws), "psg_gcn_nb_attack_field: model / workspace configuration mismatch");
    if (int rc = gcn_keep_refuses(ws, "psg_gcn_nb_attack_field")) return rc;
    return gcn_nb_loop(m, ws, images, labels, field, eps, alpha, coord_eps, coord_alpha, iters, adv_out, (hipStream_t)stream);
}

// ====================================================================================== NU attack windows
// colper.NU_attack / tcolper.tar_NU_attack for G one-room attacks in lockstep, on colours (psg_gcn_nu_window_args) or on the
// coordinate field = coord | both (psg_gcn_nu_field_window_args, an extension like the NB field loop): ONE step sequence of a
// window, shared by the eager and the captured path; dconsts_rows: the window's device rows or null.  A step is: apply (delta
// first, then the colour variable), forward, f-loss, backward, Smooth term(s), Adam step(s), latch and, on the field, the two
// coordinate sums into rows 5, 6 of the history row; the colour window is the field window with the coordinate half off.
// Everything is a launch or an asynchronous device-to-device copy on `stream`, so a window is a single chain.  The head's xyz
// graph is rebuilt by every forward: freezing it inside a colour window has not been measured, and a restart moves xyz.
template <typename Args> static int gcn_nu_steps(const Args *a, const float *dconsts_rows, psg_stream stream)
{
    constexpr bool kField = std::is_same<Args, psg_gcn_nu_field_window_args>::value;
    const int G = a->G, N = a->N;
    bool colour = true;
    if constexpr (kField) colour = a->field == PSG_NU_FIELD_BOTH;
    int rc = PSG_OK;
    for (int i = 0; i < a->n_steps && rc == PSG_OK; ++i) {
        const int step = a->step0 + i, adam_t = a->adam_t0 + i + 1;
        const int f_target = a->use_target ? a->target : 0;
        float *hist = a->hist + (size_t)i * (kField ? 7 : 5) * G;
        if constexpr (kField)
            if ((rc = psg_nu_coord_apply_rooms(a->delta, a->ori_xyz, a->mask, G, N, a->active, a->x0, stream))) break;
        if (colour && (rc = psg_nu_tanh_color_rooms(a->w, a->mask, G, N, a->x0, stream))) break;
        if ((rc = psg_gcn_forward(a->model, a->ws, a->x0, a->logits, stream))) break;
        if ((rc = psg_gcn_f_loss_grad_rooms(a->logits, a->labels, f_target, a->mask, a->mode, G, N, NCLS, a->kappa, a->tsign, a->c_f,
                                            a->dlogits, a->scal, a->pred, stream)))
            break;
        if ((rc = psg_gcn_backward(a->model, a->ws, a->dlogits, a->dx0, stream))) break;
        if (colour && (rc = psg_smooth_knn_sym_rooms(a->x0 + 3, 9, (size_t)N * 9, G, N, a->neighbour, a->scal + G, a->sgrad, a->active,
                                                     a->nn_state, stream)))
            break;
        if constexpr (kField)
            if ((rc = psg_smooth_knn_xyz_sym_rooms(a->x0, 9, (size_t)N * 9, G, N, a->neighbour, a->scal + 3 * G, a->sgrad_xyz,
                                                   a->active, a->nn_xyz, stream)))
                break;
        {
            psg::NuStepConsts consts(dconsts_rows ? dconsts_rows + 4 * i : nullptr);
            if (colour) rc = psg::nu_colour_adam(a, a->c_smooth, a->c_l2, 1, adam_t, stream);
            if constexpr (kField)
                if (rc == PSG_OK)
                    rc = psg_nu_coord_adam_step_rooms_w(a->delta, a->mx, a->vx, a->mask, a->dx0, a->sgrad_xyz, a->c_smooth_xyz,
                                                        a->c_l2_xyz, a->coord_lr, a->beta1, a->beta2, a->eps, adam_t, G, N, a->active,
                                                        a->scal + 4 * G, stream);
            if (rc == PSG_OK) rc = psg::nu_latch(a, 1, hist, step, stream);
        }
        if constexpr (kField)
            if (rc == PSG_OK) rc = psg::nu_field_hist_tail(a->scal, hist, G, (hipStream_t)stream);
    }
    return rc;
}

// what both windows require of their argument block, under the name `who` of the entry point that was called
template <typename Args> static int gcn_nu_check(const Args *a, const char *who)
{
    PSG_REQUIRE(a->n_steps > 0 && a->G > 0 && a->N > 0, "%s: n_steps=%d G=%d N=%d out of range", who, a->n_steps, a->G, a->N);
    PSG_REQUIRE(a->G == a->ws->B && a->N == a->ws->N,
                "%s: rooms form only - the workspace is for %d rooms of %d points, the window for %d of %d", who, a->ws->B, a->ws->N,
                a->G, a->N);
    PSG_REQUIRE(gcn_same_cfg(a->model, a->ws), "%s: model / workspace configuration mismatch", who);
    PSG_REQUIRE(a->mode >= 0 && a->mode <= 2, "%s: mode %d out of range", who, a->mode);
    PSG_REQUIRE(a->mode == 0 || (a->mask && a->n_mask), "%s: modes 1 and 2 need mask and n_mask", who);
    PSG_REQUIRE((a->mode == 2) == (a->use_target != 0), "%s: mode 2 is the one that takes a target class", who);
    PSG_REQUIRE(!a->use_target || (a->target >= 0 && a->target < NCLS), "%s: target class %d out of range", who, a->target);
    PSG_REQUIRE(a->neighbour > 0 && a->neighbour <= 16 && a->N <= 8192, "%s: neighbour=%d (1..16) / N=%d (<= 8192) out of range", who,
                a->neighbour, a->N);
    return gcn_keep_refuses(a->ws, who);
}

// Runs or replays the window.  What a captured window is valid for: the argument block without what the device rows carry
// (step, the step sizes), and whether the forward builds its graphs or takes the ones psg_gcn_set_graphs supplied (the two
// enqueue different launches).  slot3: the field window's fourth device-row constant, or null.
template <typename Args> static int gcn_nu_run(const Args *a, psg_nu_graph *graph, const float *slot3, psg_stream stream)
{
    struct Key { Args a; int fixed_graphs; } key;
    memset(&key, 0, sizeof(key));
    key.a = *a;
    key.a.step0 = 0; key.a.adam_t0 = 0; key.a.lr = 0.0f;
    if constexpr (std::is_same<Args, psg_gcn_nu_field_window_args>::value) key.a.coord_lr = 0.0f;
    key.fixed_graphs = a->ws->fixed_graphs ? 1 : 0;
    return nu_graph_window(a->ws->prof.on ? nullptr : graph, &key, sizeof(key), a->model->gen, a->ws->gen, a->n_steps, a->step0,
                           a->adam_t0, a->lr, a->beta1, a->beta2, (hipStream_t)stream,
                           [&](const float *rows) { return gcn_nu_steps(a, rows, stream); }, slot3);
}

extern "C" int psg_gcn_nu_window(const psg_gcn_nu_window_args *a, psg_nu_graph *graph, psg_stream stream)
{
    PSG_REQUIRE(a && a->model && a->ws && a->w && a->m && a->v && a->x0 && a->ori && a->labels && a->logits && a->dlogits && a->dx0 &&
                    a->sgrad && a->pred && a->scal && a->nn_state && a->hist && a->out && a->active && a->exit_step,
                "psg_gcn_nu_window: null argument");
    if (int rc = gcn_nu_check(a, "psg_gcn_nu_window")) return rc;
    return gcn_nu_run(a, graph, nullptr, stream);
}

extern "C" int psg_gcn_nu_field_window(const psg_gcn_nu_field_window_args *a, psg_nu_graph *graph, psg_stream stream)
{
    PSG_REQUIRE(a && a->model && a->ws && a->delta && a->mx && a->vx && a->ori_xyz && a->sgrad_xyz && a->nn_xyz && a->x0 && a->labels &&
                    a->logits && a->dlogits && a->dx0 && a->pred && a->scal && a->hist && a->out && a->active && a->exit_step,
                "psg_gcn_nu_field_window: null argument");
    PSG_REQUIRE(a->field == PSG_NU_FIELD_COORD || a->field == PSG_NU_FIELD_BOTH,
                "psg_gcn_nu_field_window: field %d is neither coord (%d) nor both (%d); colours alone are psg_gcn_nu_window", a->field,
                PSG_NU_FIELD_COORD, PSG_NU_FIELD_BOTH);
    PSG_REQUIRE(a->field != PSG_NU_FIELD_BOTH || (a->w && a->m && a->v && a->ori && a->sgrad && a->nn_state),
                "psg_gcn_nu_field_window: field both needs the colour state");
    if (int rc = gcn_nu_check(a, "psg_gcn_nu_field_window")) return rc;
    // slot 3 of the device rows: the coordinate variable's step size coord_lr / (1 - beta1^t), as
    // psg_nu_coord_adam_step_rooms_w computes it from its arguments
    float slot3[PSG_NU_GRAPH_MAX_STEPS];
    for (int i = 0; i < a->n_steps && i < PSG_NU_GRAPH_MAX_STEPS; ++i)
        slot3[i] = (float)((double)a->coord_lr / (1.0 - pow((double)a->beta1, (double)(a->adam_t0 + i + 1))));
    return gcn_nu_run(a, graph, slot3, stream);
}
