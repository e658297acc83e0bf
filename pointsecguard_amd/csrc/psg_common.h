// Internal helpers shared by the libpsg translation units (not part of the C ABI).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include <functional>
#include <string>
#include <vector>

#include "../../include/psg.h"

namespace psg {

void set_error(const char *fmt, ...);

// Blocking host <-> device copy that does NOT go through the legacy default stream: hipMemcpy synchronises with every
// blocking stream of the process, which is an error - for the copying thread AND for the capture - while another host
// thread captures a hipGraph on one ("operation would make the legacy stream depend on a capturing blocking stream":
// the one-call-per-room NU harness builds its model copies from twelve threads).  A non-blocking stream of its own per call.
hipError_t copy_sync(void *dst, const void *src, size_t bytes, hipMemcpyKind kind);
// The same for hipMemset.  Measured (tools/capture_probe.hip, round 5): ANOTHER host thread's hipMemcpy / hipMemset on the
// legacy stream - and its hipDeviceSynchronize - INVALIDATE a hipStreamCaptureModeThreadLocal capture in progress on any
// stream of the process, blocking or not (the caller gets hipErrorStreamCaptureImplicit / ...Unsupported, the capturing
// thread's next launch hipErrorStreamCaptureInvalidated); hipMalloc / hipFree, stream and event creation,
// the LDS opt-in (allow_big_lds), async work on stream 0 and hipStreamSynchronize do not.  So no entry point that can run beside a
// capture (creation, upload, forward / backward / attack) uses the legacy-stream forms; only the test read-backs
// (psg_*_debug_read, psg_gcn_knn_stats, psg_rla_sampler_possibility) synchronise the device.
hipError_t memset_sync(void *dst, int value, size_t bytes);

#define PSG_CHECK_HIP(expr)                                                                      \
    do {                                                                                         \
        hipError_t _e = (expr);                                                                  \
        if (_e != hipSuccess) {                                                                  \
            psg::set_error("%s:%d: %s failed: %s", __FILE__, __LINE__, #expr, hipGetErrorString(_e)); \
            return PSG_ERR_HIP;                                                                  \
        }                                                                                        \
    } while (0)

#define PSG_REQUIRE(cond, ...)                                                                   \
    do {                                                                                         \
        if (!(cond)) {                                                                           \
            psg::set_error(__VA_ARGS__);                                                         \
            return PSG_ERR_ARG;                                                                  \
        }                                                                                        \
    } while (0)

// Every environment switch the library reads goes through these two (psg_api.hip): they return the variable's value and
// record its NAME, so that psg_env_switches() can tell a caller (bench.py prints them and refuses the result-changing
// ones) which non-default switches this process runs under.  Switches select between tested paths or turn on diagnosis;
// the only ones that change RESULTS exist in -DPSG_DIAG_BUILD libraries.
const char *env_str(const char *name);
int env_int(const char *name, int dflt);

// Diagnosis only (PSG_TRACE_SYNC=1, eager launches outside any stream capture): after every checked launch the device is
// synchronised and the launch site is written to stderr, so that a run that stops shows the last launch that completed
// and the one that did not (tools/profile_round.sh gmfma_trace; DESIGN.md section 4, "the counter-pass hang").
// A site is "file:line", optionally "#variant" behind it, without whitespace: PSG_SITE where the launch is written.  A launch
// helper takes the site from its CALLER (psg_pn2.hip: launch_lds), so that paths which share the helper - or one source
// line: PSG_SITE "#colour" - keep sites of their own; tests/test_gpu_alt_paths.py tells the switch-selected paths apart by them.
bool trace_sync_enabled();
void trace_sync_point(const char *site);

#define PSG_STR_(x) #x
#define PSG_STR(x) PSG_STR_(x)
#define PSG_SITE __FILE__ ":" PSG_STR(__LINE__)
#define PSG_LAUNCH_CHECK_AT(site)                                                                \
    do {                                                                                         \
        PSG_CHECK_HIP(hipGetLastError());                                                        \
        if (psg::trace_sync_enabled()) psg::trace_sync_point(site);                               \
    } while (0)
#define PSG_LAUNCH_CHECK() PSG_LAUNCH_CHECK_AT(PSG_SITE)

// The one dynamic-LDS opt-in of the library (psg_api.hip): a launch that asks for more than 48 KiB calls this first.  The
// kernel is opted into the device maximum (160 KiB less its static LDS; the attribute changes neither code nor occupancy) by ONE driver call per
// kernel and process - memoised under a mutex: the one-call-per-room NU harness launches from twelve host threads - so a
// launch path never reaches the driver for a kernel that is opted in.  Under PSG_TRACE_SYNC every driver call is printed.
hipError_t allow_big_lds(const void *kern);

// Every model / workspace handle gets a process-unique, never re-used generation number at creation.  The hipGraph keys of the
// replayed loops compare THESE, not handle addresses: the allocator may hand a new handle the address of a freed one, and a
// graph keyed on the address would then replay kernels whose arguments point into the freed arena (advisor, round 4).
uint64_t next_generation();
uint64_t pn2_model_generation(const psg_pn2_model *m);
int pn2_forward_lean(psg_pn2_model *m, psg_pn2_ws *ws, int fwd, const float *x0, float *logp_out, psg_stream stream);
// psg_pn2_backward for the colour channels of the input gradient only (the NU loop; psg_pn2.hip)
int pn2_backward_colour(psg_pn2_model *m, psg_pn2_ws *ws, int fwd, const float *dlogp, float *dx0_out, psg_stream stream);
uint64_t pn2_ws_generation(const psg_pn2_ws *ws);
// The model / workspace requirements of psg_pn2_backward_full (SSG, split first layers) under the caller's name `who`, for
// entry points that enqueue other work before they reach it (psg_pn2_nu_field_step): PSG_OK or PSG_ERR_ARG with a message.
int pn2_full_grad_check(const psg_pn2_model *m, const psg_pn2_ws *ws, const char *who);

// hipGraph bookkeeping of the replayed loops (psg_pn2_nb_attack, psg_pn2_nu_window, psg_gcn_nb_attack, psg_rla_bim_attack): a capture that
// fails falls back to the eager launches - correct, but slower - so it is COUNTED, per handle and for the process
// (psg_capture_stats), and a handle whose capture failed does not try again for the same key.
struct CaptureCounters { long long tried = 0, failed = 0, replays = 0, eager = 0; };
void capture_note(CaptureCounters *own, int tried, int failed, int replays, int eager);

// One instantiated hipGraph of a handle and the capture-or-replay sequence around it (psg_api.hip).  The KEY - what the graph
// is valid for - and the policy - when to capture, on which stream to replay - stay with the call site; this is the one
// copy of the fragile part.
struct GraphSlot {
    hipGraphExec_t exec = nullptr;
    bool capture_failed = false;     // the capture for the current key failed once: stay eager instead of trying in every call
    CaptureCounters cap;
    // Captures the launches `body` enqueues on `st` (ThreadLocal mode) and instantiates them into `exec`; counted.  A capture
    // that fails (refused on the legacy default stream, or invalidated - the notes on copy_sync / memset_sync above and DESIGN
    // 5i name what can do that) has executed nothing: false, `exec` stays null, `capture_failed` is set so that the key is not
    // tried again, and the caller runs the body eagerly - where a genuine launch error shows again.
    bool capture(hipStream_t st, const std::function<int()> &body);
    // the key changed: wait for replays in flight on `st`, drop the graph, allow a new capture
    hipError_t forget(hipStream_t st);
    hipError_t replay(hipStream_t st, int n = 1);     // n launches of `exec` on `st`, counted
    void note_eager(int n = 1) { capture_note(&cap, 0, 0, 0, n); }     // n bodies ran eagerly although a graph was wanted
    void destroy();                  // in the handle's destructor
};

// The capture-or-replay policy of the NU windows (psg_attack.hip), shared by psg_pn2_nu_window, psg_pointnet_nu_window,
// psg_gcn_nu_window, psg_rla_nu_window and psg_rla_tbim_window:
// writes the step constants {step, lr / (1 - beta1^t), sqrt(1 - beta2^t), slot3 ? slot3[i] : 0} of the window's n_steps steps into the handle's
// device rows, then runs `steps(rows)` eagerly (first window of a `key`, or after a failed capture), captures it (second
// window) or replays the captured graph.  `key` is the window's argument block with what the device rows carry zeroed;
// model_gen / ws_gen are the generation numbers of its handles.  graph == null: `steps(nullptr)`, eagerly.
int nu_graph_window(psg_nu_graph *graph, const void *key, size_t key_bytes, uint64_t model_gen, uint64_t ws_gen, int n_steps,
                    int step0, int adam_t0, float lr, float beta1, float beta2, hipStream_t st,
                    const std::function<int(const float *)> &steps, const float *slot3 = nullptr);
// While set (per host thread), psg_nu_adam_step(_rooms), psg_nu_step_latch, psg_rla_nu_adam_clouds and psg_rla_nu_latch_clouds
// read their step constants from this device row.
void nu_set_step_consts(const float *row);
const float *nu_step_consts();
// The step walkers set a step's row through this scope: the row holds from here to the end of the enclosing block and is
// cleared on every way out of it.
struct NuStepConsts {
    explicit NuStepConsts(const float *row) { nu_set_step_consts(row); }
    ~NuStepConsts() { nu_set_step_consts(nullptr); }
    NuStepConsts(const NuStepConsts &) = delete;
    NuStepConsts &operator=(const NuStepConsts &) = delete;
};
// The tail every NU step walker ends in, over its own argument block `a` (the blocks share these field names).
// Adam step on the colour variable of G attacks of `rows` batch rows: the lockstep form for two attacks and more; one attack
// is the batch form - the same arithmetic (its L2 sum at scal + 2 * G = scal + 2), and what it runs past an exit is discarded
// with the latch's snapshot either way.
template <typename Args> int nu_colour_adam(const Args *a, float c_smooth, float c_l2, int rows, int adam_t, psg_stream stream)
{
    const int G = a->G, B = G * rows;
    return G > 1 ? psg_nu_adam_step_rooms(a->w, a->m, a->v, a->mask, a->dx0, a->x0, a->ori, a->sgrad, c_smooth, c_l2, a->lr, a->beta1,
                                          a->beta2, a->eps, adam_t, B, a->N, a->active, a->scal + 2 * G, stream)
                 : psg_nu_adam_step(a->w, a->m, a->v, a->mask, a->dx0, a->x0, a->ori, a->sgrad, c_smooth, c_l2, a->lr, a->beta1, a->beta2,
                                    a->eps, adam_t, B, a->N, a->scal + 2 * G, stream);
}
// statistics, history row `hist_step` and exit latch of step `step`
template <typename Args> int nu_latch(const Args *a, int rows, float *hist_step, int step, psg_stream stream)
{
    return psg_nu_step_latch(a->pred, a->labels, a->use_target ? a->target : 0, a->mode ? a->mask : nullptr,
                             a->mode ? a->n_mask : nullptr, a->G, rows, a->N, a->mode, a->scal, hist_step, a->x0, a->out, a->active,
                             a->exit_step, step, stream);
}
// scal rows 3, 4 (Smooth_xyz, L2_xyz of the coordinate-field NU steps) into rows 5, 6 of hist_step [7][G], zeroed (psg_attack.hip)
int nu_field_hist_tail(float *scal, float *hist_step, int G, hipStream_t st);

// Optional per-launch HIP-event timing of a workspace (psg_*_prof_enable / psg_*_prof_read): pairs of events recorded on
// the LAUNCH stream around a launch (or a group of launches) with a tag and the algorithmic FLOPs of that launch; off in
// normal operation (one branch per launch).  bench.py's `roofline` objects are computed from these.
struct EvLog {
    bool on = false;
    std::vector<hipEvent_t> ev;      // pairs
    std::vector<int> tag;
    std::vector<double> flop, bytes;     // algorithmic FLOPs / bytes of the tagged launch
    size_t used = 0;
    void reset(bool enable) { on = enable; used = 0; tag.clear(); flop.clear(); bytes.clear(); }
    void destroy() { for (hipEvent_t e : ev) (void)hipEventDestroy(e); ev.clear(); }
    // sums per tag; blocks until the events have completed
    int read(int n_tags, double *total_ms, int *counts, double *flops, double *bytes_out = nullptr)
    {
        for (int i = 0; i < n_tags; ++i) { total_ms[i] = 0.0; counts[i] = 0; if (flops) flops[i] = 0.0; if (bytes_out) bytes_out[i] = 0.0; }
        for (size_t i = 0; i < tag.size(); ++i) {
            float ms = 0.f;
            if (hipEventSynchronize(ev[2 * i + 1]) != hipSuccess) return -1;
            if (hipEventElapsedTime(&ms, ev[2 * i], ev[2 * i + 1]) != hipSuccess) return -1;
            if (tag[i] < n_tags) {
                total_ms[tag[i]] += ms; counts[tag[i]] += 1;
                if (flops) flops[tag[i]] += flop[i];
                if (bytes_out) bytes_out[tag[i]] += bytes[i];
            }
        }
        return 0;
    }
};
struct EvScope {
    EvLog *log; hipStream_t st; hipEvent_t stop = nullptr;
    EvScope(EvLog *l, int tag, double flop, hipStream_t s, double bytes = 0.0) : log(l), st(s)
    {
        if (!log || !log->on) { log = nullptr; return; }
        while (log->used + 2 > log->ev.size()) {
            hipEvent_t e;
            if (hipEventCreate(&e) != hipSuccess) { log = nullptr; return; }
            log->ev.push_back(e);
        }
        hipEvent_t start = log->ev[log->used];
        stop = log->ev[log->used + 1];
        log->used += 2;
        log->tag.push_back(tag);
        log->flop.push_back(flop);
        log->bytes.push_back(bytes);
        (void)hipEventRecord(start, st);
    }
    ~EvScope() { if (log) (void)hipEventRecord(stop, st); }
};

static inline int ceil_div(int a, int b) { return (a + b - 1) / b; }
static inline int round_up(int a, int b) { return ceil_div(a, b) * b; }

// Model weights: a device copy of `h`, recorded on the model's `allocs` (which its destroy frees).  Null when the allocation
// or the copy failed - after a failed copy the block is already on `allocs` -; model creation turns that into PSG_ERR_HIP.
template <typename T> T *upload(std::vector<void *> &allocs, const std::vector<T> &h)
{
    void *p = nullptr;
    if (hipMalloc(&p, h.size() * sizeof(T)) != hipSuccess) return nullptr;
    allocs.push_back(p);
    if (copy_sync(p, h.data(), h.size() * sizeof(T), hipMemcpyHostToDevice) != hipSuccess) return nullptr;
    return (T *)p;
}

// Workspace arenas: every block 256-byte aligned, carved in a fixed order.  With a null base `take` only counts.
struct Bump {
    char *base = nullptr;
    size_t off = 0;
    template <typename T> T *take(size_t n)
    {
        off = (off + 255) & ~(size_t)255;
        T *p = base ? (T *)(base + off) : nullptr;
        off += n * sizeof(T);
        return p;
    }
};
// Runs `layout(Bump &)` twice: without a base for the size (rounded up to 256 bytes -> *bytes), then on the allocated *arena.
// A failed hipMalloc is reported under the entry point's name `who`; the caller still owns its handle.
template <typename Layout> int carve_arena(void **arena, size_t *bytes, const char *who, Layout &&layout)
{
    Bump size;
    layout(size);
    *bytes = (size.off + 255) & ~(size_t)255;
    const hipError_t e = hipMalloc(arena, *bytes);
    if (e != hipSuccess) {
        set_error("%s: hipMalloc(%zu) failed: %s", who, *bytes, hipGetErrorString(e));
        return PSG_ERR_HIP;
    }
    Bump bp;
    bp.base = (char *)*arena;
    layout(bp);
    return PSG_OK;
}

}  // namespace psg

struct psg_ctx {
    int device;
    int num_cu;
};
