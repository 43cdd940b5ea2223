// capi.hip -- extern "C" boundary (include/afesp.h): argument checks and one call each into the layers behind it (the integral layer:
// integrals.h), and the synthetic-input generators.
#include <atomic>
#include <chrono>
#include <mutex>
#include <cstdio>
#include <cstring>
#include <thread>
#include <vector>

#include "../../include/afesp.h"
#include "integrals.h"
#include "ccsd_so.h"
#include "comm.h"
#include "fused.h"
#include "tall.h"

using namespace afesp;

struct afesp_ctx {
    Context cx;
    CCState cc;
    SOState so;
    Integrals in;   // the resident AO / MO integrals (integrals.h)
    // With the chains of a small-system iteration spread over lanes, issuing ~110 launches from the host (~4 us each) is
    // what is left; from the second call on the iteration is therefore replayed as a hipGraph (captured across the
    // lanes).  Only used where lanes are (small systems); AFESP_NO_GRAPH=1 keeps plain launches.
    struct GraphSlot {
        hipGraphExec_t exec = nullptr;
        int64_t epoch = -1;      // Context::scratch_epoch at capture
        int calls = 0;
        bool disabled = false;
        void reset()
        {
            if (exec) (void)hipGraphExecDestroy(exec);
            exec = nullptr;
            calls = 0;
            disabled = knobs().no_graph;
        }
    } graph_cc;
    // the launch-fused path of a small system (fused.h): the recorded and levelled call sequences of the spin-free solver --
    // intermediates alone, amplitudes alone (the term-by-term entry points) and the whole iteration
    FusedSlot fused_int, fused_amp, fused_iter;
    FusedSlot fused_so;   // ... and the spin-orbital iteration (build_tau / F / W + update_amplitudes)
    void cc_programs_reset()
    {
        graph_cc.reset();
        fused_slot_reset(cx, fused_int);
        fused_slot_reset(cx, fused_amp);
        fused_slot_reset(cx, fused_iter);
    }
    void so_programs_reset() { fused_slot_reset(cx, fused_so); }
};

namespace {

// The code-object preload (afesp_ctx_create) runs ONCE per process and device: the first context of a device starts the start-up
// thread, later ones start none.  What makes it safe beside the caller's own launches -- and two callers' launches beside each other --
// is not this claim but first_use.h: every first use of a kernel function, by the preload lists and by every launch site alike, is
// made under ONE process-wide lock (the round-5 abort "Cannot find Symbol with name ...slice_phys_kernel..." was the start-up thread
// and afesp_synthetic_init resolving that one function at the same moment).  Entry points therefore no longer wait for the preload
// (round 5 made them: the first Fock builds of els_amd run beside it again).
struct PreloadClaim {
    std::mutex mu;
    unsigned long long claimed = 0;   // bit per device (a device id >= 64 is never claimed: its kernels load on first use, under the lock)
    bool claim(int dev)
    {
        std::lock_guard<std::mutex> lk(mu);
        if (dev < 0 || dev >= 64 || (claimed >> dev) & 1ull) return false;
        claimed |= 1ull << dev;
        return true;
    }
};
PreloadClaim g_preload;

// What every entry point that takes a context goes through: the body runs with the context's device selected, and what it throws
// becomes the return code and the context's last error.
template <class F>
int entry(afesp_ctx* c, F&& f)
{
    if (!c) return 1;
    Context& cx = c->cx;
    first_use_tls_device() = cx.device;   // (the launch sites' per-device flags, first_use.h)
    knobs_refresh();                       // (every AFESP_* variable follows the environment call by call, knobs.h)
    // A body that threw may have forked lanes without joining them: before the caller can free or re-initialise anything, every
    // lane is idle and lane 0 is the one in use again.
    auto failed = [&](const char* what, int code) {
        cx.last_error = what;
        if (!cx.lanes.empty()) {
            cx.quiesce();
            cx.use_lane(0);
            cx.marks_used = 0;
        }
        return code ? code : 1;
    };
    try {
        AFESP_HIP(hipSetDevice(cx.device));
        f(cx);
        return 0;
    } catch (const Error& e) {
        return failed(e.what(), e.code);
    } catch (const std::exception& e) {
        return failed(e.what(), 1);
    }
}

// Device-only timing of `body` on the context's stream: one warm call, then ms per call over `reps` of them
template <class Body>
double time_on_stream(Context& cx, int reps, Body body)
{
    struct Event { hipEvent_t e = nullptr; ~Event() { if (e) (void)hipEventDestroy(e); } } a, b;   // (destroyed on every path)
    AFESP_HIP(hipEventCreate(&a.e));
    AFESP_HIP(hipEventCreate(&b.e));
    body();
    AFESP_HIP(hipEventRecord(a.e, cx.stream));
    for (int r = 0; r < reps; ++r) body();
    AFESP_HIP(hipEventRecord(b.e, cx.stream));
    AFESP_HIP(hipEventSynchronize(b.e));
    float ms = 0.f;
    AFESP_HIP(hipEventElapsedTime(&ms, a.e, b.e));
    return (double)ms / (reps > 0 ? reps : 1);
}

// splitmix64 -> uniform in [0,1)
__device__ __forceinline__ double hash_uniform(uint64_t x)
{
    x += 0x9E3779B97F4A7C15ull;
    x = (x ^ (x >> 30)) * 0xBF58476D1CE4E5B9ull;
    x = (x ^ (x >> 27)) * 0x94D049BB133111EBull;
    x ^= x >> 31;
    return (double)(x >> 11) * (1.0 / 9007199254740992.0);
}
__global__ void synth_packed_kernel(double* packed, int64_t n, double scale, uint64_t seed)
{
    for (int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; k < n; k += (int64_t)gridDim.x * blockDim.x)
        packed[k] = scale * (2.0 * hash_uniform(seed + (uint64_t)k) - 1.0);
}

}  // namespace

// Runs `body` (launches on the context's lanes, no host synchronisation) directly for the first AFESP_GRAPH_AFTER calls,
// then captures it into a graph once and replays the graph afterwards.  Nothing executes during capture, so a failed
// capture simply falls back to running the body.
template <typename Body>
static void replay(afesp_ctx* ctx, afesp_ctx::GraphSlot& g, bool eligible, Body body)
{
    Context& cx = ctx->cx;
    if (g.exec && g.epoch != cx.scratch_epoch) {   // a scratch buffer the graph refers to may have been freed since
        (void)hipGraphExecDestroy(g.exec);
        g.exec = nullptr;
        g.calls = 0;
    }
    if (g.exec) {
        AFESP_HIP(hipGraphLaunch(g.exec, cx.stream));
        return;
    }
    if (!eligible || g.disabled) {
        body();
        return;
    }
    // Capturing and instantiating the ~110-node graph costs ~10 ms; a replay saves ~0.1 ms over the laned launches.  A real
    // molecule converges in 15-30 iterations, so the capture waits until a context has iterated long enough for it to pay
    // (AFESP_GRAPH_AFTER, default 40 calls).
    const int graph_after = knobs().graph_after;
    if (g.calls == 0 || g.epoch != cx.scratch_epoch || g.calls < graph_after) {
        // first call, or cached scratch buffers were dropped since the last one: whatever the body (re)builds or allocates is
        // done here, outside any capture
        body();
        g.calls = (g.epoch != cx.scratch_epoch) ? 1 : g.calls + 1;
        g.epoch = cx.scratch_epoch;
        return;
    }
    // The capture is opened on the origin stream (lane 0).  A body that throws half-way leaves another lane selected and
    // events outstanding: both are put back BEFORE the capture is ended, and the capture is ended on the origin stream --
    // ending it on a lane's stream would leave lane 0 capturing for ever, and the direct run below would execute nothing.
    cx.use_lane(0);
    hipStream_t origin = cx.stream;
    hipGraph_t graph = nullptr;
    if (hipStreamBeginCapture(origin, hipStreamCaptureModeThreadLocal) != hipSuccess) {
        (void)hipGetLastError();
        g.disabled = true;
        body();
        return;
    }
    bool ok = true;
    try {
        body();
    } catch (...) {
        ok = false;
    }
    cx.use_lane(0);
    cx.marks_used = 0;
    const hipError_t e = hipStreamEndCapture(origin, &graph);
    if (ok && e == hipSuccess && graph && hipGraphInstantiate(&g.exec, graph, nullptr, nullptr, 0) == hipSuccess) {
        (void)hipGraphDestroy(graph);
        g.epoch = cx.scratch_epoch;
        AFESP_HIP(hipGraphLaunch(g.exec, cx.stream));
        return;
    }
    if (knobs().graph_debug) fprintf(stderr, "afesp: graph capture failed (body ok %d, end capture %d)\n", (int)ok, (int)e);
    (void)hipGetLastError();
    if (graph) (void)hipGraphDestroy(graph);
    g.exec = nullptr;
    g.disabled = true;
    // a failed capture (e.g. lanes left unjoined by the throw) has been invalidated by EndCapture; make sure of it
    hipStreamCaptureStatus st = hipStreamCaptureStatusNone;
    if (hipStreamIsCapturing(origin, &st) != hipSuccess || st != hipStreamCaptureStatusNone) {
        (void)hipGetLastError();
        throw Error(2, "afesp: the stream is still capturing after a failed graph capture");
    }
    for (size_t i = 1; i < cx.lanes.size(); ++i) {   // lanes that were pulled into the capture are out of it as well
        hipStreamCaptureStatus ls = hipStreamCaptureStatusNone;
        if (hipStreamIsCapturing(cx.lanes[i].stream, &ls) != hipSuccess || ls != hipStreamCaptureStatusNone) {
            (void)hipGetLastError();
            throw Error(2, "afesp: a lane is still capturing after a failed graph capture");
        }
    }
    body();
}

// One iteration up to the energy kernels (no host synchronisation): the launch-fused program of a small system (fused.h; recorded
// from the very calls below on first use), the call-by-call sequence otherwise.
static bool ccsd_iteration_body(afesp_ctx* ctx)   // true: the launch-fused program ran (read with ccsd_tail_read)
{
    if (ccsd_uses_lanes(ctx->cc) &&
        fused_exec(ctx->cx, ctx->fused_iter, [&] {
            ccsd_intermediates(ctx->cx, ctx->cc, true);
            ccsd_amplitudes(ctx->cx, ctx->cc, true);
            ccsd_tail_launch(ctx->cx, ctx->cc);
        }))
        return true;
    // Large systems (one stream, whole-tensor products): the same two-kernel tail -- P(ia/jb) + division, the energy / rms sums and the
    // DIIS history push in ONE pass over the residual instead of three (update, energy, push: 26 against 23 passes over o^2 v^2 elements at
    // eight history vectors, and no host wait between the energy and the push); the <= 17 x 17 system is then solved on the host.
    // AFESP_LARGE_TAIL=0: the three kernels.
    if (!ccsd_uses_lanes(ctx->cc) && knobs().large_tail) {
        ccsd_intermediates(ctx->cx, ctx->cc, true);
        ccsd_amplitudes(ctx->cx, ctx->cc, true);
        ccsd_tail_launch(ctx->cx, ctx->cc);
        return true;
    }
    ctx->cc.tail_pending = false;
    replay(ctx, ctx->graph_cc, ccsd_uses_lanes(ctx->cc), [&] {
        ccsd_intermediates(ctx->cx, ctx->cc, true);
        ccsd_amplitudes(ctx->cx, ctx->cc);
        ccsd_energy_launch(ctx->cx, ctx->cc);
    });
    return false;
}

extern "C" {

int afesp_version(void) { return 1; }
int64_t afesp_neri(int64_t nbasis) { return neri_of(nbasis); }

int afesp_ctx_create(int device, afesp_ctx** out)
{
    if (!out) return 1;
    *out = nullptr;
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) return 10;   // no GPU: fail loudly, no CPU fallback
    if (device < 0 || device >= ndev) return 11;
    if (hipSetDevice(device) != hipSuccess) return 12;
    afesp_ctx* c = new afesp_ctx();
    c->cx.device = device;
    int rc = entry(c, [&](Context&) {
        AFESP_HIP(hipStreamCreate(&c->cx.stream));
        c->cx.scal = c->cx.alloc(64 + 18 * 512);
        AFESP_HIP(hipHostMalloc((void**)&c->cx.scal_host, sizeof(double) * 64, hipHostMallocDefault));
        AFESP_HIP(hipHostMalloc((void**)&c->cx.res_host, sizeof(double) * (8 + 256 + 72), hipHostMallocCoherent | hipHostMallocMapped));
        memset(c->cx.res_host, 0, sizeof(double) * (8 + 256 + 72));
        AFESP_HIP(hipHostGetDevicePointer((void**)&c->cx.res_dev, c->cx.res_host, 0));
        c->cx.ws.bytes = (size_t)256 << 20;   // split-K slabs
        c->cx.ws.ptr = c->cx.alloc((int64_t)(c->cx.ws.bytes / sizeof(double)));
        c->cx.sync();
        // The device code of a translation unit is loaded on the first use of one of its kernels -- 55-70 ms in all, which a
        // small molecule would pay inside its first CCSD iteration.  Ask for it now, on a thread of its own: the caller goes
        // on with its host work (parsing eri.dat, the SCF set-up) meanwhile.  AFESP_NO_PRELOAD=1 switches it off.
        if (!knobs().no_preload) {
            // one start-up thread per process and device (PreloadClaim); a later context of the device starts none
            if (g_preload.claim(device)) c->cx.startup = std::thread([device, c] {
                first_use_tls_device() = device;
                if (hipSetDevice(device) != hipSuccess) return;
                // (the parallel streams of the call-by-call iteration: small systems run the launch-fused iteration on ONE stream since
                // round 4, so the 10-25 ms of queue creation are only spent ahead of time on request; fork() makes them when needed)
                if (knobs().preload_lanes) Context::prepare_lanes(c->cx.prepared, 6);   // (the context itself is not touched: fork() adopts them)
                {
                    // the runtime's own first-use set-up (staging buffers of pageable copies, its fill / copy kernels): ~8 ms that
                    // the first plan upload of a process would otherwise pay inside the first CCSD iteration
                    void* d = nullptr;
                    hipStream_t st = nullptr;
                    std::vector<double> h(4096, 1.0);
                    if (hipStreamCreateWithFlags(&st, hipStreamNonBlocking) == hipSuccess && hipMalloc(&d, h.size() * sizeof(double)) == hipSuccess) {
                        (void)hipMemsetAsync(d, 0, h.size() * sizeof(double), st);
                        (void)hipMemcpyAsync(d, h.data(), h.size() * sizeof(double), hipMemcpyHostToDevice, st);
                        (void)hipMemcpyAsync((char*)d + 8192, d, 8192, hipMemcpyDeviceToDevice, st);
                        (void)hipMemcpyAsync(h.data(), d, h.size() * sizeof(double), hipMemcpyDeviceToHost, st);
                        (void)hipStreamSynchronize(st);
                    }
                    if (d) (void)hipFree(d);
                    if (st) (void)hipStreamDestroy(st);
                    (void)hipGetLastError();
                }
                const bool dbg = knobs().preload_debug;   // time per translation unit on stderr
                auto timed = [dbg](const char* what, void (*fn)()) {
                    const auto t0 = std::chrono::steady_clock::now();
                    fn();
                    if (dbg) fprintf(stderr, "afesp preload %-10s %7.2f ms\n", what, std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count());
                };
                // (the gather kernel's module -- 10 ms to load, a hundred instantiations -- is not asked for: a small system never
                // launches it, and whatever loads here holds the runtime's lock against the caller's own first launches, e.g. the
                // Fock builds of the SCF that els_amd starts at once; a large system loads it with its first product.
                // AFESP_PRELOAD_GETT=1 restores it.)
                timed("kernels", preload_kernels);
                timed("fused", preload_fused);
                timed("contract", preload_contract);
                timed("small path", preload_small_path_kernels);
                timed("triples", preload_triples);
                timed("ccsd_so", preload_ccsd_so);
                timed("uhf", preload_uhf_kernels);
                timed("integrals", preload_integrals);
                if (knobs().preload_gett) timed("gett", preload_gett);
            });
        }
    });
    if (rc) {
        if (c->cx.startup.joinable()) c->cx.startup.join();
        delete c;
        return rc;
    }
    *out = c;
    return 0;
}

void afesp_ctx_destroy(afesp_ctx* ctx)
{
    if (!ctx) return;
    first_use_tls_device() = ctx->cx.device;   // (no guard here: the thread would otherwise keep its previous call's device)
    (void)hipSetDevice(ctx->cx.device);
    if (ctx->cx.startup.joinable()) ctx->cx.startup.join();
    ctx->cc_programs_reset();
    ctx->so_programs_reset();
    comm_destroy(ctx->cx.comm);
    ctx->cx.comm = nullptr;
    triples_plan_free(ctx->cc);
    so_triples_plan_free(ctx->so);
    ring_free(ctx->cx, ctx->cc);   // (the host-side descriptor of the ring launches; its device blocks go with the context)
    delete ctx;
}

const char* afesp_last_error(const afesp_ctx* ctx) { return ctx ? ctx->cx.last_error.c_str() : "null context"; }

int afesp_ao2mo_mp2(afesp_ctx* ctx, int64_t nbasis, int64_t nocc, const double* canon_coeff, const double* canon_levels,
                    const double* eri_packed, double* eri_mo_packed, double* e_mp2)
{
    return entry(ctx, [&](Context& cx) {
        if (nbasis <= 0 || nocc <= 0 || nbasis - nocc <= 0 || nbasis > 1024) throw Error(1, "afesp_ao2mo_mp2: bad extents");
        const double emp2 = ao2mo_mp2(cx, ctx->in, ctx->cc, nbasis, nocc, canon_coeff, canon_levels, eri_packed, eri_mo_packed);
        if (e_mp2) *e_mp2 = emp2;
    });
}

int afesp_mo_window(afesp_ctx* ctx, int64_t nbasis, int64_t nocc, int64_t n_frozen_core, int64_t n_frozen_virt,
                    const double* canon_levels, const double* eri_mo_packed, double* eri_act, double* e_mp2)
{
    return entry(ctx, [&](Context& cx) {
        const int64_t n = nbasis, nfc = n_frozen_core, nfv = n_frozen_virt;
        if (n <= 0 || n > 1024 || nocc <= 0 || nocc >= n || !canon_levels) throw Error(1, "afesp_mo_window: bad extents");
        if (nfc < 0 || nfv < 0) throw Error(1, "afesp_mo_window: negative number of frozen orbitals");
        if (nfc >= nocc) throw Error(1, "afesp_mo_window: no active occupied orbital left");
        if (nfv >= n - nocc) throw Error(1, "afesp_mo_window: no active virtual orbital left");
        if (!eri_mo_packed && (!ctx->in.mo || ctx->in.mo_n != n))
            throw Error(1, "afesp_mo_window: eri_mo_packed is NULL and no MO integrals are resident for this basis size "
                           "(call afesp_ao2mo_mp2 first; a window is taken once)");
        const double emp2 = mo_window(cx, ctx->in, ctx->cc, n, nocc, nfc, nfv, canon_levels, eri_mo_packed, eri_act);
        if (e_mp2) *e_mp2 = emp2;
    });
}

int afesp_mp2_vv_density(afesp_ctx* ctx, int64_t nbasis, int64_t nocc, int64_t n_frozen_core, const double* canon_levels, double* d_vv,
                         double* e_mp2)
{
    return entry(ctx, [&](Context& cx) {
        const int64_t n = nbasis, nfc = n_frozen_core;
        if (n <= 0 || n > 1024 || nocc <= 0 || nocc >= n || !canon_levels || !d_vv) throw Error(1, "afesp_mp2_vv_density: bad extents");
        if (nfc < 0) throw Error(1, "afesp_mp2_vv_density: negative number of frozen orbitals");
        if (nfc >= nocc) throw Error(1, "afesp_mp2_vv_density: no active occupied orbital left");
        if (!ctx->in.mo || ctx->in.mo_n != n)
            throw Error(1, "afesp_mp2_vv_density: no MO integrals are resident for this basis size (call afesp_ao2mo_mp2 first, and "
                           "afesp_mo_window afterwards)");
        const double emp2 = mp2_vv_density(cx, ctx->in, n, nocc, nfc, canon_levels, d_vv);
        if (e_mp2) *e_mp2 = emp2;
    });
}

int afesp_ccsd_init(afesp_ctx* ctx, int64_t nocc, int64_t nvirt, const double* eri_mo_packed, const double* canon_levels,
                    int diis_n_errmat)
{
    return entry(ctx, [&](Context& cx) {
        const int64_t n = nocc + nvirt;
        if (nocc <= 0 || nvirt <= 0 || n > 1024) throw Error(1, "afesp_ccsd_init: bad extents");
        const double* src = ctx->in.mo;
        double* tmp = nullptr;
        if (eri_mo_packed) {
            // (a same-shape state is about to be initialised where it lies: the packed integrals it kept for ccsd_need_vvvv go back
            // to the arena BEFORE their successor is asked for -- a geometry scan never holds two packed arrays)
            if (ccsd_can_reinit(ctx->cc, (int)nocc, (int)nvirt, diis_n_errmat) && ctx->cc.eri_own) {
                cx.quiesce();
                if (ctx->cc.eri_src == ctx->cc.eri_own) ctx->cc.eri_src = nullptr;
                cx.release(ctx->cc.eri_own);
                ctx->cc.eri_own = nullptr;
            }
            tmp = cx.alloc(neri_of(n));
            AFESP_HIP(hipMemcpyAsync(tmp, eri_mo_packed, sizeof(double) * neri_of(n), hipMemcpyHostToDevice, cx.stream));
            src = tmp;
        } else if (!src || ctx->in.mo_n != n) {
            throw Error(1, "afesp_ccsd_init: no MO integrals resident for this basis size (call afesp_ao2mo_mp2 first)");
        }
        // (a state of the same extents is initialised again where it lies: its compiled programs stay)
        if (!ccsd_can_reinit(ctx->cc, (int)nocc, (int)nvirt, diis_n_errmat)) {
            ctx->cc_programs_reset();
            cx.drop_scratch("ao2mo_");   // the AO->MO temporaries
        } else {
            ctx->graph_cc.reset();
        }
        ccsd_init(cx, ctx->cc, (int)nocc, (int)nvirt, src, canon_levels, diis_n_errmat);
        if (tmp) {
            // a large system forms <ef|ab> on request only (ccsd_need_vvvv): its state keeps the device copy of the integrals
            if (ctx->cc.v_vvvv.d) { cx.release(tmp); ctx->cc.eri_src = nullptr; }
            else ctx->cc.eri_own = tmp;
        }
    });
}

int afesp_ccsd_energy(afesp_ctx* ctx, double e_tol, double t_tol, double* energy, double* rms_sq, int* converged)
{
    return entry(ctx, [&](Context& cx) {
        if (!ctx->cc.ready) throw Error(1, "afesp_ccsd_energy: call afesp_ccsd_init first");
        int conv = ccsd_energy(cx, ctx->cc, e_tol, t_tol);
        if (energy) *energy = ctx->cc.energy;
        if (rms_sq) *rms_sq = ctx->cc.rms;
        if (converged) *converged = conv;
    });
}

int afesp_ccsd_update_intermediates(afesp_ctx* ctx)
{
    return entry(ctx, [&](Context& cx) {
        if (!ctx->cc.ready) throw Error(1, "call afesp_ccsd_init first");
        ccsd_refresh_sharding(cx, ctx->cc);
        if (!(ccsd_uses_lanes(ctx->cc) && fused_exec(cx, ctx->fused_int, [&] { ccsd_intermediates(cx, ctx->cc); })))
            ccsd_intermediates(cx, ctx->cc);
        cx.sync();
    });
}
int afesp_ccsd_update_amplitudes(afesp_ctx* ctx)
{
    return entry(ctx, [&](Context& cx) {
        ctx->cc.amp_epoch = ++cx.amp_clock;   // (the amplitudes may change: derived copies go stale)
        if (!ctx->cc.ready) throw Error(1, "call afesp_ccsd_init first");
        ccsd_refresh_sharding(cx, ctx->cc);
        ctx->cc.tail_pending = false;
        if (!(ccsd_uses_lanes(ctx->cc) && fused_exec(cx, ctx->fused_amp, [&] { ccsd_amplitudes(cx, ctx->cc); })))
            ccsd_amplitudes(cx, ctx->cc);
        cx.sync();
    });
}

int afesp_ccsd_iterate(afesp_ctx* ctx, double e_tol, double t_tol, double* energy, double* rms_sq, int* converged)
{
    return entry(ctx, [&](Context& cx) {
        ctx->cc.amp_epoch = ++cx.amp_clock;   // (the amplitudes may change: derived copies go stale)
        if (!ctx->cc.ready) throw Error(1, "afesp_ccsd_iterate: call afesp_ccsd_init first");
        ccsd_refresh_sharding(cx, ctx->cc);
        const bool fused = ccsd_iteration_body(ctx);
        int conv = fused ? ccsd_tail_read(cx, ctx->cc, e_tol, t_tol) : ccsd_energy_read(cx, ctx->cc, e_tol, t_tol);
        if (energy) *energy = ctx->cc.energy;
        if (rms_sq) *rms_sq = ctx->cc.rms;
        if (converged) *converged = conv;
    });
}

int afesp_ccsd_diis(afesp_ctx* ctx)
{
    return entry(ctx, [&](Context& cx) {
        ctx->cc.amp_epoch = ++cx.amp_clock;   // (the amplitudes may change: derived copies go stale)
        if (!ctx->cc.ready) throw Error(1, "afesp_ccsd_diis: call afesp_ccsd_init first");
        ccsd_diis_update(cx, ctx->cc);
    });
}

int afesp_ccsd_solve(afesp_ctx* ctx, int maxiter, double e_tol, double t_tol, double* iter_energy, double* iter_rms_sq, int* niter)
{
    return entry(ctx, [&](Context& cx) {
        ctx->cc.amp_epoch = ++cx.amp_clock;   // (the amplitudes may change: derived copies go stale)
        if (!ctx->cc.ready) throw Error(1, "afesp_ccsd_solve: call afesp_ccsd_init first");
        CCState& s = ctx->cc;
        // ccsd.f90:314-315, :325
        s.energy = s.energy_old = 0.0;
        k_fill(cx, s.t2_old.d, s.t2_old.size(), 0.0);
        ccsd_energy(cx, s, e_tol, t_tol);
        if (iter_energy) iter_energy[0] = s.energy;
        if (iter_rms_sq) iter_rms_sq[0] = s.rms;
        int result = -1;
        ccsd_refresh_sharding(cx, s);
        for (int it = 1; it <= maxiter; ++it) {
            const bool fused = ccsd_iteration_body(ctx);
            int conv = fused ? ccsd_tail_read(cx, s, e_tol, t_tol) : ccsd_energy_read(cx, s, e_tol, t_tol);
            if (iter_energy) iter_energy[it] = s.energy;
            if (iter_rms_sq) iter_rms_sq[it] = s.rms;
            if (conv) {
                result = it;
                break;
            }
            ccsd_diis_update(cx, s);
        }
        if (result < 0 && maxiter > 0) diis_check_flag(cx, host_scalars(cx, DIIS_FLAG_SLOT + 1));   // a solve that failed after the last energy read
        if (niter) *niter = result;
    });
}

int afesp_ccsd_get_amplitudes(afesp_ctx* ctx, double* t1, double* t2)
{
    return entry(ctx, [&](Context& cx) {
        if (!ctx->cc.ready) throw Error(1, "afesp_ccsd_get_amplitudes: no CCSD state");
        if (t1) AFESP_HIP(hipMemcpyAsync(t1, ctx->cc.t1.d, sizeof(double) * ctx->cc.t1.size(), hipMemcpyDeviceToHost, cx.stream));
        if (t2) AFESP_HIP(hipMemcpyAsync(t2, ctx->cc.t2.d, sizeof(double) * ctx->cc.t2.size(), hipMemcpyDeviceToHost, cx.stream));
        diis_check_flag(cx, host_scalars(cx, DIIS_FLAG_SLOT + 1));   // afesp_ccsd_diis does not wait for its solve: a failure surfaces here at the latest
    });
}

int afesp_ccsd_set_amplitudes(afesp_ctx* ctx, const double* t1, const double* t2)
{
    return entry(ctx, [&](Context& cx) {
        ctx->cc.amp_epoch = ++cx.amp_clock;   // (the amplitudes may change: derived copies go stale)
        if (!ctx->cc.ready) throw Error(1, "afesp_ccsd_set_amplitudes: no CCSD state");
        // (a large system holds I_ovov / I_voov and copies of the OLD amplitudes in the layout of its ring launches (ring.hip): an
        // afesp_ccsd_update_amplitudes that follows without new intermediates reads the reference-layout tensors and the new amplitudes)
        if (ring_live(ctx->cc)) {
            ring_tg_materialize(cx, ctx->cc, ctx->cc.I_ovov, ctx->cc.I_voov);
            ring_invalidate(ctx->cc);
        }
        ctx->cc.amps_touched = true;
        // (a launch-fused iteration has pushed its own result into the DIIS history already: afesp_ccsd_diis extrapolates the amplitudes
        // current at the call, so it pushes again -- into the same slot, the tail has advanced no counter)
        ctx->cc.tail_pending = false;
        if (t2) ctx->cc.hist_plain = ctx->cc.nerr + 1;   // (its error vector may lack the amplitudes' symmetry: full DIIS sums until it has left the history)
        if (t1) AFESP_HIP(hipMemcpyAsync(ctx->cc.t1.d, t1, sizeof(double) * ctx->cc.t1.size(), hipMemcpyHostToDevice, cx.stream));
        if (t2) AFESP_HIP(hipMemcpyAsync(ctx->cc.t2.d, t2, sizeof(double) * ctx->cc.t2.size(), hipMemcpyHostToDevice, cx.stream));
        cx.sync();
    });
}

int afesp_ccsd_get_tensor(afesp_ctx* ctx, const char* name, double* out, int64_t capacity)
{
    return entry(ctx, [&](Context& cx) {
        if (!ctx->cc.ready) throw Error(1, "afesp_ccsd_get_tensor: no CCSD state");
        CCState& s = ctx->cc;
        struct { const char* n; const Tensor* t; } tab[] = {
            {"v_oovv", &s.v_oovv}, {"v_ovov", &s.v_ovov}, {"v_vvov", &s.v_vvov}, {"v_oovo", &s.v_oovo}, {"v_oooo", &s.v_oooo},
            {"v_vvvv", &s.v_vvvv}, {"I_vo", &s.I_vo}, {"I_vv", &s.I_vv}, {"I_oo_p", &s.I_oo_p}, {"I_oo", &s.I_oo},
            {"c_oovv", &s.c}, {"asym_t2", &s.asym}, {"x_voov", &s.x_voov}, {"I_oooo", &s.I_oooo}, {"I_ovov", &s.I_ovov},
            {"I_voov", &s.I_voov}, {"I_ooov_p", &s.I_ooov_p}, {"r1", &s.r1}, {"r2", &s.r2},
            {"D1", &s.D1}, {"D2", &s.D2}, {"t1", &s.t1}, {"t2", &s.t2}};
        if (!strcmp(name, "I_vovv_p")) {   // not formed by the iteration (ccsd.hip): built from the current t1 on request
            const int64_t O = s.o, V = s.v;
            if (V * O * V * V > capacity) throw Error(1, "afesp_ccsd_get_tensor: buffer too small for I_vovv_p");
            Tensor t = view(cx.scratch("I_vovv_p", V * O * V * V), {V, O, V, V});
            ccsd_build_I_vovv_p(cx, s, t);
            AFESP_HIP(hipMemcpyAsync(out, t.d, sizeof(double) * t.size(), hipMemcpyDeviceToHost, cx.stream));
            cx.sync();
            return;
        }
        if (!strcmp(name, "v_vvvv")) ccsd_need_vvvv(cx, s);
        for (auto& e : tab)
            if (!strcmp(e.n, name)) {
                if (e.t->size() > capacity) throw Error(1, std::string("afesp_ccsd_get_tensor: buffer too small for ") + name);
                const double* src = e.t->d;
                // the residuals of a laned iteration lie in partial buffers that the update kernel adds up (ccsd_amplitudes)
                // (only what the LAST amplitudes call left there: a launch-fused or large-system call after a laned one has none)
                auto add_partial = [&](double* dst, const char* buf) {
                    auto it = cx.cache.find(buf);
                    if (s.partials_live && it != cx.cache.end()) k_axpby(cx, dst, 1.0, (const double*)it->second.first, 1.0, e.t->size());
                };
                if (!strcmp(name, "r2")) {   // the reference's tmp_t2 before P(ia/jb) includes 1/2 pp; it is kept packed here
                    double* full = cx.scratch("r2_full", e.t->size());
                    k_r2_full(cx, full, s.r2.d, s.pp, s.o, s.v);
                    add_partial(full, "r2_lane2");
                    add_partial(full, "r2_lane3");
                    if (ring_res_live(s)) k_add_swapped(cx, full, ring_Y(s), s.o, s.v);   // a ring term of a large system's residual (ring.hip)
                    src = full;
                } else if (ring_live(s) && (!strcmp(name, "I_ovov") || !strcmp(name, "I_voov"))) {
                    // a large system's iteration holds these two in the layout its ring products read (ring.hip): turned back on request
                    const int64_t O = s.o, V = s.v;
                    Tensor io = view(cx.scratch("ring_I_ovov", e.t->size()), {O, V, O, V}), iv = view(cx.scratch("ring_I_voov", e.t->size()), {V, O, O, V});
                    ring_tg_materialize(cx, s, io, iv);
                    src = !strcmp(name, "I_ovov") ? io.d : iv.d;
                } else if (!strcmp(name, "r1")) {
                    double* full = cx.scratch("r1_full", e.t->size());
                    k_copy(cx, full, s.r1.d, e.t->size());
                    add_partial(full, "r1_lane5");
                    src = full;
                }
                AFESP_HIP(hipMemcpyAsync(out, src, sizeof(double) * e.t->size(), hipMemcpyDeviceToHost, cx.stream));
                cx.sync();
                return;
            }
        throw Error(1, std::string("afesp_ccsd_get_tensor: unknown tensor ") + name);
    });
}

int64_t afesp_ccsd_t_ntriples(int64_t nocc) { return triples_count((int)nocc); }

int afesp_ccsd_t_shard_bounds(afesp_ctx* ctx, int64_t nocc, int64_t nvirt, int cr, int world, int64_t* bounds)
{
    return entry(ctx, [&](Context& cx) {
        if (nocc < 1 || nvirt < 1 || world < 1 || !bounds) throw Error(1, "afesp_ccsd_t_shard_bounds: bad arguments");
        triples_shard_bounds((int)nocc, (int)nvirt, cr != 0, world, bounds);
    });
}

int afesp_ccsd_t(afesp_ctx* ctx, int64_t t_begin, int64_t t_end, double out[4])
{
    return entry(ctx, [&](Context& cx) { ccsd_triples(cx, ctx->cc, t_begin, t_end, out); });
}

int afesp_ccsd_t_plain(afesp_ctx* ctx, int64_t t_begin, int64_t t_end, double out[2])
{
    return entry(ctx, [&](Context& cx) { ccsd_triples(cx, ctx->cc, t_begin, t_end, out, false, false); });
}

int afesp_ccsd_cr_intermediates(afesp_ctx* ctx)
{
    return entry(ctx, [&](Context& cx) {
        ctx->cc.cr_epoch = ++cx.amp_clock;
        ccsd_cr_intermediates(cx, ctx->cc);
        cx.sync();
    });
}

int afesp_ccsd_t_cr(afesp_ctx* ctx, int64_t t_begin, int64_t t_end, double out[6])
{
    return entry(ctx, [&](Context& cx) { ccsd_triples(cx, ctx->cc, t_begin, t_end, out, true); });
}

// ---------------------------------------------------------------- input / output side of the path
int afesp_read_eri_text(afesp_ctx* ctx, const char* path, int64_t nbasis, double* eri_packed, int64_t* nread)
{
    return entry(ctx, [&](Context& cx) {
        if (nbasis <= 0 || nbasis > 1024 || !path) throw Error(1, "afesp_read_eri_text: bad arguments");
        const int64_t lines = read_eri_text(cx, ctx->in, path, nbasis, eri_packed);
        if (nread) *nread = lines;
    });
}

// Packed AO integrals from a host array (for callers that already hold int_store%eri), same residency as the reader's.
int afesp_set_eri(afesp_ctx* ctx, int64_t nbasis, const double* eri_packed)
{
    return entry(ctx, [&](Context& cx) {
        if (nbasis <= 0 || nbasis > 1024 || !eri_packed) throw Error(1, "afesp_set_eri: bad arguments");
        ctx->in.upload_ao(cx, nbasis, eri_packed);
    });
}

// build_fock (src/hf.f90:349-385) on the resident packed AO integrals
int afesp_build_fock(afesp_ctx* ctx, int64_t nbasis, const double* density, const double* core_hamil, double* fock)
{
    return entry(ctx, [&](Context& cx) {
        if (!ctx->in.ao || ctx->in.ao_n != nbasis || !density || !core_hamil || !fock)
            throw Error(1, "afesp_build_fock: no AO integrals resident for this basis size (afesp_read_eri_text / afesp_set_eri)");
        const int64_t n2 = nbasis * nbasis;
        double* buf = cx.scratch("fock_io", 3 * n2);
        AFESP_HIP(hipMemcpyAsync(buf, density, sizeof(double) * n2, hipMemcpyHostToDevice, cx.stream));
        AFESP_HIP(hipMemcpyAsync(buf + n2, core_hamil, sizeof(double) * n2, hipMemcpyHostToDevice, cx.stream));
        int64_t L = 0;
        const double* u = ctx->in.half_unpacked(cx, nbasis, L);
        double* work = cx.scratch("fock_work", k_build_fock_work((int)nbasis));
        ctx->in.half_restamp(cx);
        k_build_fock(cx, buf + 2 * n2, buf + n2, buf, u, work, (int)nbasis, (int)L);
        AFESP_HIP(hipMemcpyAsync(fock, buf + 2 * n2, sizeof(double) * n2, hipMemcpyDeviceToHost, cx.stream));
        cx.sync();
    });
}

int afesp_write_fcidump(afesp_ctx* ctx, const char* path, int64_t nbasis, int64_t* nwritten)
{
    return entry(ctx, [&](Context& cx) {
        if (!ctx->in.mo || ctx->in.mo_n != nbasis || !path)
            throw Error(1, "afesp_write_fcidump: no MO integrals resident for this basis size (call afesp_ao2mo_mp2 first)");
        const int64_t lines = write_fcidump(cx, ctx->in, path, nbasis);
        if (nwritten) *nwritten = lines;
    });
}

// ---------------------------------------------------------------- the active space as a Hamiltonian on disk
int afesp_core_operator(afesp_ctx* ctx, int64_t nbasis, int64_t n_frozen_core, int64_t n_frozen_virt, const double* canon_coeff,
                        const double* core_hamil_ao, double* h_act, double* e_core)
{
    return entry(ctx, [&](Context& cx) {
        const int64_t n = nbasis, nfc = n_frozen_core, nfv = n_frozen_virt;
        if (n <= 0 || n > 1024 || !canon_coeff || !core_hamil_ao || !h_act || !e_core) throw Error(1, "afesp_core_operator: bad extents");
        if (nfc < 0 || nfv < 0) throw Error(1, "afesp_core_operator: negative number of frozen orbitals");
        if (nfc + nfv >= n) throw Error(1, "afesp_core_operator: no active orbital left");
        if (!ctx->in.mo || ctx->in.mo_n != n)
            throw Error(1, "afesp_core_operator: no MO integrals are resident for this basis size (call afesp_ao2mo_mp2 first, and "
                           "afesp_mo_window afterwards)");
        core_operator(cx, ctx->in, n, nfc, nfv, canon_coeff, core_hamil_ao, h_act, e_core);
    });
}

int afesp_ucore_operator(afesp_ctx* ctx, int64_t nbasis, int64_t n_frozen_core, int64_t n_frozen_virt, const double* coeff_a,
                         const double* coeff_b, const double* core_hamil_ao, double* h_act_a, double* h_act_b, double* e_core)
{
    return entry(ctx, [&](Context& cx) {
        const int64_t n = nbasis, nfc = n_frozen_core, nfv = n_frozen_virt;
        if (n <= 0 || n > 1024 || !coeff_a || !coeff_b || !core_hamil_ao || !h_act_a || !h_act_b || !e_core)
            throw Error(1, "afesp_ucore_operator: bad extents");
        if (nfc < 0 || nfv < 0) throw Error(1, "afesp_ucore_operator: negative number of frozen orbitals");
        if (nfc + nfv >= n) throw Error(1, "afesp_ucore_operator: no active orbital left");
        if (!ctx->in.uhf_aa || ctx->in.uhf_n != n)
            throw Error(1, "afesp_ucore_operator: no UHF MO integrals resident for this basis size (call afesp_ao2mo_ump2 first, and "
                           "afesp_umo_window afterwards)");
        ucore_operator(cx, ctx->in, n, nfc, nfv, coeff_a, coeff_b, core_hamil_ao, h_act_a, h_act_b, e_core);
    });
}

int afesp_write_fcidump_active(afesp_ctx* ctx, const char* path, int64_t n_act, int64_t nelec_act, int64_t ms2, const double* h_act,
                               double e_core_total, double threshold, int64_t* nwritten)
{
    return entry(ctx, [&](Context& cx) {
        if (!path || !h_act || n_act <= 0 || nelec_act < 0 || nelec_act > 2 * n_act || !(threshold >= 0.0))
            throw Error(1, "afesp_write_fcidump_active: bad arguments");
        if (!ctx->in.mo || ctx->in.mo_n != n_act)
            throw Error(1, "afesp_write_fcidump_active: no MO integrals resident for this number of orbitals (afesp_ao2mo_mp2 / "
                           "afesp_mo_window first)");
        const int64_t lines = write_fcidump_active(cx, ctx->in, path, n_act, nelec_act, ms2, h_act, e_core_total, threshold);
        if (nwritten) *nwritten = lines;
    });
}

int afesp_write_fcidump_uactive(afesp_ctx* ctx, const char* path, int64_t n_act, int64_t nalpha_act, int64_t nbeta_act, const double* h_act_a,
                                const double* h_act_b, double e_core_total, double threshold, int64_t* nwritten)
{
    return entry(ctx, [&](Context& cx) {
        if (!path || !h_act_a || !h_act_b || n_act <= 0 || nalpha_act < 0 || nbeta_act < 0 || nalpha_act > n_act || nbeta_act > n_act ||
            !(threshold >= 0.0))
            throw Error(1, "afesp_write_fcidump_uactive: bad arguments");
        if (!ctx->in.uhf_aa || ctx->in.uhf_n != n_act)
            throw Error(1, "afesp_write_fcidump_uactive: no UHF MO integrals resident for this number of orbitals (afesp_ao2mo_ump2 / "
                           "afesp_umo_window first)");
        const int64_t lines = write_fcidump_uactive(cx, ctx->in, path, n_act, nalpha_act, nbeta_act, h_act_a, h_act_b, e_core_total, threshold);
        if (nwritten) *nwritten = lines;
    });
}

// ---------------------------------------------------------------- a standard FCIDUMP as input
int afesp_fcidump_scan(const char* path, int64_t* norb, int64_t* nelec, int64_t* ms2, int* uhf, int64_t* nlines)
{
    try {
        return fcidump_scan(path, norb, nelec, ms2, uhf, nlines);
    } catch (const std::exception&) {
        return 1;
    }
}

int afesp_read_fcidump(afesp_ctx* ctx, const char* path, int64_t nbasis, int64_t nocc, double* h_mo, double* fock, double* levels,
                       double* e_core, double* e_ref, double* fock_offdiag, double* eri_mo_packed, int64_t* nread)
{
    return entry(ctx, [&](Context& cx) {
        if (!path) throw Error(1, "afesp_read_fcidump: path is NULL");
        if (nbasis <= 0 || nbasis > 1024 || nocc < 0 || nocc > nbasis) throw Error(1, "afesp_read_fcidump: bad extents");
        FcidumpResult r;
        r.h[0] = h_mo; r.fock[0] = fock; r.levels[0] = levels; r.eri[0] = eri_mo_packed;
        read_fcidump(cx, ctx->in, ctx->cc, path, nbasis, nocc, r);
        if (e_core) *e_core = r.e_core;
        if (e_ref) *e_ref = r.e_ref;
        if (fock_offdiag) *fock_offdiag = r.fock_offdiag;
        if (nread) *nread = r.nread;
    });
}

int afesp_read_fcidump_uhf(afesp_ctx* ctx, const char* path, int64_t nbasis, int64_t nalpha, int64_t nbeta, double* h_a, double* h_b,
                           double* fock_a, double* fock_b, double* levels_a, double* levels_b, double* e_core, double* e_ref,
                           double* fock_offdiag, double* eri_aa, double* eri_ab, double* eri_bb, int64_t* nread)
{
    return entry(ctx, [&](Context& cx) {
        if (!path) throw Error(1, "afesp_read_fcidump_uhf: path is NULL");
        if (nbasis <= 0 || nbasis > 1024 || nalpha < 0 || nbeta < 0 || nalpha > nbasis || nbeta > nbasis)
            throw Error(1, "afesp_read_fcidump_uhf: bad extents");
        FcidumpResult r;
        r.h[0] = h_a; r.h[1] = h_b; r.fock[0] = fock_a; r.fock[1] = fock_b; r.levels[0] = levels_a; r.levels[1] = levels_b;
        r.eri[0] = eri_aa; r.eri[1] = eri_bb; r.eri[2] = eri_ab;
        read_fcidump_uhf(cx, ctx->in, path, nbasis, nalpha, nbeta, r);
        if (e_core) *e_core = r.e_core;
        if (e_ref) *e_ref = r.e_ref;
        if (fock_offdiag) *fock_offdiag = r.fock_offdiag;
        if (nread) *nread = r.nread;
    });
}

// ---------------------------------------------------------------- restricted open-shell references
int afesp_mo_fock_ro(afesp_ctx* ctx, int64_t nbasis, int64_t nalpha, int64_t nbeta, const double* h_mo, double* fock_a, double* fock_b,
                     double* e_ref_elec)
{
    return entry(ctx, [&](Context& cx) {
        if (nbasis <= 0 || nbasis > 1024 || nalpha < 0 || nbeta < 0 || nalpha < nbeta || nalpha > nbasis || !h_mo || !fock_a || !fock_b ||
            !e_ref_elec)
            throw Error(1, "afesp_mo_fock_ro: bad extents or a NULL argument (need 0 <= nbeta <= nalpha <= nbasis)");
        if (!ctx->in.mo || ctx->in.mo_n != nbasis)
            throw Error(1, "afesp_mo_fock_ro: no packed MO integrals resident for this basis size (afesp_ao2mo_mp2 / afesp_read_fcidump / "
                           "afesp_read_fcidump_rohf)");
        *e_ref_elec = mo_fock_ro(cx, ctx->in, nbasis, nalpha, nbeta, h_mo, fock_a, fock_b);
    });
}

int afesp_read_fcidump_rohf(afesp_ctx* ctx, const char* path, int64_t nbasis, int64_t nalpha, int64_t nbeta, double* h_mo, double* fock_a,
                            double* fock_b, double* e_core, double* e_ref, double* fock_offdiag, double* eri_mo_packed, int64_t* nread)
{
    return entry(ctx, [&](Context& cx) {
        if (!path) throw Error(1, "afesp_read_fcidump_rohf: path is NULL");
        if (nbasis <= 0 || nbasis > 1024 || nalpha < 0 || nbeta < 0 || nalpha < nbeta || nalpha > nbasis)
            throw Error(1, "afesp_read_fcidump_rohf: bad extents (need 0 <= nbeta <= nalpha <= nbasis)");
        FcidumpResult r;
        r.h[0] = h_mo; r.fock[0] = fock_a; r.fock[1] = fock_b; r.eri[0] = eri_mo_packed;
        read_fcidump_rohf(cx, ctx->in, ctx->cc, path, nbasis, nalpha, nbeta, r);
        if (e_core) *e_core = r.e_core;
        if (e_ref) *e_ref = r.e_ref;
        if (fock_offdiag)
            for (int k = 0; k < 3; ++k) fock_offdiag[k] = r.fock_offdiag3[k];
        if (nread) *nread = r.nread;
    });
}

int afesp_mo_rotate_uhf(afesp_ctx* ctx, int64_t nbasis, const double* u_a, const double* u_b, double* eri_aa, double* eri_ab, double* eri_bb)
{
    return entry(ctx, [&](Context& cx) {
        if (nbasis <= 0 || nbasis > 1024 || !u_a || !u_b) throw Error(1, "afesp_mo_rotate_uhf: bad extents or a NULL rotation");
        mo_rotate_uhf(cx, ctx->in, nbasis, u_a, u_b, eri_aa, eri_ab, eri_bb);
    });
}

// ---------------------------------------------------------------- spin-orbital path
int afesp_ccsd_so_init(afesp_ctx* ctx, int64_t nbasis, int64_t nel, const double* eri_mo_packed, const double* canon_levels,
                       int diis_n_errmat, int flags)
{
    return entry(ctx, [&](Context& cx) {
        if (nbasis <= 0 || nbasis > 512 || nel <= 0 || nel >= 2 * nbasis) throw Error(1, "afesp_ccsd_so_init: bad extents");
        const double* src = ctx->in.mo;
        double* tmp = nullptr;
        if (eri_mo_packed) {
            tmp = cx.alloc(neri_of(nbasis));
            AFESP_HIP(hipMemcpyAsync(tmp, eri_mo_packed, sizeof(double) * neri_of(nbasis), hipMemcpyHostToDevice, cx.stream));
            src = tmp;
        } else if (!src || ctx->in.mo_n != nbasis) {
            throw Error(1, "afesp_ccsd_so_init: no MO integrals resident for this basis size (call afesp_ao2mo_mp2 first)");
        }
        cx.drop_scratch("ao2mo_");   // the AO->MO temporaries
        ctx->so_programs_reset();
        so_init(cx, ctx->so, (int)nbasis, (int)nel, src, canon_levels, diis_n_errmat, (flags & AFESP_SO_FOO_AS_PUBLISHED) != 0);
        ctx->so.amp_epoch = ++cx.amp_clock;
        if (tmp) cx.release(tmp);
    });
}

int afesp_ccsd_so_energy(afesp_ctx* ctx, double e_tol, double t_tol, double* energy, double* rms_sq, int* converged)
{
    return entry(ctx, [&](Context& cx) {
        if (!ctx->so.ready) throw Error(1, "afesp_ccsd_so_energy: call afesp_ccsd_so_init first");
        int conv = so_energy(cx, ctx->so, e_tol, t_tol);
        if (energy) *energy = ctx->so.energy;
        if (rms_sq) *rms_sq = ctx->so.rms;
        if (converged) *converged = conv;
    });
}

int afesp_ccsd_so_iterate(afesp_ctx* ctx, double e_tol, double t_tol, double* energy, double* rms_sq, int* converged)
{
    return entry(ctx, [&](Context& cx) {
        if (!ctx->so.ready) throw Error(1, "afesp_ccsd_so_iterate: call afesp_ccsd_so_init first");
        ctx->so.amp_epoch = ++cx.amp_clock;   // (the amplitudes may change: derived copies go stale)
        // (the levelled sequence of fused.h where the system is small enough for its products to be launch-bound: the big ones
        // keep their own kernels inside it)
        auto body = [&] {
            diis_save(cx, ctx->so);
            so_intermediates(cx, ctx->so);
            so_amplitudes(cx, ctx->so);
        };
        if (!(ctx->so.t2.size() <= ((int64_t)1 << 22) && fused_exec(cx, ctx->fused_so, body))) body();
        int conv = so_energy(cx, ctx->so, e_tol, t_tol);
        if (energy) *energy = ctx->so.energy;
        if (rms_sq) *rms_sq = ctx->so.rms;
        if (converged) *converged = conv;
    });
}

int afesp_ccsd_so_diis(afesp_ctx* ctx)
{
    return entry(ctx, [&](Context& cx) {
        if (!ctx->so.ready) throw Error(1, "afesp_ccsd_so_diis: call afesp_ccsd_so_init first");
        ctx->so.amp_epoch = ++cx.amp_clock;
        diis_update(cx, ctx->so);
    });
}

int afesp_ccsd_so_get_amplitudes(afesp_ctx* ctx, double* t1, double* t2)
{
    return entry(ctx, [&](Context& cx) {
        if (!ctx->so.ready) throw Error(1, "afesp_ccsd_so_get_amplitudes: no spin-orbital CCSD state");
        SOState& s = ctx->so;
        if (t1) AFESP_HIP(hipMemcpyAsync(t1, s.t1.d, sizeof(double) * s.t1.size(), hipMemcpyDeviceToHost, cx.stream));
        if (t2) AFESP_HIP(hipMemcpyAsync(t2, s.t2.d, sizeof(double) * s.t2.size(), hipMemcpyDeviceToHost, cx.stream));
        cx.sync();
    });
}

int afesp_ccsd_so_set_amplitudes(afesp_ctx* ctx, const double* t1, const double* t2)
{
    return entry(ctx, [&](Context& cx) {
        if (!ctx->so.ready) throw Error(1, "afesp_ccsd_so_set_amplitudes: no spin-orbital CCSD state");
        ctx->so.amp_epoch = ++cx.amp_clock;
        SOState& s = ctx->so;
        if (t1) AFESP_HIP(hipMemcpyAsync(s.t1.d, t1, sizeof(double) * s.t1.size(), hipMemcpyHostToDevice, cx.stream));
        if (t2) AFESP_HIP(hipMemcpyAsync(s.t2.d, t2, sizeof(double) * s.t2.size(), hipMemcpyHostToDevice, cx.stream));
        cx.sync();
    });
}

int afesp_ccsd_so_get_tensor(afesp_ctx* ctx, const char* name, double* out, int64_t capacity)
{
    return entry(ctx, [&](Context& cx) {
        if (!ctx->so.ready) throw Error(1, "afesp_ccsd_so_get_tensor: no spin-orbital CCSD state");
        SOState& s = ctx->so;
        if (!strcmp(name, "W_vvvv")) so_build_W_vvvv(cx, s);   // not formed by the iteration (so_ladder): built from the current t1 on request
        struct { const char* n; const Tensor* t; } tab[] = {
            {"F_vv", &s.F_vv}, {"F_oo", &s.F_oo}, {"F_ov", &s.F_ov}, {"W_oooo", &s.W_oooo}, {"W_vvvv", &s.W_vvvv},
            {"W_ovvo", &s.W_ovvo}, {"tau", &s.tau}, {"tau_tilde", &s.tau_t}, {"oovv", &s.oovv}, {"vvvv", &s.vvvv},
            {"t1", &s.t1}, {"t2", &s.t2}, {"f_ov", &s.f_ov}, {"f_oo", &s.f_oo}, {"f_vv", &s.f_vv}};
        for (auto& e : tab)
            if (!strcmp(e.n, name)) {
                if (!e.t->d) throw Error(1, std::string("afesp_ccsd_so_get_tensor: this state holds no ") + name + " (afesp_ccsd_uso_init_fock makes one that does)");
                if (e.t->size() > capacity) throw Error(1, std::string("afesp_ccsd_so_get_tensor: buffer too small for ") + name);
                AFESP_HIP(hipMemcpyAsync(out, e.t->d, sizeof(double) * e.t->size(), hipMemcpyDeviceToHost, cx.stream));
                cx.sync();
                return;
            }
        throw Error(1, std::string("afesp_ccsd_so_get_tensor: unknown tensor ") + name);
    });
}

int64_t afesp_ccsd_so_t_ntriples(int64_t nocc) { return so_triples_count((int)nocc); }

int afesp_ccsd_so_t(afesp_ctx* ctx, int64_t t_begin, int64_t t_end, double* e_t)
{
    return entry(ctx, [&](Context& cx) {
        const double e = so_triples(cx, ctx->so, t_begin, t_end);
        if (e_t) *e_t = e;
    });
}

// ---------------------------------------------------------------- open-shell (UHF-based) path
int afesp_build_fock_uhf(afesp_ctx* ctx, int64_t nbasis, const double* dens_a, const double* dens_b, const double* core_hamil,
                         double* fock_a, double* fock_b)
{
    return entry(ctx, [&](Context& cx) {
        if (!ctx->in.ao || ctx->in.ao_n != nbasis || !dens_a || !dens_b || !core_hamil || !fock_a || !fock_b)
            throw Error(1, "afesp_build_fock_uhf: no AO integrals resident for this basis size (afesp_read_eri_text / afesp_set_eri)");
        const int64_t n2 = nbasis * nbasis;
        double* buf = cx.scratch("fock_uio", 5 * n2);   // [ Da | Db | H | Fa | Fb ]
        AFESP_HIP(hipMemcpyAsync(buf, dens_a, sizeof(double) * n2, hipMemcpyHostToDevice, cx.stream));
        AFESP_HIP(hipMemcpyAsync(buf + n2, dens_b, sizeof(double) * n2, hipMemcpyHostToDevice, cx.stream));
        AFESP_HIP(hipMemcpyAsync(buf + 2 * n2, core_hamil, sizeof(double) * n2, hipMemcpyHostToDevice, cx.stream));
        // the half-unpacked integrals afesp_build_fock keeps (same buffer, same validity)
        int64_t L = 0;
        const double* u = ctx->in.half_unpacked(cx, nbasis, L);
        double* work = cx.scratch("fock_uwork", k_build_fock_uhf_work((int)nbasis));
        ctx->in.half_restamp(cx);
        k_build_fock_uhf(cx, buf + 3 * n2, buf + 4 * n2, buf + 2 * n2, buf, buf + n2, u, work, (int)nbasis, (int)L);
        AFESP_HIP(hipMemcpyAsync(fock_a, buf + 3 * n2, sizeof(double) * n2, hipMemcpyDeviceToHost, cx.stream));
        AFESP_HIP(hipMemcpyAsync(fock_b, buf + 4 * n2, sizeof(double) * n2, hipMemcpyDeviceToHost, cx.stream));
        cx.sync();
    });
}

int afesp_ao2mo_ump2(afesp_ctx* ctx, int64_t nbasis, int64_t nalpha, int64_t nbeta, const double* coeff_a, const double* coeff_b,
                     const double* levels_a, const double* levels_b, const double* eri_packed, double* eri_aa, double* eri_ab,
                     double* eri_bb, double* e_ump2)
{
    return entry(ctx, [&](Context& cx) {
        const int64_t n = nbasis, na = nalpha, nb = nbeta;
        if (n <= 0 || n > 1024 || na < 0 || nb < 0 || na > n || nb > n || na + nb <= 0 || !coeff_a || !coeff_b || !levels_a || !levels_b)
            throw Error(1, "afesp_ao2mo_ump2: bad extents");
        const double e2 = ao2mo_ump2(cx, ctx->in, n, na, nb, coeff_a, coeff_b, levels_a, levels_b, eri_packed, eri_aa, eri_ab, eri_bb);
        if (e_ump2) *e_ump2 = e2;
    });
}

int afesp_umo_window(afesp_ctx* ctx, int64_t nbasis, int64_t nalpha, int64_t nbeta, int64_t n_frozen_core, int64_t n_frozen_virt,
                     const double* levels_a, const double* levels_b, double* eri_aa, double* eri_ab, double* eri_bb, double* e_ump2)
{
    return entry(ctx, [&](Context& cx) {
        const int64_t n = nbasis, nfc = n_frozen_core, nfv = n_frozen_virt;
        if (n <= 0 || n > 1024 || nalpha < 0 || nbeta < 0 || nalpha > n || nbeta > n || !levels_a || !levels_b)
            throw Error(1, "afesp_umo_window: bad extents");
        if (nfc < 0 || nfv < 0) throw Error(1, "afesp_umo_window: negative number of frozen orbitals");
        // what afesp_ccsd_uso_init accepts for the active extents: a spin may be left without occupied (or without virtual) orbitals,
        // the two spins together keep at least one of each
        const int64_t na = n - nfc - nfv, oa = nalpha - nfc, ob = nbeta - nfc;
        if (na <= 0 || oa < 0 || ob < 0 || oa + ob <= 0) throw Error(1, "afesp_umo_window: no active occupied orbital left");
        if (oa > na || ob > na || oa + ob >= 2 * na) throw Error(1, "afesp_umo_window: no active virtual orbital left");
        if (!ctx->in.uhf_aa || ctx->in.uhf_n != n)
            throw Error(1, "afesp_umo_window: no UHF MO integrals resident for this basis size (call afesp_ao2mo_ump2 first; a window is "
                           "taken once)");
        if (na != n) ctx->in.window_uhf(cx, na, nfc);
        const double e2 = ump2_of_blocks(cx, ctx->in, levels_a + nfc, levels_b + nfc, oa, ob, eri_aa, eri_ab, eri_bb);
        if (e_ump2) *e_ump2 = e2;
    });
}

int afesp_ump2_vv_density(afesp_ctx* ctx, int64_t nbasis, int64_t nalpha, int64_t nbeta, int64_t n_frozen_core, const double* levels_a,
                          const double* levels_b, double* d_a, double* d_b, double* e_ump2)
{
    return entry(ctx, [&](Context& cx) {
        const int64_t n = nbasis, nfc = n_frozen_core;
        if (n <= 0 || n > 1024 || nalpha < 0 || nbeta < 0 || nalpha > n || nbeta > n || !levels_a || !levels_b || !d_a || !d_b)
            throw Error(1, "afesp_ump2_vv_density: bad extents");
        if (nfc < 0) throw Error(1, "afesp_ump2_vv_density: negative number of frozen orbitals");
        if (nalpha - nfc < 0 || nbeta - nfc < 0 || nalpha + nbeta - 2 * nfc <= 0)
            throw Error(1, "afesp_ump2_vv_density: no active occupied orbital left");
        if (!ctx->in.uhf_aa || ctx->in.uhf_n != n)
            throw Error(1, "afesp_ump2_vv_density: no UHF MO integrals resident for this basis size (call afesp_ao2mo_ump2 first, and "
                           "afesp_umo_window afterwards)");
        const double e2 = ump2_vv_density(cx, ctx->in, n, nalpha, nbeta, nfc, levels_a, levels_b, d_a, d_b);
        if (e_ump2) *e_ump2 = e2;
    });
}

int afesp_ccsd_uso_init(afesp_ctx* ctx, int64_t nbasis, int64_t nalpha, int64_t nbeta, const double* levels_a, const double* levels_b,
                        int diis_n_errmat)
{
    return entry(ctx, [&](Context& cx) {
        if (nbasis <= 0 || nbasis > 512 || nalpha < 0 || nbeta < 0 || nalpha > nbasis || nbeta > nbasis || nalpha + nbeta <= 0 ||
            nalpha + nbeta >= 2 * nbasis || !levels_a || !levels_b)
            throw Error(1, "afesp_ccsd_uso_init: bad extents");
        if (!ctx->in.uhf_aa || ctx->in.uhf_n != nbasis)
            throw Error(1, "afesp_ccsd_uso_init: no UHF MO integrals resident for this basis size (call afesp_ao2mo_ump2 first)");
        const int64_t o = nalpha + nbeta, v = 2 * nbasis - o;
        cx.drop_scratch("ao2mo_");   // the AO->MO temporaries
        ctx->so_programs_reset();
        so_free(cx, ctx->so);        // (a previous state's memory counts as available)
        // against the free device memory plus the context's idle blocks: the resident UHF (and RHF) integral blocks are in use
        size_t free_b = 0, total_b = 0;
        AFESP_HIP(hipMemGetInfo(&free_b, &total_b));
        if (so_state_bytes(o, v, diis_n_errmat) > 0.9 * ((double)free_b + (double)cx.arena.idle_bytes))
            throw Error(1, "afesp_ccsd_uso_init: the dense spin-orbital state of this system does not fit the free device memory");
        so_init_uhf(cx, ctx->so, (int)nbasis, (int)nalpha, (int)nbeta, ctx->in.uhf_aa, ctx->in.uhf_bb, ctx->in.uhf_ab, levels_a, levels_b, diis_n_errmat);
        ctx->so.amp_epoch = ++cx.amp_clock;
    });
}

int afesp_ccsd_uso_init_fock(afesp_ctx* ctx, int64_t nbasis, int64_t nalpha, int64_t nbeta, const double* fock_a, const double* fock_b,
                             int diis_n_errmat, double* e_mp2)
{
    return entry(ctx, [&](Context& cx) {
        if (nbasis <= 0 || nbasis > 512 || nalpha < 0 || nbeta < 0 || nalpha > nbasis || nbeta > nbasis || nalpha + nbeta <= 0 ||
            nalpha + nbeta >= 2 * nbasis || !fock_a || !fock_b)
            throw Error(1, "afesp_ccsd_uso_init_fock: bad extents");
        if (!ctx->in.uhf_aa || ctx->in.uhf_n != nbasis)
            throw Error(1, "afesp_ccsd_uso_init_fock: no UHF MO integrals resident for this basis size (call afesp_mo_rotate_uhf or "
                           "afesp_ao2mo_ump2 first)");
        const int64_t o = nalpha + nbeta, v = 2 * nbasis - o;
        cx.drop_scratch("ao2mo_");   // the transform's temporaries
        ctx->so_programs_reset();
        so_free(cx, ctx->so);        // (a previous state's memory counts as available)
        size_t free_b = 0, total_b = 0;
        AFESP_HIP(hipMemGetInfo(&free_b, &total_b));
        if (so_state_bytes(o, v, diis_n_errmat) > 0.9 * ((double)free_b + (double)cx.arena.idle_bytes))
            throw Error(1, "afesp_ccsd_uso_init_fock: the dense spin-orbital state of this system does not fit the free device memory");
        const double e2 = so_init_fock(cx, ctx->so, (int)nbasis, (int)nalpha, (int)nbeta, ctx->in.uhf_aa, ctx->in.uhf_bb, ctx->in.uhf_ab, fock_a,
                                       fock_b, diis_n_errmat);
        ctx->so.amp_epoch = ++cx.amp_clock;
        if (e_mp2) *e_mp2 = e2;
    });
}

// ---------------------------------------------------------------- operator layer on host arrays
int afesp_contract(afesp_ctx* ctx, double alpha, const double* A, const char* la, const int64_t* dimsA, const double* B,
                   const char* lb, const int64_t* dimsB, double beta, double* C, const char* lc, const int64_t* dimsC,
                   int force_split, int force_tm, int force_tn)
{
    return entry(ctx, [&](Context& cx) {
        auto mk = [&](const char* l, const int64_t* dims) {
            Tensor t;
            t.rank = (int)strlen(l);
            if (t.rank > 6) throw Error(1, "afesp_contract: rank > 6");
            int64_t s = 1;
            for (int i = 0; i < t.rank; ++i) {
                t.dim[i] = dims[i];
                t.stride[i] = s;
                s *= dims[i];
            }
            t.d = cx.alloc(s);
            return t;
        };
        Tensor tA = mk(la, dimsA), tB = mk(lb, dimsB), tC = mk(lc, dimsC);
        AFESP_HIP(hipMemcpyAsync(tA.d, A, sizeof(double) * tA.size(), hipMemcpyHostToDevice, cx.stream));
        AFESP_HIP(hipMemcpyAsync(tB.d, B, sizeof(double) * tB.size(), hipMemcpyHostToDevice, cx.stream));
        AFESP_HIP(hipMemcpyAsync(tC.d, C, sizeof(double) * tC.size(), hipMemcpyHostToDevice, cx.stream));
        try {
            contract(cx, alpha, tA, la, tB, lb, beta, tC, lc, 1, nullptr, nullptr, nullptr, force_split, force_tm, force_tn);
        } catch (...) {   // (a refused product: the copies above still read the caller's arrays, and the three blocks go back)
            (void)hipStreamSynchronize(cx.stream);
            cx.release(tA.d); cx.release(tB.d); cx.release(tC.d);
            throw;
        }
        AFESP_HIP(hipMemcpyAsync(C, tC.d, sizeof(double) * tC.size(), hipMemcpyDeviceToHost, cx.stream));
        cx.sync();
        cx.release(tA.d); cx.release(tB.d); cx.release(tC.d);
    });
}

int afesp_gemm(afesp_ctx* ctx, char transA, char transB, int64_t m, int64_t n, int64_t k, double alpha, const double* A,
               const double* B, double beta, double* C)
{
    // dgemm_wrapper (linalg.fpp:58-89): leading dimensions follow from the logical shapes
    const bool ta = (transA == 'T' || transA == 't'), tb = (transB == 'T' || transB == 't');
    int64_t dA[2] = {ta ? k : m, ta ? m : k}, dB[2] = {tb ? n : k, tb ? k : n}, dC[2] = {m, n};
    return afesp_contract(ctx, alpha, A, ta ? "km" : "mk", dA, B, tb ? "nk" : "kn", dB, beta, C, "mn", dC, 0, 0, 0);
}

int afesp_permute4(afesp_ctx* ctx, const int64_t dims[4], const char order[4], const double* in, double* out, int has_beta, double beta)
{
    return entry(ctx, [&](Context& cx) {
        // omp_reshape (linalg.fpp:136-147): character d of `order` names the input index in output position d
        const char names[5] = "ijkl";
        char lo[5] = {0, 0, 0, 0, 0};
        int64_t od[4];
        for (int d = 0; d < 4; ++d) {
            int p = order[d] - '1';
            if (p < 0 || p > 3) throw Error(1, "afesp_permute4: bad order string");
            lo[d] = names[p];
            od[d] = dims[p];
        }
        Tensor tin = cx.tensor({dims[0], dims[1], dims[2], dims[3]}), tout = cx.tensor({od[0], od[1], od[2], od[3]});
        AFESP_HIP(hipMemcpyAsync(tin.d, in, sizeof(double) * tin.size(), hipMemcpyHostToDevice, cx.stream));
        if (has_beta) AFESP_HIP(hipMemcpyAsync(tout.d, out, sizeof(double) * tout.size(), hipMemcpyHostToDevice, cx.stream));
        permute_add(cx, 1.0, tin, names, has_beta ? beta : 0.0, tout, lo);
        AFESP_HIP(hipMemcpyAsync(out, tout.d, sizeof(double) * tout.size(), hipMemcpyDeviceToHost, cx.stream));
        cx.sync();
        cx.release(tin.d); cx.release(tout.d);
    });
}

// ---------------------------------------------------------------- synthetic inputs generated in HBM
int afesp_synthetic_init(afesp_ctx* ctx, int64_t nocc, int64_t nvirt, double scale, uint64_t seed, int diis_n_errmat)
{
    return entry(ctx, [&](Context& cx) {
        const int64_t n = nocc + nvirt, ne = neri_of(n);
        if (nocc <= 0 || nvirt <= 0 || n > 1024) throw Error(1, "afesp_synthetic_init: bad extents");
        std::vector<double> e((size_t)n);
        for (int64_t i = 0; i < nocc; ++i) e[i] = -2.0 + (nocc > 1 ? (double)i / (double)(nocc - 1) : 0.0);
        for (int64_t a = 0; a < nvirt; ++a) e[nocc + a] = 1.0 + (nvirt > 1 ? 2.0 * (double)a / (double)(nvirt - 1) : 0.0);
        double* packed = cx.alloc(ne);
        AFESP_KLAUNCH(synth_packed_kernel, dim3(4096), dim3(256), 0, cx.stream, packed, ne, scale, seed);
        AFESP_HIP(hipGetLastError());
        if (!ccsd_can_reinit(ctx->cc, (int)nocc, (int)nvirt, diis_n_errmat)) ctx->cc_programs_reset();
        else ctx->graph_cc.reset();
        ccsd_init(cx, ctx->cc, (int)nocc, (int)nvirt, packed, e.data(), diis_n_errmat);
        if (ctx->cc.v_vvvv.d) { cx.release(packed); ctx->cc.eri_src = nullptr; }
        else ctx->cc.eri_own = packed;   // kept for ccsd_need_vvvv
    });
}

// Hashed packed AO integrals left on the device as afesp_read_eri_text would leave them (AO->MO timing: bench.py)
int afesp_synthetic_ao(afesp_ctx* ctx, int64_t nbasis, double scale, uint64_t seed)
{
    return entry(ctx, [&](Context& cx) {
        if (nbasis <= 0 || nbasis > 1024) throw Error(1, "afesp_synthetic_ao: bad extents");
        double* ao = ctx->in.adopt_ao(cx, nbasis);
        AFESP_KLAUNCH(synth_packed_kernel, dim3(4096), dim3(256), 0, cx.stream, ao, neri_of(nbasis), scale, seed);
        AFESP_HIP(hipGetLastError());
        cx.sync();
    });
}

// Floating-point operations of one particle-particle ladder as this context evaluates it (plain a <= b form or the
// symmetric/antisymmetric pair form, ccsd.hip)
int afesp_ccsd_pp_ladder_flop(afesp_ctx* ctx, double* flop)
{
    return entry(ctx, [&](Context& cx) {
        if (!ctx->cc.ready) throw Error(1, "afesp_ccsd_pp_ladder_flop: no CCSD state");
        const double O = ctx->cc.o, V = ctx->cc.v, ps = V * (V + 1) / 2, pa = V * (V - 1) / 2;
        if (flop) *flop = ctx->cc.pp_sym ? 2.0 * (O * (O + 1) / 2 * ps * ps + O * (O - 1) / 2 * pa * pa) : 2.0 * O * O * V * V * ps;
    });
}

// Floating-point operations of one CCSD iteration as this context evaluates it: SURVEY.md 8(d)'s sum over the contraction sites,
// with the pp-ladder and the t2 x <ef|ia> product counted in the form they are executed (plain, a <= b, or over pair indices)
int afesp_ccsd_iteration_flop(afesp_ctx* ctx, double* flop)
{
    return entry(ctx, [&](Context& cx) {
        if (!ctx->cc.ready) throw Error(1, "afesp_ccsd_iteration_flop: no CCSD state");
        const double O = ctx->cc.o, V = ctx->cc.v, ps = V * (V + 1) / 2, pa = V * (V - 1) / 2, os = O * (O + 1) / 2, oa = O * (O - 1) / 2;
        const bool sym = ctx->cc.pp_sym;
        const double pp = sym ? 2.0 * (os * ps * ps + oa * pa * pa) : 2.0 * O * O * V * V * ps;
        const double ooov = sym ? 2.0 * O * V * (os * ps + oa * pa) : 2.0 * O * O * O * V * V * V;
        const double o3v3 = O * O * O * V * V * V;
        // large-system path (round 5): c <ij|ef> -> I_oooo and the hole-hole ladder over pair indices (the latter inside the pp-ladder's
        // products), and the bare t(i,e) <ab|ej> term as a copy of x_voov instead of a third o^2 v^3 product
        const bool large = !ccsd_uses_lanes(ctx->cc);
        const double oooo = (sym && large) ? 4.0 * (os * os * ps + oa * oa * pa) : 2.0 * O * O * O * O * V * V;
        // (... and asym(m,i,e,f) <ef|ma> -> r1 as a trace of the pair-form t2 <ef|ia> product: one more o^2 v^3 product that is not executed)
        const double o2v3 = large ? (sym ? 14.0 : 16.0) : 18.0;
        if (flop)
            *flop = pp + ooov + 12.0 * o3v3 + oooo + 2.0 * O * O * O * O * V + o2v3 * O * O * V * V * V +
                    2.0 * O * V * V * V + 14.0 * O * O * O * V * V;
    });
}

int afesp_bench_stream(afesp_ctx* ctx, int64_t n, int reps, double* ms_per_launch)
{
    return entry(ctx, [&](Context& cx) {
        double* x = cx.scratch("bench_x", n);
        double* y = cx.scratch("bench_y", n);
        k_fill(cx, x, n, 1.0);
        k_fill(cx, y, n, 2.0);
        const double ms = time_on_stream(cx, reps, [&] { k_axpby(cx, y, 0.5, x, 0.25, n); });
        if (ms_per_launch) *ms_per_launch = ms;
    });
}

int afesp_profile(afesp_ctx* ctx, int enable, double out[8])
{
    return entry(ctx, [&](Context& cx) {
        if (out) {
            out[0] = cx.prof_gemm_ms; out[1] = (double)cx.prof_gemm_launches; out[2] = cx.prof_gemm_flop;
            out[3] = cx.prof_orbit_ms; out[4] = (double)cx.prof_orbit_launches; out[5] = cx.prof_orbit_bytes;
            out[6] = cx.prof_gemm_flop_padded; out[7] = (double)cx.prof_gemm_kind;
        }
        cx.prof = enable != 0;
        cx.prof_gemm_ms = cx.prof_gemm_flop = cx.prof_gemm_flop_padded = cx.prof_orbit_ms = cx.prof_orbit_bytes = 0.0;
        cx.prof_gemm_launches = cx.prof_orbit_launches = 0;
    });
}

int afesp_set_tuning(int group_m, int force_tm, int force_tn, int force_split)
{
    g_allow_wide = !(group_m & 0x10000); g_dbg = (group_m >> 17) & 7; group_m &= 0xffff;
    g_group_m = group_m; g_force_tm = force_tm; g_force_tn = force_tn; g_force_split = force_split;
    return 0;
}

// Device-only timing of one labelled contraction on hashed operands (tuning / roofline measurements).
int afesp_bench_contract(afesp_ctx* ctx, const char* la, const int64_t* dimsA, const char* lb, const int64_t* dimsB,
                         const char* lc, const int64_t* dimsC, int reps, double* ms_per_launch)
{
    return entry(ctx, [&](Context& cx) {
        auto mk = [&](const char* l, const int64_t* dims, uint64_t seed) {
            Tensor t;
            t.rank = (int)strlen(l);
            int64_t s = 1;
            for (int i = 0; i < t.rank; ++i) { t.dim[i] = dims[i]; t.stride[i] = s; s *= dims[i]; }
            t.d = cx.alloc(s);
            AFESP_KLAUNCH(synth_packed_kernel, dim3(4096), dim3(256), 0, cx.stream, t.d, s, 1.0, seed);
            return t;
        };
        Tensor tA = mk(la, dimsA, 1), tB = mk(lb, dimsB, 2), tC = mk(lc, dimsC, 3);
        const double ms = time_on_stream(cx, reps, [&] { contract(cx, 1.0, tA, la, tB, lb, 0.0, tC, lc); });
        if (ms_per_launch) *ms_per_launch = ms;
        cx.release(tA.d); cx.release(tB.d); cx.release(tC.d);
    });
}

int afesp_time_pp_ladder(afesp_ctx* ctx, int reps, double* ms_per_launch)
{
    return entry(ctx, [&](Context& cx) {
        if (!ctx->cc.ready) throw Error(1, "afesp_time_pp_ladder: no CCSD state");
        const double ms = time_on_stream(cx, reps, [&] { ccsd_pp_ladder(cx, ctx->cc); });
        if (ms_per_launch) *ms_per_launch = ms;
    });
}

// ---------------------------------------------------------------- multi-GPU: the sum over ranks (comm.h)
int afesp_device_count(void)
{
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) { (void)hipGetLastError(); return 0; }
    return n;
}

int afesp_comm_unique_id(char id_out[128])
{
    if (!id_out) return 1;
    try {
        comm_unique_id(id_out);
        return 0;
    } catch (const Error& e) {
        return e.code ? e.code : 1;
    } catch (...) {
        return 1;
    }
}

int afesp_comm_init(afesp_ctx* ctx, int rank, int world, int transport, const char* bootstrap_path, const char* unique_id)
{
    return entry(ctx, [&](Context& cx) {
        if (cx.comm) throw Error(1, "afesp_comm_init: this context already has a communicator");
        cx.comm = comm_create(cx, rank, world, transport, bootstrap_path, unique_id);
        ctx->cc_programs_reset();   // a captured iteration does not contain the rank split
    });
}

int afesp_comm_destroy(afesp_ctx* ctx)
{
    return entry(ctx, [&](Context& cx) {
        cx.sync();
        comm_destroy(cx.comm);
        cx.comm = nullptr;
        ctx->cc_programs_reset();
    });
}

int afesp_allreduce_sum(afesp_ctx* ctx, double* inout, int64_t n)
{
    return entry(ctx, [&](Context& cx) {
        if (n < 0 || (n > 0 && !inout)) throw Error(1, "afesp_allreduce_sum: bad arguments");
        if (!cx.comm) return;   // single rank: the sum over one rank
        comm_allreduce_host(cx, cx.comm, inout, n);
    });
}

int afesp_ccsd_is_split(afesp_ctx* ctx, int* split)
{
    return entry(ctx, [&](Context& cx) {
        if (!ctx->cc.ready || !split) throw Error(1, "afesp_ccsd_is_split: no CCSD state");
        ccsd_refresh_sharding(cx, ctx->cc);
        *split = ctx->cc.sharded ? 1 : 0;
    });
}

int afesp_ccsd_set_fused(afesp_ctx* ctx, int mode)
{
    return entry(ctx, [&](Context& cx) {
        if (mode < -1 || mode > 1) throw Error(1, "afesp_ccsd_set_fused: mode is -1 (environment), 0 (call by call) or 1 (launch-fused)");
        cx.fused_mode = mode;
    });
}

int afesp_ccsd_iteration_launches(afesp_ctx* ctx, int* launches)
{
    return entry(ctx, [&](Context& cx) {
        if (!launches) throw Error(1, "afesp_ccsd_iteration_launches: null argument");
        *launches = fused_launches(ctx->fused_iter.prog);
    });
}

int afesp_ccsd_set_split(afesp_ctx* ctx, int mode)
{
    return entry(ctx, [&](Context& cx) {
        if (mode < -1 || mode > 1) throw Error(1, "afesp_ccsd_set_split: mode is -1 (environment), 0 (replicas) or 1 (split)");
        cx.cc_split_mode = mode;
    });
}

int afesp_ccsd_t_block_size(afesp_ctx* ctx, int64_t nocc, int64_t nvirt, int cr, int* block_size)
{
    return entry(ctx, [&](Context& cx) {
        if (nocc < 1 || nvirt < 1 || !block_size) throw Error(1, "afesp_ccsd_t_block_size: bad arguments");
        *block_size = triples_block_size((int)nocc, (int)nvirt, cr != 0);
    });
}

// diagnostic builds of the GEMM kernel (AFESP_GETT_VARIANT bit 64): the per-wave cycle stamps of the last launch
int afesp_debug_stamps(unsigned long long* out, int n)
{
    knobs_refresh();
    if (n < 0) return triples_read_orbit_stamps(out, -n) == hipSuccess ? 0 : 1;   // the (T) orbit kernel's phase sums
    if (knobs().stamps_grouped) return gett_read_stamps_grouped(out, n) == hipSuccess ? 0 : 1;
    return gett_read_stamps(out, n) == hipSuccess ? 0 : 1;
}

// which kernel took the products of this context so far (tests: a shape that should stream did, the LDS-DMA GEMM ran with 96-row tiles)
int afesp_test_ring_path(int64_t nocc, int64_t nvirt)
{
    knobs_refresh();
    CCState s;
    s.o = (int)nocc;
    s.v = (int)nvirt;
    return ring_tg_applies(s) ? 1 : 0;
}

uint64_t afesp_first_use_count(void) { return first_use_count().load(std::memory_order_relaxed); }

int afesp_launch_counts(afesp_ctx* ctx, uint64_t out[4])
{
    return entry(ctx, [&](Context& cx) {
        out[0] = cx.n_tall; out[1] = cx.n_gett; out[2] = cx.tg.launches; out[3] = cx.tg.launches_mixed;
    });
}

// device arena of the context: {driver allocations so far, requests served from idle blocks, idle bytes, live bytes}
int afesp_arena_stats(afesp_ctx* ctx, double out[4])
{
    return entry(ctx, [&](Context& cx) {
        const Arena& a = cx.arena;
        size_t live = 0;
        for (auto& kv : a.live) live += kv.second;
        out[0] = (double)a.driver_calls; out[1] = (double)a.reuse_hits; out[2] = (double)a.idle_bytes; out[3] = (double)live;
    });
}

int afesp_test_inject(afesp_ctx* ctx, int what)
{
    return entry(ctx, [&](Context& cx) { cx.test_throw = what; });
}

}  // extern "C"
