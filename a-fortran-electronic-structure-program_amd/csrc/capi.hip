// capi.hip -- extern "C" boundary (include/afesp.h): argument checks and one call each into the layers behind it (the integral layer:
// integrals.h; the drivers of the two CCSD solvers: solver.h), and the synthetic-input generators.
#include <atomic>
#include <chrono>
#include <mutex>
#include <cstdio>
#include <cstring>
#include <thread>
#include <vector>

#include "../../include/afesp.h"
#include "integrals.h"
#include "solver.h"
#include "density2_so.h"
#include "relax_so.h"
#include "eom_ipea_so.h"
#include "eom_ipea_t_so.h"
#include "response_so.h"
#include "davidson_test.h"
#include "small_eig.h"
#include "comm.h"
#include "tall.h"

using namespace afesp;

struct afesp_ctx {
    Context cx;
    Solver sv;      // the two CCSD solver states and their compiled programs (solver.h)
    Integrals in;   // the resident AO / MO integrals (integrals.h)
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

// what an energy evaluation or an iteration reports, into the caller's optional outputs
void report(const StepResult& r, double* energy, double* rms_sq, int* converged)
{
    if (energy) *energy = r.energy;
    if (rms_sq) *rms_sq = r.rms;
    if (converged) *converged = r.converged;
}

// what a Davidson step reports, for the iterate entry points
void davidson_report(const Davidson& E, int conv, double* omega, double* resnorm, int* flags, int* nsigma, int* converged)
{
    for (int k = 0; k < E.nroots; ++k) {
        if (omega) omega[k] = E.omega[k];
        if (resnorm) resnorm[k] = E.resnorm[k];
        if (flags) flags[k] = E.flags[k];
    }
    if (nsigma) *nsigma = E.nsigma;
    if (converged) *converged = conv;
}

// ---- the EOM-CCSD eigenproblems: EE, EE left, IP and EA on one driver (eom_so.h).  An entry point is its name and its kind; those of the
// ipea family give their sector instead (and EOM_KINDS for the kind, EOM_KIND_IP_LEFT for the left side of either sector), which is checked
// first, as ever, and chooses the kind.
// call(cx, state, kind) does the work: the driver's function with the entry point's own arguments, or the step and its report.
template <class Call>
int eom_call(afesp_ctx* ctx, const char* who, EomKind kind, const int* sector, Call&& call)
{
    return entry(ctx, [&](Context& cx) {
        if (sector && !so_eom_sector_ok(*sector)) throw Error(1, std::string(who) + ": sector must be AFESP_EOM_IP (1) or AFESP_EOM_EA (2)");
        if (sector) kind = so_eom_kind_of_sector(*sector, kind == EOM_KIND_IP_LEFT);
        call(cx, ctx->sv.need_so((std::string(who) + ": no spin-orbital CCSD state").c_str()).so, kind);
    });
}

template <class... A, class... B>
int eom_entry(afesp_ctx* ctx, const char* who, EomKind kind, const int* sector, void (*driver)(Context&, SOState&, EomKind, A...), B... args)
{
    return eom_call(ctx, who, kind, sector, [&](Context& cx, SOState& so, EomKind k) { driver(cx, so, k, args...); });
}

int eom_iterate_entry(afesp_ctx* ctx, const char* who, EomKind kind, const int* sector, double tol, double* omega, double* resnorm,
                      int* flags, int* nsigma, int* converged)
{
    return eom_call(ctx, who, kind, sector, [&](Context& cx, SOState& so, EomKind k) {
        if (!(tol > 0.0)) throw Error(1, std::string(who) + ": tol must be positive");
        const int conv = so_eom_iterate(cx, so, k, tol);
        davidson_report(so.eom[k]->d, conv, omega, resnorm, flags, nsigma, converged);
    });
}

}  // namespace

extern "C" {

int afesp_version(void) { return 8; }
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
    davidson_test_destroy(ctx->cx);
    ctx->sv.destroy(ctx->cx);
    comm_destroy(ctx->cx.comm);
    ctx->cx.comm = nullptr;
    delete ctx;
}

const char* afesp_last_error(const afesp_ctx* ctx) { return ctx ? ctx->cx.last_error.c_str() : "null context"; }

int afesp_ao2mo_mp2(afesp_ctx* ctx, int64_t nbasis, int64_t nocc, const double* canon_coeff, const double* canon_levels,
                    const double* eri_packed, double* eri_mo_packed, double* e_mp2)
{
    return entry(ctx, [&](Context& cx) {
        if (nbasis <= 0 || nocc <= 0 || nbasis - nocc <= 0 || nbasis > 1024) throw Error(1, "afesp_ao2mo_mp2: bad extents");
        const double emp2 = ao2mo_mp2(cx, ctx->in, ctx->sv, nbasis, nocc, canon_coeff, canon_levels, eri_packed, eri_mo_packed);
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
        const double emp2 = mo_window(cx, ctx->in, ctx->sv, n, nocc, nfc, nfv, canon_levels, eri_mo_packed, eri_act);
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
        if (!eri_mo_packed && (!ctx->in.mo || ctx->in.mo_n != n))
            throw Error(1, "afesp_ccsd_init: no MO integrals resident for this basis size (call afesp_ao2mo_mp2 first)");
        ctx->sv.init(cx, (int)nocc, (int)nvirt, eri_mo_packed, ctx->in.mo, false, canon_levels, diis_n_errmat);
    });
}

int afesp_ccsd_energy(afesp_ctx* ctx, double e_tol, double t_tol, double* energy, double* rms_sq, int* converged)
{
    return entry(ctx, [&](Context& cx) {
        report(ctx->sv.need_cc("afesp_ccsd_energy: call afesp_ccsd_init first").energy(cx, e_tol, t_tol), energy, rms_sq, converged);
    });
}

int afesp_ccsd_update_intermediates(afesp_ctx* ctx)
{
    return entry(ctx, [&](Context& cx) { ctx->sv.need_cc("call afesp_ccsd_init first").update_intermediates(cx); });
}
int afesp_ccsd_update_amplitudes(afesp_ctx* ctx)
{
    return entry(ctx, [&](Context& cx) { ctx->sv.need_cc("call afesp_ccsd_init first").update_amplitudes(cx); });
}

int afesp_ccsd_iterate(afesp_ctx* ctx, double e_tol, double t_tol, double* energy, double* rms_sq, int* converged)
{
    return entry(ctx, [&](Context& cx) {
        report(ctx->sv.need_cc("afesp_ccsd_iterate: call afesp_ccsd_init first").iterate(cx, e_tol, t_tol), energy, rms_sq, converged);
    });
}

int afesp_ccsd_diis(afesp_ctx* ctx)
{
    return entry(ctx, [&](Context& cx) { ctx->sv.need_cc("afesp_ccsd_diis: call afesp_ccsd_init first").diis(cx); });
}

int afesp_ccsd_solve(afesp_ctx* ctx, int maxiter, double e_tol, double t_tol, double* iter_energy, double* iter_rms_sq, int* niter)
{
    return entry(ctx, [&](Context& cx) {
        const int result = ctx->sv.need_cc("afesp_ccsd_solve: call afesp_ccsd_init first").solve(cx, maxiter, e_tol, t_tol, iter_energy, iter_rms_sq);
        if (niter) *niter = result;
    });
}

int afesp_ccsd_get_amplitudes(afesp_ctx* ctx, double* t1, double* t2)
{
    return entry(ctx, [&](Context& cx) { ctx->sv.need_cc("afesp_ccsd_get_amplitudes: no CCSD state").get_amplitudes(cx, t1, t2); });
}

int afesp_ccsd_set_amplitudes(afesp_ctx* ctx, const double* t1, const double* t2)
{
    return entry(ctx, [&](Context& cx) { ctx->sv.need_cc("afesp_ccsd_set_amplitudes: no CCSD state").set_amplitudes(cx, t1, t2); });
}

int afesp_ccsd_get_tensor(afesp_ctx* ctx, const char* name, double* out, int64_t capacity)
{
    return entry(ctx, [&](Context& cx) { ctx->sv.need_cc("afesp_ccsd_get_tensor: no CCSD state").fetch_tensor(cx, name, out, capacity); });
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
    return entry(ctx, [&](Context& cx) { ccsd_triples(cx, ctx->sv.cc, t_begin, t_end, out); });
}

int afesp_ccsd_t_plain(afesp_ctx* ctx, int64_t t_begin, int64_t t_end, double out[2])
{
    return entry(ctx, [&](Context& cx) { ccsd_triples(cx, ctx->sv.cc, t_begin, t_end, out, false, false); });
}

int afesp_ccsd_cr_intermediates(afesp_ctx* ctx)
{
    return entry(ctx, [&](Context& cx) { ctx->sv.cr_intermediates(cx); });
}

int afesp_ccsd_t_cr(afesp_ctx* ctx, int64_t t_begin, int64_t t_end, double out[6])
{
    return entry(ctx, [&](Context& cx) { ccsd_triples(cx, ctx->sv.cc, t_begin, t_end, out, true); });
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
        build_fock(cx, ctx->in, nbasis, density, core_hamil, fock);
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
        read_fcidump(cx, ctx->in, ctx->sv, path, nbasis, nocc, r);
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
        read_fcidump_rohf(cx, ctx->in, ctx->sv, path, nbasis, nalpha, nbeta, r);
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
        if (!eri_mo_packed && (!ctx->in.mo || ctx->in.mo_n != nbasis))
            throw Error(1, "afesp_ccsd_so_init: no MO integrals resident for this basis size (call afesp_ao2mo_mp2 first)");
        ctx->sv.so_init_packed(cx, (int)nbasis, (int)nel, eri_mo_packed, ctx->in.mo, canon_levels, diis_n_errmat,
                               (flags & AFESP_SO_FOO_AS_PUBLISHED) != 0);
    });
}

int afesp_ccsd_so_energy(afesp_ctx* ctx, double e_tol, double t_tol, double* energy, double* rms_sq, int* converged)
{
    return entry(ctx, [&](Context& cx) {
        report(ctx->sv.need_so("afesp_ccsd_so_energy: call afesp_ccsd_so_init first").so_energy_step(cx, e_tol, t_tol), energy, rms_sq, converged);
    });
}

int afesp_ccsd_so_iterate(afesp_ctx* ctx, double e_tol, double t_tol, double* energy, double* rms_sq, int* converged)
{
    return entry(ctx, [&](Context& cx) {
        report(ctx->sv.need_so("afesp_ccsd_so_iterate: call afesp_ccsd_so_init first").so_iterate(cx, e_tol, t_tol), energy, rms_sq, converged);
    });
}

int afesp_ccsd_so_diis(afesp_ctx* ctx)
{
    return entry(ctx, [&](Context& cx) { ctx->sv.need_so("afesp_ccsd_so_diis: call afesp_ccsd_so_init first").so_diis(cx); });
}

int afesp_ccsd_so_get_amplitudes(afesp_ctx* ctx, double* t1, double* t2)
{
    return entry(ctx, [&](Context& cx) { ctx->sv.need_so("afesp_ccsd_so_get_amplitudes: no spin-orbital CCSD state").so_get_amplitudes(cx, t1, t2); });
}

int afesp_ccsd_so_set_amplitudes(afesp_ctx* ctx, const double* t1, const double* t2)
{
    return entry(ctx, [&](Context& cx) { ctx->sv.need_so("afesp_ccsd_so_set_amplitudes: no spin-orbital CCSD state").so_set_amplitudes(cx, t1, t2); });
}

int afesp_ccsd_so_get_tensor(afesp_ctx* ctx, const char* name, double* out, int64_t capacity)
{
    return entry(ctx, [&](Context& cx) { ctx->sv.need_so("afesp_ccsd_so_get_tensor: no spin-orbital CCSD state").so_fetch_tensor(cx, name, out, capacity); });
}

// ---- Lambda and the one-particle density (lambda_so.h)
int afesp_ccsd_so_lambda_init(afesp_ctx* ctx, int diis_n_errmat)
{
    return entry(ctx, [&](Context& cx) { ctx->sv.need_so("afesp_ccsd_so_lambda_init: no spin-orbital CCSD state").so_lambda_begin(cx, diis_n_errmat); });
}

int afesp_ccsd_so_lambda_iterate(afesp_ctx* ctx, double e_tol, double l_tol, double* pseudo_energy, double* rms_sq, int* converged)
{
    return entry(ctx, [&](Context& cx) {
        report(ctx->sv.need_so("afesp_ccsd_so_lambda_iterate: no spin-orbital CCSD state").so_lambda_step(cx, e_tol, l_tol), pseudo_energy, rms_sq, converged);
    });
}

int afesp_ccsd_so_lambda_energy(afesp_ctx* ctx, double e_tol, double l_tol, double* pseudo_energy, double* rms_sq, int* converged)
{
    return entry(ctx, [&](Context& cx) {
        report(ctx->sv.need_so("afesp_ccsd_so_lambda_energy: no spin-orbital CCSD state").so_lambda_energy_step(cx, e_tol, l_tol), pseudo_energy, rms_sq,
               converged);
    });
}

int afesp_ccsd_so_lambda_diis(afesp_ctx* ctx)
{
    return entry(ctx, [&](Context& cx) { ctx->sv.need_so("afesp_ccsd_so_lambda_diis: no spin-orbital CCSD state").so_lambda_diis(cx); });
}

int afesp_ccsd_so_get_lambda(afesp_ctx* ctx, double* l1, double* l2)
{
    return entry(ctx, [&](Context& cx) { ctx->sv.need_so("afesp_ccsd_so_get_lambda: no spin-orbital CCSD state").so_get_lambda(cx, l1, l2); });
}

int afesp_ccsd_so_set_lambda(afesp_ctx* ctx, const double* l1, const double* l2)
{
    return entry(ctx, [&](Context& cx) { ctx->sv.need_so("afesp_ccsd_so_set_lambda: no spin-orbital CCSD state").so_set_lambda(cx, l1, l2); });
}

int afesp_ccsd_so_density(afesp_ctx* ctx, double* d, int64_t capacity)
{
    return entry(ctx, [&](Context& cx) { so_density(cx, ctx->sv.need_so("afesp_ccsd_so_density: no spin-orbital CCSD state").so, d, capacity); });
}

// ---- the EOM-CCSD eigenproblems (eom_so.h): one-liners over eom_entry / eom_iterate_entry
int afesp_ccsd_so_eom_init(afesp_ctx* ctx, int nroots, int max_space)
{
    return eom_entry(ctx, "afesp_ccsd_so_eom_init", EOM_KIND_EE, nullptr, so_eom_init, nroots, max_space);
}
int afesp_ccsd_so_eom_sigma(afesp_ctx* ctx, int nvec, const double* r1, const double* r2, double* s1, double* s2)
{
    return eom_entry(ctx, "afesp_ccsd_so_eom_sigma", EOM_KIND_EE, nullptr, so_eom_sigma_host, nvec, r1, r2, s1, s2);
}
int afesp_ccsd_so_eom_guess(afesp_ctx* ctx)
{
    return eom_entry(ctx, "afesp_ccsd_so_eom_guess", EOM_KIND_EE, nullptr, so_eom_guess);
}
int afesp_ccsd_so_eom_set_guess(afesp_ctx* ctx, int k, const double* r1, const double* r2)
{
    return eom_entry(ctx, "afesp_ccsd_so_eom_set_guess", EOM_KIND_EE, nullptr, so_eom_set_guess, k, r1, r2);
}
int afesp_ccsd_so_eom_iterate(afesp_ctx* ctx, double tol, double* omega, double* resnorm, int* flags, int* nsigma, int* converged)
{
    return eom_iterate_entry(ctx, "afesp_ccsd_so_eom_iterate", EOM_KIND_EE, nullptr, tol, omega, resnorm, flags, nsigma, converged);
}
int afesp_ccsd_so_eom_get_vector(afesp_ctx* ctx, int k, double* r1, double* r2)
{
    return eom_entry(ctx, "afesp_ccsd_so_eom_get_vector", EOM_KIND_EE, nullptr, so_eom_get_vector, k, r1, r2);
}

int afesp_ccsd_so_eom_left_init(afesp_ctx* ctx, int nroots, int max_space)
{
    return eom_entry(ctx, "afesp_ccsd_so_eom_left_init", EOM_KIND_EE_LEFT, nullptr, so_eom_init, nroots, max_space);
}
int afesp_ccsd_so_eom_lsigma(afesp_ctx* ctx, int nvec, const double* l1, const double* l2, double* s1, double* s2)
{
    return eom_entry(ctx, "afesp_ccsd_so_eom_lsigma", EOM_KIND_EE_LEFT, nullptr, so_eom_sigma_host, nvec, l1, l2, s1, s2);
}
int afesp_ccsd_so_eom_left_guess(afesp_ctx* ctx)
{
    return eom_entry(ctx, "afesp_ccsd_so_eom_left_guess", EOM_KIND_EE_LEFT, nullptr, so_eom_guess);
}
int afesp_ccsd_so_eom_left_set_guess(afesp_ctx* ctx, int k, const double* l1, const double* l2)
{
    return eom_entry(ctx, "afesp_ccsd_so_eom_left_set_guess", EOM_KIND_EE_LEFT, nullptr, so_eom_set_guess, k, l1, l2);
}
int afesp_ccsd_so_eom_left_iterate(afesp_ctx* ctx, double tol, double* omega, double* resnorm, int* flags, int* nsigma, int* converged)
{
    return eom_iterate_entry(ctx, "afesp_ccsd_so_eom_left_iterate", EOM_KIND_EE_LEFT, nullptr, tol, omega, resnorm, flags, nsigma, converged);
}
int afesp_ccsd_so_eom_left_get_vector(afesp_ctx* ctx, int k, double* l1, double* l2)
{
    return eom_entry(ctx, "afesp_ccsd_so_eom_left_get_vector", EOM_KIND_EE_LEFT, nullptr, so_eom_get_vector, k, l1, l2);
}

int afesp_ccsd_so_eom_ipea_init(afesp_ctx* ctx, int sector, int nroots, int max_space)
{
    return eom_entry(ctx, "afesp_ccsd_so_eom_ipea_init", EOM_KINDS, &sector, so_eom_init, nroots, max_space);
}
int afesp_ccsd_so_eom_ipea_sigma(afesp_ctx* ctx, int sector, int nvec, const double* r1, const double* r2, double* s1, double* s2)
{
    return eom_entry(ctx, "afesp_ccsd_so_eom_ipea_sigma", EOM_KINDS, &sector, so_eom_sigma_host, nvec, r1, r2, s1, s2);
}
int afesp_ccsd_so_eom_ipea_guess(afesp_ctx* ctx, int sector)
{
    return eom_entry(ctx, "afesp_ccsd_so_eom_ipea_guess", EOM_KINDS, &sector, so_eom_guess);
}
int afesp_ccsd_so_eom_ipea_set_guess(afesp_ctx* ctx, int sector, int k, const double* r1, const double* r2)
{
    return eom_entry(ctx, "afesp_ccsd_so_eom_ipea_set_guess", EOM_KINDS, &sector, so_eom_set_guess, k, r1, r2);
}
int afesp_ccsd_so_eom_ipea_iterate(afesp_ctx* ctx, int sector, double tol, double* omega, double* resnorm, int* flags, int* nsigma, int* converged)
{
    return eom_iterate_entry(ctx, "afesp_ccsd_so_eom_ipea_iterate", EOM_KINDS, &sector, tol, omega, resnorm, flags, nsigma, converged);
}
int afesp_ccsd_so_eom_ipea_get_vector(afesp_ctx* ctx, int sector, int k, double* r1, double* r2)
{
    return eom_entry(ctx, "afesp_ccsd_so_eom_ipea_get_vector", EOM_KINDS, &sector, so_eom_get_vector, k, r1, r2);
}

int afesp_eig_general(int n, const double* a, int lda, double* wr, double* wi, double* vr) { return eig_general(n, a, lda, wr, wi, vr); }

// ---- the two-particle density of the spin-orbital state (density2_so.h)
int afesp_ccsd_so_density2_build(afesp_ctx* ctx)
{
    return entry(ctx, [&](Context& cx) { so_density2_build(cx, ctx->sv.need_so("afesp_ccsd_so_density2_build: no spin-orbital CCSD state").so); });
}

int afesp_ccsd_so_density2_get(afesp_ctx* ctx, const char* name, double* out, int64_t capacity)
{
    return entry(ctx, [&](Context& cx) {
        so_density2_get(cx, ctx->sv.need_so("afesp_ccsd_so_density2_get: no spin-orbital CCSD state").so, name, out, capacity);
    });
}

int afesp_ccsd_so_density2_energy(afesp_ctx* ctx, double* e)
{
    return entry(ctx, [&](Context& cx) { so_density2_energy(cx, ctx->sv.need_so("afesp_ccsd_so_density2_energy: no spin-orbital CCSD state").so, e); });
}

int afesp_ccsd_so_density2_expect(afesp_ctx* ctx, const double* A, const double* B, double* value)
{
    return entry(ctx, [&](Context& cx) {
        SOState& s = ctx->sv.need_so("afesp_ccsd_so_density2_expect: no spin-orbital CCSD state").so;
        if (!value) throw Error(1, "afesp_ccsd_so_density2_expect: NULL argument");
        *value = so_density2_expect(cx, s, A, B);
    });
}

// ---- orbital relaxation of the spin-orbital density (relax_so.h)
int afesp_ccsd_so_orbital_gradient(afesp_ctx* ctx, int fock_response, double* w, int64_t capacity)
{
    return entry(ctx, [&](Context& cx) {
        so_orbital_gradient(cx, ctx->sv.need_so("afesp_ccsd_so_orbital_gradient: no spin-orbital CCSD state").so, fock_response, w, capacity);
    });
}

int afesp_ccsd_so_zvector_apply(afesp_ctx* ctx, const double* x, double* y)
{
    return entry(ctx, [&](Context& cx) { so_zvector_apply(cx, ctx->sv.need_so("afesp_ccsd_so_zvector_apply: no spin-orbital CCSD state").so, x, y); });
}

int afesp_ccsd_so_zvector_solve(afesp_ctx* ctx, double tol, int maxiter, double* z, int* iters, double* resid)
{
    return entry(ctx, [&](Context& cx) {
        so_zvector_solve(cx, ctx->sv.need_so("afesp_ccsd_so_zvector_solve: no spin-orbital CCSD state").so, tol, maxiter, z, iters, resid);
    });
}

int afesp_ccsd_so_relaxed_density(afesp_ctx* ctx, double* d, int64_t capacity)
{
    return entry(ctx, [&](Context& cx) {
        so_relaxed_density(cx, ctx->sv.need_so("afesp_ccsd_so_relaxed_density: no spin-orbital CCSD state").so, d, capacity);
    });
}

int afesp_ccsd_so_relax_pair_row(afesp_ctx* ctx, int which, double* out, int reps, double* ms)
{
    return entry(ctx, [&](Context& cx) {
        const double t = so_relax_pair_row(cx, ctx->sv.need_so("afesp_ccsd_so_relax_pair_row: no spin-orbital CCSD state").so, which, out, reps);
        if (ms) *ms = t;
    });
}

// ---- the left-hand side of the EOM-IP / EOM-EA sectors and their Dyson orbitals (eom_ipea_so.h, eom_ipea_left_so.hip)
int afesp_ccsd_so_eom_ipea_lsigma(afesp_ctx* ctx, int sector, int nvec, const double* l1, const double* l2, double* s1, double* s2)
{
    return eom_entry(ctx, "afesp_ccsd_so_eom_ipea_lsigma", EOM_KIND_IP_LEFT, &sector, so_eom_sigma_host, nvec, l1, l2, s1, s2);
}
int afesp_ccsd_so_eom_ipea_left_init(afesp_ctx* ctx, int sector, int nroots, int max_space)
{
    return eom_entry(ctx, "afesp_ccsd_so_eom_ipea_left_init", EOM_KIND_IP_LEFT, &sector, so_eom_init, nroots, max_space);
}
int afesp_ccsd_so_eom_ipea_left_guess(afesp_ctx* ctx, int sector)
{
    return eom_entry(ctx, "afesp_ccsd_so_eom_ipea_left_guess", EOM_KIND_IP_LEFT, &sector, so_eom_guess);
}
int afesp_ccsd_so_eom_ipea_left_set_guess(afesp_ctx* ctx, int sector, int k, const double* l1, const double* l2)
{
    return eom_entry(ctx, "afesp_ccsd_so_eom_ipea_left_set_guess", EOM_KIND_IP_LEFT, &sector, so_eom_set_guess, k, l1, l2);
}
int afesp_ccsd_so_eom_ipea_left_iterate(afesp_ctx* ctx, int sector, double tol, double* omega, double* resnorm, int* flags, int* nsigma,
                                        int* converged)
{
    return eom_iterate_entry(ctx, "afesp_ccsd_so_eom_ipea_left_iterate", EOM_KIND_IP_LEFT, &sector, tol, omega, resnorm, flags, nsigma, converged);
}
int afesp_ccsd_so_eom_ipea_left_get_vector(afesp_ctx* ctx, int sector, int k, double* l1, double* l2)
{
    return eom_entry(ctx, "afesp_ccsd_so_eom_ipea_left_get_vector", EOM_KIND_IP_LEFT, &sector, so_eom_get_vector, k, l1, l2);
}
int afesp_ccsd_so_eom_ipea_dyson(afesp_ctx* ctx, int sector, int nvec, const double* l1, const double* l2, const double* r1, const double* r2,
                                 double* dl, double* dr)
{
    return eom_call(ctx, "afesp_ccsd_so_eom_ipea_dyson", EOM_KINDS, &sector, [&](Context& cx, SOState& so, EomKind) {
        so_eom_ipea_dyson(cx, so, sector, nvec, l1, l2, r1, r2, dl, dr);
    });
}

// ---- EOM-EE-CCSD reference coupling and the bilinear density (eom_so.h, eom_left_so.hip)
int afesp_ccsd_so_eom_ref_coupling(afesp_ctx* ctx, int nvec, const double* r1, const double* r2, double* c)
{
    return entry(ctx, [&](Context& cx) {
        so_eom_ref_coupling(cx, ctx->sv.need_so("afesp_ccsd_so_eom_ref_coupling: no spin-orbital CCSD state").so, nvec, r1, r2, c);
    });
}

int afesp_ccsd_so_eom_density(afesp_ctx* ctx, double l0, const double* l1, const double* l2, double r0, const double* r1, const double* r2,
                              double* d, int64_t capacity)
{
    return entry(ctx, [&](Context& cx) {
        so_eom_density(cx, ctx->sv.need_so("afesp_ccsd_so_eom_density: no spin-orbital CCSD state").so, l0, l1, l2, r0, r1, r2, d, capacity);
    });
}

// ---- EOM-CCSD linear response (response_so.h)
int afesp_ccsd_so_response_xi(afesp_ctx* ctx, int nop, const double* x, double* xi1, double* xi2)
{
    return entry(ctx, [&](Context& cx) {
        so_response_xi_host(cx, ctx->sv.need_so("afesp_ccsd_so_response_xi: no spin-orbital CCSD state").so, nop, x, xi1, xi2);
    });
}

int afesp_ccsd_so_response_init(afesp_ctx* ctx, int nop, const double* x, int nfreq_signed, const double* omega, int max_space)
{
    return entry(ctx, [&](Context& cx) {
        so_response_init(cx, ctx->sv.need_so("afesp_ccsd_so_response_init: no spin-orbital CCSD state").so, nop, x, nfreq_signed, omega, max_space);
    });
}

int afesp_ccsd_so_response_iterate(afesp_ctx* ctx, double tol, double* resnorm, int* nsigma, int* converged)
{
    return entry(ctx, [&](Context& cx) {
        SOState& so = ctx->sv.need_so("afesp_ccsd_so_response_iterate: no spin-orbital CCSD state").so;
        if (!(tol > 0.0)) throw Error(1, "afesp_ccsd_so_response_iterate: tol must be positive");
        const int conv = so_response_iterate(cx, so, tol);
        davidson_report(so.resp->d, conv, nullptr, resnorm, nullptr, nsigma, converged);
    });
}

int afesp_ccsd_so_response_get_vector(afesp_ctx* ctx, int iop, int ifreq, double* r1, double* r2)
{
    return entry(ctx, [&](Context& cx) {
        so_response_get_vector(cx, ctx->sv.need_so("afesp_ccsd_so_response_get_vector: no spin-orbital CCSD state").so, iop, ifreq, r1, r2);
    });
}

int afesp_ccsd_so_response_function(afesp_ctx* ctx, int nfreq, const double* omega, double* out)
{
    return entry(ctx, [&](Context& cx) {
        so_response_function(cx, ctx->sv.need_so("afesp_ccsd_so_response_function: no spin-orbital CCSD state").so, nfreq, omega, out);
    });
}

int afesp_lu_solve(int n, double* a, int lda, int nrhs, double* b, int ldb, double floor) { return lu_solve(n, a, lda, nrhs, b, ldb, floor); }

// ---- the same at complex frequencies (response_so.h)
int afesp_ccsd_so_response_init_complex(afesp_ctx* ctx, int nop, const double* x, int nfreq_signed, const double* z, int max_space)
{
    return entry(ctx, [&](Context& cx) {
        so_response_init_complex(cx, ctx->sv.need_so("afesp_ccsd_so_response_init_complex: no spin-orbital CCSD state").so, nop, x, nfreq_signed, z, max_space);
    });
}

int afesp_ccsd_so_response_get_vector_complex(afesp_ctx* ctx, int iop, int ifreq, double* r1_re, double* r2_re, double* r1_im, double* r2_im)
{
    return entry(ctx, [&](Context& cx) {
        so_response_get_vector_complex(cx, ctx->sv.need_so("afesp_ccsd_so_response_get_vector_complex: no spin-orbital CCSD state").so, iop, ifreq, r1_re,
                                       r2_re, r1_im, r2_im);
    });
}

int afesp_ccsd_so_response_function_complex(afesp_ctx* ctx, int nfreq, const double* z, double* out)
{
    return entry(ctx, [&](Context& cx) {
        so_response_function_complex(cx, ctx->sv.need_so("afesp_ccsd_so_response_function_complex: no spin-orbital CCSD state").so, nfreq, z, out);
    });
}

int afesp_lu_solve_complex(int n, double* a, int lda, int nrhs, double* b, int ldb, double floor)
{
    return lu_solve_complex(n, a, lda, nrhs, b, ldb, floor);
}

int64_t afesp_ccsd_so_t_ntriples(int64_t nocc) { return so_triples_count((int)nocc); }

int afesp_ccsd_so_t(afesp_ctx* ctx, int64_t t_begin, int64_t t_end, double* e_t)
{
    return entry(ctx, [&](Context& cx) {
        const double e = so_triples(cx, ctx->sv.so, t_begin, t_end);
        if (e_t) *e_t = e;
    });
}

int afesp_ccsd_so_lambda_t(afesp_ctx* ctx, int64_t t_begin, int64_t t_end, double* e_lt)
{
    return entry(ctx, [&](Context& cx) {
        const double e = so_lambda_triples(cx, ctx->sv.so, t_begin, t_end);
        if (e_lt) *e_lt = e;
    });
}

int afesp_ccsd_so_eom_t(afesp_ctx* ctx, int nstates, const double* omega, const double* l1, const double* l2, const double* r1,
                        const double* r2, int64_t t_begin, int64_t t_end, double* delta)
{
    return entry(ctx, [&](Context& cx) { so_eom_triples(cx, ctx->sv.so, nstates, omega, l1, l2, r1, r2, t_begin, t_end, delta); });
}

// ---- the triples correction to EOM-IP / EOM-EA roots (eom_ipea_t_so.h)
int64_t afesp_ccsd_so_eom_ipea_t_nitems(int sector, int nocc) { return so_eom_sector_ok(sector) ? so_eom_ipea_t_items(sector, nocc) : 0; }
int afesp_ccsd_so_eom_ipea_t(afesp_ctx* ctx, int sector, int nstates, const double* omega, const double* l1, const double* l2,
                             const double* r1, const double* r2, int64_t begin, int64_t end, double* delta)
{
    return entry(ctx, [&](Context& cx) { so_eom_ipea_triples(cx, ctx->sv.so, sector, nstates, omega, l1, l2, r1, r2, begin, end, delta); });
}

// ---------------------------------------------------------------- open-shell (UHF-based) path
int afesp_build_fock_uhf(afesp_ctx* ctx, int64_t nbasis, const double* dens_a, const double* dens_b, const double* core_hamil,
                         double* fock_a, double* fock_b)
{
    return entry(ctx, [&](Context& cx) {
        if (!ctx->in.ao || ctx->in.ao_n != nbasis || !dens_a || !dens_b || !core_hamil || !fock_a || !fock_b)
            throw Error(1, "afesp_build_fock_uhf: no AO integrals resident for this basis size (afesp_read_eri_text / afesp_set_eri)");
        build_fock_uhf(cx, ctx->in, nbasis, dens_a, dens_b, core_hamil, fock_a, fock_b);
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
    return entry(ctx, [&](Context& cx) { ctx->sv.uso_init(cx, ctx->in, nbasis, nalpha, nbeta, levels_a, levels_b, diis_n_errmat); });
}

int afesp_ccsd_uso_init_fock(afesp_ctx* ctx, int64_t nbasis, int64_t nalpha, int64_t nbeta, const double* fock_a, const double* fock_b,
                             int diis_n_errmat, double* e_mp2)
{
    return entry(ctx, [&](Context& cx) {
        const double e2 = ctx->sv.uso_init_fock(cx, ctx->in, nbasis, nalpha, nbeta, fock_a, fock_b, diis_n_errmat);
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
        ctx->sv.init(cx, (int)nocc, (int)nvirt, nullptr, packed, true, e.data(), diis_n_errmat);   // (`packed` is the state's from here on)
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

// Floating-point operations of one particle-particle ladder / one CCSD iteration as this context evaluates it (solver.hip)
int afesp_ccsd_pp_ladder_flop(afesp_ctx* ctx, double* flop)
{
    return entry(ctx, [&](Context& cx) {
        const double f = ctx->sv.need_cc("afesp_ccsd_pp_ladder_flop: no CCSD state").pp_ladder_flop();
        if (flop) *flop = f;
    });
}

int afesp_ccsd_iteration_flop(afesp_ctx* ctx, double* flop)
{
    return entry(ctx, [&](Context& cx) {
        const double f = ctx->sv.need_cc("afesp_ccsd_iteration_flop: no CCSD state").iteration_flop();
        if (flop) *flop = f;
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
        CCState& cc = ctx->sv.need_cc("afesp_time_pp_ladder: no CCSD state").cc;
        const double ms = time_on_stream(cx, reps, [&] { ccsd_pp_ladder(cx, cc); });
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
        ctx->sv.cc_programs_reset(cx);   // a captured iteration does not contain the rank split
    });
}

int afesp_comm_destroy(afesp_ctx* ctx)
{
    return entry(ctx, [&](Context& cx) {
        cx.sync();
        comm_destroy(cx.comm);
        cx.comm = nullptr;
        ctx->sv.cc_programs_reset(cx);
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
        if (!split) throw Error(1, "afesp_ccsd_is_split: no CCSD state");
        *split = ctx->sv.need_cc("afesp_ccsd_is_split: no CCSD state").is_split(cx) ? 1 : 0;
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
        *launches = ctx->sv.iteration_launches();
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

// ---- the test entry to the block Davidson unit (davidson_test.h)
int afesp_test_davidson_create(afesp_ctx* ctx, int64_t n1, int64_t nvec, double w2, int follow, int nroots, int max_space, int r, const double* d,
                               const double* U, const double* V, const double* diag)
{
    return entry(ctx, [&](Context& cx) { davidson_test_create(cx, n1, nvec, w2, follow, nroots, max_space, r, d, U, V, diag); });
}

int afesp_test_davidson_destroy(afesp_ctx* ctx)
{
    return entry(ctx, [&](Context& cx) { davidson_test_destroy(cx); });
}

int afesp_test_davidson_set_guess(afesp_ctx* ctx, int k, const double* x1, const double* x2)
{
    return entry(ctx, [&](Context& cx) { davidson_test_set_guess(cx, k, x1, x2); });
}

static void davidson_test_report(Context& cx, const char* who, int conv, double* omega, double* resnorm, int* flags, int counts[4], int* converged)
{
    const Davidson& E = davidson_test_need(cx, who).d;
    davidson_report(E, conv, omega, resnorm, flags, nullptr, converged);
    if (counts) counts[0] = E.nsigma, counts[1] = E.ncollapse, counts[2] = E.nb, counts[3] = E.npend;
}

int afesp_test_davidson_iterate(afesp_ctx* ctx, double tol, double* omega, double* resnorm, int* flags, int counts[4], int* converged)
{
    return entry(ctx, [&](Context& cx) { davidson_test_report(cx, "afesp_test_davidson_iterate", davidson_test_iterate(cx, tol), omega, resnorm, flags, counts, converged); });
}

int afesp_test_davidson_linear_start(afesp_ctx* ctx, int nrhs, const double* rhs, const double* shifts)
{
    return entry(ctx, [&](Context& cx) { davidson_test_linear_start(cx, nrhs, rhs, shifts); });
}

int afesp_test_davidson_linear_start_complex(afesp_ctx* ctx, int nrhs, const double* rhs, const double* shift_re, const double* shift_im)
{
    return entry(ctx, [&](Context& cx) { davidson_test_linear_start_complex(cx, nrhs, rhs, shift_re, shift_im); });
}

int afesp_test_davidson_linear_iterate(afesp_ctx* ctx, double tol, double* resnorm, int* flags, int counts[4], int* converged)
{
    return entry(ctx, [&](Context& cx) { davidson_test_report(cx, "afesp_test_davidson_linear_iterate", davidson_test_linear_iterate(cx, tol), nullptr, resnorm, flags, counts, converged); });
}

int afesp_test_davidson_get_vector(afesp_ctx* ctx, int k, double* x1, double* x2)
{
    return entry(ctx, [&](Context& cx) { davidson_test_get_vector(cx, k, x1, x2); });
}

int afesp_test_davidson_fetch(afesp_ctx* ctx, const char* what, double* out, int64_t capacity, int64_t* count)
{
    return entry(ctx, [&](Context& cx) {
        const int64_t n = davidson_test_fetch(cx, what, out, capacity);
        if (count) *count = n;
    });
}

}  // extern "C"
