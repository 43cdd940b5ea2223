// solver.hip -- the drivers of the spin-free and the spin-orbital CCSD solver (solver.h).
#include <cstdio>
#include <cstring>

#include "solver.h"
#include "integrals.h"

namespace afesp {

void GraphSlot::reset()
{
    if (exec) (void)hipGraphExecDestroy(exec);
    exec = nullptr;
    calls = 0;
    disabled = knobs().no_graph;
}

void Solver::cc_programs_reset(Context& cx)
{
    graph_cc.reset();
    fused_slot_reset(cx, fused_int);
    fused_slot_reset(cx, fused_amp);
    fused_slot_reset(cx, fused_iter);
}

void Solver::destroy(Context& cx)
{
    cc_programs_reset(cx);
    so_programs_reset(cx);
    triples_plan_free(cc);
    so_triples_plan_free(so);
    so_lambda_free(cx, so);   // (the host-side object of a Lambda state)
    ring_free(cx, cc);   // (the host-side descriptor of the ring launches; its device blocks go with the context)
}

namespace {

// Runs `body` (launches on the context's lanes, no host synchronisation) directly for the first AFESP_GRAPH_AFTER calls,
// then captures it into a graph once and replays the graph afterwards.  Nothing executes during capture, so a failed
// capture simply falls back to running the body.
template <typename Body>
void replay(Context& cx, GraphSlot& g, bool eligible, Body body)
{
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

// `body` as the slot's launch-fused program where `small` says the system is one for it and the program can be had (fused.h: recorded
// from the very calls of `body` on first use), else call by call
template <typename Body>
void fused_or_direct(Context& cx, bool small, FusedSlot& slot, Body body)
{
    if (!(small && fused_exec(cx, slot, body))) body();
}

// t1 / t2 of either state to the host (no wait) and from it (waits); a null pointer leaves that one out
template <typename State>
void amps_to_host(Context& cx, const State& s, double* t1, double* t2)
{
    if (t1) AFESP_HIP(hipMemcpyAsync(t1, s.t1.d, sizeof(double) * s.t1.size(), hipMemcpyDeviceToHost, cx.stream));
    if (t2) AFESP_HIP(hipMemcpyAsync(t2, s.t2.d, sizeof(double) * s.t2.size(), hipMemcpyDeviceToHost, cx.stream));
}
template <typename State>
void amps_from_host(Context& cx, State& s, const double* t1, const double* t2)
{
    if (t1) AFESP_HIP(hipMemcpyAsync(s.t1.d, t1, sizeof(double) * s.t1.size(), hipMemcpyHostToDevice, cx.stream));
    if (t2) AFESP_HIP(hipMemcpyAsync(s.t2.d, t2, sizeof(double) * s.t2.size(), hipMemcpyHostToDevice, cx.stream));
    cx.sync();
}

}  // namespace

// ---------------------------------------------------------------- spin-free
void Solver::init(Context& cx, int o, int v, const double* host, double* dev, bool adopt, const double* levels, int diis_nerr)
{
    // (a state of the same extents is initialised again where it lies: its compiled programs stay)
    const bool again = ccsd_can_reinit(cc, o, v, diis_nerr);
    double* mine = adopt ? dev : nullptr;   // an array that is this state's to keep or to give back
    if (host) {
        // (the packed integrals the state kept for ccsd_need_vvvv go back to the arena BEFORE their successor is asked for -- a
        // geometry scan never holds two packed arrays)
        if (again && cc.eri_own) {
            cx.quiesce();
            eri_gone(cc.eri_own);
            cx.release(cc.eri_own);
            cc.eri_own = nullptr;
        }
        const int64_t ne = neri_of(o + v);
        mine = cx.alloc(ne);
        AFESP_HIP(hipMemcpyAsync(mine, host, sizeof(double) * ne, hipMemcpyHostToDevice, cx.stream));
    }
    if (!again) {
        cc_programs_reset(cx);
        if (!adopt) cx.drop_scratch("ao2mo_");   // the AO->MO temporaries (an array made for this state comes from no transform)
    } else {
        graph_cc.reset();
    }
    ccsd_init(cx, cc, o, v, mine ? mine : dev, levels, diis_nerr);
    if (mine) {
        // a large system forms <ef|ab> on request only (ccsd_need_vvvv): its state keeps the device copy of the integrals
        if (cc.v_vvvv.d) { cx.release(mine); cc.eri_src = nullptr; }
        else cc.eri_own = mine;
    }
}

void Solver::update_intermediates(Context& cx)
{
    ccsd_refresh_sharding(cx, cc);
    cc.int_split = false;   // (ccsd_intermediates says so again when it runs split; a launch-fused program never does, and does not pass there)
    fused_or_direct(cx, ccsd_uses_lanes(cc), fused_int, [&] { ccsd_intermediates(cx, cc); });
    cx.sync();
}

void Solver::update_amplitudes(Context& cx)
{
    cc.amp_epoch = ++cx.amp_clock;
    ccsd_refresh_sharding(cx, cc);
    cc.tail_pending = false;
    // (what the LAST update left is said by ccsd_amplitudes when it runs; a launch-fused program does not pass there, is never split and
    // leaves no laned partial residuals -- the getter added a laned update's stale ones to the residual of a launch-fused update after it)
    cc.amp_split = cc.partials_live = false;
    fused_or_direct(cx, ccsd_uses_lanes(cc), fused_amp, [&] { ccsd_amplitudes(cx, cc); });
    cx.sync();
}

// One iteration up to the energy kernels (no host synchronisation): the launch-fused program of a small system (fused.h; recorded
// from the very calls below on first use), the call-by-call sequence otherwise.
bool Solver::iteration_body(Context& cx)
{
    auto with_tail = [&] {
        ccsd_intermediates(cx, cc, true);
        ccsd_amplitudes(cx, cc, true);
        ccsd_tail_launch(cx, cc);
    };
    if (ccsd_uses_lanes(cc) && fused_exec(cx, fused_iter, with_tail)) {
        cc.partials_live = false;   // (the whole residual lies in r2 / r1, whatever a laned iteration before this one left: update_amplitudes)
        return true;
    }
    // Large systems (one stream, whole-tensor products): the same two-kernel tail -- P(ia/jb) + division, the energy / rms sums and the
    // DIIS history push in ONE pass over the residual instead of three (update, energy, push: 26 against 23 passes over o^2 v^2 elements at
    // eight history vectors, and no host wait between the energy and the push); the <= 17 x 17 system is then solved on the host.
    // AFESP_LARGE_TAIL=0: the three kernels.
    if (!ccsd_uses_lanes(cc) && knobs().large_tail) {
        with_tail();
        return true;
    }
    cc.tail_pending = false;
    replay(cx, graph_cc, ccsd_uses_lanes(cc), [&] {
        ccsd_intermediates(cx, cc, true);
        ccsd_amplitudes(cx, cc);
        ccsd_energy_launch(cx, cc);
    });
    if (graph_cc.exec) cc.partials_live = true;   // (a replayed iteration is a laned one: its partial residuals lie where the captured call left them)
    return false;
}

StepResult Solver::step(Context& cx, double e_tol, double t_tol)
{
    ccsd_refresh_sharding(cx, cc);
    cc.int_split = cc.amp_split = false;   // (a replayed or launch-fused iteration is never split; one that runs split says so itself)
    const bool tail = iteration_body(cx);
    const int conv = tail ? ccsd_tail_read(cx, cc, e_tol, t_tol) : ccsd_energy_read(cx, cc, e_tol, t_tol);
    return {cc.energy, cc.rms, conv};
}

int Solver::solve(Context& cx, int maxiter, double e_tol, double t_tol, double* iter_energy, double* iter_rms_sq)
{
    cc.amp_epoch = ++cx.amp_clock;
    // ccsd.f90:314-315, :325
    cc.energy = cc.energy_old = 0.0;
    k_fill(cx, cc.t2_old.d, cc.t2_old.size(), 0.0);
    auto record = [&](int it, const StepResult& r) {
        if (iter_energy) iter_energy[it] = r.energy;
        if (iter_rms_sq) iter_rms_sq[it] = r.rms;
    };
    record(0, energy(cx, e_tol, t_tol));
    for (int it = 1; it <= maxiter; ++it) {
        const StepResult r = step(cx, e_tol, t_tol);
        record(it, r);
        if (r.converged) return it;
        ccsd_diis_update(cx, cc);
    }
    if (maxiter > 0) diis_check_flag(cx, host_scalars(cx, DIIS_FLAG_SLOT + 1));   // a solve that failed after the last energy read
    return -1;
}

void Solver::get_amplitudes(Context& cx, double* t1, double* t2)
{
    amps_to_host(cx, cc, t1, t2);
    diis_check_flag(cx, host_scalars(cx, DIIS_FLAG_SLOT + 1));   // afesp_ccsd_diis does not wait for its solve: a failure surfaces here at the latest
}

void Solver::set_amplitudes(Context& cx, const double* t1, const double* t2)
{
    cc.amp_epoch = ++cx.amp_clock;
    // (a large system holds I_ovov / I_voov and copies of the OLD amplitudes in the layout of its ring launches (ring.hip): an
    // afesp_ccsd_update_amplitudes that follows without new intermediates reads the reference-layout tensors and the new amplitudes)
    if (ring_live(cc)) {
        ring_tg_materialize(cx, cc, cc.I_ovov, cc.I_voov);
        ring_invalidate(cc);
    }
    cc.amps_touched = true;
    // (a launch-fused iteration has pushed its own result into the DIIS history already: afesp_ccsd_diis extrapolates the amplitudes
    // current at the call, so it pushes again -- into the same slot, the tail has advanced no counter)
    cc.tail_pending = false;
    if (t2) cc.hist_plain = cc.nerr + 1;   // (its error vector may lack the amplitudes' symmetry: full DIIS sums until it has left the history)
    amps_from_host(cx, cc, t1, t2);
}

void Solver::fetch_tensor(Context& cx, const char* name, double* out, int64_t capacity)
{
    CCState& s = cc;
    const int64_t O = s.o, V = s.v;
    struct { const char* n; const Tensor* t; } tab[] = {
        {"v_oovv", &s.v_oovv}, {"v_ovov", &s.v_ovov}, {"v_vvov", &s.v_vvov}, {"v_oovo", &s.v_oovo}, {"v_oooo", &s.v_oooo},
        {"v_vvvv", &s.v_vvvv}, {"I_vo", &s.I_vo}, {"I_vv", &s.I_vv}, {"I_oo_p", &s.I_oo_p}, {"I_oo", &s.I_oo},
        {"c_oovv", &s.c}, {"asym_t2", &s.asym}, {"x_voov", &s.x_voov}, {"I_oooo", &s.I_oooo}, {"I_ovov", &s.I_ovov},
        {"I_voov", &s.I_voov}, {"I_ooov_p", &s.I_ooov_p}, {"r1", &s.r1}, {"r2", &s.r2},
        {"D1", &s.D1}, {"D2", &s.D2}, {"t1", &s.t1}, {"t2", &s.t2}};
    auto is = [&](const char* n) { return !strcmp(name, n); };
    if (is("v_vvvv")) ccsd_need_vvvv(cx, s);
    Tensor vovv = view(nullptr, {V, O, V, V});   // I_vovv_p: not formed by the iteration (ccsd.hip), built from the current t1 on request
    const Tensor* t = is("I_vovv_p") ? &vovv : nullptr;
    for (auto& e : tab)
        if (is(e.n)) t = e.t;
    // What only a split call leaves behind (tests/test_gpu_cc_split.py): the rank-partial T1 residual and the packed ladder PP(i,j,p) of the
    // last ccsd_amplitudes, and the buffer into which the last ccsd_intermediates put the slice of t2 <ef|ia> + t1 x_voov that it took out of
    // I_ooov_p -- the buffer as it lies: outside the slice it holds what earlier calls left.  After an unsplit call they hold something else.
    Tensor split_only;
    if (is("r1_sh") || is("pp") || is("ooov_sh")) {
        const bool amp = !is("ooov_sh");
        auto osh = cx.cache.find("ooov_sh");
        if (!(amp ? s.amp_split : (s.int_split && osh != cx.cache.end())))
            throw Error(1, std::string("afesp_ccsd_get_tensor: ") + name + " is served only when the last " +
                               (amp ? "update of the amplitudes" : "update of the intermediates") +
                               " of this state ran split (afesp_ccsd_set_split): it did not");
        split_only = is("r1_sh") ? view(s.r1_sh, {O, V}) : is("pp") ? view(s.pp, {O, O, V * (V + 1) / 2}) : view((double*)osh->second.first, {O, O, O, V});
        t = &split_only;
    }
    if (!t) throw Error(1, std::string("afesp_ccsd_get_tensor: unknown tensor ") + name);
    if (t->size() > capacity) throw Error(1, std::string("afesp_ccsd_get_tensor: buffer too small for ") + name);
    const double* src = t->d;
    if (t == &vovv) {
        vovv.d = cx.scratch("I_vovv_p", vovv.size());
        ccsd_build_I_vovv_p(cx, s, vovv);
        src = vovv.d;
    } else if (is("r2") || is("r1")) {
        src = ccsd_residual_full(cx, s, is("r2"));
    } else if (ring_live(s) && (is("I_ovov") || is("I_voov"))) {
        // a large system's iteration holds these two in the layout its ring products read (ring.hip): turned back on request
        Tensor io = view(cx.scratch("ring_I_ovov", t->size()), {O, V, O, V}), iv = view(cx.scratch("ring_I_voov", t->size()), {V, O, O, V});
        ring_tg_materialize(cx, s, io, iv);
        src = is("I_ovov") ? io.d : iv.d;
    }
    AFESP_HIP(hipMemcpyAsync(out, src, sizeof(double) * t->size(), hipMemcpyDeviceToHost, cx.stream));
    cx.sync();
}

// (plain a <= b form or the symmetric/antisymmetric pair form, ccsd.hip)
double Solver::pp_ladder_flop() const
{
    const double O = cc.o, V = cc.v, ps = V * (V + 1) / 2, pa = V * (V - 1) / 2;
    return cc.pp_sym ? 2.0 * (O * (O + 1) / 2 * ps * ps + O * (O - 1) / 2 * pa * pa) : 2.0 * O * O * V * V * ps;
}

// SURVEY.md 8(d)'s sum over the contraction sites, with the pp-ladder and the t2 x <ef|ia> product counted in the form they are
// executed (plain, a <= b, or over pair indices)
double Solver::iteration_flop() const
{
    const double O = cc.o, V = cc.v, ps = V * (V + 1) / 2, pa = V * (V - 1) / 2, os = O * (O + 1) / 2, oa = O * (O - 1) / 2;
    const bool sym = cc.pp_sym;
    const double pp = pp_ladder_flop();
    const double ooov = sym ? 2.0 * O * V * (os * ps + oa * pa) : 2.0 * O * O * O * V * V * V;
    const double o3v3 = O * O * O * V * V * V;
    // large-system path (round 5): c <ij|ef> -> I_oooo and the hole-hole ladder over pair indices (the latter inside the pp-ladder's
    // products), and the bare t(i,e) <ab|ej> term as a copy of x_voov instead of a third o^2 v^3 product
    const bool large = !ccsd_uses_lanes(cc);
    const double oooo = (sym && large) ? 4.0 * (os * os * ps + oa * oa * pa) : 2.0 * O * O * O * O * V * V;
    // (... and asym(m,i,e,f) <ef|ma> -> r1 as a trace of the pair-form t2 <ef|ia> product: one more o^2 v^3 product that is not executed)
    const double o2v3 = large ? (sym ? 14.0 : 16.0) : 18.0;
    return pp + ooov + 12.0 * o3v3 + oooo + 2.0 * O * O * O * O * V + o2v3 * O * O * V * V * V + 2.0 * O * V * V * V +
           14.0 * O * O * O * V * V;
}

// ---------------------------------------------------------------- spin-orbital
void Solver::so_init_packed(Context& cx, int nbasis, int nel, const double* host, const double* dev, const double* levels, int diis_nerr,
                            bool foo_as_published)
{
    double* tmp = nullptr;
    if (host) {
        tmp = cx.alloc(neri_of(nbasis));
        AFESP_HIP(hipMemcpyAsync(tmp, host, sizeof(double) * neri_of(nbasis), hipMemcpyHostToDevice, cx.stream));
        dev = tmp;
    }
    cx.drop_scratch("ao2mo_");   // the AO->MO temporaries
    so_programs_reset(cx);
    so_init(cx, so, nbasis, nel, dev, levels, diis_nerr, foo_as_published);
    so.amp_epoch = ++cx.amp_clock;
    if (tmp) cx.release(tmp);
}

// What the two initialisations from the resident UHF blocks share: the checks (in the caller's name `who`), and room made and measured
void Solver::uso_begin(Context& cx, const Integrals& in, const char* who, const char* hint, int64_t nbasis, int64_t nalpha, int64_t nbeta,
                       bool pointers_ok, int diis_nerr)
{
    if (nbasis <= 0 || nbasis > 512 || nalpha < 0 || nbeta < 0 || nalpha > nbasis || nbeta > nbasis || nalpha + nbeta <= 0 ||
        nalpha + nbeta >= 2 * nbasis || !pointers_ok)
        throw Error(1, std::string(who) + ": bad extents");
    if (!in.uhf_aa || in.uhf_n != nbasis)
        throw Error(1, std::string(who) + ": no UHF MO integrals resident for this basis size (call " + hint + " first)");
    const int64_t o = nalpha + nbeta, v = 2 * nbasis - o;
    cx.drop_scratch("ao2mo_");   // the AO->MO temporaries
    so_programs_reset(cx);
    so_free(cx, so);             // (a previous state's memory counts as available)
    // against the free device memory plus the context's idle blocks: the resident UHF (and RHF) integral blocks are in use
    if (!cx.fits(so_state_bytes(o, v, diis_nerr)))
        throw Error(1, std::string(who) + ": the dense spin-orbital state of this system does not fit the free device memory");
}

void Solver::uso_init(Context& cx, const Integrals& in, int64_t nbasis, int64_t nalpha, int64_t nbeta, const double* levels_a,
                      const double* levels_b, int diis_nerr)
{
    uso_begin(cx, in, "afesp_ccsd_uso_init", "afesp_ao2mo_ump2", nbasis, nalpha, nbeta, levels_a && levels_b, diis_nerr);
    so_init_uhf(cx, so, (int)nbasis, (int)nalpha, (int)nbeta, in.uhf_aa, in.uhf_bb, in.uhf_ab, levels_a, levels_b, diis_nerr);
    so.amp_epoch = ++cx.amp_clock;
}

double Solver::uso_init_fock(Context& cx, const Integrals& in, int64_t nbasis, int64_t nalpha, int64_t nbeta, const double* fock_a,
                             const double* fock_b, int diis_nerr)
{
    uso_begin(cx, in, "afesp_ccsd_uso_init_fock", "afesp_mo_rotate_uhf or afesp_ao2mo_ump2", nbasis, nalpha, nbeta, fock_a && fock_b, diis_nerr);
    const double e2 = so_init_fock(cx, so, (int)nbasis, (int)nalpha, (int)nbeta, in.uhf_aa, in.uhf_bb, in.uhf_ab, fock_a, fock_b, diis_nerr);
    so.amp_epoch = ++cx.amp_clock;
    return e2;
}

StepResult Solver::so_iterate(Context& cx, double e_tol, double t_tol)
{
    so.amp_epoch = ++cx.amp_clock;
    // (the levelled sequence of fused.h where the system is small enough for its products to be launch-bound: the big ones
    // keep their own kernels inside it)
    fused_or_direct(cx, so.t2.size() <= ((int64_t)1 << 22), fused_so, [&] {
        diis_save(cx, so);
        so_intermediates(cx, so);
        so_amplitudes(cx, so);
    });
    return so_energy_step(cx, e_tol, t_tol);
}

void Solver::so_get_amplitudes(Context& cx, double* t1, double* t2)
{
    amps_to_host(cx, so, t1, t2);
    cx.sync();
}

void Solver::so_set_amplitudes(Context& cx, const double* t1, const double* t2)
{
    so.amp_epoch = ++cx.amp_clock;
    amps_from_host(cx, so, t1, t2);
}

void Solver::so_get_lambda(Context& cx, double* l1, double* l2)
{
    SOLambda& L = so_lambda_need(so, "afesp_ccsd_so_get_lambda");
    if (l1) AFESP_HIP(hipMemcpyAsync(l1, L.l1.d, sizeof(double) * L.l1.size(), hipMemcpyDeviceToHost, cx.stream));
    if (l2) AFESP_HIP(hipMemcpyAsync(l2, L.l2.d, sizeof(double) * L.l2.size(), hipMemcpyDeviceToHost, cx.stream));
    cx.sync();
}

void Solver::so_set_lambda(Context& cx, const double* l1, const double* l2)
{
    SOLambda& L = so_lambda_need(so, "afesp_ccsd_so_set_lambda");
    L.stamp = ++cx.lam_clock;
    if (l1) AFESP_HIP(hipMemcpyAsync(L.l1.d, l1, sizeof(double) * L.l1.size(), hipMemcpyHostToDevice, cx.stream));
    if (l2) AFESP_HIP(hipMemcpyAsync(L.l2.d, l2, sizeof(double) * L.l2.size(), hipMemcpyHostToDevice, cx.stream));
    cx.sync();
}

void Solver::so_fetch_tensor(Context& cx, const char* name, double* out, int64_t capacity)
{
    SOState& s = so;
    if (!strcmp(name, "W_vvvv")) so_build_W_vvvv(cx, s);   // not formed by the iteration (so_ladder): built from the current t1 on request
    struct { const char* n; const Tensor* t; } tab[] = {
        {"F_vv", &s.F_vv}, {"F_oo", &s.F_oo}, {"F_ov", &s.F_ov}, {"W_oooo", &s.W_oooo}, {"W_vvvv", &s.W_vvvv},
        {"W_ovvo", &s.W_ovvo}, {"tau", &s.tau}, {"tau_tilde", &s.tau_t}, {"oovv", &s.oovv}, {"vvvv", &s.vvvv},
        {"t1", &s.t1}, {"t2", &s.t2}, {"f_ov", &s.f_ov}, {"f_oo", &s.f_oo}, {"f_vv", &s.f_vv}, {"D1", &s.D1}};
    // the intermediates of a live Lambda state (lambda_so.h), in its storage; G_vv / G_oo as of the last iteration or density
    static const char* const lam_names[] = {"H_ov", "H_oo", "H_vv", "H_oooo", "H_vovv", "H_ooov", "H_ovvo", "H_vvvo", "H_ovoo", "lam_tau", "G_vv", "G_oo"};
    for (size_t q = 0; q < sizeof(lam_names) / sizeof(lam_names[0]); ++q)
        if (!strcmp(lam_names[q], name)) {
            SOLambda& L = so_lambda_need(s, "afesp_ccsd_so_get_tensor");
            const Tensor* lam[] = {&L.Hov, &L.Hoo, &L.Hvv, &L.Hoooo, &L.Hvovv, &L.Hooov, &L.Hovvo, &L.Hvvvo, &L.Hovoo, &L.tau, &L.Gvv, &L.Goo};
            if (lam[q]->size() > capacity) throw Error(1, std::string("afesp_ccsd_so_get_tensor: buffer too small for ") + name);
            AFESP_HIP(hipMemcpyAsync(out, lam[q]->d, sizeof(double) * lam[q]->size(), hipMemcpyDeviceToHost, cx.stream));
            cx.sync();
            return;
        }
    if (!strcmp(name, "levels")) {   // the level of every spin orbital, occupied first: lev of a UHF- or Fock-fed state, the spatial e of an RHF-fed one
        const int64_t o = s.o, n = (int64_t)s.o + s.v;
        if (!s.ready || (!s.lev && !s.e)) throw Error(1, "afesp_ccsd_so_get_tensor: no spin-orbital state holds levels");
        if (n > capacity) throw Error(1, "afesp_ccsd_so_get_tensor: buffer too small for levels");
        if (s.lev) {
            AFESP_HIP(hipMemcpyAsync(out, s.lev, sizeof(double) * n, hipMemcpyDeviceToHost, cx.stream));
            cx.sync();
        } else {
            std::vector<double> e((size_t)(n / 2));
            AFESP_HIP(hipMemcpyAsync(e.data(), s.e, sizeof(double) * e.size(), hipMemcpyDeviceToHost, cx.stream));
            cx.sync();
            for (int64_t p = 0; p < n; ++p) out[p] = e[(size_t)(p < o ? p / 2 : (p - o) / 2 + o / 2)];   // (interleaved spins: ipea_level)
        }
        return;
    }
    for (auto& e : tab)
        if (!strcmp(e.n, name)) {
            if (!e.t->d) throw Error(1, std::string("afesp_ccsd_so_get_tensor: this state holds no ") + name + " (afesp_ccsd_uso_init_fock makes one that does)");
            if (e.t->size() > capacity) throw Error(1, std::string("afesp_ccsd_so_get_tensor: buffer too small for ") + name);
            AFESP_HIP(hipMemcpyAsync(out, e.t->d, sizeof(double) * e.t->size(), hipMemcpyDeviceToHost, cx.stream));
            cx.sync();
            return;
        }
    throw Error(1, std::string("afesp_ccsd_so_get_tensor: unknown tensor ") + name);
}

}  // namespace afesp
