// solver.h -- the solver layer: the drivers of the two CCSD solvers between the C boundary (capi.hip checks the arguments) and the
// solvers' own steps (ccsd.h, ccsd_so.h).  What lives here and nowhere else: which form an iteration takes (launch-fused, large-tail,
// graph-replayed, plain) and the read that goes with it, the compiled programs of a state and when they die, who owns the packed
// integrals a state keeps for ccsd_need_vvvv, and the epoch stamp of everything that may change the amplitudes (solver.hip).
#pragma once
#include "ccsd_so.h"
#include "lambda_so.h"
#include "fused.h"

namespace afesp {

struct Integrals;   // integrals.h

// With the chains of a small-system iteration spread over lanes, issuing ~110 launches from the host (~4 us each) is
// what is left; from the second call on the iteration is therefore replayed as a hipGraph (captured across the
// lanes).  Only used where lanes are (small systems); AFESP_NO_GRAPH=1 keeps plain launches.
struct GraphSlot {
    hipGraphExec_t exec = nullptr;
    int64_t epoch = -1;      // Context::scratch_epoch at capture
    int calls = 0;
    bool disabled = false;
    void reset();
};

struct StepResult { double energy, rms; int converged; };   // what an energy evaluation or an iteration reports

// The two solver states of a context and their compiled programs.  Every function that may change t1 / t2 (resp. the CR intermediates)
// stamps the state's amp_epoch (cr_epoch) itself: what is derived from them -- the (T) operand copies, triples.hip -- is rebuilt then.
struct Solver {
    CCState cc;
    SOState so;
    GraphSlot graph_cc;
    // the launch-fused path of a small system (fused.h): the recorded and levelled call sequences of the spin-free solver --
    // intermediates alone, amplitudes alone (the term-by-term entry points) and the whole iteration
    FusedSlot fused_int, fused_amp, fused_iter;
    FusedSlot fused_so;   // ... and the spin-orbital iteration (build_tau / F / W + update_amplitudes)

    void cc_programs_reset(Context& cx);
    void so_programs_reset(Context& cx) { fused_slot_reset(cx, fused_so); }
    void destroy(Context& cx);   // the programs and the host-side plans; the states' device blocks go with the context
    // the state an entry point needs, or the caller's own message
    Solver& need_cc(const char* message) { if (!cc.ready) throw Error(1, message); return *this; }
    Solver& need_so(const char* message) { if (!so.ready) throw Error(1, message); return *this; }

    // ---- spin-free.  The packed MO integrals of init: `host` (uploaded; a large system's state keeps that copy for ccsd_need_vvvv), else
    // `dev` on the device -- the context's resident array (adopt = false) or one the caller filled for this state alone (adopt = true)
    void init(Context& cx, int o, int v, const double* host, double* dev, bool adopt, const double* levels, int diis_nerr);
    // the array at this address is going away: a state reading it can no longer form <ef|ab>
    void eri_gone(const double* packed) { if (cc.eri_src == packed) cc.eri_src = nullptr; }
    StepResult energy(Context& cx, double e_tol, double t_tol) { const int conv = ccsd_energy(cx, cc, e_tol, t_tol); return {cc.energy, cc.rms, conv}; }
    void update_intermediates(Context& cx);
    void update_amplitudes(Context& cx);
    StepResult iterate(Context& cx, double e_tol, double t_tol) { cc.amp_epoch = ++cx.amp_clock; return step(cx, e_tol, t_tol); }
    void diis(Context& cx) { cc.amp_epoch = ++cx.amp_clock; ccsd_diis_update(cx, cc); }
    // iter_energy / iter_rms_sq (maxiter + 1 entries, or null) per iteration; returns the iteration that converged, -1: none did
    int solve(Context& cx, int maxiter, double e_tol, double t_tol, double* iter_energy, double* iter_rms_sq);
    void get_amplitudes(Context& cx, double* t1, double* t2);
    void set_amplitudes(Context& cx, const double* t1, const double* t2);
    void fetch_tensor(Context& cx, const char* name, double* out, int64_t capacity);
    void cr_intermediates(Context& cx) { cc.cr_epoch = ++cx.amp_clock; ccsd_cr_intermediates(cx, cc); cx.sync(); }
    bool is_split(Context& cx) { ccsd_refresh_sharding(cx, cc); return cc.sharded; }
    int iteration_launches() const { return fused_launches(fused_iter.prog); }
    // Floating-point operations of one particle-particle ladder / one whole iteration as this state evaluates it
    double pp_ladder_flop() const;
    double iteration_flop() const;

    // ---- spin-orbital: from packed RHF-type integrals (`host`, else `dev`: resident), or from the three resident UHF blocks
    void so_init_packed(Context& cx, int nbasis, int nel, const double* host, const double* dev, const double* levels, int diis_nerr,
                        bool foo_as_published);
    void uso_init(Context& cx, const Integrals& in, int64_t nbasis, int64_t nalpha, int64_t nbeta, const double* levels_a,
                  const double* levels_b, int diis_nerr);
    double uso_init_fock(Context& cx, const Integrals& in, int64_t nbasis, int64_t nalpha, int64_t nbeta, const double* fock_a,
                         const double* fock_b, int diis_nerr);
    StepResult so_energy_step(Context& cx, double e_tol, double t_tol) { const int conv = so_energy(cx, so, e_tol, t_tol); return {so.energy, so.rms, conv}; }
    StepResult so_iterate(Context& cx, double e_tol, double t_tol);
    void so_diis(Context& cx) { so.amp_epoch = ++cx.amp_clock; diis_update(cx, so); }
    void so_get_amplitudes(Context& cx, double* t1, double* t2);
    void so_set_amplitudes(Context& cx, const double* t1, const double* t2);
    void so_fetch_tensor(Context& cx, const char* name, double* out, int64_t capacity);
    // ---- Lambda and the one-particle density of the spin-orbital state (lambda_so.h).  None of these writes t1 / t2 or stamps amp_epoch: the
    // Lambda state belongs to the epoch it was built for, and whatever stamps a new one makes it stale
    void so_lambda_begin(Context& cx, int diis_nerr) { so_lambda_init(cx, so, diis_nerr); }
    StepResult so_lambda_step(Context& cx, double e_tol, double l_tol) { so_lambda_iterate(cx, so); return so_lambda_result(cx, e_tol, l_tol); }
    StepResult so_lambda_energy_step(Context& cx, double e_tol, double l_tol) { so_lambda_energy(cx, so); return so_lambda_result(cx, e_tol, l_tol); }
    void so_lambda_diis(Context& cx)
    {
        SOLambda& L = so_lambda_need(so, "afesp_ccsd_so_lambda_diis");
        L.stamp = ++cx.lam_clock;
        diis_update(cx, L);
    }
    void so_get_lambda(Context& cx, double* l1, double* l2);
    void so_set_lambda(Context& cx, const double* l1, const double* l2);

private:
    StepResult so_lambda_result(Context& cx, double e_tol, double l_tol)
    {
        const int conv = so_lambda_read(cx, so, e_tol, l_tol);
        return {so.lam->pseudo, so.lam->rms, conv};
    }
    bool iteration_body(Context& cx);                              // true: read with ccsd_tail_read
    StepResult step(Context& cx, double e_tol, double t_tol);      // one iteration and the read that matches its form
    void uso_begin(Context& cx, const Integrals& in, const char* who, const char* hint, int64_t nbasis, int64_t nalpha, int64_t nbeta,
                   bool pointers_ok, int diis_nerr);
};

}  // namespace afesp
