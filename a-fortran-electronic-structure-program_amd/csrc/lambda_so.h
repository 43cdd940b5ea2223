// lambda_so.h -- the left-hand (Lambda) solution of spin-orbital CCSD and the unrelaxed one-particle density built from it
// (Gauss and Stanton, J. Chem. Phys. 103, 3561 (1995)).  With R1, R2 the residuals so_amplitudes evaluates before its
// division and L(t, l) = E(t) + sum l1 R1 + 1/4 sum l2 R2, the Lambda residual is G = dL/dt = X - D l; one iteration is the Jacobi step
// l <- l + G / D = X / D.  Everything in X that depends on t alone is built once (so_lambda_init) for one amp_epoch of the state.
#pragma once
#include <vector>
#include "ccsd_so.h"

namespace afesp {

struct SODensity2;   // density2_so.h
struct SORelax;      // relax_so.h

// statuses of the Lambda entry points beside 1 (argument error: no spin-orbital state) and 2 (HIP error)
constexpr int LAMBDA_ERR_FOO = 20;        // the state keeps the reference's transposed F_mi term: no consistent Lagrangian
constexpr int LAMBDA_ERR_STALE = 21;      // no Lambda state, or t1 / t2 may have changed since so_lambda_init
constexpr int LAMBDA_ERR_CAPACITY = 22;   // so_density: the caller's buffer is too small (density2_so.h: or the device memory)

struct SOLambda : DiisRing {   // amp = [l1 ; l2]
    int64_t epoch = -1;        // SOState::amp_epoch the intermediates were built for
    int64_t stamp = -1;        // ++Context::lam_clock by whoever writes l1 / l2 (init, iterate, diis, set_lambda): what copies of them go by
    Tensor l1, l2, x1, x2, l2_old;
    Tensor tau;                // of the t1 / t2 of `epoch` (the state's own tau is that of its last so_intermediates)
    // lambda-independent H-bar elements; Hoo / Hvv without the diagonal of f (the denominators)
    Tensor Hov, Hoo, Hvv;      // (m,e) (m,i) (a,e)
    Tensor Hoooo;              // (m,n,i,j)
    Tensor Hvovv, Hooov;       // (a,m,e,f) (m,n,i,e)
    Tensor Hovvo;              // (m,b,e,j)
    Tensor Hvvvo;              // H_abei stored (i,e,a,b)
    Tensor Hovoo;              // (m,b,i,j)
    Tensor Gvv, Goo;           // G_ae = -1/2 t_mnef l_mnaf, G_mi = 1/2 t_mnef l_inef, of the current l2
    double pseudo = 0.0, pseudo_old = 0.0, rms = 0.0;
    SODensity2* d2 = nullptr;  // the two-particle density built for one (epoch, stamp) (density2_so.h); released wherever this state is
    SORelax* rx = nullptr;     // the orbital gradient and Z-vector beside it (relax_so.h); released wherever d2 is
};

// ---- host helpers of every spin-orbital unit, written once
// A recording context (cx.rec) is refused by every entry above the T iteration: "<who>: <what> not part of a recorded ... sequence", e.g.
// ("so_lambda", "the Lambda equations are")
inline void so_need_plain(Context& cx, const char* who, const char* what)
{
    if (cx.rec) throw Error(1, std::string(who) + ": " + what + " not part of a recorded (launch-fused) sequence");
}
// the two-particle density built for the current t and lambda (density2_so.hip), or LAMBDA_ERR_STALE in the caller's name
SODensity2& so_density2_need(SOState& s, const char* who);
// C(alpha, A, "labels", B, "labels", beta, C, "labels"): contract() on one context, the form every term of these units is written in
inline auto contractor(Context& cx)
{
    return [&cx](double al, const Tensor& A, const char* la, const Tensor& B, const char* lb, double be, const Tensor& Cc, const char* lc) {
        contract(cx, al, A, la, B, lb, be, Cc, lc);
    };
}

// device bytes of the Lambda state and its working set (beside so_state_bytes)
double so_lambda_bytes(int64_t o, int64_t v, int diis_nerr);
// Builds the intermediates from the state's current t1 / t2 (converged or not) and sets l = t.  Throws LAMBDA_ERR_FOO on a state whose
// F_mi term is the reference's transposed one.
void so_lambda_init(Context& cx, SOState& s, int diis_nerr);
// the live Lambda state of `s`, or LAMBDA_ERR_STALE in the caller's name
SOLambda& so_lambda_need(SOState& s, const char* who);
void so_lambda_iterate(Context& cx, SOState& s);   // diis_save + one Jacobi update; the monitor sums are left for so_lambda_read
// pseudo energy 1/4 sum <ij||ab> l2 + sum f_ia l1 and sum (l2 - l2_old)^2; l2_old <- l2
void so_lambda_energy(Context& cx, SOState& s);
int so_lambda_read(Context& cx, SOState& s, double e_tol, double l_tol);   // the host read of either and the convergence rule
// the symmetrised correlation part of the unrelaxed one-particle density, (o+v)^2 column-major in the state's spin-orbital order
void so_density(Context& cx, SOState& s, double* d_host, int64_t capacity);
// the same matrix left on the device (the cached buffer lam_density, valid until the next call of either)
double* so_density_device(Context& cx, SOState& s, const char* who);
// The density blocks into the symmetric (o+v)^2 matrix D (device, column-major), every sum in a fixed order:
//   oo: 1/2 (doo(m,i) + doo(i,m)),  vv: 1/2 (dvv(a,e) + dvv(e,a)),  ov and vo: 1/2 (dov(m,e) + w t1(m,e) + l0 r1(m,e) + L1(m,e))
// (r1, L1 null: absent).  The ground state's is w = 1, no r1, L1 = l1; the EOM states': eom_left_so.hip.
void so_density_assemble(Context& cx, SOState& s, double* D, const double* doo, const double* dvv, const double* dov, const double* r1,
                         const double* L1, double w, double l0);
void so_relax_free(Context& cx, SOLambda& L);   // relax_so.hip
// Lambda-CCSD(T): the triples [t_begin, t_end) of so_triples' own list with l1 / l2 in the left factor (triples.hip)
double so_lambda_triples(Context& cx, SOState& s, int64_t t_begin, int64_t t_end);
// The triples correction to EOM-EE-CCSD excitation energies (triples.hip): nstates left / right vectors laid out as t1 / t2,
// one after the other (host); delta[nstates].  Needs no Lambda state.
void so_eom_triples(Context& cx, SOState& s, int nstates, const double* omega, const double* l1, const double* l2, const double* r1,
                    const double* r2, int64_t t_begin, int64_t t_end, double* delta);
void preload_lambda_so();

// afesp_profile on the spin-orbital drivers: three events per chunk (before the products, between them and the orbit pass, after it), read
// once the call's result is on the host; adds to Context::prof_gemm_ms / prof_orbit_ms as the spin-free driver does.  Nothing without it.
struct SOStamps {
    Context& cx;
    std::vector<hipEvent_t> evs;
    explicit SOStamps(Context& c) : cx(c) {}
    void stamp()
    {
        if (!cx.prof) return;
        hipEvent_t e;
        AFESP_HIP(hipEventCreate(&e));
        AFESP_HIP(hipEventRecord(e, cx.stream));
        evs.push_back(e);
    }
    void read()
    {
        if (!evs.empty()) AFESP_HIP(hipEventSynchronize(evs.back()));
        for (size_t q = 0; q + 2 < evs.size(); q += 3) {
            float a = 0.f, b = 0.f;
            AFESP_HIP(hipEventElapsedTime(&a, evs[q], evs[q + 1]));
            AFESP_HIP(hipEventElapsedTime(&b, evs[q + 1], evs[q + 2]));
            cx.prof_gemm_ms += a;
            cx.prof_orbit_ms += b;
            cx.prof_gemm_launches += 1;
            cx.prof_orbit_launches += 1;
        }
    }
    ~SOStamps() { for (hipEvent_t e : evs) (void)hipEventDestroy(e); }
};

}  // namespace afesp
