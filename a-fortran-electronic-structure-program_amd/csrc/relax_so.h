// relax_so.h -- orbital relaxation of the spin-orbital CCSD density.  With L(f, g; t, l) the Lagrangian of lambda_so.h as
// a functional of the state's (f, g), D and Gamma its derivatives (so_density, density2_so.h), kappa antisymmetric over all o + v spin
// orbitals with kappa_ai = -kappa_ia its only elements and U = exp(kappa):
//   w0_ai = d/dkappa_ai L(U^T f U, g transformed by U on all four indices) at kappa = 0, t and l held fixed
//         = 2 (X_ai - X_ia),  X_pq = sum_r f_pr D_rq + 1/2 sum_rst <pr||st> Gamma_qrst;
//   w_ai  = w0_ai + 2 sum_pq D_pq <pa||qi>      (fock_response: f = h + sum_k <pk||qk> follows the occupied space);
//   A_ai,bj = delta_ab delta_ij (e_a - e_i) + <ab||ij> + <aj||ib>,   A z = -w;
//   D_rel = D + 1/2 z on the ov and vo blocks   (the Hartree-Fock Hessian in kappa is 2 A, the mixed derivative with h -> h + eps V is 2 V_ai).
// The two o v^4 terms of X -- <ab||cd> Gamma_ibcd and <ib||cd> Gamma_abcd -- run on the pair-stored va / ga through one kernel
// (relax_pair_row_kernel); everything else through contract().  w, z and the vectors of the solve are (i,a) arrays laid out as t1.
#pragma once
#include "density2_so.h"

namespace afesp {

constexpr int RELAX_ERR_NOT_HF = 24;          // the reference of a so_init_fock state is not stationary in the spin-orbital rotations
constexpr int RELAX_ERR_NOT_CONVERGED = 25;   // the Z-vector solve did not reach tol within maxiter, or broke down on p A p = 0 (a singular A)

struct SORelax {
    int64_t epoch = -1;    // SOState::amp_epoch of the converged solve in z
    int64_t stamp = -1;    // SOLambda::stamp of it
    double* vec = nullptr; // w, z, r, p, Ap, M^-1 r: six vectors of o v
    int iters = 0;
    int negative = 0;      // steps of the last solve along a direction of negative curvature (an unstable reference)
    double resid = 0.0;
};

double so_relax_bytes(int64_t o, int64_t v);
// Every call needs a live two-particle density of the current t and l (LAMBDA_ERR_STALE otherwise; nothing is read), refuses a recording
// context (1) and writes nothing of t, l, the epochs, the Lambda intermediates, Gamma, a (T) plan or an EOM state.
void so_orbital_gradient(Context& cx, SOState& s, int fock_response, double* w_host, int64_t capacity);
void so_zvector_apply(Context& cx, SOState& s, const double* x_host, double* y_host);
// preconditioned conjugate gradients from z = 0 on w with fock_response = 1; RELAX_ERR_NOT_HF on a so_init_fock state,
// RELAX_ERR_NOT_CONVERGED (iters / resid still reported) when tol is not reached; z_host may be null
void so_zvector_solve(Context& cx, SOState& s, double tol, int maxiter, double* z_host, int* iters, double* resid);
// needs the converged solve of the current t and l (LAMBDA_ERR_STALE otherwise)
void so_relaxed_density(Context& cx, SOState& s, double* d_host, int64_t capacity);
// out(i,a) = sum_b sum_{c<d} P(ab; cd) Q(i,b,c,d) alone (tools/relax_time.py and the tests time / check it apart): one warm call, then
// `reps` timed ones -> ms per call on the device; out_host may be null
double so_relax_pair_row(Context& cx, SOState& s, int which /* 0: (va, Gamma_ovvv), 1: (ga, <ib||cd>) */, double* out_host, int reps);
void preload_relax_so();

}  // namespace afesp
