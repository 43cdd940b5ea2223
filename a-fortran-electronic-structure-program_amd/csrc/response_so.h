// response_so.h -- EOM-CCSD linear response on the spin-orbital CCSD state: static and dynamic polarisabilities.  For a
// real symmetric one-body operator X over the o + v spin orbitals, X-bar = exp(-T) X_N exp(T):
//   xi^X_mu = <mu| X-bar |0>                                   (so_response_xi: residual(f + X) - residual(f) at fixed t)
//   (A - omega) R^X(omega) = -xi^X                             (A: the matrix of so_eom_sigma; the linear mode of davidson_so.h)
//   <<X;Y>>_omega = Phi[X, R^Y(omega)] + Phi[Y, R^X(-omega)]
//   Phi[X, R] = Tr(X gamma(1, lambda; 0, R)) - Tr(X D) <lambda, R>    (gamma: so_eom_density, D: so_density)
// the EOM-CC response function of Stanton and Bartlett (no term quadratic in R).  The state borrows the H-bar elements of the live Lambda
// state through so_eom_sigma, has a basis of its own beside the EOM states, and writes nothing of t, lambda, the H-bar elements, a (T)
// plan or an EOM Davidson state.
#pragma once
#include "eom_so.h"

namespace afesp {

constexpr int RESPONSE_ERR_POLE = DAVIDSON_ERR_POLE;   // 26: a frequency is at a root of the projected EOM matrix
constexpr int RESPONSE_ERR_NOT_CONVERGED = 27;         // so_response_function: a solution it needs has |rho| >= tol of the last step (or no step yet)
constexpr int RESPONSE_MAX_SYSTEMS = 64;               // operators x signed frequencies of one state

struct SOResponse {
    Davidson d;                  // linear mode: system j = iop + nop ifreq, shift omega[ifreq], right-hand side xi_iop
    int nop = 0, nfreq = 0;
    std::vector<double> x;       // the operators, nop x (o+v)^2 column-major (host)
    std::vector<double> omega;   // the signed frequencies
    double* xi = nullptr;        // nop device vectors [xi1; xi2]
    int64_t lam_stamp = -1;      // SOLambda::stamp of the l1 / l2 the response function reads
    bool stepped = false;        // so_response_iterate has run: d.flags are those of its last step
    std::vector<double> phi;     // phi[a + nop j] = Phi[X_a, R_j] of the converged system j (so_response_function fills it)
    std::vector<char> have_phi;
    // complex frequencies (so_response_init_complex): z[ifreq] = omega[ifreq] + i gamma[ifreq], the Davidson state in its
    // complex linear mode, solution j = P_j + i Q_j, phi of P_j and phi_im[a + nop j] = Phi[X_a, Q_j] (Phi is linear in R)
    bool cplx = false;
    std::vector<double> gamma, phi_im;
};

// device bytes of the response state and the working set of its sigma builds and density calls
double so_response_bytes(int64_t o, int64_t v, int nop, int nsys, int max_space, bool cplx = false);
// nop operators (host, (o+v)^2 column-major each, symmetric: status 1 otherwise) -> nop vectors [xi1; xi2] one after the other at `xi`
// (device, o v + o^2 v^2 apart), at the state's current t1 / t2.  One dressed-operator kernel and one assemble kernel for the batch; an
// operator's vector does not depend on what else is in the batch.
void so_response_xi(Context& cx, SOState& s, int nop, const double* x_host, double* xi);
void so_response_xi_host(Context& cx, SOState& s, int nop, const double* x, double* xi1, double* xi2);   // host in / out (the test entry)
// Needs a live Lambda state (LAMBDA_ERR_STALE otherwise); releases an earlier response state.  nop >= 1, nfreq >= 1 signed frequencies,
// nop nfreq <= RESPONSE_MAX_SYSTEMS, 2 nop nfreq <= max_space <= 4096.
void so_response_init(Context& cx, SOState& s, int nop, const double* x, int nfreq, const double* omega, int max_space);
void so_response_free(Context& cx, SOState& s);
SOResponse& so_response_need(SOState& s, const char* who);
int so_response_iterate(Context& cx, SOState& s, double tol);   // one step of davidson_linear_iterate -> 1 when every system has converged
void so_response_get_vector(Context& cx, SOState& s, int iop, int ifreq, double* r1, double* r2);
// out[(f nop + a) nop + b] = <<X_a;X_b>>_omega[f] from the resident solutions at +omega and -omega: status 1 for a frequency that is not
// in the state's list, RESPONSE_ERR_NOT_CONVERGED for one whose solutions have not converged
void so_response_function(Context& cx, SOState& s, int nfreq, const double* omega, double* out);
// ---- complex frequencies z = omega + i gamma: (A - z) R^X(z) = -xi^X with R = P + i Q, A and xi real, on the complex
// linear mode of davidson_so.h; <<X;Y>>_z = Phi[X, R^Y(z)] + Phi[Y, R^X(-z)], the analytic continuation of the function above.
// z: nfreq (re, im) pairs.  Ownership, stamps and staleness as so_response_init; releases an earlier response state of either kind;
// 4 nop nfreq <= max_space <= 4096.  so_response_iterate steps whichever kind of state there is; the other entry points answer status 1
// on a state of the other kind.
void so_response_init_complex(Context& cx, SOState& s, int nop, const double* x, int nfreq, const double* z, int max_space);
void so_response_get_vector_complex(Context& cx, SOState& s, int iop, int ifreq, double* r1_re, double* r2_re, double* r1_im, double* r2_im);
// out[2 ((f nop + a) nop + b) + {0, 1}] = Re, Im of <<X_a;X_b>>_z[f].  R^X(-z) is the resident solution at -z where the list has it,
// otherwise the conjugate of the one at -conj(z) (R(conj z) = conj R(z); for an imaginary z that is z itself: one solve), otherwise
// status 1; RESPONSE_ERR_NOT_CONVERGED as above.
void so_response_function_complex(Context& cx, SOState& s, int nfreq, const double* z, double* out);
void preload_response_so();

}  // namespace afesp
