// eom_so.h -- EOM-EE-CCSD excitation energies on the spin-orbital CCSD state.  The right-hand EOM matrix in the singles
// and doubles space is the Jacobian A = dR/dt of the residuals so_amplitudes evaluates before its division: sigma(r) = A r is contracted
// from the lambda-independent H-bar elements a live SOLambda keeps resident (borrowed, not copied), and the lowest eigenvalues of A come
// from a block Davidson iteration whose vectors never leave the device.  On full (i,j,a,b) storage <x, y> = sum x1 y1 + 1/4 sum x2 y2.
#pragma once
#include "davidson_so.h"
#include "lambda_so.h"

namespace afesp {

struct SOEom {
    Davidson d;                 // n1 = o v, nvec = o v + o^2 v^2, w2 = 1/4, diag = -D (the a,b-symmetrised mean of D2 behind the singles)
    bool left = false;          // the left-hand state (SOState::eom_left): its sigma is so_eom_lsigma, A^T in place of A, and it follows the
                                // states of the caller's guesses
};

// device bytes of the EOM state and the working set of a sigma build (beside so_state_bytes and so_lambda_bytes)
double so_eom_bytes(int64_t o, int64_t v, int nroots, int max_space);
// Needs a live Lambda state (LAMBDA_ERR_STALE otherwise; so_lambda_init refuses LAMBDA_ERR_FOO states); releases an earlier EOM state
// left: the left-hand Davidson state beside the right-hand one (SOState::eom_left; eigenvectors of A^T, the sigma build of
// so_eom_lsigma).  The two states share every rule and every line of code but the sigma build; no call with one flag touches the other.
void so_eom_init(Context& cx, SOState& s, int nroots, int max_space, bool left = false);
void so_eom_free(Context& cx, SOState& s);   // both states
// sigma = A r on device vectors [r1; r2] / [s1; s2] of length o v + o^2 v^2 (r2 antisymmetric in i,j and in a,b)
void so_eom_sigma(Context& cx, SOState& s, const double* r, double* sigma);
// host in / out: nvec vectors one after the other (the test entry)
void so_eom_sigma_host(Context& cx, SOState& s, int nvec, const double* r1, const double* r2, double* s1, double* s2);
// pending vectors: unit vectors on the nroots smallest -D over the unique amplitudes (ties by flat index), or the caller's own
void so_eom_guess(Context& cx, SOState& s, bool left = false);   // (-D is the diagonal of A^T too: the same unit vectors)
void so_eom_set_guess(Context& cx, SOState& s, int k, const double* r1, const double* r2, bool left = false);
// One Davidson step (davidson_iterate).  -> 1 when every root has |rho_k| < tol
int so_eom_iterate(Context& cx, SOState& s, double tol, bool left = false);
void so_eom_get_vector(Context& cx, SOState& s, int k, double* r1, double* r2, bool left = false);
SOEom& so_eom_need(SOState& s, const char* who, bool left = false);
// the diagonal guess of A as the Davidson unit reads it, -D, into a vector of o v + o^2 v^2 (the EE states' and the response state's)
void so_eom_fill_diag(Context& cx, SOState& s, double* diag);
void preload_eom_so();

// ---- the left-hand side (eom_left_so.hip)
// device bytes of the left Davidson state and the working set of a left sigma build and of a density call
double so_eom_left_bytes(int64_t o, int64_t v, int nroots, int max_space);
// sigma_L = A^T l on device vectors [l1; l2] / [s1; s2]: the X of so_lambda_iterate without its two inhomogeneous terms, minus D l, not
// divided.  G_vv / G_oo of l2 go to buffers of its own: nothing of the live Lambda state, of t1 / t2 or of either EOM state is written.
void so_eom_lsigma(Context& cx, SOState& s, const double* l, double* sigma);
void so_eom_lsigma_host(Context& cx, SOState& s, int nvec, const double* l1, const double* l2, double* s1, double* s2);
// c[k] = sum H_ia r_ia + 1/4 sum <ij||ab> r_ijab of nvec host vectors (r0 = c / omega is the caller's)
void so_eom_ref_coupling(Context& cx, SOState& s, int nvec, const double* r1, const double* r2, double* c);
// The symmetrised one-particle matrix of <0| (l0 + L) H-bar (r0 + R) |0> differentiated by f, (o+v)^2 column-major in the state's order;
// l1 / l2 both null or both given (host vectors), and r1 / r2 likewise: an absent vector is zero and is not read.
void so_eom_density(Context& cx, SOState& s, double l0, const double* l1, const double* l2, double r0, const double* r1, const double* r2,
                    double* d_host, int64_t capacity);
void preload_eom_left_so();

}  // namespace afesp
