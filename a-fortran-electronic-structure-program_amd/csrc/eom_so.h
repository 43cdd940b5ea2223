// eom_so.h -- EOM-EE-CCSD excitation energies on the spin-orbital CCSD state.  The right-hand EOM matrix in the singles
// and doubles space is the Jacobian A = dR/dt of the residuals so_amplitudes evaluates before its division: sigma(r) = A r is contracted
// from the lambda-independent H-bar elements a live SOLambda keeps resident (borrowed, not copied), and the lowest eigenvalues of A come
// from a block Davidson iteration whose vectors never leave the device.  On full (i,j,a,b) storage <x, y> = sum x1 y1 + 1/4 sum x2 y2.
#pragma once
#include "lambda_so.h"

#include <vector>

namespace afesp {

constexpr int EOM_FLAG_CONVERGED = 1;   // per-root flags of so_eom_iterate
constexpr int EOM_FLAG_COMPLEX = 2;     // the projected root has an imaginary part: the real part of its vector is used

struct SOEom {
    int64_t epoch = -1;          // SOState::amp_epoch of the Lambda state whose H-bar elements are borrowed
    int nroots = 0, max_space = 0;
    int64_t nvec = 0;            // o v + o^2 v^2
    int nb = 0;                  // basis columns b_p and their sigma_p
    int npend = 0;               // pending vectors (guesses or corrections) in `pend`
    bool user_guess = false;     // the pending vectors are the caller's (so_eom_set_guess): a further one joins them instead of starting over
    bool ritz = false;           // x / sx / omega / y are those of the current basis
    double *B = nullptr, *S = nullptr;        // max_space columns each
    double *pend = nullptr;                   // nroots columns
    double *x = nullptr, *sx = nullptr;       // Ritz vectors x_k = sum_p y_pk b_p and sum_p y_pk sigma_p, nroots columns each
    double *corr = nullptr;                   // the corrections of the last Ritz pass, nroots columns
    double *partial = nullptr, *sums = nullptr, *coef = nullptr;   // reduction partials, their ordered sums, coefficients (device)
    std::vector<double> G;       // projected matrix <b_p, sigma_q>, max_space x max_space column-major (host)
    std::vector<double> omega, resnorm;
    std::vector<int> flags;
    int nsigma = 0, ncollapse = 0;
    // The left state started from the caller's guesses follows the states it was given: the Ritz values of its first step -- for right
    // eigenvectors as guesses these are the right-hand roots themselves, their span being invariant under A -- and at every later step
    // the Ritz pairs nearest to them, not the lowest ones.  Empty: the lowest roots (every right-hand state, the unit guesses).
    std::vector<double> target;
    bool left = false;          // the left-hand state (SOState::eom_left): its sigma is so_eom_lsigma, A^T in place of A
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
// One Davidson step: (collapse if the pending vectors do not fit,) orthonormalise the pending vectors, build their sigma, extend the
// projected matrix, solve it on the host, Ritz pass.  -> 1 when every root has |rho_k| < tol
int so_eom_iterate(Context& cx, SOState& s, double tol, bool left = false);
void so_eom_get_vector(Context& cx, SOState& s, int k, double* r1, double* r2, bool left = false);
SOEom& so_eom_need(SOState& s, const char* who, bool left = false);
void preload_eom_so();
// the fixed-order reduction of this unit for its siblings: blocks of a partial-sum grid over nvec elements, and out[b] = the ordered
// sum of partial[b nblk .. (b + 1) nblk)
int so_eom_reduce_blocks(int64_t nvec);
void so_eom_reduce_final(Context& cx, double* out, const double* partial, int nout, int nblk);

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
