// davidson_so.h -- the block Davidson iteration for the lowest (or the followed) eigenvalues of a non-symmetric matrix that is given as a
// sigma build on device vectors.  A vector has n1 elements of weight 1 and nvec - n1 of weight w2 in the metric
// <x, y> = sum x1 y1 + w2 sum x2 y2; the vectors never leave the device.  The unit knows nothing of coupled cluster: its users are
// EOM-EE-CCSD, right and left (eom_so.h), and the EOM-IP and EOM-EA sectors (eom_ipea_so.h).
//
// Linear mode (davidson_linear_*; its user is response_so.h): the same basis, sigma storage, orthonormalisation, Gram panel
// collapse and fused pass solve (A - shift_j) x_j = -rhs_j for `nroots` systems at once on ONE basis -- every pending correction costs one sigma build
// that serves every system.  The eigenvalue entry points above are untouched by it.
//
// Complex linear mode (davidson_linear_start_complex): the shifts are complex, z_j = omega_j + i gamma_j, the matrix and the
// right-hand sides stay real.  The basis, sigma storage, G and prhs are the real ones; a solution x_j = P_j + i Q_j takes two columns
// (2 j: real part, 2 j + 1: imaginary part) of x, sx, corr and pend, the projected solve is a complex LU on the host, and one fused pass of
// its own (davidson_cfused_kernel) forms both columns of every system from one sweep over B and S.
#pragma once
#include "afesp_internal.h"

#include <functional>
#include <string>
#include <vector>

namespace afesp {

constexpr int EOM_FLAG_CONVERGED = 1;   // per-root flags of davidson_iterate
constexpr int EOM_FLAG_COMPLEX = 2;     // the projected root has an imaginary part: the real part of its vector is used

struct Davidson {
    int64_t epoch = -1;          // the owner's stamp of what the sigma build borrows (SOState::amp_epoch of the Lambda state)
    int nroots = 0, max_space = 0;
    int64_t n1 = 0, nvec = 0;    // elements of weight 1; all elements
    double w2 = 0.0;             // weight of the elements behind the first n1
    // A following state started from the caller's guesses keeps the states it was given: the Ritz values of its first step -- for
    // eigenvectors of the transposed matrix as guesses these are the roots themselves, their span being invariant -- and at every later
    // step the Ritz pairs nearest to them, not the lowest ones.  `target` empty: the lowest roots.
    bool follow = false;
    std::vector<double> target;
    int nb = 0;                  // basis columns b_p and their sigma_p
    int npend = 0;               // pending vectors (guesses or corrections) in `pend`
    bool user_guess = false;     // the pending vectors are the caller's: a further one joins them instead of starting over
    bool ritz = false;           // x / sx / omega are those of the current basis
    double *B = nullptr, *S = nullptr;        // max_space columns each
    double *pend = nullptr;                   // nroots columns
    double *x = nullptr, *sx = nullptr;       // Ritz vectors x_k = sum_p y_pk b_p and sum_p y_pk sigma_p, nroots columns each
    double *corr = nullptr;                   // the corrections of the last Ritz pass, nroots columns
    double *partial = nullptr, *sums = nullptr, *coef = nullptr;   // reduction partials, their ordered sums, coefficients (device)
    double *diag = nullptr;      // the diagonal guess of the matrix, nvec long: corr = rho / (omega - diag)
    std::vector<double> G;       // projected matrix <b_p, sigma_q>, max_space x max_space column-major (host)
    std::vector<double> omega, resnorm;
    std::vector<int> flags;
    int nsigma = 0, ncollapse = 0;
    // linear mode: system j has the shift `shift[j]` and the right-hand side column j % nrhs of `rhs` (device, nvec apart, borrowed);
    // prhs[p + max_space a] = <b_p, rhs_a> (host)
    const double* rhs = nullptr;
    int nrhs = 0;
    std::vector<double> shift, prhs;
    // complex linear mode: `wide` -- pend, x, sx, corr have 2 nroots columns and coef room for complex coefficients (davidson_alloc);
    // `cplx` -- the last start was davidson_linear_start_complex; shift_im[j] = gamma_j beside shift[j] = omega_j
    bool wide = false, cplx = false;
    std::vector<double> shift_im;
};

constexpr int DAVIDSON_ERR_POLE = 26;   // davidson_linear_iterate: a shift is at a root of the projected matrix

using DavidsonSigma = std::function<void(const double* r, double* sigma)>;   // sigma = A r on device vectors

// device bytes of a state
double davidson_bytes(double nvec, int nroots, int max_space);
double davidson_bytes_complex(double nvec, int nsys, int max_space);   // the same of a state allocated with wide = true
// fill_diag writes `diag` once (launches on cx.stream).  A failed allocation leaves what was allocated to the caller's davidson_free.
// wide: two columns per system in pend, x, sx and corr -- what davidson_linear_start_complex needs; every other entry point runs on a
// wide state as on a plain one.
void davidson_alloc(Context& cx, Davidson& D, int64_t n1, int64_t nvec, double w2, bool follow, int nroots, int max_space,
                    const std::function<void(double* diag)>& fill_diag, bool wide = false);
void davidson_free(Context& cx, Davidson& D);
void davidson_restart(Davidson& D);   // no basis, no pending vectors, no targets
// Messages carry the caller's names: prefix + "iterate", "guess", "set_guess", "get_vector".
// The caller's guess k from host halves of n1 and nvec - n1 elements; the first of a block of them starts over
void davidson_set_pending_from_host(Context& cx, Davidson& D, const std::string& prefix, int k, const double* r1, const double* r2);
// One step: (collapse if the pending vectors do not fit,) orthonormalise the pending vectors, build their sigma, extend the projected
// matrix, solve it on the host, Ritz pass.  -> 1 when every root has |rho_k| < tol
int davidson_iterate(Context& cx, Davidson& D, const std::string& prefix, double tol, const DavidsonSigma& sigma);
void davidson_get_vector(Context& cx, Davidson& D, const std::string& prefix, int k, double* r1, double* r2);
// ---- linear mode.  Start: no basis, and the pending vectors are the preconditioned right-hand sides rhs_j / (shift_j - diag) (the
// denominator guarded as the Ritz pass guards it).  nrhs columns in rhs, nroots shifts.
void davidson_linear_start(Context& cx, Davidson& D, const double* rhs, int nrhs, const double* shifts);
// One step: (collapse onto the current x_j if the pending vectors do not fit,) orthonormalise the pending vectors, build their sigma,
// extend the projected matrix and the projected right-hand sides, solve (G - shift_j) y_j = -B^T rhs_j on the host by LU, then one fused
// pass: x_j = B y_j, rho_j = rhs_j + (S - shift_j B) y_j, |rho_j| and the corrections rho_j / (shift_j - diag) of the systems with
// |rho_j| >= tol, which become the pending vectors scaled by 1 / |rho_j| (the drop threshold of the orthonormalisation is absolute).
// D.x holds the solutions, D.resnorm their residual norms, D.flags bit 0 |rho_j| < tol.  -> 1 when every system has converged.
// Throws DAVIDSON_ERR_POLE when a pivot of a projected system is below 1e-10 max(|G|_max, |shift_j|): the basis has been extended and
// the sigma builds counted by then, no pending vector is left, and a repeated call only solves the same systems and throws again.
// On a state started by davidson_linear_start_complex it makes the complex step below instead (D.cplx).
int davidson_linear_iterate(Context& cx, Davidson& D, const std::string& prefix, double tol, const DavidsonSigma& sigma);
// ---- complex linear mode: (A - z_j) x_j = -rhs_j with z_j = shift_re[j] + i shift_im[j], x_j = P_j + i Q_j, on a wide state with
// 4 nroots <= max_space and nroots <= 64.  Start: no basis; the pending vectors are Re and Im of rhs_j / (z_j - diag), in that order per
// system (where |z_j - diag| < 1e-4 the denominator is the real +-1e-4 with the sign of its real part, + for zero) -- a system with
// gamma_j = 0 gives an exactly zero imaginary vector, which the orthonormalisation drops.
// Step (davidson_linear_iterate): collapse onto Re x_j, Im x_j of every system in column order if the pending vectors do not fit; the
// pending vectors as in the real mode; (G - z_j) y_j = -B^T rhs_j by complex LU with partial pivoting on |pivot| on the host
// (DAVIDSON_ERR_POLE for |pivot| <= 1e-10 max(|G|_max, |z_j|)); one fused pass: P_j = B Re y_j, Q_j = B Im y_j, S P_j, S Q_j,
//   rho_re = rhs_j + S P_j - omega_j P_j + gamma_j Q_j,   rho_im = S Q_j - omega_j Q_j - gamma_j P_j,
// |rho_j|^2 = |rho_re|^2 + |rho_im|^2 in the unit's metric, and the corrections rho_j / (z_j - diag) (complex division, guarded as above);
// Re and Im of corr_j / |rho_j| of the systems with |rho_j| >= tol are the next pending vectors.  D.omega holds Re z_j.
void davidson_linear_start_complex(Context& cx, Davidson& D, const double* rhs, int nrhs, const double* shift_re, const double* shift_im);
// the fixed-order reduction of this unit for others: blocks of a partial-sum grid over nvec elements, and out[b] = the ordered sum of
// partial[b nblk .. (b + 1) nblk)
int davidson_reduce_blocks(int64_t nvec);
void davidson_reduce_final(Context& cx, double* out, const double* partial, int nout, int nblk);

}  // namespace afesp
