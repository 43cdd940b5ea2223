// davidson_test.h -- the test entry to the block Davidson unit (davidson_so.h): one Davidson state per context whose
// operator is data, A = diag(d) + U V^T with U, V of nvec x r, so that tests/test_gpu_davidson.py can run the unit at any vector length,
// metric, root count and mode and read back everything it holds.  The state is separate from the EOM and response states, borrows
// nothing from a CCSD state and is freed with the context.  No product code path goes through this file.
#pragma once
#include "davidson_so.h"

namespace afesp {

struct DavidsonTest {
    Davidson d;
    int r = 0;                                      // columns of U and V
    double *dd = nullptr, *U = nullptr, *V = nullptr;   // the operator (device)
    double *vpart = nullptr, *vt = nullptr;         // block partials of V^T x and their ordered sums
    double* rhs = nullptr;                          // linear mode: the right-hand sides (device, nvec apart)
    bool linear = false;                            // the last start was davidson_test_linear_start
    int y_nb = -1;                                  // basis size of the last step that finished: its coefficients are what `coef` holds
};

// status 1 with a message unless 1 <= nvec, 0 <= n1 <= nvec, w2 > 0, 1 <= nroots <= nvec, 2 nroots <= max_space <= 4096, 0 <= r <= 64
void davidson_test_create(Context& cx, int64_t n1, int64_t nvec, double w2, int follow, int nroots, int max_space, int r, const double* d,
                          const double* U, const double* V, const double* diag);
void davidson_test_destroy(Context& cx);   // (no state: nothing)
DavidsonTest& davidson_test_need(Context& cx, const char* who);
void davidson_test_sigma(Context& cx, DavidsonTest& T, const double* x, double* s);   // s = d o x + U (V^T x), device vectors
void davidson_test_set_guess(Context& cx, int k, const double* x1, const double* x2);
int davidson_test_iterate(Context& cx, double tol);          // -> 1 when every root has converged
void davidson_test_linear_start(Context& cx, int nrhs, const double* rhs_host, const double* shifts);
// the complex linear mode (davidson_linear_start_complex): nroots shifts shift_re + i shift_im; status 1 unless 4 nroots <= max_space and
// nroots <= 64.  A state created for the real modes is allocated again with two columns per system, its diagonal carried over.
void davidson_test_linear_start_complex(Context& cx, int nrhs, const double* rhs_host, const double* shift_re, const double* shift_im);
int davidson_test_linear_iterate(Context& cx, double tol);   // (the real or the complex step, whichever start came last)
void davidson_test_get_vector(Context& cx, int k, double* x1, double* x2);
// what: B, S, pend (the first nb, nb, npend columns), x, sx, corr (nroots columns), diag, G (nb x nb column-major), prhs (nb x nrhs), y (the
// coefficients of the last step, nb x nr, and behind them the nr values of omega the Ritz pass was given; status 1 when no step has finished
// on the present basis -- before the first step, after a restart, after a step that threw at a pole --), target, counts ({nsigma,
// ncollapse, nb, npend}) -> the number of doubles written; status 1 when `capacity` is smaller.  After a complex start x, sx and corr hold
// 2 nroots columns (2 j: real part of system j, 2 j + 1: imaginary part) and y is Re y (nb x nroots), Im y (nb x nroots), then the nroots
// values of omega and of gamma; on a real state every string answers as it always did.
int64_t davidson_test_fetch(Context& cx, const char* what, double* out, int64_t capacity);

}  // namespace afesp
