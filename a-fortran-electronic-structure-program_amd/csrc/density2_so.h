// density2_so.h -- the correlation part of the two-particle density of spin-orbital CCSD.  With L(t, l) the Lagrangian
// of lambda_so.h and D the density of so_density, Gamma over all o + v spin orbitals (the state's order, occupied first) is
//   antisymmetric in p,q and in r,s,  Gamma_pqrs = Gamma_rspq  (the symmetry of real integrals),
//   normalised so that  L = sum_pq f_pq D_pq + 1/4 sum_pqrs <pq||rs> Gamma_pqrs  for every (f, g),
// i.e. Gamma is the derivative of L in g with f held fixed, as D is its derivative in f with g held fixed.  The full density
// <a+_p a+_q a_s a_r> adds the reference determinant's and the one-particle parts (afesp_amd.density.total_rdm2).
// Stored: the unique blocks oooo(i,j,k,l) ooov(i,j,k,a) oovv(i,j,a,b) ovov(i,a,j,b) ovvv(i,a,b,c), dense, first index fastest; vvvv only
// as ga(ab, cd), a < b, c < d, pair index a + b (b - 1) / 2, leading dimension SOState::lad_ka (the ladder's).  Every other block is an
// image of one of these.  No orbital relaxation.
#pragma once
#include "lambda_so.h"

namespace afesp {

struct SODensity2 {
    int64_t epoch = -1;    // SOState::amp_epoch of the build
    int64_t stamp = -1;    // SOLambda::stamp of the build: any writer of l1 / l2 draws a new one
    Tensor oooo, ooov, oovv, ovov, ovvv;
    double* ga = nullptr;  // (v(v-1)/2)^2 with leading dimension lad_ka; null when v < 2
};

// device bytes of the stored blocks and of the working set of a build
double so_density2_bytes(int64_t o, int64_t v);
// Builds Gamma for the current t and l of a live Lambda state (LAMBDA_ERR_STALE otherwise; LAMBDA_ERR_CAPACITY when it does not fit).
// Writes G_vv / G_oo of the Lambda state for the current l2 as so_density does, and nothing else of t, l or any other state.
void so_density2_build(Context& cx, SOState& s);
// name: oooo ooov oovv ovov ovvv (the stored block), vvvv_pairs ((v(v-1)/2)^2 dense, column-major), vvvv (the dense v^4 expansion) and
// full (the whole (o+v)^4 Gamma, first index fastest), the last two assembled on the host for small cases and tests
void so_density2_get(Context& cx, SOState& s, const char* name, double* out, int64_t capacity);
// e[0] = sum f D; e[1..6] = 1/4 sum <pq||rs> Gamma_pqrs over the family oooo, ooov, oovv, ovov, ovvv, vvvv with all its images; e[7] = their sum
void so_density2_energy(Context& cx, SOState& s, double* e);
// sum_pqrs Gamma_pqrs A_pr B_qs; A, B (o+v)^2 column-major on the host
double so_density2_expect(Context& cx, SOState& s, const double* A, const double* B);
void so_density2_free(Context& cx, SOLambda& L);
void preload_density2_so();

}  // namespace afesp
