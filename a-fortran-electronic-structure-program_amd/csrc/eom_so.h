// eom_so.h -- EOM-CCSD on the spin-orbital CCSD state: the right-hand EOM-EE matrix in the singles and doubles space is
// the Jacobian A = dR/dt of the residuals so_amplitudes evaluates before its division: sigma(r) = A r is contracted from the
// lambda-independent H-bar elements a live SOLambda keeps resident (borrowed, not copied), and the lowest eigenvalues of A come from a
// block Davidson iteration whose vectors never leave the device.  On full (i,j,a,b) storage <x, y> = sum x1 y1 + 1/4 sum x2 y2.
// The same driver serves the six eigenproblems -- EE, EE left (A^T), IP and EA (eom_ipea_so.h) and their left
// sides: one state
// type, one slot per kind in SOState::eom, and what differs per kind in one descriptor (eom_problem in eom_so.hip).
#pragma once
#include "davidson_so.h"
#include "lambda_so.h"

namespace afesp {

// EomKind (ccsd_so.h): EOM_KIND_EE, EOM_KIND_EE_LEFT, EOM_KIND_IP, EOM_KIND_EA, EOM_KIND_IP_LEFT, EOM_KIND_EA_LEFT.  The sectors of the C interface (AFESP_EOM_IP / AFESP_EOM_EA):
constexpr int EOM_SECTOR_IP = 1, EOM_SECTOR_EA = 2;
inline bool so_eom_sector_ok(int sector) { return sector == EOM_SECTOR_IP || sector == EOM_SECTOR_EA; }
inline EomKind so_eom_kind_of_sector(int sector, bool left = false)
{
    return sector == EOM_SECTOR_IP ? (left ? EOM_KIND_IP_LEFT : EOM_KIND_IP) : (left ? EOM_KIND_EA_LEFT : EOM_KIND_EA);
}

struct SOEom {
    Davidson d;                 // EE: n1 = o v, n2 = o^2 v^2, w2 = 1/4, diag = -D; IP: n1 = o, n2 = o^2 v; EA: n1 = v, n2 = o v^2; w2 = 1/2
    EomKind kind = EOM_KIND_EE; // its slot in SOState::eom.  The left state follows the states of the caller's guesses
};

// ---- the driver of every kind.  All need a live Lambda state (LAMBDA_ERR_STALE otherwise; so_lambda_init refuses LAMBDA_ERR_FOO states);
// no call for one kind touches the state of another.
// device bytes of the EE state and the working set of a sigma build (beside so_state_bytes and so_lambda_bytes)
double so_eom_bytes(int64_t o, int64_t v, int nroots, int max_space);
void so_eom_init(Context& cx, SOState& s, EomKind kind, int nroots, int max_space);   // releases an earlier state of that kind
void so_eom_free(Context& cx, SOState& s);                                            // every kind
// host in / out: nvec vectors one after the other through the kind's sigma build (the test entry); needs the Lambda state only
void so_eom_sigma_host(Context& cx, SOState& s, EomKind kind, int nvec, const double* r1, const double* r2, double* s1, double* s2);
// pending vectors: the kind's unit vectors on the nroots smallest diagonal elements over the unique amplitudes (ties by flat index), or
// the caller's own
void so_eom_guess(Context& cx, SOState& s, EomKind kind);
void so_eom_set_guess(Context& cx, SOState& s, EomKind kind, int k, const double* r1, const double* r2);
// One Davidson step (davidson_iterate).  -> 1 when every root has |rho_k| < tol
int so_eom_iterate(Context& cx, SOState& s, EomKind kind, double tol);
void so_eom_get_vector(Context& cx, SOState& s, EomKind kind, int k, double* r1, double* r2);
SOEom& so_eom_need(SOState& s, EomKind kind, const char* who);
constexpr const char *EOM_WHO = "so_eom", *EOM_PLAIN = "the EOM equations are";   // every EOM entry: so_need_plain(cx, EOM_WHO, EOM_PLAIN)

// ---- EE, right-hand side (eom_so.hip)
// sigma = A r on device vectors [r1; r2] / [s1; s2] of length o v + o^2 v^2 (r2 antisymmetric in i,j and in a,b)
void so_eom_sigma(Context& cx, SOState& s, const double* r, double* sigma);
// the diagonal guess of A as the Davidson unit reads it, -D, into a vector of o v + o^2 v^2 (the EE states' and the response state's)
void so_eom_fill_diag(Context& cx, SOState& s, double* diag);
void preload_eom_so();   // (this and the other two units' lists: once per process, whoever calls)

// ---- EE, left-hand side (eom_left_so.hip)
// device bytes of the left Davidson state and the working set of a left sigma build and of a density call
double so_eom_left_bytes(int64_t o, int64_t v, int nroots, int max_space);
// sigma_L = A^T l on device vectors [l1; l2] / [s1; s2]: the X of so_lambda_iterate without its two inhomogeneous terms, minus D l, not
// divided.  G_vv / G_oo of l2 go to buffers of its own: nothing of the live Lambda state, of t1 / t2 or of any EOM state is written.
void so_eom_lsigma(Context& cx, SOState& s, const double* l, double* sigma);
// sum_{x < n1} a1[x] y[x] + 1/4 sum_{x < n2} a2[x] y[n1 + x] of device vectors, block partials and the Davidson unit's ordered final sum:
// the metric <l, r> (a1 = l1, a2 = l2) and the reference coupling (a1 = H_ov, a2 = <ij||ab>).  -> the sum on the device, in a cached buffer
// that holds until the next call
const double* so_eom_wdot(Context& cx, const double* a1, const double* a2, const double* y, int64_t n1, int64_t n2);
// c[k] = sum H_ia r_ia + 1/4 sum <ij||ab> r_ijab of nvec host vectors (r0 = c / omega is the caller's)
void so_eom_ref_coupling(Context& cx, SOState& s, int nvec, const double* r1, const double* r2, double* c);
// The symmetrised one-particle matrix of <0| (l0 + L) H-bar (r0 + R) |0> differentiated by f, (o+v)^2 column-major in the state's order;
// l1 / l2 both null or both given (host vectors), and r1 / r2 likewise: an absent vector is zero and is not read.
void so_eom_density(Context& cx, SOState& s, double l0, const double* l1, const double* l2, double r0, const double* r1, const double* r2,
                    double* d_host, int64_t capacity);
void preload_eom_left_so();

}  // namespace afesp
