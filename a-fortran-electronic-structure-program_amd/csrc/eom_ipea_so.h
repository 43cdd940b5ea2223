// eom_ipea_so.h -- EOM-IP-CCSD and EOM-EA-CCSD on the spin-orbital CCSD state: ionisation potentials in the 1h + 2h1p
// sector, r = [r1(i); r2(i,j,a)] with r2 antisymmetric in i,j, and electron affinities in the 1p + 2p1h sector, r = [r1(a); r2(i,a,b)]
// with r2 antisymmetric in a,b.  Either sector is EOM-EE (eom_so.h) into a ghost orbital that interacts with nothing, so sigma(r) is
// contracted from the same H-bar elements of the live SOLambda (borrowed, not copied), and the lowest eigenvalues come from the block
// Davidson iteration of davidson_so.h.  On full storage <x, y> = sum x1 y1 + 1/2 sum x2 y2.
#pragma once
#include "davidson_so.h"
#include "lambda_so.h"

namespace afesp {

constexpr int EOM_SECTOR_IP = 1, EOM_SECTOR_EA = 2;

struct SOEomX {
    Davidson d;                 // IP: n1 = o, n2 = o^2 v; EA: n1 = v, n2 = o v^2; w2 = 1/2; diag = -e_i, -(e_i + e_j - e_a) / e_a, -(e_i - e_a - e_b)
    int sector = 0;
};

inline bool so_eom_sector_ok(int sector) { return sector == EOM_SECTOR_IP || sector == EOM_SECTOR_EA; }
// device bytes of a sector's state and the working set of one of its sigma builds
double so_eom_ipea_bytes(int64_t o, int64_t v, int sector, int nroots, int max_space);
// Needs a live Lambda state (LAMBDA_ERR_STALE otherwise); releases an earlier state of the same sector, leaves the other sector's and
// the EE state alone
void so_eom_ipea_init(Context& cx, SOState& s, int sector, int nroots, int max_space);
void so_eom_ipea_free(Context& cx, SOState& s);   // both sectors
// sigma = A r on device vectors [r1; r2] / [s1; s2] of the sector
void so_eom_ipea_sigma(Context& cx, SOState& s, int sector, const double* r, double* sigma);
// host in / out: nvec vectors one after the other (the test entry); needs the Lambda state only
void so_eom_ipea_sigma_host(Context& cx, SOState& s, int sector, int nvec, const double* r1, const double* r2, double* s1, double* s2);
// pending vectors: unit vectors on the nroots smallest diagonal elements over the unique amplitudes (ties by flat index), each with a fixed
// small admixture of every unique amplitude so that no Ms block or irreducible representation is invisible to the iteration
void so_eom_ipea_guess(Context& cx, SOState& s, int sector);
void so_eom_ipea_set_guess(Context& cx, SOState& s, int sector, int k, const double* r1, const double* r2);
int so_eom_ipea_iterate(Context& cx, SOState& s, int sector, double tol);   // one Davidson step -> 1 when every root has |rho_k| < tol
void so_eom_ipea_get_vector(Context& cx, SOState& s, int sector, int k, double* r1, double* r2);
SOEomX& so_eom_ipea_need(SOState& s, int sector, const char* who);
void preload_eom_ipea_so();

}  // namespace afesp
