// eom_ipea_so.h -- EOM-IP-CCSD and EOM-EA-CCSD on the spin-orbital CCSD state: ionisation potentials in the 1h + 2h1p
// sector, r = [r1(i); r2(i,j,a)] with r2 antisymmetric in i,j, and electron affinities in the 1p + 2p1h sector, r = [r1(a); r2(i,a,b)]
// with r2 antisymmetric in a,b.  Either sector is EOM-EE (eom_so.h) into a ghost orbital that interacts with nothing, so sigma(r) is
// contracted from the same H-bar elements of the live SOLambda (borrowed, not copied).  On full storage <x, y> = sum x1 y1 + 1/2 sum x2 y2.
// This unit holds what is the sectors' own -- the sigma build, the diagonal, the guess vectors; their Davidson states are driven by
// eom_so.h's driver (kinds EOM_KIND_IP, EOM_KIND_EA).
#pragma once
#include "eom_so.h"

namespace afesp {

// device bytes of a sector's state and the working set of one of its sigma builds
double so_eom_ipea_bytes(int64_t o, int64_t v, int sector, int nroots, int max_space);
// sigma = A r on device vectors [r1; r2] / [s1; s2] of the sector
void so_eom_ipea_sigma(Context& cx, SOState& s, int sector, const double* r, double* sigma);
// the diagonal of the sector's matrix on full storage: -e_i, -(e_i + e_j - e_a) / e_a, -(e_i - e_a - e_b)
void so_eom_ipea_fill_diag(Context& cx, SOState& s, int sector, double* diag);
// the flat indices of the unique amplitudes behind the first n1: (i < j, a) / (i, a < b), appended in the order the guesses break ties in
void so_eom_ipea_unique(const SOState& s, int sector, std::vector<int64_t>& idx);
// the guess on the unique amplitude p into x: +1 there, -1 on its image, and a fixed small admixture of every unique amplitude so that no
// Ms block or irreducible representation is invisible to the iteration
void so_eom_ipea_unit(Context& cx, SOState& s, int sector, double* x, int64_t p);
void preload_eom_ipea_so();

}  // namespace afesp
