// eom_ipea_so.h -- EOM-IP-CCSD and EOM-EA-CCSD on the spin-orbital CCSD state: ionisation potentials in the 1h + 2h1p
// sector, r = [r1(i); r2(i,j,a)] with r2 antisymmetric in i,j, and electron affinities in the 1p + 2p1h sector, r = [r1(a); r2(i,a,b)]
// with r2 antisymmetric in a,b.  Either sector is EOM-EE (eom_so.h) into a ghost orbital that interacts with nothing, so sigma(r) is
// contracted from the same H-bar elements of the live SOLambda (borrowed, not copied).  On full storage <x, y> = sum x1 y1 + 1/2 sum x2 y2.
// This unit holds what is the sectors' own -- the sigma build, the diagonal, the guess vectors; their Davidson states are driven by
// eom_so.h's driver (kinds EOM_KIND_IP, EOM_KIND_EA).  The left-hand side of both sectors (eom_ipea_left_so.hip): the left
// sigma build sigma_L = A^T l, transposed in that metric, for the kinds EOM_KIND_IP_LEFT / EOM_KIND_EA_LEFT, and the Dyson orbitals.
#pragma once
#include "eom_so.h"

namespace afesp {

namespace {
// the level of spin orbital p (occupied first) of either kind of state: lev of a UHF- or Fock-fed one, the spatial e of an RHF-fed one
// (interleaved spins: so_denominators_kernel)
__device__ __forceinline__ double ipea_level(const double* e, const double* lev, int o, int p)
{
    return lev ? lev[p] : (p < o ? e[p / 2] : e[(p - o) / 2 + o / 2]);
}

// The diagonal of a sector's matrix on full storage.  IP: -e_i, then -((e_i + e_j) - e_a); EA: e_a, then (e_a + e_b) - e_i.  The bracketed
// sum is symmetric in the antisymmetric pair to the bit, so a product with an antisymmetric vector stays antisymmetric to the bit.
__device__ __forceinline__ double ipea_diag(int sector, const double* e, const double* lev, int o, int v, int64_t x)
{
    if (sector == EOM_SECTOR_IP) {
        if (x < o) return -ipea_level(e, lev, o, (int)x);
        const int64_t y = x - o;
        const int i = (int)(y % o), j = (int)((y / o) % o), a = (int)(y / ((int64_t)o * o));
        return -__dadd_rn(__dadd_rn(ipea_level(e, lev, o, i), ipea_level(e, lev, o, j)), -ipea_level(e, lev, o, o + a));
    }
    if (x < v) return ipea_level(e, lev, o, o + (int)x);
    const int64_t y = x - v;
    const int i = (int)(y % o), a = (int)((y / o) % v), b = (int)(y / ((int64_t)o * v));
    return __dadd_rn(__dadd_rn(ipea_level(e, lev, o, o + a), ipea_level(e, lev, o, o + b)), -ipea_level(e, lev, o, i));
}
}  // namespace

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
// W(i,a,b) = 1/2 sum_ef <ab||ef> x(i,e,f) of an x antisymmetric in e,f (<ab||ef> = <ef||ab>: the ladder of sigma and of sigma_L alike), in
// the T iteration's pair buffers where the state has them
void so_eom_ea_ladder_bare(Context& cx, SOState& s, const Tensor& x2, const Tensor& W);
void preload_eom_ipea_so();

// ---- the left-hand side (eom_ipea_left_so.hip)
// device bytes of a sector's left Davidson state and the working set of a left sigma build
double so_eom_ipea_left_bytes(int64_t o, int64_t v, int sector, int nroots, int max_space);
// sigma_L = A^T l on device vectors [l1; l2] / [s1; s2] of the sector: <l, sigma(r)> = <sigma_L(l), r> in the sector's metric.  Every
// intermediate of l2 goes to buffers of this unit: nothing of t1 / t2, lambda, the Lambda state or any EOM state is written.
void so_eom_ipea_lsigma(Context& cx, SOState& s, int sector, const double* l, double* sigma);
// The Dyson vectors of nvec left and / or right host vectors of the sector over all o + v spin orbitals, (o+v) x nvec column-major in the
// state's order: dl = <0| L e^-T a_p e^T |0>, dr = <0| (1 + Lambda) e^-T a_p^+ e^T R |0> (IP; a_p^+ / a_p for EA), phases by the ghost
// construction.  l1 / l2 both null (dl is not written) or both given, and r1 / r2 / dr likewise.  Needs the live Lambda state (it reads
// lambda) and no Davidson state; writes nothing resident.
void so_eom_ipea_dyson(Context& cx, SOState& s, int sector, int nvec, const double* l1, const double* l2, const double* r1, const double* r2,
                       double* dl, double* dr);
void preload_eom_ipea_left_so();

}  // namespace afesp
