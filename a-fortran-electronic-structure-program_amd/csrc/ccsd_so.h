// ccsd_so.h -- device-resident state of the spin-orbital CCSD solver and its (T) correction
// (reference: do_ccsd_spinorb ccsd.f90:71-277, build_tau/F/W :678-905, update_amplitudes :907-1038,
//  do_ccsd_t_spinorb :1812-1922).  Spin orbitals are interleaved alpha,beta as in ccsd.f90:108-143; o and v are
// spin-orbital counts (geometry.f90:44-45: nocc = nel, nvirt = 2 nbasis - nel).
#pragma once
#include "ccsd.h"

namespace afesp {

struct SOLambda;   // lambda_so.h
struct SOEom;      // eom_so.h
enum EomKind { EOM_KIND_EE = 0, EOM_KIND_EE_LEFT, EOM_KIND_IP, EOM_KIND_EA, EOM_KIND_IP_LEFT, EOM_KIND_EA_LEFT, EOM_KINDS };   // the EOM eigenproblems and their slots below
struct SOResponse; // response_so.h

struct SOState : DiisRing {
    int o = 0, v = 0, n = 0;
    bool ready = false;
    bool foo_as_published = false;   // see so_build_F
    double* e = nullptr;             // spatial orbital energies on device, length n (the RHF-fed state)
    double* lev = nullptr;           // ... or the level of every spin orbital, length o + v (the UHF-fed state, so_init_uhf)
    // antisymmetrised slices <pq||rs> (ccsd.f90:193-207)
    Tensor oooo, ooov, ovoo, oovo, oovv, ovvo, ovvv, vovv, vvvv;
    Tensor D1, D2, t1, t2, t2_old, r1, r2;
    Tensor F_vv, F_oo, F_ov, W_oooo, W_vvvv, W_ovvo, tau, tau_t;
    Tensor t1_w;                     // t1 as the last so_intermediates saw it
    double energy = 0.0, energy_old = 0.0, rms = 0.0;
    void* tplan = nullptr;           // cached (T) launch plan (triples_so.hip)
    int64_t amp_epoch = 0;           // bumped by every entry point that may change t1 / t2: the (T) operand copies are rebuilt only then
    // 1/2 tau_ijef W_abef (ccsd.f90:1021-1024) without W_abef (so_ladder): the bare part over antisymmetric pairs -- va(ef, ab) =
    // <ab||ef> for e < f, a < b built once, ta(ij, ef) = tau for i < j, e < f and the product pa(ij, ab) per iteration
    double *va = nullptr, *ta = nullptr, *pa = nullptr;
    int64_t* lad_tab = nullptr;
    int64_t lad_ka = 0, lad_na = 0;  // even leading dimensions: v(v-1)/2 and o(o-1)/2 rounded up
    // A state with a full Fock matrix (so_init_fock: a non-HF reference, e.g. a restricted open-shell determinant): the levels are its
    // diagonal (lev); f_ov(i,a), the off-diagonal f_oo(m,i) and the off-diagonal f_vv(a,e) in the state's spin-orbital order enter
    // Stanton's Eqs. 1-5 as extra terms.  Null on every other state, whose launches are those of before.
    bool fock = false;
    Tensor f_ov, f_oo, f_vv;
    double f_offdiag = 0.0;          // largest |f_oo|, |f_vv| off-diagonal element: (T) is defined for (semi)canonical orbitals only
    SOLambda* lam = nullptr;         // the Lambda state made by so_lambda_init for one amp_epoch (lambda_so.h); released by so_free
    SOEom* eom[EOM_KINDS] = {};      // the EOM states that borrow lam's H-bar elements, one per kind (eom_so.h); released wherever lam is
    SOResponse* resp = nullptr;      // the linear-response state beside them (response_so.h), released with it
};

// eri_mo_dev: packed chemist MO integrals on the device (length neri(nbasis)); e_host: spatial orbital energies (host)
void so_init(Context& cx, SOState& s, int nbasis, int nel, const double* eri_mo_dev, const double* e_host, int diis_nerr,
             bool foo_as_published);
// The same state from canonical UHF orbitals (n spatial functions, na alpha and nb beta electrons).  Spin-orbital order: occupied =
// alpha occupied (na), then beta occupied (nb); virtual = alpha virtual (n - na), then beta virtual (n - nb) -- o = na + nb, v = 2n - o.
// aa / bb: packed (8-fold) alpha-alpha / beta-beta MO integrals on the device; ab: ab[tri(p,q) npair + tri(r,s)] = (p q | r s),
// pq alpha, rs beta.  ea / eb: the n alpha / beta orbital energies (host).  F_mi always takes Stanton's published order.
void so_init_uhf(Context& cx, SOState& s, int nbasis, int na, int nb, const double* aa, const double* bb, const double* ab,
                 const double* ea_host, const double* eb_host, int diis_nerr);
// The UHF-ordered state on orbitals that do not diagonalise the spin Fock operators fa / fb (n x n, host, symmetric): levels from their
// diagonals, the rest kept as f_ov / f_oo / f_vv; the start amplitudes are t1 = f_ia / D_ia, t2 = <ij||ab> / D_ijab and the return value is
// sum f_ia^2 / D_ia + 1/4 sum <ij||ab>^2 / D_ijab (in semicanonical orbitals: the ROHF-MBPT(2) energy).
double so_init_fock(Context& cx, SOState& s, int nbasis, int na, int nb, const double* aa, const double* bb, const double* ab,
                    const double* fa_host, const double* fb_host, int diis_nerr);
// device bytes the dense spin-orbital state of o occupied and v virtual spin orbitals needs (iteration and (T) working set)
double so_state_bytes(int64_t o, int64_t v, int diis_nerr);
void so_free(Context& cx, SOState& s);
void so_intermediates(Context& cx, SOState& s);   // build_tau, build_F, build_W
void so_amplitudes(Context& cx, SOState& s);      // update_amplitudes
void so_build_W_vvvv(Context& cx, SOState& s);    // W_abef itself (ccsd.f90:852-861), on request: the iteration never forms it
int so_energy(Context& cx, SOState& s, double e_tol, double t_tol);
// out[b] = the sum of partial[b nblk .. (b + 1) nblk), b < nout, in a fixed order (device; the final sum of the CCSD and Lambda energy
// partials); f_ov given: block 0 adds sum_{x < n1} f_ov(x) l1(x) before its tree
void so_sum2(Context& cx, double* out, const double* partial, int nout, int nblk, const double* f_ov = nullptr, const double* l1 = nullptr,
             int64_t n1 = 0);
// out(ijab) = sum_{e<f} x(ijef) <ab||ef> over antisymmetric pairs against va (the bare part of so_amplitudes' ladder; x: tau or lambda_2)
void so_ladder_bare(Context& cx, SOState& s, const Tensor& x, const Tensor& out);
// xa(ij, ef) = x(i,j,e,f) for i < j, e < f with leading dimension lad_na: so_ladder_bare's packer, into a buffer of the caller's
void so_pair_pack(Context& cx, SOState& s, const Tensor& x, double* xa);
void so_lambda_free(Context& cx, SOState& s);     // lambda_so.hip (releases the EOM state too: it borrows from the Lambda state)
void so_eom_free(Context& cx, SOState& s);        // eom_so.hip (every kind)
void so_response_free(Context& cx, SOState& s);   // response_so.hip
// (T): contribution of the triples i<j<k with flat index in [t_begin, t_end) to E_T (ccsd.f90:1910)
int64_t so_triples_count(int o);
double so_triples(Context& cx, SOState& s, int64_t t_begin, int64_t t_end);
void so_triples_plan_free(SOState& s);

}  // namespace afesp
