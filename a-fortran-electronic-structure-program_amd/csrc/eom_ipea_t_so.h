// eom_ipea_t_so.h -- the non-iterative triples correction to EOM-IP-CCSD and EOM-EA-CCSD roots of the spin-orbital CCSD state (DESIGN.md
// 4.23): EOM-(T) of lambda_so.h's so_eom_triples in the ghost embedding that defines the sectors (eom_ipea_so.h), restricted to the 3h2p
// determinants (IP: i<j<k, a<b) or the 3p2h determinants (EA: i<j, a<b<c), which are the only triples of the enlarged system whose
// numerators do not vanish.  For a root w, a left vector (l1, l2) and a right vector (r1, r2) of the sector, H the bare Hamiltonian:
//   m(mu) = <mu| [H, R2] + [[H, R1], T2] |0>,   l(mu) = <0| (L1 + L2) H |mu>,   delta = sum_mu l(mu) m(mu) / (w - D_eps(mu)).
#pragma once
#include "eom_ipea_so.h"

namespace afesp {

// Items: IP the triples i<j<k in so_triples' numbering, EA the pairs i<j numbered j(j-1)/2 + i (device_util.h: pair_count, unpair_lt)
int64_t so_eom_ipea_t_items(int sector, int o);
// delta[nstates] over the items [begin, end).  The vectors are host arrays, nstates of them one after the other, in the sector's layout
// (IP l1[o], l2[o,o,v]; EA l1[v], l2[o,v,v]).  Uses g, f, the levels and t2; every buffer is this unit's own (ipt_*): nothing of t, lambda,
// the epochs of the amplitudes, a Lambda, EOM or response state or the operand copies of (T) / Lambda-(T) / EOM-(T) is written.
void so_eom_ipea_triples(Context& cx, SOState& s, int sector, int nstates, const double* omega, const double* l1, const double* l2,
                         const double* r1, const double* r2, int64_t begin, int64_t end, double* delta);
void preload_eom_ipea_t_so();

// ---- shared with triples.hip
void so_triples_guard(const SOState& s, const char* who);   // the state is there; a Fock state's oo / vv blocks are diagonal
// out[q] += sum of partial[q][0..nblk) for q < nq in a fixed order, two stages when there are many partials; `tmp` holds nq * 128 doubles
void sum_partials(Context& cx, double* out, const double* partial, int nq, int nblk, double* tmp);
int64_t device_pool_budget();                               // bytes of one (T) block pool (AFESP_T_POOL_GIB)

}  // namespace afesp
