// integrals_kernels.h -- the kernel wrappers of the integral layer (integrals_kernels.hip).  Only integrals.hip calls them: the AO Fock
// builds, the layout and pair-transform kernels of AO->MO, the orbital windows, the MP2 / UMP2 energies, the FNO amplitude gathers, the
// frozen-core fold, the FCIDUMP scatter, the MO Fock operators and the stream compaction.
#pragma once
#include "afesp_internal.h"

namespace afesp {

void k_mp2_energy(Context& cx, double* out1, const double* v_oovv, const double* D2, int o, int v);
double k_mp2_packed(Context& cx, const double* eri_packed, const double* e_host, int o, int v);   // the same from the packed MO integrals (device), one launch, result on the host; e_host: the n orbital energies
// pair-symmetric AO->MO: u(i,j,KL) from the packed array; out(k,l,PQ) = in(q,p,tri(k,l)); packed[tri(PQ,RS)] = full(s,r,PQ)
// (ld: leading dimension of the squared-up arrays, 0 = n; the LDS-DMA transforms pad it to whole K steps -- integrals_kernels.hip, pair_square_kernel)
void k_unpack_half(Context& cx, double* u, const double* packed, int n, int64_t c_begin = 0, int64_t c_end = -1, int ld = 0);   // slab of (kl) pairs
void k_pair_transpose(Context& cx, double* out, const double* in, int n, int ld = 0);
void k_pad_rows_zero(Context& cx, double* x, int n, int ld, int64_t ncol);   // x(n .. ld - 1, c) = 0 for every column c
// out(:,:,S) = C in(:,:,S) C^T for npairs symmetric n x n blocks, n <= 64: both quarter transforms of a pair index in one launch
void k_pair_xform(Context& cx, double* out, const double* in, const double* C, int n, int64_t npairs, int mode = 0);   // modes: integrals_kernels.hip
void k_square_transpose(Context& cx, double* out, const double* in, int64_t n);                                        // out(y, x) = in(x, y)
void k_pair_square_packed(Context& cx, double* out, const double* g, int n, int64_t c_begin, int64_t c_end);   // out(k,l,P) = g(P, tri(k,l))
void k_tri_pack(Context& cx, double* g, const double* half, int n, int64_t k_begin, int64_t k_end);           // g(PQ,K) = half(q,p,K)
void k_pack_pairs(Context& cx, double* packed, const double* full, int n, int64_t p_begin = 0, int64_t p_end = -1, int ld = 0);
void k_pack_cols(Context& cx, double* cols, const double* full, int n);   // cols[PQ np + RS] = full(s,r,PQ), every RS
// the active orbital window [lo, lo + n_act): packed over n -> packed over n_act; the [npair x npair] alpha-beta block likewise
void k_window_pack(Context& cx, double* dst, const double* src, int n_act, int lo);
void k_window_pairs(Context& cx, double* dst, const double* src, int n_act, int n, int lo);
// the padded coefficient transpose and the offset tables of a quarter transform on the LDS-DMA GEMM (integrals.hip, ao2mo_tg_prepare): every
// column of a slab, the columns (r, PQ) with r <= p(PQ) only, the columns x2 < cnt only -- one launch each, described at the kernels
void k_ao2mo_ct(Context& cx, double* ct, const double* c, int n, int Kc);
void k_ao2mo_tables(Context& cx, uint32_t* rowA, uint32_t* colB, int64_t* offCm, int64_t* offCn, int n, int Kc, int64_t ncol, int64_t ld);
void k_ao2mo_tables_tri(Context& cx, uint32_t* colB, int64_t* offCn, const int64_t* cstart, int n, int64_t np, int64_t sl, int64_t ld);
void k_ao2mo_tables_lo(Context& cx, uint32_t* colB, int64_t* offCn, int n, int cnt, int64_t ncol, int64_t ld);
// MP1 amplitude operands of the virtual-virtual MP2 density (afesp_mp2_vv_density / afesp_ump2_vv_density), gathered out of the resident
// MO integrals with the contraction index fastest; o active occupied orbitals from orbital nfc on, v virtuals from orbital nfc + o on,
// e_dev: the levels of the whole basis.  Each call leaves its share of the MP2 energy in cx.scal[slot].
//   k_fno_amps:    T(j,i,c; a) = (ia|jc) / D, Tt = 2 T - T with i and j exchanged (closed shell); Tt == nullptr: T = [(ia|jc) - (ic|ja)] / D
//                  alone, the same-spin amplitudes of one spin
//   k_fno_amps_ab: the opposite-spin amplitudes (ia|JB) / D out of the npair x npair alpha-beta block, beta_cols = false: T(J,B,i; a)
//                  (rows for D alpha), true: T(J,i,a; B) (rows for D beta)
void k_fno_amps(Context& cx, double* T, double* Tt, const double* packed, const double* e_dev, int nfc, int o, int v, int slot);
void k_fno_amps_ab(Context& cx, double* T, const double* ab, const double* ea_dev, const double* eb_dev, int n, int nfc, int oa, int ob, int va,
                   int vb, bool beta_cols, int slot);
// The field of the nfc frozen orbitals on the active window [nfc, nfc + n_act) (afesp_core_operator / afesp_ucore_operator): h_act (n_act x
// n_act, symmetric to the bit) = window of hmo (n x n) + the core's Coulomb and exchange out of the packed array over n orbitals, and
// *e_core = the core's own energy.  one_spin: the same-spin weights of an open shell (J - K, half the pair sum) instead of 2 J - K.
//   k_core_fold_ab: adds the opposite-spin Coulomb terms of the npair x npair alpha-beta block to both h_a and h_b; *e_core = sum_cD (cc|DD)
void k_core_fold(Context& cx, double* h_act, double* e_core, const double* hmo, const double* packed, int n, int nfc, int n_act, bool one_spin);
void k_core_fold_ab(Context& cx, double* h_a, double* h_b, double* e_core, const double* ab, int n, int nfc, int n_act);
// Order-preserving stream compaction: the elements of x[0, total) with |x| > thr as (flat index, value) pairs in rising index order.
//   k_compact_count:   counts[0 .. k_compact_chunks(total)] = exclusive prefix sums of the per-chunk survivor counts, the last = their number
//   k_compact_scatter: the pairs, into arrays of that many elements
int64_t k_compact_chunks(int64_t total);
void k_compact_count(Context& cx, int64_t* counts, const double* x, int64_t total, double thr);
void k_compact_scatter(Context& cx, int64_t* out_idx, double* out_val, const int64_t* prefix, const double* x, int64_t total, double thr);

// The FCIDUMP reader (afesp_read_fcidump / _uhf).  k_fcidump_scatter: `count` records (device copy of fcidump_parse.h's
// Record) into the targets, three launches: duplicates of earlier chunks checked against the visited map, stores, read-back; conflicting
// duplicates are counted in err[0], the smallest offending line number lands in err[1].  k_fock_mo: F = h + sum_{i < nocc} [wj (pq|ii) -
// (pi|qi)] over all n orbitals, one wave per pair, symmetric to the bit; k_fock_mo_ab adds the opposite-spin Coulomb terms to both spins.
namespace fcidump { struct Record; }
struct FcidumpTargets {
    double* eri[3];              // closed shell: [0] packed; open shell: aa, bb packed, ab npair x npair (row: alpha pair)
    double* h[2];                // n x n (open shell: alpha, beta)
    double* ecore;
    uint32_t* visited;           // one bit per slot
    unsigned long long* err;     // [0] conflicting duplicates, [1] smallest line number among them
    int64_t n, np, ne, nslots;   // spatial orbitals, npair, neri, number of slots (the core energy is the last one)
    int uhf;
};
void k_fcidump_scatter(Context& cx, const FcidumpTargets& T, const fcidump::Record* rec, int64_t count);
void k_fock_mo(Context& cx, double* F, const double* h, const double* packed, int n, int nocc, double wj);
void k_fock_mo_ab(Context& cx, double* fa, double* fb, const double* ab, int n, int na, int nb);
// The two spin Fock operators of the restricted determinant that fills the first na / nb orbitals, from h (n x n, device) and the packed
// MO integrals: one wave per pair, fixed summation order, symmetric to the bit
void k_fock_ro(Context& cx, double* fa, double* fb, const double* h, const double* packed, int n, int na, int nb);
// Fock matrix from the half-unpacked integrals u(x,y,P) (k_unpack_half); work holds k_build_fock_work(n) doubles
void k_build_fock(Context& cx, double* fock, const double* hcore, const double* dens, const double* u, double* work, int n, int ld = 0);
int64_t k_build_fock_work(int n);
// the unrestricted pair F_s = H + J[Da + Db] - K[D_s] on the same integrals; work holds k_build_fock_uhf_work(n) doubles
void k_build_fock_uhf(Context& cx, double* fa, double* fb, const double* hcore, const double* da, const double* db, const double* u,
                      double* work, int n, int ld = 0);
int64_t k_build_fock_uhf_work(int n);
// E(UMP2) from the resident alpha-alpha / beta-beta packed and alpha-beta full blocks (afesp_ao2mo_ump2), one launch, on the host
double k_ump2(Context& cx, const double* aa, const double* bb, const double* ab, const double* ea_dev, const double* eb_dev, int n, int na,
              int nb);

}  // namespace afesp
