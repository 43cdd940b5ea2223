/*
 * afesp.h -- C-ABI of libafesp_hip.so: the MI355X (gfx950) coupled-cluster engine behind the AFESP hot path.
 *
 * The reference (brianz98/A-Fortran-Electronic-Structure-Program) has no FFI: the path is entered by three
 * use-associated calls in src/main.F90:98,105,112.  This header is the boundary a Fortran host binds with
 * ISO_C_BINDING (interface block + binding in INTEGRATION.md): flat column-major fp64 arrays plus extents, exactly
 * what the reference already did for its own accelerator variant (do_ccsd_t_spinorb_acc, src/ccsd.f90:1924-1938).
 *
 * Conventions
 *   - every array is Fortran column-major, fp64, index order as declared in the reference
 *     (t1(o,v), t2(o,o,v,v): first index fastest; virtual indices 1..v with the o offset removed, src/ccsd.f90:429,438)
 *   - packed ERI arrays use the reference's 8-fold order (src/integrals.f90:187-210): ij = i(i-1)/2+j (i>=j, 1-based),
 *     ijkl = ij(ij-1)/2+kl (ij>=kl); length npair(npair+1)/2, npair = n(n+1)/2
 *   - canon_coeff is (MO, AO): row = MO, column = AO (src/hf.f90:102,127)
 *   - host pointers are borrowed for the duration of the call; device memory is owned by the context
 *   - every function returns 0 on success; non-zero -> afesp_last_error(ctx) (the Fortran host maps it to error(),
 *     src/error_handling.f90:7-20).  Without a usable GPU afesp_ctx_create fails: there is no CPU fallback.
 *   - extents are int64_t / int (the reference's int32 packed-index limit n<=99, src/integrals.f90:21, is lifted)
 *
 * Environment variables.  The library needs none.  Every AFESP_* variable it understands is defined, with its default, in ONE
 * place -- csrc/knobs.h -- and follows the environment at the granularity of one call of this header (re-read at the top of every
 * entry point; never in the middle of one).  Three kinds:
 *   TEST-ONLY path selectors (they choose which kernels evaluate a quantity; results agree to ~1e-13 but summation orders differ --
 *     tests use them to send a small system down a large system's path or to hold two forms of one product against each other; not
 *     for production use):  AFESP_SMALL_MAX, AFESP_NO_LANES, AFESP_FUSED, AFESP_FUSED_LANES, AFESP_PP_SYM, AFESP_RING_TG,
 *     AFESP_RING_TG_MIN, AFESP_RING_PACK, AFESP_LARGE_TAIL, AFESP_TALL, AFESP_TALL_MIN, AFESP_TALL_DUAL, AFESP_GETT_SK, AFESP_T_GEMM,
 *     AFESP_T_ONE_POOL, AFESP_CC_REINIT, AFESP_CC_SHARD, AFESP_CC_TIME_SLICE, AFESP_AO2MO_TG, AFESP_AO2MO_PAIR, AFESP_AO2MO_MIXED, AFESP_AO2MO_PAD,
 *     AFESP_AO2MO_BLOCKED, AFESP_MP2_PACKED, AFESP_NO_GRAPH, AFESP_GRAPH_AFTER, AFESP_NO_PRELOAD, AFESP_PRELOAD_LANES,
 *     AFESP_PRELOAD_GETT, AFESP_PLAN_VERIFY
 *   tuning (tile / slice / pool sizes, scheduling):  AFESP_PP_SPLIT, AFESP_PP_TILES, AFESP_REPACK_MIN, AFESP_PLAN_DEVICE_FROM,
 *     AFESP_FUSED_BIG_FLOP, AFESP_FUSED_ITEMS, AFESP_FUSED_MIN_STEPS, AFESP_FUSED_MAX_MFMA, AFESP_FUSED_NB, AFESP_SPLIT_BELOW,
 *     AFESP_SPLIT_MIN_STEPS, AFESP_TG_PATCH, AFESP_TG_GRID, AFESP_TG_PRIO_SHIFT, AFESP_TG_DYNAMIC, AFESP_T_BLOCK, AFESP_T_POOL_GIB,
 *     AFESP_T_SPLIT_TILES, AFESP_RELAX_MCAP, AFESP_RELAX_QCAP, AFESP_FCIDUMP_CHUNK_KIB
 *   diagnostics (printing, measurement; no effect on results):  AFESP_TG_DBG, AFESP_GRAPH_DEBUG, AFESP_PRELOAD_DEBUG,
 *     AFESP_FUSED_DEBUG, AFESP_FUSED_PER_OP, AFESP_GETT_DEBUG, AFESP_T_DEBUG, AFESP_CONTRACT_TRACE, AFESP_STAMPS_GROUPED
 */
#ifndef AFESP_H
#define AFESP_H
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct afesp_ctx afesp_ctx;

/* Context = one GPU (HIP device `device`), one stream, resident tensors.  One context per process per GPU. */
int afesp_ctx_create(int device, afesp_ctx** out);
void afesp_ctx_destroy(afesp_ctx* ctx);
const char* afesp_last_error(const afesp_ctx* ctx);
int afesp_version(void);
int64_t afesp_neri(int64_t nbasis); /* packed length, src/integrals.f90:175-176 */

/* Replaces `call do_mp2_spatial(sys, int_store)` (src/main.F90:98, src/mp2.f90:261-449).
 *   in : nbasis n, nocc o, canon_coeff[n*n] (MO,AO), canon_levels[n], eri_packed[neri] (AO basis; may be NULL after
 *        afesp_read_eri_text -- the AO integrals are then already on the device)
 *   out: eri_mo_packed[neri] (may be NULL: the MO integrals then stay on the device only), *e_mp2
 * The transformed integrals stay resident in the context for afesp_ccsd_init(..., eri_mo_packed = NULL). */
int afesp_ao2mo_mp2(afesp_ctx* ctx, int64_t nbasis, int64_t nocc, const double* canon_coeff, const double* canon_levels,
                    const double* eri_packed, double* eri_mo_packed, double* e_mp2);

/* Active orbital window [n_frozen_core, nbasis - n_frozen_virt) (frozen core / frozen virtuals; the reference has neither).  Replaces
 * the MO integrals resident after afesp_ao2mo_mp2 (eri_mo_packed == NULL) -- or takes them from the host -- by their window over
 * n_act = nbasis - n_frozen_core - n_frozen_virt orbitals, left resident exactly as afesp_ao2mo_mp2 leaves a basis of n_act functions:
 * afesp_ccsd_init(nocc - nfc, nvirt - nfv, NULL, canon_levels + nfc, ...), afesp_ccsd_so_init(n_act, nel - 2 nfc, NULL,
 * canon_levels + nfc, ...), the (T) calls, shard bounds and afesp_write_fcidump(n_act) then act on the window (with canonical orbitals
 * the active Fock matrix is diagonal with the same levels: no new equations).  *e_mp2 = frozen-core MP2 energy (mp2.f90:418-440 over
 * the active occupied / virtual orbitals).  eri_act (may be NULL) receives the packed window, neri(n_act) doubles.
 * A gather on the device after the full transform; the full array goes back to the context's arena inside the call, and a CCSD
 * state initialised from it can no longer form v_vvvv on request (as after a new afesp_ao2mo_mp2).  n_frozen_core = n_frozen_virt = 0
 * is legal and leaves the resident array as it is.
 * Status 1, with the resident integrals untouched: a negative count; no active occupied (nfc >= nocc) or no active virtual
 * (nfv >= nbasis - nocc) orbital left; NULL source with nothing resident for nbasis (so also a second window on a windowed context). */
int afesp_mo_window(afesp_ctx* ctx, int64_t nbasis, int64_t nocc, int64_t n_frozen_core, int64_t n_frozen_virt,
                    const double* canon_levels, const double* eri_mo_packed, double* eri_act, double* e_mp2);

/* Replaces init_cc + init_diis_cc_t (src/ccsd.f90:313-316, :404-615).
 *   eri_mo_packed: packed MO integrals from the host, or NULL to use the ones afesp_ao2mo_mp2 left on the device.
 *   diis_n_errmat: sys%ccsd_diis_n_errmat (<2 switches DIIS off, src/ccsd.f90:593-595). */
int afesp_ccsd_init(afesp_ctx* ctx, int64_t nocc, int64_t nvirt, const double* eri_mo_packed, const double* canon_levels,
                    int diis_n_errmat);

/* One pass of the loop body src/ccsd.f90:340-360: save t for DIIS, update_restricted_intermediates,
 * update_amplitudes_restricted, update_cc_energy.  *rms_sq is the UN-rooted sum of (dT2)^2 the reference stores and
 * prints (src/ccsd.f90:1806); *converged follows src/ccsd.f90:1805. */
int afesp_ccsd_iterate(afesp_ctx* ctx, double e_tol, double t_tol, double* energy, double* rms_sq, int* converged);
/* update_cc_energy alone on the current amplitudes (the "MP1" line, src/ccsd.f90:325). */
int afesp_ccsd_energy(afesp_ctx* ctx, double e_tol, double t_tol, double* energy, double* rms_sq, int* converged);
/* update_diis_cc (src/ccsd.f90:395, :617-676).  It extrapolates the amplitudes current at the call: a set handed in with
 * afesp_ccsd_set_amplitudes after the last afesp_ccsd_iterate is what enters the history. */
int afesp_ccsd_diis(afesp_ctx* ctx);
/* The whole solver loop src/ccsd.f90:325-396.  iter_energy / iter_rms_sq (length maxiter+1, may be NULL) receive the
 * iteration table incl. entry 0 = "MP1".  *niter = iterations taken, or -1 if not converged within maxiter. */
int afesp_ccsd_solve(afesp_ctx* ctx, int maxiter, double e_tol, double t_tol, double* iter_energy, double* iter_rms_sq,
                     int* niter);
/* Converged amplitudes (what move_alloc hands to int_store_cc, src/ccsd.f90:386-387). */
int afesp_ccsd_get_amplitudes(afesp_ctx* ctx, double* t1, double* t2);
/* t2 must carry the symmetry of closed-shell amplitudes, t2(i,j,a,b) = t2(j,i,b,a) -- every set the solver itself produces does, to the
 * bit; the residual is formed as r2 + its image and the pp-ladder over pair indices.  (A large system sums its DIIS overlaps over a <= b
 * only; for the nerr iterations in which the error vector of a handed-in set is part of the history it sums every element, so a set that
 * is symmetric up to rounding costs nothing in accuracy.) */
int afesp_ccsd_set_amplitudes(afesp_ctx* ctx, const double* t1, const double* t2);
/* Named device tensor -> host (tests / debugging).  Names: v_oovv v_ovov v_vvov v_oovo v_oooo v_vvvv I_vo I_vv I_oo_p
 * I_oo c_oovv asym_t2 x_voov I_oooo I_ovov I_voov I_vovv_p I_ooov_p r1 r2 D1 D2 t1 t2
 * (v_vvvv and I_vovv_p are not kept by a large system's iteration and are formed by this call; v_vvvv needs the packed MO
 * integrals the solver was initialised from: status 1 if afesp_ao2mo_mp2 has replaced them since afesp_ccsd_init;
 * r2 is the T2 residual before P(ia/jb) up to terms held as their images under (i <-> j, a <-> b): r2(ijab) + r2(jiba) is what
 * equals the same sum of the reference's tmp_t2, src/ccsd.f90:1720-1728)
 * Three more names are served only as a rank-split call left them (afesp_ccsd_set_split, or AFESP_CC_TIME_SLICE; read-only, for
 * tests/test_gpu_cc_split.py); otherwise status 1, with a message that says so, and the context stays usable:
 *   r1_sh   (o, v)        the rank-partial part of the T1 residual, as the last update of the amplitudes ran split: r1 - r1_sh is the
 *                         replicated part (with a communicator r1_sh is the sum over ranks and r1 the whole residual);
 *   pp      (o, o, v (v + 1) / 2)   the packed ladder PP(i,j,p), p = a + b (b + 1) / 2 over a <= b, same condition: this rank's rows,
 *                         zero elsewhere (with a communicator: the sum);
 *   ooov_sh (o, o, o, v)  the t2 <ef|ia> + t1 x_voov terms that the last update of the intermediates, run split, took out of
 *                         I_ooov_p(j,k,i,a) for this rank's slice of a; the buffer as it lies: outside the slice it holds what
 *                         earlier calls left there (at first: nothing defined). */
int afesp_ccsd_get_tensor(afesp_ctx* ctx, const char* name, double* out, int64_t capacity);
/* intermediates / amplitude equations separately (src/ccsd.f90:350,357), for term-by-term parity tests.  The two calls are ONE update
 * of one set of amplitudes, as in the reference's loop: terms are regrouped between them (the t1-dressed parts of I_vovv_p, the bare
 * t(i,e) <ab|ej> term), so amplitudes replaced in between give a residual that is neither the old nor the new one. */
int afesp_ccsd_update_intermediates(afesp_ctx* ctx);
int afesp_ccsd_update_amplitudes(afesp_ctx* ctx);

/* Replaces `call do_ccsd_t_spatial(...)` (src/main.F90:112, src/ccsd.f90:2018-2293) on the amplitudes resident in ctx.
 * The (i<=j<=k) triples are numbered 0..afesp_ccsd_t_ntriples-1; [t_begin, t_end) selects this rank's shard (the sums
 * of all shards are what one RCCL all-reduce combines; the D base term 1+2|t1|^2+asym.c, src/ccsd.f90:2243, is added by
 * the shard that holds triple 0).
 *   out[0] = E[T]  (src/ccsd.f90:2218-2219)     out[1] = E(T) incl. the z term (:2220 as in R/CR mode = the correct (T))
 *   out[2] = D[T]  (:2230-2231, :2243)          out[3] = D(T) (:2232) */
int64_t afesp_ccsd_t_ntriples(int64_t nocc);
int afesp_ccsd_t(afesp_ctx* ctx, int64_t t_begin, int64_t t_end, double out[4]);
/* Shard boundaries for `world` ranks: rank r evaluates [bounds[r], bounds[r+1]) (bounds has world+1 entries, bounds[0] = 0,
 * bounds[world] = afesp_ccsd_t_ntriples).  The reference splits the (i,j,k) loop `collapse(3) schedule(static,10)` over its
 * threads (src/ccsd.f90:2091); here the triples are evaluated block triple by block triple of the occupied index, and a block
 * triple cut by a shard end costs more per triple, so equal counts are not equal times: the boundaries equalise a cost
 * estimate instead.  Identical on every rank; cr != 0 for shards of afesp_ccsd_t_cr (its pool holds two sets of blocks).
 * Any other partition of the list is valid too -- the sums of the shards add up to the whole. */
int afesp_ccsd_t_shard_bounds(afesp_ctx* ctx, int64_t nocc, int64_t nvirt, int cr, int world, int64_t* bounds);
/* The same for the plain CCSD(T)_spatial / CCSD[T]_spatial types, which need neither y nor the D sums (the reference skips
 * them there as well, src/ccsd.f90:2181-2185, :2228-2247): out[0] = E[T], out[1] = E(T).  Cheaper: the z term is evaluated
 * once per element instead of at its six permutations (csrc/triples_orbit.h). */
int afesp_ccsd_t_plain(afesp_ctx* ctx, int64_t t_begin, int64_t t_end, double out[2]);

/* Completely renormalised CCSD[T]/(T).  afesp_ccsd_cr_intermediates replaces
 * build_cr_ccsd_t_intermediates (src/ccsd.f90:381, :2338-2551) and must be called on the converged amplitudes, before any
 * further afesp_ccsd_iterate.  afesp_ccsd_t_cr = afesp_ccsd_t plus the generalised-moment sums:
 *   out[4] = sum t_bar.M3 (src/ccsd.f90:2223-2224)   out[5] = out[4] + sum z_bar.M3 (:2225)
 * so that E_CR[T] = out[4]/out[2] and E_CR(T) = out[5]/out[3] (src/ccsd.f90:2268-2272).  Same sharding contract. */
int afesp_ccsd_cr_intermediates(afesp_ctx* ctx);
int afesp_ccsd_t_cr(afesp_ctx* ctx, int64_t t_begin, int64_t t_end, double out[6]);

/* Input/output side of the path.
 * afesp_read_eri_text replaces the two-body loop of read_integrals_in (src/integrals.f90:146-161): parses `eri.dat`
 * ("i j a b value", 1-based) straight into the 8-fold packed array and leaves it ON THE DEVICE, so that a following
 * afesp_ao2mo_mp2(..., eri_packed = NULL, ...) transforms without another host pass; eri_packed (may be NULL) also
 * receives the packed host copy the SCF needs, *nread the number of lines.
 * afesp_write_fcidump replaces write_fcidump (src/mp2.f90:451-487) from the MO integrals resident after
 * afesp_ao2mo_mp2: same line format (I3,I3,I3,I3,ES17.9), same 1e-7 threshold, same (header-less) content. */
int afesp_read_eri_text(afesp_ctx* ctx, const char* path, int64_t nbasis, double* eri_packed, int64_t* nread);
/* The same residency from an array the caller already holds (int_store%eri). */
int afesp_set_eri(afesp_ctx* ctx, int64_t nbasis, const double* eri_packed);
/* Replaces build_fock (src/hf.f90:349-385), the O(n^4) step of every SCF iteration, on the resident packed AO
 * integrals: fock(i,j) = core_hamil(i,j) + sum_kl density(k,l) [2 (ij|kl) - (ik|jl)]; n x n column-major host arrays. */
int afesp_build_fock(afesp_ctx* ctx, int64_t nbasis, const double* density, const double* core_hamil, double* fock);
int afesp_write_fcidump(afesp_ctx* ctx, const char* path, int64_t nbasis, int64_t* nwritten);

/* Spin-orbital path: replaces `call do_ccsd_spinorb(sys, int_store, int_store_cc)` (src/main.F90:67,
 * src/ccsd.f90:71-277) and `call do_ccsd_t_spinorb(...)` (src/main.F90:79, src/ccsd.f90:1812-1922).
 * Spin orbitals are interleaved alpha,beta (src/ccsd.f90:108-143); the spin-orbital extents are the reference's
 * (src/geometry.f90:44-45): nocc = nel, nvirt = 2*nbasis - nel.  Arrays: t1(nocc,nvirt), t2(nocc,nocc,nvirt,nvirt).
 *   afesp_ccsd_so_init    = antisymmetrised integrals + slices (:108-207), init_cc(.not.restricted), init_diis_cc_t.
 *                           eri_mo_packed NULL = the MO integrals afesp_ao2mo_mp2 left on the device; canon_levels has
 *                           nbasis entries (spatial).  flags bit 0 (AFESP_SO_FOO_AS_PUBLISHED): put the tau~ term of F_mi
 *                           where Stanton's Eq. 4 has it; by default it lands transposed, as src/ccsd.f90:789-794 codes it
 *                           (the reference's shipped ref_out predates that dgemm and needs the flag to be reproduced).
 *   afesp_ccsd_so_energy  = update_cc_energy, unrestricted branch (:1783-1806); same outputs as afesp_ccsd_energy.
 *   afesp_ccsd_so_iterate = build_tau, build_F, build_W, update_amplitudes, update_cc_energy (:229-251 loop body).
 *   afesp_ccsd_so_diis    = update_diis_cc (:274).
 *   afesp_ccsd_so_t       = E_T of src/ccsd.f90:1910 restricted to the triples i<j<k numbered [t_begin, t_end) of
 *                           afesp_ccsd_so_t_ntriples(nocc) (the summand is antisymmetric in i,j,k; shards add up). */
#define AFESP_SO_FOO_AS_PUBLISHED 1
int afesp_ccsd_so_init(afesp_ctx* ctx, int64_t nbasis, int64_t nel, const double* eri_mo_packed, const double* canon_levels,
                       int diis_n_errmat, int flags);
int afesp_ccsd_so_energy(afesp_ctx* ctx, double e_tol, double t_tol, double* energy, double* rms_sq, int* converged);
int afesp_ccsd_so_iterate(afesp_ctx* ctx, double e_tol, double t_tol, double* energy, double* rms_sq, int* converged);
int afesp_ccsd_so_diis(afesp_ctx* ctx);
int afesp_ccsd_so_get_amplitudes(afesp_ctx* ctx, double* t1, double* t2);
int afesp_ccsd_so_set_amplitudes(afesp_ctx* ctx, const double* t1, const double* t2);
/* name: F_vv F_oo F_ov W_oooo (stored i,j,m,n) W_vvvv (stored e,f,a,b) W_ovvo tau tau_tilde oovv vvvv t1 t2, D1 (the singles denominators
 * e_i - e_a), levels (the level of every spin orbital, nocc + nvirt of them, occupied first).
 * With a live Lambda state (afesp_ccsd_so_lambda_init; status 21 without one or with a stale one) also its t-fixed intermediates:
 * H_ov (m,e) H_oo (m,i) H_vv (a,e) H_oooo (m,n,i,j) H_vovv (a,m,e,f) H_ooov (m,n,i,e) H_ovvo (m,b,e,j) H_vvvo (H_abei stored i,e,a,b)
 * H_ovoo (m,b,i,j) lam_tau (i,j,a,b), and G_vv (a,e) G_oo (m,i) as of the last afesp_ccsd_so_lambda_iterate / afesp_ccsd_so_density */
int afesp_ccsd_so_get_tensor(afesp_ctx* ctx, const char* name, double* out, int64_t capacity);
int64_t afesp_ccsd_so_t_ntriples(int64_t nocc);
int afesp_ccsd_so_t(afesp_ctx* ctx, int64_t t_begin, int64_t t_end, double* e_t);

/* The left-hand (Lambda) solution of spin-orbital CCSD and the unrelaxed one-particle density built from it (since
 * afesp_version 2).  With R1, R2 the CCSD residuals (Stanton et al. Eqs. 1-2 minus D t, f terms included) and
 *   L(t, l) = E(t) + sum l_ia R1_ia + 1/4 sum l_ijab R2_ijab
 * the Lambda residual is G = dL/dt and the Lambda equations are G = 0, linear in l.  Any spin-orbital state takes them (afesp_ccsd_so_init
 * with AFESP_SO_FOO_AS_PUBLISHED, afesp_ccsd_uso_init, afesp_ccsd_uso_init_fock); l1 [o*v] and l2 [o*o*v*v] are laid out as t1 / t2.
 *   afesp_ccsd_so_lambda_init    = the t-dependent intermediates from the state's CURRENT t1 / t2 (converged or not: the equations are
 *                                  defined for any t), l = t, and a DIIS ring of diis_n_errmat vectors (0 .. 15; < 2: none).
 *   afesp_ccsd_so_lambda_iterate = one Jacobi step l <- l + G / D (D: the denominators of the T iteration); *pseudo_energy = 1/4 sum
 *                                  <ij||ab> l_ijab + sum f_ia l_ia, *rms_sq = sum (l2 - l2_old)^2, *converged = sqrt(rms_sq) < l_tol and
 *                                  |pseudo_energy - its previous value| < e_tol, as afesp_ccsd_so_iterate reports its numbers.
 *   afesp_ccsd_so_lambda_energy  = the same three outputs of the l that is there.
 *   afesp_ccsd_so_lambda_diis    = update_diis_cc on the Lambda ring.
 *   afesp_ccsd_so_get_lambda / _set_lambda: either pointer may be NULL.
 *   afesp_ccsd_so_density        = d [(o+v)^2, column-major, the state's spin-orbital order, occupied first] = 1/2 (dL/df_pq + dL/df_qp)
 *                                  at the current t and l: the correlation part, symmetrised; the full density adds 1 on the occupied
 *                                  diagonal.  No orbital relaxation.
 * Call order: converge CCSD -> _lambda_init -> [_lambda_iterate, _lambda_diis] until converged -> _density.  None of them writes t1 / t2, so
 * afesp_ccsd_so_t before and after gives the same bits.  Every call that may change t1 / t2 (_iterate, _diis, _set_amplitudes, an init)
 * makes the Lambda state stale; it is then refused, never recomputed on stale intermediates.
 * Statuses, each with afesp_last_error: 1 no spin-orbital state (or a bad diis_n_errmat); AFESP_LAMBDA_UNPUBLISHED_FOO a state made by
 * afesp_ccsd_so_init without AFESP_SO_FOO_AS_PUBLISHED (the reference's transposed F_mi term has no consistent Lagrangian);
 * AFESP_LAMBDA_STALE no Lambda state or a stale one; AFESP_LAMBDA_CAPACITY capacity < (o+v)^2 (nothing is launched). */
#define AFESP_LAMBDA_UNPUBLISHED_FOO 20
#define AFESP_LAMBDA_STALE 21
#define AFESP_LAMBDA_CAPACITY 22
int afesp_ccsd_so_lambda_init(afesp_ctx* ctx, int diis_n_errmat);
int afesp_ccsd_so_lambda_iterate(afesp_ctx* ctx, double e_tol, double l_tol, double* pseudo_energy, double* rms_sq, int* converged);
int afesp_ccsd_so_lambda_energy(afesp_ctx* ctx, double e_tol, double l_tol, double* pseudo_energy, double* rms_sq, int* converged);
int afesp_ccsd_so_lambda_diis(afesp_ctx* ctx);
int afesp_ccsd_so_get_lambda(afesp_ctx* ctx, double* l1, double* l2);
int afesp_ccsd_so_set_lambda(afesp_ctx* ctx, const double* l1, const double* l2);
int afesp_ccsd_so_density(afesp_ctx* ctx, double* d, int64_t capacity);

/* The two-particle density of spin-orbital CCSD: the correlation part Gamma of the current t and l of a live Lambda state,
 * over all o + v spin orbitals in the state's order (occupied first).  Gamma is antisymmetric in p,q and in r,s, Gamma_pqrs = Gamma_rspq (the
 * symmetry of real integrals), and normalised so that
 *   L = sum_pq f_pq D_pq + 1/4 sum_pqrs <pq||rs> Gamma_pqrs     for every (f, g), D that of afesp_ccsd_so_density
 * -- the derivative of L in g with f held fixed: for p<q, r<s and x the perturbation with +-eps on the antisymmetric images of (pq,rs) and
 * of (rs,pq), [L(g+x) - L(g-x)] / 2 eps is Gamma_pqrs if (pq) = (rs) and 2 Gamma_pqrs otherwise.  With g0 the reference determinant's
 * occupation matrix the full density <a+_p a+_q a_s a_r> is
 *   Gtot_pqrs = (g0_pr g0_qs - g0_ps g0_qr) + (D_pr g0_qs + D_qs g0_pr - D_ps g0_qr - D_qr g0_ps) + Gamma_pqrs,
 * E_elec = sum h gamma + 1/4 sum g Gtot, and <S^2> = N/2 + Ms^2 - sum_PQ Gtot[P beta, Q alpha, Q beta, P alpha] in one common spatial
 * basis.  At converged t and l, sum f D + 1/4 sum g Gamma is the CCSD correlation energy.  No orbital relaxation.
 *   afesp_ccsd_so_density2_build  = Gamma for the current t and l: the unique blocks oooo ooov oovv ovov ovvv, and vvvv only over
 *                                   antisymmetric pairs (no dense v^4 array exists on the device).  Any later writer of t1 / t2 or l1 / l2
 *                                   makes the build stale; the calls below then return AFESP_LAMBDA_STALE and read nothing.
 *   afesp_ccsd_so_density2_get    = name: oooo (i,j,k,l) ooov (i,j,k,a) oovv (i,j,a,b) ovov (i,a,j,b) ovvv (i,a,b,c), the stored block, first
 *                                   index fastest; vvvv_pairs (ab,cd), a<b, c<d, pair index a + b (b - 1) / 2, [v(v-1)/2]^2 column-major; vvvv,
 *                                   the dense v^4 expansion, and full, the whole (o+v)^4 Gamma, both written on the host for small cases
 *                                   and tests.  Every block is antisymmetric / pair-symmetric to the bit, with zero diagonals.
 *   afesp_ccsd_so_density2_energy = e[0] = sum f D with the state's f (levels on the diagonal, f_ov / f_oo / f_vv where it has them);
 *                                   e[1..6] = 1/4 sum <pq||rs> Gamma_pqrs over the family oooo, ooov, oovv, ovov, ovvv, vvvv with all its
 *                                   images; e[7] = e[1] + ... + e[6].
 *   afesp_ccsd_so_density2_expect = *value = sum_pqrs Gamma_pqrs A_pr B_qs; A, B [(o+v)^2, column-major, the state's order].  The
 *                                   reference and one-particle parts of a two-body expectation value are one-body algebra of the caller.
 * None of them writes t1 / t2, l1 / l2, the epochs, the Lambda intermediates (G_vv / G_oo are rebuilt for the current l as
 * afesp_ccsd_so_density does), a (T) plan or an EOM state.  The build is released with the Lambda state.
 * Statuses: 1 no spin-orbital state, a NULL argument, an unknown name or a recording context; AFESP_LAMBDA_UNPUBLISHED_FOO as
 * afesp_ccsd_so_lambda_init; AFESP_LAMBDA_STALE no live Lambda state (build) or no live build (get / energy / expect);
 * AFESP_LAMBDA_CAPACITY capacity too small (nothing is launched) or the build does not fit the device memory. */
int afesp_ccsd_so_density2_build(afesp_ctx* ctx);
int afesp_ccsd_so_density2_get(afesp_ctx* ctx, const char* name, double* out, int64_t capacity);
int afesp_ccsd_so_density2_energy(afesp_ctx* ctx, double* e /* [8] */);
int afesp_ccsd_so_density2_expect(afesp_ctx* ctx, const double* A, const double* B, double* value);

/* Orbital relaxation of the spin-orbital CCSD density (afesp_version 3).  With L(f, g; t, l) the Lagrangian above as a
 * functional of the state's (f, g), kappa an antisymmetric matrix over all o + v spin orbitals whose only non-zero elements are
 * kappa_ai = -kappa_ia, and U = exp(kappa):
 *   afesp_ccsd_so_orbital_gradient = w[i + o a], laid out as t1.  fock_response = 0: w0_ai = d/dkappa_ai L(U^T f U, g transformed by U on all
 *                                    four indices) at kappa = 0 with t and l held fixed and f, g rotated as plain tensors
 *                                    = 2 (X_ai - X_ia), X_pq = sum_r f_pr D_rq + 1/2 sum_rst <pr||st> Gamma_qrst; defined for any t and l.
 *                                    fock_response = 1: f is h + sum_k <pk||qk>, so rotating the occupied space changes f:
 *                                    w_ai = w0_ai + 2 sum_pq D_pq <pa||qi>.  Any other flag: status 1.
 *   afesp_ccsd_so_zvector_apply    = y = A x, both [o v] as t1, A_ai,bj = delta_ab delta_ij (e_a - e_i) + <ab||ij> + <aj||ib> with the
 *                                    state's levels.
 *   afesp_ccsd_so_zvector_solve    = A z = -w (fock_response = 1) by conjugate gradients from z = 0, preconditioned with e_a - e_i, until
 *                                    the residual 2-norm is below tol.  *iters and *resid are written whenever the iteration ran; z (may be
 *                                    NULL) only on success.  Spin-forbidden elements of z stay exact zeros.  On the interleaved
 *                                    (RHF-fed) state the two spin-exchange parts (below) share the one budget maxiter, *iters is
 *                                    their sum, and each part is held to tol / sqrt(2), so that *resid, the norm over both, is
 *                                    below tol: size maxiter for the two parts together.
 *   afesp_ccsd_so_relaxed_density  = D_rel [(o+v)^2 as afesp_ccsd_so_density] = D with 1/2 z_ai added to the ov and vo blocks, symmetric to
 *                                    the bit: for h -> h + eps V with the Hartree-Fock reference re-optimised at every eps,
 *                                    d(E_ref + E_CCSD)/d eps = sum_pq V_pq (g0 + D_rel)_pq at converged t and l.
 *   afesp_ccsd_so_relax_pair_row   = DIAGNOSTIC, not part of the supported interface and free to disappear: the o v^4 part alone, for
 *                                    tools/relax_time.py and the tests: out[i + o a] = sum_b sum_{c<d} P(ab;cd) Q(i,b,c,d) with
 *                                    (P, Q) = (<ab||cd>, Gamma_ibcd) for which = 0 and (Gamma_abcd, <ib||cd>) for which = 1; *ms = device
 *                                    milliseconds per call over `reps` calls after a warm one (out and ms may be NULL).
 * Call order: afesp_ccsd_so_lambda_init ... (Lambda converged) -> afesp_ccsd_so_density2_build -> _orbital_gradient / _zvector_apply /
 * _zvector_solve -> _relaxed_density.  Every call needs the live build of the current t and l, and _relaxed_density a converged solve of
 * them: whatever writes t1 / t2 or l1 / l2 makes both stale (AFESP_LAMBDA_STALE, nothing is read).  None of the calls writes t1 / t2,
 * l1 / l2, the epochs, the Lambda intermediates (G_vv / G_oo are rebuilt for the current l as afesp_ccsd_so_density does), Gamma, a (T)
 * plan or an EOM state; the vectors are released with the Lambda state.
 * Statuses: 1 no spin-orbital state, a NULL or bad argument or a recording context; AFESP_LAMBDA_STALE as above; AFESP_LAMBDA_CAPACITY
 * capacity too small (nothing is launched) or no device memory; AFESP_RELAX_NOT_HF _zvector_solve / _relaxed_density on a state made
 * by afesp_ccsd_uso_init_fock, whose reference is not stationary in the spin-orbital rotations (_orbital_gradient and _zvector_apply
 * take every state Lambda takes); AFESP_RELAX_NOT_CONVERGED tol not reached within maxiter, or a breakdown p A p = 0 (a singular orbital
 * Hessian: an instability threshold of the reference; a nearly singular one stagnates and ends at maxiter) -- the solve is then not
 * usable.  Negative curvature alone (an unstable but stationary reference, A indefinite) does not stop the iteration: the equations
 * still have their solution.  On the interleaved (RHF-fed) state, whose operator commutes with the exchange of the two spins, the part of
 * the right-hand side that is symmetric under the exchange and the antisymmetric one are solved one after the other, each kept in its
 * part to the bit, so that the rounding noise of a spin-pure right-hand side never reaches a triplet instability of the reference. */
#define AFESP_RELAX_NOT_HF 24
#define AFESP_RELAX_NOT_CONVERGED 25
int afesp_ccsd_so_orbital_gradient(afesp_ctx* ctx, int fock_response, double* w /* [o*v], as t1 */, int64_t capacity);
int afesp_ccsd_so_zvector_apply(afesp_ctx* ctx, const double* x, double* y);
int afesp_ccsd_so_zvector_solve(afesp_ctx* ctx, double tol, int maxiter, double* z /* may be NULL */, int* iters, double* resid);
int afesp_ccsd_so_relaxed_density(afesp_ctx* ctx, double* d /* (o+v)^2 as afesp_ccsd_so_density */, int64_t capacity);
int afesp_ccsd_so_relax_pair_row(afesp_ctx* ctx, int which, double* out, int reps, double* ms);

/* Lambda-CCSD(T) (Kucharski and Bartlett 1998, Taube and Bartlett 2008; a-CCSD(T) of Crawford and Stanton 1998): the
 * triples correction with the left factor taken from the left-hand state.  With pp_x, hh_x the particle / hole products of x2 with
 * <fp||bc> / <ma||qr>, wc_x the connected and wd_x the disconnected numerator of afesp_ccsd_so_t built from x = t or x = l, P(y) = y(abc)
 * - y(bac) - y(cba) and D = e_i + e_j + e_k - e_a - e_b - e_c,
 *   afesp_ccsd_so_lambda_t = sum over the triples i<j<k numbered [t_begin, t_end) of afesp_ccsd_so_t_ntriples(nocc), and over a, b, c, of
 *                            P(wc_l + wd_l) P(wc_t) / D / 6
 * at the current t and l (converged or not; with l = t it is afesp_ccsd_so_t term for term).  The enumeration is afesp_ccsd_so_t's, so
 * shards add up; on a state with a full Fock matrix wd_l carries f_ia l_jkbc.  It writes none of t1 / t2, l1 / l2, the epochs, the Lambda
 * intermediates, the EOM states or the DIIS rings: afesp_ccsd_so_t, the Lambda residual and the density give the same bits before and
 * after.  Device memory: a second operand pair and a second block pool beside those of afesp_ccsd_so_t (AFESP_T_POOL_GIB sizes one pool).
 * Statuses: 1 no spin-orbital state, a recording context, a Fock state whose oo / vv blocks are not diagonal (as afesp_ccsd_so_t), or a
 * second pool that does not fit; AFESP_LAMBDA_STALE no Lambda state or a stale one.  An empty range gives 0. */
int afesp_ccsd_so_lambda_t(afesp_ctx* ctx, int64_t t_begin, int64_t t_end, double* e_lt);

/* Non-iterative triples correction to EOM-EE-CCSD excitation energies (afesp_version 6).  For an excitation energy w, a left
 * vector (l1, l2) and a right vector (r1, r2), laid out as t1 / t2, with |mu3> the triply excited determinants and H the bare Hamiltonian,
 *   m(mu3) = <mu3| [H, R2] + [[H, R1], T2] |0>,   l(mu3) = <0| (L1 + L2) H |mu3>,   delta = sum_mu3 l m / (w - (e_a + e_b + e_c - e_i - e_j - e_k)).
 * In the notation of afesp_ccsd_so_lambda_t:  l = wc_l + wd_l,  m = wc_r2[g] + wc_t2[gR]  with gR the one-index transform of g by r1, and
 *   delta[s] = sum over the triples i<j<k numbered [t_begin, t_end), and over a, b, c, of  P(l) P(m) / (D + w[s]) / 6.
 * With w = 0, l = lambda, r = (0, t2) it is afesp_ccsd_so_lambda_t term for term; it is bilinear in (l, r).  The caller passes biorthonormal
 * vectors (<l, r> = 1) and watches small |D + w| itself.  nstates vectors follow one another in l1 / l2 / r1 / r2 (host).  The enumeration
 * is afesp_ccsd_so_t's, so shards add up.  Uses g, f, the levels and t2 only: no Lambda state is needed, and nothing of t, lambda, the
 * epochs, the Lambda, EOM or response states or the operand copies of (T) / Lambda-(T) is written.  Device memory: two block pools as
 * afesp_ccsd_so_lambda_t, a left operand pair and a right one of twice its size.  Statuses: 1 no spin-orbital state, a NULL argument,
 * nstates < 1, a recording context, a Fock state whose oo / vv blocks are not diagonal, or a second pool that does not fit.  An empty
 * range, o < 3 or v < 3 give zeros. */
int afesp_ccsd_so_eom_t(afesp_ctx* ctx, int nstates, const double* omega, const double* l1, const double* l2, const double* r1,
                        const double* r2, int64_t t_begin, int64_t t_end, double* delta /* [nstates] */);

/* EOM-EE-CCSD excitation energies of the spin-orbital state.  The right-hand EOM matrix in the singles and doubles space
 * is the Jacobian A = dR/dt of the residuals above over the unique amplitudes; sigma(r) = A r for r = [r1 [o*v]; r2 [o*o*v*v]] laid out as
 * t1 / t2, r2 antisymmetric in i,j and in a,b.  On that storage <x, y> = sum x1 y1 + 1/4 sum x2 y2.  The excitation energies are the lowest
 * eigenvalues of A at the converged t.  The H-bar elements are those of the live Lambda state (borrowed): afesp_ccsd_so_lambda_init must
 * have been called for the current t1 / t2 -- Lambda itself need not be converged -- and status 21 (AFESP_LAMBDA_STALE) is returned
 * without one or with a stale one.  None of these calls writes t1 / t2, lambda or the epoch.
 *   afesp_ccsd_so_eom_sigma     = s = A r for nvec vectors stored one after the other (host in / out); needs no afesp_ccsd_so_eom_init.
 *   afesp_ccsd_so_eom_init      = a block Davidson state for the nroots lowest roots with at most max_space basis vectors
 *                                 (1 <= nroots <= unique dimension, 2 nroots <= max_space <= 4096 -- the projected problem is solved
 *                                 densely on the host --; status 1 otherwise, or if it does not fit);
 *                                 released by afesp_ccsd_so_lambda_init, by every init of the state and with the context.
 *   afesp_ccsd_so_eom_guess     = unit vectors on the nroots smallest -D (the diagonal guess of A) over the unique amplitudes, ties by flat
 *                                 index; afesp_ccsd_so_eom_set_guess = the caller's vector k (0-based) instead.  _eom_guess starts over, and
 *                                 so does the first _eom_set_guess after an _eom_init, an _eom_guess or an _eom_iterate; further
 *                                 _eom_set_guess calls join that block, and a k left out is a zero vector, which is dropped.
 *   afesp_ccsd_so_eom_iterate   = one Davidson step: the pending vectors are orthonormalised against the basis (dropped below 1e-10),
 *                                 their sigma built, the projected matrix extended and solved on the host, then x_k, rho_k = A x_k -
 *                                 omega_k x_k and the corrections rho_k / (omega_k + D) of the roots with |rho_k| >= tol are formed.  When
 *                                 basis and pending vectors exceed max_space the basis is first collapsed onto the nroots Ritz vectors.
 *                                 omega, resnorm, flags: nroots entries each (NULL: not wanted); flags[k] bit 0: |rho_k| < tol, bit 1: the
 *                                 projected root had an imaginary part (the real part of its vector is used).  *nsigma = sigma builds
 *                                 since the guess, *converged = every root has |rho_k| < tol.
 *   afesp_ccsd_so_eom_get_vector = Ritz vector k of the last step, <x, x> = 1.
 *   afesp_eig_general           = the host eigen-solver of the projected matrix (no context, no GPU): eigenvalues wr + i wi of the real
 *                                 n x n column-major a, ordered by real part (ties: a complex pair stays adjacent, wi > 0 first), and
 *                                 right eigenvectors vr [n*n]: unit columns; a pair's two columns hold real and imaginary part.
 *                                 Returns 0, 1 (bad argument) or 2 (no convergence). */
#define AFESP_EOM_CONVERGED 1
#define AFESP_EOM_COMPLEX 2
int afesp_ccsd_so_eom_init(afesp_ctx* ctx, int nroots, int max_space);
int afesp_ccsd_so_eom_sigma(afesp_ctx* ctx, int nvec, const double* r1, const double* r2, double* s1, double* s2);
int afesp_ccsd_so_eom_guess(afesp_ctx* ctx);
int afesp_ccsd_so_eom_set_guess(afesp_ctx* ctx, int k, const double* r1, const double* r2);
int afesp_ccsd_so_eom_iterate(afesp_ctx* ctx, double tol, double* omega, double* resnorm, int* flags, int* nsigma, int* converged);
int afesp_ccsd_so_eom_get_vector(afesp_ctx* ctx, int k, double* r1, double* r2);
int afesp_eig_general(int n, const double* a, int lda, double* wr, double* wi, double* vr);

/* EOM-EE-CCSD left eigenvectors, and excited-state and transition densities.  EOM-CC is not Hermitian: a root's left
 * eigenvector l A = omega l differs from its right one.  Vectors are host arrays laid out as t1 / t2, as above, with the same metric;
 * every call needs the live Lambda state (status 21 without one or with a stale one, 20 where Lambda is refused) and writes nothing of
 * t1 / t2, lambda, the Lambda state or the right-hand EOM state.
 *   afesp_ccsd_so_eom_lsigma       = s = A^T l for nvec vectors stored one after the other; needs no afesp_ccsd_so_eom_left_init.
 *   afesp_ccsd_so_eom_left_init    = a second block Davidson state, for A^T, beside the right-hand one and with its rules (arguments,
 *                                    release); _left_guess (the same unit vectors: -D is the diagonal of A^T too), _left_set_guess (the
 *                                    converged right vectors are the natural guess), _left_iterate and _left_get_vector are the
 *                                    right-hand calls on that state, with one difference: started by _left_set_guess, the iteration
 *                                    follows the Ritz values of its first step (the right-hand roots, when the guesses are converged
 *                                    right vectors) and returns the Ritz pairs nearest to them, not the lowest roots.
 *   afesp_ccsd_so_eom_ref_coupling = c[k] = sum H_ia r_ia + 1/4 sum <ij||ab> r_ijab of nvec right vectors: the coupling of R to the
 *                                    reference, r0 = c / omega.
 *   afesp_ccsd_so_eom_density      = d [(nocc+nvirt)^2, column-major, symmetric, in the state's spin-orbital order]: with
 *                                      F(f) = <0| (l0 + L) H-bar (r0 + R) |0>
 *                                           = l0 r0 E + l0 dE.r + r0 <l, R(t)> + <l, A r> + E <l, r> + sum l_ijab r_ia R1_jb,
 *                                    d_pq = 1/2 (dF/df_pq + dF/df_qp), bilinear in (l0, l) and (r0, r).  l1 / l2 are both NULL (a zero
 *                                    vector, not read) or both given, and so are r1 / r2 (status 1 otherwise); status 22 if capacity <
 *                                    (nocc+nvirt)^2.  (1, lambda; 1, 0) is afesp_ccsd_so_density; (0, L_k; r0_k, R_k) with <L_k, R_k> = 1
 *                                    the correlation part of excited state k's density; (1, lambda; r0_k, R_k) and (0, L_k; 1, 0) the
 *                                    transition densities gamma^0k and gamma^k0. */
int afesp_ccsd_so_eom_lsigma(afesp_ctx* ctx, int nvec, const double* l1, const double* l2, double* s1, double* s2);
int afesp_ccsd_so_eom_left_init(afesp_ctx* ctx, int nroots, int max_space);
int afesp_ccsd_so_eom_left_guess(afesp_ctx* ctx);
int afesp_ccsd_so_eom_left_set_guess(afesp_ctx* ctx, int k, const double* l1, const double* l2);
int afesp_ccsd_so_eom_left_iterate(afesp_ctx* ctx, double tol, double* omega, double* resnorm, int* flags, int* nsigma, int* converged);
int afesp_ccsd_so_eom_left_get_vector(afesp_ctx* ctx, int k, double* l1, double* l2);
int afesp_ccsd_so_eom_ref_coupling(afesp_ctx* ctx, int nvec, const double* r1, const double* r2, double* c);
int afesp_ccsd_so_eom_density(afesp_ctx* ctx, double l0, const double* l1, const double* l2, double r0, const double* r1, const double* r2,
                              double* d, int64_t capacity);

/* EOM-CCSD linear response: static and dynamic polarisabilities (afesp_version 4).  X is a real symmetric one-body
 * operator over the nocc + nvirt spin orbitals in the state's order, (nocc+nvirt)^2 column-major; X_N its normal-ordered part and
 * X-bar = exp(-T) X_N exp(T).  Vectors are laid out as t1 / t2 with the metric <x, y> = sum x1 y1 + 1/4 sum x2 y2, as above.
 *   xi^X_mu            = <mu| X-bar |0> = residual(f + X) - residual(f) at fixed t (the residual is linear in f):
 *                          X~_kj = X_kj + sum_c X_kc t_jc,   X~_bc = X_bc - sum_k t_kb X_kc
 *                          xi_ia = X_ai + sum_b X_ab t_ib - sum_j t_ja X_ji + sum_jb X_jb (t_ijab - t_ib t_ja)
 *                          xi_ijab = P(ab) sum_c X~_bc t_ijac - P(ij) sum_k X~_kj t_ikab
 *   R^X(omega)         : (A - omega) R^X(omega) = -xi^X with A the matrix of afesp_ccsd_so_eom_sigma
 *   <<X;Y>>_omega      = Phi[X, R^Y(omega)] + Phi[Y, R^X(-omega)]
 *   Phi[X, R]          = <0| (1 + Lambda) (X-bar - <X-bar>) R |0> = Tr(X gamma(1, lambda; 0, R)) - Tr(X D) <lambda, R>
 *                        with gamma afesp_ccsd_so_eom_density (it holds the disconnected E <l, r> piece) and D afesp_ccsd_so_density
 *   alpha_XY(omega)    = -<<X;Y>>_omega
 * This is the EOM-CC response function (Stanton and Bartlett 1993), not the LR-CC one: the term quadratic in the perturbed amplitudes is
 * absent by definition, <<X;Y>>_omega = <<Y;X>>_-omega holds but alpha_XY(omega) != alpha_YX(omega) in general off omega = 0; for two
 * electrons it is exact.  Real frequencies here; complex ones: the _complex entry points below.
 *   afesp_ccsd_so_response_xi         = xi1 [nop * o*v], xi2 [nop * o*o*v*v] of nop operators x [nop * (o+v)^2] at the current t1 / t2, one
 *                                       after the other (host in / out; needs neither a Lambda nor a response state).  An operator's
 *                                       vector has the same bits whatever else is in the batch; xi2 is antisymmetric to the bit.
 *   afesp_ccsd_so_response_init       = the response state: the operators, the nfreq_signed signed frequencies omega to solve for each
 *                                       (a polarisability at omega needs +omega and -omega in the list; 0 once), and a basis of at most
 *                                       max_space vectors SHARED by all nop * nfreq_signed systems (at most 64 systems,
 *                                       2 nop nfreq_signed <= max_space <= 4096; status 1 otherwise, or if it does not fit).  Owned by
 *                                       the Lambda state beside the EOM states and released with them; it has a basis of its own and
 *                                       writes nothing of t1 / t2, lambda, the epochs, the H-bar elements, a (T) plan or an EOM Davidson state
 *                                       (_function rebuilds G_vv / G_oo of the current lambda, as afesp_ccsd_so_density does).
 *   afesp_ccsd_so_response_iterate    = one step: the pending vectors (at first the preconditioned right-hand sides xi / (omega + D))
 *                                       are orthonormalised against the basis, ONE sigma build each serves every system, the projected
 *                                       matrix G and right-hand sides are extended, (G - omega_j) y_j = -B^T xi_j is solved on the host
 *                                       by LU with partial pivoting, then x_j = B y_j, rho_j = xi_j + (A - omega_j) x_j and the
 *                                       corrections rho_j / (omega_j + D) / |rho_j| of the systems with |rho_j| >= tol; a full space collapses onto
 *                                       the current x_j.  resnorm: nop * nfreq_signed entries, system iop + nop * ifreq (NULL: not
 *                                       wanted); *nsigma = sigma builds since _init; *converged = every system has |rho_j| < tol.
 *   afesp_ccsd_so_response_get_vector = R^X_iop(omega[ifreq]) of the last step.
 *   afesp_ccsd_so_response_function   = out[(f * nop + a) * nop + b] = <<X_a;X_b>>_omega[f] for nfreq frequencies, from the resident
 *                                       solutions at +omega[f] and -omega[f].
 *   afesp_lu_solve                    = TEST ENTRY, not part of the supported interface and free to disappear: the host LU solve of the
 *                                       projected systems (csrc/small_eig.h; no context, no GPU) for the CPU tests: a x = b in place,
 *                                       a [n*n] and b [n*nrhs] column-major; 0, 1 (bad argument) or 2 (a pivot not above `floor`).
 * Statuses: 1 no spin-orbital state, a NULL or bad argument, a non-symmetric operator (beyond 1e-12 of its largest element), nop < 1, a
 * frequency asked of _function that is not in the state's list at both signs, or a recording context; AFESP_LAMBDA_STALE (21) without a
 * live Lambda state or response state, or after anything wrote t1 / t2 or l1 / l2 (20 is afesp_ccsd_so_lambda_init's refusal);
 * AFESP_RESPONSE_POLE from _iterate: a pivot of a projected system is below 1e-10 max(|G|, |omega|) -- the frequency is at a root of the
 * projected EOM matrix, an excitation energy, where no response is defined; by then the step has extended the basis and counted its sigma builds and no pending
 * vector is left, so a repeated _iterate only solves the same projected systems and returns 26 again (start over with _init);
 * AFESP_RESPONSE_NOT_CONVERGED from _function: a solution it needs has not reached the tol of the last _iterate (or no step was made). */
#define AFESP_RESPONSE_POLE 26
#define AFESP_RESPONSE_NOT_CONVERGED 27
int afesp_ccsd_so_response_xi(afesp_ctx* ctx, int nop, const double* x, double* xi1, double* xi2);
int afesp_ccsd_so_response_init(afesp_ctx* ctx, int nop, const double* x, int nfreq_signed, const double* omega, int max_space);
int afesp_ccsd_so_response_iterate(afesp_ctx* ctx, double tol, double* resnorm, int* nsigma, int* converged);
int afesp_ccsd_so_response_get_vector(afesp_ctx* ctx, int iop, int ifreq, double* r1, double* r2);
int afesp_ccsd_so_response_function(afesp_ctx* ctx, int nfreq, const double* omega, double* out /* [nfreq*nop*nop] */);
int afesp_lu_solve(int n, double* a, int lda, int nrhs, double* b, int ldb, double floor);

/* The same response function at complex frequencies z = omega + i gamma (afesp_version 5): damped spectra, alpha(i omega)
 * and C6.  A and xi^X are real, R = P + i Q:
 *   (A - z) R^X(z) = -xi^X      <=>      (A - omega) P + gamma Q = -xi,   (A - omega) Q - gamma P = 0
 *   <<X;Y>>_z          = Phi[X, R^Y(z)] + Phi[Y, R^X(-z)],   Phi[X, P + i Q] = Phi[X, P] + i Phi[X, Q],   alpha_XY(z) = -<<X;Y>>_z
 *   R(conj z)          = conj R(z)
 * the analytic continuation of the function above: with gamma > 0 nothing is singular at an excitation energy, Im alpha(omega + i gamma)
 * is the absorption profile, alpha(i u) the integrand of the Casimir-Polder integral.  The basis of the solver stays real and every sigma
 * build serves every system; a solution takes two vectors.
 *   afesp_ccsd_so_response_init_complex       = as _init with nfreq_signed complex frequencies z [2 * nfreq_signed: re, im]; at most 64
 *                                               systems, 4 nop nfreq_signed <= max_space <= 4096.  Releases an earlier response state of
 *                                               either kind.  afesp_ccsd_so_response_iterate steps a state of either kind.
 *   afesp_ccsd_so_response_get_vector_complex = Re and Im of R^X_iop(z[ifreq]) of the last step.
 *   afesp_ccsd_so_response_function_complex   = out[2 * ((f * nop + a) * nop + b) + {0, 1}] = Re, Im of <<X_a;X_b>>_z[f].  R^X(-z) is the
 *                                               resident solution at -z where the list has it, otherwise the conjugate of the one at
 *                                               -conj(z) -- for an imaginary z that is z itself: one solve per imaginary frequency.
 *   afesp_lu_solve_complex                    = TEST ENTRY, as afesp_lu_solve: the host LU of the projected complex systems; a and b hold
 *                                               (re, im) pairs, element (i, j) at a[2 * (i + lda * j)]; pivoting on |pivot|; 0, 1 or 2.
 * Statuses as above; in addition 1 when a real entry point (_get_vector, _function) is called on a state made by _init_complex or a
 * _complex one on a state made by _init -- no silent reinterpretation --, and 1 from _function_complex for a z whose -z and -conj(z) are
 * both missing from the list.  With gamma != 0 a pole (26) cannot occur; it remains for gamma = 0. */
int afesp_ccsd_so_response_init_complex(afesp_ctx* ctx, int nop, const double* x, int nfreq_signed, const double* z, int max_space);
int afesp_ccsd_so_response_get_vector_complex(afesp_ctx* ctx, int iop, int ifreq, double* r1_re, double* r2_re, double* r1_im, double* r2_im);
int afesp_ccsd_so_response_function_complex(afesp_ctx* ctx, int nfreq, const double* z, double* out /* [2*nfreq*nop*nop] */);
int afesp_lu_solve_complex(int n, double* a, int lda, int nrhs, double* b, int ldb, double floor);

/* EOM-IP-CCSD and EOM-EA-CCSD on the same state: ionisation potentials omega = E(N-1) - E(N) in the 1h + 2h1p sector,
 * r1(nocc), r2(nocc,nocc,nvirt) antisymmetric in its first two indices, and electron affinities omega = E(N+1) - E(N) in the 1p + 2p1h
 * sector, r1(nvirt), r2(nocc,nvirt,nvirt) antisymmetric in its last two.  <x, y> = sum x1 y1 + 1/2 sum x2 y2; the unique amplitudes are
 * i, then (i < j, a) / a, then (i, a < b).  `sector` is AFESP_EOM_IP or AFESP_EOM_EA (status 1 otherwise).  The calls are those of the
 * EE sector above with the same rules and statuses, one Davidson state per sector beside the EE one: status 21 without a live Lambda
 * state or with a stale one, and from _iterate, _guess, _set_guess and _get_vector without an _init of that sector; _sigma needs the
 * Lambda state only.  None writes t1 / t2, lambda, the epoch or the EE state.  One rule differs: the vectors of _guess are the unit vectors
 * on the nroots smallest diagonal elements, each with a fixed 1e-3 admixture of every unique amplitude, because sigma couples neither
 * different Ms nor different irreducible representations and a wanted root may lie in a block that holds none of those elements.  nroots is at most the number of unique amplitudes (with
 * one occupied spin orbital the IP sector has no doubles: nocc). */
#define AFESP_EOM_IP 1
#define AFESP_EOM_EA 2
int afesp_ccsd_so_eom_ipea_init(afesp_ctx* ctx, int sector, int nroots, int max_space);
int afesp_ccsd_so_eom_ipea_sigma(afesp_ctx* ctx, int sector, int nvec, const double* r1, const double* r2, double* s1, double* s2);
int afesp_ccsd_so_eom_ipea_guess(afesp_ctx* ctx, int sector);
int afesp_ccsd_so_eom_ipea_set_guess(afesp_ctx* ctx, int sector, int k, const double* r1, const double* r2);
int afesp_ccsd_so_eom_ipea_iterate(afesp_ctx* ctx, int sector, double tol, double* omega, double* resnorm, int* flags, int* nsigma,
                                   int* converged);
int afesp_ccsd_so_eom_ipea_get_vector(afesp_ctx* ctx, int sector, int k, double* r1, double* r2);

/* The left-hand side of both sectors, Dyson orbitals and pole strengths (afesp_version 7).  sigma_L = A^T l, the transpose
 * in the sector's metric: <l, sigma(r)> = <sigma_L(l), r>; the vectors are laid out as the right-hand ones.
 *   afesp_ccsd_so_eom_ipea_lsigma   = s = A^T l for nvec vectors stored one after the other; needs the Lambda state only.
 *   afesp_ccsd_so_eom_ipea_left_*   = one more block Davidson state per sector, for A^T, beside the right-hand one and with its rules
 *                                     (arguments, statuses, the guesses of _left_guess with their admixture).  From the caller's guesses
 *                                     (_left_set_guess with the converged right vectors) the state follows the states of the guesses, as
 *                                     afesp_ccsd_so_eom_left_* does: root k of the left state is root k of the right one.
 *   afesp_ccsd_so_eom_ipea_dyson    = the Dyson vectors of nvec left and / or right vectors over all nocc + nvirt spin orbitals in the
 *                                     state's order, (nocc + nvirt) x nvec column-major:
 *                                       dl[p] = <0| L e^-T a_p e^T |0>,  dr[p] = <0| (1 + Lambda) e^-T a_p^+ e^T R |0>     (IP; a_p^+ / a_p: EA)
 *                                     with the phases of the ghost-orbital construction that defines the sectors.  For a biorthonormal
 *                                     pair <L_k, R_k> = 1 the pole strength is sum_p dl[p] dr[p].  l1 / l2 both NULL (dl is not written)
 *                                     or both given, and r1 / r2 / dr likewise; a half-given pair is status 1.  Needs the live Lambda
 *                                     state (status 21 otherwise: it reads lambda) and no Davidson state.
 * None writes t1 / t2, lambda, the epoch or the state of another kind. */
int afesp_ccsd_so_eom_ipea_lsigma(afesp_ctx* ctx, int sector, int nvec, const double* l1, const double* l2, double* s1, double* s2);
int afesp_ccsd_so_eom_ipea_left_init(afesp_ctx* ctx, int sector, int nroots, int max_space);
int afesp_ccsd_so_eom_ipea_left_guess(afesp_ctx* ctx, int sector);
int afesp_ccsd_so_eom_ipea_left_set_guess(afesp_ctx* ctx, int sector, int k, const double* l1, const double* l2);
int afesp_ccsd_so_eom_ipea_left_iterate(afesp_ctx* ctx, int sector, double tol, double* omega, double* resnorm, int* flags, int* nsigma,
                                        int* converged);
int afesp_ccsd_so_eom_ipea_left_get_vector(afesp_ctx* ctx, int sector, int k, double* l1, double* l2);
int afesp_ccsd_so_eom_ipea_dyson(afesp_ctx* ctx, int sector, int nvec, const double* l1, const double* l2, const double* r1, const double* r2,
                                 double* dl, double* dr);

/* Non-iterative triples correction to EOM-IP-CCSD and EOM-EA-CCSD roots (afesp_version 8): afesp_ccsd_so_eom_t's correction
 * in the ghost-orbital embedding that defines the sectors.  For a root w of sector 1 (IP) or 2 (EA), a left vector (l1, l2) and a right
 * vector (r1, r2) in the sector's layout (IP x1[nocc], x2[nocc,nocc,nvirt]; EA x1[nvirt], x2[nocc,nvirt,nvirt]), H the bare Hamiltonian,
 *   m(mu) = <mu| [H, R2] + [[H, R1], T2] |0>,   l(mu) = <0| (L1 + L2) H |mu>,   delta = sum_mu l(mu) m(mu) / (w - D_eps(mu))
 * over the 3h2p determinants (IP: i<j<k, a<b, D_eps = e_a + e_b - e_i - e_j - e_k) or the 3p2h determinants (EA: i<j, a<b<c,
 * D_eps = e_a + e_b + e_c - e_i - e_j).  This is the bare-H, lowest-order member of the EOM-IP/EA-CCSD* family.
 * Items: for IP the triples i<j<k in afesp_ccsd_so_t's numbering (afesp_ccsd_so_t_ntriples of them); for EA the pairs i<j numbered
 * j (j - 1) / 2 + i, the library's triangular pair numbering (nocc (nocc - 1) / 2 of them).  afesp_ccsd_so_eom_ipea_t_nitems returns
 * the count (0 for a bad sector).  delta[s] is the sum over the items [begin, end), clipped to the list, so shards add up.
 * The caller passes biorthonormal vectors (<l, r> = 1 in the sector's metric) and watches small |w - D_eps| itself.  nstates vectors follow
 * one another in l1 / l2 / r1 / r2 (host).  Uses g, f, the levels and t2 only: no Lambda state and no Davidson state is needed, and nothing of
 * t, lambda, the epochs, the Lambda, EOM or response states or the operand copies of (T) / Lambda-(T) / EOM-(T) is written.  Device memory:
 * the images of a chunk of items, bounded by AFESP_T_POOL_GIB (at least one item: 6 nvirt^2 doubles for IP, 6 nvirt^3 for EA), beside
 * copies of <vo||vv> and t2.  Statuses: 1 no spin-orbital state, a bad sector, a NULL argument, nstates < 1, a recording context, a Fock
 * state whose oo / vv blocks are not diagonal, or a chunk that does not fit the free device memory.  An empty range gives zeros, and so
 * do IP with nocc < 3 or nvirt < 2 and EA with nocc < 2 or nvirt < 3. */
int afesp_ccsd_so_eom_ipea_t(afesp_ctx* ctx, int sector, int nstates, const double* omega, const double* l1, const double* l2,
                             const double* r1, const double* r2, int64_t begin, int64_t end, double* delta /* [nstates] */);
int64_t afesp_ccsd_so_eom_ipea_t_nitems(int sector, int nocc);

/* Open-shell (UHF-based) path.  The reference accepts calc_type = "UHF" but runs its spin-orbital CCSD/(T) on doubled RHF
 * orbitals only (src/main.F90:48-52); these calls feed the same spin-orbital solver with canonical UHF orbitals.
 *   afesp_build_fock_uhf = fock_s = core_hamil + J[dens_a + dens_b] - K[dens_s] for s = a, b on the resident packed AO integrals
 *                          (afesp_set_eri / afesp_read_eri_text), dens_s = C_s,occ^T C_s,occ; n x n column-major host arrays.
 *                          With dens_a = dens_b it returns afesp_build_fock's matrix bit for bit.
 *   afesp_ao2mo_ump2     = the alpha-alpha and beta-beta MO integrals (8-fold packed, as afesp_ao2mo_mp2 writes them), the
 *                          alpha-beta block as a full npair x npair matrix eri_ab[tri(p,q) npair + tri(r,s)] = (pq|rs), pq alpha,
 *                          rs beta (npair = n(n+1)/2), and E(UMP2).  coeff_s: MO x AO column-major, as canon_coeff; levels_s: n
 *                          entries.  eri_packed NULL: the resident AO integrals.  Each output array may be NULL; the three blocks
 *                          stay on the device (apart from the RHF path's MO integrals) for afesp_ccsd_uso_init.  Bases of up to
 *                          64 functions take the LDS-resident pair transform, larger ones the gather-GEMM form; a basis whose
 *                          temporaries need the slab-blocked form is refused (status 1).
 *   afesp_ccsd_uso_init  = the spin-orbital state from those blocks.  Spin-orbital order: occupied = alpha occupied (nalpha),
 *                          then beta occupied (nbeta); virtual = alpha virtual (n - nalpha), then beta virtual (n - nbeta):
 *                          nocc = nalpha + nbeta, nvirt = 2n - nocc.  F_mi takes Stanton's published order.  A state that would
 *                          not fit the device is refused (status 1).  Afterwards afesp_ccsd_so_energy / _iterate / _diis /
 *                          _get_amplitudes / _set_amplitudes / _get_tensor / _t (with afesp_ccsd_so_t_ntriples(nocc)) drive it. */
int afesp_build_fock_uhf(afesp_ctx* ctx, int64_t nbasis, const double* dens_a, const double* dens_b, const double* core_hamil,
                         double* fock_a, double* fock_b);
int afesp_ao2mo_ump2(afesp_ctx* ctx, int64_t nbasis, int64_t nalpha, int64_t nbeta, const double* coeff_a, const double* coeff_b,
                     const double* levels_a, const double* levels_b, const double* eri_packed, double* eri_aa, double* eri_ab,
                     double* eri_bb, double* e_ump2);
int afesp_ccsd_uso_init(afesp_ctx* ctx, int64_t nbasis, int64_t nalpha, int64_t nbeta, const double* levels_a, const double* levels_b,
                        int diis_n_errmat);
/* afesp_mo_window for the three blocks afesp_ao2mo_ump2 left resident: the same number of lowest orbitals is frozen for both spins and
 * the same number of highest ones dropped; afterwards afesp_ccsd_uso_init(n_act, nalpha - nfc, nbeta - nfc, levels_a + nfc,
 * levels_b + nfc, ...).  The active extents must be ones afesp_ccsd_uso_init accepts (a spin may keep no occupied orbital, the two
 * together keep at least one occupied and one virtual spin orbital); otherwise, for a negative count, or with no blocks resident for
 * nbasis: status 1, blocks untouched.  eri_aa / eri_bb (neri(n_act)) and eri_ab (npair_act^2) may be NULL.  *e_ump2 = frozen-core UMP2. */
int afesp_umo_window(afesp_ctx* ctx, int64_t nbasis, int64_t nalpha, int64_t nbeta, int64_t n_frozen_core, int64_t n_frozen_virt,
                     const double* levels_a, const double* levels_b, double* eri_aa, double* eri_ab, double* eri_bb, double* e_ump2);

/* Frozen natural orbitals (the reference has none): the virtual-virtual block of the MP2 one-particle density, from the
 * MO integrals a transform left resident and BEFORE any window.  i, j run over the active occupied orbitals (the n_frozen_core lowest
 * excluded), a, b, c over all virtuals.
 *   closed shell, t(i,j,a,b) = (ia|jb) / (e_i + e_j - e_a - e_b):   D(a,b) = sum_ijc [2 t(i,j,a,c) - t(i,j,c,a)] t(i,j,b,c)
 *   open shell,   t_ss(i,j,a,b) = [(ia|jb) - (ib|ja)] / D,  t_ab(i,J,a,B) = (ia|JB) / D:
 *                 D_a(a,b) = 1/2 sum_{ijc in alpha} t_aa(ijac) t_aa(ijbc) + sum_{i in alpha; J, C in beta} t_ab(iJaC) t_ab(iJbC);  D_b: the mirror image
 * (trace D = the number of electron pairs promoted per spin; nalpha = nbeta with equal orbitals gives D_a = D_b = D).
 *   in : the levels of the whole basis;   out: d_vv[v*v] (v = nbasis - nocc), d_a[va*va], d_b[vb*vb]: column-major, symmetric to the bit;
 *        *e_mp2 / *e_ump2 (may be NULL) = the frozen-core MP2 energy of the full virtual space, what afesp_mo_window / afesp_umo_window
 *        report for (n_frozen_core, 0) -- the "full space" term of the Delta-MP2 correction of a truncated virtual space.
 * HIP builder kernels gather the MP1 amplitudes out of the packed arrays into two scratch operands (o^2 v^2 doubles each) with the
 * contraction index (i,j,c) fastest; the products D = T~^T T (M = N = v, K = o^2 v) run through the GEMM layer; the scratch goes back to the
 * context's arena inside the call.  Every resident array is left untouched: the host diagonalises D, rotates the virtual block of the
 * coefficients, calls afesp_ao2mo_mp2 / afesp_ao2mo_ump2 again on the resident AO integrals (eri_packed = NULL) and takes the window.
 * Status 1, nothing touched: a negative count, no active occupied orbital (n_frozen_core >= nocc), NULL levels or output, nothing resident
 * for nbasis (so also after a window), scratch that does not fit the free device memory. */
int afesp_mp2_vv_density(afesp_ctx* ctx, int64_t nbasis, int64_t nocc, int64_t n_frozen_core, const double* canon_levels, double* d_vv,
                         double* e_mp2);
int afesp_ump2_vv_density(afesp_ctx* ctx, int64_t nbasis, int64_t nalpha, int64_t nbeta, int64_t n_frozen_core, const double* levels_a,
                          const double* levels_b, double* d_a, double* d_b, double* e_ump2);

/* The active space as a Hamiltonian on disk (the reference's write_fcidump has no header, no one-electron part and no
 * window).  Two steps: the frozen-core operator BEFORE the window (the window throws the core orbitals away), the file AFTER it.
 *
 * afesp_core_operator / afesp_ucore_operator act on the full MO integrals a transform left resident.  c, d run over the n_frozen_core
 * lowest orbitals, p, q over the active window [n_frozen_core, nbasis - n_frozen_virt); h_mo = C h_ao C^T with C (MO, AO) as canon_coeff:
 *   closed shell:  h_act(p,q) = h_mo(p,q) + sum_c [2 (pq|cc) - (pc|qc)]
 *                  e_core     = 2 sum_c h_mo(c,c) + sum_cd [2 (cc|dd) - (cd|cd)]
 *   open shell:    h_act_a(p,q) = h_mo_a(p,q) + sum_{c in alpha} [(pq|cc) - (pc|qc)]_aa + sum_{C in beta} (pq|CC)_ab;  h_act_b: the mirror image
 *                  e_core = sum_c h_a(c,c) + sum_C h_b(C,C) + 1/2 sum_cd [(cc|dd) - (cd|cd)]_aa + 1/2 sum_CD [...]_bb + sum_cD (cc|DD)_ab
 *   in : canon_coeff / coeff_a / coeff_b [n*n] (MO, AO), core_hamil_ao [n*n];   out: h_act [n_act*n_act] column-major, symmetric to the
 *        bit; *e_core electronic (the caller adds the nuclear repulsion).  n_frozen_core = 0 is legal: the window of h_mo, e_core = 0.
 * h_mo runs through the GEMM layer; one wave per active pair gathers the core's field out of the packed arrays in a fixed order.
 * Every resident array is left untouched.  Status 1, nothing touched: a negative count, no active orbital left, a NULL argument,
 * nothing resident for nbasis (so also after a window).
 *
 * afesp_write_fcidump_active / _uactive write whatever is resident for n_act orbitals -- the window after afesp_mo_window /
 * afesp_umo_window, the full basis without one -- as a standard FCIDUMP.  The integrals with |value| > threshold are compacted on the
 * device in canonical order (threshold = 0: everything except exact zeros), only they cross to the host, which formats them (on up to 16
 * threads; the file is the same bytes run to run).  *nwritten (may be NULL) = the number of lines after the header.  Format:
 *    &FCI NORB=<n>,NELEC=<nelec>,MS2=<ms2>,
 *     ORBSYM=1,1,...,1,
 *     ISYM=1,
 *    &END
 *    <value> <i> <j> <k> <l>
 * the value as %23.15E, four blank-separated 1-based indices, chemists' notation (ij|kl).  First the two-electron lines in the canonical
 * order of the packed array (i >= j, k >= l, ij >= kl), then h(i,j) i j 0 0 for i >= j with |h| > threshold, last e_core_total 0 0 0 0
 * (always written; e_core plus the nuclear repulsion).
 * Open shell: the header gains the line UHF=.TRUE., ; NORB = 2 n_act spin orbitals, NELEC = nalpha_act + nbeta_act, MS2 their difference;
 * indices are spin-orbital numbers, interleaved as on the spin-orbital path above: spatial orbital p (1-based) is 2p - 1 for alpha and 2p
 * for beta.  Blocks in this order: alpha-alpha (8-fold unique), beta-beta (8-fold unique), alpha-beta (every p >= q, r >= s, once, as
 * (p_a q_a | r_b s_b)), h_alpha, h_beta, the core energy.  Spin-forbidden integrals are never written.
 * Status 1: a NULL path or matrix, a negative threshold, nothing resident for n_act. */
int afesp_core_operator(afesp_ctx* ctx, int64_t nbasis, int64_t n_frozen_core, int64_t n_frozen_virt, const double* canon_coeff,
                        const double* core_hamil_ao, double* h_act, double* e_core);
int afesp_ucore_operator(afesp_ctx* ctx, int64_t nbasis, int64_t n_frozen_core, int64_t n_frozen_virt, const double* coeff_a,
                         const double* coeff_b, const double* core_hamil_ao, double* h_act_a, double* h_act_b, double* e_core);
int afesp_write_fcidump_active(afesp_ctx* ctx, const char* path, int64_t n_act, int64_t nelec_act, int64_t ms2, const double* h_act,
                               double e_core_total, double threshold, int64_t* nwritten);
int afesp_write_fcidump_uactive(afesp_ctx* ctx, const char* path, int64_t n_act, int64_t nalpha_act, int64_t nbeta_act, const double* h_act_a,
                                const double* h_act_b, double e_core_total, double threshold, int64_t* nwritten);

/* A standard FCIDUMP as input: the way in for MO integrals that another program -- or afesp_write_fcidump_active --
 * wrote.  No SCF and no transform: the file's orbitals are taken in file order and the FIRST nocc (nalpha / nbeta) of them are occupied.
 *
 * Format: the one documented at afesp_write_fcidump_active above, read liberally.  The namelist may be closed by &END or by / ; keys in any
 * letter case, over any number of lines, in any order; ORBSYM, ISYM and unknown keys are ignored (no point-group handling); a missing MS2
 * is 0; UHF=.TRUE. selects the writer's spin-orbital numbering (spatial orbital p is 2p - 1 for alpha, 2p for beta).  Body lines
 * "value i j k l": fields separated by blanks and/or one comma, reals with E or D exponents (strtod: correctly rounded), blank lines and
 * \r tolerated, lines in any order, the four indices of a two-electron line in any of the 8 equivalent arrangements, the alpha-beta
 * integral as (aa|bb) or (bb|aa).  Integrals not mentioned are zero, a missing core-energy line means e_core = 0.
 * Duplicates: several lines may name one slot (files that list symmetry partners do); they must agree to the bit.  A duplicate that
 * disagrees is an error wherever in the file the two lines are -- never "the last one wins".
 *
 * afesp_fcidump_scan: host only, no context, no device: the header and *nlines = the non-blank lines after it.  Non-zero: NULL or
 *   unreadable path, no &FCI, no terminator, no NORB / NELEC.
 * afesp_read_fcidump (closed shell: NORB = nbasis, NELEC = 2 nocc, MS2 = 0, no UHF flag) and afesp_read_fcidump_uhf (UHF=.TRUE.,
 *   NORB = 2 nbasis, NELEC = nalpha + nbeta, MS2 = nalpha - nbeta) read the file in chunks of AFESP_FCIDUMP_CHUNK_KIB KiB: the host parses
 *   a chunk on up to 16 threads into 32-byte records while the device scatters the previous one -- the host never holds the integrals.
 *   On success the packed array is resident exactly as afesp_ao2mo_mp2 leaves the MO integrals of nbasis functions (the three blocks: as
 *   afesp_ao2mo_ump2 leaves them), so everything that accepts eri_mo_packed = NULL works on it: afesp_ccsd_init, afesp_ccsd_so_init,
 *   afesp_ccsd_uso_init, afesp_mo_window / afesp_umo_window (a (0, 0) window reports the MP2 energy), afesp_mp2_vv_density,
 *   afesp_write_fcidump*.  Resident AO integrals are left alone.
 *   out (each may be NULL; matrices column-major, symmetric to the bit):
 *     h_mo [n*n]      the one-electron matrix of the file
 *     fock [n*n]      closed shell: F(p,q) = h(p,q) + sum_{i < nocc} [2 (pq|ii) - (pi|qi)]
 *                     open shell:   F_a = h_a + sum_{i in alpha occ} [(pq|ii) - (pi|qi)]_aa + sum_{I in beta occ} (pq|II)_ab; F_b the mirror image
 *     levels [n]      the diagonal of fock
 *     *e_core         the value on the 0 0 0 0 line
 *     *e_ref          the energy of the determinant: e_core + sum_i [h(i,i) + F(i,i)]   (open shell: e_core + 1/2 sum_{i in alpha} [h_a + F_a](i,i)
 *                     + 1/2 sum_{I in beta} [h_b + F_b](I,I))
 *     *fock_offdiag   max_{p != q} |F(p,q)| over both spins.  The library reports it and does not judge it: the solvers assume canonical
 *                     orbitals, the caller decides what it accepts (els_amd and Engine.read_fcidump refuse above 1e-6)
 *     eri_*           host copies of the packed arrays;  *nread = lines after the header
 *   Status 1, everything resident untouched, no output written, afesp_last_error with the line number where there is one: a NULL path or
 *   an unreadable file; no &FCI or no terminator; a header that disagrees with the arguments; a malformed line; an index outside
 *   0..NORB; a line that is neither a two-electron, a one-electron nor the core-energy line; a spin-forbidden element in a UHF file; more
 *   than one core-energy line; a duplicate that disagrees; arrays that do not fit the device. */
int afesp_fcidump_scan(const char* path, int64_t* norb, int64_t* nelec, int64_t* ms2, int* uhf, int64_t* nlines);
int afesp_read_fcidump(afesp_ctx* ctx, const char* path, int64_t nbasis, int64_t nocc, double* h_mo, double* fock, double* levels,
                       double* e_core, double* e_ref, double* fock_offdiag, double* eri_mo_packed, int64_t* nread);
int afesp_read_fcidump_uhf(afesp_ctx* ctx, const char* path, int64_t nbasis, int64_t nalpha, int64_t nbeta, double* h_a, double* h_b,
                           double* fock_a, double* fock_b, double* levels_a, double* levels_b, double* e_core, double* e_ref,
                           double* fock_offdiag, double* eri_aa, double* eri_ab, double* eri_bb, int64_t* nread);

/* ---- Restricted open-shell (ROHF) references: non-HF CCSD and CCSD(T) on the dense spin-orbital solver.
 * A restricted open-shell determinant -- one set of orbitals, the first nalpha / nbeta of them occupied, nalpha >= nbeta -- has two spin
 * Fock operators with f_ia != 0 and non-diagonal occupied and virtual blocks.  The route: one packed MO array (a restricted FCIDUMP, or
 * afesp_ao2mo_mp2) -> the two operators (afesp_mo_fock_ro / afesp_read_fcidump_rohf) -> the caller diagonalises the occupied and the
 * virtual block of each spin (semicanonical orbitals; afesp_amd/rohf.py) -> afesp_mo_rotate_uhf -> afesp_ccsd_uso_init_fock ->
 * afesp_ccsd_so_energy / _iterate / _diis -> afesp_ccsd_so_t.  No ROHF SCF: the orbitals come from a file or from the caller.
 *
 * afesp_mo_fock_ro: on the packed MO array resident for nbasis (afesp_ao2mo_mp2, afesp_read_fcidump, afesp_read_fcidump_rohf)
 *     F_a(p,q) = h(p,q) + sum_{i < nalpha} [(pq|ii) - (pi|qi)] + sum_{i < nbeta} (pq|ii)
 *     F_b(p,q) = h(p,q) + sum_{i < nbeta}  [(pq|ii) - (pi|qi)] + sum_{i < nalpha} (pq|ii)
 *     *e_ref_elec = 1/2 sum_{i < nalpha} [h + F_a](i,i) + 1/2 sum_{i < nbeta} [h + F_b](i,i)
 *   h_mo, fock_a, fock_b [n*n] column-major; the outputs are symmetric to the bit (one wave per orbital pair, fixed summation order).
 *   Nothing resident is touched.  Status 1: a negative count, nalpha < nbeta, nalpha > nbasis, a NULL argument, nothing resident for nbasis.
 * afesp_read_fcidump_rohf: afesp_read_fcidump for the file with MS2 = nalpha - nbeta >= 0 and no UHF flag (NORB = nbasis, NELEC = nalpha +
 *   nbeta): the same parse, scatter, duplicate rule, error list and residency (the packed array is left as afesp_read_fcidump leaves it).
 *   fock_a / fock_b as above, *e_ref = *e_core + e_ref_elec, fock_offdiag[3] = max |F| over both spins of the occupied-occupied
 *   off-diagonal, the virtual-virtual off-diagonal and the occupied-virtual elements -- reported, not judged.  Each output may be NULL.
 * afesp_mo_rotate_uhf: the resident packed MO integrals in the orbitals phi'_p = sum_q u_s(p,q) phi_q of spin s (u_s [n*n] column-major,
 *   (new orbital, old orbital), like canon_coeff), as the three blocks (aa|aa), (aa|bb), (bb|bb) left resident exactly as afesp_ao2mo_ump2
 *   leaves them; afesp_umo_window works on them afterwards.  The transform is afesp_ao2mo_ump2's with the packed MO array as its source
 *   (the LDS-resident pair transform up to 64 functions, the gather-GEMM form above; a size that needs the slab-blocked form is
 *   refused as there).  The packed array and resident AO integrals stay untouched and valid.  eri_* (host copies) may be NULL.
 * afesp_ccsd_uso_init_fock: the state of afesp_ccsd_uso_init from the resident three blocks with the full spin Fock matrices fock_a /
 *   fock_b [n*n] of the SAME orbitals: the levels are their diagonals, f_ov and the off-diagonal f_oo / f_vv (afesp_ccsd_so_get_tensor
 *   "f_ov", "f_oo", "f_vv"; the state's spin-orbital order) enter Stanton et al. Eqs. 1-5:
 *     F_ae += (1 - d_ae) f_ae - 1/2 f_me t_ma,  F_mi += (1 - d_mi) f_mi + 1/2 t_ie f_me,  F_me += f_me,  T1 residual += f_ia,
 *     E += sum f_ia t_ia;  start amplitudes t1 = f_ia / D_ia, t2 = <ij||ab> / D_ijab;
 *     *e_mp2 = sum f_ia^2 / D_ia + 1/4 sum <ij||ab>^2 / D_ijab  (semicanonical orbitals: the ROHF-MBPT(2) energy).
 *   Only a state made by this call executes these terms.  afesp_ccsd_so_t on it adds f_ia t_jk^bc to the disconnected triples
 *   (ROHF-CCSD(T), Watts, Gauss, Bartlett 1993) and returns status 1 if an off-diagonal f_oo or f_vv element exceeds 1e-8 in magnitude:
 *   (T) is defined in semicanonical orbitals only. */
int afesp_mo_fock_ro(afesp_ctx* ctx, int64_t nbasis, int64_t nalpha, int64_t nbeta, const double* h_mo, double* fock_a, double* fock_b,
                     double* e_ref_elec);
int afesp_read_fcidump_rohf(afesp_ctx* ctx, const char* path, int64_t nbasis, int64_t nalpha, int64_t nbeta, double* h_mo, double* fock_a,
                            double* fock_b, double* e_core, double* e_ref, double* fock_offdiag, double* eri_mo_packed, int64_t* nread);
int afesp_mo_rotate_uhf(afesp_ctx* ctx, int64_t nbasis, const double* u_a, const double* u_b, double* eri_aa, double* eri_ab, double* eri_bb);
int afesp_ccsd_uso_init_fock(afesp_ctx* ctx, int64_t nbasis, int64_t nalpha, int64_t nbeta, const double* fock_a, const double* fock_b,
                             int diis_n_errmat, double* e_mp2);

/* ---- Multi-GPU: one process per GPU, each with its own context.  The reference has no distributed layer;
 * its (T) loop ends in an OpenMP `reduction(+: ...)` over threads (src/ccsd.f90:2091, entered from src/main.F90:112).  Here
 * every rank evaluates its shard [bounds[r], bounds[r+1]) of the triple list (afesp_ccsd_t_shard_bounds) and that
 * reduction becomes ONE sum over the ranks of the 2...6 partial scalars: afesp_allreduce_sum.
 *   transport AFESP_COMM_RCCL: ncclAllReduce(sum, fp64) on the context's stream (xGMI between the GPUs of a node); librccl is
 *             opened on the first call, a single-rank run never needs it.
 *   transport AFESP_COMM_HOST: ranks of one node add through a file-backed shared segment in a fixed rank order.  For
 *             rehearsing the rank logic where ranks SHARE a GPU (RCCL refuses two ranks on one device); host memory only.
 *   bootstrap_path: a file name in a directory every rank sees, unique to this job (the launcher makes it): rank 0 publishes
 *             the RCCL unique id there / it backs the shared segment; removed once every rank has joined.  With
 *             unique_id != NULL (128 bytes from afesp_comm_unique_id on rank 0, distributed by the caller -- bench.py
 *             broadcasts it through torch.distributed) no file is used.
 * A communicator alone does not change how the CCSD iteration is evaluated: splitting it over the ranks is a separate, opt-in
 * switch (afesp_ccsd_set_split below).  Once that is on, every rank must make the same sequence of afesp_ccsd_* calls. */
#define AFESP_COMM_RCCL 0
#define AFESP_COMM_HOST 1
int afesp_device_count(void);
int afesp_comm_unique_id(char id_out[128]);
int afesp_comm_init(afesp_ctx* ctx, int rank, int world, int transport, const char* bootstrap_path, const char* unique_id);
int afesp_comm_destroy(afesp_ctx* ctx);
/* in-place sum over the ranks of n host doubles (every rank passes the same n) */
int afesp_allreduce_sum(afesp_ctx* ctx, double* inout, int64_t n);
/* The CCSD iteration split over the ranks of the communicator: the o^3 v^3 ring products, the pp-ladder and every other term that
 * carries a virtual index which can be sliced (the whole T2 residual, the <eb|ia> products, I_vv, two T1 terms) are evaluated for
 * the rank's slice of that index; one all-reduce of [PP | partial T2 residual | partial T1 residual] per iteration; amplitudes,
 * DIIS history and energies stay replicated and identical on every rank (replaces nothing in the reference: its iteration is
 * one process, src/ccsd.f90:340-395).  While the split is on, afesp_ccsd_get_tensor returns sliced intermediates as a rank built
 * them (I_vv, I_ovov, I_voov, x_voov: the rank's slice; I_ooov_p without its t2 <ef|ia> and x_voov terms).
 * Opt-in: mode 1 = split, 0 = replicas, -1 = as the environment says (AFESP_CC_SHARD=1 splits; default replicas;
 * AFESP_CC_SHARD=0 keeps replicas whatever mode says).  *split of afesp_ccsd_is_split = what the next iteration will do. */
int afesp_ccsd_set_split(afesp_ctx* ctx, int mode);
int afesp_ccsd_is_split(afesp_ctx* ctx, int* split);
/* Small systems (o^2 v^2 <= 2^20 amplitudes, one rank): the iteration of afesp_ccsd_iterate / afesp_ccsd_solve -- every contraction
 * site of update_restricted_intermediates and update_amplitudes_restricted (src/ccsd.f90:1040-1312, :1538-1732), update_cc_energy
 * (:1764-1806) and the first half of update_diis_cc (:633-663) -- runs as a compiled sequence of ~11 launches, one grouped launch
 * per dependency level (csrc/fused.h), instead of ~75 launches call by call.  mode 1 = on, 0 = off (the call-by-call path on
 * parallel streams, graph-replayed after AFESP_GRAPH_AFTER iterations), -1 = as the environment says (AFESP_FUSED=0 switches it
 * off; default on).  *launches of afesp_ccsd_iteration_launches = kernel launches of one compiled iteration (0: not compiled,
 * or not eligible). */
int afesp_ccsd_set_fused(afesp_ctx* ctx, int mode);
int afesp_ccsd_iteration_launches(afesp_ctx* ctx, int* launches);
/* Occupied block size of the (T) triple enumeration on this rank's device (it depends on the device memory size and on the
 * AFESP_T_POOL_GIB / AFESP_T_SPLIT_TILES environment): ranks whose values differ would enumerate different flat orders, so
 * callers compare it across ranks before sharding (bench.py and els_amd put it into their first all-reduce). */
int afesp_ccsd_t_block_size(afesp_ctx* ctx, int64_t nocc, int64_t nvirt, int cr, int* block_size);

/* The context's device arena (csrc/contract.hip): out = {allocations that reached the driver, requests served from blocks the
 * context had given back, idle bytes, live bytes}. */
int afesp_arena_stats(afesp_ctx* ctx, double out[4]);

/* Test hook: what = 1 makes the next laned (small-system) amplitude update throw once, from a lane other than the main one
 * -- the failure mode of a capture that dies half-way (tests/test_gpu_cc.py). */
int afesp_test_inject(afesp_ctx* ctx, int what);
/* Test / diagnostic hook, per context: the block Davidson unit of the EOM and response solvers (csrc/davidson_so.h) on a matrix given as
 * data, A = diag(d) + U V^T with U, V of nvec x r column-major (r <= 64; a dense m x m matrix is d = 0, U = A, V = 1), in the metric of n1
 * elements of weight 1 and nvec - n1 of weight w2.  One state per context, beside the EOM and response states and freed with the context
 * (tests/test_gpu_davidson.py).  create: 1 <= nroots <= nvec, 2 nroots <= max_space <= 4096, status 1 otherwise; `diag` is the
 * preconditioner diagonal, given apart from d; follow != 0 keeps the roots nearest to the guess step's.  set_guess / iterate /
 * get_vector are the unit's eigenvalue calls (x1: the first n1 elements, x2: the rest), linear_start / linear_iterate its linear mode for
 * (A - shifts[j]) x_j = -rhs[j % nrhs], j < nroots, with status 26 at a pole as afesp_ccsd_so_response_iterate has it.  counts =
 * {sigma builds, collapses, basis vectors, pending vectors}.  fetch copies what the state holds: what = "B", "S" (basis vectors), "pend"
 * (pending vectors), "x", "sx", "corr" (nroots columns), "diag", "G" (basis x basis, column-major), "prhs" (basis x nrhs), "y" (the
 * coefficients of the last step, basis x roots, then the values of omega given to the Ritz pass; status 1 when no step has finished on the
 * present basis, as after a step that ended at a pole), "target", "counts"; *count = doubles
 * written, status 1 when capacity is smaller.  linear_start_complex starts the complex linear mode (A - (shift_re[j] + i shift_im[j])) x_j =
 * -rhs[j % nrhs] (4 nroots <= max_space and nroots <= 64, status 1 otherwise); linear_iterate then makes its steps, and "x", "sx", "corr"
 * hold 2 nroots columns (2 j: real part of system j, 2 j + 1: imaginary part), "y" Re y and Im y (basis x roots each), then omega and gamma.
 * On a state in a real mode every string answers as before. */
int afesp_test_davidson_create(afesp_ctx* ctx, int64_t n1, int64_t nvec, double w2, int follow, int nroots, int max_space, int r, const double* d,
                               const double* U, const double* V, const double* diag);
int afesp_test_davidson_destroy(afesp_ctx* ctx);
int afesp_test_davidson_set_guess(afesp_ctx* ctx, int k, const double* x1, const double* x2);
int afesp_test_davidson_iterate(afesp_ctx* ctx, double tol, double* omega, double* resnorm, int* flags, int counts[4], int* converged);
int afesp_test_davidson_linear_start(afesp_ctx* ctx, int nrhs, const double* rhs, const double* shifts);
int afesp_test_davidson_linear_start_complex(afesp_ctx* ctx, int nrhs, const double* rhs, const double* shift_re, const double* shift_im);
int afesp_test_davidson_linear_iterate(afesp_ctx* ctx, double tol, double* resnorm, int* flags, int counts[4], int* converged);
int afesp_test_davidson_get_vector(afesp_ctx* ctx, int k, double* x1, double* x2);
int afesp_test_davidson_fetch(afesp_ctx* ctx, const char* what, double* out, int64_t capacity, int64_t* count);
/* Test / diagnostic hook, per context: launches so far of {the streamed tall x skinny kernel, the gather kernel through the operator
 * layer's planner, the LDS-DMA GEMM with 128-row tiles, the LDS-DMA GEMM with 96-row tiles where the rows end} -- tests check with it
 * that a product took the kernel meant for its shape (tests/test_gpu_operators.py, tests/test_gpu_cc.py). */
int afesp_launch_counts(afesp_ctx* ctx, uint64_t out[4]);
/* Test / diagnostic hook, per process: launch sites that have resolved their kernel function under the process-wide first-use lock so
 * far (csrc/first_use.h: every first use of a kernel function -- by a launch, an occupancy query or the start-up thread's preload -- is
 * made under one lock, so two host threads never first-touch a translation unit or a function at the same time). */
uint64_t afesp_first_use_count(void);
/* Test hook, host logic only (no device needed): 1 if a system of these extents takes the grouped ring launches of the LDS-DMA GEMM
 * (csrc/ring.hip: from o v = 3584 on, and only while the 32-bit row byte offsets of an operand reach every row, 8 Kc o v < 4 GiB),
 * 0 if its six o^3 v^3 ring products stay on the gather kernel. */
int afesp_test_ring_path(int64_t nocc, int64_t nvirt);
/* Diagnostic builds only: n > 0: per (workgroup, wave) cycle sums of the GEMM kernel's last launch (tools/stamp_probe.py);
 * n < 0: the first -n phase sums of the (T) orbit kernel since the last call (tools/orbit_stamps.py).  Zeros in a shipped build. */
int afesp_debug_stamps(unsigned long long* out, int n);

/* Operator layer (src/linalg.fpp), exported for parity tests against the oracle.
 * afesp_gemm    = dgemm_wrapper (src/linalg.fpp:58-89): C(m x n) = alpha op(A) op(B) + beta C, host arrays.
 * afesp_permute4 = omp_reshape (src/linalg.fpp:99-156): out(perm) = beta*out + in; has_beta=0 zeroes `out` first. */
int afesp_gemm(afesp_ctx* ctx, char transA, char transB, int64_t m, int64_t n, int64_t k, double alpha, const double* A,
               const double* B, double beta, double* C);
int afesp_permute4(afesp_ctx* ctx, const int64_t dims[4], const char order[4], const double* in, double* out, int has_beta,
                   double beta);
/* General labelled contraction on host arrays (tests): C[lc] = alpha sum A[la] B[lb] + beta C[lc], dense col-major. */
int afesp_contract(afesp_ctx* ctx, double alpha, const double* A, const char* la, const int64_t* dimsA, const double* B,
                   const char* lb, const int64_t* dimsB, double beta, double* C, const char* lc, const int64_t* dimsC,
                   int force_split, int force_tm, int force_tn);

/* ---- device-resident entry points used by bench.py (inputs generated in HBM; nothing crosses PCIe in the timed region)
 * Fill the context with the SURVEY.md 8(d) synthetic system: identity C, ladder orbital energies, hashed ERIs of
 * magnitude `scale` carrying the 8-fold symmetry, written straight into the physicist slices. */
int afesp_synthetic_init(afesp_ctx* ctx, int64_t nocc, int64_t nvirt, double scale, uint64_t seed, int diis_n_errmat);
/* Hashed packed AO integrals of magnitude `scale` left resident on the device, as afesp_read_eri_text leaves a file's:
 * afesp_ao2mo_mp2(eri_packed = NULL) then transforms them (AO->MO timing at sizes with no bundled eri.dat). */
int afesp_synthetic_ao(afesp_ctx* ctx, int64_t nbasis, double scale, uint64_t seed);
/* Floating-point operations of one particle-particle ladder (src/ccsd.f90:1669) as this context evaluates it. */
int afesp_ccsd_pp_ladder_flop(afesp_ctx* ctx, double* flop);
/* ... and of one whole CCSD iteration (src/ccsd.f90:340-395; SURVEY.md 8(d) sum with the two pair-form products as executed). */
int afesp_ccsd_iteration_flop(afesp_ctx* ctx, double* flop);
/* Kernel-only timing helpers: average HIP-event milliseconds per launch over `reps` launches on the context stream. */
int afesp_time_pp_ladder(afesp_ctx* ctx, int reps, double* ms_per_launch);
/* y = a x + b y on n doubles (8 B per lane, 24 n bytes of HBM traffic per launch): PMC calibration / achievable-bandwidth probe. */
int afesp_bench_stream(afesp_ctx* ctx, int64_t n, int reps, double* ms_per_launch);
/* Same for an arbitrary labelled contraction on hashed device operands (dense column-major extents). */
int afesp_bench_contract(afesp_ctx* ctx, const char* la, const int64_t* dimsA, const char* lb, const int64_t* dimsB,
                         const char* lc, const int64_t* dimsC, int reps, double* ms_per_launch);
/* HIP-event timing of the (T) launches on the context stream.  Returns the totals accumulated since the previous call
 * (out = {GEMM ms, GEMM launches, GEMM flop, orbit-kernel ms, orbit launches, orbit algorithmic bytes, GEMM flop including the
 * zero padding its tiles execute, GEMM kernel: 1 LDS-DMA kernel / 0 gather kernel}), clears them and switches the
 * instrumentation on/off for the following afesp_ccsd_t calls. */
int afesp_profile(afesp_ctx* ctx, int enable, double out[8]);
/* Process-wide tuning overrides of the GEMM launcher (0 = heuristic): tile-walk group, tile code, split-K.  Tile codes (tm, tn): tm, tn in
 * {1, 2, 4}, (8,8), (8,16), (16,8), (16,7), (16,6); any other forced pair makes the products that reach the launcher fail (status 3). */
int afesp_set_tuning(int group_m, int force_tm, int force_tn, int force_split);

#ifdef __cplusplus
}
#endif
#endif
