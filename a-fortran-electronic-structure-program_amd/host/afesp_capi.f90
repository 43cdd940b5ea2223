!> ISO_C_BINDING view of include/afesp.h -- the thin C-ABI between the Fortran host and the HIP engine.
!> Every routine returns a status (0 = ok); the host maps non-zero to its error() (reference: src/error_handling.f90:7-20).
module afesp_capi
   use, intrinsic :: iso_c_binding
   implicit none
   private
   public :: afesp_ctx_create, afesp_ctx_destroy, afesp_last_error, afesp_ao2mo_mp2, afesp_ccsd_init, afesp_ccsd_energy, &
             afesp_ccsd_iterate, afesp_ccsd_diis, afesp_ccsd_get_amplitudes, afesp_ccsd_t, afesp_ccsd_t_ntriples, &
             afesp_neri, afesp_error_text, afesp_ccsd_cr_intermediates, afesp_ccsd_t_cr, afesp_ccsd_so_init, &
             afesp_ccsd_so_energy, afesp_ccsd_so_iterate, afesp_ccsd_so_diis, afesp_ccsd_so_t, afesp_ccsd_so_t_ntriples, &
             afesp_read_eri_text, afesp_write_fcidump, afesp_build_fock, afesp_ccsd_t_plain, afesp_device_count, &
             afesp_comm_init, afesp_comm_destroy, afesp_allreduce_sum, afesp_ccsd_t_shard_bounds, afesp_ccsd_t_block_size, &
             afesp_build_fock_uhf, afesp_ao2mo_ump2, afesp_ccsd_uso_init, afesp_mo_window, afesp_umo_window, &
             afesp_mp2_vv_density, afesp_ump2_vv_density, &
             afesp_core_operator, afesp_ucore_operator, afesp_write_fcidump_active, afesp_write_fcidump_uactive, &
             afesp_fcidump_scan, afesp_read_fcidump, afesp_read_fcidump_uhf, &
             afesp_mo_fock_ro, afesp_read_fcidump_rohf, afesp_mo_rotate_uhf, afesp_ccsd_uso_init_fock, &
             afesp_ccsd_so_lambda_init, afesp_ccsd_so_lambda_energy, afesp_ccsd_so_lambda_iterate, afesp_ccsd_so_lambda_diis, &
             afesp_ccsd_so_density, afesp_ccsd_so_lambda_t, afesp_ccsd_so_eom_t, afesp_ccsd_so_get_tensor, &
             afesp_ccsd_so_density2_build, afesp_ccsd_so_density2_get, afesp_ccsd_so_density2_energy, afesp_ccsd_so_density2_expect, &
             afesp_ccsd_so_zvector_solve, afesp_ccsd_so_relaxed_density, &
             afesp_ccsd_so_eom_init, afesp_ccsd_so_eom_sigma, afesp_ccsd_so_eom_guess, afesp_ccsd_so_eom_set_guess, &
             afesp_ccsd_so_eom_iterate, afesp_ccsd_so_eom_get_vector, afesp_eig_general, &
             afesp_ccsd_so_eom_lsigma, afesp_ccsd_so_eom_left_init, afesp_ccsd_so_eom_left_guess, afesp_ccsd_so_eom_left_set_guess, &
             afesp_ccsd_so_eom_left_iterate, afesp_ccsd_so_eom_left_get_vector, afesp_ccsd_so_eom_ref_coupling, &
             afesp_ccsd_so_eom_density, &
             afesp_ccsd_so_eom_ipea_init, afesp_ccsd_so_eom_ipea_sigma, afesp_ccsd_so_eom_ipea_guess, afesp_ccsd_so_eom_ipea_set_guess, &
             afesp_ccsd_so_eom_ipea_iterate, afesp_ccsd_so_eom_ipea_get_vector, AFESP_EOM_IP, AFESP_EOM_EA, &
             afesp_ccsd_so_eom_ipea_lsigma, afesp_ccsd_so_eom_ipea_left_init, afesp_ccsd_so_eom_ipea_left_guess, &
             afesp_ccsd_so_eom_ipea_left_set_guess, afesp_ccsd_so_eom_ipea_left_iterate, afesp_ccsd_so_eom_ipea_left_get_vector, &
             afesp_ccsd_so_eom_ipea_dyson, afesp_ccsd_so_eom_ipea_t, afesp_ccsd_so_eom_ipea_t_nitems, &
             afesp_ccsd_so_response_init, afesp_ccsd_so_response_iterate, afesp_ccsd_so_response_function, &
             afesp_ccsd_so_response_init_complex, afesp_ccsd_so_response_function_complex, &
             AFESP_COMM_RCCL, AFESP_COMM_HOST

   integer(c_int), parameter :: AFESP_COMM_RCCL = 0, AFESP_COMM_HOST = 1
   integer(c_int), parameter :: AFESP_EOM_IP = 1, AFESP_EOM_EA = 2   ! the sector of the afesp_ccsd_so_eom_ipea_* calls

   interface
      function afesp_ctx_create(device, ctx) bind(C, name='afesp_ctx_create') result(rc)
         import :: c_int, c_ptr
         integer(c_int), value :: device
         type(c_ptr), intent(out) :: ctx
         integer(c_int) :: rc
      end function
      subroutine afesp_ctx_destroy(ctx) bind(C, name='afesp_ctx_destroy')
         import :: c_ptr
         type(c_ptr), value :: ctx
      end subroutine
      function afesp_last_error(ctx) bind(C, name='afesp_last_error') result(msg)
         import :: c_ptr
         type(c_ptr), value :: ctx
         type(c_ptr) :: msg
      end function
      function afesp_neri(nbasis) bind(C, name='afesp_neri') result(n)
         import :: c_int64_t
         integer(c_int64_t), value :: nbasis
         integer(c_int64_t) :: n
      end function
      !> replaces `call do_mp2_spatial(sys, int_store)` (reference src/main.F90:98)
      function afesp_ao2mo_mp2(ctx, nbasis, nocc, canon_coeff, canon_levels, eri_packed, eri_mo_packed, e_mp2) &
         bind(C, name='afesp_ao2mo_mp2') result(rc)
         import :: c_int, c_int64_t, c_double, c_ptr
         type(c_ptr), value :: ctx
         integer(c_int64_t), value :: nbasis, nocc
         real(c_double), intent(in) :: canon_coeff(*), canon_levels(*)
         type(c_ptr), value :: eri_packed             ! c_loc(int_store%eri), or c_null_ptr after afesp_read_eri_text
         type(c_ptr), value :: eri_mo_packed          ! c_null_ptr keeps the MO integrals on the device only
         real(c_double), intent(out) :: e_mp2
         integer(c_int) :: rc
      end function
      !> replaces init_cc + init_diis_cc_t (reference src/ccsd.f90:313-316)
      function afesp_ccsd_init(ctx, nocc, nvirt, eri_mo_packed, canon_levels, diis_n_errmat) &
         bind(C, name='afesp_ccsd_init') result(rc)
         import :: c_int, c_int64_t, c_double, c_ptr
         type(c_ptr), value :: ctx
         integer(c_int64_t), value :: nocc, nvirt
         type(c_ptr), value :: eri_mo_packed
         real(c_double), intent(in) :: canon_levels(*)
         integer(c_int), value :: diis_n_errmat
         integer(c_int) :: rc
      end function
      !> update_cc_energy on the current amplitudes (reference src/ccsd.f90:325)
      function afesp_ccsd_energy(ctx, e_tol, t_tol, energy, rms_sq, converged) bind(C, name='afesp_ccsd_energy') result(rc)
         import :: c_int, c_double, c_ptr
         type(c_ptr), value :: ctx
         real(c_double), value :: e_tol, t_tol
         real(c_double), intent(out) :: energy, rms_sq
         integer(c_int), intent(out) :: converged
         integer(c_int) :: rc
      end function
      !> one pass of the loop body (reference src/ccsd.f90:340-360)
      function afesp_ccsd_iterate(ctx, e_tol, t_tol, energy, rms_sq, converged) bind(C, name='afesp_ccsd_iterate') result(rc)
         import :: c_int, c_double, c_ptr
         type(c_ptr), value :: ctx
         real(c_double), value :: e_tol, t_tol
         real(c_double), intent(out) :: energy, rms_sq
         integer(c_int), intent(out) :: converged
         integer(c_int) :: rc
      end function
      !> update_diis_cc (reference src/ccsd.f90:395)
      function afesp_ccsd_diis(ctx) bind(C, name='afesp_ccsd_diis') result(rc)
         import :: c_int, c_ptr
         type(c_ptr), value :: ctx
         integer(c_int) :: rc
      end function
      function afesp_ccsd_get_amplitudes(ctx, t1, t2) bind(C, name='afesp_ccsd_get_amplitudes') result(rc)
         import :: c_int, c_double, c_ptr
         type(c_ptr), value :: ctx
         real(c_double), intent(out) :: t1(*), t2(*)
         integer(c_int) :: rc
      end function
      function afesp_ccsd_t_ntriples(nocc) bind(C, name='afesp_ccsd_t_ntriples') result(n)
         import :: c_int64_t
         integer(c_int64_t), value :: nocc
         integer(c_int64_t) :: n
      end function
      !> replaces `call do_ccsd_t_spatial(...)` (reference src/main.F90:112); out = E[T], E(T), D[T], D(T)
      function afesp_ccsd_t(ctx, t_begin, t_end, out) bind(C, name='afesp_ccsd_t') result(rc)
         import :: c_int, c_int64_t, c_double, c_ptr
         type(c_ptr), value :: ctx
         integer(c_int64_t), value :: t_begin, t_end
         real(c_double), intent(out) :: out(4)
         integer(c_int) :: rc
      end function
      !> the same for the plain CCSD(T)/CCSD[T] types: out = E[T], E(T) (no y, no D sums -- reference src/ccsd.f90:2181-2185)
      function afesp_ccsd_t_plain(ctx, t_begin, t_end, out) bind(C, name='afesp_ccsd_t_plain') result(rc)
         import :: c_int, c_int64_t, c_double, c_ptr
         type(c_ptr), value :: ctx
         integer(c_int64_t), value :: t_begin, t_end
         real(c_double), intent(out) :: out(2)
         integer(c_int) :: rc
      end function
      !> replaces build_cr_ccsd_t_intermediates (reference src/ccsd.f90:381)
      function afesp_ccsd_cr_intermediates(ctx) bind(C, name='afesp_ccsd_cr_intermediates') result(rc)
         import :: c_int, c_ptr
         type(c_ptr), value :: ctx
         integer(c_int) :: rc
      end function
      !> (T) with the completely renormalised moment sums: out = E[T], E(T), D[T], D(T), sum t_bar.M3, sum (t_bar+z_bar).M3
      function afesp_ccsd_t_cr(ctx, t_begin, t_end, out) bind(C, name='afesp_ccsd_t_cr') result(rc)
         import :: c_int, c_int64_t, c_double, c_ptr
         type(c_ptr), value :: ctx
         integer(c_int64_t), value :: t_begin, t_end
         real(c_double), intent(out) :: out(6)
         integer(c_int) :: rc
      end function
      !> replaces the two-body loop of read_integrals_in (reference src/integrals.f90:146-161); the packed AO integrals
      !> also stay on the device for afesp_ao2mo_mp2(..., eri_packed = c_null_ptr, ...)
      function afesp_read_eri_text(ctx, path, nbasis, eri_packed, nread) bind(C, name='afesp_read_eri_text') result(rc)
         import :: c_int, c_int64_t, c_double, c_ptr, c_char
         type(c_ptr), value :: ctx
         character(kind=c_char), intent(in) :: path(*)
         integer(c_int64_t), value :: nbasis
         real(c_double), intent(out) :: eri_packed(*)
         integer(c_int64_t), intent(out) :: nread
         integer(c_int) :: rc
      end function
      !> replaces build_fock (reference src/hf.f90:349-385) on the packed AO integrals resident after afesp_read_eri_text
      function afesp_build_fock(ctx, nbasis, density, core_hamil, fock) bind(C, name='afesp_build_fock') result(rc)
         import :: c_int, c_int64_t, c_double, c_ptr
         type(c_ptr), value :: ctx
         integer(c_int64_t), value :: nbasis
         real(c_double), intent(in) :: density(*), core_hamil(*)
         real(c_double), intent(out) :: fock(*)
         integer(c_int) :: rc
      end function
      !> open-shell path (include/afesp.h): F_s = H + J[Da + Db] - K[D_s] for both spins
      function afesp_build_fock_uhf(ctx, nbasis, dens_a, dens_b, core_hamil, fock_a, fock_b) &
         bind(C, name='afesp_build_fock_uhf') result(rc)
         import :: c_int, c_int64_t, c_double, c_ptr
         type(c_ptr), value :: ctx
         integer(c_int64_t), value :: nbasis
         real(c_double), intent(in) :: dens_a(*), dens_b(*), core_hamil(*)
         real(c_double), intent(out) :: fock_a(*), fock_b(*)
         integer(c_int) :: rc
      end function
      !> the alpha-alpha, alpha-beta and beta-beta MO integrals (left on the device) and E(UMP2)
      function afesp_ao2mo_ump2(ctx, nbasis, nalpha, nbeta, coeff_a, coeff_b, levels_a, levels_b, eri_packed, eri_aa, eri_ab, &
                                eri_bb, e_ump2) bind(C, name='afesp_ao2mo_ump2') result(rc)
         import :: c_int, c_int64_t, c_double, c_ptr
         type(c_ptr), value :: ctx
         integer(c_int64_t), value :: nbasis, nalpha, nbeta
         real(c_double), intent(in) :: coeff_a(*), coeff_b(*), levels_a(*), levels_b(*)
         type(c_ptr), value :: eri_packed, eri_aa, eri_ab, eri_bb
         real(c_double), intent(out) :: e_ump2
         integer(c_int) :: rc
      end function
      !> the spin-orbital CCSD state from those blocks; afesp_ccsd_so_* drive it afterwards
      function afesp_ccsd_uso_init(ctx, nbasis, nalpha, nbeta, levels_a, levels_b, diis_n_errmat) &
         bind(C, name='afesp_ccsd_uso_init') result(rc)
         import :: c_int, c_int64_t, c_double, c_ptr
         type(c_ptr), value :: ctx
         integer(c_int64_t), value :: nbasis, nalpha, nbeta
         real(c_double), intent(in) :: levels_a(*), levels_b(*)
         integer(c_int), value :: diis_n_errmat
         integer(c_int) :: rc
      end function
      !> the active orbital window [nfc, nbasis - nfv) of the resident MO integrals (frozen core / frozen virtuals): afterwards
      !> afesp_ccsd_init / afesp_ccsd_so_init / the (T) calls take the active extents and canon_levels(nfc + 1:)
      function afesp_mo_window(ctx, nbasis, nocc, n_frozen_core, n_frozen_virt, canon_levels, eri_mo_packed, eri_act, e_mp2) &
         bind(C, name='afesp_mo_window') result(rc)
         import :: c_int, c_int64_t, c_double, c_ptr
         type(c_ptr), value :: ctx
         integer(c_int64_t), value :: nbasis, nocc, n_frozen_core, n_frozen_virt
         real(c_double), intent(in) :: canon_levels(*)
         type(c_ptr), value :: eri_mo_packed, eri_act
         real(c_double), intent(out) :: e_mp2
         integer(c_int) :: rc
      end function
      !> the same for the three blocks afesp_ao2mo_ump2 left; afterwards afesp_ccsd_uso_init with the active extents
      function afesp_umo_window(ctx, nbasis, nalpha, nbeta, n_frozen_core, n_frozen_virt, levels_a, levels_b, eri_aa, eri_ab, &
                                eri_bb, e_ump2) bind(C, name='afesp_umo_window') result(rc)
         import :: c_int, c_int64_t, c_double, c_ptr
         type(c_ptr), value :: ctx
         integer(c_int64_t), value :: nbasis, nalpha, nbeta, n_frozen_core, n_frozen_virt
         real(c_double), intent(in) :: levels_a(*), levels_b(*)
         type(c_ptr), value :: eri_aa, eri_ab, eri_bb
         real(c_double), intent(out) :: e_ump2
         integer(c_int) :: rc
      end function
      !> frozen natural orbitals: the virtual-virtual block of the MP2 one-particle density from the resident MO integrals, before any
      !> window (include/afesp.h); d_vv is v x v, symmetric to the bit; e_mp2 = the frozen-core MP2 energy of the full virtual space
      function afesp_mp2_vv_density(ctx, nbasis, nocc, n_frozen_core, canon_levels, d_vv, e_mp2) &
         bind(C, name='afesp_mp2_vv_density') result(rc)
         import :: c_int, c_int64_t, c_double, c_ptr
         type(c_ptr), value :: ctx
         integer(c_int64_t), value :: nbasis, nocc, n_frozen_core
         real(c_double), intent(in) :: canon_levels(*)
         real(c_double), intent(out) :: d_vv(*)
         real(c_double), intent(out) :: e_mp2
         integer(c_int) :: rc
      end function
      !> the same for the three blocks afesp_ao2mo_ump2 left: d_a (va x va), d_b (vb x vb)
      function afesp_ump2_vv_density(ctx, nbasis, nalpha, nbeta, n_frozen_core, levels_a, levels_b, d_a, d_b, e_ump2) &
         bind(C, name='afesp_ump2_vv_density') result(rc)
         import :: c_int, c_int64_t, c_double, c_ptr
         type(c_ptr), value :: ctx
         integer(c_int64_t), value :: nbasis, nalpha, nbeta, n_frozen_core
         real(c_double), intent(in) :: levels_a(*), levels_b(*)
         real(c_double), intent(out) :: d_a(*), d_b(*)
         real(c_double), intent(out) :: e_ump2
         integer(c_int) :: rc
      end function
      !> the frozen-core operator of the window [nfc, nbasis - nfv) and the core energy from the full resident MO integrals, BEFORE the
      !> window (include/afesp.h): h_act is n_act x n_act, symmetric to the bit; e_core is electronic
      function afesp_core_operator(ctx, nbasis, n_frozen_core, n_frozen_virt, canon_coeff, core_hamil_ao, h_act, e_core) &
         bind(C, name='afesp_core_operator') result(rc)
         import :: c_int, c_int64_t, c_double, c_ptr
         type(c_ptr), value :: ctx
         integer(c_int64_t), value :: nbasis, n_frozen_core, n_frozen_virt
         real(c_double), intent(in) :: canon_coeff(*), core_hamil_ao(*)
         real(c_double), intent(out) :: h_act(*)
         real(c_double), intent(out) :: e_core
         integer(c_int) :: rc
      end function
      function afesp_ucore_operator(ctx, nbasis, n_frozen_core, n_frozen_virt, coeff_a, coeff_b, core_hamil_ao, h_act_a, h_act_b, &
                                    e_core) bind(C, name='afesp_ucore_operator') result(rc)
         import :: c_int, c_int64_t, c_double, c_ptr
         type(c_ptr), value :: ctx
         integer(c_int64_t), value :: nbasis, n_frozen_core, n_frozen_virt
         real(c_double), intent(in) :: coeff_a(*), coeff_b(*), core_hamil_ao(*)
         real(c_double), intent(out) :: h_act_a(*), h_act_b(*)
         real(c_double), intent(out) :: e_core
         integer(c_int) :: rc
      end function
      !> the integrals resident for n_act orbitals as a standard FCIDUMP (header, two-electron, one-electron, core energy: include/afesp.h)
      function afesp_write_fcidump_active(ctx, path, n_act, nelec_act, ms2, h_act, e_core_total, threshold, nwritten) &
         bind(C, name='afesp_write_fcidump_active') result(rc)
         import :: c_int, c_int64_t, c_double, c_ptr, c_char
         type(c_ptr), value :: ctx
         character(kind=c_char), intent(in) :: path(*)
         integer(c_int64_t), value :: n_act, nelec_act, ms2
         real(c_double), intent(in) :: h_act(*)
         real(c_double), value :: e_core_total, threshold
         integer(c_int64_t), intent(out) :: nwritten
         integer(c_int) :: rc
      end function
      function afesp_write_fcidump_uactive(ctx, path, n_act, nalpha_act, nbeta_act, h_act_a, h_act_b, e_core_total, threshold, &
                                           nwritten) bind(C, name='afesp_write_fcidump_uactive') result(rc)
         import :: c_int, c_int64_t, c_double, c_ptr, c_char
         type(c_ptr), value :: ctx
         character(kind=c_char), intent(in) :: path(*)
         integer(c_int64_t), value :: n_act, nalpha_act, nbeta_act
         real(c_double), intent(in) :: h_act_a(*), h_act_b(*)
         real(c_double), value :: e_core_total, threshold
         integer(c_int64_t), intent(out) :: nwritten
         integer(c_int) :: rc
      end function
      !> a standard FCIDUMP as input (include/afesp.h).  afesp_fcidump_scan: host only, the header and the number of lines after it
      function afesp_fcidump_scan(path, norb, nelec, ms2, uhf, nlines) bind(C, name='afesp_fcidump_scan') result(rc)
         import :: c_int, c_int64_t, c_char
         character(kind=c_char), intent(in) :: path(*)
         integer(c_int64_t), intent(out) :: norb, nelec, ms2, nlines
         integer(c_int), intent(out) :: uhf
         integer(c_int) :: rc
      end function
      !> the file onto the device, resident as afesp_ao2mo_mp2 leaves its result; h_mo, fock (n x n), levels (n) and eri_mo_packed may be
      !> c_null_ptr; e_ref = the energy of the determinant of the first nocc orbitals, fock_offdiag = max |F(p,q)|, p /= q
      function afesp_read_fcidump(ctx, path, nbasis, nocc, h_mo, fock, levels, e_core, e_ref, fock_offdiag, eri_mo_packed, nread) &
         bind(C, name='afesp_read_fcidump') result(rc)
         import :: c_int, c_int64_t, c_double, c_ptr, c_char
         type(c_ptr), value :: ctx
         character(kind=c_char), intent(in) :: path(*)
         integer(c_int64_t), value :: nbasis, nocc
         type(c_ptr), value :: h_mo, fock, levels, eri_mo_packed
         real(c_double), intent(out) :: e_core, e_ref, fock_offdiag
         integer(c_int64_t), intent(out) :: nread
         integer(c_int) :: rc
      end function
      !> the same for a UHF=.TRUE. file: the three blocks resident as afesp_ao2mo_ump2 leaves them
      function afesp_read_fcidump_uhf(ctx, path, nbasis, nalpha, nbeta, h_a, h_b, fock_a, fock_b, levels_a, levels_b, e_core, e_ref, &
                                      fock_offdiag, eri_aa, eri_ab, eri_bb, nread) bind(C, name='afesp_read_fcidump_uhf') result(rc)
         import :: c_int, c_int64_t, c_double, c_ptr, c_char
         type(c_ptr), value :: ctx
         character(kind=c_char), intent(in) :: path(*)
         integer(c_int64_t), value :: nbasis, nalpha, nbeta
         type(c_ptr), value :: h_a, h_b, fock_a, fock_b, levels_a, levels_b, eri_aa, eri_ab, eri_bb
         real(c_double), intent(out) :: e_core, e_ref, fock_offdiag
         integer(c_int64_t), intent(out) :: nread
         integer(c_int) :: rc
      end function
      !> restricted open-shell references (include/afesp.h): the two spin Fock operators of a restricted determinant on the resident packed
      !> MO array, the reader of a restricted file with MS2 >= 0, the spin-dependent rotation of the resident MO integrals into the three
      !> blocks of the open-shell path, and the spin-orbital state with the full Fock matrices of those orbitals
      function afesp_mo_fock_ro(ctx, nbasis, nalpha, nbeta, h_mo, fock_a, fock_b, e_ref_elec) bind(C, name='afesp_mo_fock_ro') result(rc)
         import :: c_int, c_int64_t, c_double, c_ptr
         type(c_ptr), value :: ctx
         integer(c_int64_t), value :: nbasis, nalpha, nbeta
         real(c_double), intent(in) :: h_mo(*)
         real(c_double), intent(out) :: fock_a(*), fock_b(*), e_ref_elec
         integer(c_int) :: rc
      end function
      function afesp_read_fcidump_rohf(ctx, path, nbasis, nalpha, nbeta, h_mo, fock_a, fock_b, e_core, e_ref, fock_offdiag, &
                                       eri_mo_packed, nread) bind(C, name='afesp_read_fcidump_rohf') result(rc)
         import :: c_int, c_int64_t, c_double, c_ptr, c_char
         type(c_ptr), value :: ctx
         character(kind=c_char), intent(in) :: path(*)
         integer(c_int64_t), value :: nbasis, nalpha, nbeta
         type(c_ptr), value :: h_mo, fock_a, fock_b, eri_mo_packed
         real(c_double), intent(out) :: e_core, e_ref, fock_offdiag(3)
         integer(c_int64_t), intent(out) :: nread
         integer(c_int) :: rc
      end function
      function afesp_mo_rotate_uhf(ctx, nbasis, u_a, u_b, eri_aa, eri_ab, eri_bb) bind(C, name='afesp_mo_rotate_uhf') result(rc)
         import :: c_int, c_int64_t, c_double, c_ptr
         type(c_ptr), value :: ctx
         integer(c_int64_t), value :: nbasis
         real(c_double), intent(in) :: u_a(*), u_b(*)
         type(c_ptr), value :: eri_aa, eri_ab, eri_bb
         integer(c_int) :: rc
      end function
      function afesp_ccsd_uso_init_fock(ctx, nbasis, nalpha, nbeta, fock_a, fock_b, diis_n_errmat, e_mp2) &
         bind(C, name='afesp_ccsd_uso_init_fock') result(rc)
         import :: c_int, c_int64_t, c_double, c_ptr
         type(c_ptr), value :: ctx
         integer(c_int64_t), value :: nbasis, nalpha, nbeta
         real(c_double), intent(in) :: fock_a(*), fock_b(*)
         integer(c_int), value :: diis_n_errmat
         real(c_double), intent(out) :: e_mp2
         integer(c_int) :: rc
      end function
      !> replaces write_fcidump (reference src/mp2.f90:451-487)
      function afesp_write_fcidump(ctx, path, nbasis, nwritten) bind(C, name='afesp_write_fcidump') result(rc)
         import :: c_int, c_int64_t, c_ptr, c_char
         type(c_ptr), value :: ctx
         character(kind=c_char), intent(in) :: path(*)
         integer(c_int64_t), value :: nbasis
         integer(c_int64_t), intent(out) :: nwritten
         integer(c_int) :: rc
      end function
      !> replaces the integral/slice/init part of do_ccsd_spinorb (reference src/ccsd.f90:100-215); flags bit 0 = Stanton's
      !> index order for the tau~ term of F_mi (see include/afesp.h)
      function afesp_ccsd_so_init(ctx, nbasis, nel, eri_mo_packed, canon_levels, diis_n_errmat, flags) &
         bind(C, name='afesp_ccsd_so_init') result(rc)
         import :: c_int, c_int64_t, c_double, c_ptr
         type(c_ptr), value :: ctx
         integer(c_int64_t), value :: nbasis, nel
         type(c_ptr), value :: eri_mo_packed
         real(c_double), intent(in) :: canon_levels(*)
         integer(c_int), value :: diis_n_errmat, flags
         integer(c_int) :: rc
      end function
      !> update_cc_energy, unrestricted branch (reference src/ccsd.f90:217)
      function afesp_ccsd_so_energy(ctx, e_tol, t_tol, energy, rms_sq, converged) bind(C, name='afesp_ccsd_so_energy') result(rc)
         import :: c_int, c_double, c_ptr
         type(c_ptr), value :: ctx
         real(c_double), value :: e_tol, t_tol
         real(c_double), intent(out) :: energy, rms_sq
         integer(c_int), intent(out) :: converged
         integer(c_int) :: rc
      end function
      !> build_tau, build_F, build_W, update_amplitudes, update_cc_energy (reference src/ccsd.f90:238-245)
      function afesp_ccsd_so_iterate(ctx, e_tol, t_tol, energy, rms_sq, converged) bind(C, name='afesp_ccsd_so_iterate') result(rc)
         import :: c_int, c_double, c_ptr
         type(c_ptr), value :: ctx
         real(c_double), value :: e_tol, t_tol
         real(c_double), intent(out) :: energy, rms_sq
         integer(c_int), intent(out) :: converged
         integer(c_int) :: rc
      end function
      function afesp_ccsd_so_diis(ctx) bind(C, name='afesp_ccsd_so_diis') result(rc)
         import :: c_int, c_ptr
         type(c_ptr), value :: ctx
         integer(c_int) :: rc
      end function
      !> Lambda of the spin-orbital state and its unrelaxed one-particle density (include/afesp.h): init from the current t1 / t2, then
      !> Jacobi steps with DIIS on the Lambda ring; d is (o+v) x (o+v) in the state's spin-orbital order
      function afesp_ccsd_so_lambda_init(ctx, diis_n_errmat) bind(C, name='afesp_ccsd_so_lambda_init') result(rc)
         import :: c_int, c_ptr
         type(c_ptr), value :: ctx
         integer(c_int), value :: diis_n_errmat
         integer(c_int) :: rc
      end function
      function afesp_ccsd_so_lambda_energy(ctx, e_tol, l_tol, pseudo_energy, rms_sq, converged) &
         bind(C, name='afesp_ccsd_so_lambda_energy') result(rc)
         import :: c_int, c_double, c_ptr
         type(c_ptr), value :: ctx
         real(c_double), value :: e_tol, l_tol
         real(c_double), intent(out) :: pseudo_energy, rms_sq
         integer(c_int), intent(out) :: converged
         integer(c_int) :: rc
      end function
      function afesp_ccsd_so_lambda_iterate(ctx, e_tol, l_tol, pseudo_energy, rms_sq, converged) &
         bind(C, name='afesp_ccsd_so_lambda_iterate') result(rc)
         import :: c_int, c_double, c_ptr
         type(c_ptr), value :: ctx
         real(c_double), value :: e_tol, l_tol
         real(c_double), intent(out) :: pseudo_energy, rms_sq
         integer(c_int), intent(out) :: converged
         integer(c_int) :: rc
      end function
      function afesp_ccsd_so_lambda_diis(ctx) bind(C, name='afesp_ccsd_so_lambda_diis') result(rc)
         import :: c_int, c_ptr
         type(c_ptr), value :: ctx
         integer(c_int) :: rc
      end function
      function afesp_ccsd_so_density(ctx, d, capacity) bind(C, name='afesp_ccsd_so_density') result(rc)
         import :: c_int, c_int64_t, c_double, c_ptr
         type(c_ptr), value :: ctx
         real(c_double), intent(out) :: d(*)
         integer(c_int64_t), value :: capacity
         integer(c_int) :: rc
      end function
      ! the two-particle density of the current t and lambda of a live Lambda state (include/afesp.h)
      function afesp_ccsd_so_density2_build(ctx) bind(C, name='afesp_ccsd_so_density2_build') result(rc)
         import :: c_int, c_ptr
         type(c_ptr), value :: ctx
         integer(c_int) :: rc
      end function
      function afesp_ccsd_so_density2_get(ctx, name, gamma, capacity) bind(C, name='afesp_ccsd_so_density2_get') result(rc)
         import :: c_int, c_int64_t, c_double, c_char, c_ptr
         type(c_ptr), value :: ctx
         character(kind=c_char), intent(in) :: name(*)
         real(c_double), intent(out) :: gamma(*)
         integer(c_int64_t), value :: capacity
         integer(c_int) :: rc
      end function
      function afesp_ccsd_so_density2_energy(ctx, e) bind(C, name='afesp_ccsd_so_density2_energy') result(rc)
         import :: c_int, c_double, c_ptr
         type(c_ptr), value :: ctx
         real(c_double), intent(out) :: e(8)
         integer(c_int) :: rc
      end function
      function afesp_ccsd_so_density2_expect(ctx, a, b, val) bind(C, name='afesp_ccsd_so_density2_expect') result(rc)
         import :: c_int, c_double, c_ptr
         type(c_ptr), value :: ctx
         real(c_double), intent(in) :: a(*), b(*)
         real(c_double), intent(out) :: val
         integer(c_int) :: rc
      end function
      ! orbital relaxation: the Z-vector equations and the relaxed one-particle density (include/afesp.h)
      function afesp_ccsd_so_zvector_solve(ctx, tol, maxiter, z, iters, resid) bind(C, name='afesp_ccsd_so_zvector_solve') result(rc)
         import :: c_int, c_double, c_ptr
         type(c_ptr), value :: ctx
         real(c_double), value :: tol
         integer(c_int), value :: maxiter
         real(c_double), intent(out) :: z(*)
         integer(c_int), intent(out) :: iters
         real(c_double), intent(out) :: resid
         integer(c_int) :: rc
      end function
      function afesp_ccsd_so_relaxed_density(ctx, d, capacity) bind(C, name='afesp_ccsd_so_relaxed_density') result(rc)
         import :: c_int, c_int64_t, c_double, c_ptr
         type(c_ptr), value :: ctx
         real(c_double), intent(out) :: d(*)
         integer(c_int64_t), value :: capacity
         integer(c_int) :: rc
      end function
      ! EOM-EE-CCSD excitation energies on the live Lambda state's H-bar elements (include/afesp.h)
      function afesp_ccsd_so_eom_init(ctx, nroots, max_space) bind(C, name='afesp_ccsd_so_eom_init') result(rc)
         import :: c_int, c_ptr
         type(c_ptr), value :: ctx
         integer(c_int), value :: nroots, max_space
         integer(c_int) :: rc
      end function
      function afesp_ccsd_so_eom_sigma(ctx, nvec, r1, r2, s1, s2) bind(C, name='afesp_ccsd_so_eom_sigma') result(rc)
         import :: c_int, c_double, c_ptr
         type(c_ptr), value :: ctx
         integer(c_int), value :: nvec
         real(c_double), intent(in) :: r1(*), r2(*)
         real(c_double), intent(out) :: s1(*), s2(*)
         integer(c_int) :: rc
      end function
      function afesp_ccsd_so_eom_guess(ctx) bind(C, name='afesp_ccsd_so_eom_guess') result(rc)
         import :: c_int, c_ptr
         type(c_ptr), value :: ctx
         integer(c_int) :: rc
      end function
      function afesp_ccsd_so_eom_set_guess(ctx, k, r1, r2) bind(C, name='afesp_ccsd_so_eom_set_guess') result(rc)
         import :: c_int, c_double, c_ptr
         type(c_ptr), value :: ctx
         integer(c_int), value :: k
         real(c_double), intent(in) :: r1(*), r2(*)
         integer(c_int) :: rc
      end function
      function afesp_ccsd_so_eom_iterate(ctx, tol, omega, resnorm, flags, nsigma, converged) &
         bind(C, name='afesp_ccsd_so_eom_iterate') result(rc)
         import :: c_int, c_double, c_ptr
         type(c_ptr), value :: ctx
         real(c_double), value :: tol
         real(c_double), intent(out) :: omega(*), resnorm(*)
         integer(c_int), intent(out) :: flags(*), nsigma, converged
         integer(c_int) :: rc
      end function
      function afesp_ccsd_so_eom_get_vector(ctx, k, r1, r2) bind(C, name='afesp_ccsd_so_eom_get_vector') result(rc)
         import :: c_int, c_double, c_ptr
         type(c_ptr), value :: ctx
         integer(c_int), value :: k
         real(c_double), intent(out) :: r1(*), r2(*)
         integer(c_int) :: rc
      end function
      ! EOM-EE-CCSD left eigenvectors (the right-hand calls on a second Davidson state, for A^T), the coupling of right vectors to the
      ! reference and the bilinear one-particle density (include/afesp.h)
      function afesp_ccsd_so_eom_lsigma(ctx, nvec, l1, l2, s1, s2) bind(C, name='afesp_ccsd_so_eom_lsigma') result(rc)
         import :: c_int, c_double, c_ptr
         type(c_ptr), value :: ctx
         integer(c_int), value :: nvec
         real(c_double), intent(in) :: l1(*), l2(*)
         real(c_double), intent(out) :: s1(*), s2(*)
         integer(c_int) :: rc
      end function
      function afesp_ccsd_so_eom_left_init(ctx, nroots, max_space) bind(C, name='afesp_ccsd_so_eom_left_init') result(rc)
         import :: c_int, c_ptr
         type(c_ptr), value :: ctx
         integer(c_int), value :: nroots, max_space
         integer(c_int) :: rc
      end function
      function afesp_ccsd_so_eom_left_guess(ctx) bind(C, name='afesp_ccsd_so_eom_left_guess') result(rc)
         import :: c_int, c_ptr
         type(c_ptr), value :: ctx
         integer(c_int) :: rc
      end function
      function afesp_ccsd_so_eom_left_set_guess(ctx, k, l1, l2) bind(C, name='afesp_ccsd_so_eom_left_set_guess') result(rc)
         import :: c_int, c_double, c_ptr
         type(c_ptr), value :: ctx
         integer(c_int), value :: k
         real(c_double), intent(in) :: l1(*), l2(*)
         integer(c_int) :: rc
      end function
      function afesp_ccsd_so_eom_left_iterate(ctx, tol, omega, resnorm, flags, nsigma, converged) &
         bind(C, name='afesp_ccsd_so_eom_left_iterate') result(rc)
         import :: c_int, c_double, c_ptr
         type(c_ptr), value :: ctx
         real(c_double), value :: tol
         real(c_double), intent(out) :: omega(*), resnorm(*)
         integer(c_int), intent(out) :: flags(*), nsigma, converged
         integer(c_int) :: rc
      end function
      function afesp_ccsd_so_eom_left_get_vector(ctx, k, l1, l2) bind(C, name='afesp_ccsd_so_eom_left_get_vector') result(rc)
         import :: c_int, c_double, c_ptr
         type(c_ptr), value :: ctx
         integer(c_int), value :: k
         real(c_double), intent(out) :: l1(*), l2(*)
         integer(c_int) :: rc
      end function
      function afesp_ccsd_so_eom_ref_coupling(ctx, nvec, r1, r2, c) bind(C, name='afesp_ccsd_so_eom_ref_coupling') result(rc)
         import :: c_int, c_double, c_ptr
         type(c_ptr), value :: ctx
         integer(c_int), value :: nvec
         real(c_double), intent(in) :: r1(*), r2(*)
         real(c_double), intent(out) :: c(*)
         integer(c_int) :: rc
      end function
      ! (l1 / l2 and r1 / r2 are C pointers: c_null_ptr for an absent vector, c_loc of the array otherwise)
      function afesp_ccsd_so_eom_density(ctx, l0, l1, l2, r0, r1, r2, d, capacity) bind(C, name='afesp_ccsd_so_eom_density') result(rc)
         import :: c_int, c_int64_t, c_double, c_ptr
         type(c_ptr), value :: ctx
         real(c_double), value :: l0, r0
         type(c_ptr), value :: l1, l2, r1, r2
         real(c_double), intent(out) :: d(*)
         integer(c_int64_t), value :: capacity
         integer(c_int) :: rc
      end function
      ! EOM-CCSD linear response (include/afesp.h): x holds nop operators of (o+v)^2 each, omega the signed frequencies
      function afesp_ccsd_so_response_init(ctx, nop, x, nfreq_signed, omega, max_space) bind(C, name='afesp_ccsd_so_response_init') result(rc)
         import :: c_int, c_double, c_ptr
         type(c_ptr), value :: ctx
         integer(c_int), value :: nop, nfreq_signed, max_space
         real(c_double), intent(in) :: x(*), omega(*)
         integer(c_int) :: rc
      end function
      function afesp_ccsd_so_response_iterate(ctx, tol, resnorm, nsigma, converged) bind(C, name='afesp_ccsd_so_response_iterate') result(rc)
         import :: c_int, c_double, c_ptr
         type(c_ptr), value :: ctx
         real(c_double), value :: tol
         real(c_double), intent(out) :: resnorm(*)
         integer(c_int), intent(out) :: nsigma, converged
         integer(c_int) :: rc
      end function
      function afesp_ccsd_so_response_function(ctx, nfreq, omega, res) bind(C, name='afesp_ccsd_so_response_function') result(rc)
         import :: c_int, c_double, c_ptr
         type(c_ptr), value :: ctx
         integer(c_int), value :: nfreq
         real(c_double), intent(in) :: omega(*)
         real(c_double), intent(out) :: res(*)
         integer(c_int) :: rc
      end function
      ! the same at complex frequencies: z holds (re, im) pairs, res (re, im) pairs of <<X_a;X_b>>_z; _iterate steps either kind of state
      function afesp_ccsd_so_response_init_complex(ctx, nop, x, nfreq_signed, z, max_space) &
         bind(C, name='afesp_ccsd_so_response_init_complex') result(rc)
         import :: c_int, c_double, c_ptr
         type(c_ptr), value :: ctx
         integer(c_int), value :: nop, nfreq_signed, max_space
         real(c_double), intent(in) :: x(*), z(*)
         integer(c_int) :: rc
      end function
      function afesp_ccsd_so_response_function_complex(ctx, nfreq, z, res) bind(C, name='afesp_ccsd_so_response_function_complex') result(rc)
         import :: c_int, c_double, c_ptr
         type(c_ptr), value :: ctx
         integer(c_int), value :: nfreq
         real(c_double), intent(in) :: z(*)
         real(c_double), intent(out) :: res(*)
         integer(c_int) :: rc
      end function
      ! EOM-IP-CCSD / EOM-EA-CCSD: the same calls with a sector (AFESP_EOM_IP, AFESP_EOM_EA) behind the context (include/afesp.h)
      function afesp_ccsd_so_eom_ipea_init(ctx, sector, nroots, max_space) bind(C, name='afesp_ccsd_so_eom_ipea_init') result(rc)
         import :: c_int, c_ptr
         type(c_ptr), value :: ctx
         integer(c_int), value :: sector, nroots, max_space
         integer(c_int) :: rc
      end function
      function afesp_ccsd_so_eom_ipea_sigma(ctx, sector, nvec, r1, r2, s1, s2) bind(C, name='afesp_ccsd_so_eom_ipea_sigma') result(rc)
         import :: c_int, c_double, c_ptr
         type(c_ptr), value :: ctx
         integer(c_int), value :: sector, nvec
         real(c_double), intent(in) :: r1(*), r2(*)
         real(c_double), intent(out) :: s1(*), s2(*)
         integer(c_int) :: rc
      end function
      function afesp_ccsd_so_eom_ipea_guess(ctx, sector) bind(C, name='afesp_ccsd_so_eom_ipea_guess') result(rc)
         import :: c_int, c_ptr
         type(c_ptr), value :: ctx
         integer(c_int), value :: sector
         integer(c_int) :: rc
      end function
      function afesp_ccsd_so_eom_ipea_set_guess(ctx, sector, k, r1, r2) bind(C, name='afesp_ccsd_so_eom_ipea_set_guess') result(rc)
         import :: c_int, c_double, c_ptr
         type(c_ptr), value :: ctx
         integer(c_int), value :: sector, k
         real(c_double), intent(in) :: r1(*), r2(*)
         integer(c_int) :: rc
      end function
      function afesp_ccsd_so_eom_ipea_iterate(ctx, sector, tol, omega, resnorm, flags, nsigma, converged) &
         bind(C, name='afesp_ccsd_so_eom_ipea_iterate') result(rc)
         import :: c_int, c_double, c_ptr
         type(c_ptr), value :: ctx
         integer(c_int), value :: sector
         real(c_double), value :: tol
         real(c_double), intent(out) :: omega(*), resnorm(*)
         integer(c_int), intent(out) :: flags(*), nsigma, converged
         integer(c_int) :: rc
      end function
      function afesp_ccsd_so_eom_ipea_get_vector(ctx, sector, k, r1, r2) bind(C, name='afesp_ccsd_so_eom_ipea_get_vector') result(rc)
         import :: c_int, c_double, c_ptr
         type(c_ptr), value :: ctx
         integer(c_int), value :: sector, k
         real(c_double), intent(out) :: r1(*), r2(*)
         integer(c_int) :: rc
      end function
      ! the left-hand side of both sectors and the Dyson orbitals (include/afesp.h).  _dyson takes c_ptr arguments: c_loc of the
      ! vectors, or c_null_ptr for an absent side
      function afesp_ccsd_so_eom_ipea_lsigma(ctx, sector, nvec, l1, l2, s1, s2) bind(C, name='afesp_ccsd_so_eom_ipea_lsigma') result(rc)
         import :: c_int, c_double, c_ptr
         type(c_ptr), value :: ctx
         integer(c_int), value :: sector, nvec
         real(c_double), intent(in) :: l1(*), l2(*)
         real(c_double), intent(out) :: s1(*), s2(*)
         integer(c_int) :: rc
      end function
      function afesp_ccsd_so_eom_ipea_left_init(ctx, sector, nroots, max_space) &
         bind(C, name='afesp_ccsd_so_eom_ipea_left_init') result(rc)
         import :: c_int, c_ptr
         type(c_ptr), value :: ctx
         integer(c_int), value :: sector, nroots, max_space
         integer(c_int) :: rc
      end function
      function afesp_ccsd_so_eom_ipea_left_guess(ctx, sector) bind(C, name='afesp_ccsd_so_eom_ipea_left_guess') result(rc)
         import :: c_int, c_ptr
         type(c_ptr), value :: ctx
         integer(c_int), value :: sector
         integer(c_int) :: rc
      end function
      function afesp_ccsd_so_eom_ipea_left_set_guess(ctx, sector, k, l1, l2) &
         bind(C, name='afesp_ccsd_so_eom_ipea_left_set_guess') result(rc)
         import :: c_int, c_double, c_ptr
         type(c_ptr), value :: ctx
         integer(c_int), value :: sector, k
         real(c_double), intent(in) :: l1(*), l2(*)
         integer(c_int) :: rc
      end function
      function afesp_ccsd_so_eom_ipea_left_iterate(ctx, sector, tol, omega, resnorm, flags, nsigma, converged) &
         bind(C, name='afesp_ccsd_so_eom_ipea_left_iterate') result(rc)
         import :: c_int, c_double, c_ptr
         type(c_ptr), value :: ctx
         integer(c_int), value :: sector
         real(c_double), value :: tol
         real(c_double), intent(out) :: omega(*), resnorm(*)
         integer(c_int), intent(out) :: flags(*), nsigma, converged
         integer(c_int) :: rc
      end function
      function afesp_ccsd_so_eom_ipea_left_get_vector(ctx, sector, k, l1, l2) &
         bind(C, name='afesp_ccsd_so_eom_ipea_left_get_vector') result(rc)
         import :: c_int, c_double, c_ptr
         type(c_ptr), value :: ctx
         integer(c_int), value :: sector, k
         real(c_double), intent(out) :: l1(*), l2(*)
         integer(c_int) :: rc
      end function
      function afesp_ccsd_so_eom_ipea_dyson(ctx, sector, nvec, l1, l2, r1, r2, dl, dr) &
         bind(C, name='afesp_ccsd_so_eom_ipea_dyson') result(rc)
         import :: c_int, c_ptr
         type(c_ptr), value :: ctx
         integer(c_int), value :: sector, nvec
         type(c_ptr), value :: l1, l2, r1, r2, dl, dr
         integer(c_int) :: rc
      end function
      function afesp_eig_general(n, a, lda, wr, wi, vr) bind(C, name='afesp_eig_general') result(rc)
         import :: c_int, c_double
         integer(c_int), value :: n, lda
         real(c_double), intent(in) :: a(*)
         real(c_double), intent(out) :: wr(*), wi(*), vr(*)
         integer(c_int) :: rc
      end function
      function afesp_ccsd_so_t_ntriples(nocc) bind(C, name='afesp_ccsd_so_t_ntriples') result(n)
         import :: c_int64_t
         integer(c_int64_t), value :: nocc
         integer(c_int64_t) :: n
      end function
      !> replaces `call do_ccsd_t_spinorb(...)` (reference src/main.F90:79): e_t = E_T of src/ccsd.f90:1910
      function afesp_ccsd_so_t(ctx, t_begin, t_end, e_t) bind(C, name='afesp_ccsd_so_t') result(rc)
         import :: c_int, c_int64_t, c_double, c_ptr
         type(c_ptr), value :: ctx
         integer(c_int64_t), value :: t_begin, t_end
         real(c_double), intent(out) :: e_t
         integer(c_int) :: rc
      end function
      !> Lambda-CCSD(T): the triples [t_begin, t_end) of afesp_ccsd_so_t's list with the Lambda amplitudes in the left factor (needs a live
      !> Lambda state: status 21 otherwise)
      function afesp_ccsd_so_lambda_t(ctx, t_begin, t_end, e_lt) bind(C, name='afesp_ccsd_so_lambda_t') result(rc)
         import :: c_int, c_int64_t, c_double, c_ptr
         type(c_ptr), value :: ctx
         integer(c_int64_t), value :: t_begin, t_end
         real(c_double), intent(out) :: e_lt
         integer(c_int) :: rc
      end function
      !> The non-iterative triples correction to nstates EOM-EE-CCSD excitation energies from biorthonormal left and right vectors (laid out
      !> as t1 / t2, one state after the other) over the triples [t_begin, t_end) of afesp_ccsd_so_t's list; delta(nstates)
      function afesp_ccsd_so_eom_t(ctx, nstates, omega, l1, l2, r1, r2, t_begin, t_end, delta) bind(C, name='afesp_ccsd_so_eom_t') result(rc)
         import :: c_int, c_int64_t, c_double, c_ptr
         type(c_ptr), value :: ctx
         integer(c_int), value :: nstates
         real(c_double), intent(in) :: omega(*), l1(*), l2(*), r1(*), r2(*)
         integer(c_int64_t), value :: t_begin, t_end
         real(c_double), intent(out) :: delta(*)
         integer(c_int) :: rc
      end function
      !> the non-iterative triples correction to EOM-IP (sector 1) / EOM-EA (sector 2) roots over the items [begin, end): IP the triples
      !> i<j<k of afesp_ccsd_so_t's list, EA the pairs i<j numbered j (j - 1) / 2 + i; nstates vectors in the sector's layout one after the other
      function afesp_ccsd_so_eom_ipea_t(ctx, sector, nstates, omega, l1, l2, r1, r2, t_begin, t_end, delta) &
         bind(C, name='afesp_ccsd_so_eom_ipea_t') result(rc)
         import :: c_int, c_int64_t, c_double, c_ptr
         type(c_ptr), value :: ctx
         integer(c_int), value :: sector, nstates
         real(c_double), intent(in) :: omega(*), l1(*), l2(*), r1(*), r2(*)
         integer(c_int64_t), value :: t_begin, t_end
         real(c_double), intent(out) :: delta(*)
         integer(c_int) :: rc
      end function
      function afesp_ccsd_so_eom_ipea_t_nitems(sector, nocc) bind(C, name='afesp_ccsd_so_eom_ipea_t_nitems') result(n)
         import :: c_int, c_int64_t
         integer(c_int), value :: sector, nocc
         integer(c_int64_t) :: n
      end function
      !> a named tensor of the spin-orbital state (name NUL-terminated; 'D1': the singles denominators e_i - e_a, (o, v);
      !> 'levels': the levels of the o + v spin orbitals themselves, occupied first)
      function afesp_ccsd_so_get_tensor(ctx, name, buf, capacity) bind(C, name='afesp_ccsd_so_get_tensor') result(rc)
         import :: c_int, c_int64_t, c_double, c_ptr, c_char
         type(c_ptr), value :: ctx
         character(kind=c_char), intent(in) :: name(*)
         real(c_double), intent(out) :: buf(*)
         integer(c_int64_t), value :: capacity
         integer(c_int) :: rc
      end function
      !> ---- multi-GPU: one process per GPU; the OpenMP reduction of the reference's (T) loop (src/ccsd.f90:2091) becomes a
      !> sum over ranks
      function afesp_device_count() bind(C, name='afesp_device_count') result(n)
         import :: c_int
         integer(c_int) :: n
      end function
      function afesp_comm_init(ctx, rank, world, transport, bootstrap_path, unique_id) bind(C, name='afesp_comm_init') result(rc)
         import :: c_int, c_ptr, c_char
         type(c_ptr), value :: ctx
         integer(c_int), value :: rank, world, transport
         character(kind=c_char), intent(in) :: bootstrap_path(*)
         type(c_ptr), value :: unique_id              ! c_null_ptr: the id travels through bootstrap_path
         integer(c_int) :: rc
      end function
      function afesp_comm_destroy(ctx) bind(C, name='afesp_comm_destroy') result(rc)
         import :: c_int, c_ptr
         type(c_ptr), value :: ctx
         integer(c_int) :: rc
      end function
      function afesp_allreduce_sum(ctx, inout, n) bind(C, name='afesp_allreduce_sum') result(rc)
         import :: c_int, c_int64_t, c_double, c_ptr
         type(c_ptr), value :: ctx
         real(c_double), intent(inout) :: inout(*)
         integer(c_int64_t), value :: n
         integer(c_int) :: rc
      end function
      function afesp_ccsd_t_shard_bounds(ctx, nocc, nvirt, cr, world, bounds) bind(C, name='afesp_ccsd_t_shard_bounds') result(rc)
         import :: c_int, c_int64_t, c_ptr
         type(c_ptr), value :: ctx
         integer(c_int64_t), value :: nocc, nvirt
         integer(c_int), value :: cr, world
         integer(c_int64_t), intent(out) :: bounds(*)
         integer(c_int) :: rc
      end function
      function afesp_ccsd_t_block_size(ctx, nocc, nvirt, cr, block_size) bind(C, name='afesp_ccsd_t_block_size') result(rc)
         import :: c_int, c_int64_t, c_ptr
         type(c_ptr), value :: ctx
         integer(c_int64_t), value :: nocc, nvirt
         integer(c_int), value :: cr
         integer(c_int), intent(out) :: block_size
         integer(c_int) :: rc
      end function
   end interface

contains

   !> Copy the engine's last error message into a Fortran string.
   function afesp_error_text(ctx) result(text)
      type(c_ptr), intent(in) :: ctx
      character(len=:), allocatable :: text
      type(c_ptr) :: p
      character(kind=c_char), pointer :: chars(:)
      integer :: n
      p = afesp_last_error(ctx)
      text = ''
      if (.not. c_associated(p)) return
      call c_f_pointer(p, chars, [4096])
      n = 0
      do while (n < 4096)
         if (chars(n + 1) == c_null_char) exit
         n = n + 1
      end do
      allocate (character(len=n) :: text)
      block
         integer :: i
         do i = 1, n
            text(i:i) = chars(i)
         end do
      end block
   end function

end module afesp_capi
