!> els_amd -- Fortran host of the MI355X coupled-cluster engine.
!>
!> Keeps the reference's user surface (els.in namelist and calc_type strings: reference src/system.f90:81-167;
!> s.dat/t.dat/v.dat/eri.dat/geom.dat/guess_in.dat in the working directory: src/integrals.f90:69-73, src/geometry.f90:23,
!> src/hf.f90:153-191; the stdout energy table: src/main.F90:123-175) and hands the dense-tensor path -- AO->MO + MP2,
!> CCSD, (T) -- to libafesp_hip.so through the ISO_C_BINDING interfaces in afesp_capi.f90.  Host-side work that stays
!> here is O(n^4) at most: input parsing and restricted Hartree-Fock.
module host_support
   use, intrinsic :: iso_fortran_env, only: dp => real64, i8 => int64, out => output_unit, err => error_unit
   implicit none
contains
   !> same contract as the reference's error(): four lines on stderr, then `stop '999'`
   subroutine fail(where, why)
      character(*), intent(in) :: where, why
      write (err, '(1X, A)') 'ERROR.'
      write (err, '(1X, A)') 'Programme stops in procedure: '//trim(where)//'.'
      write (err, '(1X, A)') 'Reason: '//trim(why)//'.'
      write (err, '(1X, A)') 'EXITING...'
      error stop '999'   ! the reference uses a plain STOP (exit status 0); a failing run should fail its caller
   end subroutine
   function seconds() result(t)
      real(dp) :: t
      integer(i8) :: c, r
      call system_clock(c, r)
      t = real(c, dp)/real(r, dp)
   end function
end module host_support

module host_config
   use host_support
   implicit none
   integer, parameter :: LEVEL_RHF = 0, LEVEL_MP2 = 1, LEVEL_CCSD = 2, LEVEL_CCSD_T = 3
   type run_config
      character(40) :: calc_type = 'CCSD(T)_spatial'
      real(dp) :: scf_e_tol = 1e-6_dp, scf_d_tol = 1e-6_dp, ccsd_e_tol = 1e-6_dp, ccsd_t_tol = 1e-6_dp
      integer :: scf_diis_n_errmat = 6, ccsd_diis_n_errmat = 8, scf_maxiter = 50, ccsd_maxiter = 50
      logical :: write_fcidump = .false., scf_read_guess = .false., scf_write_guess = .false.
      logical :: fcidump_active = .false.   ! the space the solvers run in as a standard FCIDUMP (header, frozen-core operator, core energy)
      logical :: fcidump_in = .false.       ! MO integrals from ./FCIDUMP: no s.dat / t.dat / v.dat / eri.dat / geom.dat, no SCF, no transform
      integer :: level = LEVEL_CCSD_T
      logical :: paren = .false., renorm = .false., comp_renorm = .false.
      logical :: spinorb = .false.   ! the _spinorb calculation types (reference src/system.f90:117-137)
      logical :: uhf = .false.       ! the open-shell types UHF_scf, UMP2, UCCSD, UCCSD(T) (canonical UHF orbitals)
      logical :: rohf = .false.      ! ROHF-MP2, ROHF-CCSD, ROHF-CCSD(T): a restricted open-shell determinant from a FCIDUMP (uhf is set too:
                                     ! semicanonical orbitals differ by spin, the open-shell branch runs them with the full Fock matrices)
      integer :: charge = 0, multiplicity = 1
      ! active orbital window of the correlated steps (no counterpart in the reference); all three absent: every orbital correlated
      logical :: frozen_core = .false.   ! freeze the noble-gas cores counted from geom.dat
      integer :: n_frozen_core = -1      ! explicit number of lowest MOs to freeze (-1: not given); wins over frozen_core
      integer :: n_frozen_virt = 0       ! highest MOs dropped
      ! frozen natural orbitals: the virtual space truncated in the basis of the MP2 natural virtuals; at most one of the two keys
      integer :: fno_n_virt = -1         ! number of natural virtuals kept (-1: off)
      real(dp) :: fno_occ_tol = 0.0_dp   ! keep every natural virtual whose occupation is at least this (0: off)
      ! after a converged spin-orbital CCSD: the Lambda equations and the natural occupation numbers of the unrelaxed one-particle density
      logical :: cc_density = .false.
      ! after a converged spin-orbital CCSD: the Lambda equations and the triples correction with the left-hand state in its left factor
      logical :: cc_lambda_t = .false.
      ! after a converged spin-orbital CCSD: the Lambda equations, the two-particle density, the density-side energy and <S^2>
      logical :: cc_rdm2 = .false.
      ! ... the Lambda equations, the two-particle density, the Z-vector equations and the orbital-relaxed one-particle density
      logical :: cc_relaxed = .false.
      ! after a converged spin-orbital CCSD: this many EOM-EE-CCSD excitation energies (0: off)
      integer :: eom_nroots = 0
      ! ... and their left eigenvectors, from the right ones as guess (needs eom_nroots > 0)
      logical :: eom_left = .false.
      ! ... and the non-iterative triples correction to every root from its left and right vector (needs eom_left)
      logical :: eom_triples = .false.
      ! ... this many EOM-IP-CCSD ionisation potentials / EOM-EA-CCSD electron affinities (0: off)
      integer :: eom_ip_nroots = 0, eom_ea_nroots = 0
      ! ... and the left eigenvectors and pole strengths of those roots (needs one of the two > 0)
      logical :: eom_ipea_left = .false.
      ! ... and the non-iterative triples correction to those roots from their left and right vectors (needs eom_ipea_left)
      logical :: eom_ipea_triples = .false.
      ! after a converged spin-orbital CCSD: the EOM-CCSD polarisability alpha(omega) of the operators in dipx.dat / dipy.dat / dipz.dat
      ! (AO basis, the format of t.dat) at the n_polar_omega real frequencies polar_omega (default: the static one)
      logical :: cc_polar = .false.
      real(dp) :: polar_omega(8) = 0.0_dp
      integer :: n_polar_omega = 1
      ! ... polar_gamma > 0: every polar_omega is solved at omega + i polar_gamma (DESIGN.md 4.20) and the table gains Re / Im of the mean
      ! and the absorption cross-section; polar_c6_npts > 0: the mean at i u_k on that many Casimir-Polder grid points and the
      ! homo-dimer C6.  Both at their defaults: the path above, untouched.
      real(dp) :: polar_gamma = 0.0_dp
      integer :: polar_c6_npts = 0
   end type
contains
   !> &elsinput namelist; keys that are absent keep the defaults above (the reference leaves them undefined).
   subroutine read_config(cfg)
      type(run_config), intent(out) :: cfg
      character(40) :: calc_type
      real(dp) :: scf_e_tol, scf_d_tol, ccsd_e_tol, ccsd_t_tol
      integer :: scf_diis_n_errmat, ccsd_diis_n_errmat, scf_maxiter, ccsd_maxiter, unit, ios, charge, multiplicity
      integer :: n_frozen_core, n_frozen_virt, fno_n_virt, eom_nroots, eom_ip_nroots, eom_ea_nroots
      real(dp) :: fno_occ_tol
      logical :: write_fcidump, scf_read_guess, scf_write_guess, there, frozen_core, fcidump_active, fcidump_in, cc_density, cc_lambda_t
      logical :: eom_left, eom_triples, cc_rdm2, cc_relaxed, cc_polar, eom_ipea_left, eom_ipea_triples
      real(dp) :: polar_omega(8), polar_gamma
      integer :: polar_c6_npts
      real(dp), parameter :: omega_unset = huge(1.0_dp)
      namelist /elsinput/ calc_type, scf_e_tol, scf_d_tol, scf_diis_n_errmat, ccsd_e_tol, ccsd_t_tol, &
         ccsd_diis_n_errmat, scf_maxiter, ccsd_maxiter, write_fcidump, scf_read_guess, scf_write_guess, charge, multiplicity, &
         frozen_core, n_frozen_core, n_frozen_virt, fno_n_virt, fno_occ_tol, fcidump_active, fcidump_in, &
         cc_density, cc_lambda_t, eom_nroots, eom_ip_nroots, eom_ea_nroots, eom_left, eom_triples, eom_ipea_left, eom_ipea_triples, cc_rdm2, cc_relaxed, &
         cc_polar, polar_omega, polar_gamma, polar_c6_npts
      type(run_config) :: d
      calc_type = d%calc_type; scf_e_tol = d%scf_e_tol; scf_d_tol = d%scf_d_tol; ccsd_e_tol = d%ccsd_e_tol
      ccsd_t_tol = d%ccsd_t_tol; scf_diis_n_errmat = d%scf_diis_n_errmat; ccsd_diis_n_errmat = d%ccsd_diis_n_errmat
      scf_maxiter = d%scf_maxiter; ccsd_maxiter = d%ccsd_maxiter; write_fcidump = d%write_fcidump
      scf_read_guess = d%scf_read_guess; scf_write_guess = d%scf_write_guess
      charge = d%charge; multiplicity = d%multiplicity
      frozen_core = d%frozen_core; n_frozen_core = d%n_frozen_core; n_frozen_virt = d%n_frozen_virt
      fno_n_virt = d%fno_n_virt; fno_occ_tol = d%fno_occ_tol; fcidump_active = d%fcidump_active
      fcidump_in = d%fcidump_in; cc_density = d%cc_density; eom_nroots = d%eom_nroots
      cc_lambda_t = d%cc_lambda_t; cc_rdm2 = d%cc_rdm2; cc_relaxed = d%cc_relaxed
      eom_ip_nroots = d%eom_ip_nroots; eom_ea_nroots = d%eom_ea_nroots; eom_left = d%eom_left; eom_triples = d%eom_triples
      eom_ipea_left = d%eom_ipea_left; eom_ipea_triples = d%eom_ipea_triples
      cc_polar = d%cc_polar; polar_omega = omega_unset
      polar_gamma = d%polar_gamma; polar_c6_npts = d%polar_c6_npts
      inquire (file='els.in', exist=there)
      if (.not. there) call fail('system::read_system_in', 'input file els.in does not exist')
      open (newunit=unit, file='els.in', action='read', status='old')
      read (unit, nml=elsinput, iostat=ios)
      close (unit)
      if (ios /= 0) call fail('system::read_system_in', 'invalid input file format!')
      cfg%calc_type = calc_type; cfg%scf_e_tol = scf_e_tol; cfg%scf_d_tol = scf_d_tol; cfg%ccsd_e_tol = ccsd_e_tol
      cfg%ccsd_t_tol = ccsd_t_tol; cfg%scf_diis_n_errmat = scf_diis_n_errmat; cfg%ccsd_diis_n_errmat = ccsd_diis_n_errmat
      cfg%scf_maxiter = scf_maxiter; cfg%ccsd_maxiter = ccsd_maxiter; cfg%write_fcidump = write_fcidump
      cfg%scf_read_guess = scf_read_guess; cfg%scf_write_guess = scf_write_guess
      cfg%charge = charge; cfg%multiplicity = multiplicity
      cfg%frozen_core = frozen_core; cfg%n_frozen_core = n_frozen_core; cfg%n_frozen_virt = max(n_frozen_virt, 0)
      if (n_frozen_core < -1 .or. n_frozen_virt < -1) &
         call fail('system::read_system_in', 'n_frozen_core and n_frozen_virt must be non-negative integers!')
      cfg%fno_n_virt = fno_n_virt; cfg%fno_occ_tol = fno_occ_tol
      cfg%fcidump_active = fcidump_active
      if (fcidump_active .and. write_fcidump) &
         call fail('system::read_system_in', 'write_fcidump and fcidump_active both write FCIDUMP: choose one')
      if (fno_n_virt < -1) call fail('system::read_system_in', 'fno_n_virt must be a non-negative integer!')
      if (fno_occ_tol < 0.0_dp) call fail('system::read_system_in', 'fno_occ_tol must be a non-negative number!')
      if (fno_n_virt >= 0 .and. fno_occ_tol > 0.0_dp) &
         call fail('system::read_system_in', 'fno_n_virt and fno_occ_tol exclude each other!')
      if ((fno_n_virt >= 0 .or. fno_occ_tol > 0.0_dp) .and. n_frozen_virt > 0) &
         call fail('system::read_system_in', 'frozen natural orbitals and n_frozen_virt exclude each other!')
      select case (trim(calc_type))
      case ('RHF');              cfg%level = LEVEL_RHF
      case ('MP2_spatial');      cfg%level = LEVEL_MP2
      case ('CCSD_spatial');     cfg%level = LEVEL_CCSD
      case ('CCSD(T)_spatial');  cfg%level = LEVEL_CCSD_T; cfg%paren = .true.
      case ('CCSD[T]_spatial');  cfg%level = LEVEL_CCSD_T
      case ('RCCSD(T)_spatial'); cfg%level = LEVEL_CCSD_T; cfg%paren = .true.; cfg%renorm = .true.
      case ('RCCSD[T]_spatial'); cfg%level = LEVEL_CCSD_T; cfg%renorm = .true.
      case ('CRCCSD(T)_spatial'); cfg%level = LEVEL_CCSD_T; cfg%paren = .true.; cfg%comp_renorm = .true.
      case ('CRCCSD[T]_spatial'); cfg%level = LEVEL_CCSD_T; cfg%comp_renorm = .true.
      ! the reference runs its restricted SCF and the spin-free MP2 for these as well (src/main.F90:49-64)
      case ('UHF');              cfg%level = LEVEL_RHF; cfg%spinorb = .true.
      case ('MP2_spinorb');      cfg%level = LEVEL_MP2; cfg%spinorb = .true.
      case ('CCSD_spinorb');     cfg%level = LEVEL_CCSD; cfg%spinorb = .true.
      case ('CCSD(T)_spinorb');  cfg%level = LEVEL_CCSD_T; cfg%spinorb = .true.
      ! open-shell types: unrestricted SCF, then the spin-orbital path on its orbitals
      case ('UHF_scf');          cfg%level = LEVEL_RHF; cfg%uhf = .true.
      case ('UMP2');             cfg%level = LEVEL_MP2; cfg%uhf = .true.
      case ('UCCSD');            cfg%level = LEVEL_CCSD; cfg%uhf = .true.
      case ('UCCSD(T)');         cfg%level = LEVEL_CCSD_T; cfg%uhf = .true.
      ! restricted open-shell references: orbitals from a restricted FCIDUMP with MS2 >= 0, no SCF
      case ('ROHF-MP2');         cfg%level = LEVEL_MP2; cfg%uhf = .true.; cfg%rohf = .true.
      case ('ROHF-CCSD');        cfg%level = LEVEL_CCSD; cfg%uhf = .true.; cfg%rohf = .true.
      case ('ROHF-CCSD(T)');     cfg%level = LEVEL_CCSD_T; cfg%uhf = .true.; cfg%rohf = .true.
      case default
         call fail('system::read_system_in', 'Unrecognised calculation type!')
      end select
      if (multiplicity < 1) call fail('system::read_system_in', 'invalid input file format!')
      cfg%fcidump_in = fcidump_in
      cfg%cc_density = cc_density
      if (cc_density .and. .not. (cfg%level >= LEVEL_CCSD .and. (cfg%spinorb .or. cfg%uhf))) call fail('system::read_system_in', &
         trim(calc_type)//' takes no cc_density: the Lambda equations run on the spin-orbital CCSD types!')
      if (cc_density .and. fcidump_in .and. cfg%uhf .and. .not. cfg%rohf) call fail('system::read_system_in', &
         'cc_density on a UHF FCIDUMP: the file does not hold the overlap of its alpha and beta orbitals, which the spin-summed density needs!')
      cfg%cc_rdm2 = cc_rdm2
      if (cc_rdm2 .and. .not. (cfg%level >= LEVEL_CCSD .and. (cfg%spinorb .or. cfg%uhf))) call fail('system::read_system_in', &
         trim(calc_type)//' takes no cc_rdm2: the Lambda equations run on the spin-orbital CCSD types!')
      if (cc_rdm2 .and. fcidump_in .and. cfg%uhf .and. .not. cfg%rohf) call fail('system::read_system_in', &
         'cc_rdm2 on a UHF FCIDUMP: the file does not hold the overlap of its alpha and beta orbitals, which <S^2> needs!')
      cfg%cc_relaxed = cc_relaxed
      if (cc_relaxed .and. (cfg%rohf .or. .not. (cfg%level >= LEVEL_CCSD .and. (cfg%spinorb .or. cfg%uhf)))) &
         call fail('system::read_system_in', trim(calc_type)//' takes no cc_relaxed: the Z-vector equations run on the spin-orbital CCSD '// &
                   'types with a Hartree-Fock reference!')
      if (cc_relaxed .and. fcidump_in .and. cfg%uhf) call fail('system::read_system_in', &
         'cc_relaxed on a UHF FCIDUMP: the file does not hold the overlap of its alpha and beta orbitals, which the spin-summed density needs!')
      if (cc_relaxed .and. (frozen_core .or. n_frozen_core > 0 .or. n_frozen_virt > 0 .or. fno_n_virt >= 0 .or. fno_occ_tol > 0.0_dp)) &
         call fail('system::read_system_in', 'cc_relaxed with a frozen-core / frozen-virtual window or frozen natural orbitals: the windowed '// &
                   'state lacks the core-active integrals that orbital relaxation needs!')
      ! (Lambda-(T) needs no overlap of the alpha and beta orbitals: a UHF FCIDUMP takes it)
      cfg%cc_lambda_t = cc_lambda_t
      if (cc_lambda_t .and. .not. (cfg%level >= LEVEL_CCSD .and. (cfg%spinorb .or. cfg%uhf))) call fail('system::read_system_in', &
         trim(calc_type)//' takes no cc_lambda_t: the Lambda equations run on the spin-orbital CCSD types!')
      cfg%eom_nroots = eom_nroots
      if (eom_nroots < 0) call fail('system::read_system_in', 'eom_nroots must be a non-negative integer!')
      if (eom_nroots > 0 .and. .not. (cfg%level >= LEVEL_CCSD .and. (cfg%spinorb .or. cfg%uhf))) call fail('system::read_system_in', &
         trim(calc_type)//' takes no eom_nroots: the EOM-CCSD equations run on the spin-orbital CCSD types!')
      cfg%eom_left = eom_left
      if (eom_left .and. eom_nroots == 0) call fail('system::read_system_in', &
         'eom_left needs eom_nroots > 0: the left eigenvectors are those of the EOM-EE-CCSD roots it asks for!')
      cfg%eom_triples = eom_triples
      if (eom_triples .and. .not. (eom_nroots > 0 .and. eom_left)) call fail('system::read_system_in', &
         'eom_triples needs eom_nroots > 0 and eom_left: the triples correction contracts the left and right vectors of '// &
         'the EOM-EE-CCSD roots!')
      cfg%cc_polar = cc_polar
      if (cc_polar .and. .not. (cfg%level >= LEVEL_CCSD .and. (cfg%spinorb .or. cfg%uhf))) call fail('system::read_system_in', &
         trim(calc_type)//' takes no cc_polar: the response equations run on the spin-orbital CCSD types!')
      if (cc_polar .and. fcidump_in) call fail('system::read_system_in', &
         'cc_polar with fcidump_in: the operator files dipx.dat / dipy.dat / dipz.dat are in the AO basis, which a FCIDUMP run does not have!')
      if (cc_polar) then   ! (an input error before anything runs; polarizability_report reads them after CCSD)
         inquire (file='dipx.dat', exist=there)
         if (.not. there) call fail('system::read_system_in', 'cc_polar: the operator file dipx.dat does not exist!')
         inquire (file='dipy.dat', exist=there)
         if (.not. there) call fail('system::read_system_in', 'cc_polar: the operator file dipy.dat does not exist!')
         inquire (file='dipz.dat', exist=there)
         if (.not. there) call fail('system::read_system_in', 'cc_polar: the operator file dipz.dat does not exist!')
      end if
      cfg%n_polar_omega = count(polar_omega /= omega_unset)   ! (the values given, from the front)
      if (cfg%n_polar_omega > 0) then
         if (any(polar_omega(:cfg%n_polar_omega) == omega_unset)) call fail('system::read_system_in', 'invalid input file format!')
         cfg%polar_omega(:cfg%n_polar_omega) = polar_omega(:cfg%n_polar_omega)
      else
         cfg%n_polar_omega = 1
      end if
      if (.not. polar_gamma >= 0.0_dp) call fail('system::read_system_in', 'polar_gamma is a damping in Eh, zero (real frequencies) or positive!')
      if (polar_c6_npts < 0 .or. polar_c6_npts > 21) call fail('system::read_system_in', &
         'polar_c6_npts is the number of Casimir-Polder grid points, 0 (off) to 21 (three operators each, 64 systems in one response state)!')
      cfg%polar_gamma = polar_gamma; cfg%polar_c6_npts = polar_c6_npts
      cfg%eom_ip_nroots = eom_ip_nroots; cfg%eom_ea_nroots = eom_ea_nroots
      if (eom_ip_nroots < 0) call fail('system::read_system_in', 'eom_ip_nroots must be a non-negative integer!')
      if (eom_ea_nroots < 0) call fail('system::read_system_in', 'eom_ea_nroots must be a non-negative integer!')
      if (eom_ip_nroots > 0 .and. .not. (cfg%level >= LEVEL_CCSD .and. (cfg%spinorb .or. cfg%uhf))) call fail('system::read_system_in', &
         trim(calc_type)//' takes no eom_ip_nroots: the EOM-CCSD equations run on the spin-orbital CCSD types!')
      if (eom_ea_nroots > 0 .and. .not. (cfg%level >= LEVEL_CCSD .and. (cfg%spinorb .or. cfg%uhf))) call fail('system::read_system_in', &
         trim(calc_type)//' takes no eom_ea_nroots: the EOM-CCSD equations run on the spin-orbital CCSD types!')
      cfg%eom_ipea_left = eom_ipea_left
      if (eom_ipea_left .and. eom_ip_nroots == 0 .and. eom_ea_nroots == 0) call fail('system::read_system_in', &
         'eom_ipea_left needs eom_ip_nroots > 0 or eom_ea_nroots > 0: the left eigenvectors and pole strengths are those of '// &
         'the EOM-IP-CCSD / EOM-EA-CCSD roots they ask for!')
      cfg%eom_ipea_triples = eom_ipea_triples
      if (eom_ipea_triples .and. .not. (eom_ipea_left .and. (eom_ip_nroots > 0 .or. eom_ea_nroots > 0))) call fail('system::read_system_in', &
         'eom_ipea_triples needs eom_ipea_left and eom_ip_nroots > 0 or eom_ea_nroots > 0: the triples correction contracts '// &
         'the left and right vectors of the EOM-IP-CCSD / EOM-EA-CCSD roots!')
      if (cfg%rohf) then   ! no ROHF SCF here: the orbitals come from a file, and a frozen core reaches this path as an active-space file
         if (.not. fcidump_in) call fail('system::read_system_in', trim(calc_type)// &
            ' needs fcidump_in = .true.: there is no ROHF SCF, the restricted open-shell orbitals come from a FCIDUMP!')
         if (frozen_core .or. n_frozen_core >= 0 .or. n_frozen_virt > 0) call fail('system::read_system_in', trim(calc_type)// &
            ' takes no frozen_core / n_frozen_core / n_frozen_virt: freeze the core in the file (an active-space FCIDUMP carries the core operator)!')
         if (fno_n_virt >= 0 .or. fno_occ_tol > 0.0_dp) call fail('system::read_system_in', trim(calc_type)// &
            ' takes no frozen natural orbitals (fno_n_virt / fno_occ_tol)!')
         if (fcidump_active) call fail('system::read_system_in', trim(calc_type)//' takes no fcidump_active!')
      end if
      if (fcidump_in) then   ! the file replaces everything up to the MO integrals: what needs AO data or writes the same file is refused
         if (frozen_core) call fail('system::read_system_in', &
            'fcidump_in: frozen_core counts atoms in geom.dat, which is not read: give n_frozen_core!')
         if (fno_n_virt >= 0 .or. fno_occ_tol > 0.0_dp) call fail('system::read_system_in', &
            'fcidump_in: frozen natural orbitals need the AO integrals, which are not read!')
         if (write_fcidump .or. fcidump_active) call fail('system::read_system_in', &
            'fcidump_in reads FCIDUMP: write_fcidump / fcidump_active would overwrite it!')
         if (scf_read_guess .or. scf_write_guess) call fail('system::read_system_in', &
            'fcidump_in runs no SCF: scf_read_guess / scf_write_guess have nothing to act on!')
         if (cfg%level == LEVEL_RHF) call fail('system::read_system_in', 'fcidump_in runs no SCF: choose a correlated calculation type!')
      end if
      if (.not. cfg%uhf .and. (charge /= 0 .or. multiplicity /= 1)) &
         call fail('system::read_system_in', 'charge and multiplicity need an open-shell calculation type!')
   end subroutine
end module host_config

module host_inputs
   use host_support
   implicit none
   type molecule
      integer :: nbasis = 0, natoms = 0, nel = 0, nocc = 0, nvirt = 0
      integer :: ncore = 0   ! doubly occupied noble-gas core orbitals of the atoms (-1: an atom beyond Kr, no count)
      real(dp) :: e_nuc = 0.0_dp
      real(dp), allocatable :: ovlp(:, :), hcore(:, :), eri(:)
      real(dp), allocatable :: ke(:, :), en(:, :)   ! t.dat and v.dat, the two parts of hcore (absent when the integrals come from a FCIDUMP)
   end type
contains
   pure function pair(i, j) result(ij)     ! 1-based lower-triangle index
      integer, intent(in) :: i, j
      integer(i8) :: ij, a, b
      a = max(i, j); b = min(i, j)
      ij = a*(a - 1)/2 + b
   end function
   pure function eri_slot(i, j, k, l) result(ijkl)
      integer, intent(in) :: i, j, k, l
      integer(i8) :: ijkl, ij, kl, a, b
      ij = pair(i, j); kl = pair(k, l)
      a = max(ij, kl); b = min(ij, kl)
      ijkl = a*(a - 1)/2 + b
   end function

   subroutine read_two_index(file, mat, n)
      character(*), intent(in) :: file
      real(dp), allocatable, intent(inout) :: mat(:, :)
      integer, intent(inout) :: n
      integer :: unit, ios, i, j
      real(dp) :: x
      if (n == 0) then    ! first pass: the largest index is the number of basis functions
         open (newunit=unit, file=file, status='old', action='read')
         do
            read (unit, *, iostat=ios) i, j, x
            if (ios /= 0) exit
            n = max(n, i, j)
         end do
         close (unit)
      end if
      allocate (mat(n, n)); mat = 0.0_dp
      open (newunit=unit, file=file, status='old', action='read')
      do
         read (unit, *, iostat=ios) i, j, x
         if (ios /= 0) exit
         mat(i, j) = x; mat(j, i) = x
      end do
      close (unit)
   end subroutine

   !> engine_reads_eri: leave mol%eri allocated and zero -- the caller fills it with afesp_read_eri_text, which also
   !> leaves the packed AO integrals on the device (reference loop: src/integrals.f90:146-161)
   subroutine read_molecule(mol, engine_reads_eri)
      type(molecule), intent(out) :: mol
      logical, intent(in) :: engine_reads_eri
      real(dp), allocatable :: xyz(:, :)
      integer, allocatable :: z(:)
      integer :: unit, ios, i, j, k, l, a
      integer(i8) :: npair, neri
      real(dp) :: x, charge
      write (out, '(1X, 16("-"))'); write (out, '(1X, A)') 'Integral read-in'; write (out, '(1X, 16("-"))')
      call read_two_index('s.dat', mol%ovlp, mol%nbasis)
      call read_two_index('t.dat', mol%ke, mol%nbasis)
      call read_two_index('v.dat', mol%en, mol%nbasis)
      allocate (mol%hcore(mol%nbasis, mol%nbasis)); mol%hcore = mol%ke + mol%en
      npair = int(mol%nbasis, i8)*(mol%nbasis + 1)/2
      neri = npair*(npair + 1)/2
      allocate (mol%eri(neri)); mol%eri = 0.0_dp
      if (.not. engine_reads_eri) then
         open (newunit=unit, file='eri.dat', status='old', action='read')
         do
            read (unit, *, iostat=ios) i, j, k, l, x
            if (ios /= 0) exit
            mol%eri(eri_slot(i, j, k, l)) = x
         end do
         close (unit)
         write (out, *) 'Done reading integrals!'
      end if
      open (newunit=unit, file='geom.dat', status='old', action='read')
      read (unit, *) mol%natoms
      allocate (z(mol%natoms), xyz(3, mol%natoms))
      do a = 1, mol%natoms
         read (unit, *) charge, xyz(:, a)
         z(a) = int(charge)
      end do
      close (unit)
      mol%nel = sum(z); mol%nocc = mol%nel/2; mol%nvirt = mol%nbasis - mol%nocc
      mol%ncore = 0      ! the core below each atom's valence shell: He for Z <= 10, Ne for Z <= 18, Ar for Z <= 36
      do a = 1, mol%natoms
         if (z(a) > 36 .or. mol%ncore < 0) then
            mol%ncore = -1
         else if (z(a) > 18) then
            mol%ncore = mol%ncore + 9
         else if (z(a) > 10) then
            mol%ncore = mol%ncore + 5
         else if (z(a) > 2) then
            mol%ncore = mol%ncore + 1
         end if
      end do
      mol%e_nuc = 0.0_dp
      do j = 2, mol%natoms
         do i = 1, j - 1
            mol%e_nuc = mol%e_nuc + z(i)*z(j)/norm2(xyz(:, i) - xyz(:, j))
         end do
      end do
   end subroutine
end module host_inputs

module host_linalg
   use host_support
   implicit none
contains
   !> Cyclic Jacobi eigensolver for a real symmetric matrix: A = V diag(w) V^T, w ascending.
   subroutine sym_eig(a_in, w, v)
      real(dp), intent(in) :: a_in(:, :)
      real(dp), intent(out) :: w(:), v(:, :)
      real(dp), allocatable :: a(:, :), col(:)
      real(dp) :: off, theta, t, c, s, apq, app, aqq, tmp
      integer :: n, p, q, k, sweep, imin
      n = size(a_in, 1)
      allocate (a(n, n), col(n)); a = a_in
      v = 0.0_dp
      do p = 1, n; v(p, p) = 1.0_dp; end do
      do sweep = 1, 100
         off = 0.0_dp
         do q = 2, n; do p = 1, q - 1; off = off + a(p, q)**2; end do; end do
         if (off < 1e-30_dp) exit
         do q = 2, n
            do p = 1, q - 1
               apq = a(p, q)
               if (abs(apq) < 1e-300_dp) cycle
               app = a(p, p); aqq = a(q, q)
               theta = (aqq - app)/(2.0_dp*apq)
               t = sign(1.0_dp, theta)/(abs(theta) + sqrt(theta*theta + 1.0_dp))
               c = 1.0_dp/sqrt(t*t + 1.0_dp); s = t*c
               do k = 1, n
                  tmp = a(k, p); a(k, p) = c*tmp - s*a(k, q); a(k, q) = s*tmp + c*a(k, q)
               end do
               do k = 1, n
                  tmp = a(p, k); a(p, k) = c*tmp - s*a(q, k); a(q, k) = s*tmp + c*a(q, k)
               end do
               do k = 1, n
                  tmp = v(k, p); v(k, p) = c*tmp - s*v(k, q); v(k, q) = s*tmp + c*v(k, q)
               end do
            end do
         end do
      end do
      do p = 1, n; w(p) = a(p, p); end do
      do p = 1, n - 1          ! selection sort, ascending
         imin = p - 1 + minloc(w(p:n), 1)
         if (imin /= p) then
            tmp = w(p); w(p) = w(imin); w(imin) = tmp
            col = v(:, p); v(:, p) = v(:, imin); v(:, imin) = col
         end if
      end do
   end subroutine

   !> Dense solve A x = b (A symmetric, full storage), Gaussian elimination with partial pivoting.
   subroutine solve(a, b, info)
      real(dp), intent(inout) :: a(:, :), b(:)
      integer, intent(out) :: info
      integer :: n, k, i, p
      real(dp) :: f
      real(dp), allocatable :: row(:)
      n = size(b); info = 0
      allocate (row(n))
      do k = 1, n
         p = k - 1 + maxloc(abs(a(k:n, k)), 1)
         if (a(p, k) == 0.0_dp) then; info = k; return; end if
         if (p /= k) then
            row = a(k, :); a(k, :) = a(p, :); a(p, :) = row
            f = b(k); b(k) = b(p); b(p) = f
         end if
         do i = k + 1, n
            f = a(i, k)/a(k, k)
            a(i, k:n) = a(i, k:n) - f*a(k, k:n)
            b(i) = b(i) - f*b(k)
         end do
      end do
      do k = n, 1, -1
         b(k) = (b(k) - dot_product(a(k, k + 1:n), b(k + 1:n)))/a(k, k)
      end do
   end subroutine
end module host_linalg

!> Frozen natural orbitals, host side (afesp_amd/fno.py is the same algebra in numpy): eigenvectors of the virtual-virtual MP2 density the
!> engine returns, the cut, and the rotation of the virtual block of the coefficients with the kept and the discarded natural virtuals
!> made canonical among themselves.  v x v work: the Jacobi solver of host_linalg serves.
module host_fno
   use host_support
   use host_linalg
   implicit none
   real(dp), parameter :: fno_degenerate_rtol = 1e-8_dp
contains
   !> D = U diag(occ) U^T, occupations in descending order
   subroutine fno_occupations(d, occ, u)
      real(dp), intent(in) :: d(:, :)
      real(dp), allocatable, intent(out) :: occ(:), u(:, :)
      real(dp), allocatable :: w(:), vec(:, :)
      integer :: v, k
      v = size(d, 1)
      allocate (occ(v), u(v, v), w(v), vec(v, v))
      if (v == 0) return
      call sym_eig(d, w, vec)
      do k = 1, v
         occ(k) = w(v + 1 - k); u(:, k) = vec(:, v + 1 - k)
      end do
   end subroutine
   !> the smallest count >= n_keep that does not split a set of occupations agreeing to a relative 1e-8
   pure function fno_widen(occ, n_keep) result(k)
      real(dp), intent(in) :: occ(:)
      integer, intent(in) :: n_keep
      integer :: k
      k = n_keep
      do while (k > 0 .and. k < size(occ))
         if (abs(occ(k) - occ(k + 1)) > fno_degenerate_rtol*max(abs(occ(k)), abs(occ(k + 1)))) exit
         k = k + 1
      end do
   end function
   !> the virtual rows of coeff (MO x AO) become [kept ; discarded] natural virtuals, each block canonical within itself: the projection
   !> of the (diagonal) virtual Fock matrix on the block is diagonalised, which gives the block's levels and a rotation
   subroutine fno_rotate(coeff, levels, nocc, u, n_keep)
      real(dp), intent(inout) :: coeff(:, :), levels(:)
      integer, intent(in) :: nocc, n_keep
      real(dp), intent(in) :: u(:, :)
      real(dp), allocatable :: cv(:, :), ev(:), ub(:, :), x(:, :), f(:, :), e(:), r(:, :)
      integer :: n, v, blk, lo, hi, m, k
      n = size(coeff, 1); v = size(u, 1)
      allocate (cv(v, size(coeff, 2)), ev(v))
      cv = coeff(nocc + 1:n, :); ev = levels(nocc + 1:n)
      do blk = 1, 2
         lo = merge(1, n_keep + 1, blk == 1); hi = merge(n_keep, v, blk == 1)
         m = hi - lo + 1
         if (m <= 0) cycle
         allocate (ub(v, m), x(v, m), f(m, m), e(m), r(m, m))
         ub = u(:, lo:hi)
         do k = 1, m; x(:, k) = ev*ub(:, k); end do
         f = matmul(transpose(ub), x)
         f = 0.5_dp*(f + transpose(f))
         call sym_eig(f, e, r)
         coeff(nocc + lo:nocc + hi, :) = matmul(transpose(matmul(ub, r)), cv)
         levels(nocc + lo:nocc + hi) = e
         deallocate (ub, x, f, e, r)
      end do
   end subroutine
end module host_fno

module host_scf
   use, intrinsic :: iso_c_binding
   use host_support
   use host_config
   use host_inputs
   use host_linalg
   use afesp_capi
   implicit none
contains
   !> Restricted Hartree-Fock with the reference's iteration (src/hf.f90:21-151): symmetric orthogonalisation, Fock
   !> guess = H_core or guess_in.dat, DIIS on FDS-SDF from the second stored matrix on, convergence on |dD| and |dE|.
   !> Returns canon_coeff(MO, AO) and canon_levels.
   !> on_device: the O(n^4) Fock build (src/hf.f90:349-385) runs on the engine, from the packed AO integrals it read.
   subroutine rhf(cfg, mol, e_hf, coeff, levels, converged, ctx, on_device)
      type(run_config), intent(in) :: cfg
      type(molecule), intent(in) :: mol
      type(c_ptr), intent(in) :: ctx
      logical, intent(in) :: on_device
      real(dp), intent(out) :: e_hf
      real(dp), allocatable, intent(out) :: coeff(:, :), levels(:)
      logical, intent(out) :: converged
      integer :: n, nocc, iter, i, j, k, l, slot, nact, m, unit, ios, info
      real(dp), allocatable :: x(:, :), fock(:, :), fprime(:, :), vec(:, :), w(:), dens(:, :), dold(:, :), sv(:), u(:, :)
      real(dp), allocatable :: fhist(:, :, :), ehist(:, :, :), bmat(:, :), rhs(:)
      real(dp) :: energy, eold, rms, val, t0, t1
      n = mol%nbasis; nocc = mol%nocc
      write (out, '(1X, 23("-"))'); write (out, '(1X, A)') 'Restricted Hartree-Fock'; write (out, '(1X, 23("-"))')
      allocate (x(n, n), fock(n, n), fprime(n, n), vec(n, n), w(n), dens(n, n), dold(n, n), sv(n), u(n, n))
      allocate (coeff(n, n), levels(n))
      call sym_eig(mol%ovlp, sv, u)
      do j = 1, n; vec(:, j) = u(:, j)/sqrt(sv(j)); end do
      x = matmul(vec, transpose(u))                       ! S^-1/2
      fock = mol%hcore
      if (cfg%scf_read_guess) then
         write (out, *) 'Reading previous AO Fock matrix as guess...'
         open (newunit=unit, file='guess_in.dat', status='old', action='read')
         do
            read (unit, *, iostat=ios) i, j, val
            if (ios /= 0) exit
            fock(i, j) = val
         end do
         close (unit)
      end if
      m = cfg%scf_diis_n_errmat
      if (m >= 2) then
         allocate (fhist(n, n, m), ehist(n, n, m)); fhist = 0.0_dp; ehist = 0.0_dp
      end if
      slot = 0; nact = 0; energy = 0.0_dp; dold = 0.0_dp; converged = .false.
      write (out, '(75("-"))')
      write (out, '(1X, A, 3X, A, 3X, A, 3X, A, 3X, A)') 'Iteration', '     Energy    ', '    deltaE     ', '   delta RMS D ', '  Time  '
      write (out, '(75("-"))')
      t0 = seconds()
      do iter = 1, cfg%scf_maxiter
         fprime = matmul(transpose(x), matmul(fock, x))
         call sym_eig(fprime, w, vec)
         coeff = transpose(matmul(x, vec))               ! rows are MOs
         dens = matmul(transpose(coeff(1:nocc, :)), coeff(1:nocc, :))
         eold = energy
         energy = sum(dens*(mol%hcore + fock))
         rms = sqrt(sum((dens - dold)**2))
         dold = dens
         t1 = seconds()
         write (out, '(1X, I9, 3X, F15.10, 3X, F15.10, 3X, F15.10, 3X, F8.6)') iter, energy, energy - eold, rms, t1 - t0
         t0 = t1
         if (rms < cfg%scf_d_tol .and. abs(energy - eold) < cfg%scf_e_tol) then
            converged = .true.
            exit
         end if
         ! Fock build: F = H + sum_kl D(k,l) [2 (ij|kl) - (ik|jl)]
         if (on_device) then
            if (afesp_build_fock(ctx, int(n, c_int64_t), dens, mol%hcore, fock) /= 0) &
               call fail('hf::build_fock', afesp_error_text(ctx))
         else
         do j = 1, n
            do i = 1, n
               val = mol%hcore(i, j)
               do l = 1, n
                  do k = 1, n
                     val = val + dens(k, l)*(2.0_dp*mol%eri(eri_slot(i, j, k, l)) - mol%eri(eri_slot(i, k, j, l)))
                  end do
               end do
               fock(i, j) = val
            end do
         end do
         end if
         if (m >= 2) then
            slot = slot + 1; if (slot > m) slot = slot - m
            if (nact < m) nact = nact + 1
            fhist(:, :, slot) = fock
            ehist(:, :, slot) = matmul(fock, matmul(dens, mol%ovlp)) - matmul(mol%ovlp, matmul(dens, fock))
            if (nact > 1) then
               allocate (bmat(nact + 1, nact + 1), rhs(nact + 1))
               bmat = -1.0_dp; bmat(nact + 1, nact + 1) = 0.0_dp; rhs = 0.0_dp; rhs(nact + 1) = -1.0_dp
               do i = 1, nact
                  do j = 1, nact
                     bmat(i, j) = sum(ehist(:, :, i)*ehist(:, :, j))
                  end do
               end do
               call solve(bmat, rhs, info)
               if (info /= 0) call fail('hf::update_diis', 'Linear solve failed!')
               fock = 0.0_dp
               do i = 1, nact; fock = fock + rhs(i)*fhist(:, :, i); end do
               deallocate (bmat, rhs)
            end if
         end if
      end do
      e_hf = energy; levels = w
      if (converged) then
         write (out, '(75("-"))')
         write (out, '(1X, A)') 'Convergence reached within tolerance.'
         write (out, '(1X, A, 1X, F15.8)') 'Final SCF Energy (Hartree):', energy
         write (out, '(1X, A)') 'Orbital energies (Hartree):'
         do i = n, 1, -1; write (out, '(1X, I3, 1X, F15.8)') i, w(i); end do
         if (cfg%scf_write_guess) then
            write (out, *) 'Writing AO Fock matrix for future use...'
            open (newunit=unit, file='guess_out.dat', status='replace', action='write')
            do i = 1, n; do j = 1, n; write (unit, '(I0, 1X, I0, 1X, ES16.9)') i, j, fock(i, j); end do; end do
            close (unit)
         end if
      else
         write (out, '(1X, A)') 'Convergence not reached, please increase maxiter.'
      end if
   end subroutine

   !> Unrestricted Hartree-Fock, the rhf iteration above for two spins (afesp_amd/uhf.py is the same algorithm): both Fock
   !> matrices start from H_core or guess_in.dat, D_s = C_s,occ^T C_s,occ, E = 1/2 sum [(Da + Db) H + Da Fa + Db Fb], the rms change
   !> is the mean of the two spins' squared changes, and DIIS takes one set of coefficients for the concatenated error vectors.
   !> on_device: F_s = H + J[Da + Db] - K[D_s] by afesp_build_fock_uhf.  Returns <S^2> with the orbitals.
   subroutine uhf(cfg, mol, na, nb, e_hf, ca, cb, la, lb, s2, converged, ctx, on_device)
      type(run_config), intent(in) :: cfg
      type(molecule), intent(in) :: mol
      integer, intent(in) :: na, nb
      type(c_ptr), intent(in) :: ctx
      logical, intent(in) :: on_device
      real(dp), intent(out) :: e_hf, s2
      real(dp), allocatable, intent(out) :: ca(:, :), cb(:, :), la(:), lb(:)
      logical, intent(out) :: converged
      integer :: n, iter, i, j, k, l, slot, nact, m, unit, ios, info
      real(dp), allocatable :: x(:, :), fa(:, :), fb(:, :), vec(:, :), da(:, :), db(:, :), daold(:, :), dbold(:, :), sv(:), u(:, :)
      real(dp), allocatable :: fhist(:, :, :, :), ehist(:, :, :, :), bmat(:, :), rhs(:), ov(:, :)
      real(dp) :: energy, eold, rms, val, jv, t0, t1, sz
      n = mol%nbasis
      write (out, '(1X, 25("-"))'); write (out, '(1X, A)') 'Unrestricted Hartree-Fock'; write (out, '(1X, 25("-"))')
      write (out, '(1X, A, 1X, I0, 1X, I0)') 'Alpha and beta electrons:', na, nb
      allocate (x(n, n), fa(n, n), fb(n, n), vec(n, n), da(n, n), db(n, n), daold(n, n), dbold(n, n), sv(n), u(n, n))
      allocate (ca(n, n), cb(n, n), la(n), lb(n))
      call sym_eig(mol%ovlp, sv, u)
      do j = 1, n; vec(:, j) = u(:, j)/sqrt(sv(j)); end do
      x = matmul(vec, transpose(u))                       ! S^-1/2
      fa = mol%hcore
      if (cfg%scf_read_guess) then
         write (out, *) 'Reading previous AO Fock matrix as guess...'
         open (newunit=unit, file='guess_in.dat', status='old', action='read')
         do
            read (unit, *, iostat=ios) i, j, val
            if (ios /= 0) exit
            fa(i, j) = val
         end do
         close (unit)
      end if
      fb = fa
      m = cfg%scf_diis_n_errmat
      if (m >= 2) then
         allocate (fhist(n, n, 2, m), ehist(n, n, 2, m)); fhist = 0.0_dp; ehist = 0.0_dp
      end if
      slot = 0; nact = 0; energy = 0.0_dp; daold = 0.0_dp; dbold = 0.0_dp; converged = .false.
      write (out, '(75("-"))')
      write (out, '(1X, A, 3X, A, 3X, A, 3X, A, 3X, A)') 'Iteration', '     Energy    ', '    deltaE     ', '   delta RMS D ', '  Time  '
      write (out, '(75("-"))')
      t0 = seconds()
      do iter = 1, cfg%scf_maxiter
         call sym_eig(matmul(transpose(x), matmul(fa, x)), la, vec)
         ca = transpose(matmul(x, vec))
         call sym_eig(matmul(transpose(x), matmul(fb, x)), lb, vec)
         cb = transpose(matmul(x, vec))
         da = matmul(transpose(ca(1:na, :)), ca(1:na, :))
         db = matmul(transpose(cb(1:nb, :)), cb(1:nb, :))
         eold = energy
         energy = 0.5_dp*(sum(da*(mol%hcore + fa)) + sum(db*(mol%hcore + fb)))
         rms = sqrt(0.5_dp*(sum((da - daold)**2) + sum((db - dbold)**2)))
         daold = da; dbold = db
         t1 = seconds()
         write (out, '(1X, I9, 3X, F15.10, 3X, F15.10, 3X, F15.10, 3X, F8.6)') iter, energy, energy - eold, rms, t1 - t0
         t0 = t1
         if (rms < cfg%scf_d_tol .and. abs(energy - eold) < cfg%scf_e_tol) then
            converged = .true.
            exit
         end if
         if (on_device) then
            if (afesp_build_fock_uhf(ctx, int(n, c_int64_t), da, db, mol%hcore, fa, fb) /= 0) &
               call fail('hf::build_fock_uhf', afesp_error_text(ctx))
         else
         do j = 1, n
            do i = 1, n
               jv = mol%hcore(i, j)
               do l = 1, n
                  do k = 1, n
                     jv = jv + (da(k, l) + db(k, l))*mol%eri(eri_slot(i, j, k, l))
                  end do
               end do
               fa(i, j) = jv; fb(i, j) = jv
               do l = 1, n
                  do k = 1, n
                     val = mol%eri(eri_slot(i, k, j, l))
                     fa(i, j) = fa(i, j) - da(k, l)*val
                     fb(i, j) = fb(i, j) - db(k, l)*val
                  end do
               end do
            end do
         end do
         end if
         if (m >= 2) then
            slot = slot + 1; if (slot > m) slot = slot - m
            if (nact < m) nact = nact + 1
            fhist(:, :, 1, slot) = fa; fhist(:, :, 2, slot) = fb
            ehist(:, :, 1, slot) = matmul(fa, matmul(da, mol%ovlp)) - matmul(mol%ovlp, matmul(da, fa))
            ehist(:, :, 2, slot) = matmul(fb, matmul(db, mol%ovlp)) - matmul(mol%ovlp, matmul(db, fb))
            if (nact > 1) then
               allocate (bmat(nact + 1, nact + 1), rhs(nact + 1))
               bmat = -1.0_dp; bmat(nact + 1, nact + 1) = 0.0_dp; rhs = 0.0_dp; rhs(nact + 1) = -1.0_dp
               do i = 1, nact
                  do j = 1, nact
                     bmat(i, j) = sum(ehist(:, :, :, i)*ehist(:, :, :, j))
                  end do
               end do
               call solve(bmat, rhs, info)
               if (info /= 0) call fail('hf::update_diis', 'Linear solve failed!')
               fa = 0.0_dp; fb = 0.0_dp
               do i = 1, nact
                  fa = fa + rhs(i)*fhist(:, :, 1, i); fb = fb + rhs(i)*fhist(:, :, 2, i)
               end do
               deallocate (bmat, rhs)
            end if
         end if
      end do
      e_hf = energy
      ! <S^2> = Sz (Sz + 1) + n_beta - sum_ij |<i_alpha|j_beta>|^2 over the occupied orbitals
      sz = 0.5_dp*(na - nb)
      ov = matmul(ca(1:na, :), matmul(mol%ovlp, transpose(cb(1:nb, :))))
      s2 = sz*(sz + 1.0_dp) + nb - sum(ov*ov)
      if (converged) then
         write (out, '(75("-"))')
         write (out, '(1X, A)') 'Convergence reached within tolerance.'
         write (out, '(1X, A, 1X, F15.8)') 'Final SCF Energy (Hartree):', energy
         write (out, '(1X, A, 1X, F10.6)') '<S^2>:', s2
         write (out, '(1X, A)') 'Alpha orbital energies (Hartree):'
         do i = n, 1, -1; write (out, '(1X, I3, 1X, F15.8)') i, la(i); end do
         write (out, '(1X, A)') 'Beta orbital energies (Hartree):'
         do i = n, 1, -1; write (out, '(1X, I3, 1X, F15.8)') i, lb(i); end do
      else
         write (out, '(1X, A)') 'Convergence not reached, please increase maxiter.'
      end if
   end subroutine
end module host_scf

program els_amd
   use, intrinsic :: iso_c_binding
   use host_support
   use host_config
   use host_inputs
   use host_scf
   use host_fno
   use host_linalg
   use afesp_capi
   implicit none
   type(run_config) :: cfg
   type(molecule) :: mol
   type(c_ptr) :: ctx
   real(dp), allocatable :: coeff(:, :), levels(:), t1(:, :)
   real(dp), allocatable :: cb(:, :), lb(:)     ! beta orbitals of the open-shell types (alpha: coeff / levels)
   real(dp) :: s2
   integer :: na, nb
   ! the active orbital window [nfc, nbasis - nfv): active basis size, occupied / virtual counts, electrons and spin counts
   integer :: nfc, nfv, n_act, o_act, v_act, nel_act, na_act, nb_act
   logical :: windowed
   ! frozen natural orbitals: asked for, natural virtuals kept, MP2 in the full virtual space, the Delta MP2 correction
   logical :: fno
   integer :: fno_kept, vmin
   real(dp) :: e_mp2_full, delta_mp2
   ! fcidump_active: the frozen-core operator(s) of the window and the core energy, taken before the window
   real(dp), allocatable :: h_act(:, :), h_act_b(:, :)
   real(dp) :: e_core
   ! ROHF types: the spin Fock matrices of the file's determinant in semicanonical orbitals
   real(dp), allocatable :: fock_sa(:, :), fock_sb(:, :)
   ! cc_density: <beta orbital b | alpha orbital a> over the whole basis where the two sets differ (UHF: C_b S C_a^T; ROHF: u_b u_a^T)
   real(dp), allocatable :: ab_overlap(:, :)
   character(len=16) :: mp2name, ccname
   real(dp) :: e_hf, e_mp2, e_ccsd, energy, eold, rms, tq(6), t0, t1s, tstart, t1diag, e_highest
   real(dp) :: e_bt, e_pt, e_rbt, e_rpt, e_crbt, e_crpt
   integer(c_int) :: rc, conv
   integer :: iter, device, rank, world, transport, sb
   integer(c_int64_t), allocatable :: bounds(:)
   integer(c_int64_t) :: t_lo, t_hi
   real(dp) :: red(9)
   character(256) :: my_error
   integer :: rc_mine
   character(len=512) :: comm_file
   logical :: scf_ok, cc_ok, compat, have_ctx
   logical :: lambda_live = .false.   ! lambda_solve has converged Lambda for the CCSD state (cc_density, cc_lambda_t)
   real(dp) :: e_lt = 0.0_dp          ! the Lambda-CCSD(T) correction (cc_lambda_t)
   integer(c_int64_t) :: nlines
   character(len=32) :: envval
   character(len=80) :: calcname
   real(dp), parameter :: fcidump_threshold = 1e-12_dp   ! fcidump_active keeps every integral above this (16 digits are written)

   tstart = seconds()
   ! Rank mode (one process per GPU, started by host/els_mgpu.sh or any launcher that sets these): AFESP_RANK / AFESP_WORLD,
   ! AFESP_COMM = rccl (default) | host, AFESP_COMM_FILE = bootstrap file unique to the job.  Every rank runs the calculation
   ! (RHF, AO->MO and the CCSD iterations as replicas); the (T) triples are split over the ranks and summed with one
   ! all-reduce, where the reference's OpenMP reduction sits (src/ccsd.f90:2091).  Only rank 0 prints.
   rank = 0; world = 1; transport = AFESP_COMM_RCCL; comm_file = ''
   call get_environment_variable('AFESP_WORLD', envval)
   if (len_trim(envval) > 0) read (envval, *) world
   call get_environment_variable('AFESP_RANK', envval)
   if (len_trim(envval) > 0) read (envval, *) rank
   if (world < 1 .or. rank < 0 .or. rank >= world) call fail('main', 'AFESP_RANK / AFESP_WORLD are inconsistent')
   if (world > 1) then
      call get_environment_variable('AFESP_COMM', envval)
      if (trim(envval) == 'host') transport = AFESP_COMM_HOST
      call get_environment_variable('AFESP_COMM_FILE', comm_file)
      if (len_trim(comm_file) == 0) call fail('main', 'AFESP_WORLD > 1 needs AFESP_COMM_FILE (a bootstrap file unique to the job)')
      if (rank > 0) open (unit=out, file='/dev/null', action='write')     ! rank 0 owns stdout
   end if
   write (out, '(1X, 64("="))')
   write (out, '(1X, A)') 'A Fortran Electronic Structure Programme (AFESP) -- MI355X engine host'
   write (out, '(1X, 64("="))')
   call read_config(cfg)
   if (rank > 0) then   ! every rank runs the replicated stages in the same directory: the files are rank 0's to write
      cfg%scf_write_guess = .false.; cfg%write_fcidump = .false.; cfg%fcidump_active = .false.
   end if
   ! Post-HF levels: the engine context exists from the start, and the engine reads eri.dat (the packed AO integrals
   ! then stay on the device for the AO->MO transform; the host copy feeds the SCF)
   have_ctx = cfg%level >= LEVEL_MP2
   if (cfg%fcidump_in) then
      call scan_input_file()   ! extents and electron counts from the header of ./FCIDUMP
   else
      call read_molecule(mol, have_ctx)
   end if
   if (have_ctx) then
      device = 0
      if (world > 1 .and. afesp_device_count() > 0) device = mod(rank, int(afesp_device_count()))   ! one GPU per rank
      call get_environment_variable('AFESP_DEVICE', envval)
      if (len_trim(envval) > 0) read (envval, *) device
      rc = afesp_ctx_create(int(device, c_int), ctx)
      if (rc /= 0) call fail('main', 'no usable MI355X device: afesp_ctx_create failed (the engine has no CPU fallback)')
      if (world > 1) then
         rc = afesp_comm_init(ctx, int(rank, c_int), int(world, c_int), int(transport, c_int), trim(comm_file)//c_null_char, c_null_ptr)
         if (rc /= 0) call fail('main', afesp_error_text(ctx))
         write (out, '(1X, A, I0, A, A)') 'Ranks: ', world, ', transport ', merge('host', 'rccl', transport == AFESP_COMM_HOST)
      end if
      if (.not. cfg%fcidump_in) then
         rc = afesp_read_eri_text(ctx, 'eri.dat'//c_null_char, int(mol%nbasis, c_int64_t), mol%eri, nlines)
         if (rc /= 0) call fail('integrals::read_integrals_in', afesp_error_text(ctx))
         write (out, *) 'Done reading integrals!'
      end if
   end if
   write (out, '(1X, 20("-"))'); write (out, '(1X, A)') 'System information'; write (out, '(1X, 20("-"))')
   if (cfg%uhf .and. .not. cfg%fcidump_in) then   ! nel = sum Z - charge, n_alpha - n_beta = multiplicity - 1
      mol%nel = mol%nel - cfg%charge
      if (mol%nel < 0 .or. mod(mol%nel + cfg%multiplicity - 1, 2) /= 0) &
         call fail('system::read_system_in', 'charge and multiplicity do not fit the electron count!')
      na = (mol%nel + cfg%multiplicity - 1)/2; nb = (mol%nel - cfg%multiplicity + 1)/2
      if (nb < 0 .or. na > mol%nbasis) call fail('system::read_system_in', 'charge and multiplicity do not fit the electron count!')
      if (cfg%level >= LEVEL_MP2 .and. na + nb >= 2*mol%nbasis) &
         call fail('system::read_system_in', 'no virtual spin orbital for a correlated calculation!')
   end if
   write (out, '(1X, A, 1X, I0)') 'Number of electrons:', mol%nel
   write (out, '(1X, A, 1X, I0)') 'Number of basis functions:', mol%nbasis
   if (cfg%uhf) then
      if (.not. cfg%fcidump_in) write (out, '(1X, A, 1X, I0, 1X, I0)') 'Charge and multiplicity:', cfg%charge, cfg%multiplicity
      if (cfg%fcidump_in) write (out, '(1X, A, 1X, I0, 1X, I0)') 'Alpha and beta electrons (NELEC, MS2 of the file):', na, nb
      write (out, '(1X, A, 1X, I0)') 'Number of occupied orbitals:', na + nb
      write (out, '(1X, A, 1X, I0)') 'Number of virtual orbitals:', 2*mol%nbasis - na - nb
   else if (cfg%spinorb) then   ! spin-orbital counts, reference src/geometry.f90:44-45
      write (out, '(1X, A, 1X, I0)') 'Number of occupied orbitals:', mol%nel
      write (out, '(1X, A, 1X, I0)') 'Number of virtual orbitals:', 2*mol%nbasis - mol%nel
   else
      write (out, '(1X, A, 1X, I0)') 'Number of occupied orbitals:', mol%nocc
      write (out, '(1X, A, 1X, I0)') 'Number of virtual orbitals:', mol%nvirt
   end if
   ! the active orbital window of the correlated steps
   nfc = 0; nfv = 0
   if (cfg%level >= LEVEL_MP2) then
      nfv = cfg%n_frozen_virt
      if (cfg%n_frozen_core >= 0) then
         nfc = cfg%n_frozen_core
      else if (cfg%frozen_core) then
         if (mol%ncore < 0) call fail('system::read_system_in', 'frozen_core: no core count for atoms beyond Kr, give n_frozen_core')
         nfc = mol%ncore
      end if
   end if
   windowed = nfc > 0 .or. nfv > 0
   n_act = mol%nbasis - nfc - nfv; o_act = mol%nocc - nfc; v_act = mol%nvirt - nfv; nel_act = mol%nel - 2*nfc
   if (cfg%uhf) then
      na_act = na - nfc; nb_act = nb - nfc
   else
      na_act = o_act; nb_act = o_act
   end if
   if (windowed) then
      write (out, '(1X, A, 1X, I0)') 'Number of frozen core orbitals:', nfc
      write (out, '(1X, A, 1X, I0)') 'Number of frozen virtual orbitals:', nfv
      if (cfg%uhf) then   ! (what afesp_ccsd_uso_init accepts: a spin may keep no occupied orbital)
         if (n_act <= 0 .or. na_act < 0 .or. nb_act < 0 .or. na_act + nb_act <= 0) &
            call fail('system::read_system_in', 'the frozen core leaves no active occupied orbital')
         if (na_act > n_act .or. na_act + nb_act >= 2*n_act) &
            call fail('system::read_system_in', 'the frozen virtual orbitals leave no active virtual orbital')
      else
         if (o_act <= 0) call fail('system::read_system_in', 'the frozen core leaves no active occupied orbital')
         if (v_act <= 0) call fail('system::read_system_in', 'the frozen virtual orbitals leave no active virtual orbital')
      end if
   end if
   fno = cfg%level >= LEVEL_MP2 .and. (cfg%fno_n_virt >= 0 .or. cfg%fno_occ_tol > 0.0_dp)
   fno_kept = 0; e_mp2_full = 0.0_dp; delta_mp2 = 0.0_dp
   if (fno .and. cfg%fno_n_virt >= 0) then   ! (an open shell counts in the smaller of its two virtual spaces)
      vmin = mol%nvirt
      if (cfg%uhf) vmin = mol%nbasis - max(na, nb)
      if (cfg%fno_n_virt < 1 .or. cfg%fno_n_virt > vmin) call fail('system::read_system_in', &
         'fno_n_virt leaves no active virtual orbital or exceeds the number of virtual orbitals')
   end if
   write (out, '(1X, A, 1X, ES15.8)') 'E_nuc:', mol%e_nuc
   write (out, '(1X, A, 1X, A)') 'calc_type:', trim(cfg%calc_type)

   t0 = seconds()
   if (cfg%fcidump_in) then
      call read_input_file()   ! the integrals onto the device, levels and the reference determinant's energy from them
   else if (cfg%uhf) then
      call uhf(cfg, mol, na, nb, e_hf, coeff, cb, levels, lb, s2, scf_ok, ctx, have_ctx)
      write (out, '(1X, A, 1X, F16.8, A)') 'Time taken for unrestricted Hartree-Fock:', seconds() - t0, 's'
   else
      call rhf(cfg, mol, e_hf, coeff, levels, scf_ok, ctx, have_ctx)
      write (out, '(1X, A, 1X, F16.8, A)') 'Time taken for restricted Hartree-Fock:', seconds() - t0, 's'
   end if
   e_highest = 0.0_dp; e_mp2 = 0.0_dp; e_ccsd = 0.0_dp; t1diag = 0.0_dp; tq = 0.0_dp; cc_ok = .false.
   e_bt = 0.0_dp; e_pt = 0.0_dp; e_rbt = 0.0_dp; e_rpt = 0.0_dp; e_crbt = 0.0_dp; e_crpt = 0.0_dp

   if (cfg%uhf .and. cfg%level >= LEVEL_MP2 .and. scf_ok) then
      ! ---------------- open shells: UMP2 from the three spin blocks, then the spin-orbital CCSD / (T) on them
      t0 = seconds()
      mp2name = merge('ROHF-MBPT(2)', 'UMP2        ', cfg%rohf); ccname = merge('ROHF-CCSD', 'UCCSD    ', cfg%rohf)
      write (out, '(1X, 10("-"))'); write (out, '(1X, A)') trim(mp2name); write (out, '(1X, 10("-"))')
      if (.not. cfg%fcidump_in) then
         write (out, '(1X, A)') 'Performing AO to MO ERI transformation (alpha-alpha, alpha-beta, beta-beta)...'
         rc = afesp_ao2mo_ump2(ctx, int(mol%nbasis, c_int64_t), int(na, c_int64_t), int(nb, c_int64_t), coeff, cb, levels, lb, &
                               c_null_ptr, c_null_ptr, c_null_ptr, c_null_ptr, e_mp2)
         if (rc /= 0) call fail('mp2::do_ump2', afesp_error_text(ctx))
      end if
      if (fno) call open_shell_fno()   ! natural virtuals of both spins, second transform; sets nfv and the active extents
      if (cfg%fcidump_active) call core_operator_before_window()
      if (cfg%rohf) then   ! the state with the full Fock matrices of the semicanonical orbitals: its start amplitudes give ROHF-MBPT(2)
         rc = afesp_ccsd_uso_init_fock(ctx, int(n_act, c_int64_t), int(na_act, c_int64_t), int(nb_act, c_int64_t), fock_sa, fock_sb, &
                                       int(cfg%ccsd_diis_n_errmat, c_int), e_mp2)
         if (rc /= 0) call fail('ccsd::init_cc', afesp_error_text(ctx))
      else if (windowed .or. fno .or. cfg%fcidump_in) then   ! the three blocks over the active orbitals, and the frozen-core UMP2 energy
         ! (integrals read from a file: this call, with nothing frozen too, is the one that reports the UMP2 energy)
         rc = afesp_umo_window(ctx, int(mol%nbasis, c_int64_t), int(na, c_int64_t), int(nb, c_int64_t), int(nfc, c_int64_t), &
                               int(nfv, c_int64_t), levels, lb, c_null_ptr, c_null_ptr, c_null_ptr, e_mp2)
         if (rc /= 0) call fail('mp2::do_ump2', afesp_error_text(ctx))
      end if
      if (cfg%fcidump_active) call dump_active_space()
      if (cfg%rohf) then
         write (out, '(1X, A, 1X, F18.12)') 'ROHF-MBPT(2) correlation energy (Hartree):', e_mp2
      else
      write (out, '(1X, A, 1X, F15.8)') 'UMP2 correlation energy (Hartree):', e_mp2
      end if
      if (fno) call print_fno_energies('UMP2')
      e_highest = e_mp2
      write (out, '(1X, A, 1X, F16.8, A)') 'Time taken for '//trim(mp2name)//':', seconds() - t0, 's'
      if (cfg%level >= LEVEL_CCSD) then
         t0 = seconds()
         write (out, '(1X, 10("-"))'); write (out, '(1X, A)') 'CCSD'; write (out, '(1X, 10("-"))')
         if (.not. cfg%rohf) then   ! (a ROHF state exists already: afesp_ccsd_uso_init_fock above)
         write (out, '(1X, A)') 'Forming slices of antisymmetrised spinorbital ERIs from the UHF blocks...'
         rc = afesp_ccsd_uso_init(ctx, int(n_act, c_int64_t), int(na_act, c_int64_t), int(nb_act, c_int64_t), levels(nfc + 1:), &
                                  lb(nfc + 1:), int(cfg%ccsd_diis_n_errmat, c_int))
         if (rc /= 0) call fail('ccsd::init_cc', afesp_error_text(ctx))
         end if
         rc = afesp_ccsd_so_energy(ctx, cfg%ccsd_e_tol, cfg%ccsd_t_tol, energy, rms, conv)
         if (rc /= 0) call fail('ccsd::update_cc_energy', afesp_error_text(ctx))
         write (out, '(75("-"))')
         write (out, '(1X, A, 3X, A, 3X, A, 3X, A, 3X, A)') 'Iteration', '     Energy    ', '    deltaE     ', '  delta RMS T2 ', '  Time  '
         write (out, '(75("-"))')
         write (out, '(1X, A9, 3X, F15.12, 3X, F15.12, 3X, F15.12)') 'MP1', energy, energy, rms
         t1s = seconds()
         do iter = 1, cfg%ccsd_maxiter
            eold = energy
            rc = afesp_ccsd_so_iterate(ctx, cfg%ccsd_e_tol, cfg%ccsd_t_tol, energy, rms, conv)
            if (rc /= 0) call fail('ccsd::update_amplitudes', afesp_error_text(ctx))
            write (out, '(1X, I9, 3X, F15.12, 3X, F15.12, 3X, F15.12, 3X, F8.6)') iter, energy, energy - eold, rms, seconds() - t1s
            t1s = seconds()
            if (conv /= 0) then
               cc_ok = .true.
               exit
            end if
            rc = afesp_ccsd_so_diis(ctx)
            if (rc /= 0) call fail('ccsd::update_diis_cc', 'Linear solve failed!')
         end do
         if (cc_ok) then
            write (out, '(75("-"))')
            write (out, '(1X, A)') 'Convergence reached within tolerance.'
            write (out, '(1X, A, 1X, F15.12)') 'Final '//trim(ccname)//' Energy (Hartree):', energy
            e_ccsd = energy; e_highest = e_ccsd
         end if
         write (out, '(1X, A, 1X, F16.8, A)') 'Time taken for '//trim(ccname)//':', seconds() - t0, 's'
         if (cfg%cc_density .and. cc_ok) then
            if (.not. cfg%rohf) ab_overlap = matmul(cb, matmul(mol%ovlp, transpose(coeff)))
            call lambda_and_occupations(n_act, na_act, nb_act, .false.)
         end if
         if (cfg%cc_rdm2 .and. cc_ok) then
            if (.not. cfg%rohf .and. .not. allocated(ab_overlap)) ab_overlap = matmul(cb, matmul(mol%ovlp, transpose(coeff)))
            call rdm2_energy_and_spin(n_act, na_act, nb_act, .false.)
         end if
         if (cfg%cc_relaxed .and. cc_ok) then
            if (.not. allocated(ab_overlap)) ab_overlap = matmul(cb, matmul(mol%ovlp, transpose(coeff)))
            call relaxed_density_report(n_act, na_act, nb_act, .false.)
         end if
         if ((cfg%cc_lambda_t .or. cfg%eom_ipea_left) .and. cc_ok .and. .not. lambda_live) call lambda_solve()
         if (cfg%eom_nroots > 0 .and. cc_ok) call eom_excitations(na_act + nb_act, 2*n_act - na_act - nb_act)
         if (cfg%eom_ip_nroots > 0 .and. cc_ok) call eom_ipea(AFESP_EOM_IP, cfg%eom_ip_nroots, na_act + nb_act, 2*n_act - na_act - nb_act)
         if (cfg%eom_ea_nroots > 0 .and. cc_ok) call eom_ipea(AFESP_EOM_EA, cfg%eom_ea_nroots, na_act + nb_act, 2*n_act - na_act - nb_act)
         if (cfg%cc_polar .and. cc_ok) call polarizability_report(n_act, na_act, nb_act, .false.)
         if (cfg%level == LEVEL_CCSD_T .and. cc_ok) then
            t0 = seconds()
            write (out, '(1X, 10("-"))'); write (out, '(1X, A)') 'CCSD(T)'; write (out, '(1X, 10("-"))')
            t_hi = afesp_ccsd_so_t_ntriples(int(na_act + nb_act, c_int64_t))     ! i<j<k triples, an even split over the ranks
            t_lo = (int(rank, c_int64_t)*t_hi)/world; t_hi = (int(rank + 1, c_int64_t)*t_hi)/world
            rc = afesp_ccsd_so_t(ctx, t_lo, t_hi, tq(1))
            if (world > 1) then   ! (every rank enters the sum, a failed shard as a flag: as in the spin-orbital branch below)
               rc_mine = rc; my_error = ''
               if (rc_mine /= 0) then; my_error = afesp_error_text(ctx); tq(1) = 0.0_dp; end if
               tq(2) = merge(1.0_dp, 0.0_dp, rc_mine /= 0)
               rc = afesp_allreduce_sum(ctx, tq, 2_c_int64_t)
               if (rc_mine /= 0) call fail('ccsd::do_ccsd_t_spinorb', trim(my_error))
               if (rc == 0 .and. tq(2) > 0.5_dp) call fail('ccsd::do_ccsd_t_spinorb', 'the (T) shard of another rank failed')
            end if
            if (rc /= 0) call fail('ccsd::do_ccsd_t_spinorb', afesp_error_text(ctx))
            e_pt = e_ccsd + tq(1)
            e_highest = e_pt
            if (cfg%rohf) then
               write (out, '(1X, A, 1X, F18.12)') 'ROHF-CCSD(T) correlation energy (Hartree):', e_pt
            else
            write (out, '(1X, A, 1X, F15.9)') 'UCCSD(T) correlation energy (Hartree):', e_pt
            end if
            write (out, '(1X, A, 1X, F16.8, A)') 'Time taken for '//trim(ccname)//'(T):', seconds() - t0, 's'
         end if
         if (cfg%cc_lambda_t .and. cc_ok .and. cfg%rohf) call lambda_triples(na_act + nb_act, 'ROHF-ΛCCSD(T)')
         if (cfg%cc_lambda_t .and. cc_ok .and. .not. cfg%rohf) call lambda_triples(na_act + nb_act, 'UΛCCSD(T)')
      end if
   else if (cfg%level >= LEVEL_MP2 .and. scf_ok) then
      ! ---------------- MP2: AO->MO transform + energy on the device (reference do_mp2_spatial)
      t0 = seconds()
      write (out, '(1X, 10("-"))'); write (out, '(1X, A)') 'MP2'; write (out, '(1X, 10("-"))')
      if (.not. cfg%fcidump_in) then
         write (out, '(1X, A)') 'Performing AO to MO ERI transformation...'
         rc = afesp_ao2mo_mp2(ctx, int(mol%nbasis, c_int64_t), int(mol%nocc, c_int64_t), coeff, levels, c_null_ptr, c_null_ptr, e_mp2)
         if (rc /= 0) call fail('mp2::do_mp2_spatial', afesp_error_text(ctx))
      end if
      if (fno) then   ! the FCIDUMP (if asked for) is of the canonical integrals; then natural virtuals and the second transform
         if (cfg%write_fcidump) call dump_integrals()
         call closed_shell_fno()
      end if
      if (cfg%fcidump_active) call core_operator_before_window()
      if (windowed .or. fno .or. cfg%fcidump_in) then   ! (integrals read from a file: the MP2 energy comes from this call in any case)
         ! frozen orbitals: the FCIDUMP (if asked for) is of the full integrals; then the window over the active orbitals replaces
         ! them on the device, and the MP2 energy is the frozen-core one
         if (cfg%write_fcidump .and. .not. fno) call dump_integrals()
         rc = afesp_mo_window(ctx, int(mol%nbasis, c_int64_t), int(mol%nocc, c_int64_t), int(nfc, c_int64_t), int(nfv, c_int64_t), &
                              levels, c_null_ptr, c_null_ptr, e_mp2)
         if (rc /= 0) call fail('mp2::do_mp2_spatial', afesp_error_text(ctx))
      end if
      if (cfg%fcidump_active) call dump_active_space()
      write (out, '(1X, A)') 'Calculating MP2 energy...'
      write (out, '(1X, A, 1X, F15.8)') 'MP2 correlation energy (Hartree):', e_mp2
      if (fno) call print_fno_energies('MP2')
      e_highest = e_mp2
      if (cfg%write_fcidump .and. .not. windowed .and. .not. fno) call dump_integrals()        ! reference src/mp2.f90:445-447
      t1s = seconds()
      write (out, '(1X, A, 1X, F16.8, A)') 'Time taken for restricted MP2:', t1s - t0, 's'

      if (cfg%level >= LEVEL_CCSD .and. cfg%spinorb) then
         ! ---------------- spin-orbital CCSD (reference do_ccsd_spinorb, src/ccsd.f90:71-277), same loop structure
         t0 = seconds()
         write (out, '(1X, 10("-"))'); write (out, '(1X, A)') 'CCSD'; write (out, '(1X, 10("-"))')
         write (out, '(1X, A)') 'Forming antisymmetrised spinorbital ERIs...'
         write (out, '(1X, A)') 'Forming slices of antisymmetrised spinorbital ERIs'
         write (out, '(1X, A)') 'Initialise CC intermediate tensors and DIIS auxilliary arrays...'
         ! AFESP_SO_FOO_AS_PUBLISHED=1: tau~ term of F_mi in Stanton's index order (what the reference's shipped
         ! ref_out was computed with); default: as src/ccsd.f90:789-794 accumulates it today
         call get_environment_variable('AFESP_SO_FOO_AS_PUBLISHED', envval)
         rc = afesp_ccsd_so_init(ctx, int(n_act, c_int64_t), int(nel_act, c_int64_t), c_null_ptr, levels(nfc + 1:), &
                                 int(cfg%ccsd_diis_n_errmat, c_int), merge(1_c_int, 0_c_int, trim(envval) == '1'))
         if (rc /= 0) call fail('ccsd::init_cc', afesp_error_text(ctx))
         write (out, '(1X, A, 1X, F8.6, A)') 'Time taken:', seconds() - t0, ' s'
         write (out, *)
         write (out, '(1X, A)') 'Initialisation done, now entering iterative CC solver...'
         rc = afesp_ccsd_so_energy(ctx, cfg%ccsd_e_tol, cfg%ccsd_t_tol, energy, rms, conv)
         if (rc /= 0) call fail('ccsd::update_cc_energy', afesp_error_text(ctx))
         write (out, '(75("-"))')
         write (out, '(1X, A, 3X, A, 3X, A, 3X, A, 3X, A)') 'Iteration', '     Energy    ', '    deltaE     ', '  delta RMS T2 ', '  Time  '
         write (out, '(75("-"))')
         write (out, '(1X, A9, 3X, F15.12, 3X, F15.12, 3X, F15.12)') 'MP1', energy, energy, rms
         t1s = seconds()
         do iter = 1, cfg%ccsd_maxiter
            eold = energy
            rc = afesp_ccsd_so_iterate(ctx, cfg%ccsd_e_tol, cfg%ccsd_t_tol, energy, rms, conv)
            if (rc /= 0) call fail('ccsd::update_amplitudes', afesp_error_text(ctx))
            write (out, '(1X, I9, 3X, F15.12, 3X, F15.12, 3X, F15.12, 3X, F8.6)') iter, energy, energy - eold, rms, seconds() - t1s
            t1s = seconds()
            if (conv /= 0) then
               cc_ok = .true.
               exit
            end if
            rc = afesp_ccsd_so_diis(ctx)
            if (rc /= 0) call fail('ccsd::update_diis_cc', 'Linear solve failed!')
         end do
         if (cc_ok) then
            write (out, '(75("-"))')
            write (out, '(1X, A)') 'Convergence reached within tolerance.'
            write (out, '(1X, A, 1X, F15.12)') 'Final CCSD Energy (Hartree):', energy
            e_ccsd = energy; e_highest = e_ccsd
         end if
         write (out, '(1X, A, 1X, F16.8, A)') 'Time taken for unrestricted CCSD:', seconds() - t0, 's'
         if (cfg%cc_density .and. cc_ok) call lambda_and_occupations(n_act, nel_act/2, nel_act/2, .true.)
         if (cfg%cc_rdm2 .and. cc_ok) call rdm2_energy_and_spin(n_act, nel_act/2, nel_act/2, .true.)
         if (cfg%cc_relaxed .and. cc_ok) call relaxed_density_report(n_act, nel_act/2, nel_act/2, .true.)
         if ((cfg%cc_lambda_t .or. cfg%eom_ipea_left) .and. cc_ok .and. .not. lambda_live) call lambda_solve()
         if (cfg%eom_nroots > 0 .and. cc_ok) call eom_excitations(nel_act, 2*n_act - nel_act)
         if (cfg%eom_ip_nroots > 0 .and. cc_ok) call eom_ipea(AFESP_EOM_IP, cfg%eom_ip_nroots, nel_act, 2*n_act - nel_act)
         if (cfg%eom_ea_nroots > 0 .and. cc_ok) call eom_ipea(AFESP_EOM_EA, cfg%eom_ea_nroots, nel_act, 2*n_act - nel_act)
         if (cfg%cc_polar .and. cc_ok) call polarizability_report(n_act, nel_act/2, nel_act/2, .true.)
         if (cfg%level == LEVEL_CCSD_T .and. cc_ok) then
            ! ---------------- spin-orbital (T) (reference do_ccsd_t_spinorb, src/ccsd.f90:1812-1922)
            t0 = seconds()
            write (out, '(1X, 10("-"))'); write (out, '(1X, A)') 'CCSD(T)'; write (out, '(1X, 10("-"))')
            t_hi = afesp_ccsd_so_t_ntriples(int(nel_act, c_int64_t))     ! i<j<k triples, an even split over the ranks
            t_lo = (int(rank, c_int64_t)*t_hi)/world; t_hi = (int(rank + 1, c_int64_t)*t_hi)/world
            rc = afesp_ccsd_so_t(ctx, t_lo, t_hi, tq(1))
            if (world > 1) then
               ! a rank whose shard failed still enters the sum -- with a flag in it -- so that every rank leaves the collective
               ! and all of them stop together (a rank that stopped before the all-reduce would leave the others in it for ever)
               rc_mine = rc; my_error = ''
               if (rc_mine /= 0) then; my_error = afesp_error_text(ctx); tq(1) = 0.0_dp; end if
               tq(2) = merge(1.0_dp, 0.0_dp, rc_mine /= 0)
               rc = afesp_allreduce_sum(ctx, tq, 2_c_int64_t)
               if (rc_mine /= 0) call fail('ccsd::do_ccsd_t_spinorb', trim(my_error))
               if (rc == 0 .and. tq(2) > 0.5_dp) call fail('ccsd::do_ccsd_t_spinorb', 'the (T) shard of another rank failed')
            end if
            if (rc /= 0) call fail('ccsd::do_ccsd_t_spinorb', afesp_error_text(ctx))
            e_pt = e_ccsd + tq(1)
            e_highest = e_pt
            write (out, '(1X, A, 1X, F15.9)') 'Unrestricted CCSD(T) correlation energy (Hartree):', e_pt
            write (out, '(1X, A, 1X, F16.8, A)') 'Time taken for unrestricted CCSD(T):', seconds() - t0, 's'
         end if
         if (cfg%cc_lambda_t .and. cc_ok) call lambda_triples(nel_act, 'Unrestricted ΛCCSD(T)')
      else if (cfg%level >= LEVEL_CCSD) then
         ! ---------------- CCSD (reference do_ccsd_spatial): the solver loop stays here, one C call per reference call
         t0 = seconds()
         write (out, '(1X, 10("-"))'); write (out, '(1X, A)') 'CCSD'; write (out, '(1X, 10("-"))')
         write (out, '(1X, A)') 'Initialise CC intermediate tensors and DIIS auxilliary arrays...'
         rc = afesp_ccsd_init(ctx, int(o_act, c_int64_t), int(v_act, c_int64_t), c_null_ptr, levels(nfc + 1:), &
                              int(cfg%ccsd_diis_n_errmat, c_int))
         if (rc /= 0) call fail('ccsd::init_cc', afesp_error_text(ctx))
         write (out, '(1X, A, 1X, F8.6, A)') 'Time taken:', seconds() - t0, ' s'
         write (out, *)
         write (out, '(1X, A)') 'Initialisation done, now entering iterative CC solver...'
         rc = afesp_ccsd_energy(ctx, cfg%ccsd_e_tol, cfg%ccsd_t_tol, energy, rms, conv)
         if (rc /= 0) call fail('ccsd::update_cc_energy', afesp_error_text(ctx))
         write (out, '(75("-"))')
         write (out, '(1X, A, 3X, A, 3X, A, 3X, A, 3X, A)') 'Iteration', '     Energy    ', '    deltaE     ', '  delta RMS T2 ', '  Time  '
         write (out, '(75("-"))')
         write (out, '(1X, A9, 3X, F15.12, 3X, F15.12, 3X, F15.12)') 'MP1', energy, energy, rms
         t1s = seconds()
         do iter = 1, cfg%ccsd_maxiter
            eold = energy
            rc = afesp_ccsd_iterate(ctx, cfg%ccsd_e_tol, cfg%ccsd_t_tol, energy, rms, conv)
            if (rc /= 0) call fail('ccsd::update_amplitudes_restricted', afesp_error_text(ctx))
            write (out, '(1X, I9, 3X, F15.12, 3X, F15.12, 3X, F15.12, 3X, F8.6)') iter, energy, energy - eold, rms, seconds() - t1s
            t1s = seconds()
            if (conv /= 0) then
               cc_ok = .true.
               exit
            end if
            rc = afesp_ccsd_diis(ctx)
            if (rc /= 0) call fail('ccsd::update_diis_cc', 'Linear solve failed!')
         end do
         if (cc_ok) then
            allocate (t1(o_act, v_act))
            block
               real(dp), allocatable :: t2(:)
               allocate (t2(int(o_act, i8)**2*int(v_act, i8)**2))
               rc = afesp_ccsd_get_amplitudes(ctx, t1, t2)
            end block
            t1diag = sqrt(sum(t1**2))/sqrt(real(nel_act, dp))   ! (the correlated electrons)
            write (out, '(75("-"))')
            write (out, '(1X, A)') 'Convergence reached within tolerance.'
            write (out, '(1X, A, 1X, F15.12)') 'Final CCSD Energy (Hartree):', energy
            write (out, '(1X, A, 1X, F8.5)') 'T1 diagnostic:', t1diag
            if (t1diag > 0.02_dp) write (out, '(1X, A)') 'Significant multireference character detected, CCSD result might be unreliable!'
            e_ccsd = energy; e_highest = e_ccsd
            if (cfg%comp_renorm) then          ! reference src/ccsd.f90:377-382
               rc = afesp_ccsd_cr_intermediates(ctx)
               if (rc /= 0) call fail('ccsd::build_cr_ccsd_t_intermediates', afesp_error_text(ctx))
            end if
         end if
         write (out, '(1X, A, 1X, F16.8, A)') 'Time taken for restricted CCSD:', seconds() - t0, 's'

         if (cfg%level == LEVEL_CCSD_T .and. cc_ok) then
            ! ---------------- (T) (reference do_ccsd_t_spatial): this rank's shard of the (i<=j<=k) list, then one sum over ranks
            t0 = seconds()
            write (out, '(1X, 10("-"))'); write (out, '(1X, A)') 'CCSD(T)'; write (out, '(1X, 10("-"))')
            ! this rank's shard of the (i<=j<=k) list (the whole list for one rank); the ranks must enumerate the triples in
            ! the same order, i.e. agree on the occupied block size: it rides along in the all-reduce
            allocate (bounds(world + 1))
            rc = afesp_ccsd_t_shard_bounds(ctx, int(o_act, c_int64_t), int(v_act, c_int64_t), &
                                           merge(1_c_int, 0_c_int, cfg%comp_renorm), int(world, c_int), bounds)
            if (rc /= 0) call fail('ccsd::do_ccsd_t_spatial', afesp_error_text(ctx))
            t_lo = bounds(rank + 1); t_hi = bounds(rank + 2)
            if (cfg%comp_renorm) then
               rc = afesp_ccsd_t_cr(ctx, t_lo, t_hi, tq)
            else if (cfg%renorm) then
               rc = afesp_ccsd_t(ctx, t_lo, t_hi, tq(1:4))
            else                               ! plain types: no y, no D sums (reference src/ccsd.f90:2181-2185)
               rc = afesp_ccsd_t_plain(ctx, t_lo, t_hi, tq(1:2))
            end if
            if (world > 1) then                ! the reference's reduction(+: ...) over threads, src/ccsd.f90:2091
               ! Every rank enters the sum, also one whose shard failed: its failure rides along as a flag, so that all ranks
               ! leave the collective and stop together (ncclAllReduce has no time-out: ranks left waiting would wait for ever).
               rc_mine = rc; my_error = ''
               if (rc_mine /= 0) then; my_error = afesp_error_text(ctx); tq = 0.0_dp; end if
               sb = 0
               if (rc_mine == 0) rc_mine = afesp_ccsd_t_block_size(ctx, int(o_act, c_int64_t), int(v_act, c_int64_t), &
                                                                   merge(1_c_int, 0_c_int, cfg%comp_renorm), sb)
               if (rc_mine /= 0 .and. len_trim(my_error) == 0) my_error = afesp_error_text(ctx)
               red(1:6) = tq; red(7) = real(sb, dp); red(8) = real(sb, dp)**2; red(9) = merge(1.0_dp, 0.0_dp, rc_mine /= 0)
               rc = afesp_allreduce_sum(ctx, red, 9_c_int64_t)
               if (rc_mine /= 0) call fail('ccsd::do_ccsd_t_spatial', trim(my_error))
               if (rc == 0 .and. red(9) > 0.5_dp) call fail('ccsd::do_ccsd_t_spatial', 'the (T) shard of another rank failed')
               if (rc == 0 .and. abs(red(8)*world - red(7)**2) > 0.5_dp) &
                  call fail('ccsd::do_ccsd_t_spatial', 'the ranks enumerate the triples in different block sizes (unequal devices or AFESP_T_* settings)')
               tq = red(1:6)
            end if
            if (rc /= 0) call fail('ccsd::do_ccsd_t_spatial', afesp_error_text(ctx))
            ! The reference's plain CCSD(T)_spatial never fills z3_bar (src/ccsd.f90:2211-2215) and therefore prints
            ! E[T] on its "CCSD(T)" line.  AFESP_T_COMPAT=1 reproduces that printout; the default prints the (T) value
            ! the reference itself produces in its R/CR modes.
            call get_environment_variable('AFESP_T_COMPAT', envval)
            compat = (trim(envval) == '1') .and. .not. (cfg%renorm .or. cfg%comp_renorm)
            e_bt = e_ccsd + tq(1)
            e_pt = e_ccsd + merge(tq(1), tq(2), compat)
            e_highest = e_bt
            if (cfg%paren) e_highest = e_pt
            calcname = merge('CCSD(T)', 'CCSD[T]', cfg%paren)
            if (cfg%renorm .or. cfg%comp_renorm) then
               e_rbt = e_ccsd + tq(1)/tq(3)
               e_rpt = e_ccsd + tq(2)/tq(4)
               e_highest = merge(e_rpt, e_rbt, cfg%paren)
            end if
            if (cfg%comp_renorm) then          ! reference src/ccsd.f90:2267-2274
               e_crbt = e_ccsd + tq(5)/tq(3)
               e_crpt = e_ccsd + tq(6)/tq(4)
               e_highest = merge(e_crpt, e_crbt, cfg%paren)
            end if
            if (cfg%renorm) calcname = 'renormalised '//trim(calcname)
            if (cfg%comp_renorm) calcname = 'completely renormalised '//trim(calcname)
            write (out, '(1X, A, 1X, F15.9)') 'Restricted '//trim(calcname)//' correlation energy (Hartree):', e_highest
            write (out, '(1X, A, 1X, F16.8, A)') 'Time taken for restricted '//trim(calcname)//':', seconds() - t0, 's'
         end if
      end if
   else if (scf_ok) then
      e_highest = 0.0_dp
   end if
   if (have_ctx) then
      if (world > 1) rc = afesp_comm_destroy(ctx)
      call afesp_ctx_destroy(ctx)
   end if

   ! ---------------- final table: same labels and formats as the reference (src/main.F90:123-175)
   write (out, '(1X, 64("="))')
   write (out, '(1X, A)') 'Final energy breakdown'
   if (cfg%rohf) then
   write (out, '(1X, A, 1X, F15.10)') 'ROHF reference energy:         ', e_hf + mol%e_nuc
   if (cfg%level >= LEVEL_MP2) then
      write (out, '(1X, A, 1X, F15.10)') 'ROHF-MBPT(2) correlation energy:', e_mp2
      write (out, '(1X, A, 1X, F15.10)') 'ROHF-MBPT(2) energy:           ', e_mp2 + e_hf + mol%e_nuc
   end if
   if (cfg%level >= LEVEL_CCSD) then
      write (out, '(1X, A, 1X, F15.10)') 'ROHF-CCSD correlation energy:  ', e_ccsd
      write (out, '(1X, A, 1X, F15.10)') 'ROHF-CCSD energy:              ', e_ccsd + e_hf + mol%e_nuc
   end if
   if (cfg%level == LEVEL_CCSD_T) then
      write (out, '(1X, A, 1X, F15.10)') 'ROHF-CCSD(T) correlation energy:', e_pt
      write (out, '(1X, A, 1X, F15.10)') 'ROHF-CCSD(T) energy:           ', e_pt + e_hf + mol%e_nuc
   end if
   if (cfg%cc_lambda_t) then
      write (out, '(1X, A, 1X, F15.10)') 'ROHF-ΛCCSD(T) correlation energy:', e_ccsd + e_lt
      write (out, '(1X, A, 1X, F15.10)') 'ROHF-ΛCCSD(T) energy:          ', e_ccsd + e_lt + e_hf + mol%e_nuc
   end if
   else if (cfg%uhf) then
   write (out, '(1X, A, 1X, F15.10)') 'UHF energy:                    ', e_hf + mol%e_nuc
   if (.not. cfg%fcidump_in) write (out, '(1X, A, 1X, F15.10)') '<S^2>:                         ', s2
   if (cfg%level >= LEVEL_MP2) then
      write (out, '(1X, A, 1X, F15.10)') 'UMP2 correlation energy:       ', e_mp2
      write (out, '(1X, A, 1X, F15.10)') 'UMP2 energy:                   ', e_mp2 + e_hf + mol%e_nuc
   end if
   if (cfg%level >= LEVEL_CCSD) then
      write (out, '(1X, A, 1X, F15.10)') 'UCCSD correlation energy:      ', e_ccsd
      write (out, '(1X, A, 1X, F15.10)') 'UCCSD energy:                  ', e_ccsd + e_hf + mol%e_nuc
   end if
   if (cfg%level == LEVEL_CCSD_T) then
      write (out, '(1X, A, 1X, F15.10)') 'UCCSD(T) correlation energy:   ', e_pt
      write (out, '(1X, A, 1X, F15.10)') 'UCCSD(T) energy:               ', e_pt + e_hf + mol%e_nuc
   end if
   if (cfg%cc_lambda_t) then
      write (out, '(1X, A, 1X, F15.10)') 'UΛCCSD(T) correlation energy:  ', e_ccsd + e_lt
      write (out, '(1X, A, 1X, F15.10)') 'UΛCCSD(T) energy:              ', e_ccsd + e_lt + e_hf + mol%e_nuc
   end if
   else
   write (out, '(1X, A, 1X, F15.10)') 'RHF energy:                    ', e_hf + mol%e_nuc
   if (cfg%level >= LEVEL_MP2) then
      write (out, '(1X, A, 1X, F15.10)') 'MP2 correlation energy:        ', e_mp2
      write (out, '(1X, A, 1X, F15.10)') 'MP2 energy:                    ', e_mp2 + e_hf + mol%e_nuc
   end if
   if (cfg%level >= LEVEL_CCSD) then
      write (out, '(1X, A, 1X, F15.10)') 'CCSD correlation energy:       ', e_ccsd
      write (out, '(1X, A, 1X, F15.10)') 'CCSD energy:                   ', e_ccsd + e_hf + mol%e_nuc
   end if
   if (cfg%cc_lambda_t) then
      write (out, '(1X, A, 1X, F15.10)') 'ΛCCSD(T) correlation energy:   ', e_ccsd + e_lt
      write (out, '(1X, A, 1X, F15.10)') 'ΛCCSD(T) energy:               ', e_ccsd + e_lt + e_hf + mol%e_nuc
   end if
   if (cfg%level == LEVEL_CCSD_T .and. cfg%spinorb) then        ! reference src/main.F90:156-158
      write (out, '(1X, A, 1X, F15.10)') 'CCSD(T) correlation energy:    ', e_pt
      write (out, '(1X, A, 1X, F15.10)') 'CCSD(T) energy:                ', e_pt + e_hf + mol%e_nuc
   else if (cfg%level == LEVEL_CCSD_T) then
      write (out, '(1X, A, 1X, F15.10)') 'CCSD[T] correlation energy:    ', e_bt
      write (out, '(1X, A, 1X, F15.10)') 'CCSD[T] energy:                ', e_bt + e_hf + mol%e_nuc
      if (cfg%paren) then
         write (out, '(1X, A, 1X, F15.10)') 'CCSD(T) correlation energy:    ', e_pt
         write (out, '(1X, A, 1X, F15.10)') 'CCSD(T) energy:                ', e_pt + e_hf + mol%e_nuc
      end if
      if (cfg%renorm .or. cfg%comp_renorm) then
         write (out, '(1X, A, 1X, F15.10)') 'R-CCSD[T] correlation energy:  ', e_rbt
         write (out, '(1X, A, 1X, F15.10)') 'R-CCSD[T] energy:              ', e_rbt + e_hf + mol%e_nuc
         if (cfg%paren) then
            write (out, '(1X, A, 1X, F15.10)') 'R-CCSD(T) correlation energy:  ', e_rpt
            write (out, '(1X, A, 1X, F15.10)') 'R-CCSD(T) energy:              ', e_rpt + e_hf + mol%e_nuc
         end if
         if (cfg%comp_renorm) then
            write (out, '(1X, A, 1X, F15.10)') 'CR-CCSD[T] correlation energy: ', e_crbt
            write (out, '(1X, A, 1X, F15.10)') 'CR-CCSD[T] energy:             ', e_crbt + e_hf + mol%e_nuc
            if (cfg%paren) then
               write (out, '(1X, A, 1X, F15.10)') 'CR-CCSD(T) correlation energy: ', e_crpt
               write (out, '(1X, A, 1X, F15.10)') 'CR-CCSD(T) energy:             ', e_crpt + e_hf + mol%e_nuc
            end if
         end if
      end if
   end if
   if (cfg%level >= LEVEL_CCSD .and. .not. cfg%spinorb) then    ! reference src/main.F90:162
      write (out, '(1X, 47("-"))')
      write (out, '(1X, A, 1X, F15.10)') 'T1 diagnostic:                 ', t1diag
   end if
   if (cfg%renorm .or. cfg%comp_renorm) then
      write (out, '(1X, A, 1X, F15.10)') 'D[T]:                          ', tq(3)
      if (cfg%paren) write (out, '(1X, A, 1X, F15.10)') 'D(T):                          ', tq(4)
   end if
   end if
   if (fno .and. cfg%level >= LEVEL_CCSD) then   ! the truncated virtual space corrected by what MP2 lost in it
      write (out, '(1X, 47("-"))')
      write (out, '(1X, A, 1X, F15.10)') 'Delta MP2 (full - FNO space):  ', delta_mp2
      write (out, '(1X, A, 1X, F15.10)') 'CCSD + Delta MP2 correlation:  ', e_ccsd + delta_mp2
      if (cfg%level == LEVEL_CCSD_T) write (out, '(1X, A, 1X, F15.10)') 'Final + Delta MP2 correlation: ', e_highest + delta_mp2
   end if
   write (out, '(1X, 47("-"))')
   write (out, '(1X, A, 1X, F15.10)') 'Total electronic energy:       ', e_hf + e_highest
   write (out, '(1X, A, 1X, F15.10)') 'Nuclear repulsion:             ', mol%e_nuc
   write (out, '(1X, A, 1X, F15.10)') 'Total energy:                  ', e_hf + e_highest + mol%e_nuc
   write (out, '(1X, 64("="))')
   write (out, '(1X, A, 1X, F16.8)') 'Total execution time:', seconds() - tstart
contains
   !> the cut in one spin's occupations: the count asked for, or every occupation >= fno_occ_tol
   function fno_count(occ) result(k)
      real(dp), intent(in) :: occ(:)
      integer :: k
      if (cfg%fno_n_virt >= 0) then
         k = cfg%fno_n_virt
      else
         k = count(occ >= cfg%fno_occ_tol)
      end if
   end function
   !> Lambda of the converged spin-orbital CCSD state: Jacobi steps with DIIS, the CCSD table's format.  One solve serves cc_density,
   !> cc_lambda_t and the EOM sectors (which borrow its H-bar elements).
   subroutine lambda_solve()
      real(dp) :: pe, pe_old, lrms
      integer(c_int) :: lconv
      integer :: it
      logical :: ok
      write (out, '(1X, 10("-"))'); write (out, '(1X, A)') 'CCSD Lambda'; write (out, '(1X, 10("-"))')
      rc = afesp_ccsd_so_lambda_init(ctx, int(cfg%ccsd_diis_n_errmat, c_int))
      if (rc /= 0) call fail('ccsd::init_lambda', afesp_error_text(ctx))
      rc = afesp_ccsd_so_lambda_energy(ctx, cfg%ccsd_e_tol, cfg%ccsd_t_tol, pe, lrms, lconv)
      if (rc /= 0) call fail('ccsd::update_lambda_energy', afesp_error_text(ctx))
      write (out, '(75("-"))')
      write (out, '(1X, A, 3X, A, 3X, A, 3X, A, 3X, A)') 'Iteration', ' Pseudo energy ', '    deltaE     ', '  delta RMS L2 ', '  Time  '
      write (out, '(75("-"))')
      write (out, '(1X, A9, 3X, F15.12, 3X, F15.12, 3X, F15.12)') 'L = T', pe, pe, lrms
      ok = .false.
      t1s = seconds()
      do it = 1, cfg%ccsd_maxiter
         pe_old = pe
         rc = afesp_ccsd_so_lambda_iterate(ctx, cfg%ccsd_e_tol, cfg%ccsd_t_tol, pe, lrms, lconv)
         if (rc /= 0) call fail('ccsd::update_lambda', afesp_error_text(ctx))
         write (out, '(1X, I9, 3X, F15.12, 3X, F15.12, 3X, F15.12, 3X, F8.6)') it, pe, pe - pe_old, lrms, seconds() - t1s
         t1s = seconds()
         if (lconv /= 0) then
            ok = .true.
            exit
         end if
         rc = afesp_ccsd_so_lambda_diis(ctx)
         if (rc /= 0) call fail('ccsd::update_diis_cc', 'Linear solve failed!')
      end do
      write (out, '(75("-"))')
      if (.not. ok) call fail('ccsd::do_lambda', 'the Lambda equations did not converge!')
      write (out, '(1X, A)') 'Convergence reached within tolerance.'
      lambda_live = .true.
   end subroutine
   !> cc_lambda_t: Lambda-CCSD(T) of the converged state and its converged Lambda -- this rank's shard of the i<j<k list, then the flagged
   !> sum over the ranks of the (T) branches.
   subroutine lambda_triples(nel_so, label)
      integer, intent(in) :: nel_so
      character(*), intent(in) :: label
      real(dp) :: lq(2), tl
      integer(c_int64_t) :: l_lo, l_hi
      integer(c_int) :: lrc_mine
      character(512) :: l_error
      tl = seconds()
      write (out, '(1X, 10("-"))'); write (out, '(1X, A)') 'Lambda-CCSD(T)'; write (out, '(1X, 10("-"))')
      l_hi = afesp_ccsd_so_t_ntriples(int(nel_so, c_int64_t))
      l_lo = (int(rank, c_int64_t)*l_hi)/world; l_hi = (int(rank + 1, c_int64_t)*l_hi)/world
      lq = 0.0_dp
      rc = afesp_ccsd_so_lambda_t(ctx, l_lo, l_hi, lq(1))
      if (world > 1) then   ! (every rank enters the sum, a failed shard as a flag: as in the (T) branches)
         lrc_mine = rc; l_error = ''
         if (lrc_mine /= 0) then; l_error = afesp_error_text(ctx); lq(1) = 0.0_dp; end if
         lq(2) = merge(1.0_dp, 0.0_dp, lrc_mine /= 0)
         rc = afesp_allreduce_sum(ctx, lq, 2_c_int64_t)
         if (lrc_mine /= 0) call fail('ccsd::do_lambda_ccsd_t', trim(l_error))
         if (rc == 0 .and. lq(2) > 0.5_dp) call fail('ccsd::do_lambda_ccsd_t', 'the Lambda-(T) shard of another rank failed')
      end if
      if (rc /= 0) call fail('ccsd::do_lambda_ccsd_t', afesp_error_text(ctx))
      e_lt = lq(1)
      if (cfg%rohf) then   ! (the formats of the (T) lines of the same branch)
         write (out, '(1X, A, 1X, F18.12)') 'E(ΛCCSD(T)) correction (Hartree):', e_lt
         write (out, '(1X, A, 1X, F18.12)') label//' correlation energy (Hartree):', e_ccsd + e_lt
      else
         write (out, '(1X, A, 1X, F15.9)') 'E(ΛCCSD(T)) correction (Hartree):', e_lt
         write (out, '(1X, A, 1X, F15.9)') label//' correlation energy (Hartree):', e_ccsd + e_lt
      end if
      write (out, '(1X, A, 1X, F16.8, A)') 'Time taken for Lambda-CCSD(T):', seconds() - tl, 's'
   end subroutine
   !> orbital (within the whole basis: the window starts behind nfc) and spin of every spin orbital of a state over n active orbitals
   subroutine spin_orbital_map(n, nalpha, nbeta, interleaved, orb, spin)
      integer, intent(in) :: n, nalpha, nbeta
      logical, intent(in) :: interleaved
      integer, intent(out) :: orb(:), spin(:)
      integer :: x, o
      o = nalpha + nbeta
      do x = 1, 2*n
         if (interleaved) then
            orb(x) = (x + 1)/2; spin(x) = mod(x + 1, 2)
         else if (x <= nalpha) then
            orb(x) = x; spin(x) = 0
         else if (x <= o) then
            orb(x) = x - nalpha; spin(x) = 1
         else if (x <= o + n - nalpha) then
            orb(x) = nalpha + (x - o); spin(x) = 0
         else
            orb(x) = nbeta + (x - o - (n - nalpha)); spin(x) = 1
         end if
         orb(x) = orb(x) + nfc
      end do
   end subroutine
   !> cc_density: Lambda of the converged spin-orbital CCSD state (Jacobi steps with DIIS, the CCSD table's format), then the spin-summed
   !> natural occupation numbers of the unrelaxed one-particle density over the whole basis (frozen core orbitals doubly occupied, dropped
   !> virtuals empty).  The state's spin-orbital order over its n active orbitals is interleaved (2 P + spin: the RHF-fed state) or blocked
   !> (occupied alpha, occupied beta, virtual alpha, virtual beta).
   subroutine lambda_and_occupations(n, nalpha, nbeta, interleaved)
      integer, intent(in) :: n, nalpha, nbeta
      logical, intent(in) :: interleaved
      real(dp), allocatable :: d(:, :), ds(:, :), dsb(:, :), occ(:), u(:, :)
      integer, allocatable :: orb(:), spin(:)
      real(dp) :: tl
      integer :: x, y, o, nf
      tl = seconds()
      call lambda_solve()
      nf = mol%nbasis
      allocate (d(2*n, 2*n), ds(nf, nf), dsb(nf, nf), orb(2*n), spin(2*n))
      rc = afesp_ccsd_so_density(ctx, d, int(size(d), c_int64_t))
      if (rc /= 0) call fail('ccsd::density', afesp_error_text(ctx))
      o = nalpha + nbeta
      call spin_orbital_map(n, nalpha, nbeta, interleaved, orb, spin)
      ! each spin's density in its own orbitals: the frozen core and the reference determinant on the diagonal, then the correlation part
      ! (which has no element between the spins); the beta one is brought into the alpha orbitals before the two are added
      ds = 0.0_dp; dsb = 0.0_dp
      do x = 1, nfc
         ds(x, x) = 1.0_dp; dsb(x, x) = 1.0_dp
      end do
      do y = 1, 2*n
         do x = 1, 2*n
            if (spin(x) /= spin(y)) cycle
            if (spin(x) == 0) then
               ds(orb(x), orb(y)) = ds(orb(x), orb(y)) + d(x, y)
            else
               dsb(orb(x), orb(y)) = dsb(orb(x), orb(y)) + d(x, y)
            end if
         end do
         if (y <= o .and. spin(y) == 0) ds(orb(y), orb(y)) = ds(orb(y), orb(y)) + 1.0_dp
         if (y <= o .and. spin(y) == 1) dsb(orb(y), orb(y)) = dsb(orb(y), orb(y)) + 1.0_dp
      end do
      if (allocated(ab_overlap)) then
         ds = ds + matmul(transpose(ab_overlap), matmul(dsb, ab_overlap))
      else
         ds = ds + dsb
      end if
      ds = 0.5_dp*(ds + transpose(ds))
      call fno_occupations(ds, occ, u)
      write (out, '(1X, A)') 'Natural occupation numbers (unrelaxed CCSD one-particle density, spin-summed):'
      write (out, '(5(1X, F14.10))') occ
      write (out, '(1X, A, 1X, F14.10)') 'Sum of natural occupation numbers:', sum(occ)
      write (out, '(1X, A, 1X, F16.8, A)') 'Time taken for CCSD Lambda and density:', seconds() - tl, 's'
   end subroutine
   !> cc_rdm2: the two-particle density of the converged state and its converged Lambda (one solve serves cc_density, cc_lambda_t and the EOM
   !> sectors too), the density-side correlation energy sum f D + 1/4 sum g Gamma beside E(CCSD), and <S^2> = N/2 + Ms^2 - sum_PQ
   !> Gtot[P beta, Q alpha, Q beta, P alpha] of the reference determinant and of CCSD (unrelaxed).  The correlation part of the sum is the
   !> library's expectation value with the spin-flip overlaps as its two matrices; the reference and one-particle parts are one-body algebra
   !> over the frozen core (doubly occupied, uncorrelated) and the state's spin orbitals.
   subroutine rdm2_energy_and_spin(n, nalpha, nbeta, interleaved)
      integer, intent(in) :: n, nalpha, nbeta
      logical, intent(in) :: interleaved
      real(dp), allocatable :: d(:, :), dx(:, :), g0(:, :), a(:, :)
      integer, allocatable :: orb(:), spin(:), orbx(:), spinx(:)
      real(dp) :: tl, e8(8), corr, flips_ref, flips, ms, nel
      integer :: x, y, o, m, c2
      tl = seconds()
      if (.not. lambda_live) call lambda_solve()
      rc = afesp_ccsd_so_density2_build(ctx)
      if (rc /= 0) call fail('ccsd::density2', afesp_error_text(ctx))
      rc = afesp_ccsd_so_density2_energy(ctx, e8)
      if (rc /= 0) call fail('ccsd::density2_energy', afesp_error_text(ctx))
      write (out, '(1X, A, 1X, F15.12)') 'Density-side CCSD correlation energy (Hartree):', e8(1) + e8(8)
      write (out, '(1X, A, 1X, ES10.3)') 'Difference to E(CCSD) (Hartree):', e8(1) + e8(8) - e_ccsd
      o = nalpha + nbeta; c2 = 2*nfc; m = c2 + 2*n
      allocate (d(2*n, 2*n), dx(m, m), g0(m, m), a(m, m), orb(2*n), spin(2*n), orbx(m), spinx(m))
      rc = afesp_ccsd_so_density(ctx, d, int(size(d), c_int64_t))
      if (rc /= 0) call fail('ccsd::density', afesp_error_text(ctx))
      call spin_orbital_map(n, nalpha, nbeta, interleaved, orb, spin)
      do x = 1, nfc   ! the frozen core in front: alpha, then beta
         orbx(x) = x; spinx(x) = 0; orbx(nfc + x) = x; spinx(nfc + x) = 1
      end do
      orbx(c2 + 1:) = orb; spinx(c2 + 1:) = spin
      dx = 0.0_dp; g0 = 0.0_dp; a = 0.0_dp
      dx(c2 + 1:, c2 + 1:) = d
      do x = 1, c2 + o
         g0(x, x) = 1.0_dp
      end do
      do y = 1, m   ! a(x beta, y alpha) = <beta orbital of x | alpha orbital of y>
         do x = 1, m
            if (spinx(x) /= 1 .or. spinx(y) /= 0) cycle
            if (allocated(ab_overlap)) then
               a(x, y) = ab_overlap(orbx(x), orbx(y))
            else if (orbx(x) == orbx(y)) then
               a(x, y) = 1.0_dp
            end if
         end do
      end do
      ! Gamma_pqrs S_ps S_rq = -Gamma_pqsr S_ps S_rq: A_pr B_qs with A the (beta, alpha) overlap over the state's spin orbitals, B = A^T
      rc = afesp_ccsd_so_density2_expect(ctx, a(c2 + 1:, c2 + 1:), transpose(a(c2 + 1:, c2 + 1:)), corr)
      if (rc /= 0) call fail('ccsd::density2_expect', afesp_error_text(ctx))
      flips_ref = flip_pair(g0, g0, a)
      flips = flips_ref + flip_pair(dx, g0, a) + flip_pair(g0, dx, a) - corr
      nel = real(c2 + o, dp); ms = 0.5_dp*real(nalpha - nbeta, dp)
      write (out, '(1X, A, 1X, F14.10)') '<S^2> of the reference determinant:', 0.5_dp*nel + ms*ms - flips_ref
      write (out, '(1X, A, 1X, F14.10)') '<S^2> of CCSD (unrelaxed two-particle density):', 0.5_dp*nel + ms*ms - flips
      write (out, '(1X, A, 1X, F16.8, A)') 'Time taken for the CCSD two-particle density:', seconds() - tl, 's'
   end subroutine
   !> cc_relaxed: the orbital-relaxed one-particle density of the converged state (DESIGN.md 4.18).  Shares the one Lambda solve; builds the
   !> two-particle density of the current t and lambda, solves the Z-vector equations on the device and prints the iteration count, the
   !> residual and the largest |z|, the natural occupation numbers of the relaxed density and -- when t.dat and v.dat were read -- <T> and
   !> <V_ne> of the unrelaxed and of the relaxed density.  No orbital window (refused with the key): the state's orbitals are all of them.
   subroutine relaxed_density_report(n, nalpha, nbeta, interleaved)
      integer, intent(in) :: n, nalpha, nbeta
      logical, intent(in) :: interleaved
      real(dp), allocatable :: d(:, :), z(:), da(:, :), db(:, :), ds(:, :), occ(:), u(:, :), ta(:, :), tb(:, :), va(:, :), vb(:, :)
      integer, allocatable :: orb(:), spin(:)
      integer(c_int) :: zit
      real(dp) :: tl, zres, ex(2, 2)
      integer :: x, y, o, pass
      tl = seconds()
      if (.not. lambda_live) call lambda_solve()
      rc = afesp_ccsd_so_density2_build(ctx)
      if (rc /= 0) call fail('ccsd::density2', afesp_error_text(ctx))
      o = nalpha + nbeta
      allocate (d(2*n, 2*n), z(o*(2*n - o)), da(n, n), db(n, n), orb(2*n), spin(2*n))
      rc = afesp_ccsd_so_zvector_solve(ctx, 1.0e-10_dp, 100_c_int, z, zit, zres)
      if (rc /= 0) call fail('ccsd::zvector', afesp_error_text(ctx))
      write (out, '(1X, A, 1X, I0)') 'Z-vector iterations:', zit
      write (out, '(1X, A, 1X, ES10.3)') 'Z-vector residual norm:', zres
      write (out, '(1X, A, 1X, ES14.7)') 'Largest |z|:', maxval(abs(z))
      call spin_orbital_map(n, nalpha, nbeta, interleaved, orb, spin)
      if (allocated(mol%ke)) then
         ta = matmul(coeff, matmul(mol%ke, transpose(coeff))); va = matmul(coeff, matmul(mol%en, transpose(coeff)))
         if (cfg%uhf) then
            tb = matmul(cb, matmul(mol%ke, transpose(cb))); vb = matmul(cb, matmul(mol%en, transpose(cb)))
         else
            tb = ta; vb = va
         end if
      end if
      do pass = 1, 2   ! the unrelaxed density, then the relaxed one
         if (pass == 1) then
            rc = afesp_ccsd_so_density(ctx, d, int(size(d), c_int64_t))
         else
            rc = afesp_ccsd_so_relaxed_density(ctx, d, int(size(d), c_int64_t))
         end if
         if (rc /= 0) call fail('ccsd::relaxed_density', afesp_error_text(ctx))
         da = 0.0_dp; db = 0.0_dp   ! each spin's density in its own orbitals, the reference determinant on the diagonal
         do y = 1, 2*n
            do x = 1, 2*n
               if (spin(x) /= spin(y)) cycle
               if (spin(x) == 0) then
                  da(orb(x), orb(y)) = da(orb(x), orb(y)) + d(x, y)
               else
                  db(orb(x), orb(y)) = db(orb(x), orb(y)) + d(x, y)
               end if
            end do
            if (y <= o .and. spin(y) == 0) da(orb(y), orb(y)) = da(orb(y), orb(y)) + 1.0_dp
            if (y <= o .and. spin(y) == 1) db(orb(y), orb(y)) = db(orb(y), orb(y)) + 1.0_dp
         end do
         if (allocated(mol%ke)) then
            ex(1, pass) = sum(da*ta) + sum(db*tb); ex(2, pass) = sum(da*va) + sum(db*vb)
         end if
         if (pass == 1) cycle
         if (allocated(ab_overlap)) then
            ds = da + matmul(transpose(ab_overlap), matmul(db, ab_overlap))
         else
            ds = da + db
         end if
         ds = 0.5_dp*(ds + transpose(ds))
         call fno_occupations(ds, occ, u)
         write (out, '(1X, A)') 'Natural occupation numbers (relaxed CCSD one-particle density, spin-summed):'
         write (out, '(5(1X, F14.10))') occ
         write (out, '(1X, A, 1X, F14.10)') 'Sum of relaxed natural occupation numbers:', sum(occ)
      end do
      if (allocated(mol%ke)) then
         write (out, '(1X, A, 1X, F16.8)') '<T> (unrelaxed CCSD density, Hartree):', ex(1, 1)
         write (out, '(1X, A, 1X, F16.8)') '<T> (relaxed CCSD density, Hartree):', ex(1, 2)
         write (out, '(1X, A, 1X, F16.8)') '<V_ne> (unrelaxed CCSD density, Hartree):', ex(2, 1)
         write (out, '(1X, A, 1X, F16.8)') '<V_ne> (relaxed CCSD density, Hartree):', ex(2, 2)
      end if
      write (out, '(1X, A, 1X, F16.8, A)') 'Time taken for the relaxed CCSD density:', seconds() - tl, 's'
   end subroutine
   !> cc_polar: the EOM-CCSD polarisability alpha(omega) = -<<mu;mu>>_omega of the converged state (DESIGN.md 4.19).  The three operators
   !> are read from dipx.dat / dipy.dat / dipz.dat (AO basis, the format of t.dat) and transformed with the SCF coefficients as
   !> cc_relaxed transforms T and V_ne; Lambda is the one solve shared with cc_density, cc_lambda_t and the EOM sectors; all right-hand
   !> sides (3 operators x +-omega, every frequency) share one basis.  Prints one 3 x 3 table per frequency with the isotropic mean and the
   !> anisotropy, the sigma builds and the largest residual.
   subroutine polarizability_report(n, nalpha, nbeta, interleaved)
      integer, intent(in) :: n, nalpha, nbeta
      logical, intent(in) :: interleaved
      character(8), parameter :: files(3) = ['dipx.dat', 'dipy.dat', 'dipz.dat']
      real(dp), parameter :: polar_tol = 1.0e-8_dp
      real(dp), allocatable :: ao(:, :), ma(:, :), mb(:, :), xso(:, :, :), signed(:), res(:), rf(:, :, :, :)
      integer, allocatable :: orb(:), spin(:)
      integer(c_int) :: nsig, pconv
      integer(c_int64_t) :: o8, v8, nunique
      real(dp) :: tp, alpha(3, 3), sym(3, 3), mean, aniso
      integer :: c, x, y, f, ns, nb_ao, ms, it, nsys
      logical :: there, ok
      tp = seconds()
      write (out, '(1X, 10("-"))'); write (out, '(1X, A)') 'EOM-CCSD polarisability'; write (out, '(1X, 10("-"))')
      allocate (orb(2*n), spin(2*n), xso(2*n, 2*n, 3))
      call spin_orbital_map(n, nalpha, nbeta, interleaved, orb, spin)
      do c = 1, 3
         inquire (file=files(c), exist=there)
         if (.not. there) call fail('polar::read_operators', 'operator file '//files(c)//' does not exist')
         nb_ao = mol%nbasis
         if (allocated(ao)) deallocate (ao)
         call read_two_index(files(c), ao, nb_ao)
         ma = matmul(coeff, matmul(ao, transpose(coeff)))
         if (cfg%uhf) then
            mb = matmul(cb, matmul(ao, transpose(cb)))
         else
            mb = ma
         end if
         do y = 1, 2*n
            do x = 1, 2*n
               if (spin(x) /= spin(y)) then
                  xso(x, y, c) = 0.0_dp
               else if (spin(x) == 0) then
                  xso(x, y, c) = 0.5_dp*(ma(orb(x), orb(y)) + ma(orb(y), orb(x)))
               else
                  xso(x, y, c) = 0.5_dp*(mb(orb(x), orb(y)) + mb(orb(y), orb(x)))
               end if
            end do
         end do
      end do
      if (.not. lambda_live) call lambda_solve()
      if (cfg%polar_gamma > 0.0_dp) then   ! damped response: every frequency at omega + i gamma (DESIGN.md 4.20)
         call polar_damped_table(xso, nalpha + nbeta, 2*n - nalpha - nbeta)
         if (cfg%polar_c6_npts > 0) call polar_c6_table(xso, nalpha + nbeta, 2*n - nalpha - nbeta)
         write (out, '(1X, A, 1X, F16.8, A)') 'Time taken for the EOM-CCSD polarisability:', seconds() - tp, 's'
         return
      end if
      ! the signed list: +omega and -omega of every frequency, each value once
      allocate (signed(2*cfg%n_polar_omega)); ns = 0
      do f = 1, cfg%n_polar_omega
         do c = 1, -1, -2
            if (.not. any(signed(:ns) == c*cfg%polar_omega(f))) then
               ns = ns + 1; signed(ns) = c*cfg%polar_omega(f) + 0.0_dp
            end if
         end do
      end do
      nsys = 3*ns
      o8 = int(nalpha + nbeta, c_int64_t); v8 = int(2*n - nalpha - nbeta, c_int64_t)
      nunique = o8*v8 + (o8*(o8 - 1)/2)*(v8*(v8 - 1)/2)
      ms = min(4096, max(2*nsys, int(min(nunique, int(8*nsys, c_int64_t)))))
      rc = afesp_ccsd_so_response_init(ctx, 3_c_int, xso, int(ns, c_int), signed, int(ms, c_int))
      if (rc /= 0) call fail('polar::init_response', afesp_error_text(ctx))
      allocate (res(nsys), rf(3, 3, cfg%n_polar_omega, 1))
      ok = .false.
      do it = 1, 100
         rc = afesp_ccsd_so_response_iterate(ctx, polar_tol, res, nsig, pconv)
         if (rc /= 0) call fail('polar::iterate', afesp_error_text(ctx))
         if (pconv /= 0) then
            ok = .true.
            exit
         end if
      end do
      if (.not. ok) call fail('polar::do_response', 'the response equations did not converge!')
      rc = afesp_ccsd_so_response_function(ctx, int(cfg%n_polar_omega, c_int), cfg%polar_omega, rf)
      if (rc /= 0) call fail('polar::response_function', afesp_error_text(ctx))
      do f = 1, cfg%n_polar_omega
         alpha = -transpose(rf(:, :, f, 1))   ! (the library's rows are the first operator: out[(f nop + a) nop + b])
         sym = 0.5_dp*(alpha + transpose(alpha))
         mean = (sym(1, 1) + sym(2, 2) + sym(3, 3))/3.0_dp
         aniso = sqrt(0.5_dp*((sym(1, 1) - sym(2, 2))**2 + (sym(2, 2) - sym(3, 3))**2 + (sym(3, 3) - sym(1, 1))**2) &
                      + 3.0_dp*(sym(1, 2)**2 + sym(2, 3)**2 + sym(3, 1)**2))
         write (out, '(2X, A, F14.8, A)') 'omega = ', cfg%polar_omega(f), ' Eh'
         do c = 1, 3
            write (out, '(4X, A1, 2X, 3F18.10)') 'xyz'(c:c), alpha(c, :)
         end do
         write (out, '(4X, A, F18.10, 3X, A, F18.10)') 'mean ', mean, 'anisotropy ', aniso
      end do
      write (out, '(2X, A, I0, 3X, A, ES11.3)') 'response sigma builds: ', nsig, 'largest residual: ', maxval(res)
      if (cfg%polar_c6_npts > 0) call polar_c6_table(xso, nalpha + nbeta, 2*n - nalpha - nbeta)
      write (out, '(1X, A, 1X, F16.8, A)') 'Time taken for the EOM-CCSD polarisability:', seconds() - tp, 's'
   end subroutine
   !> alpha(z) = -<<mu;mu>>_z of the three operators xso at the nz complex frequencies z(1:2, :) = (re, im): the signed list (z, and -z
   !> where Re z /= 0 -- for an imaginary z its partner is its own conjugate --, each value once), one response state on one real basis,
   !> the steps, the function.  alpha(a, b, f) = (re, im) in alpha(1:2, a, b, f).
   subroutine polar_complex_solve(xso, o, v, nz, z, alpha, nsig, maxres)
      real(dp), intent(in) :: xso(:, :, :), z(:, :)
      integer, intent(in) :: o, v, nz
      real(dp), intent(out) :: alpha(:, :, :, :), maxres
      integer(c_int), intent(out) :: nsig
      real(dp), parameter :: polar_tol = 1.0e-8_dp
      real(dp), allocatable :: signed(:, :), res(:), rf(:, :, :, :)
      integer(c_int) :: pconv
      integer(c_int64_t) :: o8, v8, nunique
      integer :: f, c, g, ns, nsys, ms, it, a, b
      logical :: ok, seen
      real(dp) :: cand(2)
      allocate (signed(2, 2*nz)); ns = 0
      do f = 1, nz
         do c = 1, -1, -2
            if (c == -1 .and. z(1, f) == 0.0_dp) cycle
            cand = c*z(:, f) + 0.0_dp
            seen = .false.
            do g = 1, ns
               if (signed(1, g) == cand(1) .and. signed(2, g) == cand(2)) seen = .true.
            end do
            if (.not. seen) then
               ns = ns + 1; signed(:, ns) = cand
            end if
         end do
      end do
      nsys = 3*ns
      if (nsys > 64) call fail('polar::init_response', 'more than 64 response systems: fewer frequencies or grid points!')
      o8 = int(o, c_int64_t); v8 = int(v, c_int64_t)
      nunique = o8*v8 + (o8*(o8 - 1)/2)*(v8*(v8 - 1)/2)
      ms = min(4096, max(4*nsys, int(min(nunique + int(2*nsys, c_int64_t), int(16*nsys, c_int64_t)))))
      rc = afesp_ccsd_so_response_init_complex(ctx, 3_c_int, xso, int(ns, c_int), signed, int(ms, c_int))
      if (rc /= 0) call fail('polar::init_response', afesp_error_text(ctx))
      allocate (res(nsys), rf(2, 3, 3, nz))
      ok = .false.
      do it = 1, 100
         rc = afesp_ccsd_so_response_iterate(ctx, polar_tol, res, nsig, pconv)
         if (rc /= 0) call fail('polar::iterate', afesp_error_text(ctx))
         if (pconv /= 0) then
            ok = .true.
            exit
         end if
      end do
      if (.not. ok) call fail('polar::do_response', 'the response equations did not converge!')
      rc = afesp_ccsd_so_response_function_complex(ctx, int(nz, c_int), z, rf)
      if (rc /= 0) call fail('polar::response_function', afesp_error_text(ctx))
      do f = 1, nz
         do b = 1, 3
            do a = 1, 3
               alpha(:, a, b, f) = -rf(:, b, a, f)   ! (the library's rows are the first operator: out[2 ((f nop + a) nop + b)])
            end do
         end do
      end do
      maxres = maxval(res)
   end subroutine
   !> polar_gamma > 0: per frequency the real and the imaginary 3 x 3 table of alpha(omega + i gamma), Re and Im of the isotropic mean and
   !> the absorption cross-section sigma(omega) = 4 pi omega / c Im mean (atomic units)
   subroutine polar_damped_table(xso, o, v)
      real(dp), intent(in) :: xso(:, :, :)
      integer, intent(in) :: o, v
      real(dp), parameter :: light_speed = 137.035999084_dp, pi = 3.14159265358979323846_dp
      real(dp), allocatable :: z(:, :), alpha(:, :, :, :)
      integer(c_int) :: nsig
      real(dp) :: maxres, mean(2)
      integer :: f, c, part, nf
      nf = cfg%n_polar_omega
      allocate (z(2, nf), alpha(2, 3, 3, nf))
      z(1, :) = cfg%polar_omega(:nf); z(2, :) = cfg%polar_gamma
      call polar_complex_solve(xso, o, v, nf, z, alpha, nsig, maxres)
      do f = 1, nf
         write (out, '(2X, A, F14.8, A, F14.8, A)') 'omega = ', z(1, f), ' Eh   gamma = ', z(2, f), ' Eh'
         do part = 1, 2
            do c = 1, 3
               write (out, '(4X, A2, 1X, A1, 2X, 3F18.10)') merge('Re', 'Im', part == 1), 'xyz'(c:c), alpha(part, c, :, f)
            end do
         end do
         mean = (alpha(:, 1, 1, f) + alpha(:, 2, 2, f) + alpha(:, 3, 3, f))/3.0_dp
         write (out, '(4X, A, F18.10, 3X, A, F18.10, 3X, A, F18.10)') 'Re mean ', mean(1), 'Im mean ', mean(2), &
            'sigma ', 4.0_dp*pi*z(1, f)/light_speed*mean(2)
      end do
      write (out, '(2X, A, I0, 3X, A, ES11.3)') 'response sigma builds: ', nsig, 'largest residual: ', maxres
   end subroutine
   !> polar_c6_npts > 0: the isotropic mean at i u_k on the Gauss-Legendre grid t_k in (-1, 1) mapped by u = u0 (1 + t) / (1 - t), weights
   !> w_k 2 u0 / (1 - t_k)^2, u0 = 0.3, and the homo-dimer C6 = (3 / pi) sum_k weight_k mean(i u_k)^2.  One solve per grid point (the
   !> partner of an imaginary frequency is its own conjugate), all points in one response state.
   subroutine polar_c6_table(xso, o, v)
      real(dp), intent(in) :: xso(:, :, :)
      integer, intent(in) :: o, v
      real(dp), parameter :: u0 = 0.3_dp, pi = 3.14159265358979323846_dp
      real(dp), allocatable :: t(:), w(:), z(:, :), alpha(:, :, :, :), mean(:)
      integer(c_int) :: nsig
      real(dp) :: maxres, c6
      integer :: k, np
      np = cfg%polar_c6_npts
      allocate (t(np), w(np), z(2, np), alpha(2, 3, 3, np), mean(np))
      call gauss_legendre(np, t, w)
      z(1, :) = 0.0_dp; z(2, :) = u0*(1.0_dp + t)/(1.0_dp - t)
      w = w*2.0_dp*u0/(1.0_dp - t)**2
      call polar_complex_solve(xso, o, v, np, z, alpha, nsig, maxres)
      write (out, '(2X, A, I0, A, F10.6)') 'Casimir-Polder grid: ', np, ' points, u0 = ', u0
      c6 = 0.0_dp
      do k = 1, np
         mean(k) = (alpha(1, 1, 1, k) + alpha(1, 2, 2, k) + alpha(1, 3, 3, k))/3.0_dp
         write (out, '(4X, A, I3, 3X, A, F18.10, 3X, A, F18.10, 3X, A, F18.10)') 'point', k, 'u ', z(2, k), 'weight ', w(k), 'mean(iu) ', mean(k)
         c6 = c6 + w(k)*mean(k)**2
      end do
      c6 = 3.0_dp/pi*c6
      write (out, '(2X, A, F18.10)') 'C6 (homo-dimer) = ', c6
      write (out, '(2X, A, I0, 3X, A, ES11.3)') 'C6 response sigma builds: ', nsig, 'largest residual: ', maxres
   end subroutine
   !> nodes (ascending) and weights of the n-point Gauss-Legendre rule on (-1, 1): Newton's iteration on P_n from the Chebyshev guess
   subroutine gauss_legendre(n, t, w)
      integer, intent(in) :: n
      real(dp), intent(out) :: t(n), w(n)
      real(dp), parameter :: pi = 3.14159265358979323846_dp
      real(dp) :: x, p0, p1, p2, dp1, dx
      integer :: i, j, it
      do i = 1, n
         x = -cos(pi*(real(i, dp) - 0.25_dp)/(real(n, dp) + 0.5_dp))
         do it = 1, 100
            p0 = 1.0_dp; p1 = x
            do j = 2, n
               p2 = (real(2*j - 1, dp)*x*p1 - real(j - 1, dp)*p0)/real(j, dp)
               p0 = p1; p1 = p2
            end do
            dp1 = real(n, dp)*(x*p1 - p0)/(x*x - 1.0_dp)
            dx = p1/dp1
            x = x - dx
            if (abs(dx) < 1.0e-15_dp) exit
         end do
         p0 = 1.0_dp; p1 = x
         do j = 2, n
            p2 = (real(2*j - 1, dp)*x*p1 - real(j - 1, dp)*p0)/real(j, dp)
            p0 = p1; p1 = p2
         end do
         dp1 = real(n, dp)*(x*p1 - p0)/(x*x - 1.0_dp)
         t(i) = x
         w(i) = 2.0_dp/((1.0_dp - x*x)*dp1*dp1)
      end do
   end subroutine
   !> sum over p, r beta and q, s alpha of (x_pr y_qs - x_ps y_qr) S_ps S_rq, S the non-zero (beta, alpha) block of a
   function flip_pair(xm, ym, a) result(val)
      real(dp), intent(in) :: xm(:, :), ym(:, :), a(:, :)
      real(dp) :: val
      real(dp), allocatable :: w(:, :)
      integer :: p
      w = matmul(matmul(xm, a), matmul(ym, transpose(a)))
      val = 0.0_dp
      do p = 1, size(w, 1)
         val = val + w(p, p)
      end do
      val = val - sum(xm*a)*sum(ym*transpose(a))
   end function
   !> eom_nroots: the lowest EOM-EE-CCSD excitation energies of the converged spin-orbital CCSD state (o occupied, v virtual spin orbitals) by
   !> the library's block Davidson iteration.  The H-bar elements are those of the Lambda state: the one cc_density left, else one made here
   !> (Lambda itself is not iterated).  The spin-orbital space holds every Ms component: a triplet appears threefold.
   subroutine eom_excitations(o, v)
      integer, intent(in) :: o, v
      real(dp), parameter :: hartree_ev = 27.211386245988_dp, eom_tol = 1.0e-8_dp
      real(dp), allocatable :: omega(:), res(:), x1(:), x2(:), w1(:), omega_l(:), res_l(:)
      integer(c_int), allocatable :: flags(:), flags_l(:)
      integer(c_int) :: nsig, econv
      integer :: nr, ms, it, k
      integer(c_int64_t) :: o8, v8, nunique   ! (o^2 v^2 and the pair counts leave 32 bits long before the state leaves the device)
      real(dp) :: te
      logical :: ok
      te = seconds()
      write (out, '(1X, 10("-"))'); write (out, '(1X, A)') 'EOM-CCSD'; write (out, '(1X, 10("-"))')
      nr = cfg%eom_nroots
      o8 = int(o, c_int64_t); v8 = int(v, c_int64_t)
      nunique = o8*v8 + (o8*(o8 - 1)/2)*(v8*(v8 - 1)/2)
      ms = max(2*nr, int(min(nunique, int(8*nr, c_int64_t))))
      if (.not. lambda_live) then
         rc = afesp_ccsd_so_lambda_init(ctx, 0_c_int)
         if (rc /= 0) call fail('eom::init_hbar', afesp_error_text(ctx))
      end if
      rc = afesp_ccsd_so_eom_init(ctx, int(nr, c_int), int(ms, c_int))
      if (rc /= 0) call fail('eom::init_eom', afesp_error_text(ctx))
      rc = afesp_ccsd_so_eom_guess(ctx)
      if (rc /= 0) call fail('eom::guess', afesp_error_text(ctx))
      allocate (omega(nr), res(nr), flags(nr), w1(nr), x1(o8*v8), x2(o8*o8*v8*v8))
      ok = .false.
      do it = 1, 100
         rc = afesp_ccsd_so_eom_iterate(ctx, eom_tol, omega, res, flags, nsig, econv)
         if (rc /= 0) call fail('eom::davidson_step', afesp_error_text(ctx))
         if (econv /= 0) then
            ok = .true.
            exit
         end if
      end do
      if (.not. ok) call fail('eom::do_eom', 'the EOM-CCSD Davidson iteration did not converge!')
      do k = 1, nr
         rc = afesp_ccsd_so_eom_get_vector(ctx, int(k - 1, c_int), x1, x2)
         if (rc /= 0) call fail('eom::get_vector', afesp_error_text(ctx))
         w1(k) = sum(x1*x1)
      end do
      write (out, '(1X, A, 1X, I0, A, I0, A, I0, A)') 'Davidson steps:', it, ', sigma builds: ', nsig, ', at most ', ms, ' basis vectors'
      write (out, '(75("-"))')
      write (out, '(1X, A, 3X, A, 3X, A, 3X, A, 3X, A)') 'Root', '  omega (Hartree) ', '    omega (eV)    ', '  |r1|^2  ', ' Residual '
      write (out, '(75("-"))')
      do k = 1, nr
         if (iand(flags(k), 2_c_int) /= 0) then
            write (out, '(1X, I4, 3X, F18.12, 3X, F18.10, 3X, F10.8, 3X, ES10.3, 1X, A)') k, omega(k), omega(k)*hartree_ev, w1(k), res(k), 'complex'
         else
            write (out, '(1X, I4, 3X, F18.12, 3X, F18.10, 3X, F10.8, 3X, ES10.3)') k, omega(k), omega(k)*hartree_ev, w1(k), res(k)
         end if
      end do
      write (out, '(75("-"))')
      ! eom_left: the left eigenvectors of the same roots on a Davidson state of its own, from the right vectors as guess
      if (cfg%eom_left) then
         rc = afesp_ccsd_so_eom_left_init(ctx, int(nr, c_int), int(ms, c_int))
         if (rc /= 0) call fail('eom::init_left', afesp_error_text(ctx))
         do k = 1, nr
            rc = afesp_ccsd_so_eom_get_vector(ctx, int(k - 1, c_int), x1, x2)
            if (rc /= 0) call fail('eom::get_vector', afesp_error_text(ctx))
            rc = afesp_ccsd_so_eom_left_set_guess(ctx, int(k - 1, c_int), x1, x2)
            if (rc /= 0) call fail('eom::left_guess', afesp_error_text(ctx))
         end do
         allocate (omega_l(nr), res_l(nr), flags_l(nr))
         ok = .false.
         do it = 1, 100
            rc = afesp_ccsd_so_eom_left_iterate(ctx, eom_tol, omega_l, res_l, flags_l, nsig, econv)
            if (rc /= 0) call fail('eom::left_davidson_step', afesp_error_text(ctx))
            if (econv /= 0) then
               ok = .true.
               exit
            end if
         end do
         if (.not. ok) call fail('eom::do_eom_left', 'the left EOM-CCSD Davidson iteration did not converge!')
         write (out, '(1X, A, 1X, I0, A, I0)') 'Left eigenvectors: Davidson steps:', it, ', sigma builds: ', nsig
         write (out, '(75("-"))')
         write (out, '(1X, A, 3X, A, 3X, A, 3X, A, 3X, A)') 'Root', 'omega left (Eh)   ', ' omega left (eV)  ', '|left-right|', ' Residual '
         write (out, '(75("-"))')
         do k = 1, nr
            write (out, '(1X, I4, 3X, F18.12, 3X, F18.10, 3X, ES12.3, 3X, ES10.3)') k, omega_l(k), omega_l(k)*hartree_ev, &
               abs(omega_l(k) - omega(k)), res_l(k)
         end do
         write (out, '(75("-"))')
         if (cfg%eom_triples) call eom_triples_report(o, v, nr, omega)
      end if
      write (out, '(1X, A, 1X, F16.8, A)') 'Time taken for EOM-CCSD:', seconds() - te, 's'
   end subroutine
   !> eom_triples: the non-iterative triples correction to the nr roots just solved.  The left vectors are biorthonormalised against the
   !> right ones inside every cluster of degenerate roots (S^-1 L, S_jk = <L_j, R_k> = sum l1 r1 + 1/4 sum l2 r2), all roots go to the
   !> library in one call on this rank's shard of the i<j<k list, and the shards are summed as in the (T) branches.  A root whose omega
   !> comes within 0.05 Eh (a diagnostic constant) of the smallest triples denominator is flagged.
   subroutine eom_triples_report(o, v, nr, omega)
      integer, intent(in) :: o, v, nr
      real(dp), intent(in) :: omega(:)
      real(dp), parameter :: hartree_ev = 27.211386245988_dp, intruder_gap = 0.05_dp, degeneracy_tol = 1.0e-6_dp
      real(dp), allocatable :: r1(:, :), r2(:, :), l1(:, :), l2(:, :), b1(:, :), b2(:, :), s(:, :), si(:, :), red(:), d1(:, :), eo(:), ev(:)
      integer, allocatable :: order(:)
      integer :: k, j, a, b, c0, c1, nc, piv
      integer(c_int64_t) :: n1, n2, t_lo, t_hi
      integer(c_int) :: rc_mine
      character(512) :: my_error
      real(dp) :: tt, lowest, f, gap
      tt = seconds()
      n1 = int(o, c_int64_t)*v; n2 = n1*n1
      allocate (r1(n1, nr), r2(n2, nr), l1(n1, nr), l2(n2, nr), b1(n1, nr), b2(n2, nr), order(nr), red(nr + 1))
      do k = 1, nr
         rc = afesp_ccsd_so_eom_get_vector(ctx, int(k - 1, c_int), r1(:, k), r2(:, k))
         if (rc /= 0) call fail('eom::get_vector', afesp_error_text(ctx))
         rc = afesp_ccsd_so_eom_left_get_vector(ctx, int(k - 1, c_int), l1(:, k), l2(:, k))
         if (rc /= 0) call fail('eom::left_get_vector', afesp_error_text(ctx))
      end do
      ! roots in ascending order, clusters of neighbours within degeneracy_tol
      do k = 1, nr
         order(k) = k
      end do
      do k = 2, nr
         j = k
         do while (j > 1)
            if (omega(order(j - 1)) <= omega(order(j))) exit
            a = order(j); order(j) = order(j - 1); order(j - 1) = a
            j = j - 1
         end do
      end do
      c0 = 1
      do while (c0 <= nr)
         c1 = c0
         do while (c1 < nr)
            if (abs(omega(order(c1 + 1)) - omega(order(c1))) >= degeneracy_tol) exit
            c1 = c1 + 1
         end do
         nc = c1 - c0 + 1
         allocate (s(nc, nc), si(nc, nc))
         do a = 1, nc
            do b = 1, nc
               s(a, b) = sum(l1(:, order(c0 + a - 1))*r1(:, order(c0 + b - 1))) + 0.25_dp*sum(l2(:, order(c0 + a - 1))*r2(:, order(c0 + b - 1)))
            end do
         end do
         ! si = s^-1 by Gauss-Jordan elimination with row pivoting
         si = 0.0_dp
         do a = 1, nc
            si(a, a) = 1.0_dp
         end do
         do a = 1, nc
            piv = a
            do b = a + 1, nc
               if (abs(s(b, a)) > abs(s(piv, a))) piv = b
            end do
            if (abs(s(piv, a)) < 1.0e-8_dp) call fail('eom::biorthonormalise', &
               'the overlap of the left and right vectors of a cluster of roots is singular: the two solves found different states!')
            if (piv /= a) then
               s([a, piv], :) = s([piv, a], :); si([a, piv], :) = si([piv, a], :)
            end if
            f = 1.0_dp/s(a, a)
            s(a, :) = s(a, :)*f; si(a, :) = si(a, :)*f
            do b = 1, nc
               if (b /= a) then
                  f = s(b, a)
                  s(b, :) = s(b, :) - f*s(a, :); si(b, :) = si(b, :) - f*si(a, :)
               end if
            end do
         end do
         do a = 1, nc
            b1(:, order(c0 + a - 1)) = 0.0_dp; b2(:, order(c0 + a - 1)) = 0.0_dp
            do b = 1, nc
               b1(:, order(c0 + a - 1)) = b1(:, order(c0 + a - 1)) + si(a, b)*l1(:, order(c0 + b - 1))
               b2(:, order(c0 + a - 1)) = b2(:, order(c0 + a - 1)) + si(a, b)*l2(:, order(c0 + b - 1))
            end do
         end do
         deallocate (s, si)
         c0 = c1 + 1
      end do
      ! one call for all roots on this rank's shard, then the flagged sum over the ranks
      t_hi = afesp_ccsd_so_t_ntriples(int(o, c_int64_t))
      t_lo = (int(rank, c_int64_t)*t_hi)/world; t_hi = (int(rank + 1, c_int64_t)*t_hi)/world
      red = 0.0_dp
      rc = afesp_ccsd_so_eom_t(ctx, int(nr, c_int), omega, b1, b2, r1, r2, t_lo, t_hi, red)
      if (world > 1) then
         rc_mine = rc; my_error = ''
         if (rc_mine /= 0) then; my_error = afesp_error_text(ctx); red = 0.0_dp; end if
         red(nr + 1) = merge(1.0_dp, 0.0_dp, rc_mine /= 0)
         rc = afesp_allreduce_sum(ctx, red, int(nr + 1, c_int64_t))
         if (rc_mine /= 0) call fail('eom::do_eom_triples', trim(my_error))
         if (rc == 0 .and. red(nr + 1) > 0.5_dp) call fail('eom::do_eom_triples', 'the triples shard of another rank failed')
      end if
      if (rc /= 0) call fail('eom::do_eom_triples', afesp_error_text(ctx))
      ! the smallest triples denominator from the levels: the three highest occupied and the three lowest virtual ones
      lowest = huge(1.0_dp)
      if (o >= 3 .and. v >= 3) then
         allocate (d1(o, v), eo(o), ev(v))
         rc = afesp_ccsd_so_get_tensor(ctx, 'D1'//c_null_char, d1, n1)
         if (rc /= 0) call fail('eom::levels', afesp_error_text(ctx))
         eo = d1(:, 1); ev = d1(1, 1) - d1(1, :)      ! the levels relative to the first virtual one
         lowest = 0.0_dp
         do k = 1, 3
            a = maxloc(eo, 1); lowest = lowest - eo(a); eo(a) = -huge(1.0_dp)
            a = minloc(ev, 1); lowest = lowest + ev(a); ev(a) = huge(1.0_dp)
         end do
      end if
      write (out, '(1X, A)') 'Non-iterative triples correction to the EOM-CCSD excitation energies'
      write (out, '(100("-"))')
      write (out, '(1X, A, 3X, A, 3X, A, 3X, A, 3X, A)') 'Root', '   omega (Eh)     ', 'delta omega (Eh)  ', ' omega+delta (Eh) ', ' omega+delta (eV) '
      write (out, '(100("-"))')
      do k = 1, nr
         write (out, '(1X, I4, 3X, F18.12, 3X, F18.12, 3X, F18.12, 3X, F18.10)') k, omega(k), red(k), omega(k) + red(k), (omega(k) + red(k))*hartree_ev
      end do
      write (out, '(100("-"))')
      do k = 1, nr
         gap = abs(omega(k) - lowest)
         if (gap < intruder_gap) write (out, '(1X, A, I0, A, F8.4, A)') 'Root ', k, ': omega is within ', gap, &
            ' Eh of a triples denominator: the correction is not reliable'
      end do
      write (out, '(1X, A, 1X, F16.8, A)') 'Time taken for the EOM-CCSD triples correction:', seconds() - tt, 's'
   end subroutine
   !> eom_ip_nroots / eom_ea_nroots: the lowest EOM-IP-CCSD ionisation potentials (1h + 2h1p) or EOM-EA-CCSD electron affinities (1p + 2p1h) of the
   !> converged spin-orbital CCSD state, after Lambda and EOM-EE where those were asked for.  The H-bar elements are those of the Lambda
   !> state they left, else of one made here.  Nothing is filtered: a closed-shell reference shows every doublet twofold.
   subroutine eom_ipea(sector, nr, o, v)
      integer(c_int), intent(in) :: sector
      integer, intent(in) :: nr, o, v
      real(dp), parameter :: hartree_ev = 27.211386245988_dp, eom_tol = 1.0e-8_dp
      real(dp), allocatable :: omega(:), res(:), x1(:), x2(:), w1(:)
      integer(c_int), allocatable :: flags(:)
      integer(c_int) :: nsig, econv
      integer :: ms, it, k
      integer(c_int64_t) :: o8, v8, nunique, n1, n2
      real(dp) :: te
      logical :: ok
      character(6) :: what
      te = seconds()
      what = merge('EOM-IP', 'EOM-EA', sector == AFESP_EOM_IP)
      write (out, '(1X, 11("-"))'); write (out, '(1X, A)') what//'-CCSD'; write (out, '(1X, 11("-"))')
      o8 = int(o, c_int64_t); v8 = int(v, c_int64_t)
      if (sector == AFESP_EOM_IP) then
         n1 = o8; n2 = o8*o8*v8; nunique = o8 + (o8*(o8 - 1)/2)*v8
      else
         n1 = v8; n2 = o8*v8*v8; nunique = v8 + o8*(v8*(v8 - 1)/2)
      end if
      ms = max(2*nr, int(min(nunique, int(8*nr, c_int64_t))))
      if (.not. lambda_live .and. cfg%eom_nroots <= 0 .and. .not. (sector == AFESP_EOM_EA .and. cfg%eom_ip_nroots > 0)) then
         rc = afesp_ccsd_so_lambda_init(ctx, 0_c_int)
         if (rc /= 0) call fail('eom_ipea::init_hbar', afesp_error_text(ctx))
      end if
      rc = afesp_ccsd_so_eom_ipea_init(ctx, sector, int(nr, c_int), int(ms, c_int))
      if (rc /= 0) call fail('eom_ipea::init_eom', afesp_error_text(ctx))
      rc = afesp_ccsd_so_eom_ipea_guess(ctx, sector)
      if (rc /= 0) call fail('eom_ipea::guess', afesp_error_text(ctx))
      allocate (omega(nr), res(nr), flags(nr), w1(nr), x1(n1), x2(n2))
      ok = .false.
      do it = 1, 100
         rc = afesp_ccsd_so_eom_ipea_iterate(ctx, sector, eom_tol, omega, res, flags, nsig, econv)
         if (rc /= 0) call fail('eom_ipea::davidson_step', afesp_error_text(ctx))
         if (econv /= 0) then
            ok = .true.
            exit
         end if
      end do
      if (.not. ok) call fail('eom_ipea::do_eom', 'the '//what//'-CCSD Davidson iteration did not converge!')
      do k = 1, nr
         rc = afesp_ccsd_so_eom_ipea_get_vector(ctx, sector, int(k - 1, c_int), x1, x2)
         if (rc /= 0) call fail('eom_ipea::get_vector', afesp_error_text(ctx))
         w1(k) = sum(x1*x1)
      end do
      write (out, '(1X, A, 1X, I0, A, I0, A, I0, A)') 'Davidson steps:', it, ', sigma builds: ', nsig, ', at most ', ms, ' basis vectors'
      write (out, '(75("-"))')
      write (out, '(1X, A, 3X, A, 3X, A, 3X, A, 3X, A)') 'Root', '  omega (Hartree) ', '    omega (eV)    ', '  |r1|^2  ', ' Residual '
      write (out, '(75("-"))')
      do k = 1, nr
         if (iand(flags(k), 2_c_int) /= 0) then
            write (out, '(1X, I4, 3X, F18.12, 3X, F18.10, 3X, F10.8, 3X, ES10.3, 1X, A)') k, omega(k), omega(k)*hartree_ev, w1(k), res(k), 'complex'
         else
            write (out, '(1X, I4, 3X, F18.12, 3X, F18.10, 3X, F10.8, 3X, ES10.3)') k, omega(k), omega(k)*hartree_ev, w1(k), res(k)
         end if
      end do
      write (out, '(75("-"))')
      if (cfg%eom_ipea_left) call eom_ipea_left_report(sector, what, nr, ms, int(o + v), n1, n2, omega)
      write (out, '(1X, A, 1X, F16.8, A)') 'Time taken for '//what//'-CCSD:', seconds() - te, 's'
   end subroutine
   !> eom_ipea_left: the left eigenvectors of the nr roots just solved, on a Davidson state of its own from the right vectors as guess,
   !> biorthonormalised against the right ones inside every cluster of degenerate roots (S^-1 L, S_jk = <L_j, R_k> = sum l1 r1 +
   !> 1/2 sum l2 r2: every doublet of a closed-shell reference is a twofold cluster; roots with one and the same right vector are one state),
   !> and the pole strengths sum_p gamma_L(p) gamma_R(p) of
   !> the Dyson vectors, with the converged Lambda the main program solved before the sector.
   subroutine eom_ipea_left_report(sector, what, nr, ms, nso, n1, n2, omega)
      integer(c_int), intent(in) :: sector
      character(6), intent(in) :: what
      integer, intent(in) :: nr, ms, nso
      integer(c_int64_t), intent(in) :: n1, n2
      real(dp), intent(in) :: omega(:)
      real(dp), parameter :: hartree_ev = 27.211386245988_dp, eom_tol = 1.0e-8_dp, degeneracy_tol = 1.0e-6_dp
      real(dp), allocatable, target :: r1(:, :), r2(:, :), b1(:, :), b2(:, :), dl(:, :), dr(:, :)
      real(dp), allocatable :: l1(:, :), l2(:, :), omega_l(:), res_l(:), s(:, :), si(:, :)
      integer(c_int), allocatable :: flags_l(:)
      integer, allocatable :: order(:), owner(:), st(:)
      integer(c_int) :: nsig, econv
      integer :: it, k, j, a, b, c0, c1, nc, piv
      real(dp) :: f
      logical :: ok
      allocate (r1(n1, nr), r2(n2, nr), l1(n1, nr), l2(n2, nr), b1(n1, nr), b2(n2, nr), dl(nso, nr), dr(nso, nr), order(nr), owner(nr), st(nr))
      allocate (omega_l(nr), res_l(nr), flags_l(nr))
      rc = afesp_ccsd_so_eom_ipea_left_init(ctx, sector, int(nr, c_int), int(ms, c_int))
      if (rc /= 0) call fail('eom_ipea::init_left', afesp_error_text(ctx))
      do k = 1, nr
         rc = afesp_ccsd_so_eom_ipea_get_vector(ctx, sector, int(k - 1, c_int), r1(:, k), r2(:, k))
         if (rc /= 0) call fail('eom_ipea::get_vector', afesp_error_text(ctx))
         rc = afesp_ccsd_so_eom_ipea_left_set_guess(ctx, sector, int(k - 1, c_int), r1(:, k), r2(:, k))
         if (rc /= 0) call fail('eom_ipea::left_guess', afesp_error_text(ctx))
      end do
      ok = .false.
      do it = 1, 100
         rc = afesp_ccsd_so_eom_ipea_left_iterate(ctx, sector, eom_tol, omega_l, res_l, flags_l, nsig, econv)
         if (rc /= 0) call fail('eom_ipea::left_davidson_step', afesp_error_text(ctx))
         if (econv /= 0) then
            ok = .true.
            exit
         end if
      end do
      if (.not. ok) call fail('eom_ipea::do_eom_left', 'the left '//what//'-CCSD Davidson iteration did not converge!')
      do k = 1, nr
         rc = afesp_ccsd_so_eom_ipea_left_get_vector(ctx, sector, int(k - 1, c_int), l1(:, k), l2(:, k))
         if (rc /= 0) call fail('eom_ipea::left_get_vector', afesp_error_text(ctx))
      end do
      ! roots in ascending order, clusters of neighbours within degeneracy_tol
      do k = 1, nr
         order(k) = k
      end do
      do k = 2, nr
         j = k
         do while (j > 1)
            if (omega(order(j - 1)) <= omega(order(j))) exit
            a = order(j); order(j) = order(j - 1); order(j - 1) = a
            j = j - 1
         end do
      end do
      c0 = 1
      do while (c0 <= nr)
         c1 = c0
         do while (c1 < nr)
            if (abs(omega(order(c1 + 1)) - omega(order(c1))) >= degeneracy_tol) exit
            c1 = c1 + 1
         end do
         ! the distinct states of the cluster: roots whose right vectors are equal to the bit are one state (the library gives both members
         ! of a pair that rounding split into omega +- i epsilon the pair's one real vector); st(1 .. nc) are the states' first roots
         nc = 0
         do k = c0, c1
            owner(order(k)) = order(k)
            do a = 1, nc
               if (all(r1(:, order(k)) == r1(:, st(a))) .and. all(r2(:, order(k)) == r2(:, st(a)))) owner(order(k)) = st(a)
            end do
            if (owner(order(k)) == order(k)) then
               nc = nc + 1; st(nc) = order(k)
            end if
         end do
         allocate (s(nc, nc), si(nc, nc))
         do a = 1, nc
            do b = 1, nc
               s(a, b) = sum(l1(:, st(a))*r1(:, st(b))) + 0.5_dp*sum(l2(:, st(a))*r2(:, st(b)))
            end do
         end do
         ! si = s^-1 by Gauss-Jordan elimination with partial pivoting (clusters are multiplets: a few roots)
         si = 0.0_dp
         do a = 1, nc
            si(a, a) = 1.0_dp
         end do
         do a = 1, nc
            piv = a
            do b = a + 1, nc
               if (abs(s(b, a)) > abs(s(piv, a))) piv = b
            end do
            if (abs(s(piv, a)) < 1.0e-8_dp) call fail('eom_ipea::biorthonormalise', &
               'the overlap of the left and right vectors of a cluster of degenerate roots is singular: the two solves found different states!')
            if (piv /= a) then
               s([a, piv], :) = s([piv, a], :); si([a, piv], :) = si([piv, a], :)
            end if
            f = 1.0_dp/s(a, a)
            s(a, :) = f*s(a, :); si(a, :) = f*si(a, :)
            do b = 1, nc
               if (b /= a) then
                  f = s(b, a)
                  s(b, :) = s(b, :) - f*s(a, :); si(b, :) = si(b, :) - f*si(a, :)
               end if
            end do
         end do
         do a = 1, nc
            b1(:, st(a)) = 0.0_dp; b2(:, st(a)) = 0.0_dp
            do b = 1, nc
               b1(:, st(a)) = b1(:, st(a)) + si(a, b)*l1(:, st(b))
               b2(:, st(a)) = b2(:, st(a)) + si(a, b)*l2(:, st(b))
            end do
         end do
         do k = c0, c1
            if (owner(order(k)) /= order(k)) then
               b1(:, order(k)) = b1(:, owner(order(k))); b2(:, order(k)) = b2(:, owner(order(k)))
            end if
         end do
         deallocate (s, si)
         c0 = c1 + 1
      end do
      rc = afesp_ccsd_so_eom_ipea_dyson(ctx, sector, int(nr, c_int), c_loc(b1), c_loc(b2), c_loc(r1), c_loc(r2), c_loc(dl), c_loc(dr))
      if (rc /= 0) call fail('eom_ipea::dyson', afesp_error_text(ctx))
      write (out, '(1X, A, 1X, I0, A, I0)') 'Left eigenvectors: Davidson steps:', it, ', sigma builds: ', nsig
      write (out, '(96("-"))')
      write (out, '(1X, A, 3X, A, 3X, A, 3X, A, 3X, A, 3X, A)') 'Root', 'omega left (Eh)   ', ' omega left (eV)  ', '|left-right|', ' Residual ', &
         '  Pole strength   '
      write (out, '(96("-"))')
      do k = 1, nr
         write (out, '(1X, I4, 3X, F18.12, 3X, F18.10, 3X, ES12.3, 3X, ES10.3, 3X, F18.14)') k, omega_l(k), omega_l(k)*hartree_ev, &
            abs(omega_l(k) - omega(k)), res_l(k), sum(dl(:, k)*dr(:, k))
      end do
      write (out, '(96("-"))')
      if (cfg%eom_ipea_triples) then
         if (sector == AFESP_EOM_IP) then
            call eom_ipea_triples_report(sector, what, nr, int(n1), nso - int(n1), omega, b1, b2, r1, r2)
         else
            call eom_ipea_triples_report(sector, what, nr, nso - int(n1), int(n1), omega, b1, b2, r1, r2)
         end if
      end if
   end subroutine
   !> eom_ipea_triples: the non-iterative triples correction to the nr roots of a sector from the biorthonormal left vectors b1 / b2 and the
   !> right vectors r1 / r2 of eom_ipea_left_report.  All roots go to the library in one call on this rank's shard of the sector's items
   !> (IP: the triples i<j<k; EA: the pairs i<j), and the shards are summed as in the (T) branches.  A root whose omega comes within 0.05 Eh
   !> (a diagnostic constant) of the smallest 3h2p / 3p2h denominator is flagged.
   subroutine eom_ipea_triples_report(sector, what, nr, o, v, omega, b1, b2, r1, r2)
      integer(c_int), intent(in) :: sector
      character(6), intent(in) :: what
      integer, intent(in) :: nr, o, v
      real(dp), intent(in) :: omega(:), b1(:, :), b2(:, :), r1(:, :), r2(:, :)
      real(dp), parameter :: hartree_ev = 27.211386245988_dp, intruder_gap = 0.05_dp
      real(dp), allocatable :: red(:), d1(:, :), eo(:), ev(:)
      integer :: k, a, no, nv
      integer(c_int64_t) :: t_lo, t_hi
      integer(c_int) :: rc_mine
      character(512) :: my_error
      real(dp) :: tt, lowest, gap
      tt = seconds()
      allocate (red(nr + 1))
      ! one call for all roots on this rank's shard, then the flagged sum over the ranks
      t_hi = afesp_ccsd_so_eom_ipea_t_nitems(sector, int(o, c_int))
      t_lo = (int(rank, c_int64_t)*t_hi)/world; t_hi = (int(rank + 1, c_int64_t)*t_hi)/world
      red = 0.0_dp
      rc = afesp_ccsd_so_eom_ipea_t(ctx, sector, int(nr, c_int), omega, b1, b2, r1, r2, t_lo, t_hi, red)
      if (world > 1) then
         rc_mine = rc; my_error = ''
         if (rc_mine /= 0) then; my_error = afesp_error_text(ctx); red = 0.0_dp; end if
         red(nr + 1) = merge(1.0_dp, 0.0_dp, rc_mine /= 0)
         rc = afesp_allreduce_sum(ctx, red, int(nr + 1, c_int64_t))
         if (rc_mine /= 0) call fail('eom_ipea::do_triples', trim(my_error))
         if (rc == 0 .and. red(nr + 1) > 0.5_dp) call fail('eom_ipea::do_triples', 'the triples shard of another rank failed')
      end if
      if (rc /= 0) call fail('eom_ipea::do_triples', afesp_error_text(ctx))
      ! the smallest denominator from the levels: the three (two) highest occupied and the two (three) lowest virtual ones for IP (EA)
      no = merge(3, 2, sector == AFESP_EOM_IP); nv = merge(2, 3, sector == AFESP_EOM_IP)
      lowest = huge(1.0_dp)
      if (o >= no .and. v >= nv) then
         allocate (d1(o + v, 1), eo(o), ev(v))
         rc = afesp_ccsd_so_get_tensor(ctx, 'levels'//c_null_char, d1, int(o + v, c_int64_t))
         if (rc /= 0) call fail('eom_ipea::levels', afesp_error_text(ctx))
         eo = d1(1:o, 1); ev = d1(o + 1:o + v, 1)      ! the levels themselves: 2 - 3 (3 - 2) of them, a common shift does not cancel
         lowest = 0.0_dp
         do k = 1, no
            a = maxloc(eo, 1); lowest = lowest - eo(a); eo(a) = -huge(1.0_dp)
         end do
         do k = 1, nv
            a = minloc(ev, 1); lowest = lowest + ev(a); ev(a) = huge(1.0_dp)
         end do
      end if
      write (out, '(1X, A)') 'Non-iterative triples correction to the '//what//'-CCSD roots'
      write (out, '(100("-"))')
      write (out, '(1X, A, 3X, A, 3X, A, 3X, A, 3X, A)') 'Root', '   omega (Eh)     ', 'delta omega (Eh)  ', ' omega+delta (Eh) ', ' omega+delta (eV) '
      write (out, '(100("-"))')
      do k = 1, nr
         write (out, '(1X, I4, 3X, F18.12, 3X, F18.12, 3X, F18.12, 3X, F18.10)') k, omega(k), red(k), omega(k) + red(k), (omega(k) + red(k))*hartree_ev
      end do
      write (out, '(100("-"))')
      do k = 1, nr
         gap = abs(omega(k) - lowest)
         if (gap < intruder_gap) write (out, '(1X, A, I0, A, F8.4, A)') 'Root ', k, ': omega is within ', gap, &
            ' Eh of a triples denominator: the correction is not reliable'
      end do
      write (out, '(1X, A, 1X, F16.8, A)') 'Time taken for the '//what//'-CCSD triples correction:', seconds() - tt, 's'
   end subroutine
   subroutine print_fno_cut(asked, kept_occ, dropped_occ, any_dropped)
      integer, intent(in) :: asked
      real(dp), intent(in) :: kept_occ, dropped_occ
      logical, intent(in) :: any_dropped
      if (fno_kept == asked) then
         write (out, '(1X, A, 1X, I0)') 'Number of natural virtuals kept:', fno_kept
      else
         write (out, '(1X, A, 1X, I0, A, I0, A)') 'Number of natural virtuals kept:', fno_kept, ' (asked for ', asked, &
            ': degenerate occupations are kept together)'
      end if
      write (out, '(1X, A, 1X, ES15.8)') 'Smallest kept occupation:', kept_occ
      if (any_dropped) write (out, '(1X, A, 1X, ES15.8)') 'Largest discarded occupation:', dropped_occ
   end subroutine
   !> after the window: e_mp2 is the MP2 energy in the FNO space
   subroutine print_fno_energies(what)
      character(*), intent(in) :: what
      delta_mp2 = e_mp2_full - e_mp2
      write (out, '(1X, A, 1X, F15.10)') what//' correlation energy, all virtuals (Hartree):', e_mp2_full
      write (out, '(1X, A, 1X, F15.10)') what//' correlation energy, natural virtuals (Hartree):', e_mp2
      write (out, '(1X, A, 1X, F15.10)') 'Delta MP2 (Hartree):', delta_mp2
   end subroutine
   !> closed shell: the MP2 virtual density of the canonical integrals just transformed, its natural virtuals, the cut, the rotated
   !> coefficients and levels in place of the canonical ones, and the second transform on the AO integrals resident on the device
   !> (its own MP2 energy is not meaningful: Fock is not diagonal between the kept and the discarded block).  Every rank does the
   !> same algebra on the same D: no collective.
   subroutine closed_shell_fno()
      real(dp), allocatable :: d(:, :), occ(:), u(:, :)
      integer :: asked
      real(dp) :: dummy
      write (out, '(1X, A)') 'Forming the MP2 natural virtual orbitals...'
      allocate (d(mol%nvirt, mol%nvirt))
      rc = afesp_mp2_vv_density(ctx, int(mol%nbasis, c_int64_t), int(mol%nocc, c_int64_t), int(nfc, c_int64_t), levels, d, e_mp2_full)
      if (rc /= 0) call fail('mp2::natural_virtuals', afesp_error_text(ctx))
      call fno_occupations(d, occ, u)
      asked = fno_count(occ)
      if (asked < 1) call fail('mp2::natural_virtuals', 'fno_occ_tol leaves no natural virtual orbital')
      fno_kept = fno_widen(occ, asked)
      call print_fno_cut(asked, occ(fno_kept), occ(min(fno_kept + 1, mol%nvirt)), fno_kept < mol%nvirt)
      call fno_rotate(coeff, levels, mol%nocc, u, fno_kept)
      nfv = mol%nvirt - fno_kept
      n_act = mol%nbasis - nfc - nfv; v_act = fno_kept
      rc = afesp_ao2mo_mp2(ctx, int(mol%nbasis, c_int64_t), int(mol%nocc, c_int64_t), coeff, levels, c_null_ptr, c_null_ptr, dummy)
      if (rc /= 0) call fail('mp2::natural_virtuals', afesp_error_text(ctx))
   end subroutine
   !> open shell: both spins' densities and natural virtuals; the window drops the same number of orbitals from both spins, so the count
   !> is taken in the smaller virtual space (a threshold: the larger of the two spins' counts, i.e. the smaller number dropped), and a
   !> degenerate set in either spin moves the cut of both
   subroutine open_shell_fno()
      real(dp), allocatable :: da(:, :), db(:, :), occa(:), occb(:), ua(:, :), ub(:, :)
      integer :: va, vb, asked, drop, new
      real(dp) :: dummy
      write (out, '(1X, A)') 'Forming the MP2 natural virtual orbitals...'
      va = mol%nbasis - na; vb = mol%nbasis - nb; vmin = min(va, vb)
      allocate (da(va, va), db(vb, vb))
      rc = afesp_ump2_vv_density(ctx, int(mol%nbasis, c_int64_t), int(na, c_int64_t), int(nb, c_int64_t), int(nfc, c_int64_t), levels, lb, &
                                 da, db, e_mp2_full)
      if (rc /= 0) call fail('mp2::natural_virtuals', afesp_error_text(ctx))
      call fno_occupations(da, occa, ua)
      call fno_occupations(db, occb, ub)
      if (cfg%fno_n_virt >= 0) then
         asked = cfg%fno_n_virt
      else
         asked = vmin - min(va - fno_count(occa), vb - fno_count(occb))
      end if
      if (asked < 1) call fail('mp2::natural_virtuals', 'fno_occ_tol leaves no natural virtual orbital')
      drop = vmin - asked
      do
         new = min(va - fno_widen(occa, va - drop), vb - fno_widen(occb, vb - drop))
         if (new == drop) exit
         drop = new
      end do
      fno_kept = vmin - drop
      if (va <= vb) then
         call print_fno_cut(asked, occa(va - drop), occa(min(va - drop + 1, va)), drop > 0)
      else
         call print_fno_cut(asked, occb(vb - drop), occb(min(vb - drop + 1, vb)), drop > 0)
      end if
      call fno_rotate(coeff, levels, na, ua, va - drop)
      call fno_rotate(cb, lb, nb, ub, vb - drop)
      nfv = drop
      n_act = mol%nbasis - nfc - nfv
      rc = afesp_ao2mo_ump2(ctx, int(mol%nbasis, c_int64_t), int(na, c_int64_t), int(nb, c_int64_t), coeff, cb, levels, lb, &
                            c_null_ptr, c_null_ptr, c_null_ptr, c_null_ptr, dummy)
      if (rc /= 0) call fail('mp2::natural_virtuals', afesp_error_text(ctx))
   end subroutine
   !> fcidump_in, first half (no device): the header of ./FCIDUMP gives the extents and the electron counts; the calculation type must
   !> match the kind of file.  The core energy of the file holds the nuclear repulsion: e_nuc stays 0 and e_hf is the total energy.
   subroutine scan_input_file()
      integer(c_int64_t) :: norb, nelec, ms2, nl
      integer(c_int) :: file_uhf
      rc = afesp_fcidump_scan('FCIDUMP'//c_null_char, norb, nelec, ms2, file_uhf, nl)
      if (rc /= 0) call fail('integrals::read_fcidump', 'fcidump_in: FCIDUMP is missing, unreadable or has no &FCI ... &END header')
      write (out, '(1X, A, I0, A, I0, A, I0, A, L1, A, I0)') 'FCIDUMP header: NORB ', norb, ', NELEC ', nelec, ', MS2 ', ms2, ', UHF ', &
         file_uhf /= 0, ', lines ', nl
      if (cfg%rohf) then   ! a restricted file with MS2 >= 0 (MS2 = 0: the closed-shell limit)
         if (file_uhf /= 0) call fail('integrals::read_fcidump', &
            'fcidump_in: the file says UHF=.TRUE.: it takes UMP2, UCCSD or UCCSD(T), not '//trim(cfg%calc_type))
         if (ms2 < 0 .or. mod(nelec + ms2, 2_c_int64_t) /= 0) call fail('integrals::read_fcidump', &
            'fcidump_in: '//trim(cfg%calc_type)//' needs a restricted file with MS2 >= 0 of the parity of NELEC')
         mol%e_nuc = 0.0_dp; mol%natoms = 0; mol%ncore = -1
         mol%nel = int(nelec); mol%nbasis = int(norb)
         na = int((nelec + ms2)/2); nb = int((nelec - ms2)/2)
         if (nb < 0 .or. na > mol%nbasis .or. na + nb <= 0 .or. na + nb >= 2*mol%nbasis) &
            call fail('integrals::read_fcidump', 'fcidump_in: NELEC and MS2 do not fit NORB, or leave no virtual spin orbital')
         mol%nocc = nb; mol%nvirt = mol%nbasis - na
         return
      end if
      if (file_uhf /= 0 .and. .not. cfg%uhf) call fail('integrals::read_fcidump', &
         'fcidump_in: the file says UHF=.TRUE.: it takes UMP2, UCCSD or UCCSD(T), not '//trim(cfg%calc_type))
      if (file_uhf == 0 .and. cfg%uhf) call fail('integrals::read_fcidump', &
         'fcidump_in: a closed-shell file takes the _spatial and _spinorb types, not '//trim(cfg%calc_type))
      mol%e_nuc = 0.0_dp; mol%natoms = 0; mol%ncore = -1
      mol%nel = int(nelec)
      if (cfg%uhf) then
         if (mod(norb, 2_c_int64_t) /= 0 .or. mod(nelec + ms2, 2_c_int64_t) /= 0) call fail('integrals::read_fcidump', &
            'fcidump_in: UHF=.TRUE. with an odd NORB, or NELEC and MS2 of different parity')
         mol%nbasis = int(norb/2)
         na = int((nelec + ms2)/2); nb = int((nelec - ms2)/2)
         if (na < 0 .or. nb < 0 .or. na > mol%nbasis .or. nb > mol%nbasis .or. na + nb >= 2*mol%nbasis) &
            call fail('integrals::read_fcidump', 'fcidump_in: NELEC and MS2 do not fit NORB, or leave no virtual spin orbital')
         mol%nocc = nb; mol%nvirt = mol%nbasis - na
      else
         if (ms2 /= 0 .or. mod(nelec, 2_c_int64_t) /= 0) call fail('integrals::read_fcidump', &
            'fcidump_in: an open shell without UHF=.TRUE. (restricted open-shell orbitals are not supported)')
         mol%nbasis = int(norb); mol%nocc = int(nelec/2); mol%nvirt = mol%nbasis - mol%nocc
         if (mol%nocc <= 0 .or. mol%nvirt <= 0) call fail('integrals::read_fcidump', 'fcidump_in: no occupied or no virtual orbital')
      end if
   end subroutine
   !> second half, where the SCF would run: the integrals onto the device (resident as a transform leaves them), the levels = the
   !> diagonal of the Fock operator of the file's determinant, e_hf = that determinant's energy.  The solvers assume canonical
   !> orbitals: the largest off-diagonal Fock element is printed in every run and refused above 1e-6 (a policy value: a file from a
   !> converged SCF lies orders of magnitude below it).
   subroutine read_input_file()
      real(dp), parameter :: canonical_tol = 1e-6_dp
      real(dp) :: e_core_file, offdiag
      real(dp), allocatable, target :: la_t(:), lb_t(:)
      write (out, '(1X, 10("-"))'); write (out, '(1X, A)') 'FCIDUMP'; write (out, '(1X, 10("-"))')
      write (out, '(1X, A)') 'Reading MO integrals from FCIDUMP (no SCF, no AO to MO transformation)...'
      if (cfg%rohf) then
         call read_rohf_file()
         return
      end if
      allocate (la_t(mol%nbasis), lb_t(mol%nbasis))
      if (cfg%uhf) then
         rc = afesp_read_fcidump_uhf(ctx, 'FCIDUMP'//c_null_char, int(mol%nbasis, c_int64_t), int(na, c_int64_t), int(nb, c_int64_t), &
                                     c_null_ptr, c_null_ptr, c_null_ptr, c_null_ptr, c_loc(la_t), c_loc(lb_t), e_core_file, e_hf, &
                                     offdiag, c_null_ptr, c_null_ptr, c_null_ptr, nlines)
      else
         rc = afesp_read_fcidump(ctx, 'FCIDUMP'//c_null_char, int(mol%nbasis, c_int64_t), int(mol%nocc, c_int64_t), c_null_ptr, &
                                 c_null_ptr, c_loc(la_t), e_core_file, e_hf, offdiag, c_null_ptr, nlines)
      end if
      if (rc /= 0) call fail('integrals::read_fcidump', afesp_error_text(ctx))
      allocate (levels(mol%nbasis)); levels = la_t
      if (cfg%uhf) then
         allocate (lb(mol%nbasis)); lb = lb_t
      end if
      s2 = 0.0_dp
      write (out, '(1X, A, I0)') 'Lines read: ', nlines
      write (out, '(1X, A, 1X, F18.10)') 'Core energy of the file (Hartree):', e_core_file
      write (out, '(1X, A, 1X, F18.10)') 'Reference determinant energy (Hartree):', e_hf
      write (out, '(1X, A, 1X, ES10.3)') 'Largest off-diagonal Fock element:', offdiag
      if (.not. offdiag <= canonical_tol) then
         write (my_error, '(A, ES10.3, A, ES8.1, A)') 'fcidump_in: the orbitals of the file are not canonical: max |F(p,q)|, p /= q, is ', &
            offdiag, ', above ', canonical_tol, ' (the solvers assume canonical orbitals)'
         call fail('integrals::read_fcidump', trim(my_error))
      end if
      scf_ok = .true.
      write (out, '(1X, A, 1X, F16.8, A)') 'Time taken for reading the FCIDUMP:', seconds() - t0, 's'
   end subroutine
   !> the ROHF types: the restricted file onto the device, the two spin Fock operators of its determinant, semicanonical orbitals (the
   !> occupied and the virtual block of each spin diagonalised on the host), and the resident integrals rotated into the three blocks of the
   !> open-shell path.  The off-diagonal Fock elements of the file are printed and not judged: such orbitals are not canonical.
   subroutine read_rohf_file()
      real(dp) :: e_core_file, offd(3)
      real(dp), allocatable, target :: fa(:, :), fb(:, :)
      real(dp), allocatable :: ua(:, :), ub(:, :)
      integer :: n, p
      n = mol%nbasis
      allocate (fa(n, n), fb(n, n), ua(n, n), ub(n, n), fock_sa(n, n), fock_sb(n, n))
      rc = afesp_read_fcidump_rohf(ctx, 'FCIDUMP'//c_null_char, int(n, c_int64_t), int(na, c_int64_t), int(nb, c_int64_t), c_null_ptr, &
                                   c_loc(fa), c_loc(fb), e_core_file, e_hf, offd, c_null_ptr, nlines)
      if (rc /= 0) call fail('integrals::read_fcidump', afesp_error_text(ctx))
      write (out, '(1X, A, I0)') 'Lines read: ', nlines
      write (out, '(1X, A, 1X, F18.10)') 'Core energy of the file (Hartree):', e_core_file
      write (out, '(1X, A, 1X, F20.12)') 'Reference determinant energy (Hartree):', e_hf
      write (out, '(1X, A, 1X, ES10.3)') 'Largest occupied-occupied off-diagonal Fock element:', offd(1)
      write (out, '(1X, A, 1X, ES10.3)') 'Largest virtual-virtual off-diagonal Fock element:', offd(2)
      write (out, '(1X, A, 1X, ES10.3)') 'Largest occupied-virtual Fock element:', offd(3)
      call semicanonical(fa, na, ua, fock_sa)
      call semicanonical(fb, nb, ub, fock_sb)
      ab_overlap = matmul(ub, transpose(ua))
      write (out, '(1X, A)') 'Rotating the MO integrals into semicanonical orbitals (alpha-alpha, alpha-beta, beta-beta)...'
      rc = afesp_mo_rotate_uhf(ctx, int(n, c_int64_t), ua, ub, c_null_ptr, c_null_ptr, c_null_ptr)
      if (rc /= 0) call fail('integrals::read_fcidump', afesp_error_text(ctx))
      allocate (levels(n), lb(n))
      do p = 1, n
         levels(p) = fock_sa(p, p); lb(p) = fock_sb(p, p)
      end do
      s2 = 0.0_dp
      scf_ok = .true.
      write (out, '(1X, A, 1X, F16.8, A)') 'Time taken for reading the FCIDUMP:', seconds() - t0, 's'
   end subroutine
   !> u(new, old) diagonalises f(1:o, 1:o) and f(o+1:, o+1:); g = u f u^T, symmetric, those two blocks diagonal to the bit
   subroutine semicanonical(f, o, u, g)
      real(dp), intent(in) :: f(:, :)
      integer, intent(in) :: o
      real(dp), intent(out) :: u(:, :), g(:, :)
      real(dp), allocatable :: w(:), v(:, :)
      integer :: n, lo, hi, m, blk, p, q
      n = size(f, 1)
      u = 0.0_dp
      do blk = 1, 2
         lo = merge(1, o + 1, blk == 1); hi = merge(o, n, blk == 1); m = hi - lo + 1
         if (m <= 0) cycle
         allocate (w(m), v(m, m))
         call sym_eig(f(lo:hi, lo:hi), w, v)
         u(lo:hi, lo:hi) = transpose(v)
         deallocate (w, v)
      end do
      g = matmul(u, matmul(f, transpose(u)))
      g = 0.5_dp*(g + transpose(g))
      do q = 1, n
         do p = 1, n
            if (p /= q .and. ((p <= o) .eqv. (q <= o))) g(p, q) = 0.0_dp
         end do
      end do
   end subroutine
   !> fcidump_active, first half: the frozen-core operator of the window and the core energy from the full MO integrals of the (last)
   !> transform -- before the window, which throws the core orbitals away (with natural virtuals: in the rotated orbitals)
   subroutine core_operator_before_window()
      allocate (h_act(n_act, n_act))
      if (cfg%uhf) then
         allocate (h_act_b(n_act, n_act))
         rc = afesp_ucore_operator(ctx, int(mol%nbasis, c_int64_t), int(nfc, c_int64_t), int(nfv, c_int64_t), coeff, cb, mol%hcore, &
                                   h_act, h_act_b, e_core)
      else
         rc = afesp_core_operator(ctx, int(mol%nbasis, c_int64_t), int(nfc, c_int64_t), int(nfv, c_int64_t), coeff, mol%hcore, h_act, &
                                  e_core)
      end if
      if (rc /= 0) call fail('mp2::write_fcidump_active', afesp_error_text(ctx))
   end subroutine
   !> second half: the integrals the solvers then run on (the window, or the whole basis), h_act and e_core + E_nuc as a standard FCIDUMP
   subroutine dump_active_space()
      write (out, '(1X, A)') 'Writing FCIDUMP file (active space)...'
      if (cfg%uhf) then
         rc = afesp_write_fcidump_uactive(ctx, 'FCIDUMP'//c_null_char, int(n_act, c_int64_t), int(na_act, c_int64_t), &
                                          int(nb_act, c_int64_t), h_act, h_act_b, e_core + mol%e_nuc, fcidump_threshold, nlines)
         if (rc /= 0) call fail('mp2::write_fcidump_active', afesp_error_text(ctx))
         write (out, '(1X, A, I0, A, I0, A, I0, A, F18.10)') 'FCIDUMP: NORB ', 2*n_act, ', NELEC ', na_act + nb_act, ', lines ', nlines, &
            ', core energy ', e_core + mol%e_nuc
      else
         rc = afesp_write_fcidump_active(ctx, 'FCIDUMP'//c_null_char, int(n_act, c_int64_t), int(nel_act, c_int64_t), 0_c_int64_t, &
                                         h_act, e_core + mol%e_nuc, fcidump_threshold, nlines)
         if (rc /= 0) call fail('mp2::write_fcidump_active', afesp_error_text(ctx))
         write (out, '(1X, A, I0, A, I0, A, I0, A, F18.10)') 'FCIDUMP: NORB ', n_act, ', NELEC ', nel_act, ', lines ', nlines, &
            ', core energy ', e_core + mol%e_nuc
      end if
      write (out, '(1X, A)') 'Done writing FCIDUMP file!'
   end subroutine
   !> FCIDUMP of the MO integrals resident after the AO->MO transform (reference src/mp2.f90:445-447)
   subroutine dump_integrals()
      write (out, '(1X, A)') 'Writing FCIDUMP file...'
      rc = afesp_write_fcidump(ctx, 'FCIDUMP'//c_null_char, int(mol%nbasis, c_int64_t), nlines)
      if (rc /= 0) call fail('mp2::write_fcidump', afesp_error_text(ctx))
      write (out, '(1X, A)') 'Done writing FCIDUMP file!'
   end subroutine
end program els_amd
