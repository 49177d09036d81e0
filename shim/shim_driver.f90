! Test driver for the Fortran shim (tests/test_gpu_shim.py): plays the part of x_drive — fills COMMON /GDATA_x/ from a
! raw file, calls INTEGRATE_x(TIN, TOUT) exactly as gas.f:173 | aer.f:217 | tot.f:604 do, writes the COMMON block back.
!   usage: shim_driver <g|a|t> <in.bin> <out.bin>      in.bin = ncell, then per cell C(NSPEC), RCONST(NREACT)  (float64)
!          shim_driver <G|A|T> <in.bin> <out.bin>      the same cells as ONE batched call, INTEGRATE_BATCH_x — the call a two-pass
!                                                      kpp_driver makes per mechanism and 10-s step (INTEGRATION.md); out.bin then
!                                                      ends with per cell IERR and the 8 statistics, and the call's wall time in ms
!          shim_driver <OG|OA|OT> <in.bin> <out.bin>   the batched call under Rosenbrock_x's options: in.bin starts with IPAR(20), RPAR(20), ATOL(NVAR),
!                                                      RTOL(NVAR) (float64), handed to MISTRA_SET_OPTIONS_x once, and goes on as for <G|A|T>; out.bin likewise,
!                                                      with the IERR of MISTRA_SET_OPTIONS_x behind the wall time
!          shim_driver <XG|XA|XT> <in.bin> <out.bin>   Rosenbrock_x itself, batched, any of its five methods: in.bin = IPAR(20), RPAR(20), ATOL(NVAR), RTOL(NVAR),
!                                                      TSTART, TEND, ncell, then the cells as for <G|A|T> (float64), all handed to ONE call of ROSENBROCK_BATCH_x;
!                                                      out.bin = per cell VAR, TEXIT, HEXIT, then per cell IERR and the 8 statistics
!          shim_driver <YG|YA|YT> <in.bin> <out.bin>   the same with tolerances per cell: in.bin = IPAR(20), RPAR(20), TSTART, TEND, ncell, ntol, then per cell VAR,
!                                                      FIX, RCONST, ATOL(ntol), RTOL(ntol), all handed to ONE call of ROSENBROCK_BATCH_CELLS_x; out.bin as for <XG|XA|XT>
!          shim_driver <ZG|ZA|ZT> <in.bin> <out.bin>   a series of Rosenbrock_x calls: in.bin = IPAR(20), RPAR(20), ATOL(NVAR), RTOL(NVAR), ncell, nleg, carry (0 | 1), ntol,
!                                                      TIMES(nleg + 1), then the cells as for <G|A|T>.  ntol = 0: ONE call of ROSENBROCK_BATCH_SERIES_x with the pair; ntol = 1 or
!                                                      NVAR: ONE call of ROSENBROCK_BATCH_SERIES_CELLS_x, every cell's row the first ntol entries of the pair.  out.bin = per leg
!                                                      and cell VAR, TEXIT, HEXIT, IERR, the 8 statistics
!          shim_driver <NG|NA|NT> <in.bin> <out.bin>   the series with rate constants and FIX of the leg's own: in.bin = IPAR(20), RPAR(20), ATOL(NVAR), RTOL(NVAR), ncell,
!                                                      nleg, carry (0 | 1), ntol, nrcleg, nfixleg, TIMES(nleg + 1), VAR(NVAR, ncell), FIX(NFIX, ncell, nfixleg),
!                                                      RCONST(NREACT, ncell, nrcleg).  ntol = 0: ONE call of ROSENBROCK_BATCH_SERIES_RATES_x; ntol = 1 or NVAR: ONE call of
!                                                      ROSENBROCK_BATCH_SERIES_RATES_CELLS_x, every cell's row the first ntol entries of the pair.  out.bin as for <ZG|ZA|ZT>
!          shim_driver <MG|MA|MT> <in.bin> <out.bin>   the series with rate constants linear in time over each leg: in.bin as for <NG|NA|NT> with ntol = 0 and nrcleg =
!                                                      nleg + 1, RCONST(NREACT, ncell, nleg + 1) the node blocks at TIMES.  ONE call of
!                                                      ROSENBROCK_BATCH_SERIES_LINRATES_x; out.bin as for <ZG|ZA|ZT>
!          shim_driver <BG|BA|BT> <in.bin> <out.bin>   the series with rates with the reaction flux of every leg: in.bin as for <NG|NA|NT>.  ntol = 0: ONE call of
!                                                      ROSENBROCK_BATCH_SERIES_FLUX_x; ntol = 1 or NVAR: ONE call of ROSENBROCK_BATCH_SERIES_FLUX_CELLS_x.  out.bin as for
!                                                      <ZG|ZA|ZT> with FLUX(NREACT) of the leg and cell behind every record
!          shim_driver <WG|WA|WT> <in.bin> <out.bin>   Rosenbrock_x with the reaction flux: in.bin = IPAR(20), RPAR(20), ATOL(NVAR), RTOL(NVAR), TSTART, TEND, ncell, ntol, then
!                                                      the cells as for <G|A|T>.  ntol = 0: ONE call of ROSENBROCK_BATCH_FLUX_x with the pair; ntol = 1 or NVAR: ONE call of
!                                                      ROSENBROCK_BATCH_FLUX_CELLS_x, every cell's row the first ntol entries of the pair.  out.bin = per cell VAR, TEXIT,
!                                                      HEXIT, IERR, the 8 statistics, FLUX(NREACT)
!          shim_driver <IG|IA|IT> <in.bin> <out.bin>   Rosenbrock_x with dense output: in.bin = IPAR(20), RPAR(20), ATOL(NVAR), RTOL(NVAR), TSTART, TEND, ncell, ntol, ns, TS(ns),
!                                                      then the cells as for <G|A|T>.  ntol = 0: ONE call of ROSENBROCK_BATCH_DENSE_x with the pair; ntol = 1 or NVAR: ONE call
!                                                      of ROSENBROCK_BATCH_DENSE_CELLS_x, every cell's row the first ntol entries of the pair.  out.bin = per cell VAR, TEXIT,
!                                                      HEXIT, IERR, the 8 statistics, NOUT, then YS(NVAR, ncell, ns)
!          shim_driver <PG|PA|PT> <in.bin> <out.bin>   the operators: in.bin = ncell, nshift, funrhs (0 | 1), nrhs, SHIFT(nshift), then the cells as for <G|A|T>, then
!                                                      RHS(NVAR, ncell, nrhs); ONE call each of FUN_BATCH_x, JAC_SP_BATCH_x and LINSOLVE_BATCH_x.  out.bin = VDOT(NVAR, ncell),
!                                                      JVS(LU_NONZERO, ncell), X(NVAR, ncell, funrhs + nrhs), ISING(ncell)
!          shim_driver <LG|LA|LT> <in.bin> <out.bin>   the replay: in.bin = IPAR(20), RPAR(20), ATOL(NVAR), RTOL(NVAR), TSTART, TEND, ncell, ntol, cap, hrows,
!                                                      HSTEPS(cap, hrows), NSTEPS(hrows) as doubles, then the cells as for <G|A|T>.  ntol = 0: ONE call of
!                                                      ROSENBROCK_BATCH_REPLAY_x with the pair; ntol = 1 or NVAR: ONE call of ROSENBROCK_BATCH_REPLAY_CELLS_x, every
!                                                      cell's row the first ntol entries of the pair.  out.bin = per cell VAR, TEXIT, HEXIT, IERR, the 8 statistics,
!                                                      ERRLOG(cap) (set to -7.25 in front of the call)
!          shim_driver <Eg|Ea|Et> <in.bin> <out.bin>   in.bin = ncell, then per cell VAR, FIX, ENV (the vector MISTRA_RATES_ENV_x packs,
!                                                      mistra_kpp_rates.f90): UPDATE_RCONST_BATCH_x, then INTEGRATE_BATCH_ENV_x (rates and
!                                                      integrator on the device, RCONST never crosses PCIe); out.bin = per cell VAR,
!                                                      then per cell IERR + 8 statistics, then per cell RCONST of the first call
!          shim_driver D <in.bin> <out.bin>            one 10-s step of a column through the SINGLE-PASS batched driver (shim/mistra_kpp_drive.f90,
!                                                      shim/kpp_drive.patch): this program plays kpp_driver and x_drive's prologue — per layer it puts the
!                                                      recorded values into the COMMON blocks (shim_driver_env_set.f90), calls KPP_DRIVE_STAGE_x as the
!                                                      patched x_drive does, and behind the loop kpp_drive_run_arrays on its own copies of the model
!                                                      arrays (what KPP_DRIVE_RUN of mistra_kpp_model.f90 does inside the model).  in.bin (float64):
!                                                      n, j1, j5, nlev, nrxn, nl, nrep | maps of the three mechanisms | il(nlev) | s1(j1,n) s3(j5,n)
!                                                      sl1(121,4,n) sion1(55,4,n) bg(2,nrxn,nlev) bgs(2,122,n) | per layer: mech, k, air, h2o, env(nenv).
!                                                      out.bin: the arrays after the step | per layer ierr, 8 statistics, texit, hexit | per repetition
!                                                      the wall times (ms) of the staging loop and of the device call(s)
!          shim_driver D2 <in.bin> <out.bin>           the same column step TWICE in a row under step reuse: MISTRA_STEP_REUSE_g/_a/_t(.true.) first, the second
!                                                      step on the arrays the first one left (tkpp = 10).  in.bin as for D (nrep is not used).  out.bin: the arrays
!                                                      after the second step | per step and layer: mech, k, ierr, 8 statistics, texit, hexit, H
!          shim_driver DP <in.bin> <out.bin>           the column step of D under an integrator policy: in.bin starts with METHOD, ATOL_FACTOR, ATOL_FLOOR (float64),
!                                                      handed to MISTRA_SET_POLICY_g/_a/_t for the mechanisms the step has layers of, and goes on as for D; out.bin as for D
!          shim_driver <Ka|Kt|Ha|Ht|Va|Vt|Sa|St|Qa|Qt|Ca|Rg|Ra|Rt> <in.bin> <out.bin>   liq_parm's kernels through shim/mistra_kpp_liq.f90 (SURVEY §8 f3): K = FAST_K_MT_BATCH
!                                                      (in: nlayer, nka, nkt, nkc, nspec, ka, ifeed, nkc_l | kw | rq | ff cw cm freep alpha vmean xkmt t p vt;
!                                                      out: xkmt, vt), H = HENRY_BATCH (in: nlayer, nspec | tt; out: henry), V = V_MEAN_BATCH (the same shapes; out: vmean), S = ST_COEFF_BATCH (in: nlayer, nspec, lpJoyce14bc, lpBuxmann15alph | env(5,nlayer); out: alpha), R = DRY_RATES_BATCH (in: nlayer | tt, freep, rcd(2,nlayer), vmean4 / henry4 (4,nlayer); out: xkmtd, xeq, henry4), C = CW_RC_BATCH (in: nlayer, nkt, nka, dry, ka, ifeed | kw, rq, e, crys4, ff, feu, cloud; out: rc, cw, cm, conv2, below), Q = EQUIL_CO_BATCH (in: nlayer,
!                                                      nkc, j6, nspec | tt conv2 xgamma xkef xkeb; out: xkef, xkeb)
! After the call the one-cell mode also writes ATOL(1), RTOL(1) (INTEGRATE_x resets them, gas.f:745-746).
program shim_driver
  use mistra_kpp_rates
  implicit none
  character(len=256) :: a1, fin, fout
  call get_command_argument(1, a1)
  call get_command_argument(2, fin)
  call get_command_argument(3, fout)
  select case (a1(1:1))
  case ('g'); call run_g(trim(fin), trim(fout))
  case ('a'); call run_a(trim(fin), trim(fout))
  case ('t'); call run_t(trim(fin), trim(fout))
  case ('G'); call run_batch(0, 102, 3, 331, trim(fin), trim(fout))
  case ('A'); call run_batch(1, 257, 5, 979, trim(fin), trim(fout))
  case ('T'); call run_batch(2, 417, 7, 1627, trim(fin), trim(fout))
  case ('D'); call run_drive(trim(fin), trim(fout), a1(2:2) == '2', a1(2:2) == 'P')
  case ('O')
     select case (a1(2:2))
     case ('G'); call run_batch(0, 102, 3, 331, trim(fin), trim(fout), .true.)
     case ('A'); call run_batch(1, 257, 5, 979, trim(fin), trim(fout), .true.)
     case ('T'); call run_batch(2, 417, 7, 1627, trim(fin), trim(fout), .true.)
     case default; stop 'mechanism must be G, A or T'
     end select
  case ('X')
     select case (a1(2:2))
     case ('G'); call run_rosenbrock(0, 102, 3, 331, trim(fin), trim(fout))
     case ('A'); call run_rosenbrock(1, 257, 5, 979, trim(fin), trim(fout))
     case ('T'); call run_rosenbrock(2, 417, 7, 1627, trim(fin), trim(fout))
     case default; stop 'mechanism must be G, A or T'
     end select
  case ('Y')
     select case (a1(2:2))
     case ('G'); call run_rosenbrock_cells(0, 102, 3, 331, trim(fin), trim(fout))
     case ('A'); call run_rosenbrock_cells(1, 257, 5, 979, trim(fin), trim(fout))
     case ('T'); call run_rosenbrock_cells(2, 417, 7, 1627, trim(fin), trim(fout))
     case default; stop 'mechanism must be G, A or T'
     end select
  case ('Z')
     select case (a1(2:2))
     case ('G'); call run_series(0, 102, 3, 331, trim(fin), trim(fout))
     case ('A'); call run_series(1, 257, 5, 979, trim(fin), trim(fout))
     case ('T'); call run_series(2, 417, 7, 1627, trim(fin), trim(fout))
     case default; stop 'mechanism must be G, A or T'
     end select
  case ('N')
     select case (a1(2:2))
     case ('G'); call run_series_rates(0, 102, 3, 331, trim(fin), trim(fout), .false., .false.)
     case ('A'); call run_series_rates(1, 257, 5, 979, trim(fin), trim(fout), .false., .false.)
     case ('T'); call run_series_rates(2, 417, 7, 1627, trim(fin), trim(fout), .false., .false.)
     case default; stop 'mechanism must be G, A or T'
     end select
  case ('M')
     select case (a1(2:2))
     case ('G'); call run_series_rates(0, 102, 3, 331, trim(fin), trim(fout), .true., .false.)
     case ('A'); call run_series_rates(1, 257, 5, 979, trim(fin), trim(fout), .true., .false.)
     case ('T'); call run_series_rates(2, 417, 7, 1627, trim(fin), trim(fout), .true., .false.)
     case default; stop 'mechanism must be G, A or T'
     end select
  case ('B')
     select case (a1(2:2))
     case ('G'); call run_series_rates(0, 102, 3, 331, trim(fin), trim(fout), .false., .true.)
     case ('A'); call run_series_rates(1, 257, 5, 979, trim(fin), trim(fout), .false., .true.)
     case ('T'); call run_series_rates(2, 417, 7, 1627, trim(fin), trim(fout), .false., .true.)
     case default; stop 'mechanism must be G, A or T'
     end select
  case ('W')
     select case (a1(2:2))
     case ('G'); call run_flux(0, 102, 3, 331, trim(fin), trim(fout))
     case ('A'); call run_flux(1, 257, 5, 979, trim(fin), trim(fout))
     case ('T'); call run_flux(2, 417, 7, 1627, trim(fin), trim(fout))
     case default; stop 'mechanism must be G, A or T'
     end select
  case ('I')
     select case (a1(2:2))
     case ('G'); call run_dense(0, 102, 3, 331, trim(fin), trim(fout))
     case ('A'); call run_dense(1, 257, 5, 979, trim(fin), trim(fout))
     case ('T'); call run_dense(2, 417, 7, 1627, trim(fin), trim(fout))
     case default; stop 'mechanism must be G, A or T'
     end select
  case ('L')
     select case (a1(2:2))
     case ('G'); call run_replay(0, 102, 3, 331, trim(fin), trim(fout))
     case ('A'); call run_replay(1, 257, 5, 979, trim(fin), trim(fout))
     case ('T'); call run_replay(2, 417, 7, 1627, trim(fin), trim(fout))
     case default; stop 'mechanism must be G, A or T'
     end select
  case ('P')
     select case (a1(2:2))
     case ('G'); call run_ops(0, 102, 3, 331, 1110, trim(fin), trim(fout))
     case ('A'); call run_ops(1, 257, 5, 979, 6579, trim(fin), trim(fout))
     case ('T'); call run_ops(2, 417, 7, 1627, 13503, trim(fin), trim(fout))
     case default; stop 'mechanism must be G, A or T'
     end select
  case ('K', 'H', 'Q', 'V', 'S', 'C', 'R')
     select case (a1(2:2))
     case ('g')
        if (a1(1:1) /= 'R') stop 'mechanism must be a or t'
        call run_liq(a1(1:1), 1, trim(fin), trim(fout))
     case ('a'); call run_liq(a1(1:1), 2, trim(fin), trim(fout))
     case ('t'); call run_liq(a1(1:1), 3, trim(fin), trim(fout))
     case default; stop 'mechanism must be a or t'
     end select
  case ('E')
     select case (a1(2:2))
     case ('g'); call run_env(0, 102, 3, 331, nenv_g, trim(fin), trim(fout))
     case ('a'); call run_env(1, 257, 5, 979, nenv_a, trim(fin), trim(fout))
     case ('t'); call run_env(2, 417, 7, 1627, nenv_t, trim(fin), trim(fout))
     case default; stop 'mechanism must be g, a or t'
     end select
  case default; stop 'mechanism must be g, a or t'
  end select
contains
  subroutine run_g(fin, fout)
    character(len=*), intent(in) :: fin, fout
    integer, parameter :: NVAR = 102, NFIX = 3, NREACT = 331
    double precision :: C(NVAR + NFIX), RCONST(NREACT), TIME, DT, ATOL(NVAR), RTOL(NVAR), STEPMIN, STEPMAX
    common /GDATA_g/ C, RCONST, TIME, DT, ATOL, RTOL, STEPMIN, STEPMAX
    double precision :: tkpp, tend, rn
    integer :: n, i
    open (11, file=fin, access='stream', form='unformatted', status='old')
    open (12, file=fout, access='stream', form='unformatted', status='replace')
    read (11) rn
    n = int(rn)
    do i = 1, n
       read (11) C, RCONST
       tkpp = 0.d0
       tend = 10.d0
       call INTEGRATE_g(tkpp, tend)
       write (12) C(1:NVAR), tkpp, STEPMIN, ATOL(1), RTOL(1)
    end do
    close (11); close (12)
  end subroutine run_g
  subroutine run_a(fin, fout)
    character(len=*), intent(in) :: fin, fout
    integer, parameter :: NVAR = 257, NFIX = 5, NREACT = 979
    double precision :: C(NVAR + NFIX), RCONST(NREACT), TIME, DT, ATOL(NVAR), RTOL(NVAR), STEPMIN, STEPMAX
    common /GDATA_a/ C, RCONST, TIME, DT, ATOL, RTOL, STEPMIN, STEPMAX
    double precision :: tkpp, tend, rn
    integer :: n, i
    open (11, file=fin, access='stream', form='unformatted', status='old')
    open (12, file=fout, access='stream', form='unformatted', status='replace')
    read (11) rn
    n = int(rn)
    do i = 1, n
       read (11) C, RCONST
       tkpp = 0.d0
       tend = 10.d0
       call INTEGRATE_a(tkpp, tend)
       write (12) C(1:NVAR), tkpp, STEPMIN, ATOL(1), RTOL(1)
    end do
    close (11); close (12)
  end subroutine run_a
  subroutine run_t(fin, fout)
    character(len=*), intent(in) :: fin, fout
    integer, parameter :: NVAR = 417, NFIX = 7, NREACT = 1627
    double precision :: C(NVAR + NFIX), RCONST(NREACT), TIME, DT, ATOL(NVAR), RTOL(NVAR), STEPMIN, STEPMAX
    common /GDATA_t/ C, RCONST, TIME, DT, ATOL, RTOL, STEPMIN, STEPMAX
    double precision :: tkpp, tend, rn
    integer :: n, i
    open (11, file=fin, access='stream', form='unformatted', status='old')
    open (12, file=fout, access='stream', form='unformatted', status='replace')
    read (11) rn
    n = int(rn)
    do i = 1, n
       read (11) C, RCONST
       tkpp = 0.d0
       tend = 10.d0
       call INTEGRATE_t(tkpp, tend)
       write (12) C(1:NVAR), tkpp, STEPMIN, ATOL(1), RTOL(1)
    end do
    close (11); close (12)
  end subroutine run_t
  subroutine run_batch(mech, NVAR, NFIX, NREACT, fin, fout, with_options)
    integer, intent(in) :: mech, NVAR, NFIX, NREACT
    character(len=*), intent(in) :: fin, fout
    logical, intent(in), optional :: with_options
    double precision :: ropt(40)
    double precision, allocatable :: ATOL(:), RTOL(:)
    integer :: IPAR(20), ierr_opt
    double precision, allocatable :: VAR(:, :), VAR0(:, :), FIX(:, :), RCONST(:, :), TEXIT(:), HEXIT(:), rec(:)
    integer, allocatable :: IERR(:), ISTAT(:, :)
    double precision :: rn, tin, tout
    integer :: n, i, rep
    integer(8) :: c0, c1, rate
    open (11, file=fin, access='stream', form='unformatted', status='old')
    open (12, file=fout, access='stream', form='unformatted', status='replace')
    ierr_opt = 0
    if (present(with_options)) then      ! what a model with an edited INTEGRATE_x does once after start-up
       allocate (ATOL(NVAR), RTOL(NVAR))
       read (11) ropt, ATOL, RTOL
       IPAR = int(ropt(1:20))
       select case (mech)
       case (0); call MISTRA_SET_OPTIONS_g(IPAR, ropt(21:40), ATOL, RTOL, ierr_opt)
       case (1); call MISTRA_SET_OPTIONS_a(IPAR, ropt(21:40), ATOL, RTOL, ierr_opt)
       case (2); call MISTRA_SET_OPTIONS_t(IPAR, ropt(21:40), ATOL, RTOL, ierr_opt)
       end select
    end if
    read (11) rn
    n = int(rn)
    allocate (VAR(NVAR, n), VAR0(NVAR, n), FIX(NFIX, n), RCONST(NREACT, n), TEXIT(n), HEXIT(n), IERR(n), ISTAT(8, n), rec(NVAR + NFIX + NREACT))
    do i = 1, n                      ! pass 1 of a batched kpp_driver: every layer's C and RCONST, as x_drive prepares them
       read (11) rec
       VAR0(:, i) = rec(1:NVAR)
       FIX(:, i) = rec(NVAR + 1:NVAR + NFIX)
       RCONST(:, i) = rec(NVAR + NFIX + 1:)
    end do
    do rep = 1, 2                    ! the second call is the timed one (the first pays the library's start-up)
       VAR = VAR0
       tin = 0.d0
       tout = 10.d0
       call system_clock(c0, rate)
       select case (mech)
       case (0); call INTEGRATE_BATCH_g(n, VAR, FIX, RCONST, tin, tout, TEXIT, HEXIT, IERR, ISTAT)
       case (1); call INTEGRATE_BATCH_a(n, VAR, FIX, RCONST, tin, tout, TEXIT, HEXIT, IERR, ISTAT)
       case (2); call INTEGRATE_BATCH_t(n, VAR, FIX, RCONST, tin, tout, TEXIT, HEXIT, IERR, ISTAT)
       end select
       call system_clock(c1)
    end do
    do i = 1, n
       write (12) VAR(:, i), TEXIT(i), HEXIT(i), 1.d-25, 1.d-3
    end do
    do i = 1, n
       write (12) dble(IERR(i)), dble(ISTAT(:, i))
    end do
    write (12) 1.d3 * dble(c1 - c0) / dble(rate)
    if (present(with_options)) write (12) dble(ierr_opt)
    close (11); close (12)
  end subroutine run_batch
  subroutine run_rosenbrock(mech, NVAR, NFIX, NREACT, fin, fout)
    integer, intent(in) :: mech, NVAR, NFIX, NREACT
    character(len=*), intent(in) :: fin, fout
    double precision :: ropt(40), tt(3)
    double precision, allocatable :: ATOL(:), RTOL(:), VAR(:, :), FIX(:, :), RCONST(:, :), TEXIT(:), HEXIT(:), rec(:)
    integer :: IPAR(20), n, i
    integer, allocatable :: IERR(:), ISTAT(:, :)
    open (11, file=fin, access='stream', form='unformatted', status='old')
    open (12, file=fout, access='stream', form='unformatted', status='replace')
    allocate (ATOL(NVAR), RTOL(NVAR))
    read (11) ropt, ATOL, RTOL, tt      ! tt: TSTART, TEND, ncell
    IPAR = int(ropt(1:20))
    n = int(tt(3))
    allocate (VAR(NVAR, n), FIX(NFIX, n), RCONST(NREACT, n), TEXIT(n), HEXIT(n), IERR(n), ISTAT(8, n), rec(NVAR + NFIX + NREACT))
    do i = 1, n
       read (11) rec
       VAR(:, i) = rec(1:NVAR)
       FIX(:, i) = rec(NVAR + 1:NVAR + NFIX)
       RCONST(:, i) = rec(NVAR + NFIX + 1:)
    end do
    select case (mech)
    case (0); call ROSENBROCK_BATCH_g(n, VAR, FIX, RCONST, tt(1), tt(2), ATOL, RTOL, ropt(21:40), IPAR, TEXIT, HEXIT, IERR, ISTAT)
    case (1); call ROSENBROCK_BATCH_a(n, VAR, FIX, RCONST, tt(1), tt(2), ATOL, RTOL, ropt(21:40), IPAR, TEXIT, HEXIT, IERR, ISTAT)
    case (2); call ROSENBROCK_BATCH_t(n, VAR, FIX, RCONST, tt(1), tt(2), ATOL, RTOL, ropt(21:40), IPAR, TEXIT, HEXIT, IERR, ISTAT)
    end select
    do i = 1, n
       write (12) VAR(:, i), TEXIT(i), HEXIT(i)
    end do
    do i = 1, n
       write (12) dble(IERR(i)), dble(ISTAT(:, i))
    end do
    close (11); close (12)
  end subroutine run_rosenbrock
  subroutine run_rosenbrock_cells(mech, NVAR, NFIX, NREACT, fin, fout)
    integer, intent(in) :: mech, NVAR, NFIX, NREACT
    character(len=*), intent(in) :: fin, fout
    double precision :: ropt(40), tt(4)
    double precision, allocatable :: ATOL(:, :), RTOL(:, :), VAR(:, :), FIX(:, :), RCONST(:, :), TEXIT(:), HEXIT(:), rec(:)
    integer :: IPAR(20), n, ntol, i
    integer, allocatable :: IERR(:), ISTAT(:, :)
    open (11, file=fin, access='stream', form='unformatted', status='old')
    open (12, file=fout, access='stream', form='unformatted', status='replace')
    read (11) ropt, tt      ! tt: TSTART, TEND, ncell, ntol
    IPAR = int(ropt(1:20))
    n = int(tt(3))
    ntol = int(tt(4))
    allocate (VAR(NVAR, n), FIX(NFIX, n), RCONST(NREACT, n), ATOL(ntol, n), RTOL(ntol, n), TEXIT(n), HEXIT(n), IERR(n), ISTAT(8, n))
    allocate (rec(NVAR + NFIX + NREACT + 2 * ntol))
    do i = 1, n
       read (11) rec
       VAR(:, i) = rec(1:NVAR)
       FIX(:, i) = rec(NVAR + 1:NVAR + NFIX)
       RCONST(:, i) = rec(NVAR + NFIX + 1:NVAR + NFIX + NREACT)
       ATOL(:, i) = rec(NVAR + NFIX + NREACT + 1:NVAR + NFIX + NREACT + ntol)
       RTOL(:, i) = rec(NVAR + NFIX + NREACT + ntol + 1:)
    end do
    select case (mech)
    case (0); call ROSENBROCK_BATCH_CELLS_g(n, VAR, FIX, RCONST, tt(1), tt(2), ATOL, RTOL, ntol, ropt(21:40), IPAR, TEXIT, HEXIT, IERR, ISTAT)
    case (1); call ROSENBROCK_BATCH_CELLS_a(n, VAR, FIX, RCONST, tt(1), tt(2), ATOL, RTOL, ntol, ropt(21:40), IPAR, TEXIT, HEXIT, IERR, ISTAT)
    case (2); call ROSENBROCK_BATCH_CELLS_t(n, VAR, FIX, RCONST, tt(1), tt(2), ATOL, RTOL, ntol, ropt(21:40), IPAR, TEXIT, HEXIT, IERR, ISTAT)
    end select
    do i = 1, n
       write (12) VAR(:, i), TEXIT(i), HEXIT(i)
    end do
    do i = 1, n
       write (12) dble(IERR(i)), dble(ISTAT(:, i))
    end do
    close (11); close (12)
  end subroutine run_rosenbrock_cells
  subroutine run_flux(mech, NVAR, NFIX, NREACT, fin, fout)
    integer, intent(in) :: mech, NVAR, NFIX, NREACT
    character(len=*), intent(in) :: fin, fout
    double precision :: ropt(40), tt(4)
    double precision, allocatable :: ATOL(:), RTOL(:), AROW(:, :), RROW(:, :), VAR(:, :), FIX(:, :), RCONST(:, :), TEXIT(:), HEXIT(:), FLUX(:, :), rec(:)
    integer :: IPAR(20), n, ntol, i
    integer, allocatable :: IERR(:), ISTAT(:, :)
    open (11, file=fin, access='stream', form='unformatted', status='old')
    open (12, file=fout, access='stream', form='unformatted', status='replace')
    allocate (ATOL(NVAR), RTOL(NVAR))
    read (11) ropt, ATOL, RTOL, tt      ! tt: TSTART, TEND, ncell, ntol
    IPAR = int(ropt(1:20))
    n = int(tt(3))
    ntol = int(tt(4))
    allocate (VAR(NVAR, n), FIX(NFIX, n), RCONST(NREACT, n), TEXIT(n), HEXIT(n), IERR(n), ISTAT(8, n), FLUX(NREACT, n))
    allocate (rec(NVAR + NFIX + NREACT), AROW(max(ntol, 1), n), RROW(max(ntol, 1), n))
    FLUX = -7.25d0
    do i = 1, n
       read (11) rec
       VAR(:, i) = rec(1:NVAR)
       FIX(:, i) = rec(NVAR + 1:NVAR + NFIX)
       RCONST(:, i) = rec(NVAR + NFIX + 1:)
       if (ntol > 0) then
          AROW(:, i) = ATOL(1:ntol)
          RROW(:, i) = RTOL(1:ntol)
       end if
    end do
    if (ntol == 0) then
       select case (mech)
       case (0); call ROSENBROCK_BATCH_FLUX_g(n, VAR, FIX, RCONST, tt(1), tt(2), ATOL, RTOL, ropt(21:40), IPAR, TEXIT, HEXIT, IERR, ISTAT, FLUX)
       case (1); call ROSENBROCK_BATCH_FLUX_a(n, VAR, FIX, RCONST, tt(1), tt(2), ATOL, RTOL, ropt(21:40), IPAR, TEXIT, HEXIT, IERR, ISTAT, FLUX)
       case (2); call ROSENBROCK_BATCH_FLUX_t(n, VAR, FIX, RCONST, tt(1), tt(2), ATOL, RTOL, ropt(21:40), IPAR, TEXIT, HEXIT, IERR, ISTAT, FLUX)
       end select
    else
       select case (mech)
       case (0); call ROSENBROCK_BATCH_FLUX_CELLS_g(n, VAR, FIX, RCONST, tt(1), tt(2), AROW, RROW, ntol, ropt(21:40), IPAR, TEXIT, HEXIT, IERR, ISTAT, FLUX)
       case (1); call ROSENBROCK_BATCH_FLUX_CELLS_a(n, VAR, FIX, RCONST, tt(1), tt(2), AROW, RROW, ntol, ropt(21:40), IPAR, TEXIT, HEXIT, IERR, ISTAT, FLUX)
       case (2); call ROSENBROCK_BATCH_FLUX_CELLS_t(n, VAR, FIX, RCONST, tt(1), tt(2), AROW, RROW, ntol, ropt(21:40), IPAR, TEXIT, HEXIT, IERR, ISTAT, FLUX)
       end select
    end if
    do i = 1, n
       write (12) VAR(:, i), TEXIT(i), HEXIT(i), dble(IERR(i)), dble(ISTAT(:, i)), FLUX(:, i)
    end do
    close (11); close (12)
  end subroutine run_flux
  subroutine run_replay(mech, NVAR, NFIX, NREACT, fin, fout)
    integer, intent(in) :: mech, NVAR, NFIX, NREACT
    character(len=*), intent(in) :: fin, fout
    double precision :: ropt(40), tt(6)
    double precision, allocatable :: ATOL(:), RTOL(:), AROW(:, :), RROW(:, :), VAR(:, :), FIX(:, :), RCONST(:, :), TEXIT(:), HEXIT(:), HSTEPS(:, :), CNT(:), &
         ERRLOG(:, :), rec(:)
    integer :: IPAR(20), n, ntol, cap, hrows, i
    integer, allocatable :: IERR(:), ISTAT(:, :), NSTEPS(:)
    open (11, file=fin, access='stream', form='unformatted', status='old')
    open (12, file=fout, access='stream', form='unformatted', status='replace')
    allocate (ATOL(NVAR), RTOL(NVAR))
    read (11) ropt, ATOL, RTOL, tt      ! tt: TSTART, TEND, ncell, ntol, cap, hrows
    IPAR = int(ropt(1:20))
    n = int(tt(3)); ntol = int(tt(4)); cap = int(tt(5)); hrows = int(tt(6))
    allocate (HSTEPS(cap, hrows), CNT(hrows), NSTEPS(hrows))
    read (11) HSTEPS, CNT
    NSTEPS = int(CNT)
    allocate (VAR(NVAR, n), FIX(NFIX, n), RCONST(NREACT, n), TEXIT(n), HEXIT(n), IERR(n), ISTAT(8, n), ERRLOG(cap, n))
    allocate (rec(NVAR + NFIX + NREACT), AROW(max(ntol, 1), n), RROW(max(ntol, 1), n))
    ERRLOG = -7.25d0
    do i = 1, n
       read (11) rec
       VAR(:, i) = rec(1:NVAR)
       FIX(:, i) = rec(NVAR + 1:NVAR + NFIX)
       RCONST(:, i) = rec(NVAR + NFIX + 1:)
       if (ntol > 0) then
          AROW(:, i) = ATOL(1:ntol)
          RROW(:, i) = RTOL(1:ntol)
       end if
    end do
    if (ntol == 0) then
       select case (mech)
       case (0); call ROSENBROCK_BATCH_REPLAY_g(n, VAR, FIX, RCONST, tt(1), tt(2), ATOL, RTOL, ropt(21:40), IPAR, cap, hrows, HSTEPS, NSTEPS, TEXIT, HEXIT, IERR, ISTAT, ERRLOG)
       case (1); call ROSENBROCK_BATCH_REPLAY_a(n, VAR, FIX, RCONST, tt(1), tt(2), ATOL, RTOL, ropt(21:40), IPAR, cap, hrows, HSTEPS, NSTEPS, TEXIT, HEXIT, IERR, ISTAT, ERRLOG)
       case (2); call ROSENBROCK_BATCH_REPLAY_t(n, VAR, FIX, RCONST, tt(1), tt(2), ATOL, RTOL, ropt(21:40), IPAR, cap, hrows, HSTEPS, NSTEPS, TEXIT, HEXIT, IERR, ISTAT, ERRLOG)
       end select
    else
       select case (mech)
       case (0); call ROSENBROCK_BATCH_REPLAY_CELLS_g(n, VAR, FIX, RCONST, tt(1), tt(2), AROW, RROW, ntol, ropt(21:40), IPAR, cap, hrows, HSTEPS, NSTEPS, TEXIT, HEXIT, &
            IERR, ISTAT, ERRLOG)
       case (1); call ROSENBROCK_BATCH_REPLAY_CELLS_a(n, VAR, FIX, RCONST, tt(1), tt(2), AROW, RROW, ntol, ropt(21:40), IPAR, cap, hrows, HSTEPS, NSTEPS, TEXIT, HEXIT, &
            IERR, ISTAT, ERRLOG)
       case (2); call ROSENBROCK_BATCH_REPLAY_CELLS_t(n, VAR, FIX, RCONST, tt(1), tt(2), AROW, RROW, ntol, ropt(21:40), IPAR, cap, hrows, HSTEPS, NSTEPS, TEXIT, HEXIT, &
            IERR, ISTAT, ERRLOG)
       end select
    end if
    do i = 1, n
       write (12) VAR(:, i), TEXIT(i), HEXIT(i), dble(IERR(i)), dble(ISTAT(:, i)), ERRLOG(:, i)
    end do
    close (11); close (12)
  end subroutine run_replay
  subroutine run_ops(mech, NVAR, NFIX, NREACT, NNZ, fin, fout)
    integer, intent(in) :: mech, NVAR, NFIX, NREACT, NNZ
    character(len=*), intent(in) :: fin, fout
    double precision :: hd(4)
    double precision, allocatable :: SHIFT(:), VAR(:, :), FIX(:, :), RCONST(:, :), VDOT(:, :), JVS(:, :), RHS(:, :, :), X(:, :, :), rec(:)
    integer :: n, nshift, nrhs, nrow, i
    integer, allocatable :: ISING(:)
    logical :: funrhs
    open (11, file=fin, access='stream', form='unformatted', status='old')
    open (12, file=fout, access='stream', form='unformatted', status='replace')
    read (11) hd      ! ncell, nshift, funrhs, nrhs
    n = int(hd(1)); nshift = int(hd(2)); funrhs = hd(3) /= 0.0d0; nrhs = int(hd(4))
    nrow = nrhs + merge(1, 0, funrhs)
    allocate (SHIFT(nshift), VAR(NVAR, n), FIX(NFIX, n), RCONST(NREACT, n), VDOT(NVAR, n), JVS(NNZ, n), RHS(NVAR, n, max(nrhs, 1)), X(NVAR, n, nrow), ISING(n))
    allocate (rec(NVAR + NFIX + NREACT))
    read (11) SHIFT
    do i = 1, n
       read (11) rec
       VAR(:, i) = rec(1:NVAR)
       FIX(:, i) = rec(NVAR + 1:NVAR + NFIX)
       RCONST(:, i) = rec(NVAR + NFIX + 1:)
    end do
    if (nrhs > 0) read (11) RHS(:, :, 1:nrhs)
    VDOT = -7.25d0; JVS = -7.25d0; X = -7.25d0; ISING = -7
    select case (mech)
    case (0)
       call FUN_BATCH_g(n, VAR, FIX, RCONST, VDOT)
       call JAC_SP_BATCH_g(n, VAR, FIX, RCONST, JVS)
       call LINSOLVE_BATCH_g(n, VAR, FIX, RCONST, nshift, SHIFT, funrhs, nrhs, RHS, X, ISING)
    case (1)
       call FUN_BATCH_a(n, VAR, FIX, RCONST, VDOT)
       call JAC_SP_BATCH_a(n, VAR, FIX, RCONST, JVS)
       call LINSOLVE_BATCH_a(n, VAR, FIX, RCONST, nshift, SHIFT, funrhs, nrhs, RHS, X, ISING)
    case (2)
       call FUN_BATCH_t(n, VAR, FIX, RCONST, VDOT)
       call JAC_SP_BATCH_t(n, VAR, FIX, RCONST, JVS)
       call LINSOLVE_BATCH_t(n, VAR, FIX, RCONST, nshift, SHIFT, funrhs, nrhs, RHS, X, ISING)
    end select
    write (12) VDOT, JVS, X, dble(ISING)
    close (11); close (12)
  end subroutine run_ops
  subroutine run_dense(mech, NVAR, NFIX, NREACT, fin, fout)
    integer, intent(in) :: mech, NVAR, NFIX, NREACT
    character(len=*), intent(in) :: fin, fout
    double precision :: ropt(40), tt(5)
    double precision, allocatable :: ATOL(:), RTOL(:), AROW(:, :), RROW(:, :), VAR(:, :), FIX(:, :), RCONST(:, :), TEXIT(:), HEXIT(:), TS(:), YS(:, :, :), rec(:)
    integer :: IPAR(20), n, ntol, ns, i
    integer, allocatable :: IERR(:), ISTAT(:, :), NOUT(:)
    open (11, file=fin, access='stream', form='unformatted', status='old')
    open (12, file=fout, access='stream', form='unformatted', status='replace')
    allocate (ATOL(NVAR), RTOL(NVAR))
    read (11) ropt, ATOL, RTOL, tt      ! tt: TSTART, TEND, ncell, ntol, ns
    IPAR = int(ropt(1:20))
    n = int(tt(3))
    ntol = int(tt(4))
    ns = int(tt(5))
    allocate (TS(ns))
    read (11) TS
    allocate (VAR(NVAR, n), FIX(NFIX, n), RCONST(NREACT, n), TEXIT(n), HEXIT(n), IERR(n), ISTAT(8, n), NOUT(n), YS(NVAR, n, ns))
    allocate (rec(NVAR + NFIX + NREACT), AROW(max(ntol, 1), n), RROW(max(ntol, 1), n))
    YS = -7.25d0
    NOUT = -77
    do i = 1, n
       read (11) rec
       VAR(:, i) = rec(1:NVAR)
       FIX(:, i) = rec(NVAR + 1:NVAR + NFIX)
       RCONST(:, i) = rec(NVAR + NFIX + 1:)
       if (ntol > 0) then
          AROW(:, i) = ATOL(1:ntol)
          RROW(:, i) = RTOL(1:ntol)
       end if
    end do
    if (ntol == 0) then
       select case (mech)
       case (0); call ROSENBROCK_BATCH_DENSE_g(n, VAR, FIX, RCONST, tt(1), tt(2), ATOL, RTOL, ropt(21:40), IPAR, TEXIT, HEXIT, IERR, ISTAT, ns, TS, YS, NOUT)
       case (1); call ROSENBROCK_BATCH_DENSE_a(n, VAR, FIX, RCONST, tt(1), tt(2), ATOL, RTOL, ropt(21:40), IPAR, TEXIT, HEXIT, IERR, ISTAT, ns, TS, YS, NOUT)
       case (2); call ROSENBROCK_BATCH_DENSE_t(n, VAR, FIX, RCONST, tt(1), tt(2), ATOL, RTOL, ropt(21:40), IPAR, TEXIT, HEXIT, IERR, ISTAT, ns, TS, YS, NOUT)
       end select
    else
       select case (mech)
       case (0); call ROSENBROCK_BATCH_DENSE_CELLS_g(n, VAR, FIX, RCONST, tt(1), tt(2), AROW, RROW, ntol, ropt(21:40), IPAR, TEXIT, HEXIT, IERR, ISTAT, ns, TS, YS, NOUT)
       case (1); call ROSENBROCK_BATCH_DENSE_CELLS_a(n, VAR, FIX, RCONST, tt(1), tt(2), AROW, RROW, ntol, ropt(21:40), IPAR, TEXIT, HEXIT, IERR, ISTAT, ns, TS, YS, NOUT)
       case (2); call ROSENBROCK_BATCH_DENSE_CELLS_t(n, VAR, FIX, RCONST, tt(1), tt(2), AROW, RROW, ntol, ropt(21:40), IPAR, TEXIT, HEXIT, IERR, ISTAT, ns, TS, YS, NOUT)
       end select
    end if
    do i = 1, n
       write (12) VAR(:, i), TEXIT(i), HEXIT(i), dble(IERR(i)), dble(ISTAT(:, i)), dble(NOUT(i))
    end do
    write (12) YS
    close (11); close (12)
  end subroutine run_dense
  subroutine run_series(mech, NVAR, NFIX, NREACT, fin, fout)
    integer, intent(in) :: mech, NVAR, NFIX, NREACT
    character(len=*), intent(in) :: fin, fout
    double precision :: ropt(40), tt(4)
    double precision, allocatable :: ATOL(:), RTOL(:), AROW(:, :), RROW(:, :), TIMES(:), VAR(:, :), FIX(:, :), RCONST(:, :), VSER(:, :, :), TEXIT(:, :), HEXIT(:, :), rec(:)
    integer :: IPAR(20), n, nleg, ntol, i, l
    logical :: carry
    integer, allocatable :: IERR(:, :), ISTAT(:, :, :)
    open (11, file=fin, access='stream', form='unformatted', status='old')
    open (12, file=fout, access='stream', form='unformatted', status='replace')
    allocate (ATOL(NVAR), RTOL(NVAR))
    read (11) ropt, ATOL, RTOL, tt      ! tt: ncell, nleg, carry, ntol
    IPAR = int(ropt(1:20))
    n = int(tt(1))
    nleg = int(tt(2))
    carry = tt(3) /= 0.d0
    ntol = int(tt(4))
    allocate (TIMES(nleg + 1))
    read (11) TIMES
    allocate (VAR(NVAR, n), FIX(NFIX, n), RCONST(NREACT, n), VSER(NVAR, n, nleg), TEXIT(n, nleg), HEXIT(n, nleg), IERR(n, nleg), ISTAT(8, n, nleg))
    allocate (rec(NVAR + NFIX + NREACT), AROW(max(ntol, 1), n), RROW(max(ntol, 1), n))
    do i = 1, n
       read (11) rec
       VAR(:, i) = rec(1:NVAR)
       FIX(:, i) = rec(NVAR + 1:NVAR + NFIX)
       RCONST(:, i) = rec(NVAR + NFIX + 1:)
       if (ntol > 0) then
          AROW(:, i) = ATOL(1:ntol)
          RROW(:, i) = RTOL(1:ntol)
       end if
    end do
    if (ntol == 0) then
       select case (mech)
       case (0); call ROSENBROCK_BATCH_SERIES_g(n, VAR, FIX, RCONST, nleg, TIMES, ATOL, RTOL, ropt(21:40), IPAR, carry, VSER, TEXIT, HEXIT, IERR, ISTAT)
       case (1); call ROSENBROCK_BATCH_SERIES_a(n, VAR, FIX, RCONST, nleg, TIMES, ATOL, RTOL, ropt(21:40), IPAR, carry, VSER, TEXIT, HEXIT, IERR, ISTAT)
       case (2); call ROSENBROCK_BATCH_SERIES_t(n, VAR, FIX, RCONST, nleg, TIMES, ATOL, RTOL, ropt(21:40), IPAR, carry, VSER, TEXIT, HEXIT, IERR, ISTAT)
       end select
    else
       select case (mech)
       case (0); call ROSENBROCK_BATCH_SERIES_CELLS_g(n, VAR, FIX, RCONST, nleg, TIMES, AROW, RROW, ntol, ropt(21:40), IPAR, carry, VSER, TEXIT, HEXIT, IERR, ISTAT)
       case (1); call ROSENBROCK_BATCH_SERIES_CELLS_a(n, VAR, FIX, RCONST, nleg, TIMES, AROW, RROW, ntol, ropt(21:40), IPAR, carry, VSER, TEXIT, HEXIT, IERR, ISTAT)
       case (2); call ROSENBROCK_BATCH_SERIES_CELLS_t(n, VAR, FIX, RCONST, nleg, TIMES, AROW, RROW, ntol, ropt(21:40), IPAR, carry, VSER, TEXIT, HEXIT, IERR, ISTAT)
       end select
    end if
    do l = 1, nleg
       do i = 1, n
          write (12) VSER(:, i, l), TEXIT(i, l), HEXIT(i, l), dble(IERR(i, l)), dble(ISTAT(:, i, l))
       end do
    end do
    close (11); close (12)
  end subroutine run_series
  subroutine run_series_rates(mech, NVAR, NFIX, NREACT, fin, fout, lin, flx)
    integer, intent(in) :: mech, NVAR, NFIX, NREACT
    character(len=*), intent(in) :: fin, fout
    logical, intent(in) :: lin      ! <MG|MA|MT>: RCONST holds nrcleg = nleg + 1 node blocks, rate constants linear in time over each leg
    logical, intent(in) :: flx      ! <BG|BA|BT>: the reaction flux of every leg too
    double precision, allocatable :: FLUX(:, :, :)
    double precision :: ropt(40), tt(6)
    double precision, allocatable :: ATOL(:), RTOL(:), AROW(:, :), RROW(:, :), TIMES(:), VAR(:, :), FIX(:, :, :), RCONST(:, :, :), VSER(:, :, :), TEXIT(:, :), HEXIT(:, :)
    integer :: IPAR(20), n, nleg, ntol, nrc, nfx, i, l
    logical :: carry
    integer, allocatable :: IERR(:, :), ISTAT(:, :, :)
    open (11, file=fin, access='stream', form='unformatted', status='old')
    open (12, file=fout, access='stream', form='unformatted', status='replace')
    allocate (ATOL(NVAR), RTOL(NVAR))
    read (11) ropt, ATOL, RTOL, tt      ! tt: ncell, nleg, carry, ntol, nrcleg, nfixleg
    IPAR = int(ropt(1:20))
    n = int(tt(1))
    nleg = int(tt(2))
    carry = tt(3) /= 0.d0
    ntol = int(tt(4))
    nrc = int(tt(5))
    nfx = int(tt(6))
    allocate (TIMES(nleg + 1))
    read (11) TIMES
    allocate (VAR(NVAR, n), FIX(NFIX, n, nfx), RCONST(NREACT, n, nrc), VSER(NVAR, n, nleg), TEXIT(n, nleg), HEXIT(n, nleg), IERR(n, nleg), ISTAT(8, n, nleg))
    allocate (AROW(max(ntol, 1), n), RROW(max(ntol, 1), n))
    read (11) VAR, FIX, RCONST
    do i = 1, n
       if (ntol > 0) then
          AROW(:, i) = ATOL(1:ntol)
          RROW(:, i) = RTOL(1:ntol)
       end if
    end do
    if (flx) then
       allocate (FLUX(NREACT, n, nleg))
       if (ntol == 0) then
          select case (mech)
          case (0); call ROSENBROCK_BATCH_SERIES_FLUX_g(n, VAR, FIX, RCONST, nleg, nrc, nfx, TIMES, ATOL, RTOL, ropt(21:40), IPAR, carry, VSER, TEXIT, HEXIT, IERR, ISTAT, &
               FLUX)
          case (1); call ROSENBROCK_BATCH_SERIES_FLUX_a(n, VAR, FIX, RCONST, nleg, nrc, nfx, TIMES, ATOL, RTOL, ropt(21:40), IPAR, carry, VSER, TEXIT, HEXIT, IERR, ISTAT, &
               FLUX)
          case (2); call ROSENBROCK_BATCH_SERIES_FLUX_t(n, VAR, FIX, RCONST, nleg, nrc, nfx, TIMES, ATOL, RTOL, ropt(21:40), IPAR, carry, VSER, TEXIT, HEXIT, IERR, ISTAT, &
               FLUX)
          end select
       else
          select case (mech)
          case (0); call ROSENBROCK_BATCH_SERIES_FLUX_CELLS_g(n, VAR, FIX, RCONST, nleg, nrc, nfx, TIMES, AROW, RROW, ntol, ropt(21:40), IPAR, carry, VSER, TEXIT, HEXIT, &
               IERR, ISTAT, FLUX)
          case (1); call ROSENBROCK_BATCH_SERIES_FLUX_CELLS_a(n, VAR, FIX, RCONST, nleg, nrc, nfx, TIMES, AROW, RROW, ntol, ropt(21:40), IPAR, carry, VSER, TEXIT, HEXIT, &
               IERR, ISTAT, FLUX)
          case (2); call ROSENBROCK_BATCH_SERIES_FLUX_CELLS_t(n, VAR, FIX, RCONST, nleg, nrc, nfx, TIMES, AROW, RROW, ntol, ropt(21:40), IPAR, carry, VSER, TEXIT, HEXIT, &
               IERR, ISTAT, FLUX)
          end select
       end if
    else if (lin) then
       if (ntol /= 0 .or. nrc /= nleg + 1) stop 'the series with rate constants linear in time: ntol = 0 and nrcleg = nleg + 1'
       select case (mech)
       case (0); call ROSENBROCK_BATCH_SERIES_LINRATES_g(n, VAR, FIX, RCONST, nleg, nfx, TIMES, ATOL, RTOL, ropt(21:40), IPAR, carry, VSER, TEXIT, HEXIT, IERR, ISTAT)
       case (1); call ROSENBROCK_BATCH_SERIES_LINRATES_a(n, VAR, FIX, RCONST, nleg, nfx, TIMES, ATOL, RTOL, ropt(21:40), IPAR, carry, VSER, TEXIT, HEXIT, IERR, ISTAT)
       case (2); call ROSENBROCK_BATCH_SERIES_LINRATES_t(n, VAR, FIX, RCONST, nleg, nfx, TIMES, ATOL, RTOL, ropt(21:40), IPAR, carry, VSER, TEXIT, HEXIT, IERR, ISTAT)
       end select
    else if (ntol == 0) then
       select case (mech)
       case (0); call ROSENBROCK_BATCH_SERIES_RATES_g(n, VAR, FIX, RCONST, nleg, nrc, nfx, TIMES, ATOL, RTOL, ropt(21:40), IPAR, carry, VSER, TEXIT, HEXIT, IERR, ISTAT)
       case (1); call ROSENBROCK_BATCH_SERIES_RATES_a(n, VAR, FIX, RCONST, nleg, nrc, nfx, TIMES, ATOL, RTOL, ropt(21:40), IPAR, carry, VSER, TEXIT, HEXIT, IERR, ISTAT)
       case (2); call ROSENBROCK_BATCH_SERIES_RATES_t(n, VAR, FIX, RCONST, nleg, nrc, nfx, TIMES, ATOL, RTOL, ropt(21:40), IPAR, carry, VSER, TEXIT, HEXIT, IERR, ISTAT)
       end select
    else
       select case (mech)
       case (0); call ROSENBROCK_BATCH_SERIES_RATES_CELLS_g(n, VAR, FIX, RCONST, nleg, nrc, nfx, TIMES, AROW, RROW, ntol, ropt(21:40), IPAR, carry, VSER, TEXIT, HEXIT, &
            IERR, ISTAT)
       case (1); call ROSENBROCK_BATCH_SERIES_RATES_CELLS_a(n, VAR, FIX, RCONST, nleg, nrc, nfx, TIMES, AROW, RROW, ntol, ropt(21:40), IPAR, carry, VSER, TEXIT, HEXIT, &
            IERR, ISTAT)
       case (2); call ROSENBROCK_BATCH_SERIES_RATES_CELLS_t(n, VAR, FIX, RCONST, nleg, nrc, nfx, TIMES, AROW, RROW, ntol, ropt(21:40), IPAR, carry, VSER, TEXIT, HEXIT, &
            IERR, ISTAT)
       end select
    end if
    do l = 1, nleg
       do i = 1, n
          write (12) VSER(:, i, l), TEXIT(i, l), HEXIT(i, l), dble(IERR(i, l)), dble(ISTAT(:, i, l))
          if (flx) write (12) FLUX(:, i, l)
       end do
    end do
    close (11); close (12)
  end subroutine run_series_rates
  subroutine run_env(mech, NVAR, NFIX, NREACT, NENV, fin, fout)
    integer, intent(in) :: mech, NVAR, NFIX, NREACT, NENV
    character(len=*), intent(in) :: fin, fout
    double precision, allocatable :: VAR(:, :), FIX(:, :), ENV(:, :), RCONST(:, :), TEXIT(:), HEXIT(:), rec(:)
    integer, allocatable :: IERR(:), ISTAT(:, :)
    double precision :: rn, tin, tout
    integer :: n, i
    open (11, file=fin, access='stream', form='unformatted', status='old')
    open (12, file=fout, access='stream', form='unformatted', status='replace')
    read (11) rn
    n = int(rn)
    allocate (VAR(NVAR, n), FIX(NFIX, n), ENV(NENV, n), RCONST(NREACT, n), TEXIT(n), HEXIT(n), IERR(n), ISTAT(8, n), rec(NVAR + NFIX + NENV))
    do i = 1, n
       read (11) rec
       VAR(:, i) = rec(1:NVAR)
       FIX(:, i) = rec(NVAR + 1:NVAR + NFIX)
       ENV(:, i) = rec(NVAR + NFIX + 1:)
    end do
    tin = 0.d0
    tout = 10.d0
    select case (mech)
    case (0)
       call UPDATE_RCONST_BATCH_g(n, ENV, RCONST)
       call INTEGRATE_BATCH_ENV_g(n, VAR, FIX, ENV, tin, tout, TEXIT, HEXIT, IERR, ISTAT)
    case (1)
       call UPDATE_RCONST_BATCH_a(n, ENV, RCONST)
       call INTEGRATE_BATCH_ENV_a(n, VAR, FIX, ENV, tin, tout, TEXIT, HEXIT, IERR, ISTAT)
    case (2)
       call UPDATE_RCONST_BATCH_t(n, ENV, RCONST)
       call INTEGRATE_BATCH_ENV_t(n, VAR, FIX, ENV, tin, tout, TEXIT, HEXIT, IERR, ISTAT)
    end select
    do i = 1, n
       write (12) VAR(:, i)
    end do
    do i = 1, n
       write (12) dble(IERR(i)), dble(ISTAT(:, i))
    end do
    do i = 1, n
       write (12) RCONST(:, i)
    end do
    close (11); close (12)
  end subroutine run_env
  subroutine run_liq(what, mech, fin, fout)
    use mistra_kpp_liq
    character(len=1), intent(in) :: what
    integer, intent(in) :: mech
    character(len=*), intent(in) :: fin, fout
    double precision :: h(8)
    integer :: nl, nka, nkt, nkc, nspec, ka, ifeed, nkc_l, j6
    integer, allocatable :: kw(:)
    double precision, allocatable :: tmp(:), rq(:), ff(:), cw(:), cm(:), freep(:), alpha(:), vmean(:), xkmt(:), t(:), p(:), vt(:), henry(:), conv2(:), xgamma(:), &
                                     xkef(:), xkeb(:)
    open (11, file=fin, access='stream', form='unformatted', status='old')
    open (12, file=fout, access='stream', form='unformatted', status='replace')
    select case (what)
    case ('K')
       read (11) h
       nl = int(h(1)); nka = int(h(2)); nkt = int(h(3)); nkc = int(h(4)); nspec = int(h(5)); ka = int(h(6)); ifeed = int(h(7)); nkc_l = int(h(8))
       allocate (tmp(nka), kw(nka), rq(nkt * nka), ff(nkt * nka * nl), cw(nkc * nl), cm(nkc * nl), freep(nl), alpha(nspec * nl), vmean(nspec * nl), &
                 xkmt(nspec * nkc * nl), t(nl), p(nl), vt(nkc * nl))
       read (11) tmp; kw = int(tmp)
       read (11) rq, ff, cw, cm, freep, alpha, vmean, xkmt, t, p, vt
       call FAST_K_MT_BATCH(mech, nl, ff, rq, nka, kw, ka, ifeed, nkc_l, cw, cm, freep, alpha, vmean, xkmt, t, p, vt)
       write (12) xkmt, vt
    case ('H')
       read (11) h(1:2)
       nl = int(h(1)); nspec = int(h(2))
       allocate (t(nl), henry(nspec * nl))
       read (11) t
       henry = -7.d0
       call HENRY_BATCH(mech, nl, t, henry)
       write (12) henry
    case ('V')
       read (11) h(1:2)
       nl = int(h(1)); nspec = int(h(2))
       allocate (t(nl), vmean(nspec * nl))
       read (11) t
       vmean = -7.d0
       call V_MEAN_BATCH(mech, nl, t, vmean)
       write (12) vmean
    case ('S')
       read (11) h(1:4)
       nl = int(h(1)); nspec = int(h(2))
       allocate (t(5 * nl), alpha(nspec * nl))
       read (11) t
       alpha = -7.d0
       call ST_COEFF_BATCH(mech, nl, h(3) /= 0.d0, h(4) /= 0.d0, t, alpha)
       write (12) alpha
    case ('C')
       call run_cw_rc()
    case ('R')
       read (11) h(1:1)
       nl = int(h(1))
       allocate (t(nl), freep(nl), rq(2 * nl), vmean(4 * nl), xkmt(8 * nl), henry(nl), alpha(4 * nl))
       read (11) t, freep, rq, vmean
       alpha = vmean      ! (gas: the Henry entries before the call, in/out)
       xkmt = -7.d0; henry = -7.d0
       call DRY_RATES_BATCH(mech == 1, nl, t, freep, rq, vmean, xkmt, henry, alpha)
       write (12) xkmt, henry, alpha
    case ('Q')
       read (11) h(1:4)
       nl = int(h(1)); nkc = int(h(2)); j6 = int(h(3)); nspec = int(h(4))
       allocate (t(nl), conv2(nkc * nl), xgamma(j6 * nkc * nl), xkef(nspec * nkc * nl), xkeb(nspec * nkc * nl))
       read (11) t, conv2, xgamma, xkef, xkeb
       call EQUIL_CO_BATCH(mech, nl, nkc, j6, t, conv2, xgamma, xkef, xkeb)
       write (12) xkef, xkeb
    end select
    close (11); close (12)
  end subroutine run_liq
  subroutine run_cw_rc()      ! (units 11 and 12 are open)
    use mistra_kpp_liq
    double precision :: h(6), crys4(4)
    integer :: nl, nkt, nka, ka, ifeed, nb
    logical :: dry
    integer, allocatable :: kw(:), cloud(:), below(:)
    double precision, allocatable :: tmp(:), rq(:), e(:), ff(:), feu(:), rc(:), cw(:), cm(:), conv2(:)
    read (11) h
    nl = int(h(1)); nkt = int(h(2)); nka = int(h(3)); dry = h(4) /= 0.d0; ka = int(h(5)); ifeed = int(h(6))
    nb = merge(2, 4, dry)
    allocate (tmp(nka), kw(nka), rq(nkt * nka), e(nkt), ff(nkt * nka * nl), feu(nl), cloud(4 * nl), below(nl), rc(nb * nl), cw(nb * nl), cm(nb * nl), conv2(nb * nl))
    read (11) tmp; kw = int(tmp)
    read (11) rq, e, crys4, ff, feu
    deallocate (tmp); allocate (tmp(4 * nl))
    read (11) tmp; cloud = int(tmp)
    rc = -7.d0; cw = -7.d0; cm = -7.d0; conv2 = -7.d0; below = -7
    call CW_RC_BATCH(nl, nkt, nka, dry, ff, rq, e, kw, ka, ifeed, feu, cloud, crys4, rc, cw, cm, conv2, below)
    write (12) rc, cw, cm, conv2, dble(below)
    ! once more with the spectrum registered for direct transfers, as LIQ_PIN_ONCE does for the model's /cb52/ (same bits; the test compares)
    call PIN_HOST(ff, nkt * nka * nl)
    rc = -7.d0; cw = -7.d0; cm = -7.d0; conv2 = -7.d0; below = -7
    call CW_RC_BATCH(nl, nkt, nka, dry, ff, rq, e, kw, ka, ifeed, feu, cloud, crys4, rc, cw, cm, conv2, below)
    write (12) rc, cw, cm, conv2, dble(below)
  end subroutine run_cw_rc
  subroutine run_drive(fin, fout, twice, policy)
    use mistra_kpp_drive
    character(len=*), intent(in) :: fin, fout
    logical, intent(in) :: twice      ! two consecutive steps under step reuse instead of nrep repetitions of one
    logical, intent(in) :: policy     ! the step under an integrator policy, read in front of the header
    double precision :: pol(3)
    integer :: ierr_pol
    external :: MISTRA_SET_POLICY_g, MISTRA_SET_POLICY_a, MISTRA_SET_POLICY_t
    integer, parameter :: j2 = 121, j6 = 55, nkc = 4, nbgs = 122      ! global_params.f90:96-103, bud_s_g.f:63
    integer, parameter :: nenv(3) = [nenv_g, nenv_a, nenv_t]
    double precision :: hdr(7)
    integer :: n, j1, j5, nlev, nrxn, nl, nrep, i, m, rep, cnt, k, ierr, istat(8)
    integer, allocatable :: gm(:, :, :), gk(:, :), rm(:, :, :), rk(:, :), il(:), lmech(:), lk(:)
    double precision, allocatable :: tmp(:), s1(:, :), s3(:, :), sl1(:, :, :), sion1(:, :, :), bg(:, :, :), bgs(:, :, :), lscal(:, :), lenv(:, :)
    double precision, allocatable :: s1_0(:, :), s3_0(:, :), sl1_0(:, :, :), sion1_0(:, :, :), bg_0(:, :, :), bgs_0(:, :, :), times(:, :)
    double precision :: texit, hexit, hlast, tkpp
    double precision, allocatable :: steps(:, :, :)
    integer :: j
    integer(8) :: c0, c1, c2, rate
    external :: MISTRA_STEP_REUSE_g, MISTRA_STEP_REUSE_a, MISTRA_STEP_REUSE_t
    external :: MISTRA_RATES_ENV_SET_g, MISTRA_RATES_ENV_SET_a, MISTRA_RATES_ENV_SET_t, KPP_DRIVE_STAGE_g, KPP_DRIVE_STAGE_a, KPP_DRIVE_STAGE_t
    open (11, file=fin, access='stream', form='unformatted', status='old')
    open (12, file=fout, access='stream', form='unformatted', status='replace')
    if (policy) read (11) pol
    read (11) hdr
    n = int(hdr(1)); j1 = int(hdr(2)); j5 = int(hdr(3)); nlev = int(hdr(4)); nrxn = int(hdr(5)); nl = int(hdr(6)); nrep = int(hdr(7))
    allocate (gm(2, j1, 3), gk(j1, 3), rm(2, j5, 3), rk(j5, 3), il(nlev), tmp(max(2 * j1, 2 * j5, nlev)))
    do m = 1, 3
       read (11) tmp(1:2 * j1); gm(:, :, m) = reshape(int(tmp(1:2 * j1)), [2, j1])
       read (11) tmp(1:j1); gk(:, m) = int(tmp(1:j1))
       read (11) tmp(1:2 * j5); rm(:, :, m) = reshape(int(tmp(1:2 * j5)), [2, j5])
       read (11) tmp(1:j5); rk(:, m) = int(tmp(1:j5))
    end do
    read (11) tmp(1:nlev); il = int(tmp(1:nlev))
    allocate (s1(j1, n), s3(j5, n), sl1(j2, nkc, n), sion1(j6, nkc, n), bg(2, nrxn, nlev), bgs(2, nbgs, n))
    read (11) s1, s3, sl1, sion1, bg, bgs
    allocate (lmech(nl), lk(nl), lscal(2, nl), lenv(maxval(nenv), nl), times(2, nrep))
    do i = 1, nl
       read (11) hdr(1:4)
       lmech(i) = int(hdr(1)); lk(i) = int(hdr(2)); lscal(:, i) = hdr(3:4)
       read (11) lenv(1:nenv(lmech(i)), i)
    end do
    s1_0 = s1; s3_0 = s3; sl1_0 = sl1; sion1_0 = sion1; bg_0 = bg; bgs_0 = bgs
    do m = 1, 3      ! once per run, as KPP_DRIVE_RUN does on its first call (here only for the mechanisms the recorded step has layers of: the
       if (any(lmech == m)) call kpp_drive_maps(m, j1, gm(:, :, m), gk(:, m), j5, rm(:, :, m), rk(:, m))      ! file holds real maps only for those)
    end do
    if (policy) then
       ierr_pol = 0
       if (any(lmech == 1)) call MISTRA_SET_POLICY_g(int(pol(1)), pol(2), pol(3), ierr_pol)
       if (ierr_pol == 0 .and. any(lmech == 2)) call MISTRA_SET_POLICY_a(int(pol(1)), pol(2), pol(3), ierr_pol)
       if (ierr_pol == 0 .and. any(lmech == 3)) call MISTRA_SET_POLICY_t(int(pol(1)), pol(2), pol(3), ierr_pol)
       if (ierr_pol /= 0) stop 'the policy was refused'
    end if
    if (twice) then
       nrep = 2
       deallocate (times); allocate (times(2, nrep), steps(14, nl, nrep))
       call MISTRA_STEP_REUSE_g(.true.); call MISTRA_STEP_REUSE_a(.true.); call MISTRA_STEP_REUSE_t(.true.)
    end if
    do rep = 1, nrep      ! (the first repetition pays the library's start-up and the first allocation of the staging blocks)
       if (.not. twice .or. rep == 1) then
          s1 = s1_0; s3 = s3_0; sl1 = sl1_0; sion1 = sion1_0; bg = bg_0; bgs = bgs_0
       end if
       tkpp = merge(10.d0 * dble(rep - 1), 0.d0, twice)
       call system_clock(c0, rate)
       call kpp_drive_begin
       do i = 1, nl       ! kpp_driver's layer loop: per-layer set-up and the x_drive prologue (here: the recorded values back into the COMMON blocks), then the hand-over
          select case (lmech(i))
          case (1); call MISTRA_RATES_ENV_SET_g(lenv(:, i)); call KPP_DRIVE_STAGE_g(lk(i), lscal(1, i), lscal(2, i))
          case (2); call MISTRA_RATES_ENV_SET_a(lenv(:, i)); call KPP_DRIVE_STAGE_a(lk(i), lscal(1, i), lscal(2, i))
          case (3); call MISTRA_RATES_ENV_SET_t(lenv(:, i)); call KPP_DRIVE_STAGE_t(lk(i), lscal(1, i), lscal(2, i))
          end select
       end do
       call system_clock(c1)
       call kpp_drive_run_arrays(tkpp, 10.d0, n, s1, s3, sl1, sion1, nrxn, nlev, il, bg, bgs)
       call system_clock(c2)
       times(1, rep) = 1.d3 * dble(c1 - c0) / dble(rate)
       times(2, rep) = 1.d3 * dble(c2 - c1) / dble(rate)
       if (twice) then      ! per mechanism in staging order, as below
          j = 0
          do m = 1, 3
             do i = 1, kpp_drive_count(m)
                j = j + 1
                call kpp_drive_last(m, i, k, ierr, istat, texit, hexit, hlast)
                steps(:, j, rep) = [dble(m), dble(k), dble(ierr), dble(istat), texit, hexit, hlast]
             end do
          end do
       end if
    end do
    write (12) s1, s3, sl1, sion1, bg, bgs
    if (twice) then
       write (12) steps
       close (11); close (12)
       return
    end if
    do m = 1, 3           ! per mechanism in staging order (= layer order within the mechanism)
       cnt = kpp_drive_count(m)
       do i = 1, cnt
          call kpp_drive_last(m, i, k, ierr, istat, texit, hexit)
          write (12) dble(m), dble(k), dble(ierr), dble(istat), texit, hexit
       end do
    end do
    write (12) times
    close (11); close (12)
  end subroutine run_drive
end program shim_driver
