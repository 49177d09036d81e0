! Fortran side of the drop-in boundary: the reference's own subroutine surface,
!     SUBROUTINE INTEGRATE_g / INTEGRATE_a / INTEGRATE_t (TIN, TOUT)          gas.f:710 | aer.f:1408 | tot.f:2812
! implemented on top of the C ABI (include/mistra_chem.h) through ISO_C_BINDING, plus the batched form a two-pass
! kpp_driver calls once per mechanism and 10-s step (INTEGRATION.md):
!     SUBROUTINE INTEGRATE_BATCH_g / _a / _t (NCELL, VAR, FIX, RCONST, TIN, TOUT, TEXIT, HEXIT, IERR, ISTAT)
!
! Same names, same two REAL*8 arguments by reference, same data path: everything else travels through
! COMMON /GDATA_x/, whose member order is restated below from gas_Global.h:29-58 (aer_Global.h, tot_Global.h alike):
!     C(NSPEC) [= VAR(NVAR) followed by FIX(NFIX)], RCONST(NREACT), TIME, DT, ATOL(NVAR), RTOL(NVAR), STEPMIN, STEPMAX
! A maintainer drops this file into src/ and removes (or renames) the three generated INTEGRATE_x routines; x_drive,
! Update_RCONST_x, the budgets and kpp_driver stay untouched (INTEGRATION.md shows the link line and the
! link-time alternative that needs no source edit).  Behaviour kept from the reference: VAR is advanced in place,
! TIN returns the exit time, STEPMIN the last step, RTOL/ATOL are (re)set to 1e-3 / 1e-25, an unsuccessful
! integration writes the lines of ros_ErrorMsg_x (gas.f:1474-1509) and of INTEGRATE_x (gas.f:764-767) to unit 6 and the
! model carries on; so does ros_PrepareMatrix_x's 'Warning: LU Decomposition returned ising =' line with the row of the zero
! pivot (gas.f:1456; the kernel records the rows, mistra_chem_singular_rows hands them out), once per failed decomposition.
!
! A model whose INTEGRATE_x carries other options than the generated ones (gas.f:739-746 edited: tolerances, step bounds, factors) hands them
! over once, after which every call above uses them (include/mistra_chem.h: mistra_chem_set_options):
!     SUBROUTINE MISTRA_SET_OPTIONS_g / _a / _t (IPAR, RPAR, ATOL, RTOL, IERR)      Rosenbrock_x's own IPAR(20), RPAR(20), AbsTol(NVAR), RelTol(NVAR)
!     SUBROUTINE MISTRA_CLEAR_OPTIONS_g / _a / _t ()                                 back to INTEGRATE_x's values
! IERR = 1, or the code Rosenbrock_x would return for them (gas.f:936-1053): its ros_ErrorMsg_x lines go to unit 6 and the previous options stay.
!
! OPT-IN, not the reference's behaviour (include/mistra_chem.h: mistra_chem_set_step_reuse): every layer starts at the last accepted step size of its previous
! column step of the mechanism instead of Hstart = 1e-3 (gas.f:743).  Call once after start-up, next to MISTRA_SET_OPTIONS_x if that is called:
!     SUBROUTINE MISTRA_STEP_REUSE_g / _a / _t (ON)                                  ON logical; the single-pass batched driver (KPP_DRIVE_RUN) keeps the steps
! and for a caller that orders its own batches, the batched form with a first step size per cell (<= 0: the reference's), HEXIT of one call being HSTART of the next:
!     SUBROUTINE INTEGRATE_BATCH_H_g / _a / _t (NCELL, VAR, FIX, RCONST, TIN, TOUT, HSTART, TEXIT, HEXIT, IERR, ISTAT)
!
! OPT-IN, not the reference's behaviour (include/mistra_chem.h: mistra_chem_set_policy; INTEGRATION.md 4l): another of Rosenbrock_x's five methods and / or
! a cell-relative AbsTol = MAX(ATOL_FLOOR, ATOL_FACTOR * MAXVAL(ABS(VAR))) for every call above and for the single-pass batched driver (KPP_DRIVE_RUN);
! everything else stays the options in force.  Call once after start-up, next to MISTRA_SET_OPTIONS_x if that is called:
!     SUBROUTINE MISTRA_SET_POLICY_g / _a / _t (METHOD, ATOL_FACTOR, ATOL_FLOOR, IERR)  METHOD 1 .. 5 (2 keeps Ros3; 0 is refused), ATOL_FACTOR 0 = the options' AbsTol
!     SUBROUTINE MISTRA_CLEAR_POLICY_g / _a / _t ()
! IERR = 0, or 1 where the library refuses the values: its text goes to unit 6 and the previous policy stays.
!
! One layer below INTEGRATE_x: Rosenbrock_x itself for NCELL cells, with its own argument list and ALL FIVE methods (IPAR(4) = 1 Ros2, 2 Ros3, 3 Ros4,
! 4 Rodas3, 5 Rodas4, 0 = Ros4; include/mistra_chem.h: mistra_chem_rosenbrock_ex).  The options are the call's alone: the ones MISTRA_SET_OPTIONS_x put
! in force are neither read nor changed.
!     SUBROUTINE ROSENBROCK_BATCH_g / _a / _t (NCELL, VAR, FIX, RCONST, TSTART, TEND, ATOL, RTOL, RPAR, IPAR, TEXIT, HEXIT, IERR, ISTAT)
! IERR(k) = 1 or Rosenbrock_x's code, also for options it refuses (-1 .. -5: VAR untouched); ros_ErrorMsg_x's lines go to unit 6 for every failed cell.
! The same with tolerances PER CELL (mistra_chem_rosenbrock_cells_ex): ATOL(NTOL,NCELL), RTOL(NTOL,NCELL), NTOL = 1 or NVAR (IPAR(2) = 0 needs NVAR).
! IERR = -5 is then a cell's own result: the cell is reported as ROSENBROCK_BATCH_x reports it, the others run.
!     SUBROUTINE ROSENBROCK_BATCH_CELLS_g / _a / _t (NCELL, VAR, FIX, RCONST, TSTART, TEND, ATOL, RTOL, NTOL, RPAR, IPAR, TEXIT, HEXIT, IERR, ISTAT)
!
! A SERIES of such calls in one launch (mistra_chem_rosenbrock_series_ex; INTEGRATION.md 4m): NLEG legs over TIMES(1:NLEG+1), leg l one call of Rosenbrock_x from
! TIMES(l) to TIMES(l+1) on the state leg l-1 left, the state on the GPU from the first time to the last.  VAR is not changed; leg l returns VSER(:,k,l),
! TEXIT(k,l), HEXIT(k,l), IERR(k,l), ISTAT(:,k,l), bit for bit what ROSENBROCK_BATCH_x called NLEG times returns.  CARRY (logical): a later leg starts with the
! previous leg's HEXIT of the cell where that is > 0 instead of RPAR(3).  ros_ErrorMsg_x's lines go to unit 6 for every failed leg and cell, in leg order.
!     SUBROUTINE ROSENBROCK_BATCH_SERIES_g / _a / _t (NCELL, VAR, FIX, RCONST, NLEG, TIMES, ATOL, RTOL, RPAR, IPAR, CARRY, VSER, TEXIT, HEXIT, IERR, ISTAT)
!     SUBROUTINE ROSENBROCK_BATCH_SERIES_CELLS_g / _a / _t (NCELL, VAR, FIX, RCONST, NLEG, TIMES, ATOL, RTOL, NTOL, RPAR, IPAR, CARRY, VSER, TEXIT, HEXIT, IERR, ISTAT)
! The same with RATE CONSTANTS AND FIX OF THE LEG'S OWN (mistra_chem_rosenbrock_series_rates_ex; INTEGRATION.md 4q): Update_RCONST_x + INTEGRATE_x, NLEG times, in
! one launch.  RCONST(NREACT,NCELL,NRCLEG), FIX(NFIX,NCELL,NFIXLEG), each count 1 (shared by all legs) or NLEG: leg l integrates with RCONST(:,:,l) and FIX(:,:,l),
! bit for bit what ROSENBROCK_BATCH_x called NLEG times with those returns.  The printed lines are the series'.
!     SUBROUTINE ROSENBROCK_BATCH_SERIES_RATES_g / _a / _t (NCELL, VAR, FIX, RCONST, NLEG, NRCLEG, NFIXLEG, TIMES, ATOL, RTOL, RPAR, IPAR, CARRY, VSER, TEXIT, HEXIT,
!                                                            IERR, ISTAT)
!     SUBROUTINE ROSENBROCK_BATCH_SERIES_RATES_CELLS_g / _a / _t (NCELL, VAR, FIX, RCONST, NLEG, NRCLEG, NFIXLEG, TIMES, ATOL, RTOL, NTOL, RPAR, IPAR, CARRY, VSER,
!                                                                  TEXIT, HEXIT, IERR, ISTAT)
! The same with RATE CONSTANTS LINEAR IN TIME OVER EACH LEG (mistra_chem_rosenbrock_series_linrates_ex; INTEGRATION.md 4s): RNODES(NREACT,NCELL,NLEG+1), block l the
! rate constants AT TIMES(l); inside leg l every function evaluation reads them at its own time and the stages add H*gamma*dFdT (IPAR(1) = 0).  FIX(NFIX,NCELL,NFIXLEG)
! stays piecewise constant, NFIXLEG 1 or NLEG.  The printed lines are the series'.
!     SUBROUTINE ROSENBROCK_BATCH_SERIES_LINRATES_g / _a / _t (NCELL, VAR, FIX, RNODES, NLEG, NFIXLEG, TIMES, ATOL, RTOL, RPAR, IPAR, CARRY, VSER, TEXIT, HEXIT,
!                                                               IERR, ISTAT)
! The series with rates WITH THE REACTION FLUX OF EVERY LEG (mistra_chem_rosenbrock_series_flux_ex; INTEGRATION.md 4t): FLUX(NREACT,NCELL,NLEG) behind the argument
! lists of ROSENBROCK_BATCH_SERIES_RATES_x / _RATES_CELLS_x, FLUX(:,k,l) what ROSENBROCK_BATCH_FLUX_x returns for the call that leg l of cell k is; no leg's sum is
! carried into the next, a refused leg's column is zero.  Everything else, the printed lines included, is what those entries return.
!     SUBROUTINE ROSENBROCK_BATCH_SERIES_FLUX_g / _a / _t (NCELL, VAR, FIX, RCONST, NLEG, NRCLEG, NFIXLEG, TIMES, ATOL, RTOL, RPAR, IPAR, CARRY, VSER, TEXIT, HEXIT,
!                                                           IERR, ISTAT, FLUX)
!     SUBROUTINE ROSENBROCK_BATCH_SERIES_FLUX_CELLS_g / _a / _t (NCELL, VAR, FIX, RCONST, NLEG, NRCLEG, NFIXLEG, TIMES, ATOL, RTOL, NTOL, RPAR, IPAR, CARRY, VSER,
!                                                                 TEXIT, HEXIT, IERR, ISTAT, FLUX)
!
! THE REACTION FLUX (mistra_chem_rosenbrock_flux_ex; INTEGRATION.md 4n): ROSENBROCK_BATCH_x / ROSENBROCK_BATCH_CELLS_x with one more result behind their
! argument lists, FLUX(NREACT,NCELL): every reaction's rate integrated over the call by the trapezoid rule on the accepted states.  Everything else is what
! those entries return, bit for bit, ros_ErrorMsg_x's lines and the zero-pivot warnings included; a refused cell's FLUX column is zero.
!     SUBROUTINE ROSENBROCK_BATCH_FLUX_g / _a / _t (NCELL, VAR, FIX, RCONST, TSTART, TEND, ATOL, RTOL, RPAR, IPAR, TEXIT, HEXIT, IERR, ISTAT, FLUX)
!     SUBROUTINE ROSENBROCK_BATCH_FLUX_CELLS_g / _a / _t (NCELL, VAR, FIX, RCONST, TSTART, TEND, ATOL, RTOL, NTOL, RPAR, IPAR, TEXIT, HEXIT, IERR, ISTAT, FLUX)
! DENSE OUTPUT (mistra_chem_rosenbrock_dense_ex; INTEGRATION.md 4o): ROSENBROCK_BATCH_x / ROSENBROCK_BATCH_CELLS_x with NS, TS(NS), YS(NVAR,NCELL,NS),
! NOUT(NCELL) behind their argument lists: the state at the NS sample times TS inside the one call, by the cubic Hermite interpolant between the accepted
! states; NOUT(k) samples of cell k were reached, the columns behind them are zero.  Everything else is what those entries return, bit for bit,
! ros_ErrorMsg_x's lines and the zero-pivot warnings included.
!     SUBROUTINE ROSENBROCK_BATCH_DENSE_g / _a / _t (NCELL, VAR, FIX, RCONST, TSTART, TEND, ATOL, RTOL, RPAR, IPAR, TEXIT, HEXIT, IERR, ISTAT, NS, TS, YS, NOUT)
!     SUBROUTINE ROSENBROCK_BATCH_DENSE_CELLS_g / _a / _t (NCELL, VAR, FIX, RCONST, TSTART, TEND, ATOL, RTOL, NTOL, RPAR, IPAR, TEXIT, HEXIT, IERR, ISTAT,
!                                                          NS, TS, YS, NOUT)
! THE OPERATORS (mistra_chem_ops_ex; INTEGRATION.md 4p): KPP's building blocks at the states the caller gives, NCELL cells per call, no integration; the
! options in force, the policy and step reuse are not involved.  VDOT(NVAR,NCELL) = Fun_x; JVS(LU_NONZERO,NCELL) = Jac_SP_x in LU_CROW / LU_ICOL order, the
! fill-in slots zero; X(NVAR,NCELL,j) solves (SHIFT*I - Jac_SP_x) X = B for the cell's own Fun_x (FUNRHS, logical: j = 1) followed by RHS(NVAR,NCELL,1:NRHS);
! SHIFT(NSHIFT), NSHIFT = 1 (shared) or NCELL; ISING(NCELL) is KppDecomp_x's IER (a cell with ISING > 0 is not factorised: its X is zero).
!     SUBROUTINE FUN_BATCH_g / _a / _t (NCELL, VAR, FIX, RCONST, VDOT)
!     SUBROUTINE JAC_SP_BATCH_g / _a / _t (NCELL, VAR, FIX, RCONST, JVS)
!     SUBROUTINE LINSOLVE_BATCH_g / _a / _t (NCELL, VAR, FIX, RCONST, NSHIFT, SHIFT, FUNRHS, NRHS, RHS, X, ISING)
! THE REPLAY (mistra_chem_rosenbrock_replay_ex; INTEGRATION.md 4r): Ros3 along the step sequences the caller prescribes, every step accepted.  HSTEPS(CAP,HROWS),
! NSTEPS(HROWS), HROWS = 1 (one sequence shared by all cells) or NCELL; step n of cell k is made with H = HSTEPS(n, its row) and leaves Rosenbrock_x's Err in
! ERRLOG(n,k), ERRLOG(CAP,NCELL); entries behind a cell's count are not touched.  IPAR(4) must be 2; RPAR is decoded and ignored; TEND gives the direction.
! TEXIT: the T reached, HEXIT: the last step made.  ros_ErrorMsg_x's lines and the zero-pivot warning (IERR = -8, no halving) as ROSENBROCK_BATCH_x writes them,
! with one difference: the H those lines print is the last step MADE (0 where none was), not the prescribed step that ended the cell — that one is
! HSTEPS(ISTAT(3,k) + 1, the cell's row), which the caller holds.
!     SUBROUTINE ROSENBROCK_BATCH_REPLAY_g / _a / _t (NCELL, VAR, FIX, RCONST, TSTART, TEND, ATOL, RTOL, RPAR, IPAR, CAP, HROWS, HSTEPS, NSTEPS, TEXIT, HEXIT,
!                                                     IERR, ISTAT, ERRLOG)
!     SUBROUTINE ROSENBROCK_BATCH_REPLAY_CELLS_g / _a / _t (NCELL, VAR, FIX, RCONST, TSTART, TEND, ATOL, RTOL, NTOL, RPAR, IPAR, CAP, HROWS, HSTEPS, NSTEPS,
!                                                           TEXIT, HEXIT, IERR, ISTAT, ERRLOG)
module mistra_chem_c_api
  use iso_c_binding
  implicit none
  interface
     function mistra_chem_integrate_common_status(mech, gdata, tin, tout, ierr, t_err, h_err, nsng) &
          bind(C, name="mistra_chem_integrate_common_status") result(rc)
       import :: c_int, c_ptr, c_double, c_int32_t
       integer(c_int), value :: mech
       type(c_ptr), value :: gdata
       real(c_double) :: tin, tout, t_err, h_err
       integer(c_int32_t) :: ierr, nsng
       integer(c_int) :: rc
     end function mistra_chem_integrate_common_status
     function mistra_chem_integrate_ex(mech, ncell, var_in, fix, rconst, tin, tout, var_out, ierr, stats, t_h) &
          bind(C, name="mistra_chem_integrate_ex") result(rc)
       import :: c_int, c_double, c_int32_t
       integer(c_int), value :: mech, ncell
       real(c_double), value :: tin, tout
       real(c_double) :: var_in(*), fix(*), rconst(*), var_out(*), t_h(*)
       integer(c_int32_t) :: ierr(*), stats(*)
       integer(c_int) :: rc
     end function mistra_chem_integrate_ex
     function mistra_chem_integrate_env_ex(mech, ncell, var_in, fix, env, tin, tout, var_out, ierr, stats, t_h) &
          bind(C, name="mistra_chem_integrate_env_ex") result(rc)
       import :: c_int, c_double, c_int32_t
       integer(c_int), value :: mech, ncell
       real(c_double), value :: tin, tout
       real(c_double) :: var_in(*), fix(*), env(*), var_out(*), t_h(*)
       integer(c_int32_t) :: ierr(*), stats(*)
       integer(c_int) :: rc
     end function mistra_chem_integrate_env_ex
     function mistra_chem_init_devices(n_devices, device_ids) bind(C, name="mistra_chem_init_devices") result(rc)
       import :: c_int, c_ptr
       integer(c_int), value :: n_devices
       type(c_ptr), value :: device_ids
       integer(c_int) :: rc
     end function mistra_chem_init_devices
     function mistra_chem_singular_rows(mech, cell, rows8) bind(C, name="mistra_chem_singular_rows") result(rc)
       import :: c_int, c_int32_t
       integer(c_int), value :: mech, cell
       integer(c_int32_t) :: rows8(8)
       integer(c_int) :: rc
     end function mistra_chem_singular_rows
     function mistra_chem_set_options(mech, ipar, rpar, atol, rtol, ierr) bind(C, name="mistra_chem_set_options") result(rc)
       import :: c_int, c_ptr
       integer(c_int), value :: mech
       type(c_ptr), value :: ipar, rpar, atol, rtol, ierr      ! ipar = c_null_ptr clears
       integer(c_int) :: rc
     end function mistra_chem_set_options
     function mistra_chem_integrate_hstart_ex(mech, ncell, var_in, fix, rconst, env, tin, tout, var_out, ierr, stats, t_h, hstart) &
          bind(C, name="mistra_chem_integrate_hstart_ex") result(rc)
       import :: c_int, c_double, c_int32_t, c_ptr
       integer(c_int), value :: mech, ncell
       real(c_double), value :: tin, tout
       real(c_double) :: var_in(*), fix(*), rconst(*), var_out(*), t_h(*)
       type(c_ptr), value :: env      ! c_null_ptr: rate constants are given
       real(c_double), intent(in) :: hstart(*)
       integer(c_int32_t) :: ierr(*), stats(*)
       integer(c_int) :: rc
     end function mistra_chem_integrate_hstart_ex
     function mistra_chem_rosenbrock_ex(mech, ncell, var_in, fix, rconst, tstart, tend, atol, rtol, rpar, ipar, var_out, ierr, stats, t_h) &
          bind(C, name="mistra_chem_rosenbrock_ex") result(rc)
       import :: c_int, c_double, c_int32_t
       integer(c_int), value :: mech, ncell
       real(c_double), value :: tstart, tend
       real(c_double) :: var_in(*), fix(*), rconst(*), var_out(*), t_h(*)
       real(c_double), intent(in) :: atol(*), rtol(*), rpar(20)
       integer(c_int32_t), intent(in) :: ipar(20)
       integer(c_int32_t) :: ierr(*), stats(*)
       integer(c_int) :: rc
     end function mistra_chem_rosenbrock_ex
     function mistra_chem_rosenbrock_cells_ex(mech, ncell, var_in, fix, rconst, tstart, tend, atol, rtol, ntol, rpar, ipar, var_out, ierr, stats, t_h) &
          bind(C, name="mistra_chem_rosenbrock_cells_ex") result(rc)
       import :: c_int, c_double, c_int32_t
       integer(c_int), value :: mech, ncell, ntol
       real(c_double), value :: tstart, tend
       real(c_double) :: var_in(*), fix(*), rconst(*), var_out(*), t_h(*)
       real(c_double), intent(in) :: atol(*), rtol(*), rpar(20)
       integer(c_int32_t), intent(in) :: ipar(20)
       integer(c_int32_t) :: ierr(*), stats(*)
       integer(c_int) :: rc
     end function mistra_chem_rosenbrock_cells_ex
     function mistra_chem_rosenbrock_flux_ex(mech, ncell, var_in, fix, rconst, tstart, tend, atol, rtol, rpar, ipar, var_out, ierr, stats, t_h, flux) &
          bind(C, name="mistra_chem_rosenbrock_flux_ex") result(rc)
       import :: c_int, c_double, c_int32_t
       integer(c_int), value :: mech, ncell
       real(c_double), value :: tstart, tend
       real(c_double) :: var_in(*), fix(*), rconst(*), var_out(*), t_h(*), flux(*)
       real(c_double), intent(in) :: atol(*), rtol(*), rpar(20)
       integer(c_int32_t), intent(in) :: ipar(20)
       integer(c_int32_t) :: ierr(*), stats(*)
       integer(c_int) :: rc
     end function mistra_chem_rosenbrock_flux_ex
     function mistra_chem_rosenbrock_flux_cells_ex(mech, ncell, var_in, fix, rconst, tstart, tend, atol, rtol, ntol, rpar, ipar, var_out, ierr, stats, t_h, &
          flux) bind(C, name="mistra_chem_rosenbrock_flux_cells_ex") result(rc)
       import :: c_int, c_double, c_int32_t
       integer(c_int), value :: mech, ncell, ntol
       real(c_double), value :: tstart, tend
       real(c_double) :: var_in(*), fix(*), rconst(*), var_out(*), t_h(*), flux(*)
       real(c_double), intent(in) :: atol(*), rtol(*), rpar(20)
       integer(c_int32_t), intent(in) :: ipar(20)
       integer(c_int32_t) :: ierr(*), stats(*)
       integer(c_int) :: rc
     end function mistra_chem_rosenbrock_flux_cells_ex
     function mistra_chem_rosenbrock_dense_ex(mech, ncell, var_in, fix, rconst, tstart, tend, atol, rtol, rpar, ipar, var_out, ierr, stats, t_h, ns, ts, &
          ysample, nout) bind(C, name="mistra_chem_rosenbrock_dense_ex") result(rc)
       import :: c_int, c_double, c_int32_t
       integer(c_int), value :: mech, ncell, ns
       real(c_double), value :: tstart, tend
       real(c_double) :: var_in(*), fix(*), rconst(*), var_out(*), t_h(*), ysample(*)
       real(c_double), intent(in) :: atol(*), rtol(*), rpar(20), ts(*)
       integer(c_int32_t), intent(in) :: ipar(20)
       integer(c_int32_t) :: ierr(*), stats(*), nout(*)
       integer(c_int) :: rc
     end function mistra_chem_rosenbrock_dense_ex
     function mistra_chem_rosenbrock_dense_cells_ex(mech, ncell, var_in, fix, rconst, tstart, tend, atol, rtol, ntol, rpar, ipar, var_out, ierr, stats, t_h, &
          ns, ts, ysample, nout) bind(C, name="mistra_chem_rosenbrock_dense_cells_ex") result(rc)
       import :: c_int, c_double, c_int32_t
       integer(c_int), value :: mech, ncell, ntol, ns
       real(c_double), value :: tstart, tend
       real(c_double) :: var_in(*), fix(*), rconst(*), var_out(*), t_h(*), ysample(*)
       real(c_double), intent(in) :: atol(*), rtol(*), rpar(20), ts(*)
       integer(c_int32_t), intent(in) :: ipar(20)
       integer(c_int32_t) :: ierr(*), stats(*), nout(*)
       integer(c_int) :: rc
     end function mistra_chem_rosenbrock_dense_cells_ex
     function mistra_chem_rosenbrock_series_ex(mech, ncell, var_in, fix, rconst, nleg, times, atol, rtol, rpar, ipar, carry_h, hstart, var_series, ierr, &
          stats, t_h) bind(C, name="mistra_chem_rosenbrock_series_ex") result(rc)
       import :: c_int, c_double, c_int32_t, c_ptr
       integer(c_int), value :: mech, ncell, nleg, carry_h
       type(c_ptr), value :: hstart
       real(c_double) :: var_in(*), fix(*), rconst(*), var_series(*), t_h(*)
       real(c_double), intent(in) :: times(*), atol(*), rtol(*), rpar(20)
       integer(c_int32_t), intent(in) :: ipar(20)
       integer(c_int32_t) :: ierr(*), stats(*)
       integer(c_int) :: rc
     end function mistra_chem_rosenbrock_series_ex
     function mistra_chem_rosenbrock_series_cells_ex(mech, ncell, var_in, fix, rconst, nleg, times, atol, rtol, ntol, rpar, ipar, carry_h, hstart, var_series, &
          ierr, stats, t_h) bind(C, name="mistra_chem_rosenbrock_series_cells_ex") result(rc)
       import :: c_int, c_double, c_int32_t, c_ptr
       integer(c_int), value :: mech, ncell, nleg, ntol, carry_h
       type(c_ptr), value :: hstart
       real(c_double) :: var_in(*), fix(*), rconst(*), var_series(*), t_h(*)
       real(c_double), intent(in) :: times(*), atol(*), rtol(*), rpar(20)
       integer(c_int32_t), intent(in) :: ipar(20)
       integer(c_int32_t) :: ierr(*), stats(*)
       integer(c_int) :: rc
     end function mistra_chem_rosenbrock_series_cells_ex
     function mistra_chem_rosenbrock_series_rates_ex(mech, ncell, var_in, fix, rconst, rconst_legs, fix_legs, nleg, times, atol, rtol, rpar, ipar, carry_h, hstart, &
          var_series, ierr, stats, t_h) bind(C, name="mistra_chem_rosenbrock_series_rates_ex") result(rc)
       import :: c_int, c_double, c_int32_t, c_ptr
       integer(c_int), value :: mech, ncell, rconst_legs, fix_legs, nleg, carry_h
       type(c_ptr), value :: hstart
       real(c_double) :: var_in(*), fix(*), rconst(*), var_series(*), t_h(*)
       real(c_double), intent(in) :: times(*), atol(*), rtol(*), rpar(20)
       integer(c_int32_t), intent(in) :: ipar(20)
       integer(c_int32_t) :: ierr(*), stats(*)
       integer(c_int) :: rc
     end function mistra_chem_rosenbrock_series_rates_ex
     function mistra_chem_rosenbrock_series_rates_cells_ex(mech, ncell, var_in, fix, rconst, rconst_legs, fix_legs, nleg, times, atol, rtol, ntol, rpar, ipar, &
          carry_h, hstart, var_series, ierr, stats, t_h) bind(C, name="mistra_chem_rosenbrock_series_rates_cells_ex") result(rc)
       import :: c_int, c_double, c_int32_t, c_ptr
       integer(c_int), value :: mech, ncell, rconst_legs, fix_legs, nleg, ntol, carry_h
       type(c_ptr), value :: hstart
       real(c_double) :: var_in(*), fix(*), rconst(*), var_series(*), t_h(*)
       real(c_double), intent(in) :: times(*), atol(*), rtol(*), rpar(20)
       integer(c_int32_t), intent(in) :: ipar(20)
       integer(c_int32_t) :: ierr(*), stats(*)
       integer(c_int) :: rc
     end function mistra_chem_rosenbrock_series_rates_cells_ex
     function mistra_chem_rosenbrock_series_linrates_ex(mech, ncell, var_in, fix, rconst_nodes, fix_legs, nleg, times, atol, rtol, rpar, ipar, carry_h, hstart, &
          var_series, ierr, stats, t_h) bind(C, name="mistra_chem_rosenbrock_series_linrates_ex") result(rc)
       import :: c_int, c_double, c_int32_t, c_ptr
       integer(c_int), value :: mech, ncell, fix_legs, nleg, carry_h
       type(c_ptr), value :: hstart
       real(c_double) :: var_in(*), fix(*), rconst_nodes(*), var_series(*), t_h(*)
       real(c_double), intent(in) :: times(*), atol(*), rtol(*), rpar(20)
       integer(c_int32_t), intent(in) :: ipar(20)
       integer(c_int32_t) :: ierr(*), stats(*)
       integer(c_int) :: rc
     end function mistra_chem_rosenbrock_series_linrates_ex
     function mistra_chem_rosenbrock_series_flux_ex(mech, ncell, var_in, fix, rconst, rconst_legs, fix_legs, nleg, times, atol, rtol, rpar, ipar, carry_h, hstart, &
          var_series, ierr, stats, t_h, flux_series) bind(C, name="mistra_chem_rosenbrock_series_flux_ex") result(rc)
       import :: c_int, c_double, c_int32_t, c_ptr
       integer(c_int), value :: mech, ncell, rconst_legs, fix_legs, nleg, carry_h
       type(c_ptr), value :: hstart
       real(c_double) :: var_in(*), fix(*), rconst(*), var_series(*), t_h(*), flux_series(*)
       real(c_double), intent(in) :: times(*), atol(*), rtol(*), rpar(20)
       integer(c_int32_t), intent(in) :: ipar(20)
       integer(c_int32_t) :: ierr(*), stats(*)
       integer(c_int) :: rc
     end function mistra_chem_rosenbrock_series_flux_ex
     function mistra_chem_rosenbrock_series_flux_cells_ex(mech, ncell, var_in, fix, rconst, rconst_legs, fix_legs, nleg, times, atol, rtol, ntol, rpar, ipar, &
          carry_h, hstart, var_series, ierr, stats, t_h, flux_series) bind(C, name="mistra_chem_rosenbrock_series_flux_cells_ex") result(rc)
       import :: c_int, c_double, c_int32_t, c_ptr
       integer(c_int), value :: mech, ncell, rconst_legs, fix_legs, nleg, ntol, carry_h
       type(c_ptr), value :: hstart
       real(c_double) :: var_in(*), fix(*), rconst(*), var_series(*), t_h(*), flux_series(*)
       real(c_double), intent(in) :: times(*), atol(*), rtol(*), rpar(20)
       integer(c_int32_t), intent(in) :: ipar(20)
       integer(c_int32_t) :: ierr(*), stats(*)
       integer(c_int) :: rc
     end function mistra_chem_rosenbrock_series_flux_cells_ex
     function mistra_chem_ops_ex(mech, ncell, var, fix, rconst, vdot, jvs, nshift, shift, fun_rhs, nrhs, rhs, x, ising) &
          bind(C, name="mistra_chem_ops_ex") result(rc)
       import :: c_int, c_double, c_ptr
       integer(c_int), value :: mech, ncell, nshift, fun_rhs, nrhs
       real(c_double), intent(in) :: var(*), fix(*), rconst(*)
       type(c_ptr), value :: vdot, jvs, shift, rhs, x, ising      ! each c_null_ptr where the call has none (include/mistra_chem.h)
       integer(c_int) :: rc
     end function mistra_chem_ops_ex
     function mistra_chem_rosenbrock_replay_ex(mech, ncell, var_in, fix, rconst, tstart, tend, atol, rtol, rpar, ipar, cap, hrows, hsteps, nsteps, var_out, &
          ierr, stats, t_h, err_log) bind(C, name="mistra_chem_rosenbrock_replay_ex") result(rc)
       import :: c_int, c_double, c_int32_t
       integer(c_int), value :: mech, ncell, cap, hrows
       real(c_double), value :: tstart, tend
       real(c_double) :: var_in(*), fix(*), rconst(*), var_out(*), t_h(*), err_log(*)
       real(c_double), intent(in) :: atol(*), rtol(*), rpar(20), hsteps(*)
       integer(c_int32_t), intent(in) :: ipar(20), nsteps(*)
       integer(c_int32_t) :: ierr(*), stats(*)
       integer(c_int) :: rc
     end function mistra_chem_rosenbrock_replay_ex
     function mistra_chem_rosenbrock_replay_cells_ex(mech, ncell, var_in, fix, rconst, tstart, tend, atol, rtol, ntol, rpar, ipar, cap, hrows, hsteps, nsteps, &
          var_out, ierr, stats, t_h, err_log) bind(C, name="mistra_chem_rosenbrock_replay_cells_ex") result(rc)
       import :: c_int, c_double, c_int32_t
       integer(c_int), value :: mech, ncell, ntol, cap, hrows
       real(c_double), value :: tstart, tend
       real(c_double) :: var_in(*), fix(*), rconst(*), var_out(*), t_h(*), err_log(*)
       real(c_double), intent(in) :: atol(*), rtol(*), rpar(20), hsteps(*)
       integer(c_int32_t), intent(in) :: ipar(20), nsteps(*)
       integer(c_int32_t) :: ierr(*), stats(*)
       integer(c_int) :: rc
     end function mistra_chem_rosenbrock_replay_cells_ex
     function mistra_chem_set_step_reuse(mech, on) bind(C, name="mistra_chem_set_step_reuse") result(rc)
       import :: c_int
       integer(c_int), value :: mech, on
       integer(c_int) :: rc
     end function mistra_chem_set_step_reuse
     function mistra_chem_set_policy(mech, method, atol_factor, atol_floor) bind(C, name="mistra_chem_set_policy") result(rc)
       import :: c_int, c_double
       integer(c_int), value :: mech, method
       real(c_double), value :: atol_factor, atol_floor
       integer(c_int) :: rc
     end function mistra_chem_set_policy
     function mistra_chem_check_policy(mech, method, atol_factor, atol_floor) bind(C, name="mistra_chem_check_policy") result(rc)
       import :: c_int, c_double
       integer(c_int), value :: mech, method
       real(c_double), value :: atol_factor, atol_floor
       integer(c_int) :: rc
     end function mistra_chem_check_policy
     function mistra_chem_clear_policy(mech) bind(C, name="mistra_chem_clear_policy") result(rc)
       import :: c_int
       integer(c_int), value :: mech
       integer(c_int) :: rc
     end function mistra_chem_clear_policy
     function mistra_chem_last_error() bind(C, name="mistra_chem_last_error") result(msg)
       import :: c_ptr
       type(c_ptr) :: msg
     end function mistra_chem_last_error
  end interface
contains
  subroutine mistra_chem_fail(where)
    character(len=*), intent(in) :: where
    character(kind=c_char), pointer :: txt(:)
    integer :: i
    call c_f_pointer(mistra_chem_last_error(), txt, [256])
    write (0, '(3a)', advance='no') ' mistra_chem: ', where, ' failed: '
    do i = 1, 256
       if (txt(i) == c_null_char) exit
       write (0, '(a)', advance='no') txt(i)
    end do
    write (0, *)
    error stop 'mistra_chem: GPU integrator unavailable (there is no CPU fallback)'
  end subroutine mistra_chem_fail

  ! Use the first n GPUs of the node for the batched calls (one block of cells and one host thread per device inside the
  ! library).  Optional: without it the first call initialises device MISTRA_CHEM_DEVICE (default 0).
  subroutine mistra_chem_use_devices(n)
    integer, intent(in) :: n
    if (mistra_chem_init_devices(int(n, c_int), c_null_ptr) /= 0) call mistra_chem_fail('mistra_chem_init_devices')
  end subroutine mistra_chem_use_devices

  ! The reference's messages for an unsuccessful integration, statement by statement: ros_ErrorMsg_x (gas.f:1474-1509)
  ! and the PRINT of INTEGRATE_x (gas.f:764-767).  sfx = 'g' | 'a' | 't'.
  ! mech, cell (0-based index into the last batch): where the rows of the zero pivots are asked for
  subroutine mistra_chem_report(sfx, code, t, h, tin, nsng, mech, cell)
    character(len=1), intent(in) :: sfx
    integer, intent(in) :: code, nsng, mech, cell
    double precision, intent(in) :: t, h, tin
    integer :: i
    integer(c_int32_t) :: rows(8)
    if (nsng > 0) then
       rows = 0
       if (mistra_chem_singular_rows(int(mech, c_int), int(cell, c_int), rows) /= 0) call mistra_chem_fail('mistra_chem_singular_rows')
       do i = 1, nsng       ! (the kernel keeps the first eight rows of a call; a ninth failed decomposition repeats the eighth)
          print *, 'Warning: LU Decomposition returned ising = ', int(rows(min(i, 8)))
       end do
    end if
    if (code >= 0) return
    call mistra_chem_error_lines(sfx, code, t, h)
    print *, 'Rosenbrock: Unsucessful step at T=', tin, ' (IERR=', code, ')'
  end subroutine mistra_chem_report

  ! ros_ErrorMsg_x (gas.f:1474-1509)
  subroutine mistra_chem_error_lines(sfx, code, t, h)
    character(len=1), intent(in) :: sfx
    integer, intent(in) :: code
    double precision, intent(in) :: t, h
    write (6, *) 'Forced exit from Rosenbrock_'//sfx//' due to the following error:'
    if (code == -1) then
       write (6, *) '--> Improper value for maximal no of steps'
    else if (code == -2) then
       write (6, *) '--> Selected Rosenbrock method not implemented'
    else if (code == -3) then
       write (6, *) '--> Hmin/Hmax/Hstart must be positive'
    else if (code == -4) then
       write (6, *) '--> FacMin/FacMax/FacRej must be positive'
    else if (code == -5) then
       write (6, *) '--> Improper tolerance values'
    else if (code == -6) then
       write (6, *) '--> No of steps exceeds maximum bound'
    else if (code == -7) then
       write (6, *) '--> Step size too small: T + 10*H = T', ' or H < Roundoff'
    else if (code == -8) then
       write (6, *) '--> Matrix is repeatedly singular'
    else
       write (6, 102) 'Unknown Error code: ', code
    end if
102 format('       ', A, I4)
    write (6, 103) t, h
103 format('        T=', E15.7, ' and H=', E15.7)
  end subroutine mistra_chem_error_lines

  ! Rosenbrock_x's options for every later call of the mechanism.  A refusal of Rosenbrock_x's own (IERR -1 .. -5) writes the lines it would
  ! write (ros_ErrorMsg_x is called with H = 0 there; T is the call's Tstart, which no call has given yet: 0) and leaves the previous options
  ! in force; anything else the library refuses (a method other than Ros3) stops the program like every other failure.
  subroutine set_options(mech, sfx, nvar, IPAR, RPAR, ATOL, RTOL, IERR)
    integer, intent(in) :: mech, nvar
    character(len=1), intent(in) :: sfx
    integer(c_int32_t), target :: IPAR(20)
    real(c_double), target :: RPAR(20), ATOL(nvar), RTOL(nvar)
    integer :: IERR
    integer(c_int32_t), target :: code
    code = 0
    if (mistra_chem_set_options(int(mech, c_int), c_loc(IPAR), c_loc(RPAR), c_loc(ATOL), c_loc(RTOL), c_loc(code)) /= 0) then
       if (code >= 0) call mistra_chem_fail('MISTRA_SET_OPTIONS_'//sfx)
       call mistra_chem_error_lines(sfx, int(code), 0.d0, 0.d0)
    end if
    IERR = code
  end subroutine set_options

  subroutine clear_options(mech, sfx)
    integer, intent(in) :: mech
    character(len=1), intent(in) :: sfx
    if (mistra_chem_set_options(int(mech, c_int), c_null_ptr, c_null_ptr, c_null_ptr, c_null_ptr, c_null_ptr) /= 0) &
         call mistra_chem_fail('MISTRA_CLEAR_OPTIONS_'//sfx)
  end subroutine clear_options

  subroutine step_reuse(mech, sfx, ON)
    integer, intent(in) :: mech
    character(len=1), intent(in) :: sfx
    logical, intent(in) :: ON
    if (mistra_chem_set_step_reuse(int(mech, c_int), int(merge(1, 0, ON), c_int)) /= 0) call mistra_chem_fail('MISTRA_STEP_REUSE_'//sfx)
  end subroutine step_reuse

  ! The integrator policy of the mechanism.  Values the library refuses (its checks alone, no device) leave the previous policy in force: the text goes to
  ! unit 6 and IERR = 1; anything else that fails stops the program like every other failure.
  subroutine set_policy(mech, sfx, METHOD, ATOL_FACTOR, ATOL_FLOOR, IERR)
    integer, intent(in) :: mech
    character(len=1), intent(in) :: sfx
    integer, intent(in) :: METHOD
    real(c_double), intent(in) :: ATOL_FACTOR, ATOL_FLOOR
    integer :: IERR
    character(kind=c_char), pointer :: txt(:)
    integer :: i
    IERR = 0
    if (mistra_chem_check_policy(int(mech, c_int), int(METHOD, c_int), ATOL_FACTOR, ATOL_FLOOR) /= 0) then
       call c_f_pointer(mistra_chem_last_error(), txt, [512])
       write (6, '(3a)', advance='no') ' MISTRA_SET_POLICY_', sfx, ': '
       do i = 1, 512
          if (txt(i) == c_null_char) exit
          write (6, '(a)', advance='no') txt(i)
       end do
       write (6, *)
       IERR = 1
       return
    end if
    if (mistra_chem_set_policy(int(mech, c_int), int(METHOD, c_int), ATOL_FACTOR, ATOL_FLOOR) /= 0) call mistra_chem_fail('MISTRA_SET_POLICY_'//sfx)
  end subroutine set_policy

  subroutine clear_policy(mech, sfx)
    integer, intent(in) :: mech
    character(len=1), intent(in) :: sfx
    if (mistra_chem_clear_policy(int(mech, c_int)) /= 0) call mistra_chem_fail('MISTRA_CLEAR_POLICY_'//sfx)
  end subroutine clear_policy

  ! the three one-cell routines and the three batched ones differ in sizes only
  subroutine integrate_one(mech, sfx, gdata, TIN, TOUT)
    integer, intent(in) :: mech
    character(len=1), intent(in) :: sfx
    type(c_ptr), intent(in) :: gdata
    real(c_double) :: TIN, TOUT
    integer(c_int32_t) :: ierr, nsng
    real(c_double) :: t_err, h_err, tin_in
    tin_in = TIN
    if (mistra_chem_integrate_common_status(int(mech, c_int), gdata, TIN, TOUT, ierr, t_err, h_err, nsng) /= 0) &
         call mistra_chem_fail('INTEGRATE_'//sfx)
    if (ierr < 0 .or. nsng > 0) call mistra_chem_report(sfx, int(ierr), t_err, h_err, tin_in, int(nsng), mech, 0)
  end subroutine integrate_one

  ! use_env: RCONST holds the rate evaluator's inputs (MISTRA_RATES_ENV_x) instead of rate constants: Update_RCONST_x runs on the GPU too
  ! HSTART: a first step size per cell (rate constants only)
  subroutine integrate_batch(mech, sfx, NCELL, VAR, FIX, RCONST, TIN, TOUT, TEXIT, HEXIT, IERR, ISTAT, use_env, HSTART)
    integer, intent(in) :: mech, NCELL
    character(len=1), intent(in) :: sfx
    logical, intent(in), optional :: use_env
    real(c_double), intent(in), optional :: HSTART(NCELL)
    logical :: env
    real(c_double) :: VAR(*), FIX(*), RCONST(*), TEXIT(NCELL), HEXIT(NCELL)
    real(c_double), intent(in) :: TIN, TOUT
    integer(c_int32_t) :: IERR(NCELL), ISTAT(8, NCELL)
    real(c_double), allocatable :: th(:, :)
    integer :: k
    if (NCELL <= 0) return
    env = .false.
    if (present(use_env)) env = use_env
    allocate (th(3, NCELL))
    if (present(HSTART)) then
       if (mistra_chem_integrate_hstart_ex(int(mech, c_int), int(NCELL, c_int), VAR, FIX, RCONST, c_null_ptr, TIN, TOUT, VAR, IERR, ISTAT, th, HSTART) /= 0) &
            call mistra_chem_fail('INTEGRATE_BATCH_H_'//sfx)
    else if (env) then
       if (mistra_chem_integrate_env_ex(int(mech, c_int), int(NCELL, c_int), VAR, FIX, RCONST, TIN, TOUT, VAR, IERR, ISTAT, th) /= 0) &
            call mistra_chem_fail('INTEGRATE_BATCH_ENV_'//sfx)
    else
       if (mistra_chem_integrate_ex(int(mech, c_int), int(NCELL, c_int), VAR, FIX, RCONST, TIN, TOUT, VAR, IERR, ISTAT, th) /= 0) &
            call mistra_chem_fail('INTEGRATE_BATCH_'//sfx)
    end if
    do k = 1, NCELL            ! the messages in layer order, as the serial loop would have written them
       TEXIT(k) = th(1, k)
       HEXIT(k) = th(2, k)
       if (IERR(k) < 0 .or. ISTAT(8, k) > 0) call mistra_chem_report(sfx, int(IERR(k)), th(1, k), th(3, k), TIN, int(ISTAT(8, k)), mech, k - 1)
    end do
    deallocate (th)
  end subroutine integrate_batch

  ! Rosenbrock_x for NCELL cells with the call's own options; the messages in cell order, as a serial loop over Rosenbrock_x would have written them
  ! (ros_PrepareMatrix_x's warnings, then ros_ErrorMsg_x's lines: a refusal is reported at T = Tstart, H = 0 as Rosenbrock_x does, gas.f:955)
  ! NTOL present: ATOL / RTOL hold a row of NTOL entries per cell (ROSENBROCK_BATCH_CELLS_x)
  ! FLUX present: the flux entries, which return FLUX(NREACT,NCELL) besides (ROSENBROCK_BATCH_FLUX_x, ROSENBROCK_BATCH_FLUX_CELLS_x)
  ! NS, TS, YS, NOUT present: the dense-output entries, which return YS(NVAR,NCELL,NS) and NOUT(NCELL) besides (ROSENBROCK_BATCH_DENSE_x, _DENSE_CELLS_x)
  subroutine rosenbrock_batch(mech, sfx, NCELL, VAR, FIX, RCONST, TSTART, TEND, ATOL, RTOL, RPAR, IPAR, TEXIT, HEXIT, IERR, ISTAT, NTOL, FLUX, NS, TS, YS, NOUT)
    integer, intent(in) :: mech, NCELL
    integer, intent(in), optional :: NTOL, NS
    real(c_double), optional :: FLUX(*), YS(*)
    real(c_double), intent(in), optional :: TS(*)
    integer(c_int32_t), optional :: NOUT(*)
    character(len=1), intent(in) :: sfx
    real(c_double) :: VAR(*), FIX(*), RCONST(*), TEXIT(NCELL), HEXIT(NCELL)
    real(c_double), intent(in) :: TSTART, TEND, ATOL(*), RTOL(*), RPAR(20)
    integer(c_int32_t), intent(in) :: IPAR(20)
    integer(c_int32_t) :: IERR(NCELL), ISTAT(8, NCELL)
    real(c_double), allocatable :: th(:, :)
    integer(c_int32_t) :: rows(8)
    integer :: k, i
    if (NCELL <= 0) return
    allocate (th(3, NCELL))
    if (present(NS) .and. present(NTOL)) then
       if (mistra_chem_rosenbrock_dense_cells_ex(int(mech, c_int), int(NCELL, c_int), VAR, FIX, RCONST, TSTART, TEND, ATOL, RTOL, int(NTOL, c_int), RPAR, IPAR, &
            VAR, IERR, ISTAT, th, int(NS, c_int), TS, YS, NOUT) /= 0) call mistra_chem_fail('ROSENBROCK_BATCH_DENSE_CELLS_'//sfx)
    else if (present(NS)) then
       if (mistra_chem_rosenbrock_dense_ex(int(mech, c_int), int(NCELL, c_int), VAR, FIX, RCONST, TSTART, TEND, ATOL, RTOL, RPAR, IPAR, VAR, IERR, ISTAT, th, &
            int(NS, c_int), TS, YS, NOUT) /= 0) call mistra_chem_fail('ROSENBROCK_BATCH_DENSE_'//sfx)
    else if (present(FLUX) .and. present(NTOL)) then
       if (mistra_chem_rosenbrock_flux_cells_ex(int(mech, c_int), int(NCELL, c_int), VAR, FIX, RCONST, TSTART, TEND, ATOL, RTOL, int(NTOL, c_int), RPAR, IPAR, &
            VAR, IERR, ISTAT, th, FLUX) /= 0) call mistra_chem_fail('ROSENBROCK_BATCH_FLUX_CELLS_'//sfx)
    else if (present(FLUX)) then
       if (mistra_chem_rosenbrock_flux_ex(int(mech, c_int), int(NCELL, c_int), VAR, FIX, RCONST, TSTART, TEND, ATOL, RTOL, RPAR, IPAR, VAR, IERR, ISTAT, th, &
            FLUX) /= 0) call mistra_chem_fail('ROSENBROCK_BATCH_FLUX_'//sfx)
    else if (present(NTOL)) then
       if (mistra_chem_rosenbrock_cells_ex(int(mech, c_int), int(NCELL, c_int), VAR, FIX, RCONST, TSTART, TEND, ATOL, RTOL, int(NTOL, c_int), RPAR, IPAR, &
            VAR, IERR, ISTAT, th) /= 0) call mistra_chem_fail('ROSENBROCK_BATCH_CELLS_'//sfx)
    else
       if (mistra_chem_rosenbrock_ex(int(mech, c_int), int(NCELL, c_int), VAR, FIX, RCONST, TSTART, TEND, ATOL, RTOL, RPAR, IPAR, VAR, IERR, ISTAT, th) /= 0) &
            call mistra_chem_fail('ROSENBROCK_BATCH_'//sfx)
    end if
    do k = 1, NCELL
       TEXIT(k) = th(1, k)
       HEXIT(k) = th(2, k)
       if (ISTAT(8, k) > 0) then
          rows = 0
          if (mistra_chem_singular_rows(int(mech, c_int), int(k - 1, c_int), rows) /= 0) call mistra_chem_fail('mistra_chem_singular_rows')
          do i = 1, ISTAT(8, k)
             print *, 'Warning: LU Decomposition returned ising = ', int(rows(min(i, 8)))
          end do
       end if
       if (IERR(k) < -5) then
          call mistra_chem_error_lines(sfx, int(IERR(k)), th(1, k), th(3, k))
       else if (IERR(k) < 0) then
          call mistra_chem_error_lines(sfx, int(IERR(k)), TSTART, 0.d0)
       end if
    end do
    deallocate (th)
  end subroutine rosenbrock_batch

  ! A series of Rosenbrock_x calls for NCELL cells in one launch; the messages leg by leg and in cell order, as NLEG calls of ROSENBROCK_BATCH_x would have
  ! written ros_ErrorMsg_x's lines (a refusal at T = the leg's start, H = 0).  The rows of zero pivots are not recorded for a series: no warning lines.
  ! NTOL present: ATOL / RTOL hold a row of NTOL entries per cell (ROSENBROCK_BATCH_SERIES_CELLS_x)
  ! NRCLEG and NFIXLEG present: RCONST and FIX hold that many blocks of NCELL cells, 1 or NLEG (ROSENBROCK_BATCH_SERIES_RATES_x / _RATES_CELLS_x)
  ! LINEAR present (with NFIXLEG): RCONST holds the NLEG + 1 node blocks of rate constants linear in time over each leg (ROSENBROCK_BATCH_SERIES_LINRATES_x)
  ! FLUX present (with NRCLEG and NFIXLEG): the reaction flux of every leg, FLUX(NREACT,NCELL,NLEG) (ROSENBROCK_BATCH_SERIES_FLUX_x / _FLUX_CELLS_x)
  subroutine rosenbrock_series(mech, sfx, NCELL, VAR, FIX, RCONST, NLEG, TIMES, ATOL, RTOL, RPAR, IPAR, CARRY, VSER, TEXIT, HEXIT, IERR, ISTAT, NTOL, NRCLEG, NFIXLEG, &
       LINEAR, FLUX)
    integer, intent(in) :: mech, NCELL, NLEG
    integer, intent(in), optional :: NTOL, NRCLEG, NFIXLEG
    logical, intent(in), optional :: LINEAR
    real(c_double), optional :: FLUX(*)
    character(len=1), intent(in) :: sfx
    logical, intent(in) :: CARRY
    real(c_double) :: VAR(*), FIX(*), RCONST(*), VSER(*), TEXIT(NCELL, *), HEXIT(NCELL, *)
    real(c_double), intent(in) :: TIMES(*), ATOL(*), RTOL(*), RPAR(20)
    integer(c_int32_t), intent(in) :: IPAR(20)
    integer(c_int32_t) :: IERR(NCELL, *), ISTAT(8, NCELL, *)
    real(c_double), allocatable :: th(:, :, :)
    integer :: k, l
    if (NCELL <= 0) return
    allocate (th(3, NCELL, max(NLEG, 1)))
    if (present(LINEAR) .and. present(NFIXLEG)) then
       if (mistra_chem_rosenbrock_series_linrates_ex(int(mech, c_int), int(NCELL, c_int), VAR, FIX, RCONST, int(NFIXLEG, c_int), int(NLEG, c_int), TIMES, ATOL, RTOL, &
            RPAR, IPAR, int(merge(1, 0, CARRY), c_int), c_null_ptr, VSER, IERR, ISTAT, th) /= 0) call mistra_chem_fail('ROSENBROCK_BATCH_SERIES_LINRATES_'//sfx)
    else if (present(FLUX) .and. present(NRCLEG) .and. present(NFIXLEG)) then
       if (present(NTOL)) then
          if (mistra_chem_rosenbrock_series_flux_cells_ex(int(mech, c_int), int(NCELL, c_int), VAR, FIX, RCONST, int(NRCLEG, c_int), int(NFIXLEG, c_int), &
               int(NLEG, c_int), TIMES, ATOL, RTOL, int(NTOL, c_int), RPAR, IPAR, int(merge(1, 0, CARRY), c_int), c_null_ptr, VSER, IERR, ISTAT, th, FLUX) /= 0) &
               call mistra_chem_fail('ROSENBROCK_BATCH_SERIES_FLUX_CELLS_'//sfx)
       else
          if (mistra_chem_rosenbrock_series_flux_ex(int(mech, c_int), int(NCELL, c_int), VAR, FIX, RCONST, int(NRCLEG, c_int), int(NFIXLEG, c_int), &
               int(NLEG, c_int), TIMES, ATOL, RTOL, RPAR, IPAR, int(merge(1, 0, CARRY), c_int), c_null_ptr, VSER, IERR, ISTAT, th, FLUX) /= 0) &
               call mistra_chem_fail('ROSENBROCK_BATCH_SERIES_FLUX_'//sfx)
       end if
    else if (present(NRCLEG) .and. present(NFIXLEG)) then
       if (present(NTOL)) then
          if (mistra_chem_rosenbrock_series_rates_cells_ex(int(mech, c_int), int(NCELL, c_int), VAR, FIX, RCONST, int(NRCLEG, c_int), int(NFIXLEG, c_int), &
               int(NLEG, c_int), TIMES, ATOL, RTOL, int(NTOL, c_int), RPAR, IPAR, int(merge(1, 0, CARRY), c_int), c_null_ptr, VSER, IERR, ISTAT, th) /= 0) &
               call mistra_chem_fail('ROSENBROCK_BATCH_SERIES_RATES_CELLS_'//sfx)
       else
          if (mistra_chem_rosenbrock_series_rates_ex(int(mech, c_int), int(NCELL, c_int), VAR, FIX, RCONST, int(NRCLEG, c_int), int(NFIXLEG, c_int), &
               int(NLEG, c_int), TIMES, ATOL, RTOL, RPAR, IPAR, int(merge(1, 0, CARRY), c_int), c_null_ptr, VSER, IERR, ISTAT, th) /= 0) &
               call mistra_chem_fail('ROSENBROCK_BATCH_SERIES_RATES_'//sfx)
       end if
    else if (present(NTOL)) then
       if (mistra_chem_rosenbrock_series_cells_ex(int(mech, c_int), int(NCELL, c_int), VAR, FIX, RCONST, int(NLEG, c_int), TIMES, ATOL, RTOL, int(NTOL, c_int), &
            RPAR, IPAR, int(merge(1, 0, CARRY), c_int), c_null_ptr, VSER, IERR, ISTAT, th) /= 0) call mistra_chem_fail('ROSENBROCK_BATCH_SERIES_CELLS_'//sfx)
    else
       if (mistra_chem_rosenbrock_series_ex(int(mech, c_int), int(NCELL, c_int), VAR, FIX, RCONST, int(NLEG, c_int), TIMES, ATOL, RTOL, RPAR, IPAR, &
            int(merge(1, 0, CARRY), c_int), c_null_ptr, VSER, IERR, ISTAT, th) /= 0) call mistra_chem_fail('ROSENBROCK_BATCH_SERIES_'//sfx)
    end if
    do l = 1, NLEG
       do k = 1, NCELL
          TEXIT(k, l) = th(1, k, l)
          HEXIT(k, l) = th(2, k, l)
          if (IERR(k, l) < -5) then
             call mistra_chem_error_lines(sfx, int(IERR(k, l)), th(1, k, l), th(3, k, l))
          else if (IERR(k, l) < 0) then
             call mistra_chem_error_lines(sfx, int(IERR(k, l)), TIMES(l), 0.d0)
          end if
       end do
    end do
    deallocate (th)
  end subroutine rosenbrock_series

  ! The replay for NCELL cells in one launch; the messages in cell order as ROSENBROCK_BATCH_x writes them.  NTOL present: ATOL / RTOL hold a row of NTOL
  ! entries per cell (ROSENBROCK_BATCH_REPLAY_CELLS_x)
  subroutine rosenbrock_replay(mech, sfx, NCELL, VAR, FIX, RCONST, TSTART, TEND, ATOL, RTOL, RPAR, IPAR, CAP, HROWS, HSTEPS, NSTEPS, TEXIT, HEXIT, IERR, ISTAT, &
       ERRLOG, NTOL)
    integer, intent(in) :: mech, NCELL, CAP, HROWS
    integer, intent(in), optional :: NTOL
    character(len=1), intent(in) :: sfx
    real(c_double) :: VAR(*), FIX(*), RCONST(*), TEXIT(NCELL), HEXIT(NCELL), ERRLOG(*)
    real(c_double), intent(in) :: TSTART, TEND, ATOL(*), RTOL(*), RPAR(20), HSTEPS(*)
    integer(c_int32_t), intent(in) :: IPAR(20), NSTEPS(*)
    integer(c_int32_t) :: IERR(NCELL), ISTAT(8, NCELL)
    real(c_double), allocatable :: th(:, :)
    integer(c_int32_t) :: rows(8)
    integer :: k, i
    if (NCELL <= 0) return
    allocate (th(3, NCELL))
    if (present(NTOL)) then
       if (mistra_chem_rosenbrock_replay_cells_ex(int(mech, c_int), int(NCELL, c_int), VAR, FIX, RCONST, TSTART, TEND, ATOL, RTOL, int(NTOL, c_int), RPAR, IPAR, &
            int(CAP, c_int), int(HROWS, c_int), HSTEPS, NSTEPS, VAR, IERR, ISTAT, th, ERRLOG) /= 0) call mistra_chem_fail('ROSENBROCK_BATCH_REPLAY_CELLS_'//sfx)
    else
       if (mistra_chem_rosenbrock_replay_ex(int(mech, c_int), int(NCELL, c_int), VAR, FIX, RCONST, TSTART, TEND, ATOL, RTOL, RPAR, IPAR, int(CAP, c_int), &
            int(HROWS, c_int), HSTEPS, NSTEPS, VAR, IERR, ISTAT, th, ERRLOG) /= 0) call mistra_chem_fail('ROSENBROCK_BATCH_REPLAY_'//sfx)
    end if
    do k = 1, NCELL
       TEXIT(k) = th(1, k)
       HEXIT(k) = th(2, k)
       if (ISTAT(8, k) > 0) then
          rows = 0
          if (mistra_chem_singular_rows(int(mech, c_int), int(k - 1, c_int), rows) /= 0) call mistra_chem_fail('mistra_chem_singular_rows')
          do i = 1, ISTAT(8, k)
             print *, 'Warning: LU Decomposition returned ising = ', int(rows(min(i, 8)))
          end do
       end if
       if (IERR(k) < -5) then
          call mistra_chem_error_lines(sfx, int(IERR(k)), th(1, k), th(3, k))
       else if (IERR(k) < 0) then
          call mistra_chem_error_lines(sfx, int(IERR(k)), TSTART, 0.d0)
       end if
    end do
    deallocate (th)
  end subroutine rosenbrock_replay

  ! FUN_BATCH_x, JAC_SP_BATCH_x, LINSOLVE_BATCH_x: the one C entry, what the call does not have as c_null_ptr
  subroutine ops_batch(mech, what, NCELL, VAR, FIX, RCONST, VDOT, JVS, NSHIFT, SHIFT, FUNRHS, NRHS, RHS, X, ISING)
    integer, intent(in) :: mech, NCELL
    character(len=*), intent(in) :: what
    real(c_double), intent(in) :: VAR(*), FIX(*), RCONST(*)
    real(c_double), optional, target :: VDOT(*), JVS(*), SHIFT(*), RHS(*), X(*)
    integer(c_int32_t), optional, target :: ISING(*)
    integer, optional, intent(in) :: NSHIFT, NRHS
    logical, optional, intent(in) :: FUNRHS
    type(c_ptr) :: pv, pj, ps, pr, px, pi
    integer(c_int) :: ns, nr, fr
    pv = c_null_ptr; pj = c_null_ptr; ps = c_null_ptr; pr = c_null_ptr; px = c_null_ptr; pi = c_null_ptr
    ns = 1; nr = 0; fr = 0
    if (present(VDOT)) pv = c_loc(VDOT)
    if (present(JVS)) pj = c_loc(JVS)
    if (present(X)) then
       px = c_loc(X); ps = c_loc(SHIFT); pi = c_loc(ISING)
       ns = int(NSHIFT, c_int); nr = int(NRHS, c_int)
       if (FUNRHS) fr = 1
       if (nr > 0) pr = c_loc(RHS)
    end if
    if (mistra_chem_ops_ex(int(mech, c_int), int(NCELL, c_int), VAR, FIX, RCONST, pv, pj, ns, ps, fr, nr, pr, px, pi) /= 0) call mistra_chem_fail(what)
  end subroutine ops_batch
end module mistra_chem_c_api

subroutine INTEGRATE_g(TIN, TOUT)
  use iso_c_binding
  use mistra_chem_c_api
  use mistra_kpp_batch
  implicit none
  real(c_double) :: TIN, TOUT
  integer, parameter :: NVAR = 102, NFIX = 3, NREACT = 331              ! gas_Parameters.h:28-49
  real(c_double), target :: C(NVAR + NFIX)
  real(c_double) :: RCONST(NREACT), TIME, DT, ATOL(NVAR), RTOL(NVAR), STEPMIN, STEPMAX
  common /GDATA_g/ C, RCONST, TIME, DT, ATOL, RTOL, STEPMIN, STEPMAX
  select case (kpp_pass)            ! two-pass layer loop of a batched kpp_driver (mistra_kpp_batch.f90); 0 = serial
  case (1)
     call kpp_batch_store(1, C, RCONST)
  case (2)
     call kpp_batch_fetch(1, C, TIN, STEPMIN)
     RTOL = 1.0d-3                  ! as INTEGRATE_x leaves them (gas.f:745-746)
     ATOL = 1.0d-25
  case default
     call integrate_one(0, 'g', c_loc(C), TIN, TOUT)
  end select
end subroutine INTEGRATE_g

subroutine INTEGRATE_a(TIN, TOUT)
  use iso_c_binding
  use mistra_chem_c_api
  use mistra_kpp_batch
  implicit none
  real(c_double) :: TIN, TOUT
  integer, parameter :: NVAR = 257, NFIX = 5, NREACT = 979              ! aer_Parameters.h:28-49
  real(c_double), target :: C(NVAR + NFIX)
  real(c_double) :: RCONST(NREACT), TIME, DT, ATOL(NVAR), RTOL(NVAR), STEPMIN, STEPMAX
  common /GDATA_a/ C, RCONST, TIME, DT, ATOL, RTOL, STEPMIN, STEPMAX
  select case (kpp_pass)            ! two-pass layer loop of a batched kpp_driver (mistra_kpp_batch.f90); 0 = serial
  case (1)
     call kpp_batch_store(2, C, RCONST)
  case (2)
     call kpp_batch_fetch(2, C, TIN, STEPMIN)
     RTOL = 1.0d-3                  ! as INTEGRATE_x leaves them (gas.f:745-746)
     ATOL = 1.0d-25
  case default
     call integrate_one(1, 'a', c_loc(C), TIN, TOUT)
  end select
end subroutine INTEGRATE_a

subroutine INTEGRATE_t(TIN, TOUT)
  use iso_c_binding
  use mistra_chem_c_api
  use mistra_kpp_batch
  implicit none
  real(c_double) :: TIN, TOUT
  integer, parameter :: NVAR = 417, NFIX = 7, NREACT = 1627             ! tot_Parameters.h:28-49
  real(c_double), target :: C(NVAR + NFIX)
  real(c_double) :: RCONST(NREACT), TIME, DT, ATOL(NVAR), RTOL(NVAR), STEPMIN, STEPMAX
  common /GDATA_t/ C, RCONST, TIME, DT, ATOL, RTOL, STEPMIN, STEPMAX
  select case (kpp_pass)            ! two-pass layer loop of a batched kpp_driver (mistra_kpp_batch.f90); 0 = serial
  case (1)
     call kpp_batch_store(3, C, RCONST)
  case (2)
     call kpp_batch_fetch(3, C, TIN, STEPMIN)
     RTOL = 1.0d-3                  ! as INTEGRATE_x leaves them (gas.f:745-746)
     ATOL = 1.0d-25
  case default
     call integrate_one(2, 't', c_loc(C), TIN, TOUT)
  end select
end subroutine INTEGRATE_t

! ---- batched form: what INTEGRATE_x does to COMMON /GDATA_x/, for NCELL cells at once.
!   VAR(NVAR,NCELL)  in: concentrations, out: after [TIN, TOUT]            (C(1:NVAR) of each cell)
!   FIX(NFIX,NCELL), RCONST(NREACT,NCELL)  in                              (C(NVAR+1:NSPEC), RCONST of each cell)
!   TEXIT(NCELL), HEXIT(NCELL)  out: what the serial call leaves in TIN and STEPMIN (gas.f:769-770)
!   IERR(NCELL)  out: 1 or the negative code of ros_ErrorMsg_x;  ISTAT(8,NCELL) out: COMMON /Statistics/ per cell
subroutine INTEGRATE_BATCH_g(NCELL, VAR, FIX, RCONST, TIN, TOUT, TEXIT, HEXIT, IERR, ISTAT)
  use iso_c_binding
  use mistra_chem_c_api
  implicit none
  integer :: NCELL
  real(c_double) :: VAR(102, *), FIX(3, *), RCONST(331, *), TIN, TOUT, TEXIT(*), HEXIT(*)
  integer(c_int32_t) :: IERR(*), ISTAT(8, *)
  call integrate_batch(0, 'g', NCELL, VAR, FIX, RCONST, TIN, TOUT, TEXIT, HEXIT, IERR, ISTAT)
end subroutine INTEGRATE_BATCH_g

subroutine INTEGRATE_BATCH_a(NCELL, VAR, FIX, RCONST, TIN, TOUT, TEXIT, HEXIT, IERR, ISTAT)
  use iso_c_binding
  use mistra_chem_c_api
  implicit none
  integer :: NCELL
  real(c_double) :: VAR(257, *), FIX(5, *), RCONST(979, *), TIN, TOUT, TEXIT(*), HEXIT(*)
  integer(c_int32_t) :: IERR(*), ISTAT(8, *)
  call integrate_batch(1, 'a', NCELL, VAR, FIX, RCONST, TIN, TOUT, TEXIT, HEXIT, IERR, ISTAT)
end subroutine INTEGRATE_BATCH_a

subroutine INTEGRATE_BATCH_t(NCELL, VAR, FIX, RCONST, TIN, TOUT, TEXIT, HEXIT, IERR, ISTAT)
  use iso_c_binding
  use mistra_chem_c_api
  implicit none
  integer :: NCELL
  real(c_double) :: VAR(417, *), FIX(7, *), RCONST(1627, *), TIN, TOUT, TEXIT(*), HEXIT(*)
  integer(c_int32_t) :: IERR(*), ISTAT(8, *)
  call integrate_batch(2, 't', NCELL, VAR, FIX, RCONST, TIN, TOUT, TEXIT, HEXIT, IERR, ISTAT)
end subroutine INTEGRATE_BATCH_t

! ---- OPT-IN: the same with a first step size per cell, HSTART(NCELL) (<= 0: the reference's 1e-3, or RPAR(3) of the options in force); the caller keeps
!      the steps, HEXIT of one call being HSTART of the next for the same cells
subroutine INTEGRATE_BATCH_H_g(NCELL, VAR, FIX, RCONST, TIN, TOUT, HSTART, TEXIT, HEXIT, IERR, ISTAT)
  use iso_c_binding
  use mistra_chem_c_api
  implicit none
  integer :: NCELL
  real(c_double) :: VAR(102, *), FIX(3, *), RCONST(331, *), TIN, TOUT, HSTART(NCELL), TEXIT(*), HEXIT(*)
  integer(c_int32_t) :: IERR(*), ISTAT(8, *)
  call integrate_batch(0, 'g', NCELL, VAR, FIX, RCONST, TIN, TOUT, TEXIT, HEXIT, IERR, ISTAT, HSTART=HSTART)
end subroutine INTEGRATE_BATCH_H_g

subroutine INTEGRATE_BATCH_H_a(NCELL, VAR, FIX, RCONST, TIN, TOUT, HSTART, TEXIT, HEXIT, IERR, ISTAT)
  use iso_c_binding
  use mistra_chem_c_api
  implicit none
  integer :: NCELL
  real(c_double) :: VAR(257, *), FIX(5, *), RCONST(979, *), TIN, TOUT, HSTART(NCELL), TEXIT(*), HEXIT(*)
  integer(c_int32_t) :: IERR(*), ISTAT(8, *)
  call integrate_batch(1, 'a', NCELL, VAR, FIX, RCONST, TIN, TOUT, TEXIT, HEXIT, IERR, ISTAT, HSTART=HSTART)
end subroutine INTEGRATE_BATCH_H_a

subroutine INTEGRATE_BATCH_H_t(NCELL, VAR, FIX, RCONST, TIN, TOUT, HSTART, TEXIT, HEXIT, IERR, ISTAT)
  use iso_c_binding
  use mistra_chem_c_api
  implicit none
  integer :: NCELL
  real(c_double) :: VAR(417, *), FIX(7, *), RCONST(1627, *), TIN, TOUT, HSTART(NCELL), TEXIT(*), HEXIT(*)
  integer(c_int32_t) :: IERR(*), ISTAT(8, *)
  call integrate_batch(2, 't', NCELL, VAR, FIX, RCONST, TIN, TOUT, TEXIT, HEXIT, IERR, ISTAT, HSTART=HSTART)
end subroutine INTEGRATE_BATCH_H_t

! ---- the same from the rate evaluator's inputs: Update_RCONST_x + INTEGRATE_x of NCELL layers in one call, RCONST never on the host.
!   ENV(nenv_x,NCELL): per layer what MISTRA_RATES_ENV_x (mistra_kpp_rates.f90) packs from the COMMON blocks
subroutine INTEGRATE_BATCH_ENV_g(NCELL, VAR, FIX, ENV, TIN, TOUT, TEXIT, HEXIT, IERR, ISTAT)
  use iso_c_binding
  use mistra_chem_c_api
  implicit none
  integer :: NCELL
  real(c_double) :: VAR(102, *), FIX(3, *), ENV(74, *), TIN, TOUT, TEXIT(*), HEXIT(*)
  integer(c_int32_t) :: IERR(*), ISTAT(8, *)
  call integrate_batch(0, 'g', NCELL, VAR, FIX, ENV, TIN, TOUT, TEXIT, HEXIT, IERR, ISTAT, .true.)
end subroutine INTEGRATE_BATCH_ENV_g

subroutine INTEGRATE_BATCH_ENV_a(NCELL, VAR, FIX, ENV, TIN, TOUT, TEXIT, HEXIT, IERR, ISTAT)
  use iso_c_binding
  use mistra_chem_c_api
  implicit none
  integer :: NCELL
  real(c_double) :: VAR(257, *), FIX(5, *), ENV(330, *), TIN, TOUT, TEXIT(*), HEXIT(*)
  integer(c_int32_t) :: IERR(*), ISTAT(8, *)
  call integrate_batch(1, 'a', NCELL, VAR, FIX, ENV, TIN, TOUT, TEXIT, HEXIT, IERR, ISTAT, .true.)
end subroutine INTEGRATE_BATCH_ENV_a

subroutine INTEGRATE_BATCH_ENV_t(NCELL, VAR, FIX, ENV, TIN, TOUT, TEXIT, HEXIT, IERR, ISTAT)
  use iso_c_binding
  use mistra_chem_c_api
  implicit none
  integer :: NCELL
  real(c_double) :: VAR(417, *), FIX(7, *), ENV(544, *), TIN, TOUT, TEXIT(*), HEXIT(*)
  integer(c_int32_t) :: IERR(*), ISTAT(8, *)
  call integrate_batch(2, 't', NCELL, VAR, FIX, ENV, TIN, TOUT, TEXIT, HEXIT, IERR, ISTAT, .true.)
end subroutine INTEGRATE_BATCH_ENV_t

! ---- Rosenbrock_x's options in place of the seven values INTEGRATE_x hard-codes (gas.f:739-746): call once after the edit, before the first step
subroutine MISTRA_SET_OPTIONS_g(IPAR, RPAR, ATOL, RTOL, IERR)
  use iso_c_binding
  use mistra_chem_c_api
  implicit none
  integer(c_int32_t) :: IPAR(20)
  real(c_double) :: RPAR(20), ATOL(102), RTOL(102)
  integer :: IERR
  call set_options(0, 'g', 102, IPAR, RPAR, ATOL, RTOL, IERR)
end subroutine MISTRA_SET_OPTIONS_g

subroutine MISTRA_SET_OPTIONS_a(IPAR, RPAR, ATOL, RTOL, IERR)
  use iso_c_binding
  use mistra_chem_c_api
  implicit none
  integer(c_int32_t) :: IPAR(20)
  real(c_double) :: RPAR(20), ATOL(257), RTOL(257)
  integer :: IERR
  call set_options(1, 'a', 257, IPAR, RPAR, ATOL, RTOL, IERR)
end subroutine MISTRA_SET_OPTIONS_a

subroutine MISTRA_SET_OPTIONS_t(IPAR, RPAR, ATOL, RTOL, IERR)
  use iso_c_binding
  use mistra_chem_c_api
  implicit none
  integer(c_int32_t) :: IPAR(20)
  real(c_double) :: RPAR(20), ATOL(417), RTOL(417)
  integer :: IERR
  call set_options(2, 't', 417, IPAR, RPAR, ATOL, RTOL, IERR)
end subroutine MISTRA_SET_OPTIONS_t

subroutine MISTRA_CLEAR_OPTIONS_g()
  use mistra_chem_c_api
  implicit none
  call clear_options(0, 'g')
end subroutine MISTRA_CLEAR_OPTIONS_g

subroutine MISTRA_CLEAR_OPTIONS_a()
  use mistra_chem_c_api
  implicit none
  call clear_options(1, 'a')
end subroutine MISTRA_CLEAR_OPTIONS_a

subroutine MISTRA_CLEAR_OPTIONS_t()
  use mistra_chem_c_api
  implicit none
  call clear_options(2, 't')
end subroutine MISTRA_CLEAR_OPTIONS_t

! ---- OPT-IN step reuse of the single-pass batched driver (include/mistra_chem.h: mistra_chem_set_step_reuse): call once after start-up
subroutine MISTRA_STEP_REUSE_g(ON)
  use mistra_chem_c_api
  implicit none
  logical :: ON
  call step_reuse(0, 'g', ON)
end subroutine MISTRA_STEP_REUSE_g

subroutine MISTRA_STEP_REUSE_a(ON)
  use mistra_chem_c_api
  implicit none
  logical :: ON
  call step_reuse(1, 'a', ON)
end subroutine MISTRA_STEP_REUSE_a

subroutine MISTRA_STEP_REUSE_t(ON)
  use mistra_chem_c_api
  implicit none
  logical :: ON
  call step_reuse(2, 't', ON)
end subroutine MISTRA_STEP_REUSE_t

! ---- OPT-IN integrator policy (include/mistra_chem.h: mistra_chem_set_policy): call once after start-up
subroutine MISTRA_SET_POLICY_g(METHOD, ATOL_FACTOR, ATOL_FLOOR, IERR)
  use iso_c_binding
  use mistra_chem_c_api
  implicit none
  integer :: METHOD, IERR
  real(c_double) :: ATOL_FACTOR, ATOL_FLOOR
  call set_policy(0, 'g', METHOD, ATOL_FACTOR, ATOL_FLOOR, IERR)
end subroutine MISTRA_SET_POLICY_g

subroutine MISTRA_CLEAR_POLICY_g()
  use mistra_chem_c_api
  implicit none
  call clear_policy(0, 'g')
end subroutine MISTRA_CLEAR_POLICY_g

subroutine MISTRA_SET_POLICY_a(METHOD, ATOL_FACTOR, ATOL_FLOOR, IERR)
  use iso_c_binding
  use mistra_chem_c_api
  implicit none
  integer :: METHOD, IERR
  real(c_double) :: ATOL_FACTOR, ATOL_FLOOR
  call set_policy(1, 'a', METHOD, ATOL_FACTOR, ATOL_FLOOR, IERR)
end subroutine MISTRA_SET_POLICY_a

subroutine MISTRA_CLEAR_POLICY_a()
  use mistra_chem_c_api
  implicit none
  call clear_policy(1, 'a')
end subroutine MISTRA_CLEAR_POLICY_a

subroutine MISTRA_SET_POLICY_t(METHOD, ATOL_FACTOR, ATOL_FLOOR, IERR)
  use iso_c_binding
  use mistra_chem_c_api
  implicit none
  integer :: METHOD, IERR
  real(c_double) :: ATOL_FACTOR, ATOL_FLOOR
  call set_policy(2, 't', METHOD, ATOL_FACTOR, ATOL_FLOOR, IERR)
end subroutine MISTRA_SET_POLICY_t

subroutine MISTRA_CLEAR_POLICY_t()
  use mistra_chem_c_api
  implicit none
  call clear_policy(2, 't')
end subroutine MISTRA_CLEAR_POLICY_t

! ---- Rosenbrock_x, batched: the reference's argument list (gas.f:777) in front of the per-cell results.  ATOL / RTOL: NVAR entries (IPAR(2) = 0) or one.
subroutine ROSENBROCK_BATCH_g(NCELL, VAR, FIX, RCONST, TSTART, TEND, ATOL, RTOL, RPAR, IPAR, TEXIT, HEXIT, IERR, ISTAT)
  use iso_c_binding
  use mistra_chem_c_api
  implicit none
  integer :: NCELL
  real(c_double) :: VAR(102, *), FIX(3, *), RCONST(331, *), TSTART, TEND, ATOL(*), RTOL(*), RPAR(20), TEXIT(*), HEXIT(*)
  integer(c_int32_t) :: IPAR(20), IERR(*), ISTAT(8, *)
  call rosenbrock_batch(0, 'g', NCELL, VAR, FIX, RCONST, TSTART, TEND, ATOL, RTOL, RPAR, IPAR, TEXIT, HEXIT, IERR, ISTAT)
end subroutine ROSENBROCK_BATCH_g

subroutine ROSENBROCK_BATCH_a(NCELL, VAR, FIX, RCONST, TSTART, TEND, ATOL, RTOL, RPAR, IPAR, TEXIT, HEXIT, IERR, ISTAT)
  use iso_c_binding
  use mistra_chem_c_api
  implicit none
  integer :: NCELL
  real(c_double) :: VAR(257, *), FIX(5, *), RCONST(979, *), TSTART, TEND, ATOL(*), RTOL(*), RPAR(20), TEXIT(*), HEXIT(*)
  integer(c_int32_t) :: IPAR(20), IERR(*), ISTAT(8, *)
  call rosenbrock_batch(1, 'a', NCELL, VAR, FIX, RCONST, TSTART, TEND, ATOL, RTOL, RPAR, IPAR, TEXIT, HEXIT, IERR, ISTAT)
end subroutine ROSENBROCK_BATCH_a

subroutine ROSENBROCK_BATCH_t(NCELL, VAR, FIX, RCONST, TSTART, TEND, ATOL, RTOL, RPAR, IPAR, TEXIT, HEXIT, IERR, ISTAT)
  use iso_c_binding
  use mistra_chem_c_api
  implicit none
  integer :: NCELL
  real(c_double) :: VAR(417, *), FIX(7, *), RCONST(1627, *), TSTART, TEND, ATOL(*), RTOL(*), RPAR(20), TEXIT(*), HEXIT(*)
  integer(c_int32_t) :: IPAR(20), IERR(*), ISTAT(8, *)
  call rosenbrock_batch(2, 't', NCELL, VAR, FIX, RCONST, TSTART, TEND, ATOL, RTOL, RPAR, IPAR, TEXIT, HEXIT, IERR, ISTAT)
end subroutine ROSENBROCK_BATCH_t

! ---- ... with tolerances per cell: ATOL(NTOL,NCELL), RTOL(NTOL,NCELL)
subroutine ROSENBROCK_BATCH_CELLS_g(NCELL, VAR, FIX, RCONST, TSTART, TEND, ATOL, RTOL, NTOL, RPAR, IPAR, TEXIT, HEXIT, IERR, ISTAT)
  use iso_c_binding
  use mistra_chem_c_api
  implicit none
  integer :: NCELL, NTOL
  real(c_double) :: VAR(102, *), FIX(3, *), RCONST(331, *), TSTART, TEND, ATOL(NTOL, *), RTOL(NTOL, *), RPAR(20), TEXIT(*), HEXIT(*)
  integer(c_int32_t) :: IPAR(20), IERR(*), ISTAT(8, *)
  call rosenbrock_batch(0, 'g', NCELL, VAR, FIX, RCONST, TSTART, TEND, ATOL, RTOL, RPAR, IPAR, TEXIT, HEXIT, IERR, ISTAT, NTOL)
end subroutine ROSENBROCK_BATCH_CELLS_g

subroutine ROSENBROCK_BATCH_CELLS_a(NCELL, VAR, FIX, RCONST, TSTART, TEND, ATOL, RTOL, NTOL, RPAR, IPAR, TEXIT, HEXIT, IERR, ISTAT)
  use iso_c_binding
  use mistra_chem_c_api
  implicit none
  integer :: NCELL, NTOL
  real(c_double) :: VAR(257, *), FIX(5, *), RCONST(979, *), TSTART, TEND, ATOL(NTOL, *), RTOL(NTOL, *), RPAR(20), TEXIT(*), HEXIT(*)
  integer(c_int32_t) :: IPAR(20), IERR(*), ISTAT(8, *)
  call rosenbrock_batch(1, 'a', NCELL, VAR, FIX, RCONST, TSTART, TEND, ATOL, RTOL, RPAR, IPAR, TEXIT, HEXIT, IERR, ISTAT, NTOL)
end subroutine ROSENBROCK_BATCH_CELLS_a

subroutine ROSENBROCK_BATCH_CELLS_t(NCELL, VAR, FIX, RCONST, TSTART, TEND, ATOL, RTOL, NTOL, RPAR, IPAR, TEXIT, HEXIT, IERR, ISTAT)
  use iso_c_binding
  use mistra_chem_c_api
  implicit none
  integer :: NCELL, NTOL
  real(c_double) :: VAR(417, *), FIX(7, *), RCONST(1627, *), TSTART, TEND, ATOL(NTOL, *), RTOL(NTOL, *), RPAR(20), TEXIT(*), HEXIT(*)
  integer(c_int32_t) :: IPAR(20), IERR(*), ISTAT(8, *)
  call rosenbrock_batch(2, 't', NCELL, VAR, FIX, RCONST, TSTART, TEND, ATOL, RTOL, RPAR, IPAR, TEXIT, HEXIT, IERR, ISTAT, NTOL)
end subroutine ROSENBROCK_BATCH_CELLS_t

! ---- a series of Rosenbrock_x calls in one launch: the legs' results side by side, VSER(NVAR,NCELL,NLEG), TEXIT / HEXIT / IERR (NCELL,NLEG), ISTAT(8,NCELL,NLEG)
subroutine ROSENBROCK_BATCH_SERIES_g(NCELL, VAR, FIX, RCONST, NLEG, TIMES, ATOL, RTOL, RPAR, IPAR, CARRY, VSER, TEXIT, HEXIT, IERR, ISTAT)
  use iso_c_binding
  use mistra_chem_c_api
  implicit none
  integer :: NCELL, NLEG
  logical :: CARRY
  real(c_double) :: VAR(102, *), FIX(3, *), RCONST(331, *), TIMES(*), ATOL(*), RTOL(*), RPAR(20), VSER(102, NCELL, *), TEXIT(NCELL, *), HEXIT(NCELL, *)
  integer(c_int32_t) :: IPAR(20), IERR(NCELL, *), ISTAT(8, NCELL, *)
  call rosenbrock_series(0, 'g', NCELL, VAR, FIX, RCONST, NLEG, TIMES, ATOL, RTOL, RPAR, IPAR, CARRY, VSER, TEXIT, HEXIT, IERR, ISTAT)
end subroutine ROSENBROCK_BATCH_SERIES_g

subroutine ROSENBROCK_BATCH_SERIES_CELLS_g(NCELL, VAR, FIX, RCONST, NLEG, TIMES, ATOL, RTOL, NTOL, RPAR, IPAR, CARRY, VSER, TEXIT, HEXIT, IERR, ISTAT)
  use iso_c_binding
  use mistra_chem_c_api
  implicit none
  integer :: NCELL, NLEG, NTOL
  logical :: CARRY
  real(c_double) :: VAR(102, *), FIX(3, *), RCONST(331, *), TIMES(*), ATOL(NTOL, *), RTOL(NTOL, *), RPAR(20), VSER(102, NCELL, *), TEXIT(NCELL, *), HEXIT(NCELL, *)
  integer(c_int32_t) :: IPAR(20), IERR(NCELL, *), ISTAT(8, NCELL, *)
  call rosenbrock_series(0, 'g', NCELL, VAR, FIX, RCONST, NLEG, TIMES, ATOL, RTOL, RPAR, IPAR, CARRY, VSER, TEXIT, HEXIT, IERR, ISTAT, NTOL)
end subroutine ROSENBROCK_BATCH_SERIES_CELLS_g

subroutine ROSENBROCK_BATCH_SERIES_a(NCELL, VAR, FIX, RCONST, NLEG, TIMES, ATOL, RTOL, RPAR, IPAR, CARRY, VSER, TEXIT, HEXIT, IERR, ISTAT)
  use iso_c_binding
  use mistra_chem_c_api
  implicit none
  integer :: NCELL, NLEG
  logical :: CARRY
  real(c_double) :: VAR(257, *), FIX(5, *), RCONST(979, *), TIMES(*), ATOL(*), RTOL(*), RPAR(20), VSER(257, NCELL, *), TEXIT(NCELL, *), HEXIT(NCELL, *)
  integer(c_int32_t) :: IPAR(20), IERR(NCELL, *), ISTAT(8, NCELL, *)
  call rosenbrock_series(1, 'a', NCELL, VAR, FIX, RCONST, NLEG, TIMES, ATOL, RTOL, RPAR, IPAR, CARRY, VSER, TEXIT, HEXIT, IERR, ISTAT)
end subroutine ROSENBROCK_BATCH_SERIES_a

subroutine ROSENBROCK_BATCH_SERIES_CELLS_a(NCELL, VAR, FIX, RCONST, NLEG, TIMES, ATOL, RTOL, NTOL, RPAR, IPAR, CARRY, VSER, TEXIT, HEXIT, IERR, ISTAT)
  use iso_c_binding
  use mistra_chem_c_api
  implicit none
  integer :: NCELL, NLEG, NTOL
  logical :: CARRY
  real(c_double) :: VAR(257, *), FIX(5, *), RCONST(979, *), TIMES(*), ATOL(NTOL, *), RTOL(NTOL, *), RPAR(20), VSER(257, NCELL, *), TEXIT(NCELL, *), HEXIT(NCELL, *)
  integer(c_int32_t) :: IPAR(20), IERR(NCELL, *), ISTAT(8, NCELL, *)
  call rosenbrock_series(1, 'a', NCELL, VAR, FIX, RCONST, NLEG, TIMES, ATOL, RTOL, RPAR, IPAR, CARRY, VSER, TEXIT, HEXIT, IERR, ISTAT, NTOL)
end subroutine ROSENBROCK_BATCH_SERIES_CELLS_a

subroutine ROSENBROCK_BATCH_SERIES_t(NCELL, VAR, FIX, RCONST, NLEG, TIMES, ATOL, RTOL, RPAR, IPAR, CARRY, VSER, TEXIT, HEXIT, IERR, ISTAT)
  use iso_c_binding
  use mistra_chem_c_api
  implicit none
  integer :: NCELL, NLEG
  logical :: CARRY
  real(c_double) :: VAR(417, *), FIX(7, *), RCONST(1627, *), TIMES(*), ATOL(*), RTOL(*), RPAR(20), VSER(417, NCELL, *), TEXIT(NCELL, *), HEXIT(NCELL, *)
  integer(c_int32_t) :: IPAR(20), IERR(NCELL, *), ISTAT(8, NCELL, *)
  call rosenbrock_series(2, 't', NCELL, VAR, FIX, RCONST, NLEG, TIMES, ATOL, RTOL, RPAR, IPAR, CARRY, VSER, TEXIT, HEXIT, IERR, ISTAT)
end subroutine ROSENBROCK_BATCH_SERIES_t

subroutine ROSENBROCK_BATCH_SERIES_CELLS_t(NCELL, VAR, FIX, RCONST, NLEG, TIMES, ATOL, RTOL, NTOL, RPAR, IPAR, CARRY, VSER, TEXIT, HEXIT, IERR, ISTAT)
  use iso_c_binding
  use mistra_chem_c_api
  implicit none
  integer :: NCELL, NLEG, NTOL
  logical :: CARRY
  real(c_double) :: VAR(417, *), FIX(7, *), RCONST(1627, *), TIMES(*), ATOL(NTOL, *), RTOL(NTOL, *), RPAR(20), VSER(417, NCELL, *), TEXIT(NCELL, *), HEXIT(NCELL, *)
  integer(c_int32_t) :: IPAR(20), IERR(NCELL, *), ISTAT(8, NCELL, *)
  call rosenbrock_series(2, 't', NCELL, VAR, FIX, RCONST, NLEG, TIMES, ATOL, RTOL, RPAR, IPAR, CARRY, VSER, TEXIT, HEXIT, IERR, ISTAT, NTOL)
end subroutine ROSENBROCK_BATCH_SERIES_CELLS_t

! ---- the series with rate constants linear in time over each leg: RNODES(NREACT,NCELL,NLEG+1) at TIMES(1:NLEG+1), FIX(NFIX,NCELL,NFIXLEG), NFIXLEG 1 or NLEG
subroutine ROSENBROCK_BATCH_SERIES_LINRATES_g(NCELL, VAR, FIX, RNODES, NLEG, NFIXLEG, TIMES, ATOL, RTOL, RPAR, IPAR, CARRY, VSER, TEXIT, HEXIT, IERR, ISTAT)
  use iso_c_binding
  use mistra_chem_c_api
  implicit none
  integer :: NCELL, NLEG, NFIXLEG
  logical :: CARRY
  real(c_double) :: VAR(102, *), FIX(3, NCELL, *), RNODES(331, NCELL, *), TIMES(*), ATOL(*), RTOL(*), RPAR(20), VSER(102, NCELL, *), TEXIT(NCELL, *), HEXIT(NCELL, *)
  integer(c_int32_t) :: IPAR(20), IERR(NCELL, *), ISTAT(8, NCELL, *)
  call rosenbrock_series(0, 'g', NCELL, VAR, FIX, RNODES, NLEG, TIMES, ATOL, RTOL, RPAR, IPAR, CARRY, VSER, TEXIT, HEXIT, IERR, ISTAT, NFIXLEG=NFIXLEG, LINEAR=.true.)
end subroutine ROSENBROCK_BATCH_SERIES_LINRATES_g

subroutine ROSENBROCK_BATCH_SERIES_LINRATES_a(NCELL, VAR, FIX, RNODES, NLEG, NFIXLEG, TIMES, ATOL, RTOL, RPAR, IPAR, CARRY, VSER, TEXIT, HEXIT, IERR, ISTAT)
  use iso_c_binding
  use mistra_chem_c_api
  implicit none
  integer :: NCELL, NLEG, NFIXLEG
  logical :: CARRY
  real(c_double) :: VAR(257, *), FIX(5, NCELL, *), RNODES(979, NCELL, *), TIMES(*), ATOL(*), RTOL(*), RPAR(20), VSER(257, NCELL, *), TEXIT(NCELL, *), HEXIT(NCELL, *)
  integer(c_int32_t) :: IPAR(20), IERR(NCELL, *), ISTAT(8, NCELL, *)
  call rosenbrock_series(1, 'a', NCELL, VAR, FIX, RNODES, NLEG, TIMES, ATOL, RTOL, RPAR, IPAR, CARRY, VSER, TEXIT, HEXIT, IERR, ISTAT, NFIXLEG=NFIXLEG, LINEAR=.true.)
end subroutine ROSENBROCK_BATCH_SERIES_LINRATES_a

subroutine ROSENBROCK_BATCH_SERIES_LINRATES_t(NCELL, VAR, FIX, RNODES, NLEG, NFIXLEG, TIMES, ATOL, RTOL, RPAR, IPAR, CARRY, VSER, TEXIT, HEXIT, IERR, ISTAT)
  use iso_c_binding
  use mistra_chem_c_api
  implicit none
  integer :: NCELL, NLEG, NFIXLEG
  logical :: CARRY
  real(c_double) :: VAR(417, *), FIX(7, NCELL, *), RNODES(1627, NCELL, *), TIMES(*), ATOL(*), RTOL(*), RPAR(20), VSER(417, NCELL, *), TEXIT(NCELL, *), HEXIT(NCELL, *)
  integer(c_int32_t) :: IPAR(20), IERR(NCELL, *), ISTAT(8, NCELL, *)
  call rosenbrock_series(2, 't', NCELL, VAR, FIX, RNODES, NLEG, TIMES, ATOL, RTOL, RPAR, IPAR, CARRY, VSER, TEXIT, HEXIT, IERR, ISTAT, NFIXLEG=NFIXLEG, LINEAR=.true.)
end subroutine ROSENBROCK_BATCH_SERIES_LINRATES_t

! ---- the series with rates with the reaction flux of every leg: FLUX(NREACT,NCELL,NLEG) behind the argument lists of ROSENBROCK_BATCH_SERIES_RATES_x / _RATES_CELLS_x
subroutine ROSENBROCK_BATCH_SERIES_FLUX_g(NCELL, VAR, FIX, RCONST, NLEG, NRCLEG, NFIXLEG, TIMES, ATOL, RTOL, RPAR, IPAR, CARRY, VSER, TEXIT, HEXIT, &
     IERR, ISTAT, FLUX)
  use iso_c_binding
  use mistra_chem_c_api
  implicit none
  integer :: NCELL, NLEG, NRCLEG, NFIXLEG
  logical :: CARRY
  real(c_double) :: VAR(102, *), FIX(3, NCELL, *), RCONST(331, NCELL, *), TIMES(*), ATOL(*), RTOL(*), RPAR(20), VSER(102, NCELL, *), TEXIT(NCELL, *), HEXIT(NCELL, *)
  real(c_double) :: FLUX(331, NCELL, *)
  integer(c_int32_t) :: IPAR(20), IERR(NCELL, *), ISTAT(8, NCELL, *)
  call rosenbrock_series(0, 'g', NCELL, VAR, FIX, RCONST, NLEG, TIMES, ATOL, RTOL, RPAR, IPAR, CARRY, VSER, TEXIT, HEXIT, IERR, ISTAT, &
       NRCLEG=NRCLEG, NFIXLEG=NFIXLEG, FLUX=FLUX)
end subroutine ROSENBROCK_BATCH_SERIES_FLUX_g

subroutine ROSENBROCK_BATCH_SERIES_FLUX_CELLS_g(NCELL, VAR, FIX, RCONST, NLEG, NRCLEG, NFIXLEG, TIMES, ATOL, RTOL, NTOL, RPAR, IPAR, CARRY, VSER, TEXIT, HEXIT, &
     IERR, ISTAT, FLUX)
  use iso_c_binding
  use mistra_chem_c_api
  implicit none
  integer :: NCELL, NLEG, NRCLEG, NFIXLEG, NTOL
  logical :: CARRY
  real(c_double) :: VAR(102, *), FIX(3, NCELL, *), RCONST(331, NCELL, *), TIMES(*), ATOL(NTOL, *), RTOL(NTOL, *), RPAR(20), VSER(102, NCELL, *), TEXIT(NCELL, *), &
       HEXIT(NCELL, *)
  real(c_double) :: FLUX(331, NCELL, *)
  integer(c_int32_t) :: IPAR(20), IERR(NCELL, *), ISTAT(8, NCELL, *)
  call rosenbrock_series(0, 'g', NCELL, VAR, FIX, RCONST, NLEG, TIMES, ATOL, RTOL, RPAR, IPAR, CARRY, VSER, TEXIT, HEXIT, IERR, ISTAT, &
       NTOL=NTOL, NRCLEG=NRCLEG, NFIXLEG=NFIXLEG, FLUX=FLUX)
end subroutine ROSENBROCK_BATCH_SERIES_FLUX_CELLS_g

subroutine ROSENBROCK_BATCH_SERIES_FLUX_a(NCELL, VAR, FIX, RCONST, NLEG, NRCLEG, NFIXLEG, TIMES, ATOL, RTOL, RPAR, IPAR, CARRY, VSER, TEXIT, HEXIT, &
     IERR, ISTAT, FLUX)
  use iso_c_binding
  use mistra_chem_c_api
  implicit none
  integer :: NCELL, NLEG, NRCLEG, NFIXLEG
  logical :: CARRY
  real(c_double) :: VAR(257, *), FIX(5, NCELL, *), RCONST(979, NCELL, *), TIMES(*), ATOL(*), RTOL(*), RPAR(20), VSER(257, NCELL, *), TEXIT(NCELL, *), HEXIT(NCELL, *)
  real(c_double) :: FLUX(979, NCELL, *)
  integer(c_int32_t) :: IPAR(20), IERR(NCELL, *), ISTAT(8, NCELL, *)
  call rosenbrock_series(1, 'a', NCELL, VAR, FIX, RCONST, NLEG, TIMES, ATOL, RTOL, RPAR, IPAR, CARRY, VSER, TEXIT, HEXIT, IERR, ISTAT, &
       NRCLEG=NRCLEG, NFIXLEG=NFIXLEG, FLUX=FLUX)
end subroutine ROSENBROCK_BATCH_SERIES_FLUX_a

subroutine ROSENBROCK_BATCH_SERIES_FLUX_CELLS_a(NCELL, VAR, FIX, RCONST, NLEG, NRCLEG, NFIXLEG, TIMES, ATOL, RTOL, NTOL, RPAR, IPAR, CARRY, VSER, TEXIT, HEXIT, &
     IERR, ISTAT, FLUX)
  use iso_c_binding
  use mistra_chem_c_api
  implicit none
  integer :: NCELL, NLEG, NRCLEG, NFIXLEG, NTOL
  logical :: CARRY
  real(c_double) :: VAR(257, *), FIX(5, NCELL, *), RCONST(979, NCELL, *), TIMES(*), ATOL(NTOL, *), RTOL(NTOL, *), RPAR(20), VSER(257, NCELL, *), TEXIT(NCELL, *), &
       HEXIT(NCELL, *)
  real(c_double) :: FLUX(979, NCELL, *)
  integer(c_int32_t) :: IPAR(20), IERR(NCELL, *), ISTAT(8, NCELL, *)
  call rosenbrock_series(1, 'a', NCELL, VAR, FIX, RCONST, NLEG, TIMES, ATOL, RTOL, RPAR, IPAR, CARRY, VSER, TEXIT, HEXIT, IERR, ISTAT, &
       NTOL=NTOL, NRCLEG=NRCLEG, NFIXLEG=NFIXLEG, FLUX=FLUX)
end subroutine ROSENBROCK_BATCH_SERIES_FLUX_CELLS_a

subroutine ROSENBROCK_BATCH_SERIES_FLUX_t(NCELL, VAR, FIX, RCONST, NLEG, NRCLEG, NFIXLEG, TIMES, ATOL, RTOL, RPAR, IPAR, CARRY, VSER, TEXIT, HEXIT, &
     IERR, ISTAT, FLUX)
  use iso_c_binding
  use mistra_chem_c_api
  implicit none
  integer :: NCELL, NLEG, NRCLEG, NFIXLEG
  logical :: CARRY
  real(c_double) :: VAR(417, *), FIX(7, NCELL, *), RCONST(1627, NCELL, *), TIMES(*), ATOL(*), RTOL(*), RPAR(20), VSER(417, NCELL, *), TEXIT(NCELL, *), HEXIT(NCELL, *)
  real(c_double) :: FLUX(1627, NCELL, *)
  integer(c_int32_t) :: IPAR(20), IERR(NCELL, *), ISTAT(8, NCELL, *)
  call rosenbrock_series(2, 't', NCELL, VAR, FIX, RCONST, NLEG, TIMES, ATOL, RTOL, RPAR, IPAR, CARRY, VSER, TEXIT, HEXIT, IERR, ISTAT, &
       NRCLEG=NRCLEG, NFIXLEG=NFIXLEG, FLUX=FLUX)
end subroutine ROSENBROCK_BATCH_SERIES_FLUX_t

subroutine ROSENBROCK_BATCH_SERIES_FLUX_CELLS_t(NCELL, VAR, FIX, RCONST, NLEG, NRCLEG, NFIXLEG, TIMES, ATOL, RTOL, NTOL, RPAR, IPAR, CARRY, VSER, TEXIT, HEXIT, &
     IERR, ISTAT, FLUX)
  use iso_c_binding
  use mistra_chem_c_api
  implicit none
  integer :: NCELL, NLEG, NRCLEG, NFIXLEG, NTOL
  logical :: CARRY
  real(c_double) :: VAR(417, *), FIX(7, NCELL, *), RCONST(1627, NCELL, *), TIMES(*), ATOL(NTOL, *), RTOL(NTOL, *), RPAR(20), VSER(417, NCELL, *), TEXIT(NCELL, *), &
       HEXIT(NCELL, *)
  real(c_double) :: FLUX(1627, NCELL, *)
  integer(c_int32_t) :: IPAR(20), IERR(NCELL, *), ISTAT(8, NCELL, *)
  call rosenbrock_series(2, 't', NCELL, VAR, FIX, RCONST, NLEG, TIMES, ATOL, RTOL, RPAR, IPAR, CARRY, VSER, TEXIT, HEXIT, IERR, ISTAT, &
       NTOL=NTOL, NRCLEG=NRCLEG, NFIXLEG=NFIXLEG, FLUX=FLUX)
end subroutine ROSENBROCK_BATCH_SERIES_FLUX_CELLS_t

! ---- the series with rate constants and FIX of the leg's own: RCONST(NREACT,NCELL,NRCLEG), FIX(NFIX,NCELL,NFIXLEG), each count 1 or NLEG
subroutine ROSENBROCK_BATCH_SERIES_RATES_g(NCELL, VAR, FIX, RCONST, NLEG, NRCLEG, NFIXLEG, TIMES, ATOL, RTOL, RPAR, IPAR, CARRY, VSER, TEXIT, HEXIT, IERR, ISTAT)
  use iso_c_binding
  use mistra_chem_c_api
  implicit none
  integer :: NCELL, NLEG, NRCLEG, NFIXLEG
  logical :: CARRY
  real(c_double) :: VAR(102, *), FIX(3, NCELL, *), RCONST(331, NCELL, *), TIMES(*), ATOL(*), RTOL(*), RPAR(20), VSER(102, NCELL, *), TEXIT(NCELL, *), HEXIT(NCELL, *)
  integer(c_int32_t) :: IPAR(20), IERR(NCELL, *), ISTAT(8, NCELL, *)
  call rosenbrock_series(0, 'g', NCELL, VAR, FIX, RCONST, NLEG, TIMES, ATOL, RTOL, RPAR, IPAR, CARRY, VSER, TEXIT, HEXIT, IERR, ISTAT, NRCLEG=NRCLEG, NFIXLEG=NFIXLEG)
end subroutine ROSENBROCK_BATCH_SERIES_RATES_g

subroutine ROSENBROCK_BATCH_SERIES_RATES_CELLS_g(NCELL, VAR, FIX, RCONST, NLEG, NRCLEG, NFIXLEG, TIMES, ATOL, RTOL, NTOL, RPAR, IPAR, CARRY, VSER, TEXIT, HEXIT, IERR, &
     ISTAT)
  use iso_c_binding
  use mistra_chem_c_api
  implicit none
  integer :: NCELL, NLEG, NRCLEG, NFIXLEG, NTOL
  logical :: CARRY
  real(c_double) :: VAR(102, *), FIX(3, NCELL, *), RCONST(331, NCELL, *), TIMES(*), ATOL(NTOL, *), RTOL(NTOL, *), RPAR(20), VSER(102, NCELL, *), TEXIT(NCELL, *), &
       HEXIT(NCELL, *)
  integer(c_int32_t) :: IPAR(20), IERR(NCELL, *), ISTAT(8, NCELL, *)
  call rosenbrock_series(0, 'g', NCELL, VAR, FIX, RCONST, NLEG, TIMES, ATOL, RTOL, RPAR, IPAR, CARRY, VSER, TEXIT, HEXIT, IERR, ISTAT, NTOL, NRCLEG, NFIXLEG)
end subroutine ROSENBROCK_BATCH_SERIES_RATES_CELLS_g

subroutine ROSENBROCK_BATCH_SERIES_RATES_a(NCELL, VAR, FIX, RCONST, NLEG, NRCLEG, NFIXLEG, TIMES, ATOL, RTOL, RPAR, IPAR, CARRY, VSER, TEXIT, HEXIT, IERR, ISTAT)
  use iso_c_binding
  use mistra_chem_c_api
  implicit none
  integer :: NCELL, NLEG, NRCLEG, NFIXLEG
  logical :: CARRY
  real(c_double) :: VAR(257, *), FIX(5, NCELL, *), RCONST(979, NCELL, *), TIMES(*), ATOL(*), RTOL(*), RPAR(20), VSER(257, NCELL, *), TEXIT(NCELL, *), HEXIT(NCELL, *)
  integer(c_int32_t) :: IPAR(20), IERR(NCELL, *), ISTAT(8, NCELL, *)
  call rosenbrock_series(1, 'a', NCELL, VAR, FIX, RCONST, NLEG, TIMES, ATOL, RTOL, RPAR, IPAR, CARRY, VSER, TEXIT, HEXIT, IERR, ISTAT, NRCLEG=NRCLEG, NFIXLEG=NFIXLEG)
end subroutine ROSENBROCK_BATCH_SERIES_RATES_a

subroutine ROSENBROCK_BATCH_SERIES_RATES_CELLS_a(NCELL, VAR, FIX, RCONST, NLEG, NRCLEG, NFIXLEG, TIMES, ATOL, RTOL, NTOL, RPAR, IPAR, CARRY, VSER, TEXIT, HEXIT, IERR, &
     ISTAT)
  use iso_c_binding
  use mistra_chem_c_api
  implicit none
  integer :: NCELL, NLEG, NRCLEG, NFIXLEG, NTOL
  logical :: CARRY
  real(c_double) :: VAR(257, *), FIX(5, NCELL, *), RCONST(979, NCELL, *), TIMES(*), ATOL(NTOL, *), RTOL(NTOL, *), RPAR(20), VSER(257, NCELL, *), TEXIT(NCELL, *), &
       HEXIT(NCELL, *)
  integer(c_int32_t) :: IPAR(20), IERR(NCELL, *), ISTAT(8, NCELL, *)
  call rosenbrock_series(1, 'a', NCELL, VAR, FIX, RCONST, NLEG, TIMES, ATOL, RTOL, RPAR, IPAR, CARRY, VSER, TEXIT, HEXIT, IERR, ISTAT, NTOL, NRCLEG, NFIXLEG)
end subroutine ROSENBROCK_BATCH_SERIES_RATES_CELLS_a

subroutine ROSENBROCK_BATCH_SERIES_RATES_t(NCELL, VAR, FIX, RCONST, NLEG, NRCLEG, NFIXLEG, TIMES, ATOL, RTOL, RPAR, IPAR, CARRY, VSER, TEXIT, HEXIT, IERR, ISTAT)
  use iso_c_binding
  use mistra_chem_c_api
  implicit none
  integer :: NCELL, NLEG, NRCLEG, NFIXLEG
  logical :: CARRY
  real(c_double) :: VAR(417, *), FIX(7, NCELL, *), RCONST(1627, NCELL, *), TIMES(*), ATOL(*), RTOL(*), RPAR(20), VSER(417, NCELL, *), TEXIT(NCELL, *), HEXIT(NCELL, *)
  integer(c_int32_t) :: IPAR(20), IERR(NCELL, *), ISTAT(8, NCELL, *)
  call rosenbrock_series(2, 't', NCELL, VAR, FIX, RCONST, NLEG, TIMES, ATOL, RTOL, RPAR, IPAR, CARRY, VSER, TEXIT, HEXIT, IERR, ISTAT, NRCLEG=NRCLEG, NFIXLEG=NFIXLEG)
end subroutine ROSENBROCK_BATCH_SERIES_RATES_t

subroutine ROSENBROCK_BATCH_SERIES_RATES_CELLS_t(NCELL, VAR, FIX, RCONST, NLEG, NRCLEG, NFIXLEG, TIMES, ATOL, RTOL, NTOL, RPAR, IPAR, CARRY, VSER, TEXIT, HEXIT, IERR, &
     ISTAT)
  use iso_c_binding
  use mistra_chem_c_api
  implicit none
  integer :: NCELL, NLEG, NRCLEG, NFIXLEG, NTOL
  logical :: CARRY
  real(c_double) :: VAR(417, *), FIX(7, NCELL, *), RCONST(1627, NCELL, *), TIMES(*), ATOL(NTOL, *), RTOL(NTOL, *), RPAR(20), VSER(417, NCELL, *), TEXIT(NCELL, *), &
       HEXIT(NCELL, *)
  integer(c_int32_t) :: IPAR(20), IERR(NCELL, *), ISTAT(8, NCELL, *)
  call rosenbrock_series(2, 't', NCELL, VAR, FIX, RCONST, NLEG, TIMES, ATOL, RTOL, RPAR, IPAR, CARRY, VSER, TEXIT, HEXIT, IERR, ISTAT, NTOL, NRCLEG, NFIXLEG)
end subroutine ROSENBROCK_BATCH_SERIES_RATES_CELLS_t

! ---- the reaction flux: ROSENBROCK_BATCH_x / ROSENBROCK_BATCH_CELLS_x with FLUX(NREACT,NCELL) behind their argument lists
subroutine ROSENBROCK_BATCH_FLUX_g(NCELL, VAR, FIX, RCONST, TSTART, TEND, ATOL, RTOL, RPAR, IPAR, TEXIT, HEXIT, IERR, ISTAT, FLUX)
  use iso_c_binding
  use mistra_chem_c_api
  implicit none
  integer :: NCELL
  real(c_double) :: VAR(102, *), FIX(3, *), RCONST(331, *), TSTART, TEND, ATOL(*), RTOL(*), RPAR(20), TEXIT(*), HEXIT(*), FLUX(331, *)
  integer(c_int32_t) :: IPAR(20), IERR(*), ISTAT(8, *)
  call rosenbrock_batch(0, 'g', NCELL, VAR, FIX, RCONST, TSTART, TEND, ATOL, RTOL, RPAR, IPAR, TEXIT, HEXIT, IERR, ISTAT, FLUX=FLUX)
end subroutine ROSENBROCK_BATCH_FLUX_g

subroutine ROSENBROCK_BATCH_FLUX_CELLS_g(NCELL, VAR, FIX, RCONST, TSTART, TEND, ATOL, RTOL, NTOL, RPAR, IPAR, TEXIT, HEXIT, IERR, ISTAT, FLUX)
  use iso_c_binding
  use mistra_chem_c_api
  implicit none
  integer :: NCELL, NTOL
  real(c_double) :: VAR(102, *), FIX(3, *), RCONST(331, *), TSTART, TEND, ATOL(NTOL, *), RTOL(NTOL, *), RPAR(20), TEXIT(*), HEXIT(*), FLUX(331, *)
  integer(c_int32_t) :: IPAR(20), IERR(*), ISTAT(8, *)
  call rosenbrock_batch(0, 'g', NCELL, VAR, FIX, RCONST, TSTART, TEND, ATOL, RTOL, RPAR, IPAR, TEXIT, HEXIT, IERR, ISTAT, NTOL, FLUX)
end subroutine ROSENBROCK_BATCH_FLUX_CELLS_g

subroutine ROSENBROCK_BATCH_FLUX_a(NCELL, VAR, FIX, RCONST, TSTART, TEND, ATOL, RTOL, RPAR, IPAR, TEXIT, HEXIT, IERR, ISTAT, FLUX)
  use iso_c_binding
  use mistra_chem_c_api
  implicit none
  integer :: NCELL
  real(c_double) :: VAR(257, *), FIX(5, *), RCONST(979, *), TSTART, TEND, ATOL(*), RTOL(*), RPAR(20), TEXIT(*), HEXIT(*), FLUX(979, *)
  integer(c_int32_t) :: IPAR(20), IERR(*), ISTAT(8, *)
  call rosenbrock_batch(1, 'a', NCELL, VAR, FIX, RCONST, TSTART, TEND, ATOL, RTOL, RPAR, IPAR, TEXIT, HEXIT, IERR, ISTAT, FLUX=FLUX)
end subroutine ROSENBROCK_BATCH_FLUX_a

subroutine ROSENBROCK_BATCH_FLUX_CELLS_a(NCELL, VAR, FIX, RCONST, TSTART, TEND, ATOL, RTOL, NTOL, RPAR, IPAR, TEXIT, HEXIT, IERR, ISTAT, FLUX)
  use iso_c_binding
  use mistra_chem_c_api
  implicit none
  integer :: NCELL, NTOL
  real(c_double) :: VAR(257, *), FIX(5, *), RCONST(979, *), TSTART, TEND, ATOL(NTOL, *), RTOL(NTOL, *), RPAR(20), TEXIT(*), HEXIT(*), FLUX(979, *)
  integer(c_int32_t) :: IPAR(20), IERR(*), ISTAT(8, *)
  call rosenbrock_batch(1, 'a', NCELL, VAR, FIX, RCONST, TSTART, TEND, ATOL, RTOL, RPAR, IPAR, TEXIT, HEXIT, IERR, ISTAT, NTOL, FLUX)
end subroutine ROSENBROCK_BATCH_FLUX_CELLS_a

subroutine ROSENBROCK_BATCH_FLUX_t(NCELL, VAR, FIX, RCONST, TSTART, TEND, ATOL, RTOL, RPAR, IPAR, TEXIT, HEXIT, IERR, ISTAT, FLUX)
  use iso_c_binding
  use mistra_chem_c_api
  implicit none
  integer :: NCELL
  real(c_double) :: VAR(417, *), FIX(7, *), RCONST(1627, *), TSTART, TEND, ATOL(*), RTOL(*), RPAR(20), TEXIT(*), HEXIT(*), FLUX(1627, *)
  integer(c_int32_t) :: IPAR(20), IERR(*), ISTAT(8, *)
  call rosenbrock_batch(2, 't', NCELL, VAR, FIX, RCONST, TSTART, TEND, ATOL, RTOL, RPAR, IPAR, TEXIT, HEXIT, IERR, ISTAT, FLUX=FLUX)
end subroutine ROSENBROCK_BATCH_FLUX_t

subroutine ROSENBROCK_BATCH_FLUX_CELLS_t(NCELL, VAR, FIX, RCONST, TSTART, TEND, ATOL, RTOL, NTOL, RPAR, IPAR, TEXIT, HEXIT, IERR, ISTAT, FLUX)
  use iso_c_binding
  use mistra_chem_c_api
  implicit none
  integer :: NCELL, NTOL
  real(c_double) :: VAR(417, *), FIX(7, *), RCONST(1627, *), TSTART, TEND, ATOL(NTOL, *), RTOL(NTOL, *), RPAR(20), TEXIT(*), HEXIT(*), FLUX(1627, *)
  integer(c_int32_t) :: IPAR(20), IERR(*), ISTAT(8, *)
  call rosenbrock_batch(2, 't', NCELL, VAR, FIX, RCONST, TSTART, TEND, ATOL, RTOL, RPAR, IPAR, TEXIT, HEXIT, IERR, ISTAT, NTOL, FLUX)
end subroutine ROSENBROCK_BATCH_FLUX_CELLS_t

! ---- dense output: ROSENBROCK_BATCH_x / ROSENBROCK_BATCH_CELLS_x with NS, TS(NS), YS(NVAR,NCELL,NS), NOUT(NCELL) behind their argument lists
subroutine ROSENBROCK_BATCH_DENSE_g(NCELL, VAR, FIX, RCONST, TSTART, TEND, ATOL, RTOL, RPAR, IPAR, TEXIT, HEXIT, IERR, ISTAT, NS, TS, YS, NOUT)
  use iso_c_binding
  use mistra_chem_c_api
  implicit none
  integer :: NCELL, NS
  real(c_double) :: VAR(102, *), FIX(3, *), RCONST(331, *), TSTART, TEND, ATOL(*), RTOL(*), RPAR(20), TEXIT(*), HEXIT(*), TS(*), YS(102, NCELL, *)
  integer(c_int32_t) :: IPAR(20), IERR(*), ISTAT(8, *), NOUT(*)
  call rosenbrock_batch(0, 'g', NCELL, VAR, FIX, RCONST, TSTART, TEND, ATOL, RTOL, RPAR, IPAR, TEXIT, HEXIT, IERR, ISTAT, NS=NS, TS=TS, YS=YS, NOUT=NOUT)
end subroutine ROSENBROCK_BATCH_DENSE_g

subroutine ROSENBROCK_BATCH_DENSE_CELLS_g(NCELL, VAR, FIX, RCONST, TSTART, TEND, ATOL, RTOL, NTOL, RPAR, IPAR, TEXIT, HEXIT, IERR, ISTAT, NS, TS, YS, NOUT)
  use iso_c_binding
  use mistra_chem_c_api
  implicit none
  integer :: NCELL, NTOL, NS
  real(c_double) :: VAR(102, *), FIX(3, *), RCONST(331, *), TSTART, TEND, ATOL(NTOL, *), RTOL(NTOL, *), RPAR(20), TEXIT(*), HEXIT(*), TS(*), YS(102, NCELL, *)
  integer(c_int32_t) :: IPAR(20), IERR(*), ISTAT(8, *), NOUT(*)
  call rosenbrock_batch(0, 'g', NCELL, VAR, FIX, RCONST, TSTART, TEND, ATOL, RTOL, RPAR, IPAR, TEXIT, HEXIT, IERR, ISTAT, NTOL=NTOL, NS=NS, TS=TS, YS=YS, NOUT=NOUT)
end subroutine ROSENBROCK_BATCH_DENSE_CELLS_g

subroutine ROSENBROCK_BATCH_DENSE_a(NCELL, VAR, FIX, RCONST, TSTART, TEND, ATOL, RTOL, RPAR, IPAR, TEXIT, HEXIT, IERR, ISTAT, NS, TS, YS, NOUT)
  use iso_c_binding
  use mistra_chem_c_api
  implicit none
  integer :: NCELL, NS
  real(c_double) :: VAR(257, *), FIX(5, *), RCONST(979, *), TSTART, TEND, ATOL(*), RTOL(*), RPAR(20), TEXIT(*), HEXIT(*), TS(*), YS(257, NCELL, *)
  integer(c_int32_t) :: IPAR(20), IERR(*), ISTAT(8, *), NOUT(*)
  call rosenbrock_batch(1, 'a', NCELL, VAR, FIX, RCONST, TSTART, TEND, ATOL, RTOL, RPAR, IPAR, TEXIT, HEXIT, IERR, ISTAT, NS=NS, TS=TS, YS=YS, NOUT=NOUT)
end subroutine ROSENBROCK_BATCH_DENSE_a

subroutine ROSENBROCK_BATCH_DENSE_CELLS_a(NCELL, VAR, FIX, RCONST, TSTART, TEND, ATOL, RTOL, NTOL, RPAR, IPAR, TEXIT, HEXIT, IERR, ISTAT, NS, TS, YS, NOUT)
  use iso_c_binding
  use mistra_chem_c_api
  implicit none
  integer :: NCELL, NTOL, NS
  real(c_double) :: VAR(257, *), FIX(5, *), RCONST(979, *), TSTART, TEND, ATOL(NTOL, *), RTOL(NTOL, *), RPAR(20), TEXIT(*), HEXIT(*), TS(*), YS(257, NCELL, *)
  integer(c_int32_t) :: IPAR(20), IERR(*), ISTAT(8, *), NOUT(*)
  call rosenbrock_batch(1, 'a', NCELL, VAR, FIX, RCONST, TSTART, TEND, ATOL, RTOL, RPAR, IPAR, TEXIT, HEXIT, IERR, ISTAT, NTOL=NTOL, NS=NS, TS=TS, YS=YS, NOUT=NOUT)
end subroutine ROSENBROCK_BATCH_DENSE_CELLS_a

subroutine ROSENBROCK_BATCH_DENSE_t(NCELL, VAR, FIX, RCONST, TSTART, TEND, ATOL, RTOL, RPAR, IPAR, TEXIT, HEXIT, IERR, ISTAT, NS, TS, YS, NOUT)
  use iso_c_binding
  use mistra_chem_c_api
  implicit none
  integer :: NCELL, NS
  real(c_double) :: VAR(417, *), FIX(7, *), RCONST(1627, *), TSTART, TEND, ATOL(*), RTOL(*), RPAR(20), TEXIT(*), HEXIT(*), TS(*), YS(417, NCELL, *)
  integer(c_int32_t) :: IPAR(20), IERR(*), ISTAT(8, *), NOUT(*)
  call rosenbrock_batch(2, 't', NCELL, VAR, FIX, RCONST, TSTART, TEND, ATOL, RTOL, RPAR, IPAR, TEXIT, HEXIT, IERR, ISTAT, NS=NS, TS=TS, YS=YS, NOUT=NOUT)
end subroutine ROSENBROCK_BATCH_DENSE_t

subroutine ROSENBROCK_BATCH_DENSE_CELLS_t(NCELL, VAR, FIX, RCONST, TSTART, TEND, ATOL, RTOL, NTOL, RPAR, IPAR, TEXIT, HEXIT, IERR, ISTAT, NS, TS, YS, NOUT)
  use iso_c_binding
  use mistra_chem_c_api
  implicit none
  integer :: NCELL, NTOL, NS
  real(c_double) :: VAR(417, *), FIX(7, *), RCONST(1627, *), TSTART, TEND, ATOL(NTOL, *), RTOL(NTOL, *), RPAR(20), TEXIT(*), HEXIT(*), TS(*), YS(417, NCELL, *)
  integer(c_int32_t) :: IPAR(20), IERR(*), ISTAT(8, *), NOUT(*)
  call rosenbrock_batch(2, 't', NCELL, VAR, FIX, RCONST, TSTART, TEND, ATOL, RTOL, RPAR, IPAR, TEXIT, HEXIT, IERR, ISTAT, NTOL=NTOL, NS=NS, TS=TS, YS=YS, NOUT=NOUT)
end subroutine ROSENBROCK_BATCH_DENSE_CELLS_t

! ---- the operators (mistra_chem_ops_ex; INTEGRATION.md 4p): Fun_x, Jac_SP_x and solves with SHIFT*I - Jac_SP_x at the states given, no integration
subroutine FUN_BATCH_g(NCELL, VAR, FIX, RCONST, VDOT)
  use iso_c_binding
  use mistra_chem_c_api
  implicit none
  integer :: NCELL
  real(c_double) :: VAR(102, *), FIX(3, *), RCONST(331, *), VDOT(102, *)
  call ops_batch(0, 'FUN_BATCH_g', NCELL, VAR, FIX, RCONST, VDOT=VDOT)
end subroutine FUN_BATCH_g

subroutine JAC_SP_BATCH_g(NCELL, VAR, FIX, RCONST, JVS)
  use iso_c_binding
  use mistra_chem_c_api
  implicit none
  integer :: NCELL
  real(c_double) :: VAR(102, *), FIX(3, *), RCONST(331, *), JVS(1110, *)
  call ops_batch(0, 'JAC_SP_BATCH_g', NCELL, VAR, FIX, RCONST, JVS=JVS)
end subroutine JAC_SP_BATCH_g

subroutine LINSOLVE_BATCH_g(NCELL, VAR, FIX, RCONST, NSHIFT, SHIFT, FUNRHS, NRHS, RHS, X, ISING)
  use iso_c_binding
  use mistra_chem_c_api
  implicit none
  integer :: NCELL, NSHIFT, NRHS
  logical :: FUNRHS
  real(c_double) :: VAR(102, *), FIX(3, *), RCONST(331, *), SHIFT(*), RHS(102, NCELL, *), X(102, NCELL, *)
  integer(c_int32_t) :: ISING(*)
  call ops_batch(0, 'LINSOLVE_BATCH_g', NCELL, VAR, FIX, RCONST, NSHIFT=NSHIFT, SHIFT=SHIFT, FUNRHS=FUNRHS, NRHS=NRHS, RHS=RHS, X=X, ISING=ISING)
end subroutine LINSOLVE_BATCH_g

subroutine FUN_BATCH_a(NCELL, VAR, FIX, RCONST, VDOT)
  use iso_c_binding
  use mistra_chem_c_api
  implicit none
  integer :: NCELL
  real(c_double) :: VAR(257, *), FIX(5, *), RCONST(979, *), VDOT(257, *)
  call ops_batch(1, 'FUN_BATCH_a', NCELL, VAR, FIX, RCONST, VDOT=VDOT)
end subroutine FUN_BATCH_a

subroutine JAC_SP_BATCH_a(NCELL, VAR, FIX, RCONST, JVS)
  use iso_c_binding
  use mistra_chem_c_api
  implicit none
  integer :: NCELL
  real(c_double) :: VAR(257, *), FIX(5, *), RCONST(979, *), JVS(6579, *)
  call ops_batch(1, 'JAC_SP_BATCH_a', NCELL, VAR, FIX, RCONST, JVS=JVS)
end subroutine JAC_SP_BATCH_a

subroutine LINSOLVE_BATCH_a(NCELL, VAR, FIX, RCONST, NSHIFT, SHIFT, FUNRHS, NRHS, RHS, X, ISING)
  use iso_c_binding
  use mistra_chem_c_api
  implicit none
  integer :: NCELL, NSHIFT, NRHS
  logical :: FUNRHS
  real(c_double) :: VAR(257, *), FIX(5, *), RCONST(979, *), SHIFT(*), RHS(257, NCELL, *), X(257, NCELL, *)
  integer(c_int32_t) :: ISING(*)
  call ops_batch(1, 'LINSOLVE_BATCH_a', NCELL, VAR, FIX, RCONST, NSHIFT=NSHIFT, SHIFT=SHIFT, FUNRHS=FUNRHS, NRHS=NRHS, RHS=RHS, X=X, ISING=ISING)
end subroutine LINSOLVE_BATCH_a

subroutine FUN_BATCH_t(NCELL, VAR, FIX, RCONST, VDOT)
  use iso_c_binding
  use mistra_chem_c_api
  implicit none
  integer :: NCELL
  real(c_double) :: VAR(417, *), FIX(7, *), RCONST(1627, *), VDOT(417, *)
  call ops_batch(2, 'FUN_BATCH_t', NCELL, VAR, FIX, RCONST, VDOT=VDOT)
end subroutine FUN_BATCH_t

subroutine JAC_SP_BATCH_t(NCELL, VAR, FIX, RCONST, JVS)
  use iso_c_binding
  use mistra_chem_c_api
  implicit none
  integer :: NCELL
  real(c_double) :: VAR(417, *), FIX(7, *), RCONST(1627, *), JVS(13503, *)
  call ops_batch(2, 'JAC_SP_BATCH_t', NCELL, VAR, FIX, RCONST, JVS=JVS)
end subroutine JAC_SP_BATCH_t

subroutine LINSOLVE_BATCH_t(NCELL, VAR, FIX, RCONST, NSHIFT, SHIFT, FUNRHS, NRHS, RHS, X, ISING)
  use iso_c_binding
  use mistra_chem_c_api
  implicit none
  integer :: NCELL, NSHIFT, NRHS
  logical :: FUNRHS
  real(c_double) :: VAR(417, *), FIX(7, *), RCONST(1627, *), SHIFT(*), RHS(417, NCELL, *), X(417, NCELL, *)
  integer(c_int32_t) :: ISING(*)
  call ops_batch(2, 'LINSOLVE_BATCH_t', NCELL, VAR, FIX, RCONST, NSHIFT=NSHIFT, SHIFT=SHIFT, FUNRHS=FUNRHS, NRHS=NRHS, RHS=RHS, X=X, ISING=ISING)
end subroutine LINSOLVE_BATCH_t

! ---- the replay (mistra_chem_rosenbrock_replay_ex; INTEGRATION.md 4r): Ros3 along prescribed step sequences, every step accepted, its Err in ERRLOG
subroutine ROSENBROCK_BATCH_REPLAY_g(NCELL, VAR, FIX, RCONST, TSTART, TEND, ATOL, RTOL, RPAR, IPAR, CAP, HROWS, HSTEPS, NSTEPS, TEXIT, HEXIT, IERR, ISTAT, ERRLOG)
  use iso_c_binding
  use mistra_chem_c_api
  implicit none
  integer :: NCELL, CAP, HROWS
  real(c_double) :: VAR(102, *), FIX(3, *), RCONST(331, *), TSTART, TEND, ATOL(102), RTOL(102), RPAR(20), HSTEPS(CAP, *), TEXIT(*), HEXIT(*), ERRLOG(CAP, *)
  integer(c_int32_t) :: IPAR(20), NSTEPS(*), IERR(*), ISTAT(8, *)
  call rosenbrock_replay(0, 'g', NCELL, VAR, FIX, RCONST, TSTART, TEND, ATOL, RTOL, RPAR, IPAR, CAP, HROWS, HSTEPS, NSTEPS, TEXIT, HEXIT, IERR, ISTAT, ERRLOG)
end subroutine ROSENBROCK_BATCH_REPLAY_g

subroutine ROSENBROCK_BATCH_REPLAY_CELLS_g(NCELL, VAR, FIX, RCONST, TSTART, TEND, ATOL, RTOL, NTOL, RPAR, IPAR, CAP, HROWS, HSTEPS, NSTEPS, TEXIT, HEXIT, IERR, &
     ISTAT, ERRLOG)
  use iso_c_binding
  use mistra_chem_c_api
  implicit none
  integer :: NCELL, NTOL, CAP, HROWS
  real(c_double) :: VAR(102, *), FIX(3, *), RCONST(331, *), TSTART, TEND, ATOL(NTOL, *), RTOL(NTOL, *), RPAR(20), HSTEPS(CAP, *), TEXIT(*), HEXIT(*), ERRLOG(CAP, *)
  integer(c_int32_t) :: IPAR(20), NSTEPS(*), IERR(*), ISTAT(8, *)
  call rosenbrock_replay(0, 'g', NCELL, VAR, FIX, RCONST, TSTART, TEND, ATOL, RTOL, RPAR, IPAR, CAP, HROWS, HSTEPS, NSTEPS, TEXIT, HEXIT, IERR, ISTAT, ERRLOG, &
       NTOL=NTOL)
end subroutine ROSENBROCK_BATCH_REPLAY_CELLS_g

subroutine ROSENBROCK_BATCH_REPLAY_a(NCELL, VAR, FIX, RCONST, TSTART, TEND, ATOL, RTOL, RPAR, IPAR, CAP, HROWS, HSTEPS, NSTEPS, TEXIT, HEXIT, IERR, ISTAT, ERRLOG)
  use iso_c_binding
  use mistra_chem_c_api
  implicit none
  integer :: NCELL, CAP, HROWS
  real(c_double) :: VAR(257, *), FIX(5, *), RCONST(979, *), TSTART, TEND, ATOL(257), RTOL(257), RPAR(20), HSTEPS(CAP, *), TEXIT(*), HEXIT(*), ERRLOG(CAP, *)
  integer(c_int32_t) :: IPAR(20), NSTEPS(*), IERR(*), ISTAT(8, *)
  call rosenbrock_replay(1, 'a', NCELL, VAR, FIX, RCONST, TSTART, TEND, ATOL, RTOL, RPAR, IPAR, CAP, HROWS, HSTEPS, NSTEPS, TEXIT, HEXIT, IERR, ISTAT, ERRLOG)
end subroutine ROSENBROCK_BATCH_REPLAY_a

subroutine ROSENBROCK_BATCH_REPLAY_CELLS_a(NCELL, VAR, FIX, RCONST, TSTART, TEND, ATOL, RTOL, NTOL, RPAR, IPAR, CAP, HROWS, HSTEPS, NSTEPS, TEXIT, HEXIT, IERR, &
     ISTAT, ERRLOG)
  use iso_c_binding
  use mistra_chem_c_api
  implicit none
  integer :: NCELL, NTOL, CAP, HROWS
  real(c_double) :: VAR(257, *), FIX(5, *), RCONST(979, *), TSTART, TEND, ATOL(NTOL, *), RTOL(NTOL, *), RPAR(20), HSTEPS(CAP, *), TEXIT(*), HEXIT(*), ERRLOG(CAP, *)
  integer(c_int32_t) :: IPAR(20), NSTEPS(*), IERR(*), ISTAT(8, *)
  call rosenbrock_replay(1, 'a', NCELL, VAR, FIX, RCONST, TSTART, TEND, ATOL, RTOL, RPAR, IPAR, CAP, HROWS, HSTEPS, NSTEPS, TEXIT, HEXIT, IERR, ISTAT, ERRLOG, &
       NTOL=NTOL)
end subroutine ROSENBROCK_BATCH_REPLAY_CELLS_a

subroutine ROSENBROCK_BATCH_REPLAY_t(NCELL, VAR, FIX, RCONST, TSTART, TEND, ATOL, RTOL, RPAR, IPAR, CAP, HROWS, HSTEPS, NSTEPS, TEXIT, HEXIT, IERR, ISTAT, ERRLOG)
  use iso_c_binding
  use mistra_chem_c_api
  implicit none
  integer :: NCELL, CAP, HROWS
  real(c_double) :: VAR(417, *), FIX(7, *), RCONST(1627, *), TSTART, TEND, ATOL(417), RTOL(417), RPAR(20), HSTEPS(CAP, *), TEXIT(*), HEXIT(*), ERRLOG(CAP, *)
  integer(c_int32_t) :: IPAR(20), NSTEPS(*), IERR(*), ISTAT(8, *)
  call rosenbrock_replay(2, 't', NCELL, VAR, FIX, RCONST, TSTART, TEND, ATOL, RTOL, RPAR, IPAR, CAP, HROWS, HSTEPS, NSTEPS, TEXIT, HEXIT, IERR, ISTAT, ERRLOG)
end subroutine ROSENBROCK_BATCH_REPLAY_t

subroutine ROSENBROCK_BATCH_REPLAY_CELLS_t(NCELL, VAR, FIX, RCONST, TSTART, TEND, ATOL, RTOL, NTOL, RPAR, IPAR, CAP, HROWS, HSTEPS, NSTEPS, TEXIT, HEXIT, IERR, &
     ISTAT, ERRLOG)
  use iso_c_binding
  use mistra_chem_c_api
  implicit none
  integer :: NCELL, NTOL, CAP, HROWS
  real(c_double) :: VAR(417, *), FIX(7, *), RCONST(1627, *), TSTART, TEND, ATOL(NTOL, *), RTOL(NTOL, *), RPAR(20), HSTEPS(CAP, *), TEXIT(*), HEXIT(*), ERRLOG(CAP, *)
  integer(c_int32_t) :: IPAR(20), NSTEPS(*), IERR(*), ISTAT(8, *)
  call rosenbrock_replay(2, 't', NCELL, VAR, FIX, RCONST, TSTART, TEND, ATOL, RTOL, RPAR, IPAR, CAP, HROWS, HSTEPS, NSTEPS, TEXIT, HEXIT, IERR, ISTAT, ERRLOG, &
       NTOL=NTOL)
end subroutine ROSENBROCK_BATCH_REPLAY_CELLS_t
