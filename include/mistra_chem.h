/* mistra_chem.h — C ABI of the MI355X-native chemistry integrator (libmistra_chem.so).
 *
 * This is the drop-in boundary for ONE path of the reference model (Mistra-UEA/Mistra): the per-grid-cell KPP
 * Rosenbrock (Ros3) integrator of the gas / aer / tot mechanisms.  Each entry point below names the reference
 * interface it replaces (file:line under the reference's src/).  Plain pointers and sizes only.
 *
 * Semantics shared by the integrate calls (what the reference does for one cell, gas.f:710-773):
 *   input   VAR(NVAR), FIX(NFIX), RCONST(NREACT)   = COMMON /GDATA_x/  C(1:NVAR), C(NVAR+1:NSPEC), RCONST
 *                                                    (gas_Global.h:29-41 | aer_Global.h | tot_Global.h)
 *   options as INTEGRATE_x fixes them unless mistra_chem_set_options has put others in force: Ros3, RTOL 1e-3, ATOL 1e-25 (scalar), Hstart 1e-3 s, Hmin 0,
 *           Hmax |TOUT-TIN|, FacMin 0.2, FacMax 6, FacRej 0.1, FacSafe 0.9, at most 100000 steps (gas.f:739-746, 950-1043)
 *   output  VAR after integrating from TIN to TOUT; ierr = 1 on success or the negative code of
 *           ros_ErrorMsg_x (gas.f:1474-1509: -6 too many steps, -7 step too small, -8 matrix repeatedly singular);
 *           like the reference, VAR then holds whatever state was reached ("print and continue", gas.f:764-767);
 *           stats = COMMON /Statistics/ for that call: Nfun,Njac,Nstp,Nacc,Nrej,Ndec,Nsol,Nsng (gas.f:913-915).
 * Arrays are cell-major: cell c occupies [c*N, (c+1)*N).  Cells are independent (kpp.f90:4310-4470 loops over k).
 * All functions return 0 on success, non-zero on error (mistra_chem_last_error() gives the text).  There is no CPU
 * fallback: without a usable HIP device every compute entry point fails.
 */
#ifndef MISTRA_CHEM_H
#define MISTRA_CHEM_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MISTRA_MECH_GAS 0 /* gas.f  : NVAR 102, NFIX 3, NREACT 331, LU_NONZERO 1110  */
#define MISTRA_MECH_AER 1 /* aer.f  : NVAR 257, NFIX 5, NREACT 979, LU_NONZERO 6579  */
#define MISTRA_MECH_TOT 2 /* tot.f  : NVAR 417, NFIX 7, NREACT 1627, LU_NONZERO 13503 */
/* Two USER MECHANISM SLOTS, compiled from mechanism tables when the library is built (mistra_amd/build.py: MISTRA_USER_MECHS = at most two
 * table paths separated by colons; unset: the demo tables demo_g and demo_a, cut from gas and aer by tools/derive_mech.py; empty: none).  The
 * kernels of a slot are compiled for the SIZES of its table (NVAR 64 .. 512); at run time the slot loads <mech dir>/<name>.mech, <name> the
 * stem of the build-time table: a table with the same sizes and other contents runs (the schedule is compiled at init), one with other
 * sizes fails mistra_chem_init with "does not match the compiled kernel sizes", and so does one of the same sizes for which the schedule
 * compiler needs more partial-sum cells than the build-time table did, plus two ("out of VM temp cells"); a directory without the table
 * leaves the slot out and the rest of the library as it is.
 * A user slot has: mistra_chem_dims, _mech_name, _describe, _integrate, _integrate_ex, _integrate_device, _integrate_device_hstart,
 * _integrate_hstart_ex (rate constants, not env), _singular_rows, _debug_first_step(_ex), _check_options, _set_options, _get_options,
 * _rosenbrock_ex and _rosenbrock_device with Ros3 (ipar[3] = 2), their per-cell tolerance forms _rosenbrock_cells_ex / _cells_device likewise,
 * _cell_atol_device, and the split of a host batch over the device slots.  Every other entry that
 * takes a mechanism id (rates, hand-over, drive, liq_parm, the COMMON-block entry, step reuse, the step-control trace, the four other methods)
 * fails for it with one text that names the slot, before it touches a device.  An id of a slot the library was not built with is an
 * "unknown mechanism id", as 5 and up are. */
#define MISTRA_MECH_USER0 3
#define MISTRA_MECH_USER1 4

/* How many user mechanism slots this library was built with (0 .. 2).  Works before init. */
int mistra_chem_user_mechs(void);

/* "gas" | "aer" | "tot" | the stem of a user slot's table; NULL for an unknown id.  Works before init. */
const char* mistra_chem_mech_name(int mech);

/* Select the HIP device, load the mechanism tables — gas, aer, tot and those of the user slots the library was built with
 * (directory: env MISTRA_MECH_DIR, else ../mech next to the library) — and upload their kernel schedules.  A user slot whose
 * table is not in that directory is left out (its entries then fail with a text that says so); gas, aer and tot must be there.
 * Replaces nothing in the reference (its tables are compiled in: BLOCK DATA JACOBIAN_SPARSE_DATA_x, gas.f:6718 | aer.f:23480 | tot.f:44435); call once before anything else. */
int mistra_chem_init(int device);

/* The same on several GPUs of the node, for a single-process caller such as the reference's Fortran program (the model is
 * serial, kpp.f90:4168): mistra_chem_integrate then cuts the batch into contiguous blocks of cells, one block and one host
 * thread per device — the layer loop of kpp_driver (kpp.f90:4310-4470) carries nothing from one k to the next, so
 * nothing is exchanged.  device_ids = NULL means devices 0 .. n_devices-1; the first one listed is the primary device
 * (one-cell entry points, mistra_chem_describe).  A device may be listed more than once: every listing is a slot of its
 * own (tables, staging buffers, host thread), so the blocks that share a GPU overlap one block's copies with the other's
 * kernel — and the split can be exercised on a one-GPU box.  Replaces a previous init. */
int mistra_chem_init_devices(int n_devices, const int* device_ids);

/* Number of devices the library is initialised on (0 before init). */
int mistra_chem_device_count(void);

/* Release device memory.  Safe to call more than once. */
void mistra_chem_finalize(void);

/* Sizes of a mechanism (gas_Parameters.h:28-49 and siblings).  Any pointer may be NULL.  Works before init. */
int mistra_chem_dims(int mech, int* nvar, int* nfix, int* nreact, int* lu_nonzero);

/* INTEGRATE_x(TIN,TOUT) for ncell cells, host buffers (gas.f:710 | aer.f:1408 | tot.f:2812; called by x_drive at
 * gas.f:173 | aer.f:217 | tot.f:604).  Copies inputs to the device, integrates, copies results back, synchronous.
 * var_out may alias var_in.  ierr (ncell) and stats (ncell*8) may be NULL. */
int mistra_chem_integrate(int mech, int ncell, const double* var_in, const double* fix, const double* rconst,
                          double tin, double tout, double* var_out, int32_t* ierr, int32_t* stats);

/* The same with what INTEGRATE_x leaves behind per cell besides VAR: t_h (ncell*3, may be NULL) receives, per cell, the exit
 * time (-> TIN, gas.f:769), the last accepted step size (-> STEPMIN, gas.f:770) and the step size H when the integrator
 * returned (the H of ros_ErrorMsg_x's message, gas.f:1506).  This is the call a batched kpp_driver makes: one per
 * mechanism and 10-s step for all layers that run it. */
int mistra_chem_integrate_ex(int mech, int ncell, const double* var_in, const double* fix, const double* rconst,
                             double tin, double tout, double* var_out, int32_t* ierr, int32_t* stats, double* t_h);

/* The same from the rate evaluator's inputs instead of the rate constants (mistra_chem_update_rconst below: env [ncell]
 * [mistra_chem_rates_env_size(mech)], what MISTRA_RATES_ENV_x of shim/mistra_kpp_rates.f90 packs per layer): Update_RCONST_x
 * (gas.f:172) and INTEGRATE_x (gas.f:173) of x_drive in one call, RCONST made on the device — 74 / 330 / 544 doubles per layer go
 * up instead of 331 / 979 / 1627. */
int mistra_chem_integrate_env_ex(int mech, int ncell, const double* var_in, const double* fix, const double* env, double tin,
                                 double tout, double* var_out, int32_t* ierr, int32_t* stats, double* t_h);

/* Same call on device-resident buffers (hipMalloc'ed or torch tensors), asynchronous on `hip_stream` (a hipStream_t of
 * that device; NULL = its default stream).  The call runs on the device the buffers live on, which must be one the
 * library was initialised on.  d_ierr (ncell) and d_stats (ncell*8) are required;
 * d_texit_hexit (ncell*2: what INTEGRATE_x leaves in TIN and STEPMIN, gas.f:769-770) may be NULL. */
int mistra_chem_integrate_device(int mech, int ncell, const double* d_var_in, const double* d_fix,
                                 const double* d_rconst, double tin, double tout, double* d_var_out,
                                 int32_t* d_ierr, int32_t* d_stats, double* d_texit_hexit, void* hip_stream);

/* OPT-IN, NOT the reference's behaviour: the same call with a first step size per cell.  INTEGRATE_x starts
 * every call at Hstart = 1e-3 s (gas.f:743) and works its way up to the step the chemistry allows, ~130 steps per call in
 * cloudy layers; a caller that feeds each cell's last step size (d_texit_hexit[2c+1] of the previous chemistry timestep)
 * back as d_hstart[c] skips that ramp.  Results then differ from the reference's at the level of the integrator's own
 * tolerance (study: profiles/r02_hstart_reuse_study.txt).  d_hstart = NULL, or an entry <= 0, gives the reference's 1e-3. */
int mistra_chem_integrate_device_hstart(int mech, int ncell, const double* d_var_in, const double* d_fix,
                                        const double* d_rconst, double tin, double tout, double* d_var_out,
                                        int32_t* d_ierr, int32_t* d_stats, double* d_texit_hexit,
                                        const double* d_hstart, void* hip_stream);

/* OPT-IN likewise, for a caller that is not a torch program: mistra_chem_integrate_ex (rconst given, env = NULL) or mistra_chem_integrate_env_ex (env given,
 * rconst = NULL) — exactly one of the two — with a first step size per cell in HOST memory, hstart [ncell]; hstart = NULL, or an entry <= 0, gives the
 * reference's value (1e-3, or RPAR(3) of the options in force).  The library cannot key a caller-ordered batch by layer, so here the caller keeps the step
 * sizes: t_h[3c+1] of one call is hstart[c] of the next (shim/mistra_kpp_shim.f90: INTEGRATE_BATCH_H_x).  With several device slots every block of cells takes
 * its own part of hstart.  The batched driver keeps them itself: mistra_chem_set_step_reuse below. */
int mistra_chem_integrate_hstart_ex(int mech, int ncell, const double* var_in, const double* fix, const double* rconst, const double* env, double tin,
                                    double tout, double* var_out, int32_t* ierr, int32_t* stats, double* t_h, const double* hstart);

/* Fortran-callable per-cell entry points with the reference's own signature, `SUBROUTINE INTEGRATE_x(TIN,TOUT)`
 * (REAL*8 by reference; data through COMMON /GDATA_x/).  `gdata` is the address of that COMMON block, laid out
 * C(NSPEC), RCONST(NREACT), TIME, DT, ATOL(NVAR), RTOL(NVAR), STEPMIN, STEPMAX (gas_Global.h:29-58).  On return VAR
 * is updated in place, *tin = exit time, STEPMIN = last step size, ATOL/RTOL are set as INTEGRATE_x sets them (or to the options in force), and an
 * unsuccessful integration prints the reference's message.  The ISO_C_BINDING shim in shim/ passes the COMMON block. */
int mistra_chem_integrate_common(int mech, void* gdata, double* tin, double* tout);

/* The same without the messages, for a caller that prints them itself as the reference does (the Fortran shim writes
 * ros_ErrorMsg_x's and INTEGRATE_x's lines to unit 6, gas.f:1474-1509, 764-767): *ierr = IERR of Rosenbrock_x (1 = success),
 * *t_err / *h_err = T and H when the integrator returned (the two numbers of ros_ErrorMsg_x's last line), *nsng = how
 * often the decomposition met a zero pivot (the reference prints one warning per occurrence, gas.f:1456).  Any of the four
 * may be NULL. */
int mistra_chem_integrate_common_status(int mech, void* gdata, double* tin, double* tout, int32_t* ierr, double* t_err,
                                        double* h_err, int32_t* nsng);

/* Rosenbrock_x's options (gas.f:777-1108 | aer.f | tot.f), one layer below INTEGRATE_x, which hard-codes seven of them (gas.f:739-746).  A
 * model whose gas.f / aer.f / tot.f carry other values there calls mistra_chem_set_options once after init; every
 * integrate path of that mechanism then uses them — mistra_chem_integrate(_ex, _env_ex, _device, _device_hstart),
 * mistra_chem_integrate_common(_status), mistra_chem_drive(_begin, _device).  The arguments are Rosenbrock_x's own and are decoded
 * as it decodes them (gas.f:936-1053):
 *   ipar[20] = IPAR   [0] /= 0: autonomous, ros_FunTimeDerivative_x is not evaluated (one Fun count and the HG*dFdT terms less per step,
 *                     gas.f:1221, 1268); [1] = 0: vector tolerances atol[NVAR], rtol[NVAR], anything else: atol[0], rtol[0] alone are read
 *                     (and alone checked); [2] Max_no_steps, 0 = 100000, < 0: IERR -1; [3] the method, 0 = Ros4 (sic), outside 0..5:
 *                     IERR -2; [10..17] are ignored (INTEGRATE_x zeroes them: the statistics start at 0).
 *   rpar[20] = RPAR   [0] Hmin, 0 = 0; [1] Hmax = min(rpar[1], |Tend-Tstart|), 0 = |Tend-Tstart|; [2] Hstart = min(rpar[2],
 *                     |Tend-Tstart|), 0 = max(Hmin, 1e-5) — each < 0: IERR -3; [3..6] FacMin, FacMax, FacRej, FacSafe, 0 = 0.2, 6, 0.1,
 *                     0.9, < 0: IERR -4.
 *   atol, rtol        AbsTol <= 0, RelTol <= 10 eps or RelTol >= 1 in an entry that is read: IERR -5.
 * Only Ros3 (ipar[3] = 2) is built: the four other valid methods are refused by the library (non-zero return), which is not a code
 * of Rosenbrock_x's; Ros2, Ros4, Rodas3 and Rodas4 run through mistra_chem_rosenbrock_ex / _device below, whose options travel with the
 * call.  One vector pair per call, shared by all cells, as in KPP.  A per-cell first step size of
 * mistra_chem_integrate_device_hstart, of mistra_chem_integrate_hstart_ex or remembered under mistra_chem_set_step_reuse still goes before rpar[2]; ipar[2] /= 0 goes before mistra_chem_debug_set_max_steps.
 *
 * mistra_chem_check_options: the decode alone, pure host arithmetic, works before init.  *ierr = 1, or the IERR Rosenbrock_x would return
 * (-1 .. -5; the call itself then still returns 0); a valid method that is not built: non-zero return, *ierr = 0.  For *ierr = 1,
 * resolved_r[7] (may be NULL) = Hmin, Hmax, Hstart, FacMin, FacMax, FacRej, FacSafe as RosenbrockIntegrator_x receives them for a call over
 * interval = |Tend-Tstart|, resolved_i[3] (may be NULL) = Max_no_steps, autonomous (0/1), vector tolerances (0/1). */
int mistra_chem_check_options(int mech, const int32_t* ipar, const double* rpar, const double* atol, const double* rtol, double interval,
                              int32_t* ierr, double* resolved_r, int32_t* resolved_i);

/* Puts the options in force for `mech`, process-wide, on every device the library runs on, until they are replaced or cleared (ipar = NULL:
 * back to INTEGRATE_x's values; the other pointers are then ignored), or mistra_chem_finalize is called; they outlive a re-initialisation.
 * Options Rosenbrock_x would refuse (*ierr = its code, may be NULL) or whose method is not built (*ierr = 0) make the call fail and leave the
 * previous ones in force.  While options are set the integrator runs in a kernel instantiation of its own — also where the values equal
 * INTEGRATE_x's, with bit-identical results — and the diagnostic kernels, which keep INTEGRATE_x's values, fail (mistra_chem_debug_first_step).
 * Fails while a column step of the mechanism is open (mistra_chem_drive_begin), like the other host-buffer calls.  Initialises the library like
 * the Fortran entry points if nothing has. */
int mistra_chem_set_options(int mech, const int32_t* ipar, const double* rpar, const double* atol, const double* rtol, int32_t* ierr);

/* The options in force: *is_set = 0 (INTEGRATE_x's values, nothing else is written) or 1, then ipar[20], rpar[20] as they were given and
 * atol[NVAR], rtol[NVAR] as the integrator uses them (scalar tolerances: entry 1 repeated); each of the four may be NULL.  These are also what
 * mistra_chem_integrate_common(_status) leaves in ATOL / RTOL of COMMON /GDATA_x/ while options are set. */
int mistra_chem_get_options(int mech, int32_t* is_set, int32_t* ipar, double* rpar, double* atol, double* rtol);

/* Rosenbrock_x(Y,Tstart,Tend,AbsTol,RelTol,RPAR,IPAR,IERR) (gas.f:777 | aer.f | tot.f) for ncell cells, with ALL FIVE methods: ipar[3] = 1 Ros2,
 * 2 Ros3, 3 Ros4, 4 Rodas3, 5 Rodas4, 0 = Ros4 as in the reference (gas.f:1057-1077).  The options are the call's own: ipar[20], rpar[20],
 * atol, rtol as described above (one vector pair shared by all cells; atol[0], rtol[0] alone unless ipar[1] = 0), decoded as Rosenbrock_x decodes
 * them.  The options in force (mistra_chem_set_options) are neither read nor changed, step reuse is not involved; ipar[2] /= 0 goes before
 * mistra_chem_debug_set_max_steps.  Ros3 runs the options kernel of mistra_chem_set_options (bit-identical results), each other method a kernel
 * of its own per mechanism, compiled from the tables mistra_chem_method_table returns.
 *
 * A refusal by Rosenbrock_x is a RESULT, not a failure of the call: for IERR -1 .. -5 every cell's ierr is the code, var_out = var_in, stats
 * and t_h are zero, the call returns 0 and no kernel is launched — Rosenbrock_x returns before it touches Y (gas.f:936-1053).
 *
 * mistra_chem_rosenbrock_ex: host buffers, laid out as mistra_chem_integrate_ex's (t_h[ncell][3] = Texit, Hexit, H; ierr, stats, t_h may be
 * NULL); the batch is split over the device slots as there; fails while a column step of the mechanism is open; initialises the library like
 * the Fortran entry points if nothing has.
 * mistra_chem_rosenbrock_device: device buffers on the device they live on, asynchronous on hip_stream; atol, rtol, rpar, ipar are HOST arrays,
 * read before the call returns.  d_texit_hexit[ncell][2] and d_hstart[ncell] may be NULL; d_hstart as in mistra_chem_integrate_device_hstart:
 * an entry > 0 goes before rpar[2].  The call's options block is copied to the device on hip_stream in front of its kernel, so calls queued
 * back to back on one stream each run with their own.  Each mechanism and device slot keeps MISTRA_ROSENBROCK_CALLS_IN_FLIGHT such blocks: a call
 * that finds all of them still in use by unfinished kernels waits (on the host) for the oldest. */
#define MISTRA_ROSENBROCK_CALLS_IN_FLIGHT 8
int mistra_chem_rosenbrock_ex(int mech, int ncell, const double* var_in, const double* fix, const double* rconst,
                              double tstart, double tend, const double* atol, const double* rtol,
                              const double* rpar, const int32_t* ipar,
                              double* var_out, int32_t* ierr, int32_t* stats, double* t_h);
int mistra_chem_rosenbrock_device(int mech, int ncell, const double* d_var_in, const double* d_fix, const double* d_rconst,
                                  double tstart, double tend, const double* atol, const double* rtol,   /* host arrays */
                                  const double* rpar, const int32_t* ipar,                              /* host arrays */
                                  double* d_var_out, int32_t* d_ierr, int32_t* d_stats, double* d_texit_hexit,
                                  const double* d_hstart, void* hip_stream);

/* ---- The step-control trace: the same calls (Ros3 only: ipar[3] = 2, anything else fails with a text) run by a kernel that also records every
 * attempt that reaches ros_ErrorNorm_x (gas.f:1279).  var_out, ierr, stats and t_h are bit-identical to the untraced call's.  Per attempt r of cell c:
 *   trace_d[c][r][0..3] = T at the start of the step | H as attempted, after any halving by ros_PrepareMatrix_x | Err | share
 *   trace_i[c][r][0..1] = species | code
 * species (1-based) is the one with the largest term (Yerr_i / (AbsTol_i + RelTol_i*Ymax_i))**2 of ros_ErrorNorm_x's sum: ties go to the lowest
 * species number, a NaN term never wins, and where no term is positive species = 0 and share = 0.  share = that term / (NVAR * Err**2).
 * code = 1 if the attempt was accepted, else 0, plus 2 x the decompositions that returned a zero pivot within the attempt.
 * ntrace[c] is the TRUE number of attempts (= stats[c][2]); records past cap are not written, and rows past min(ntrace, cap) are not touched.
 * cap = 0 is legal (trace_d and trace_i may then be NULL).  ctrl[c][NVAR], optional (NULL), counts per species the attempts it controlled — all of
 * them, also those past cap.  A refusal by Rosenbrock_x (-1 .. -5) stays a result: ntrace = 0, the logs and ctrl are not written.
 * cap < 0, a NULL ntrace and cap > 0 with a NULL log array fail with a text before a device is touched.
 * _trace_ex: host arrays (the logs go up and come back, so untouched rows keep the caller's contents); _trace_device: device arrays, in stream order. */
int mistra_chem_rosenbrock_trace_ex(int mech, int ncell, const double* var_in, const double* fix, const double* rconst,
                                    double tstart, double tend, const double* atol, const double* rtol,
                                    const double* rpar, const int32_t* ipar,
                                    double* var_out, int32_t* ierr, int32_t* stats, double* t_h,
                                    int cap, double* trace_d, int32_t* trace_i, int32_t* ntrace, int32_t* ctrl);
int mistra_chem_rosenbrock_trace_device(int mech, int ncell, const double* d_var_in, const double* d_fix, const double* d_rconst,
                                        double tstart, double tend, const double* atol, const double* rtol,   /* host arrays */
                                        const double* rpar, const int32_t* ipar,                              /* host arrays */
                                        double* d_var_out, int32_t* d_ierr, int32_t* d_stats, double* d_texit_hexit,
                                        const double* d_hstart, void* hip_stream,
                                        int cap, double* d_trace_d, int32_t* d_trace_i, int32_t* d_ntrace, int32_t* d_ctrl);

/* ---- Tolerances PER CELL: the four calls above with atol[ncell][ntol], rtol[ncell][ntol] in place of the shared pair; everything else is as documented
 * there (the options block of the call — ipar, rpar — travels as it does, MISTRA_ROSENBROCK_CALLS_IN_FLIGHT of them; d_hstart; the trace is Ros3 only;
 * a user slot runs Ros3 and refuses the other methods and the trace with its text).  Cell c integrates with row c.
 *   ntol is 1 or NVAR.  ipar[1] = 0 (vector tolerances) needs ntol = NVAR and reads every entry of a row; ipar[1] /= 0 reads entry 0 of each row, with
 *   either width, and never looks at the others.  Any other ntol, a NULL tolerance array or a negative ncell fail with a text and a non-zero return
 *   before a device is touched: these are the entries' rule, not codes of Rosenbrock_x.
 *   IERR = -5 is a result PER CELL: a cell whose row holds, in an entry that is read, AbsTol <= 0, RelTol <= 10*eps or RelTol >= 1 (gas.f:1045-1053,
 *   compared as written there: a NaN passes) leaves as a refused call leaves — var_out = var_in (aliasing stays legal), ierr = -5, stats, t_h /
 *   d_texit_hexit zero, ntrace = 0, its log rows and ctrl not written — and the other cells run.  The kernel makes that check, since the rows may live
 *   on the device.  -1 .. -4 depend on ipar / rpar alone: whole-call results decided on the host, ahead of -5 as Rosenbrock_x orders its checks, no kernel.
 * _cells_ex / _trace_cells_ex: host arrays; the batch is split over the device slots, each block with its own tolerance rows; they fail while a column
 * step of the mechanism is open.
 * _cells_device / _trace_cells_device: d_atol, d_rtol are DEVICE arrays on the cells' device, read by the kernel IN STREAM ORDER without a copy: they
 * must stay valid and unchanged until the kernel has run (rpar, ipar stay host arrays read before the call returns).  Host memory the device cannot
 * reach is refused with a text. */
int mistra_chem_rosenbrock_cells_ex(int mech, int ncell, const double* var_in, const double* fix, const double* rconst,
                                    double tstart, double tend, const double* atol, const double* rtol, int ntol,
                                    const double* rpar, const int32_t* ipar,
                                    double* var_out, int32_t* ierr, int32_t* stats, double* t_h);
int mistra_chem_rosenbrock_cells_device(int mech, int ncell, const double* d_var_in, const double* d_fix, const double* d_rconst,
                                        double tstart, double tend, const double* d_atol, const double* d_rtol, int ntol,   /* device arrays */
                                        const double* rpar, const int32_t* ipar,                                            /* host arrays */
                                        double* d_var_out, int32_t* d_ierr, int32_t* d_stats, double* d_texit_hexit,
                                        const double* d_hstart, void* hip_stream);
int mistra_chem_rosenbrock_trace_cells_ex(int mech, int ncell, const double* var_in, const double* fix, const double* rconst,
                                          double tstart, double tend, const double* atol, const double* rtol, int ntol,
                                          const double* rpar, const int32_t* ipar,
                                          double* var_out, int32_t* ierr, int32_t* stats, double* t_h,
                                          int cap, double* trace_d, int32_t* trace_i, int32_t* ntrace, int32_t* ctrl);
int mistra_chem_rosenbrock_trace_cells_device(int mech, int ncell, const double* d_var_in, const double* d_fix, const double* d_rconst,
                                              double tstart, double tend, const double* d_atol, const double* d_rtol, int ntol,   /* device arrays */
                                              const double* rpar, const int32_t* ipar,                                            /* host arrays */
                                              double* d_var_out, int32_t* d_ierr, int32_t* d_stats, double* d_texit_hexit,
                                              const double* d_hstart, void* hip_stream,
                                              int cap, double* d_trace_d, int32_t* d_trace_i, int32_t* d_ntrace, int32_t* d_ctrl);

/* THE REACTION FLUX: Rosenbrock_x as the four entries above run it, plus every reaction's rate integrated over the call.  One more
 * output, flux [ncell][NREACT]; with the call's accepted states Y_0 = Y(Tstart), Y_1 .. Y_N, accepted step sizes H_0 .. H_(N-1) and D = Direction (+-1)
 *     flux[r] = sum over n = 0 .. N-1, in time order, of (0.5 * (D*H_n)) * (A_r(Y_n) + A_r(Y_(n+1))),   A_r(Y) = RCT(r) * X * X * X as Fun_x forms it,
 * every multiply and add rounded once, flux[r] starting at +0.0.  A_r(Y_n), n < N, is the product the step's own first Fun_x forms: rejected attempts and
 * stage evaluations contribute nothing.  A_r(Y_N) takes one more evaluation of the A products at the state the call returns (a normal return, and -6 / -7
 * at Texit; after -8 the failing step's own Fun_x has closed the last accepted step); it is not a Fun_x call and is not counted in Nfun.  A backward
 * call carries the sign of D: S * flux (S: the stoichiometric matrix) approximates Y(Texit) - Y(Tstart) in either direction, to the trapezoid's accuracy.
 * var_out, ierr, stats and t_h / d_texit_hexit are bit for bit those of mistra_chem_rosenbrock_ex / _device (the cells forms: _cells_ex / _cells_device)
 * with the same arguments, d_hstart included.  A call that makes no accepted step returns zeros; so does a refusal (-1 .. -5, whole call or, in the cells
 * forms, per cell) in the rows it covers.  The options travel with the call (MISTRA_ROSENBROCK_CALLS_IN_FLIGHT blocks); the options in force, the
 * integrator policy and step reuse are not involved.  The _ex forms split the batch over the device slots and fail while a column step of the mechanism
 * is open.  A null flux fails with a text before a device is touched.  The series form is mistra_chem_rosenbrock_series_flux_ex / _device (below: one row
 * per leg); there is no trace form and no user slot: both user ids fail with the slot's text. */
int mistra_chem_rosenbrock_flux_ex(int mech, int ncell, const double* var_in, const double* fix, const double* rconst, double tstart, double tend,
                                   const double* atol, const double* rtol, const double* rpar, const int32_t* ipar, double* var_out, int32_t* ierr,
                                   int32_t* stats, double* t_h, double* flux /* [ncell][NREACT] */);
int mistra_chem_rosenbrock_flux_device(int mech, int ncell, const double* d_var_in, const double* d_fix, const double* d_rconst, double tstart,
                                       double tend, const double* atol, const double* rtol, const double* rpar, const int32_t* ipar,   /* host arrays */
                                       double* d_var_out, int32_t* d_ierr, int32_t* d_stats, double* d_texit_hexit, const double* d_hstart,
                                       void* hip_stream, double* d_flux);                                                            /* in stream order */
int mistra_chem_rosenbrock_flux_cells_ex(int mech, int ncell, const double* var_in, const double* fix, const double* rconst, double tstart,
                                         double tend, const double* atol, const double* rtol, int ntol,                             /* rows per cell */
                                         const double* rpar, const int32_t* ipar, double* var_out, int32_t* ierr, int32_t* stats, double* t_h,
                                         double* flux);
int mistra_chem_rosenbrock_flux_cells_device(int mech, int ncell, const double* d_var_in, const double* d_fix, const double* d_rconst, double tstart,
                                             double tend, const double* d_atol, const double* d_rtol, int ntol,                     /* device arrays */
                                             const double* rpar, const int32_t* ipar,                                               /* host arrays */
                                             double* d_var_out, int32_t* d_ierr, int32_t* d_stats, double* d_texit_hexit,
                                             const double* d_hstart, void* hip_stream, double* d_flux);

/* A SERIES: several output times in one call and one kernel launch, the cell's state, FIX and the rate constants on chip from the first time to the
 * last.  nleg >= 1 legs over times[0 .. nleg]; leg k is one call of Rosenbrock_x(Y, times[k], times[k+1], AbsTol, RelTol, RPAR,
 * IPAR, IERR) on the state leg k-1 left, and returns what that call returns into block k of the per-leg outputs:
 *     var_series [nleg][ncell][NVAR]   ierr [nleg][ncell]   stats [nleg][ncell][8]   t_h [nleg][ncell][3] (host: Texit, Hexit, H)
 *     d_texit_hexit [nleg][ncell][2] (device).  ierr, stats, t_h (host) and d_texit_hexit (device) may be NULL.
 * The results are bit for bit those of the nleg calls of mistra_chem_rosenbrock_ex / _device (the cells forms: mistra_chem_rosenbrock_cells_ex /
 * _device) they replace.  Every per-call quantity starts afresh in every leg: T, Direction, Hmax and the first step from the leg's interval, the reject
 * flags, the eight counters, IERR, Hexit, the run of singular decompositions, Max_no_steps.  A leg that ends with IERR < 0 (-6, -7, -8) does not end
 * the series: the next leg starts at its own time times[k+1] from the state as left, as the next call would.
 * First step: leg 0 as mistra_chem_rosenbrock_device decides it (hstart[c] > 0 goes before rpar[2]); a later leg takes the options' Hstart and no
 * per-cell value (carry_h = 0: Rosenbrock_x called again), or the previous leg's Hexit of the cell where that is > 0 (carry_h /= 0: what passing the
 * previous call's Hexit as d_hstart does).
 * Refusals of Rosenbrock_x stay results: -1 .. -4, and -5 on a shared pair, fill every leg as nleg refused calls would (var = var_in, the code,
 * zeros) and launch nothing; -5 on per-cell rows is the kernel's, once, and fills every leg of that cell alone.
 * times: a HOST array, read before the call returns (it travels with the call's options block; calls queued back to back on one stream each run with
 * their own, MISTRA_ROSENBROCK_CALLS_IN_FLIGHT of them); finite and strictly monotone, ascending or descending (descending: every leg integrates
 * backward).  A time that is not finite, a repeated time, a change of direction, nleg < 1 or nleg > MISTRA_SERIES_MAX_LEGS, null times or var_series
 * fail with a text before a device is touched.  MISTRA_SERIES_MAX_LEGS = 4096: the times ride behind the options in the call's block, 32 KiB of it
 * per call in flight, pinned on the host and resident on the device per mechanism and device slot.
 * Each cell's inputs are read before any of its outputs is written: var_in may alias the block of one leg of var_series.
 * The entries ignore the options in force, the integrator policy and step reuse, have no trace form, record no zero-pivot rows
 * (mistra_chem_singular_rows keeps describing the last call that is not a series) and do not exist for a user slot (both ids fail with the slot's
 * text).  The _ex forms split the batch over the device slots and fail while a column step of the mechanism is open. */
#define MISTRA_SERIES_MAX_LEGS 4096
int mistra_chem_rosenbrock_series_ex(int mech, int ncell, const double* var_in, const double* fix, const double* rconst,
                                     int nleg, const double* times, const double* atol, const double* rtol,
                                     const double* rpar, const int32_t* ipar, int carry_h, const double* hstart /* [ncell] or NULL */,
                                     double* var_series, int32_t* ierr, int32_t* stats, double* t_h);
int mistra_chem_rosenbrock_series_device(int mech, int ncell, const double* d_var_in, const double* d_fix, const double* d_rconst,
                                         int nleg, const double* times, const double* atol, const double* rtol,
                                         const double* rpar, const int32_t* ipar,                                                 /* host arrays */
                                         double* d_var_series, int32_t* d_ierr, int32_t* d_stats, double* d_texit_hexit,
                                         int carry_h, const double* d_hstart, void* hip_stream);
int mistra_chem_rosenbrock_series_cells_ex(int mech, int ncell, const double* var_in, const double* fix, const double* rconst,
                                           int nleg, const double* times, const double* atol, const double* rtol, int ntol,        /* rows per cell */
                                           const double* rpar, const int32_t* ipar, int carry_h, const double* hstart,
                                           double* var_series, int32_t* ierr, int32_t* stats, double* t_h);
int mistra_chem_rosenbrock_series_cells_device(int mech, int ncell, const double* d_var_in, const double* d_fix, const double* d_rconst,
                                               int nleg, const double* times, const double* d_atol, const double* d_rtol, int ntol,  /* device arrays */
                                               const double* rpar, const int32_t* ipar,                                            /* host arrays */
                                               double* d_var_series, int32_t* d_ierr, int32_t* d_stats, double* d_texit_hexit,
                                               int carry_h, const double* d_hstart, void* hip_stream);

/* A SERIES WITH RATE CONSTANTS AND FIX OF THE LEG'S OWN: Update_RCONST_x + INTEGRATE_x, nleg times, in one launch.  The series
 * entries above with two counts behind rconst:
 *     rconst [rconst_legs][ncell][NREACT]      fix [fix_legs][ncell][NFIX]      each count 1 (one block shared by all legs) or nleg.
 * Leg k is one call of Rosenbrock_x from times[k] to times[k+1] on the state leg k-1 left, with RCONST = block k of rconst and FIX = block k of fix
 * (block 0 where the count is 1): piecewise constant over the series, the model's operator splitting.  Everything else is the series': the outputs
 * and their layout, the first step and carry_h, the refusals that stay results, the times, what is ignored.  The results are bit for bit those of
 * mistra_chem_rosenbrock_ex / _device (the cells forms: mistra_chem_rosenbrock_cells_ex / _device) called leg by leg with leg k's rows; with both
 * counts 1 the call IS the series entry of the same name without "_rates".
 * A count that is neither 1 nor nleg fails with a text before a device is touched, as do the series' own refusals and a user slot (the slot's text).
 * rconst and fix are read at the head of every leg, not once: they may not alias var_series, and the device forms' arrays must stay untouched until
 * the kernel has finished (stream order).  The _ex forms upload each device slot's block of every leg with one 2-D copy.  The layout of rconst is the
 * one mistra_chem_update_rconst_device writes for nleg*ncell rows, leg-major: its output goes in as it is. */
int mistra_chem_rosenbrock_series_rates_ex(int mech, int ncell, const double* var_in, const double* fix, const double* rconst,
                                           int rconst_legs, int fix_legs,
                                           int nleg, const double* times, const double* atol, const double* rtol,
                                           const double* rpar, const int32_t* ipar, int carry_h, const double* hstart /* [ncell] or NULL */,
                                           double* var_series, int32_t* ierr, int32_t* stats, double* t_h);
int mistra_chem_rosenbrock_series_rates_device(int mech, int ncell, const double* d_var_in, const double* d_fix, const double* d_rconst,
                                               int rconst_legs, int fix_legs,
                                               int nleg, const double* times, const double* atol, const double* rtol,
                                               const double* rpar, const int32_t* ipar,                                           /* host arrays */
                                               double* d_var_series, int32_t* d_ierr, int32_t* d_stats, double* d_texit_hexit,
                                               int carry_h, const double* d_hstart, void* hip_stream);
int mistra_chem_rosenbrock_series_rates_cells_ex(int mech, int ncell, const double* var_in, const double* fix, const double* rconst,
                                                 int rconst_legs, int fix_legs,
                                                 int nleg, const double* times, const double* atol, const double* rtol, int ntol,  /* rows per cell */
                                                 const double* rpar, const int32_t* ipar, int carry_h, const double* hstart,
                                                 double* var_series, int32_t* ierr, int32_t* stats, double* t_h);
int mistra_chem_rosenbrock_series_rates_cells_device(int mech, int ncell, const double* d_var_in, const double* d_fix, const double* d_rconst,
                                                     int rconst_legs, int fix_legs,
                                                     int nleg, const double* times, const double* d_atol, const double* d_rtol, int ntol,  /* device arrays */
                                                     const double* rpar, const int32_t* ipar,                                      /* host arrays */
                                                     double* d_var_series, int32_t* d_ierr, int32_t* d_stats, double* d_texit_hexit,
                                                     int carry_h, const double* d_hstart, void* hip_stream);

/* A SERIES WITH RATE CONSTANTS LINEAR IN TIME OVER EACH LEG: Rosenbrock_x as the non-autonomous integrator it is.  The series with
 * rates above with node blocks in place of rconst and its count:
 *     rconst_nodes [nleg + 1][ncell][NREACT]      block k the rate constants AT times[k]: what mistra_chem_update_rconst_device writes for (nleg + 1)*ncell
 *                                                 env rows, node-major
 *     fix [fix_legs][ncell][NFIX]                 fix_legs 1 or nleg, piecewise constant as above.
 * Inside leg k reaction r of a cell has, with R0 = rconst_nodes[k], R1 = rconst_nodes[k+1], w = 1/(times[k+1] - times[k]) and d = R1[r] - R0[r],
 *     R_r(tau) = R0[r] + ((tau - times[k]) * w) * d      dR_r/dt = d * w      every operation rounded on its own (no fused multiply-add),
 * so equal node blocks give R0 at every tau.  The step is RosenbrockIntegrator_x: Fcn0 and Jac0 read R(T), a stage that evaluates anew reads R(T +
 * ros_Alpha(i)*Direction*H), and with ipar[0] = 0 every stage with ros_Gamma(i) /= 0 adds (Direction*H*ros_Gamma(i))*dFdT, where dFdT = Fun(Y, FIX, dR/dt)
 * is the exact time derivative (Fun is linear in the rate constants) in the place of ros_FunTimeDerivative_x's finite difference: one Fun call, counted in
 * Nfun as KPP counts its own.  With ipar[0] /= 0 there is no dFdT and no such term; the stages still read R(tau).  Everything else is the series': outputs
 * and layout, the first step and carry_h, the refusals that stay results, the failure codes per leg.  With equal node blocks the results are those of the
 * series with rates on the shared block, up to the sign of a zero.
 * fix_legs not in {1, nleg}, a null rconst_nodes, the series' own refusals and a user slot (the slot's text) fail with a text before a device is touched.
 * rconst_nodes is read at every function evaluation: it may not alias var_series, and the device forms' array must stay untouched until the kernel has
 * finished (stream order).  The _ex forms upload each device slot's cells of the nleg + 1 blocks with one 2-D copy. */
int mistra_chem_rosenbrock_series_linrates_ex(int mech, int ncell, const double* var_in, const double* fix, const double* rconst_nodes,
                                              int fix_legs,
                                              int nleg, const double* times, const double* atol, const double* rtol,
                                              const double* rpar, const int32_t* ipar, int carry_h, const double* hstart /* [ncell] or NULL */,
                                              double* var_series, int32_t* ierr, int32_t* stats, double* t_h);
int mistra_chem_rosenbrock_series_linrates_device(int mech, int ncell, const double* d_var_in, const double* d_fix, const double* d_rconst_nodes,
                                                  int fix_legs,
                                                  int nleg, const double* times, const double* atol, const double* rtol,
                                                  const double* rpar, const int32_t* ipar,                                        /* host arrays */
                                                  double* d_var_series, int32_t* d_ierr, int32_t* d_stats, double* d_texit_hexit,
                                                  int carry_h, const double* d_hstart, void* hip_stream);
int mistra_chem_rosenbrock_series_linrates_cells_ex(int mech, int ncell, const double* var_in, const double* fix, const double* rconst_nodes,
                                                    int fix_legs,
                                                    int nleg, const double* times, const double* atol, const double* rtol, int ntol,  /* rows per cell */
                                                    const double* rpar, const int32_t* ipar, int carry_h, const double* hstart,
                                                    double* var_series, int32_t* ierr, int32_t* stats, double* t_h);
int mistra_chem_rosenbrock_series_linrates_cells_device(int mech, int ncell, const double* d_var_in, const double* d_fix, const double* d_rconst_nodes,
                                                        int fix_legs,
                                                        int nleg, const double* times, const double* d_atol, const double* d_rtol, int ntol,  /* device arrays */
                                                        const double* rpar, const int32_t* ipar,                                   /* host arrays */
                                                        double* d_var_series, int32_t* d_ierr, int32_t* d_stats, double* d_texit_hexit,
                                                        int carry_h, const double* d_hstart, void* hip_stream);

/* A SERIES WITH THE REACTION FLUX OF EVERY LEG: a budget time series in one launch.  The series with rates above (rconst_legs and
 * fix_legs each 1 or nleg; with both 1 the plain series) with one more output behind its arguments:
 *     flux_series [nleg][ncell][NREACT]      block k, row c: EXACTLY what mistra_chem_rosenbrock_flux_device returns in flux[c] for the call that leg k is —
 * from times[k] to times[k+1] on the state leg k-1 left, with leg k's rate constants and FIX, the first step the series gives the leg (carry_h / hstart as
 * above), the flux entries' trapezoid on the leg's accepted states.  Nothing is carried from one leg's sum into the next: every leg starts at +0.0 and
 * its first evaluation only records A_r(Y_0).  After IERR = -6 / -7 the leg's sum is closed at Texit with the leg's own rate constants, after -8 it is
 * closed as it stands; the next leg starts afresh (a failed leg does not end the series).  A refusal gives +0.0 rows in every leg it covers: -1 .. -5 on
 * the whole call (nothing is launched; the device forms zero the rows in stream order) and -5 per cell in the cells forms.
 * var_series, ierr, stats and t_h / d_texit_hexit are bit for bit those of mistra_chem_rosenbrock_series_rates_ex / _device (the cells forms likewise)
 * with the same arguments.  flux_series may not alias any other array of the call.
 * A null flux_series fails with its own text before a device is touched, as do the series' own refusals; a user slot fails with the slot's text ("has no
 * reaction-flux entries").  There is no form with rate constants linear in time (mistra_chem_rosenbrock_series_linrates_* has no flux), no trace form
 * and no dense-output form.  The _ex forms stage the rows per device slot and split the batch over the slots as the series does. */
int mistra_chem_rosenbrock_series_flux_ex(int mech, int ncell, const double* var_in, const double* fix, const double* rconst,
                                          int rconst_legs, int fix_legs,
                                          int nleg, const double* times, const double* atol, const double* rtol,
                                          const double* rpar, const int32_t* ipar, int carry_h, const double* hstart /* [ncell] or NULL */,
                                          double* var_series, int32_t* ierr, int32_t* stats, double* t_h,
                                          double* flux_series /* [nleg][ncell][NREACT] */);
int mistra_chem_rosenbrock_series_flux_device(int mech, int ncell, const double* d_var_in, const double* d_fix, const double* d_rconst,
                                              int rconst_legs, int fix_legs,
                                              int nleg, const double* times, const double* atol, const double* rtol,
                                              const double* rpar, const int32_t* ipar,                                            /* host arrays */
                                              double* d_var_series, int32_t* d_ierr, int32_t* d_stats, double* d_texit_hexit,
                                              int carry_h, const double* d_hstart, void* hip_stream, double* d_flux_series);      /* in stream order */
int mistra_chem_rosenbrock_series_flux_cells_ex(int mech, int ncell, const double* var_in, const double* fix, const double* rconst,
                                                int rconst_legs, int fix_legs,
                                                int nleg, const double* times, const double* atol, const double* rtol, int ntol,   /* rows per cell */
                                                const double* rpar, const int32_t* ipar, int carry_h, const double* hstart,
                                                double* var_series, int32_t* ierr, int32_t* stats, double* t_h, double* flux_series);
int mistra_chem_rosenbrock_series_flux_cells_device(int mech, int ncell, const double* d_var_in, const double* d_fix, const double* d_rconst,
                                                    int rconst_legs, int fix_legs,
                                                    int nleg, const double* times, const double* d_atol, const double* d_rtol, int ntol,  /* device arrays */
                                                    const double* rpar, const int32_t* ipar,                                       /* host arrays */
                                                    double* d_var_series, int32_t* d_ierr, int32_t* d_stats, double* d_texit_hexit,
                                                    int carry_h, const double* d_hstart, void* hip_stream, double* d_flux_series);

/* DENSE OUTPUT: the state at ns sample times INSIDE one call of Rosenbrock_x, without changing the call (a series, above, is nleg calls).
 * Everything mistra_chem_rosenbrock_ex / _device (the cells forms: _cells_ex / _cells_device) return with the same arguments, d_hstart included, bit for
 * bit (var_out, ierr, stats, t_h / d_texit_hexit), plus
 *     ysample [ns][ncell][NVAR]  (the series' block layout)      nout [ncell]: the number of samples reached, always a prefix of ts.
 * The call's accepted states are Y_0 = Y(Tstart), Y_1 .. Y_N at the kernel's own times T_0 = Tstart, T_(n+1) = T_n + dh_n, dh_n = D*H_n the signed accepted
 * step, D = Direction (Tend >= Tstart ? 1 : -1), F_n = Fun_x(Y_n) as the step's own first Fun_x forms it.  Samples are taken in order: after step n is
 * accepted, every sample not yet taken with D*(ts[k] - T_(n+1)) <= 0 belongs to step n; on a normal return (IERR = 1) every sample still left belongs to the
 * last accepted step (the loop ends with |Tend - T_N| < Roundoff: Tend may lie an ulp beyond T_N); on IERR = -6 / -7 / -8 the ones left are not reached; a
 * call with no accepted step reaches none.  The value, per species, with th = (ts[k] - T_n) / dh_n, Y0 = Y_n, Y1 = Y_(n+1), F0 = F_n, F1 = F_(n+1), every
 * multiply, add and subtract rounded once, in this order:
 *     d = Y1 - Y0    hf0 = dh*F0    hf1 = dh*F1    om = 1.0 - th
 *     c = ((1.0 - 2.0*th)*d - om*hf0) + th*hf1
 *     u = (om*Y0 + th*Y1) - (th*om)*c
 * — the cubic Hermite interpolant (local error O(H^4): Ros3's order; for the order-4 methods it is the interpolant's order, not the method's).  th = 1
 * gives Y1 exactly: the last step of a completed call is clipped to |Tend - T|, so a sample at Tend equals var_out bit for bit.  F_(n+1) is the next
 * step's first Fun_x; on a normal return, and on -6 / -7 with a step still open, it takes one more Fun_x at the state the call returns, not counted in
 * Nfun (made only where a sample is still to be taken); after -8 the failing step's own Fun_x has closed the last accepted step.
 * Rows >= nout[c] are written +0.0.  Refusals stay results: -1 .. -5 (whole call or, in the cells forms, per cell) give the sibling's result with nout = 0
 * and +0.0 rows; the host-refused ones launch nothing.
 * ts: a HOST array, read before the call returns (it travels behind the call's options block as a series' times do; queued calls each run with their
 * own); 1 <= ns <= MISTRA_DENSE_MAX_TIMES; every ts[k] finite, strictly monotone in the call's direction, D*(ts[k] - Tstart) > 0 and D*(Tend - ts[k]) >= 0.
 * A violation, a null ts, ysample or nout fails with its own text before a device is touched.  The options travel with the call; the options in force, the
 * integrator policy and step reuse are not involved.  There is no series, flux or trace form, no driver hook and no user slot (both ids fail with the
 * slot's text).  The _ex forms split the batch over the device slots and fail while a column step of the mechanism is open. */
#define MISTRA_DENSE_MAX_TIMES MISTRA_SERIES_MAX_LEGS
int mistra_chem_rosenbrock_dense_ex(int mech, int ncell, const double* var_in, const double* fix, const double* rconst, double tstart, double tend,
                                    const double* atol, const double* rtol, const double* rpar, const int32_t* ipar, double* var_out, int32_t* ierr,
                                    int32_t* stats, double* t_h, int ns, const double* ts, double* ysample, int32_t* nout);
int mistra_chem_rosenbrock_dense_device(int mech, int ncell, const double* d_var_in, const double* d_fix, const double* d_rconst, double tstart,
                                        double tend, const double* atol, const double* rtol, const double* rpar, const int32_t* ipar,   /* host arrays */
                                        double* d_var_out, int32_t* d_ierr, int32_t* d_stats, double* d_texit_hexit, const double* d_hstart,
                                        void* hip_stream, int ns, const double* ts /* host */, double* d_ysample, int32_t* d_nout);    /* in stream order */
int mistra_chem_rosenbrock_dense_cells_ex(int mech, int ncell, const double* var_in, const double* fix, const double* rconst, double tstart,
                                          double tend, const double* atol, const double* rtol, int ntol,                             /* rows per cell */
                                          const double* rpar, const int32_t* ipar, double* var_out, int32_t* ierr, int32_t* stats, double* t_h,
                                          int ns, const double* ts, double* ysample, int32_t* nout);
int mistra_chem_rosenbrock_dense_cells_device(int mech, int ncell, const double* d_var_in, const double* d_fix, const double* d_rconst, double tstart,
                                              double tend, const double* d_atol, const double* d_rtol, int ntol,                     /* device arrays */
                                              const double* rpar, const int32_t* ipar,                                               /* host arrays */
                                              double* d_var_out, int32_t* d_ierr, int32_t* d_stats, double* d_texit_hexit,
                                              const double* d_hstart, void* hip_stream, int ns, const double* ts /* host */, double* d_ysample,
                                              int32_t* d_nout);

/* THE OPERATORS: KPP's four building blocks — Fun_x, Jac_SP_x, KppDecomp_x, KppSolve_x — at a state the caller gives, for a batch of cells, with no
 * integration.  Per cell, V = var, F = fix, RCT = rconst:
 *     vdot [ncell][NVAR]        Fun_x(V, F, RCT)
 *     jvs  [ncell][LU_NONZERO]  Jac_SP_x(V, F, RCT) in KPP's slot order (LU_CROW / LU_ICOL: mistra_chem_jac_pattern); the fill-in slots are +0.0
 *     x    [fun_rhs + nrhs][ncell][NVAR]  (the series' block layout)   A x_j = b_j with A = shift*I - J, J the matrix of jvs: ros_PrepareMatrix_x's Ghimj
 *          for shift = 1/(Direction*H*gamma), backward Euler's matrix for shift = 1/h.  A is factorised once per cell, then solved for every right-hand
 *          side: the cell's own vdot (fun_rhs /= 0: row 0 of x) followed by the nrhs rows of rhs [nrhs][ncell][NVAR].  shift may have any sign and be zero.
 *     ising [ncell]             what KppDecomp_x returns in IER: the first row (1-based) whose PREPARED diagonal is exactly zero, otherwise 0.  Where
 *          ising > 0 no factorisation runs and the cell's rows of x are +0.0; vdot and jvs are produced all the same.  A pivot that becomes zero, tiny
 *          or non-finite DURING the elimination is not flagged, exactly as in KPP: the rows then hold what the arithmetic gives (inf / NaN).
 * vdot and jvs are the values the integrator's own first Fun_x / Jac_SP_x of a step form, and the fun_rhs row is that step's K(1) for its shift, bit for bit
 * (the right-hand side rides through the factorisation as a step's stage 1 does).  Every row of rhs goes through the full KppSolve_x: its result does not
 * depend on where the row stands, on the other rows, or on what else the call asks for.
 * vdot, jvs: each may be NULL (not wanted).  x NULL: no solve; nrhs, rhs, shift and ising are then not looked at.  nshift: 1 (one shift shared by all cells)
 * or ncell.  Refused with a text of its own before a device is touched: x, vdot and jvs all NULL; x with fun_rhs + nrhs < 1; nrhs < 0 or above
 * MISTRA_OPS_MAX_RHS; nrhs > 0 with a NULL rhs; a NULL ising or shift with x; nshift neither 1 nor ncell; (_ex) a shift that is not finite.
 * _device: device arrays, shift included (nshift entries); asynchronous on the stream, no options block and so no in-flight limit.  _ex splits the batch
 * over the device slots as mistra_chem_rosenbrock_ex does and fails while a column step of the mechanism is open.  Nothing process-wide is read: the
 * options in force, the integrator policy and step reuse are not involved.  No user slot: both ids fail with the slot's text, mistra_chem_jac_pattern too.
 * mistra_chem_jac_pattern needs no device and no mistra_chem_init: it reads <mechanism directory>/<name>.mech; each pointer may be NULL. */
#define MISTRA_OPS_MAX_RHS 256
int mistra_chem_jac_pattern(int mech, int32_t* crow /* [NVAR+1] */, int32_t* icol /* [LU_NONZERO] */, int32_t* diag /* [NVAR] */);   /* 1-based: LU_CROW, LU_ICOL, LU_DIAG */
int mistra_chem_ops_ex(int mech, int ncell, const double* var, const double* fix, const double* rconst, double* vdot, double* jvs, int nshift,
                       const double* shift, int fun_rhs, int nrhs, const double* rhs, double* x, int32_t* ising);
int mistra_chem_ops_device(int mech, int ncell, const double* d_var, const double* d_fix, const double* d_rconst, double* d_vdot, double* d_jvs, int nshift,
                           const double* d_shift, int fun_rhs, int nrhs, const double* d_rhs, double* d_x, int32_t* d_ising, void* hip_stream);

/* THE REPLAY: Ros3 along a step sequence the caller prescribes.  Step n of a cell is made with H = hsteps[row][n] and accepted whatever
 * its error estimate; the estimate (Rosenbrock_x's Err of that step under the call's tolerances) goes to err_log[cell][n].  The sequence is what the
 * step-control trace hands out: the records of a traced call whose code has bit 0 set, H as attempted.  A replay of those steps under the traced call's
 * arguments repeats that call's accepted steps operand for operand: var_out and Texit equal the traced call's bit for bit and err_log its accepted records'
 * Err, provided no accepted step of the trace met a zero pivot.  Perturbed copies of a cell replayed along ONE sequence give a smooth map from the
 * perturbation to the end state (internal numerical differentiation): central differences of them are good to round-off / eps, where differences of two
 * adaptive calls carry the tolerance.
 *   cap, hrows, hsteps [hrows][cap], nsteps [hrows]   the table: hrows = 1 (one sequence shared by all cells) or ncell (row and count per cell);
 *          0 <= nsteps[r] <= cap.  Entries of hsteps behind a row's count are not read.
 *   err_log [ncell][cap], may be NULL (not wanted)     entries behind a cell's count are not touched
 * Of the options the call reads ipar[0] (Autonomous), ipar[1] and atol / rtol, and ipar[3], which must be 2 (Ros3); rpar is decoded as Rosenbrock_x decodes it
 * (codes -1 .. -4 are whole-call results decided on the host, -5 as in the siblings) and then ignored: there are no Hmin, Hmax, Hstart and factors, no
 * clipping to tend and no Max_no_steps.  tstart is where T starts; tend gives the direction (tend >= tstart: forward) and nothing else.
 * Per cell: ierr = 1, or -7 where a step fails Rosenbrock_x's test (T + 0.1*H == T or H <= Roundoff; the cell leaves with the steps made so far), or -8 where
 * a step's matrix has a zero pivot (no halving: Nsng = 1, the row in mistra_chem_singular_rows after _ex, the cell leaves at the last accepted state).
 * stats: Nstp = Nacc = Njac = Ndec = the steps made, Nsol three times that, Nrej = 0 (a -8 exit: one more Njac and Ndec, Nsng = 1).  t_h [ncell][3] / d_texit_hexit [ncell][2]: the T reached, the last H
 * made (0: none), and (t_h) the same H again.  nsteps = 0 is legal: var_out = var_in, ierr = 1, zeros.
 * Refused with a text before a device is touched: cap < 0; hrows neither 1 nor ncell; NULL hsteps with cap > 0; NULL nsteps; a count outside 0 .. cap where
 * the counts are host arrays; a method other than Ros3; a user slot.
 * _ex: host arrays; the batch is split over the device slots as mistra_chem_rosenbrock_trace_ex splits it, each block with its rows; fails while a column
 * step of the mechanism is open.  _device: the cell data are device arrays and the call is asynchronous on the stream; hsteps / nsteps are HOST arrays where
 * hrows = 1 (read before the call returns; the nsteps[0] steps travel behind the call's options, MISTRA_ROSENBROCK_CALLS_IN_FLIGHT blocks: nsteps[0] <=
 * MISTRA_REPLAY_MAX_SHARED, refused with a text otherwise)
 * and DEVICE arrays where hrows = ncell > 1 (read in stream order; host memory the cells' device cannot reach is refused with a text; the kernel clamps a count
 * above cap to cap and takes a negative one as 0).
 * _cells: tolerances per cell as in mistra_chem_rosenbrock_cells_ex; a row refused with -5 leaves as there and its err_log row is not written.
 * Nothing process-wide is read: the options in force, the integrator policy and step reuse are not involved. */
#define MISTRA_REPLAY_MAX_SHARED MISTRA_SERIES_MAX_LEGS
int mistra_chem_rosenbrock_replay_ex(int mech, int ncell, const double* var_in, const double* fix, const double* rconst, double tstart, double tend,
                                     const double* atol, const double* rtol, const double* rpar, const int32_t* ipar, int cap, int hrows,
                                     const double* hsteps, const int32_t* nsteps, double* var_out, int32_t* ierr, int32_t* stats, double* t_h,
                                     double* err_log);
int mistra_chem_rosenbrock_replay_cells_ex(int mech, int ncell, const double* var_in, const double* fix, const double* rconst, double tstart, double tend,
                                           const double* atol, const double* rtol, int ntol,                                         /* rows per cell */
                                           const double* rpar, const int32_t* ipar, int cap, int hrows, const double* hsteps, const int32_t* nsteps,
                                           double* var_out, int32_t* ierr, int32_t* stats, double* t_h, double* err_log);
int mistra_chem_rosenbrock_replay_device(int mech, int ncell, const double* d_var_in, const double* d_fix, const double* d_rconst, double tstart,
                                         double tend, const double* atol, const double* rtol, const double* rpar, const int32_t* ipar,      /* host arrays */
                                         int cap, int hrows, const double* hsteps, const int32_t* nsteps,      /* host (hrows = 1) or device (hrows = ncell) */
                                         double* d_var_out, int32_t* d_ierr, int32_t* d_stats, double* d_texit_hexit, double* d_err_log, void* hip_stream);
int mistra_chem_rosenbrock_replay_cells_device(int mech, int ncell, const double* d_var_in, const double* d_fix, const double* d_rconst, double tstart,
                                               double tend, const double* d_atol, const double* d_rtol, int ntol,                     /* device arrays */
                                               const double* rpar, const int32_t* ipar,                                               /* host arrays */
                                               int cap, int hrows, const double* hsteps, const int32_t* nsteps, double* d_var_out, int32_t* d_ierr,
                                               int32_t* d_stats, double* d_texit_hexit, double* d_err_log, void* hip_stream);

/* AbsTol from each cell's own state, on the device in stream order: d_atol[c] = max(floor, factor * max_i |d_var[c][i]|), i over NVAR.  NaN entries
 * are ignored; a cell with no positive entry gets floor.  The product is one rounding of two exact operands, so the host restatement
 * max(floor, factor * fmax-reduction of |var|) gives the same bits.  factor or floor that is not finite and positive fails with a text before a device
 * is touched.  Needs NVAR alone: user slots have it.  d_atol is a tolerance array of width ntol = 1 for the cells entries above. */
int mistra_chem_cell_atol_device(int mech, int ncell, const double* d_var, double factor, double floor, double* d_atol, void* hip_stream);

/* OPT-IN integrator policy, one per mechanism, process-wide, off by default: what the entries that carry no options of their own
 * run instead of Ros3 and the options' AbsTol.  While none is set nothing differs from a library without these entries.
 *   method       1 .. 5 in IPAR(4)'s numbering: Ros2, Ros3, Ros4, Rodas3, Rodas4.  0 is refused with a text (in Rosenbrock_x it selects Ros4: a quiet
 *                default here would be a trap); 2 keeps Ros3 and sets the tolerance part alone.  A user slot has Ros3 only.
 *   atol_factor  0: no cell-relative AbsTol, the options in force supply AbsTol.  Otherwise atol_factor and atol_floor are finite and positive
 *                (mistra_chem_cell_atol_device's rule and texts), and every species of a cell gets AbsTol = max(atol_floor, atol_factor * max_i |VAR(i)|),
 *                the maximum over the state the integrator receives, NaN entries ignored, formed once per call inside the integrator kernel.
 * Everything else — RelTol, Hmin / Hmax / Hstart, the four factors, Max_no_steps, the autonomous flag — stays the options in force:
 * mistra_chem_set_options' when set, else INTEGRATE_x's values.  Options and policy are kept apart: setting or clearing one keeps the other, and
 * mistra_chem_set_options goes on refusing the four other methods.
 * Honoured by mistra_chem_integrate, _integrate_ex, _integrate_env_ex, _integrate_hstart_ex, _integrate_device, _integrate_device_hstart,
 * _integrate_common(_status) (ATOL / RTOL written to the COMMON block stay the options' values), mistra_chem_drive_device and mistra_chem_drive / _begin /
 * _end, on every device slot.  Ignored by the entries whose options travel with the call (mistra_chem_rosenbrock*) and by mistra_chem_debug_first_step(_ex),
 * which stays the Ros3 diagnostic.  Step reuse works with a policy (a remembered step goes before Hstart); set and clear empty the step memory and fail
 * while a column step of the mechanism is open.
 * mistra_chem_check_policy: the checks alone, no device, works before init.  mistra_chem_get_policy: *is_set = 0 | 1, the rest written when set; any of
 * them may be NULL; works before init.
 * Environment, read once by the first initialisation or the first policy entry: MISTRA_CHEM_METHOD and MISTRA_CHEM_ATOL_REL set gas, aer and tot,
 * MISTRA_CHEM_METHOD_G / _A / _T and MISTRA_CHEM_ATOL_REL_G / _A / _T one of them and go before the former.  A method is a name (ros2, ros3, ros4, rodas3,
 * rodas4, any letter case) or 1 .. 5; ATOL_REL is `factor` or `factor,floor` (floor 1e-25 when left out).  A value that cannot be read makes
 * mistra_chem_init and every policy entry fail with a text that names the variable.  mistra_chem_finalize puts the environment's policy back. */
int mistra_chem_set_policy(int mech, int method, double atol_factor, double atol_floor);
int mistra_chem_clear_policy(int mech);
int mistra_chem_get_policy(int mech, int32_t* is_set, int32_t* method, double* atol_factor, double* atol_floor);
int mistra_chem_check_policy(int mech, int method, double atol_factor, double atol_floor);

/* The method tables the kernels were compiled with (Ros2_x .. Rodas4_x, gas.f:1514-1895), pure host, works before init: method 1 .. 5, 0 = 3.
 * *S = ros_S; A15 / C15 = ros_A / ros_C, row-wise lower triangle, S*(S-1)/2 entries; M6, E6, gamma6 = ros_M, ros_E, ros_Gamma; newf6 =
 * ros_NewF (0/1); *elo = ros_ELO.  Entries past the method's own are zero; any pointer may be NULL.  (ros_Alpha is not kept: Fun_x ignores T.) */
int mistra_chem_method_table(int method, int* S, double* A15, double* C15, double* M6, double* E6, double* gamma6,
                             int32_t* newf6, double* elo);

/* The rows of the zero pivots a cell met: what KppDecomp_x returns in IER — the first row k whose diagonal is exactly zero when the
 * elimination reaches it (gas.f:6157) — and ros_PrepareMatrix_x prints once per failed decomposition ("Warning: LU Decomposition
 * returned ising = k", gas.f:1456) before it halves H.  rows8[0 .. min(Nsng, 8)-1] = row numbers (1-based, = species numbers) in
 * order of occurrence for cell `cell` (0-based index into the batch) of the LAST host-buffer integration of this mechanism
 * (mistra_chem_integrate[_ex], mistra_chem_integrate_common[_status]); entries past Nsng are undefined.  The rows stay on the
 * device until asked for: call it only for cells whose statistics report Nsng > 0 (the Fortran shim does, to print the line). */
int mistra_chem_singular_rows(int mech, int cell, int32_t* rows8);

/* Update_RCONST_x for ncell cells (gas.f:275 | aer.f:304 | tot.f:1040; called by x_drive right before INTEGRATE_x, gas.f:172):
 * rconst[cell][NREACT] from env[cell][mistra_chem_rates_env_size(mech)], the per-cell inputs the generated routine and its
 * rate laws (kpp.f90:7127-8601) read from COMMON /cb_1/, /kpp_rate_x/, /ph_r_x/ and C.  Sizes: gas 74 doubles, aer 330,
 * tot 544 (instead of the 331 / 807 / 1627 rate constants); gas e.g.: aircc, te, h2oppm, pk | conv1, xhal, xiod, xhet1,
 * xhet2 | ycwd(1:2) | ph_rat(1:47) | FIX(1:3) | what fdhetg reads.  The layout of each mechanism is listed by name in
 * mistra_amd/mech/<mech>.rates_env.json (made by tools/extract_rates.py together with the rate table <mech>.rates the
 * library loads); Fortran array names there index as the reference declares them (kpp.f90:7140-7180).  Host buffers /
 * device buffers on a HIP stream.  The lazy initialisation of the Fortran-facing entry points applies to the host-buffer
 * form. */
int mistra_chem_rates_env_size(int mech);
/* The deepest operand stack any postfix program of a rate table (<mech>.rates; stcoeff = 0) or of a table of accommodation coefficients
 * (<mech>.stcoeff; stcoeff = 1) needs, read by the loader the library itself uses; needs no device.  -1 where that loader refuses the file
 * (mistra_chem_last_error() says why): the evaluator's stack holds 12 entries per thread, a table with a deeper program is not loaded. */
int mistra_chem_table_stack_depth(const char* path, int stcoeff);
int mistra_chem_update_rconst(int mech, int ncell, const double* env, double* rconst);
int mistra_chem_update_rconst_device(int mech, int ncell, const double* d_env, double* d_rconst, void* hip_stream);

/* ---- The hand-over halves of the per-layer drivers on the device: what gas_drive / aer_drive / tot_drive
 * (gas.f:60-217 | aer.f:59-246 | tot.f:59-982, with aer_mk.dat / aer_km.dat) do around Update_RCONST_x + INTEGRATE_x, for a batch of
 * layers ("cells") whose data stay in HBM.  Per layer k, cell-major:
 *   s1 [j1], s3 [j5]          s1(1:j1,k), s3(1:j5,k) of module gas_common (non-radical / radical gases)
 *   sl1 [nkc][j2]             sl1(1:j2,1:nkc,k) of COMMON /blck17/ (the layer's Fortran slab as it stands in memory), j2 = 121, nkc = 4
 *   sion1 [nkc][j6]           sion1(1:j6,1:nkc,k), j6 = 55
 *   scal [6]                  air, h2o, cvv1..cvv4 (the drivers' arguments; gas reads the first two, aer the first four)
 *   var [NVAR], fix [NFIX]    C = VAR | FIX of COMMON /GDATA_x/
 *   bg [NREACT][2]            bg(1:2,1:NREACT,kl) of COMMON /budg/ (bud_x.f): [..][0] instantaneous rate, [..][1] += dt * rate
 *   bgs [122][2]              bgs(1:2,1:122,k) of COMMON /budgs/ (bud_s_x.f); slots the mechanism does not set are left alone
 * Everything is index work and plain products in the reference's operation order: bit-identical results.
 *
 * mistra_chem_set_species_maps: the model's species index maps (module gas_common, built once by mk_interface, utils.f90:82-140, from
 * the user's species lists) for one mechanism: gas_m2k [j1][2] = gas_m2k_x(1:2,j) (C index, s1 index), gas_k2m [j1] = gas_k2m_x(j)
 * (C index of s1(j)), rad_* likewise for s3; 1-based as the Fortran holds them.  Host arrays; call once after init.  Restriction: every C index
 * must be a VARIABLE species (1..NVAR) — match_mk_indexes searches all NSPEC names, so a user list naming a fixed species (O2, N2, H2O ...) is
 * legal in the reference; here it is refused with "species map entry out of range" (no shipped gas_species / gas_radical list names one).
 * mistra_chem_drive_dims: j2, j6, nkc (global_params.f90:96-103) and the slot count of bgs.  Any pointer may be NULL. */
int mistra_chem_set_species_maps(int mech, int j1, const int32_t* gas_m2k, const int32_t* gas_k2m, int j5,
                                 const int32_t* rad_m2k, const int32_t* rad_k2m);
int mistra_chem_drive_dims(int mech, int* j2, int* j6, int* nkc, int* nbgs);

/* x_drive up to (not including) Update_RCONST_x (gas.f:132-167 | aer.f:152-214 | tot.f:212-599): C <- s1, s3 through the maps, FIX
 * from air / h2o / cvv, the liquid-phase species from sl1 / sion1 — which aer_drive and tot_drive first clamp to >= 0 IN PLACE
 * (tot.f:226-227), so d_sl1 / d_sion1 are in/out.  Entries of VAR that the driver does not set (KPP's dummy products) keep what
 * d_var holds, as COMMON /GDATA_x/ does in the reference.  Asynchronous on hip_stream. */
int mistra_chem_pack_device(int mech, int ncell, const double* d_s1, const double* d_s3, double* d_sl1, double* d_sion1,
                            const double* d_scal, double* d_var, double* d_fix, void* hip_stream);

/* The concentrations Update_RCONST_x reads (C(ind_Hplz), FIX(..) ...: the `c(i)` / `fix(i)` entries of the rate evaluator's input
 * vector, mistra_amd/mech/<mech>.rates_env.json) copied from the packed C into d_env [ncell][rates_env_size]; the other entries
 * (/cb_1/, /kpp_rate_x/, ph_rat: MISTRA_RATES_ENV_x of shim/mistra_kpp_rates.f90) are the caller's. */
int mistra_chem_rates_env_from_c_device(int mech, int ncell, const double* d_var, const double* d_fix, double* d_env, void* hip_stream);

/* bud_x (bud_g.f | bud_a.f | bud_t.f: every reaction's rate RCONST(i) * reactants, called by x_drive for the layers in il(1:nlev),
 * gas.f:179-184) and bud_s_x (bud_s_g.f | ..: the selected sulphur / DMS rates, every layer, gas.f:187) on the state the integration
 * left.  d_bg or d_bgs may be NULL (a caller passes to d_bg only the layers that are budget levels). */
int mistra_chem_budgets_device(int mech, int ncell, const double* d_var, const double* d_fix, const double* d_rconst, double dt,
                               double* d_bg, double* d_bgs, void* hip_stream);

/* The hand-over after the integration (gas.f:189-215 | aer.f:229-244 | tot.f:619-982): s1, s3 through the inverse maps, sl1 / sion1
 * from the liquid-phase species. */
int mistra_chem_unpack_device(int mech, int ncell, const double* d_var, double* d_s1, double* d_s3, double* d_sl1, double* d_sion1,
                              void* hip_stream);

/* One x_drive per layer for a batch of layers without anything but the model arrays crossing PCIe: pack -> env <- C -> Update_RCONST_x
 * -> INTEGRATE_x(tin, tin + dt) -> budgets -> hand-over, all on hip_stream.  d_env: the rate evaluator's input with the caller's
 * part filled in.  d_bg / d_bgs / d_texit_hexit may be NULL. */
int mistra_chem_drive_device(int mech, int ncell, double* d_s1, double* d_s3, double* d_sl1, double* d_sion1, const double* d_scal,
                             double* d_env, double* d_var, double* d_fix, double tin, double dt, int32_t* d_ierr, int32_t* d_stats,
                             double* d_texit_hexit, double* d_bg, double* d_bgs, void* hip_stream);

/* The same from the model's own arrays in HOST memory: what a Fortran caller hands over (shim/mistra_kpp_drive.f90: KPP_DRIVE_RUN) —
 * ONE call per mechanism and 10-s step for all layers that run it (kpp.f90:4454-4467 chooses the mechanism per layer), instead of one
 * x_drive per layer.  The arrays are the model's, dimensioned for n layers, layer k at its Fortran place:
 *   layer [nlayer]            the k of each layer of the batch, 1-based, in the order of the layer loop
 *   s1 [n][j1], s3 [n][j5]    s1(1:j1,1:n), s3(1:j5,1:n) of module gas_common (j1, j5: as given to mistra_chem_set_species_maps)
 *   sl1 [n][nkc][j2]          COMMON /blck17/ sl1(j2,nkc,n); sion1 [n][nkc][j6] likewise
 *   scal [nlayer][6], env [nlayer][rates_env_size]      per layer of the batch (not per k): air, h2o, cvv1..4 and the rate evaluator's input
 *                             with the caller's part filled in (MISTRA_RATES_ENV_x); the concentrations in it are refilled on the device
 *   bg [nlev][nrxn][2]        COMMON /budg/ bg(2,nrxn,nlev) (global_params.f90:110-115), or NULL; bg_level [nlayer]: kl (1-based) where layer
 *                             i is the budget level il(kl), else 0 (gas.f:179-184)
 *   bgs [n][122][2]           COMMON /budgs/ bgs(2,122,n), or NULL
 * in/out: s1, s3, sl1, sion1 (rows of the batch's layers), bg (rows of its levels), bgs.  Out, per layer of the batch, each may be NULL: ierr,
 * stats [8], t_h [3] as mistra_chem_integrate_ex returns them; c_packed [nlayer][NVAR+NFIX]: C = VAR | FIX as the pack half handed it to
 * INTEGRATE_x (diagnostics / tests).  KPP's dummy products, which the drivers never set, start from 0 in every layer (the reference carries
 * the previous layer's leftovers: INTEGRATION.md §4).  Synchronous; one pinned block up, the device chain on a private stream, one block down. */
int mistra_chem_drive(int mech, int nlayer, const int32_t* layer, int n, double* s1, double* s3, double* sl1, double* sion1, const double* scal,
                      const double* env, double tin, double dt, int32_t* ierr, int32_t* stats, double* t_h, double* bg, int nrxn,
                      const int32_t* bg_level, double* bgs, double* c_packed);
/* The same in two halves, so that the three mechanisms of one column step run SIDE BY SIDE on the device: kpp_driver gives every layer to one of
 * gas / aer / tot (kpp.f90:4454-4467), the three batches touch disjoint rows of the model arrays, and a column's 148 cells leave most of the GPU's 256 CUs
 * idle behind any one mechanism — a step then lasts as long as its slowest cell, not as the three mechanisms' slowest cells in a row (BTZ96: 14.4 -> 8.4 ms,
 * INTEGRATION.md §4d).  mistra_chem_drive_begin takes mistra_chem_drive's arguments, gathers the layers, and returns once the copies and kernels are
 * enqueued on the mechanism's private stream; mistra_chem_drive_end(mech) waits for them and scatters the results into the arrays given to begin.  Between
 * the two the caller must not touch those arrays' rows (nor ierr, stats, t_h, c_packed).  One step per mechanism may be open at a time: while it is,
 * the host-buffer calls of that mechanism fail — mistra_chem_drive(_begin), mistra_chem_integrate(_ex, _env_ex), mistra_chem_update_rconst,
 * mistra_chem_integrate_common(_status), mistra_chem_set_species_maps, mistra_chem_singular_rows, mistra_chem_debug_first_step — until
 * mistra_chem_drive_end has fetched it; the *_device calls, the liq_parm calls and the other mechanisms are not affected.
 * shim/mistra_kpp_drive.f90: KPP_DRIVE_RUN issues all mechanisms, then fetches them in mechanism order. */
int mistra_chem_drive_begin(int mech, int nlayer, const int32_t* layer, int n, double* s1, double* s3, double* sl1, double* sion1, const double* scal,
                      const double* env, double tin, double dt, int32_t* ierr, int32_t* stats, double* t_h, double* bg, int nrxn,
                      const int32_t* bg_level, double* bgs, double* c_packed);
int mistra_chem_drive_end(int mech);

/* OPT-IN, NOT the reference's behaviour: carry every layer's step size from one column step to the next.  INTEGRATE_x starts
 * every call at Hstart = 1e-3 s (gas.f:743) and leaves the last accepted step in STEPMIN (gas.f:770) for a driver to feed back; the reference never does.  With
 * reuse on for `mech`, mistra_chem_drive(_begin) keeps a step memory on the device — one double per model layer k = 1..n (n: the call's argument), 0 = none —
 * and, on the mechanism's stream, in order with the rest of the chain: starts layer[i] at mem[layer[i] - 1] (mistra_chem_integrate_device_hstart's d_hstart;
 * 0: the call's Hstart), and after the integrator clears the whole memory and stores Hexit of the layers that returned IERR = 1.  So a layer starts from the
 * call's Hstart again if it was not in the mechanism's PREVIOUS column step (cloud formed or went: it ran another mechanism in between) or if it failed there.
 * The three mechanisms' memories are independent.  A remembered step goes before RPAR(3) of the options in force, which serves (or 1e-3) where there is none.
 * The memory is forgotten when reuse is switched, on mistra_chem_set_options (also when it clears them), on mistra_chem_finalize and every re-initialisation, and
 * when n changes.  Off (the default) nothing of this runs: the reference's path, bit for bit.  mistra_chem_drive_device is not affected: a device-resident
 * caller composes the public pieces with mistra_chem_integrate_device_hstart.
 *
 * mistra_chem_set_step_reuse / mistra_chem_get_step_reuse (-> 0 | 1): host state, per mechanism, process-wide; they work before init and without a device, and the
 * flag outlives mistra_chem_finalize.  MISTRA_CHEM_HSTART_REUSE=1 in the environment turns reuse on for all three mechanisms when the library starts (read once,
 * by the first initialisation or the first of these two calls; unset or 0: off) — for a model binary that is already linked.
 * mistra_chem_get_step_memory / mistra_chem_set_step_memory: the memory of `mech` from / to a host double[n], for a restart file (a restarted run that puts it
 * back after turning reuse on continues like an uninterrupted one) or to look at it.  get: zeros while nothing is remembered; n must else be the memory's.  set:
 * entries finite and >= 0.  Primary device; they initialise the library like the Fortran entry points.
 * set_step_reuse, get_step_memory and set_step_memory fail while a column step of the mechanism is open, like the other host-buffer calls. */
int mistra_chem_set_step_reuse(int mech, int on);
int mistra_chem_get_step_reuse(int mech);
int mistra_chem_get_step_memory(int mech, int n, double* h);
int mistra_chem_set_step_memory(int mech, int n, const double* h);

/* ---- liq_parm, first slice: the gas <-> particle mass-transfer coefficients of fast_k_mt_a (mech = aer;
 * kpp.f90:2683-2947) and fast_k_mt_t (mech = tot; kpp.f90:2421-2676), called by liq_parm every 120 s (kpp.f90:617,637), for nlayer
 * layers at once.  Per layer, as the COMMON blocks hold them for that k:
 *   d_ff [nka][nkt]           ff(1:nkt,1:nka,k) of /cb52/: the 2-D particle spectrum (nkt = nka = 70)
 *   d_cw, d_cm [nkc]          cw(1:nkc,k), cm(1:nkc,k) of /blck12/ (liquid water content per chemical bin; cm is the activity switch)
 *   d_freep                   freep(k): mean free path (the routine's argument)
 *   d_alpha, d_vmean [NSPEC]  alpha(:,k), vmean(:,k) of /kpp_2aer/ | /kpp_2tot/ (accommodation coefficients, mean molecular speeds)
 *   d_xkmt [nkc][NSPEC]       xkmt(:,1:nkc,k) of /kpp_laer/ | /kpp_ltot/: in/out — written for the 50 exchanged species of the active
 *                             bins (cm > 0 and cw > 0), everything else left as it is, like the reference
 *   d_t, d_p                  t(k), p(k) of /cb53/: temperature and pressure (arguments of the terminal velocity vterm, str.f90:2793)
 *   d_vt [nkc]                vt(1:nkc,k) of /kpp_vt/: in/out — the LWC-weighted sedimentation velocity of every bin with cw > 0 ("computed
 *                             whatever LWC", kpp.f90:2421-2432: also for bins with cm = 0), read by SR sedl (str.f90:2704, 2751); bins with
 *                             cw <= 0 left as they are.  d_vt = NULL: not computed (then d_t, d_p may be NULL too)
 * and for the call: d_rq [nka][nkt] = rq(1:nkt,1:nka) of /cb50/ (particle radii, um), kw [nkw] (host; nkw must be nka = 70) and ka of /blck06/,
 * ifeed and nkc_l of module config.  The summation order is the reference's: bit-identical coefficients; vt likewise up to 10 um radius
 * (Stokes regime), to the last place of the device log / exp above (Beard's polynomial).  With d_vt the call does everything
 * fast_k_mt_a / fast_k_mt_t do: the Fortran call can be dropped.  Asynchronous on hip_stream; nothing is staged, kw travels with the launch. */
int mistra_chem_fast_k_mt_device(int mech, int nlayer, const double* d_ff, const double* d_rq, const int32_t* kw, int nkw, int ka, int ifeed,
                                 int nkc_l, const double* d_cw, const double* d_cm, const double* d_freep, const double* d_alpha,
                                 const double* d_vmean, double* d_xkmt, const double* d_t, const double* d_p, double* d_vt, void* hip_stream);

/* ---- liq_parm, second slice: the Henry constants of henry_a (mech = aer; kpp.f90:1914-2145) | henry_t (tot;
 * kpp.f90:1676-1907) and the forward / backward rate constants of the aqueous equilibria of equil_co_a (kpp.f90:3162-3363) | equil_co_t
 * (kpp.f90:2954-3155), which liq_parm calls every time step (kpp.f90:614-616, 634-636), for nlayer layers at once.  Per layer k:
 *   d_tt                      tt(k): temperature (/cb53/ t)
 *   d_henry [NSPEC]           henry(:,k) of /kpp_laer/ | /kpp_ltot/: written whole — the inverse dimensionless constant of the species
 *                             the routine lists, 0 for the others (NSPEC = NVAR + NFIX)
 *   d_conv2 [nkc]             conv2(1:nkc,k) of /blck13/ (1/(1000 cw); <= 0 = no liquid water in the bin)
 *   d_xgamma [nkc][j6]        xgamma(1:j6,1:nkc,k) of /kpp_mol/ (activity coefficients)
 *   d_xkef, d_xkeb [nkc][NSPEC]   xkef(:,1:nkc,k), xkeb(:,1:nkc,k) of /kpp_laer/ | /kpp_ltot/: in/out — a bin with conv2 <= 0 is zeroed, in
 *                             the others the listed species are written and the rest left as they are, like the reference; equil_co_a sets
 *                             bins 1..2 only, equil_co_t all four
 * The tables (mistra_amd/mech/<mech>.liq) are cut out of the reference source by tools/extract_liq.py; products are formed in the
 * reference's order, exp is the device library's (last-place differences against the host libm). */
int mistra_chem_henry_device(int mech, int nlayer, const double* d_tt, double* d_henry, void* hip_stream);
/* v_mean_a (tt,nmaxf) (kpp.f90:1472-1670) | v_mean_t (kpp.f90:1268-1465), which liq_parm calls every time step (kpp.f90:612, 632): the mean
 * molecular speeds vmean(:,k) = sqrt(tt(k)/M)*4.60138 of the species the routine lists, 0 for the others, for nlayer layers at once.
 *   d_tt [nlayer]             tt(k)
 *   d_vmean [nlayer][NSPEC]   vmean(:,k) of /kpp_2aer/ | /kpp_2tot/, written whole (NSPEC = NVAR + NFIX).  The reference zeroes the layers above
 *                             nmaxf as well (`vmean(:,:) = 0._dp`): a caller that replaces the routine does that once, they never change.
 * Table: mistra_amd/mech/<mech>.vmean, cut out of the reference source by tools/extract_vmean.py.  Quotient, square root and product round
 * once each as in the compiled reference: bit-identical (tests/test_gpu_liq.py). */
int mistra_chem_v_mean_device(int mech, int nlayer, const double* d_tt, double* d_vmean, void* hip_stream);
/* st_coeff_a (kpp.f90:857-1038) | st_coeff_t (kpp.f90:664-851), which liq_parm calls every time step (kpp.f90:614, 634): the accommodation
 * coefficients alpha(:,k) fast_k_mt_x reads, for nlayer layers at once.
 *   lp_joyce14bc, lp_buxmann15alph   the namelist switches of module config the routine branches on (alpha(NO3), alpha(N2O5) = a_n2o5(k,1),
 *                             kpp.f90:8377; alpha(ICl), alpha(IBr))
 *   d_env [nlayer][5]         per layer: t(k) (/cb53/), cw(1,k), cm(1,k) (/blck12/), sion1(13,1,k), sion1(14,1,k) (/blck17/) — the last four are
 *                             read by a_n2o5 only
 *   d_alpha [nlayer][NSPEC]   alpha(:,k) of /kpp_2aer/ | /kpp_2tot/, written whole: 0.1 for the species the routine does not list, min(1, .)
 *                             applied (NSPEC = NVAR + NFIX).  The reference computes layers 2..nf; layer 1 keeps the default 0.1.
 * Tables: mistra_amd/mech/<mech>.stcoeff (tools/extract_stcoeff.py: every assignment a postfix program, run by the evaluator of the rate
 * constants); the restated table is bit-exact against the running model on the CPU, the device to the last place of its exp. */
int mistra_chem_st_coeff_device(int mech, int nlayer, int lp_joyce14bc, int lp_buxmann15alph, const double* d_env, double* d_alpha, void* hip_stream);
int mistra_chem_equil_co_device(int mech, int nlayer, int nkc, int j6, const double* d_tt, const double* d_conv2, const double* d_xgamma,
                                double* d_xkef, double* d_xkeb, void* hip_stream);

/* The liq_parm kernels above on HOST buffers (same layouts, layer-major as the model holds them: every array of the reference has the
 * layer as its last dimension, so a run of layers kmin..kmax is handed over in place — ff(1,1,kmin), xkmt(1,1,kmin) ...): what the Fortran
 * shim calls (shim/mistra_kpp_liq.f90: FAST_K_MT_BATCH, HENRY_BATCH, V_MEAN_BATCH, ST_COEFF_BATCH, EQUIL_CO_BATCH, CW_RC_BATCH, DRY_RATES_BATCH; drop-ins with the reference's own signatures in
 * shim/mistra_kpp_model.f90).  Synchronous; primary device. */
int mistra_chem_fast_k_mt(int mech, int nlayer, const double* ff, const double* rq, const int32_t* kw, int nkw, int ka, int ifeed, int nkc_l,
                          const double* cw, const double* cm, const double* freep, const double* alpha, const double* vmean, double* xkmt,
                          const double* t, const double* p, double* vt);
int mistra_chem_henry(int mech, int nlayer, const double* tt, double* henry);
int mistra_chem_v_mean(int mech, int nlayer, const double* tt, double* vmean);
int mistra_chem_st_coeff(int mech, int nlayer, int lp_joyce14bc, int lp_buxmann15alph, const double* env, double* alpha);
/* cw_rc (nmaxf) (kpp.f90:2152-2414; liq_parm calls it every time step, kpp.f90:609) and, with dry != 0, dry_cw_rc (nmax) (kpp.f90:4580-4690): liquid water
 * content, mean radius, and — cw_rc — the water mass and the chemistry switch conv2 of the particle bins of nlayer layers, as moments of the
 * two-dimensional particle spectrum summed in the reference's own order (bit-identical: tests/test_gpu_liq.py).  Mechanism-independent.  Host buffers,
 * layer-major as the model holds them:
 *   ff [nlayer][nka][nkt]     ff(1:nkt,1:nka,k) of /cb52/;  rq [nka][nkt], e [nkt]: /cb50/;  kw [nka], ka: /blck06/;  ifeed: module config
 *   feu [nlayer]              relative humidity feu(k) of /cb54/;  cloud [nlayer][4]: cloud(1:nkc,k) of /kpp_l1/ as 0 | 1 (the hysteresis of bins 1, 2)
 *   crys4 [4]                 xcryssulf, xcrysss, xdelisulf, xdeliss of /kpp_crys/
 *   rc, cw, cm, conv2 [nlayer][4]   rc(:,k) of /blck11/, cw(:,k), cm(:,k) of /blck12/, conv2(:,k) of /blck13/;  with dry: rc, cw [nlayer][2] = rcd(:,k),
 *                             cwd(:,k) of the dry-aerosol common blocks, and e, feu, cloud, crys4, cm, conv2, below are not touched (may be NULL)
 *   below [nlayer]            1 where feu(k) < min(xcryssulf, xcrysss): the reference prints `k, feu(k), ' below both crystal. points'` for those
 *                             layers up to kinv (the Fortran drop-in does, shim/mistra_kpp_model.f90); may be NULL
 * cw_rc computes layers 2..nmaxf, dry_cw_rc nf+1..nmax: the caller hands over that run of layers. */
/* The host-buffer entries below gather their inputs into a pinned arena, send it up in one stream, and hand the outputs back the same way.  A caller whose
 * arrays never move — the model's COMMON blocks: ff of /cb52/ is 5.9 MB, /kpp_ltot/ 4.4 MB — registers them ONCE with mistra_chem_pin_host; from then on a
 * block that lies inside a registered range is copied straight from / to the caller's memory at the link's rate (no staging copy).  The range must stay
 * mapped until mistra_chem_unpin_host or mistra_chem_finalize; ranges must not overlap.  Not for memory the caller may free (the reference has no such
 * call: its arrays are static; shim/mistra_kpp_model.f90: LIQ_PIN_ONCE). */
int mistra_chem_pin_host(void* p, size_t bytes);
int mistra_chem_unpin_host(void* p);
/* dry_rates_g (tt,freep,nmax) (kpp.f90:4697-4853; gas != 0) | dry_rates_a (freep,nmaxf) (:4860-5073) | dry_rates_t (freep,nmaxf) (:5079-5198), called by
 * liq_parm every time step (kpp.f90:651-653): the mass-transfer coefficients of HNO3, N2O5, NH3, H2SO4 — the routines' idr list, in that order — onto the
 * dry aerosol of bins 1 and 2, and the equilibrium constant of HNO3.  The four species sit at mechanism-specific places of the model's NSPEC-wide arrays:
 * the caller (shim/mistra_kpp_model.f90: DRY_RATES_HIP_g/_a/_t) gathers vmean and scatters the results, so these arrays are compact.  Host buffers:
 *   tt, freep [nlayer]        temperature (/cb53/ t; dry_rates_g: its argument tt) and mean free path of the layers k = 2..nmax
 *   rcd [nlayer][2]           rcd(1:2,k) of /blck11/
 *   vmean4 [nlayer][4]        vmean(idr(l),k) of /kpp_2aer/ | /kpp_2tot/ (aer, tot; NULL for gas: dry_rates_g forms its own)
 *   xkmtd [nlayer][2][4]      out: xkmtd(idr(l),kc,k);   xeq [nlayer]: out: xeq(ind_HNO3,k)
 *   henry4 [nlayer][4]        gas only, in/out: henry(idr(l),k) of /kpp_dryg/ (HNO3 is set, then every positive entry becomes 1/(henry*FCT), as the reference does) */
int mistra_chem_dry_rates(int gas, int nlayer, const double* tt, const double* freep, const double* rcd, const double* vmean4, double* xkmtd, double* xeq,
                          double* henry4);
int mistra_chem_cw_rc(int nlayer, int nkt, int nka, int dry, const double* ff, const double* rq, const double* e, const int32_t* kw, int ka, int ifeed,
                      const double* feu, const int32_t* cloud, const double* crys4, double* rc, double* cw, double* cm, double* conv2, int32_t* below);
int mistra_chem_equil_co(int mech, int nlayer, int nkc, int j6, const double* tt, const double* conv2, const double* xgamma, double* xkef,
                         double* xkeb);

/* Diagnostics for the phase-level parity tests: integrates the cells like mistra_chem_integrate (results discarded) with the
 * kernel variant that writes out, per cell, the intermediate results of the FIRST attempt of the first Rosenbrock step
 * (gas.f:1201-1262): dump[cell][5*NVAR + 2*LU_NONZERO + 2] = Fcn0 (Fun_x) | Ghimj as ros_PrepareMatrix_x builds it | Ghimj
 * after KppDecomp_x in the kernel's form (multipliers in L; the rows of the solves' tail chain row-scaled by 1/U(k,k)) |
 * 1/U(k,k) | K(1) | K(2) | K(3) (KppSolve_x results of the three stages) | Err (ros_ErrorNorm_x) | H. */
int mistra_chem_debug_first_step(int mech, int ncell, const double* var_in, const double* fix, const double* rconst,
                                 double tin, double tout, double* dump);
/* The same at a first step size of the caller's choosing, handing back what that kernel variant finished with.  hstart [ncell] (host,
 * may be null): first step size per cell as in mistra_chem_integrate_device_hstart (entries <= 0: the reference's 1e-3); the dumped
 * attempt then runs at H = min(hstart, |tout - tin|).  var_out [ncell][NVAR], ierr [ncell], stats [ncell][8] (host, each may be null):
 * results of the integration the dump variant carried to its end, to be compared with the product kernel's on the same inputs. */
int mistra_chem_debug_first_step_ex(int mech, int ncell, const double* var_in, const double* fix, const double* rconst,
                                    double tin, double tout, const double* hstart, double* dump, double* var_out, int32_t* ierr,
                                    int32_t* stats);

/* Test hook for the one exit of RosenbrockIntegrator_x that INTEGRATE_x's fixed options put out of a test's reach: IERR = -6, "No of steps
 * exceeds maximum bound" (gas.f:1199-1202), taken when Nstp > Max_no_steps = IPAR(3), which INTEGRATE_x leaves at its default of 100000
 * (gas.f:729-732, 845-846, 1042).  Sets that bound for every later integrate call of the process; max_steps <= 0 restores 100000.  The
 * compiled reference is driven the same way (Rosenbrock_x called with IPAR(3) set) in tests/test_oracle.py. */
int mistra_chem_debug_set_max_steps(int max_steps);

/* Text of the last error on this thread ("" if none). */
const char* mistra_chem_last_error(void);

/* The gather-sum programs of a mechanism as the schedule compiler builds them, for tests; needs no device and no mistra_chem_init.
 * which: 0 the Vdot program in full, 1 the JVS program, 2 Vdot as the kernel runs it (the full program without the terms of the sums
 * that run as chain passes), 3 those chain passes.  info[14] = workgroup size, waves, outputs per lane, words in recs, chain passes
 * on (0 | 1), number of passes, rows of the longest wave in full / as run, modelled ticks of the slowest wave in full / as run, LDS
 * byte address of the 0.0 cell, of the trash cell, of the program's source array, of XS.  wave_base[waves], rows[waves]: of program
 * `which`; mask[waves]: lanes whose species is chained; chained[4 * passes]: the chained species (0-based) in pass order, one per
 * 16-lane row, -1 = none; pass_wave[passes].  recs: the records, [(wave_base[w] + row) * 64 + lane][8], four LDS byte addresses and
 * four float coefficients.  Every array but info may be null.  Returns 0, or -1 with mistra_chem_last_error. */
int mistra_chem_gsum_program(int mech, int which, int64_t* info, uint32_t* wave_base, int32_t* rows, uint64_t* mask, int32_t* chained,
                             int32_t* pass_wave, uint32_t* recs, int64_t recs_cap);

/* One line describing the schedule built for a mechanism (rounds, slots); for logs. */
const char* mistra_chem_describe(int mech);

#ifdef __cplusplus
}
#endif
#endif /* MISTRA_CHEM_H */
