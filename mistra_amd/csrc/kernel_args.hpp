// Plain-old-data argument blocks shared by the host API (capi.cpp) and the device code (ros3_kernel.hip).
#pragma once
#include <cstdint>

namespace mistra {

constexpr int kProfSlots = 16;   // phase counters of the profiling kernel variant
// ... and behind them, per cell, the gather-sum machine's per-wave stamps (lap() stamps wave 0 only): for each of the first kProfWaves
// waves four sums of cycles since wave 0 entered the evaluator — {fun: reached the sums' call, left it; fun_jac: likewise} — then the
// number of fun and of fun_jac calls.  All waves of a workgroup read one clock (one CU).
constexpr int kProfWaves = 8;
constexpr int kProfStride = kProfSlots + 4 * kProfWaves + 2;
constexpr int kVmSweepUpdPerRec = 3;   // updates per record of the sweep programs (schedule.hpp: VM_SWEEP_UPD_PER_REC; ros3_kernel.hip: vm_run)

struct VmDev {                 // LDS VM program in device memory (see schedule.hpp)
  const uint32_t* wave_base;   // [NW]         first record row of each wave's stream
  const uint16_t* blk_n;       // [nrounds*NW] record rows per (round, wave): uploaded, but no kernel reads it (the host-side copy serves the emulator)
  const uint32_t* recs;        // uint4 per lane and row, 16-byte aligned
  int nrounds;
};

struct GsDev {                 // gather-sum program in device memory (see schedule.hpp)
  const uint32_t* wave_base;   // [NW]     first row of each wave's stream
  const uint16_t* rows;        // [NW]     rows of each wave's stream, multiples of 4
  const uint32_t* recs;        // two uint4 per lane and row: 4 LDS byte addresses, 4 float coefficients
};

struct ScaleDev {              // final scaling of the factorisation (schedule.hpp: ScaleProgram)
  const uint32_t* recs;        // u32x4 per lane and slot: two (tgt, aux) LDS byte-address pairs
  int nslots;                  // per lane, multiple of 8
  int wave_slots;              // wave w starts at slot w*wave_slots (nslots + the look-ahead slack)
};

struct TailDev {               // tail chain of the triangular solves (schedule.hpp: TailSolve)
  const uint32_t* fwd;         // the host-side 16-bit tables (TailSolve::fwd / bwd): uploaded, but no kernel reads them — the device
  const uint32_t* bwd;         //   gathers through the address tables below
  const uint32_t* fwd_addr[2]; // per register: u32x4 per lane and group of 4 columns, columns ascending, one LDS byte address per word
  const uint32_t* bwd_addr[2]; //   (tail_solve); bwd: columns descending; null past the tail's registers
};

struct DenseDev {              // dense tail block (schedule.hpp: DenseTail); null where the mechanism has none
  const uint32_t* row_info;    // [192][4]: first M cell of a row's column range, absent-column mask lo / hi, 0 (the kernel keeps rows 0..63)
  const uint16_t* schur_cells; // [8 * DENSE_KB * 64]: operand cells of the Schur steps in MFMA lane order (schedule.hpp: DenseTail)
};

// Rosenbrock_x's options as the kernel's options instantiations (VARIANT 3: Ros3 and the four method kernels) read them: one block of doubles
// in device memory — per mechanism and device slot for the options in force (mistra_chem_set_options), per call for mistra_chem_rosenbrock_ex /
// _device — resolved by the host (capi.cpp: resolve_options, after gas.f:936-1053).  The method is not in the block: it picks the kernel.  What depends on the call's
// interval is left to the kernel: Hmax = min(HMAX, |Tend-Tstart|), H = min(min(HSTART, |Tend-Tstart|), Hmax).
enum RosOptSlot : int {
  kOptHmin = 0,        // RPAR(1)
  kOptHmax,            // RPAR(2); +inf where RPAR(2) = 0
  kOptHstart,          // RPAR(3); max(Hmin, 1e-5) where RPAR(3) = 0
  kOptFacMin, kOptFacMax, kOptFacRej, kOptFacSafe,      // RPAR(4:7), defaults filled in
  kOptAutonomous,      // 1.0: IPAR(1) /= 0 (no ros_FunTimeDerivative_x: one Fun count and the HG*dFdT terms less per step); 0.0: time dependent
  kOptTol              // AbsTol(1:NVAR) then RelTol(1:NVAR); scalar tolerances (IPAR(2) /= 0) arrive as entry 1 repeated
};

struct KernelArgs {
  // per-cell data, cell-major (one cell's VAR / FIX / RCONST contiguous, as COMMON /GDATA_x/ holds them)
  const double* var_in;        // [ncell][NVAR]
  const double* fix;           // [ncell][NFIX]
  const double* rconst;        // [ncell][NREACT]
  double* var_out;             // [ncell][NVAR]   may alias var_in
  int32_t* ierr;               // [ncell]         1 = success, <0 = ros_ErrorMsg code (gas.f:1474)
  int32_t* stats;              // [ncell][8]      Nfun,Njac,Nstp,Nacc,Nrej,Ndec,Nsol,Nsng  (COMMON /Statistics/)
  double* texit_hexit;         // [ncell][2] or null: what INTEGRATE_x leaves in TIN and STEPMIN
  const double* hstart;        // [ncell] or null: first step size per cell instead of INTEGRATE_x's 1e-3 (opt-in, not the reference's behaviour)
  double* h_last;              // [ncell] or null: the step size H when the integrator returned (ros_ErrorMsg_x prints it, gas.f:1506)
  int32_t* sing_rows;          // [ncell][8] or null: rows (1-based) of the zero pivots KppDecomp_x met in this call, in order of occurrence — the
                               //   IER it returns and ros_PrepareMatrix_x prints (gas.f:6157, 1456); entries past min(Nsng, 8) are not written
  double* dump;                // [ncell][5*NVAR + 2*LU_NONZERO + 2] or null: first-step dump (kernel VARIANT 2): Fcn0 | Ghimj prepared |
                               //   Ghimj factorised (kernel form) | R | K1 | K2 | K3 | Err, H  of the first attempt of the first step
  unsigned long long* prof;    // [ncell][kProfStride] or null: shader-clock cycles per phase, then per wave of the sums (diagnostics, see capi.cpp)
  double tin, tout;
  int32_t ncell;
  int32_t n_temps;             // partial-sum cells the solve programs use (zeroed per solve)
  int32_t max_steps;           // Max_no_steps of RosenbrockIntegrator_x (gas.f:1199): 100000, the default INTEGRATE_x leaves (capi.cpp: make_args)
  // mechanism schedule
  const double* consts;        // [NCONST]
  const uint64_t* fun_fac;
  const uint64_t* jac_fac;
  const uint16_t* jvs_pos;
  const uint16_t* zero_pos;
  const uint16_t* diag_pos;
  GsDev vdot, jvs;
  VmDev lu, solve_head_fwd, solve_head_bwd;
  ScaleDev lu_scale;
  TailDev tail;
  DenseDev dense;
  const double* opt;           // [kOptTol + 2*NVAR] or null: Rosenbrock_x's options (RosOptSlot); set = the options instantiation runs (VARIANT 3)
  // step-control trace (kernel VARIANT 4, ros_unit_kernel.hip; mistra_chem_rosenbrock_trace_ex / _device): one record per attempt that reaches
  // ros_ErrorNorm_x.  Read by the trace kernels only; null / 0 everywhere else (capi.cpp: make_args).
  double* trace_d;             // [ncell][trace_cap][4] or null: T at the step's start, H as attempted, Err, share of the largest term in NVAR*Err**2
  int32_t* trace_i;            // [ncell][trace_cap][2] or null: species (1-based) of the largest term, 0 = none | code = accepted + 2 * zero pivots of the attempt
  int32_t* ntrace;             // [ncell]: the TRUE number of attempts (records past trace_cap are not written)
  int32_t* ctrl;               // [ncell][NVAR] or null: attempts each species controlled
  int32_t trace_cap;
  // tolerances per cell (mistra_chem_rosenbrock_cells_ex / _device and their trace forms; options instantiations only): species s of cell c reads
  // entry c*tol_cell_stride + s*tol_spec_stride of each array instead of the pair in the options block, and the kernel makes Rosenbrock_x's
  // check of them (gas.f:1045-1053, IERR = -5) per cell.  Null = the block's pair, checked by the host (capi.cpp: make_args).
  const double* tol_abs;       // [ncell][tol_cell_stride] or null
  const double* tol_rel;       // [ncell][tol_cell_stride] or null
  int32_t tol_cell_stride;     // the row width ntol: 1 or NVAR
  int32_t tol_spec_stride;     // 1: vector tolerances (IPAR(2) = 0), 0: scalar ones (entry 0 of the row for every species)
  // the integrator policy's cell-relative AbsTol (mistra_chem_set_policy; options instantiations only, tol_abs null): every species of a cell gets
  // max(tol_cell_floor, tol_cell_factor * max_i |VAR(i)|), formed by the kernel from the state it receives, once per call; RelTol stays the block's.
  // 0 = off: the block's AbsTol.  The host has validated both (capi.cpp: check_policy); the entries whose options travel with the call pass 0.
  double tol_cell_factor;
  double tol_cell_floor;
  // a series (kernel VARIANT 5, ros_unit_kernel.hip; mistra_chem_rosenbrock_series_ex / _device and their cells forms): nleg legs over times[0 .. nleg],
  // leg k one call of Rosenbrock_x from times[k] to times[k+1] on the state leg k-1 left.  Read by the series kernels only, which do not read tin / tout;
  // null / 0 everywhere else (capi.cpp: make_args).  Leg k writes var_out + k*leg_var, ierr + k*leg_ierr, stats + k*leg_stats, texit_hexit + k*leg_th and
  // h_last + k*leg_h (strides in elements; the kernel forms the 64-bit offsets where it uses them).
  const double* times;         // [nleg + 1]: the device copy, behind the call's options block; nothing writes it while the kernel runs (scalar loads)
  int32_t nleg;
  int32_t carry_h;             // /= 0: a later leg's first step is the previous leg's Hexit of the cell where that is > 0, else the options' Hstart
  int64_t leg_var, leg_ierr, leg_stats, leg_th, leg_h;
  // the reaction flux (kernel VARIANT 6, ros_unit_kernel.hip; mistra_chem_rosenbrock_flux_ex / _device and their cells forms): [ncell][NREACT], every
  // reaction's rate integrated over the call, written once per cell when it leaves (a cell refused with -5: +0.0).  Read by the flux kernels and by the
  // series kernels with the flux of every leg (VARIANT 11: [nleg][ncell][NREACT], leg_flux below); null everywhere else (capi.cpp: make_args).
  double* flux;
  // dense output (kernel VARIANT 7, in the series units of ros_unit_kernel.hip; mistra_chem_rosenbrock_dense_ex / _device and their cells forms): the state
  // at dense_ns sample times inside the one call from tin to tout, by the cubic Hermite interpolant between the accepted states.  The
  // sample times are `times`[0 .. dense_ns), behind the call's options block as a series keeps its own (nleg stays 0).  Sample k of cell c is the row
  // dense_out + k*dense_block + c*NVAR; dense_nout[c] samples were reached, the rows behind them are written +0.0.  Read by the dense kernels only; null /
  // 0 everywhere else (capi.cpp: make_args).
  double* dense_out;           // [dense_ns][dense_block]
  int32_t* dense_nout;         // [ncell]
  int32_t dense_ns;
  int64_t dense_block;         // elements from one sample's block to the next: ncell*NVAR of the launch
  // the operators (kernel VARIANT 8, in the trace units of ros_unit_kernel.hip; mistra_chem_ops_ex / _device): Fun_x, Jac_SP_x and solves with
  // shift*I - Jac_SP_x at the state var_in holds, once, no integration.  The right-hand sides are the cell's own Fun_x (ops_fun_rhs:
  // row 0 of ops_x) followed by ops_nrhs rows of ops_rhs; row j of cell c is at j*block + c*NVAR of either array.  Read by the operator kernels only,
  // which read nothing of the integration's arguments but var_in, fix, rconst, ncell, n_temps and the schedule; null / 0 everywhere else (capi.cpp: make_args).
  double* ops_vdot;            // [ncell][NVAR] or null: not wanted
  double* ops_jvs;             // [ncell][LU_NONZERO] or null: not wanted; KPP's slot order, the fill-in slots +0.0
  double* ops_x;               // [ops_fun_rhs + ops_nrhs][ops_x_block] or null: no solve
  const double* ops_rhs;       // [ops_nrhs][ops_rhs_block]
  const double* ops_shift;     // cell c reads entry c*ops_shift_stride
  int32_t* ops_ising;          // [ncell]: KppDecomp_x's IER, the first row (1-based) whose prepared diagonal is exactly zero, else 0 (set with ops_x)
  int32_t ops_shift_stride;    // 0: one shift shared by all cells, 1: one per cell
  int32_t ops_fun_rhs;         // /= 0: the cell's Fun_x is right-hand side 0
  int32_t ops_nrhs;
  int64_t ops_x_block, ops_rhs_block;      // elements from one row's block to the next: ncell*NVAR of the caller's arrays
  // a series with rate constants and FIX of the leg's own (the series kernels; mistra_chem_rosenbrock_series_rates_ex / _device and their cells forms):
  // leg k reads rconst + k*leg_rconst and fix + k*leg_fix (strides in elements), piecewise constant over the series as Update_RCONST_x in front of
  // every call leaves them.  0 = one block for every leg.  Read by the series kernels only; 0 everywhere else (capi.cpp: make_args).
  int64_t leg_rconst, leg_fix;
  // chain passes of the Vdot sums (schedule.hpp: GsumChain), read by the kernels of a mechanism whose trait enables them; `vdot` above is
  // then the lean program.  (At the end of the block: every other argument keeps its offset.)
  GsDev vdot_pass;
  const uint64_t* vdot_chain_mask;      // [NW] lanes whose species is chained
  // the replay (kernel VARIANT 9, in the trace units of ros_unit_kernel.hip; mistra_chem_rosenbrock_replay_ex / _device and their cells forms): the cell makes
  // the steps of its row of replay_h, all accepted, instead of choosing them.  replay_h_stride = 0: one row and one count shared by all
  // cells, the row behind the call's options block (scalar loads: nothing writes it while the kernel runs); else cell c reads row c*replay_h_stride and
  // replay_n[c], clamped to replay_cap.  Step n of cell c leaves its Err in replay_err[c*replay_cap + n]; entries past the cell's count are not written.
  // Read by the replay kernels only; null / 0 everywhere else (capi.cpp: make_args).  (Behind the chain passes: every other argument keeps its offset.)
  const double* replay_h;      // [replay_cap] or [ncell][replay_h_stride]
  const int32_t* replay_n;     // [1] or [ncell]
  int64_t replay_h_stride;
  int32_t replay_cap;
  double* replay_err;          // [ncell][replay_cap] or null: not wanted
  // a series with rate constants linear in time over each leg (kernel VARIANT 10, in the method and trace units of ros_unit_kernel.hip;
  // mistra_chem_rosenbrock_series_linrates_ex / _device and their cells forms): rconst holds nleg + 1 node blocks leg_rconst elements
  // apart, block k the rate constants at times[k]; leg k reads blocks k and k + 1.  /= 0 selects those kernels (capi.cpp: launch), which read the series'
  // arguments and nothing else of their own; 0 everywhere else (capi.cpp: make_args).  (At the end of the block: every other argument keeps its offset.)
  int32_t lin_rates;
  // a series with the reaction flux of every leg (kernel VARIANT 11, beside VARIANT 10 in the method and trace units of ros_unit_kernel.hip;
  // mistra_chem_rosenbrock_series_flux_ex / _device and their cells forms): leg k writes its [ncell][NREACT] rows at flux + k*leg_flux
  // (a stride in elements, ncell*NREACT of the launch).  With a.times and a.flux both set, /= 0 selects those kernels (capi.cpp: launch), which read the
  // series' arguments, flux and this; 0 everywhere else (capi.cpp: make_args).  (At the end of the block: every other argument keeps its offset.)
  int64_t leg_flux;
};

}  // namespace mistra
