// Update_RCONST_x on the device: the rate constants of a batch of cells from each cell's meteorology,
// switches, photolysis rates and the few concentrations the rate laws read, instead of 8*NREACT bytes per cell from the host.
//
// The generated Update_RCONST_x (gas.f:275-666 | aer.f:304-1364 | tot.f:1040-2768) is one assignment per reaction,
//     RCONST(i) = <product of switches, literals, rate-law calls, array elements>
// tools/extract_rates.py turns those into postfix programs (mistra_amd/mech/<mech>.rates); this file holds the evaluator
// and the rate-law functions of kpp.f90:7127-8376 that the three mechanisms call.  What a rate law reads from COMMON itself
// (uptake coefficients, liquid water, a few concentrations) it finds through the table's slot list (FS_*, tools/extract_rates.py:
// fslot_names), so the functions are the same code for every mechanism.
// Arithmetic follows the reference statement by statement: Fortran evaluation order, integer arguments converted where
// the reference converts them, DEFAULT-REAL literals as the double nearest their float32 — `300.` is exact,
// `8.314` is 8.31400012969970703, `0.21` is 0.209999993443489075, `10**(-6.16)` is the single-precision power
// 6.91831189669755986e-07 (what flang folds it to; tools/extract_rates.py documents the check).  exp, pow and log10 are the
// device library's: they differ from the host libm's in the last place, which is the whole of the stated tolerance
// (tests/test_gpu_rates.py: 1e-13 relative).  Built with -ffp-contract=off like the rest.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "rates.hpp"

namespace mistra {

namespace {

constexpr double kR8314 = 8.31400012969970703;          // 8.314  as a default-real literal
constexpr double k021 = 0.209999993443489075;           // 0.21
constexpr double kTenPowM616 = 6.91831189669755986e-07; // 10**(-6.16): INTEGER ** REAL is evaluated in single precision

struct Cb1 { double aircc, te, h2oppm, pk; };           // COMMON /cb_1/ (kpp.f90:7140)

// MAX(a, b) as the reference's compiler makes it: a select on a > b.  A NaN in b comes through (fdhet*'s max(0.d0, x1+x2) is NaN), a NaN in a
// does not (uplim's max(c, 0.d0) is 0 for c = NaN): both are in tests/golden/rates_edges_<mech>.npz from the compiled reference
__device__ __forceinline__ double fmax_fortran(double a, double b) { return a > b ? a : b; }

// kpp.f90:7127  farr=a*exp(b/te), b INTEGER
__device__ double farr(const Cb1& c, double a, double b) { return a * exp(b / c.te); }
// kpp.f90:7149  farr_sp=a*((te/b)**c)*exp(d/te), b and d INTEGER
__device__ double farr_sp(const Cb1& c, double a, double b, double cc, double d) { return (a * pow(c.te / b, cc)) * exp(d / c.te); }
// Troe fall-off shared by ATK_3 (kpp.f90:7171), ATK_3f (:7301), fbck (:7355), fbckJ (:7383), fbck2 (:7411); tref = 300. | 298.
__device__ double troe(const Cb1& c, double a1, double a2, double b1, double b2, double fc, double tref) {
  const double a0 = (a1 * c.aircc) * pow(c.te / tref, a2);
  const double b0 = b1 * pow(c.te / tref, b2);
  const double l = log10(a0 / b0);
  return (a0 / (1.0 + a0 / b0)) * pow(fc, 1.0 / (1.0 + l * l));
}
// kpp.f90:7327  sHNO3: func(a,b) = a*exp(b*tte), tte = 1./te, b INTEGER
__device__ double shno3(const Cb1& c, double a1, double b1, double a2, double b2, double a3, double b3) {
  const double tte = 1.0 / c.te;
  const double f1 = a1 * exp(b1 * tte), f2 = a2 * exp(b2 * tte), f3 = a3 * exp(b3 * tte);
  return f1 + ((f3 * c.aircc) / (1.0 + (f3 * c.aircc) / f2));
}
// kpp.f90:7483  sp_23
__device__ double sp_23(const Cb1& c, double a1, double b1, double a2, double b2, double a3, double b3) {
  const double tte = 1.0 / c.te;
  const double f1 = a1 * exp(b1 * tte), f2 = (a2 * c.aircc) * exp(b2 * tte);
  const double f3 = (((a3 * c.aircc) * c.h2oppm) * 1.0e-6) * exp(b3 * tte);
  return (f1 + f2) * (1.0 + f3);
}
// kpp.f90:7540  fcn: x2=8.314*te; xmg=pk/x2; fcn=10**(-6.16)*exp(-90.7d3/x2)*xmg*x1
__device__ double fcn(const Cb1& c, double x1) {
  const double x2 = kR8314 * c.te, xmg = c.pk / x2;
  return ((kTenPowM616 * exp(-90.7e3 / x2)) * xmg) * x1;
}
// kpp.f90:8351  DMS_add
__device__ double dms_add(const Cb1& c) {
  const double o2 = k021 * c.aircc, tte = 1.0 / c.te;
  return ((9.5e-39 * exp(5270.0 * tte)) * o2) / (1.0 + (7.5e-29 * exp(5610.0 * tte)) * o2);
}
// positions in the table's slot list of what the rate laws read from COMMON (tools/extract_rates.py: fslot_names)
enum { FS_H2OL = 0, FS_CLM = 4, FS_BRM = 8, FS_YXKMT_N2O5 = 12, FS_YXKMT_CLNO3 = 16, FS_YXKMT_BRNO3 = 20, FS_YCW = 24,
       FS_YXKMTD_N2O5 = 28, FS_YXKMTD_BRNO3 = 30, FS_YXKMTD_CLNO3 = 32, FS_YXKMTD_HNO3 = 34, FS_YXKMTD_NH3 = 36,
       FS_YXKMTD_H2SO4 = 38, FS_YCWD = 40, FS_YHENRY_HNO3 = 42, FS_YXEQ_HNO3 = 43, FS_C_HNO3 = 44, FS_C_HNO3L = 45,
       FS_C_NO3ML = 47, FS_XHAL = 49 };

struct Env {
  const double* e;
  const int32_t* fs;
  __device__ double at(int f) const { return e[fs[f]]; }            // the value behind slot-list position f
  __device__ bool has(int f) const { return fs[f] >= 0; }
};

// kpp.f90:8198 fdhetg | :8269 fdheta | :8311 fdhett (na, nb): uptake on dry aerosol.  The three differ in the "aqueous" HNO3
// of the nb = 1 branch: gas knows no NO3- species and takes C(HNO3lz)*1.5d3 (a hard-coded pH 2, kpp.f90:8232-8233); aer and
// tot take C(HNO3lz)+C(NO3mlz) behind a guard on the denominator (kpp.f90:8285-8291).
__device__ double fdhet(const Env& v, int na, int nb) {
  const double ycwd = v.at(FS_YCWD + na - 1);
  if (nb == 1) {
    const double yx = v.at(FS_YXKMTD_HNO3 + na - 1);
    const double x1 = yx * ycwd;
    double caq;
    if (v.has(FS_C_NO3ML)) {
      caq = 0.0;
      if ((v.at(FS_YXEQ_HNO3) + 1.0e-2) != 0.0) caq = ((v.at(FS_C_HNO3L + na - 1) + v.at(FS_C_NO3ML + na - 1)) * 1.0e-2) / (v.at(FS_YXEQ_HNO3) + 1.0e-2);
    } else {
      caq = ((v.at(FS_C_HNO3L + na - 1) * 1.5e3) * 1.0e-2) / (v.at(FS_YXEQ_HNO3) + 1.0e-2);
    }
    double x2 = 0.0;
    if (v.at(FS_C_HNO3) != 0.0 && v.at(FS_YHENRY_HNO3) != 0.0) x2 = ((-yx) / (v.at(FS_C_HNO3) * v.at(FS_YHENRY_HNO3))) * caq;
    return fmax_fortran(0.0, x1 + x2);
  }
  const int sp = nb == 2 ? FS_YXKMTD_N2O5 : nb == 3 ? FS_YXKMTD_NH3 : FS_YXKMTD_H2SO4;
  return v.at(sp + na - 1) * ycwd;
}
// kpp.f90:7562  farr2=a0*exp(dble(b0)*(1.d0/te-3.3557d-3))
__device__ double farr2(const Cb1& c, double a0, double b0) { return a0 * exp(b0 * (1.0 / c.te - 3.3557e-3)); }
// kpp.f90:7582  fhet_t(a0,b0,c0): bin a0 = 1..4; b0 picks the reaction partner (H2O | Cl- | Br-), c0 the gas (N2O5 | ClNO3 | BrNO3)
__device__ double fhet_t(const Env& v, int a0, int b0, int c0) {
  const double h2oa = v.at(FS_H2OL + a0 - 1);
  const double hetT = (h2oa + 5.0e2 * v.at(FS_CLM + a0 - 1)) + 3.0e5 * v.at(FS_BRM + a0 - 1);
  const double xbr = b0 == 1 ? h2oa : b0 == 2 ? 5.0e2 : 3.0e5;
  const double xtr = v.at((c0 == 1 ? FS_YXKMT_N2O5 : c0 == 2 ? FS_YXKMT_CLNO3 : FS_YXKMT_BRNO3) + a0 - 1);
  return hetT > 0.0 ? ((xtr * v.at(FS_YCW + a0 - 1)) * xbr) / hetT : 0.0;
}
// kpp.f90:8023 fhet_da | :8111 fhet_dt (xliq, xhet, a0, b0, c0), a0 = 1..2: on the deliquesced aerosol (xhet = 0) or on the dry one
__device__ double fhet_d(const Env& v, double xliq, double xhet, int a0, int b0, int c0) {
  constexpr double k5555 = 55.549999237060547;      // 55.55 as a default-real literal
  const double xhal = v.at(FS_XHAL);
  double xtr, h2oa, hetT, yw;
  if (xhet == 0.0) {
    xtr = v.at((c0 == 1 ? FS_YXKMT_N2O5 : c0 == 2 ? FS_YXKMT_CLNO3 : FS_YXKMT_BRNO3) + a0 - 1);
    h2oa = v.at(FS_H2OL + a0 - 1);
    hetT = (h2oa + 5.0e2 * v.at(FS_CLM + a0 - 1)) + 3.0e5 * v.at(FS_BRM + a0 - 1);
    yw = v.at(FS_YCW + a0 - 1);
    if (xhal == 0.0) {
      if (c0 == 2 || c0 == 3) xtr = 0.0;
      hetT = v.at(FS_H2OL + a0 - 1);
    }
  } else {      // (note the reference's order here: c0 = 2 is BrNO3, c0 = 3 ClNO3, kpp.f90:8066-8068)
    xtr = v.at((c0 == 1 ? FS_YXKMTD_N2O5 : c0 == 2 ? FS_YXKMTD_BRNO3 : FS_YXKMTD_CLNO3) + a0 - 1);
    h2oa = (k5555 * v.at(FS_YCWD + a0 - 1)) * 1.0e3;
    hetT = (h2oa + 5.0e2 * v.at(FS_CLM + a0 - 1)) + 3.0e5 * v.at(FS_BRM + a0 - 1);
    yw = v.at(FS_YCWD + a0 - 1);
    if (xhal == 0.0) {
      if (c0 == 2 || c0 == 3) xtr = 0.0;
      hetT = (k5555 * v.at(FS_YCWD + a0 - 1)) * 1.0e3;
    }
  }
  const double xbr = b0 == 1 ? h2oa : b0 == 2 ? 5.0e2 : 3.0e5;
  double r = hetT > 0.0 ? ((xtr * yw) * xbr) / hetT : 0.0;
  if ((c0 == 2 || c0 == 3 || b0 == 2 || b0 == 3) && xhal == 0.0) r = 0.0;
  if (xliq == 0.0) r = 0.0;
  return r;
}

// ---- st_coeff_a / st_coeff_t (kpp.f90:857-1038 | 664-851) run through the same evaluator (tools/extract_stcoeff.py writes their assignments as
//      postfix programs over env = [t, cw(1,k), cm(1,k), sion1(13,1,k), sion1(14,1,k)]); what they call beyond + - * /:
__device__ __forceinline__ double fmin_fortran(double a, double b) { return (a < b || b != b) ? a : b; }
// kpp.f90:8377  a_n2o5(k,kc), kc = 1: uptake coefficient of N2O5 on the sulfate aerosol from its water, nitrate and chloride content
__device__ double a_n2o5(double cw1, double cm1, double s13, double s14) {
  double xno3m = 0.0, xclm = 0.0, xh2o = 0.0;
  if (cw1 > 0.0) {
    xno3m = (s13 / cw1) * 1.0e-3;
    xclm = (s14 / cw1) * 1.0e-3;
  }
  if (cm1 > 0.0 && cw1 > 0.0) xh2o = 55.55 * (cm1 / cw1);
  const double xk2f = 1.15e6 - 1.15e6 * exp(-0.13 * xh2o);
  double denom = 1.0;
  if (xno3m > 0.0) denom = (1.0 + (6.0e-2 * xh2o) / xno3m) + (29.0 * xclm) / xno3m;
  return (3.2e-8 * xk2f) * (1.0 - (1.0 / denom));
}

__global__ __launch_bounds__(256) void update_rconst_kernel(const RatesDev R, const double* __restrict__ env, double* __restrict__ rconst,
                                                            int ncell) {
  // lane = cell, wave = a contiguous run of reactions: the 64 lanes of a wave interpret the SAME program (no divergence in
  // the op / rate-law switches, program words and literals are wave-uniform loads); a thread per (cell, reaction) had every
  // lane on another program.  blockIdx.x: group of 64 cells; blockIdx.y * 4 + wave: chunk of reactions.
  const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const int nchunk = 4 * (int)gridDim.y, chunk = (int)blockIdx.y * 4 + wave, per = (R.nreact + nchunk - 1) / nchunk;
  const int r_begin = chunk * per, r_end = r_begin + per < R.nreact ? r_begin + per : R.nreact;
  const int cell_raw = (int)blockIdx.x * 64 + lane;
  const bool live = cell_raw < ncell;
  const int cell = live ? cell_raw : ncell - 1;      // (idle lanes repeat the last cell and do not store)
  const double* e = env + (size_t)cell * R.nenv;
  const Cb1 cb{e[0], e[1], e[2], e[3]};
  const Env ev{e, R.fslot};
  constexpr double dclim = 1.0e10;      // the reaction-rate ceiling of dmin2 / uplim / uparm / uplip / uparp
  // operand stack of the postfix programs: one LDS column per thread (a private array indexed by the stack pointer would live in
  // scratch memory: a global round trip per push and pop)
  __shared__ double stack_cells[kRatesStackDepth][256];      // (the loaders hold every program to this depth: rates_stack_depth)
#define st_at(i) stack_cells[(i)][threadIdx.x]
  for (int r = r_begin; r < r_end; r++) {
  int sp = 0;
  for (int w = R.offs[r]; w < R.offs[r + 1]; w++) {
    const int word = R.words[w], op = word & 0xFF, arg = word >> 8;
    switch (op) {
      case 0: st_at(sp++) = R.consts[arg]; break;
      case 1: st_at(sp++) = e[arg]; break;
      case 2: sp--; st_at(sp - 1) = st_at(sp - 1) + st_at(sp); break;
      case 3: sp--; st_at(sp - 1) = st_at(sp - 1) - st_at(sp); break;
      case 4: sp--; st_at(sp - 1) = st_at(sp - 1) * st_at(sp); break;
      case 5: sp--; st_at(sp - 1) = st_at(sp - 1) / st_at(sp); break;
      case 6: st_at(sp - 1) = -st_at(sp - 1); break;
      default: {      // call: arguments are the top of the stack, first argument deepest
        double v = 0.0;
        switch (arg) {
          case 0: sp -= 2; v = farr(cb, st_at(sp), st_at(sp + 1)); break;
          case 1: sp -= 4; v = farr_sp(cb, st_at(sp), st_at(sp + 1), st_at(sp + 2), st_at(sp + 3)); break;
          case 2: sp -= 5; v = troe(cb, st_at(sp), st_at(sp + 1), st_at(sp + 2), st_at(sp + 3), st_at(sp + 4), 300.0); break;       // ATK_3
          case 3: sp -= 5; v = troe(cb, st_at(sp), st_at(sp + 1), st_at(sp + 2), st_at(sp + 3), st_at(sp + 4), 298.0); break;       // ATK_3f
          case 4: sp -= 6; v = shno3(cb, st_at(sp), st_at(sp + 1), st_at(sp + 2), st_at(sp + 3), st_at(sp + 4), st_at(sp + 5)); break;
          case 5: sp -= 7; v = troe(cb, st_at(sp), st_at(sp + 1), st_at(sp + 2), st_at(sp + 3), st_at(sp + 4), 300.0) / (st_at(sp + 5) * exp(st_at(sp + 6) / cb.te)); break;   // fbck
          case 6: sp -= 6; v = troe(cb, st_at(sp), st_at(sp + 1), st_at(sp + 2), st_at(sp + 3), 0.6, 300.0) / (st_at(sp + 4) * exp(st_at(sp + 5) / cb.te)); break;        // fbckJ
          case 7: {   // fbck2 (kpp.f90:7411): ak=5.44d-9, bk=14192.d0; 0 where ck = 0
            sp -= 6;
            const double x1 = troe(cb, st_at(sp), st_at(sp + 1), st_at(sp + 2), st_at(sp + 3), st_at(sp + 4), 300.0), ck = st_at(sp + 5);
            v = ck != 0.0 ? x1 / (((((5.44e-9 * exp(14192.0 / cb.te)) * kR8314) / 101325.0) * cb.te) / ck) : 0.0;
            break;
          }
          case 8: sp -= 2; v = st_at(sp) * (1.0 + cb.aircc / st_at(sp + 1)); break;                                         // sp_17
          case 9: sp -= 6; v = sp_23(cb, st_at(sp), st_at(sp + 1), st_at(sp + 2), st_at(sp + 3), st_at(sp + 4), st_at(sp + 5)); break;
          case 10: sp -= 1; v = fcn(cb, st_at(sp)); break;
          case 11: v = dms_add(cb); break;
          case 12: sp -= 2; v = fdhet(ev, (int)st_at(sp), (int)st_at(sp + 1)); break;
          case 13: sp -= 2; v = farr2(cb, st_at(sp), st_at(sp + 1)); break;
          case 14: sp -= 3; v = fhet_t(ev, (int)st_at(sp), (int)st_at(sp + 1), (int)st_at(sp + 2)); break;
          case 15: sp -= 5; v = fhet_d(ev, st_at(sp), st_at(sp + 1), (int)st_at(sp + 2), (int)st_at(sp + 3), (int)st_at(sp + 4)); break;
          case 16: {   // fliq_60 (kpp.f90:7662): a1*exp(dble(b1)*(1.d0/te-3.3557d-3))*c/(c+0.1d0/d)
            sp -= 4;
            const double a1 = st_at(sp), b1 = st_at(sp + 1), c = st_at(sp + 2), d = st_at(sp + 3);
            v = d > 0.0 ? ((a1 * exp(b1 * (1.0 / cb.te - 3.3557e-3))) * c) / (c + 0.1 / d) : 0.0;
            break;
          }
          case 17: sp -= 1; v = st_at(sp) < dclim ? st_at(sp) : dclim; break;                    // dmin2 = dmin1(a, 1.d10)
          case 18: sp -= 1; v = st_at(sp) < dclim * 2.0 ? st_at(sp) : dclim * 2.0; break;        // dmin3 = dmin1(a, 2.d10)
          case 19: {   // flsc4 = a*b*c**3 (kpp.f90:7755); c**3 as the compiler expands it: c*c*c
            sp -= 3;
            const double c = st_at(sp + 2);
            v = c > 0.0 ? (st_at(sp) * st_at(sp + 1)) * ((c * c) * c) : 0.0;
            break;
          }
          case 20: {   // flsc5 = a*b**2*c**4 (kpp.f90:7778); c**4 as the reference's compiler expands it: ((c*c)*c)*c
            sp -= 3;
            const double b = st_at(sp + 1), c = st_at(sp + 2);
            v = c > 0.0 ? (st_at(sp) * (b * b)) * (((c * c) * c) * c) : 0.0;
            break;
          }
          case 21: sp -= 2; v = st_at(sp + 1) > 1.0e-15 ? st_at(sp) / st_at(sp + 1) : 0.0; break;    // flsc6 (kpp.f90:7801)
          case 22: {   // uplim = a/(1 + b/dclim*max(c,0)*d) (kpp.f90:7862)
            sp -= 4;
            const double a = st_at(sp), b = st_at(sp + 1), c = st_at(sp + 2), d = st_at(sp + 3);
            v = d > 0.0 ? a / (1.0 + ((b / dclim) * fmax_fortran(c, 0.0)) * d) : 0.0;
            break;
          }
          case 23: {   // uparm = a0*exp(dble(b0)*(1/te-3.3557d-3))/(1+c/dclim*d*e) (kpp.f90:7888)
            sp -= 5;
            const double a0 = st_at(sp), b0 = st_at(sp + 1), c = st_at(sp + 2), d = st_at(sp + 3), ee = st_at(sp + 4);
            v = d > 0.0 ? (a0 * exp(b0 * (1.0 / cb.te - 3.3557e-3))) / (1.0 + ((c / dclim) * d) * ee) : 0.0;
            break;
          }
          case 24: {   // uplip = a/(1 + a/dclim*max(b,0)*c)*c**2 (kpp.f90:7916)
            sp -= 3;
            const double a = st_at(sp), b = st_at(sp + 1), c = st_at(sp + 2);
            v = c > 0.0 ? (a / (1.0 + ((a / dclim) * fmax_fortran(b, 0.0)) * c)) * (c * c) : 0.0;
            break;
          }
          case 25: {   // uparp = k/(1 + k/dclim*c*d)*d**2, k = a0*exp(dble(b0)*(1/te-3.3557d-3)) (kpp.f90:7942)
            sp -= 4;
            const double a0 = st_at(sp), b0 = st_at(sp + 1), c = st_at(sp + 2), d = st_at(sp + 3);
            const double k = a0 * exp(b0 * (1.0 / cb.te - 3.3557e-3));
            v = d > 0.0 ? (k / (1.0 + ((k / dclim) * c) * d)) * (d * d) : 0.0;
            break;
          }
          case 26: sp -= 1; v = exp(st_at(sp)); break;                                                                      // the intrinsic, st_coeff_x
          case 27: sp -= 4; v = a_n2o5(st_at(sp), st_at(sp + 1), st_at(sp + 2), st_at(sp + 3)); break;
          case 28: sp -= 2; v = fmin_fortran(st_at(sp), st_at(sp + 1)); break;                                              // min(a, b)
        }
        st_at(sp++) = v;
      }
    }
  }
  if (live) rconst[(size_t)cell * R.nreact + r] = st_at(0);
  }
}
#undef st_at

}  // namespace

hipError_t launch_update_rconst(const RatesDev& R, const double* d_env, double* d_rconst, int ncell, hipStream_t stream) {
  if (ncell <= 0) return hipSuccess;
  // enough workgroups to fill the chip even for a column's worth of cells: the reactions are cut into 4 * gy chunks
  const unsigned gx = (unsigned)((ncell + 63) / 64);
  unsigned gy = gx >= 2048 ? 1u : (2048u + gx - 1) / gx;
  const unsigned gy_max = (unsigned)((R.nreact + 15) / 16);      // at least four reactions per wave
  if (gy > gy_max) gy = gy_max;
  hipLaunchKernelGGL(update_rconst_kernel, dim3(gx, gy), dim3(256), 0, stream, R, d_env, d_rconst, ncell);
  return hipGetLastError();
}

}  // namespace mistra
